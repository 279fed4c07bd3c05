"""The scenes of tests/mapper_scenes.py, checked without a GPU:

  * each scene holds the populations it is there to exercise (rays with exactly 3 and exactly 4 frames in view, own
    frame in and out of the window, entries behind a camera, every way a frustum point is rejected, keyframes with no,
    partial and full overlap, all three segments of the radius map), and every one of its decisions is firm;
  * mapper_scenes.warp_terms in float64 is the pinned restatement (tests/pix_warp_ref.py) and its autograd gradient;
  * six deliberate mistakes, applied to a copy of the restatement, move its output on these scenes by at least 100x the
    tolerance tests/test_gpu_mapper_kernels.py uses, or flip decisions where that file demands exact equality: fy -> fx
    in the projection, the translation column of the inverse pose dropped, one cofactor pair of the 3x3 inverse
    transposed, a zero border in place of the reflect border of the Sobel, t = 1 for a single overlap sample, the
    partial sums of the loss after the 256th ignored;
  * the derived colour-gradient bounds hold for a float32 numpy evaluation of the same formulas."""
import functools

import numpy as np
import pytest
import torch

import color_grad_ref
import keyframe_select_ref as ksr
import mapper_scenes as ms
from pix_warp_ref import pix_warp_loss

LOSS_RTOL = 1e-5                       # test_gpu_mapper_kernels: the loss against float64
GRAD_BOUND = 4 * 1e-7                  # 4 E32, E32 rounded up from the measured 4.8e-8: the mutations must clear 100x


@functools.lru_cache(maxsize=None)
def scene(name):
    c = ms.warp_scene(**ms.WARP_SCENES[name])
    return c, ms.warp_terms(c)


def _in_view(c, r):
    H, W = c["H"], c["W"]
    seen = (r["u"] > 5) & (r["u"] < W - 5) & (r["v"] > 5) & (r["v"] < H - 5) & (r["z"] < 0)
    return seen & (c["frame_indices"][None, :] != c["indices"][:, None])


def test_cameras_are_general():
    rng = np.random.default_rng(0)
    c = ms.general_window(64, rng, 0.08, turned=(7, 40)).astype(np.float64)
    R = c[:, :3, :3]
    assert np.abs(R).min() >= ms.R_MIN and np.abs(R).max() < 1 - 1e-3
    assert np.abs(R @ R.transpose(0, 2, 1) - np.eye(3)).max() < 1e-6 and np.allclose(np.linalg.det(R), 1, atol=1e-6)
    assert np.ptp(c[:, :3, 3], axis=0).min() > 0.2                       # translations in every direction
    axes = R[:, :, 2]                                                    # the viewing axes share a direction ...
    assert (axes[[0, 1, 2]] @ axes[3] > 0.95).all()
    assert axes[7] @ axes[3] < -0.95 and axes[40] @ axes[3] < -0.95      # ... but for the turned cameras
    for (H, W), (fx, fy, cx, cy) in ms.INTRINSICS.items():
        assert abs(fx - fy) >= 0.15 * max(fx, fy)
        assert abs(cx - (W - 1) / 2) > 0.3 and abs(cy - (H - 1) / 2) > 0.3 and cx % 1 and cy % 1


@pytest.mark.parametrize("name", list(ms.WARP_SCENES))
def test_warp_scene_populations(name):
    c, r = scene(name)
    a = ms.WARP_SCENES[name]
    H, W, N = c["H"], c["W"], a["N"]
    assert r["mask"].shape == (N, a["M"]) and len(c["depth"]) == N
    # firm: no entry within the margin of a threshold, no read entry within it of a texel boundary
    u, v, z = r["u"], r["v"], r["z"]
    for x, t in ((u, 5), (u, W - 5), (v, 5), (v, H - 5), (z, 0)):
        assert np.abs(x - t).min() >= ms.WARP_MARGIN
    for q in (u - 0.5, v - 0.5):
        f = (q - np.floor(q))[r["mask"]]
        assert f.min() >= ms.WARP_MARGIN and f.max() <= 1 - ms.WARP_MARGIN
    assert ms.WARP_MARGIN >= 100 * np.spacing(np.float32(W))             # 100 fp32 spacings of u, v at this size
    assert r["mask"][N - 1].sum() >= 4                                   # the last ray is a kept one
    n = _in_view(c, r).sum(1)
    outside = c["indices"] == ms.OUTSIDE_ID
    print(f"{name}: kept rays {(r['ray_kept'] > 0).sum()} of {N}, frames in view {np.bincount(n)[:7]}, "
          f"own frame outside {outside.sum()}, entries behind a camera {(z > 0).sum()}")
    if N >= 255:
        assert (n == 3).any() and (n == 4).any() and (n == 0).any()      # dropped by one frame, kept by one frame
        assert (outside & (n >= 4)).any() and (~outside & (n >= 4)).any()
        assert not np.isin(ms.OUTSIDE_ID, c["frame_indices"])
    if a.get("turned"):
        turned = list(a["turned"])
        elsewhere = ~np.isin(c["indices"], c["frame_indices"][turned])   # rays that do not start in a turned camera
        assert (z > 0).sum() >= N and (z[elsewhere][:, turned] > 0).all() and (r["ray_kept"][~elsewhere] == 0).all()
        assert not r["mask"][:, turned].any()
    if name == "m64":
        assert r["mask"][:, 63].sum() > 10
    if name in ("m5", "m6"):
        assert 90 <= (r["ray_kept"] > 0).sum() <= 250
    if name == "m64" or name == "m63":
        assert (r["ray_kept"] > 0).sum() >= 150 and (z > 0).sum() > 1000
    if name == "nonrigid":
        B = c["c2ws"][:, :3, :3].astype(np.float64)
        assert (np.abs(B @ B.transpose(0, 2, 1) - np.eye(3)).max((1, 2)) > 0.05).all()
        assert (np.linalg.det(B) > 0.5).all() and (np.linalg.cond(B) < 2.6).all()
        assert (r["ray_kept"] > 0).sum() >= 10
    if name == "duplicate":
        assert c["frame_indices"][0] == c["frame_indices"][1]
        own = c["indices"] == c["frame_indices"][0]
        assert own.any() and not r["mask"][own][:, :2].any() and r["mask"][~own][:, :2].any()


@pytest.mark.parametrize("name", ["m5", "m6", "m64", "nonrigid", "duplicate", "n1", "n257"])
def test_warp_terms_are_the_restatement(name):
    c, r = scene(name)
    t = lambda k: torch.from_numpy(np.ascontiguousarray(c[k]))
    dep = t("depth").double().requires_grad_(True)
    loss, mask = pix_warp_loss(t("rays_o"), t("rays_d"), dep, t("c2ws"), c["fx"], c["fy"], c["cx"], c["cy"], c["W"],
                               c["H"], t("frame_indices"), t("indices"), t("images"), t("gt"))
    loss.backward()
    assert np.array_equal(mask.numpy(), r["mask"]) and r["count"] == int(mask.sum())
    assert abs(float(loss.detach()) - r["loss"]) <= 1e-13 * abs(r["loss"])
    g = dep.grad.numpy()
    assert np.abs(g - r["grad"]).max() <= 1e-12 * np.abs(g).max()
    assert (r["scale"] >= np.abs(r["grad"])).all() and ((r["scale"] == 0) == (r["ray_kept"] == 0)).all()
    full = ms.blocked_loss(r["ray_loss"], r["ray_kept"])
    assert full[1] == r["count"] and abs(full[0] - r["loss"]) <= 1e-13 * abs(r["loss"])


def test_warp_float32_figure():
    """the float32 evaluation decides as float64 does on the firm scenes; its gradient error relative to the scale"""
    worst = {}
    for name in ms.WARP_SCENES:
        c, r = scene(name)
        r32 = ms.warp_terms(c, np.float32)
        assert r32["grad"].dtype == np.float32 and np.array_equal(r32["mask"], r["mask"])
        k = r["scale"] > 0
        worst[name] = float((np.abs(r32["grad"] - r["grad"])[k] / r["scale"][k]).max())
        assert abs(r32["loss"] - r["loss"]) <= LOSS_RTOL * abs(r["loss"])
    print("float32 gradient error / scale:", {k: f"{v:.2e}" for k, v in worst.items()})
    assert 4 * max(worst.values()) <= GRAD_BOUND                         # what the mutations below are held against


@pytest.mark.parametrize("mutate", ["fy_fx", "no_translation", "cofactor"])
@pytest.mark.parametrize("name", ["m5", "m64", "nonrigid"])
def test_warp_scenes_catch_a_wrong_projection(name, mutate):
    c, r = scene(name)
    w = ms.warp_terms(c, mutate=mutate)
    flipped = int((w["mask"] != r["mask"]).sum())
    dl = abs(w["loss"] - r["loss"]) / abs(r["loss"]) if w["count"] else np.inf
    same = (w["ray_kept"] == r["ray_kept"]) & (w["mask"] == r["mask"]).all(1) & (r["ray_kept"] > 0)
    dg = float((np.abs(w["grad"] - r["grad"])[same] / r["scale"][same]).max()) if same.any() else np.inf
    print(f"{name} {mutate}: kept entries {r['count']} -> {w['count']} ({flipped} flipped), loss off by {dl:.2e}, "
          f"gradient off by {dg:.2e} of the scale on rays that keep their frames")
    assert flipped > 0 and w["count"] != r["count"]                      # the count must be exact
    assert dl >= 100 * LOSS_RTOL
    assert dg >= 100 * GRAD_BOUND


def test_warp_scene_catches_a_finish_pass_without_its_loop():
    c, r = scene("n65537")
    assert len(r["ray_loss"]) == 65537 and r["ray_kept"][65536] >= 4
    full = ms.blocked_loss(r["ray_loss"], r["ray_kept"])
    cut = ms.blocked_loss(r["ray_loss"], r["ray_kept"], max_parts=256)
    assert full[1] == r["count"] and cut[1] == r["count"] - r["ray_kept"][65536] != full[1]


# ---- frustum selection and keyframe overlap --------------------------------------------------------------------------
def mutated_project(mutate):
    """keyframe_select_ref.project with one deliberate mistake"""
    def project(c2w, X, fx, fy, cx, cy):
        w2c = ms.mutate_w2c(np.linalg.inv(np.asarray(c2w, np.float64)), mutate)
        p = np.asarray(X, np.float64) @ w2c[:3, :3].T + w2c[:3, 3]
        a, b, c = -p[:, 0], p[:, 1], p[:, 2]
        z = c + 1e-5
        return (fx * a + cx * c) / z, ((fx if mutate == "fy_fx" else fy) * b + cy * c) / z, z
    return project


FRUSTUM = [(shape, n, kind) for shape in ((23, 37), (48, 64)) for n in (1, 257, 3000) for kind in ("holes", "patch")]


def test_mutated_project_is_the_restatement_when_unmutated():
    s = ms.frustum_scene(23, 37, 257, seed=1)
    for a, b in zip(mutated_project(None)(s["c2w"], s["points"], *s["K"]), ksr.project(s["c2w"], s["points"], *s["K"])):
        assert np.array_equal(a, b)


@pytest.mark.parametrize("shape,n,kind", FRUSTUM)
def test_frustum_scene_populations(shape, n, kind):
    H, W = shape
    s = ms.frustum_scene(H, W, n, seed=n + H, kind=kind)
    assert s["points"].shape == (n, 3) and s["points"].dtype == np.float32 and np.abs(s["c2w"][:3, 3]).min() > 0.05
    for edge in (-4.0, 6.0):
        mask, d = ksr.frustum_ref(s["points"], s["c2w"], s["depth"], *s["K"], H, W, edge)
        assert not ms.frustum_near(d, H, W, edge).any()                  # every point is firm
        u_out, v_out = ~((d["u"] < W - edge) & (d["u"] > edge)), ~((d["v"] < H - edge) & (d["v"] > edge))
        behind, far = d["negz"] < 0, d["negz"] > d["depth"] + 0.5
        alone = lambda x: int((x & ((u_out.astype(int) + v_out + behind + far) == 1)).sum())
        replaced = (d["sample"] == 0) & ~u_out & ~v_out & ~behind
        print(f"{kind} {H}x{W} n {n} edge {edge}: kept {mask.sum()}, rejected only by u {alone(u_out)} v {alone(v_out)}"
              f" behind {alone(behind)} too far {alone(far)}, decided by the maximum {replaced.sum()}")
        if n >= 257:
            assert mask.sum() >= 8 and min(alone(u_out), alone(v_out), alone(behind), alone(far)) >= 1
            assert replaced.sum() >= 5 and (mask & replaced).any() and (~mask & replaced).any()
            if kind == "patch":
                assert 0 < (d["sample"] > 0).sum() <= 0.05 * n and d["sample"].max() > 2.0
            else:
                assert (d["sample"] > 0).sum() >= 0.2 * n


@pytest.mark.parametrize("mutate", ["fy_fx", "no_translation", "cofactor"])
def test_frustum_and_overlap_scenes_catch_a_wrong_projection(monkeypatch, mutate):
    for (H, W), n, kind in FRUSTUM:
        if n < 257:
            continue
        s = ms.frustum_scene(H, W, n, seed=n + H, kind=kind)
        for edge in (-4.0, 6.0):
            monkeypatch.undo()
            want, _ = ksr.frustum_ref(s["points"], s["c2w"], s["depth"], *s["K"], H, W, edge)
            monkeypatch.setattr(ksr, "project", mutated_project(mutate))
            got, _ = ksr.frustum_ref(s["points"], s["c2w"], s["depth"], *s["K"], H, W, edge)
            print(f"{mutate}: frustum {kind} {H}x{W} n {n} edge {edge}: {int((got != want).sum())} decisions flipped")
            assert (got != want).sum() >= (20 if n == 3000 else 1), (H, W, n, kind, edge, int((got != want).sum()))
    for n_kf, R, S in ((1, 37, 3), (5, 200, 8), (64, 300, 9)):
        s = ms.overlap_scene(n_kf, R, S, seed=7 * n_kf + R)
        args = (s["rays_o"], s["rays_d"], s["depth"], s["c2ws"], *s["K"], s["H"], s["W"])
        monkeypatch.undo()
        want, _ = ksr.overlap_ref(*args, n_samples=S, edge=s["edge"])
        monkeypatch.setattr(ksr, "project", mutated_project(mutate))
        got, _ = ksr.overlap_ref(*args, n_samples=S, edge=s["edge"])
        assert (got != want).sum() >= max(1, n_kf // 4), (n_kf, got, want)


OVERLAP = [(n_kf, R, S) for n_kf in (1, 5, 64) for R, S in ((1, 1), (1, 8), (37, 3), (200, 8), (300, 9))]


@pytest.mark.parametrize("n_kf,R,S", OVERLAP)
def test_overlap_scene_populations(n_kf, R, S):
    s = ms.overlap_scene(n_kf, R, S, seed=7 * n_kf + R)
    valid = s["depth"] > 0
    pts = ms.overlap_samples(s["rays_o"][valid], s["rays_d"][valid], s["depth"][valid], S).reshape(-1, 3)
    assert np.array_equal(pts, ksr.sample_points(s["rays_o"], s["rays_d"], s["depth"], S))
    _, near = ms.overlap_inside(pts, s["c2ws"], s["K"], s["H"], s["W"], s["edge"])
    assert not near.any()                                                # every sample is firm in every keyframe
    want, total = ksr.overlap_ref(s["rays_o"], s["rays_d"], s["depth"], s["c2ws"], *s["K"], s["H"], s["W"], n_samples=S,
                                  edge=s["edge"])
    assert total == valid.sum() * S and (R < 37 or 0 < (~valid).sum() < R)
    print(f"K {n_kf} R {R} S {S}: {total} samples, keyframes with no {(want == 0).sum()}, all {(want == total).sum()},"
          f" some {((want > 0) & (want < total)).sum()}")
    if n_kf >= 5:
        assert want[0] == total and want[2] == 0                         # the rays' own camera, a camera turned away
    if n_kf >= 5 and R >= 37:
        assert ((want > 0) & (want < total)).sum() >= 3


@pytest.mark.parametrize("n_kf", [1, 5, 64])
def test_overlap_scene_catches_a_single_sample_at_the_far_end(monkeypatch, n_kf):
    assert torch.linspace(0.0, 1.0, 1).tolist() == [0.0] and np.linspace(0.0, 1.0, 1).tolist() == [0.0]
    s = ms.overlap_scene(n_kf, 1, 1, seed=7 * n_kf + 1)
    args = (s["rays_o"], s["rays_d"], s["depth"], s["c2ws"], *s["K"], s["H"], s["W"])
    want, _ = ksr.overlap_ref(*args, n_samples=1, edge=s["edge"])

    def far_end(rays_o, rays_d, depth, n_samples):
        keep = np.asarray(depth) > 0
        return ms.overlap_samples(rays_o[keep], rays_d[keep], depth[keep], n_samples, single_t=1.0).reshape(-1, 3)
    monkeypatch.setattr(ksr, "sample_points", far_end)
    got, _ = ksr.overlap_ref(*args, n_samples=1, edge=s["edge"])
    assert (got != want).any(), (got, want)


# ---- colour-gradient maps --------------------------------------------------------------------------------------------
COLOR_SIZES = [(1, 1), (1, 17), (17, 1), (15, 16), (16, 16), (17, 33), (37, 53)]


def float32_maps(image):
    """gray, Sobel and magnitude in float32 numpy (the radii come from that magnitude in double, as in the kernel)"""
    im = np.asarray(image, np.float32)
    co = np.array([0.2125, 0.7154, 0.0721], np.float32)
    gray = (im[..., 0] * co[0] + im[..., 1] * co[1]) + im[..., 2] * co[2]
    g = np.pad(gray, 1, mode="edge")
    s = lambda a: (a[..., :-2] + np.float32(2) * a[..., 1:-1] + a[..., 2:]) / np.float32(4)
    gy = s(g[2:, :]) - s(g[:-2, :])
    gx = (s(g[:, 2:].T) - s(g[:, :-2].T)).T
    mag = np.sqrt(gx * gx + gy * gy)
    assert mag.dtype == np.float32
    return mag


def test_color_images_cover_the_radius_map():
    im = ms.color_image(37, 53, seed=9, kind="segments")
    mag = color_grad_ref.sobel_magnitude(im["image"])
    thr = float(np.float32(0.15))
    flat, slope, clipped = mag < 0.01, (mag > 0.011) & (mag < 0.149), mag > thr
    print("pixels below 0.01:", flat.sum(), "on the slope:", slope.sum(), "clipped:", clipped.sum())
    assert min(flat.sum(), slope.sum(), clipped.sum()) >= 300
    ref = color_grad_ref.color_grad_maps_ref(im["image"])
    assert (ref["r_add"][flat] == 0.08).all() and np.allclose(ref["r_add"][clipped], 0.02, atol=1e-9)
    assert ((ref["r_add"][slope] < 0.0796) & (ref["r_add"][slope] > 0.0204)).all()
    assert 0.2 < im["valid"].mean() < 0.9
    for H, W in COLOR_SIZES:                                             # noise: the border carries large gradients
        if H * W > 1:
            m = color_grad_ref.sobel_magnitude(ms.color_image(H, W, seed=H * 64 + W)["image"])
            assert m[ms.border_mask(H, W)].max() > 0.05


@pytest.mark.parametrize("H,W", COLOR_SIZES)
def test_color_bounds_hold_for_a_float32_evaluation(H, W):
    worst = {}
    for im in [ms.color_image(H, W, seed=H * 64 + W)] + ([ms.color_image(H, W, seed=9, kind="segments")]
                                                         if (H, W) == (37, 53) else []):
        mag32 = float32_maps(im["image"])
        for depth in (None, im["depth"]):
            ref = color_grad_ref.color_grad_maps_ref(im["image"], depth_add=depth, depth_query=depth)
            b = ms.color_grad_bounds(ref, im["image"], depth_add=depth, depth_query=depth)
            got = dict(grad=mag32.astype(np.float64))
            for name, k in (("r_add", 1.0), ("r_query", 2.0)):
                r = color_grad_ref.radius_map(mag32.astype(np.float64), k * 0.08, k * 0.02, 0.15)
                got[name] = (r if depth is None else r / 3.0 * depth.astype(np.float64)).astype(np.float32)
            for name in got:
                worst[name] = max(worst.get(name, 0.0), float((np.abs(got[name] - ref[name]) / b[name]).max()))
    print(f"{H}x{W}: float32 evaluation / derived bound", {k: f"{v:.2f}" for k, v in worst.items()})
    assert max(worst.values()) <= 1.0, worst


def zero_border_magnitude(image):
    """color_grad_ref.sobel_magnitude with a zero border in place of the repeated border pixel"""
    g = np.pad(color_grad_ref.gray(image), 1, mode="constant")
    s = lambda a: (a[..., :-2] + 2 * a[..., 1:-1] + a[..., 2:]) / 4
    gy = s(g[2:, :]) - s(g[:-2, :])
    gx = (s(g[:, 2:].T) - s(g[:, :-2].T)).T
    return np.sqrt(gx ** 2 + gy ** 2)


@pytest.mark.parametrize("H,W", COLOR_SIZES[1:])
def test_color_images_catch_a_zero_border(monkeypatch, H, W):
    im = ms.color_image(H, W, seed=H * 64 + W)
    ref = color_grad_ref.color_grad_maps_ref(im["image"])
    b = ms.color_grad_bounds(ref, im["image"])
    monkeypatch.setattr(color_grad_ref, "sobel_magnitude", zero_border_magnitude)
    wrong = color_grad_ref.color_grad_maps_ref(im["image"])
    border = ms.border_mask(H, W)
    off = np.abs(wrong["grad"] - ref["grad"]) / b["grad"]
    assert np.median(off[border]) >= 100 and (off[~border] == 0).all()   # most border pixels, and only they
    assert (np.abs(wrong["r_add"] - ref["r_add"]) / b["r_add"])[border].max() >= 100
