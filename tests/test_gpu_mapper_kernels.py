"""The mapper's window kernels on general cameras: the pixel-warping loss (csrc/warp.hip), frustum feature selection and
keyframe overlap (csrc/select.hip) and the colour-gradient maps (csrc/color_grad.hip) against their float64
restatements (tests/pix_warp_ref.py, tests/keyframe_select_ref.py, tests/color_grad_ref.py - each pinned to the
reference's own recordings without a GPU) on the scenes of tests/mapper_scenes.py: general rotations with translation,
fx != fy, an off-centre principal point, cameras turned away, ragged sizes.  tests/test_mapper_scenes.py shows without a
GPU that these scenes hold what they are there for and tell six deliberately wrong kernels from a right one.

The scenes are firm (mapper_scenes: whatever sits near a threshold is redrawn in the generator), so every ray, point and
sample is compared and every decision - the kept (ray, frame) count, the frustum mask, count and indices, the overlap
counts - must be exactly the restatement's.

Pixel-warping loss.  Loss: relative 1e-5 against float64.  Gradient: per ray,
    |kernel - float64| <= 4 E32 * scale(ray),
scale the ray's sum of |terms| (mapper_scenes.warp_terms) and E32 the largest error, relative to that scale, of the same
formulas evaluated in float32 numpy on the host over all the warp scenes of this file.  Measured E32 = 4.8e-8 (the
65537-ray scene; the smaller scenes give 5e-9 ... 3.6e-8), so the bound is 1.9e-7 of the scale; the kernel's largest
error is 4.6e-8 of it.  The kernel contracts to FMA and inverts the pose in double: its rounding differs from a float32
composition but is of the same order.  The figure is computed where the test runs, not copied from here.  A ray with
fewer than 4 frames in view has scale 0: its gradient must be exactly 0.

Colour-gradient maps, from the fp32 unit roundoff u = 2^-24 (mapper_scenes.color_grad_bounds; G = max |rgb|):
    gray   three rounded coefficients and three rounded operations, partial sums <= G:                 4 u G
    Sobel  six taps of total weight 2 summed in double, rounded once to fp32:                  8 u G + u |gx|
    grad   sqrt(gx^2 + gy^2), four roundings (a relative 2 u), the inputs' errors at most sqrt(2)-fold:
           |kernel - float64| <= u (12 G + 3.5 grad)
    radii  continuous and piecewise linear: that times |slope| = (rmax - rmin) / (thr - 0.01) (times depth / 3 when
           scaled) plus one fp32 ulp of the radius.
A float32 numpy evaluation of the same formulas stays within 0.21 of the grad bound and 0.15 of the radius bounds on
these images (test_mapper_scenes.test_color_bounds_hold_for_a_float32_evaluation): the derived bounds stand as they are.
Border rows and columns are asserted apart from the interior."""
import functools

import numpy as np
import pytest
import torch

import mapper_scenes as ms
from color_grad_ref import color_grad_maps_ref
from keyframe_select_ref import frustum_ref, overlap_ref
from pix_warp_ref import pix_warp_loss as ref_loss

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def warp_case(name):
    """the scene, its float64 restatement (loss, gradient, mask), the per-ray scale and the float32 figure"""
    c = ms.warp_scene(**ms.WARP_SCENES[name])
    t = lambda k: torch.from_numpy(np.ascontiguousarray(c[k]))
    dep = t("depth").double().requires_grad_(True)
    loss, mask = ref_loss(t("rays_o"), t("rays_d"), dep, t("c2ws"), c["fx"], c["fy"], c["cx"], c["cy"], c["W"], c["H"],
                          t("frame_indices"), t("indices"), t("images"), t("gt"))
    loss.backward()
    t64, t32 = ms.warp_terms(c), ms.warp_terms(c, np.float32)
    assert np.array_equal(t64["mask"], mask.numpy()) and np.array_equal(t32["mask"], t64["mask"])
    kept = t64["scale"] > 0
    e32 = float((np.abs(t32["grad"] - t64["grad"])[kept] / t64["scale"][kept]).max())
    return dict(c=c, loss=float(loss.detach()), grad=dep.grad.numpy(), mask=mask.numpy(), scale=t64["scale"], e32=e32)


@functools.lru_cache(maxsize=None)
def warp_e32():
    e = {name: warp_case(name)["e32"] for name in ms.WARP_SCENES}
    print("float32 gradient error / scale per scene:", {k: f"{v:.2e}" for k, v in e.items()})
    return max(e.values())


def _hip_warp(c, dev, layout, nan_to_zero=False):
    from glorie_slam_amd.warp_loss import FrameTable, pix_warping_loss
    t = lambda k: torch.from_numpy(np.ascontiguousarray(c[k])).to(dev)
    dep = t("depth").requires_grad_(True)
    imgs = t("images")
    if layout == "table":
        imgs = FrameTable([im.permute(2, 0, 1).contiguous() for im in imgs], channels_first=True)
    elif layout == "chw":
        imgs = imgs.permute(0, 3, 1, 2).contiguous()
    loss, count = pix_warping_loss(t("rays_o"), t("rays_d"), dep, t("c2ws"), c["fx"], c["fy"], c["cx"], c["cy"], c["W"],
                                   c["H"], t("frame_indices"), t("indices"), imgs, t("gt"), nan_to_zero=nan_to_zero,
                                   channels_first=layout == "chw", return_count=True)
    loss.backward()
    torch.cuda.synchronize()
    return loss.detach().cpu(), dep.grad.cpu(), int(count)


def _check_warp(gpu, name, layouts):
    r = warp_case(name)
    c, bound = r["c"], 4.0 * warp_e32()
    out = [_hip_warp(c, gpu, lay) for lay in layouts]
    loss, grad, count = out[0]
    for other in out[1:]:                                         # the layouts read the same texels
        assert torch.equal(other[0], loss) and torch.equal(other[1], grad) and other[2] == count
    assert count == int(r["mask"].sum()), (count, int(r["mask"].sum()))
    assert abs(float(loss) - r["loss"]) <= 1e-5 * abs(r["loss"]), (float(loss), r["loss"])
    err = np.abs(grad.double().numpy() - r["grad"])
    dropped = r["mask"].sum(1) == 0
    assert (grad.numpy()[dropped] == 0).all()
    kept = ~dropped
    ratio = err[kept] / r["scale"][kept]
    print(f"{name}: kept entries {count}, loss {float(loss):.6f}, gradient error / scale {ratio.max():.2e} / {bound:.1e}")
    assert (err <= bound * r["scale"]).all(), (int(np.argmax(err - bound * r["scale"])), ratio.max(), bound)
    return r


@pytest.mark.parametrize("name", ["m5", "m6", "m63", "m64", "nonrigid", "duplicate"])
def test_warp_matches_the_restatement_on_general_windows(gpu, name):
    r = _check_warp(gpu, name, ("hwc", "table", "chw") if name in ("m5", "m63") else ("hwc", "table"))
    if name == "m64":                                             # bit 63 of the per-ray frame mask is used
        assert r["mask"][:, 63].any()


@pytest.mark.parametrize("N", [1, 255, 256, 257, 65537])
def test_warp_matches_the_restatement_at_ragged_ray_counts(gpu, N):
    """one ray, a workgroup less one, one workgroup, one more, and 257 partial sums: the finish pass's second trip"""
    r = _check_warp(gpu, f"n{N}", ("hwc", "table"))
    assert r["mask"][N - 1].sum() >= 4                            # the last partial sum carries a count


def test_warp_arguments(gpu):
    c = dict(warp_case("m5")["c"])
    # a window of 4 whose rays all start in it: 3 other frames at the most, nothing is kept
    own = np.isin(c["indices"], c["frame_indices"][:4])
    four = {**c, "c2ws": c["c2ws"][:4], "frame_indices": c["frame_indices"][:4], "images": c["images"][:4],
            **{k: c[k][own] for k in ("rays_o", "rays_d", "depth", "indices", "gt")}}
    assert own.sum() > 100 and not ms.warp_terms(four)["mask"].any()
    for layout in ("hwc", "table"):
        loss, grad, count = _hip_warp(four, gpu, layout)
        assert torch.isnan(loss) and (grad == 0).all() and count == 0
        loss0, grad0, _ = _hip_warp(four, gpu, layout, nan_to_zero=True)
        assert float(loss0) == 0.0 and (grad0 == 0).all()
    # 65 frames, and images of 10 rows or columns: refused by the wrapper and by the C entry point
    many = {**c, "c2ws": np.repeat(c["c2ws"][:1], 65, 0), "frame_indices": np.arange(65),
            "images": np.repeat(c["images"][:1], 65, 0)}
    with pytest.raises(ValueError, match="up to 64 frames"):
        _hip_warp(many, gpu, "hwc")
    from glorie_slam_amd import _lib as L
    for H, W in ((10, 37), (23, 10)):
        small = {**c, "H": H, "W": W, "images": np.zeros((5, H, W, 3), np.float32)}
        with pytest.raises(L.GlorieError):
            _hip_warp(small, gpu, "hwc")
    lib, f = L.load(), torch.zeros(64, device=gpu)
    i64 = torch.zeros(64, dtype=torch.int64, device=gpu)
    args = lambda M, H, W: (L.ptr(f), L.ptr(f), L.ptr(f), L.ptr(i64), 1, L.ptr(f), L.ptr(i64), M, L.ptr(f), None, 0, H,
                            W, 1.0, 1.0, 1.0, 1.0, L.ptr(f), 0, L.ptr(f), L.ptr(f), L.ptr(f), L.ptr(f), None, None)
    for M, H, W in ((65, 23, 37), (5, 10, 37), (5, 23, 10)):
        assert lib.glorie_pix_warp_fwd(*args(M, H, W)) != 0


# ---- frustum selection -----------------------------------------------------------------------------------------------
def _t(x, dev):
    return torch.from_numpy(np.ascontiguousarray(x)).to(dev)


@pytest.mark.parametrize("shape", [(23, 37), (48, 64)])
@pytest.mark.parametrize("n", [1, 257, 3000])
@pytest.mark.parametrize("kind", ["holes", "patch"])
def test_frustum_is_the_restatement_on_a_general_camera(gpu, shape, n, kind):
    from glorie_slam_amd.keyframe_select import frustum_feature_mask
    s = ms.frustum_scene(*shape, n, seed=n + shape[0], kind=kind)
    H, W = shape
    for edge in (-4.0, 6.0):
        mask, count, idx = frustum_feature_mask(_t(s["points"], gpu), _t(s["c2w"], gpu), _t(s["depth"], gpu), *s["K"],
                                                H, W, edge, return_indices=True)
        torch.cuda.synchronize()
        want, d = frustum_ref(s["points"], s["c2w"], s["depth"], *s["K"], H, W, edge)
        got = mask.cpu().numpy().astype(bool)
        print(f"{kind} {H}x{W} n {n} edge {edge}: kept {int(count)}, restatement {int(want.sum())}, "
              f"samples replaced by the maximum {int((d['sample'] == 0).sum())}")
        assert np.array_equal(got, want), np.nonzero(got != want)[0][:10]
        assert int(count) == int(want.sum())
        assert np.array_equal(idx[:int(count)].cpu().numpy(), np.nonzero(want)[0])


# ---- keyframe overlap ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_kf", [1, 5, 64])
@pytest.mark.parametrize("R,n_samples", [(1, 1), (1, 8), (37, 3), (200, 8), (300, 9)])
def test_overlap_counts_are_the_restatement(gpu, n_kf, R, n_samples):
    from glorie_slam_amd.keyframe_select import keyframe_overlap
    s = ms.overlap_scene(n_kf, R, n_samples, seed=7 * n_kf + R)
    inside, total = keyframe_overlap(_t(s["rays_o"], gpu), _t(s["rays_d"], gpu), _t(s["depth"], gpu),
                                     _t(s["c2ws"], gpu), *s["K"], s["H"], s["W"], n_samples=n_samples, edge=s["edge"],
                                     return_counts=True)
    want, wtotal = overlap_ref(s["rays_o"], s["rays_d"], s["depth"], s["c2ws"], *s["K"], s["H"], s["W"],
                               n_samples=n_samples, edge=s["edge"])
    got = inside.cpu().numpy()
    print(f"K {n_kf} R {R} S {n_samples}: counts {got[:8]} restatement {want[:8]} of {wtotal}")
    assert int(total) == wtotal == int((s["depth"] > 0).sum()) * n_samples
    assert np.array_equal(got, want), (got, want)


# ---- colour-gradient maps --------------------------------------------------------------------------------------------
COLOR_SIZES = [(1, 1), (1, 17), (17, 1), (15, 16), (16, 16), (17, 33), (37, 53)]


def _check_color(gpu, im, chw, with_valid, with_depth):
    from glorie_slam_amd.color_grad import color_grad_maps
    H, W = im["valid"].shape
    img = _t(im["image"], gpu)
    if chw:
        img = img.permute(2, 0, 1).contiguous()
    valid = im["valid"] if with_valid else None
    depth = im["depth"] if with_depth else None
    got = color_grad_maps(img, valid=_t(valid, gpu) if with_valid else None,
                          depth_add=_t(depth, gpu) if with_depth else None,
                          depth_query=_t(depth, gpu) if with_depth else None)
    torch.cuda.synchronize()
    ref = color_grad_maps_ref(im["image"], valid=valid, depth_add=depth, depth_query=depth)
    bounds = ms.color_grad_bounds(ref, im["image"], depth_add=depth, depth_query=depth)
    border = ms.border_mask(H, W)
    for name in ("grad", "r_add", "r_query"):
        g = got[name].cpu().numpy().astype(np.float64)
        assert g.shape == (H, W)
        if name == "grad" and with_valid:
            assert (g[~valid] == -1.0).all()
        err, b = np.abs(g - ref[name]), bounds[name]
        for where, sel in (("border", border), ("interior", ~border)):
            if sel.any():
                assert (err[sel] <= b[sel]).all(), (name, where, H, W, chw, float((err[sel] / b[sel]).max()))


@pytest.mark.parametrize("chw", [False, True])
@pytest.mark.parametrize("H,W", COLOR_SIZES)
def test_color_grad_maps_at_ragged_sizes(gpu, H, W, chw):
    im = ms.color_image(H, W, seed=H * 64 + W)
    for with_valid in (False, True):
        for with_depth in (False, True):
            _check_color(gpu, im, chw, with_valid, with_depth)


@pytest.mark.parametrize("chw", [False, True])
def test_color_grad_maps_on_the_three_radius_segments(gpu, chw):
    im = ms.color_image(37, 53, seed=9, kind="segments")
    for with_depth in (False, True):
        _check_color(gpu, im, chw, True, with_depth)
