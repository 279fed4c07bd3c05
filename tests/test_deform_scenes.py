"""The scenes of tests/deform_scenes.py and the float32 compositions of tests/deform_ref.py, checked without a GPU:

  * the cameras are general (quaternion components, fx against fy, principal point, translation);
  * every deformation scene holds its planted keyframes, points and layouts, every z-buffer scene its planted points,
    each with the outcome it is there for; at most 1 % of a z-buffer scene's bits are cleared for firmness and the
    float32 composition puts every firm point in the pixel float64 puts it in;
  * the scale: the integer sums deform.hip documents, carried out exactly, stay within 2^(2b-61) of the exact rational
    quotient in every keyframe of every scene (b: the bit length of the count) - the premise of the bound
    tests/test_gpu_deform_kernels.py derives - while a sequential float32 sum misses the nearest float32 on the
    wide-range keyframes (else the assertion on the scale would be vacuous), and an exponent without the bit length
    overflows int64 on the narrow ones;
  * deliberate mistakes in the restatement each change its output: fx and fy swapped, a rotation entry transposed, cx in
    place of cy, the skipped row dropped, >= turned into > at the zero border; t = 1 for a single sample;
  * torch.linspace with one step returns its start."""
import fractions

import numpy as np
import pytest
import torch

import deform_scenes as ds
from deform_ref import deform_ref, linspace_two_sided, proj_depth_ref, quat_rot

SIZES = (1, 63, 64, 65, 257, 1000)


def _deform(c, N_add=3, fix=False, **kw):
    return deform_ref(c["poses"], c["disps_up"], c["valid"], c["dirty"], *ds.ref_indices(c), c["prev"], N_add,
                      ds.NEAR, ds.FAR, fix, *c["K"], **kw)


def _proj(c, **kw):
    return proj_depth_ref(c["full_pcl"], c["full_mask"], c["counter"], 0, None, *c["K"],
                          **{"w2c": c["w2c"], "row": -1, **kw})


def test_cameras_are_general():
    rng = np.random.default_rng(3)
    for _ in range(20):
        p = ds.general_pose(rng)
        assert np.abs(p[3:]).min() >= ds.Q_MIN and np.abs(p[:3]).min() >= 0.2
        R = quat_rot(p[3:])
        assert np.abs(R @ R.T - np.eye(3)).max() < 1e-6 and np.abs(R).max() < 0.999
    for n in SIZES:
        c = ds.deform_scene(n)
        assert np.abs(c["poses"][:, 3:]).min() >= ds.Q_MIN and np.abs(c["poses"][:, :3]).min() >= 0.2
    for (H, W), (fx, fy, cx, cy) in ds.ZK.items():
        assert 0.19 <= abs(fx - fy) / max(fx, fy) <= 0.25
        assert cx != cy and abs(cx - (W - 1) / 2) > 0.3 and abs(cy - (H - 1) / 2) > 0.3 and cx != W / 2 and cy != H / 2
    for H, W, counter in ds.ZBUF_SCENES:
        c = ds.zbuf_scene(H, W, counter)
        assert np.abs(c["c2w"][:3, :3]).min() >= 0.2 and np.abs(c["c2w"][:3, 3]).min() >= 0.2


@pytest.mark.parametrize("n", SIZES)
def test_deform_scene_populations(n):
    scenes = {lay: ds.deform_scene(n, lay) for lay in ds.LAYOUTS}
    c = scenes["runs"]
    assert len(c["vidx"]) == n and c["B"] == 7 and (c["H"], c["W"]) == (23, 37)
    assert c["dirty"].sum() == 6 and not c["dirty"][ds.CLEAN] and not (c["vidx"] == ds.EMPTY).any()
    for lay, s in scenes.items():                                   # the same points in another order
        back = np.argsort(s["ids"])
        for k in ("vidx", "pj", "pi", "prev"):
            assert np.array_equal(s[k][back], c[k][np.argsort(c["ids"])])
        ok = ds.in_range(s)
        px = s["vidx"][ok] * 10000 + s["pj"][ok] * 100 + s["pi"][ok]
        assert len(np.unique(px)) == ok.sum()                       # a pixel of its own per point
    frame = np.where(ds.moved(c), c["vidx"], -1)
    valid_count = {v: len(ds.frame_terms(c, v)[0]) for v in range(c["B"])}
    if n >= 257:
        assert valid_count[ds.ONE] == 1 and valid_count[ds.K63] == 63 and valid_count[ds.K64] == 64
        assert valid_count[ds.HOLES] == 0 and (frame == ds.HOLES).sum() >= 40 and valid_count[ds.WIDE] >= 17
        assert (c["vidx"] == ds.CLEAN).sum() >= 20
        # one hole point with previous depth 1.0f per dirty keyframe with points
        unit = np.isin(c["ids"], c["unit"])
        assert sorted(c["vidx"][unit]) == [ds.WIDE, ds.ONE, ds.K63, ds.K64, ds.HOLES]
        assert (c["prev"][unit] == np.float32(1)).all() and not c["valid"][c["vidx"][unit], c["pj"][unit], c["pi"][unit]].any()
        oor = np.isin(c["ids"], c["oor"])
        bad = sorted(zip(c["vidx"][oor], c["pj"][oor], c["pi"][oor]))
        assert [b[0] for b in bad] == [-1, ds.WIDE, ds.WIDE, c["B"]] and (ds.WIDE, c["H"], 7) in bad and (ds.WIDE, 8, -1) in bad
        assert not ds.in_range(c)[oor].any() and ds.in_range(c).sum() == n - 4
        # layouts: the runs are no multiples of 64 and some wave holds one keyframe; interleaved, none does
        runs = np.diff(np.concatenate([[0], np.nonzero(np.diff(frame))[0] + 1, [n]]))
        assert (runs[runs > 1] % 64 != 0).all() and runs.max() >= 65
        pad = lambda s: np.concatenate([np.where(ds.moved(s), s["vidx"], -1), np.full(-n % 64, -1)])   # lanes past n: -1
        waves = lambda s: pad(s).reshape(-1, 64)
        assert any(len(np.unique(w)) == 1 and w[0] >= 0 for w in waves(c))
        assert not any(len(np.unique(w)) == 1 for w in waves(scenes["interleaved"]))
        mixed = [len(np.unique(w)) for w in waves(scenes["mixed"])]
        assert min(mixed) >= 1 and max(mixed) >= 3
    prev = c["prev"][ds.in_range(c)]
    assert prev.min() >= 1e-3 and prev.max() <= 1.3e3
    if n >= 257:
        assert prev.min() < 1e-2 and prev.max() > 1e2


@pytest.mark.parametrize("n", SIZES)
def test_scale_premises(n):
    c = ds.deform_scene(n)
    differs = 0
    for v in np.nonzero(c["dirty"])[0]:
        prev, d, holes = ds.frame_terms(c, v)
        if len(prev) == 0:
            assert ds.exact_scale(prev, d) is None
            continue
        exact = ds.exact_scale(prev, d)
        q, bits, top = ds.integer_scale(prev, d)
        rel = abs(q - exact) / exact
        assert bits == len(prev).bit_length() and top < 2 ** 61
        assert rel <= fractions.Fraction(2) ** (2 * bits - 61), (v, float(rel))
        lo, hi = ds.f32_neighbours(exact)
        assert fractions.Fraction(float(lo)) <= exact <= fractions.Fraction(float(hi)) and hi <= np.nextafter(lo, np.float32(np.inf))
        nearest = np.float32(float(exact))
        seq = ds.sequential_f32_scale(prev, d)
        print(f"n {n} keyframe {v}: {len(prev)} terms, integer quotient off by {float(rel):.1e}, sequential float32 "
              f"{'=' if seq == nearest else '!='} nearest float32 ({abs(float(seq) / float(exact) - 1):.1e})")
        differs += seq != nearest
        if v in (ds.K63, ds.K64) and n >= 257:
            # without the count's bit length in the exponent the sum of these terms leaves int64
            pp = [fractions.Fraction(float(p)) ** 2 for p in prev]
            pd = [fractions.Fraction(float(p)) * fractions.Fraction(float(x)) for p, x in zip(prev, d)]
            assert max(sum(pp), sum(pd)) / max(pp + pd) > 8
    if n >= 257:
        assert differs >= 2, "the sequential float32 sum lands on the nearest float32: the scale assertion is vacuous"


@pytest.mark.parametrize("n", [65, 1000])
def test_float32_composition_of_the_deformation(n):
    c = ds.deform_scene(n)
    live = ds.moved(c)
    for N_add, fix in ((1, False), (1, True), (2, False), (3, True), (5, False)):
        p64, d64, c64 = _deform(c, N_add, fix)
        p32, d32, c32 = _deform(c, N_add, fix, dtype=np.float32, new_depth=d64.astype(np.float32))
        assert p32.dtype == np.float32 and c32.dtype == np.float32
        rows = np.repeat(live, N_add)
        scale = np.abs(p64[live]).max(1, keepdims=True) + 1e-30
        assert np.isnan(p64[~live]).all() and np.isnan(c32[~rows]).all()
        e = np.abs(p32[live] - p64[live]) / scale
        assert 0 < e.max() < 1e-5, e.max()
        e = np.abs(c32[rows] - c64[rows]) / (np.abs(c64[rows]).max(1, keepdims=True) + 1e-30)
        assert 0 < e.max() < 1e-5, e.max()
        # a single sample sits at the near end / at -0.04
        if N_add == 1:
            two = _deform(c, 2, fix)[2]
            assert np.allclose(c64[rows], two[0::2][live], rtol=1e-12, atol=0)
            assert np.abs(c64[rows] / two[1::2][live] - 1).max() > 1e-3     # the far end (t = 1, +0.04) is elsewhere


@pytest.mark.parametrize("mutate", ["fy_fx", "cx_cy", "transpose"])
def test_deformation_mutations_change_the_output(mutate):
    c = ds.deform_scene(257)
    live = ds.moved(c)
    p, _, cl = _deform(c)
    q, _, cm = _deform(c, mutate=mutate)
    scale = np.abs(p[live]).max(1)
    off = np.abs(q[live] - p[live]).max(1) / scale
    print(f"{mutate}: positions move by {np.median(off):.2e} (median) of their size")
    assert np.median(off) > 1e-3 and (off > 1e-4).mean() > 0.9      # 100x any float32 error and more, nearly everywhere


@pytest.mark.parametrize("H,W,counter", ds.ZBUF_SCENES)
def test_zbuf_scene_populations(H, W, counter):
    c = ds.zbuf_scene(H, W, counter)
    assert c["full_pcl"].shape == (counter + 1, H, W, 3) and c["cleared"] <= 0.01, c["cleared"]
    ref, det = _proj(c, details=True)
    r32, d32 = _proj(c, details=True, dtype=np.float32)
    assert r32.dtype == np.float32
    print(f"{H} x {W} x {counter}: cleared share {c['cleared']:.4f}, covered pixels {(ref > 0).sum()} of {H * W}")
    if counter == 0:
        assert not ref.any() and not c["planted"]
        return
    # firm: every point read is DELTA away from a pixel border (where near the image) and from z = 0
    with np.errstate(invalid="ignore"):
        u, v, z = det["u"], det["v"], det["z"]
        for x, n in ((u, W), (v, H)):
            near = (x > -1) & (x < n + 1)
            assert np.abs(x - np.round(x))[near].min() >= ds.DELTA
        assert np.nanmin(np.abs(z)) >= ds.Z_MIN
        # float32 moves no point to another pixel, and by far less than DELTA
        assert np.array_equal(d32["inside"], det["inside"])
        m = det["inside"]
        assert np.array_equal(np.floor(d32["u"][m]), np.floor(u[m])) and np.array_equal(np.floor(d32["v"][m]), np.floor(v[m]))
        assert max(np.abs(d32["u"][m] - u[m]).max(), np.abs(d32["v"][m] - v[m]).max()) < ds.DELTA / 20
    assert np.array_equal(r32 > 0, ref > 0) and np.abs(r32[ref > 0] / ref[ref > 0] - 1).max() < 1e-5
    # planted points: present, firm (their bits are as planted), with the outcome they are there for
    P = c["planted"]
    assert set(P) == {"behind", "left", "right", "above", "below", "u_neg", "v_neg", "dup", "pair_nf", "pair_fn",
                      "masked", "inf", "nan", "row_first", "row_last"}
    bits, flat = c["full_mask"].reshape(-1), c["full_pcl"].reshape(-1, 3)
    where = {int(k): n for n, k in enumerate(det["index"])}
    at = lambda name: [where[k] for k in P[name]["index"] if k in where]
    for name, p in P.items():
        assert all(k < counter * H * W for k in p["index"])
        assert [bool(bits[k]) for k in p["index"]] == ([False, True] if name == "masked" else [True] * len(p["index"])), name
    for name in ("behind", "left", "right", "above", "below", "u_neg", "v_neg", "inf", "nan"):
        assert len(at(name)) == 1 and not det["inside"][at(name)].any(), name
    assert z[at("behind")[0]] > 1 and np.isinf(flat[P["inf"]["index"][0]]).any() and np.isnan(flat[P["nan"]["index"][0]]).any()
    assert -1 < u[at("u_neg")[0]] < 0 and 0 < v[at("u_neg")[0]] < H and -1 < v[at("v_neg")[0]] < 0 and 0 < u[at("v_neg")[0]] < W
    assert u[at("left")[0]] < -1 and u[at("right")[0]] > W + 1 and v[at("above")[0]] < -1 and v[at("below")[0]] > H + 1
    for name, row in (("row_first", 0), ("row_last", H - 1)):
        k, (r, col) = P[name]["index"][0], P[name]["pixel"]
        assert k // W == row and abs(ref[r, col] - 0.5) < 1e-5 and not abs(_proj(c, row=row)[r, col] - 0.5) < 1e-5
    for name in ("dup", "pair_nf", "pair_fn"):
        k = at(name)
        r, col = P[name]["pixel"]
        assert len(k) == 2 and det["inside"][k].all() and (np.floor(v[k]) == r).all() and (np.floor(u[k]) == col).all(), name
        assert abs(ref[r, col] - min(P[name]["depth"])) < 1e-5
    a, b = P["dup"]["index"]
    assert np.array_equal(flat[a], flat[b])
    assert -z[at("pair_nf")[0]] < -z[at("pair_nf")[1]] and -z[at("pair_fn")[0]] > -z[at("pair_fn")[1]]
    if counter >= 3:
        assert P["pair_fn"]["index"][0] >= H * W > P["pair_nf"]["index"][1] and b >= H * W > a
    r, col = P["masked"]["pixel"]
    assert len(at("masked")) == 1 and abs(ref[r, col] - 0.7) < 1e-5
    everything = c["full_mask"].copy()
    everything[:counter] = True
    with np.errstate(invalid="ignore"):
        assert abs(_proj({**c, "full_mask": everything})[r, col] - 0.4) < 1e-5
    # ordinary points are at least 1 away, the map behind the counter would have won everywhere it projects
    planted = np.isin(det["index"], [k for p in P.values() for k in p["index"]])
    assert (-z[det["inside"] & ~planted]).min() > 1.0
    beyond = _proj({**c, "counter": counter + 1})
    assert ((beyond > 0) & (beyond < 0.21)).sum() > H * W // 2
    # the skipped row matters at both ends and in the middle
    assert 0 < c["mid_row"] < H - 1
    for row in (0, H - 1, c["mid_row"]):
        assert not np.array_equal(_proj(c, row=row), ref), row


@pytest.mark.parametrize("mutate", ["fy_fx", "cx_cy", "transpose", "no_skip_row", "gt_zero"])
def test_projection_mutations_change_the_output(mutate):
    changed = []
    for c in [ds.zbuf_scene(23, 37, 3), ds.zbuf_scene(5, 7, 1), ds.border_scene()]:
        row = c["mid_row"]
        a, b = _proj(c, row=row), _proj(c, row=row, mutate=mutate)
        changed.append(float(((a > 0) != (b > 0)).mean()) + float((np.abs(a - b) > 1e-3 * np.abs(a)).mean()))
    print(mutate, changed)
    if mutate == "gt_zero":                                         # only an exact zero tells > from >=
        assert changed[0] == 0 and changed[1] == 0 and changed[2] > 0
    else:
        assert changed[0] > 0.02 and changed[1] > 0


def test_border_scene_is_exact():
    c = ds.border_scene()
    for dtype in (np.float64, np.float32):
        out, det = _proj(c, dtype=dtype, details=True)
        for name, axis in (("u_zero", "u"), ("v_zero", "v")):
            k = c["planted"][name]["index"][0]
            assert det[axis][k] == 0 and np.signbit(det[axis][k]) and det["inside"][k]
            assert abs(out[c["planted"][name]["pixel"]] - 2.0) < 1e-5
        assert (out == 0).sum() == 2 and (np.abs(out - 4.0) < 1e-5).sum() == out.size - 4   # their two slots are taken


def test_single_step_linspace_is_its_start():
    assert torch.linspace(0, 1, 1).tolist() == [0.0]
    assert torch.linspace(-0.04, 0.04, 1).tolist() == [float(np.float32(-0.04))]
    assert linspace_two_sided(0.0, 1.0, 1, np.float32).tolist() == [0.0]
    assert linspace_two_sided(-0.04, 0.04, 1, np.float32).tolist() == [float(np.float32(-0.04))]
    for steps in (2, 3, 5):                                          # the two-sided form is torch's, bit for bit
        for a, b in ((0.0, 1.0), (-0.04, 0.04)):
            assert np.array_equal(linspace_two_sided(a, b, steps, np.float32), torch.linspace(a, b, steps).numpy())
