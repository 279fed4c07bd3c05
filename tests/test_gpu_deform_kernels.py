"""The cloud deformation, the refresh of the unprojected maps and the z-buffer / proxy-depth kernels (csrc/deform.hip;
glorie_proj_depth of csrc/render.hip is the same z-buffer pass) against the float64 restatement of tests/deform_ref.py on
the scenes of tests/deform_scenes.py: general poses, fx != fy, an off-centre principal point, ragged sizes, point
layouts in which no wave holds a single keyframe, out-of-range indices, planted z-buffer cases.
tests/test_deform_scenes.py shows without a GPU that the scenes hold what they are there for.

Scale s_v = sum(prev d) / sum(prev^2).  The kernels sum integers: every term, exact in double, times 2^e and rounded to
int64, e such that the largest term lies in [2^(60-b), 2^(61-b)), b the bit length of the keyframe's count.  The sum that
holds the largest term is then at least 2^(60-b) and off by at most count / 2 < 2^(b-1), a relative 2^(2b-61).  The new
depths of the scenes are 0.7 .. 1.4 times the previous ones, so the other sum is of the same size, and
test_deform_scenes.test_scale_premises holds the quotient of the two exact integer sums to that figure in every keyframe
(with new depths unrelated to the previous ones the smaller sum is off by more, 9e-15 on one trial keyframe).
The quotient is then rounded once to double (2^-53), once to float (u = 2^-24), and s_v * prev once more (u); two
roundings to float compound to less than 2u - u^2 / 2, which leaves room for the double's.  So
    the new depth of a hole point with prev = 1.0f is one of the two float32 neighbours of the exact rational s_v;
    every other hole point: |d - s_v prev| <= (2^-23 + 2^(2b-61)) s_v prev.
A sequential float32 sum is off by 1e-7 to 3e-7 on these keyframes and misses the first of the two.

Positions and z-buffer depths: e_gpu <= FACTOR * e_f32 with FACTOR = 4, the yardstick of tests/test_gpu_tsdf.py: both
errors against float64, e_f32 that of the float32 numpy composition of the same formulas (deform_ref's dtype argument).
Positions are evaluated on the depth the kernel itself stored, so an error of the scale cannot hide in them; their error
is measured per component against |t| + |rd z| of its row, the size its roundings act on.  Pixel coverage of the
z-buffer is exact: the scenes are firm."""
import fractions
import functools
import types

import numpy as np
import pytest
import torch

import deform_scenes as ds
from deform_ref import c2w_of_pose, deform_ref, proj_depth_ref, proxy_depth_ref

pytestmark = pytest.mark.gpu

FACTOR = 4.0
SENTINEL = -7.25                                # fills every output row before a call
EINVAL = -1


def _dev(a, gpu):
    return torch.from_numpy(np.ascontiguousarray(a)).to(gpu)


def _ratio(tag, e_gpu, e_f32):
    print(f"{tag}: error gpu {e_gpu:.3e} / float32 numpy {e_f32:.3e} = {e_gpu / max(e_f32, 1e-300):.3f}")
    assert e_gpu <= FACTOR * e_f32, tag


@functools.lru_cache(maxsize=None)
def _scene(n, layout):
    return ds.deform_scene(n, layout)


# ---- glorie_npc_deform -----------------------------------------------------------------------------------------------
def _state(gpu, c, N_add, fix, extra_rows=0):
    K = c["K"]
    video = types.SimpleNamespace(poses=_dev(c["poses"], gpu), disps_up=_dev(c["disps_up"], gpu),
                                  valid_depth_mask=_dev(c["valid"], gpu), npc_dirty=_dev(c["dirty"], gpu),
                                  intrinsics=torch.tensor([K], device=gpu).repeat(c["B"], 1) / 8.0, down_scale=8)
    video.fresh_disps_up = lambda: video.disps_up
    n = len(c["vidx"])
    prev = np.where(ds.moved(c), c["prev"], np.float32(SENTINEL))    # the depth of a point that stays is never read
    npc = types.SimpleNamespace(_input_video_idx=_dev(c["vidx"], gpu), _input_j=_dev(c["pj"], gpu), _input_i=_dev(c["pi"], gpu),
                                _input_depth=_dev(prev, gpu), _input_pos=torch.full((n, 3), SENTINEL, device=gpu),
                                _cloud_pos=torch.full((n * N_add + extra_rows, 3), SENTINEL, device=gpu),
                                _full_pcl=None, _full_mask=None, N_add=N_add, near_end_surface=ds.NEAR,
                                far_end_surface=ds.FAR, fix_interval_when_add_along_ray=fix)
    npc.pts_num = lambda: npc._cloud_pos.shape[0]
    return video, npc


def _deform(gpu, c, N_add, fix):
    """-> (input_pos [n,3], input_depth [n], cloud [n,N_add,3]) f32 numpy, stats, flags after"""
    from glorie_slam_amd.neural_point import deform_points
    video, npc = _state(gpu, c, N_add, fix)
    stats = torch.zeros(2, dtype=torch.int64, device=gpu)
    assert deform_points(npc, video, *c["K"], stats=stats, rebuild_index=False)
    torch.cuda.synchronize()
    out = [t.cpu().numpy() for t in (npc._input_pos, npc._input_depth, npc._cloud_pos)]
    return out[0], out[1], out[2].reshape(-1, N_add, 3), stats.tolist(), video.npc_dirty.cpu().numpy()


def _check_scale(c, depth, tag):
    live, worst = ds.moved(c), 0.0
    F = fractions.Fraction
    for v in np.nonzero(c["dirty"])[0]:
        prev, d, holes = ds.frame_terms(c, v)
        mine = live & (c["vidx"] == v)
        # a point with a valid depth gets 1.0f / disps_up, correctly rounded
        assert np.array_equal(depth[mine & ~holes], d), (tag, v)
        if len(prev) == 0:                                           # the all-holes keyframe: scale 1, bit for bit
            assert np.array_equal(depth[holes].view(np.int32), c["prev"][holes].view(np.int32)), (tag, v)
            continue
        exact, bits = ds.exact_scale(prev, d), len(prev).bit_length()
        lo, hi = ds.f32_neighbours(exact)
        bound = F(2) ** -23 + F(2) ** (2 * bits - 61)
        for p in np.nonzero(holes)[0]:
            got, was = depth[p], c["prev"][p]
            if was == np.float32(1):
                assert got in (lo, hi), (tag, v, got, lo, hi)
            want = exact * F(float(was))
            r = abs(F(float(got)) - want) / (bound * want)
            worst = max(worst, float(r))
            assert r <= 1, (tag, v, p, float(got), float(want), float(r))
    if live.any():
        print(f"{tag}: hole depths against the exact scale, error / bound {worst:.3f}")


def _check_positions(c, pos, depth, cloud, N_add, fix, tag):
    live = ds.moved(c)
    args = (c["poses"], c["disps_up"], c["valid"], c["dirty"], *ds.ref_indices(c), c["prev"], N_add, ds.NEAR, ds.FAR, fix,
            *c["K"])
    p64, _, c64 = deform_ref(*args, new_depth=depth.astype(np.float64))
    p32, _, c32 = deform_ref(*args, new_depth=depth, dtype=np.float32)
    ro = np.stack([c2w_of_pose(p)[:3, 3] for p in c["poses"]])[c["vidx"][live]]
    c64, c32 = c64.reshape(-1, N_add, 3)[live], c32.reshape(-1, N_add, 3)[live]
    size = lambda x, o: np.abs(o).max(-1, keepdims=True) + np.abs(x - o).max(-1, keepdims=True)
    for name, got, r64, r32, o in (("input_pos", pos[live], p64[live], p32[live], ro),
                                   ("cloud_pos", cloud[live], c64, c32, ro[:, None, :])):
        s = size(r64, o)
        e_gpu, e_f32 = float((np.abs(got - r64) / s).max()), float((np.abs(r32 - r64) / s).max())
        _ratio(f"{tag} {name}", e_gpu, e_f32)


def _check_deform(gpu, n, layout, N_add, fix):
    c = _scene(n, layout)
    tag = f"deform n {n} {layout} N_add {N_add} fix {int(fix)}"
    pos, depth, cloud, stats, flags = _deform(gpu, c, N_add, fix)
    live = ds.moved(c)
    # untouched rows: clean keyframes and out-of-range indices
    for name, x in (("input_pos", pos), ("input_depth", depth), ("cloud_pos", cloud)):
        assert (x[~live] == np.float32(SENTINEL)).all(), f"{tag}: {name} of a point that stays was written"
    assert np.isfinite(pos[live]).all() and np.isfinite(cloud[live]).all() and (depth[live] > 0).all(), tag
    assert stats == [int(c["dirty"].sum()), int(live.sum())], (tag, stats)
    assert not flags.any()
    _check_scale(c, depth, tag)
    _check_positions(c, pos, depth, cloud, N_add, fix, tag)
    return c, pos, depth, cloud


@pytest.mark.parametrize("fix", [False, True])
@pytest.mark.parametrize("N_add", [1, 2, 3, 5])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 257, 1000])
def test_deform_matches_the_restatement(gpu, n, N_add, fix):
    """less than a wave, a wave less one, one wave, one more, and the scenes with the planted keyframes, in all three
    layouts"""
    for layout in ds.LAYOUTS:
        _check_deform(gpu, n, layout, N_add, fix)


def test_deform_does_not_depend_on_the_layout(gpu):
    """the same points in three orders: every point's outputs are bitwise equal, and so are two runs"""
    outs = {}
    for layout in ds.LAYOUTS:
        c = _scene(1000, layout)
        pos, depth, cloud, *_ = _deform(gpu, c, 3, False)
        back = np.argsort(c["ids"])
        outs[layout] = [x[back].view(np.int32) for x in (pos, depth, cloud)]
    for layout in ds.LAYOUTS[1:]:
        for a, b in zip(outs["runs"], outs[layout]):
            assert np.array_equal(a, b), layout
    c = _scene(1000, "interleaved")
    again = _deform(gpu, c, 3, False)
    back = np.argsort(c["ids"])
    for a, b in zip(outs["interleaved"], again[:3]):
        assert np.array_equal(a, b[back].view(np.int32))


def test_deform_arguments(gpu):
    from glorie_slam_amd import _lib as L
    from glorie_slam_amd.neural_point import deform_points
    c = _scene(65, "runs")
    video, npc = _state(gpu, c, 3, False, extra_rows=1)             # cloud_rows != n * N_add
    with pytest.raises(L.GlorieError, match="GLORIE_EINVAL"):
        deform_points(npc, video, *c["K"], rebuild_index=False)
    torch.cuda.synchronize()
    assert bool((npc._cloud_pos == SENTINEL).all()) and bool(video.npc_dirty.any())
    # no input points, no keyframes: the entry point returns before it reads a pointer
    lib, null = L.load(), None
    tail = (3, 0.95, 1.05, 0, *[float(k) for k in c["K"]], null, null, L.stream_ptr())
    assert lib.glorie_npc_deform(null, null, null, null, 7, 23, 37, null, null, null, null, null, 0, null, 0, *tail) == 0
    assert lib.glorie_npc_deform(null, null, null, null, 0, 23, 37, null, null, null, null, null, 5, null, 15, *tail) == 0
    assert lib.glorie_npc_deform(null, null, null, null, 7, 23, 37, null, null, null, null, null, 5, null, 14, *tail) == EINVAL
    assert lib.glorie_npc_deform_workspace(0) == 0 and lib.glorie_npc_deform_workspace(7) == 7 * 24


# ---- glorie_iproj_dirty ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W", [(23, 37), (5, 7)])
def test_iproj_dirty_refreshes_the_dirty_maps_only(gpu, H, W):
    from glorie_slam_amd import droid_backends
    from glorie_slam_amd.neural_point import iproj_dirty, se3_inv
    rng = np.random.default_rng(H)
    B, K = 5, ds.ZK[(H, W)]
    dirty = np.array([True, False, True, True, False])
    video = types.SimpleNamespace(poses=_dev(np.stack([ds.general_pose(rng) for _ in range(B)]), gpu),
                                  disps_up=_dev((1.0 / rng.uniform(0.5, 5.0, (B, H, W))).astype(np.float32), gpu),
                                  valid_depth_mask=_dev(rng.uniform(size=(B, H, W)) > 0.4, gpu),
                                  intrinsics=torch.tensor([K], device=gpu).repeat(B, 1) / 8.0, down_scale=8)
    video.fresh_disps_up = lambda: video.disps_up
    want = droid_backends.iproj(se3_inv(video.poses), video.disps_up, (video.intrinsics[0] * 8.0).contiguous())
    d = _dev(dirty, gpu)
    for clear in (0, 1):
        video.npc_dirty = d.clone()
        npc = types.SimpleNamespace(_full_pcl=torch.full((B, H, W, 3), SENTINEL, device=gpu),
                                    _full_mask=torch.full((B, H, W), 0x5A, dtype=torch.uint8, device=gpu).view(torch.bool))
        iproj_dirty(npc, video, clear_flags=bool(clear))
        torch.cuda.synchronize()
        assert torch.equal(npc._full_pcl[d], want[d]) and bool((npc._full_pcl[~d] == SENTINEL).all())
        mask = npc._full_mask.view(torch.uint8)
        assert torch.equal(mask[d], video.valid_depth_mask.view(torch.uint8)[d]) and bool((mask[~d] == 0x5A).all())
        assert torch.equal(video.npc_dirty, torch.zeros_like(d) if clear else d)
    assert bool(torch.isfinite(want).all()) and float(want.abs().max()) > 1.0


# ---- the z-buffer pass -----------------------------------------------------------------------------------------------
def _zbuf_inputs(gpu, c, mask="scene"):
    bits = {"scene": c["full_mask"], "full": np.ones_like(c["full_mask"]), None: None}[mask]
    return (_dev(c["full_pcl"], gpu), None if bits is None else _dev(bits, gpu).view(torch.uint8), _dev(c["w2c"], gpu),
            [float(k) for k in c["K"]])


def _proj_depth(gpu, c, mask="scene"):
    """glorie_proj_depth over the first `counter` maps -> the depth bits [H,W] int32 (+inf where nothing projects)"""
    from glorie_slam_amd import _lib as L
    pts, bits, w2c, K = _zbuf_inputs(gpu, c, mask)
    out = torch.full((c["H"], c["W"]), float("inf"), device=gpu)
    L.check(L.load().glorie_proj_depth(L.ptr(pts), L.ptr(bits), c["counter"] * c["H"] * c["W"], L.ptr(w2c), *K, c["H"],
                                       c["W"], L.ptr(out), L.stream_ptr()), "glorie_proj_depth")
    torch.cuda.synchronize()
    return out.view(torch.int32).cpu().numpy()


def _proxy_depth(gpu, c, skip_row=-1, droid=None, mono=None, counter=None):
    """glorie_proxy_depth -> (status, out [H,W] f32, z-buffer bits [H,W] int32)"""
    from glorie_slam_amd import _lib as L
    pts, bits, w2c, K = _zbuf_inputs(gpu, c)
    H, W = c["H"], c["W"]
    droid = torch.zeros(H, W, device=gpu) if droid is None else _dev(np.asarray(droid, np.float32), gpu)
    mono = None if mono is None else _dev(np.asarray(mono, np.float32), gpu)
    zbuf, out = torch.full((H, W), SENTINEL, device=gpu), torch.full((H, W), SENTINEL, device=gpu)
    status = L.load().glorie_proxy_depth(L.ptr(pts), L.ptr(bits), c["counter"] if counter is None else counter, H, W,
                                         skip_row, L.ptr(w2c), *K, L.ptr(droid), L.ptr(mono), L.ptr(zbuf), L.ptr(out),
                                         L.stream_ptr())
    torch.cuda.synchronize()
    return status, out.cpu().numpy(), zbuf.view(torch.int32).cpu().numpy()


def _restated(c, row, dtype=np.float64, **kw):
    with np.errstate(invalid="ignore", over="ignore"):
        return proj_depth_ref(c["full_pcl"], c["full_mask"], c["counter"], 0, None, *c["K"], dtype=dtype,
                              **{"w2c": c["w2c"], "row": row, **kw})


def _check_depth(tag, got, ref, f32):
    assert np.array_equal(got > 0, ref > 0), f"{tag}: pixel coverage differs in {int(((got > 0) != (ref > 0)).sum())} pixels"
    assert np.array_equal(f32 > 0, ref > 0)
    hit = ref > 0
    if not hit.any():
        assert not got.any()
        return
    _ratio(tag, float(np.abs(got[hit] / ref[hit] - 1).max()), float(np.abs(f32[hit] / ref[hit] - 1).max()))


@pytest.mark.parametrize("H,W,counter", ds.ZBUF_SCENES)
def test_zbuf_matches_the_restatement(gpu, H, W, counter):
    c = ds.zbuf_scene(H, W, counter)
    assert (counter * H * W) % 256 != 0 or counter == 0
    for row in (-1, 0, H - 1, c["mid_row"]):
        status, got, bits = _proxy_depth(gpu, c, row)
        assert status == 0
        _check_depth(f"zbuf {H} x {W} x {counter} skip_row {row}", got, _restated(c, row), _restated(c, row, np.float32))
        # the z-buffer keeps +inf where nothing projects, the result has 0 there
        inf = bits == 0x7f800000
        assert np.array_equal(inf, got == 0) and np.array_equal(bits[~inf], got[~inf].view(np.int32))
        if row == -1:
            whole, whole_bits = got, bits
    # the same mask through glorie_proj_depth: the same bits; no mask is a full mask
    assert np.array_equal(_proj_depth(gpu, c, "scene"), whole_bits)
    assert np.array_equal(_proj_depth(gpu, c, None), _proj_depth(gpu, c, "full"))
    if not counter:
        return
    # the planted cases, by name
    P, ref = c["planted"], _restated(c, -1)
    near = lambda pixel, depth: abs(whole[pixel] - depth) < 1e-5
    assert near(P["pair_nf"]["pixel"], 0.6) and near(P["pair_fn"]["pixel"], 0.6), "two points in one pixel: the nearer wins"
    assert near(P["dup"]["pixel"], 0.8)
    assert near(P["masked"]["pixel"], 0.7), "a nearer point with a cleared bit must not win"
    assert near(P["row_first"]["pixel"], 0.5) and near(P["row_last"]["pixel"], 0.5)
    for name in ("inf", "nan", "behind", "u_neg", "v_neg"):         # these write nothing: their pixel shows what lies
        pixel = P[name]["pixel"]                                    # behind, an ordinary point (more than 1 away) or none
        assert ref[pixel] == 0 or ref[pixel] > 1.0
        assert whole[pixel] == 0 or whole[pixel] > 1.0, f"{name} wrote {whole[pixel]}"


def test_zbuf_points_on_the_zero_border_are_inside(gpu):
    """u == -0.0 and v == -0.0 exactly: `>= 0` holds, the points land in column 0 and row 0"""
    c = ds.border_scene()
    status, got, _ = _proxy_depth(gpu, c)
    assert status == 0
    _check_depth("zbuf zero border", got, _restated(c, -1), _restated(c, -1, np.float32))
    for name in ("u_zero", "v_zero"):
        assert abs(got[c["planted"][name]["pixel"]] - 2.0) < 1e-5, name
    assert (got == 0).sum() == 2


def test_proxy_depth_arguments(gpu):
    c = ds.zbuf_scene(5, 7, 1)
    for kw in (dict(skip_row=5), dict(skip_row=-2), dict(counter=-1)):
        status, out, _ = _proxy_depth(gpu, c, **kw)
        assert status == EINVAL and (out == np.float32(SENTINEL)).all(), kw
    assert _proxy_depth(gpu, c, skip_row=4)[0] == 0


def test_proxy_finalize_truth_table(gpu):
    """tracker depth {> 0, 0, < 0, NaN} x projection {hit, none} x mono prior {given, null}"""
    H, W, K = 2, 4, (4.0, 4.0, 2.0, 1.0)
    jj, ii = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    pcl = (ds.pixel_dirs(ii + 0.5, jj * 0 + 0.5, K) * 2.0).astype(np.float32)[None]       # every point aims at row 0
    mask = np.zeros((1, H, W), bool)
    mask[0, 0] = True                                                # ... and only map row 0 is read: view row 1 is empty
    c = dict(full_pcl=pcl, full_mask=mask, counter=1, H=H, W=W, K=K, w2c=np.eye(4, dtype=np.float32))
    nan = np.float32("nan")
    droid = np.array([[1.5, 0.0, -2.0, nan]] * 2, np.float32)
    mono = np.arange(7, 15, dtype=np.float32).reshape(H, W)
    p = -(np.float32(-2.0) + np.float32(1e-6))                       # the projected depth, -(c + eps) in float32
    proj = _proj_depth(gpu, c).view(np.float32)
    assert np.array_equal(proj, np.array([[p] * 4, [np.inf] * 4], np.float32))
    proj = np.where(np.isinf(proj), 0, proj)
    want = {True: np.array([[1.5, p, p, p], [1.5, 12.0, -2.0, nan]], np.float32),
            False: np.array([[1.5, p, p, p], [1.5, 0.0, -2.0, nan]], np.float32)}
    for given in (True, False):
        status, got, _ = _proxy_depth(gpu, c, droid=droid, mono=mono if given else None)
        assert status == 0 and np.array_equal(got, want[given], equal_nan=True), (given, got)
        ref = proxy_depth_ref(proj, droid, mono, use_mono_to_complete=given)
        assert np.array_equal(got, ref.astype(np.float32), equal_nan=True)


def test_proxy_render_depth_wrapper(gpu):
    """neural_point.proxy_render_depth on a general view: the inverse of c2w is taken in float32 on the device, so the
    float32 yardstick inverts in float32 too; counter is clamped to the maps there are; no maps: tracker, then mono"""
    from glorie_slam_amd.neural_point import proxy_render_depth
    c = ds.zbuf_scene(23, 37, 3)
    H, W, K = c["H"], c["W"], c["K"]
    rng = np.random.default_rng(5)
    droid = np.where(rng.uniform(size=(H, W)) < 0.4, rng.uniform(0.5, 3.0, (H, W)), 0.0).astype(np.float32)
    mono = rng.uniform(4.0, 5.0, (H, W)).astype(np.float32)
    npc = types.SimpleNamespace(_full_pcl=_dev(c["full_pcl"], gpu), _full_mask=_dev(c["full_mask"], gpu))
    for value, mws, maps, row in ((3, 3 - c["mid_row"], 3, c["mid_row"]), (99, 99 - H, 4, -1)):   # 99: clamped to 4 maps
        video = types.SimpleNamespace(counter=types.SimpleNamespace(value=value))
        with np.errstate(invalid="ignore", over="ignore"):
            p64, p32 = (proj_depth_ref(c["full_pcl"], c["full_mask"], maps, 0, c["c2w"], *K, dtype=t, row=row)
                        for t in (np.float64, np.float32))
        if maps == 3:                                                # all three sources of the result occur
            assert (p64 > 0).sum() > H * W // 2 and ((p64 == 0) & (droid == 0)).sum() > 5
        for use_mono in (True, False):
            got = proxy_render_depth(npc, video, _dev(c["c2w"], gpu), _dev(droid, gpu), _dev(mono, gpu), mws, *K,
                                     use_mono_to_complete=use_mono).cpu().numpy()
            want = proxy_depth_ref(p64, droid, mono, use_mono)
            from_proj = (droid == 0) & (p64 > 0)
            assert np.array_equal(got[~from_proj], want[~from_proj].astype(np.float32))
            f32 = proxy_depth_ref(p32, droid, mono, use_mono)
            _check_depth(f"proxy_render_depth counter {value} mono {int(use_mono)}", np.where(from_proj, got, 0),
                         np.where(from_proj, want, 0), np.where(from_proj, f32, 0))
        if maps == 4:                                                # the map behind the three was read
            assert ((got > 0.19) & (got < 0.21)).sum() > H * W // 4
    video = types.SimpleNamespace(counter=types.SimpleNamespace(value=3))
    bare = types.SimpleNamespace(_full_pcl=None, _full_mask=None)
    got = proxy_render_depth(bare, video, _dev(c["c2w"], gpu), _dev(droid, gpu), _dev(mono, gpu), 1, *K).cpu().numpy()
    assert np.array_equal(got, np.where(droid > 0, droid, mono))
