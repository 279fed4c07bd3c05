"""Parity of the HIP geometry kernels with the oracle."""
import functools

import numpy as np
import pytest
import torch

import geom_ref
import glorie_slam_amd.synth as synth
from oracle import geom as ogeom

pytestmark = pytest.mark.gpu


def _t(x, dev):
    return torch.from_numpy(np.ascontiguousarray(x)).to(dev)


@pytest.fixture(scope="module")
def graph():
    return synth.keyframe_graph(K=6, h=30, w=40, radius=3)


def test_reproject(gpu, graph):
    from glorie_slam_amd import droid_backends as db
    g = graph
    ii = np.concatenate([g["ii"], [2]]).astype(np.int64)   # + one stereo edge (ii == jj)
    jj = np.concatenate([g["jj"], [2]]).astype(np.int64)
    ref_c, ref_v = ogeom.reproject(g["poses"], g["disps"], g["intrinsics"], ii, jj)
    c, v = db.reproject(_t(g["poses"], gpu), _t(g["disps"], gpu), _t(g["intrinsics"], gpu),
                        _t(ii, gpu), _t(jj, gpu))
    # strict fp32 (no contraction) in the reference's operation order: bit-identical to the oracle
    assert np.array_equal(c.cpu().numpy(), ref_c)
    assert np.array_equal(v.cpu().numpy(), ref_v)


def test_frame_distance(gpu, graph):
    from glorie_slam_amd import droid_backends as db
    g = graph
    K = g["K"]
    ii, jj = np.meshgrid(np.arange(K), np.arange(K), indexing="ij")
    ii, jj = ii.reshape(-1).astype(np.int64), jj.reshape(-1).astype(np.int64)
    for beta in (0.3, 0.75):
        ref = ogeom.frame_distance(g["poses"], g["disps"], g["intrinsics"][0], ii, jj, beta)
        got = db.frame_distance(_t(g["poses"], gpu), _t(g["disps"], gpu), _t(g["intrinsics"][0], gpu),
                                _t(ii, gpu), _t(jj, gpu), beta).cpu().numpy()
        # same per-thread accumulation order, same tree, no contraction: the distances graph topology is
        # thresholded on are bit-identical to the oracle
        assert np.array_equal(got, ref), float(np.abs(got - ref).max())


def test_frame_distance_invalid_returns_1000(gpu, graph):
    from glorie_slam_amd import droid_backends as db
    g = graph
    poses = g["poses"].copy()
    poses[1, :3] = (0, 0, -50.0)  # everything lands behind the camera
    ii = np.array([0], np.int64)
    jj = np.array([1], np.int64)
    got = db.frame_distance(_t(poses, gpu), _t(g["disps"], gpu), _t(g["intrinsics"][0], gpu),
                            _t(ii, gpu), _t(jj, gpu), 0.3).cpu().numpy()
    assert got[0] == 1000.0


def test_iproj(gpu, graph):
    from glorie_slam_amd import droid_backends as db
    g = graph
    ref = ogeom.iproj(g["poses"], g["disps"], g["intrinsics"][0])
    got = db.iproj(_t(g["poses"], gpu), _t(g["disps"], gpu), _t(g["intrinsics"][0], gpu)).cpu().numpy()
    np.testing.assert_allclose(got, ref, rtol=1e-5, atol=1e-5)


def test_depth_filter(gpu):
    from glorie_slam_amd import droid_backends as db
    g = synth.keyframe_graph(K=9, h=24, w=32, radius=2)
    ix = np.array([0, 3, 4, 8], np.int64)
    thresh = (0.01 * (1.0 / g["disps"][ix]).mean((1, 2))).astype(np.float32) * 4
    ref = ogeom.depth_filter(g["poses"], g["disps"], g["intrinsics"][0], ix, thresh)
    got = db.depth_filter(_t(g["poses"], gpu), _t(g["disps"], gpu), _t(g["intrinsics"][0], gpu),
                          _t(ix, gpu), _t(thresh, gpu)).cpu().numpy()
    assert ref.max() >= 2 and (ref > 0).mean() > 0.2
    # integer counts: bit-exact (the kernels of geom.hip round every fp32 operation on its own, like the oracle)
    assert np.array_equal(got, ref)


@pytest.mark.parametrize("half", [True, False])
def test_cvx_upsample(gpu, half):
    from glorie_slam_amd import droid_backends as db
    rng = np.random.default_rng(0)
    B, h, w = 5, 12, 18
    disps = rng.uniform(0.2, 1.0, (B, h, w)).astype(np.float32)
    ix = np.array([3, 0, 4], np.int64)
    mask = (rng.standard_normal((3, 576, h, w)) * 2).astype(np.float16 if half else np.float32)
    ref = ogeom.cvx_upsample(disps[ix], mask, np.float16 if half else None)
    up = torch.zeros(B, 8 * h, 8 * w, device=gpu)
    db.cvx_upsample(_t(disps, gpu), _t(ix, gpu), _t(mask, gpu), up, softmax_f32=False)
    got = up.cpu().numpy()
    np.testing.assert_allclose(got[ix], ref, rtol=1e-3 if half else 1e-5, atol=2e-4 if half else 1e-6)
    assert np.all(got[[1, 2]] == 0)
    if half:
        # channels-last logits (layout of the upmask convolution) take the nhwc kernel: same values
        up2 = torch.zeros(B, 8 * h, 8 * w, device=gpu)
        mcl = _t(mask, gpu).contiguous(memory_format=torch.channels_last)
        db.cvx_upsample(_t(disps, gpu), _t(ix, gpu), mcl, up2, softmax_f32=False)
        assert torch.equal(up2, up)


# ---- general rotations, per-frame intrinsics, points behind the camera, ragged maps (tests/geom_ref.py) ---------------------
# The graphs above rotate about y only (qx == qz == 0: half the terms of se3.hiph are multiplied by an exact zero), share one
# intrinsics row and keep every point valid.  geom_ref's scenes do not, and tests/test_geom_ref.py holds the oracle used here
# to a float64 matrix reference on exactly these inputs.
# 1 pixel; one ragged row; odd h*w below one workgroup; exactly one workgroup; one workgroup + 4 pixels; several workgroups
SHAPES = [(1, 1), (1, 7), (7, 9), (16, 16), (13, 20), (30, 40)]


@functools.lru_cache(maxsize=None)
def general(h, w):
    g = geom_ref.general_graph(6, h, w)
    g["ii_s"] = np.concatenate([g["ii"], [1, 4]]).astype(np.int64)     # all ordered pairs + two stereo edges (ii == jj)
    g["jj_s"] = np.concatenate([g["jj"], [1, 4]]).astype(np.int64)
    g["reproject"] = ogeom.reproject(g["poses"], g["disps"], g["intrinsics"], g["ii_s"], g["jj_s"])
    return g


@pytest.mark.parametrize("h,w", SHAPES)
def test_reproject_general_poses(gpu, h, w):
    from glorie_slam_amd import droid_backends as db
    g = general(h, w)
    ref_c, ref_v = g["reproject"]
    if h * w > 1:
        assert set(np.unique(ref_v).tolist()) == {0.0, 1.0}
    c, v = db.reproject(_t(g["poses"], gpu), _t(g["disps"], gpu), _t(g["intrinsics"], gpu),
                        _t(g["ii_s"], gpu), _t(g["jj_s"], gpu))
    assert np.array_equal(c.cpu().numpy(), ref_c)
    assert np.array_equal(v.cpu().numpy(), ref_v)


@pytest.mark.parametrize("h,w", SHAPES)
def test_reproject_motion_general_poses(gpu, h, w):
    """reproject(motion=...) == reproject, then motion_padded: same coordinates, same fp16 map, untouched border"""
    from glorie_slam_amd import droid_backends as db
    from glorie_slam_amd.update_ops import PaddedFlow
    g = general(h, w)
    N = len(g["ii_s"])
    rng = np.random.default_rng(h * 100 + w)
    target = _t((g["reproject"][0] + rng.normal(0, 40, (N, h, w, 2))).astype(np.float32), gpu)
    args = [_t(g[k], gpu) for k in ("poses", "disps", "intrinsics", "ii_s", "jj_s")]
    coords, valid = db.reproject(*args)
    y, x = torch.meshgrid(torch.arange(h, device=gpu, dtype=torch.float32),
                          torch.arange(w, device=gpu, dtype=torch.float32), indexing="ij")
    two = db.motion_padded(coords, torch.stack([x, y], -1).contiguous(), target, PaddedFlow(N, h, w, gpu))
    pf = PaddedFlow(N, h, w, gpu)
    fused_c, fused_v = db.reproject(*args, motion=(target, pf))
    assert torch.equal(fused_c, coords) and torch.equal(fused_v, valid)
    assert torch.equal(pf.buf, two.buf)
    inner = pf.interior()
    assert (inner == 64).any() and (inner == -64).any()           # the clamp is hit on both sides
    border = pf.buf.clone()
    border[:, 3:3 + h, 3:3 + w] = 0
    assert inner.abs().max() > 0 and not border.any()


@pytest.mark.parametrize("beta", [0.3, 0.75])
@pytest.mark.parametrize("h,w", SHAPES)
def test_frame_distance_general_poses(gpu, h, w, beta):
    from glorie_slam_amd import droid_backends as db
    g = general(h, w)
    K = g["K"]
    ii, jj = np.meshgrid(np.arange(K), np.arange(K), indexing="ij")
    ii, jj = ii.reshape(-1).astype(np.int64), jj.reshape(-1).astype(np.int64)
    ref = ogeom.frame_distance(g["poses"], g["disps"], g["intrinsics"][0], ii, jj, beta)
    if (h, w) == (30, 40):
        assert (ref == 1000.0).any() and (ref < 1000.0).any()      # a mix of valid and invalid pixels on both sides of 0.75
    got = db.frame_distance(_t(g["poses"], gpu), _t(g["disps"], gpu), _t(g["intrinsics"][0], gpu),
                            _t(ii, gpu), _t(jj, gpu), beta).cpu().numpy()
    assert np.array_equal(got, ref), float(np.abs(got - ref).max())


@pytest.mark.parametrize("h,w", SHAPES)
def test_iproj_general_poses(gpu, h, w):
    from glorie_slam_amd import droid_backends as db
    g = general(h, w)
    ref = ogeom.iproj(g["poses"], g["disps"], g["intrinsics"][0])
    got = db.iproj(_t(g["poses"], gpu), _t(g["disps"], gpu), _t(g["intrinsics"][0], gpu)).cpu().numpy()
    # no contraction, correctly rounded division, the oracle's operation order: the same bits (test_iproj keeps its tolerance)
    assert np.array_equal(got, ref), float(np.abs(got - ref).max())


@pytest.mark.parametrize("h,w", [(7, 9), (13, 20), (24, 32)])
def test_depth_filter_general_poses(gpu, h, w):
    """multi-view consistent planes seen under general rotations; ix = every frame, so the window ix-3..ix+5 is clipped
    at both ends of the buffer"""
    from glorie_slam_amd import droid_backends as db
    g = geom_ref.plane_graph(9, h, w)
    ix = np.arange(9, dtype=np.int64)
    thresh = (0.01 * (1.0 / g["disps"][ix]).mean((1, 2))).astype(np.float32) * 4
    ref = ogeom.depth_filter(g["poses"], g["disps"], g["intrinsics"][0], ix, thresh)
    if (h, w) == (24, 32):
        assert ref.max() >= 4
    got = db.depth_filter(_t(g["poses"], gpu), _t(g["disps"], gpu), _t(g["intrinsics"][0], gpu),
                          _t(ix, gpu), _t(thresh, gpu)).cpu().numpy()
    assert np.array_equal(got, ref)


# 1 pixel (scalar path, no second pixel); h*w odd (scalar path throughout, pairs that straddle a row end); w odd with h*w even
# (vector path with straddling pairs); h*w = 15 and 63 (ragged last group of 8 of the channels-last kernel); the size above
@pytest.mark.parametrize("half", [True, False])
@pytest.mark.parametrize("h,w", [(1, 1), (7, 9), (10, 13), (3, 5), (12, 18)])
def test_cvx_upsample_ragged_maps(gpu, h, w, half):
    from glorie_slam_amd import droid_backends as db, _lib as L
    rng = np.random.default_rng(h * 100 + w)
    B = 5
    disps = rng.uniform(0.2, 1.0, (B, h, w)).astype(np.float32)
    ix = np.array([3, 0, 4], np.int64)
    mask = (rng.standard_normal((3, 576, h, w)) * 2).astype(np.float16 if half else np.float32)
    ref = ogeom.cvx_upsample(disps[ix], mask, np.float16 if half else None)
    up = torch.zeros(B, 8 * h, 8 * w, device=gpu)
    d_disps, d_ix, d_mask = _t(disps, gpu), _t(ix, gpu), _t(mask, gpu)
    db.cvx_upsample(d_disps, d_ix, d_mask, up, softmax_f32=False)
    got = up.cpu().numpy()
    np.testing.assert_allclose(got[ix], ref, rtol=1e-3 if half else 1e-5, atol=2e-4 if half else 1e-6)
    assert np.all(got[[1, 2]] == 0)
    if not half:
        return
    # channels-last logits: the nhwc kernel, same bits (a 1x1 map is contiguous in both layouts and stays on the planar path)
    up2 = torch.zeros(B, 8 * h, 8 * w, device=gpu)
    db.cvx_upsample(d_disps, d_ix, d_mask.contiguous(memory_format=torch.channels_last), up2, softmax_f32=False)
    assert torch.equal(up2, up)
    if (h, w) == (7, 9):
        # a pixel stride above 576: the logits are the first 576 of 640 channels of a wider channels-last buffer.
        # droid_backends.cvx_upsample always passes 576, so this goes through the library entry it calls.
        wide = torch.full((3, h, w, 640), 30.0, dtype=torch.float16, device=gpu)
        wide[..., :576] = d_mask.permute(0, 2, 3, 1)
        up3 = torch.zeros(B, 8 * h, 8 * w, device=gpu)
        L.check(L.load().glorie_cvx_upsample_nhwc(L.ptr(d_disps), L.ptr(d_ix), L.ptr(wide), 640, L.ptr(up3),
                                                  3, h, w, 0, L.stream_ptr()), "glorie_cvx_upsample_nhwc")
        assert torch.equal(up3, up)
