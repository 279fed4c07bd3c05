"""glorie_ray_samples_near (the on-device probe march of the rays without a depth prior) against the float64
restatement of tests/near_pcl_ref.py on firm rays, against ray_samples on the rays that do have depth, and against the
KNN kernel's own neighbour counts."""
import numpy as np
import pytest
import torch

import near_pcl_ref as ref

pytestmark = pytest.mark.gpu
S0 = 10
_STATE = {}


def _npc(gpu):
    """the scene's cloud in a NeuralPointCloud (cell list built once) and its rays on the device"""
    if "npc" not in _STATE:
        from glorie_slam_amd.neural_point import NeuralPointCloud
        sc = ref.scene()
        cfg = {"device": str(gpu), "model": {"c_dim": 32},
               "pointcloud": {"nn_weighting": "distance", "use_dynamic_radius": True, "min_nn_num": 2, "nn_num": 8,
                              "radius_query": ref.RADIUS, "radius_add": 0.04, "radius_min": 0.02}}
        t = lambda x: torch.from_numpy(x).to(gpu)
        npc = NeuralPointCloud(cfg)
        npc.add_points(t(sc["cloud"]), t(sc["geo"]), t(sc["col"]))
        _STATE.update(npc=npc, o=t(sc["rays_o"]), d=t(sc["rays_d"]), depth=t(sc["depth"]), radius=t(sc["radius"]))
    return _STATE["npc"], _STATE


def _march(gpu, far, n, S=S0, depth=None, radius=True, index=None, o=None, d=None):
    from glorie_slam_amd import point_ops
    npc, st = _npc(gpu)
    o, d = (st["o"], st["d"]) if o is None else (o, d)
    rad = st["radius"][:o.shape[0]] if radius else None
    return point_ops.ray_samples_near(npc.index if index is None else index, ref.RADIUS, o, d, depth, rad, S, 0.95, 1.05, ref.NEAR, far, n)


def _bits(x):
    return x.detach().cpu().numpy().view(np.uint32)


def _check_against_ref(out, m, S):
    z, pts, views, rs, near_mask, bracket = out
    firm = m["firm"]
    assert (~firm).mean() <= ref.MAX_NON_FIRM_SHARE
    assert near_mask.dtype == torch.bool and bracket.dtype == torch.int32 and z.shape == (firm.shape[0], S)
    assert np.array_equal(bracket.cpu().numpy()[firm], m["bracket"][firm])
    assert np.array_equal(near_mask.cpu().numpy()[firm], m["near_mask"][firm])
    assert np.array_equal(_bits(z)[firm], m["z"][firm].view(np.uint32))


def test_chunk_width_is_what_the_cases_were_chosen_for(gpu):
    from glorie_slam_amd import point_ops
    assert point_ops.near_pcl_chunk() == 64


@pytest.mark.parametrize("far,n", ref.CASES)
def test_march_equals_restatement_on_firm_rays(gpu, far, n):
    """every ray marched (depth null): bracket, near_mask and the z-values bit for bit; pts = o + dir * z from torch ops on
    the kernel's z, views and per-sample radius repeated"""
    _, st = _npc(gpu)
    out = _march(gpu, far, n)
    _check_against_ref(out, ref.scene_march(far, n, S0), S0)
    z, pts, views, rs, near_mask, bracket = out
    assert torch.equal(pts, (st["o"][:, None, :] + st["d"][:, None, :] * z[:, :, None]).reshape(-1, 3))
    assert torch.equal(views, st["d"].repeat_interleave(S0, dim=0)) and torch.equal(rs, st["radius"].repeat_interleave(S0))
    # the far end as a one-element device tensor (no host read) gives the same bits
    out_t = _march(gpu, torch.tensor([far], dtype=torch.float32, device=gpu), n)
    for a, b in zip(out, out_t):
        assert torch.equal(a, b)


@pytest.mark.parametrize("S", [1, 10, 32])
def test_sample_counts(gpu, S):
    out = _march(gpu, 6.0, 25, S=S)
    _check_against_ref(out, ref.scene_march(6.0, 25, S), S)
    out = _march(gpu, 5.0, 160, S=S, radius=False)
    _check_against_ref(out, ref.scene_march(5.0, 160, S), S)
    assert out[3] is None


def test_more_than_32_samples_is_unsupported(gpu):
    from glorie_slam_amd import _lib
    with pytest.raises(_lib.GlorieError):
        _march(gpu, 6.0, 25, S=33)


def test_mixed_batch_and_camera_variant(gpu):
    """every fifth depth zeroed: the rays with depth are bitwise those of ray_samples (near_mask 1, bracket -1), the others
    those of the all-marched call; the camera variant forms the same rays itself and agrees bitwise"""
    import glorie_slam_amd.synth as synth
    from glorie_slam_amd import point_ops
    npc, st = _npc(gpu)
    t = lambda x: torch.from_numpy(x).to(gpu)
    ro, rd, depth, radius, c2w = synth.box_rays(24, 32, fx=16.0, fy=16.0, cx=15.5, cy=11.5)
    R = ref.N_RAYS
    o, d, rad = t(ro[:R]), t(rd[:R]), t(radius[:R])                     # the view's own rays (none turned away)
    g = t(depth[:R]).clone()
    g[::5] = 0.0
    has = (g > 0)
    far = torch.minimum(5 * g.mean(), torch.max(g * 1.2)).reshape(1)
    mixed = point_ops.ray_samples_near(npc.index, ref.RADIUS, o, d, g, rad, S0, 0.95, 1.05, ref.NEAR, far, 25)
    plain = point_ops.ray_samples(o, d, g, rad, S0, 0.95, 1.05)
    allm = point_ops.ray_samples_near(npc.index, ref.RADIUS, o, d, None, rad, S0, 0.95, 1.05, ref.NEAR, far, 25)
    assert int(plain[4]) == int((~has).sum()) == (R + 4) // 5
    hs = has.repeat_interleave(S0)
    assert torch.equal(mixed[0][has], plain[0][has])
    for k in (1, 2, 3):
        assert torch.equal(mixed[k][hs], plain[k][hs])
        assert torch.equal(mixed[k][~hs], allm[k][~hs])
    assert torch.equal(mixed[0][~has], allm[0][~has])
    assert bool(mixed[4][has].all()) and bool((mixed[5][has] == -1).all())
    assert torch.equal(mixed[4][~has], allm[4][~has]) and torch.equal(mixed[5][~has], allm[5][~has])
    assert int(mixed[4][~has].sum()) > 100                              # the marched rays do find their brackets
    # restatement on the marched rays
    m = ref.march(ref.scene()["cloud"], ro[:R], rd[:R], ref.NEAR, float(far.cpu()[0]), 25, S0)
    sel = (~has).cpu().numpy() & m["firm"]
    assert (~m["firm"]).mean() <= ref.MAX_NON_FIRM_SHARE
    assert np.array_equal(mixed[5].cpu().numpy()[sel], m["bracket"][sel])
    assert np.array_equal(_bits(mixed[0])[sel], m["z"][sel].view(np.uint32))
    cam = point_ops.camera_block(c2w, 16.0, 16.0, 15.5, 11.5, gpu)
    for first, n_r, gg, rr in ((0, R, g, rad), (37, R - 37, g[37:], rad[37:]), (37, R - 37, None, None)):
        a = point_ops.ray_samples_near_camera(npc.index, ref.RADIUS, cam, 32, first, n_r, gg, rr, S0, 0.95, 1.05, ref.NEAR,
                                              far, 25)
        b = point_ops.ray_samples_near(npc.index, ref.RADIUS, o[first:], d[first:], gg, rr, S0, 0.95, 1.05, ref.NEAR, far, 25)
        for x, y in zip(a, b):
            assert (x is None and y is None) or torch.equal(x, y)


def test_no_rays(gpu):
    _, st = _npc(gpu)
    out = _march(gpu, 6.0, 25, o=st["o"][:0], d=st["d"][:0])
    assert out[0].shape == (0, S0) and out[1].shape == (0, 3) and out[4].shape == (0,) and out[5].shape == (0, 2)


def test_empty_cloud(gpu):
    from glorie_slam_amd.point_ops import KnnIndex
    idx = KnnIndex(gpu, cell_size=0.06, max_cells=1 << 12)
    idx.reset()
    z, pts, views, rs, near_mask, bracket = _march(gpu, 6.0, 25, index=idx)
    assert not bool(near_mask.any()) and bool((bracket == -1).all())
    want = torch.from_numpy(np.linspace(ref.NEAR, 6.0, S0).astype(np.float32)).to(gpu)
    assert torch.equal(z, want[None, :].expand_as(z))


def test_far_before_near(gpu):
    """far < near (and a NaN far): the call returns, every ray is invalid, the samples span [near, far]"""
    z, pts, views, rs, near_mask, bracket = _march(gpu, 0.1, 25)
    torch.cuda.synchronize()
    assert not bool(near_mask.any()) and bool((bracket[:, 1] == -1).all())
    want = torch.from_numpy(np.linspace(ref.NEAR, float(np.float32(0.1)), S0).astype(np.float32)).to(gpu)
    assert torch.equal(z, want[None, :].expand_as(z))
    z, pts, views, rs, near_mask, bracket = _march(gpu, float("nan"), 300)
    torch.cuda.synchronize()
    assert not bool(near_mask.any()) and bool((bracket == -1).all()) and bool(torch.isnan(z[:, 1:]).all())


@pytest.mark.parametrize("far,n", [(6.0, 25), (5.0, 160)])
def test_occupancy_equals_knn_counts(gpu, far, n):
    """the probes rebuilt from the documented formula and searched by find_neighbors_faiss(step='query'): `count > 0` of
    the first probes of every ray, up to its second occupied one, is exactly the kernel's bracket - same bits, same
    predicate, no firmness needed"""
    npc, st = _npc(gpu)
    z, pts, views, rs, near_mask, bracket = _march(gpu, far, n)
    z32 = torch.from_numpy(ref.probe_depths(ref.NEAR, far, n)[1]).to(gpu)
    probes = (st["o"][:, None, :] + st["d"][:, None, :] * z32[None, :, None]).reshape(-1, 3)
    nn = npc.find_neighbors_faiss(probes, step='query')[2].reshape(-1, n)
    occ = (nn > 0).cpu().numpy()
    want = np.full((occ.shape[0], 2), -1, np.int32)
    for r in range(occ.shape[0]):
        idx = np.flatnonzero(occ[r])[:2]
        want[r, :idx.size] = idx
    assert np.array_equal(bracket.cpu().numpy(), want)
    assert np.array_equal(near_mask.cpu().numpy(), want[:, 1] >= 0)
