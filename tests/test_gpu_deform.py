"""The cloud deformation and the proxy depth on HIP (glorie_slam_amd/neural_point.py deform_points / iproj_dirty /
proxy_render_depth, csrc/deform.hip) and SequenceRunner's bind_npc_with_pose / render_depth keys (reference:
src/neural_point.py:378-575, src/mapper.py:246-279, :557-573, :705-730).

  * against the reference's values (tests/golden/deform.npz) and the float64 restatement (tests/deform_ref.py);
  * against the torch update_points_pos(npc, video) on a 64-keyframe video with ~300k input points;
  * bitwise repeatable, recorded into a hipGraph and replayed on new poses and flags, edge cases, a rigid motion;
  * the runner: points follow a moved trajectory, the training depth is the proxy depth, the < 100-pixel skip, eager
    and recorded losses, the keys absent, a loop-closing sequence."""
import types

import numpy as np
import pytest
import torch

from deform_ref import c2w_and_depth_ref, deform_ref, proj_depth_ref, proxy_depth_ref
from test_deform_oracle import deform_case, load

pytestmark = pytest.mark.gpu


def _t(x, dev):
    return (x if torch.is_tensor(x) else torch.from_numpy(np.ascontiguousarray(x))).to(dev)


def _quat(R):
    w = np.sqrt(max(1 + R[0, 0] + R[1, 1] + R[2, 2], 1e-12)) / 2
    return np.array([(R[2, 1] - R[1, 2]) / (4 * w), (R[0, 2] - R[2, 0]) / (4 * w), (R[1, 0] - R[0, 1]) / (4 * w), w])


def _video(gpu, B, H, W, fx, fy, cx, cy, N_add=3, fix=False):
    from glorie_slam_amd.depth_video import DepthVideo
    from glorie_slam_amd.pipeline import synthetic_cfg
    cfg = synthetic_cfg(gpu, B, H, W)
    cfg["cam"].update(H=H, W=W, fx=fx, fy=fy, cx=cx, cy=cy)
    cfg["mapping"]["render_depth"] = "proxy"
    cfg["pointcloud"].update(N_add=N_add, fix_interval_when_add_along_ray=fix, near_end_surface=0.95,
                             far_end_surface=1.05)
    video = DepthVideo(cfg)
    video.intrinsics[:] = torch.tensor([fx, fy, cx, cy], device=gpu) / 8.0
    return cfg, video


def _npc(cfg, video, vidx, pj, pi, prev, cloud=None):
    from glorie_slam_amd.neural_point import NeuralPointCloud
    dev = video.poses.device
    npc = NeuralPointCloud(cfg, video)
    n = len(vidx)
    npc._input_video_idx, npc._input_j, npc._input_i = (_t(x, dev).long() for x in (vidx, pj, pi))
    npc._input_depth = _t(prev, dev).float().contiguous()
    npc._input_pos = torch.zeros(n, 3, device=dev)
    npc._cloud_pos = torch.zeros(n * npc.N_add, 3, device=dev) if cloud is None else cloud.clone()
    npc._pts_num = npc._cloud_pos.shape[0]
    npc.index.set_points(npc._cloud_pos)
    return npc


def _state(npc, video):
    s = {k: getattr(npc, k).clone() for k in ("_input_pos", "_input_depth", "_cloud_pos")}
    if npc._full_pcl is not None:
        s.update(_full_pcl=npc._full_pcl.clone(), _full_mask=npc._full_mask.clone())
    s.update(flags=video.npc_dirty.clone(), poses=video.poses.clone())
    return s


def _restore(npc, video, s):
    for k in ("_input_pos", "_input_depth", "_cloud_pos", "_full_pcl", "_full_mask"):
        if k in s:
            getattr(npc, k).copy_(s[k])
    video.npc_dirty.copy_(s["flags"])
    video.poses.copy_(s["poses"])


def _fixture_state(gpu, c, N_add, fix):
    B = c["poses"].shape[0]
    cfg, video = _video(gpu, B, c["H"], c["W"], c["fx"], c["fy"], c["cx"], c["cy"], N_add, fix)
    video.poses[:] = _t(c["poses"], gpu)
    video.disps_up[:] = _t(c["disps_up"], gpu)
    video.valid_depth_mask[:] = _t(c["valid"], gpu)
    video.npc_dirty[:] = _t(c["dirty"], gpu)
    video.counter.value = 6
    npc = _npc(cfg, video, c["input_video_idx"], c["input_j"], c["input_i"], c["input_depth"])
    return video, npc


@pytest.mark.parametrize("name", ["n3", "n5", "fix"])
def test_deform_matches_the_reference(gpu, name):
    from glorie_slam_amd.neural_point import deform_points
    c = load()
    N_add, fix = (int(x) for x in c[f"deform_{name}_args"])
    video, npc = _fixture_state(gpu, c, N_add, bool(fix))
    before = _state(npc, video)
    assert deform_points(npc, video, c["fx"], c["fy"], c["cx"], c["cy"])
    vidx = c["input_video_idx"]
    dirty, holes = c["dirty"][vidx], vidx == 5
    keep = dirty & ~holes
    pos, depth, cloud = (x.cpu().numpy() for x in (npc._input_pos, npc._input_depth, npc._cloud_pos))
    np.testing.assert_allclose(pos[keep], c[f"deform_{name}_pos"][keep], rtol=1e-5, atol=1e-5)
    np.testing.assert_allclose(depth[keep], c[f"deform_{name}_depth"][keep], rtol=1e-5)
    rows = np.repeat(keep, N_add)
    np.testing.assert_allclose(cloud[rows], c[f"deform_{name}_cloud"][rows], rtol=1e-5, atol=1e-5)
    # clean keyframes: every byte unchanged
    assert np.array_equal(pos[~dirty], before["_input_pos"].cpu().numpy()[~dirty])
    assert np.array_equal(cloud[~np.repeat(dirty, N_add)], before["_cloud_pos"].cpu().numpy()[~np.repeat(dirty, N_add)])
    # the keyframe whose points all lie on holes: scale 1 (documented deviation from the reference's NaN)
    rp, rd, rc = deform_case(c, name)
    assert np.isfinite(pos[holes]).all() and np.array_equal(depth[holes], c["input_depth"][holes])
    np.testing.assert_allclose(pos[holes], rp[holes], rtol=1e-5, atol=1e-5)
    np.testing.assert_allclose(cloud[np.repeat(holes, N_add)], rc[np.repeat(holes, N_add)], rtol=1e-5, atol=1e-5)
    # flags cleared; the unprojected maps of the dirty keyframes are add_points(idx)'s
    assert not bool(video.npc_dirty.any())
    from glorie_slam_amd.neural_point import NeuralPointCloud
    ref = NeuralPointCloud(npc.cfg, video)
    idx = torch.tensor(np.nonzero(c["dirty"])[0], device=gpu)
    ref.add_points(idx)
    assert torch.equal(ref.full_pcl(), npc.full_pcl()) and torch.equal(ref.full_mask(), npc.full_mask())


def _big(gpu, B=64, H=120, W=160, n_pts=300_000, N_add=3, seed=0, runs=4):
    """a video of B keyframes with random poses / depths / valid masks and n_pts input points in runs interleaved over
    the keyframes"""
    rng = np.random.default_rng(seed)
    fx, fy, cx, cy = 100.0, 100.0, W / 2 - 0.5, H / 2 - 0.5
    cfg, video = _video(gpu, B, H, W, fx, fy, cx, cy, N_add)
    poses = np.zeros((B, 7), np.float32)
    for b in range(B):
        q = np.concatenate([rng.normal(0, 0.1, 3), [1.0]])
        poses[b, 3:] = q / np.linalg.norm(q)
        poses[b, :3] = rng.normal(0, 0.3, 3)
    disps = (1.0 / rng.uniform(1.0, 4.0, (B, H, W))).astype(np.float32)
    valid = rng.uniform(0, 1, (B, H, W)) > 0.15
    video.poses[:] = _t(poses, gpu)
    video.disps_up[:] = _t(disps, gpu)
    video.valid_depth_mask[:] = _t(valid, gpu)
    video.counter.value = B
    per = n_pts // (B * runs)
    vidx = np.concatenate([np.full(per + int(rng.integers(-20, 20)), k) for r in range(runs) for k in rng.permutation(B)])
    pj, pi = rng.integers(0, H, len(vidx)), rng.integers(0, W, len(vidx))
    prev = (1.0 / disps[vidx, pj, pi] * rng.uniform(0.9, 1.1, len(vidx))).astype(np.float32)
    npc = _npc(cfg, video, vidx, pj, pi, prev, cloud=torch.randn(len(vidx) * N_add, 3, device=gpu))
    return video, npc, (fx, fy, cx, cy), vidx


@pytest.mark.parametrize("n_dirty", [25, 64])
def test_deform_matches_torch_update_points_pos(gpu, n_dirty):
    from glorie_slam_amd import neural_point as NP
    from glorie_slam_amd.point_ops import KnnIndex
    video, npc, cam, vidx = _big(gpu)
    assert npc._input_pos.shape[0] > 290_000
    flags = torch.zeros(64, dtype=torch.bool, device=gpu)
    flags[torch.randperm(64, generator=torch.Generator().manual_seed(1))[:n_dirty].to(gpu)] = True
    video.npc_dirty[:] = flags
    s0 = _state(npc, video)
    NP.update_points_pos(npc, video)                               # the torch yardstick
    want = _state(npc, video)
    assert not bool(video.npc_dirty.any())
    npc._full_pcl.zero_()
    npc._full_mask.zero_()
    _restore(npc, video, s0)
    stats = torch.zeros(2, dtype=torch.int64, device=gpu)
    assert NP.deform_points(npc, video, *cam, stats=stats)
    got = _state(npc, video)
    np.testing.assert_allclose(got["_input_pos"].cpu().numpy(), want["_input_pos"].cpu().numpy(), rtol=1e-5, atol=1e-5)
    np.testing.assert_allclose(got["_input_depth"].cpu().numpy(), want["_input_depth"].cpu().numpy(), rtol=1e-5)
    np.testing.assert_allclose(got["_cloud_pos"].cpu().numpy(), want["_cloud_pos"].cpu().numpy(), rtol=1e-5, atol=1e-5)
    assert torch.equal(got["_full_pcl"], want["_full_pcl"]) and torch.equal(got["_full_mask"], want["_full_mask"])
    assert not bool(video.npc_dirty.any())
    moved = int(flags.cpu().numpy()[vidx].sum())
    assert stats.tolist() == [n_dirty, moved]
    # the rebuilt index searches like a fresh one over the same cloud
    fresh = KnnIndex(gpu, cell_size=0.06, max_cells=1 << 21)
    fresh.set_points(npc.cloud_pos())
    q = npc.cloud_pos()[::97] + 0.01
    a, b = npc.index.search(q, 8, radius=0.1), fresh.search(q, 8, radius=0.1)
    assert all(torch.equal(x, y) for x, y in zip(a, b))


def test_deform_is_repeatable_and_records_into_a_graph(gpu):
    from glorie_slam_amd import neural_point as NP
    video, npc, cam, _ = _big(gpu, B=16, H=60, W=80, n_pts=40_000)
    video.npc_dirty[::2] = True
    s0 = _state(npc, video)
    NP.deform_points(npc, video, *cam, rebuild_index=False)
    first = _state(npc, video)
    _restore(npc, video, s0)
    NP.deform_points(npc, video, *cam, rebuild_index=False)
    second = _state(npc, video)
    assert all(torch.equal(first[k], second[k]) for k in first)
    # record deform + unproject, then move the poses and change the flags: the replay equals the eager call
    _restore(npc, video, s0)
    stats = torch.zeros(2, dtype=torch.int64, device=gpu)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        NP.deform_points(npc, video, *cam, stats=stats, rebuild_index=False)
    torch.cuda.synchronize()
    _restore(npc, video, s0)
    video.poses[:16, :3] += 0.05
    video.npc_dirty[:] = False
    video.npc_dirty[1:16:3] = True
    s1 = _state(npc, video)
    g.replay()
    replayed = _state(npc, video)
    _restore(npc, video, s1)
    NP.deform_points(npc, video, *cam, rebuild_index=False)
    eager = _state(npc, video)
    assert all(torch.equal(replayed[k], eager[k]) for k in eager)
    assert not bool(video.npc_dirty.any()) and int(stats[0]) == 5


def test_deform_edge_cases(gpu):
    from glorie_slam_amd import _lib as L
    from glorie_slam_amd import neural_point as NP
    video, npc, cam, vidx = _big(gpu, B=8, H=48, W=64, n_pts=8_000)
    NP.deform_points(npc, video, *cam)                              # allocates full_pcl with nothing dirty
    s0 = _state(npc, video)
    assert NP.deform_points(npc, video, *cam)
    s1 = _state(npc, video)
    assert all(torch.equal(s0[k], s1[k]) for k in s0)               # nothing dirty: every byte unchanged
    # an empty cloud returns and leaves the flags set
    from glorie_slam_amd.neural_point import NeuralPointCloud
    empty = NeuralPointCloud(npc.cfg, video)
    video.npc_dirty[2] = True
    assert not NP.deform_points(empty, video, *cam) and bool(video.npc_dirty[2])
    # a dirty keyframe without points: its map is refreshed, the others untouched
    keep = torch.from_numpy(vidx != 3).to(gpu)
    rows = keep.repeat_interleave(npc.N_add)
    for k in ("_input_video_idx", "_input_j", "_input_i", "_input_depth", "_input_pos"):
        setattr(npc, k, getattr(npc, k)[keep].contiguous())
    npc._cloud_pos = npc._cloud_pos[rows].contiguous()
    npc._pts_num = npc._cloud_pos.shape[0]
    video.npc_dirty[:] = False
    video.npc_dirty[3] = True
    video.disps_up[3] *= 0.5
    before = npc._cloud_pos.clone()
    assert NP.deform_points(npc, video, *cam)
    assert torch.equal(before, npc._cloud_pos) and not bool(video.npc_dirty.any())
    ref = NeuralPointCloud(npc.cfg, video)
    ref.add_points(3)
    assert torch.equal(ref.full_pcl()[3], npc.full_pcl()[3])
    # the all-holes rule: keyframe 1 loses every valid pixel -> its points keep their depth, follow the pose
    video.valid_depth_mask[1] = False
    video.npc_dirty[1] = True
    m1 = npc._input_video_idx == 1
    d_before = npc._input_depth[m1].clone()
    NP.deform_points(npc, video, *cam)
    assert torch.equal(npc._input_depth[m1], d_before) and bool(torch.isfinite(npc._input_pos).all())
    # cloud rows without an input point (the plain add_points(pts) path): an error status
    npc.geo_feats = torch.zeros(npc._cloud_pos.shape[0], npc.c_dim, device=gpu)
    npc.col_feats = torch.zeros_like(npc.geo_feats)
    npc.add_points(torch.zeros(4, 3, device=gpu))
    video.npc_dirty[1] = True
    with pytest.raises(L.GlorieError):
        NP.deform_points(npc, video, *cam)


def test_rigid_motion_moves_every_point(gpu):
    from glorie_slam_amd import neural_point as NP
    video, npc, cam, _ = _big(gpu, B=16, H=60, W=80, n_pts=40_000)
    video.npc_dirty[:16] = True
    NP.deform_points(npc, video, *cam)
    p0 = npc._input_pos.double().cpu().numpy()
    c0 = npc._cloud_pos.double().cpu().numpy()
    ang = 0.3
    RT = np.array([[np.cos(ang), -np.sin(ang), 0], [np.sin(ang), np.cos(ang), 0], [0, 0, 1]]) @ \
        np.array([[1, 0, 0], [0, np.cos(0.2), -np.sin(0.2)], [0, np.sin(0.2), np.cos(0.2)]])
    tT = np.array([0.3, -0.2, 0.5])
    poses = video.poses[:16].double().cpu().numpy()
    for b in range(16):
        x, y, z, w = poses[b, 3:]
        R = np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                      [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                      [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])
        R2 = R @ RT.T                                               # w2c' = w2c T^-1
        poses[b, :3] = poses[b, :3] - R2 @ tT
        poses[b, 3:] = _quat(R2)
    video.poses[:16] = torch.from_numpy(poses).float().to(gpu)
    video.npc_dirty[:16] = True
    NP.deform_points(npc, video, *cam)
    np.testing.assert_allclose(npc._input_pos.cpu().numpy(), p0 @ RT.T + tT, rtol=1e-5, atol=1e-5)
    np.testing.assert_allclose(npc._cloud_pos.cpu().numpy(), c0 @ RT.T + tT, rtol=1e-5, atol=1e-5)


def _proxy_npc(c, gpu, counter):
    npc = types.SimpleNamespace(_full_pcl=_t(c["full_pcl"], gpu), _full_mask=_t(c["full_mask"], gpu))
    video = types.SimpleNamespace(counter=types.SimpleNamespace(value=counter))
    return npc, video


def test_proxy_depth_matches_the_reference(gpu):
    from glorie_slam_amd.neural_point import proxy_render_depth
    c = load()
    H, W, mws = c["H"], c["W"], int(c["mapping_window_size"])
    cam = (c["fx"], c["fy"], c["cx"], c["cy"])
    droid, mono, c2w = _t(c["proxy_droid"], gpu), _t(c["proxy_mono"], gpu), _t(c["proxy_c2w"], gpu)
    for counter in (3, 9):                                           # row -2 (wrapped to H - 2) and row 4
        npc, video = _proxy_npc(c, gpu, counter)
        proj = proj_depth_ref(c["full_pcl"], c["full_mask"], counter, mws, c["proxy_c2w"], *cam)
        for use_mono in (1, 0):
            got = proxy_render_depth(npc, video, c2w, droid, mono, mws, *cam, use_mono_to_complete=bool(use_mono))
            got = got.cpu().numpy()
            np.testing.assert_allclose(got, c[f"proxy_c{counter}_m{use_mono}"], rtol=1e-5, atol=0)
            np.testing.assert_allclose(got, proxy_depth_ref(proj, c["proxy_droid"], c["proxy_mono"], bool(use_mono)),
                                       rtol=1e-5, atol=0)
        # the projection alone: no tracker depth, no mono completion
        alone = proxy_render_depth(npc, video, c2w, torch.zeros_like(droid), mono, mws, *cam, use_mono_to_complete=False)
        np.testing.assert_allclose(alone.cpu().numpy(), c[f"proj_c{counter}"], rtol=1e-5, atol=0)
    # a row outside [-H, H) (the reference raises IndexError): nothing zeroed, against the restatement
    counter = mws + H + 3
    npc, video = _proxy_npc(c, gpu, counter)
    got = proxy_render_depth(npc, video, c2w, droid, mono, mws, *cam)
    proj = proj_depth_ref(c["full_pcl"], c["full_mask"], counter, mws, c["proxy_c2w"], *cam)
    np.testing.assert_allclose(got.cpu().numpy(), proxy_depth_ref(proj, c["proxy_droid"], c["proxy_mono"]), rtol=1e-5,
                               atol=0)
    # repeatable
    again = proxy_render_depth(npc, video, c2w, droid, mono, mws, *cam)
    assert torch.equal(got, again)


# ---- SequenceRunner --------------------------------------------------------------------------------------------------
H_RUN, W_RUN, ITERS, RAYS = 240, 320, 6, 1000


def _runner(gpu, monkeypatch, K, keys=True, graphs=False, probe=None, few_valid=(), corrupt_holes=False, **opts):
    """keyframes [0, K] of the synthetic stream set up as init_state does (disps_up = 1 / full), timestamps = ids,
    valid_depth_mask with a band of holes and a random 10 %; keys: bind_npc_with_pose + render_depth "proxy" in the cfg.
    corrupt_holes: disps_up halved where the mask is false (a depth a runner that ignored the mask would train on);
    c["true_depth"] [K+1,H,W] is 1 / disps_up before that"""
    import glorie_slam_amd.pipeline as P
    orig = P.synthetic_cfg

    def cfg(*a, **k):
        c = orig(*a, **k)
        if keys:
            c["pointcloud"]["bind_npc_with_pose"] = True
            c["mapping"]["render_depth"] = "proxy"
        return c
    monkeypatch.setattr(P, "synthetic_cfg", cfg)
    run, c = P.synthetic_runner(gpu, K + 1, map_iters=ITERS, map_rays=RAYS, H=H_RUN, W=W_RUN)
    monkeypatch.setattr(P, "synthetic_cfg", orig)
    for key, val in opts.items():
        setattr(run, key, val)
    run.map_graph = graphs
    if probe is not None:
        run.map_probe = lambda k, t: probe(run, k, t)
    video, imgs = c["video"], P.synthetic_images(K + 1, H_RUN, W_RUN)
    g = torch.Generator().manual_seed(7)
    for k in range(K + 1):
        run.init_state(k)
        video.timestamp[k] = k
        run.images[k] = imgs[k].to(gpu)
        m = torch.rand(H_RUN, W_RUN, generator=g) > 0.1
        m[:, 40 + 20 * k: 90 + 20 * k] = False
        if k in few_valid:
            m[:] = False
            m[:5, :10] = True                                       # 50 valid pixels
        video.valid_depth_mask[k] = m.to(gpu)
    video.intrinsics[:K + 1] = c["intrinsics"].to(gpu) / 8.0
    video.counter.value = K + 1
    c["true_depth"] = 1.0 / video.disps_up[:K + 1].double().cpu().numpy()
    if corrupt_holes:
        video.disps_up[:K + 1] = torch.where(video.valid_depth_mask[:K + 1], video.disps_up[:K + 1],
                                             0.5 * video.disps_up[:K + 1])
    return run, c


def _expected_depth(run, f):
    """restated proxy depth of frame f against the runner's current unprojected maps"""
    v, ren = run.video, run.renderer
    pose = v.poses[f].cpu().numpy()
    disps = v.disps_up[f].cpu().numpy()
    valid = v.valid_depth_mask[f].cpu().numpy()
    c2w, wq, droid = c2w_and_depth_ref(pose, disps, valid, run.mono_priors[f].cpu().numpy())
    n = v.counter.value
    proj = proj_depth_ref(run.npc.full_pcl()[:n].cpu().numpy(), run.npc.full_mask()[:n].cpu().numpy(), n,
                          run.mapping_window_size, c2w, ren.fx, ren.fy, ren.cx, ren.cy)
    return proxy_depth_ref(proj, droid, wq), droid, proj


WINDOW = dict(keyframe_selection_method="overlap", mapping_window_size=4)


def test_runner_trains_on_the_proxy_depth(gpu, monkeypatch):
    seen = []

    def probe(run, k, t):
        if seen and seen[-1][0] == k:
            return
        win = t["window"]
        window = list(win["window"]) if win is not None else [k]
        per = win["per"] if win is not None else RAYS
        exp = {f: _expected_depth(run, f) for f in window}
        seen.append((k, window, per, t["pix"].clone(), t["d"].clone(), exp))

    run, c = _runner(gpu, monkeypatch, 4, probe=probe, corrupt_holes=True, **WINDOW)
    for k in range(5):
        run.map_keyframe(k)
    assert run.render_depth == "proxy" and run.bind_npc_with_pose and run.use_mono_to_complete
    assert len(seen) == 5 and any(len(w) > 2 for _, w, *_ in seen)
    full = c["true_depth"]
    up = 1.0 / c["video"].disps_up[:5].double().cpu().numpy()           # doubled at the holes
    # the synthetic prior is an affine distortion of the depth: m_wq recovers it (fp32 sums of the alignment)
    v = c["video"]
    for f, m in run.mono_priors.items():
        wq = (m * v.depth_scale[f] + v.depth_shift[f]).double().cpu().numpy()
        np.testing.assert_allclose(wq, full[f], rtol=1e-3)
    n_mono = 0
    for k, window, per, pix, d, exp in seen:
        for n, f in enumerate(window):
            sl = slice(n * per, (n + 1) * per)
            ii, jj = pix[0, sl].cpu().numpy(), pix[1, sl].cpu().numpy()
            want, droid, proj = (x[jj, ii] for x in exp[f])
            got = d[sl].cpu().numpy()
            rel = np.abs(got - want) / want
            assert (rel > 1e-3).mean() < 1e-2, (k, f, (rel > 1e-3).mean())
            # where neither the tracker nor the projection has a depth: the aligned mono prior = the true depth (up to
            # the rays whose point fp32 puts in a neighbouring pixel)
            mono = (droid == 0) & (proj == 0)
            off = np.abs(got[mono] / full[f][jj[mono], ii[mono]] - 1) > 1e-3
            assert off.mean() < 2e-2 if mono.any() else True, (k, f, off.mean())
            n_mono += int(mono.sum())
            # at the holes the target is not 1 / disps_up (what the runner trains on without the keys): the projection or
            # the prior, about half of it here
            holes = droid == 0
            assert holes.any() and (np.abs(got[holes] / up[f][jj[holes], ii[holes]] - 1) > 0.05).mean() > 0.98
            np.testing.assert_allclose(got[droid > 0], droid[droid > 0], rtol=1e-6)
    assert n_mono > 50


def test_runner_points_follow_a_moved_trajectory(gpu, monkeypatch):
    K = 3
    run, c = _runner(gpu, monkeypatch, K)
    video, npc = c["video"], c["npc"]
    for k in range(K):
        run.map_keyframe(k)
    vidx = npc._input_video_idx.clone()
    p0 = npc._input_pos.double().cpu().numpy()
    RT = np.array([[np.cos(0.2), 0, np.sin(0.2)], [0, 1, 0], [-np.sin(0.2), 0, np.cos(0.2)]])
    tT = np.array([0.1, 0.2, -0.3])
    poses = video.poses[:K + 1].double().cpu().numpy()
    for b in range(K + 1):
        x, y, z, w = poses[b, 3:]
        R = np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                      [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                      [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])
        R2 = R @ RT.T
        poses[b, :3] = poses[b, :3] - R2 @ tT
        poses[b, 3:] = _quat(R2)
    video.poses[:K + 1] = torch.from_numpy(poses).float().to(gpu)
    video.set_dirty(0, K)
    run.map_keyframe(K)
    n0 = p0.shape[0]
    np.testing.assert_allclose(npc._input_pos[:n0].cpu().numpy(), p0 @ RT.T + tT, rtol=1e-4, atol=1e-4)
    assert torch.equal(npc._input_video_idx[:n0], vidx)
    # nothing was dirty before keyframe K: those calls returned without a launch or an index rebuild
    assert run.deform_stats["calls"] == 1 and run.deform_stats["dirty_keyframes"] == K
    assert run.deform_stats["points_moved"] == n0 and not bool(video.npc_dirty.any())


def test_runner_skips_frames_with_few_valid_depths(gpu, monkeypatch):
    wins = []
    run, c = _runner(gpu, monkeypatch, 3, few_valid=(1,),
                     probe=lambda run, k, t: wins.append((k, list(t["window"]["window"]), t["window"]["per"])),
                     **WINDOW)
    out = [run.map_keyframe(k) for k in range(4)]
    assert run.skipped == [1] and out[1] is None and all(out[k] is not None for k in (0, 2, 3))
    assert len(run.windows) == 3 and all(1 not in w for w in run.windows)
    # rays per frame count the skipped frame: keyframe 1 was in keyframe 2's window (k - 1)
    k2 = [(window, per) for k, window, per in wins if k == 2]
    assert k2 and all(per == RAYS // (len(window) + 1) for window, per in k2)


def test_runner_recorded_losses_agree(gpu, monkeypatch):
    def losses(graphs):
        run, _ = _runner(gpu, monkeypatch, 3, graphs=graphs, **WINDOW)
        return run, np.array([run.map_keyframe(k) for k in range(4)], dtype=np.float64)
    _, le = losses(False)
    _, l2 = losses(False)
    graph, lg = losses(True)
    assert graph.map_graph_stats["captures"] >= 1 and np.isfinite(lg).all()
    noise = np.abs(l2 - le).max()
    assert np.abs(lg - le).max() <= max(4.0 * noise, 3e-2 * np.abs(le).max()), (lg, le, noise)


def test_runner_without_the_keys(gpu, monkeypatch):
    import glorie_slam_amd.pipeline as P
    calls = []
    monkeypatch.setattr(P, "deform_points", lambda *a, **k: calls.append(1))
    seen = []
    run, c = _runner(gpu, monkeypatch, 2, keys=False, probe=lambda run, k, t: seen.append((k, t["pix"].clone(),
                                                                                          t["d"].clone())))
    for k in range(3):
        run.map_keyframe(k)
    assert run.render_depth is None and not run.bind_npc_with_pose and not calls and run.skipped == []
    du = c["video"].disps_up
    for k, pix, d in seen:
        want = torch.where(du[k] > 0, 1.0 / du[k].clamp_min(1e-6), torch.zeros_like(du[k]))[pix[1], pix[0]]
        assert torch.equal(d, want)


def test_long_sequence_with_both_keys(gpu):
    from glorie_slam_amd.pipeline import synthetic_long_runner
    run, c, frames = synthetic_long_runner(gpu, n_frames=48, leg=16, map_iters=4, map_rays=500, buffer=64, ba_every=12,
                                           H=H_RUN, W=W_RUN)
    run.bind_npc_with_pose, run.render_depth = True, "proxy"
    res = run.run(frames(), c["intrinsics"])
    assert res["mapped"] == len(run.losses) + len(run.skipped) and not run.skipped
    assert np.isfinite(np.array(run.losses)).all()
    assert run.deform_stats["calls"] > 0 and run.deform_stats["dirty_keyframes"] > 0
    assert run.deform_stats["points_moved"] > 0
    # the run closed a loop (a global BA over [0, t) inside the frontend) and ran the periodic global BAs
    assert getattr(run.frontend, "last_loop_t", 0) > 0 and len(run.timing["ba_ms"]) > 0
    assert bool(torch.isfinite(run.npc.cloud_pos()).all()) and not bool(run.video.npc_dirty.any())


def test_runner_mono_render_depth_and_deformation(gpu, monkeypatch):
    """render_depth "mono" given to the runner (not in the cfg) with bind_npc_with_pose: the keyframe being mapped and a
    keyframe not mapped yet are dirty, their priors are loaded on demand; the points follow a moved trajectory and every
    frame trains on its aligned mono prior"""
    K = 3
    seen = []

    def probe(run, k, t):
        v = run.video
        wq = run.mono_priors[k] * v.depth_scale[k] + v.depth_shift[k]
        seen.append((k, t["d"].clone(), wq[t["pix"][1], t["pix"][0]].clone()))

    run, c = _runner(gpu, monkeypatch, K, keys=False, probe=probe, bind_npc_with_pose=True, render_depth="mono")
    video, npc = c["video"], c["npc"]
    assert "render_depth" not in run.cfg["mapping"]
    for k in range(K - 1):
        run.map_keyframe(k)
    p0 = npc._input_pos.double().cpu().numpy()
    RT = np.array([[np.cos(0.2), 0, np.sin(0.2)], [0, 1, 0], [-np.sin(0.2), 0, np.cos(0.2)]])
    tT = np.array([0.1, 0.2, -0.3])
    poses = video.poses[:K + 1].double().cpu().numpy()
    for b in range(K + 1):
        x, y, z, w = poses[b, 3:]
        R = np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                      [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                      [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])
        R2 = R @ RT.T
        poses[b, :3] = poses[b, :3] - R2 @ tT
        poses[b, 3:] = _quat(R2)
    video.poses[:K + 1] = torch.from_numpy(poses).float().to(gpu)
    video.set_dirty(0, K + 1)                       # K - 1 (mapped next) and K (not mapped) are dirty
    assert run.map_keyframe(K - 1) is not None
    assert sorted(run.mono_priors) == list(range(K + 1)) and not bool(video.npc_dirty.any())
    assert run.deform_stats == {"calls": 1, "dirty_keyframes": K + 1, "points_moved": p0.shape[0]}
    # the points of keyframes 0 .. K-2 were re-placed from the moved poses and their re-aligned priors
    np.testing.assert_allclose(npc._input_pos[:p0.shape[0]].cpu().numpy(), p0 @ RT.T + tT, rtol=0, atol=1e-2)
    assert float(np.abs(p0 @ RT.T + tT - p0).max()) > 0.2
    # the training depth is m_wq
    assert [k for k, *_ in seen[::ITERS]] == list(range(K))
    for k, d, wq in seen:
        torch.testing.assert_close(d, wq, rtol=1e-6, atol=0)
