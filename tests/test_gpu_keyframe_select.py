"""Keyframe selection on the HIP kernels (glorie_slam_amd/keyframe_select.py, csrc/select.hip) and SequenceRunner's use of
it (reference: src/mapper.py:126-244, :541-554, :591-621, :675-677).

  * against the reference's own values (tests/golden/keyframe_select.npz, tests/golden/make_keyframe_select.py);
  * against the float64 restatement (tests/keyframe_select_ref.py) at the product shape: the 524,286-point box cloud
    seen by a 640x480 camera whose depth map has holes, and at prefixes of it from one point to just past one chunk of
    the scan;
  * repeated calls bitwise equal, the empty cases, an all-zero depth map, a recorded call replayed;
  * SequenceRunner with keyframe_selection_method "overlap" (windows of selected + [k-1, k], a turned-away keyframe never
    selected), with frustum_feature_selection (only rows inside the mask change, eager and recorded agree), and with the
    options off (nothing changes)."""
import numpy as np
import pytest
import torch

from keyframe_select_ref import frustum_ref, overlap_ref
from test_keyframe_select_oracle import load

pytestmark = pytest.mark.gpu


def _t(x, dev):
    return (x if torch.is_tensor(x) else torch.from_numpy(np.ascontiguousarray(x))).to(dev)


def _frustum(dev, pts, c2w, depth, K, H, W, edge):
    from glorie_slam_amd.keyframe_select import frustum_feature_mask
    mask, count, idx = frustum_feature_mask(_t(pts, dev), _t(c2w, dev), _t(depth, dev), *K, H, W, edge,
                                            return_indices=True)
    torch.cuda.synchronize()
    n = int(count)
    return mask.cpu().numpy(), n, idx[:n].cpu().numpy()


def test_frustum_matches_the_reference(gpu):
    c = load()
    K = (c["fx"], c["fy"], c["cx"], c["cy"])
    for edge in (-4, 6):
        want = c[f"frustum_mask_{edge}"]
        mask, n, idx = _frustum(gpu, c["frustum_points"], c["frustum_c2w"], c["frustum_depth"], K, c["H"], c["W"], edge)
        assert np.array_equal(mask, want), (edge, int((mask != want).sum()))
        assert n == int(want.sum()) and np.array_equal(idx, np.nonzero(want)[0])
        from glorie_slam_amd.keyframe_select import get_mask_from_c2w
        assert get_mask_from_c2w(_t(c["frustum_c2w"], gpu), c["frustum_depth"], _t(c["frustum_points"], gpu), *K,
                                 c["H"], c["W"], edge) == np.nonzero(want)[0].tolist()


def test_overlap_matches_the_reference(gpu):
    from glorie_slam_amd.keyframe_select import keyframe_overlap, overlap_candidates
    c = load()
    S = int(c["overlap_samples"])
    inside, total = keyframe_overlap(_t(c["overlap_rays_o"], gpu), _t(c["overlap_rays_d"], gpu),
                                     _t(c["overlap_ray_depth"], gpu), _t(c["overlap_c2ws"], gpu), c["fx"], c["fy"],
                                     c["cx"], c["cy"], c["H"], c["W"], n_samples=S, return_counts=True)
    total = int(total)
    want = np.round(c["overlap_percent"] * total).astype(np.int64)
    assert np.array_equal(inside.cpu().numpy(), want)
    percent = keyframe_overlap(_t(c["overlap_rays_o"], gpu), _t(c["overlap_rays_d"], gpu),
                               _t(c["overlap_ray_depth"], gpu), _t(c["overlap_c2ws"], gpu), c["fx"], c["fy"], c["cx"],
                               c["cy"], c["H"], c["W"], n_samples=S).cpu().numpy()
    assert np.array_equal(percent, c["overlap_percent"])
    assert overlap_candidates(percent)[:int(c["overlap_k"])] == c["overlap_selected"].tolist()


def product_case(holes=True):
    """the bench's box cloud and camera (synth.box_cloud, synth.box_rays) with the camera's depth map, a few holes in it"""
    from glorie_slam_amd import synth
    pts, _, _ = synth.box_cloud()
    _, _, depth, _, c2w = synth.box_rays()
    H, W = 480, 640
    depth = depth.reshape(H, W).copy()
    if holes:
        depth[100:140, 200:260] = 0
        depth[300:310, :] = 0
        depth[:, 620:] = 0
    return pts, c2w, depth, (320.0, 320.0, 319.5, 239.5), H, W


def test_frustum_matches_the_restatement_at_the_product_shape(gpu):
    pts, c2w, depth, K, H, W = product_case()
    assert pts.shape[0] == 524286
    for edge in (-4.0, 6.0):
        mask, n, idx = _frustum(gpu, pts, c2w, depth, K, H, W, edge)
        ref, d = frustum_ref(pts, c2w, depth, *K, H, W, edge)
        assert n == int(mask.sum()) and np.array_equal(idx, np.nonzero(mask)[0])
        rel = lambda x, t: np.abs(x - t) <= 1e-4 * np.maximum(np.abs(t), 1.0)
        q = lambda x: np.abs(x * 32 - np.floor(x * 32) - 0.5) < 1e-2          # a 1/32-px rounding boundary
        near = rel(d["u"], edge) | rel(d["u"], W - edge) | rel(d["v"], edge) | rel(d["v"], H - edge) | \
            rel(d["negz"], 0.0) | rel(d["negz"], d["depth"] + 0.5) | q(d["u"]) | q(d["v"])
        diff = mask.astype(bool) != ref
        print(f"edge {edge}: kept {n} of {len(pts)}, restatement {int(ref.sum())}, differing {int(diff.sum())}")
        assert not (diff & ~near).any(), np.nonzero(diff & ~near)[0][:10]
        assert ref.sum() > 50000 and (~ref).sum() > 50000 and (d["sample"] == 0).any()


@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257, 1000, 262144, 262145, 263000])
def test_frustum_matches_the_restatement_at_ragged_sizes(gpu, n):
    """the first n points of a fixed permutation of the product cloud: one point, partial waves and workgroups, and the
    first workgroups past one 1024-workgroup chunk of the scan (262144 points = 1024 workgroups of 256)"""
    pts, c2w, depth, K, H, W = product_case()
    pts = pts[np.random.default_rng(11).permutation(len(pts))[:n]]
    for edge in (-4.0, 6.0):
        mask, count, idx = _frustum(gpu, pts, c2w, depth, K, H, W, edge)
        ref, d = frustum_ref(pts, c2w, depth, *K, H, W, edge)
        assert mask.shape == (n,)
        assert count == int(mask.sum()) and np.array_equal(idx, np.nonzero(mask)[0])
        rel = lambda x, t: np.abs(x - t) <= 1e-4 * np.maximum(np.abs(t), 1.0)
        q = lambda x: np.abs(x * 32 - np.floor(x * 32) - 0.5) < 1e-2          # a 1/32-px rounding boundary
        near = rel(d["u"], edge) | rel(d["u"], W - edge) | rel(d["v"], edge) | rel(d["v"], H - edge) | \
            rel(d["negz"], 0.0) | rel(d["negz"], d["depth"] + 0.5) | q(d["u"]) | q(d["v"])
        diff = mask.astype(bool) != ref
        print(f"n {n} edge {edge}: kept {count}, restatement {int(ref.sum())}, differing {int(diff.sum())}, "
              f"near a threshold {near.mean():.4f}")
        assert not (diff & ~near).any(), np.nonzero(diff & ~near)[0][:10]
        if n >= 256:                                               # the band must not be what passes the test
            assert near.mean() <= 0.05, near.mean()


def test_repeated_calls_and_empty_cases(gpu):
    from glorie_slam_amd.keyframe_select import frustum_feature_mask, keyframe_overlap
    pts, c2w, depth, K, H, W = product_case()
    first = _frustum(gpu, pts, c2w, depth, K, H, W, -4.0)
    for _ in range(3):
        again = _frustum(gpu, pts, c2w, depth, K, H, W, -4.0)
        assert np.array_equal(again[0], first[0]) and again[1] == first[1] and np.array_equal(again[2], first[2])
    # n = 0
    mask, count = frustum_feature_mask(torch.zeros(0, 3, device=gpu), _t(c2w, gpu), _t(depth, gpu), *K, H, W, -4)
    assert mask.numel() == 0 and int(count) == 0
    # an all-zero depth map: every sample is 0 and so is the maximum - kept are the points with 0 <= -z <= 0.5
    zero = np.zeros_like(depth)
    mask, n, idx = _frustum(gpu, pts, c2w, zero, K, H, W, -4.0)
    ref, _ = frustum_ref(pts, c2w, zero, *K, H, W, -4.0)
    assert n == int(ref.sum()) == int(mask.sum())
    # overlap: K = 0, R = 0, and repeated calls
    o, d = torch.zeros(10, 3, device=gpu), torch.randn(10, 3, device=gpu)
    dep = torch.rand(10, device=gpu) + 1.0
    c2ws = _t(np.stack([c2w, c2w]), gpu)
    assert keyframe_overlap(o, d, dep, c2ws[:0], *K, H, W).numel() == 0
    inside, total = keyframe_overlap(o[:0], d[:0], dep[:0], c2ws, *K, H, W, return_counts=True)
    assert inside.tolist() == [0, 0] and int(total) == 0
    assert torch.isnan(keyframe_overlap(o[:0], d[:0], dep[:0], c2ws, *K, H, W)).all()
    a = keyframe_overlap(o, d, dep, c2ws, *K, H, W, return_counts=True)[0]
    for _ in range(3):
        assert torch.equal(keyframe_overlap(o, d, dep, c2ws, *K, H, W, return_counts=True)[0], a)


def test_overlap_matches_the_restatement_with_many_keyframes(gpu):
    """200 rays of the box camera x 8 samples against 64 keyframes turned and moved about the box centre"""
    from glorie_slam_amd.keyframe_select import keyframe_overlap
    from glorie_slam_amd import synth
    ro, rd, depth, _, c2w = synth.box_rays()
    g = np.random.default_rng(3)
    sel = g.choice(len(depth), 200, replace=False)
    ro, rd, dep = ro[sel], rd[sel], depth[sel].copy()
    dep[:20] = 0                                                   # rays without depth are skipped
    c2ws = []
    for k in range(64):
        a = 0.1 * k
        R = np.array([[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1]]) @ c2w[:3, :3]
        M = np.eye(4)
        M[:3, :3], M[:3, 3] = R, g.uniform(-0.5, 0.5, 3)
        c2ws.append(M)
    c2ws = np.stack(c2ws).astype(np.float32)
    K = (320.0, 320.0, 319.5, 239.5)
    inside, total = keyframe_overlap(_t(ro, gpu), _t(rd, gpu), _t(dep, gpu), _t(c2ws, gpu), *K, 480, 640,
                                     return_counts=True)
    want, wtotal = overlap_ref(ro, rd, dep, c2ws, *K, 480, 640)
    assert int(total) == wtotal == 180 * 8
    got = inside.cpu().numpy()
    assert (want > 0).sum() > 5 and (want == 0).sum() > 5
    assert np.abs(got - want).max() <= 2, np.abs(got - want).max()      # only samples at a threshold may differ


def test_recorded_call_replays_the_eager_result(gpu):
    from glorie_slam_amd.keyframe_select import frustum_feature_mask, keyframe_overlap
    pts, c2w, depth, K, H, W = product_case()
    P, C, D = _t(pts, gpu), _t(c2w, gpu), _t(depth, gpu)
    from glorie_slam_amd import synth
    ro, rd, dep, _, _ = synth.box_rays()
    ro, rd, dep = _t(ro[::1536], gpu), _t(rd[::1536], gpu), _t(dep[::1536], gpu)
    C2 = torch.stack([C, C])
    eager = frustum_feature_mask(P, C, D, *K, H, W, -4.0, return_indices=True)
    eager_in = keyframe_overlap(ro, rd, dep, C2, *K, H, W, return_counts=True)[0]
    torch.cuda.synchronize()
    s = torch.cuda.Stream(gpu)
    s.wait_stream(torch.cuda.current_stream(gpu))
    with torch.cuda.stream(s):                    # warm the allocator outside the capture
        frustum_feature_mask(P, C, D, *K, H, W, -4.0, return_indices=True)
    torch.cuda.current_stream(gpu).wait_stream(s)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = frustum_feature_mask(P, C, D, *K, H, W, -4.0, return_indices=True)
        out_in = keyframe_overlap(ro, rd, dep, C2, *K, H, W, return_counts=True)[0]
    for _ in range(2):
        out[0].zero_(), out[1].fill_(-1), out_in.fill_(-1)
        g.replay()
        torch.cuda.synchronize()
        n = int(eager[1])
        assert torch.equal(out[0], eager[0]) and int(out[1]) == n and torch.equal(out[2][:n], eager[2][:n])
        assert torch.equal(out_in, eager_in)


# ---- SequenceRunner --------------------------------------------------------------------------------------------------
K_RUN, ITERS, RAYS, TURNED = 8, 6, 1000, 2


def _quat_mul(a, b):
    ax, ay, az, aw = a
    bx, by, bz, bw = b
    return torch.stack([aw * bx + ax * bw + ay * bz - az * by, aw * by - ax * bz + ay * bw + az * bx,
                        aw * bz + ax * by - ay * bx + az * bw, aw * bw - ax * bx - ay * by - az * bz])


def _run(gpu, graphs, turned=None, probe=None, **opts):
    """K_RUN keyframes of the synthetic stream mapped as in test_gpu_pix_warp._window_run; turned: this keyframe's pose is
    rotated by pi about its camera's y axis (it looks away from every other one)"""
    from glorie_slam_amd.pipeline import synthetic_images, synthetic_runner
    run, c = synthetic_runner(gpu, K_RUN, zero_flow_head=True, map_iters=ITERS, map_rays=RAYS)
    for key, val in opts.items():
        setattr(run, key, val)
    run.map_graph = graphs
    if probe is not None:
        run.map_probe = lambda k, t: probe(run, k, t)
    video, imgs = c["video"], synthetic_images(K_RUN)
    poses = c["poses"][:K_RUN].clone()
    if turned is not None:
        p = poses[turned]
        flip = torch.tensor([0.0, 1.0, 0.0, 0.0], device=p.device, dtype=p.dtype)      # pi about y, w2c side
        poses[turned, 3:] = _quat_mul(flip, p[3:])
        poses[turned, :3] = p[:3] * torch.tensor([-1.0, 1.0, -1.0], device=p.device, dtype=p.dtype)
    video.poses[:K_RUN] = poses
    video.disps[:K_RUN] = c["disps"][:K_RUN]
    video.disps_up[:K_RUN] = torch.nn.functional.interpolate(c["disps"][:K_RUN, None], scale_factor=8, mode="bilinear",
                                                             align_corners=False)[:, 0]
    video.counter.value = K_RUN
    losses = []
    for k in range(K_RUN):
        run.images[k] = imgs[k].to(gpu)
        losses.append(run.map_keyframe(k))
    torch.cuda.synchronize()
    return run, np.array(losses)


def _full_overlap(run, k, f):
    """restatement: samples of every pixel of k's view with depth, inside keyframe f (a superset of any draw)"""
    from glorie_slam_amd.common import get_rays_from_uv
    depth, c2w = run._keyframe_view(k)
    H, W = depth.shape
    jj, ii = torch.meshgrid(torch.arange(0, H, device=depth.device), torch.arange(0, W, device=depth.device),
                            indexing="ij")
    ren = run.renderer
    ro, rd = get_rays_from_uv(ii.reshape(-1).float(), jj.reshape(-1).float(), c2w, ren.fx, ren.fy, ren.cx, ren.cy,
                              depth.device)
    c2wf = run._keyframe_view(f)[1].cpu().numpy()
    inside, _ = overlap_ref(ro.reshape(-1, 3).cpu().numpy(), rd.reshape(-1, 3).cpu().numpy(),
                            depth.reshape(-1).cpu().numpy(), c2wf[None], ren.fx, ren.fy, ren.cx, ren.cy, H, W)
    return int(inside[0])


def test_runner_overlap_windows(gpu):
    run, _ = _run(gpu, True, turned=TURNED, keyframe_selection_method="overlap", mapping_window_size=5)
    again, _ = _run(gpu, True, turned=TURNED, keyframe_selection_method="overlap", mapping_window_size=5)
    print("windows", run.windows)
    assert run.windows == again.windows                            # same seed, same windows
    assert run.windows[0] == [0] and run.windows[1] == [0, 1]
    n_sel = 0
    for k, w in enumerate(run.windows):
        sel = w[:-2] if k > 0 else []
        assert w[-1] == k and (k == 0 or w[-2] == k - 1) and len(w) <= 5
        assert len(set(sel)) == len(sel) and all(0 <= f < k - 1 for f in sel)
        assert TURNED not in sel
        for f in sel:
            assert _full_overlap(run, k, f) > 0, (k, f)
        n_sel += len(sel)
    assert n_sel >= 6
    assert _full_overlap(run, TURNED + 2, TURNED) == 0              # the turned keyframe sees none of the others
    assert run.map_graph_stats["captures"] >= 1


def test_runner_global_windows(gpu):
    run, _ = _run(gpu, False, keyframe_selection_method="global", mapping_window_size=5)
    for k, w in enumerate(run.windows):
        sel = w[:-2] if k > 0 else []
        assert len(sel) == min(3, max(k - 1, 0)) and len(set(sel)) == len(sel) and all(0 <= f < k - 1 for f in sel)


@pytest.mark.parametrize("pix_warping", [False, True])
def test_runner_frustum_trains_only_the_masked_rows(gpu, pix_warping):
    snaps = {}

    def probe(run, k, t):
        if k not in snaps:
            snaps[k] = (run.npc.geo_feats.clone(), run.npc.col_feats.clone(), t["frustum"].clone())

    opts = dict(frustum_feature_selection=True, frustum_edge=-4.0, pix_warping=pix_warping, mapping_window_size=5,
                keyframe_selection_method="overlap")
    eager, le = _run(gpu, False, **opts)
    eager2, l2 = _run(gpu, False, **opts)
    graph, lg = _run(gpu, True, **opts)
    assert graph.map_graph_stats["captures"] >= 1
    assert len(eager.frustum_counts) == K_RUN and all(n > 0 for n in eager.frustum_counts)
    noise = np.abs(l2 - le).max()
    print("frustum counts", eager.frustum_counts, "loss noise", noise, "graph-eager", np.abs(lg - le).max())
    assert np.abs(lg - le).max() <= max(4.0 * noise, 3e-2 * np.abs(le).max()), (lg, le, noise)

    # one more keyframe of a fresh run, watched from inside: rows outside the mask keep their bits
    for graphs in (False, True):
        snaps.clear()
        run, _ = _run(gpu, graphs, probe=probe, **opts)
        k = K_RUN - 1
        geo0, col0, mask = snaps[k]
        m = mask.bool()
        n = geo0.shape[0]
        geo1, col1 = run.npc.geo_feats[:n], run.npc.col_feats[:n]
        assert int(m.sum()) == run.frustum_counts[k] and 0 < int(m.sum()) < n
        assert torch.equal(geo1[~m], geo0[~m]) and torch.equal(col1[~m], col0[~m])
        st = run.last_optimizer.state
        mg = st[id(run.last_optimizer.param_groups[1]["params"][0])]["m"]
        got_grad = (mg != 0).any(1)
        assert not (got_grad & ~m).any()                          # moments of rows outside the mask untouched
        changed = (geo1 != geo0).any(1)
        assert got_grad.sum() > 0 and int(changed[got_grad].sum()) >= 0.99 * int(got_grad.sum())


def test_runner_options_off_change_nothing(gpu):
    for pix_warping in (False, True):
        kw = dict(pix_warping=pix_warping, mapping_window_size=5 if pix_warping else 1)
        base, lb = _run(gpu, True, **kw)
        off, lo = _run(gpu, True, keyframe_selection_method=None, frustum_feature_selection=False, **kw)
        again, la = _run(gpu, True, **kw)
        old = [list(range(max(0, k - kw["mapping_window_size"] + 1), k + 1)) for k in range(K_RUN)]
        assert base.windows == off.windows == old
        assert base.frustum_counts == off.frustum_counts == []
        assert base.map_graph_stats == off.map_graph_stats
        noise = np.abs(la - lb).max()
        assert np.abs(lo - lb).max() <= max(4.0 * noise, 1e-6 * np.abs(lb).max()), (lo, lb, noise)
    # the constructor: keys absent -> off; cfg keys -> on; explicit False beats the config
    from glorie_slam_amd.pipeline import SequenceRunner
    cfg = {**base.cfg, "mapping": {"keyframe_selection_method": "overlap", "frustum_feature_selection": True,
                                   "frustum_edge": -4, "mapping_window_size": 5}}
    r = SequenceRunner(base.net, base.video, cfg, base.npc, base.decoders, base.renderer, lambda *a: None)
    assert r.keyframe_selection_method == "overlap" and r.frustum_feature_selection and r.frustum_edge == -4.0
    r = SequenceRunner(base.net, base.video, cfg, base.npc, base.decoders, base.renderer, lambda *a: None,
                       keyframe_selection_method=False, frustum_feature_selection=False)
    assert r.keyframe_selection_method is None and not r.frustum_feature_selection
    assert base.keyframe_selection_method is None and not base.frustum_feature_selection
