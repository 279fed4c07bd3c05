"""Colour-gradient radii and the gradient-ranked pixel draw on the HIP kernels (glorie_slam_amd/color_grad.py,
csrc/color_grad.hip) and SequenceRunner's use of them (reference: src/mapper.py:309-321, :449-453, :538, :719,
:767-784; src/utils/common.py:96-186).

  * against the reference's own values (tests/golden/color_grad.npz, tests/golden/make_color_grad.py), both layouts;
  * the top-M selection against the restatement's (-key, index) order at 640x480 and 1200x680, with large ties, fewer
    valid keys than M, M = n and no valid key, and at flat sizes from one key to a few workgroups;
  * repeated calls bitwise equal, a recorded call replayed on new inputs equal to the eager call;
  * SequenceRunner with the radius keys (per-frame query radii, insertion radii, eager and recorded losses), with
    pixels_based_on_color_grad (an is_pts_grad=True insertion on the selected pixels), and without the keys."""
import numpy as np
import pytest
import torch

from color_grad_ref import color_grad_maps_ref, top_indices_ref
from test_color_grad_oracle import load

pytestmark = pytest.mark.gpu


def _t(x, dev):
    return (x if torch.is_tensor(x) else torch.from_numpy(np.ascontiguousarray(x))).to(dev)


@pytest.mark.parametrize("channels_first", [False, True])
def test_maps_match_the_reference(gpu, channels_first):
    from glorie_slam_amd.color_grad import color_grad_maps, dynamic_radius_maps
    c = load()
    img = _t(c["image"], gpu)
    if channels_first:
        img = img.permute(2, 0, 1).contiguous()
    m = color_grad_maps(img, valid=_t(c["valid"].astype(bool), gpu), **c["args"])
    np.testing.assert_allclose(m["grad"].cpu().numpy(), c["grad"], rtol=1e-6, atol=2e-7)
    np.testing.assert_allclose(m["r_add"].cpu().numpy(), c["r_add"], rtol=1e-6)
    np.testing.assert_allclose(m["r_query"].cpu().numpy(), c["r_query"], rtol=1e-6)
    a = c["args"]
    ra, rq = dynamic_radius_maps(img, a["radius_add_max"], a["radius_add_min"], a["radius_query_ratio"],
                                 a["color_grad_threshold"])
    assert torch.equal(ra, m["r_add"]) and torch.equal(rq, m["r_query"])
    # depth-scaled maps: the unscaled map / 3 * depth in double, rounded once
    d = _t(c["depth"], gpu)
    s = color_grad_maps(img, depth_add=d, depth_query=d, **c["args"])
    np.testing.assert_allclose(s["r_add"].cpu().numpy(), c["r_add"].astype(np.float64) / 3 * c["depth"], rtol=1e-6)
    np.testing.assert_allclose(s["r_query"].cpu().numpy(), c["r_query"].astype(np.float64) / 3 * c["depth"],
                               rtol=1e-6)
    with pytest.raises(Exception):
        color_grad_maps(img, color_grad_threshold=0.01)


def test_candidates_match_the_reference(gpu):
    from glorie_slam_amd.color_grad import color_grad_maps, top_indices
    c = load()
    n = int(c["n"])
    grad = color_grad_maps(_t(c["image"], gpu), valid=_t(c["valid"].astype(bool), gpu), outputs=("grad",))["grad"]
    idx, valid = top_indices(grad, 5 * n)
    assert np.array_equal(idx.cpu().numpy(), c["candidates"]) and int(valid) == 5 * n


def test_samples_with_pixel_grad_match_the_reference(gpu, monkeypatch):
    import glorie_slam_amd.color_grad as cg
    c = load()
    monkeypatch.setattr(cg, "draw_candidates", lambda m, n, generator=None: torch.arange(min(m, n)))
    fx, fy, cx, cy = (float(x) for x in c["intrinsics"])
    ro, rd, d, col, i, j = cg.get_samples_with_pixel_grad(0, c["H"], 0, c["W"], int(c["n"]), c["H"], c["W"], fx, fy, cx,
                                                          cy, _t(c["c2w"], gpu), _t(c["depth"], gpu),
                                                          _t(c["image"], gpu), gpu, _t(c["valid"].astype(bool), gpu))
    assert np.array_equal(i.cpu().numpy(), c["s_i"]) and np.array_equal(j.cpu().numpy(), c["s_j"])
    for got, want in ((ro, c["s_rays_o"]), (rd, c["s_rays_d"]), (d, c["s_depth"]), (col, c["s_color"])):
        np.testing.assert_allclose(got.cpu().numpy(), want, rtol=1e-6, atol=1e-6)
    # a region smaller than the image (around the sharp band): candidates outside it filtered afterwards
    monkeypatch.undo()
    idx = cg.get_sample_uv_with_grad(0, 96, 90, 128, 30, _t(c["image"], gpu), _t(c["valid"].astype(bool), gpu))
    r, q = idx.cpu().numpy() // c["W"], idx.cpu().numpy() % c["W"]
    assert len(idx) == 30 and ((r >= 0) & (r < 96) & (q >= 90) & (q < 128)).all()
    assert np.isin(idx.cpu().numpy(), top_indices_ref(c["grad"], 150)[0]).all()
    with pytest.raises(ValueError):                    # fewer candidates in the region than picks, as np.random.choice
        cg.get_sample_uv_with_grad(0, 20, 0, 20, 30, _t(c["image"], gpu), _t(c["valid"].astype(bool), gpu))


def _keys(kind, n, seed):
    g = np.random.default_rng(seed)
    if kind == "random":
        k = g.uniform(0, 1, n).astype(np.float32)
        k[g.uniform(0, 1, n) < 0.1] = -1.0
    elif kind == "ties":                                    # large flat regions: a handful of values, zero among them
        k = g.choice(np.array([0.0, 0.0, 0.0, 0.25, 0.5, 0.5, 1.0], np.float32), n)
    elif kind == "few_valid":
        k = np.full(n, -1.0, np.float32)
        k[g.choice(n, 1234, replace=False)] = g.uniform(0, 1, 1234).astype(np.float32)
    else:                                                   # all invalid
        k = np.full(n, -1.0, np.float32)
    return k


@pytest.mark.parametrize("shape", [(480, 640), (680, 1200)])
@pytest.mark.parametrize("kind", ["random", "ties", "few_valid", "invalid"])
def test_top_m_matches_the_restatement(gpu, shape, kind):
    from glorie_slam_amd.color_grad import top_indices
    n = shape[0] * shape[1]
    keys = _keys(kind, n, shape[0] + len(kind))
    for M in (5000, n) if kind == "random" else (5000,):
        idx, valid = top_indices(_t(keys, gpu), M)
        want, want_valid = top_indices_ref(keys, M)
        assert np.array_equal(idx.cpu().numpy(), want), (kind, M)
        assert int(valid) == want_valid
    with pytest.raises(ValueError):
        top_indices(_t(keys, gpu), n + 1)
    if kind not in ("random", "ties"):
        return
    # the sizes at which the count / scan / rank chain changes path: one key, a partial wave, one wave and one key more, a
    # partial second workgroup, more than one workgroup (the two shapes above are past 1024 workgroups)
    for m in (1, 63, 64, 65, 257, 2049):
        small = _keys(kind, m, shape[0] + m)
        for M in sorted({1, max(m // 2, 1), m}):
            idx, valid = top_indices(_t(small, gpu), M)
            want, want_valid = top_indices_ref(small, M)
            assert np.array_equal(idx.cpu().numpy(), want), (kind, m, M)
            assert int(valid) == want_valid, (kind, m, M)


def test_repeat_and_replay(gpu):
    from glorie_slam_amd.color_grad import color_grad_maps, top_indices
    H, W, M = 480, 640, 5000
    g = torch.Generator().manual_seed(3)
    img = torch.rand(3, H, W, generator=g).to(gpu)
    valid = (torch.rand(H, W, generator=g) > 0.2).to(gpu)
    first = None
    for _ in range(3):
        m = color_grad_maps(img, valid=valid)
        idx, v = top_indices(m["grad"], M)
        out = [m["grad"], m["r_add"], m["r_query"], idx, v]
        if first is None:
            first = [t.clone() for t in out]
        assert all(torch.equal(a, b) for a, b in zip(first, out))
    # record maps + selection on static buffers, replay on new inputs
    s_img, s_valid = img.clone(), valid.clone()
    torch.cuda.synchronize()
    side = torch.cuda.Stream(gpu)
    side.wait_stream(torch.cuda.current_stream(gpu))
    with torch.cuda.stream(side):                     # warm-up outside the recording
        color_grad_maps(s_img, valid=s_valid)
    torch.cuda.current_stream(gpu).wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        gm = color_grad_maps(s_img, valid=s_valid)
        gidx, gv = top_indices(gm["grad"], M)
    for seed in (7, 8):
        g = torch.Generator().manual_seed(seed)
        s_img.copy_(torch.rand(3, H, W, generator=g).to(gpu))
        s_valid.copy_((torch.rand(H, W, generator=g) > 0.5).to(gpu))
        graph.replay()
        m = color_grad_maps(s_img, valid=s_valid)
        idx, v = top_indices(m["grad"], M)
        torch.cuda.synchronize()
        assert torch.equal(gm["grad"], m["grad"]) and torch.equal(gm["r_query"], m["r_query"])
        assert torch.equal(gidx, idx) and torch.equal(gv, v)


# ---- SequenceRunner --------------------------------------------------------------------------------------------------
K_RUN, ITERS, RAYS = 5, 6, 1000
KEYS = dict(radius_add_max=0.08, radius_add_min=0.02, radius_query_ratio=2, color_grad_threshold=0.15)


def _run(gpu, graphs, monkeypatch, keys=True, grad_pixels=0, probe=None, draw_identity=False, **opts):
    """K_RUN keyframes of the synthetic stream; keys: the radius keys in cfg["pointcloud"]; grad_pixels: the mapping key
    pixels_based_on_color_grad.  Every add_neural_points call is recorded"""
    import glorie_slam_amd.color_grad as cg
    import glorie_slam_amd.pipeline as P
    orig_cfg = P.synthetic_cfg

    def cfg(*a, **k):
        c = orig_cfg(*a, **k)
        if keys:
            c["pointcloud"].update(KEYS)
        if grad_pixels:
            c["mapping"]["pixels_based_on_color_grad"] = grad_pixels
        return c
    monkeypatch.setattr(P, "synthetic_cfg", cfg)
    if draw_identity:
        monkeypatch.setattr(cg, "draw_candidates", lambda m, n, generator=None: torch.arange(min(m, n)))
    run, c = P.synthetic_runner(gpu, K_RUN, zero_flow_head=True, map_iters=ITERS, map_rays=RAYS)
    monkeypatch.setattr(P, "synthetic_cfg", orig_cfg)
    for key, val in opts.items():
        setattr(run, key, val)
    run.map_graph = graphs
    if probe is not None:
        run.map_probe = lambda k, t: probe(run, k, t)
    calls = []
    add = run.npc.add_neural_points

    def recording_add(ro, rd, d, col, k, i, j, **kw):
        r = kw.get("dynamic_radius")
        calls.append(dict(k=k, i=i.clone(), j=j.clone(), d=d.clone(), is_pts_grad=kw.get("is_pts_grad", False),
                          radius=r.clone() if r is not None else None))
        return add(ro, rd, d, col, k, i, j, **kw)
    run.npc.add_neural_points = recording_add
    video, imgs = c["video"], P.synthetic_images(K_RUN)
    video.poses[:K_RUN] = c["poses"][:K_RUN]
    video.disps[:K_RUN] = c["disps"][:K_RUN]
    video.disps_up[:K_RUN] = torch.nn.functional.interpolate(c["disps"][:K_RUN, None], scale_factor=8, mode="bilinear",
                                                             align_corners=False)[:, 0]
    video.counter.value = K_RUN
    losses = []
    for k in range(K_RUN):
        run.images[k] = imgs[k].to(gpu)
        losses.append(run.map_keyframe(k))
    torch.cuda.synchronize()
    return run, np.array(losses), calls


def _restated(run, f):
    """float64 restatement of frame f's (r_add, r_query) scaled by its view depth"""
    depth = run._keyframe_view(f)[0].cpu().numpy()
    m = color_grad_maps_ref(run.images[f].cpu().numpy(), depth_add=depth, depth_query=depth, **KEYS)
    return m["r_add"], m["r_query"]


WINDOW = dict(keyframe_selection_method="overlap", mapping_window_size=4)


def test_runner_query_radii_follow_each_window_frame(gpu, monkeypatch):
    seen = []

    def probe(run, k, t):
        seen.append((k, list(t["window"]["window"]) if t["window"] is not None else [k], t["window"],
                     t["radius"].clone(), t["pix"].clone()))

    run, losses, calls = _run(gpu, False, monkeypatch, probe=probe, **WINDOW)
    assert run.color_grad is not None and np.isfinite(losses).all()
    assert any(len(w) > 1 for _, w, *_ in seen)
    for k, window, win, radius, pix in seen:
        per = win["per"] if win is not None else RAYS
        for n, f in enumerate(window):
            sl = slice(n * per, (n + 1) * per)
            ii, jj = pix[0, sl].cpu().numpy(), pix[1, sl].cpu().numpy()
            want = _restated(run, f)[1][jj, ii]
            np.testing.assert_allclose(radius[sl].cpu().numpy(), want, rtol=1e-5, atol=1e-9)
    # insertion: the stride grid of every keyframe takes its r_add / 3 * depth
    assert len(calls) == K_RUN and not any(c["is_pts_grad"] for c in calls)
    for c in calls:
        want = _restated(run, c["k"])[0][c["j"].cpu().numpy(), c["i"].cpu().numpy()]
        np.testing.assert_allclose(c["radius"].cpu().numpy(), want, rtol=1e-5, atol=1e-9)


def test_runner_recorded_losses_agree(gpu, monkeypatch):
    _, le, _ = _run(gpu, False, monkeypatch, **WINDOW)
    _, l2, _ = _run(gpu, False, monkeypatch, **WINDOW)
    graph, lg, _ = _run(gpu, True, monkeypatch, **WINDOW)
    assert graph.map_graph_stats["captures"] >= 1
    noise = np.abs(l2 - le).max()
    print("loss noise", noise, "graph-eager", np.abs(lg - le).max())
    assert np.abs(lg - le).max() <= max(4.0 * noise, 3e-2 * np.abs(le).max()), (lg, le, noise)


def test_runner_gradient_anchoring(gpu, monkeypatch):
    from glorie_slam_amd.color_grad import color_grad_maps
    n = 300
    run, losses, calls = _run(gpu, False, monkeypatch, grad_pixels=n, draw_identity=True)
    assert run.pixels_based_on_color_grad == n and np.isfinite(losses).all()
    grad_calls = [c for c in calls if c["is_pts_grad"]]
    assert len(grad_calls) == K_RUN and [c["k"] for c in calls] == [k for k in range(K_RUN) for _ in (0, 1)]
    H, W = run.video.ht, run.video.wd
    for c in grad_calls:
        depth = run._keyframe_view(c["k"])[0]
        grad = color_grad_maps(run.images[c["k"]], valid=depth > 0, outputs=("grad",))["grad"].cpu().numpy()
        cand, _ = top_indices_ref(grad, 5 * n)
        first = cand[:n]
        first = first[depth.cpu().numpy().reshape(-1)[first] > 0]
        assert np.array_equal(c["j"].cpu().numpy() * W + c["i"].cpu().numpy(), first)
        want = _restated(run, c["k"])[0][c["j"].cpu().numpy(), c["i"].cpu().numpy()]
        np.testing.assert_allclose(c["radius"].cpu().numpy(), want, rtol=1e-5, atol=1e-9)


def test_runner_without_the_keys_keeps_the_constant_radius(gpu, monkeypatch):
    seen = []
    run, losses, calls = _run(gpu, False, monkeypatch, keys=False,
                              probe=lambda run, k, t: seen.append(t["radius"].clone()))
    assert run.color_grad is None and run.pixels_based_on_color_grad == 0
    const = 0.5 * (run.npc.radius_add + run.npc.radius_query)
    assert len(calls) == K_RUN and not any(c["is_pts_grad"] for c in calls)
    for c in calls:
        assert torch.equal(c["radius"], torch.full_like(c["d"], const))
    assert seen and all(torch.equal(r, torch.full_like(r, const)) for r in seen)
