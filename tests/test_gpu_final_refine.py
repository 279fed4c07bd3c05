"""SequenceRunner.final_refine (reference: src/mapper.py:816-855) on the synthetic stream: 8 keyframes mapped as in
test_gpu_keyframe_select._run (6 iterations of 1000 rays each), then the refinement.  The windows follow the host rule,
an iteration's rays are the per-frame composition's, the decoders keep their bits, the features move only where Adam saw
a gradient, the mapper's bookkeeping stays, and the map fits the keyframes better afterwards."""
import math

import numpy as np
import pytest
import torch

from window_rays_ref import EPS32, rays_d_f64

pytestmark = pytest.mark.gpu


def _fixed_batch(run, gpu, n=4096, seed=11):
    """n pixels over all mapped keyframes (frame-major), drawn once from a seeded generator"""
    from glorie_slam_amd.window_rays import WindowTable
    frames = [f for f in range(run.mapped) if f not in run.skipped]
    per = n // len(frames)
    g = torch.Generator(device="cpu").manual_seed(seed)
    ii = torch.randint(0, run.video.wd, (per * len(frames),), generator=g).to(gpu)
    jj = torch.randint(0, run.video.ht, (per * len(frames),), generator=g).to(gpu)
    views = [run._keyframe_view(f) for f in frames]
    table = WindowTable([v[0] for v in views], [run.images[f] for f in frames], torch.stack([v[1] for v in views]))
    return table, ii, jj, per


def _fixed_loss(run, batch):
    """the shared loss of the mapping iterations on the fixed batch, without grad, on the cloud's current features"""
    from glorie_slam_amd.window_rays import window_rays
    table, ii, jj, per = batch
    ren, npc = run.renderer, run.npc
    with torch.no_grad():
        ro, rd, d, col, radius = window_rays(table, ii, jj, per, ren.fx, ren.fy, ren.cx, ren.cy,
                                             const_radius=0.5 * (npc.radius_add + npc.radius_query))
        loss, _, _, seen = run._mapping_loss(ro, rd, d, col, radius, npc.geo_feats, npc.col_feats)
    return float(loss), float(seen.sum())


@pytest.fixture(scope="module")
def refined(gpu):
    from test_gpu_keyframe_select import K_RUN, _run
    run, _ = _run(gpu, False)
    run.mapped = K_RUN
    npc, dec = run.npc, run.decoders
    book = dict(losses=list(run.losses), windows=[list(w) for w in run.windows], frustum=list(run.frustum_counts),
                graph=dict(run.map_graph_stats), mapped=run.mapped, n_timed=len(run.timing["map_iter_ms"]))
    dec_before = [(p.detach().clone(), p.requires_grad) for p in dec.parameters()]
    feats0 = (npc.geo_feats.detach().clone(), npc.col_feats.detach().clone())
    batch = _fixed_batch(run, gpu)
    loss_before = _fixed_loss(run, batch)
    seen = {"iters": [], "first": {}, "feats_before_last_pass": None}

    def probe(k, t):
        o = t["refine"]
        seen["iters"].append((o, k, float(t["loss"])))
        if o not in seen["first"]:
            seen["first"][o] = {key: (t[key].clone() if torch.is_tensor(t[key]) else t[key])
                                for key in ("ro", "rd", "d", "gt_col", "radius", "pix", "window", "warp", "frustum")}
            if o == 1:
                seen["feats_before_last_pass"] = (npc.geo_feats.detach().clone(), npc.col_feats.detach().clone())
    run.map_probe = probe
    res = run.final_refine(outer_iters=2)
    run.map_probe = None
    loss_after = _fixed_loss(run, batch)
    return dict(run=run, res=res, book=book, dec_before=dec_before, feats0=feats0, seen=seen, loss_before=loss_before,
                loss_after=loss_after)


def test_windows_and_bookkeeping(refined):
    from test_gpu_keyframe_select import ITERS, K_RUN, RAYS
    run, res, book = refined["run"], refined["res"], refined["book"]
    assert len(run.refine_windows) == 2 and res["window_sizes"] == [K_RUN - 2] * 2
    for w in run.refine_windows:
        assert w[-1] == K_RUN - 1 and len(set(w)) == len(w) == min(K_RUN - 1, K_RUN - 3) + 1
        assert set(w[:-1]) <= set(range(K_RUN - 1))
    assert res["per"] == RAYS // 7 == 1000 // 7
    assert res["pix_warping"] is False and res["ms_per_iter"] > 0
    # two passes of 2 * map_iters iterations, each announced to the probe with its pass index and the last window frame
    its = refined["seen"]["iters"]
    assert [o for o, _, _ in its] == [0] * (2 * ITERS) + [1] * (2 * ITERS) and all(k == K_RUN - 1 for _, k, _ in its)
    assert len(run.refine_losses) == 2 and res["losses"] == run.refine_losses
    for o, (first, last) in enumerate(run.refine_losses):
        assert math.isfinite(first) and math.isfinite(last)
        mine = [l for p, _, l in its if p == o]
        assert first == mine[0] and last == mine[-1]
    # the mapper's own records are where they were
    assert run.losses == book["losses"] and run.windows == book["windows"] and run.frustum_counts == book["frustum"]
    assert run.map_graph_stats == book["graph"] and run.mapped == book["mapped"]
    assert len(run.timing["map_iter_ms"]) == book["n_timed"] and run._render_views is None
    assert run.renderer.assume_depth is False


def test_iteration_rays_are_the_per_frame_composition(refined):
    run = refined["run"]
    ren = run.renderer
    for o, t in refined["seen"]["first"].items():
        win, pix = t["window"], t["pix"]
        per = win["per"]
        assert win["window"] == run.refine_windows[o] and t["d"].shape[0] == per * len(win["window"])
        assert t["warp"] is None and t["frustum"] is None
        for n, f in enumerate(win["window"]):
            sl = slice(n * per, (n + 1) * per)
            ro, rd, d, col, ii, jj, radius = run._keyframe_rays(f, view=win["views"][f], pix=(pix[0, sl], pix[1, sl]))
            assert torch.equal(t["ro"][sl], ro) and torch.equal(t["d"][sl], d) and torch.equal(t["gt_col"][sl], col)
            assert torch.equal(t["radius"][sl], radius)
            _, S = rays_d_f64(win["views"][f][1].cpu().numpy()[None], ii.cpu().numpy(), jj.cpu().numpy(), per, ren.fx,
                              ren.fy, ren.cx, ren.cy)
            err = (t["rd"][sl].double() - rd.double()).abs().cpu().numpy()
            assert (err <= 5 * EPS32 * S).all(), (o, f, float((err / S).max()) / EPS32)


def test_decoders_frozen_features_trained(refined):
    run = refined["run"]
    npc = run.npc
    for p, (before, req) in zip(run.decoders.parameters(), refined["dec_before"]):
        assert torch.equal(p.detach().view(torch.int32), before.view(torch.int32)) and p.requires_grad == req
    geo0, col0 = refined["feats0"]
    assert npc.geo_feats.shape == geo0.shape and npc.col_feats.shape == col0.shape       # no point was inserted
    assert int((npc.geo_feats != geo0).any(1).sum()) > 0 and int((npc.col_feats != col0).any(1).sum()) > 0
    # rows Adam never saw a gradient for in the last pass (both moments zero) kept their bits through it
    opt = run.last_optimizer
    assert [len(g["params"]) for g in opt.param_groups] == [1, 1]                        # [geo], [col_f]: no decoder group
    for group, now, before in zip(opt.param_groups, (npc.geo_feats, npc.col_feats), refined["seen"]["feats_before_last_pass"]):
        st = opt.state[id(group["params"][0])]
        idle = (st["m"] == 0).all(1) & (st["v"] == 0).all(1)
        print("rows", idle.numel(), "idle", int(idle.sum()))
        assert bool(idle.any()) and not bool(idle.all())
        assert torch.equal(now[idle].view(torch.int32), before[idle].view(torch.int32))
        assert bool((now[~idle] != before[~idle]).any())


def test_the_map_fits_the_keyframes_better(refined):
    (before, n0), (after, n1) = refined["loss_before"], refined["loss_after"]
    print("fixed-batch loss before", before, "after", after, "seen rays", n0, n1)
    assert math.isfinite(before) and math.isfinite(after) and n0 > 0
    assert after < before


def test_save_final_pcl(refined, tmp_path):
    from glorie_slam_amd.generate_mesh import read_ply
    run = refined["run"]
    geo = run.npc.geo_feats.detach().clone()
    res = run.final_refine(outer_iters=0, save_final_pcl=True, output=str(tmp_path))
    assert res["window_sizes"] == [] and torch.equal(run.npc.geo_feats, geo)
    # the cloud holds N_add neural points per anchored input point: npc_cloud.npy has pts_num() rows, final_point_cloud.npy
    # one row per input point (the arrays the reference stacks, mapper.py:839-842)
    n, n_in = run.npc.pts_num(), run.npc.input_pos().shape[0]
    cloud = np.load(tmp_path / "final_point_cloud.npy")
    pos = np.load(tmp_path / "npc_cloud.npy")
    assert n_in > 0 and n == run.npc.N_add * n_in
    assert cloud.shape == (n_in, 6) and pos.shape == (n, 3)
    np.testing.assert_array_equal(pos, run.npc.cloud_pos().cpu().numpy())
    np.testing.assert_array_equal(cloud[:, :3], run.npc.input_pos().cpu().numpy())
    np.testing.assert_array_equal(cloud[:, 3:], run.npc.input_rgb().cpu().numpy())
    assert cloud[:, 3:].max() > 1.5                                  # the cloud stores colours in 0..255
    vertices, faces, colors = read_ply(str(tmp_path / "final_point_cloud.ply"))
    assert faces.shape == (0, 3)
    np.testing.assert_array_equal(vertices, cloud[:, :3].astype(np.float32))
    # (input_rgb / 255 goes through write_ply's x 255 and rounding: a colour at a rounding tie may land on its neighbour)
    assert np.abs(colors.astype(np.int64) - np.rint(cloud[:, 3:].astype(np.float64)).astype(np.int64)).max() <= 1


def test_run_gains_only_the_keyword(refined, monkeypatch):
    run = refined["run"]
    calls = []
    monkeypatch.setattr(run, "final_refine", lambda *a, **k: calls.append((a, k)))
    monkeypatch.setattr(run.backend, "dense_ba", lambda steps: (0, 0))
    monkeypatch.setattr(run, "map_pending", lambda: None)
    intr = torch.tensor([320.0, 320.0, 319.5, 239.5])
    summary = run.run(iter(()), intr)
    assert calls == []
    assert sorted(summary) == ["final_ba_edges", "keyframes", "losses", "mapped", "points", "timing"]
    assert run.run(iter(()), intr, final_refine=True).keys() == summary.keys()
    assert calls == [((), {})]


def test_errors_before_any_gpu_work(gpu):
    from glorie_slam_amd.pipeline import synthetic_runner
    run, _ = synthetic_runner(gpu, 4, map_iters=2)
    state = run.gen.get_state()
    with pytest.raises(ValueError):
        run.final_refine()                                           # nothing mapped
    run.mapped, run.video.counter.value = 70, 70
    with pytest.raises(ValueError):
        run.final_refine(pix_warping=True)                           # 68 window frames
    assert torch.equal(run.gen.get_state(), state) and run.refine_losses == []
    assert all(p.requires_grad for p in run.decoders.parameters())


def test_proxy_depth_radius_maps_and_skipped_frames(gpu, monkeypatch):
    """render_depth "proxy", bind_npc_with_pose and colour-gradient radii: the iteration's radii are every window
    frame's own query map at the drawn pixels; a skipped keyframe is in no window"""
    from glorie_slam_amd import color_grad as CG
    from test_gpu_deform import RAYS, _runner
    firsts = []

    def probe(run, k, t):
        if "refine" in t and not any(o == t["refine"] for o, *_ in firsts):
            firsts.append((t["refine"], t["window"], t["pix"].clone(), t["radius"].clone(), t["d"].clone()))

    K = 5
    run, c = _runner(gpu, monkeypatch, K, few_valid=(1,), probe=probe)
    run.color_grad = dict(color_grad_threshold=CG.COLOR_GRAD_THRESHOLD, radius_add_max=CG.RADIUS_ADD_MAX,
                          radius_add_min=CG.RADIUS_ADD_MIN, radius_query_ratio=CG.RADIUS_QUERY_RATIO)
    for k in range(K + 1):
        run.map_keyframe(k)
        run.mapped += 1
    assert run.skipped == [1]
    c["video"].set_dirty(0, K + 1)                                   # the refinement deforms the cloud first
    calls = run.deform_stats["calls"]
    res = run.final_refine(outer_iters=2, iters=2)
    assert run.deform_stats["calls"] == calls + 1 and run._render_views is None
    assert res["per"] == RAYS // (K - 1 + 1) and res["window_sizes"] == [K - 1] * 2     # 3 of {0, 2, 3, 4}, then 5
    assert len(firsts) == 2
    for w in run.refine_windows:
        assert 1 not in w and w[-1] == K and len(set(w)) == len(w)
    for o, win, pix, radius, d in firsts:
        per = win["per"]
        for n, f in enumerate(win["window"]):
            sl = slice(n * per, (n + 1) * per)
            rmap = run._radius_maps(f, win["views"][f], add=False)[1]
            assert torch.equal(radius[sl], rmap[pix[1, sl], pix[0, sl]])
            assert torch.equal(d[sl], win["views"][f][0][pix[1, sl], pix[0, sl]])
    assert all(math.isfinite(x) for pair in run.refine_losses for x in pair)


def test_pixel_warping_in_the_refinement(gpu):
    from test_gpu_keyframe_select import K_RUN, _run
    values = []
    run, _ = _run(gpu, False, pix_warping=True, mapping_window_size=5)
    run.mapped = K_RUN
    run.map_probe = lambda k, t: values.append(t["warp"]["value"].clone()) if ("refine" in t and t["warp"]) else None
    n_warp = len(run.warp_losses)
    res = run.final_refine(outer_iters=1, iters=3, pix_warping=True)
    assert res["pix_warping"] is True and len(values) == 3
    assert all(math.isfinite(float(v)) for v in values)
    assert len(run.warp_losses) == n_warp
    # the runner's setting is the default
    assert run.final_refine(outer_iters=1, iters=1)["pix_warping"] is True
    assert run.final_refine(outer_iters=1, iters=1, pix_warping=False)["pix_warping"] is False
