"""SequenceRunner with mapping_schedule=True (glorie_slam_amd/pipeline.py; reference src/mapper.py:390-515, :598-638) on the
synthetic runner at the smallest size the runner tests use: rays drawn among the valid pixels only, the iteration counts
and the geometry / colour split of the host rule, the stages' learning rates, what the geometry stage leaves alone, the
gate against its restatement with a planted outlier, "mono" drawing every pixel, pixels_adding; and, with the default
mapping_schedule=False, a run bit-equal to one on a runner built without the argument."""
import functools

import numpy as np
import pytest
import torch

from map_sample_ref import depth_gate_ref

pytestmark = pytest.mark.gpu

H, W, RAYS = 168, 224, 600
K = 4                                           # keyframes 0 .. 3
RATES = {"init": {"geometry": {"decoders_lr": 0.002, "geometry_lr": 0.02, "color_lr": 0.0},
                  "color": {"decoders_lr": 0.004, "geometry_lr": 0.006, "color_lr": 0.007}},
         "stage": {"geometry": {"decoders_lr": 0.001, "geometry_lr": 0.03, "color_lr": 0.0},
                   "color": {"decoders_lr": 0.005, "geometry_lr": 0.0055, "color_lr": 0.0045}}}
MAPPING = dict(RATES, iters_first=10, iters=6, geo_iter_first=3, geo_iter_ratio=0.3, min_iter_ratio=0.95,
               w_geo_loss=1.0, w_color_loss=0.1)
# a keyframe that sees what keyframe 0 saw (few insertions), one whose surface is new (many), one with far pixels
SAME_KEYFRAME, FAR_KEYFRAME, OUTLIER_KEYFRAME = 1, 2, 3


def rect(k):
    """the rectangle of keyframe k without depth: rows, columns"""
    return slice(20 + 10 * k, 70 + 10 * k), slice(30 + 20 * k, 100 + 20 * k)


OUTLIER = (slice(150, 160), slice(0, 60))       # the pixels of OUTLIER_KEYFRAME that lie 50 times too far


def _runner(gpu, monkeypatch, schedule=True, mapping=None, masks=False, pass_argument=True, **attrs):
    """keyframes [0, K) of the synthetic stream as init_state sets them up, with a wrapper that zeroes disps_up in rect(k)
    (and moves keyframe FAR_KEYFRAME away, and plants the outlier); masks: what render_depth needs of the tracker"""
    import glorie_slam_amd.pipeline as P
    orig_cfg, orig_cls = P.synthetic_cfg, P.SequenceRunner

    def cfg(*a, **k):
        c = orig_cfg(*a, **k)
        c["mapping"].update(mapping or {})
        return c
    monkeypatch.setattr(P, "synthetic_cfg", cfg)
    if pass_argument:
        monkeypatch.setattr(P, "SequenceRunner", functools.partial(orig_cls, mapping_schedule=schedule))
    run, c = P.synthetic_runner(gpu, K, map_iters=4, map_rays=RAYS, H=H, W=W)
    monkeypatch.setattr(P, "synthetic_cfg", orig_cfg)
    monkeypatch.setattr(P, "SequenceRunner", orig_cls)
    run.add_stride = 4
    for key, val in attrs.items():
        setattr(run, key, val)
    video, imgs = c["video"], P.synthetic_images(K, H, W)
    inner = run.init_state

    first = {}

    def init_state(k, tstamp=None):
        inner(k, tstamp)
        if k == 0:
            first.update(pose=video.poses[0].clone(), disps_up=video.disps_up[0].clone())
        if k == SAME_KEYFRAME:                                          # the view of keyframe 0 again: little to insert
            video.poses[k] = first["pose"]
            video.disps_up[k] = first["disps_up"]
        if k == FAR_KEYFRAME:
            video.disps_up[k] *= 0.6
        if k == OUTLIER_KEYFRAME:
            video.disps_up[k][OUTLIER] /= 50.0
        video.disps_up[k][rect(k)] = 0
    run.init_state = init_state
    for k in range(K):
        run.init_state(k)
        video.timestamp[k] = k
        run.images[k] = imgs[k].to(gpu)
        if masks:
            video.valid_depth_mask[k] = (video.disps_up[k] > 0)
    video.intrinsics[:K] = c["intrinsics"].to(gpu) / 8.0
    video.counter.value = K
    return run, c


def _expected_schedule(init, pts):
    """the host rule, restated (src/mapper.py:613-629)"""
    if init:
        n, bound = MAPPING["iters_first"], MAPPING["geo_iter_first"]
    else:
        it = MAPPING["iters"]
        n = int(np.clip(int(it * pts / 300), int(MAPPING["min_iter_ratio"] * it), 2 * it))
        bound = int(n * MAPPING["geo_iter_ratio"])
    return n, sum(1 for t in range(n) if t <= bound)


@pytest.fixture(scope="module")
def scheduled(gpu):
    mp = pytest.MonkeyPatch()
    try:
        run, c = _runner(gpu, mp, mapping=MAPPING, keyframe_selection_method="global", mapping_window_size=3)
    finally:
        mp.undo()
    dec, npc = run.decoders, run.npc
    geo_dec0 = [p.detach().clone() for p in dec.geo_decoder.parameters()]
    col_dec0 = [p.detach().clone() for p in dec.color_decoder.parameters()]
    flags0 = [p.requires_grad for p in dec.parameters()]
    probes, added = [], []
    add = npc.add_neural_points

    def counting_add(*a, **kw):
        n = add(*a, **kw)
        added[-1].append(int(n))
        return n
    npc.add_neural_points = counting_add

    def probe(k, t):
        opt = run.last_optimizer
        keep = {key: t[key].clone() for key in ("d", "ii", "jj", "gate", "gate_stats", "seen", "pix")}
        keep.update(k=k, stage=t["stage"], lrs=t["lrs"], group_lrs=[g["lr"] for g in opt.param_groups],
                    window=list(t["window"]["window"]) if t["window"] is not None else [k],
                    per=t["window"]["per"] if t["window"] is not None else RAYS,
                    geo=opt.param_groups[1]["params"][0].detach().clone(),
                    col=opt.param_groups[2]["params"][0].detach().clone(),
                    col_requires_grad=[p.requires_grad for p in dec.color_decoder.parameters()],
                    geo_requires_grad=[p.requires_grad for p in dec.geo_decoder.parameters()])
        probes.append(keep)
    run.map_probe = probe
    for k in range(K):
        added.append([])
        run.map_keyframe(k)
    run.map_probe = None
    return dict(run=run, c=c, probes=probes, added=[sum(a) for a in added], geo_dec0=geo_dec0, col_dec0=col_dec0,
                flags0=flags0)


def test_rays_are_valid_pixels(scheduled):
    run = scheduled["run"]
    multi = False
    for p in scheduled["probes"]:
        assert bool((p["d"] > 0).all())
        assert torch.equal(p["pix"], torch.stack([p["ii"], p["jj"]]))
        n = len(p["window"]) * p["per"]
        assert p["d"].shape == (n,) and p["per"] == RAYS // min(p["k"] + 1, 3) and len(p["window"]) == min(p["k"] + 1, 3)
        multi |= len(p["window"]) > 1
        ii, jj = p["ii"].cpu().numpy(), p["jj"].cpu().numpy()
        for m, f in enumerate(p["window"]):
            sl = slice(m * p["per"], (m + 1) * p["per"])
            rows, cols = rect(f)
            inside = (jj[sl] >= rows.start) & (jj[sl] < rows.stop) & (ii[sl] >= cols.start) & (ii[sl] < cols.stop)
            assert not inside.any()
            depth = run._keyframe_view(f)[0]
            assert torch.equal(p["d"][sl], depth[p["jj"][sl], p["ii"][sl]])
    assert multi


def test_iteration_counts_and_stages(scheduled):
    run, probes, added = scheduled["run"], scheduled["probes"], scheduled["added"]
    expected = [_expected_schedule(k == 0, added[k]) for k in range(K)]
    assert run.schedules == expected and expected[0] == (10, 4)
    it = MAPPING["iters"]
    raw = [int(it * a / 300) for a in added[1:]]
    print("inserted", added, "raw", raw, "schedules", run.schedules)
    assert min(raw) < int(0.95 * it) and max(raw) > 2 * it               # both clip bounds are met
    assert (int(0.95 * it), 2) in expected[1:] and (2 * it, 4) in expected[1:]
    for k in range(K):
        mine = [p for p in probes if p["k"] == k]
        n, n_geo = expected[k]
        assert [p["stage"] for p in mine] == ["geometry"] * n_geo + ["color"] * (n - n_geo)
        for p in mine:
            lrs = RATES["init" if k == 0 else "stage"][p["stage"]]
            assert p["lrs"] == lrs
            assert p["group_lrs"] == [lrs["decoders_lr"], lrs["geometry_lr"], lrs["color_lr"]]
    assert len(run.losses) == K and len(run.windows) == K and all(np.isfinite(l).all() for l in run.losses)


def test_geometry_stage_leaves_colour_alone(scheduled):
    run, probes = scheduled["run"], scheduled["probes"]
    for k in range(K):
        mine = [p for p in probes if p["k"] == k]
        n_geo = run.schedules[k][1]
        assert len(mine) > n_geo                                          # a colour iteration follows
        for t in range(1, n_geo + 1):                                     # the probe of iteration t sees t steps
            assert torch.equal(mine[t]["col"], mine[0]["col"])
            assert not torch.equal(mine[t]["geo"], mine[t - 1]["geo"])
        assert not torch.equal(mine[-1]["col"], mine[n_geo]["col"]) if len(mine) > n_geo + 1 else True
        for p in mine:
            assert not any(p["geo_requires_grad"])                        # fix_geo_decoder
            assert all(p["col_requires_grad"]) == (p["stage"] == "color") and any(p["col_requires_grad"]) == (
                p["stage"] == "color")
    dec = run.decoders
    assert all(torch.equal(a, b) for a, b in zip(scheduled["geo_dec0"], dec.geo_decoder.parameters()))
    assert any(not torch.equal(a, b) for a, b in zip(scheduled["col_dec0"], dec.color_decoder.parameters()))
    assert [p.requires_grad for p in dec.parameters()] == scheduled["flags0"]          # restored


def test_gate_and_the_planted_outlier(scheduled):
    probes = scheduled["probes"]
    hit = 0
    for p in probes:
        keep, stats = depth_gate_ref(p["d"].cpu().numpy())
        assert np.array_equal(p["gate"].cpu().numpy(), keep)
        assert np.array_equal(p["gate_stats"].cpu().numpy().view(np.uint32), stats.view(np.uint32))
        assert bool((p["seen"] <= p["gate"]).all())
        if OUTLIER_KEYFRAME in p["window"]:
            m = p["window"].index(OUTLIER_KEYFRAME)
            sl = slice(m * p["per"], (m + 1) * p["per"])
            ii, jj, gate = p["ii"][sl].cpu().numpy(), p["jj"][sl].cpu().numpy(), p["gate"][sl].cpu().numpy()
            far = (jj >= OUTLIER[0].start) & (jj < OUTLIER[0].stop) & (ii >= OUTLIER[1].start) & (ii < OUTLIER[1].stop)
            hit += int(far.sum())
            assert not gate[far].any() and gate[~far].all()
    assert hit > 0


def test_mono_draws_every_pixel(gpu, monkeypatch):
    import glorie_slam_amd.pipeline as P
    modes = []
    orig = P.ValidIndex

    def spy(table, mode="depth"):
        modes.append(mode)
        return orig(table, mode)
    monkeypatch.setattr(P, "ValidIndex", spy)
    run, c = _runner(gpu, monkeypatch, mapping=dict(MAPPING, render_depth="mono", iters_first=3, geo_iter_first=0),
                     masks=True)
    inside = []

    def probe(k, t):
        rows, cols = rect(k)
        ii, jj = t["ii"], t["jj"]
        inside.append(int(((jj >= rows.start) & (jj < rows.stop) & (ii >= cols.start) & (ii < cols.stop)).sum()))
        assert bool((t["d"] > 0).all())                                   # the aligned prior has a depth everywhere
    run.map_probe = probe
    run.map_keyframe(0)
    assert run.render_depth == "mono" and modes == ["all"] and run.schedules == [(3, 1)]
    area = (50 * 70) / (H * W)
    assert all(0.5 * area * RAYS < n < 1.5 * area * RAYS for n in inside)  # the tracker's hole is drawn like any region


def test_pixels_adding_inserts_valid_pixels(gpu, monkeypatch):
    run, c = _runner(gpu, monkeypatch, mapping=dict(MAPPING, pixels_adding=500, iters_first=1))
    calls = []
    add = run.npc.add_neural_points

    def spy(ro, rd, d, col, k, ii, jj, **kw):
        calls.append((d.clone(), ii.clone(), jj.clone(), kw.get("dynamic_radius")))
        return add(ro, rd, d, col, k, ii, jj, **kw)
    run.npc.add_neural_points = spy
    run.map_keyframe(0)
    (d, ii, jj, radius), = calls
    assert d.shape == (500,) and bool((d > 0).all()) and radius is not None and radius.shape == (500,)
    rows, cols = rect(0)
    assert not bool(((jj >= rows.start) & (jj < rows.stop) & (ii >= cols.start) & (ii < cols.stop)).any())
    assert torch.equal(d, run._keyframe_view(0)[0][jj, ii]) and len(torch.unique(jj * W + ii)) > 400
    assert run.npc.pts_num() > 0 and run.schedules == [(1, 1)]
    # without the key the stride grid is used
    run2, _ = _runner(gpu, monkeypatch, mapping=dict(MAPPING, iters_first=1))
    calls.clear()
    add2 = run2.npc.add_neural_points
    run2.npc.add_neural_points = lambda ro, rd, d, col, k, ii, jj, **kw: (calls.append(d.shape[0]),
                                                                             add2(ro, rd, d, col, k, ii, jj, **kw))[1]
    run2.map_keyframe(0)
    assert calls == [(H // 4) * (W // 4)]


def test_default_off_is_the_runner_without_the_argument(gpu, monkeypatch):
    runs = []
    for pass_argument in (False, True):
        run, _ = _runner(gpu, monkeypatch, schedule=False, pass_argument=pass_argument, mapping=MAPPING,
                         keyframe_selection_method="global", mapping_window_size=3)
        for k in range(3):
            run.map_keyframe(k)
        assert run.mapping_schedule is False and run.schedules == []
        runs.append(run)
    a, b = runs
    assert a.losses == b.losses and a.windows == b.windows and len(a.losses) == 3
    assert torch.equal(a.npc.geo_feats, b.npc.geo_feats) and torch.equal(a.npc.col_feats, b.npc.col_feats)
    assert torch.equal(a.npc.cloud_pos(), b.npc.cloud_pos())
    for p, q in zip(a.decoders.parameters(), b.decoders.parameters()):
        assert torch.equal(p, q)
