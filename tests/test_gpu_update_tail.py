"""The fused tail of the update operator, bit for bit against the launches it replaces: glorie_heads_finish (conv_stencil +
segment_mean + the target sum of update_bookkeeping), glorie_eta_finish (conv3x3_small of the eta head + the eta half of
update_bookkeeping), and FactorGraph.update with FusedUpdate.fuse_tail off and on."""
import numpy as np
import pytest
import torch

import glorie_slam_amd.synth as synth
from glorie_slam_amd import _lib as L, update_ops as U

pytestmark = pytest.mark.gpu


def _cl_map(gen, n, c, h, w, dev):
    """seeded fp16 channels-last map [n,c,h,w], as the step's convolutions leave them"""
    x = torch.randn((n, h, w, c), generator=gen, dtype=torch.float32).half()
    return x.to(dev).permute(0, 3, 1, 2)


def _bookkeeping(coords1, delta, target, eta, frames, table, damping_ba, G, HW, ep, age):
    n_target = coords1.numel() if coords1 is not None else 0
    L.check(L.load().glorie_update_bookkeeping(L.ptr(coords1), L.ptr(delta), L.ptr(target), n_target, L.ptr(eta),
                                               L.ptr(frames), L.ptr(table), L.ptr(damping_ba), G, HW, ep, L.ptr(age),
                                               age.numel() if age is not None else 0, L.stream_ptr()),
            "glorie_update_bookkeeping")


HEADS_CASES = [
    # (h, w, ix, with coords1 / target and the weights' own buffer)
    (5, 7, [0, 0, 1, 2, 2], True),            # 35 pixels per map: 256-element tiles straddle maps
    (3, 5, [0, 0, 1, 2, 2], False),           # delta and weight only
    (12, 20, [1, 0, 0, 2, 0, 1, 0], True),    # unsorted: a group of one, a group of four
]


@pytest.mark.parametrize("h,w,ix,book", HEADS_CASES)
def test_heads_finish_matches_three_launches(gpu, h, w, ix, book):
    gen = torch.Generator().manual_seed(1234 + h)
    n, G, K, groups = len(ix), max(ix) + 1, 2, 2
    acts = (U.ACT_NONE, U.ACT_SIGMOID)
    rows = torch.randn((groups * 9 * K, n * h * w), generator=gen).to(gpu)
    bias = torch.randn(groups * K, generator=gen).to(gpu)
    x = _cl_map(gen, n, 128, h, w, gpu)
    ix_t = torch.tensor(ix, dtype=torch.int64, device=gpu)
    coords1 = (torch.rand((1, n, h, w, K), generator=gen) * 30).to(gpu) if book else None
    new_empty = lambda: torch.full((1, n, h, w, K), float("nan"), device=gpu)

    wo_old = new_empty() if book else None
    dw_old = U.conv_stencil(rows, bias, n, h, w, groups, K, acts, out_last=wo_old)
    agg_old = U.segment_mean(x, ix_t, G)
    if book:
        target_old = new_empty()
        _bookkeeping(coords1, dw_old[0], target_old, None, None, None, None, 0, h * w, 0.0, None)

    wo = new_empty() if book else None
    target = new_empty() if book else None
    dw, agg = U.heads_finish(rows, bias, n, h, w, groups, K, acts, x, ix_t, G, out_last=wo, coords1=coords1, target=target)
    torch.cuda.synchronize()
    assert torch.equal(agg, agg_old)
    assert agg.is_contiguous(memory_format=torch.channels_last)
    assert torch.equal(dw[0], dw_old[0])
    if book:
        assert torch.equal(wo, wo_old)
        assert torch.equal(target, target_old)
        assert torch.isfinite(target).all()
    else:
        assert torch.equal(dw[1], dw_old[1])


def test_heads_finish_argument_checks(gpu):
    gen = torch.Generator().manual_seed(5)
    n, h, w = 2, 3, 5
    rows = torch.randn((36, n * h * w), generator=gen).to(gpu)
    bias = torch.zeros(4, device=gpu)
    x = _cl_map(gen, n, 128, h, w, gpu)
    ix = torch.tensor([0, 1], dtype=torch.int64, device=gpu)
    acts = (U.ACT_NONE, U.ACT_SIGMOID)
    c1 = torch.zeros((1, n, h, w, 2), device=gpu)
    with pytest.raises(RuntimeError):
        U.heads_finish(rows, bias, n, h, w, 2, 2, acts, x, ix, 2, coords1=c1)                 # target missing
    with pytest.raises(RuntimeError):
        U.heads_finish(rows, bias, n, h, w, 2, 2, acts, x, ix, 2, coords1=c1, target=c1[:, :1])
    with pytest.raises(RuntimeError):
        U.heads_finish(rows[:, :-1], bias, n, h, w, 2, 2, acts, x, ix, 2)
    with pytest.raises(RuntimeError):
        U.heads_finish(rows, bias, n, h, w, 2, 2, acts, x, ix.int(), 2)


# rows_per_block 0 = the library's choice (2): 5 rows -> blocks of 2, 2, 1; 1 and 3: every row / every third row a block
ETA_CASES = [(5, 7, 0, 5), (3, 5, 0, 700), (1, 9, 0, 1000), (12, 20, 0, 300), (5, 7, 1, 0), (12, 20, 3, 5), (3, 5, 8, 5)]


@pytest.mark.parametrize("h,w,rpb,n_edges", ETA_CASES)
def test_eta_finish_matches_conv3x3_small_and_bookkeeping(gpu, h, w, rpb, n_edges):
    """n_edges: fewer than one workgroup (5), more than one (300, 700), more than the launch has threads (1000 on 3 maps of
    one row: 3 workgroups), none.  A map of one row has no neighbours above or below; the maps hold different values, so a
    row block that read its halo across a map boundary would not reproduce the per-map convolution."""
    gen = torch.Generator().manual_seed(99 + h * w + rpb)
    G, B, ep = 3, 8, 1e-7
    a2 = _cl_map(gen, G, 128, h, w, gpu)
    wgt = (torch.randn((1, 128, 3, 3), generator=gen) * 0.05).to(gpu)
    wp = U.pack_conv3x3_small([wgt])
    bias = torch.randn(1, generator=gen).to(gpu)
    frames = torch.tensor([4, 1, 6], dtype=torch.int64, device=gpu)
    table0 = torch.rand((B, h, w), generator=gen).to(gpu)
    age0 = torch.randint(0, 50, (n_edges,), generator=gen, dtype=torch.int64).to(gpu)

    eta_old = U.conv3x3_small(a2, wp, bias, 1, (U.ACT_SOFTPLUS,), scale=0.01)
    table_old, age_old = table0.clone(), age0.clone()
    ba_old = torch.full((G, h, w), float("nan"), device=gpu)
    _bookkeeping(None, None, None, eta_old, frames, table_old, ba_old, G, h * w, ep, age_old if n_edges else None)

    table, age = table0.clone(), age0.clone()
    ba = torch.full((G, h, w), float("nan"), device=gpu)
    eta = U.eta_finish(a2, wp, bias, frames, table, ba, ep, age if n_edges else None, scale=0.01, rows_per_block=rpb)
    torch.cuda.synchronize()
    assert eta.shape == eta_old.shape
    assert torch.equal(eta, eta_old)
    assert torch.equal(table, table_old)                          # the rows `frames` names, and no other
    assert torch.equal(table[[0, 2, 3, 5, 7]], table0[[0, 2, 3, 5, 7]])
    assert torch.equal(ba, ba_old) and torch.isfinite(ba).all()
    assert torch.equal(age, age_old) and torch.equal(age, age0 + 1)


def test_eta_finish_ages_only_and_unsupported_width(gpu):
    """G = 0 with ages is a valid call (as for glorie_update_bookkeeping); a map too wide for three rows of taps in LDS
    launches nothing and reports it"""
    lib = L.load()
    age = torch.arange(600, dtype=torch.int64, device=gpu)
    L.check(lib.glorie_eta_finish(None, 128, None, None, 0.01, None, None, None, None, 1e-7, L.ptr(age), 600, 0, 0, 4, 4,
                                  L.stream_ptr()), "glorie_eta_finish")
    torch.cuda.synchronize()
    assert torch.equal(age, torch.arange(600, dtype=torch.int64, device=gpu) + 1)
    gen = torch.Generator().manual_seed(3)
    h, w = 3, 640                                                  # 3 * 640 * 9 floats > 64 KB
    a2 = _cl_map(gen, 1, 128, h, w, gpu)
    wp = U.pack_conv3x3_small([torch.zeros((1, 128, 3, 3), device=gpu)])
    frames = torch.zeros(1, dtype=torch.int64, device=gpu)
    table, ba = torch.zeros((1, h, w), device=gpu), torch.zeros((1, h, w), device=gpu)
    assert U.eta_finish(a2, wp, None, frames, table, ba, 1e-7, strict=False) is None
    with pytest.raises(L.GlorieError):
        U.eta_finish(a2, wp, None, frames, table, ba, 1e-7)


def _cfg(dev, H, W, buffer):
    return {"cam": {"H_out": H, "W_out": W},
            "tracking": {"buffer": buffer, "backend": {"BA_type": "DSPO"}, "mono_thres": 0.1,
                         "multiview_filter": {"thresh": 0.25, "visible_num": 2}, "store_images": False},
            "device": str(dev), "setting": "t", "scene": "s", "data": {"output": "/tmp"}}


def _run_steps(dev, fuse_tail, use_graphs, K=4, h=16, w=24, steps=4):
    """`steps` updates with alternating stages on the 4-keyframe graph; the state after every step"""
    from glorie_slam_amd.depth_video import DepthVideo
    from glorie_slam_amd.droid_net import UpdateModule
    from glorie_slam_amd.factor_graph import FactorGraph
    g = synth.keyframe_graph(K=K, h=h, w=w, radius=3)
    fmaps, nets, inps = synth.feature_maps(K, h, w)
    video = DepthVideo(_cfg(dev, 8 * h, 8 * w, K))
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)
    video.poses[:K], video.disps[:K] = t(g["poses"][:K]), t(g["disps"][:K])
    video.intrinsics[:] = t(g["intrinsics"][0])
    video.fmaps[:K], video.nets[:K], video.inps[:K] = t(fmaps), t(nets), t(inps)
    video.counter.value = K
    rng = np.random.default_rng(0)
    mono = g["disps"][:K] * rng.uniform(0.7, 1.4, (K, 1, 1)) + rng.uniform(-0.03, 0.03, (K, 1, 1))
    video.mono_disps[:K] = t(mono.astype(np.float32))
    torch.manual_seed(43)
    net = UpdateModule().to(dev).eval()
    graph = FactorGraph(video, net, device=str(dev), use_graphs=use_graphs)
    assert graph.fast_update.fuse_tail and graph.fast_update.fuse_heads          # the default
    graph.fast_update.fuse_tail = fuse_tail
    graph.add_factors(torch.as_tensor(g["ii"], device=dev), torch.as_tensor(g["jj"], device=dev))
    states = []
    for i in range(steps):
        graph.update(t0=1, t1=K, itrs=2, opt_type="pose_depth" if i % 2 == 0 else "depth_scale")
        torch.cuda.synchronize()
        states.append({"net": graph.net.float().clone(), "target": graph.target.clone(), "weight": graph.weight.clone(),
                       "damping": graph.damping.clone(), "poses": video.poses.clone(), "disps": video.disps.clone(),
                       "disps_up": video.disps_up.clone(), "age": graph.age.clone()})
    return states, graph


@pytest.mark.parametrize("use_graphs", [False, True])
def test_update_steps_equal_with_and_without_fused_tail(gpu, use_graphs):
    off, _ = _run_steps(gpu, False, use_graphs)
    on, graph = _run_steps(gpu, True, use_graphs)
    if use_graphs:
        assert graph.stats["captures"] == 2 and graph.stats["replays"] == 2      # both stages recorded and replayed
    for step, (a, b) in enumerate(zip(off, on)):
        for name in ("net", "target", "weight", "damping", "poses", "disps", "disps_up", "age"):
            assert torch.isfinite(a[name].float()).all(), (step, name)
            assert torch.equal(a[name], b[name]), (step, name)
    assert int(on[-1]["age"].min()) == len(on)                                   # incremented once per step


def test_fused_tail_takes_over_the_bookkeeping(gpu, monkeypatch):
    """with fuse_tail the eager step calls the two new entry points once each and none of glorie_conv_stencil,
    glorie_segment_mean, glorie_conv3x3_small, glorie_update_bookkeeping; without it, those four (five launches:
    glorie_conv3x3_small is two) and neither new one - three launches fewer.  The library keeps no launch counter: the calls
    of its entry points are counted here."""
    counts = {}
    names = ("glorie_heads_finish", "glorie_eta_finish", "glorie_conv_stencil", "glorie_segment_mean",
             "glorie_conv3x3_small", "glorie_update_bookkeeping")

    class Counting:
        def __init__(self, lib):
            self._lib = lib

        def __getattr__(self, name):
            fn = getattr(self._lib, name)
            if name in names:
                counts[name] = counts.get(name, 0) + 1
            return fn

    lib = L.load()
    monkeypatch.setattr(L, "load", lambda: Counting(lib))
    per_mode = {}
    for fuse in (False, True):
        counts.clear()
        _run_steps(gpu, fuse, False, steps=1)
        per_mode[fuse] = dict(counts)
    assert per_mode[True] == {"glorie_heads_finish": 1, "glorie_eta_finish": 1}
    assert per_mode[False] == {"glorie_conv_stencil": 1, "glorie_segment_mean": 1, "glorie_conv3x3_small": 1,
                               "glorie_update_bookkeeping": 1}
