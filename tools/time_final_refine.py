"""Cost of the final refinement's ray gather (glorie_slam_amd/window_rays.py) against the per-frame composition
(SequenceRunner._window_rays), of one refinement iteration with either, and of one whole SequenceRunner.final_refine.

    python tools/time_final_refine.py [--reps 30]

  gather:     window_rays against _window_rays in the same process at M = 8, 64 and 200 window frames of 640x480 with
              per = 1000 // (M + 1) rays of each: the two variants alternate call by call, events around every call, the
              median over `reps` (what the stream took, host-side launch gaps of the composition included) and the wall
              time of `reps` back-to-back calls per variant
  iteration:  one refinement iteration (gather, forward, loss, backward, FeatureAdam on the two feature tables, decoders
              frozen) on the cloud of 8 mapped keyframes of the synthetic stream, the window filled up to M slots with
              those keyframes again (an iteration's cost follows its ray count, not which frames the rays come from):
              the iteration with either gather, the gather alone, and the iteration with the decoders' weight
              gradients formed (and dropped) as the mapping iterations form them, alternating, events, medians
  refine:     final_refine() with its defaults on that runner (5 passes of 40 iterations, 6-frame windows), wall time
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SIZES = (8, 64, 200)
H, W, RAYS = 480, 640, 1000


def _interleaved(variants, reps, warmup=3):
    """{name: fn} -> {name: median ms}: the variants alternate call by call, an event pair around every call"""
    for _ in range(warmup):
        for fn in variants.values():
            fn()
    torch.cuda.synchronize()
    pairs = {name: [] for name in variants}
    for _ in range(reps):
        for name, fn in variants.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            pairs[name].append((e0, e1))
    torch.cuda.synchronize()
    return {name: statistics.median(a.elapsed_time(b) for a, b in ev) for name, ev in pairs.items()}


def _wall(fn, reps):
    fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0) / reps


def _mapped_runner(dev):
    """the synthetic runner with its 8 keyframes mapped (20 iterations of 1000 rays each)"""
    import glorie_slam_amd.pipeline as P
    run, c = P.synthetic_runner(dev, 8, map_iters=20, map_rays=RAYS)
    imgs = P.synthetic_images(8)
    for k in range(8):
        run.init_state(k)
        c["video"].timestamp[k] = k
        run.images[k] = imgs[k].to(dev)
    c["video"].counter.value = 8
    for k in range(8):
        run.map_keyframe(k)
        run.mapped += 1
    return run


def _window(run, M, dev, seed=0):
    """a window of M slots over the runner's keyframes (slot s shows keyframe s % 8 under the id s) in both forms: the
    WindowTable of window_rays and the dict of _window_rays, with one draw of per = 1000 // (M + 1) pixels a slot"""
    from glorie_slam_amd.window_rays import WindowTable
    per = max(1, RAYS // (M + 1))
    base = {f: run._keyframe_view(f) for f in range(8)}
    views = {s: base[s % 8] for s in range(M)}
    for s in range(M):
        run.images[s] = run.images[s % 8]
    table = WindowTable([views[s][0] for s in range(M)], [run.images[s] for s in range(M)],
                        torch.stack([views[s][1] for s in range(M)]))
    g = torch.Generator().manual_seed(seed)
    pix = torch.stack([torch.randint(0, W, (M * per,), generator=g), torch.randint(0, H, (M * per,), generator=g)]).to(dev)
    return table, {"window": list(range(M)), "views": views, "per": per}, pix, per


def time_gather(run, dev, reps):
    from glorie_slam_amd.window_rays import window_rays
    ren, npc = run.renderer, run.npc
    const_r = 0.5 * (npc.radius_add + npc.radius_query)
    out = {}
    for M in SIZES:
        table, win, pix, per = _window(run, M, dev)
        one = lambda: window_rays(table, pix[0], pix[1], per, ren.fx, ren.fy, ren.cx, ren.cy, const_radius=const_r)
        comp = lambda: run._window_rays(win, pix)
        a, b = one(), comp()
        assert all(torch.equal(x, y) for x, y in zip((a[0], a[2], a[3], a[4]), (b[0], b[2], b[3], b[4])))
        ev = _interleaved({"window_rays": one, "per_frame": comp}, reps)
        out[f"M{M}"] = {"per": per, "rays": M * per, "window_rays_ms": round(ev["window_rays"], 4),
                        "per_frame_ms": round(ev["per_frame"], 3),
                        "window_rays_wall_ms": round(_wall(one, reps), 4), "per_frame_wall_ms": round(_wall(comp, reps), 3)}
        print(f"gather M={M}", out[f"M{M}"], flush=True)
    return out


def time_iteration(run, dev, reps):
    from glorie_slam_amd.render_train import FeatureAdam
    from glorie_slam_amd.window_rays import window_rays
    ren, npc, dec = run.renderer, run.npc, run.decoders
    const_r = 0.5 * (npc.radius_add + npc.radius_query)
    out = {}
    params = list(dec.parameters())
    req = [p.requires_grad for p in params]
    dec.train()
    ren.assume_depth = True               # the synthetic views carry a depth at every pixel
    try:
        for M in SIZES:
            table, win, pix, per = _window(run, M, dev)
            geo = npc.geo_feats.detach().clone().requires_grad_(True)
            col_f = npc.col_feats.detach().clone().requires_grad_(True)
            opt = FeatureAdam([{"params": [geo], "lr": 0.005}, {"params": [col_f], "lr": 0.005}])
            one = lambda: window_rays(table, pix[0], pix[1], per, ren.fx, ren.fy, ren.cx, ren.cy, const_radius=const_r)
            comp = lambda: run._window_rays(win, pix)

            def iteration(gather, weight_grads=False):
                for p in params:                       # frozen decoders: the backward pass forms no weight gradient
                    p.requires_grad_(weight_grads)
                    p.grad = None
                with torch.no_grad():
                    ro, rd, d, col, radius = gather()
                opt.zero_grad()
                loss = run._mapping_loss(ro, rd, d, col, radius, geo, col_f)[0]
                loss.backward()
                opt.step()
            ev = _interleaved({"iter_window_rays": lambda: iteration(one), "iter_per_frame": lambda: iteration(comp),
                               "iter_weight_grads": lambda: iteration(one, True),
                               "gather_window_rays": one, "gather_per_frame": comp}, reps)
            out[f"M{M}"] = {"rays": M * per, "iteration_ms": round(ev["iter_window_rays"], 3),
                            "iteration_per_frame_gather_ms": round(ev["iter_per_frame"], 3),
                            "gather_ms": round(ev["gather_window_rays"], 4),
                            "gather_per_frame_ms": round(ev["gather_per_frame"], 3),
                            "rest_ms": round(ev["iter_window_rays"] - ev["gather_window_rays"], 3),
                            "iteration_with_weight_grads_ms": round(ev["iter_weight_grads"], 3)}
            print(f"iteration M={M}", out[f"M{M}"], flush=True)
    finally:
        ren.assume_depth = False
        for p, r in zip(params, req):
            p.requires_grad_(r)
            p.grad = None
        dec.eval()
    return out


def time_refine(run):
    for s in [s for s in run.images if s >= 8]:
        del run.images[s]
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    res = run.final_refine()
    torch.cuda.synchronize()
    out = {"wall_ms": round(1e3 * (time.perf_counter() - t0), 1), "ms_per_iter": round(res["ms_per_iter"], 3),
           "window_sizes": res["window_sizes"], "per": res["per"], "iterations": 5 * 2 * run.map_iters,
           "losses": [[round(a, 4), round(b, 4)] for a, b in res["losses"]]}
    print("final_refine", out, flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "tools/time_final_refine.py measures on the GPU"
    dev = torch.device("cuda:0")
    run = _mapped_runner(dev)
    res = {"gather": time_gather(run, dev, a.reps), "iteration": time_iteration(run, dev, a.reps)}
    res["final_refine"] = time_refine(run)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
