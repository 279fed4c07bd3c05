"""Cost of the mapping schedule's kernels (glorie_slam_amd/map_sample.py) against the torch composition of the reference's
formulation, and of one mapping iteration of the synthetic runner with the schedule off and on.

    python tools/time_map_schedule.py [--reps 30]

  kernels:    at 640x480 with 10 % of the pixels without depth, M = 1 / 5 / 10 window frames and 1000 // M rays of each:
              valid_index_build (once per keyframe), and per iteration sample_window_rays against the reference's sampling
              in torch (per frame mask.nonzero(), randint(count), indexing, the rays, the depth filter; concatenated) and
              depth_gate against median / max / minimum / compare and the boolean indexing of the five ray tensors.  The
              variants alternate call by call in one process, events around every call, medians over `reps`; and the
              wall time of `reps` back-to-back calls (the torch composition waits for the device in every frame)
  iteration:  map_keyframe over 8 keyframes of the synthetic stream, ms per iteration as the runner times it (wall clock
              around the keyframe's iterations, synchronised), schedule off and on alternating keyframe by keyframe, on a
              stream with a depth at every pixel and on one with a hole of 10 % in every keyframe; medians over the
              keyframes after the first
"""
import argparse
import functools
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SIZES = (1, 5, 10)
H, W, RAYS = 480, 640, 1000
K = (320.0, 320.0, 319.5, 239.5)


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


def _torch_sampling(depths, images_hwc, c2ws, per, dev):
    """the reference's get_samples(mask=depth > 0, depth_filter=True) per frame, concatenated (src/utils/common.py:57-145,
    src/mapper.py:420-465)"""
    from glorie_slam_amd.common import get_rays_from_uv
    fx, fy, cx, cy = K
    out = [[] for _ in range(6)]
    for depth, image, c2w in zip(depths, images_hwc, c2ws):
        i, j = torch.meshgrid(torch.linspace(0, W - 1, W, device=dev), torch.linspace(0, H - 1, H, device=dev), indexing="ij")
        i, j = i.t().reshape(-1), j.t().reshape(-1)
        valid_index = (depth > 0).reshape(-1).nonzero().reshape(-1)
        indices = valid_index[torch.randint(valid_index.shape[0], (per,), device=dev)]
        i, j, d, col = i[indices], j[indices], depth.reshape(-1)[indices], image.reshape(-1, 3)[indices]
        ro, rd = get_rays_from_uv(i, j, c2w, fx, fy, cx, cy, dev)
        keep = d > 0
        for o, x in zip(out, (ro[keep], rd[keep], d[keep], col[keep], i[keep].long(), j[keep].long())):
            o.append(x)
    return [torch.cat(o) for o in out]


def _torch_gate(ro, rd, d, col, ii):
    """src/mapper.py:474-482"""
    inside = d <= torch.minimum(10 * d.median(), 1.2 * torch.max(d))
    return ro[inside], rd[inside], d[inside], col[inside], ii[inside]


def time_kernels(dev, reps):
    from glorie_slam_amd.map_sample import ValidIndex, depth_gate, sample_window_rays
    from glorie_slam_amd.window_rays import WindowTable
    g = torch.Generator().manual_seed(0)
    out = {}
    for M in SIZES:
        per = RAYS // M
        depths = torch.rand(M, H, W, generator=g) * 3 + 0.5
        depths[torch.rand(M, H, W, generator=g) < 0.1] = 0
        depths = list(depths.to(dev))
        images = list(torch.rand(M, 3, H, W, generator=g).to(dev))
        images_hwc = [im.permute(1, 2, 0).contiguous() for im in images]
        c2ws = torch.eye(4, device=dev).repeat(M, 1, 1)
        table = WindowTable(depths, images, c2ws)
        index = ValidIndex(table)
        draws = torch.randint(0, 2 ** 31, (M * per,), generator=g).to(dev)
        rays = sample_window_rays(table, index, draws, per, *K)
        ours = lambda: sample_window_rays(table, index, draws, per, *K)
        theirs = lambda: _torch_sampling(depths, images_hwc, c2ws, per, dev)
        variants = {"valid_index_build": lambda: ValidIndex(table), "sample_window_rays": ours, "torch_sampling": theirs,
                    "depth_gate": lambda: depth_gate(rays[2]),
                    "torch_gate": lambda: _torch_gate(rays[0], rays[1], rays[2], rays[3], rays[5])}
        ev = _interleaved(variants, reps)
        row = {"per": per, "rays": M * per}
        for name, fn in variants.items():
            row[name + "_ms"] = round(ev[name], 4)
            row[name + "_wall_ms"] = round(_wall(fn, reps), 4)
        out[f"M{M}"] = row
        print(f"kernels M={M}", row, flush=True)
    return out


def _runner(dev, schedule, holes, iters=20):
    import glorie_slam_amd.pipeline as P
    orig = P.SequenceRunner
    P.SequenceRunner = functools.partial(orig, mapping_schedule=schedule)
    try:
        run, c = P.synthetic_runner(dev, 8, map_iters=iters, map_rays=RAYS)
    finally:
        P.SequenceRunner = orig
    run.schedule.update(iters_first=iters, iters=iters, min_iter_ratio=1.0, geo_iter_first=int(iters * 0.3))
    imgs = P.synthetic_images(8)
    for k in range(8):
        run.init_state(k)
        if holes:
            c["video"].disps_up[k][100:250, 200:400] = 0             # 30000 of 307200 pixels
        c["video"].timestamp[k] = k
        run.images[k] = imgs[k].to(dev)
    c["video"].counter.value = 8
    return run


def time_iteration(dev):
    out = {}
    for holes in (False, True):
        runs = {"off": _runner(dev, False, holes), "on": _runner(dev, True, holes)}
        for k in range(8):
            for run in runs.values():
                run.map_keyframe(k)
        row = {}
        for name, run in runs.items():
            ms = run.timing["map_iter_ms"]
            row[f"schedule_{name}_ms_per_iter"] = round(statistics.median(ms[1:]), 3)
            row[f"schedule_{name}_min_max"] = [round(min(ms[1:]), 3), round(max(ms[1:]), 3)]
        row["schedules"] = runs["on"].schedules[:3]
        out["holes" if holes else "full_depth"] = row
        print("iteration", "holes" if holes else "full_depth", row, flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "tools/time_map_schedule.py measures on the GPU"
    dev = torch.device("cuda:0")
    res = {"kernels": time_kernels(dev, a.reps), "iteration": time_iteration(dev)}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
