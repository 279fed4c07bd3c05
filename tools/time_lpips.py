"""Device time of LPIPS (glorie_slam_amd/lpips.py, csrc/lpips.hip) against the torch composition of the same formula in the
same process, its split per launch, and one keyframe's frame_metrics with and without it.

    python tools/time_lpips.py [--reps 50] [--out profiles/lpips_time.json]

  per size (480x640, 680x1200)   one call, eager and replayed from a hipGraph, with the pools as launches of their own and
                                 folded into the staging of conv2 / conv3; device time per call from events around `reps`
                                 back-to-back calls; `torch` is F.conv2d / F.max_pool2d in float32 on the device
  split                          device time of every launch of one call (torch.profiler), and the achieved FLOP/s of
                                 each convolution against the 157.3 TFLOP/s f32 matrix peak
  frame_metrics                  one 640x480 keyframe of the synthetic stream with and without lpips

The weights are seeded random numbers: the time does not depend on them."""
import argparse
import json
import os
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PEAK_F32_MATRIX = 157.3e12


def _time(fn, reps):
    for _ in range(5):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return 1e3 * e0.elapsed_time(e1) / reps


def _graphed(fn):
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        fn()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        keep = fn()
    graph.keep = keep
    return graph.replay


def seeded_weights(dev):
    from glorie_slam_amd.lpips import LAYERS
    g = torch.Generator().manual_seed(0)
    conv, lin = [], []
    for ci, co, k, _, _ in LAYERS:
        bound = (6.0 / (ci * k * k)) ** 0.5
        conv.append((((torch.rand(co, ci, k, k, generator=g) * 2 - 1) * bound).to(dev),
                     ((torch.rand(co, generator=g) * 2 - 1) * 0.1).to(dev)))
        lin.append((torch.rand(co, generator=g) * 2).to(dev))
    return conv, lin


def torch_lpips(x, y, conv, lin, shift, scale):
    """x, y [H,W,3] float32 on the device, shift, scale [1,3,1,1]: the composition torchmetrics launches"""
    from glorie_slam_amd.lpips import LAYERS, NORM_EPS
    t = torch.stack([x, y]).permute(0, 3, 1, 2)
    t = 2 * t.clamp(0.0, 1.0) - 1
    t = (t - shift) / scale
    total = 0.0
    for l, ((w, b), head, (_, _, _, s, p)) in enumerate(zip(conv, lin, LAYERS)):
        if l in (1, 2):
            t = F.max_pool2d(t, 3, 2)
        t = F.relu(F.conv2d(t, w, b, stride=s, padding=p))
        n = t / torch.sqrt(NORM_EPS + (t * t).sum(dim=1, keepdim=True))
        total = total + F.conv2d((n[0:1] - n[1:2]) ** 2, head.view(1, -1, 1, 1)).mean()
    return total


def split(metric, x, y, H, W):
    """[(launch name, microseconds)] of one call, and the FLOP/s of the convolutions; None when the profiler sees nothing"""
    from torch.autograd import DeviceType
    from torch.profiler import ProfilerActivity, profile
    from glorie_slam_amd.lpips import LAYERS, tap_shapes
    reps = 5
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        for _ in range(reps):
            metric(x, y)
        torch.cuda.synchronize()
    events = [e for e in prof.events() if "lpips_" in e.name and e.device_type == DeviceType.CUDA]
    per_call = 7 if metric.flags else 9
    if len(events) != reps * per_call:
        return None
    events.sort(key=lambda e: e.time_range.start)
    names = (["conv1", "conv2", "conv3", "conv4", "conv5", "score", "finish"] if metric.flags else
             ["conv1", "pool1", "conv2", "pool2", "conv3", "conv4", "conv5", "score", "finish"])
    flops = {f"conv{l + 1}": 2.0 * 2 * h * w * co * ci * k * k
             for l, ((h, w), (ci, co, k, _, _)) in enumerate(zip(tap_shapes(H, W), LAYERS))}
    rows = []
    for i, name in enumerate(names):
        us = sum(events[r * per_call + i].time_range.elapsed_us() for r in range(1, reps)) / (reps - 1)     # the first call warms up
        row = {"launch": name, "us": round(us, 2)}
        if name in flops:
            row["tflops"] = round(flops[name] / us / 1e6, 2)
            row["of_peak"] = round(flops[name] / (us * 1e-6) / PEAK_F32_MATRIX, 4)
        rows.append(row)
    return rows


def time_calls(dev, reps):
    from glorie_slam_amd.lpips import SCALE, SHIFT, Lpips
    from glorie_slam_amd.pipeline import synthetic_images
    conv, lin = seeded_weights(dev)
    shift, scale = (torch.tensor(v, device=dev).view(1, 3, 1, 1) for v in (SHIFT, SCALE))
    metrics = {"pool launches": Lpips(conv, lin, device=dev), "folded pools": Lpips(conv, lin, device=dev, fold_pools=True)}
    out = {}
    for H, W in ((480, 640), (680, 1200)):
        x = synthetic_images(1, H, W)[0].permute(1, 2, 0).contiguous().to(dev)
        y = (x + 0.05 * torch.randn_like(x)).clamp(0, 1)
        res = {"value": float(metrics["pool launches"](x, y)), "torch_value": float(torch_lpips(x, y, conv, lin, shift, scale))}
        print(f"{W}x{H}: lpips {res['value']:.7f}, torch composition {res['torch_value']:.7f}")
        for name, m in metrics.items():
            eager, replay = _time(lambda: m(x, y), reps), _time(_graphed(lambda: m(x, y)), reps)
            res[name] = {"eager_us": round(eager, 1), "replayed_us": round(replay, 1), "split": split(m, x, y, H, W)}
            print(f"  {name}: {eager:.1f} us eager, {replay:.1f} us replayed")
            for row in res[name]["split"] or []:
                extra = f"  {row['tflops']:.1f} TFLOP/s, {100 * row['of_peak']:.1f} % of peak" if "tflops" in row else ""
                print(f"    {row['launch']:7s} {row['us']:9.1f} us{extra}")
        ref = lambda: torch_lpips(x, y, conv, lin, shift, scale)
        res["torch"] = {"eager_us": round(_time(ref, reps), 1), "replayed_us": round(_time(_graphed(ref), reps), 1)}
        print(f"  torch composition: {res['torch']['eager_us']:.1f} us eager, {res['torch']['replayed_us']:.1f} us replayed")
        out[f"{H}x{W}"] = res
    return out, metrics["pool launches"]


def time_eval(dev, reps, metric, K=6):
    import glorie_slam_amd.pipeline as P
    from glorie_slam_amd.eval_render import _constant_radius, _score
    from glorie_slam_amd.image_metrics import frame_metrics
    run, c = P.synthetic_runner(dev, K, zero_flow_head=True, map_iters=10, map_rays=1000)
    video, imgs = c["video"], P.synthetic_images(K)
    for k in range(K):
        run.init_state(k)
        video.timestamp[k] = k
        run.images[k] = imgs[k].to(dev)
    video.counter.value = K
    for k in range(K):
        run.map_keyframe(k)
        run.mapped += 1
    k = K - 1
    depth, c2w = run._keyframe_view(k)
    gt = run.images[k].permute(1, 2, 0).contiguous()
    with torch.no_grad():
        m, color, r_depth, mask = _score(run, c2w, depth, _constant_radius(run, depth), gt, None, metric)
        without = _time(lambda: frame_metrics(color, r_depth, gt, mask), reps)
        with_lpips = _time(lambda: frame_metrics(color, r_depth, gt, mask, lpips=metric), reps)
    print(f"frame_metrics, one 640x480 keyframe: {without:.1f} us without lpips, {with_lpips:.1f} us with; "
          f"lpips {float(m['lpips']):.4f} masked {float(m['masked_lpips']):.4f}")
    return {"without_lpips_us": round(without, 1), "with_lpips_us": round(with_lpips, 1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lpips_time.json"))
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    res, metric = time_calls(dev, a.reps)
    res["frame_metrics_480x640"] = time_eval(dev, a.reps, metric)
    res["device"] = torch.cuda.get_device_name(dev)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
