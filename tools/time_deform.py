"""Cost of the cloud deformation and the proxy depth on HIP (glorie_slam_amd/neural_point.py deform_points,
proxy_render_depth) against the torch formulations, and of one keyframe's mapping with the keys off and on.

    python tools/time_deform.py [--reps 50]

  deform:   200k and 1M input points (x N_add = 3 cloud rows) over 200 keyframes of 120x160, 25 dirty and all 200 dirty:
            the launches of deform_points (deformation + unprojection, events around `reps` back-to-back calls, the index
            rebuild left out) and the whole deform_points with the rebuild (wall time); the torch update_points_pos(npc,
            video) (wall time, includes its rebuild)
  proxy:    proxy_render_depth at 640x480 over 64 and 200 unprojected keyframes, against get_proxy_render_depth
  mapping:  SequenceRunner.map_keyframe of the 6th keyframe of the synthetic 640x480 stream (20 iterations of 1000 rays),
            keys off and on (bind_npc_with_pose + render_depth "proxy"), wall time
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def _events(fn, reps):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return 1e3 * e0.elapsed_time(e1) / reps


def _wall(fn, reps):
    fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return 1e6 * (time.perf_counter() - t0) / reps


def time_deform(dev, reps):
    from glorie_slam_amd import neural_point as NP
    from test_gpu_deform import _big
    out = {}
    for n_pts in (200_000, 1_000_000):
        video, npc, cam, _ = _big(dev, B=200, H=120, W=160, n_pts=n_pts)
        for n_dirty in (25, 200):
            sel = torch.randperm(200, generator=torch.Generator().manual_seed(0))[:n_dirty].to(dev)

            def mark():
                video.npc_dirty[sel] = True

            def launches():
                mark()
                NP.deform_points(npc, video, *cam, rebuild_index=False)

            def full():
                mark()
                NP.deform_points(npc, video, *cam)

            def torch_path():
                mark()
                NP.update_points_pos(npc, video)
            key = f"{n_pts // 1000}k_{n_dirty}dirty"
            out[key] = {"hip_launches_us": round(_events(launches, reps), 1),
                        "hip_with_rebuild_us": round(_wall(full, max(reps // 5, 3)), 1),
                        "torch_us": round(_wall(torch_path, 3), 1)}
            print(key, out[key], flush=True)
        del video, npc
        torch.cuda.empty_cache()
    return out


def time_proxy(dev, reps):
    import types
    from glorie_slam_amd import neural_point as NP
    H, W = 480, 640
    fx, fy, cx, cy = 320.0, 320.0, 319.5, 239.5
    out = {}
    for n_kf in (64, 200):
        g = torch.Generator(device="cpu").manual_seed(0)
        pcl = (torch.rand(n_kf, H, W, 3, generator=g) * torch.tensor([4.0, 3.0, -3.0]) - torch.tensor([2.0, 1.5, 1.0]))
        pcl = pcl.to(dev).contiguous()
        mask = (torch.rand(n_kf, H, W, generator=g) > 0.2).to(dev)
        cfg = {"cam": {"H": H, "W": W, "fx": fx, "fy": fy, "cx": cx, "cy": cy, "H_out": H, "W_out": W},
               "mapping": {"mapping_window_size": 5}}
        video = types.SimpleNamespace(counter=types.SimpleNamespace(value=n_kf))
        npc = types.SimpleNamespace(_full_pcl=pcl, _full_mask=mask, video=video, get_device=lambda: dev,
                                    full_pcl=lambda: pcl, full_mask=lambda: mask)
        c2w = torch.eye(4, device=dev)
        droid = torch.rand(H, W, generator=g).to(dev)
        droid[:, : W // 2] = 0
        mono = torch.full((H, W), 2.0, device=dev)
        hip = _events(lambda: NP.proxy_render_depth(npc, video, c2w, droid, mono, 5, fx, fy, cx, cy), reps)
        ref = _wall(lambda: NP.get_proxy_render_depth(npc, cfg, c2w, droid, mono, dev), 5)
        out[f"{n_kf}kf"] = {"hip_us": round(hip, 1), "torch_get_proxy_render_depth_us": round(ref, 1)}
        print(n_kf, out[f"{n_kf}kf"], flush=True)
    return out


def time_mapping(dev):
    import glorie_slam_amd.pipeline as P
    out = {}
    for on in (False, True):
        run, c = P.synthetic_runner(dev, 8, map_iters=20, map_rays=1000)
        if on:
            run.bind_npc_with_pose, run.render_depth = True, "proxy"
        video = c["video"]
        imgs = P.synthetic_images(8)
        for k in range(8):
            run.init_state(k)
            video.timestamp[k] = k
            run.images[k] = imgs[k].to(dev)
        video.valid_depth_mask[:8] = True
        video.valid_depth_mask[:8, :, 200:260] = False
        video.intrinsics[:8] = c["intrinsics"].to(dev) / 8.0
        video.counter.value = 8
        for k in range(5):
            run.map_keyframe(k)
        video.set_dirty(0, 5)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        run.map_keyframe(5)
        torch.cuda.synchronize()
        out["on" if on else "off"] = round(1e3 * (time.perf_counter() - t0), 2)
        print("mapping keyframe 5, keys", "on" if on else "off", out["on" if on else "off"], "ms", flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "tools/time_deform.py measures on the GPU"
    dev = torch.device("cuda:0")
    import json
    res = {"deform": time_deform(dev, a.reps), "proxy": time_proxy(dev, a.reps), "map_keyframe_ms": time_mapping(dev)}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
