"""Cost of the keyframe selection kernels (glorie_slam_amd/keyframe_select.py) alone and of frustum selection inside a
mapping iteration.

    python tools/time_keyframe_select.py [--reps 200]

  frustum:    frustum_feature_mask with the ascending indices at 524,286 points (synth.box_cloud seen by the box_rays
              camera, 640x480) and at 2,097,144 points (the same cloud four times, jittered); device time per call from
              events around `reps` back-to-back calls
  overlap:    keyframe_overlap at 200 rays x 8 samples against 64 and 512 keyframes
  iteration:  SequenceRunner.map_keyframe of the 6th keyframe of the synthetic stream, ms per mapping iteration at 1000
              and 5000 rays, frustum_feature_selection off and on, eager and recorded (hipGraph)
"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _time(fn, reps):
    for _ in range(10):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return 1e3 * e0.elapsed_time(e1) / reps


def time_selection(dev, reps):
    from glorie_slam_amd import synth
    from glorie_slam_amd.keyframe_select import frustum_feature_mask, keyframe_overlap
    pts, _, _ = synth.box_cloud()
    ro, rd, depth, _, c2w = synth.box_rays()
    K = (320.0, 320.0, 319.5, 239.5)
    D, C = torch.from_numpy(depth.reshape(480, 640)).to(dev), torch.from_numpy(c2w).to(dev)
    rng = np.random.default_rng(0)
    big = np.concatenate([pts] + [pts + rng.normal(0, 0.01, pts.shape).astype(np.float32) for _ in range(3)])
    out = {}
    for name, p in (("524k", pts), ("2M", big)):
        P = torch.from_numpy(p).to(dev)
        out[f"frustum {name} ({len(p)} points)"] = _time(
            lambda: frustum_feature_mask(P, C, D, *K, 480, 640, -4.0, return_indices=True), reps)
    sel = rng.choice(len(depth), 200, replace=False)
    o, d, z = (torch.from_numpy(x[sel]).to(dev) for x in (ro, rd, depth))
    for nk in (64, 512):
        c2ws = C.expand(nk, 4, 4).contiguous()
        out[f"overlap 200x8 samples, {nk} keyframes"] = _time(
            lambda: keyframe_overlap(o, d, z, c2ws, *K, 480, 640, return_counts=True), reps)
    return out


def time_iteration(dev, rays, frustum, graphs, K=6, iters=20):
    from glorie_slam_amd.pipeline import synthetic_images, synthetic_runner
    run, c = synthetic_runner(dev, K, zero_flow_head=True, map_iters=iters, map_rays=rays)
    run.frustum_feature_selection = frustum
    run.map_graph = graphs
    video, imgs = c["video"], synthetic_images(K)
    video.poses[:K] = c["poses"][:K]
    video.disps[:K] = c["disps"][:K]
    video.disps_up[:K] = torch.nn.functional.interpolate(c["disps"][:K, None], scale_factor=8, mode="bilinear",
                                                         align_corners=False)[:, 0]
    video.counter.value = K
    for k in range(K):
        run.images[k] = imgs[k].to(dev)
        run.map_keyframe(k)
    return run.timing["map_iter_ms"][-1], int(run.npc.pts_num()), (run.frustum_counts or [None])[-1]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    for name, us in time_selection(dev, a.reps).items():
        print(f"{name}: {us:.1f} us per call")
    for graphs in (False, True):
        for rays in (1000, 5000):
            off, n, _ = time_iteration(dev, rays, False, graphs)
            on, _, kept = time_iteration(dev, rays, True, graphs)
            print(f"mapping iteration ({'recorded' if graphs else 'eager'}), {rays} rays, {n} points ({kept} in the "
                  f"frustum): frustum selection off {off:.2f} ms, on {on:.2f} ms per iteration")


if __name__ == "__main__":
    main()
