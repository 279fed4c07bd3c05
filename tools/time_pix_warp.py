"""Cost of the pixel-warping term (glorie_slam_amd/warp_loss.py) alone and inside a mapping iteration.

    python tools/time_pix_warp.py [--reps 200]

  term:       forward + backward of pix_warping_loss at 5000 rays x 5 frames of 640x480 (device time per call from
              events around `reps` back-to-back calls; also the forward alone)
  iteration:  SequenceRunner.map_keyframe of the 6th keyframe of the synthetic stream (window of 5 with the term on),
              ms per mapping iteration at 1000 and 5000 rays, pix_warping off and on, eager and recorded (hipGraph)
"""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def time_term(dev, reps):
    from glorie_slam_amd.warp_loss import FrameTable, pix_warping_loss
    from test_gpu_pix_warp import product_case
    c = product_case()
    t = lambda x: x.to(dev)
    table = FrameTable([im.permute(2, 0, 1).contiguous().to(dev) for im in c["images"]], channels_first=True)
    args = [t(c["rays_o"]), t(c["rays_d"]), None, t(c["c2ws"]), c["fx"], c["fy"], c["cx"], c["cy"], c["W"], c["H"],
            t(c["frame_indices"]), t(c["indices"]), table, t(c["gt"])]
    depth = t(c["depth"]).requires_grad_(True)

    def step(backward):
        a = list(args)
        a[2] = depth
        loss = pix_warping_loss(*a, nan_to_zero=True)
        if backward:
            loss.backward()
    out = {}
    for backward in (False, True):
        for _ in range(10):
            step(backward)
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            step(backward)
        e1.record()
        torch.cuda.synchronize()
        out["fwd+bwd" if backward else "fwd"] = 1e3 * e0.elapsed_time(e1) / reps
    return out


def time_iteration(dev, rays, warp, graphs, K=6, iters=20):
    from glorie_slam_amd.pipeline import synthetic_images, synthetic_runner
    run, c = synthetic_runner(dev, K, zero_flow_head=True, map_iters=iters, map_rays=rays)
    run.pix_warping, run.mapping_window_size = warp, 5
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
    return run.timing["map_iter_ms"][-1]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    term = time_term(dev, a.reps)
    print(f"term 5000 rays x 5 frames: fwd {term['fwd']:.1f} us, fwd+bwd {term['fwd+bwd']:.1f} us per call")
    for graphs in (False, True):
        for rays in (1000, 5000):
            off = time_iteration(dev, rays, False, graphs)
            on = time_iteration(dev, rays, True, graphs)
            print(f"mapping iteration ({'recorded' if graphs else 'eager'}), {rays} rays: pix_warping off {off:.2f} ms, "
                  f"on {on:.2f} ms per iteration")


if __name__ == "__main__":
    main()
