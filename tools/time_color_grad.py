"""Cost of the colour-gradient kernels (glorie_slam_amd/color_grad.py) alone, of the gradient anchoring pass per
keyframe, and of the colour-gradient radii inside a mapping iteration.

    python tools/time_color_grad.py [--reps 200]

  maps:       color_grad_maps (magnitude, r_add, r_query) of a [3,H,W] image at 640x480 and 1200x680; device time per
              call from events around `reps` back-to-back calls
  selection:  top_indices of M = 5000 over the magnitude map at the same sizes
  anchoring:  SequenceRunner._anchor_grad_points (pixels_based_on_color_grad = 1000: maps, selection, draw, depth filter,
              insertion) per keyframe, against the stride-grid insertion alone (off); wall time of the 6th keyframe
  iteration:  SequenceRunner.map_keyframe of the 6th keyframe of the synthetic stream, ms per mapping iteration at 1000
              and 5000 rays, colour-gradient radii off and on, eager and recorded (hipGraph)
"""
import argparse
import os
import sys
import time

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


def time_kernels(dev, reps):
    from glorie_slam_amd.color_grad import color_grad_maps, top_indices
    from glorie_slam_amd.pipeline import synthetic_images
    out = {}
    for H, W in ((480, 640), (680, 1200)):
        img = synthetic_images(1, H, W)[0].to(dev).contiguous()
        valid = torch.ones(H, W, dtype=torch.bool, device=dev)
        out[f"maps {W}x{H}"] = _time(lambda: color_grad_maps(img, valid=valid), reps)
        grad = color_grad_maps(img, valid=valid, outputs=("grad",))["grad"]
        out[f"top-5000 selection {W}x{H}"] = _time(lambda: top_indices(grad, 5000), reps)
    return out


def _runner(dev, K, rays, iters, radii, grad_pixels, graphs):
    import glorie_slam_amd.pipeline as P
    run, c = P.synthetic_runner(dev, K, zero_flow_head=True, map_iters=iters, map_rays=rays)
    if radii:
        from glorie_slam_amd.color_grad import (COLOR_GRAD_THRESHOLD, RADIUS_ADD_MAX, RADIUS_ADD_MIN,
                                                RADIUS_QUERY_RATIO)
        run.color_grad = dict(color_grad_threshold=COLOR_GRAD_THRESHOLD, radius_add_max=RADIUS_ADD_MAX,
                              radius_add_min=RADIUS_ADD_MIN, radius_query_ratio=RADIUS_QUERY_RATIO)
    run.pixels_based_on_color_grad = grad_pixels
    run.map_graph = graphs
    video, imgs = c["video"], P.synthetic_images(K)
    video.poses[:K] = c["poses"][:K]
    video.disps[:K] = c["disps"][:K]
    video.disps_up[:K] = torch.nn.functional.interpolate(c["disps"][:K, None], scale_factor=8, mode="bilinear",
                                                         align_corners=False)[:, 0]
    video.counter.value = K
    for k in range(K):
        run.images[k] = imgs[k].to(dev)
    return run


def time_anchoring(dev, grad_pixels, K=6):
    """ms of the insertion of keyframe K-1 (stride grid, plus the gradient pass when grad_pixels > 0)"""
    run = _runner(dev, K, 1000, 1, True, grad_pixels, False)
    for k in range(K - 1):
        run.map_keyframe(k)
    view = run._keyframe_view(K - 1)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    with torch.no_grad():
        rmaps = run._radius_maps(K - 1, view)
        ro, rd, d, col, ii, jj, radius = run._keyframe_rays(K - 1, stride=run.add_stride, radius_map=rmaps[0])
        run.npc.add_neural_points(ro, rd, d, col, K - 1, ii, jj, dynamic_radius=radius)
        if grad_pixels:
            run._anchor_grad_points(K - 1, rmaps)
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0)


def time_iteration(dev, rays, radii, graphs, K=6, iters=20):
    run = _runner(dev, K, rays, iters, radii, 0, graphs)
    for k in range(K):
        run.map_keyframe(k)
    return run.timing["map_iter_ms"][-1], int(run.npc.pts_num())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    for name, us in time_kernels(dev, a.reps).items():
        print(f"{name}: {us:.1f} us per call")
    off = min(time_anchoring(dev, 0) for _ in range(3))
    on = min(time_anchoring(dev, 1000) for _ in range(3))
    print(f"anchoring of one keyframe: stride grid {off:.2f} ms, plus 1000 gradient pixels {on:.2f} ms")
    for graphs in (False, True):
        for rays in (1000, 5000):
            t_off, n = time_iteration(dev, rays, False, graphs)
            t_on, _ = time_iteration(dev, rays, True, graphs)
            print(f"mapping iteration ({'recorded' if graphs else 'eager'}), {rays} rays, {n} points: colour-gradient "
                  f"radii off {t_off:.2f} ms, on {t_on:.2f} ms per iteration")


if __name__ == "__main__":
    main()
