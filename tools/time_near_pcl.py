"""Time of the on-device probe march for rays without a depth prior (glorie_ray_samples_near, csrc/knn.hip) against the
host route of the same commit, on the 640x480 box view (synth.box_cloud / box_rays: 524 286 points, 307 200 rays).

    python tools/time_near_pcl.py [--reps 20] [--out profiles/near_pcl_time.json]

  sampling launch     device time (events around `reps` back-to-back calls) of one launch over the whole frame with every
                      ray depth-less, at the reference's 25 probes and at render_view's probe count, and with 5 % holes
                      in the depth; `sample_near_pcl` is NeuralPointCloud.sample_near_pcl on the same depth-less rays
                      (wall time, it reads `far` and nothing else on the host)
  frame with holes    Renderer.render_img of the frame with 5 % holes, near_pcl_path "host" and "device" (wall time
                      around synchronised calls: the host route waits for the device between its strips)
  novel view          Renderer.render_view against render_img(gt_depth=None) on the host route

The decoders are seed-43 default-initialised: the time does not depend on the weights."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

H, W = 480, 640


def _device_us(fn, reps):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return round(1e3 * e0.elapsed_time(e1) / reps, 1)


def _wall_us(fn, reps):
    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return round(1e6 * (time.perf_counter() - t0) / reps, 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "near_pcl_time.json"))
    a = ap.parse_args()
    import glorie_slam_amd.synth as synth
    from glorie_slam_amd import point_ops
    from glorie_slam_amd.decoder import POINT
    from glorie_slam_amd.neural_point import NeuralPointCloud
    from glorie_slam_amd.renderer import Renderer
    dev = torch.device("cuda:0")
    cfg = {"device": str(dev),
           "pointcloud": {"nn_weighting": "distance", "use_dynamic_radius": True, "min_nn_num": 2, "nn_num": 8,
                          "radius_query": 0.08, "radius_add": 0.04, "radius_min": 0.02},
           "rendering": {"N_surface": 10, "near_end_surface": 0.95, "far_end_surface": 1.05, "sample_near_pcl": True,
                         "sigmoid_coef": 0.1, "near_end": 0.3},
           "model": {"encode_rel_pos_in_col": True, "encode_viewd": True, "c_dim": 32}}
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)
    cloud, geo, col = synth.box_cloud()
    ro, rd, depth, radius, c2w = synth.box_rays(H, W)
    npc = NeuralPointCloud(cfg)
    npc.add_points(t(cloud), t(geo), t(col))
    torch.manual_seed(43)
    dec = POINT(cfg, use_view_direction=True).eval().to(dev)
    cam = type("Cam", (), dict(H=H, W=W, fx=320.0, fy=320.0, cx=319.5, cy=239.5))()
    o, d, g, rad = t(ro), t(rd), t(depth), t(radius * 2.5)
    holes = g.clone()
    holes[torch.rand(H * W, generator=torch.Generator().manual_seed(7)).to(dev) < 0.05] = 0.0
    ren = Renderer(cfg, cam)
    S, near = ren.N_surface, ren.near_end
    n_view = int(np.ceil((10.0 - near) / npc.radius_query)) + 1
    res = {"rays": H * W, "points": int(cloud.shape[0]), "render_view_probes": n_view}

    far10 = torch.full((1,), 10.0, device=dev)
    far_h = ren._near_far(holes, dev)
    march = lambda depth_, far_, n: point_ops.ray_samples_near(npc.index, npc.radius_query, o, d, depth_, rad, S, 0.95, 1.05,
                                                              near, far_, n)
    res["sampling_launch_us"] = {
        "all_depthless_25_probes": _device_us(lambda: march(None, far10, 25), a.reps),
        f"all_depthless_{n_view}_probes": _device_us(lambda: march(None, far10, n_view), a.reps),
        "holes_5pct_25_probes": _device_us(lambda: march(holes, far_h, 25), a.reps),
        f"holes_5pct_{n_view}_probes": _device_us(lambda: march(holes, far_h, n_view), a.reps),
        "ray_samples_all_depth": _device_us(lambda: point_ops.ray_samples(o, d, g, rad, S, 0.95, 1.05), a.reps)}
    res["sample_near_pcl_wall_us"] = {
        "all_depthless": _wall_us(lambda: npc.sample_near_pcl(o, d, near, far10[0], S), a.reps),
        "holes_5pct": _wall_us(lambda: npc.sample_near_pcl(o[holes <= 0], d[holes <= 0], near, far_h[0], S), a.reps)}
    valid = int(march(None, far10, n_view)[4].sum()), int(march(None, far10, 25)[4].sum())
    res["bracketed_rays"] = {f"{n_view}_probes": valid[0], "25_probes": valid[1]}

    kw = dict(npc_geo_feats=npc.geo_feats, npc_col_feats=npc.col_feats, cloud_pos=npc.cloud_pos())
    frame = {}
    with torch.no_grad():
        for path in ("host", "device"):
            ren.near_pcl_path = path
            frame[path] = _wall_us(lambda: ren.render_img(npc, dec, t(c2w), dev, "color", gt_depth=holes.reshape(H, W),
                                                          dynamic_r_query=rad.reshape(H, W), **kw), a.reps)
        res["frame_with_5pct_holes_wall_us"] = frame
        ren.near_pcl_path = "host"
        const = torch.full((H, W), 0.5 * (npc.radius_add + npc.radius_query), device=dev)
        res["novel_view_wall_us"] = {
            "render_view": _wall_us(lambda: ren.render_view(npc, dec, t(c2w), dev, **kw), a.reps),
            "render_view_25_probes": _wall_us(lambda: ren.render_view(npc, dec, t(c2w), dev, intervals=25, **kw), a.reps),
            "render_img_no_depth_host": _wall_us(lambda: ren.render_img(npc, dec, t(c2w), dev, "color", gt_depth=None,
                                                                        dynamic_r_query=const, **kw), a.reps)}
    res["device"] = torch.cuda.get_device_name(dev)
    print(json.dumps(res, indent=1))
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
