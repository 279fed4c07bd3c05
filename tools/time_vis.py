"""Device time of the mapper's contact sheet (glorie_slam_amd/visualizer.py, csrc/vis.hip) and what surrounds it.

    python tools/time_vis.py [--reps 30] [--json profiles/vis_time.json]

  passes    the range pass (two launches) and the compose pass (one launch) at 480x640 and 680x1200, scale 1 and 2:
            every call between its own pair of events, medians of --reps; eager, and both passes replayed from one
            captured graph.  An event pair around a launch of a few microseconds mostly times the launch, so each pass
            is also issued 200 times back to back between one pair of events (`burst`: device time per call unless the
            host issues slower than the device runs)
  bytes/s   over the algorithmic bytes and the burst time.  Range pass: the three maps read once.  Compose pass: the 13
            floats of a source pixel (7 scalar maps, 2 colour maps) for each of the ceil(H / scale) ceil(W / scale)
            pixels a panel shows, read once, plus the sheet written once
  torch     the same sheet composed from torch ops on the device in the same process (alternating with the kernels); the
            number of bytes in which it differs from the kernels' sheet is printed
  jpeg      host time of the device-to-host copy, the titles and PIL's JPEG encoder for one sheet
  keyframe  one keyframe's Visualizer.vis on the synthetic runner at 480x640 split into render, projections, compose and
            file (host clock around work that ends in a synchronise)
  matplotlib  for the record, the reference's figure (twelve imshow panels, savefig at 300 dpi) from the same maps on the
            host of the same machine, where matplotlib is installed
"""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

N_SURFACE = 10


def scene(H, W, dev, seed=0):
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.rand(*s, generator=g)
    rd = r(H, W) * 4 + 0.5
    rd[r(H, W) < 0.1] = 0
    maps = dict(render_depth=rd, depth=rd + (r(H, W) - 0.5) * 0.3, color=r(H, W, 3) * 1.2 - 0.1, gt_color=r(H, W, 3),
                droid_depth=torch.where(r(H, W) < 0.8, rd, torch.zeros(())), proj_depth=torch.where(r(H, W) < 0.6, rd, torch.zeros(())),
                valid_ray_count=torch.randint(0, N_SURFACE + 1, (H, W), generator=g).float(),
                sparse_proj_depth=torch.where(r(H, W) < 0.1, rd, torch.zeros(())), mono_depth=rd * 1.25 + 0.1)
    return {k: v.contiguous().to(dev) for k, v in maps.items()}


def torch_sheet(m, n_surface, table, scale, gutter, title):
    """the sheet from torch ops, the arithmetic of include/glorie_hip.h in float32"""
    from glorie_slam_amd.visualizer import panel_boxes, sheet_size
    H, W = m["render_depth"].shape
    rd, d = m["render_depth"], m["depth"]
    res = (rd - d).abs()
    res = torch.where(res > 0.2, torch.full_like(res, 0.2), res)
    res = torch.where(rd == 0, torch.zeros_like(res), res)
    fin = lambda v: v[torch.isfinite(v)]
    droid = fin(m["droid_depth"])
    dmax = droid.max() if droid.numel() else torch.zeros((), device=rd.device)
    rf = fin(res)
    rmin, rmax = (rf.min(), rf.max()) if rf.numel() else (torch.zeros((), device=rd.device),) * 2

    def cmap(v, lo, hi):
        t = torch.where(hi == lo, torch.zeros_like(v), (v - lo) / (hi - lo))
        f = t * 256.0
        idx = torch.where(f > 0, f.clamp(max=255.0), torch.zeros_like(f)).long()
        out = table[idx]
        out[~torch.isfinite(v)] = 255
        return out

    lvl = lambda x: (torch.where(x > 0, x.clamp(max=1.0), torch.zeros_like(x)) * 255.0).to(torch.uint8)
    c = torch.round(m["color"] * 255.0) / 255.0
    cres = torch.where((rd == 0)[..., None], torch.zeros_like(c), (m["gt_color"] - c).abs())
    zero, one = torch.zeros((), device=rd.device), torch.ones((), device=rd.device)
    panels = [cmap(rd, zero, dmax), cmap(d, zero, dmax), cmap(res, rmin, rmax), lvl(m["gt_color"]), lvl(c), lvl(cres),
              cmap(m["droid_depth"], zero, dmax), cmap(m["proj_depth"], zero, dmax),
              cmap((m["proj_depth"] > 0).float(), zero, one), cmap(m["valid_ray_count"], zero, one * float(n_surface)),
              cmap(m["sparse_proj_depth"], zero, dmax), cmap(m["mono_depth"], zero, dmax)]
    SH, SW = sheet_size(H, W, scale, gutter, title)
    sheet = torch.full((SH, SW, 3), 255, dtype=torch.uint8, device=rd.device)
    ys = (torch.arange(-(-H // scale), device=rd.device) * scale + scale // 2).clamp(max=H - 1)
    xs = (torch.arange(-(-W // scale), device=rd.device) * scale + scale // 2).clamp(max=W - 1)
    for (y0, x0, ph, pw), p in zip(panel_boxes(H, W, scale, gutter, title), panels):
        sheet[y0:y0 + ph, x0:x0 + pw] = p[ys][:, xs]
    return sheet


def alternate(fns, reps, warmup=5):
    """{name: median ms}: the variants called in turn, each call between its own pair of events"""
    for _ in range(warmup):
        for fn in fns.values():
            fn()
    torch.cuda.synchronize()
    pairs = {k: [] for k in fns}
    for _ in range(reps):
        for k, fn in fns.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            pairs[k].append((e0, e1))
    torch.cuda.synchronize()
    return {k: float(np.median([a.elapsed_time(b) for a, b in v])) for k, v in pairs.items()}


def burst(fn, n=200):
    """ms per call of n calls back to back between one pair of events"""
    for _ in range(10):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n


def capture(fn, dev):
    graph, side = torch.cuda.CUDAGraph(), torch.cuda.Stream(dev)
    torch.cuda.synchronize()
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        graph.capture_begin()
        try:
            fn()
        finally:
            graph.capture_end()
    torch.cuda.current_stream(dev).wait_stream(side)
    return graph


def time_passes(H, W, scale, dev, reps):
    import glorie_slam_amd.visualizer as V
    from glorie_slam_amd import _lib as L
    m = scene(H, W, dev)
    SH, SW = V.sheet_size(H, W, scale)
    out = torch.empty(SH, SW, 3, dtype=torch.uint8, device=dev)
    ranges = torch.empty(4, device=dev)
    table = V._table(dev)
    V.contact_sheet(m, N_SURFACE, scale=scale, out=out, ranges=ranges)
    ref = torch_sheet(m, N_SURFACE, table, scale, 4, 12)
    differing = int((ref != out).sum())

    def compose_only():
        L.check(L.load().glorie_vis_compose(*(L.ptr(m[k]) for k in V.MAP_KEYS), H, W, L.ptr(ranges), float(N_SURFACE),
                                            L.ptr(table), scale, 4, 12, L.ptr(out), L.stream_ptr(dev)), "glorie_vis_compose")
    both = lambda: V.contact_sheet(m, N_SURFACE, scale=scale, out=out, ranges=ranges)
    graph = capture(both, dev)
    ms = alternate({"range": lambda: V.sheet_ranges(m, out=ranges), "compose": compose_only, "both": both,
                    "replayed": graph.replay, "torch": lambda: torch_sheet(m, N_SURFACE, table, scale, 4, 12)}, reps)
    b_range, b_compose = burst(lambda: V.sheet_ranges(m, out=ranges)), burst(compose_only)
    b_replay = burst(graph.replay)
    ph, pw = -(-H // scale), -(-W // scale)
    range_bytes, compose_bytes = 3 * 4 * H * W, 13 * 4 * ph * pw + SH * SW * 3
    row = dict(H=H, W=W, scale=scale, sheet=[SH, SW], range_us=1e3 * ms["range"], compose_us=1e3 * ms["compose"],
               both_eager_us=1e3 * ms["both"], both_replayed_us=1e3 * ms["replayed"], torch_us=1e3 * ms["torch"],
               range_burst_us=1e3 * b_range, compose_burst_us=1e3 * b_compose, replayed_burst_us=1e3 * b_replay,
               range_bytes=range_bytes, compose_bytes=compose_bytes, range_GBps=range_bytes / b_range / 1e6,
               compose_GBps=compose_bytes / b_compose / 1e6, bytes_differing_from_torch=differing)
    print(f"{H}x{W} scale {scale} (sheet {SH}x{SW}): event pair per call: range pass {row['range_us']:.1f} us, compose "
          f"{row['compose_us']:.1f} us, both eager {row['both_eager_us']:.1f} us, replayed {row['both_replayed_us']:.1f} us, torch "
          f"ops {row['torch_us']:.1f} us ({row['torch_us'] / row['both_eager_us']:.1f}x the eager passes); back to back: range "
          f"{row['range_burst_us']:.1f} us ({row['range_GBps']:.0f} GB/s on {range_bytes} B), compose "
          f"{row['compose_burst_us']:.1f} us ({row['compose_GBps']:.0f} GB/s on {compose_bytes} B), replayed "
          f"{row['replayed_burst_us']:.1f} us; {differing} bytes differ from the torch sheet")
    return row, m, out


def time_jpeg(sheet, H, W, reps=5):
    from PIL import Image

    import glorie_slam_amd.visualizer as V
    path = os.path.join(tempfile.mkdtemp(), "sheet.jpg")
    ts = {"copy": [], "titles": [], "encode": []}
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        image = Image.fromarray(sheet.cpu().numpy())
        t1 = time.perf_counter()
        V.draw_titles(image, V.panel_boxes(H, W))
        t2 = time.perf_counter()
        image.save(path, quality=90)
        t3 = time.perf_counter()
        for k, v in zip(ts, (t1 - t0, t2 - t1, t3 - t2)):
            ts[k].append(1e3 * v)
    row = {f"{k}_ms": float(np.median(v)) for k, v in ts.items()}
    row["file_bytes"] = os.path.getsize(path)
    print(f"sheet {tuple(sheet.shape)} to a JPEG: copy {row['copy_ms']:.2f} ms, titles {row['titles_ms']:.2f} ms, encode "
          f"{row['encode_ms']:.2f} ms, {row['file_bytes']} bytes")
    return row


def time_keyframe(dev, reps=5):
    """Visualizer.vis of the second keyframe of the synthetic runner at 480x640, its parts timed on their own"""
    import glorie_slam_amd.pipeline as P
    import glorie_slam_amd.visualizer as V
    from glorie_slam_amd.neural_point import proj_depth_map
    K, H, W = 2, 480, 640
    run, c = P.synthetic_runner(dev, K, map_iters=20, map_rays=1000, H=H, W=W)
    video, imgs = c["video"], P.synthetic_images(K, H, W)
    for k in range(K):
        run.init_state(k)
        video.timestamp[k] = k
        run.images[k] = imgs[k].to(dev)
    video.intrinsics[:K] = c["intrinsics"].to(dev) / 8.0
    video.counter.value = K
    run.mapping_vis = tempfile.mkdtemp()
    run.vis_options = dict(keep=True)
    for k in range(K):
        run.map_keyframe(k)
    vis, kept = run.visualizer, run.visualizer.kept[-1]
    m, c2w, npc = kept["maps"], kept["c2w"], run.npc
    cfg = run._mono_cfg()
    cfg["mapping"] = dict(cfg["mapping"], mapping_window_size=run.mapping_window_size)
    r_query = torch.full_like(m["render_depth"], 0.5 * (npc.radius_add + npc.radius_query))

    def clock(fn):
        ts = []
        for _ in range(reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ts.append(1e3 * (time.perf_counter() - t0))
        return float(np.median(ts))
    path = os.path.join(run.mapping_vis, "timed.jpg")
    row = dict(
        map_iter_ms=float(np.median(run.timing["map_iter_ms"])), points=int(npc.pts_num()),
        render_ms=clock(lambda: vis.vis_value_only(m["render_depth"], c2w, npc, run.decoders, npc.get_geo_feats(),
                                                   npc.get_col_feats(), r_query, npc.cloud_pos())),
        projections_ms=clock(lambda: (proj_depth_map(c2w.clone(), npc, dev, cfg, neural_pcl=True),
                                      proj_depth_map(c2w, npc, dev, cfg, neural_pcl=True))),
        compose_ms=clock(lambda: V.contact_sheet(m, N_SURFACE)),
        file_ms=clock(lambda: vis._write_sheet(path, kept["sheet"], (H, W))),
        whole_vis_ms=clock(lambda: vis.vis(1, 19, None, m["render_depth"], m["droid_depth"], m["mono_depth"], m["gt_color"], c2w,
                                           npc, run.decoders, npc.get_geo_feats(), npc.get_col_feats(), cfg, None,
                                           dynamic_r_query=r_query, cloud_pos=npc.cloud_pos(), cur_total_iters=20)))
    print(f"one keyframe's vis at {H}x{W} ({row['points']} points; a mapping iteration took {row['map_iter_ms']:.2f} ms): render "
          f"{row['render_ms']:.2f} ms, projections {row['projections_ms']:.2f} ms, compose {row['compose_ms']:.2f} ms, file "
          f"{row['file_ms']:.2f} ms; the whole call {row['whole_vis_ms']:.2f} ms")
    return row, {k: v.float().cpu().numpy() for k, v in m.items()}


def time_matplotlib(m):
    """the reference's figure (Visualizer.py:130-209) from host arrays: first and second call, seconds"""
    try:
        import matplotlib
    except ImportError:
        print("matplotlib is not installed here: the reference's formulation was not timed")
        return None
    matplotlib.use("Agg")
    import matplotlib.pyplot as plt
    import vis_ref as R
    res = R.depth_residual(m["render_depth"], m["depth"])
    c = R.round_level(m["color"])
    cres = np.clip(np.where((m["render_depth"] == 0)[..., None], 0, np.abs(m["gt_color"] - c)), 0, 1)
    dmax = float(np.max(m["droid_depth"]))
    panels = [(m["render_depth"], 0, dmax), (m["depth"], 0, dmax), (res, None, None), (np.clip(m["gt_color"], 0, 1), None, None),
              (np.clip(c, 0, 1), None, None), (cres, None, None), (m["droid_depth"], 0, dmax), (m["proj_depth"], 0, dmax),
              ((m["proj_depth"] > 0).astype(np.int32), 0, 1), (m["valid_ray_count"], 0, N_SURFACE),
              (m["sparse_proj_depth"], 0, dmax), (m["mono_depth"], 0, dmax)]
    path = os.path.join(tempfile.mkdtemp(), "figure.jpg")
    ts = []
    for _ in range(2):
        t0 = time.perf_counter()
        fig, axs = plt.subplots(4, 3)
        for ax, (a, lo, hi) in zip(axs.reshape(-1), panels):
            ax.imshow(a, cmap="plasma", vmin=lo, vmax=hi)
            ax.set_xticks([])
            ax.set_yticks([])
        plt.subplots_adjust(wspace=0, hspace=0.5)
        plt.savefig(path, dpi=300, bbox_inches='tight', pad_inches=0.1)
        plt.clf()
        plt.close()
        ts.append(time.perf_counter() - t0)
    print(f"matplotlib figure of the same maps on this host: {ts[0]:.2f} s the first time, {ts[1]:.2f} s the second")
    return dict(first_s=ts[0], second_s=ts[1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    if not torch.cuda.is_available():
        raise SystemExit("time_vis.py measures on the GPU; none is visible")
    dev = torch.device("cuda:0")
    rows, jpeg = [], None
    for H, W in ((480, 640), (680, 1200)):
        for scale in (1, 2):
            row, m, sheet = time_passes(H, W, scale, dev, a.reps)
            rows.append(row)
            if (H, W, scale) == (480, 640, 2):
                jpeg = time_jpeg(sheet, H, W)
    keyframe, host_maps = time_keyframe(dev)
    figure = time_matplotlib(host_maps)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump({"device": torch.cuda.get_device_name(0), "reps": a.reps, "passes": rows, "jpeg_480x640_scale2": jpeg,
                       "keyframe_480x640": keyframe, "matplotlib_480x640": figure}, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
