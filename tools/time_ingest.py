"""Device time of the frame ingest (glorie_slam_amd/ingest.py, csrc/ingest.hip) against the torch composition a caller
would otherwise write, in the same process.

    python tools/time_ingest.py [--reps 200] [--json profiles/ingest_time.json]

  cases     480x640 with the TUM freiburg1 distortion -> 384x512 (edges 8 / 8), and 680x1200 -> 320x640, each at B = 1, 16
  kernel    IngestPlan.color on uint8 frames that are already on the device: one launch
  torch     uint8 -> float, grid_sample on a precomputed grid (the undistortion; skipped without one), bilinear
            interpolate, crop, / 255.  Float arithmetic: close to the kernel's result, not equal to it (the largest
            difference in levels is printed)
  host      the numpy restatement (tests/ingest_ref.py) of one frame plus the upload of its float32 result: what the
            reference's host path costs in spirit (cv2 is not available to time)
  The two device variants alternate call by call; every call sits between its own pair of events; medians are reported.
  bytes/s is over the algorithmic bytes: the source read once plus the output written once.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

TUM_FR1 = [0.2624, -0.9531, -0.0054, 0.0026, 1.1633]
CASES = {
    "tum_480x640_to_384x512": dict(H=480, W=640, fx=517.3, fy=516.5, cx=318.6, cy=255.3, distortion=TUM_FR1,
                                   H_out=384, W_out=512, H_edge=8, W_edge=8),
    "replica_680x1200_to_320x640": dict(H=680, W=1200, fx=600.0, fy=600.0, cx=599.5, cy=339.5, H_out=320, W_out=640,
                                        H_edge=0, W_edge=0),
}


def alternate(fns, reps, warmup=10):
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


def torch_composition(plan, dev):
    """the float path on the device: -> callable(frames uint8 [B,H,W,3]) -> float32 [B,3,H_out,W_out]"""
    H, W, he, we = plan.H, plan.W, plan.H_edge, plan.W_edge
    H_res, W_res = plan.H_out + 2 * he, plan.W_out + 2 * we
    grid = None
    if plan.map is not None:
        pos = plan.map.float() / 32.0                                   # [H,W,2] source pixel positions
        grid = torch.stack([(pos[..., 0] + 0.5) * (2.0 / W) - 1.0, (pos[..., 1] + 0.5) * (2.0 / H) - 1.0], -1)[None]

    def run(frames):
        x = frames.permute(0, 3, 1, 2).float()
        if grid is not None:
            x = F.grid_sample(x, grid.expand(x.shape[0], -1, -1, -1), mode="bilinear", padding_mode="zeros",
                              align_corners=False)
        x = F.interpolate(x, size=(H_res, W_res), mode="bilinear", align_corners=False)
        return x[:, :, he:H_res - he, we:W_res - we] / 255.0

    return run


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    from glorie_slam_amd.ingest import IngestPlan
    import ingest_ref as R
    dev = torch.device("cuda:0")
    rows = []
    for name, cam in CASES.items():
        plan = IngestPlan(cam, dev)
        ref = torch_composition(plan, dev)
        host_frame = np.random.default_rng(0).integers(0, 256, (cam["H"], cam["W"], 3), dtype=np.uint8)
        he, we = cam["H_edge"], cam["W_edge"]
        H_res, W_res = cam["H_out"] + 2 * he, cam["W_out"] + 2 * we
        pos = (R.remap_positions(cam["H"], cam["W"], cam["fx"], cam["fy"], cam["cx"], cam["cy"], cam["distortion"])
               if "distortion" in cam else None)                        # per camera, not per frame: not timed
        t0 = time.perf_counter()
        mid = R.undistort(host_frame, *pos) if pos is not None else host_frame
        lv = R.resize(mid, H_res, W_res)[he:H_res - he, we:W_res - we]
        host = np.ascontiguousarray((lv.astype(np.float32) / np.float32(255)).transpose(2, 0, 1))[None]
        t1 = time.perf_counter()
        torch.from_numpy(host).to(dev)
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        for B in (1, 16):
            g = torch.Generator().manual_seed(B)
            frames = torch.randint(0, 256, (B, cam["H"], cam["W"], 3), generator=g, dtype=torch.uint8).to(dev)
            ours, theirs = plan.color(frames), ref(frames)
            diff = float((ours - theirs).abs().max()) * 255.0
            ms = alternate({"kernel": lambda: plan.color(frames), "torch": lambda: ref(frames)}, a.reps)
            nbytes = frames.numel() + ours.numel() * 4
            row = dict(case=name, B=B, kernel_us=1e3 * ms["kernel"], torch_us=1e3 * ms["torch"],
                       algorithmic_bytes=nbytes, kernel_GBps=nbytes / (ms["kernel"] * 1e-3) / 1e9,
                       max_level_difference_to_torch=diff, host_restatement_ms=1e3 * (t1 - t0),
                       host_upload_float32_ms=1e3 * (t2 - t1))
            rows.append(row)
            print(f"{name} B={B}: kernel {row['kernel_us']:.1f} us, torch composition {row['torch_us']:.1f} us "
                  f"({row['torch_us'] / row['kernel_us']:.2f}x), {row['kernel_GBps']:.1f} GB/s on {nbytes} algorithmic "
                  f"bytes; differs from the float composition by at most {diff:.2f} level")
        print(f"{name}: host restatement of one frame {1e3 * (t1 - t0):.1f} ms (numpy, not cv2), float32 upload "
              f"{1e3 * (t2 - t1):.2f} ms")
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump({"device": torch.cuda.get_device_name(0), "reps": a.reps, "rows": rows}, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
