"""Timing of the correlation adjoints (csrc/corr_bwd.hip).

    python tools/time_corr_bwd.py [--edges 36 75] [--repeats 7] [--json profiles/corr_bwd_time.json]

Device times from events around `--inner` back-to-back calls, median of --repeats after a warm-up of every shape.
  index / pyramid backward   at --edges edges of 60 x 80, fp16 and fp32, ALTERNATED in the same process with a plain zero_() of
               the same tensors - the floor any implementation pays, since the launch overwrites every element.  Reported: the
               ratio to the fill and the achieved bytes/s on the algorithmic bytes (the volume gradients written once, the
               lookup gradients and coordinates read once).
  alt-corr backward   at --alt-edges edges of 30 x 40, C = 128, the four levels of AltCorrBlock, with smooth coordinates (every
               4 x 4 tile pre-sums over its box) and with scattered ones (per-tap atomic rows).  Reported: the atomic rows issued
               (counted on the host from the kernel's box rule), the added atomic bytes per second against the chip-wide rate
               of global float atomics, and the reduction in atomic rows by the pre-sum.
  torch        autograd through the pure-torch composition of the same lookups (gathers on the all-pairs volume) in the same
               process.
Figures to report, not gates."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

from glorie_slam_amd import droid_backends as db  # noqa: E402
import corr_bwd_ref as RB  # noqa: E402   (the one Python copy of the kernel's box rule and of the pure-torch lookup)

ATOMIC_RATE = 1.3e12          # chip-wide added bytes per second of global float atomics (MI355X)


def timed_ms(fn, inner):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(inner):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / inner


def alternate(fns, repeats, inner):
    """median ms of each of `fns`, measured in turn `repeats` times after one warm-up round"""
    for f in fns:
        f()
    torch.cuda.synchronize()
    t = [[] for _ in fns]
    for _ in range(repeats):
        for k, f in enumerate(fns):
            t[k].append(timed_ms(f, inner))
    return [float(np.median(v)) for v in t], [[float(min(v)), float(max(v))] for v in t]


def torch_lookup(vol, coords, radius=3):
    """pure-torch lookup (tests/corr_bwd_ref.py::lookup_torch): vol [N, h1, w1, h2, w2], coords [N, 2, h1, w1] -> [N, 49, h1, w1]"""
    return RB.lookup_torch(vol, coords, radius).reshape(vol.shape[0], -1, vol.shape[1], vol.shape[2])


def smooth_coords(N, h, w, dev, seed=0):
    g = torch.Generator(device="cpu").manual_seed(seed)
    y, x = torch.meshgrid(torch.arange(h, dtype=torch.float32), torch.arange(w, dtype=torch.float32), indexing="ij")
    shift = torch.rand(N, 2, 1, 1, generator=g) * 8 - 4
    return (torch.stack([x, y])[None] * 1.02 + shift).contiguous().to(dev)


def scattered_coords(N, h, w, dev, seed=0):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return torch.stack([torch.rand(N, h, w, generator=g) * (w + 6) - 3, torch.rand(N, h, w, generator=g) * (h + 6) - 3], 1).to(dev)


def time_pyramid(N, dtype, repeats, inner, dev, with_torch):
    h, w, radius = 60, 80, 3
    esize = 2 if dtype == torch.float16 else 4
    coords = smooth_coords(N, h, w, dev)
    grad = torch.randn(N, 4 * 49, h, w, device=dev).to(dtype)
    shapes = [(N, h, w, h >> l, w >> l) for l in range(4)]
    levels = [torch.empty(s, dtype=dtype, device=dev) for s in shapes]
    vol0 = levels[0]
    g0 = grad[:, :49].contiguous()

    def fill_all():
        for v in levels:
            v.zero_()

    res = {}
    (t_idx, t_fill0), spread = alternate([lambda: db.corr_index_backward(vol0, coords, g0, radius), vol0.zero_], repeats, inner)
    b_idx = vol0.numel() * esize + g0.numel() * esize + coords.numel() * 4
    res["index"] = dict(kernel_ms=t_idx, fill_ms=t_fill0, ratio_to_fill=t_idx / t_fill0, bytes=b_idx,
                        GBps=b_idx / t_idx / 1e6, fill_GBps=vol0.numel() * esize / t_fill0 / 1e6, min_max_ms=spread)
    (t_pyr, t_fill), spread = alternate([lambda: db.corr_lookup_pyramid_backward(shapes, coords, grad, radius), fill_all],
                                        repeats, inner)
    b_pyr = sum(v.numel() for v in levels) * esize + grad.numel() * esize + coords.numel() * 4
    res["pyramid"] = dict(kernel_ms=t_pyr, fill_ms=t_fill, ratio_to_fill=t_pyr / t_fill, bytes=b_pyr,
                          GBps=b_pyr / t_pyr / 1e6, fill_GBps=sum(v.numel() for v in levels) * esize / t_fill / 1e6,
                          min_max_ms=spread)
    if with_torch:
        vols = [torch.zeros(s, dtype=dtype, device=dev, requires_grad=True) for s in shapes]
        out = torch.cat([torch_lookup(v, coords / 2 ** l) for l, v in enumerate(vols)], 1)
        run = lambda: torch.autograd.grad(out, vols, grad, retain_graph=True)
        (t_torch,), _ = alternate([run], 2, 1)
        res["torch_autograd_pyramid_ms"] = t_torch
        del out, vols
    return res


def atomic_rows(coords, H2, W2, C, radius=3):
    """(in-bounds taps, atomic rows the kernel issues, share of boxed tiles) for coords [B, H, W, 2] (S = 1); the branch of
    every tile comes from tests/corr_bwd_ref.py::altcorr_bwd_plan"""
    c = coords.cpu().numpy()
    B, H, W, _ = c.shape
    T = RB.ALT_TILE
    ox = np.floor(c[..., 0]).astype(np.int64) - radius
    oy = np.floor(c[..., 1]).astype(np.int64) - radius
    k = np.arange(2 * radius + 2)
    tx, ty = ox[..., None, None] + k[:, None], oy[..., None, None] + k[None, :]           # [B, H, W, ix, iy]
    inb = (tx >= 0) & (tx < W2) & (ty >= 0) & (ty < H2)
    taps = int(inb.sum())
    boxed = RB.altcorr_bwd_plan(c[:, None], C, radius)[:, 0] == RB.BOXED                  # [B, tiles_y, tiles_x]
    ntx = boxed.shape[2]
    tile = (np.arange(H)[:, None] // T) * ntx + np.arange(W)[None, :] // T
    boxed_px = boxed.reshape(B, -1)[:, tile.reshape(-1)].reshape(B, H, W)
    per_tap = int(inb[~boxed_px].sum())
    key = ((np.arange(B)[:, None, None] * boxed[0].size + tile[None])[..., None, None] * (H2 * W2) + ty * W2 + tx)
    rows_boxed = int(np.unique(key[inb & boxed_px[..., None, None]]).size)
    return taps, per_tap + rows_boxed, float(boxed.mean())


def time_altcorr(N, kind, repeats, inner, dev, with_torch):
    H, W, C, radius = 30, 40, 128, 3
    f = torch.randn(N, C, H, W, device=dev) * 0.25
    f1 = f.permute(0, 2, 3, 1).contiguous()
    c0 = (smooth_coords if kind == "smooth" else scattered_coords)(N, H, W, dev).permute(0, 2, 3, 1).contiguous()
    res = {"levels": []}
    total_ms = total_rows = total_taps = 0
    pooled = f
    fwd_inputs = []
    for l in range(4):
        f2 = pooled.permute(0, 2, 3, 1).contiguous()
        coords = (c0 / 2 ** l)[:, None].contiguous()
        grad = torch.randn(N, 1, 49, H, W, device=dev)
        (t,), spread = alternate([lambda: db.altcorr_backward(f1, f2, coords, grad, radius)], repeats, inner)
        taps, rows, share = atomic_rows(coords[:, 0], H >> l, W >> l, C)
        res["levels"].append(dict(level=l, ms=t, min_max_ms=spread[0], inbounds_taps=taps, atomic_rows=rows, boxed_tile_share=share,
                                  atomic_bytes=rows * C * 4, atomic_GBps=rows * C * 4 / t / 1e6,
                                  share_of_chip_atomic_rate=rows * C * 4 / (t * 1e-3) / ATOMIC_RATE,
                                  row_reduction=taps / max(rows, 1)))
        total_ms, total_rows, total_taps = total_ms + t, total_rows + rows, total_taps + taps
        fwd_inputs.append((f2, coords, grad))
        if l < 3:
            pooled = torch.nn.functional.avg_pool2d(pooled, 2, stride=2)
    res.update(total_ms=total_ms, atomic_rows=total_rows, inbounds_taps=total_taps, row_reduction=total_taps / max(total_rows, 1),
               floor_ms_at_chip_atomic_rate=total_rows * C * 4 / ATOMIC_RATE * 1e3)
    if with_torch:
        a = f1.clone().requires_grad_(True)
        leaves = [a]
        outs = []
        for f2, coords, _ in fwd_inputs:
            b = f2.clone().requires_grad_(True)
            leaves.append(b)
            vol = torch.einsum("bhwc,byxc->bhwyx", a, b)
            outs.append(torch_lookup(vol, coords[:, 0].permute(0, 3, 1, 2)))
        out = torch.cat(outs, 1)
        cot = torch.cat([g[:, 0] for _, _, g in fwd_inputs], 1)
        (t_torch,), _ = alternate([lambda: torch.autograd.grad(out, leaves, cot, retain_graph=True)], 2, 1)
        res["torch_autograd_ms"] = t_torch
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--edges", type=int, nargs="+", default=[36, 75])
    ap.add_argument("--alt-edges", type=int, default=150)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--torch-edges", type=int, default=36, help="largest edge count at which the torch composition is timed")
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_corr_bwd.py measures on the GPU; none found")
    dev = torch.device("cuda:0")
    out = {"device": torch.cuda.get_device_name(dev), "repeats": args.repeats, "inner": args.inner, "index_pyramid": {},
           "altcorr": {}}
    for N in args.edges:
        for dtype, name in ((torch.float16, "f16"), (torch.float32, "f32")):
            r = time_pyramid(N, dtype, args.repeats, args.inner, dev, N <= args.torch_edges)
            out["index_pyramid"][f"{N}_{name}"] = r
            print(N, name, json.dumps(r), flush=True)
            torch.cuda.empty_cache()
    for kind in ("smooth", "scattered"):
        r = time_altcorr(args.alt_edges, kind, args.repeats, args.inner, dev, True)
        out["altcorr"][kind] = r
        print("altcorr", kind, json.dumps(r), flush=True)
        torch.cuda.empty_cache()
    if args.json:
        with open(args.json, "w") as fh:
            json.dump(out, fh, indent=1)


if __name__ == "__main__":
    main()
