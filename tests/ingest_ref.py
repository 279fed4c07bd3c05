"""numpy restatement of the frame ingest (glorie_slam_amd/ingest.py, csrc/ingest.hip) as the definition has it: two
whole-image passes in int64 - undistort, then resize - followed by the crop, the channel swap and level / 255; the depth
path; the intrinsics.  The tables are built here on their own, per pixel / per column, not taken from the package.

Not a test module: tests/test_ingest_ref.py pins it by properties, the GPU tests compare the kernels with it bit for bit.
"""
import math

import numpy as np


def cam_block(H, W, H_out, W_out, H_edge=0, W_edge=0, fx=45.0, fy=44.0, cx=25.7, cy=18.2, distortion=None,
              png_depth_scale=None):
    cam = dict(H=H, W=W, fx=fx, fy=fy, cx=cx, cy=cy, H_out=H_out, W_out=W_out, H_edge=H_edge, W_edge=W_edge)
    if distortion is not None:
        cam["distortion"] = list(distortion)
    if png_depth_scale is not None:
        cam["png_depth_scale"] = png_depth_scale
    return cam


# ---- undistort stage --------------------------------------------------------------------------------------------------
def remap_positions(H, W, fx, fy, cx, cy, dist):
    """(ix, iy) int64 [H,W]: round-half-even of 32 x the distorted position of pixel (u, v), float64, pixel by pixel"""
    dist = [float(c) for c in dist]
    if len(dist) not in (4, 5, 8):
        raise ValueError(len(dist))
    k1, k2, p1, p2 = dist[:4]
    k3 = dist[4] if len(dist) > 4 else 0.0
    k4, k5, k6 = dist[5:8] if len(dist) > 5 else (0.0, 0.0, 0.0)
    ix = np.zeros((H, W), np.int64)
    iy = np.zeros((H, W), np.int64)
    for v in range(H):
        for u in range(W):
            x = (u - cx) / fx
            y = (v - cy) / fy
            r2 = x * x + y * y
            kr = (1 + ((k3 * r2 + k2) * r2 + k1) * r2) / (1 + ((k6 * r2 + k5) * r2 + k4) * r2)
            xd = x * kr + 2 * p1 * x * y + p2 * (r2 + 2 * x * x)
            yd = y * kr + p1 * (r2 + 2 * y * y) + 2 * p2 * x * y
            ix[v, u] = round(32 * (xd * fx + cx))           # Python's round: half to even
            iy[v, u] = round(32 * (yd * fy + cy))
    return ix, iy


def undistort(img, ix, iy):
    """img uint8 [H,W,C] -> uint8 [H,W,C]: (sum w p + 512) >> 10 over the 2 x 2 taps at (ix >> 5, iy >> 5), zero outside"""
    H, W, C = img.shape
    pad = np.zeros((H + 2, W + 2, C), np.int64)             # a zero frame one pixel wide: the taps just outside
    pad[1:-1, 1:-1] = img
    x0, y0 = ix >> 5, iy >> 5
    a, b = (ix & 31)[..., None], (iy & 31)[..., None]

    def tap(x, y):
        inside = (x >= -1) & (x <= W) & (y >= -1) & (y <= H)
        px = pad[np.clip(y, -1, H) + 1, np.clip(x, -1, W) + 1]
        return np.where(inside[..., None], px, 0)

    acc = ((32 - a) * (32 - b) * tap(x0, y0) + a * (32 - b) * tap(x0 + 1, y0)
           + (32 - a) * b * tap(x0, y0 + 1) + a * b * tap(x0 + 1, y0 + 1))
    return ((acc + 512) >> 10).astype(np.uint8)


# ---- resize stage -----------------------------------------------------------------------------------------------------
def resize_coords(n_src, n_dst):
    """per destination index: (s, f) with f float32 in [0,1) - the source coordinate after the clamps - and (a0, a1)"""
    s_all, f_all, a0_all, a1_all = [], [], [], []
    for d in range(n_dst):
        f = np.float32((d + 0.5) * (n_src / n_dst) - 0.5)
        s = int(math.floor(f))
        f = np.float32(f - np.float32(s))
        if s < 0:
            s, f = 0, np.float32(0)
        if s >= n_src - 1:
            s, f = n_src - 1, np.float32(0)
        a1 = int(np.rint(np.float32(2048) * f))
        a0 = int(np.rint(np.float32(2048) * np.float32(np.float32(1) - f)))
        s_all.append(s), f_all.append(f), a0_all.append(a0), a1_all.append(a1)
    return (np.array(s_all, np.int64), np.array(f_all, np.float32), np.array(a0_all, np.int64),
            np.array(a1_all, np.int64))


def resize(img, H_res, W_res):
    """img uint8 [H,W,C] -> uint8 [H_res,W_res,C]: the horizontal pass with 11-bit weights, then the vertical one"""
    H, W, _ = img.shape
    p = img.astype(np.int64)
    xs, _, xa0, xa1 = resize_coords(W, W_res)
    ys, _, yb0, yb1 = resize_coords(H, H_res)
    rows = p[:, xs] * xa0[None, :, None] + p[:, np.minimum(xs + 1, W - 1)] * xa1[None, :, None]      # [H,W_res,C]
    r0, r1 = rows[ys] >> 4, rows[np.minimum(ys + 1, H - 1)] >> 4
    out = (((yb0[:, None, None] * r0) >> 16) + ((yb1[:, None, None] * r1) >> 16) + 2) >> 2
    assert out.min() >= 0 and out.max() <= 255
    return out.astype(np.uint8)


def resize_float64(img, H_res, W_res):
    """the float64 bilinear value at the same float32 source coordinates (what the fixed-point stage approximates)"""
    H, W, _ = img.shape
    p = img.astype(np.float64)
    xs, xf, _, _ = resize_coords(W, W_res)
    ys, yf, _, _ = resize_coords(H, H_res)
    xf, yf = xf.astype(np.float64)[None, :, None], yf.astype(np.float64)[:, None, None]
    rows = p[:, xs] * (1 - xf) + p[:, np.minimum(xs + 1, W - 1)] * xf
    return rows[ys] * (1 - yf) + rows[np.minimum(ys + 1, H - 1)] * yf


# ---- the whole path ---------------------------------------------------------------------------------------------------
def color(frames, cam, swap_rb=False):
    """frames uint8 [B,H,W,3] or [H,W,3] -> float32 [B,3,H_out,W_out]"""
    frames = np.asarray(frames)
    if frames.ndim == 3:
        frames = frames[None]
    H, W = cam["H"], cam["W"]
    assert frames.dtype == np.uint8 and frames.shape[1:] == (H, W, 3)
    he, we = cam.get("H_edge", 0), cam.get("W_edge", 0)
    H_res, W_res = cam["H_out"] + 2 * he, cam["W_out"] + 2 * we
    pos = None
    if cam.get("distortion") is not None:
        pos = remap_positions(H, W, cam["fx"], cam["fy"], cam["cx"], cam["cy"], cam["distortion"])
    out = []
    for img in frames:
        if pos is not None:
            img = undistort(img, *pos)
        lv = resize(img, H_res, W_res)[he:H_res - he, we:W_res - we]
        if swap_rb:
            lv = lv[..., ::-1]
        out.append((lv.astype(np.float32) / np.float32(255)).transpose(2, 0, 1))
    return np.ascontiguousarray(np.stack(out))


def nearest_index(n_src, n_dst):
    scale = np.float32(n_src) / np.float32(n_dst)
    return np.array([min(int(math.floor(np.float32(np.float32(d) * scale))), n_src - 1) for d in range(n_dst)], np.int64)


def depth(raw, cam):
    """raw [B,H,W] or [H,W], uint16 or float32 -> float32 [B,H_out,W_out]"""
    raw = np.asarray(raw)
    if raw.ndim == 2:
        raw = raw[None]
    he, we = cam.get("H_edge", 0), cam.get("W_edge", 0)
    H_res, W_res = cam["H_out"] + 2 * he, cam["W_out"] + 2 * we
    yi = nearest_index(cam["H"], H_res)[he:H_res - he]
    xi = nearest_index(cam["W"], W_res)[we:W_res - we]
    picked = raw[:, yi][:, :, xi].astype(np.float32)
    return np.ascontiguousarray(picked / np.float32(cam.get("png_depth_scale", 1.0)))


def intrinsic(cam):
    """get_intrinsic in float32: the four numbers are float32, each factor a Python double rounded to float32 on use"""
    he, we = cam.get("H_edge", 0), cam.get("W_edge", 0)
    H_res, W_res = cam["H_out"] + 2 * he, cam["W_out"] + 2 * we
    sx, sy = np.float32(W_res / cam["W"]), np.float32(H_res / cam["H"])
    k = np.array([np.float32(cam["fx"]) * sx, np.float32(cam["fy"]) * sy, np.float32(cam["cx"]) * sx,
                  np.float32(cam["cy"]) * sy], np.float32)
    if we > 0:
        k[2] = k[2] - np.float32(we)
    if he > 0:
        k[3] = k[3] - np.float32(he)
    return k
