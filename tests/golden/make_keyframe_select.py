"""Pins of the mapper's keyframe selection against the imported reference (this container only; the reference never
travels):

    python tests/golden/make_keyframe_select.py

  keyframe_select.npz
    frustum   Mapper.get_mask_from_c2w (src/mapper.py:126-174) called unbound on CPU with a namespace `self` (H, W,
              intrinsics, frustum_edge, an `npc` whose cloud_pos() returns the points): the ascending indices it returns
              for 2863 points around one camera and a 96x128 depth map with a zero-depth hole - points in front, beyond
              depth + 0.5, behind the camera, outside each edge, inside the -4 band (their samples read 0 and take the
              maximum sample), on the hole.  Twice: frustum_edge -4 (the shipped config) and +6.
    overlap   Mapper.keyframe_selection_overlap (:176-244) with keyframe_dict = 6 keyframes (identical to the current
              view, shifted, half out of view, tilted, turned away: 0 overlap, far aside) whose poses a namespace `video`
              returns from get_pose: the rays get_samples drew (recorded by a wrapper around it), the percent_inside of
              every keyframe (recorded by shadowing `sorted` in the src.mapper namespace) and the selection, with
              np.random.permutation made the identity (the candidates in overlap order).  The current view's depth map is
              0 at every pixel whose samples would come within the margin of a decision: get_samples drops those draws.
  Every decision keeps >= 1e-2 px (and >= 1e-2 / 32 px from a 1/32-px rounding boundary of the depth sample) and 1e-3 in
  depth from its threshold in float64, so fp32 cannot flip it.

The only non-reference code executed inside the reference methods is the stand-in for cv2.remap (cv2 is not installed
here): `remap_standin`, a numpy restatement of INTER_LINEAR with BORDER_CONSTANT 0 - map coordinates rounded to 1/32 px as
cv2 does, neighbours outside the image read 0.  Every other module the import chain of src.mapper names and this
environment lacks becomes a module whose attributes are MagicMocks (never executed by these two methods).
The archive is written with fixed zip timestamps: re-running the script reproduces it bit for bit.
"""
import os
import sys
import types
from unittest import mock

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from make_pix_warp import import_mapper, rot, save_npz  # noqa: E402

OUT = os.path.dirname(os.path.abspath(__file__))

H, W = 96, 128
FX, FY, CX, CY = 80.0, 80.0, 63.5, 47.5
MARGIN_PX, MARGIN_Q, MARGIN_D = 1e-2, 1e-2, 1e-3
EDGES = (-4, 6)


def remap_standin(src, map_x, map_y, interpolation=None):
    """cv2.remap(src, map_x, map_y, INTER_LINEAR) for [n] float32 maps (BORDER_CONSTANT 0) -> [n, 1] float32"""
    src = np.asarray(src, np.float32)
    h, w = src.shape
    x = np.asarray(map_x, np.float32).reshape(-1)
    y = np.asarray(map_y, np.float32).reshape(-1)
    ok = np.isfinite(x) & np.isfinite(y)
    X = np.rint(np.where(ok, x, 0) * np.float32(32)).astype(np.int64)
    Y = np.rint(np.where(ok, y, 0) * np.float32(32)).astype(np.int64)
    x0, y0 = X >> 5, Y >> 5
    ax = ((X & 31) / np.float32(32)).astype(np.float32)
    ay = ((Y & 31) / np.float32(32)).astype(np.float32)
    one = np.float32(1)
    out = np.zeros(len(x), np.float32)
    for dx, dy, wgt in ((0, 0, (one - ay) * (one - ax)), (1, 0, (one - ay) * ax), (0, 1, ay * (one - ax)),
                        (1, 1, ay * ax)):
        xi, yi = x0 + dx, y0 + dy
        inb = ok & (xi >= 0) & (xi < w) & (yi >= 0) & (yi < h)
        out = out + np.where(inb, src[np.clip(yi, 0, h - 1), np.clip(xi, 0, w - 1)], np.float32(0)) * wgt
    return out.astype(np.float32).reshape(-1, 1)


def c2w_gl(R, t):
    M = np.eye(4)
    M[:3, :3], M[:3, 3] = R, t
    return M.astype(np.float32)


def depth_map(rng, base, hole):
    """smooth positive depth around `base`, quantised to 1/64, with a rectangular zero-depth hole"""
    low = torch.from_numpy(rng.uniform(-0.6, 0.6, (1, 1, H // 16, W // 16)))
    d = base + torch.nn.functional.interpolate(low, size=(H, W), mode="bilinear", align_corners=False)[0, 0].numpy()
    d = np.round(d * 64) / 64
    y0, y1, x0, x1 = hole
    d[y0:y1, x0:x1] = 0
    return d.astype(np.float32)


def _near_q(q):
    f = q * 32 - np.floor(q * 32)
    return np.abs(f - 0.5) < MARGIN_Q


def frustum_points(rng, c2w, depth, n):
    """n points from back-projected (u, v, -z) draws covering every branch of the selection; draws within a margin of a
    decision (for both edges) are redrawn"""
    sys.path.insert(0, os.path.dirname(OUT))
    from keyframe_select_ref import frustum_ref, remap_linear
    kinds = ["front", "beyond", "behind", "left", "right", "top", "bottom", "band", "hole"]
    pts = []
    while len(pts) < n:
        kind = kinds[len(pts) % len(kinds)]
        u, v = rng.uniform(1, W - 1), rng.uniform(1, H - 1)
        if kind == "left":
            u = rng.uniform(-30, -4.5)
        elif kind == "right":
            u = rng.uniform(W + 4.5, W + 30)
        elif kind == "top":
            v = rng.uniform(-30, -4.5)
        elif kind == "bottom":
            v = rng.uniform(H + 4.5, H + 30)
        elif kind == "band":
            if rng.uniform() < 0.5:
                u = rng.choice([rng.uniform(-3.9, -0.1), rng.uniform(W + 0.1, W + 3.9)])
            else:
                v = rng.choice([rng.uniform(-3.9, -0.1), rng.uniform(H + 0.1, H + 3.9)])
        elif kind == "hole":
            u, v = rng.uniform(61, 75), rng.uniform(31, 45)       # inside the hole: rows 30-46, cols 60-76 (main)
        s = float(remap_linear(depth, np.array([u]), np.array([v]))[0])
        t = {"front": rng.uniform(0.2, 1.0) * (s + 0.5), "beyond": s + 0.5 + rng.uniform(0.02, 1.0),
             "behind": -rng.uniform(0.1, 3.0)}.get(kind, rng.uniform(0.3, 7.0))
        z = -t                                                     # z = c + 1e-5
        c = z - 1e-5
        a = -(u * z - CX * c) / FX
        b = (v * z - CY * c) / FY
        X = (c2w.astype(np.float64) @ np.array([a, b, c, 1.0]))[:3]
        pts.append(X.astype(np.float32))
    pts = np.stack(pts)
    while True:                 # dropping a point can move the maximum sample: repeat until every point keeps its margin
        ok = np.ones(len(pts), bool)
        for edge in EDGES:
            _, dt = frustum_ref(pts, c2w, depth, FX, FY, CX, CY, H, W, edge)
            u, v = dt["u"], dt["v"]
            near = lambda x, t: np.abs(x - t) < MARGIN_PX
            ok &= ~(near(u, edge) | near(u, W - edge) | near(v, edge) | near(v, H - edge) | _near_q(u) | _near_q(v))
            ok &= (np.abs(dt["negz"]) >= MARGIN_D) & (np.abs(dt["negz"] - dt["depth"] - 0.5) >= MARGIN_D)
        if ok.all():
            return pts
        pts = pts[ok]


def run_frustum(Mapper, pts, c2w, depth, edge):
    self = types.SimpleNamespace(H=H, W=W, fx=FX, fy=FY, cx=CX, cy=CY, frustum_edge=edge, device="cpu",
                                 npc=types.SimpleNamespace(cloud_pos=lambda: torch.from_numpy(pts)))
    idx = Mapper.get_mask_from_c2w(self, torch.from_numpy(c2w), depth.copy())
    return np.asarray(idx, np.int64)


def overlap_depth(rng, c2w, kf_c2ws, n_samples):
    """the current view's depth with every pixel zeroed whose samples come within the margin of a decision in some
    keyframe (rays and samples computed in float32 as the reference does)"""
    from src.utils.common import get_rays_from_uv
    sys.path.insert(0, os.path.dirname(OUT))
    from keyframe_select_ref import project
    d = depth_map(rng, 3.0, (0, 0, 0, 0))
    d[:8, :] = 0                                                   # a band without depth: draws there are dropped
    j, i = np.meshgrid(np.arange(H, dtype=np.float32), np.arange(W, dtype=np.float32), indexing="ij")
    ro, rd = get_rays_from_uv(torch.from_numpy(i.reshape(-1)), torch.from_numpy(j.reshape(-1)), torch.from_numpy(c2w),
                              FX, FY, CX, CY, "cpu")
    dep = torch.from_numpy(d.reshape(-1, 1)).repeat(1, n_samples)
    t = torch.linspace(0.0, 1.0, steps=n_samples)
    z = dep * 0.8 * (1.0 - t) + (dep + 0.5) * t
    pts = (ro[..., None, :] + rd[..., None, :] * z[..., :, None]).reshape(-1, 3).numpy()
    bad = np.zeros(len(pts), bool)
    for kc in kf_c2ws:
        u, v, zz = project(kc, pts, FX, FY, CX, CY)
        near = lambda x, th: np.abs(x - th) < MARGIN_PX
        bad |= near(u, 20) | near(u, W - 20) | near(v, 20) | near(v, H - 20) | (np.abs(zz) < MARGIN_D)
    bad = bad.reshape(H * W, n_samples).any(1).reshape(H, W)
    d[bad] = 0
    return d


def run_overlap(m, c2w, depth, kf_c2ws, k, n_samples, pixels):
    rec = {}
    real_get_samples, real_sorted = m.get_samples, sorted

    def get_samples(*a, **kw):
        out = real_get_samples(*a, **kw)
        rec["rays_o"], rec["rays_d"], rec["depth"] = (x.numpy().astype(np.float32) for x in out[:3])
        return out

    def rec_sorted(seq, **kw):
        rec["percent"] = np.array([float(e["percent_inside"]) for e in seq])
        return real_sorted(seq, **kw)

    # video.get_pose returns the pose before the convention flip (mapper.py:217-218 flips it back)
    flip = np.diag([1.0, -1.0, -1.0, 1.0]).astype(np.float32)
    video = types.SimpleNamespace(get_pose=lambda i, dev: torch.from_numpy(kf_c2ws[i] @ flip))
    self = types.SimpleNamespace(H=H, W=W, fx=FX, fy=FY, cx=CX, cy=CY, device="cpu", video=video)
    kd = [{"video_idx": i} for i in range(len(kf_c2ws))]
    color = torch.zeros(H, W, 3)
    with mock.patch.object(m, "get_samples", get_samples), mock.patch.object(m, "sorted", rec_sorted, create=True), \
            mock.patch.object(np.random, "permutation", lambda x: np.asarray(x)):
        sel = m.Mapper.keyframe_selection_overlap(self, color, torch.from_numpy(depth), torch.from_numpy(c2w), kd, k,
                                                  N_samples=n_samples, pixels=pixels)
    rec["selected"] = np.asarray([int(s) for s in sel], np.int64)
    return rec


def main():
    m = import_mapper()
    m.cv2.remap = remap_standin
    rng = np.random.default_rng(20261016)
    out = dict(hw=np.array([H, W]), intrinsics=np.array([FX, FY, CX, CY], np.float32), edges=np.array(EDGES))

    # ---- frustum ----
    c2w = c2w_gl(rot(0.3, 0.1), [0.4, -0.2, 1.0])
    depth = depth_map(rng, 3.0, (30, 46, 60, 76))
    pts = frustum_points(rng, c2w, depth, 3000)            # 2863 after the margin filter
    out.update(frustum_points=pts, frustum_c2w=c2w, frustum_depth=depth)
    for edge in EDGES:
        idx = run_frustum(m.Mapper, pts, c2w, depth, edge)
        mask = np.zeros(len(pts), np.uint8)
        mask[idx] = 1
        out[f"frustum_mask_{edge}"] = mask
        print(f"frustum edge {edge}: {len(pts)} points, {len(idx)} kept")

    # ---- overlap ----
    S, pixels = 8, 200
    cur = c2w_gl(rot(0.0), [0.0, 0.0, 0.0])
    kfs = np.stack([cur,                                            # 0 identical
                    c2w_gl(rot(0.05), [0.3, 0.1, 0.0]),             # 1 shifted
                    c2w_gl(rot(0.45), [0.0, 0.0, 0.0]),             # 2 half out of view
                    c2w_gl(rot(np.pi), [0.0, 0.0, 0.0]),            # 3 turned away
                    c2w_gl(rot(-0.15, 0.1), [-0.2, 0.0, 0.4]),      # 4 shifted and tilted
                    c2w_gl(rot(0.0), [6.0, 0.0, 0.0])])             # 5 far aside: 0 overlap
    odepth = overlap_depth(rng, cur, kfs, S)
    torch.manual_seed(7)
    rec = run_overlap(m, cur, odepth, kfs, 3, S, pixels)
    out.update(overlap_c2w=cur, overlap_depth=odepth, overlap_c2ws=kfs, overlap_k=np.array(3),
               overlap_samples=np.array(S), overlap_pixels=np.array(pixels), overlap_rays_o=rec["rays_o"],
               overlap_rays_d=rec["rays_d"], overlap_ray_depth=rec["depth"], overlap_percent=rec["percent"],
               overlap_selected=rec["selected"])
    print("overlap: rays kept", len(rec["depth"]), "of", pixels, "percent", rec["percent"], "selected", rec["selected"])
    assert rec["percent"][3] == 0 and rec["percent"][5] == 0 and (rec["percent"][[0, 1, 2, 4]] > 0).all()
    assert len(rec["depth"]) < pixels
    path = os.path.join(OUT, "keyframe_select.npz")
    save_npz(path, out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
