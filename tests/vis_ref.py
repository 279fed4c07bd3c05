"""The contact sheet of glorie_slam_amd/visualizer.py restated in float32 numpy (include/glorie_hip.h states it; reference:
src/utils/Visualizer.py:118-203): the three ranges, the twelve panels, the layout and to_rgb8.  test_vis_ref.py pins
this file to matplotlib itself, test_gpu_vis.py and test_gpu_mapping_vis.py hold the kernels to it bit for bit."""
import numpy as np

F = np.float32
MAP_KEYS = ("render_depth", "depth", "color", "gt_color", "droid_depth", "proj_depth", "valid_ray_count",
            "sparse_proj_depth", "mono_depth")


def f32(a):
    return np.ascontiguousarray(np.asarray(a), dtype=np.float32)


def depth_residual(render_depth, depth):
    """min(|render_depth - depth|, 0.2) with a NaN kept, 0 where render_depth == 0"""
    rd, d = f32(render_depth), f32(depth)
    with np.errstate(invalid="ignore"):
        r = np.abs(rd - d)
        r = np.where(r > F(0.2), F(0.2), r)
    return np.where(rd == 0, F(0), r).astype(F)


def _finite_range(v):
    v = v[np.isfinite(v)]
    if v.size == 0:
        return F(0), F(0)
    return F(v.min()) + F(0), F(v.max()) + F(0)                 # (+ 0: a zero is +0)


def ranges(maps):
    """float32 [4]: (max droid_depth, min and max of the depth residual, 0), non-finite values skipped, [0, 0] of nothing"""
    dmax = _finite_range(f32(maps["droid_depth"]).reshape(-1))[1]
    rmin, rmax = _finite_range(depth_residual(maps["render_depth"], maps["depth"]).reshape(-1))
    return np.array([dmax, rmin, rmax, 0], dtype=F)


def colormap(v, vmin, vmax, table):
    """scalar map [..] -> uint8 [..,3]: t = (v - vmin) / (vmax - vmin) in float32 (0 when vmin == vmax), entry
    clamp(trunc(256 t), 0, 255) (NaN t: 0); a non-finite v is white"""
    v, vmin, vmax = f32(v), F(vmin), F(vmax)
    with np.errstate(all="ignore"):
        t = np.zeros_like(v) if vmin == vmax else ((v - vmin) / (vmax - vmin)).astype(F)
        f = (t * F(256)).astype(F)
        idx = np.trunc(np.where(f > 0, np.minimum(f, F(255)), F(0))).astype(np.int64)     # (NaN > 0 is false: entry 0)
    out = np.asarray(table, np.uint8)[idx]
    out[~np.isfinite(v)] = 255
    return out


def level(x):
    """trunc(255 clamp(x, 0, 1)) as uint8, NaN -> 0"""
    x = f32(x)
    with np.errstate(invalid="ignore"):
        c = np.where(x > 0, np.where(x < 1, x, F(1)), F(0)).astype(F)
    return np.trunc(c * F(255)).astype(np.uint8)


def round_level(color):
    """torch.round(color * 255) / 255 in float32 (ties to even)"""
    with np.errstate(invalid="ignore", over="ignore"):
        return (np.rint(f32(color) * F(255)) / F(255)).astype(F)


def panels(maps, n_surface, table):
    """the twelve full-resolution panels, uint8 [H,W,3] each, in the sheet's order"""
    m = {k: f32(maps[k]) for k in MAP_KEYS}
    dmax, rmin, rmax, _ = ranges(m)
    rd, c = m["render_depth"], round_level(m["color"])
    with np.errstate(invalid="ignore", over="ignore"):
        col_res = np.abs(m["gt_color"] - c)
    col_res = np.where((rd == 0)[..., None], F(0), col_res)
    return [colormap(rd, 0, dmax, table),
            colormap(m["depth"], 0, dmax, table),
            colormap(depth_residual(rd, m["depth"]), rmin, rmax, table),
            level(m["gt_color"]),
            level(c),
            level(col_res),
            colormap(m["droid_depth"], 0, dmax, table),
            colormap(m["proj_depth"], 0, dmax, table),
            colormap((m["proj_depth"] > 0).astype(F), 0, 1, table),
            colormap(m["valid_ray_count"], 0, n_surface, table),
            colormap(m["sparse_proj_depth"], 0, dmax, table),
            colormap(m["mono_depth"], 0, dmax, table)]


def panel_boxes(H, W, scale, gutter, title):
    """(y0, x0, ph, pw) of the twelve panels; ph = ceil(H / scale), pw = ceil(W / scale)"""
    ph, pw = (H + scale - 1) // scale, (W + scale - 1) // scale
    return [(gutter + r * (title + ph + gutter) + title, gutter + c * (pw + gutter), ph, pw)
            for r in range(4) for c in range(3)]


def sheet_size(H, W, scale, gutter, title):
    ph, pw = (H + scale - 1) // scale, (W + scale - 1) // scale
    return gutter + 4 * (title + ph + gutter), gutter + 3 * (pw + gutter)


def decimate(panel, scale):
    """panel pixel (y, x) shows source pixel (min(y scale + scale // 2, H-1), min(x scale + scale // 2, W-1))"""
    H, W = panel.shape[:2]
    ys = np.minimum(np.arange((H + scale - 1) // scale) * scale + scale // 2, H - 1)
    xs = np.minimum(np.arange((W + scale - 1) // scale) * scale + scale // 2, W - 1)
    return panel[ys][:, xs]


def contact_sheet(maps, n_surface, table, scale=2, gutter=4, title=12):
    """uint8 [SH,SW,3]: white, with the decimated panels in their boxes"""
    H, W = np.asarray(maps["render_depth"]).shape
    SH, SW = sheet_size(H, W, scale, gutter, title)
    sheet = np.full((SH, SW, 3), 255, np.uint8)
    for (y0, x0, ph, pw), p in zip(panel_boxes(H, W, scale, gutter, title), panels(maps, n_surface, table)):
        sheet[y0:y0 + ph, x0:x0 + pw] = decimate(p, scale)
    return sheet


def to_rgb8(color):
    """saturate(rint(255 x)) as uint8, ties to even, NaN -> 0"""
    with np.errstate(invalid="ignore", over="ignore"):
        r = np.rint(f32(color) * F(255))
        return np.where(r >= 255, 255, np.where(r > 0, r, 0)).astype(np.uint8)
