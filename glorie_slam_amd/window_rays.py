"""The rays of one training iteration over a window of keyframes in one launch (csrc/window_rays.hip; reference:
src/mapper.py:437-466 gathers them frame by frame, ray convention src/utils/common.py:39-54).

`SequenceRunner._window_rays` composes a window's rays from one `_keyframe_rays` call per frame (about ten torch
launches each) and four concatenations: fine for the 5 frames of a mapping window, not for the final refinement, whose
window is every mapped keyframe.  `WindowTable` uploads the window's depth-map, image and radius-map pointers and its
matrices once; `window_rays` then serves every iteration with one launch, no host synchronisation and nothing sized by
the data.
"""
import torch

from . import _lib as L


class WindowTable:
    """device tables of a window of M keyframes: depths M x [H,W], images M x [3,H,W] (channels_first) or [H,W,3], c2ws
    [M,4,4] (or [M,3,4]) in the renderer's OpenGL convention, radius_maps None or M x [H,W].  Maps that are not
    contiguous float32 are copied; the table holds references to what its pointers name.  Build it once per window
    (one host-to-device copy for the three pointer tables)."""

    def __init__(self, depths, images, c2ws, radius_maps=None, channels_first=True):
        depths, images = list(depths), list(images)
        radius_maps = list(radius_maps) if radius_maps is not None else None
        M = len(depths)
        if M == 0:
            raise ValueError("WindowTable needs at least one frame")
        if len(images) != M or (radius_maps is not None and len(radius_maps) != M):
            raise ValueError(f"WindowTable: {M} depth maps, {len(images)} images"
                             + (f", {len(radius_maps)} radius maps" if radius_maps is not None else ""))
        if not torch.is_tensor(c2ws):
            c2ws = torch.stack(list(c2ws))
        tensors = depths + images + (radius_maps or []) + [c2ws]
        for t in tensors:
            if not torch.is_tensor(t) or not t.is_floating_point():
                raise ValueError("WindowTable takes floating-point tensors")
        dev = depths[0].device
        if dev.type != "cuda" or any(t.device != dev for t in tensors):
            raise ValueError("WindowTable: every map and the matrices must live on one GPU")
        if depths[0].dim() != 2:
            raise ValueError(f"depth maps must be [H,W], got {tuple(depths[0].shape)}")
        H, W = depths[0].shape
        self.channels_first = bool(channels_first)
        want = (3, H, W) if self.channels_first else (H, W, 3)
        for d in depths + (radius_maps or []):
            if tuple(d.shape) != (H, W):
                raise ValueError(f"depth and radius maps must share [{H},{W}], got {tuple(d.shape)}")
        for im in images:
            if tuple(im.shape) != want:
                raise ValueError(f"images must be {want}, got {tuple(im.shape)}")
        if c2ws.dim() != 3 or c2ws.shape[0] != M or tuple(c2ws.shape[1:]) not in ((4, 4), (3, 4)):
            raise ValueError(f"c2ws must be [{M},4,4] or [{M},3,4], got {tuple(c2ws.shape)}")
        self.H, self.W, self.device = int(H), int(W), dev
        self.depths = [L.f32(d) for d in depths]
        self.images = [L.f32(im) for im in images]
        self.radius_maps = [L.f32(r) for r in radius_maps] if radius_maps is not None else None
        self.c2ws = L.homogeneous(c2ws)
        rows = [self.depths, self.images] + ([self.radius_maps] if self.radius_maps is not None else [])
        self._tables = torch.tensor([[t.data_ptr() for t in row] for row in rows], dtype=torch.int64).to(dev)

    def __len__(self):
        return len(self.depths)


def window_rays(table, ii, jj, per, fx, fy, cx, cy, const_radius=None):
    """ii, jj int64 [M * per] on the table's device, frame-major (ray r reads pixel column ii[r], row jj[r] of window slot
    r // per; the draw must lie inside the image) -> (rays_o [N,3], rays_d [N,3], depth [N], color [N,3], radius [N]).
    radius: gathered from the table's radius maps, else `const_radius` for every ray, else None"""
    if not isinstance(table, WindowTable):
        raise ValueError("window_rays takes a WindowTable")
    L.need_cuda(ii, jj)
    M, per = len(table), int(per)
    N = M * per
    if per < 0 or ii.shape != (N,) or jj.shape != (N,) or ii.dtype != torch.int64 or jj.dtype != torch.int64:
        raise ValueError(f"ii, jj must be int64 [{N}] ({M} frames x {per} rays)")
    if ii.device != table.device or jj.device != table.device:
        raise ValueError("ii, jj must live on the table's device")
    dev = table.device
    ii, jj = ii.contiguous(), jj.contiguous()
    rays_o = torch.empty(N, 3, dtype=torch.float32, device=dev)
    rays_d = torch.empty(N, 3, dtype=torch.float32, device=dev)
    depth = torch.empty(N, dtype=torch.float32, device=dev)
    color = torch.empty(N, 3, dtype=torch.float32, device=dev)
    has_maps = table.radius_maps is not None
    want = has_maps or const_radius is not None
    radius = torch.empty(N, dtype=torch.float32, device=dev) if want else None
    t = table._tables
    L.check(L.load().glorie_window_rays(L.ptr(t[0]), L.ptr(t[1]), L.ptr(t[2]) if has_maps else None, L.ptr(table.c2ws), M,
                                        per, int(table.channels_first), table.H, table.W, float(fx), float(fy),
                                        float(cx), float(cy), L.ptr(ii), L.ptr(jj),
                                        float(const_radius) if const_radius is not None else 0.0, int(want),
                                        L.ptr(rays_o), L.ptr(rays_d), L.ptr(depth), L.ptr(color), L.ptr(radius),
                                        L.stream_ptr(dev)), "glorie_window_rays")
    return rays_o, rays_d, depth, color, radius
