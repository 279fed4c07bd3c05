"""Masked ray sampling and the depth gate of the per-keyframe mapping loop (csrc/map_sample.hip; reference:
src/mapper.py:427-431 draws every window frame's pixels among the pixels of its render mask, :474-482 keeps the rays whose
depth is at most min(10 median, 1.2 max)).

`ValidIndex` builds, once per window, the rank tables of every frame's valid pixels (depth > 0); `sample_window_rays`
then maps an iteration's draws in [0, 2^31) onto them and gathers the rays in one launch, and `depth_gate` forms the
reference's `inside_mask` as 1 / 0 weights with its statistics.  No call synchronises with the host and no result is
sized by the data: the torch formulation (`nonzero`, `randint(count)`, boolean indexing, `median`) waits for the device
once per frame and iteration.
"""
import torch

from . import _lib as L
from .window_rays import WindowTable

DRAW_RANGE = 2 ** 31          # draws are integers of [0, DRAW_RANGE): rank = (draw * count) >> 31
GATE_MAX_RAYS = 1 << 22       # glorie_depth_gate's limit (one workgroup)
_MODES = {"depth": 0, "all": 1}           # GLORIE_VALID_DEPTH, GLORIE_VALID_ALL (include/glorie_hip.h)


class ValidIndex:
    """the rank tables of a WindowTable's M depth maps: words uint64 [M, nw] (stored as int64; bit p % 64 of word p // 64
    is pixel p = j * W + i, set iff depth[p] > 0) and prefix int32 [M, nw + 1] (the valid pixels below each word, the
    frame's valid count last), nw = ceil(H W / 64).  mode "all": every pixel is valid and no depth is read (the mask of
    render_depth "mono").  One launch; the tables describe the depth maps as they were when it ran"""

    def __init__(self, table, mode="depth"):
        if not isinstance(table, WindowTable):
            raise ValueError("ValidIndex takes a WindowTable")
        if mode not in _MODES:
            raise ValueError(f"mode must be 'depth' or 'all', got {mode!r}")
        M, dev = len(table), table.device
        self.table, self.mode, self.H, self.W = table, mode, table.H, table.W
        self.nw = (table.H * table.W + 63) // 64
        self.words = torch.empty(M, self.nw, dtype=torch.int64, device=dev)
        self.prefix = torch.empty(M, self.nw + 1, dtype=torch.int32, device=dev)
        L.check(L.load().glorie_valid_index_build(L.ptr(table._tables[0]), M, table.H, table.W, _MODES[mode],
                                                  L.ptr(self.words), L.ptr(self.prefix), L.stream_ptr(dev)),
                "glorie_valid_index_build")

    def __len__(self):
        return len(self.table)

    @property
    def counts(self):
        """valid pixels per frame, int32 [M] on the device (a view of the prefix table)"""
        return self.prefix[:, -1]


def sample_window_rays(table, index, draws, per, fx, fy, cx, cy, const_radius=None):
    """draws int64 [M * per] in [0, 2^31) on the table's device, frame-major: ray r of window slot m = r // per reads the
    valid pixel of rank (draws[r] * count_m) >> 31 of its slot -> (rays_o [N,3], rays_d [N,3], depth [N], color [N,3],
    radius [N], ii [N], jj [N]); the first five as `window_rays` returns them for the pixels (ii, jj), bit for bit.  A slot
    without a valid pixel yields pixel (0, 0) and depth 0 for all its rays"""
    if not isinstance(table, WindowTable):
        raise ValueError("sample_window_rays takes a WindowTable")
    if not isinstance(index, ValidIndex) or index.table is not table:
        raise ValueError("sample_window_rays takes the ValidIndex built for its WindowTable")
    if not torch.is_tensor(draws):
        raise ValueError("draws must be a tensor")
    L.need_cuda(draws)
    M, per = len(table), int(per)
    N = M * per
    if per < 0 or draws.shape != (N,) or draws.dtype != torch.int64:
        raise ValueError(f"draws must be int64 [{N}] ({M} frames x {per} rays)")
    if draws.device != table.device:
        raise ValueError("draws must live on the table's device")
    dev = table.device
    draws = draws.contiguous()
    rays_o = torch.empty(N, 3, dtype=torch.float32, device=dev)
    rays_d = torch.empty(N, 3, dtype=torch.float32, device=dev)
    depth = torch.empty(N, dtype=torch.float32, device=dev)
    color = torch.empty(N, 3, dtype=torch.float32, device=dev)
    ii = torch.empty(N, dtype=torch.int64, device=dev)
    jj = torch.empty(N, dtype=torch.int64, device=dev)
    has_maps = table.radius_maps is not None
    want = has_maps or const_radius is not None
    radius = torch.empty(N, dtype=torch.float32, device=dev) if want else None
    t = table._tables
    L.check(L.load().glorie_sample_window_rays(
        L.ptr(t[0]), L.ptr(t[1]), L.ptr(t[2]) if has_maps else None, L.ptr(table.c2ws), M, per,
        int(table.channels_first), table.H, table.W, float(fx), float(fy), float(cx), float(cy), L.ptr(draws),
        L.ptr(index.words), L.ptr(index.prefix), float(const_radius) if const_radius is not None else 0.0, int(want),
        L.ptr(rays_o), L.ptr(rays_d), L.ptr(depth), L.ptr(color), L.ptr(radius), L.ptr(ii), L.ptr(jj),
        L.stream_ptr(dev)), "glorie_sample_window_rays")
    return rays_o, rays_d, depth, color, radius, ii, jj


def depth_gate(depth):
    """depth f32 [N] on the GPU -> (keep f32 [N]: 1 where 0 < depth <= min(10 median, 1.2 max), else 0; stats f32 [4] =
    (median, max, threshold, kept count)), median (torch's lower median) and max over the entries with depth > 0.  Without
    such an entry keep and stats are 0"""
    if not torch.is_tensor(depth):
        raise ValueError("depth must be a tensor")
    L.need_cuda(depth)
    if depth.dim() != 1 or depth.dtype != torch.float32:
        raise ValueError(f"depth must be float32 [N], got {depth.dtype} {tuple(depth.shape)}")
    N = depth.shape[0]
    if N > GATE_MAX_RAYS:
        raise ValueError(f"depth_gate takes at most {GATE_MAX_RAYS} rays, got {N}")
    depth = depth.contiguous()
    keep = torch.empty_like(depth)
    if N == 0:
        return keep, torch.zeros(4, dtype=torch.float32, device=depth.device)
    stats = torch.empty(4, dtype=torch.float32, device=depth.device)
    L.check(L.load().glorie_depth_gate(L.ptr(depth), N, L.ptr(keep), L.ptr(stats), L.stream_ptr(depth.device)),
            "glorie_depth_gate")
    return keep, stats
