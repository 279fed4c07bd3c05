"""Keyframe selection of the mapper on HIP kernels (csrc/select.hip; reference: src/mapper.py:126-244,
src/utils/common.py:31-35).

  frustum_feature_mask / get_mask_from_c2w   Mapper.get_mask_from_c2w: the points inside the camera's frustum and not
                                             farther than the depth map + 0.5 (glorie_frustum_select: a memset and three
                                             or four launches, the count stays on the device - records into a hipGraph)
  keyframe_overlap                           the overlap figure of Mapper.keyframe_selection_overlap for K keyframes
                                             (glorie_keyframe_overlap: one launch, integer counts)
  keyframe_selection_overlap                 Mapper.keyframe_selection_overlap: pixel draw, the overlap counts, one host
                                             read of them, the candidates in overlap order, a random permutation
  random_select                              common.random_select (keyframe_selection_method "global")

Camera-to-world matrices are in the renderer's OpenGL convention (SequenceRunner._keyframe_view, the reference's
`c2w[:3, 1:3] *= -1`) and rigid: the kernels invert them as R^T, -R^T t.
"""
import torch

from . import _lib as L
from .common import get_rays_from_uv

OVERLAP_EDGE = 20          # mapper.py:229


def frustum_feature_mask(points, c2w, depth, fx, fy, cx, cy, H, W, edge=-4, return_indices=False):
    """points [n,3], c2w [4,4] (or [3,4]), depth [H,W], all on the device -> (mask uint8 [n], count int32 [1]) without a
    host round trip; return_indices: also int64 [n] whose first `count` entries are the kept points in ascending order"""
    L.need_cuda(points, c2w, depth)
    n = points.shape[0]
    if points.shape != (n, 3) or tuple(depth.shape) != (H, W):
        raise ValueError(f"points must be [n,3] and depth [{H},{W}], got {tuple(points.shape)} and {tuple(depth.shape)}")
    dev = points.device
    lib = L.load()
    mask = torch.empty(n, dtype=torch.uint8, device=dev)
    count = torch.empty(1, dtype=torch.int32, device=dev)
    indices = torch.empty(n, dtype=torch.int64, device=dev) if return_indices else None
    ws = L.workspace(lib.glorie_frustum_select_workspace(n), dev)
    pts, c, dep = L.f32(points), L.homogeneous(c2w), L.f32(depth)
    L.check(lib.glorie_frustum_select(L.ptr(pts), n, L.ptr(c), float(fx), float(fy), float(cx), float(cy), int(H),
                                      int(W), float(edge), L.ptr(dep), L.ptr(ws), L.ptr(mask), L.ptr(count),
                                      L.ptr(indices), L.stream_ptr(dev)), "glorie_frustum_select")
    return (mask, count, indices) if return_indices else (mask, count)


def get_mask_from_c2w(c2w, depth, points, fx, fy, cx, cy, H, W, edge=-4):
    """Mapper.get_mask_from_c2w (mapper.py:126-174): the ascending indices of the selected points as a list (one host
    read).  The reference reads points from self.npc and the intrinsics from self; here they are arguments"""
    dep = torch.as_tensor(depth, device=points.device)
    _, count, indices = frustum_feature_mask(points, c2w.to(points.device), dep, fx, fy, cx, cy, H, W, edge,
                                             return_indices=True)
    return indices[:int(count)].tolist()


def keyframe_overlap(rays_o, rays_d, depth, c2ws, fx, fy, cx, cy, H, W, n_samples=8, edge=OVERLAP_EDGE,
                     return_counts=False):
    """rays_o, rays_d [R,3], depth [R] of the current view (rays with depth <= 0 are skipped), c2ws [K,4,4] of the
    candidates -> percent_inside [K] float64 on the device (mapper.py:200-235: the share of the n_samples points per ray
    that land inside keyframe k's image, edge px in, in front of it; NaN for every k when no ray has a depth, the
    reference's 0/0).  return_counts: (inside int32 [K], number of samples) instead"""
    L.need_cuda(rays_o, rays_d, depth, c2ws)
    R = depth.shape[0]
    c = L.homogeneous(c2ws)
    if c.dim() != 3 or rays_o.shape != (R, 3) or rays_d.shape != (R, 3):
        raise ValueError("keyframe_overlap: rays_o, rays_d [R,3], depth [R], c2ws [K,4,4] expected")
    K = c.shape[0]
    dev = depth.device
    inside = torch.zeros(K, dtype=torch.int32, device=dev)
    L.check(L.load().glorie_keyframe_overlap(L.ptr(L.f32(rays_o)), L.ptr(L.f32(rays_d)), L.ptr(L.f32(depth)), R,
                                             int(n_samples), L.ptr(c), K, float(fx), float(fy), float(cx), float(cy),
                                             int(H), int(W), float(edge), L.ptr(inside), L.stream_ptr(dev)),
            "glorie_keyframe_overlap")
    total = (depth > 0).sum() * int(n_samples)
    if return_counts:
        return inside, total
    return inside.double() / total.double()


def overlap_candidates(percent_inside):
    """ids with percent_inside > 0, in decreasing overlap (a stable sort, as the reference's `sorted`)"""
    p = [float(x) for x in percent_inside]
    order = sorted(range(len(p)), key=lambda i: p[i], reverse=True)
    return [i for i in order if p[i] > 0.0]


def keyframe_selection_overlap(gt_color, mono_depth, c2w, keyframe_c2ws, k, fx, fy, cx, cy, N_samples=8, pixels=200,
                               generator=None, return_percent=False):
    """Mapper.keyframe_selection_overlap (mapper.py:176-244) -> list of at most k ids into keyframe_c2ws.
    gt_color is carried for the reference's argument list only.  `pixels` pixels are drawn uniformly over the image from
    `generator` (a CPU torch.Generator; None: torch's default); those without depth are dropped, not redrawn
    (get_samples(..., depth_filter=True)).  The candidates are the keyframes with percent_inside > 0 in decreasing order;
    the first k of a random permutation of them (drawn from `generator`) are returned.  One host read of the K figures."""
    H, W = mono_depth.shape
    dev = mono_depth.device
    K = int(keyframe_c2ws.shape[0])
    if K == 0:
        return ([], torch.zeros(0, dtype=torch.float64)) if return_percent else []
    # get_sample_uv with no mask: a flat index over the [H,W] grid, i the column, j the row
    flat = torch.randint(0, H * W, (pixels,), generator=generator).to(dev)
    i, j = flat % W, torch.div(flat, W, rounding_mode="floor")
    rays_o, rays_d = get_rays_from_uv(i.float(), j.float(), c2w.to(dev).float(), fx, fy, cx, cy, dev)
    d = mono_depth[j, i]
    percent = keyframe_overlap(rays_o.reshape(-1, 3), rays_d.reshape(-1, 3), d, keyframe_c2ws.to(dev), fx, fy, cx, cy,
                               H, W, n_samples=N_samples).cpu()
    cand = overlap_candidates(percent)
    perm = torch.randperm(len(cand), generator=generator).tolist() if cand else []
    sel = [cand[p] for p in perm][:max(int(k), 0)]
    return (sel, percent) if return_percent else sel


def random_select(l, k, generator=None):
    """common.random_select (common.py:31-35): min(l, k) distinct values of range(l) in random order"""
    if l <= 0 or k <= 0:
        return []
    return torch.randperm(int(l), generator=generator)[:min(int(l), int(k))].tolist()


def final_refine_window(mapped, skipped, counter, map_rays, generator=None, pix_warping=None):
    """the window of one pass of Mapper.final_refine (mapper.py:816-836 through optimize_map, :541-584): the 'global'
    method with mapping_window_size = counter - 1.  Host only.
    mapped: keyframes [0, mapped) have been through the mapper, `skipped` of them were not mapped; counter: the video's
    keyframe count.  The candidates are the mapped keyframes without the last one, L (keyframe_dict[:-1]);
    random_select draws max(counter - 3, 0) of them; window = selected + [L].  per = map_rays // (len(window) + 1) pixels
    of every window frame: the reference counts the current frame, which colour refinement then leaves out (:575, :584);
    at least 1 (the reference would sample none).  pix_warping=True with a window beyond the pixel-warping kernel's
    frame limit is an error (raised before anything is drawn).  -> (window, per)"""
    from .warp_loss import MAX_FRAMES
    skipped = set(int(f) for f in skipped)
    frames = [f for f in range(int(mapped)) if f not in skipped]
    if not frames:
        raise ValueError("final refinement needs at least one mapped keyframe")
    cand, last = frames[:-1], frames[-1]
    num = max(int(counter) - 3, 0)
    size = min(len(cand), num) + 1
    if pix_warping is True and size > MAX_FRAMES:
        raise ValueError(f"pix_warping supports up to {MAX_FRAMES} window frames, the refinement window has {size}")
    window = [cand[s] for s in random_select(len(cand), num, generator)] + [last]
    return window, max(1, int(map_rays) // (len(window) + 1))
