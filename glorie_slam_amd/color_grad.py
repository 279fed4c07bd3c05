"""Colour-gradient radii and the gradient-ranked pixel draw of the mapper on HIP kernels (csrc/color_grad.hip;
reference: src/mapper.py:767-784, src/utils/common.py:96-186).

  color_grad_maps              gradient magnitude (-1 off the valid mask) and the r_add / r_query maps of one image, the
                               radii optionally scaled by depth / 3 (glorie_color_grad_maps: one launch)
  dynamic_radius_maps          Mapper.run's radius block: (dynamic_r_add, dynamic_r_query), unscaled
  top_indices                  the M largest keys' indices, ascending, ties to the lowest index (glorie_topm: 12 launches,
                               no host read - records into a hipGraph)
  get_sample_uv_with_grad      common.get_sample_uv_with_grad: n of the 5n highest-gradient pixels
  get_samples_with_pixel_grad  common.get_samples_with_pixel_grad: their rays, depth, colour and pixel ids

The reference computes on the host (skimage, scipy interp1d, np.argpartition) in float64; here the maps are fp32 device
tensors, ties are resolved by index, and the n-of-5n draw comes from a torch generator.
"""
import torch

from . import _lib as L
from .common import get_rays_from_uv

# the master config's values (configs/mono_point_slam.yaml:130-133)
RADIUS_ADD_MAX, RADIUS_ADD_MIN, RADIUS_QUERY_RATIO, COLOR_GRAD_THRESHOLD = 0.08, 0.02, 2.0, 0.15


def _layout(image):
    """[H,W,3] -> (H, W, 0); [3,H,W] -> (H, W, 1)"""
    if image.dim() == 3 and image.shape[-1] == 3:
        return image.shape[0], image.shape[1], 0
    if image.dim() == 3 and image.shape[0] == 3:
        return image.shape[1], image.shape[2], 1
    raise ValueError(f"image must be [H,W,3] or [3,H,W], got {tuple(image.shape)}")


def color_grad_maps(image, color_grad_threshold=COLOR_GRAD_THRESHOLD, radius_add_max=RADIUS_ADD_MAX,
                    radius_add_min=RADIUS_ADD_MIN, radius_query_ratio=RADIUS_QUERY_RATIO, valid=None, depth_add=None,
                    depth_query=None, outputs=("grad", "r_add", "r_query")):
    """image f32 [H,W,3] or [3,H,W] on the device -> dict of the asked-for [H,W] f32 maps: "grad" (the Sobel magnitude,
    -1 where `valid` is False), "r_add", "r_query" (times depth_add / 3, depth_query / 3 when given)"""
    L.need_cuda(image, valid, depth_add, depth_query)
    H, W, chw = _layout(image)
    dev = image.device
    for name, d in (("depth_add", depth_add), ("depth_query", depth_query), ("valid", valid)):
        if d is not None and tuple(d.shape) != (H, W):
            raise ValueError(f"{name} must be [{H},{W}], got {tuple(d.shape)}")
    out = {k: torch.empty(H, W, dtype=torch.float32, device=dev) for k in outputs}
    img = L.f32(image)
    v = valid.to(torch.uint8).contiguous() if valid is not None else None
    da = L.f32(depth_add) if depth_add is not None else None
    dq = L.f32(depth_query) if depth_query is not None else None
    L.check(L.load().glorie_color_grad_maps(L.ptr(img), int(H), int(W), chw, L.ptr(v), float(color_grad_threshold),
                                            float(radius_add_max), float(radius_add_min), float(radius_query_ratio),
                                            L.ptr(da), L.ptr(dq), L.ptr(out.get("grad")), L.ptr(out.get("r_add")),
                                            L.ptr(out.get("r_query")), L.stream_ptr(dev)), "glorie_color_grad_maps")
    return out


def dynamic_radius_maps(gt_color, radius_add_max, radius_add_min, radius_query_ratio, color_grad_threshold):
    """Mapper.run (mapper.py:767-784): gt_color [H,W,3] -> (dynamic_r_add, dynamic_r_query) [H,W] f32, unscaled"""
    m = color_grad_maps(gt_color, color_grad_threshold, radius_add_max, radius_add_min, radius_query_ratio,
                        outputs=("r_add", "r_query"))
    return m["r_add"], m["r_query"]


def top_indices(keys, M):
    """keys f32 [n] (any shape, flattened) on the device -> (indices int64 [M] ascending, valid int32 [1]): the M largest
    keys, equal keys at the boundary taken lowest index first; valid = how many of them are >= 0"""
    L.need_cuda(keys)
    k = L.f32(keys.reshape(-1))
    n = k.numel()
    if not 0 <= M <= n:
        raise ValueError(f"top_indices: M={M} outside [0, {n}] (np.argpartition raises)")
    dev = k.device
    lib = L.load()
    idx = torch.empty(M, dtype=torch.int64, device=dev)
    valid = torch.empty(1, dtype=torch.int32, device=dev)
    ws = L.workspace(lib.glorie_topm_workspace(n), dev)
    L.check(lib.glorie_topm(L.ptr(k), n, int(M), L.ptr(ws), L.ptr(idx), L.ptr(valid), L.stream_ptr(dev)), "glorie_topm")
    return idx, valid


def draw_candidates(m, n, generator=None):
    """positions of the n picks among m candidates: np.random.choice(range(m), n, replace=False) of the reference,
    here the first n of a torch permutation, sorted (the candidates are ascending, so the picks come out ascending as
    np.union1d leaves them).  A CPU int64 tensor; tests replace this helper"""
    return torch.randperm(m, generator=generator)[:n].sort().values


def get_sample_uv_with_grad(H0, H1, W0, W1, n, image, valid_mask, generator=None):
    """common.get_sample_uv_with_grad (common.py:96-118): image [H,W,3] (or [3,H,W]) -> the linear indices (int64, on
    the device, ascending) of n pixels drawn from the 5n of highest gradient magnitude inside [H0,H1) x [W0,W1).
    The full image needs no host read; a smaller region filters the candidates with one"""
    H, W, _ = _layout(image)
    grad = color_grad_maps(image, valid=valid_mask, outputs=("grad",))["grad"]
    cand, _ = top_indices(grad, 5 * int(n))
    if (H0, H1, W0, W1) != (0, H, 0, W):
        r, c = cand // W, cand % W
        cand = cand[(r >= H0) & (r < H1) & (c >= W0) & (c < W1)]
    m = cand.shape[0]
    pick = draw_candidates(m, int(n), generator)
    if pick.shape[0] < int(n) or (pick.numel() and int(pick.max()) >= m):
        raise ValueError(f"cannot draw {n} of {m} candidates without replacement")
    return cand[pick.to(cand.device)]


def get_samples_with_pixel_grad(H0, H1, W0, W1, n_color, H, W, fx, fy, cx, cy, c2w, depth, color, device, valid_mask,
                                depth_filter=True, return_index=True, depth_limit=None, generator=None):
    """common.get_samples_with_pixel_grad (common.py:121-186): rays through the gradient-ranked pixels, their depth and
    colour (color [H,W,3]), the pixels without depth dropped; i the column, j the row.  Device tensors throughout"""
    assert n_color > 0, "invalid number of rays to sample."
    idx = get_sample_uv_with_grad(H0, H1, W0, W1, n_color, color, valid_mask, generator=generator)
    j, i = idx // W, idx % W
    rays_o, rays_d = get_rays_from_uv(i.float(), j.float(), c2w, fx, fy, cx, cy, device)
    sample_depth = depth[j, i]
    sample_color = color[j, i]
    if depth_filter:
        # a boolean selection (one host read), as the reference
        mask = sample_depth > 0
        if depth_limit is not None:
            mask = mask & (sample_depth < depth_limit)
        rays_o, rays_d, sample_depth, sample_color = rays_o[mask], rays_d[mask], sample_depth[mask], sample_color[mask]
        i, j = i[mask], j[mask]
    if return_index:
        return rays_o, rays_d, sample_depth, sample_color, i.to(torch.int64), j.to(torch.int64)
    return rays_o, rays_d, sample_depth, sample_color
