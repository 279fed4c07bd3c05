"""numpy restatement of glorie_valid_index_build, glorie_sample_window_rays and glorie_depth_gate (include/glorie_hip.h):
the rank tables, the integer rank map, the k-th set bit, the gather through window_rays_ref, and the gate with torch's
lower median and the fp32 threshold; with the scenes and gate vectors the tests share."""
import numpy as np

from window_rays_ref import INTRINSICS, general_c2ws, window_rays_ref

DRAW_RANGE = 2 ** 31


# ---- rank tables ----------------------------------------------------------------------------------------------------
def valid_mask(depths, mode="depth"):
    """[M,H,W] f32 -> bool [M, H W] in the reference's mask.reshape(-1) order: depth > 0 (NaN and negatives are False)"""
    depths = np.asarray(depths, np.float32)
    flat = depths.reshape(depths.shape[0], -1)
    if mode == "all":
        return np.ones(flat.shape, bool)
    with np.errstate(invalid="ignore"):
        return flat > 0


def valid_index_ref(depths, mode="depth"):
    """-> (words uint64 [M, nw], prefix int32 [M, nw + 1])"""
    mask = valid_mask(depths, mode)
    M, HW = mask.shape
    nw = (HW + 63) // 64
    bits = np.zeros((M, nw * 64), np.uint64)
    bits[:, :HW] = mask
    words = (bits.reshape(M, nw, 64) << np.arange(64, dtype=np.uint64)).sum(-1, dtype=np.uint64)
    prefix = np.zeros((M, nw + 1), np.int32)
    prefix[:, 1:] = np.cumsum(bits.reshape(M, nw, 64).sum(-1).astype(np.int64), 1)
    return words, prefix


def rank_of(draws, count):
    """(draw * count) >> 31 in exact integers; draws in [0, 2^31)"""
    return (np.asarray(draws, np.int64) * np.int64(count)) >> np.int64(31)


def kth_set_bit(word, k):
    """index of the k-th (from 0) set bit of a python int, counted from bit 0, by the kernel's popcount descent"""
    x, pos = int(word), 0
    for s in (32, 16, 8, 4, 2, 1):
        c = bin(x & ((1 << s) - 1)).count("1")
        if k >= c:
            k, x, pos = k - c, x >> s, pos + s
    return pos


def sample_pixels_ref(words, prefix, draws, per, H, W):
    """the pixel of every ray through the tables, as the kernel walks them -> (ii, jj) int64 [M * per]"""
    M, nw = words.shape
    ii, jj = np.zeros(M * per, np.int64), np.zeros(M * per, np.int64)
    for m in range(M):
        count = int(prefix[m, nw])
        if count == 0:
            continue
        for r in range(m * per, (m + 1) * per):
            rank = int(rank_of(draws[r], count))
            lo, hi = 0, nw
            while hi - lo > 1:
                mid = (lo + hi) >> 1
                lo, hi = (mid, hi) if prefix[m, mid] <= rank else (lo, mid)
            p = lo * 64 + kth_set_bit(words[m, lo], rank - int(prefix[m, lo]))
            ii[r], jj[r] = p % W, p // W
    return ii, jj


def sample_window_rays_ref(depths, images, c2ws, draws, per, fx, fy, cx, cy, mode="depth", radius_maps=None,
                           const_radius=None, channels_first=True):
    """-> (rays_o, rays_d, depth, color, radius, ii, jj): window_rays_ref at the sampled pixels, depth 0 in the slots
    without a valid pixel"""
    depths = np.asarray(depths, np.float32)
    M, H, W = depths.shape
    words, prefix = valid_index_ref(depths, mode)
    ii, jj = sample_pixels_ref(words, prefix, draws, per, H, W)
    ro, rd, d, col, rad = window_rays_ref(depths, images, c2ws, ii, jj, per, fx, fy, cx, cy, radius_maps=radius_maps,
                                          const_radius=const_radius, channels_first=channels_first)
    d = d.copy()
    empty = np.repeat(prefix[:, -1] == 0, per)
    d[empty] = 0
    return ro, rd, d, col, rad, ii, jj


def torch_masked_samples(depth, image, c2w, mask, sample, fx, fy, cx, cy, device):
    """the reference's formulation for one frame (get_samples with mask, src/utils/common.py:57-145) in torch, with the
    positions `sample` among the valid pixels given instead of drawn: the pixel grid, mask.nonzero(), indexing, the rays
    of get_rays_from_uv and the depth filter.  depth [H,W], image [H,W,3], mask bool [H,W] ->
    (rays_o, rays_d, depth, color, i, j) of the samples with depth > 0"""
    import torch
    from glorie_slam_amd.common import get_rays_from_uv
    H, W = depth.shape
    i, j = torch.meshgrid(torch.linspace(0, W - 1, W, device=device), torch.linspace(0, H - 1, H, device=device),
                          indexing="ij")
    i, j = i.t().reshape(-1), j.t().reshape(-1)
    valid_index = mask.reshape(-1).nonzero().reshape(-1)
    indices = valid_index[sample]
    i, j = i[indices], j[indices]
    d, col = depth.reshape(-1)[indices], image.reshape(-1, 3)[indices]
    ro, rd = get_rays_from_uv(i, j, c2w, fx, fy, cx, cy, device)
    keep = d > 0
    return ro[keep], rd[keep], d[keep], col[keep], i[keep].to(torch.int64), j[keep].to(torch.int64)


# ---- the gate -------------------------------------------------------------------------------------------------------
def depth_gate_ref(depth):
    """-> (keep f32 [N], stats f32 [4] = (median, max, threshold, kept)): the lower median (sorted rank (n - 1) // 2) and
    the maximum of the entries > 0, threshold = min(f32(10 median), f32(1.2f max))"""
    f = np.float32
    depth = np.asarray(depth, f)
    with np.errstate(invalid="ignore"):
        pos = depth > 0
    n = int(pos.sum())
    if n == 0:
        return np.zeros(depth.shape, f), np.zeros(4, f)
    s = np.sort(depth[pos])
    median, dmax = s[(n - 1) // 2], s[-1]
    thr = min(f(10.0) * median, f(1.2) * dmax)
    with np.errstate(invalid="ignore"):
        keep = (pos & (depth <= thr)).astype(f)
    return keep, np.array([median, dmax, thr, keep.sum()], f)


# ---- scenes ---------------------------------------------------------------------------------------------------------
# M, H, W, per: A 35 pixels, less than one word; B two words with a ragged tail, many slots; C exactly 6 words, several
# waves per slot; D 48 words, a real binary search, a ragged last wave
SHAPES = {"A": (3, 5, 7, 4), "B": (67, 9, 13, 5), "C": (2, 16, 24, 300), "D": (2, 48, 64, 130)}
DRAW_SETS = {"A": 10, "B": 1, "C": 1, "D": 1}            # iterations drawn (A: 40 draws a slot reach all of its 35 ranks)
_K = dict(INTRINSICS, D=(55.3, 54.1, 31.7, 23.4))
PATTERNS = ("half", "all", "none", "last", "tail", "bad")


def mask_pattern(name, H, W, rng):
    """a depth map [H,W] f32 whose valid pixels follow the pattern; invalid pixels are 0 except in "bad" (NaN, negative)"""
    HW = H * W
    d = rng.uniform(0.5, 4.0, HW).astype(np.float32)
    if name == "half":
        d[rng.random(HW) < 0.5] = 0
    elif name == "none":
        d[:] = 0
    elif name == "last":
        d[:HW - 1] = 0
    elif name == "tail":                                 # only pixels of the last word
        d[:(HW - 1) // 64 * 64] = 0
        d[(HW - 1) // 64 * 64::2] = 0
        d[HW - 1] = 2.5
    elif name == "bad":
        pick = rng.integers(0, 4, HW)
        d[pick == 1] = np.nan
        d[pick == 2] = -d[pick == 2]
        d[pick == 3] = 0
    else:
        assert name == "all"
    return d.reshape(H, W)


# the pattern of every frame: spread over the frames so that each scene meets what its size allows
FRAME_PATTERNS = {"A": ("half", "all", "bad"), "B": PATTERNS, "C": ("tail", "half"), "D": ("half", "last")}


def scene(name, seed=0):
    """general rotations with translation, non-integer intrinsics, the frames' masks by FRAME_PATTERNS (cycled), and
    draws int64 [sets, M * per] over [0, 2^31) with 0 and 2^31 - 1 in every slot of the first set; in A the draws of a
    slot over its ten sets begin with one draw per rank of the slot (the smallest draw that maps to it)"""
    M, H, W, per = SHAPES[name]
    sets = DRAW_SETS[name]
    rng = np.random.default_rng(seed + 7 * sum(map(ord, name)))
    pats = [FRAME_PATTERNS[name][m % len(FRAME_PATTERNS[name])] for m in range(M)]
    depths = np.stack([mask_pattern(p, H, W, rng) for p in pats])
    draws = rng.integers(0, DRAW_RANGE, (sets, M, per)).astype(np.int64)
    if name == "A":
        for m, count in enumerate(valid_mask(depths).sum(1)):
            mine = draws[:, m, :].reshape(-1)                     # the slot's draws, set-major
            mine[:count] = -((-np.arange(count, dtype=np.int64) * DRAW_RANGE) // int(count))   # ceil(q 2^31 / count)
            draws[:, m, :] = mine.reshape(sets, per)
        draws[-1, :, -2] = 0
        draws[-1, :, -1] = DRAW_RANGE - 1
    else:
        draws[0, :, 0] = 0
        draws[0, :, 1] = DRAW_RANGE - 1
    draws = draws.reshape(sets, M * per)
    return dict(M=M, H=H, W=W, per=per, K=_K[name], patterns=pats, c2ws=general_c2ws(M, rng), depths=depths,
                images=rng.uniform(0, 1, (M, 3, H, W)).astype(np.float32),
                radius_maps=rng.uniform(0.01, 0.1, (M, H, W)).astype(np.float32), draws=draws)


# ---- gate vectors ---------------------------------------------------------------------------------------------------
GATE_SIZES = (1, 2, 63, 64, 65, 1000, 1001, 5000, 70001)
GATE_KINDS = ("quantised", "equal", "mantissa", "zeros_nan", "all_zero", "outlier", "max_binds")


def gate_vector(kind, n, seed=0):
    """depth f32 [n].  quantised: steps of 1/8 with many ties around the median; equal: one value; mantissa: values that
    differ only in their lowest mantissa bits; zeros_nan: zeros and NaN interleaved with depths; all_zero; outlier: one far
    value, so that 10 median binds and drops it; max_binds: a narrow range, so that 1.2 max binds (and keeps all)"""
    rng = np.random.default_rng(seed + 131 * n + sum(map(ord, kind)))
    f = np.float32
    if kind == "quantised":
        d = (rng.integers(8, 24, n) / 8.0).astype(f)
    elif kind == "equal":
        d = np.full(n, 1.75, f)
    elif kind == "mantissa":
        d = (np.float32(2.0).view(np.uint32) + rng.integers(0, 7, n).astype(np.uint32)).view(f)
    elif kind == "zeros_nan":
        d = rng.uniform(0.5, 4.0, n).astype(f)
        d[1::3] = 0
        d[2::3] = np.nan
    elif kind == "all_zero":
        d = np.zeros(n, f)
    elif kind == "outlier":
        d = rng.uniform(1.0, 2.0, n).astype(f)
        d[n // 2] = 500.0
    else:
        assert kind == "max_binds"
        d = rng.uniform(1.0, 2.0, n).astype(f)
    return d
