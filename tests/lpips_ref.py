"""Float64 numpy restatement of LPIPS as csrc/lpips.hip computes it (torchmetrics' _LPIPS, version 0.1, AlexNet, eval mode:
im2col convolutions, explicit pooling loops), the torch composition of the same formula (F.conv2d, F.max_pool2d, in
float64 or float32) that pins it and sets the GPU tests' tolerance, and the seeded weights and scenes those tests share.

Neither torchmetrics nor the lpips package is needed: the formula is written from their sources as read."""
import functools

import numpy as np

SHIFT = (-0.030, -0.088, -0.188)
SCALE = (0.458, 0.448, 0.450)
# torchmetrics' form of the channel normalisation: f / sqrt(NORM_EPS + sum_c f^2), the eps inside the root.  The original
# lpips package divides by sqrt(sum_c f^2) + 1e-10 instead; the two differ only where a pixel's features are all ~0
NORM_EPS = 1e-8
# (Ci, Co, kernel, stride, padding) of AlexNet's features 0, 3, 6, 8, 10; a max_pool2d(3, 2) stands before the 2nd and 3rd
LAYERS = ((3, 64, 11, 4, 2), (64, 192, 5, 1, 2), (192, 384, 3, 1, 1), (384, 256, 3, 1, 1), (256, 256, 3, 1, 1))
POOL_BEFORE = (False, True, True, False, False)
MIN_SIDE = 31


def _conv_size(n, k, s, p):
    return (n + 2 * p - k) // s + 1


def _pool_size(n):
    return (n - 3) // 2 + 1


def shapes(H, W):
    """the (h, w) of the five taps of an H x W image"""
    out = []
    h, w = H, W
    for (_, _, k, s, p), pool in zip(LAYERS, POOL_BEFORE):
        if pool:
            h, w = _pool_size(h), _pool_size(w)
        h, w = _conv_size(h, k, s, p), _conv_size(w, k, s, p)
        out.append((h, w))
    return out


# ---- seeded weights and scenes ----------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def weights(seed=0):
    """{"conv": [(weight [Co,Ci,k,k], bias [Co])] * 5, "lin": [[Co]] * 5}, float32, read-only: conv weights uniform in
    +-sqrt(6 / fan_in), biases in +-0.1, lin in [0, 2) (non-negative, as the trained heads are)"""
    rng = np.random.default_rng(seed)
    conv, lin = [], []
    for ci, co, k, _, _ in LAYERS:
        bound = np.sqrt(6.0 / (ci * k * k))
        conv.append((rng.uniform(-bound, bound, (co, ci, k, k)).astype(np.float32),
                     rng.uniform(-0.1, 0.1, co).astype(np.float32)))
        lin.append(rng.uniform(0.0, 2.0, co).astype(np.float32))
    for w, b in conv:
        w.setflags(write=False)
        b.setflags(write=False)
    for l in lin:
        l.setflags(write=False)
    return {"conv": conv, "lin": lin}


def scene(H, W, seed):
    """(x, y) float32 [H,W,3]: x uniform in [0,1], y = x + 0.1 normal - some of y lies outside [0,1], so the clamp works"""
    rng = np.random.default_rng(seed)
    x = rng.uniform(0.0, 1.0, (H, W, 3))
    y = x + 0.1 * rng.standard_normal((H, W, 3))
    return x.astype(np.float32), y.astype(np.float32)


# ---- the float64 restatement ------------------------------------------------------------------------------------------------
def scale_image(img):
    """[H,W,3] -> [3,H,W] float64: clamp to [0,1], 2 v - 1, (v - shift) / scale"""
    v = np.clip(np.asarray(img, dtype=np.float64), 0.0, 1.0)
    v = 2.0 * v - 1.0
    v = (v - np.asarray(SHIFT)) / np.asarray(SCALE)
    return np.ascontiguousarray(v.transpose(2, 0, 1))


def conv2d(x, w, b, stride, pad):
    """x [Ci,h,w], w [Co,Ci,k,k], b [Co] -> [Co,oh,ow] float64 by im2col; the padding is zeros of x's own domain"""
    ci, h, wd = x.shape
    co, _, k, _ = w.shape
    oh, ow = _conv_size(h, k, stride, pad), _conv_size(wd, k, stride, pad)
    xp = np.zeros((ci, h + 2 * pad, wd + 2 * pad))
    xp[:, pad:pad + h, pad:pad + wd] = x
    cols = np.empty((ci, k, k, oh, ow))
    for ky in range(k):
        for kx in range(k):
            cols[:, ky, kx] = xp[:, ky:ky + stride * (oh - 1) + 1:stride, kx:kx + stride * (ow - 1) + 1:stride]
    out = np.asarray(w, dtype=np.float64).reshape(co, -1) @ cols.reshape(ci * k * k, oh * ow)
    return out.reshape(co, oh, ow) + np.asarray(b, dtype=np.float64)[:, None, None]


def max_pool(x):
    """max_pool2d(3, stride 2), no padding, floor mode: [C,h,w] -> [C,(h-3)//2+1,(w-3)//2+1]"""
    _, h, w = x.shape
    oh, ow = _pool_size(h), _pool_size(w)
    out = np.full((x.shape[0], oh, ow), -np.inf)
    for dy in range(3):
        for dx in range(3):
            out = np.maximum(out, x[:, dy:dy + 2 * (oh - 1) + 1:2, dx:dx + 2 * (ow - 1) + 1:2])
    return out


def features(img, wts):
    """[H,W,3] -> the five ReLU maps as [h,w,C] float64"""
    x = scale_image(img)
    maps = []
    for (w, b), (_, _, _, s, p), pool in zip(wts["conv"], LAYERS, POOL_BEFORE):
        if pool:
            x = max_pool(x)
        x = np.maximum(conv2d(x, w, b, s, p), 0.0)
        maps.append(np.ascontiguousarray(x.transpose(1, 2, 0)))
    return maps


def layer_value(fx, fy, lin):
    """[h,w,C] maps of both images and lin [C] -> mean over the pixels of sum_c lin[c] (n_x - n_y)^2"""
    nx = fx / np.sqrt(NORM_EPS + (fx * fx).sum(axis=2, keepdims=True))
    ny = fy / np.sqrt(NORM_EPS + (fy * fy).sum(axis=2, keepdims=True))
    return float((((nx - ny) ** 2) * np.asarray(lin, dtype=np.float64)).sum(axis=2).mean())


def lpips(x, y, wts):
    """x, y [H,W,3] -> (value, per_layer [5], maps: five [2,h,w,C] float64)"""
    fx, fy = features(x, wts), features(y, wts)
    per = np.array([layer_value(a, b, l) for a, b, l in zip(fx, fy, wts["lin"])])
    return float(per.sum()), per, [np.stack([a, b]) for a, b in zip(fx, fy)]


# ---- the torch composition of the same formula (what torchmetrics runs) -----------------------------------------------------
def torch_lpips(x, y, wts, dtype=None):
    """x, y [H,W,3] -> (value, per_layer [5], maps: five [2,h,w,C]) through F.conv2d and F.max_pool2d in `dtype`
    (torch.float64 pins the numpy form; torch.float32 is what the library computes); returned as float64 numpy"""
    import torch
    import torch.nn.functional as F
    dtype = dtype or torch.float64
    t = torch.stack([torch.as_tensor(np.asarray(a)).to(dtype).permute(2, 0, 1) for a in (x, y)])
    t = 2 * t.clamp(0.0, 1.0) - 1
    t = (t - torch.tensor(SHIFT, dtype=dtype).view(1, 3, 1, 1)) / torch.tensor(SCALE, dtype=dtype).view(1, 3, 1, 1)
    per, maps = [], []
    for (w, b), lin, (_, _, _, s, p), pool in zip(wts["conv"], wts["lin"], LAYERS, POOL_BEFORE):
        if pool:
            t = F.max_pool2d(t, 3, 2)
        t = F.relu(F.conv2d(t, torch.tensor(np.array(w)).to(dtype), torch.tensor(np.array(b)).to(dtype), stride=s, padding=p))
        n = t / torch.sqrt(NORM_EPS + (t * t).sum(dim=1, keepdim=True))
        d = (n[0:1] - n[1:2]) ** 2
        per.append(F.conv2d(d, torch.tensor(np.array(lin)).to(dtype).view(1, -1, 1, 1)).mean())
        maps.append(t.permute(0, 2, 3, 1).double().numpy())
    per = torch.stack(per)
    return float(per.sum()), per.double().numpy(), maps


# ---- sizes shared by the tests ---------------------------------------------------------------------------------------------
SIZES = [(31, 31), (31, 52), (52, 31), (35, 47), (63, 95), (97, 130)]

# A workgroup of csrc/lpips.hip owns PIXEL_TILE (conv1, conv2) or LATE_TILE (conv3 - 5) consecutive output pixels
# (row-major over h x w) of one image and CHANNEL_TILE output channels; K is not split.  Tap sizes one pixel short of a
# tile, exactly one tile, a tile count plus one pixel, exactly two tiles, two tiles and a ragged one:
PIXEL_TILE, LATE_TILE, CHANNEL_TILE, K_CHUNK = 64, 32, 64, 32
CONV1_TAPS = [(7, 9), (8, 8), (7, 55), (8, 16), (7, 19)]        # 63, 64, 6 * 64 + 1, 128, 133 pixels of tap 1
LATE_TAPS = [(1, 31), (4, 8), (3, 11), (8, 8), (5, 13)]         # 31, 32, 33, 64, 65 pixels of taps 3 to 5


def _side_for_conv1(n):
    return 4 * (n - 1) + 7                                       # the smallest side whose first tap is n


def _side_for_late(n):
    return _side_for_conv1(2 * (2 * n + 1) + 1)                  # ... whose last three taps are n: two pools back


TILE_CASES = ([(_side_for_conv1(h), _side_for_conv1(w)) for h, w in CONV1_TAPS]
              + [(_side_for_late(h), _side_for_late(w)) for h, w in LATE_TAPS])
for (_H, _W), (_h, _w) in zip(TILE_CASES, CONV1_TAPS):
    assert shapes(_H, _W)[0] == (_h, _w)
for (_H, _W), (_h, _w) in zip(TILE_CASES[len(CONV1_TAPS):], LATE_TAPS):
    assert shapes(_H, _W)[2:] == [(_h, _w)] * 3


@functools.lru_cache(maxsize=None)
def case(H, W, seed=None):
    """what the tests of one size share, computed once and read-only: (x, y, value, per_layer, maps) in float64 and the
    float32 composition's (value, per_layer, maps)"""
    x, y = scene(H, W, 100 + H + W if seed is None else seed)
    wts = weights()
    ref = lpips(x, y, wts)
    import torch
    f32 = torch_lpips(x, y, wts, torch.float32)
    for a in (x, y, ref[1], f32[1], *ref[2], *f32[2]):
        a.setflags(write=False)
    return x, y, ref, f32
