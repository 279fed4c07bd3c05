"""Float64 numpy restatement of the image metrics of csrc/metrics.hip (MS-SSIM with the defaults of pytorch_msssim, PSNR,
masked PSNR, depth L1), the torch composition of the same formula (depthwise conv2d + avg_pool2d, in float64 or float32)
that pins it and sets the GPU tests' tolerance, and the scenes those tests share."""
import numpy as np

WEIGHTS = (0.0448, 0.2856, 0.3001, 0.2363, 0.1333)
C1, C2 = 0.01 ** 2, 0.03 ** 2
WIN = 11


def window():
    g = np.exp(-((np.arange(WIN, dtype=np.float64) - WIN // 2) ** 2) / (2.0 * 1.5 ** 2))
    return g / g.sum()


def _valid_conv(img, g):
    """img [C,h,w] -> [C,h-10,w-10]: the separable valid convolution, rows first"""
    C, h, w = img.shape
    t = np.zeros((C, h, w - WIN + 1))
    for k in range(WIN):
        t += g[k] * img[:, :, k:k + w - WIN + 1]
    out = np.zeros((C, h - WIN + 1, w - WIN + 1))
    for k in range(WIN):
        out += g[k] * t[:, k:k + h - WIN + 1, :]
    return out


def avg_pool(img):
    """avg_pool2d(kernel 2, stride 2, padding = size % 2 per axis, count_include_pad): an odd axis gets one zero before
    and one after, every window is divided by 4.  img [C,h,w] -> [C,ceil(h/2),ceil(w/2)]"""
    C, h, w = img.shape
    ph, pw = h % 2, w % 2
    p = np.zeros((C, h + 2 * ph, w + 2 * pw))
    p[:, ph:ph + h, pw:pw + w] = img
    oh, ow = (h + 2 * ph - 2) // 2 + 1, (w + 2 * pw - 2) // 2 + 1
    p = p[:, :2 * oh, :2 * ow]
    return (p[:, 0::2, 0::2] + p[:, 0::2, 1::2] + p[:, 1::2, 0::2] + p[:, 1::2, 1::2]) / 4.0


def ssim_level(x, y, g=None):
    """x, y [C,h,w] float64 -> (ssim [C], cs [C]): the means of the two maps over the valid region"""
    g = window() if g is None else g
    mu1, mu2 = _valid_conv(x, g), _valid_conv(y, g)
    s1 = _valid_conv(x * x, g) - mu1 * mu1
    s2 = _valid_conv(y * y, g) - mu2 * mu2
    s12 = _valid_conv(x * y, g) - mu1 * mu2
    cs_map = (2.0 * s12 + C2) / (s1 + s2 + C2)
    ssim_map = ((2.0 * mu1 * mu2 + C1) / (mu1 * mu1 + mu2 * mu2 + C1)) * cs_map
    return ssim_map.mean(axis=(1, 2)), cs_map.mean(axis=(1, 2))


def ms_ssim(x, y, levels=5):
    """x, y [H,W,3] in [0,1] -> (value, per_level [levels,2,3]: (ssim, cs) of every level and channel), float64"""
    x = np.ascontiguousarray(np.asarray(x, dtype=np.float64).transpose(2, 0, 1))
    y = np.ascontiguousarray(np.asarray(y, dtype=np.float64).transpose(2, 0, 1))
    g = window()
    per = np.zeros((levels, 2, 3))
    for l in range(levels):
        assert min(x.shape[1:]) >= WIN, "a level is smaller than the window"
        per[l, 0], per[l, 1] = ssim_level(x, y, g)
        if l < levels - 1:
            x, y = avg_pool(x), avg_pool(y)
    w = np.asarray(WEIGHTS[:levels])
    terms = np.concatenate([per[:levels - 1, 1], per[levels - 1:, 0]])          # cs of the first levels, ssim of the last
    value = np.prod(np.maximum(terms, 0.0) ** w[:, None], axis=0).mean()
    return float(value), per


def psnr(x, y, mask=None):
    """-10 log10 of the mean squared difference of [H,W,3] images, over the frame or over the pixels of mask [H,W]
    (NaN on an empty mask)"""
    d2 = (np.asarray(x, dtype=np.float64) - np.asarray(y, dtype=np.float64)) ** 2
    if mask is not None:
        d2 = d2[np.asarray(mask, dtype=bool)]
    with np.errstate(invalid="ignore", divide="ignore"):
        mse = d2.sum() / d2.size if d2.size else np.float64("nan")
        return float(-10.0 * np.log10(mse))


def depth_l1(depth, gt_depth, mask):
    m = np.asarray(mask, dtype=bool)
    d = np.abs(np.asarray(depth, dtype=np.float64) - np.asarray(gt_depth, dtype=np.float64))[m]
    return float(d.sum() / d.size) if d.size else float("nan")


# ---- the torch composition of the same formula (what pytorch_msssim runs) ----------------------------------------------
def torch_ms_ssim(x, y, levels=5, dtype=None):
    """x, y [H,W,3] -> (value, per_level [levels,2,3]) through F.conv2d (depthwise, valid) and F.avg_pool2d in `dtype`
    (torch.float64 pins the numpy form; torch.float32 is what the reference library computes)"""
    import torch
    import torch.nn.functional as F
    dtype = dtype or torch.float64
    X = torch.as_tensor(np.asarray(x)).to(dtype).permute(2, 0, 1)[None]
    Y = torch.as_tensor(np.asarray(y)).to(dtype).permute(2, 0, 1)[None]
    coords = torch.arange(WIN, dtype=dtype) - WIN // 2
    g = torch.exp(-(coords ** 2) / (2 * 1.5 ** 2))
    g = g / g.sum()
    kh, kw = g.view(1, 1, WIN, 1).repeat(3, 1, 1, 1), g.view(1, 1, 1, WIN).repeat(3, 1, 1, 1)

    def filt(t):
        return F.conv2d(F.conv2d(t, kw, groups=3), kh, groups=3)

    per = torch.zeros(levels, 2, 3, dtype=dtype)
    for l in range(levels):
        mu1, mu2 = filt(X), filt(Y)
        s1, s2, s12 = filt(X * X) - mu1 * mu1, filt(Y * Y) - mu2 * mu2, filt(X * Y) - mu1 * mu2
        cs_map = (2 * s12 + C2) / (s1 + s2 + C2)
        ssim_map = ((2 * mu1 * mu2 + C1) / (mu1 * mu1 + mu2 * mu2 + C1)) * cs_map
        per[l, 0], per[l, 1] = ssim_map.flatten(2).mean(-1)[0], cs_map.flatten(2).mean(-1)[0]
        if l < levels - 1:
            pad = [s % 2 for s in X.shape[2:]]
            X, Y = F.avg_pool2d(X, 2, padding=pad), F.avg_pool2d(Y, 2, padding=pad)
    w = torch.tensor(WEIGHTS[:levels], dtype=dtype)
    terms = torch.cat([per[:levels - 1, 1], per[levels - 1:, 0]])
    value = torch.prod(torch.relu(terms) ** w[:, None], dim=0).mean()
    return float(value), per.double().numpy()


# ---- scenes shared by the tests ----------------------------------------------------------------------------------------
def scene(H, W, sigma, seed):
    """(gt, render) float32 [H,W,3] in [0,1]: sinusoids of three orientations plus pixel noise, and the same image
    with render noise of standard deviation `sigma`"""
    rng = np.random.default_rng(seed)
    yy, xx = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    gt = np.stack([0.5 + 0.25 * np.sin(0.21 * xx + 0.13 * yy + c) + 0.15 * np.sin(0.047 * xx - 0.071 * yy + 2 * c)
                   for c in range(3)], axis=-1)
    gt = np.clip(gt + 0.05 * rng.standard_normal(gt.shape), 0.0, 1.0)
    render = np.clip(gt + sigma * rng.standard_normal(gt.shape), 0.0, 1.0)
    return gt.astype(np.float32), render.astype(np.float32)


def textured(H, W, seed):
    """float32 [H,W,3] in [0.05, 0.95] with structure at every scale of a 5-level pyramid"""
    rng = np.random.default_rng(seed)
    yy, xx = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    img = 0.5 + sum(0.09 * np.sin(f * (xx * np.cos(a) + yy * np.sin(a)) + p)[..., None] * np.ones(3)
                    for f, a, p in ((0.9, 0.3, 0.0), (0.45, 1.2, 1.0), (0.22, 2.1, 2.0), (0.11, 0.8, 3.0), (0.05, 2.7, 4.0)))
    return np.clip(img + 0.04 * rng.standard_normal(img.shape), 0.05, 0.95).astype(np.float32)


def half_mask(H, W, seed):
    return np.random.default_rng(seed).random((H, W)) < 0.5


# (H, W, sigma, seed) of the scenes compared with a tolerance at five levels
SCENES = {"161x177": (161, 177, 0.05, 11), "163x161": (163, 161, 0.2, 12)}

# the output tile of one workgroup of csrc/metrics.hip is 32 wide and 16 high: widths of 32 + 9 (an empty last tile
# column), + 10 (exactly one), + 11 (a one-pixel ragged tile) and 2 * 32 + 11 (two tiles and a ragged one), heights of
# 16 + 9, + 10, + 11 and 2 * 16 + 11; (H, W, levels) with as many levels as the size allows, at most 3
TILE_W, TILE_H = 32, 16
TILE_CASES = [(25, 41, 2), (26, 42, 2), (27, 43, 2), (43, 75, 3), (43, 41, 3), (27, 75, 2)]
TILE_SIGMA = 0.1


def tile_scene(H, W):
    return scene(H, W, TILE_SIGMA, seed=20 + H + W)
