"""Float64 restatements of the adjoints of the correlation lookups and of projmap (numpy, CPU only; test infrastructure).

Written from the formulas, not from the kernels:

  lookup     out[n, i, j, y, x] = sum_{a, b in {0, 1}} wx_a wy_b vol[n, y, x, fy - r + j + b, fx - r + i + a]
             with (fx, fy) = floor(coords), (dx, dy) = coords - floor, wx = (1 - dx, dx), wy = (1 - dy, dy); a tap outside the
             plane is skipped.  Its adjoint scatters grad[n, i, j, y, x] wx_a wy_b into the same element.
  alt-corr   out[b, s, iy + rd ix, h, w] = sum_{a, b} wx_a wy_b <f1[b, h, w], f2[b, fy - r + iy + b, fx - r + ix + a]>; the
             adjoint w.r.t. f1 gathers t f2[tap], the one w.r.t. f2 scatters t f1[pixel], t = grad wx_a wy_b.
  projmap    X_j = T_ij (x, y, 1, d): the pixel grid where Z <= 0.01, (fx X / Z + cx, fy Y / Z + cy) otherwise; valid = Z > 0.25.

Every function takes `absolute=True` to return the sum of the MAGNITUDES of the terms of each result instead (the quantity the
fp32 error bounds of the GPU tests scale with) and `count=True` to count the terms.  The scene builders give dyadic / integer
scenes on which every partial sum of the adjoints is exactly representable (`assert_exact`), so that the GPU tests compare bit
for bit and an accumulation type cannot hide behind a tolerance.  `altcorr_bwd_plan` mirrors the box rule of the alt-corr
backward kernel and is used ONLY to assert that a coordinate scene reaches the branch it was written for."""
import numpy as np

import geom_ref as G

F64 = np.float64


def _window(c, radius):
    """c float32 coordinates -> (integer window origin floor(c) - r, fraction as float64)"""
    c = np.asarray(c, np.float32)
    f = np.floor(c)
    return f.astype(F64).astype(np.int64) - radius, (c - f).astype(F64)


def _mode(v, absolute, count):
    v = np.asarray(v, F64)
    if count:
        return np.ones_like(v)
    return np.abs(v) if absolute else v


# ---- index / pyramid backward ---------------------------------------------------------------------------------------------
def index_bwd_f64(coords, grad, h2, w2, radius, absolute=False, count=False):
    """coords [N, 2, h1, w1] float32 (scaled to the level), grad [N, rd, rd, h1, w1] -> volume_grad [N, h1, w1, h2, w2] float64"""
    coords = np.asarray(coords, np.float32)
    N, _, h1, w1 = coords.shape
    rd = 2 * radius + 1
    g = _mode(np.asarray(grad).reshape(N, rd, rd, h1, w1), absolute, count)
    x0, dx = _window(coords[:, 0], radius)
    y0, dy = _window(coords[:, 1], radius)
    out = np.zeros((N, h1, w1, h2, w2), F64)
    n_i, y_i, x_i = np.meshgrid(np.arange(N), np.arange(h1), np.arange(w1), indexing="ij")
    for i in range(rd):
        for j in range(rd):
            for a, wx in ((0, 1.0 - dx), (1, dx)):
                for b, wy in ((0, 1.0 - dy), (1, dy)):
                    tx, ty = x0 + i + a, y0 + j + b
                    inb = (tx >= 0) & (tx < w2) & (ty >= 0) & (ty < h2)
                    wgt = np.ones_like(wx) if count else wx * wy
                    np.add.at(out, (n_i[inb], y_i[inb], x_i[inb], ty[inb], tx[inb]), (g[:, i, j] * wgt)[inb])
    return out


def pyramid_bwd_f64(coords, grad, h2, w2, radius, num_levels, absolute=False, count=False):
    """coords [N, 2, h1, w1] float32 UNscaled, grad [N, L rd^2, h1, w1] -> list of [N, h1, w1, h2 >> l, w2 >> l]"""
    coords = np.asarray(coords, np.float32)
    N, _, h1, w1 = coords.shape
    rd = 2 * radius + 1
    g = np.asarray(grad).reshape(N, num_levels, rd, rd, h1, w1)
    return [index_bwd_f64(coords / np.float32(2 ** l), g[:, l], h2 >> l, w2 >> l, radius, absolute, count)
            for l in range(num_levels)]


# ---- alt-corr backward ----------------------------------------------------------------------------------------------------
def altcorr_bwd_f64(fmap1, fmap2, coords, grad, radius, absolute=False, count=False):
    """fmap1 [B, H, W, C], fmap2 [B, H2, W2, C], coords [B, S, H, W, 2], grad [B, S, rd^2, H, W] (channel iy + rd ix)
    -> (fmap1_grad [B, H, W, C], fmap2_grad [B, H2, W2, C]) float64"""
    f1 = _mode(np.asarray(fmap1, np.float32), absolute, count)
    f2 = _mode(np.asarray(fmap2, np.float32), absolute, count)
    coords = np.asarray(coords, np.float32)
    B, H, W, C = f1.shape
    _, H2, W2, _ = f2.shape
    S = coords.shape[1]
    rd = 2 * radius + 1
    g = _mode(np.asarray(grad).reshape(B, S, rd, rd, H, W), absolute, count)       # [b, s, ix, iy, h, w]
    x0, dx = _window(coords[..., 0], radius)
    y0, dy = _window(coords[..., 1], radius)
    g1, g2 = np.zeros((B, H, W, C), F64), np.zeros((B, H2, W2, C), F64)
    b_i, s_i, h_i, w_i = np.meshgrid(np.arange(B), np.arange(S), np.arange(H), np.arange(W), indexing="ij")
    for ix in range(rd):
        for iy in range(rd):
            for a, wx in ((0, 1.0 - dx), (1, dx)):
                for b, wy in ((0, 1.0 - dy), (1, dy)):
                    tx, ty = x0 + ix + a, y0 + iy + b
                    inb = (tx >= 0) & (tx < W2) & (ty >= 0) & (ty < H2)
                    wgt = np.ones_like(wx) if count else wx * wy
                    t = (g[:, :, ix, iy] * wgt)[inb][:, None]
                    bb, hh, ww, yy, xx = b_i[inb], h_i[inb], w_i[inb], ty[inb], tx[inb]
                    np.add.at(g1, (bb, hh, ww), t * f2[bb, yy, xx])
                    np.add.at(g2, (bb, yy, xx), t * f1[bb, hh, ww])
    return g1, g2


ALT_TILE, ALT_MAX_SLOTS = 4, 400
BOXED, PER_TAP = 0, 1


def altcorr_bwd_plan(coords, C, radius=3):
    """Mirror of the box rule of the alt-corr backward kernel: coords [B, S, H, W, 2] float32 -> branch [B, S, tiles_y, tiles_x]
    (BOXED where the box of the window origins of the 4 x 4 source tile, grown by the window, holds at most ALT_MAX_SLOTS
    targets; C does not enter the rule)"""
    coords = np.asarray(coords, np.float32)
    B, S, H, W, _ = coords.shape
    x0, _ = _window(np.clip(coords[..., 0], -2.0 ** 30, 2.0 ** 30), radius)
    y0, _ = _window(np.clip(coords[..., 1], -2.0 ** 30, 2.0 ** 30), radius)
    nty, ntx = -(-H // ALT_TILE), -(-W // ALT_TILE)
    branch = np.zeros((B, S, nty, ntx), np.int64)
    for ty in range(nty):
        for tx in range(ntx):
            sl = (slice(None), slice(None), slice(ty * ALT_TILE, (ty + 1) * ALT_TILE), slice(tx * ALT_TILE, (tx + 1) * ALT_TILE))
            bw = x0[sl].max(axis=(2, 3)) - x0[sl].min(axis=(2, 3)) + 2 * radius + 2
            bh = y0[sl].max(axis=(2, 3)) - y0[sl].min(axis=(2, 3)) + 2 * radius + 2
            area = bw * bh
            branch[:, :, ty, tx] = np.where(area <= ALT_MAX_SLOTS, BOXED, PER_TAP)
    return branch


# ---- pure-torch float64 forwards (differentiable: what torch.autograd checks the adjoints against) --------------------------
def lookup_torch(vol, coords, radius):
    """vol [N, h1, w1, h2, w2] (any float tensor, used as is), coords [N, 2, h1, w1] -> [N, rd, rd, h1, w1]; gradient for vol only"""
    import torch
    N, h1, w1, h2, w2 = vol.shape
    rd = 2 * radius + 1
    c = coords.detach().to(torch.float32)
    f = torch.floor(c)
    frac = (c - f).to(vol.dtype)
    org = f.to(torch.float64).to(torch.int64) - radius
    dx, dy, x0, y0 = frac[:, 0], frac[:, 1], org[:, 0], org[:, 1]
    flat = vol.reshape(N, h1, w1, h2 * w2)
    rows = []
    for i in range(rd):
        cols = []
        for j in range(rd):
            acc = torch.zeros((N, h1, w1), dtype=vol.dtype, device=vol.device)
            for a, wx in ((0, 1 - dx), (1, dx)):
                for b, wy in ((0, 1 - dy), (1, dy)):
                    tx, ty = x0 + i + a, y0 + j + b
                    inb = (tx >= 0) & (tx < w2) & (ty >= 0) & (ty < h2)
                    idx = (ty.clamp(0, h2 - 1) * w2 + tx.clamp(0, w2 - 1)).unsqueeze(-1)
                    acc = acc + flat.gather(-1, idx).squeeze(-1) * inb.to(vol.dtype) * wx * wy
            cols.append(acc)
        rows.append(torch.stack(cols, 1))
    return torch.stack(rows, 1)


def altcorr_torch(f1, f2, coords, radius):
    """f1 [B, H, W, C], f2 [B, H2, W2, C], coords [B, S, H, W, 2] -> [B, S, rd^2, H, W] (channel iy + rd ix): the lookup of the
    all-pairs products, which is the same function"""
    import torch
    B, H, W, C = f1.shape
    _, H2, W2, _ = f2.shape
    S = coords.shape[1]
    vol = torch.einsum("bhwc,byxc->bhwyx", f1, f2)                           # [B, H, W, H2, W2]
    outs = []
    for s in range(S):
        o = lookup_torch(vol, coords[:, s].permute(0, 3, 1, 2), radius)      # [B, ix, iy, H, W]
        outs.append(o.reshape(B, -1, H, W))
    return torch.stack(outs, 1)


def corr_block_torch(fmap1, fmap2, coords, num_levels=4, radius=3):
    """CorrBlock(fmap1, fmap2)(coords) as a pure-torch composition in the dtype of the maps: fmap [b, n, C, h, w],
    coords [b, n, h, w, 2] -> [b, n, L rd^2, h, w]"""
    import torch
    import torch.nn.functional as F
    b, n, C, h, w = fmap1.shape
    a = fmap1.reshape(b * n, C, h * w) / 4.0
    bb = fmap2.reshape(b * n, C, h * w) / 4.0
    corr = torch.matmul(a.transpose(1, 2), bb).reshape(b * n * h * w, 1, h, w)
    c = coords.permute(0, 1, 4, 2, 3).reshape(b * n, 2, h, w)
    outs = []
    for l in range(num_levels):
        vol = corr.reshape(b * n, h, w, h >> l, w >> l)
        outs.append(lookup_torch(vol, c / 2 ** l, radius).reshape(b, n, -1, h, w))
        if l + 1 < num_levels:
            corr = F.avg_pool2d(corr, 2, stride=2)
    return torch.cat(outs, 2)


def altcorr_block_torch(fmaps, coords, ii, jj, num_levels=4, radius=3):
    """AltCorrBlock(fmaps)(coords, ii, jj) as a pure-torch composition: fmaps [1, F, C, H, W], coords [1, N, H, W, 2]
    -> [1, N, L rd^2, H, W]"""
    import torch
    import torch.nn.functional as F
    B, Fr, C, H, W = fmaps.shape
    f = fmaps.reshape(B * Fr, C, H, W) / 4.0
    f1 = f.permute(0, 2, 3, 1)[ii]
    outs = []
    for l in range(num_levels):
        f2 = f.permute(0, 2, 3, 1)[jj]
        o = altcorr_torch(f1, f2, (coords[0] / 2 ** l).unsqueeze(1), radius)   # [N, 1, 49, H, W]
        outs.append(o[:, 0])
        if l + 1 < num_levels:
            f = F.avg_pool2d(f, 2, stride=2)
    return torch.cat(outs, 1).unsqueeze(0)


# ---- exactness --------------------------------------------------------------------------------------------------------------
def _lsb_exp(x, limit=60):
    x = np.asarray(x, F64)
    k = 0
    while not np.all(x * 2.0 ** k == np.rint(x * 2.0 ** k)):
        k += 1
        assert k <= limit
    return k


def assert_exact(abs_sums, lsb_exp, mant_bits, what=""):
    """every partial sum of a result is a multiple of 2^-lsb_exp bounded by the sum of the magnitudes of its terms: with
    max(abs_sums) 2^lsb_exp < 2^mant_bits each of them, in any order, is exact in a format of mant_bits significant bits.
    Returns max / 2^mant_bits."""
    worst = float(np.max(abs_sums)) * 2.0 ** lsb_exp
    assert worst < 2.0 ** mant_bits, f"{what}: partial sums reach {worst:.4g} lsbs of 2^-{lsb_exp}, more than 2^{mant_bits}"
    return worst / 2.0 ** mant_bits


def fp16_exact(x):
    x = np.asarray(x, F64)
    with np.errstate(over="ignore"):
        return bool(np.all(x.astype(np.float16).astype(F64) == x))


# ---- scenes -------------------------------------------------------------------------------------------------------------------
def dyadic_index_scene(seed, N, h1, w1, h2, w2, radius):
    """coordinates whose fractions are multiples of 1/4 and integer gradients in [-8, 8].  The coordinates hold, at fixed pixels:
    exact integers, negatives with a fraction (floor differs from truncation), windows half and wholly outside on every side,
    and +-3e9.  -> coords [N, 2, h1, w1] f32, grad [N, rd, rd, h1, w1] float64 (integers)"""
    rng = np.random.default_rng(seed)
    rd = 2 * radius + 1
    m = radius + 2
    cx = rng.integers(-m * 4, (w2 + m) * 4, (N, h1, w1)) / 4.0
    cy = rng.integers(-m * 4, (h2 + m) * 4, (N, h1, w1)) / 4.0
    c = np.stack([cx, cy], 1).astype(np.float32)
    flat = c.reshape(N, 2, -1)
    special = [(2.0, 3.0), (-0.25, -0.75), (-1.0, 0.0), (w2 - 1.0, h2 - 1.0), (-radius - 0.5, 1.25), (w2 + radius - 0.5, 2.0),
               (1.5, -radius - 0.5), (2.25, h2 + radius - 0.25), (-radius - 1.0, 2.0), (w2 + radius + 1.0, 1.0),
               (-40.0, -40.0), (3.0e9, 1.0), (1.0, -3.0e9), (-3.0e9, 3.0e9), (0.0, 0.0), (w2 - 0.75, h2 - 0.25)]
    for k, (vx, vy) in enumerate(special):
        n, p = k % N, (k * 2 + (k % N)) % (h1 * w1)
        flat[n, 0, p], flat[n, 1, p] = vx, vy
    grad = rng.integers(-8, 9, (N, rd, rd, h1, w1)).astype(F64)
    return c, grad


def altcorr_bwd_scene(seed, B, S, H, W, H2, W2, C, kind, radius=3):
    """integer features in [-2, 2], integer gradients in [-4, 4], coordinates multiples of 1/4: `smooth` (the identity map of
    the source onto the target, shifted by s: every 4 x 4 tile shares a box) or `scatter` (corr_ref.scene_scatter scaled onto
    the target: boxes of more than ALT_MAX_SLOTS targets), both with windows leaving the map"""
    import corr_ref as R
    rng = np.random.default_rng(seed)
    f1 = rng.integers(-2, 3, (B, H, W, C)).astype(np.float32)
    f2 = rng.integers(-2, 3, (B, H2, W2, C)).astype(np.float32)
    rd = 2 * radius + 1
    grad = rng.integers(-4, 5, (B, S, rd * rd, H, W)).astype(np.float32)
    y, x = np.meshgrid(np.arange(H, dtype=np.float32), np.arange(W, dtype=np.float32), indexing="ij")
    if kind == "smooth":
        base = np.stack([x * (W2 / W) - 0.75, y * (H2 / H) + 0.5], -1)
        c = np.stack([base + 1.25 * s for s in range(S)])
    else:
        sc = R.scene_scatter(H, W).transpose(1, 2, 0) * np.array([W2 / W, H2 / H], np.float32)
        sc = sc + np.where((x + y) % 5 == 0, 40.0, 0.0)[..., None]          # a few windows far outside the target
        c = np.stack([sc - 1.5 * s for s in range(S)])
    c = np.round(c * 4) / 4
    coords = np.broadcast_to(c[None], (B, S, H, W, 2)).astype(np.float32).copy()
    coords[1:] += 0.5                                                           # the second batch entry differs
    return f1, f2, coords, grad


# ---- projmap -------------------------------------------------------------------------------------------------------------------
Z_GRID, Z_VALID = 0.01, 0.25
Z_BAND = 1e-3


def projmap_scene(seed=5, K=4, h=11, w=13):
    """general rotations up to 0.6 rad, translations that put a large share of the points behind the target camera, fx != fy"""
    import glorie_slam_amd.synth as synth
    rng = np.random.default_rng(seed)
    poses = G._random_poses(rng, K, 0.1, 0.6, 0.5)
    poses[:, 2] = rng.uniform(-1.6, 1.6, K)                        # along the optical axis: Z = R z + t_z d changes sign
    disps = rng.uniform(0.2, 2.5, (K, h, w)).astype(np.float32)
    intr = (synth.camera(h, w) * np.array([1.09, 0.93, 1.04, 0.96], np.float32)).astype(np.float32)
    ii, jj = G._edges(K, None)
    return dict(poses=poses, disps=disps, intrinsics=intr, ii=ii, jj=jj)


def projmap64(poses, disps, intrinsics, ii, jj):
    """-> coords [N, h, w, 2], valid [N, h, w, 1], and the float64 point X_j [N, h, w, 3] the thresholds and bounds are taken from"""
    _, h, w = disps.shape
    fx, fy, cx, cy = np.asarray(intrinsics, F64)[:4]
    N = len(ii)
    coords, valid, X = np.zeros((N, h, w, 2)), np.zeros((N, h, w, 1)), np.zeros((N, h, w, 3))
    for n, (i, j) in enumerate(zip(ii, jj)):
        T = G.relative_matrix(poses, int(i), int(j))
        X0, x, y = G._rays(h, w, intrinsics, disps[int(i)])
        X1 = X0 @ T.T
        X[n] = X1[..., :3]
        Z = X1[..., 2]
        front = Z > Z_GRID
        Zs = np.where(front, Z, 1.0)
        coords[n, ..., 0] = np.where(front, fx * X1[..., 0] / Zs + cx, x)
        coords[n, ..., 1] = np.where(front, fy * X1[..., 1] / Zs + cy, y)
        valid[n, ..., 0] = Z > Z_VALID
    return coords, valid, X


def projmap_firm(X):
    """pixels whose Z is farther than Z_BAND from both thresholds"""
    Z = X[..., 2]
    return (np.abs(Z - Z_GRID) > Z_BAND) & (np.abs(Z - Z_VALID) > Z_BAND)


def projmap_coord_bound(scene, X):
    """fp32 bound of the projected coordinates [N, h, w, 2].  With u = 2^-24: the homogeneous ray has 2 u relative error per
    component; the relative pose (two quaternion products and a rotated translation, unit quaternions) and its action on the
    point are sums of at most 12 products of magnitudes bounded by M = |ray| + |t_ij| d, so X, Y and Z carry at most 32 u M
    absolute error each (first order, counted generously); the quotient, the product with f and the sum with c add 3 u of
    the result's magnitude.  d(f X / Z) = f (dX / Z + |X| dZ / Z^2)."""
    u = 2.0 ** -24
    poses, disps, intr, ii = scene["poses"], scene["disps"], scene["intrinsics"], scene["ii"]
    fx, fy, cx, cy = np.asarray(intr, F64)
    N, h, w, _ = X.shape
    out = np.zeros((N, h, w, 2))
    for n, (i, j) in enumerate(zip(scene["ii"], scene["jj"])):
        T = G.relative_matrix(poses, int(i), int(j))
        X0, _, _ = G._rays(h, w, intr, disps[int(i)])
        M = np.linalg.norm(X0[..., :3], axis=-1) + np.linalg.norm(T[:3, 3]) * np.abs(X0[..., 3]) \
            + np.linalg.norm(np.asarray(poses, F64)[[int(i), int(j)], :3], axis=-1).sum() * np.abs(X0[..., 3])
        dX = 32 * u * M
        Z = np.maximum(np.abs(X[n, ..., 2]), 1e-30)
        for k, (f, c) in enumerate(((fx, cx), (fy, cy))):
            q = np.abs(X[n, ..., k]) / Z
            out[n, ..., k] = f * (dX / Z + q * dX / Z) * 1.01 + 3 * u * (f * q + abs(c))
    return out
