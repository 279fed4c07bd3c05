"""Plain-torch restatement of the renderer's training path (csrc/train.hip, render_train.py) for the tests: the
decoders on already-placed samples, the compositing and the Adam update, written from the formulas in the comments of
train.hip / decoder.py / render_train.py.  It runs on the CPU in the dtype the caller gives: float64 is the reference,
float32 the yardstick a correct fp32 evaluation is allowed to differ by.  Gradients come from torch autograd.

Inputs are the ones the kernels take: the 52 decoder tensors in the order of `render_train.decoder_tensors` and
  pts [Q,3], views [Q,3], cloud_pos [Np,3], geo_feats / col_feats [Np,32], I [Q,8] int64 (-1 = missing),
  w [Q,8], has [Q] (bool / uint8), z_vals [R,S], coef, stage_color.
"""
import math

import numpy as np
import torch
import torch.nn.functional as F

# positions in the 52-tensor list (glorie_decoder_params)
G_B, G_W, G_b, G_U, G_u, G_WO, G_BO = 0, 1, 6, 11, 16, 21, 22
N_B, N_W1, N_B1, N_W2, N_B2, C_BP, C_BV = 23, 24, 25, 26, 27, 28, 29
C_W, C_b, C_U, C_u, C_WO, C_BO = 30, 35, 40, 45, 50, 51
FIXED = (C_BP, C_BV)                     # the colour decoder's Fourier matrices are not trained
COLOR_ONLY = tuple(range(N_B, 52))       # tensors the geometry stage does not touch
PLACEHOLDER = -100.0


def fourier(x, B, concat):
    """x [n,3] -> sin((2 pi x) B) [| cos((2 pi x) B)]"""
    v = (2 * math.pi * x) @ B
    return torch.cat((torch.sin(v), torch.cos(v)), -1) if concat else torch.sin(v)


def softplus100(x):
    return F.softplus(x, beta=100)


def idw(feats, I, w, has):
    """c[q] = has ? sum_k w[q][k] feats[I[q][k].clamp(min=0)] : 0"""
    c = (w[..., None] * feats[I.clamp(min=0)]).sum(1)
    return torch.where(has.bool()[:, None], c, torch.zeros_like(c))


def neighbor_feature(P, pts, cloud_pos, col_feats, I, w, has):
    """the per-neighbour network on rows [sin | cos of the relative position, col_feats[I]] and its weighted sum"""
    Ic = I.clamp(min=0)
    rel = cloud_pos[Ic] - pts[:, None, :]
    X = torch.cat([fourier(rel.reshape(-1, 3), P[N_B], True), col_feats[Ic].reshape(-1, 32)], -1)
    Fk = F.linear(softplus100(F.linear(X, P[N_W1], P[N_B1])), P[N_W2], P[N_B2]).reshape(-1, 8, 32)
    c = (w[..., None] * Fk).sum(1)
    return torch.where(has.bool()[:, None], c, torch.zeros_like(c))


def trunk(emb, c, W, b, U, u, act, pre=None):
    """A_i = act(lin_i(h)), H_i = A_i + fc_c_i(c); after layer 2 h = cat(emb, H_2)"""
    h = emb
    for i in range(5):
        z = F.linear(h, W[i], b[i])
        if pre is not None:
            pre.append(z)
        h = act(z) + F.linear(c, U[i], u[i])
        if i == 2:
            h = torch.cat([emb, h], -1)
    return h


def decode(P, pts, views, cloud_pos, geo_feats, col_feats, I, w, has, stage_color, soft=None):
    """-> occ [Q], rgb [Q,3] (zeros in the geometry stage), the ReLU pre-activations [Q,160]
    (soft: a list that receives the softplus pre-activations of the colour trunk)"""
    pre = []
    c_geo = idw(geo_feats, I, w, has)
    h = trunk(fourier(pts, P[G_B], False), c_geo, P[G_W:G_W + 5], P[G_b:G_b + 5], P[G_U:G_U + 5], P[G_u:G_u + 5],
              torch.relu, pre)
    occ = F.linear(h, P[G_WO], P[G_BO]).squeeze(-1)
    if not stage_color:
        return occ, torch.zeros(pts.shape[0], 3, dtype=occ.dtype), torch.cat(pre, -1)
    c_col = neighbor_feature(P, pts, cloud_pos, col_feats, I, w, has)
    v = views / views.norm(dim=1, keepdim=True).clamp_min(1e-12)
    emb = torch.cat([fourier(pts, P[C_BP], True), fourier(v, P[C_BV], True)], -1)
    h = trunk(emb, c_col, P[C_W:C_W + 5], P[C_b:C_b + 5], P[C_U:C_U + 5], P[C_u:C_u + 5], softplus100, soft)
    rgb = torch.sigmoid(F.linear(h, P[C_WO], P[C_BO]))
    return occ, rgb, torch.cat(pre, -1)


def placeholder_shift(occ, has):
    """raw[:, 3] = has ? occ : -100 with the -100 assigned outside the graph: the value changes, the gradient computed at
    -100 still flows into occ.  Written as occ + shift with a constant shift."""
    return torch.where(has.bool(), torch.zeros_like(occ), (PLACEHOLDER - occ).detach())


def composite(raw, z_vals, coef):
    """raw [R,S,4], z_vals [R,S] -> depth [R], rgb [R,3], weights [R,S]"""
    alpha = torch.sigmoid(coef * raw[..., 3])
    ones = torch.ones_like(alpha[:, :1])
    T = torch.cumprod(torch.cat([ones, 1.0 - alpha + 1e-10], -1), -1)[:, :-1]
    weights = alpha * T
    wsum = weights.sum(-1, keepdim=True) + 1e-10
    rgb = (weights[..., None] * raw[..., :3]).sum(-2) / wsum
    depth = (weights * z_vals).sum(-1) / wsum.squeeze(-1)
    return depth, rgb, weights


def render(P, pts, views, cloud_pos, geo_feats, col_feats, I, w, has, z_vals, coef, stage_color, shift=None):
    """-> raw [Q,4], depth [R], rgb [R,3], ReLU pre-activations"""
    occ, rgb, pre = decode(P, pts, views, cloud_pos, geo_feats, col_feats, I, w, has, stage_color)
    occ = occ + (placeholder_shift(occ, has) if shift is None else shift)
    raw = torch.cat([rgb, occ[:, None]], -1)
    R, S = z_vals.shape
    depth, rgb_map, _ = composite(raw.reshape(R, S, 4), z_vals, coef)
    return raw, depth, rgb_map, pre


def linear_loss(c_depth, c_rgb):
    """loss = sum_r c_depth[r] depth[r] + sum c_rgb[r] . rgb[r]: every ray has its own cotangents"""
    def fn(depth, rgb, lo, hi):
        return (c_depth[lo:hi].to(depth.dtype) * depth).sum() + (c_rgb[lo:hi].to(rgb.dtype) * rgb).sum()
    return fn


def _cast(t, dtype):
    return t.detach().cpu().to(dtype) if t.is_floating_point() else t.detach().cpu()


def forward_backward(params, pts, views, cloud_pos, geo_feats, col_feats, I, w, has, z_vals, coef, stage_color, loss_fn,
                     dtype=torch.float64, chunk_rays=None):
    """The whole pass in `dtype` on the CPU.  loss_fn(depth, rgb, lo, hi) is the loss of rays [lo, hi) - a sum over rays,
    so the rays may be processed in chunks and the gradients added.
    -> dict(raw, depth, rgb, pre, d_geo, d_col, grads[52] (None for the fixed Fourier matrices))"""
    P = [_cast(p, dtype).requires_grad_(i not in FIXED) for i, p in enumerate(params)]
    gf, cf = _cast(geo_feats, dtype).requires_grad_(True), _cast(col_feats, dtype).requires_grad_(True)
    pts, views, cloud_pos, w, z_vals = (_cast(t, dtype) for t in (pts, views, cloud_pos, w, z_vals))
    I, has = I.cpu(), has.cpu()
    R, S = z_vals.shape
    step = R if not chunk_rays else int(chunk_rays)
    outs = {"raw": [], "depth": [], "rgb": [], "pre": []}
    for lo in range(0, R, step):
        hi = min(R, lo + step)
        q = slice(lo * S, hi * S)
        raw, depth, rgb, pre = render(P, pts[q], views[q], cloud_pos, gf, cf, I[q], w[q], has[q], z_vals[lo:hi], coef,
                                      stage_color)
        loss_fn(depth, rgb, lo, hi).backward()
        for k, v in (("raw", raw), ("depth", depth), ("rgb", rgb), ("pre", pre)):
            outs[k].append(v.detach())
    res = {k: torch.cat(v) for k, v in outs.items()}
    zero = lambda t: torch.zeros_like(t)
    res["d_geo"] = gf.grad if gf.grad is not None else zero(gf)
    res["d_col"] = cf.grad if cf.grad is not None else zero(cf)
    res["grads"] = [None if i in FIXED else (p.grad if p.grad is not None else zero(p)) for i, p in enumerate(P)]
    return res


def composite_grad(raw, z_vals, coef, g_depth, g_rgb, dtype=torch.float64):
    """d (sum g_depth depth + sum g_rgb rgb) / d raw, by autograd over `composite`; a None cotangent counts as zero"""
    raw = _cast(raw, dtype).requires_grad_(True)
    depth, rgb, _ = composite(raw, _cast(z_vals, dtype), coef)
    loss = raw.sum() * 0
    if g_depth is not None:
        loss = loss + (_cast(g_depth, dtype) * depth).sum()
    if g_rgb is not None:
        loss = loss + (_cast(g_rgb, dtype) * rgb).sum()
    loss.backward()
    return raw.grad


def adam_ref(p, g, m, v, step, lr, b1, b2, eps, row_mask=None, dtype=torch.float64):
    """torch.optim.Adam (no amsgrad, no weight decay) -> (p, m, v) after step number `step` (>= 1).  lr, b1, b2, eps are
    rounded to float32 first: the C ABI takes floats.  row_mask [rows] bool: rows outside it keep p, m and v."""
    lr, b1, b2, eps = (float(np.float32(x)) for x in (lr, b1, b2, eps))
    p, g, m, v = (_cast(t, dtype) for t in (p, g, m, v))
    if dtype == torch.float32:
        # the straightforward fp32 evaluation: every scalar rounded to fp32 as it is formed (correctly rounded powers)
        f = np.float32
        omb1, omb2 = float(f(1) - f(b1)), float(f(1) - f(b2))
        bc1 = float(f(1) - f(np.float64(b1) ** step))
        bc2s = float(np.sqrt(f(1) - f(np.float64(b2) ** step), dtype=np.float32))
        ss = float(f(lr) / f(bc1))
    else:
        omb1, omb2 = 1.0 - b1, 1.0 - b2
        bc1 = -math.expm1(step * math.log(b1))
        bc2s = math.sqrt(-math.expm1(step * math.log(b2)))
        ss = lr / bc1
    mn = b1 * m + omb1 * g
    vn = b2 * v + omb2 * g * g
    pn = p - ss * mn / (vn.sqrt() / bc2s + eps)
    if row_mask is not None:
        keep = (~row_mask.cpu().bool()).repeat_interleave(p.numel() // row_mask.numel()).reshape(p.shape)
        pn, mn, vn = torch.where(keep, p, pn), torch.where(keep, m, mn), torch.where(keep, v, vn)
    return pn, mn, vn
