"""Float64 restatement of the mapper's pixel-warping loss (src/mapper.py:326-388, projection src/utils/common.py:324-350)
for the tests: plain torch ops, differentiable with respect to `depth` through autograd (the bilinear read is written out
so that its derivative is grid_sample's: the cell is fixed by floor, the weights carry the gradient).

Returns (loss, kept mask [N,M]).  An empty selection gives NaN and a zero gradient, as torch's mean of nothing does; rays
with a non-finite depth are never kept and get a zero gradient.
"""
import torch

EDGE, BETA = 5, 0.1


def project(c2ws, X, fx, fy, cx, cy):
    """-> u, v, zc [N,M]"""
    w2c = torch.linalg.inv(c2ws)
    p = torch.einsum("mij,nj->nmi", w2c[:, :3, :3], X) + w2c[None, :, :3, 3]
    a, b, c = p.unbind(-1)
    zc = c + 1e-5
    return (-fx * a + cx * c) / zc, (fy * b + cy * c) / zc, zc


def bilinear(images, m, x, y):
    """images [M,H,W,3]; frame index m, pixel coordinates x, y (same shape) -> [..., 3], border clamp, zero outside"""
    Hh, Ww = images.shape[1], images.shape[2]
    x = x.clamp(0, Ww - 1)
    y = y.clamp(0, Hh - 1)
    x0, y0 = torch.floor(x).detach(), torch.floor(y).detach()
    out = 0
    for dx in (0, 1):
        for dy in (0, 1):
            xi, yi = x0 + dx, y0 + dy
            wgt = (1 - (x - xi).abs()) * (1 - (y - yi).abs())
            ok = (xi >= 0) & (xi < Ww) & (yi >= 0) & (yi < Hh)
            tex = images[m, yi.clamp(0, Hh - 1).long(), xi.clamp(0, Ww - 1).long()]
            out = out + torch.where(ok[..., None], wgt[..., None] * tex, torch.zeros_like(tex))
    return out


def pix_warp_loss(rays_o, rays_d, depth, c2ws, fx, fy, cx, cy, W, H, frame_indices, indices_tensor, images, gt_color):
    """float64 throughout; images [M,H,W,3]"""
    f64 = lambda t: t.to(torch.float64)
    finite = torch.isfinite(depth)
    dep = torch.where(finite, f64(depth), torch.zeros_like(f64(depth)))
    X = f64(rays_o) + f64(rays_d) * dep[:, None]
    u, v, zc = project(f64(c2ws), X, fx, fy, cx, cy)
    mask = (u < W - EDGE) & (u > EDGE) & (v < H - EDGE) & (v > EDGE) & (zc < 0)
    mask &= (frame_indices[None, :] != indices_tensor[:, None]) & finite[:, None]
    mask &= mask.sum(dim=1, keepdim=True) >= 4
    M = c2ws.shape[0]
    m = torch.arange(M, device=u.device)[None, :].expand_as(u)
    uu = torch.where(mask, u, torch.full_like(u, 8.0))          # excluded entries read a harmless pixel
    vv = torch.where(mask, v, torch.full_like(v, 8.0))
    val = bilinear(f64(images), m, uu - 0.5, vv - 0.5)         # [N,M,3]
    diff = val - f64(gt_color)[:, None, :]
    ad = diff.abs()
    sl1 = torch.where(ad < BETA, 0.5 * diff * diff / BETA, ad - 0.5 * BETA)
    s = torch.where(mask[..., None], sl1, torch.zeros_like(sl1)).sum()
    n = int(mask.sum()) * 3
    loss = s / n if n > 0 else s * 0 + float("nan")
    return loss, mask
