"""Plain-torch restatement of the renderer's inference kernels around the decoders (csrc/render.hip): the inverse-distance
weights and feature interpolation, the per-ray sample counts and the compositing with its variance output, written from the
formula comments above the kernels.  Like tests/train_ref.py (whose `decode` is the reference of the decoders themselves) it
runs on the CPU in the dtype the caller gives: float64 is the reference, float32 the yardstick.

Inputs are the float32 tensors the kernels receive, cast up.  The one decision taken in float32 whatever the dtype is the
radius mask: the kernels compare the float32 distance with float32(r) * float32(r) rounded to float32, and so does this."""
import torch

import train_ref as tr


def composite_full(raw, z_vals, coef):
    """raw [R,S,4], z_vals [R,S] (S >= 1) -> depth [R], var [R], rgb [R,3], weights [R,S]
       alpha = sigmoid(coef occ), w_i = alpha_i prod_{j<i} (1 - alpha_j + 1e-10),
       rgb = sum w rgb / (sum w + 1e-10), depth = sum w z / (sum w + 1e-10), var = sum_s w_s (z_s - depth)^2"""
    depth, rgb, weights = tr.composite(raw, z_vals, coef)
    t = z_vals - depth[:, None]
    return depth, (weights * t * t).sum(-1), rgb, weights


def radius_squared(Q, radius=0.0, radius_per_query=None):
    """[Q] float32: float32(r) * float32(r), the product rounded to float32"""
    if radius_per_query is not None:
        r = radius_per_query.detach().cpu().reshape(-1).float()
    else:
        r = torch.full((Q,), float(radius), dtype=torch.float32)
    assert r.shape[0] == Q
    return r * r


def idw_weights(D, I, nn, radius=0.0, radius_per_query=None, min_nn=2, expo=False, dtype=torch.float64):
    """D [Q,8] float32 squared distances, I [Q,8] int64 (-1 = missing), nn [Q] neighbours inside the radius
    -> w [Q,8] = L1-normalise([I >= 0 and D <= r^2] * (expo ? exp(-20 sqrt(D)) : 1 / (D + 1e-10)), eps 1e-12), has [Q] bool"""
    D32 = D.detach().cpu().float()
    inside = (I.cpu() >= 0) & ~(D32 > radius_squared(D32.shape[0], radius, radius_per_query)[:, None])
    d = D32.to(dtype)
    base = torch.exp(-20.0 * torch.sqrt(d)) if expo else 1.0 / (d + 1e-10)
    w = torch.where(inside, base, torch.zeros_like(base))
    w = w / w.sum(1, keepdim=True).clamp_min(1e-12)
    return w, nn.cpu() >= int(min_nn)


def idw_features(feats, I, w, has):
    """c[q] = has ? sum_k w[q][k] feats[I[q][k].clamp(min=0)] : 0   (zeros, where the reference project draws a random
    placeholder feature: the occupancy of such a sample is forced to -100 either way)"""
    return tr.idw(feats, I, w, has)


TIE_RADIUS = 0.25
TIE_INSIDE = 0.0625                      # == float32(0.25) * float32(0.25): on the radius, inside
IDW_KINDS = ("plain", "exact hit", "all outside", "tie", "holes", "duplicates", "too few")


def make_idw_case(Q, Np, seed, per_query):
    """Synthetic search results (D [Q,8] float32, I [Q,8] int64, nn [Q] int32), a radius (float, or [Q] float32 with
    per_query) and the row kinds [Q] (index into IDW_KINDS), dealt round-robin over a random permutation of the rows:
      plain       random distances up to 1.6^2 r^2, nn = the number inside
      exact hit   the same with D = 0 in one slot
      all outside every distance beyond r^2 and nn = 3 all the same: has = 1, weights and feature exactly 0
      tie         r = 0.25 with D = 0.0625 (inside) and the next float32 above it (outside) in two slots
      holes       I = -1 in 1..7 slots anywhere in the row, their D left inside the radius
      duplicates  three slots naming the same point
      too few     nn = 0 with live neighbours inside the radius: feature exactly 0, weights still written
    No random distance lies within 4 float32 ulps of r^2 (asserted); the planted ties are the exception."""
    import numpy as np
    g = torch.Generator().manual_seed(seed)
    kind = (torch.arange(Q) % 7)[torch.randperm(Q, generator=g)]
    if per_query:
        r = (torch.rand(Q, generator=g) * 0.25 + 0.05).float()
        r[kind == 3] = TIE_RADIUS
    else:
        r = torch.full((Q,), TIE_RADIUS)
    r2 = r * r
    D = (torch.rand(Q, 8, generator=g) * 2.56 * r2[:, None]).float()
    I = torch.randint(0, Np, (Q, 8), generator=g)
    slot = torch.randint(0, 8, (Q,), generator=g)
    rows = torch.arange(Q)
    hit = kind == 1
    D[rows[hit], slot[hit]] = 0.0
    out = kind == 2
    D[out] = (r2[out, None] * (1.25 + torch.rand(int(out.sum()), 8, generator=g))).float()
    holes = (kind == 4)[:, None] & (torch.rand(Q, 8, generator=g) < 0.4)
    holes[rows[kind == 4], slot[kind == 4]] = True
    holes[rows[kind == 4], (slot[kind == 4] + 1) % 8] = False
    D[holes] = (D[holes] * 0.25).float()                      # inside the radius: only I = -1 switches them off
    I[holes] = -1
    dup = kind == 5
    I[dup, 3] = I[dup, 0]
    I[dup, 6] = I[dup, 0]
    few = kind == 6
    D[few, 1] = (D[few, 1] * 0.25).float()                    # a live neighbour inside the radius
    # no random distance near the radius
    ulp = torch.from_numpy(np.nextafter(r2.numpy(), np.float32(np.inf)) - r2.numpy())
    assert not bool(((D - r2[:, None]).abs() <= 4 * ulp[:, None]).any()), "a random distance within 4 ulps of r^2"
    tie = kind == 3
    assert float(np.float32(TIE_RADIUS) * np.float32(TIE_RADIUS)) == TIE_INSIDE
    D[tie, 2] = TIE_INSIDE
    D[tie, 3] = float(np.nextafter(np.float32(TIE_INSIDE), np.float32(1.0)))
    D[tie, 5] = D[tie, 5] * 0.25                              # and one neighbour well inside
    nn = ((I >= 0) & ~(D > r2[:, None])).sum(1).to(torch.int32)
    nn[out] = 3
    nn[kind == 6] = 0
    return D.contiguous(), I.contiguous(), nn, (r if per_query else TIE_RADIUS), kind


def ray_counts(has, S, min_samples):
    """has [R*S] -> counts [R] int64 of samples with neighbours, valid [R] bool = counts >= min_samples"""
    counts = has.cpu().reshape(-1, S).to(torch.int64).sum(1)
    return counts, counts >= int(min_samples)
