"""tests/render_ref.py - the float64 reference of the inference kernels of csrc/render.hip - pinned on the CPU against
loop-form numpy restatements of the same formulas (an independent statement: scalar loops, no broadcasting), on tiny inputs
that hold every edge the GPU tests plant."""
import math

import numpy as np
import pytest
import torch

import render_ref as rr


# ---------------------------------------------------------------------------------------------------------------------
# compositing
# ---------------------------------------------------------------------------------------------------------------------
def _composite_loops(raw, z, coef):
    R, S = z.shape
    depth, var, rgb, w = np.zeros(R), np.zeros(R), np.zeros((R, 3)), np.zeros((R, S))
    for r in range(R):
        T, wsum, dz, c = 1.0, 0.0, 0.0, [0.0, 0.0, 0.0]
        for s in range(S):
            x = coef * raw[r, s, 3]
            alpha = 1.0 / (1.0 + math.exp(-x)) if x > -700 else 0.0
            w[r, s] = alpha * T
            T *= 1.0 - alpha + 1e-10
            wsum += w[r, s]
            dz += w[r, s] * z[r, s]
            for k in range(3):
                c[k] += w[r, s] * raw[r, s, k]
        den = wsum + 1e-10
        depth[r] = dz / den
        rgb[r] = [v / den for v in c]
        for s in range(S):
            var[r] += w[r, s] * (z[r, s] - depth[r]) ** 2
    return depth, var, rgb, w


@pytest.mark.parametrize("S", [1, 2, 5])
@pytest.mark.parametrize("coef", [0.1, 10.0])
def test_composite_full_matches_the_loop_form(S, coef):
    g = torch.Generator().manual_seed(S)
    R = 5
    raw = torch.rand(R, S, 4, generator=g, dtype=torch.float64)
    raw[..., 3] = torch.randn(R, S, generator=g, dtype=torch.float64) * 3.0
    raw[0, :, 3] = -100.0                              # placeholders only
    raw[1, 0, 3] = 100.0                               # opaque first sample
    raw[2, S - 1, 3] = 1e3
    z = torch.sort(torch.rand(R, S, generator=g, dtype=torch.float64) + 0.5, dim=1).values
    d, v, c, w = rr.composite_full(raw, z, coef)
    ld, lv, lc, lw = _composite_loops(raw.numpy(), z.numpy(), coef)
    for got, ref in ((d, ld), (v, lv), (c, lc), (w, lw)):
        assert got.dtype == torch.float64 and got.shape == ref.shape
        np.testing.assert_allclose(got.numpy(), ref, rtol=1e-12, atol=1e-300)
    if coef == 10.0:                                   # sigmoid(-1000) is exactly 0: nothing of the ray is left
        assert float(w[0].abs().max()) == 0.0 and float(d[0]) == 0.0 and float(v[0]) == 0.0 and float(c[0].abs().max()) == 0.0
        assert float(w[1, 0]) == 1.0 and float(d[1]) == pytest.approx(float(z[1, 0]), rel=1e-9)
    else:
        assert float(w[0].min()) > 0.0
    assert float(v.min()) >= 0.0 and (S == 1 or float(v.max()) > 0.0)


# ---------------------------------------------------------------------------------------------------------------------
# inverse-distance weights and features
# ---------------------------------------------------------------------------------------------------------------------
def _idw_loops(D, I, nn, r, min_nn, expo, feats):
    Q = D.shape[0]
    w, has, c = np.zeros((Q, 8)), np.zeros(Q, bool), np.zeros((Q, feats.shape[1]))
    for q in range(Q):
        r32 = np.float32(r[q] if np.ndim(r) else r)
        r2 = np.float32(r32 * r32)
        s = 0.0
        for k in range(8):
            if I[q, k] >= 0 and D[q, k] <= r2:
                d = float(D[q, k])
                w[q, k] = math.exp(-20.0 * math.sqrt(d)) if expo else 1.0 / (d + 1e-10)
                s += w[q, k]
        for k in range(8):
            w[q, k] /= max(s, 1e-12)
        has[q] = nn[q] >= min_nn
        if has[q]:
            for k in range(8):
                c[q] += w[q, k] * feats[max(I[q, k], 0)]
    return w, has, c


@pytest.mark.parametrize("expo", [False, True])
@pytest.mark.parametrize("per_query", [False, True])
def test_idw_reference_matches_the_loop_form(per_query, expo):
    Q, Np = 28, 11
    D, I, nn, r, kind = rr.make_idw_case(Q, Np, 3, per_query)
    assert sorted(set(kind.tolist())) == list(range(7))
    feats = torch.randn(Np, 32, generator=torch.Generator().manual_seed(1), dtype=torch.float64)
    rq = dict(radius_per_query=r) if per_query else dict(radius=r)
    for min_nn in (1, 2, 3):
        w, has = rr.idw_weights(D, I, nn, min_nn=min_nn, expo=expo, **rq)
        c = rr.idw_features(feats, I, w, has)
        lw, lhas, lc = _idw_loops(D.numpy(), I.numpy(), nn.numpy(), r.numpy() if per_query else r, min_nn, expo,
                                  feats.numpy())
        assert w.dtype == torch.float64 and np.array_equal(has.numpy(), lhas)
        assert np.array_equal(w.numpy() == 0.0, lw == 0.0)
        np.testing.assert_allclose(w.numpy(), lw, rtol=1e-13, atol=0)
        np.testing.assert_allclose(c.numpy(), lc, rtol=1e-12, atol=1e-15)
        k = lambda name: kind == rr.IDW_KINDS.index(name)
        # the edges, on the reference's own output
        tie = k("tie")
        assert bool((w[tie, 2] > 0).all()) and bool((w[tie, 3] == 0).all())
        assert bool((w[k("all outside")] == 0).all()) and bool(has[k("all outside")].all())
        assert bool((c[k("all outside")] == 0).all())
        assert not bool(has[k("too few")].any()) and bool((w[k("too few")].sum(1) > 0.99).all())
        assert bool((c[k("too few")] == 0).all())
        assert bool((w[I < 0] == 0).all()) and int((I[k("holes")] < 0).sum()) >= int(k("holes").sum())
        hit = k("exact hit")
        assert bool((w[hit].max(1).values > 0.999).all()) if not expo else bool((w[hit].max(1).values > 0.125).all())
        live = w.sum(1) > 0
        np.testing.assert_allclose(w.sum(1)[live].numpy(), 1.0, rtol=1e-14)
        assert 0 < int(has.sum()) < Q


def test_radius_mask_is_decided_in_float32():
    """r = 0.1: float32(r)^2 rounded to float32 differs from the float64 square; a distance between the two is judged by the
    former, whatever dtype the weights are formed in"""
    r32 = np.float32(0.1)
    r2 = np.float32(r32 * r32)
    assert float(r2) != 0.1 * 0.1
    above = np.nextafter(r2, np.float32(1.0))
    D = torch.tensor([[float(r2), float(above), 1e-3, 1e-3, 1e-3, 1e-3, 1e-3, 1e-3]], dtype=torch.float32)
    I = torch.arange(8)[None]
    for dtype in (torch.float64, torch.float32):
        w, has = rr.idw_weights(D, I, torch.tensor([7], dtype=torch.int32), radius=0.1, min_nn=2, dtype=dtype)
        assert w.dtype == dtype and float(w[0, 0]) > 0.0 and float(w[0, 1]) == 0.0 and bool(has[0])


# ---------------------------------------------------------------------------------------------------------------------
# sample counts
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S", [1, 4])
@pytest.mark.parametrize("min_samples", [1, 3])
def test_ray_counts_matches_the_loop_form(S, min_samples):
    g = torch.Generator().manual_seed(0)
    R = 9
    has = torch.rand(R * S, generator=g) < 0.5
    has.view(R, S)[0] = False
    has.view(R, S)[1] = True
    counts, valid = rr.ray_counts(has, S, min_samples)
    assert counts.dtype == torch.int64 and valid.dtype == torch.bool
    h = has.numpy()
    for r in range(R):
        n = 0
        for s in range(S):
            n += 1 if h[r * S + s] else 0
        assert int(counts[r]) == n and bool(valid[r]) == (n >= min_samples)
    assert int(counts[0]) == 0 and int(counts[1]) == S
    # uint8 masks, as the kernels hand them on
    c8, v8 = rr.ray_counts(has.to(torch.uint8), S, min_samples)
    assert torch.equal(c8, counts) and torch.equal(v8, valid)
