"""The float64 restatements of tests/corr_bwd_ref.py, pinned without a GPU: against torch.autograd through a pure-torch float64
forward, by the dot-product identity <J x, y> = <x, J^T y> against the forward restatements of tests/corr_ref.py, and the
preconditions (exactness, branch reach, populations) of the scenes that tests/test_gpu_corr_bwd.py relies on."""
import numpy as np
import pytest
import torch

import corr_bwd_ref as RB
import corr_ref as R

F64 = np.float64


def _t(x, grad=False):
    t = torch.from_numpy(np.ascontiguousarray(x))
    return t.requires_grad_(True) if grad else t


# ---- index backward ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("radius", [3, 1])
def test_index_adjoint_equals_autograd_on_a_dyadic_scene(radius):
    N, h1, w1, h2, w2 = 2, 5, 7, 6, 9
    coords, grad = RB.dyadic_index_scene(1, N, h1, w1, h2, w2, radius)
    vol = _t(np.random.default_rng(0).integers(-4, 5, (N, h1, w1, h2, w2)).astype(F64), grad=True)
    out = RB.lookup_torch(vol, _t(coords), radius)
    out.backward(_t(grad))
    got = RB.index_bwd_f64(coords, grad, h2, w2, radius)
    assert np.abs(got - vol.grad.numpy()).max() == 0.0          # dyadic: both are exact in float64
    assert (0.1 if radius == 3 else 0.03) < (got != 0).mean() < 0.6


def test_index_dot_product_identity_against_the_forward_restatement():
    """<lookup(V), G> = <V, lookup^T(G)> with the forward of corr_ref.lookup_f64 on a scene where ITS fp16 steps are exact
    (integer volume, quarter fractions: weights multiples of 1/16, sums of at most 4 * 4 * 15 / 16)"""
    N, h1, w1, h2, w2, radius = 2, 5, 7, 6, 9, 3
    coords, grad = RB.dyadic_index_scene(2, N, h1, w1, h2, w2, radius)
    vol = np.random.default_rng(3).integers(-4, 5, (N, h1, w1, h2, w2)).astype(np.float16)
    fwd = R.lookup_f64([vol], coords, radius).astype(F64).reshape(N, 7, 7, h1, w1)
    lhs = (fwd * grad).sum()
    rhs = (vol.astype(F64) * RB.index_bwd_f64(coords, grad, h2, w2, radius)).sum()
    assert lhs == rhs and lhs != 0.0


@pytest.mark.parametrize("radius", [3, 1])
def test_dyadic_index_scene_is_exact_in_both_dtypes(radius):
    """every partial sum is a multiple of 1/16 bounded by the sum of the magnitudes: exact in fp16 (11 bits) and fp32, so a
    float16 and a float32 evaluation both equal the float64 one"""
    for (h1, w1, h2, w2) in ((5, 7, 6, 9), (3, 5, 60, 80)):
        coords, grad = RB.dyadic_index_scene(1, 2, h1, w1, h2, w2, radius)
        frac = coords[np.abs(coords) < 1e6]
        assert RB._lsb_exp(frac - np.floor(frac)) == 2
        mag = RB.index_bwd_f64(coords, grad, h2, w2, radius, absolute=True)
        RB.assert_exact(mag, 4, 11, "fp16")
        want = RB.index_bwd_f64(coords, grad, h2, w2, radius)
        assert RB.fp16_exact(want)
        # the scene has what it was written for
        x, y = coords[:, 0], coords[:, 1]
        assert (np.abs(coords) > 1e9).any() and ((x < 0) & (x != np.floor(x))).any() and (coords == np.floor(coords)).any()
        assert ((x < -radius - 1) | (x > w2 + radius)).any() and ((x > -radius - 1) & (x < 0)).any()
        cnt = RB.index_bwd_f64(coords, grad, h2, w2, radius, count=True)
        assert cnt.max() == 4 and (cnt.reshape(2, h1 * w1, -1).sum(-1) == 0).any()        # interior taps, and empty planes


def test_pyramid_restatement_is_the_four_level_calls():
    N, h1, w1, h2, w2, radius = 2, 3, 4, 13, 21, 3
    rng = np.random.default_rng(5)
    coords = np.stack([rng.uniform(-6, w2 + 6, (N, h1, w1)), rng.uniform(-6, h2 + 6, (N, h1, w1))], 1).astype(np.float32)
    grad = rng.standard_normal((N, 4 * 49, h1, w1))
    got = RB.pyramid_bwd_f64(coords, grad, h2, w2, radius, 4)
    assert [g.shape[3:] for g in got] == [(13, 21), (6, 10), (3, 5), (1, 2)]
    vols = [_t(np.zeros(g.shape), grad=True) for g in got]
    out = torch.cat([RB.lookup_torch(v, _t(coords) / 2 ** l, radius).reshape(N, 49, h1, w1) for l, v in enumerate(vols)], 1)
    out.backward(_t(grad))
    for g, v in zip(got, vols):
        assert np.abs(g - v.grad.numpy()).max() <= 1e-15 * np.abs(g).max()


# ---- alt-corr backward ------------------------------------------------------------------------------------------------------
ALT_SIZES = [((5, 7), (6, 9)), ((9, 11), (4, 5))]


@pytest.mark.parametrize("kind", ["smooth", "scatter"])
@pytest.mark.parametrize("hw,hw2", ALT_SIZES)
def test_altcorr_adjoint_equals_autograd(kind, hw, hw2):
    f1, f2, coords, grad = RB.altcorr_bwd_scene(3, 2, 3, *hw, *hw2, 8, kind)
    t1, t2 = _t(f1.astype(F64), grad=True), _t(f2.astype(F64), grad=True)
    RB.altcorr_torch(t1, t2, _t(coords), 3).backward(_t(grad.astype(F64)))
    g1, g2 = RB.altcorr_bwd_f64(f1, f2, coords, grad, 3)
    assert np.abs(g1 - t1.grad.numpy()).max() == 0.0 and np.abs(g2 - t2.grad.numpy()).max() == 0.0
    assert np.abs(g1).max() > 0 and np.abs(g2).max() > 0


def test_altcorr_dot_product_identity_against_the_forward_restatement():
    f1, f2, coords, grad = RB.altcorr_bwd_scene(4, 2, 3, 5, 7, 6, 9, 40, "smooth")
    fwd = R.altcorr_f64(f1, f2, coords, 3)
    g1, g2 = RB.altcorr_bwd_f64(f1, f2, coords, grad, 3)
    lhs = (fwd * grad).sum()
    # the forward is bilinear in (f1, f2): <J_1 f1, G> = <J_2 f2, G> = <out, G>
    assert lhs == (f1.astype(F64) * g1).sum() == (f2.astype(F64) * g2).sum() and lhs != 0.0


@pytest.mark.parametrize("C", [128, 40])
@pytest.mark.parametrize("S", [1, 3])
@pytest.mark.parametrize("hw,hw2", ALT_SIZES)
def test_altcorr_scenes_are_exact_and_reach_their_branch(C, S, hw, hw2):
    for kind, branch in (("smooth", RB.BOXED), ("scatter", RB.PER_TAP)):
        f1, f2, coords, grad = RB.altcorr_bwd_scene(7, 2, S, *hw, *hw2, C, kind)
        plan = RB.altcorr_bwd_plan(coords, C)
        if kind == "smooth":
            assert (plan == RB.BOXED).all()
        else:
            assert (plan == RB.PER_TAP).mean() > 0.5
        m1, m2 = RB.altcorr_bwd_f64(f1, f2, coords, grad, 3, absolute=True)
        RB.assert_exact(m1, 4, 24, "fmap1_grad")
        RB.assert_exact(m2, 4, 24, "fmap2_grad")
        c1, c2 = RB.altcorr_bwd_f64(f1, f2, coords, grad, 3, count=True)
        assert c2.max() > 4 * S                                   # destinations shared between source pixels
        assert (c1.reshape(2, -1, C)[..., 0] < 4 * 49 * S).any()  # windows that leave the target map


# ---- projmap ------------------------------------------------------------------------------------------------------------------
def test_projmap_scene_populations():
    s = RB.projmap_scene()
    coords, valid, X = RB.projmap64(**s)
    Z = X[..., 2]
    firm = RB.projmap_firm(X)
    assert 1.0 - firm.mean() <= 0.02                              # the condition of the GPU test
    behind, between, front = (Z <= RB.Z_GRID).mean(), ((Z > RB.Z_GRID) & (Z <= RB.Z_VALID)).mean(), (Z > RB.Z_VALID).mean()
    print(f"projmap scene: excluded {1 - firm.mean():.4f}, behind {behind:.3f}, between {between:.3f}, valid {front:.3f}")
    assert behind > 0.15 and between > 0.03 and front > 0.3
    assert s["intrinsics"][0] != s["intrinsics"][1]
    # the grid fallback is the pixel grid, the projection differs from it
    y, x = np.meshgrid(np.arange(11.0), np.arange(13.0), indexing="ij")
    back = Z <= RB.Z_GRID
    assert np.array_equal(coords[back], np.stack([x, y], -1)[None].repeat(len(Z), 0)[back])
    assert (np.abs(coords[~back] - np.stack([x, y], -1)[None].repeat(len(Z), 0)[~back]) > 1.0).mean() > 0.5
    assert np.array_equal(valid[..., 0], (Z > 0.25).astype(F64))
    bound = RB.projmap_coord_bound(s, X)
    assert np.isfinite(bound).all() and np.median(bound[firm & ~back]) < 1e-3


def test_projmap64_agrees_with_the_reprojection_reference_in_front_of_the_camera():
    """same projection as geom_ref.reproject64 (shared intrinsics) where neither fallback applies"""
    import geom_ref as G
    s = RB.projmap_scene()
    coords, _, X = RB.projmap64(**s)
    intr = np.tile(s["intrinsics"][None], (len(s["poses"]), 1))
    want, Z = G.reproject64(s["poses"], s["disps"], intr, s["ii"], s["jj"])
    m = Z > 0.1
    assert np.abs(coords[m] - want[m]).max() < 1e-9
