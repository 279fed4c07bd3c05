"""The adjoints of the correlation lookups (csrc/corr_bwd.hip), the autograd functions on top of them and projmap, against the
float64 restatements of tests/corr_bwd_ref.py (pinned without a GPU by tests/test_corr_bwd_ref.py).

On the dyadic / integer scenes every partial sum is exact in the tested dtype, so the comparison is bit for bit and neither an
accumulation type nor an order of float atomics can hide behind a tolerance.  On general data the bounds are derived here from
the number of fp32 roundings per term, in units of u = 2^-24 times the sum of the magnitudes of the terms (which the
restatements return with absolute=True); the worst ratio to the bound is printed."""
import functools

import numpy as np
import pytest
import torch

import corr_bwd_ref as RB

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
# roundings on one term g * (a * b) of a tap gradient and on the <= 4-term sum: the complements 1 - dx and 1 - dy, the weight
# product, the product with the gradient, three adds
TAP_ROUNDINGS = 7


def _gamma(n):
    return n * U / (1.0 - n * U)


def _dev(x, gpu, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(x))
    return (t if dtype is None else t.to(dtype)).to(gpu)


def _index_bwd(gpu, coords, grad, h2, w2, radius, dtype):
    """corr_index_backward through the C ABI with the output pre-filled with NaN (the launch must overwrite every element)"""
    import glorie_slam_amd._lib as L
    N, _, h1, w1 = coords.shape
    c, g = _dev(coords, gpu), _dev(grad, gpu, dtype)
    out = torch.full((N, h1, w1, h2, w2), float("nan"), dtype=dtype, device=gpu)
    L.check(L.load().glorie_corr_index_bwd(L.ptr(c), L.ptr(g), L.ptr(out), N, h1, w1, h2, w2, radius, L.dtype_code(out),
                                           L.stream_ptr()), "glorie_corr_index_bwd")
    return out


# ---- index backward, bit for bit ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float16, torch.float32], ids=["f16", "f32"])
@pytest.mark.parametrize("shape,radius", [((5, 7, 6, 9), 3), ((5, 7, 6, 9), 1), ((3, 5, 60, 80), 3)],
                         ids=["5x7-6x9-r3", "5x7-6x9-r1", "3x5-60x80-r3"])
def test_index_backward_bit_exact_on_dyadic_scenes(gpu, shape, radius, dtype):
    """quarter fractions, integer gradients: exact in fp16 and fp32 (test_corr_bwd_ref.py proves it), NaN pre-fill, planes
    whose byte offset is no multiple of 16 (6 x 9), planes of several store passes (60 x 80), windows half and wholly outside,
    floor against truncation, +-3e9"""
    from glorie_slam_amd import droid_backends as db
    h1, w1, h2, w2 = shape
    coords, grad = RB.dyadic_index_scene(1, 2, h1, w1, h2, w2, radius)
    want = RB.index_bwd_f64(coords, grad, h2, w2, radius)
    got = _index_bwd(gpu, coords, grad, h2, w2, radius, dtype)
    assert got.dtype == dtype and not torch.isnan(got).any(), "an element was not written"
    ne = got.double().cpu().numpy() != want
    assert not ne.any(), f"{int(ne.sum())} of {ne.size} differ, first at {np.argwhere(ne)[0]}"
    # the binding: same values, the reference's return list
    vol = torch.empty((2, h1, w1, h2, w2), dtype=dtype, device=gpu)
    out, = db.corr_index_backward(vol, _dev(coords, gpu), _dev(grad, gpu, dtype), radius)
    assert out.shape == vol.shape and torch.equal(out, got)
    again, = db.corr_index_backward(vol, _dev(coords, gpu), _dev(grad, gpu, dtype), radius)
    assert torch.equal(out, again)


@pytest.mark.parametrize("dtype", [torch.float16, torch.float32], ids=["f16", "f32"])
def test_index_backward_general_data_within_derived_bound(gpu, dtype):
    """f32: |err| <= gamma_7 sum |terms| (TAP_ROUNDINGS above; contraction into FMAs only removes roundings).  f16: the fp32
    value rounded once: 2^-11 (|exact| + e32) + e32 + the subnormal floor 2^-25"""
    N, h1, w1, h2, w2, radius = 2, 5, 7, 6, 9, 3
    rng = np.random.default_rng(17)
    coords = np.stack([rng.uniform(-5, w2 + 5, (N, h1, w1)), rng.uniform(-5, h2 + 5, (N, h1, w1))], 1).astype(np.float32)
    grad = rng.standard_normal((N, 7, 7, h1, w1)).astype(np.float16 if dtype == torch.float16 else np.float32)
    want = RB.index_bwd_f64(coords, grad, h2, w2, radius)
    mag = RB.index_bwd_f64(coords, grad, h2, w2, radius, absolute=True)
    got = _index_bwd(gpu, coords, grad, h2, w2, radius, dtype).double().cpu().numpy()
    e32 = _gamma(TAP_ROUNDINGS) * mag
    bound = e32 if dtype == torch.float32 else 2.0 ** -11 * (np.abs(want) + e32) + e32 + 2.0 ** -25
    err = np.abs(got - want)
    nz = bound > 0
    print(f"index backward general {dtype}: worst |err| / bound = {(err[nz] / bound[nz]).max():.3f}, max |err| {err.max():.3e}")
    assert np.all(got[~nz] == 0.0) and np.all(err <= bound) and err.max() > 0


def test_index_backward_beyond_2_31_elements(gpu):
    """N = 94 edges of 60 x 80 -> 60 x 80 in fp16: 2.17e9 elements, 4.3 GB.  Dyadic scene, so every element and the float64 sum of
    the whole tensor are exact: the first plane, the last one and those on either side of element 2^31 against the reference,
    the sum against the sum the reference predicts"""
    free, _ = torch.cuda.mem_get_info(gpu)
    if free < 12 << 30:
        pytest.skip("less than 12 GB of device memory free")
    N, h, w, radius = 94, 60, 80, 3
    coords, grad = RB.dyadic_index_scene(3, N, h, w, h, w, radius)
    assert N * h * w * h * w > 2 ** 31
    got = _index_bwd(gpu, coords, grad, h, w, radius, torch.float16)
    # predicted sum: every in-bounds term g wx wy, without materialising the tensor
    x0, dx = RB._window(coords[:, 0], radius)
    y0, dy = RB._window(coords[:, 1], radius)
    total = 0.0
    for i in range(7):
        for j in range(7):
            for a, wx in ((0, 1.0 - dx), (1, dx)):
                for b, wy in ((0, 1.0 - dy), (1, dy)):
                    tx, ty = x0 + i + a, y0 + j + b
                    inb = (tx >= 0) & (tx < w) & (ty >= 0) & (ty < h)
                    total += float((grad[:, i, j] * wx * wy)[inb].sum())
    flat = got.view(N * h * w, h * w)
    edge = 2 ** 31 // (h * w)
    for pix in (0, edge - 1, edge, edge + 1, N * h * w - 1):
        n, p = divmod(pix, h * w)
        y, x = divmod(p, w)
        want = RB.index_bwd_f64(coords[n:n + 1, :, y:y + 1, x:x + 1], grad[n:n + 1, :, :, y:y + 1, x:x + 1], h, w, radius)
        assert np.array_equal(flat[pix].double().cpu().numpy(), want.reshape(-1)), f"plane {pix}"
    s = 0.0
    for k in range(0, N * h * w, 1 << 15):                      # float64 sums of multiples of 1/16: exact
        s += float(flat[k:k + (1 << 15)].sum(dtype=torch.float64))
    assert s == total and total != 0.0


# ---- pyramid backward ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float16, torch.float32], ids=["f16", "f32"])
@pytest.mark.parametrize("h2,w2", [(12, 20), (13, 21)])
def test_pyramid_backward_equals_four_index_calls(gpu, h2, w2, dtype):
    """one launch for all levels == corr_index_backward on coords / 2^l per level, bit for bit; odd sizes: >> l truncates"""
    from glorie_slam_amd import droid_backends as db
    N, h1, w1, radius = 2, 5, 7, 3
    rng = np.random.default_rng(h2)
    coords = _dev(np.stack([rng.uniform(-9, w2 + 9, (N, h1, w1)), rng.uniform(-9, h2 + 9, (N, h1, w1))], 1).astype(np.float32), gpu)
    grad = _dev(rng.standard_normal((N, 4 * 49, h1, w1)).astype(np.float32), gpu, dtype)
    shapes = [(N, h1, w1, h2 >> l, w2 >> l) for l in range(4)]
    got = db.corr_lookup_pyramid_backward(shapes, coords, grad, radius)
    ref64 = RB.pyramid_bwd_f64(coords.cpu().numpy(), grad.double().cpu().numpy(), h2, w2, radius, 4)
    for l in range(4):
        vol = torch.empty(shapes[l], dtype=dtype, device=gpu)
        want, = db.corr_index_backward(vol, coords / 2 ** l, grad[:, l * 49:(l + 1) * 49].contiguous(), radius)
        assert got[l].shape == want.shape and torch.equal(got[l], want), f"level {l}"
        # ... and it is the adjoint: the per-level bound of the general-data test (fp16: one rounding of the fp32 value)
        mag = RB.index_bwd_f64((coords / 2 ** l).cpu().numpy(), grad[:, l * 49:(l + 1) * 49].double().cpu().numpy(), h2 >> l,
                               w2 >> l, radius, absolute=True)
        e32 = _gamma(TAP_ROUNDINGS) * mag
        bound = e32 if dtype == torch.float32 else 2.0 ** -11 * (np.abs(ref64[l]) + e32) + e32 + 2.0 ** -25
        assert np.all(np.abs(got[l].double().cpu().numpy() - ref64[l]) <= bound), f"level {l}"


# ---- alt-corr backward ----------------------------------------------------------------------------------------------------------
ALT_SIZES = [((5, 7), (6, 9)), ((9, 11), (4, 5))]


def _altcorr_bwd(gpu, f1, f2, coords, grad, radius=3):
    from glorie_slam_amd import droid_backends as db
    g1, g2, gc = db.altcorr_backward(_dev(f1, gpu), _dev(f2, gpu), _dev(coords, gpu), _dev(grad, gpu), radius)
    assert gc.shape == coords.shape and not gc.any()
    return g1, g2


@pytest.mark.parametrize("kind", ["smooth", "scatter"])
@pytest.mark.parametrize("C", [128, 40])
@pytest.mark.parametrize("S", [1, 3])
@pytest.mark.parametrize("hw,hw2", ALT_SIZES, ids=["5x7-6x9", "9x11-4x5"])
def test_altcorr_backward_bit_exact_on_integer_scenes(gpu, hw, hw2, S, C, kind):
    """integer features and gradients, quarter coordinates: every partial sum is exact in fp32 (proved on the CPU), so the
    order of the float atomics cannot matter: both gradients equal float64 bit for bit, with smooth coordinates
    (every tile pre-sums over its box) and with scattered ones (per-tap atomic rows), and two calls agree bitwise"""
    f1, f2, coords, grad = RB.altcorr_bwd_scene(7, 2, S, *hw, *hw2, C, kind)
    plan = RB.altcorr_bwd_plan(coords, C)
    assert (plan == RB.BOXED).all() if kind == "smooth" else (plan == RB.PER_TAP).mean() > 0.5
    w1, w2 = RB.altcorr_bwd_f64(f1, f2, coords, grad, 3)
    g1, g2 = _altcorr_bwd(gpu, f1, f2, coords, grad)
    for name, got, want in (("fmap1_grad", g1, w1), ("fmap2_grad", g2, w2)):
        ne = got.double().cpu().numpy() != want
        assert not ne.any(), f"{name}: {int(ne.sum())} of {ne.size} differ, first at {np.argwhere(ne)[0]}"
    h1, h2 = _altcorr_bwd(gpu, f1, f2, coords, grad)
    assert torch.equal(g1, h1) and torch.equal(g2, h2)


@pytest.mark.parametrize("kind", ["smooth", "scatter"])
@pytest.mark.parametrize("hw,hw2", ALT_SIZES, ids=["5x7-6x9", "9x11-4x5"])
def test_altcorr_backward_general_data_within_derived_bounds(gpu, hw, hw2, kind):
    """t = the tap gradient carries TAP_ROUNDINGS roundings.  fmap1_grad: n FMAs in a fixed order, n <= the number of terms of
    the element: (7 + n) u sum |terms|.  fmap2_grad: one rounded product per term and n - 1 float atomic adds in ANY order:
    (7 + 1 + n - 1) u sum |terms| - a bound that grows with the number of terms per destination"""
    B, S, C = 2, 2, 128
    rng = np.random.default_rng(23)
    f1 = (rng.standard_normal((B, *hw, C)) * 0.25).astype(np.float32)
    f2 = (rng.standard_normal((B, *hw2, C)) * 0.25).astype(np.float32)
    grad = rng.standard_normal((B, S, 49, *hw)).astype(np.float32)
    _, _, base, _ = RB.altcorr_bwd_scene(7, B, S, *hw, *hw2, C, kind)
    coords = (base + rng.uniform(-0.5, 0.5, base.shape)).astype(np.float32)
    plan = RB.altcorr_bwd_plan(coords, C)
    assert (plan == RB.BOXED).mean() > 0.9 if kind == "smooth" else (plan == RB.PER_TAP).mean() > 0.5
    w1, w2 = RB.altcorr_bwd_f64(f1, f2, coords, grad, 3)
    m1, m2 = RB.altcorr_bwd_f64(f1, f2, coords, grad, 3, absolute=True)
    n1, n2 = RB.altcorr_bwd_f64(f1, f2, coords, grad, 3, count=True)
    g1, g2 = _altcorr_bwd(gpu, f1, f2, coords, grad)
    for name, got, want, mag, n in (("fmap1_grad", g1, w1, m1, n1), ("fmap2_grad", g2, w2, m2, n2)):
        bound = (TAP_ROUNDINGS + n) * U * mag * (1 + 1e-4)
        err = np.abs(got.double().cpu().numpy() - want)
        nz = bound > 0
        print(f"altcorr backward general {kind} {hw}->{hw2} {name}: worst |err| / bound = {(err[nz] / bound[nz]).max():.3f}, "
              f"terms per element up to {int(n.max())}")
        assert np.all(err[~nz] == 0.0) and np.all(err <= bound) and err.max() > 0


# ---- autograd end to end ---------------------------------------------------------------------------------------------------
E2E_II, E2E_JJ = [0, 2], [1, 0]


@functools.lru_cache(maxsize=None)
def _e2e_scene():
    """3 frames of 16 channels on 8 x 12, 2 edges, a random cotangent; the float64 gradients of both compositions w.r.t. the
    frames, and the sums of the magnitudes of their terms (the same compositions on magnitudes: every weight is >= 0)"""
    rng = np.random.default_rng(31)
    F_, C, h, w = 3, 16, 8, 12
    fm = rng.standard_normal((1, F_, C, h, w)).astype(np.float32)
    coords = np.stack([rng.uniform(-2, w + 2, (1, 2, h, w)), rng.uniform(-2, h + 2, (1, 2, h, w))], -1).astype(np.float32)
    cot = rng.standard_normal((1, 2, 196, h, w)).astype(np.float32)
    ii, jj = torch.tensor(E2E_II), torch.tensor(E2E_JJ)
    out = {}
    for tag, sign in (("grad", False), ("mag", True)):
        for block in ("corr", "alt"):
            f = torch.from_numpy(np.abs(fm) if sign else fm).double().requires_grad_(True)
            c = torch.from_numpy(coords)
            if block == "corr":
                o = RB.corr_block_torch(f[:, ii], f[:, jj], c)
            else:
                o = RB.altcorr_block_torch(f, c, ii, jj)
            o.backward(torch.from_numpy(np.abs(cot) if sign else cot).double())
            out[block, tag] = f.grad.numpy()
            if not sign:
                out[block, "fwd"] = o.detach().numpy()
    return fm, coords, cot, out


# roundings per term: the tap gradient, the sum over the four levels (3 adds; the pooling adjoint only scales by 1/4) and
#   CorrBlock: the all-pairs matmul adjoint, one sum over the h w = 96 positions of the other map, two exact scalings
#   AltCorrBlock: every (edge, level, source pixel or tap) that reaches an element adds once: <= N L (h w + 64) adds
E2E_ROUNDINGS = {"corr": TAP_ROUNDINGS + 3 + 96 + 4, "alt": TAP_ROUNDINGS + 3 + 2 * 4 * (96 + 64) + 4}


def _e2e_gpu(gpu, block):
    from glorie_slam_amd.droid_net import AltCorrBlock, CorrBlock
    fm, coords, cot, _ = _e2e_scene()
    f = _dev(fm, gpu).requires_grad_(True)
    c = _dev(coords, gpu)
    ii, jj = torch.tensor(E2E_II, device=gpu), torch.tensor(E2E_JJ, device=gpu)
    if block == "corr":
        blk = CorrBlock(f[:, ii], f[:, jj], tiled=None)
        assert not blk.tiled
        o = blk(c)
    else:
        o = AltCorrBlock(f)(c, ii, jj)
    assert o.requires_grad
    o.backward(_dev(cot, gpu))
    with torch.no_grad():
        plain = CorrBlock(f[:, ii], f[:, jj], tiled=None)(c) if block == "corr" else AltCorrBlock(f)(c, ii, jj)
    assert not plain.requires_grad and torch.equal(plain, o.detach()), "the forward under autograd is not the no-grad forward"
    return o.detach().double().cpu().numpy(), f.grad.double().cpu().numpy()


@pytest.mark.parametrize("block", ["corr", "alt"])
def test_autograd_through_the_blocks_matches_float64(gpu, block):
    """float32 maps that require grad, .backward() of a random cotangent: the gradient w.r.t. the frames (both roles: fmap1
    and fmap2) against autograd through the pure-torch float64 composition of the same block"""
    _, _, _, ref = _e2e_scene()
    fwd, grad = _e2e_gpu(gpu, block)
    assert fwd.shape == ref[block, "fwd"].shape
    bound = E2E_ROUNDINGS[block] * U * ref[block, "mag"] * (1 + 1e-4)
    err = np.abs(grad - ref[block, "grad"])
    print(f"autograd {block}: worst |err| / bound = {(err / bound).max():.3f}, max |grad| {np.abs(grad).max():.3f}")
    assert np.all(err <= bound) and np.abs(grad).max() > 0
    assert np.abs(grad[0, 1]).max() > 0 and np.abs(grad[0, 2]).max() > 0       # frame 1 is a target only, frame 2 a source only


def test_both_blocks_give_the_same_feature_gradients(gpu):
    """they compute the same function by different kernels: within the sum of their bounds"""
    _, _, _, ref = _e2e_scene()
    assert np.abs(ref["corr", "grad"] - ref["alt", "grad"]).max() <= 1e-12 * np.abs(ref["corr", "grad"]).max()
    g_corr, g_alt = _e2e_gpu(gpu, "corr")[1], _e2e_gpu(gpu, "alt")[1]
    bound = (E2E_ROUNDINGS["corr"] * ref["corr", "mag"] + E2E_ROUNDINGS["alt"] * ref["alt", "mag"]) * U * (1 + 1e-4)
    assert np.all(np.abs(g_corr - g_alt) <= bound)


def test_no_grad_keeps_the_tiled_pyramid_and_tiled_with_grad_raises(gpu):
    from glorie_slam_amd.droid_net import CorrBlock
    fm, coords, _, _ = _e2e_scene()
    f = _dev(fm, gpu).half()
    c = _dev(coords, gpu)
    with torch.no_grad():
        blk = CorrBlock(f[:, E2E_II], f[:, E2E_JJ], tiled=None)
        assert blk.tiled
        want = CorrBlock(f[:, E2E_II], f[:, E2E_JJ], tiled=False)(c)
        assert torch.equal(blk(c), want)
    fg = f.clone().requires_grad_(True)
    assert CorrBlock(f[:, E2E_II], f[:, E2E_JJ], tiled=None).tiled          # grad mode on, nothing requires grad: as before
    blk = CorrBlock(fg[:, E2E_II], fg[:, E2E_JJ], tiled=None)
    assert not blk.tiled
    out = blk(c)
    assert torch.equal(out.detach(), want)                                    # fp16: the same values as the no-grad path
    out.float().sum().backward()
    assert fg.grad is not None and fg.grad.abs().max() > 0
    with pytest.raises(RuntimeError, match="tiled"):
        CorrBlock(fg[:, E2E_II], fg[:, E2E_JJ], tiled=True)
    with torch.no_grad():
        assert CorrBlock(fg[:, E2E_II], fg[:, E2E_JJ], tiled=True).tiled


def test_autograd_functions_have_the_reference_signatures(gpu):
    from glorie_slam_amd.droid_net import CorrLayer, CorrSampler
    coords, grad = RB.dyadic_index_scene(1, 2, 5, 7, 6, 9, 3)
    # CorrSampler runs the FORWARD lookup too, whose contract for huge coordinates is +-1e7 (corr_ref.scene_huge)
    coords = np.clip(coords, -1.0e7, 1.0e7)
    vol = torch.zeros((2, 5, 7, 6, 9), device=gpu, requires_grad=True)
    CorrSampler.apply(vol, _dev(coords, gpu), 3).backward(_dev(grad, gpu, torch.float32))
    assert np.array_equal(vol.grad.double().cpu().numpy(), RB.index_bwd_f64(coords, grad, 6, 9, 3))
    f1, f2, c, g = RB.altcorr_bwd_scene(7, 2, 1, 5, 7, 6, 9, 40, "smooth")
    t1, t2 = _dev(f1, gpu).requires_grad_(True), _dev(f2, gpu).requires_grad_(True)
    tc = _dev(c, gpu).requires_grad_(True)
    CorrLayer.apply(t1, t2, tc, 3).backward(_dev(g.reshape(2, 1, 49, 5, 7), gpu))
    w1, w2 = RB.altcorr_bwd_f64(f1, f2, c, g, 3)
    assert np.array_equal(t1.grad.double().cpu().numpy(), w1) and np.array_equal(t2.grad.double().cpu().numpy(), w2)
    assert tc.grad is not None and not tc.grad.any()                          # the reference's third output: zeros


# ---- projmap ----------------------------------------------------------------------------------------------------------------
def test_projmap_against_float64(gpu):
    """valid and the grid fallback exact on pixels whose Z is farther than 1e-3 from 0.01 and 0.25 (at most 2 % are not:
    asserted on the CPU), coordinates within the fp32 bound of corr_bwd_ref.projmap_coord_bound"""
    from glorie_slam_amd import droid_backends as db
    s = RB.projmap_scene()
    want_c, want_v, X = RB.projmap64(**s)
    firm = RB.projmap_firm(X)
    coords, valid = db.projmap(*[_dev(s[k], gpu) for k in ("poses", "disps", "intrinsics", "ii", "jj")])
    N, h, w = X.shape[:3]
    assert coords.shape == (N, h, w, 2) and valid.shape == (N, h, w, 1) and coords.dtype == valid.dtype == torch.float32
    coords, valid = coords.double().cpu().numpy(), valid.double().cpu().numpy()
    assert np.array_equal(valid[firm], want_v[firm])
    back = X[..., 2] <= RB.Z_GRID
    assert np.array_equal(coords[firm & back], want_c[firm & back])          # the pixel grid itself
    front = firm & ~back
    bound = RB.projmap_coord_bound(s, X)
    err = np.abs(coords - want_c)
    print(f"projmap: worst |err| / bound = {(err[front] / bound[front]).max():.3f}, max |err| {err[front].max():.3e} px, "
          f"{front.mean():.2f} projected, {(firm & back).mean():.2f} on the grid, {1 - firm.mean():.4f} excluded")
    assert np.all(err[front] <= bound[front])


# ---- argument errors --------------------------------------------------------------------------------------------------------
def test_argument_errors(gpu):
    from glorie_slam_amd import _lib, droid_backends as db
    vol = torch.zeros((1, 2, 3, 4, 5), dtype=torch.float16, device=gpu)
    coords = torch.zeros((1, 2, 2, 3), device=gpu)
    g = torch.zeros((1, 7, 7, 2, 3), dtype=torch.float16, device=gpu)
    with pytest.raises(RuntimeError, match="contiguous"):
        db.corr_index_backward(vol, coords, g.permute(0, 2, 1, 3, 4), 3)
    with pytest.raises(RuntimeError, match="dtype"):
        db.corr_index_backward(vol, coords, g.float(), 3)
    with pytest.raises(RuntimeError, match="float32"):
        db.corr_index_backward(vol, coords.double(), g, 3)
    with pytest.raises(_lib.GlorieError):
        db.corr_index_backward(vol, coords.cpu(), g, 3)
    with pytest.raises(_lib.GlorieError):
        db.corr_lookup_pyramid_backward([(1, 2, 3, 4, 5)], coords, torch.zeros((1, 49, 2, 3)), 3)
    f1 = torch.zeros((1, 2, 3, 8), device=gpu)
    f2 = torch.zeros((1, 4, 5, 8), device=gpu)
    c = torch.zeros((1, 1, 2, 3, 2), device=gpu)
    cg = torch.zeros((1, 1, 49, 2, 3), device=gpu)
    with pytest.raises(RuntimeError, match="float32"):
        db.altcorr_backward(f1.half(), f2, c, cg, 3)
    with pytest.raises(RuntimeError, match="contiguous"):
        db.altcorr_backward(f1, f2.permute(0, 2, 1, 3), c, cg, 3)
    with pytest.raises(_lib.GlorieError):
        db.altcorr_backward(f1, f2, c.cpu(), cg, 3)
    s = RB.projmap_scene()
    a = {k: _dev(s[k], gpu) for k in ("poses", "disps", "intrinsics", "ii", "jj")}
    with pytest.raises(RuntimeError, match="int64"):
        db.projmap(a["poses"], a["disps"], a["intrinsics"], a["ii"].int(), a["jj"])
    with pytest.raises(RuntimeError, match="contiguous"):
        db.projmap(a["poses"], a["disps"].transpose(1, 2), a["intrinsics"], a["ii"], a["jj"])
    with pytest.raises(_lib.GlorieError):
        db.projmap(a["poses"].cpu(), a["disps"], a["intrinsics"], a["ii"], a["jj"])
    # N == 0 returns without a launch
    out, = db.corr_index_backward(vol[:0], coords[:0], g[:0], 3)
    assert out.shape == (0, 2, 3, 4, 5)
