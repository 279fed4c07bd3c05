"""The claims that tests/test_gpu_corr_exact.py rests on, checked without a GPU: the scene builders of tests/corr_ref.py
really are order-free / encoder-exact, every coordinate scene reaches the kernel branches it names at every map size the
GPU tests use, and the float64 restatements agree with the oracle."""
import numpy as np
import pytest

import corr_ref as R
from oracle import corr as ocorr


def _seq_dot_fp32(a, b, order):
    """sum_c a[c, p] b[c, q] accumulated sequentially in fp32 in the given channel order (fp32 products, unfused)"""
    acc = np.zeros((a.shape[1], b.shape[1]), np.float32)
    for c in order:
        acc = acc + a[c][:, None] * b[c][None, :]
    return acc


def test_order_free_dense_scene_is_order_independent_and_fp16_exact():
    """{-8,-4,0,4,8}, 128 channels, 16 x 24: every level's dot products are the same exact number in float64 and in fp32
    under two channel orders, and survive the rounding to fp16"""
    h, w = 16, 24
    fm = R.order_free_features(1, 3, h, w)
    assert R.assert_order_free(fm, R.OTF_II, R.OTF_JJ) <= 128 * 4
    levels = ocorr.otf_pyramid(fm)
    rng = np.random.default_rng(0)
    fwd, perm = np.arange(128), rng.permutation(128)
    for l, fl in enumerate(levels):
        a32 = levels[0][0].astype(np.float32).reshape(128, -1)
        b32 = fl[1].astype(np.float32).reshape(128, -1)
        exact = a32.astype(np.float64).T @ b32.astype(np.float64)
        s0, s1 = _seq_dot_fp32(a32, b32, fwd), _seq_dot_fp32(a32, b32, perm)
        assert np.array_equal(s0.astype(np.float64), exact) and np.array_equal(s1.astype(np.float64), exact), f"level {l}"
        assert np.array_equal(exact.astype(np.float16).astype(np.float64), exact), f"level {l}"
        assert np.array_equal((a32.T @ b32).astype(np.float64), exact)            # and a BLAS order


def test_order_free_builder_rejects_general_features():
    fm = np.random.default_rng(0).standard_normal((2, 128, 8, 8)).astype(np.float16)
    with pytest.raises(AssertionError):
        R.assert_order_free(fm, [0], [1])


@pytest.mark.parametrize("h,w", R.SIZES_ALL)
def test_order_free_scenes_of_the_gpu_tests(h, w):
    R.order_free_features(h * 100 + w, 3, h, w)                                   # the builder asserts
    R.otf_integer_scene(7, 3, h, w)


@pytest.mark.parametrize("h,w", R.SIZES_ALL)
@pytest.mark.parametrize("name", list(R.OTF_SCENES))
def test_box_plan_reaches_every_intended_branch(name, h, w):
    R.check_plan(name, h, w)
    for nl in (1, 2, 3):
        R.check_plan(name, h, w, nl)


def test_box_plan_rule():
    h, w = 16, 24
    c = np.zeros((2, h, w), np.float32) + 5.5
    br, area = R.box_plan(c, h, w)
    assert (br == R.SHARED).all() and (area == 64).all()
    _, a320 = R.box_plan(R.scene_box320(h, w), h, w)
    _, a336 = R.box_plan(R.scene_box336(h, w), h, w)
    assert (a320[:, :, 0] == 320).all() and (a336[:, :, 0] == 336).all()
    br, area = R.box_plan(R.scene_scale3(h, w), h, w)
    assert (area[:, :, 0] == 29 * 29).all() and (br[:, :, 0] == R.QUADS).all() and (br[:, :, 1] == R.QUADS).all()
    assert (br[:, :, 2:] == R.SHARED).all()
    # floor, not truncation, and the clamp of large magnitudes
    c = np.zeros((2, 8, 8), np.float32)
    c[0, 0, 0], c[0, 0, 1] = -0.25, -1.0e7
    _, area = R.box_plan(c, 8, 8, 1)
    assert area[0, 0, 0] == (0 - (-1000000) + 8) * 8


def test_huge_scene_is_all_zero_in_the_oracle():
    h, w = 16, 24
    fm = R.order_free_features(1, 3, h, w)
    vols = R.otf_volumes(fm, R.OTF_II[:1], R.OTF_JJ[:1])
    out = R.otf_lookup(vols, R.scene_huge(h, w)[None])
    assert not out.view(np.uint16).any()


def test_otf_oracle_equals_float64_restatement():
    """oracle.corr.corr_otf on an order-free scene == the float64 evaluation rounded once per pinned step, and == the
    shared-volume form the GPU tests use"""
    h, w = 12, 16
    fm = R.order_free_features(h * 100 + w, 3, h, w)
    coords, ii, jj, _ = R.otf_scene_coords(h, w, ["box336", "one_quadrant", "left", "up", "scatter"])
    ref = ocorr.corr_otf(fm, coords, ii, jj)
    vols = R.otf_volumes(fm, ii, jj)
    assert np.array_equal(R.otf_lookup(vols, coords).view(np.uint16), ref.view(np.uint16))
    f64 = R.lookup_f64(vols, coords)
    assert np.array_equal(f64.view(np.uint16), ref.view(np.uint16))
    assert ref.any()


def test_dm_volumes_hold_the_special_values_and_the_oracle_never_yields_minus_zero():
    h, w = 9, 17
    coords, names = R.dm_scene_coords(h, w)
    levels = R.dm_volumes(3, len(names), h, w)
    bits = levels[0].view(np.uint16)
    assert (bits == 0x8000).any() and ((bits & 0x7c00) == 0).any() and ((bits & 0x7fff) == 0x7bff).any()
    assert ((bits & 0x7c00 == 0) & (bits & 0x3ff != 0)).any()                     # subnormals
    ref = ocorr.corr_lookup_pyramid(levels, coords, 3)
    assert np.isfinite(ref.astype(np.float32)).all()
    assert not (ref.view(np.uint16) == 0x8000).any()
    assert np.array_equal(R.lookup_f64(levels, coords).view(np.uint16), ref.view(np.uint16))
    assert not ref[names.index("huge")].view(np.uint16).any()


@pytest.mark.parametrize("h,w", [(16, 24), (13, 22)])
def test_encoder_exact_scenes_pass_their_bound(h, w):
    levels, coords = R.dm_integer_scene(5, 3, h, w)
    corr = ocorr.corr_lookup_pyramid(levels, coords, 3)
    wgt, bias = R.integer_encoder(1, -4, 4)
    out, k, frac = R.encoder_reference(corr, wgt.reshape(128, 196), bias)
    assert k <= 10 and frac < 1.0 and np.abs(corr.astype(np.float32)).max() <= 4 and (out > 0).any()
    fm, coords = R.otf_integer_scene(7, 3, h, w)
    corr = R.otf_lookup(R.otf_volumes(fm, R.OTF_ENC_II, R.OTF_ENC_JJ), coords)
    wgt, bias = R.integer_encoder(2, -1, 1, density=0.5)
    out, k, frac = R.encoder_reference(corr, wgt.reshape(128, 196), bias)
    print("volume-free: lsb 2^-%d, max|corr| %g, bound %.3g * 2^24" % (k, np.abs(corr.astype(np.float32)).max(), frac))
    assert k <= 14 and frac < 1.0 and (out > 0).any()


def test_encoder_builder_rejects_dense_quarter_scene():
    """dense +-8 features with quarter coordinates: lsb 2^-16, far beyond the bound"""
    h, w = 16, 24
    fm = R.order_free_features(1, 3, h, w)
    rng = np.random.default_rng(0)
    coords = np.stack([rng.integers(0, 4 * w, (4, h, w)), rng.integers(0, 4 * h, (4, h, w))], 1).astype(np.float32) / 4
    corr = R.otf_lookup(R.otf_volumes(fm, R.OTF_II, R.OTF_JJ), coords)
    wgt, bias = R.integer_encoder(2, -1, 1)
    with pytest.raises(AssertionError, match="encoder-exact"):
        R.encoder_reference(corr, wgt.reshape(128, 196), bias)


@pytest.mark.parametrize("case", R.ALT_CASES, ids=lambda c: f"r{c[0]}-C{c[1]}-S{c[2]}-{c[3][0]}x{c[3][1]}-{c[4][0]}x{c[4][1]}-{c[5]}")
def test_altcorr_integer_scenes_are_exact(case):
    """the bound holds for every case the GPU test runs, and there the fp32 oracle equals the float64 loop nest exactly"""
    f1, f2, c = R.altcorr_case(case)
    assert R.altcorr_exact_bound(f1, f2, c) < 1.0
    ref = R.altcorr_f64(f1, f2, c, case[0])
    assert np.array_equal(ocorr.altcorr_forward(f1, f2, c, case[0]).astype(np.float64), ref)
    if case[5] == "huge":
        assert not ref.any()
    elif case[5] == "random":
        assert ref.any()


def test_altcorr_block_scene_is_exact():
    for S, integer in ((1, False), (3, False), (1, True)):
        fm, coords = R.altcorr_block_scene(11, 16, 24, S, integer)
        ref, inputs = R.altcorr_block_f64(fm.astype(np.float32), coords, R.OTF_II, R.OTF_JJ)
        for f1, f2, c in inputs:
            assert R.altcorr_exact_bound(f1, f2, c) < 1.0
        assert ref.shape == (4, 196, 16, 24, S) and ref.any()
        assert np.array_equal(ref.astype(np.float32).astype(np.float64), ref)
    # integer coordinates: the fp16 lookup of the volume-free path is the same number
    otf = R.otf_lookup(R.otf_volumes(fm, R.OTF_II, R.OTF_JJ), coords[:, :, :, 0].transpose(0, 3, 1, 2))
    assert np.array_equal(otf.astype(np.float64), ref[..., 0])
