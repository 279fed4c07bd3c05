"""The float64 restatement of LPIPS in tests/lpips_ref.py (numpy: im2col convolutions, explicit pooling loops) pinned
against the torch composition of the same formula (F.conv2d, F.max_pool2d) in float64, and the properties the GPU tests
rely on.  No GPU."""
import numpy as np
import pytest
import torch

import lpips_ref as R

PIN_SIZES = [(31, 31), (35, 47), (63, 95)]


@pytest.mark.parametrize("H,W", PIN_SIZES)
def test_numpy_float64_agrees_with_torch_float64(H, W):
    x, y = R.scene(H, W, seed=H + W)
    wts = R.weights()
    v, per, maps = R.lpips(x, y, wts)
    tv, tper, tmaps = R.torch_lpips(x, y, wts, torch.float64)
    assert [m.shape for m in maps] == [(2, h, w, c[1]) for (h, w), c in zip(R.shapes(H, W), R.LAYERS)]
    for l, (a, b) in enumerate(zip(maps, tmaps)):
        assert a.shape == b.shape
        assert np.abs(a - b).max() <= 1e-12 * np.abs(a).max(), l
    np.testing.assert_allclose(per, tper, rtol=1e-12, atol=0)
    np.testing.assert_allclose(v, tv, rtol=1e-12, atol=0)


def test_seeded_scenes_weigh_every_layer():
    """the value is 0.15 - 0.17 with shares near 0.085 / 0.03 / 0.015 / 0.013 / 0.012: no layer is negligible in the total,
    and y leaves [0,1], so the clamp works"""
    x, y = R.scene(63, 95, seed=1)
    assert y.min() < 0.0 and y.max() > 1.0 and x.min() >= 0.0 and x.max() <= 1.0
    v, per, _ = R.lpips(x, y, R.weights())
    print(v, per)
    assert 0.15 <= v <= 0.17
    for got, want in zip(per, (0.085, 0.03, 0.015, 0.013, 0.012)):
        assert 0.6 * want <= got <= 1.5 * want


def test_identical_images_give_zero_and_the_value_is_symmetric():
    x, y = R.scene(35, 47, seed=2)
    wts = R.weights()
    v, per, _ = R.lpips(x, x.copy(), wts)
    assert v == 0.0 and np.all(per == 0.0)
    a, b = R.lpips(x, y, wts), R.lpips(y, x, wts)
    assert a[0] == b[0] and np.array_equal(a[1], b[1])


def test_inputs_outside_the_unit_range_equal_their_clamped_forms():
    x, y = R.scene(35, 47, seed=3)
    wts = R.weights()
    wild = 3.0 * x - 1.0
    assert wild.min() < 0.0 and wild.max() > 1.0
    a, b = R.lpips(wild, y, wts), R.lpips(np.clip(wild, 0.0, 1.0), np.clip(y, 0.0, 1.0), wts)
    assert a[0] == b[0] and np.array_equal(a[1], b[1])


def test_the_padding_is_zero_in_the_scaled_domain():
    """a constant image whose scaled value is not 0: with zero padding in the scaled domain conv1's border outputs see
    fewer taps than the interior and differ from it; padding with the raw value 0 (scaled: not 0) or replicating the
    constant would change them"""
    wts = R.weights()
    img = np.full((47, 47, 3), 0.8, dtype=np.float32)
    scaled = R.scale_image(img)
    assert np.all(np.abs(scaled) > 0.5)
    w, b = wts["conv"][0]
    out = R.conv2d(scaled, w, b, 4, 2)                                        # [64, 11, 11]
    interior = out[:, 1:-1, 1:-1]
    assert np.abs(interior - interior[:, :1, :1]).max() <= 1e-12              # constant away from the border
    assert np.abs(out[:, 0, :] - interior[:, :1, 0]).max() > 1e-2             # the top row is not
    # the expected border value from first principles: only taps with 2 <= ky are inside for output row 0
    full = np.asarray(w, dtype=np.float64) * scaled[:, :1, :1][None]
    want = full[:, :, 2:, :].sum(axis=(1, 2, 3)) + b
    np.testing.assert_allclose(out[:, 0, 5], want, rtol=1e-12, atol=1e-12)
    # and the torch composition pads the same way
    t = R.torch_lpips(img, img, wts, torch.float64)[2][0][0]                  # [11, 11, 64]
    np.testing.assert_allclose(t, np.maximum(out, 0.0).transpose(1, 2, 0), rtol=1e-12, atol=1e-12)


def test_a_one_hot_lin_returns_that_channel_term():
    x, y = R.scene(35, 47, seed=4)
    wts = R.weights()
    fx, fy = R.features(x, wts), R.features(y, wts)
    for l, ch in ((0, 5), (2, 300), (4, 255)):
        lin = np.zeros(R.LAYERS[l][1], dtype=np.float32)
        lin[ch] = 1.0
        nx = fx[l] / np.sqrt(R.NORM_EPS + (fx[l] ** 2).sum(axis=2, keepdims=True))
        ny = fy[l] / np.sqrt(R.NORM_EPS + (fy[l] ** 2).sum(axis=2, keepdims=True))
        want = float(((nx[..., ch] - ny[..., ch]) ** 2).mean())
        assert R.layer_value(fx[l], fy[l], lin) == want
        hot = {"conv": wts["conv"], "lin": [lin if i == l else np.zeros_like(w) for i, w in enumerate(wts["lin"])]}
        v, per, _ = R.lpips(x, y, hot)
        assert v == want and per[l] == want and per.sum() == want


def test_the_shape_chain_and_its_floor_drops():
    assert R.shapes(31, 31) == [(7, 7), (3, 3), (1, 1), (1, 1), (1, 1)]
    assert R.shapes(480, 640) == [(119, 159), (59, 79), (29, 39), (29, 39), (29, 39)]
    assert R.shapes(680, 1200) == [(169, 299), (84, 149), (41, 74), (41, 74), (41, 74)]
    # (H - 7) % 4 != 0: conv1 drops the last 1 - 3 rows
    assert [R.shapes(H, 31)[0][0] for H in (31, 32, 33, 34, 35)] == [7, 7, 7, 7, 8]
    # an even pool input drops its last row: first tap 8 -> pooled 3, as 7 does; 9 -> 4
    assert [R.shapes(H, 31)[1][0] for H in (31, 35, 39)] == [3, 3, 4]
    assert R.shapes(52, 31)[0] == (12, 7) and R.shapes(52, 31)[1] == (5, 3) and R.shapes(52, 31)[2] == (2, 1)
    # against the maps themselves
    x, _ = R.scene(52, 31, seed=5)
    assert [m.shape[:2] for m in R.features(x, R.weights())] == R.shapes(52, 31)
    # the tile cases are what they say
    assert [R.shapes(H, W)[0] for H, W in R.TILE_CASES[:5]] == R.CONV1_TAPS
    assert [R.shapes(H, W)[4] for H, W in R.TILE_CASES[5:]] == R.LATE_TAPS
    assert [h * w for h, w in R.CONV1_TAPS] == [R.PIXEL_TILE - 1, R.PIXEL_TILE, 6 * R.PIXEL_TILE + 1, 2 * R.PIXEL_TILE,
                                                2 * R.PIXEL_TILE + 5]
    assert [h * w for h, w in R.LATE_TAPS] == [R.LATE_TILE - 1, R.LATE_TILE, R.LATE_TILE + 1, 2 * R.LATE_TILE,
                                               2 * R.LATE_TILE + 1]


def test_the_tile_constants_are_the_kernels():
    import os
    import re
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "glorie_slam_amd", "csrc",
                            "lpips.hip")).read()
    for name, want in (("kBM", R.PIXEL_TILE), ("kBMLate", R.LATE_TILE), ("kBN", R.CHANNEL_TILE), ("kBK", R.K_CHUNK)):
        assert int(re.search(rf"constexpr int {name} = (\d+);", src).group(1)) == want
    from glorie_slam_amd import lpips as P
    assert (P.SHIFT, P.SCALE, P.NORM_EPS, P.LAYERS, P.MIN_SIDE) == (R.SHIFT, R.SCALE, R.NORM_EPS, R.LAYERS, R.MIN_SIDE)
    assert float(re.search(r"constexpr double kNormEps = ([0-9.e-]+);", src).group(1)) == R.NORM_EPS
