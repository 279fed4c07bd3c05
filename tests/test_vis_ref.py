"""tests/vis_ref.py, the float32 restatement the contact-sheet kernels are held to, against matplotlib itself (what the
reference draws its figure with, src/utils/Visualizer.py:130-203) where matplotlib is installed, and against values
worked out by hand where it is not needed.  No GPU."""
import numpy as np
import pytest

import vis_ref as R
from glorie_slam_amd.visualizer import PLASMA, TITLES
from glorie_slam_amd.visualizer import panel_boxes as product_boxes

F = np.float32
H, W = 37, 53


def _depth(rng, holes=True):
    d = (rng.random((H, W)) * rng.uniform(0.5, 9.0) + rng.uniform(0.0, 2.0)).astype(F)
    if holes:
        d[rng.random((H, W)) < 0.1] = 0
    return d


# ---- against matplotlib ---------------------------------------------------------------------------------------------
def test_table_is_matplotlibs():
    matplotlib = pytest.importorskip("matplotlib")
    colors = np.asarray(matplotlib.colormaps["plasma"].colors)
    assert PLASMA.shape == (256, 3) and PLASMA.dtype == np.uint8
    assert np.array_equal(PLASMA, (colors * 255).astype(np.uint8))


def _mpl(x, vmin=None, vmax=None):
    import matplotlib
    from matplotlib.colors import Normalize
    norm = Normalize(vmin, vmax)
    norm.autoscale_None(x)                                    # imshow without vmin / vmax: the data's own range
    return matplotlib.colormaps["plasma"](norm(x), bytes=True)[..., :3]


def test_scalar_panels_are_matplotlibs_bytes():
    pytest.importorskip("matplotlib")
    rng = np.random.default_rng(0)
    differing = 0
    for _ in range(40):
        x, other = _depth(rng), _depth(rng, holes=False)
        dmax = x.max()
        differing += int((R.colormap(x, 0, dmax, PLASMA) != _mpl(x, 0, dmax)).sum())                 # [0, max]
        differing += int((R.colormap(other, 0, dmax, PLASMA) != _mpl(other, 0, dmax)).sum())         # values above vmax
        res = R.depth_residual(x, other * F(0.05) + x)
        differing += int((R.colormap(res, res.min(), res.max(), PLASMA) != _mpl(res)).sum())         # its own [min, max]
        mask = (x > 0).astype(np.int32)
        differing += int((R.colormap(mask, 0, 1, PLASMA) != _mpl(mask, 0, 1)).sum())                 # fixed, integers
    counts = rng.integers(0, 11, (H, W))
    differing += int((R.colormap(counts, 0, 10, PLASMA) != _mpl(counts.astype(np.float64), 0, 10)).sum())
    differing += int((R.colormap(counts, 0, 10, PLASMA) != _mpl(counts, 0, 10)).sum())
    assert differing == 0


def test_rgb_panels_are_matplotlibs_bytes():
    matplotlib = pytest.importorskip("matplotlib")
    matplotlib.use("Agg")
    import matplotlib.pyplot as plt
    rng = np.random.default_rng(1)
    fig, ax = plt.subplots()
    try:
        for _ in range(5):
            x = (rng.random((H, W, 3)) * 1.4 - 0.2).astype(F)
            x[0, :8, 0] = (np.arange(8, dtype=F) + 100) / F(255)                      # levels themselves
            im = ax.imshow(np.clip(x, 0, 1))
            drawn = np.asarray(im.make_image(None, unsampled=True)[0])[..., :3]
            assert np.array_equal(R.level(x), drawn)
            im.remove()
    finally:
        plt.close(fig)


# ---- by hand --------------------------------------------------------------------------------------------------------
def test_layout_at_ragged_sizes():
    for (h, w, scale, gutter, title) in [(37, 53, 1, 4, 12), (37, 53, 2, 4, 12), (37, 53, 3, 0, 0), (37, 53, 5, 1, 7),
                                         (1, 1, 1, 4, 12), (2, 130, 4, 3, 2), (480, 640, 2, 4, 12)]:
        ph, pw = -(-h // scale), -(-w // scale)
        boxes = R.panel_boxes(h, w, scale, gutter, title)
        assert boxes == product_boxes(h, w, scale, gutter, title) and len(boxes) == 12 == len(TITLES)
        SH, SW = R.sheet_size(h, w, scale, gutter, title)
        assert boxes[0] == (gutter + title, gutter, ph, pw)
        y0, x0, _, _ = boxes[11]
        assert (y0 + ph + gutter, x0 + pw + gutter) == (SH, SW)                  # the border closes the sheet
        cover = np.zeros((SH, SW), np.int32)
        for y0, x0, bh, bw in boxes:
            cover[y0:y0 + bh, x0:x0 + bw] += 1
            assert y0 - title >= gutter and not cover[y0 - title:y0, x0:x0 + bw].any()   # its title strip is free
        assert cover.max() == 1 and cover.sum() == 12 * ph * pw
    assert R.sheet_size(480, 640, 2, 4, 12) == (4 + 4 * (12 + 240 + 4), 4 + 3 * (320 + 4))
    # decimation: the centre of each scale x scale block, clamped to the last row / column
    src = np.arange(7 * 11).reshape(7, 11)
    assert np.array_equal(R.decimate(src, 3), src[[1, 4, 6]][:, [1, 4, 7, 10]])
    assert np.array_equal(R.decimate(src, 1), src)
    assert np.array_equal(R.decimate(src, 5), src[[2, 6]][:, [2, 7, 10]])
    assert np.array_equal(R.decimate(src[:1, :1], 4), src[:1, :1])


def test_colormap_edges():
    v = np.array([0.0, 1.0, 3.0, -2.0, np.nan, np.inf, -np.inf], F)
    flat = R.colormap(v, 2.0, 2.0, PLASMA)                                       # vmin == vmax: t = 0
    assert np.array_equal(flat[:4], np.repeat(PLASMA[:1], 4, 0)) and (flat[4:] == 255).all()
    out = R.colormap(np.array([-1.0, 0.0, 0.5, 1.0, 1.5, 1e30, np.nan], F), 0.0, 1.0, PLASMA)
    assert np.array_equal(out[:6], PLASMA[[0, 0, 128, 255, 255, 255]]) and (out[6] == 255).all()
    # 256 t exactly on the integers: entry k for v = k dmax / 256, the last entry for v = dmax
    k = np.arange(257, dtype=F)
    assert np.array_equal(R.colormap(k * F(4.0 / 256), 0.0, 4.0, PLASMA), PLASMA[np.minimum(np.arange(257), 255)])
    # ranges: non-finite values are skipped, nothing gives [0, 0], the residual is clipped at 0.2 and 0 in the holes
    maps = dict(droid_depth=np.array([[np.nan, 2.0, np.inf, -1.0]], F), render_depth=np.array([[1.0, 0.0, 2.0, 3.0]], F),
                depth=np.array([[1.05, 9.0, np.nan, 7.0]], F))
    r = R.ranges(maps)
    assert r.dtype == F and r.tolist() == [2.0, 0.0, float(F(0.2)), 0.0]
    assert np.array_equal(R.depth_residual(maps["render_depth"], maps["depth"])[0, [1, 3]], np.array([0.0, 0.2], F))
    assert np.isnan(R.depth_residual(maps["render_depth"], maps["depth"])[0, 2])
    nothing = dict(droid_depth=np.full((2, 2), np.nan, F), render_depth=np.full((2, 2), np.nan, F), depth=np.ones((2, 2), F))
    assert R.ranges(nothing).tolist() == [0.0, 0.0, 0.0, 0.0]
    assert not np.signbit(R.ranges(dict(droid_depth=-np.zeros((1, 1), F), render_depth=np.zeros((1, 1), F),
                                        depth=np.ones((1, 1), F)))).any()


def test_rendered_rgb_truncates_a_rounded_value():
    """panel 4 is trunc(255 c) of c = rint(255 color) / 255: a level k whose float32(k / 255) * 255 falls below k would
    come out as k - 1"""
    k = np.arange(256, dtype=F)
    back = (k / F(255)) * F(255)
    below = np.flatnonzero(back < k)
    if below.size:
        j = int(below[0])
        assert R.level(R.round_level(np.array([j / 255.0], F)))[0] == j - 1
    else:
        # no such level exists in float32: the quirk never shows, and panel 4 is the rounded level itself
        assert np.array_equal(R.level(R.round_level(k / F(255))), np.arange(256, dtype=np.uint8))
    # the rounding itself: half an ulp above k / 255 still rounds to k, ties go to the even level
    x = np.nextafter(k / F(255), F(2))
    assert np.array_equal(R.level(R.round_level(x)), np.arange(256, dtype=np.uint8))
    assert R.level(np.array([np.nan, -0.5, 1.5, 1.0, 0.999], F)).tolist() == [0, 0, 255, 255, 254]
    assert R.to_rgb8(np.array([np.nan, -1.0, 2.0, np.inf, -np.inf, 0.5 / 255, 1.5 / 255, 0.999], F)).tolist()[:5] == \
        [0, 0, 255, 255, 0]
    # ties of to_rgb8 go to the even level wherever 255 x is an exact tie
    ties = ((k[:255] + F(0.5)) / F(255)).astype(F)
    exact = (ties * F(255)) == k[:255] + F(0.5)
    got = R.to_rgb8(ties)
    even = (k[:255] + (k[:255] % 2)).astype(np.uint8)
    assert exact.any() and np.array_equal(got[exact], even[exact])
