"""The numpy restatement of the frame ingest (tests/ingest_ref.py) pinned by properties, and the host tables of
glorie_slam_amd.ingest.IngestPlan against it.  No GPU: the plan is built on the CPU, where only its tables and
intrinsic() are usable."""
from fractions import Fraction

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import ingest_ref as R

TUM_FR1 = [0.2624, -0.9531, -0.0054, 0.0026, 1.1633]
SHAPES = [((37, 53), (28, 46)), ((20, 28), (33, 47)), ((24, 40), (24, 40)), ((48, 64), (24, 32)),
          ((680, 1200), (320, 640)), ((480, 640), (400, 528))]


def _img(shape, seed=0, channels=3):
    return np.random.default_rng(seed).integers(0, 256, (*shape, channels), dtype=np.uint8)


def test_equal_size_is_the_identity():
    img = _img((24, 40), 1)
    assert np.array_equal(R.resize(img, 24, 40), img)
    got = R.color(img, R.cam_block(24, 40, 24, 40))
    assert np.array_equal(got[0], (img.astype(np.float32) / np.float32(255)).transpose(2, 0, 1))


def test_exact_halving_is_the_rounded_block_mean():
    img = _img((48, 64), 2).astype(np.int64)
    want = (img[0::2, 0::2] + img[0::2, 1::2] + img[1::2, 0::2] + img[1::2, 1::2] + 2) >> 2
    assert np.array_equal(R.resize(img.astype(np.uint8), 24, 32), want)


@pytest.mark.parametrize("src,dst", SHAPES)
def test_resize_within_one_level_of_float64(src, dst):
    img = _img(src, 3)
    err = np.abs(R.resize(img, *dst).astype(np.float64) - R.resize_float64(img, *dst)).max()
    print(f"{src} -> {dst}: largest deviation {err:.3f} level")
    assert err < 1.0


def test_undistort_is_the_rounded_exact_bilinear_value():
    """floor(v + 1/2) of the exact bilinear value v at the 1/32-quantised position, in rational arithmetic"""
    H, W = 13, 17
    img = _img((H, W), 4)
    ix, iy = R.remap_positions(H, W, 15.0, 14.0, 8.3, 6.1, TUM_FR1)
    got = R.undistort(img, ix, iy)
    px = lambda x, y, c: int(img[y, x, c]) if 0 <= x < W and 0 <= y < H else 0
    outside = 0
    for v in range(H):
        for u in range(W):
            x0, y0 = int(ix[v, u]) // 32, int(iy[v, u]) // 32            # floor division
            a, b = Fraction(int(ix[v, u]) - 32 * x0, 32), Fraction(int(iy[v, u]) - 32 * y0, 32)
            outside += not (0 <= x0 and x0 + 1 < W and 0 <= y0 and y0 + 1 < H)
            for c in range(3):
                val = ((1 - a) * (1 - b) * px(x0, y0, c) + a * (1 - b) * px(x0 + 1, y0, c)
                       + (1 - a) * b * px(x0, y0 + 1, c) + a * b * px(x0 + 1, y0 + 1, c))
                assert int(got[v, u, c]) == (val + Fraction(1, 2)).__floor__(), (u, v, c)
    assert outside > 0                                                    # some taps did fall outside the image


def test_zero_distortion_is_the_identity_table():
    from glorie_slam_amd import ingest
    H, W = 37, 53
    for zeros in ([0.0] * 4, [0.0] * 5, [0.0] * 8):
        ix, iy = R.remap_positions(H, W, 45.0, 44.0, 25.7, 18.2, zeros)
        v, u = np.mgrid[0:H, 0:W]
        assert np.array_equal(ix, 32 * u) and np.array_equal(iy, 32 * v)
        tab = ingest.undistort_table(H, W, 45.0, 44.0, 25.7, 18.2, zeros)
        assert np.array_equal(tab[..., 0], 32 * u) and np.array_equal(tab[..., 1], 32 * v)
    img = _img((H, W), 5)
    assert np.array_equal(R.undistort(img, ix, iy), img)


@pytest.mark.parametrize("dist", [TUM_FR1, TUM_FR1[:4], TUM_FR1 + [0.05, -0.02, 0.01]])
def test_package_undistort_table_equals_the_restatement(dist):
    from glorie_slam_amd import ingest
    H, W = 37, 53
    ix, iy = R.remap_positions(H, W, 45.0, 44.0, 25.7, 18.2, dist)
    tab = ingest.undistort_table(H, W, 45.0, 44.0, 25.7, 18.2, dist)
    assert tab.dtype == np.int32 and np.array_equal(tab[..., 0], ix) and np.array_equal(tab[..., 1], iy)
    assert np.abs(ix - 32 * np.mgrid[0:H, 0:W][1]).max() > 32 * 0.5          # the map does move pixels
    assert (ix < 0).any() or (iy < 0).any() or (ix >> 5).max() >= W - 1 or (iy >> 5).max() >= H - 1


def test_distortion_length_is_checked():
    from glorie_slam_amd import ingest
    for n in (3, 6, 14):
        with pytest.raises(ValueError):
            ingest.undistort_table(8, 8, 5.0, 5.0, 4.0, 4.0, [0.0] * n)
    with pytest.raises(ValueError):
        ingest.IngestPlan(R.cam_block(8, 8, 8, 8, distortion=[0.0] * 14), "cpu")
    with pytest.raises(ValueError):
        ingest.IngestPlan({"H": 8, "W": 8}, "cpu")


@pytest.mark.parametrize("src,dst", SHAPES)
def test_package_resize_and_nearest_tables_equal_the_restatement(src, dst):
    from glorie_slam_amd import ingest
    for n_src, n_dst in zip(src, dst):
        s, _, a0, a1 = R.resize_coords(n_src, n_dst)
        tab = ingest.resize_table(n_src, n_dst)
        assert np.array_equal(tab[:, 0], s) and np.array_equal(tab[:, 1], np.minimum(s + 1, n_src - 1))
        assert np.array_equal(tab[:, 2], a0) and np.array_equal(tab[:, 3], a1)
        assert np.array_equal(a0 + a1, np.full(n_dst, 2048))
        assert np.array_equal(ingest.nearest_table(n_src, n_dst), R.nearest_index(n_src, n_dst))


@pytest.mark.parametrize("n_src,n_dst", [(37, 28), (20, 33), (680, 320), (480, 400), (53, 46)])
def test_nearest_index_is_torch_nearest(n_src, n_dst):
    ramp = torch.arange(n_src, dtype=torch.float32)
    want = F.interpolate(ramp[None, None, None], (1, n_dst), mode="nearest")[0, 0, 0].numpy().astype(np.int64)
    assert np.array_equal(R.nearest_index(n_src, n_dst), want)


@pytest.mark.parametrize("dtype", [np.uint16, np.float32])
def test_depth_is_torch_nearest_then_crop_then_scale(dtype):
    rng = np.random.default_rng(6)
    raw = rng.integers(0, 65536, (2, 37, 53)).astype(dtype)
    cam = R.cam_block(37, 53, 24, 40, H_edge=2, W_edge=3, png_depth_scale=5000.0)
    full = torch.from_numpy(raw.astype(np.float32) / np.float32(5000.0))       # datasets.py:56, then :117-130
    want = F.interpolate(full[:, None], (28, 46), mode="nearest")[:, 0][:, 2:-2, 3:-3]
    assert np.array_equal(R.depth(raw, cam), want.numpy())


def test_depth_division_all_uint16_values():
    v = np.arange(65536, dtype=np.uint16).reshape(1, 256, 256)
    cam = R.cam_block(256, 256, 256, 256, png_depth_scale=6553.5)
    want = (torch.from_numpy(v.astype(np.int32)).float() / torch.tensor(6553.5, dtype=torch.float32)).numpy()
    assert np.array_equal(R.depth(v, cam), want)
    exact = np.arange(65536, dtype=np.float64) / np.float64(np.float32(6553.5))
    assert np.array_equal(R.depth(v, cam).reshape(-1), exact.astype(np.float32))    # correctly rounded


CAMS = [R.cam_block(480, 640, 384, 512, 8, 8, fx=517.3, fy=516.5, cx=318.6, cy=255.3, distortion=TUM_FR1),
        R.cam_block(480, 640, 240, 320, 8, 16, fx=577.590698, fy=578.729797, cx=318.905426, cy=242.683609),
        R.cam_block(680, 1200, 320, 640, 0, 0, fx=600.0, fy=600.0, cx=599.5, cy=339.5),
        R.cam_block(37, 53, 24, 40, 2, 0), R.cam_block(37, 53, 24, 40, 0, 3)]


@pytest.mark.parametrize("cam", CAMS)
def test_intrinsic_is_the_reference_expression_in_float32(cam):
    from glorie_slam_amd.ingest import IngestPlan
    # src/utils/datasets.py:85-96, line by line
    H_res, W_res = cam["H_out"] + cam["H_edge"] * 2, cam["W_out"] + cam["W_edge"] * 2
    want = torch.as_tensor([cam["fx"], cam["fy"], cam["cx"], cam["cy"]]).float()
    want[0] *= W_res / cam["W"]
    want[1] *= H_res / cam["H"]
    want[2] *= W_res / cam["W"]
    want[3] *= H_res / cam["H"]
    if cam["W_edge"] > 0:
        want[2] -= cam["W_edge"]
    if cam["H_edge"] > 0:
        want[3] -= cam["H_edge"]
    got = IngestPlan(cam, "cpu").intrinsic()
    assert got.dtype == torch.float32 and got.shape == (4,) and torch.equal(got, want)
    assert np.array_equal(R.intrinsic(cam), want.numpy())


def test_plan_tables_are_the_cropped_restatement_tables():
    from glorie_slam_amd.ingest import IngestPlan
    cam = R.cam_block(37, 53, 24, 40, H_edge=2, W_edge=3, distortion=TUM_FR1, png_depth_scale=5000.0)
    plan = IngestPlan(cam, "cpu")
    s, _, a0, a1 = R.resize_coords(53, 46)
    assert plan.xtab.shape == (40, 4) and np.array_equal(plan.xtab[:, 0].numpy(), s[3:-3])
    assert np.array_equal(plan.xtab[:, 2].numpy(), a0[3:-3]) and np.array_equal(plan.xtab[:, 3].numpy(), a1[3:-3])
    s, _, b0, b1 = R.resize_coords(37, 28)
    assert plan.ytab.shape == (24, 4) and np.array_equal(plan.ytab[:, 0].numpy(), s[2:-2])
    assert np.array_equal(plan.ysrc.numpy(), R.nearest_index(37, 28)[2:-2])
    assert np.array_equal(plan.xsrc.numpy(), R.nearest_index(53, 46)[3:-3])
    assert plan.map.shape == (37, 53, 2) and plan.map.dtype == torch.int32
    lut = plan.lut.numpy()
    assert np.array_equal(lut, (np.arange(256) / 255.0).astype(np.float32)) and lut[255] == 1.0   # correctly rounded
    assert IngestPlan(R.cam_block(37, 53, 24, 40), "cpu").map is None


def test_cpu_tensors_are_rejected():
    from glorie_slam_amd import _lib
    from glorie_slam_amd.ingest import IngestPlan
    plan = IngestPlan(R.cam_block(8, 8, 8, 8), "cpu")
    with pytest.raises(_lib.GlorieError):
        plan.color(torch.zeros(8, 8, 3, dtype=torch.uint8))
    with pytest.raises(_lib.GlorieError):
        plan.depth(torch.zeros(8, 8, dtype=torch.float32))
