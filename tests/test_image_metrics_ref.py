"""The float64 reference of the image metrics (tests/image_metrics_ref.py) pinned without a GPU: against an independent
torch float64 composition, on inputs with exact answers, and on the conditioning of the scenes the GPU tests use."""
import numpy as np
import pytest
import torch

import image_metrics_ref as R


# ---- (a) an independent formulation -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W,levels", [(161, 177, 5), (163, 161, 5), (23, 45, 2)])
def test_numpy_form_agrees_with_the_torch_float64_composition(H, W, levels):
    gt, render = R.scene(H, W, 0.1, seed=3)
    v, per = R.ms_ssim(gt, render, levels)
    tv, tper = R.torch_ms_ssim(gt, render, levels, torch.float64)
    assert per.shape == (levels, 2, 3)
    assert abs(v - tv) <= 1e-12
    assert np.abs(per - tper).max() <= 1e-12


# ---- (b), (c), (d) exact answers ---------------------------------------------------------------------------------------------
def test_identical_images_give_exactly_one():
    x = R.textured(161, 177, seed=1)
    v, per = R.ms_ssim(x, x)
    assert v == 1.0
    assert np.all(per[:, 1] == 1.0)


def test_negated_images_give_exactly_zero_through_the_relu():
    x = R.textured(161, 177, seed=1).astype(np.float64)
    v, per = R.ms_ssim(x, 1.0 - x)
    print("cs of the negated image per level:", per[:, 1].min(axis=1), per[:, 1].max(axis=1))
    assert np.all(per[:, 1] < 0.0), "every level's cs must be negative: the relu is exercised, not skipped"
    assert v == 0.0


@pytest.mark.parametrize("a,b", [(0.3, 0.7), (0.9, 0.05)])
def test_constant_images_give_the_closed_form(a, b):
    # even sizes down the pyramid: no zero padding, every level stays constant, cs = 1, ssim = the luminance term
    H, W = 176, 192
    x, y = np.full((H, W, 3), a), np.full((H, W, 3), b)
    v, per = R.ms_ssim(x, y)
    lum = (2 * a * b + R.C1) / (a * a + b * b + R.C1)
    assert np.abs(per[:, 1] - 1.0).max() <= 1e-12
    assert np.abs(per[:, 0] - lum).max() <= 1e-12
    assert abs(v - lum ** 0.1333) <= 1e-12


# ---- (e) the pooling -------------------------------------------------------------------------------------------------------
def test_pooling_of_an_odd_ramp_pads_one_zero_on_each_side_and_divides_by_four():
    H, W = 5, 7
    yy, xx = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    r = (10.0 * yy + xx + 1.0)[None]                     # r[y, x] = 10 y + x + 1
    p = R.avg_pool(r)
    assert p.shape == (1, 3, 4)
    # windows cover rows (-1,0), (1,2), (3,4) and columns (-1,0), (1,2), (3,4), (5,6)
    assert p[0, 0, 0] == 1.0 / 4.0                       # the corner: r[0,0] alone
    assert p[0, 0, 1] == (2.0 + 3.0) / 4.0               # top border: r[0,1] + r[0,2]
    assert p[0, 0, 3] == (6.0 + 7.0) / 4.0
    assert p[0, 1, 0] == (11.0 + 21.0) / 4.0             # left border: r[1,0] + r[2,0]
    assert p[0, 1, 1] == (12.0 + 13.0 + 22.0 + 23.0) / 4.0
    assert p[0, 2, 3] == (36.0 + 37.0 + 46.0 + 47.0) / 4.0
    sizes = [161]
    for _ in range(4):
        sizes.append(R.avg_pool(np.zeros((1, sizes[-1], 11))).shape[1])
    assert sizes == [161, 81, 41, 21, 11]
    # an even axis is not padded
    e = R.avg_pool(r[:, :4, :6])
    assert e.shape == (1, 2, 3) and e[0, 0, 0] == (1.0 + 2.0 + 11.0 + 12.0) / 4.0


# ---- PSNR, masked PSNR, depth L1 ------------------------------------------------------------------------------------------
def test_psnr_and_depth_l1():
    x = np.zeros((4, 5, 3))
    y = np.full((4, 5, 3), 0.1)
    assert abs(R.psnr(x, y) - 20.0) <= 1e-12
    mask = np.zeros((4, 5), dtype=bool)
    assert np.isnan(R.psnr(x, y, mask)) and np.isnan(R.depth_l1(x[..., 0], y[..., 0], mask))
    mask[1, 2] = True
    y[1, 2] = 0.01
    assert abs(R.psnr(x, y, mask) - 40.0) <= 1e-12
    assert abs(R.depth_l1(x[..., 0], y[..., 0], mask) - 0.01) <= 1e-15
    gt, render = R.scene(37, 53, 0.1, seed=5)
    m = R.half_mask(37, 53, seed=6)
    t = torch.nn.functional.mse_loss(torch.from_numpy(gt).double()[torch.from_numpy(m)],
                                     torch.from_numpy(render).double()[torch.from_numpy(m)])
    assert abs(R.psnr(gt, render, m) - float(-10.0 * torch.log10(t))) <= 1e-12


# ---- (f) the GPU scenes are well conditioned --------------------------------------------------------------------------------
@pytest.mark.parametrize("name,floor", [("161x177", 0.5), ("163x161", 0.1)])
def test_scenes_of_the_gpu_tests_are_well_conditioned(name, floor):
    H, W, sigma, seed = R.SCENES[name]
    gt, render = R.scene(H, W, sigma, seed)
    _, per = R.ms_ssim(gt, render)
    print(name, "minimum per-level per-channel mean:", per.min())
    assert per.min() >= floor >= 0.1


@pytest.mark.parametrize("H,W,levels", R.TILE_CASES)
def test_tile_scenes_of_the_gpu_tests_are_well_conditioned(H, W, levels):
    assert {w for _, w, _ in R.TILE_CASES} == {R.TILE_W + 9, R.TILE_W + 10, R.TILE_W + 11, 2 * R.TILE_W + 11}
    assert {h for h, _, _ in R.TILE_CASES} == {R.TILE_H + 9, R.TILE_H + 10, R.TILE_H + 11, 2 * R.TILE_H + 11}
    _, per = R.ms_ssim(*R.tile_scene(H, W), levels)
    assert per.min() >= 0.1


@pytest.mark.parametrize("H,W", [(37, 53), (161, 177)])
def test_half_masks_keep_between_5_and_95_percent(H, W):
    m = R.half_mask(H, W, seed=6)
    assert 0.05 <= m.mean() <= 0.95
