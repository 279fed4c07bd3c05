"""The image-metric kernels (csrc/metrics.hip through glorie_slam_amd/image_metrics.py) against the float64 reference of
tests/image_metrics_ref.py.

MS-SSIM tolerance: the kernel and the reference library round the same formula, whose moments cancel
(G*(X.X) - mu^2 against C2 = 9e-4).  The error of the torch float32 composition against float64 on the same inputs (on
the CPU) is the yardstick: the kernel's error of every per-level value and of the result must stay within 4 times it
(two float32 summation orders of one formula differ by a few-fold case by case), with a floor of 2e-6.  The ratios are
printed under -s.  The kernel accumulates its moments in fp64, so it sits far below the bound."""
import functools

import numpy as np
import pytest
import torch

import image_metrics_ref as R

pytestmark = pytest.mark.gpu

FACTOR, FLOOR = 4.0, 2e-6


@functools.lru_cache(maxsize=None)
def _case(H, W, levels, sigma, seed):
    """(gt, render, float64 value, per-level channel means [levels,2], float32-composition errors of both)"""
    gt, render = R.scene(H, W, sigma, seed)
    v, per = R.ms_ssim(gt, render, levels)
    v32, per32 = R.torch_ms_ssim(gt, render, levels, torch.float32)
    per, per32 = per.mean(axis=2), per32.mean(axis=2)
    for a in (gt, render, per):
        a.setflags(write=False)
    return gt, render, v, per, abs(v32 - v), np.abs(per32 - per)


def _check(got_v, got_levels, case, tag):
    _, _, v, per, e32_v, e32_per = case
    err_v = abs(float(got_v) - v)
    err_per = np.abs(got_levels.double().cpu().numpy() - per)
    bound_v, bound_per = max(FACTOR * e32_v, FLOOR), np.maximum(FACTOR * e32_per, FLOOR)
    print(f"{tag}: value error {err_v:.2e} (float32 composition {e32_v:.2e}, ratio to the bound {err_v / bound_v:.3f}); "
          f"per level: largest error {err_per.max():.2e}, float32 composition {e32_per.max():.2e}, "
          f"largest ratio to the bound {(err_per / bound_per).max():.3f}")
    assert err_v <= bound_v
    assert np.all(err_per <= bound_per), (err_per, bound_per)


def _dev(a, gpu, channels_first):
    t = torch.tensor(a).to(gpu)
    return t.permute(2, 0, 1).contiguous() if channels_first else t


# ---- per-level and final values ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("channels_first", [False, True])
@pytest.mark.parametrize("name", sorted(R.SCENES))
def test_five_levels_against_float64(gpu, name, channels_first):
    """161 x 177 is the smallest legal size: its last level is 11 x 12 with a 1 x 2 valid region"""
    from glorie_slam_amd.image_metrics import ms_ssim
    H, W, sigma, seed = R.SCENES[name]
    case = _case(H, W, 5, sigma, seed)
    v, levels = ms_ssim(_dev(case[0], gpu, channels_first), _dev(case[1], gpu, channels_first),
                        channels_first=channels_first, return_levels=True)
    assert v.shape == () and levels.shape == (5, 2) and v.dtype == torch.float32
    _check(v, levels, case, f"{name} {'CHW' if channels_first else 'HWC'}")


@pytest.mark.parametrize("channels_first", [False, True])
@pytest.mark.parametrize("H,W,levels", R.TILE_CASES)
def test_tile_edges_against_float64(gpu, H, W, levels, channels_first):
    """sizes around the 32 x 16 output tile: an empty last tile column or row, exactly one, a one-pixel ragged tile, two
    tiles and a ragged one"""
    from glorie_slam_amd.image_metrics import ms_ssim
    case = _case(H, W, levels, R.TILE_SIGMA, 20 + H + W)
    v, lv = ms_ssim(_dev(case[0], gpu, channels_first), _dev(case[1], gpu, channels_first),
                    channels_first=channels_first, levels=levels, return_levels=True)
    _check(v, lv, case, f"{H}x{W} levels={levels} {'CHW' if channels_first else 'HWC'}")


def test_non_contiguous_and_float64_inputs_are_copied(gpu):
    from glorie_slam_amd.image_metrics import ms_ssim
    gt, render = _case(161, 177, 5, *R.SCENES["161x177"][2:])[:2]
    x, y = _dev(gt, gpu, False), _dev(render, gpu, False)
    want = ms_ssim(x, y)
    xc = _dev(gt, gpu, True).permute(1, 2, 0)                  # [H,W,3] view of [3,H,W] storage
    assert not xc.is_contiguous()
    assert torch.equal(ms_ssim(xc, y.double()), want)
    wide = torch.zeros(161, 177, 6, device=gpu)
    wide[..., ::2] = y
    assert torch.equal(ms_ssim(x, wide[..., ::2]), want)


def test_sizes_and_shapes_are_rejected(gpu):
    from glorie_slam_amd import _lib
    from glorie_slam_amd.image_metrics import ms_ssim
    z = torch.zeros(160, 200, 3, device=gpu)
    with pytest.raises(ValueError):
        ms_ssim(z, z)
    with pytest.raises(ValueError):
        ms_ssim(z[:, :, :2], z[:, :, :2], levels=1)
    with pytest.raises(ValueError):
        ms_ssim(z, z[:100], levels=1)
    with pytest.raises(ValueError):
        ms_ssim(z, z, levels=6)
    with pytest.raises(_lib.GlorieError):
        ms_ssim(z.cpu(), z.cpu(), levels=1)
    lib = _lib.load()
    assert lib.glorie_ms_ssim_workspace(20, 200, 2) == 0       # the second level would be 10 high
    ws = _lib.workspace(lib.glorie_ms_ssim_workspace(21, 200, 2), gpu)
    out = torch.zeros(5, device=gpu)
    z = torch.zeros(21, 200, 3, device=gpu)
    assert lib.glorie_ms_ssim(_lib.ptr(z), _lib.ptr(z), 20, 200, 0, 2, _lib.ptr(ws), _lib.ptr(out),
                              _lib.stream_ptr(gpu)) == -1      # GLORIE_EINVAL


# ---- exact cases -----------------------------------------------------------------------------------------------------------
def test_identical_negated_and_constant_images(gpu):
    from glorie_slam_amd.image_metrics import ms_ssim
    x = torch.from_numpy(R.textured(161, 177, seed=1)).to(gpu)
    v, lv = ms_ssim(x, x.clone(), return_levels=True)
    assert abs(float(v) - 1.0) <= 1e-6 and float((lv - 1.0).abs().max()) <= 1e-6
    v, lv = ms_ssim(x, 1.0 - x, return_levels=True)
    assert float(v) == 0.0
    assert bool((lv[:, 1] < -0.5).all()), "every level's cs is negative: the relu is what gives 0"
    for a, b in ((0.3, 0.7), (0.9, 0.05)):
        H, W = 176, 192                                        # even at every level: no padding, the levels stay constant
        v, lv = ms_ssim(torch.full((H, W, 3), a, device=gpu), torch.full((H, W, 3), b, device=gpu), return_levels=True)
        fa, fb = float(np.float32(a)), float(np.float32(b))
        lum = (2 * fa * fb + R.C1) / (fa * fa + fb * fb + R.C1)
        assert abs(float(v) - lum ** 0.1333) <= 1e-6
        assert float((lv[:, 1] - 1.0).abs().max()) <= 1e-6 and float((lv[:, 0] - lum).abs().max()) <= 1e-6


# ---- the frame sums ----------------------------------------------------------------------------------------------------------
def _masks(H, W):
    one = np.zeros((H, W), dtype=bool)
    one[H // 3, W // 2] = True
    return {"empty": np.zeros((H, W), dtype=bool), "full": np.ones((H, W), dtype=bool), "one": one,
            "half": R.half_mask(H, W, seed=6)}


@functools.lru_cache(maxsize=None)
def _frame(H, W):
    gt, render = R.scene(H, W, 0.1, seed=5)
    rng = np.random.default_rng(7)
    depth = rng.uniform(0.5, 4.0, (H, W)).astype(np.float32)
    gt_depth = (depth + 0.1 * rng.standard_normal((H, W))).astype(np.float32)
    return gt, render, depth, gt_depth


@pytest.mark.parametrize("mask_name", ["empty", "full", "one", "half"])
@pytest.mark.parametrize("H,W", [(37, 53), (161, 177)])
def test_frame_sums_and_mask_apply(gpu, H, W, mask_name):
    from glorie_slam_amd.image_metrics import frame_metrics, mask_apply, psnr, _frame_reduce, _mask_u8
    gt, render, depth, gt_depth = _frame(H, W)
    mask = _masks(H, W)[mask_name]
    t = lambda a: torch.from_numpy(a).to(gpu)
    tg, tr, td, tgd, tm = t(gt), t(render), t(depth), t(gt_depth), t(mask)
    keep = [x.clone() for x in (tg, tr, td, tgd, tm)]
    sums, count = _frame_reduce(tg, tr, _mask_u8(tm, H, W), td, tgd)
    want = np.array([R.psnr(gt, render), R.psnr(gt, render, mask), R.depth_l1(depth, gt_depth, mask)])
    got = sums.double().cpu().numpy()
    with np.errstate(invalid="ignore"):
        print(f"{H}x{W} {mask_name}: relative errors {np.abs(got - want) / np.abs(want)}")
    assert int(count) == int(mask.sum())
    if mask_name == "empty":
        assert np.isnan(got[1]) and np.isnan(got[2]) and np.isnan(want[1])
        np.testing.assert_allclose(got[0], want[0], rtol=1e-6, atol=0)
    else:
        np.testing.assert_allclose(got, want, rtol=1e-6, atol=0)
    # the public forms agree with it bit for bit
    assert torch.equal(psnr(tg, tr), sums[0])
    assert torch.equal(psnr(tg, tr, tm).view(torch.int32), sums[1].view(torch.int32))
    # mask-apply is the torch indexing form
    m_depth, m_color, m_gt = mask_apply(tm, td, tr, tg)
    for got_map, src in ((m_depth, td), (m_color, tr), (m_gt, tg)):
        ref = src.clone()
        ref[~tm] = 0.0
        assert torch.equal(got_map, ref)
    if H >= 161:
        fm = frame_metrics(tr, td.double(), tg, tm, gt_depth=tgd)
        assert torch.equal(fm["depth"], m_depth) and torch.equal(fm["color"], m_color) and torch.equal(fm["gt_color"], m_gt)
        for k, s in (("psnr", sums[0]), ("masked_psnr", sums[1]), ("depth_l1", sums[2])):
            assert torch.equal(fm[k].view(torch.int32), s.view(torch.int32))
        assert "depth_l1" not in frame_metrics(tr, td, tg, tm)
        for key, a, b in (("ms_ssim", gt, render), ("masked_ms_ssim", gt * mask[..., None], render * mask[..., None])):
            v = R.ms_ssim(a, b)[0]
            bound = max(FLOOR, FACTOR * abs(R.torch_ms_ssim(a, b, 5, torch.float32)[0] - v))
            print(f"{key}: error {abs(float(fm[key]) - v):.2e}, bound {bound:.2e}")
            assert abs(float(fm[key]) - v) <= bound
    # nothing was written into the inputs
    for a, b in zip((tg, tr, td, tgd, tm), keep):
        assert torch.equal(a, b)


# ---- determinism and graphs ---------------------------------------------------------------------------------------------------
def test_repeated_calls_are_bitwise_equal_and_record_into_a_graph(gpu):
    from glorie_slam_amd.image_metrics import frame_metrics, ms_ssim
    H, W = 161, 177
    t = lambda a: torch.from_numpy(a).to(gpu)
    gt, render, depth, gt_depth = (t(a) for a in _frame(H, W))
    mask = t(R.half_mask(H, W, seed=6))
    keys = ("psnr", "ms_ssim", "masked_psnr", "masked_ms_ssim", "depth_l1", "depth", "color", "gt_color")

    def run(a, b, d, gd, m):
        fm = frame_metrics(b, d, a, m, gt_depth=gd)
        v, lv = ms_ssim(a, b, return_levels=True)
        return [fm[k] for k in keys] + [v, lv]

    first = [o.clone() for o in run(gt, render, depth, gt_depth, mask)]
    for _ in range(3):
        again = run(gt, render, depth, gt_depth, mask)
        assert all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(first, again))
    # recorded on one set of inputs, replayed on another of the same shape
    static = [x.clone() for x in (gt, render, depth, gt_depth, mask)]
    side = torch.cuda.Stream(gpu)
    side.wait_stream(torch.cuda.current_stream(gpu))
    with torch.cuda.stream(side):
        run(*static)
    torch.cuda.current_stream(gpu).wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        recorded = run(*static)
    gt2, render2, depth2, gt_depth2 = (t(a) for a in (R.scene(H, W, 0.15, seed=31) + _frame(H, W)[2:][::-1]))
    mask2 = t(R.half_mask(H, W, seed=32))
    for s, new in zip(static, (gt2, render2, depth2, gt_depth2, mask2)):
        s.copy_(new)
    graph.replay()
    torch.cuda.synchronize()
    eager = run(gt2, render2, depth2, gt_depth2, mask2)
    assert all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(recorded, eager))
    assert not torch.equal(eager[1], first[1])
