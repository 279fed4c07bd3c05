"""LPIPS in the re-render evaluation (eval_render.eval_kf_imgs / eval_imgs with lpips = an lpips.Lpips) on the small
synthetic runner of tests/test_gpu_eval_render.py: the added per-frame values recomputed from the kept renders, the
reference's eight-line metrics files, and - without lpips - today's keys and file text."""
import os

import numpy as np
import pytest
import torch

import lpips_ref as R

pytestmark = pytest.mark.gpu

H, W = 168, 224
BASE = ("psnr", "ms_ssim", "masked_psnr", "masked_ms_ssim")
RESULT_KEYS = {"frames", "frame_cnt", "avg_depth_l1"} | {f"avg_{k}" for k in BASE}


@pytest.fixture(scope="module")
def ran(gpu):
    from glorie_slam_amd.lpips import Lpips
    from glorie_slam_amd.pipeline import synthetic_images, synthetic_runner
    K = 10
    run, c = synthetic_runner(gpu, K, zero_flow_head=True, map_iters=4, map_rays=600, H=H, W=W)
    imgs = synthetic_images(K, H, W)
    run.run(((k, imgs[k:k + 1]) for k in range(K)), c["intrinsics"], final_ba_steps=2)
    assert run.mapped > 3
    wts = R.weights()
    metric = Lpips([(torch.tensor(np.array(w)), torch.tensor(np.array(b))) for w, b in wts["conv"]],
                   [torch.tensor(np.array(l)) for l in wts["lin"]], device=gpu)
    return run, imgs, metric


def _today(res, label):
    """the metrics file as it is written without lpips"""
    return (f"avg_masked_{label}: {res['avg_masked_ms_ssim']}\navg_masked_psnr: {res['avg_masked_psnr']}\n"
            f"###############\navg_{label}: {res['avg_ms_ssim']}\navg_psnr: {res['avg_psnr']}\n###############\n")


def _check(res, plain, out_dir, plain_dir, log_name, label, metric, gt_of):
    n = res["frame_cnt"]
    assert n == len(res["frames"]) == plain["frame_cnt"] > 0
    # without lpips: today's keys, today's file text
    assert set(plain) == RESULT_KEYS
    assert all(set(f) == {"video_idx", "tstamp", *BASE} for f in plain["frames"])
    assert open(os.path.join(plain_dir, "logs", log_name)).read() == _today(plain, label)
    # with it: the same numbers plus the new ones
    assert set(res) == RESULT_KEYS | {"avg_lpips", "avg_masked_lpips"}
    for f, p in zip(res["frames"], plain["frames"]):
        assert set(f) == {"video_idx", "tstamp", "render", *BASE, "lpips", "masked_lpips"}
        assert all(f[k] == p[k] for k in ("video_idx", "tstamp", *BASE))
    assert all(res[f"avg_{k}"] == plain[f"avg_{k}"] for k in BASE) and res["avg_depth_l1"] is None
    for f in res["frames"]:
        gt = gt_of(f)
        render, mask = f["render"]["color"], f["render"]["mask"]
        assert 0.05 < float(mask.float().mean()), "the evaluation must see the scene"
        zero = torch.zeros((), device=gt.device)
        m_gt, m_render = torch.where(mask[..., None], gt, zero), torch.where(mask[..., None], render, zero)
        assert f["lpips"] == float(metric(gt, render)) and f["masked_lpips"] == float(metric(m_gt, m_render))
        assert f["lpips"] > 0.0 and f["masked_lpips"] > 0.0
        assert bool(mask.all()) or f["lpips"] != f["masked_lpips"], "the masked value is of the masked images"
    for k in ("lpips", "masked_lpips"):
        np.testing.assert_allclose(res[f"avg_{k}"], sum(f[k] for f in res["frames"]) / n, rtol=1e-12)
    # one frame against float64, with the value bound of tests/test_gpu_lpips.py
    f = res["frames"][0]
    a, b = gt_of(f).cpu().numpy(), f["render"]["color"].cpu().numpy()
    v = R.lpips(a, b, R.weights())[0]
    e32 = abs(R.torch_lpips(a, b, R.weights(), torch.float32)[0] - v)
    print(f"frame {f['tstamp']}: lpips {f['lpips']:.7f} against {v:.7f}, float32 composition error {e32:.2e}")
    assert abs(f["lpips"] - v) <= max(4.0 * e32, 8 * 2.0 ** -24 * abs(v))
    # the reference's eight lines in its order
    lines = open(os.path.join(out_dir, "logs", log_name)).read().split("\n")
    assert [l.split(":")[0] for l in lines] == [f"avg_masked_{label}", "avg_masked_psnr", "avg_masked_lpips",
                                                "###############", f"avg_{label}", "avg_psnr", "avg_lpips",
                                                "###############", ""]
    for i, key in ((0, "avg_masked_ms_ssim"), (1, "avg_masked_psnr"), (2, "avg_masked_lpips"), (4, "avg_ms_ssim"),
                   (5, "avg_psnr"), (6, "avg_lpips")):
        assert lines[i].split(": ")[1] == str(res[key])


def test_eval_kf_imgs_with_and_without_lpips(ran, tmp_path):
    from glorie_slam_amd.eval_render import eval_kf_imgs
    run, _, metric = ran
    out, plain_dir = str(tmp_path / "kf"), str(tmp_path / "kf_plain")
    res = eval_kf_imgs(run, output=out, keep_renders=True, lpips=metric)
    plain = eval_kf_imgs(run, output=plain_dir)
    _check(res, plain, out, plain_dir, "metrics_render_kf.txt", "ssim", metric,
           lambda f: run.images[f["video_idx"]].permute(1, 2, 0).contiguous())
    # SequenceRunner.evaluate forwards it
    again = run.evaluate(lpips=metric)
    assert [f["lpips"] for f in again["frames"]] == [f["lpips"] for f in res["frames"]]
    assert again["avg_masked_lpips"] == res["avg_masked_lpips"]


def test_eval_imgs_with_and_without_lpips(ran, tmp_path):
    from glorie_slam_amd.eval_render import eval_imgs
    from glorie_slam_amd.neural_point import se3_inv
    from glorie_slam_amd.pipeline import pose_matrix
    run, imgs, metric = ran
    poses = [pose_matrix(se3_inv(run.video.poses[k])).cpu().numpy() for k in range(2)]
    out, plain_dir = str(tmp_path / "every"), str(tmp_path / "every_plain")
    res = eval_imgs(run, ((k, imgs[k:k + 1]) for k in range(2)), poses, 1, output=out, keep_renders=True, lpips=metric)
    plain = eval_imgs(run, ((k, imgs[k:k + 1]) for k in range(2)), poses, 1, output=plain_dir)
    assert res["frame_cnt"] == 2
    _check(res, plain, out, plain_dir, "metrics_render_every.txt", "msssim", metric,
           lambda f: imgs[int(f["tstamp"])].permute(1, 2, 0).contiguous().to(run.device))


def test_frame_metrics_launches_nothing_more_without_lpips(gpu, monkeypatch):
    """lpips=None does not touch the LPIPS entry point"""
    from glorie_slam_amd import image_metrics
    from glorie_slam_amd import lpips as P
    monkeypatch.setattr(P.Lpips, "_run", lambda *a, **k: pytest.fail("LPIPS ran"))
    g = torch.Generator().manual_seed(3)
    a, b = torch.rand(H, W, 3, generator=g).to(gpu), torch.rand(H, W, 3, generator=g).to(gpu)
    depth = torch.rand(H, W, generator=g).to(gpu)
    fm = image_metrics.frame_metrics(a, depth, b, depth > 0.5)
    assert "lpips" not in fm and "masked_lpips" not in fm
