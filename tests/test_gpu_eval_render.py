"""The re-render evaluation (glorie_slam_amd/eval_render.py, SequenceRunner.evaluate) end to end on the synthetic stream
at 168 x 224 (a multiple of 8 for the tracker, the smaller side above MS-SSIM's 160): every reported number against the
float64 reference of tests/image_metrics_ref.py recomputed from the saved maps and the runner's stored images, with the
bound of tests/test_gpu_image_metrics.py; the runner is only read."""
import os

import numpy as np
import pytest
import torch

import image_metrics_ref as R

pytestmark = pytest.mark.gpu

H, W = 168, 224
FACTOR, FLOOR = 4.0, 2e-6


def _ssim_close(got, a, b, tag):
    """the bound of tests/test_gpu_image_metrics.py: 4 times the error of the float32 composition, at least 2e-6 (the
    composition is only run when the error is above the floor)"""
    v = R.ms_ssim(a, b)[0]
    err = abs(got - v)
    print(f"{tag}: {got:.7f} against {v:.7f}, error {err:.2e}")
    if err > FLOOR:
        assert err <= FACTOR * abs(R.torch_ms_ssim(a, b, 5, torch.float32)[0] - v)


def _snapshot(run):
    npc = run.npc
    return ({k: v.clone() for k, v in run.images.items()}, npc.cloud_pos().clone(), npc.geo_feats.clone(),
            npc.col_feats.clone(), run.video.poses.clone(), run.video.disps_up.clone())


def _unchanged(run, snap):
    images, pos, geo, col, poses, disps_up = snap
    assert sorted(images) == sorted(run.images) and all(torch.equal(images[k], run.images[k]) for k in images)
    npc = run.npc
    assert torch.equal(pos, npc.cloud_pos()) and torch.equal(geo, npc.geo_feats) and torch.equal(col, npc.col_feats)
    assert torch.equal(poses, run.video.poses) and torch.equal(disps_up, run.video.disps_up)


def _numbers(res):
    keys = ("psnr", "ms_ssim", "masked_psnr", "masked_ms_ssim", "depth_l1")
    rows = [[f["video_idx"], f["tstamp"]] + [f[k] for k in keys if k in f] for f in res["frames"]]
    rows.append([res["frame_cnt"]] + [res[f"avg_{k}"] for k in keys if res[f"avg_{k}"] is not None])
    return np.array([x for r in rows for x in r], dtype=np.float64)


def _check_against_the_reference(run, res, out_dir, subdir, log_name, label, gt_of, gt_depth_of=None):
    """files, line order and every per-frame number of `res`; gt_of(frame) -> the [H,W,3] float32 image it was scored on"""
    assert sorted(os.listdir(os.path.join(out_dir, subdir))) == sorted(
        f"{kind}_{int(f['tstamp']):05d}.npy" for f in res["frames"] for kind in ("depth", "color"))
    lines = open(os.path.join(out_dir, "logs", log_name)).read().split("\n")
    assert [l.split(":")[0] for l in lines] == [f"avg_masked_{label}", "avg_masked_psnr", "###############", f"avg_{label}",
                                                "avg_psnr", "###############", ""]
    for line, key in ((lines[0], "avg_masked_ms_ssim"), (lines[1], "avg_masked_psnr"), (lines[3], "avg_ms_ssim"),
                      (lines[4], "avg_psnr")):
        assert line.split(": ")[1] == str(res[key])
    keys = [k for k in ("psnr", "ms_ssim", "masked_psnr", "masked_ms_ssim", "depth_l1") if k in res["frames"][0]]
    for f in res["frames"]:
        ts = int(f["tstamp"])
        color = np.load(os.path.join(out_dir, subdir, f"color_{ts:05d}.npy"))
        depth = np.load(os.path.join(out_dir, subdir, f"depth_{ts:05d}.npy"))
        gt = gt_of(f)
        render, r_depth = f["render"]["color"].cpu().numpy(), f["render"]["depth"].float().cpu().numpy()
        mask = f["render"]["mask"].cpu().numpy()
        assert color.dtype == np.float32 and color.shape == (H, W, 3) and depth.dtype == np.float32 and depth.shape == (H, W)
        assert np.array_equal(color, np.where(mask[..., None], render, np.float32(0)))
        assert np.array_equal(depth, np.where(mask, r_depth, np.float32(0)))
        assert 0.05 < mask.mean(), "the evaluation must see the scene"
        np.testing.assert_allclose(f["psnr"], R.psnr(gt, render), rtol=1e-6)
        np.testing.assert_allclose(f["masked_psnr"], R.psnr(gt, color, mask), rtol=1e-6)
        _ssim_close(f["ms_ssim"], gt, render, f"frame {ts} ms_ssim")
        _ssim_close(f["masked_ms_ssim"], np.where(mask[..., None], gt, np.float32(0)), color, f"frame {ts} masked_ms_ssim")
        if gt_depth_of is not None:
            gd = gt_depth_of(f)
            assert not (mask & ~(gd > 0)).any()
            np.testing.assert_allclose(f["depth_l1"], R.depth_l1(depth, gd, mask), rtol=1e-6)
    n = res["frame_cnt"]
    for k in keys:
        np.testing.assert_allclose(res[f"avg_{k}"], sum(f[k] for f in res["frames"]) / n, rtol=1e-12)


def _own_poses(run, n):
    from glorie_slam_amd.neural_point import se3_inv
    from glorie_slam_amd.pipeline import pose_matrix
    return [pose_matrix(se3_inv(run.video.poses[k])).cpu().numpy() for k in range(n)]


def test_evaluate_after_a_run(gpu, tmp_path):
    from glorie_slam_amd.eval_render import eval_imgs
    from glorie_slam_amd.pipeline import synthetic_images, synthetic_runner
    K = 10
    run, c = synthetic_runner(gpu, K, zero_flow_head=True, map_iters=4, map_rays=600, H=H, W=W)
    imgs = synthetic_images(K, H, W)
    summary = run.run(((k, imgs[k:k + 1]) for k in range(K)), c["intrinsics"], final_ba_steps=2)
    assert summary["mapped"] == run.mapped > 3
    snap = _snapshot(run)
    out = str(tmp_path / "kf")
    res = run.evaluate(output=out, keep_renders=True)
    torch.cuda.synchronize()
    _unchanged(run, snap)
    assert res["frame_cnt"] == run.mapped - len(run.skipped) == len(res["frames"])
    assert [f["video_idx"] for f in res["frames"]] == [k for k in range(run.mapped) if k not in run.skipped]
    assert res["avg_depth_l1"] is None and "depth_l1" not in res["frames"][0]
    _check_against_the_reference(run, res, out, "rendered_every_keyframe", "metrics_render_kf.txt", "ssim",
                                 lambda f: run.images[f["video_idx"]].permute(1, 2, 0).cpu().numpy())
    # a second evaluation (without files, without the renders) reports the same numbers
    again = run.evaluate()
    assert "render" not in again["frames"][0]
    assert np.array_equal(_numbers(again), _numbers(res), equal_nan=True)
    _unchanged(run, snap)
    # eval_imgs on the keyframes' own poses: every fourth frame of the stream
    poses = _own_poses(run, run.mapped)
    keep = [p.copy() for p in poses]
    out = str(tmp_path / "every")
    every = eval_imgs(run, ((k, imgs[k:k + 1]) for k in range(run.mapped)), poses, 4, output=out, keep_renders=True)
    assert [f["tstamp"] for f in every["frames"]] == [float(k) for k in range(0, run.mapped, 4)]
    assert all(np.array_equal(a, b) for a, b in zip(poses, keep))
    assert all(np.isfinite(f[k]) for f in every["frames"] for k in ("psnr", "ms_ssim", "masked_psnr", "masked_ms_ssim"))
    _check_against_the_reference(run, every, out, "rendered_every_frame", "metrics_render_every.txt", "msssim",
                                 lambda f: imgs[int(f["tstamp"])].permute(1, 2, 0).numpy())
    _unchanged(run, snap)


def test_evaluate_on_the_proxy_depth_with_colour_gradient_radii(gpu, tmp_path, monkeypatch):
    """render_depth "proxy" and the colour-gradient radii: every keyframe is rendered on its proxy depth with its own
    query radius map; one keyframe has too few tracker depths and is skipped by the mapper, so by the evaluation;
    gt_depth_fn adds depth L1 and takes its holes out of the mask"""
    import glorie_slam_amd.pipeline as P
    from glorie_slam_amd.color_grad import COLOR_GRAD_THRESHOLD, RADIUS_ADD_MAX, RADIUS_ADD_MIN, RADIUS_QUERY_RATIO
    from glorie_slam_amd.eval_render import eval_imgs
    K, SKIP = 5, 2
    orig = P.synthetic_cfg

    def cfg(*a, **k):
        c = orig(*a, **k)
        c["pointcloud"].update(bind_npc_with_pose=True, radius_add_max=RADIUS_ADD_MAX, radius_add_min=RADIUS_ADD_MIN,
                               radius_query_ratio=RADIUS_QUERY_RATIO, color_grad_threshold=COLOR_GRAD_THRESHOLD)
        c["mapping"]["render_depth"] = "proxy"
        return c
    monkeypatch.setattr(P, "synthetic_cfg", cfg)
    run, c = P.synthetic_runner(gpu, K, map_iters=4, map_rays=600, H=H, W=W)
    monkeypatch.setattr(P, "synthetic_cfg", orig)
    assert run.render_depth == "proxy" and run.color_grad is not None
    video, imgs = c["video"], P.synthetic_images(K, H, W)
    g = torch.Generator().manual_seed(7)
    for k in range(K):
        run.init_state(k)
        video.timestamp[k] = k
        run.images[k] = imgs[k].to(gpu)
        m = torch.rand(H, W, generator=g) > 0.1
        m[:, 30 + 15 * k: 60 + 15 * k] = False
        if k == SKIP:
            m[:] = False
            m[:5, :10] = True                                       # 50 valid pixels: not mapped
        video.valid_depth_mask[k] = m.to(gpu)
    video.intrinsics[:K] = c["intrinsics"].to(gpu) / 8.0
    video.counter.value = K
    for k in range(K):
        run.map_keyframe(k)
        run.mapped += 1
    assert run.skipped == [SKIP]
    seen = []
    radius_maps = run._radius_maps
    monkeypatch.setattr(run, "_radius_maps", lambda f, view, **kw: (seen.append((f, kw)), radius_maps(f, view, **kw))[1])
    gt_depth = (1.0 / video.disps_up[:K]).clone()
    gt_depth[:, :7, :] = 0.0                                        # holes of the sensor
    snap = _snapshot(run)
    out = str(tmp_path / "kf")
    res = run.evaluate(output=out, gt_depth_fn=lambda ts: gt_depth[int(ts)].cpu(), keep_renders=True)
    torch.cuda.synchronize()
    _unchanged(run, snap)
    assert res["frame_cnt"] == K - 1 and [f["video_idx"] for f in res["frames"]] == [0, 1, 3, 4]
    assert [s[0] for s in seen] == [0, 1, 3, 4] and all(s[1] == {"add": False} for s in seen)
    assert res["avg_depth_l1"] is not None and np.isfinite(res["avg_depth_l1"])
    _check_against_the_reference(run, res, out, "rendered_every_keyframe", "metrics_render_kf.txt", "ssim",
                                 lambda f: run.images[f["video_idx"]].permute(1, 2, 0).cpu().numpy(),
                                 gt_depth_of=lambda f: gt_depth[f["video_idx"]].cpu().numpy())
    # eval_imgs over the unprojected keyframe maps
    out = str(tmp_path / "every")
    every = eval_imgs(run, ((k, imgs[k]) for k in range(K)), _own_poses(run, K), 3, output=out, keep_renders=True)
    assert [f["tstamp"] for f in every["frames"]] == [0.0, 3.0]
    assert all(np.isfinite(f[k]) for f in every["frames"] for k in ("psnr", "ms_ssim", "masked_psnr", "masked_ms_ssim"))
    _check_against_the_reference(run, every, out, "rendered_every_frame", "metrics_render_every.txt", "msssim",
                                 lambda f: imgs[int(f["tstamp"])].permute(1, 2, 0).numpy())
    _unchanged(run, snap)
