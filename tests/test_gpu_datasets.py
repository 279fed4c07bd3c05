"""Dataset streams on the device (glorie_slam_amd.datasets): files written with PIL come back as the restatement
(tests/ingest_ref.py) of the arrays that were written; an ArrayDataset feeds PoseTrajectoryFiller, SequenceRunner.run_stream
and traj_eval.full_traj_eval without adaptation."""
import os

import numpy as np
import pytest
import torch

import dataset_trees as T
import ingest_ref as R
import glorie_slam_amd.synth as synth

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
REC = np.load(os.path.join(HERE, "golden", "datasets.npz"))


# ---- files on disk ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["tumrgbd", "7scenes"])
def test_files_on_disk_come_back_as_the_restatement(name, gpu, tmp_path):
    from glorie_slam_amd.datasets import get_dataset
    col, dep = T.WRITERS[name](tmp_path)
    cam = T.small_cam(distortion=T.TUM_FR1 if name == "tumrgbd" else None, png_depth_scale=5000.0)
    ds = get_dataset(T.cfg_for(name, tmp_path, cam, 1, 100), device=str(gpu))
    want_poses = REC[f"{name}_1_-1_poses"]                       # max_frames 100 keeps every frame; -1 drops TUM's last
    if name == "tumrgbd":
        pairs = [tuple(REC["tum_assoc"][k][:2]) for k in REC["tum_kept"]]      # (image, depth) of every kept frame
        assert len(ds) == len(pairs) == 6 and len(want_poses) == 5
    else:
        pairs = [(k, k) for k in range(T.N)]
        assert len(ds) == T.N == len(want_poses)
    assert torch.equal(ds.get_intrinsic(), torch.from_numpy(R.intrinsic(cam)))
    items = list(ds)                                             # the stream iterates in index order and ends
    assert [it[0] for it in items] == list(range(len(ds)))
    for i, (index, color, depth, pose) in enumerate(items):
        ci, di = pairs[i]
        assert color.device == gpu and depth.device == gpu
        assert color.shape == (1, 3, 24, 40) and torch.equal(color.cpu(), torch.from_numpy(R.color(col[ci], cam)))
        assert depth.shape == (24, 40) and torch.equal(depth.cpu(), torch.from_numpy(R.depth(dep[di], cam)[0]))
        assert torch.equal(ds.get_color(i), color)
        assert pose.dtype == torch.float32 and pose.shape == (4, 4)
        if i < len(want_poses):
            if name == "tumrgbd":          # float32 of two float64 results 1e-13 apart (tests/test_datasets.py): one ulp
                assert torch.allclose(pose, torch.from_numpy(want_poses[i]).float(), rtol=0, atol=2.5e-7)
            else:
                assert torch.equal(pose, torch.from_numpy(want_poses[i]).float())
    batch = ds.get_colors(range(len(ds)))
    assert torch.equal(batch, torch.cat([it[1] for it in items]))
    with pytest.raises(IndexError):
        ds[len(ds)]


# ---- ArrayDataset through the trajectory filler ---------------------------------------------------------------------------
def test_array_dataset_feeds_the_trajectory_filler(gpu):
    """the scenario of tests/test_gpu_long_graphs.py::test_trajectory_filler_interpolates_and_refines, its hand-made stream
    replaced by an ArrayDataset (160x120 uint8 frames -> 136x104 -> crop 4 -> 128x96)"""
    from test_gpu_long_graphs import _stream_cfg, _t
    from glorie_slam_amd.datasets import ArrayDataset
    from glorie_slam_amd.depth_video import DepthVideo
    from glorie_slam_amd.droid_net import DroidNet
    from glorie_slam_amd.trajectory_filler import PoseTrajectoryFiller
    h, w, K = 12, 16, 5
    H, W = 8 * h, 8 * w
    video = DepthVideo(_stream_cfg(gpu, H, W, 16))
    gsyn = synth.keyframe_graph(K=K, h=h, w=w, radius=2)
    fmaps, nets, inps = synth.feature_maps(K, h, w)
    video.poses[:K] = _t(gsyn["poses"][:K], gpu)
    video.disps[:K] = _t(gsyn["disps"][:K], gpu)
    video.intrinsics[:] = _t(gsyn["intrinsics"][0], gpu)
    video.fmaps[:K], video.nets[:K], video.inps[:K] = _t(fmaps, gpu), _t(nets, gpu), _t(inps, gpu)
    video.timestamp[:K] = torch.arange(K, device=gpu).float() * 10.0
    video.counter.value = K
    torch.manual_seed(43)
    net = DroidNet().to(gpu).eval()
    filler = PoseTrajectoryFiller(net=net, video=video, printer=None, device=str(gpu), batch=4, iters=12)
    cam = dict(H=120, W=160, fx=150.0, fy=150.0, cx=80.0, cy=60.0, H_out=H, W_out=W, H_edge=4, W_edge=4)
    frames = np.random.default_rng(2).integers(0, 256, (6, 120, 160, 3), dtype=np.uint8)
    stream = ArrayDataset({"cam": cam}, frames, device=str(gpu))
    kf = video.poses[:K].clone()
    out = filler(stream)                                                 # batches of 4 + 2
    assert out.data.shape == (6, 7) and bool(torch.isfinite(out.data).all())
    assert video.counter.value == K and torch.equal(video.poses[:K], kf)
    assert torch.allclose(out.data[:, 3:].norm(dim=-1), torch.ones(6, device=gpu), atol=1e-4)
    assert out.inv().matrix().shape == (6, 4, 4)


# ---- run_stream and full_traj_eval ----------------------------------------------------------------------------------------
K_RUN, H_RUN, W_RUN = 4, 168, 224


def _run_stream_setup(gpu):
    from glorie_slam_amd import lie
    from glorie_slam_amd.datasets import ArrayDataset
    from glorie_slam_amd.pipeline import synthetic_images, synthetic_runner
    run, c = synthetic_runner(gpu, K_RUN, map_iters=2, map_rays=600, H=H_RUN, W=W_RUN)
    frames = (synthetic_images(K_RUN, 200, 264) * 255.0).round().to(torch.uint8).permute(0, 2, 3, 1).contiguous().numpy()
    fx, fy, cx, cy = c["intrinsics"].tolist()
    # a full-size camera whose working intrinsics are (close to) the runner's: 264x200 -> 232x176 -> crop 4 -> 224x168
    cam = dict(H=200, W=264, fx=fx * 264 / 232, fy=fy * 200 / 176, cx=(cx + 4) * 264 / 232, cy=(cy + 4) * 200 / 176,
               H_out=H_RUN, W_out=W_RUN, H_edge=4, W_edge=4)
    gt = lie.SE3(c["poses"][:K_RUN]).inv().matrix().cpu().numpy()       # the generating trajectory, camera-to-world
    return run, ArrayDataset({"cam": cam}, frames, poses=gt, device=str(gpu)), frames, cam


def test_run_stream_hands_track_the_ingested_frames(gpu):
    run, stream, frames, cam = _run_stream_setup(gpu)
    seen, track = [], run.track

    def recording_track(tstamp, image, intrinsics):
        seen.append((tstamp, image.clone(), intrinsics.clone()))
        return track(tstamp, image, intrinsics)

    run.track = recording_track
    run.run_stream(stream)
    want = torch.from_numpy(R.color(frames, cam))
    assert [s[0] for s in seen] == list(range(K_RUN))
    for k, (_, image, intrinsics) in enumerate(seen):
        assert image.shape == (1, 3, H_RUN, W_RUN) and torch.equal(image.cpu(), want[k:k + 1])
        assert torch.equal(intrinsics, stream.get_intrinsic()) and torch.equal(intrinsics, torch.from_numpy(R.intrinsic(cam)))


def test_run_stream_then_full_traj_eval(gpu, tmp_path):
    from glorie_slam_amd import lie
    from glorie_slam_amd.traj_eval import ape_statistics, full_traj_eval
    from glorie_slam_amd.trajectory_filler import PoseTrajectoryFiller
    run, stream, frames, cam = _run_stream_setup(gpu)
    summary = run.run_stream(stream)
    assert summary["keyframes"] == K_RUN and run.video.counter.value == K_RUN
    # the video buffer of this runner holds K + 2 frames: the filler parks 2 frames at a time behind the 4 keyframes
    filler = PoseTrajectoryFiller(net=run.net, video=run.video, printer=None, device=str(gpu), batch=2, iters=2)
    not_aligned, aligned, ref = full_traj_eval(filler, str(tmp_path), stream)
    assert not_aligned.shape == (K_RUN, 4, 4) and aligned.shape == ref.shape == (K_RUN, 4, 4)
    assert run.video.counter.value == K_RUN
    stamps = run.video.timestamp[:K_RUN].cpu().int().numpy()
    kf_c2w = lie.SE3(run.video.poses[:K_RUN].clone()).inv().matrix().cpu().numpy()
    assert np.array_equal(not_aligned[stamps], kf_c2w.astype(np.float64))
    assert np.array_equal(ref, np.asarray(stream.poses, np.float64))
    text = open(os.path.join(str(tmp_path), "metrics_full_traj.txt")).read()
    assert text.startswith("#" * 10 + "Full traj" + "#" * 10 + "\nscale: ")
    assert "\nrotation:\n" in text and "\ntranslation:" in text
    stats = ape_statistics(aligned, ref)
    assert text.endswith(f"statistics:\n{stats}")
    assert all(np.isfinite(v) for v in stats.values())
