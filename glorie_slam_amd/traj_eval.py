"""Keyframe trajectory evaluation (reference: src/utils/eval_traj.py:5-40 align_kf_traj, :98-134 kf_traj_eval, which call
evo): the closed-form Sim3 alignment of the estimated keyframe positions to the ground truth, and the statistics of the
absolute position error.  numpy float64 on the host - a few hundred poses.

  umeyama          least-squares similarity between two point sets (Umeyama 1991)
  align_kf_traj    the alignment of the keyframes of video.npz to ground-truth poses by timestamp
  ape_statistics   rmse, mean, median, std, min, max, sse of the translation part
  kf_traj_eval     writes metrics_kf_traj.txt and stores `scale` back into video.npz
  align_full_traj  the alignment of every frame's pose to a stream's ground truth (eval_traj.py:42-65)
  full_traj_eval   the trajectory filler over a dataset stream, keyframes from the video; writes metrics_full_traj.txt
                   (eval_traj.py:137-169)

A monocular map has no metric scale: generate_mesh.generate_mesh_kf takes the scale and the 4x4 of this alignment.
Out of scope: the trajectory plots and the camera visualiser (matplotlib).
"""
import os

import numpy as np

_STATS = ("rmse", "mean", "median", "std", "min", "max", "sse")


def umeyama(est_xyz, ref_xyz, with_scale=True):
    """est_xyz, ref_xyz [n,3] -> (r [3,3], t [3], s) minimising sum |ref - (s r est + t)|^2 (s = 1 without with_scale)"""
    x, y = np.asarray(est_xyz, np.float64), np.asarray(ref_xyz, np.float64)
    if x.shape != y.shape or x.ndim != 2 or x.shape[1] != 3 or len(x) < 3:
        raise ValueError(f"need two [n,3] point sets with n >= 3, got {x.shape} and {y.shape}")
    mx, my = x.mean(0), y.mean(0)
    xc, yc = x - mx, y - my
    var_x = (xc ** 2).sum() / len(x)
    cov = yc.T @ xc / len(x)
    u, d, vt = np.linalg.svd(cov)
    if np.count_nonzero(d > np.finfo(d.dtype).eps) < 2:
        raise ValueError("degenerate covariance: the points do not span a plane")
    sgn = np.eye(3)
    if np.linalg.det(u) * np.linalg.det(vt) < 0:
        sgn[2, 2] = -1.0
    r = u @ sgn @ vt
    s = float(np.trace(np.diag(d) @ sgn) / var_x) if with_scale else 1.0
    t = my - s * (r @ mx)
    return r, t, s


def se3(r, t):
    m = np.eye(4)
    m[:3, :3], m[:3, 3] = r, t
    return m


def _apply(poses, r, t, s):
    """scale the translations by s, then left-multiply by se3(r, t)"""
    poses = np.array(poses, np.float64, copy=True)
    poses[:, :3, 3] *= s
    return se3(r, t) @ poses


def align_kf_traj(video_npz, gt_c2w_by_timestamp, return_full_est_traj=False):
    """video_npz: path of video.npz or its dict (poses [n,4,4] c2w, timestamps [n]); gt_c2w_by_timestamp: indexable by
    the integer timestamp -> [4,4].  Keyframes whose ground-truth pose holds NaN or Inf are skipped.
    -> (r_a, t_a, s, est_poses, ref_poses): the aligned estimated poses of the kept keyframes - of all keyframes with
    return_full_est_traj - and the ground-truth poses of the kept ones"""
    video = dict(np.load(video_npz)) if isinstance(video_npz, (str, os.PathLike)) else video_npz
    poses, stamps = np.asarray(video["poses"], np.float64), np.asarray(video["timestamps"])
    est, ref = [], []
    for i in range(stamps.shape[0]):
        gt = np.asarray(gt_c2w_by_timestamp[int(stamps[i])], np.float64)
        if not np.isfinite(gt.sum()):
            continue
        est.append(poses[i])
        ref.append(gt)
    if len(est) < 3:
        raise ValueError("fewer than 3 keyframes have a finite ground-truth pose")
    est, ref = np.stack(est), np.stack(ref)
    r_a, t_a, s = umeyama(est[:, :3, 3], ref[:, :3, 3], with_scale=True)
    return r_a, t_a, s, _apply(poses if return_full_est_traj else est, r_a, t_a, s), ref


def ape_statistics(est_poses, ref_poses):
    """absolute position error |t_est - t_ref| per pose -> {rmse, mean, median, std, min, max, sse}"""
    est, ref = np.asarray(est_poses, np.float64), np.asarray(ref_poses, np.float64)
    e = np.linalg.norm(est[:, :3, 3] - ref[:, :3, 3], axis=1)
    values = (np.sqrt(np.mean(e ** 2)), np.mean(e), np.median(e), np.std(e), np.min(e), np.max(e), np.sum(e ** 2))
    return {k: float(v) for k, v in zip(_STATS, values)}


def kf_traj_eval(video_npz, out_dir, gt):
    """align the keyframes of `video_npz` (a path) to gt, write out_dir/metrics_kf_traj.txt (header, scale, rotation,
    translation, statistics, as the reference) and store `scale` in video.npz.  -> (statistics, s, r_a, t_a)"""
    r_a, t_a, s, est, ref = align_kf_traj(video_npz, gt)
    stats = ape_statistics(est, ref)
    os.makedirs(out_dir, exist_ok=True)
    text = "#" * 10 + "Keyframes traj" + "#" * 10 + "\n"
    text += f"scale: {s}\n"
    text += f"rotation:\n{r_a}\n"
    text += f"translation:{t_a}\n"
    text += f"statistics:\n{stats}"
    with open(os.path.join(out_dir, "metrics_kf_traj.txt"), "w+") as fp:
        fp.write(text)
    video = dict(np.load(video_npz))
    video["scale"] = np.array(s)
    np.savez(video_npz, **video)
    return stats, s, r_a, t_a


def align_full_traj(traj_est_full, gt_poses):
    """src/utils/eval_traj.py:42-65.  traj_est_full [n,4,4] c2w of every frame, gt_poses: n ground-truth c2w (a stream's
    `poses`).  The frames whose ground-truth pose holds NaN or Inf are skipped.
    -> (r_a, t_a, s, est_poses, ref_poses): the aligned estimates and the ground truth of the kept frames"""
    full = np.asarray(traj_est_full, np.float64)
    if len(gt_poses) != len(full):
        raise ValueError(f"{len(full)} estimated poses, {len(gt_poses)} ground-truth poses")
    est, ref = [], []
    for i in range(len(gt_poses)):
        gt = np.asarray(gt_poses[i], np.float64)
        if not np.isfinite(gt.sum()):
            continue
        est.append(full[i])
        ref.append(gt)
    if len(est) < 3:
        raise ValueError("fewer than 3 frames have a finite ground-truth pose")
    est, ref = np.stack(est), np.stack(ref)
    r_a, t_a, s = umeyama(est[:, :3, 3], ref[:, :3, 3], with_scale=True)
    return r_a, t_a, s, _apply(est, r_a, t_a, s), ref


def full_traj_eval(traj_filler, out_dir, stream):
    """src/utils/eval_traj.py:137-169: the pose of every frame of `stream` from the trajectory filler (a
    PoseTrajectoryFiller; world-to-camera, inverted here), the keyframes' entries overwritten with the keyframes' own
    poses, aligned to stream.poses; writes out_dir/metrics_full_traj.txt.
    -> (traj_est_not_aligned [n,4,4], traj_est_aligned [m,4,4], traj_ref [m,4,4]) float64 numpy, m = the frames with a
    finite ground-truth pose"""
    from . import lie
    video = traj_filler.video
    traj_est = traj_filler(stream).inv().matrix().detach().cpu().numpy().astype(np.float64)
    kf_num = video.counter.value
    kf_timestamps = video.timestamp[:kf_num].cpu().int().numpy()
    kf_poses = lie.SE3(video.poses[:kf_num].clone()).inv().matrix().detach().cpu().numpy()
    traj_est[kf_timestamps] = kf_poses
    traj_est_not_aligned = traj_est.copy()
    r_a, t_a, s, est, ref = align_full_traj(traj_est, stream.poses)
    stats = ape_statistics(est, ref)
    os.makedirs(out_dir, exist_ok=True)
    text = "#" * 10 + "Full traj" + "#" * 10 + "\n"
    text += f"scale: {s}\n"
    text += f"rotation:\n{r_a}\n"
    text += f"translation:{t_a}\n"
    text += f"statistics:\n{stats}"
    with open(os.path.join(out_dir, "metrics_full_traj.txt"), "w+") as fp:
        fp.write(text)
    return traj_est_not_aligned, est, ref
