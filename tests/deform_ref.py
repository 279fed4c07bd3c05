"""float64 numpy restatement of the cloud deformation and the proxy depth (reference: src/neural_point.py:11-16,
:378-438, :446-506, :509-575; src/depth_video.py:313-324; src/mapper.py:246-279), the oracle of tests/golden/deform.npz
and of the HIP path (csrc/deform.hip)."""
import numpy as np


def quat_rot(q):
    x, y, z, w = (float(v) for v in q)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def c2w_of_pose(pose, opengl=True):
    """DepthVideo.get_pose (SE3(w2c).inv().matrix()), columns 1 and 2 negated when opengl"""
    pose = np.asarray(pose, np.float64)
    R = quat_rot(pose[3:])
    M = np.eye(4)
    M[:3, :3], M[:3, 3] = R.T, -(R.T @ pose[:3])
    if opengl:
        M[:3, 1:3] *= -1
    return M


def deform_ref(poses, disps_up, valid, dirty, vidx, pj, pi, input_depth, N_add, near, far, fix, fx, fy, cx, cy,
               nan_scale=False):
    """-> (input_pos [n,3], input_depth [n], cloud [n*N_add,3]) after update_points_pos(npc, video) in "proxy" mode;
    rows of clean keyframes are returned as NaN (the caller keeps its own).  nan_scale: a keyframe with no valid depth
    scales by 0/0 (the reference) instead of 1"""
    n = len(vidx)
    pos = np.full((n, 3), np.nan)
    depth = np.asarray(input_depth, np.float64).copy()
    cloud = np.full((n * N_add, 3), np.nan)
    t = np.linspace(0.0, 1.0, N_add)
    for v in np.nonzero(dirty)[0]:
        m = vidx == v
        if not m.any():
            continue
        j, i = pj[m], pi[m]
        d = np.where(valid[v, j, i], 1.0 / disps_up[v, j, i].astype(np.float64), 0.0)
        prev = depth[m]
        bad = d == 0
        if bad.any():
            den = np.sum(prev[~bad] ** 2)
            s = np.sum(prev[~bad] * d[~bad]) / den if den != 0 else (np.nan if nan_scale else 1.0)
            d[bad] = s * prev[bad]
        c2w = c2w_of_pose(poses[v])
        dirs = np.stack([(i - cx) / fx, -(j - cy) / fy, -np.ones(len(i))], -1)
        rd = dirs @ c2w[:3, :3].T
        ro = c2w[:3, 3]
        pos[m] = ro + rd * d[:, None]
        depth[m] = d
        z = d[:, None] + np.linspace(-0.04, 0.04, N_add)[None] if fix else \
            near * d[:, None] * (1 - t)[None] + far * d[:, None] * t[None]
        rows = (np.nonzero(m)[0][:, None] * N_add + np.arange(N_add)[None]).reshape(-1)
        cloud[rows] = (ro + rd[:, None, :] * z[..., None]).reshape(-1, 3)
    return pos, depth, cloud


def skip_row(counter, mapping_window_size, H):
    r = int(counter) - int(mapping_window_size)
    return r % H if -H <= r < H else -1


def proj_depth_ref(full_pcl, full_mask, counter, mapping_window_size, c2w, fx, fy, cx, cy):
    """proj_depth_map(neural_pcl=False) over keyframes [0, counter) with row counter - mapping_window_size of every
    keyframe left out (none when the reference would raise): nearest point per pixel, 0 where none"""
    B, H, W = full_mask.shape
    mask = np.asarray(full_mask, bool)[:counter].copy()
    r = skip_row(counter, mapping_window_size, H)
    if r >= 0:
        mask[:, r] = False
    X = np.asarray(full_pcl, np.float64)[:counter][mask]
    w2c = np.linalg.inv(np.asarray(c2w, np.float64))
    Xc = X @ w2c[:3, :3].T + w2c[:3, 3]
    Xc[:, 0] *= -1
    z = Xc[:, 2] + 1e-6
    u = (fx * Xc[:, 0] + cx * Xc[:, 2]) / z
    v = (fy * Xc[:, 1] + cy * Xc[:, 2]) / z
    m = (u < W) & (u >= 0) & (v < H) & (v >= 0) & (-z > 0)
    out = np.full(H * W, np.inf)
    np.minimum.at(out, v[m].astype(np.int64) * W + u[m].astype(np.int64), -z[m])
    out[np.isinf(out)] = 0
    return out.reshape(H, W)


def proxy_depth_ref(proj, droid, mono, use_mono_to_complete=True):
    """get_proxy_render_depth from the projected depth"""
    p = np.asarray(droid, np.float64).copy()
    take = ~(p > 0) & (proj > 0)
    p[take] = proj[take]
    if use_mono_to_complete:
        p[p == 0] = np.asarray(mono, np.float64)[p == 0]
    return p


def align_ref(mono, target, weights):
    """align_scale_and_shift (common.py:401-437) in float64: (scale, shift)"""
    w = np.asarray(weights, np.float64)
    p, t = np.asarray(mono, np.float64), np.asarray(target, np.float64)
    a00, a01, a11 = (w * p * p).sum(), (w * p).sum(), w.sum()
    b0, b1 = (w * p * t).sum(), (w * t).sum()
    det = a00 * a11 - a01 * a01
    return (a11 * b0 - a01 * b1) / det, (-a01 * b0 + a00 * b1) / det


def c2w_and_depth_ref(pose, disps_up, valid, mono):
    """Mapper.get_c2w_and_depth: (c2w OpenGL, mono_wq, droid depth with 0 outside valid), None below 100 valid pixels"""
    if valid.sum() < 100:
        return None
    droid = np.where(valid, 1.0 / disps_up.astype(np.float64), 0.0)
    w = (mono < mono.astype(np.float64).mean() * 3) & valid
    s, b = align_ref(mono, droid, w)
    return c2w_of_pose(pose), mono * s + b, droid
