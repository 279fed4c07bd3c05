"""float64 numpy restatement of the cloud deformation and the proxy depth (reference: src/neural_point.py:11-16,
:378-438, :446-506, :509-575; src/depth_video.py:313-324; src/mapper.py:246-279), the oracle of tests/golden/deform.npz
and of the HIP path (csrc/deform.hip)."""
import numpy as np


def quat_rot(q, dtype=np.float64):
    x, y, z, w = (dtype(v) for v in q)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]], dtype)


def c2w_of_pose(pose, opengl=True, dtype=np.float64, mutate=None):
    """DepthVideo.get_pose (SE3(w2c).inv().matrix()), columns 1 and 2 negated when opengl.  In another `dtype` every
    operation is rounded on its own, in the order csrc/deform.hip documents (frame_c2w: R from the quaternion, row a of
    the result is column a of R, t_a = -(R_0a tx + R_1a ty + R_2a tz)).  mutate "transpose": a deliberate mistake, one
    pair of rotation entries swapped (tests/test_deform_scenes.py)"""
    pose = np.asarray(pose, dtype)
    R = quat_rot(pose[3:], dtype)
    M = np.eye(4, dtype=dtype)
    if dtype == np.float64:
        M[:3, :3], M[:3, 3] = R.T, -(R.T @ pose[:3])
    else:
        for a in range(3):
            M[a, :3] = R[:, a]
            M[a, 3] = -(R[0, a] * pose[0] + R[1, a] * pose[1] + R[2, a] * pose[2])
    if opengl:
        M[:3, 1:3] *= -1
    if mutate == "transpose":
        M[0, 1], M[1, 0] = M[1, 0], M[0, 1]
    return M


def linspace_two_sided(start, end, steps, dtype):
    """torch.linspace(start, end, steps) in `dtype`: the two-sided form of the ATen kernel (linspace_f32 of deform.hip)"""
    start, end = dtype(start), dtype(end)
    if steps == 1:
        return np.array([start], dtype)
    step = (end - start) / dtype(steps - 1)
    return np.array([start + step * dtype(s) if s < steps // 2 else end - step * dtype(steps - s - 1)
                     for s in range(steps)], dtype)


def _mutated_camera(fx, fy, cx, cy, mutate):
    if mutate == "fy_fx":
        fx, fy = fy, fx
    if mutate == "cx_cy":
        cy = cx
    return fx, fy, cx, cy


def deform_ref(poses, disps_up, valid, dirty, vidx, pj, pi, input_depth, N_add, near, far, fix, fx, fy, cx, cy,
               nan_scale=False, dtype=np.float64, new_depth=None, mutate=None):
    """-> (input_pos [n,3], input_depth [n], cloud [n*N_add,3]) after update_points_pos(npc, video) in "proxy" mode;
    rows of clean keyframes are returned as NaN (the caller keeps its own).  nan_scale: a keyframe with no valid depth
    scales by 0/0 (the reference) instead of 1.
    dtype: float64 is the restatement; float32 is the plain composition of the same formulas with every operation
    rounded on its own, in the order csrc/deform.hip documents (the yardstick of tests/test_gpu_deform_kernels.py).
    new_depth [n]: place the points on these depths instead of computing them (an error of the scale then cannot hide
    in the positions).  mutate: a deliberate mistake, "fy_fx", "cx_cy" or "transpose" (tests/test_deform_scenes.py)"""
    n = len(vidx)
    pos = np.full((n, 3), np.nan, dtype)
    depth = np.asarray(input_depth, dtype).copy()
    cloud = np.full((n * N_add, 3), np.nan, dtype)
    exact = dtype == np.float64
    t = np.linspace(0.0, 1.0, N_add) if exact else linspace_two_sided(0.0, 1.0, N_add, dtype)
    fx, fy, cx, cy = (dtype(x) for x in _mutated_camera(fx, fy, cx, cy, mutate))
    for v in np.nonzero(dirty)[0]:
        m = vidx == v
        if not m.any():
            continue
        j, i = pj[m], pi[m]
        if new_depth is not None:
            d = np.asarray(new_depth, dtype)[m]
        else:
            d = np.where(valid[v, j, i], dtype(1) / disps_up[v, j, i].astype(dtype), dtype(0))
            prev = depth[m]
            bad = d == 0
            if bad.any():
                den = np.sum(prev[~bad] ** 2)
                s = np.sum(prev[~bad] * d[~bad]) / den if den != 0 else (np.nan if nan_scale else 1.0)
                d[bad] = dtype(s) * prev[bad]
        c2w = c2w_of_pose(poses[v], dtype=dtype, mutate=mutate)
        dirs = np.stack([(i.astype(dtype) - cx) / fx, -((j.astype(dtype) - cy) / fy), -np.ones(len(i), dtype)], -1)
        if exact:
            rd = dirs @ c2w[:3, :3].T
        else:                                                      # row sums, left to right
            rd = np.stack([dirs[:, 0] * c2w[a, 0] + dirs[:, 1] * c2w[a, 1] + dirs[:, 2] * c2w[a, 2] for a in range(3)], -1)
        ro = c2w[:3, 3]
        pos[m] = ro + rd * d[:, None]
        depth[m] = d
        lin = np.linspace(-0.04, 0.04, N_add) if exact else linspace_two_sided(-0.04, 0.04, N_add, dtype)
        z = d[:, None] + lin[None] if fix else \
            dtype(near) * d[:, None] * (1 - t)[None] + dtype(far) * d[:, None] * t[None]
        rows = (np.nonzero(m)[0][:, None] * N_add + np.arange(N_add)[None]).reshape(-1)
        cloud[rows] = (ro + rd[:, None, :] * z[..., None]).reshape(-1, 3)
    return pos, depth, cloud


def skip_row(counter, mapping_window_size, H):
    r = int(counter) - int(mapping_window_size)
    return r % H if -H <= r < H else -1


def proj_depth_ref(full_pcl, full_mask, counter, mapping_window_size, c2w, fx, fy, cx, cy, dtype=np.float64, w2c=None,
                   row=None, mutate=None, details=False):
    """proj_depth_map(neural_pcl=False) over keyframes [0, counter) with row counter - mapping_window_size of every
    keyframe left out (none when the reference would raise): nearest point per pixel, 0 where none.
    dtype float32: the plain composition, every operation rounded on its own in the order of project() as deform.hip
    compiles it (row sums left to right, then z = c + 1e-6, u = (fx (-a) + cx c) / z, v = (fy b + cy c) / z), the matrix
    inverse in float32 as well.  w2c: the world-to-camera matrix itself (c2w is then unused); row: the image row left
    out, -1 for none (counter - mapping_window_size is then unused); mutate: a deliberate mistake, "fy_fx", "cx_cy",
    "transpose", "no_skip_row" or "gt_zero"; details: also return dict(u, v, z, inside, index) of the points read
    (index: their position in the flattened [counter, H, W] maps)"""
    B, H, W = full_mask.shape
    mask = np.asarray(full_mask, bool)[:counter].copy()
    r = skip_row(counter, mapping_window_size, H) if row is None else int(row)
    if r >= 0 and mutate != "no_skip_row":
        mask[:, r] = False
    X = np.asarray(full_pcl, dtype)[:counter][mask]
    w2c = np.linalg.inv(np.asarray(c2w, dtype)) if w2c is None else np.array(w2c, dtype)
    if mutate == "transpose":
        w2c[0, 1], w2c[1, 0] = w2c[1, 0], w2c[0, 1]
    fx, fy, cx, cy = (dtype(x) for x in _mutated_camera(fx, fy, cx, cy, mutate))
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        if dtype == np.float64:
            Xc = X @ w2c[:3, :3].T + w2c[:3, 3]
        else:
            Xc = np.stack([w2c[a, 0] * X[:, 0] + w2c[a, 1] * X[:, 1] + w2c[a, 2] * X[:, 2] + w2c[a, 3] for a in range(3)],
                          -1).reshape(-1, 3)
        Xc[:, 0] *= -1
        z = Xc[:, 2] + dtype(1e-6)
        u = (fx * Xc[:, 0] + cx * Xc[:, 2]) / z
        v = (fy * Xc[:, 1] + cy * Xc[:, 2]) / z
        lo = (lambda x: x > 0) if mutate == "gt_zero" else (lambda x: x >= 0)
        m = (u < W) & lo(u) & (v < H) & lo(v) & (-z > 0)
    out = np.full(H * W, np.inf, dtype)
    np.minimum.at(out, v[m].astype(np.int64) * W + u[m].astype(np.int64), -z[m])
    out[np.isinf(out)] = 0
    if details:
        return out.reshape(H, W), dict(u=u, v=v, z=z, inside=m, index=np.nonzero(mask.reshape(-1))[0])
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
