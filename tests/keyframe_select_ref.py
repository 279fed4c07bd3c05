"""Float64 restatement of the mapper's frustum feature selection and keyframe overlap figure (src/mapper.py:126-174 and
:176-244) for the tests: numpy, no cv2.

frustum_ref -> (mask [n] bool, details): details holds the decisive quantities (u, v, -z, the depth sample after the
zero -> maximum replacement, the sample before it) so that a test can tell a real disagreement from one at a threshold.
The depth sample is cv2.remap(INTER_LINEAR, BORDER_CONSTANT 0): map coordinates rounded to 1/32 px (round half to even),
neighbours outside the image read 0.
overlap_ref -> (inside [K] int, number of samples): rays whose depth is not > 0 are dropped (get_samples' depth_filter).
"""
import numpy as np

OVERLAP_EDGE = 20


def project(c2w, X, fx, fy, cx, cy):
    """c2w [4,4] (OpenGL convention), X [n,3] -> u, v, z (z with the + 1e-5), float64"""
    w2c = np.linalg.inv(np.asarray(c2w, np.float64))
    p = np.asarray(X, np.float64) @ w2c[:3, :3].T + w2c[:3, 3]
    a, b, c = -p[:, 0], p[:, 1], p[:, 2]
    z = c + 1e-5
    return (fx * a + cx * c) / z, (fy * b + cy * c) / z, z


def remap_linear(depth, u, v):
    """cv2.remap(depth, u, v, INTER_LINEAR) with BORDER_CONSTANT 0 at n points (float64 weights)"""
    depth = np.asarray(depth, np.float64)
    H, W = depth.shape
    out = np.zeros(len(u))
    ok = np.isfinite(u) & np.isfinite(v) & (u > -2) & (u < W + 1) & (v > -2) & (v < H + 1)
    X = np.rint(np.where(ok, u, 0) * 32).astype(np.int64)
    Y = np.rint(np.where(ok, v, 0) * 32).astype(np.int64)
    x0, y0 = X >> 5, Y >> 5
    ax, ay = (X & 31) / 32.0, (Y & 31) / 32.0
    for dx, dy, wgt in ((0, 0, (1 - ax) * (1 - ay)), (1, 0, ax * (1 - ay)), (0, 1, (1 - ax) * ay), (1, 1, ax * ay)):
        xi, yi = x0 + dx, y0 + dy
        inb = ok & (xi >= 0) & (xi < W) & (yi >= 0) & (yi < H)
        out += np.where(inb, depth[np.clip(yi, 0, H - 1), np.clip(xi, 0, W - 1)], 0.0) * wgt
    return out


def frustum_ref(points, c2w, depth, fx, fy, cx, cy, H, W, edge):
    u, v, z = project(c2w, points, fx, fy, cx, cy)
    sample = remap_linear(depth, u, v)
    d = np.where(sample == 0, sample.max() if len(sample) else 0.0, sample)
    inside = (u < W - edge) & (u > edge) & (v < H - edge) & (v > edge)
    mask = inside & (0 <= -z) & (-z <= d + 0.5)
    return mask, dict(u=u, v=v, negz=-z, depth=d, sample=sample)


def sample_points(rays_o, rays_d, depth, n_samples):
    """the reference's samples along every ray with depth > 0: [R_valid * n_samples, 3] float64"""
    keep = np.asarray(depth) > 0
    o, dr, dep = (np.asarray(x, np.float64)[keep] for x in (rays_o, rays_d, depth))
    t = np.linspace(0.0, 1.0, n_samples)
    z = (0.8 * dep)[:, None] * (1 - t) + (dep + 0.5)[:, None] * t
    return (o[:, None, :] + dr[:, None, :] * z[..., None]).reshape(-1, 3)


def overlap_ref(rays_o, rays_d, depth, c2ws, fx, fy, cx, cy, H, W, n_samples=8, edge=OVERLAP_EDGE):
    pts = sample_points(rays_o, rays_d, depth, n_samples)
    inside = []
    for c2w in c2ws:
        u, v, z = project(c2w, pts, fx, fy, cx, cy)
        inside.append(int(((u < W - edge) & (u > edge) & (v < H - edge) & (v > edge) & (z < 0)).sum()))
    return np.array(inside, np.int64), len(pts)
