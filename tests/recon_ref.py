"""Numpy restatement of the mesh evaluation of glorie_slam_amd/eval_recon.py (csrc/recon.hip): area-weighted sampling, the
ICP moments and loop, the nearest-neighbour statistics, the depth rasteriser, check_proj and depth L1, plus the meshes and
scenes of the tests.  float64 unless a dtype is given (the float32 compositions are the yardsticks of the GPU tests).

Conventions (the contract of the kernels):
  mesh      vertices [V,3], faces [F,3]; both sides of a triangle are drawn
  camera    OpenCV pinhole, K = (fx, fy, cx, cy), w2c the world-to-camera matrix; pixel (u, v) is centred on (u, v)
  depth     camera-frame z, 0 where nothing is hit

The rasteriser here is written differently from the kernel on purpose: every triangle is clipped against z = z_near into
one or two triangles, those are projected, a pixel is inside when its signed distance (in pixels) to all three projected
edges is >= -eps, and the depth comes from the plane of the unclipped triangle.  eps > 0 grows every triangle in the image
plane, eps < 0 shrinks it: a pixel whose grown and shrunk depths agree does not hang on the rounding of an edge test.
"""
import numpy as np

import tsdf_ref

EPS_PIXEL = 1e-4


# ---- meshes ----------------------------------------------------------------------------------------------------------
def uv_sphere(radius=0.3, stacks=11, slices=24, centre=(0.0, 0.0, 0.0)):
    """2 slices (stacks - 1) triangles (480 by default), outward normals"""
    v = [(0.0, 0.0, 1.0)]
    for i in range(1, stacks):
        th = np.pi * i / stacks
        for j in range(slices):
            ph = 2.0 * np.pi * j / slices
            v.append((np.sin(th) * np.cos(ph), np.sin(th) * np.sin(ph), np.cos(th)))
    v.append((0.0, 0.0, -1.0))
    ring = lambda i, j: 1 + (i - 1) * slices + j % slices
    f = []
    for j in range(slices):
        f.append((0, ring(1, j), ring(1, j + 1)))
        f.append((len(v) - 1, ring(stacks - 1, j + 1), ring(stacks - 1, j)))
    for i in range(1, stacks - 1):
        for j in range(slices):
            f.append((ring(i, j), ring(i + 1, j), ring(i + 1, j + 1)))
            f.append((ring(i, j), ring(i + 1, j + 1), ring(i, j + 1)))
    return (np.asarray(v) * radius + np.asarray(centre)).astype(np.float32), np.asarray(f, np.int32)


def box_room(lo=(-1.0, -1.5, -0.8), hi=(1.2, 1.4, 0.9)):
    """the 12 triangles of an axis-aligned box"""
    lo, hi = np.asarray(lo, np.float64), np.asarray(hi, np.float64)
    v = np.array([[(lo, hi)[(c >> a) & 1][a] for a in range(3)] for c in range(8)])
    quads = [(0, 2, 6, 4), (1, 5, 7, 3), (0, 4, 5, 1), (2, 3, 7, 6), (0, 1, 3, 2), (4, 6, 7, 5)]
    f = [t for a, b, c, d in quads for t in ((a, b, c), (a, c, d))]
    return v.astype(np.float32), np.asarray(f, np.int32)


def grid_mesh(n=64, side=0.5, bump=0.03):
    """n x n cells of two triangles over [-side/2, side/2]^2 in the plane z = bump sin(9 x) cos(7 y)"""
    c = np.linspace(-side / 2, side / 2, n + 1)
    y, x = np.meshgrid(c, c, indexing="ij")
    v = np.stack([x, y, bump * np.sin(9.0 * x) * np.cos(7.0 * y)], -1).reshape(-1, 3)
    i, j = np.meshgrid(np.arange(n), np.arange(n), indexing="ij")
    a = (i * (n + 1) + j).reshape(-1)
    f = np.concatenate([np.stack([a, a + 1, a + n + 2], 1), np.stack([a, a + n + 2, a + n + 1], 1)])
    return v.astype(np.float32), f.astype(np.int32)


def rotation(axis, degrees):
    axis = np.asarray(axis, np.float64) / np.linalg.norm(axis)
    a = np.deg2rad(degrees)
    k = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    return np.eye(3) + np.sin(a) * k + (1 - np.cos(a)) * (k @ k)


def rigid(axis, degrees, t):
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = rotation(axis, degrees), t
    return T


# ---- sampling ----------------------------------------------------------------------------------------------------------
def face_areas(vertices, faces):
    p = np.asarray(vertices, np.float64)[np.asarray(faces)]
    return 0.5 * np.linalg.norm(np.cross(p[:, 1] - p[:, 0], p[:, 2] - p[:, 0]), axis=1)


def area_cdf(vertices, faces):
    return np.cumsum(face_areas(vertices, faces))


def select_faces(cdf, u0):
    """the first face with cdf > u0 * total, and whether u0 * total lies within 1e-12 (relative to the total) of an entry"""
    x = np.asarray(u0, np.float64) * cdf[-1]
    face = np.minimum(np.searchsorted(cdf, x, side="right"), len(cdf) - 1)
    near = np.zeros(len(x), bool)
    for k in (-1, 0):
        near |= np.abs(cdf[np.clip(face + k, 0, len(cdf) - 1)] - x) <= 1e-12 * cdf[-1]
    return face, near


def barycentric_points(vertices, faces, face_of, u, dtype=np.float64):
    """p0 + a (p1 - p0) + b (p2 - p0) on the given faces, every operation in dtype"""
    T = dtype
    p = np.asarray(vertices, T)[np.asarray(faces)[face_of]]
    a, b = np.asarray(u[:, 1], T), np.asarray(u[:, 2], T)
    flip = a + b > T(1)
    a, b = np.where(flip, T(1) - a, a), np.where(flip, T(1) - b, b)
    return p[:, 0] + a[:, None] * (p[:, 1] - p[:, 0]) + b[:, None] * (p[:, 2] - p[:, 0])


def sample_surface(vertices, faces, u):
    """-> (points float64 [n,3], face_of, borderline)"""
    face, near = select_faces(area_cdf(vertices, faces), u[:, 0])
    return barycentric_points(vertices, faces, face, u), face, near


# ---- nearest neighbours --------------------------------------------------------------------------------------------------
def nn_bruteforce(queries, points, chunk=1024):
    """float64 -> (distance, index); ties to the lower index"""
    q, p = np.asarray(queries, np.float64), np.asarray(points, np.float64)
    d, i = np.empty(len(q)), np.empty(len(q), np.int64)
    for s in range(0, len(q), chunk):
        d2 = ((q[s:s + chunk, None, :] - p[None]) ** 2).sum(-1)
        i[s:s + chunk] = d2.argmin(1)
        d[s:s + chunk] = np.sqrt(d2[np.arange(d2.shape[0]), i[s:s + chunk]])
    return d, i


def nn_kdtree(queries, points):
    from scipy.spatial import cKDTree
    d, i = cKDTree(np.asarray(points, np.float64)).query(np.asarray(queries, np.float64))
    return d, i.astype(np.int64)


def accuracy(gt_pts, rec_pts):
    return float(nn_kdtree(rec_pts, gt_pts)[0].mean())


def completion(gt_pts, rec_pts):
    return float(nn_kdtree(gt_pts, rec_pts)[0].mean())


def completion_ratio(gt_pts, rec_pts, dist_th=0.05):
    return float((nn_kdtree(gt_pts, rec_pts)[0] < dist_th).mean())


def nn_stats(D, threshold):
    """-> ({sum sqrt(D), #(sqrt(D) < threshold), sum D}, the sums of the absolute terms) with D the fp32 squared distances"""
    d2 = np.asarray(D, np.float32).astype(np.float64)
    d = np.sqrt(d2)
    out = np.array([d.sum(), float((d < float(np.float32(threshold))).sum()), d2.sum()])
    return out, np.array([d.sum(), 0.0, d2.sum()])


# ---- ICP ---------------------------------------------------------------------------------------------------------------
def transform_points(T, p):
    p = np.asarray(p, np.float64)
    return p @ np.asarray(T, np.float64)[:3, :3].T + np.asarray(T, np.float64)[:3, 3]


def icp_moments(src, tgt, I, D, max_d2):
    """-> (the 17 sums, the sums of the absolute values of their terms)"""
    src, tgt = np.asarray(src, np.float64), np.asarray(tgt, np.float64)
    I = np.asarray(I)
    keep = (I >= 0) & (I < len(tgt)) & (np.asarray(D, np.float32) < np.float32(max_d2))
    p, q = src[keep], tgt[I[keep]]
    terms = np.concatenate([np.ones((len(p), 1)), p, q, (p[:, :, None] * q[:, None, :]).reshape(-1, 9),
                            ((p - q) ** 2).sum(1, keepdims=True)], 1)
    return terms.sum(0), np.abs(terms).sum(0)


def kabsch_from_moments(mom):
    n = mom[0]
    mp, mq = mom[1:4] / n, mom[4:7] / n
    cov = mom[7:16].reshape(3, 3) / n - np.outer(mp, mq)
    u, _, vt = np.linalg.svd(cov)
    sgn = np.eye(3)
    if np.linalg.det(u) * np.linalg.det(vt) < 0:
        sgn[2, 2] = -1.0
    T = np.eye(4)
    T[:3, :3] = vt.T @ sgn @ u.T
    T[:3, 3] = mq - T[:3, :3] @ mp
    return T


def icp(src, tgt, threshold=0.1, init=None, max_iteration=30, relative_fitness=1e-6, relative_rmse=1e-6, round_f32=False):
    """point-to-point ICP as eval_recon.icp_align states it; round_f32: the transformed points are rounded to float32 (what
    the kernels hand to the neighbour search) -> (T, {"fitness", "inlier_rmse", "iterations"})"""
    from scipy.spatial import cKDTree
    src, tgt = np.asarray(src, np.float32).astype(np.float64), np.asarray(tgt, np.float32).astype(np.float64)
    tree = cKDTree(tgt)
    T = np.eye(4) if init is None else np.array(init, np.float64)

    def score(T):
        cur = transform_points(T, src)
        if round_f32:
            cur = cur.astype(np.float32).astype(np.float64)
        d, i = tree.query(cur)
        mom, _ = icp_moments(cur, tgt, i, d * d, threshold * threshold)
        n = mom[0]
        return mom, n / len(src), (np.sqrt(mom[16] / n) if n > 0 else 0.0)

    mom, fitness, rmse = score(T)
    iterations = 0
    for _ in range(max_iteration):
        if mom[0] < 3:
            break
        T = kabsch_from_moments(mom) @ T
        iterations += 1
        before = (fitness, rmse)
        mom, fitness, rmse = score(T)
        if abs(before[0] - fitness) < relative_fitness and abs(before[1] - rmse) < relative_rmse:
            break
    return T, {"fitness": float(fitness), "inlier_rmse": float(rmse), "iterations": iterations}


# ---- rasteriser ----------------------------------------------------------------------------------------------------------
def _clip_near(tri, z_near):
    """Sutherland-Hodgman against z >= z_near -> a list of triangles (a fan of the clipped polygon)"""
    out = []
    for k in range(3):
        a, b = tri[k], tri[(k + 1) % 3]
        fa, fb = a[2] > z_near, b[2] > z_near
        if fa:
            out.append(a)
        if fa != fb:
            s = (z_near - a[2]) / (b[2] - a[2])
            p = a + s * (b - a)
            p[2] = z_near
            out.append(p)
    return [np.stack([out[0], out[k], out[k + 1]]) for k in range(1, len(out) - 1)]


def rasterise(vertices, faces, w2c, K, H, W, z_near=0.01, z_far=20.0, eps=0.0, dtype=np.float64):
    """-> depth [H,W] in dtype, +inf where nothing is hit (see the module text)"""
    T = dtype
    fx, fy, cx, cy = (T(k) for k in K)
    w2c = np.asarray(w2c, T)
    cam = np.asarray(vertices, T) @ w2c[:3, :3].T + w2c[:3, 3]
    zn, zf, eps = T(z_near), T(z_far), T(eps)
    depth = np.full((H, W), np.inf, T)
    for face in np.asarray(faces):
        tri = cam[face]
        if (tri[:, 2] <= zn).all() or (tri[:, 2] > zf).all():
            continue
        normal = np.cross(tri[1] - tri[0], tri[2] - tri[0])
        offset = normal @ tri[0]
        for part in _clip_near(tri, zn):
            u = fx * part[:, 0] / part[:, 2] + cx
            v = fy * part[:, 1] / part[:, 2] + cy
            x0, x1 = int(max(np.floor(u.min() - 1), 0)), int(min(np.ceil(u.max() + 1), W - 1))
            y0, y1 = int(max(np.floor(v.min() - 1), 0)), int(min(np.ceil(v.max() + 1), H - 1))
            if x1 < x0 or y1 < y0:
                continue
            area = (u[1] - u[0]) * (v[2] - v[0]) - (v[1] - v[0]) * (u[2] - u[0])
            if area == 0:
                continue
            sign = T(1) if area > 0 else T(-1)
            py, px = np.meshgrid(np.arange(y0, y1 + 1, dtype=T), np.arange(x0, x1 + 1, dtype=T), indexing="ij")
            inside = np.ones(px.shape, bool)
            for k in range(3):
                ax, ay, bx, by = u[k], v[k], u[(k + 1) % 3], v[(k + 1) % 3]
                length = np.sqrt((bx - ax) ** 2 + (by - ay) ** 2)
                if length == 0:
                    inside[:] = False
                    break
                inside &= sign * ((bx - ax) * (py - ay) - (by - ay) * (px - ax)) >= -eps * length
            with np.errstate(divide="ignore", invalid="ignore"):
                z = offset / (normal[0] * ((px - cx) / fx) + normal[1] * ((py - cy) / fy) + normal[2])
            inside &= (z > zn) & (z <= zf)
            window = depth[y0:y1 + 1, x0:x1 + 1]
            window[inside] = np.minimum(window[inside], z[inside])
    return depth


def firm_depth(vertices, faces, w2c, K, H, W, z_near=0.01, z_far=20.0):
    """-> (grown, shrunk, exact, firm): the depths at eps = +-EPS_PIXEL and 0 (+inf = uncovered) and the pixels where grown
    and shrunk agree"""
    grown = rasterise(vertices, faces, w2c, K, H, W, z_near, z_far, EPS_PIXEL)
    shrunk = rasterise(vertices, faces, w2c, K, H, W, z_near, z_far, -EPS_PIXEL)
    exact = rasterise(vertices, faces, w2c, K, H, W, z_near, z_far, 0.0)
    return grown, shrunk, exact, grown == shrunk


def points_in_view(points, w2c, K, H, W, edge):
    fx, fy, cx, cy = K
    w2c = np.asarray(w2c, np.float64)
    p = np.asarray(points, np.float64) @ w2c[:3, :3].T + w2c[:3, 3]
    front = p[:, 2] > 0
    z = np.where(front, p[:, 2], 1.0)
    u, v = fx * p[:, 0] / z + cx, fy * p[:, 1] / z + cy
    return int((front & (u > edge) & (u < W - edge) & (v > edge) & (v < H - edge)).sum())


def depth_l1(gt_depth, rec_depth):
    """-> (mean |gt - rec| over rec > 0, the number of such pixels); depths with 0 where nothing is hit"""
    gt, rec = np.asarray(gt_depth, np.float64), np.asarray(rec_depth, np.float64)
    m = rec > 0
    return (float(np.abs(gt[m] - rec[m]).mean()) if m.any() else 0.0), int(m.sum())


def to_zero(depth):
    """+inf (uncovered) -> 0, the convention of the kernels' output"""
    return np.where(np.isfinite(depth), depth, 0.0)


# ---- the scenes of the rasteriser tests: a ragged 37 x 53 frame ------------------------------------------------------------
RASTER_H, RASTER_W = 37, 53
RASTER_K = tuple(float(np.float32(k)) for k in (41.3, 40.7, 25.8, 17.6))
RASTER_NEAR, RASTER_FAR = 0.01, 20.0


def _w2c32(c2w):
    """the fp32 world-to-camera matrix the kernels take, as float64"""
    return np.linalg.inv(c2w).astype(np.float32).astype(np.float64)


def raster_scenes():
    """[(name, vertices f32, faces i32, w2c float64 with fp32 values, expected: "some" or "none")]"""
    look = tsdf_ref.look_at
    scenes = []
    tri_v = np.array([[-0.41, -0.23, 0.07], [0.52, -0.31, -0.12], [0.13, 0.47, 0.21]], np.float32)
    one = np.array([[0, 1, 2]], np.int32)
    scenes.append(("triangle", tri_v, one, _w2c32(look((0.31, -0.52, 1.13), (0.05, 0.02, 0.0))), "some"))
    # a wall of two triangles through the camera plane: the plane y = 0.4 (below the camera) from 3 behind to 3 in front
    wall_v = np.array([[-3.0, 0.4, -3.0], [3.0, 0.4, -3.0], [3.0, 0.4, 3.0], [-3.0, 0.4, 3.0]], np.float32)
    wall_f = np.array([[0, 1, 2], [0, 2, 3]], np.int32)
    for name, axis, deg in (("wall level", (1.0, 0.2, 0.1), 3.0), ("wall pitched", (1.0, -0.3, 0.2), -24.0),
                            ("wall rolled", (0.3, 1.0, 0.8), 37.0)):
        c2w = rigid(axis, deg, (0.11, -0.07, 0.05))
        scenes.append((name, wall_v, wall_f, _w2c32(c2w), "some"))
    sv, sf = uv_sphere()
    scenes.append(("sphere outside", sv, sf, _w2c32(look((0.62, 0.35, 0.28), (0.01, -0.02, 0.015))), "some"))
    scenes.append(("sphere centre", sv, sf, _w2c32(look((0.02, -0.03, 0.01), (0.7, 0.4, -0.5))), "some"))
    gv, gf = grid_mesh()
    scenes.append(("grid", gv, gf, _w2c32(look((0.13, -0.21, 1.02), (0.01, 0.0, 0.0))), "some"))
    gone_v = np.array([[-0.3, -0.2, -1.0], [0.4, -0.1, -2.0], [0.0, 0.5, -0.5],          # behind the camera
                       [5.0, 0.1, 1.0], [6.0, 0.3, 1.2], [5.5, 1.0, 0.9],                 # off screen
                       [-1.0, -1.0, 25.0], [1.0, -1.0, 24.0], [0.0, 1.0, 26.0]], np.float32)  # beyond z_far
    gone_f = np.array([[0, 1, 2], [3, 4, 5], [6, 7, 8]], np.int32)
    scenes.append(("nothing", gone_v, gone_f, _w2c32(np.eye(4)), "none"))
    return scenes


# ---- the sampling mesh and the draws of the GPU test -------------------------------------------------------------------------------------
def sampling_mesh():
    """the 12-triangle box, one face without area (index 12) and two faces whose areas differ by 1e6"""
    v, f = box_room()
    extra_v = np.array([[2.0, 0.0, 0.0], [2.5, 0.0, 0.0], [3.0, 0.0, 0.0],               # collinear: no area
                        [4.0, 0.0, 0.0], [4.001, 0.0, 0.0], [4.0, 0.001, 0.0],            # area 5e-7
                        [5.0, 0.0, 0.0], [6.0, 0.0, 0.0], [5.0, 1.0, 0.0]], np.float32)  # area 0.5
    extra_f = np.arange(9, dtype=np.int32).reshape(3, 3) + len(v)
    return np.concatenate([v, extra_v]), np.concatenate([f, extra_f])


SAMPLE_SIZES = (1, 255, 4099)
SAMPLE_SEED = 1234


def uniforms(n, seed=SAMPLE_SEED):
    """float32 [n,3] in [0,1) from a seeded torch generator on the host"""
    import torch
    return torch.rand(n, 3, generator=torch.Generator().manual_seed(seed)).numpy()
