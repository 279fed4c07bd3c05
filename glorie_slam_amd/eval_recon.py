"""Mesh evaluation on HIP kernels (csrc/recon.hip; reference: src/utils/eval_recon.py): accuracy, completion, completion
ratio and depth L1 of a reconstructed mesh against the ground-truth mesh.

  sample_surface     area-weighted surface samples (trimesh.sample.sample_surface, :107-110)
  nn_distances       squared distances of an exact 1-NN (the cell list of point_ops.KnnIndex with k = 1)
  accuracy, completion, completion_ratio     :25-43, on sample points
  icp_align          point-to-point ICP on the mesh vertices (get_align_transformation, :46-60)
  calc_3d_metric     :95-119, plus precision / recall / f-score at dist_th
  render_depth       the depth map of a mesh from a pinhole camera (the rasteriser that stands in for :166-217)
  sample_views       random cameras inside the ground truth's bound (:121-138, :171-187)
  calc_2d_metric     :141-227 depth L1 over random views
  eval_recon         :229-248; writes metrics_recon.txt; cull= cuts both meshes to given views first (cull_mesh.py)

Device tensors throughout; numpy float64 on the host only for 3x3 and 4x4 algebra.  Cameras are OpenCV pinholes whose
pixel (u, v) samples image coordinates (u, v) (tsdf.py), which is why cx = W / 2 - 0.5.

Not pinned: parity with trimesh (its RNG draws other samples), with Open3D (its ICP uses a KD-tree and applies the steps
to the points incrementally in fp64; its rasteriser is OpenGL's) and with the evaluate_3d_reconstruction package the
reference takes precision, recall and f-score from (:236) - none of them is part of this project.  Deviation: the cameras
of sample_views are placed in the axis-aligned box of the ground-truth vertices where the reference uses trimesh's
oriented bounding box.
"""
import ctypes
import os

import numpy as np
import torch

from . import _lib as L
from .point_ops import KnnIndex


# ---- arguments ---------------------------------------------------------------------------------------------------------
def _points(p, what="points"):
    if not torch.is_tensor(p):
        raise ValueError(f"{what} must be a device tensor, got {type(p).__name__}")
    L.need_cuda(p)
    if not p.dtype.is_floating_point:
        raise ValueError(f"{what} must be a floating-point tensor, got {p.dtype}")
    if p.dim() != 2 or p.shape[1] != 3:
        raise ValueError(f"{what} must be [n,3], got {tuple(p.shape)}")
    return L.f32(p.detach())


def _mesh(vertices, faces):
    """-> (vertices f32 [V,3], faces int32 [F,3]) contiguous on the device; no empty mesh"""
    vertices = _points(vertices, "vertices")
    if not torch.is_tensor(faces):
        raise ValueError(f"faces must be a device tensor, got {type(faces).__name__}")
    L.need_cuda(faces)
    if faces.dtype not in (torch.int32, torch.int64):
        raise ValueError(f"faces must be int32 or int64, got {faces.dtype}")
    if faces.dim() != 2 or faces.shape[1] != 3:
        raise ValueError(f"faces must be [F,3], got {tuple(faces.shape)}")
    if vertices.shape[0] == 0 or faces.shape[0] == 0:
        raise ValueError("the mesh is empty")
    if faces.device != vertices.device:
        raise ValueError("vertices and faces live on different devices")
    return vertices, faces.detach().to(torch.int32).contiguous()


def _intrinsics(K):
    """(fx, fy, cx, cy) or a 3x3 matrix -> four numbers rounded to fp32, what the kernels take"""
    K = np.asarray(K.detach().cpu() if torch.is_tensor(K) else K, np.float64)
    if K.shape == (3, 3):
        K = np.array([K[0, 0], K[1, 1], K[0, 2], K[1, 2]])
    if K.shape != (4,):
        raise ValueError(f"intrinsics must be (fx, fy, cx, cy) or a 3x3 matrix, got shape {K.shape}")
    return tuple(float(np.float32(v)) for v in K)


def _matrix(T, what="transform"):
    T = np.asarray(T.detach().cpu() if torch.is_tensor(T) else T, np.float64)
    if T.shape != (4, 4):
        raise ValueError(f"{what} must be 4x4, got {T.shape}")
    return np.ascontiguousarray(T)


def _w2c(c2w, device):
    return torch.from_numpy(np.linalg.inv(_matrix(c2w, "c2w"))).to(device, torch.float32).contiguous()


# ---- kernels -------------------------------------------------------------------------------------------------------------
def area_cdf(vertices, faces):
    """-> (cdf f64 [F], the total area); a face index outside [0, V) raises GlorieError (GLORIE_EINVAL)"""
    vertices, faces = _mesh(vertices, faces)
    lib, dev = L.load(), vertices.device
    F = faces.shape[0]
    cdf = torch.empty(F, dtype=torch.float64, device=dev)
    ws = L.workspace(lib.glorie_mesh_area_cdf_workspace(F), dev)
    total = ctypes.c_double(0.0)
    with torch.cuda.device(dev):
        L.check(lib.glorie_mesh_area_cdf(L.ptr(vertices), vertices.shape[0], L.ptr(faces), F, L.ptr(cdf), L.ptr(ws),
                                         ctypes.byref(total), L.stream_ptr(dev)), "glorie_mesh_area_cdf")
    return cdf, float(total.value)


def sample_surface(vertices, faces, n, generator=None, u=None):
    """n points on the surface, faces drawn by area -> (points f32 [n,3], face_of int32 [n]).  The uniforms u f32 [n,3]
    come from `generator` (a torch.Generator; seed 0 on the mesh's device when None) unless given"""
    vertices, faces = _mesh(vertices, faces)
    dev = vertices.device
    cdf, total = area_cdf(vertices, faces)
    if not total > 0.0:
        raise L.GlorieError("glorie_mesh_sample failed: GLORIE_EINVAL (the mesh has no area)")
    if u is None:
        if generator is None:
            generator = torch.Generator(device=dev).manual_seed(0)
        u = torch.rand(int(n), 3, generator=generator, device=generator.device, dtype=torch.float32).to(dev)
    u = L.f32(u.to(dev))
    if tuple(u.shape) != (int(n), 3):
        raise ValueError(f"u must be [{int(n)},3], got {tuple(u.shape)}")
    points = torch.empty(int(n), 3, dtype=torch.float32, device=dev)
    face_of = torch.empty(int(n), dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        L.check(L.load().glorie_mesh_sample(L.ptr(vertices), vertices.shape[0], L.ptr(faces), faces.shape[0], L.ptr(cdf),
                                            L.ptr(u), int(n), L.ptr(points), L.ptr(face_of), L.stream_ptr(dev)),
                "glorie_mesh_sample")
    return points, face_of


def transform_points(T, points):
    """R p + t for T = [R t; 0 1] (4x4, host float64): fp64 arithmetic, one rounding -> f32 [n,3]"""
    points = _points(points)
    T = _matrix(T)
    out = torch.empty_like(points)
    with torch.cuda.device(points.device):
        L.check(L.load().glorie_transform_points(T.ctypes.data_as(ctypes.c_void_p), L.ptr(points), points.shape[0],
                                                 L.ptr(out), L.stream_ptr(points.device)), "glorie_transform_points")
    return out


def _index(points):
    """the cell list over `points`: cells of about twice the spacing of n points spread over a surface of the cloud's size"""
    points = _points(points)
    if points.shape[0] == 0:
        raise ValueError("the point set is empty")
    extent = float((points.max(0).values - points.min(0).values).max())
    cell = max(2.0 * extent / max(points.shape[0], 1) ** 0.5, 1e-6)
    index = KnnIndex(points.device, cell_size=cell)
    index.set_points(points)
    return index


def _search(index, queries):
    D, I, _ = index.search(_points(queries, "queries"), k=1, radius=0.0)
    return D.view(-1), I.view(-1)


def nn_distances(queries, points, return_index=False):
    """the squared distance from every query to its nearest point, exact (fp32, ((dx dx + dy dy) + dz dz); ties to the
    lower index) -> f32 [Q] (, the index of that point int64 [Q])"""
    D, I = _search(_index(points), queries)
    return (D, I) if return_index else D


def nn_stats(D, threshold):
    """D f32 [Q] squared distances -> float64 [3] = (sum of distances, #(distance < threshold), sum of D) (one read-back)"""
    L.need_cuda(D)
    D = L.f32(D.detach()).view(-1)
    lib, dev = L.load(), D.device
    out = torch.empty(3, dtype=torch.float64, device=dev)
    ws = L.workspace(lib.glorie_nn_stats_workspace(D.numel()), dev)
    with torch.cuda.device(dev):
        L.check(lib.glorie_nn_stats(L.ptr(D), D.numel(), float(threshold), L.ptr(ws), L.ptr(out), L.stream_ptr(dev)),
                "glorie_nn_stats")
    return out.cpu().numpy()


def icp_moments(src, tgt, I, D, max_d2, out=None):
    """the 17 sums of glorie_icp_moments over the correspondences (src[i], tgt[I[i]]) with I >= 0 and D < max_d2 -> f64
    [17] on the device"""
    src, tgt = _points(src, "src"), _points(tgt, "tgt")
    L.need_cuda(I, D)
    if I.dtype != torch.int64 or I.numel() != src.shape[0] or D.numel() != src.shape[0]:
        raise ValueError("I must be int64 [n] and D [n] for src [n,3]")
    I, D = I.contiguous().view(-1), L.f32(D).view(-1)
    lib, dev = L.load(), src.device
    out = torch.empty(17, dtype=torch.float64, device=dev) if out is None else out
    ws = L.workspace(lib.glorie_icp_moments_workspace(src.shape[0]), dev)
    with torch.cuda.device(dev):
        L.check(lib.glorie_icp_moments(L.ptr(src), src.shape[0], L.ptr(tgt), tgt.shape[0], L.ptr(I), L.ptr(D),
                                       float(np.float32(max_d2)), L.ptr(ws), L.ptr(out), L.stream_ptr(dev)),
                "glorie_icp_moments")
    return out


# ---- eval_recon.py:25-43 ---------------------------------------------------------------------------------------------------
def accuracy(gt_pts, rec_pts):
    """mean distance from the reconstruction's points to the ground truth's"""
    D = nn_distances(rec_pts, gt_pts)
    return float(nn_stats(D, 0.0)[0] / D.numel())


def completion(gt_pts, rec_pts):
    """mean distance from the ground truth's points to the reconstruction's"""
    D = nn_distances(gt_pts, rec_pts)
    return float(nn_stats(D, 0.0)[0] / D.numel())


def completion_ratio(gt_pts, rec_pts, dist_th=0.05):
    """share of the ground truth's points with a point of the reconstruction closer than dist_th"""
    D = nn_distances(gt_pts, rec_pts)
    return float(nn_stats(D, dist_th)[1] / D.numel())


# ---- ICP -------------------------------------------------------------------------------------------------------------------
def kabsch_from_moments(mom):
    """the rigid 4x4 that minimises sum |R p + t - q|^2, from {n, sum p, sum q, sum p q^T, ..} (float64, host)"""
    n = mom[0]
    mp, mq = mom[1:4] / n, mom[4:7] / n
    cov = mom[7:16].reshape(3, 3) / n - np.outer(mp, mq)            # sum (p - mp)(q - mq)^T / n
    u, _, vt = np.linalg.svd(cov)
    sgn = np.eye(3)
    if np.linalg.det(u) * np.linalg.det(vt) < 0:
        sgn[2, 2] = -1.0
    T = np.eye(4)
    T[:3, :3] = vt.T @ sgn @ u.T
    T[:3, 3] = mq - T[:3, :3] @ mp
    return T


def icp_align(src_vertices, tgt_vertices, threshold=0.1, init=None, max_iteration=30, relative_fitness=1e-6,
              relative_rmse=1e-6):
    """Point-to-point ICP of the source points onto the target points, no scale -> (T float64 [4,4], {"fitness": share of
    the source with a target point closer than `threshold`, "inlier_rmse", "iterations": steps applied}).  Every
    iteration transforms the source with the accumulated T (fp64, one rounding), takes the exact 1-NN, sums the 17
    moments on the device (one 136-byte read-back) and left-multiplies the Kabsch step; it stops on Open3D's default
    criteria: both the fitness and the inlier rmse change by less than the relative_* numbers, or max_iteration.  Fewer
    than 3 correspondences return the current transform"""
    src, tgt = _points(src_vertices, "src_vertices"), _points(tgt_vertices, "tgt_vertices")
    if src.shape[0] == 0 or tgt.shape[0] == 0:
        raise ValueError("icp_align needs points on both sides")
    index = _index(tgt)
    T = np.eye(4) if init is None else _matrix(init, "init").copy()
    max_d2 = float(threshold) ** 2
    mom_dev = torch.empty(17, dtype=torch.float64, device=src.device)

    def score(T):
        cur = transform_points(T, src)
        D, I = _search(index, cur)
        mom = icp_moments(cur, tgt, I, D, max_d2, out=mom_dev).cpu().numpy()
        n = mom[0]
        return mom, float(n / src.shape[0]), float(np.sqrt(mom[16] / n)) if n > 0 else 0.0

    mom, fitness, rmse = score(T)
    iterations = 0
    for _ in range(int(max_iteration)):
        if mom[0] < 3:
            break
        T = kabsch_from_moments(mom) @ T
        iterations += 1
        before = (fitness, rmse)
        mom, fitness, rmse = score(T)
        if abs(before[0] - fitness) < relative_fitness and abs(before[1] - rmse) < relative_rmse:
            break
    return T, {"fitness": fitness, "inlier_rmse": rmse, "iterations": iterations}


def _aligned(rec_vertices, gt_vertices, align):
    """align: False, True (ICP of the vertices) or a 4x4 -> (the reconstruction's vertices in the ground truth's frame, T)"""
    if align is False or align is None:
        return rec_vertices, np.eye(4)
    T = icp_align(rec_vertices, gt_vertices)[0] if align is True else _matrix(align, "align")
    return transform_points(T, rec_vertices), T


# ---- eval_recon.py:95-119 --------------------------------------------------------------------------------------------------
def calc_3d_metric(rec, gt, align=True, n_samples=200000, dist_th=0.05, generator=None, return_samples=False):
    """rec, gt: (vertices, faces) on the device -> {"accuracy" cm, "completion" cm, "completion_ratio" %, "precision" %,
    "recall" %, "f-score" %} from n_samples surface samples of each mesh (the reconstruction's first, from one generator).
    precision = share of the reconstruction's samples closer than dist_th to the ground truth's, recall = the reverse
    (= completion_ratio), f-score their harmonic mean: the usual definitions, parity with evaluate_3d_reconstruction,
    trimesh and Open3D is not pinned (see the module text).  align: True (icp_align on the vertices), False or a 4x4"""
    rec_v, rec_f = _mesh(*rec)
    gt_v, gt_f = _mesh(*gt)
    if generator is None:
        generator = torch.Generator(device=rec_v.device).manual_seed(0)
    # a rigid motion keeps areas and barycentric coordinates: the samples are drawn on the mesh as it came and moved
    # afterwards, so that the draw does not hang on the last bits of the alignment
    rec_pts, _ = sample_surface(rec_v, rec_f, n_samples, generator)
    if align is not False and align is not None:
        T = icp_align(rec_v, gt_v)[0] if align is True else _matrix(align, "align")
        rec_pts = transform_points(T, rec_pts)
    gt_pts, _ = sample_surface(gt_v, gt_f, n_samples, generator)
    to_gt = nn_stats(nn_distances(rec_pts, gt_pts), dist_th)
    to_rec = nn_stats(nn_distances(gt_pts, rec_pts), dist_th)
    n = float(n_samples)
    precision, recall = to_gt[1] / n, to_rec[1] / n
    out = {"accuracy": float(to_gt[0] / n * 100.0), "completion": float(to_rec[0] / n * 100.0),
           "completion_ratio": float(recall * 100.0), "precision": float(precision * 100.0),
           "recall": float(recall * 100.0),
           "f-score": float(200.0 * precision * recall / (precision + recall)) if precision + recall > 0 else 0.0}
    return (out, rec_pts, gt_pts) if return_samples else out


# ---- depth L1 ----------------------------------------------------------------------------------------------------------------
class _Rasteriser:
    """the buffers of render_depth for one mesh and one image size"""

    def __init__(self, vertices, faces, K, H, W, z_near, z_far):
        self.vertices, self.faces = _mesh(vertices, faces)
        self.K, self.H, self.W = _intrinsics(K), int(H), int(W)
        self.z_near, self.z_far = float(z_near), float(z_far)
        dev = self.vertices.device
        self.bits = torch.empty(self.H, self.W, dtype=torch.int32, device=dev)
        self.ws = L.workspace(L.load().glorie_mesh_depth_workspace(self.faces.shape[0]), dev)

    def render(self, w2c, policy=0, out=None):
        dev = self.vertices.device
        depth = torch.empty(self.H, self.W, dtype=torch.float32, device=dev) if out is None else out
        with torch.cuda.device(dev):
            L.check(L.load().glorie_mesh_depth(L.ptr(self.vertices), self.vertices.shape[0], L.ptr(self.faces),
                                               self.faces.shape[0], L.ptr(w2c), *self.K, self.H, self.W, self.z_near,
                                               self.z_far, int(policy), L.ptr(self.ws), L.ptr(self.bits), L.ptr(depth),
                                               L.stream_ptr(dev)), "glorie_mesh_depth")
        return depth


def _camera(c2w, w2c, device):
    if w2c is None:
        return _w2c(c2w, device)
    w2c = L.f32(torch.as_tensor(w2c).to(device))
    if tuple(w2c.shape) != (4, 4):
        raise ValueError(f"w2c must be 4x4, got {tuple(w2c.shape)}")
    return w2c


def render_depth(vertices, faces, c2w, K, H, W, z_near=0.01, z_far=20.0, policy=0, w2c=None):
    """The depth map f32 [H,W] of the mesh from the OpenCV camera c2w (4x4, host or device) with intrinsics K = (fx, fy, cx,
    cy) or 3x3: the smallest camera-frame z in (z_near, z_far] along every pixel's ray, both sides of every triangle, 0
    where there is none; triangles that cross the near plane keep their part in front of it (include/glorie_hip.h).
    w2c: the world-to-camera matrix as the kernel takes it (fp32), instead of c2w.  policy: 0 auto, 1 every triangle by
    one lane, 2 every triangle by workgroups - the same bits"""
    r = _Rasteriser(vertices, faces, K, H, W, z_near, z_far)
    return r.render(_camera(c2w, w2c, r.vertices.device), policy)


def points_in_view(points, c2w, K, H, W, edge=10.0, w2c=None):
    """check_proj (:63-92): how many points project with z > 0, edge < u < W - edge, edge < v < H - edge (one read-back)"""
    points = _points(points)
    dev = points.device
    count = torch.empty(1, dtype=torch.int32, device=dev)
    cam = _camera(c2w, w2c, dev)
    with torch.cuda.device(dev):
        L.check(L.load().glorie_points_in_view(L.ptr(points), points.shape[0], L.ptr(cam), *_intrinsics(K),
                                               int(H), int(W), float(edge), L.ptr(count), L.stream_ptr(dev)),
                "glorie_points_in_view")
    return int(count.item())


def depth_l1_accumulate(gt_depth, rec_depth, err, valid, view, workspace=None):
    """slot `view` of err f64 [n_views] / valid int32 [n_views] (device) receives mean |gt_depth - rec_depth| over
    rec_depth > 0 and the number of such pixels (0: no such pixel, the view does not count); no read-back"""
    L.need_cuda(gt_depth, rec_depth, err, valid)
    gt_depth, rec_depth = L.f32(gt_depth), L.f32(rec_depth)
    if gt_depth.dim() != 2 or gt_depth.shape != rec_depth.shape:
        raise ValueError(f"two [H,W] maps are needed, got {tuple(gt_depth.shape)} and {tuple(rec_depth.shape)}")
    if err.dtype != torch.float64 or valid.dtype != torch.int32 or not 0 <= int(view) < min(err.numel(), valid.numel()):
        raise ValueError("err must be float64 and valid int32 with a slot for the view")
    H, W = gt_depth.shape
    lib, dev = L.load(), gt_depth.device
    ws = L.workspace(lib.glorie_depth_l1_workspace(H, W), dev) if workspace is None else workspace
    with torch.cuda.device(dev):
        L.check(lib.glorie_depth_l1_accumulate(L.ptr(gt_depth), L.ptr(rec_depth), H, W, L.ptr(ws), L.ptr(err), L.ptr(valid),
                                               int(view), L.stream_ptr(dev)), "glorie_depth_l1_accumulate")


def normalize(x):
    return x / np.linalg.norm(x)


def viewmatrix(z, up, pos):
    """:132-138"""
    vec2 = normalize(z)
    vec0 = normalize(np.cross(up, vec2))
    vec1 = normalize(np.cross(vec2, vec0))
    return np.stack([vec0, vec1, vec2, pos], 1)


def _draw_view(rng, centre, extents, up):
    """one camera of :171-187: the position uniform in the box, looking at a random far target rounded to 0.01"""
    origin = centre + (rng.uniform(0.0, 1.0, 3) - 0.5) * extents
    target = np.round(rng.uniform(-10000.0, 10000.0, 3), 2) - origin
    c2w = np.eye(4)
    c2w[:3, :] = viewmatrix(target, np.asarray(up, np.float64), origin)
    return c2w


def _view_box(bounds_lo, bounds_hi, shrink, lift):
    lo, hi = np.asarray(bounds_lo, np.float64), np.asarray(bounds_hi, np.float64)
    centre = 0.5 * (lo + hi)
    centre[2] += float(lift)
    return centre, (hi - lo) * np.asarray(shrink, np.float64)


def sample_views(bounds_lo, bounds_hi, n, seed, up=(0, 0, -1), shrink=(0.7, 0.7, 0.3), lift=0.0):
    """n camera-to-world matrices float64 [n,4,4] (OpenCV: z is the viewing direction) inside the axis-aligned box
    [bounds_lo, bounds_hi] shrunk about its centre by `shrink` per axis and raised by `lift` along z (the reference
    shrinks trimesh's oriented box by 0.7, 0.7, 0.3 and raises it by 0.4, :121-129); deterministic under `seed`"""
    rng = np.random.default_rng(seed)
    centre, extents = _view_box(bounds_lo, bounds_hi, shrink, lift)
    return np.stack([_draw_view(rng, centre, extents, up) for _ in range(int(n))]) if n else np.zeros((0, 4, 4))


def calc_2d_metric(rec, gt, align=True, n_imgs=1000, H=500, W=500, focal=300, unseen_points=None, views=None, seed=0,
                   z_near=0.01, z_far=20.0, edge=10.0, up=(0, 0, -1), shrink=(0.7, 0.7, 0.3), lift=0.0, max_redraws=1000,
                   return_details=False):
    """{"depth l1": cm}: the mean over the views of mean |gt depth - rec depth| over the pixels the reconstruction covers
    (:141-227); a view the reconstruction does not cover at all is skipped (:219-224).  Views: `views` [n,4,4] when
    given, else n_imgs draws of the stream of sample_views(seed) in the box of the ground truth's vertices; with
    unseen_points [m,3] a draw that sees any of them (points_in_view, one 4-byte read-back) is drawn again (:171-191).
    Every view is two rasteriser calls and one accumulator call; one read-back at the end.  return_details: also
    {"views": the cameras used, "errors": float64 per view in the unit of the mesh, "valid": pixels per view}"""
    rec_v, rec_f = _mesh(*rec)
    gt_v, gt_f = _mesh(*gt)
    dev = gt_v.device
    rec_v, _ = _aligned(rec_v, gt_v, align)
    K = (float(focal), float(focal), W / 2.0 - 0.5, H / 2.0 - 0.5)
    if views is None:
        rng = np.random.default_rng(seed)
        centre, extents = _view_box(gt_v.min(0).values.double().cpu().numpy(), gt_v.max(0).values.double().cpu().numpy(),
                                    shrink, lift)
        unseen = _points(unseen_points, "unseen_points") if unseen_points is not None else None
        used = []
        for _ in range(int(n_imgs)):
            for _ in range(int(max_redraws)):
                c2w = _draw_view(rng, centre, extents, up)
                if unseen is None or points_in_view(unseen, c2w, K, H, W, edge) == 0:
                    break
            else:
                raise L.GlorieError(f"no view without unseen points in {max_redraws} draws")
            used.append(c2w)
        views = np.stack(used) if used else np.zeros((0, 4, 4))
    else:
        views = np.stack([_matrix(v, "view") for v in views]) if len(views) else np.zeros((0, 4, 4))
    n = len(views)
    lib = L.load()
    gt_r, rec_r = _Rasteriser(gt_v, gt_f, K, H, W, z_near, z_far), _Rasteriser(rec_v, rec_f, K, H, W, z_near, z_far)
    err = torch.zeros(max(n, 1), dtype=torch.float64, device=dev)
    valid = torch.zeros(max(n, 1), dtype=torch.int32, device=dev)
    ws = L.workspace(lib.glorie_depth_l1_workspace(int(H), int(W)), dev)
    gt_depth = torch.empty(int(H), int(W), dtype=torch.float32, device=dev)
    rec_depth = torch.empty_like(gt_depth)
    w2c = torch.from_numpy(np.linalg.inv(views)).to(dev, torch.float32).contiguous() if n else None
    for i in range(n):
        gt_r.render(w2c[i], out=gt_depth)
        rec_r.render(w2c[i], out=rec_depth)
        depth_l1_accumulate(gt_depth, rec_depth, err, valid, i, workspace=ws)
    err, valid = err.cpu().numpy()[:n], valid.cpu().numpy()[:n]
    kept = err[valid > 0]
    out = {"depth l1": float(kept.mean() * 100.0) if len(kept) else float("nan")}
    return (out, {"views": views, "errors": err, "valid": valid}) if return_details else out


# ---- eval_recon.py:229-248 -------------------------------------------------------------------------------------------------
def _load(mesh, device):
    if isinstance(mesh, (str, os.PathLike)):
        from .generate_mesh import read_ply
        v, f, _ = read_ply(mesh)
        return torch.from_numpy(v).to(device), torch.from_numpy(f).to(device)
    return mesh[0], mesh[1]


def _cull_pair(rec, gt, cull):
    """both meshes cut to the same views (cull_mesh.py).  cull: {"c2ws", "K", "H", "W"} and the keywords of cull_mesh; with
    method "occlusion" and no depths both are tested against the depth of the ground truth, rasterised once per view"""
    from . import cull_mesh as C
    cull = dict(cull)
    c2ws, K, H, W = (cull.pop(k) for k in ("c2ws", "K", "H", "W"))
    method, depths = cull.pop("method", "frustum"), cull.pop("depths", None)
    rule, min_views = cull.pop("rule", "all"), cull.pop("min_views", 1)
    if method not in ("frustum", "occlusion"):
        raise ValueError(f"method must be 'frustum' or 'occlusion', got {method!r}")
    (rec_v, rec_f), (gt_v, gt_f) = rec, gt
    if method == "occlusion" and depths is None:
        counts = C.self_occlusion_visibility(gt_v, gt_f, c2ws, K, H, W, test_vertices=[rec_v, gt_v], **cull)
    else:
        counts = [C.vertex_visibility(v, c2ws, K, H, W, depths=depths if method == "occlusion" else None, **cull)
                  for v in (rec_v, gt_v)]
    return tuple(C.compact_mesh(v, f, C.select_faces(f, c, min_views, rule)) for (v, f), c in zip((rec, gt), counts))


def eval_recon(rec, gt, eval_2d=True, eval_3d=True, align=True, output=None, device="cuda", kwargs_3d=None, kwargs_2d=None,
               cull=None):
    """rec, gt: (vertices, faces) device tensors or paths of PLYs in the layout generate_mesh.write_ply writes.  The ICP
    alignment (align=True) is computed once and shared.  cull: None, or a dict {"c2ws" [M,4,4] views in the ground truth's
    frame, "K", "H", "W", "method", "depths", ..} (_cull_pair): the ground truth and the aligned reconstruction are cut to
    those views before they are scored.  -> the merged dict of calc_3d_metric and calc_2d_metric; with
    `output` also output/metrics_recon.txt, one "name: value" line per entry"""
    rec, gt = _load(rec, device), _load(gt, device)
    rec_v, rec_f = _mesh(*rec)
    gt_v, gt_f = _mesh(*gt)
    rec_v, _ = _aligned(rec_v, gt_v, align)
    if cull is not None:
        (rec_v, rec_f), (gt_v, gt_f) = _cull_pair((rec_v, rec_f), (gt_v, gt_f), cull)
    result = {}
    if eval_3d:
        result.update(calc_3d_metric((rec_v, rec_f), (gt_v, gt_f), align=False, **(kwargs_3d or {})))
    if eval_2d:
        result.update(calc_2d_metric((rec_v, rec_f), (gt_v, gt_f), align=False, **(kwargs_2d or {})))
    if output is not None:
        os.makedirs(str(output), exist_ok=True)
        with open(os.path.join(str(output), "metrics_recon.txt"), "w") as fp:
            for k, v in result.items():
                fp.write(f"{k}: {v}\n")
    return result
