"""numpy restatement of glorie_window_rays (include/glorie_hip.h) in the kernel's operation order, in fp32, a float64 matrix
formulation of the ray directions, the torch composition the runner uses per frame, and the scenes the tests share."""
import numpy as np

EPS32 = float(np.finfo(np.float32).eps)          # 2^-23: one rounding has relative size EPS32 / 2


def window_rays_ref(depths, images, c2ws, ii, jj, per, fx, fy, cx, cy, radius_maps=None, const_radius=None,
                    channels_first=True):
    """depths [M,H,W], images [M,3,H,W] (or [M,H,W,3]), c2ws [M,4,4] f32, ii / jj int64 [M * per] ->
    (rays_o [N,3], rays_d [N,3], depth [N], color [N,3], radius [N] or None), all f32.
    dx = (float(i) - cx) / fx, dy = -((float(j) - cy) / fy), dz = -1;  rays_d[a] = (dx R[a][0] + dy R[a][1]) + dz R[a][2]:
    numpy rounds every float32 array operation on its own"""
    f = np.float32
    depths, c2ws = np.asarray(depths, f), np.asarray(c2ws, f)
    M, H, W = depths.shape
    N = M * per
    assert ii.shape == (N,) and jj.shape == (N,)
    m = np.arange(N) // max(per, 1)
    i = np.clip(ii, 0, W - 1)
    j = np.clip(jj, 0, H - 1)
    fx, fy, cx, cy = f(fx), f(fy), f(cx), f(cy)
    dx = (i.astype(f) - cx) / fx
    dy = -((j.astype(f) - cy) / fy)
    dz = np.full(N, -1.0, f)
    R = c2ws[m, :3, :3]                                                  # [N,3,3]
    rays_d = np.stack([(dx * R[:, a, 0] + dy * R[:, a, 1]) + dz * R[:, a, 2] for a in range(3)], 1).astype(f)
    rays_o = c2ws[m, :3, 3].astype(f)
    images = np.asarray(images, f)
    color = images[m, :, j, i] if channels_first else images[m, j, i, :]
    if radius_maps is not None:
        radius = np.asarray(radius_maps, f)[m, j, i]
    elif const_radius is not None:
        radius = np.full(N, const_radius, f)
    else:
        radius = None
    return rays_o, rays_d, depths[m, j, i], np.ascontiguousarray(color, f), radius


def rays_d_f64(c2ws, ii, jj, per, fx, fy, cx, cy):
    """the directions as R @ dirs in float64 from the fp32 inputs -> (rays_d [N,3], S [N,3]) with
    S = |dx R0| + |dy R1| + |dz R2|, the scale of the rounding bounds"""
    f = np.float32
    c = np.asarray(c2ws, f).astype(np.float64)
    N = ii.shape[0]
    m = np.arange(N) // max(per, 1)
    fx, fy, cx, cy = (float(f(x)) for x in (fx, fy, cx, cy))
    dirs = np.stack([(ii.astype(np.float64) - cx) / fx, -(jj.astype(np.float64) - cy) / fy, -np.ones(N)], 1)
    R = c[m, :3, :3]
    terms = R * dirs[:, None, :]                                         # [N,3(a),3(term)]
    return terms.sum(-1), np.abs(terms).sum(-1)


def general_c2ws(M, rng):
    """M general rotations (a QR factor of a Gaussian matrix, determinant +1) with translations, [M,4,4] f32"""
    out = np.zeros((M, 4, 4), np.float32)
    for m in range(M):
        q, _ = np.linalg.qr(rng.standard_normal((3, 3)))
        if np.linalg.det(q) < 0:
            q[:, 0] *= -1
        out[m, :3, :3] = q
        out[m, :3, 3] = rng.uniform(-3, 3, 3)
        out[m, 3, 3] = 1
    return out


INTRINSICS = {"A": (6.37, 5.91, 3.21, 2.13), "B": (11.73, 12.19, 6.41, 4.27), "C": (20.3, 19.7, 11.6, 7.9)}
SHAPES = {"A": (3, 5, 7, 4), "B": (67, 9, 13, 5), "C": (2, 16, 24, 300)}         # M, H, W, per


def scene(name, seed=0):
    """the inputs of shape A / B / C as numpy arrays: general rotations with translation, non-integer intrinsics, a draw
    inside the image (A: the four image corners among it)"""
    M, H, W, per = SHAPES[name]
    rng = np.random.default_rng(seed + sum(map(ord, name)))
    ii = rng.integers(0, W, M * per).astype(np.int64)
    jj = rng.integers(0, H, M * per).astype(np.int64)
    if name == "A":
        ii[:4] = [0, W - 1, 0, W - 1]
        jj[:4] = [0, 0, H - 1, H - 1]
    return dict(M=M, H=H, W=W, per=per, K=INTRINSICS[name], c2ws=general_c2ws(M, rng),
                depths=rng.uniform(0.5, 4.0, (M, H, W)).astype(np.float32),
                images=rng.uniform(0, 1, (M, 3, H, W)).astype(np.float32),
                radius_maps=rng.uniform(0.01, 0.1, (M, H, W)).astype(np.float32), ii=ii, jj=jj)


def torch_composition(depths, images, c2ws, ii, jj, per, fx, fy, cx, cy, device, radius_maps=None):
    """what SequenceRunner._window_rays composes: common.get_rays_from_uv plus indexing per frame, concatenated
    (torch tensors on `device`; images [M,3,H,W])"""
    import torch
    from glorie_slam_amd.common import get_rays_from_uv
    ro, rd, d, col, rad = [], [], [], [], []
    for m in range(len(depths)):
        i, j = ii[m * per:(m + 1) * per], jj[m * per:(m + 1) * per]
        o, dd = get_rays_from_uv(i.float(), j.float(), c2ws[m], fx, fy, cx, cy, device)
        ro.append(o.reshape(-1, 3))
        rd.append(dd.reshape(-1, 3))
        d.append(depths[m][j, i])
        col.append(images[m][:, j, i].t())
        if radius_maps is not None:
            rad.append(radius_maps[m][j, i])
    cat = torch.cat
    return cat(ro).contiguous(), cat(rd).contiguous(), cat(d), cat(col).contiguous(), (cat(rad) if rad else None)
