"""Scenes for the mapper's window kernels (csrc/warp.hip, csrc/select.hip, csrc/color_grad.hip) on general cameras:
numpy on the host, no GPU.  tests/test_mapper_scenes.py checks the scenes themselves, tests/test_gpu_mapper_kernels.py
runs the kernels on them.

Cameras: `general_window` - one fixed general rotation G (the QR factor of a Gaussian matrix, determinant +1, as
window_rays_ref.general_c2ws draws it) times a small rotation about a random axis per camera, plus translations, in the
renderer's OpenGL convention.  The cameras share a view and no entry of any R is near 0 or +-1.  `INTRINSICS` have
fx != fy (19 % and more apart) and a non-integer principal point off the image centre.

Firm scenes: everything is rounded to fp32 once, the float64 side computes on the rounded values, and a ray or point any
of whose decisions sits within a band of its threshold is redrawn *in the generator* - a comparison on a firm scene
leaves nothing out afterwards and can ask for exact decisions.

  warp     WARP_MARGIN = 1e-3 px (and 1e-3 in z): u, v of every (ray, frame) entry against 5, W-5, H-5, z against 0, and
           the bilinear read's texel boundary for the entries in view.  fp32 numbers below 64 are 2^-18 = 3.8e-6 apart,
           so the margin is 262 spacings of u, v at these image sizes (1e-2 px would reject almost every ray of a
           64-frame window, 1e-3 px does not).
  frustum  the bands of test_gpu_keyframe_select's `near`: a relative 1e-4 on every threshold, 1e-2 of a 1/32-px step
           around the rounding boundary of the depth read.
  overlap  the same threshold bands on every sample of every ray against every keyframe.
"""
import numpy as np

from color_grad_ref import sobel_magnitude
from keyframe_select_ref import frustum_ref, project as select_project

U32 = 2.0 ** -24                               # fp32 unit roundoff
INTRINSICS = {(23, 37): (41.5, 33.25, 17.3, 10.6), (24, 40): (44.75, 36.5, 18.7, 12.4),
              (48, 64): (71.5, 58.25, 30.3, 22.6), (60, 80): (89.5, 72.25, 37.3, 27.6)}
R_MIN = 0.05                                   # the smallest |R_ij| any camera of a window may have
WARP_EDGE, WARP_BETA, WARP_MARGIN = 5, 0.1, 1e-3
OUTSIDE_ID = 999                               # the frame id of rays whose own frame is not in the window


def rotation(axis, angle):
    """Rodrigues: the rotation by `angle` about `axis`, [3,3] float64"""
    k = np.asarray(axis, np.float64)
    k = k / np.linalg.norm(k)
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * (K @ K)


def general_rotation(rng, floor=0.2):
    """a QR factor of a Gaussian matrix with determinant +1 whose entries are all at least `floor` in size"""
    while True:
        q, _ = np.linalg.qr(rng.standard_normal((3, 3)))
        if np.linalg.det(q) < 0:
            q[:, 0] *= -1
        if np.abs(q).min() >= floor:
            return q


def general_window(M, rng, spread, turned=(), centre=(0.3, -0.2, 0.5)):
    """M camera-to-world matrices [M,4,4] f32: c2w_m = G . dR_m with dR_m a rotation by up to `spread` rad about a
    random axis, translations `centre` + G . uniform(-2 spread, 2 spread)^3.  Cameras in `turned` are rotated by pi about
    their own y axis (what the others see lies behind them)."""
    G = general_rotation(rng)
    out = np.zeros((M, 4, 4))
    for m in range(M):
        R = G @ rotation(rng.standard_normal(3), rng.uniform(-spread, spread))
        if m in turned:
            R = R @ np.diag([-1.0, 1.0, -1.0])
        out[m, :3, :3] = R
        out[m, :3, 3] = np.asarray(centre) + G @ rng.uniform(-2 * spread, 2 * spread, 3)
        out[m, 3, 3] = 1
    out = out.astype(np.float32)
    assert np.abs(out[:, :3, :3]).min() >= R_MIN and np.abs(out[:, :3, :3]).max() <= 1 - R_MIN ** 2 / 2, \
        np.abs(out[:, :3, :3]).min()
    return out


def pixel_dirs(i, j, K):
    """camera-frame directions through pixels (i, j), z = -1 (OpenGL)"""
    fx, fy, cx, cy = K
    return np.stack([(i - cx) / fx, -(j - cy) / fy, -np.ones_like(i)], -1)


# ---- pixel-warping loss ----------------------------------------------------------------------------------------------
def warp_project(c2ws, X, K, mutate=None):
    """float64 (u, v, z) [N,M] of points X [N,3] in M cameras, the projection of pix_warp_ref.project.  `mutate` names a
    deliberate mistake (tests/test_mapper_scenes.py): "fy_fx", "no_translation", "cofactor"."""
    fx, fy, cx, cy = K
    w2c = np.linalg.inv(np.asarray(c2ws, np.float64))
    w2c = mutate_w2c(w2c, mutate)
    p = np.einsum("mij,nj->nmi", w2c[:, :3, :3], np.asarray(X, np.float64)) + w2c[None, :, :3, 3]
    a, b, c = p[..., 0], p[..., 1], p[..., 2]
    z = c + 1e-5
    return (-fx * a + cx * c) / z, ((fx if mutate == "fy_fx" else fy) * b + cy * c) / z, z


def mutate_w2c(w2c, mutate):
    """the inverse pose [..,4,4] with the translation column dropped, or one cofactor pair of its 3x3 block swapped"""
    w2c = np.array(w2c, np.float64)
    if mutate == "no_translation":
        w2c[..., :3, 3] = 0
    elif mutate == "cofactor":
        w2c[..., 0, 1], w2c[..., 1, 0] = w2c[..., 1, 0].copy(), w2c[..., 0, 1].copy()
    return w2c


def _warp_firm(c2ws, o, d, z, K, H, W):
    u, v, zc = warp_project(c2ws, o.astype(np.float64) + d.astype(np.float64) * z.astype(np.float64)[:, None], K)
    near = lambda x, t: np.abs(x - t) < WARP_MARGIN
    bad = near(u, WARP_EDGE) | near(u, W - WARP_EDGE) | near(v, WARP_EDGE) | near(v, H - WARP_EDGE) | near(zc, 0)
    seen = (u > WARP_EDGE) & (u < W - WARP_EDGE) & (v > WARP_EDGE) & (v < H - WARP_EDGE) & (zc < 0)
    for q in (u - 0.5, v - 0.5):
        f = q - np.floor(q)
        bad |= seen & ((f < WARP_MARGIN) | (f > 1 - WARP_MARGIN))
    return ~bad.any(1), seen


def warp_scene(H, W, M, N, seed, spread=0.08, turned=(), nonrigid=False, duplicate=False, outside=0.25):
    """N firm rays against a window of M general cameras with random-noise images.  A share `outside` of the rays starts
    in a camera that is not in the window (own frame id OUTSIDE_ID), the others in a window camera; `duplicate` repeats
    frame_indices[0] in slot 1; `nonrigid` gives every c2w a well-conditioned non-orthogonal 3x3 block with det > 0.
    The last ray is a kept one (whatever N is, the last partial sum of the loss carries a count)."""
    rng = np.random.default_rng(seed)
    K = INTRINSICS[(H, W)]
    cams = general_window(M + 1, rng, spread, turned).astype(np.float64)
    if nonrigid:
        for m in range(M + 1):
            while True:
                A = np.eye(3) + 0.15 * rng.standard_normal((3, 3))
                if np.linalg.det(A) > 0.5 and np.linalg.cond(A) < 2.5:
                    break
            cams[m, :3, :3] = cams[m, :3, :3] @ A
    cams = cams.astype(np.float32)
    c2ws = cams[:M]
    ids = np.sort(rng.choice(200, M, replace=False)).astype(np.int64)
    if duplicate:
        ids[1] = ids[0]
    all_ids = np.append(ids, OUTSIDE_ID)
    images = rng.uniform(0, 1, (M, H, W, 3)).astype(np.float32)

    pool = [np.zeros((0, 3), np.float32), np.zeros((0, 3), np.float32), np.zeros(0, np.float32), np.zeros(0, np.int64)]
    kept = np.zeros(0, bool)
    while len(kept) < N or not kept[N - 1:].any():
        n = max(2 * N, 256)
        src = np.where(rng.uniform(size=n) < outside, M, rng.integers(0, M, n))
        dc = pixel_dirs(rng.uniform(0, W, n), rng.uniform(0, H, n), K)
        d = np.einsum("nij,nj->ni", cams[src, :3, :3].astype(np.float64), dc).astype(np.float32)
        o, z = cams[src, :3, 3], rng.uniform(1.5, 4.0, n).astype(np.float32)
        ok, seen = _warp_firm(c2ws, o, d, z, K, H, W)
        n_in = (seen & (ids[None, :] != all_ids[src][:, None])).sum(1)
        pool = [np.concatenate([p, x[ok]]) for p, x in zip(pool, (o, d, z, src))]
        kept = np.concatenate([kept, n_in[ok] >= 4])
    last = N - 1 + int(np.argmax(kept[N - 1:]))
    sel = np.append(np.arange(N - 1), last)
    o, d, z, src = (p[sel] for p in pool)
    return dict(rays_o=o, rays_d=d, depth=z, c2ws=c2ws, frame_indices=ids, indices=all_ids[src], images=images,
                gt=rng.uniform(0, 1, (N, 3)).astype(np.float32), fx=K[0], fy=K[1], cx=K[2], cy=K[3], H=H, W=W)


# name -> warp_scene arguments: the scenes of tests/test_gpu_mapper_kernels.py (every one enters its float32 figure)
WARP_SCENES = {
    "m5": dict(H=23, W=37, M=5, N=600, seed=5),
    "m6": dict(H=23, W=37, M=6, N=600, seed=6, turned=(2,)),
    "m63": dict(H=24, W=40, M=63, N=300, seed=63, turned=(7, 40)),
    "m64": dict(H=24, W=40, M=64, N=300, seed=64, turned=(7, 40)),
    "nonrigid": dict(H=23, W=37, M=6, N=400, seed=16, nonrigid=True),
    "duplicate": dict(H=23, W=37, M=6, N=400, seed=26, duplicate=True),
    **{f"n{N}": dict(H=23, W=37, M=5, N=N, seed=100 + N % 97) for N in (1, 255, 256, 257, 65537)},
}


def warp_terms(c, dtype=np.float64, mutate=None):
    """The loss of tests/pix_warp_ref.py and its gradient with respect to depth written out term by term, in `dtype`
    arithmetic (float64: the restatement itself, test_mapper_scenes holds it to the restatement's autograd; float32:
    what a plain fp32 evaluation of the same formulas gives).  Firm scenes only: the bilinear cell is interior.

    -> dict(loss, count, grad [N], scale [N], mask [N,M], u, v, z, ray_loss [N], ray_kept [N]).  `scale` is the ray's
    sum of |terms|: every product that enters grad with its factors replaced by the sums of absolute values they are
    themselves computed from (|w2c_R| . |rays_d| for the direction, (fx |a| + cx |c|) / |z| for u, |texel| sums for the
    bilinear slopes, (|value| + |colour|) / beta for the smooth-L1 slope) - the size against which fp32 rounding of the
    gradient is measured."""
    f = lambda x: np.asarray(x, dtype)
    o, d, dep, gt, img = f(c["rays_o"]), f(c["rays_d"]), f(c["depth"]), f(c["gt"]), f(c["images"])
    fx, fy, cx, cy = (dtype(c[k]) for k in ("fx", "fy", "cx", "cy"))
    H, W, M = c["H"], c["W"], c["c2ws"].shape[0]
    w2c = np.linalg.inv(f(c["c2ws"]))
    if mutate is not None:
        w2c = f(mutate_w2c(w2c, mutate))
    assert w2c.dtype == dtype
    Rm, tm = w2c[:, :3, :3], w2c[:, :3, 3]
    X = o + d * dep[:, None]
    p = np.einsum("mij,nj->nmi", Rm, X) + tm[None]
    p_abs = np.einsum("mij,nj->nmi", np.abs(Rm), np.abs(X)) + np.abs(tm)[None]
    a, b, cc = p[..., 0], p[..., 1], p[..., 2]
    z = cc + dtype(1e-5)
    fyy = fx if mutate == "fy_fx" else fy
    u, v = (-fx * a + cx * cc) / z, (fyy * b + cy * cc) / z
    mask = (u < W - WARP_EDGE) & (u > WARP_EDGE) & (v < H - WARP_EDGE) & (v > WARP_EDGE) & (z < 0)
    mask &= np.asarray(c["frame_indices"])[None, :] != np.asarray(c["indices"])[:, None]
    mask &= mask.sum(1, keepdims=True) >= 4
    x = np.clip(np.where(mask, u, dtype(8)) - dtype(0.5), 0, W - 1)
    y = np.clip(np.where(mask, v, dtype(8)) - dtype(0.5), 0, H - 1)
    x0, y0 = np.floor(x), np.floor(y)
    xi, yi = x0.astype(np.int64), y0.astype(np.int64)
    assert xi.min() >= 0 and xi.max() + 1 < W and yi.min() >= 0 and yi.max() + 1 < H
    e, s = (x - x0)[..., None], (y - y0)[..., None]
    we, ws = 1 - e, 1 - s
    mi = np.arange(M)[None, :]
    vnw, vne, vsw, vse = img[mi, yi, xi], img[mi, yi, xi + 1], img[mi, yi + 1, xi], img[mi, yi + 1, xi + 1]
    val = vnw * we * ws + vne * e * ws + vsw * we * s + vse * e * s
    gix, giy = (vne - vnw) * ws + (vse - vsw) * s, (vsw - vnw) * we + (vse - vne) * e
    gix_abs = (np.abs(vne) + np.abs(vnw)) * ws + (np.abs(vse) + np.abs(vsw)) * s
    giy_abs = (np.abs(vsw) + np.abs(vnw)) * we + (np.abs(vse) + np.abs(vne)) * e
    diff = val - gt[:, None, :]
    ad = np.abs(diff)
    beta = dtype(WARP_BETA)
    quad = ad < beta
    sl1 = np.where(quad, dtype(0.5) * diff * diff / beta, ad - dtype(0.5) * beta)
    dl = np.where(quad, diff / beta, np.sign(diff))
    dl_abs = np.where(quad, (np.abs(val) + np.abs(gt[:, None, :])) / beta, 1)
    dp = np.einsum("mij,nj->nmi", Rm, d)
    dp_abs = np.einsum("mij,nj->nmi", np.abs(Rm), np.abs(d))
    da, db, dc = dp[..., 0], dp[..., 1], dp[..., 2]
    du, dv = (-fx * da + cx * dc - u * dc) / z, (fyy * db + cy * dc - v * dc) / z
    az = np.abs(z)
    u_abs, v_abs = (fx * p_abs[..., 0] + cx * p_abs[..., 2]) / az, (fy * p_abs[..., 1] + cy * p_abs[..., 2]) / az
    du_abs = (fx * dp_abs[..., 0] + (cx + u_abs) * dp_abs[..., 2]) / az
    dv_abs = (fy * dp_abs[..., 1] + (cy + v_abs) * dp_abs[..., 2]) / az
    m3 = mask[..., None]
    terms = np.where(m3, dl * (gix * du[..., None] + giy * dv[..., None]), 0)
    terms_abs = np.where(m3, dl_abs * (gix_abs * du_abs[..., None] + giy_abs * dv_abs[..., None]), 0)
    count = int(mask.sum())
    ray_loss = np.where(m3, sl1, 0).sum((1, 2))
    n3 = dtype(3 * count) if count else dtype("nan")
    return dict(loss=ray_loss.sum() / n3, count=count, grad=terms.sum((1, 2)) / n3 if count else np.zeros(len(dep)),
                scale=terms_abs.sum((1, 2)) / n3 if count else np.zeros(len(dep)), mask=mask, u=u, v=v, z=z,
                ray_loss=ray_loss, ray_kept=mask.sum(1))


def blocked_loss(ray_loss, ray_kept, block=256, max_parts=None):
    """loss and count as the kernels reduce them: one partial per `block` rays, then the partials (only the first
    `max_parts` of them - the deliberate mistake of a finish pass without its stride loop)"""
    n = -(-len(ray_loss) // block)
    parts = [(ray_loss[k * block:(k + 1) * block].sum(), int(ray_kept[k * block:(k + 1) * block].sum()))
             for k in range(n)][:max_parts]
    count = sum(p[1] for p in parts)
    return (sum(p[0] for p in parts) / (3 * count) if count else float("nan")), count


# ---- frustum selection -----------------------------------------------------------------------------------------------
def frustum_near(d, H, W, edge):
    """the decisions of frustum_ref's details `d` that a rounding could flip (test_gpu_keyframe_select's bands)"""
    rel = lambda x, t: np.abs(x - t) <= 1e-4 * np.maximum(np.abs(t), 1.0)
    q = lambda x: np.abs(x * 32 - np.floor(x * 32) - 0.5) < 1e-2
    return rel(d["u"], edge) | rel(d["u"], W - edge) | rel(d["v"], edge) | rel(d["v"], H - edge) | \
        rel(d["negz"], 0.0) | rel(d["negz"], d["depth"] + 0.5) | q(d["u"]) | q(d["v"])


def frustum_scene(H, W, n, seed, kind="holes", edges=(-4.0, 6.0)):
    """n firm points around the frustum of one general camera with translation, firm for every edge of `edges` at once.
    kind "holes": a depth map of 2 - 3.5 with a zero row band, a zero column band and scattered zeros; "patch": a depth
    map that is zero but for a 5 x 5 patch - nearly every sample is 0 and the few on the patch (one point in 50 is aimed
    at it) set the maximum that replaces them; a single point samples 0 and the maximum is 0."""
    rng = np.random.default_rng(seed)
    K = INTRINSICS[(H, W)]
    c2w = general_window(1, rng, 0.1)[0]
    if kind == "holes":
        depth = rng.uniform(2.0, 3.5, (H, W)).astype(np.float32)
        depth[rng.uniform(size=(H, W)) < 0.1] = 0
        depth[H // 3:H // 3 + 3, :] = 0
        depth[:, 2 * W // 3:2 * W // 3 + 4] = 0
    else:
        depth = np.zeros((H, W), np.float32)
        depth[H // 2 - 2:H // 2 + 3, W // 2 - 2:W // 2 + 3] = rng.uniform(2.5, 3.5, (5, 5)).astype(np.float32)
    aimed = n // 50 if kind == "patch" else 0    # the first points of a "patch" cloud look at the patch

    def draw(idx):
        k = len(idx)
        dist = rng.uniform(-1.0, 5.5, k)
        i, j = rng.uniform(-8, W + 8, k), rng.uniform(-8, H + 8, k)
        aim = idx < aimed
        i[aim], j[aim] = rng.uniform(W // 2 - 1, W // 2 + 2, k)[aim], rng.uniform(H // 2 - 1, H // 2 + 2, k)[aim]
        dc = pixel_dirs(i, j, K) * dist[:, None]
        return (c2w[:3, 3].astype(np.float64) + dc @ c2w[:3, :3].astype(np.float64).T).astype(np.float32)

    pts = draw(np.arange(n))
    while True:                                 # the maximum couples the points: judge the whole cloud every time
        bad = np.zeros(n, bool)
        for edge in edges:
            bad |= frustum_near(frustum_ref(pts, c2w, depth, *K, H, W, edge)[1], H, W, edge)
        if not bad.any():
            break
        pts[bad] = draw(np.nonzero(bad)[0])
    return dict(points=pts, c2w=c2w, depth=depth, K=K, H=H, W=W)


# ---- keyframe overlap ------------------------------------------------------------------------------------------------
def overlap_samples(o, d, dep, n_samples, single_t=0.0):
    """the samples of one ray set [R, n_samples, 3] float64 as keyframe_select_ref.sample_points places them
    (`single_t`: where a single sample sits; the reference's linspace puts it at 0)"""
    t = np.linspace(0.0, 1.0, n_samples) if n_samples > 1 else np.array([single_t])
    dep = np.asarray(dep, np.float64)
    z = (0.8 * dep)[:, None] * (1 - t) + (dep + 0.5)[:, None] * t
    return np.asarray(o, np.float64)[:, None, :] + np.asarray(d, np.float64)[:, None, :] * z[..., None]


def overlap_inside(pts, c2ws, K, H, W, edge):
    """[n, K] bool: point inside keyframe k; and whether any of its decisions is near a threshold"""
    rel = lambda x, t: np.abs(x - t) <= 1e-4 * np.maximum(np.abs(t), 1.0)
    ins, near = [], []
    for c2w in c2ws:
        u, v, z = select_project(c2w, pts, *K)
        ins.append((u < W - edge) & (u > edge) & (v < H - edge) & (v > edge) & (z < 0))
        near.append(rel(u, edge) | rel(u, W - edge) | rel(v, edge) | rel(v, H - edge) | rel(z, 0.0))
    return np.stack(ins, 1), np.stack(near, 1)


def overlap_scene(n_kf, R, n_samples, seed, H=60, W=80, edge=20):
    """R firm rays of a general camera with n_samples samples each against n_kf general keyframes.  With 5 keyframes and
    more, keyframe 0 is the rays' own camera (every sample inside: the pixels are drawn inside the edge band) and
    keyframes 2, 6, 10, ... are turned away (none inside).  From 37 rays on every sixth ray has zero depth.  A ray with
    a single sample is drawn so that its near and far end fall differently in some keyframe."""
    rng = np.random.default_rng(seed)
    K = INTRINSICS[(H, W)]
    cams = general_window(n_kf + 1, rng, 0.12, turned=tuple(range(2, n_kf, 4)))
    cur, c2ws = cams[n_kf], cams[:n_kf].copy()
    if n_kf >= 5:
        c2ws[0] = cur

    def draw(k):
        dc = pixel_dirs(rng.uniform(edge + 1, W - edge - 1, k), rng.uniform(edge + 1, H - edge - 1, k), K)
        d = (dc @ cur[:3, :3].astype(np.float64).T).astype(np.float32)
        return np.broadcast_to(cur[:3, 3], (k, 3)).copy(), d, rng.uniform(1.0, 4.0, k).astype(np.float32)

    o, d, dep = draw(R)
    while True:
        pts = overlap_samples(o, d, dep, n_samples)
        ins, near = overlap_inside(pts.reshape(-1, 3), c2ws, K, H, W, edge)
        bad = near.reshape(R, -1).any(1)
        if n_samples == 1:
            far = overlap_inside(overlap_samples(o, d, dep, 1, single_t=1.0).reshape(-1, 3), c2ws, K, H, W, edge)
            bad |= far[1].any(1) | (far[0] == ins).all(1)
        if not bad.any():
            break
        k = int(bad.sum())
        o[bad], d[bad], dep[bad] = draw(k)
    if R >= 37:
        dep[::6] = 0
    return dict(rays_o=o, rays_d=d, depth=dep, c2ws=c2ws, K=K, H=H, W=W, edge=edge, n_samples=n_samples)


# ---- colour-gradient maps --------------------------------------------------------------------------------------------
def color_image(H, W, seed, kind="noise"):
    """[H,W,3] f32 image, a validity mask and a depth map.  "noise": uniform noise (the border pixels carry large
    gradients); "segments": three column bands of horizontal ramps whose Sobel magnitude 2 x slope sits below 0.01, on
    the radius map's slope, and above the threshold 0.15"""
    rng = np.random.default_rng(seed)
    if kind == "noise":
        img = rng.uniform(0, 1, (H, W, 3))
    else:
        slope = np.repeat([0.002, 0.03, 0.2], -(-W // 3))[:W]
        img = np.broadcast_to(np.cumsum(slope)[None, :, None], (H, W, 3)) + 1e-4 * rng.uniform(0, 1, (H, W, 3))
    return dict(image=img.astype(np.float32), valid=rng.uniform(size=(H, W)) < 0.7,
                depth=rng.uniform(0.5, 4.0, (H, W)).astype(np.float32))


def color_grad_bounds(ref, image, depth_add=None, depth_query=None, thr=0.15, rmax=0.08, rmin=0.02, ratio=2.0):
    """Per-pixel bounds on |kernel - float64 restatement| for the maps of color_grad_maps_ref's result `ref`, from the
    fp32 unit roundoff u = 2^-24 alone.  G = max |rgb| bounds every gray value (the coefficients sum to 1).

      gray   three fp32 coefficients (each rounded: u) and three rounded operations, every partial sum <= G:   4 u G
      Sobel  six taps of total weight 2 in double (no further error), one rounding to fp32:       8 u G + u |gx|
      mag    sqrt(gx^2 + gy^2), the two squares, the sum and the root each rounded once: a relative 2 u, on top of the
             inputs' errors, which a 2-norm passes on at most sqrt(2)-fold:
             sqrt(2) (8 u G + u g) + 2 u g  <=  u (12 G + 3.5 g)
      radii  the map is continuous and piecewise linear: the magnitude's bound times |slope| (times depth / 3 when
             scaled), plus one fp32 ulp of the radius for the final rounding."""
    G = float(np.abs(np.asarray(image, np.float64)).max())
    g = sobel_magnitude(image)
    b_grad = U32 * (12 * G + 3.5 * g)
    ulp = lambda r: np.spacing(np.abs(r).astype(np.float32)).astype(np.float64)
    out = dict(grad=b_grad)
    for name, k, depth in (("r_add", 1.0, depth_add), ("r_query", ratio, depth_query)):
        slope = k * (rmax - rmin) / (thr - 0.01)
        s = 1.0 if depth is None else np.asarray(depth, np.float64) / 3.0
        out[name] = b_grad * slope * s + ulp(ref[name])
    return out


def border_mask(H, W):
    b = np.zeros((H, W), bool)
    b[[0, -1], :] = True
    b[:, [0, -1]] = True
    return b
