"""Scenes for the cloud deformation and z-buffer kernels (csrc/deform.hip) on general cameras: numpy on the host, no GPU.
tests/test_deform_scenes.py checks the scenes themselves, tests/test_gpu_deform_kernels.py runs the kernels on them.  The
float64 restatement and the float32 compositions are tests/deform_ref.py (its `dtype` argument).

Cameras: every stored pose is a world-to-camera quaternion whose four components are all at least 0.2 in size (the
rotation is mapper_scenes.general_rotation) with a translation of 0.2 to 1 per axis; fx and fy are 19-25 % apart, cx and
cy differ and neither is the image centre (mapper_scenes.INTRINSICS at 23 x 37, ZK for the other z-buffer sizes).

Deformation scenes (deform_scene): 23 x 37 maps in B = 7 slots.  Four valid-depth counts are planted (none, 1, 63, 64)
and each needs a dirty keyframe of its own, so there are five dirty keyframes with points where three would not hold
them:
    slot 0  "wide"   dirty, previous depths log-uniform over 1e-3 .. 1e3 (as in every slot but 2 and 4), new depths
                     0.7 .. 1.4 times the previous ones
    slot 1  "one"    dirty, exactly one point with a valid depth, the others on holes
    slot 2  "k63"    dirty, exactly 63 points with a valid depth, all within a factor 1.25 of one level: the sum of
                     their terms is ~ 50 x the largest, which an exponent without the count's bit length overflows
    slot 3  "clean"  not dirty
    slot 4  "k64"    dirty, exactly 64 (the count's bit length changes here), narrow like slot 2
    slot 5  "empty"  dirty, no points
    slot 6  "holes"  dirty, every point on a hole (scale 1, the documented deviation)
Scenes of 257 points and more hold all of these, one hole point with previous depth exactly 1.0f per dirty keyframe
(its new depth is the scale itself) and four points with one out-of-range index each.  The smaller scenes (1, 63, 64,
65 points: less than, exactly and just over a wave) spread their points over the same slots without the planted counts.
Every point has a pixel of its own within its keyframe.  Three layouts order the same points differently: "runs"
(contiguous per keyframe), "interleaved" (round robin over the keyframes: no wave holds a single keyframe), "mixed"
(the runs cut into pieces of 1 to 100 points, shuffled).

Z-buffer scenes (zbuf_scene): `counter` maps of H x W points unprojected from cameras near a general view camera, one
more map behind them that must not be read, and planted points (see zbuf_scene).  Firmness is an input: the generator
clears the mask bit of every point whose float64 u or v lies within DELTA px of an integer while within a pixel of the
image, or whose |z| < Z_MIN; what remains is compared in full.  border_scene is the one scene on a special camera
(identity pose, dyadic intrinsics): its points project to u == 0 and v == 0 exactly in float32 and float64 alike, which
no general camera can offer to a firm scene.
"""
import fractions
import math

import numpy as np

from mapper_scenes import INTRINSICS, general_rotation, pixel_dirs, rotation

H_DEFORM, W_DEFORM, B_DEFORM = 23, 37, 7
WIDE, ONE, K63, CLEAN, K64, EMPTY, HOLES = range(7)
SLOTS_WITH_POINTS = (WIDE, ONE, K63, CLEAN, K64, HOLES)
DIRTY = np.array([True, True, True, False, True, True, True])
NEAR, FAR = 0.95, 1.05
Q_MIN = 0.2                                    # the smallest quaternion component of a stored pose
ZK = {(5, 7): (9.5, 7.6, 3.6, 1.4), (23, 37): INTRINSICS[(23, 37)], (37, 53): (66.5, 53.25, 24.3, 16.6)}
DELTA, Z_MIN = 1e-3, 1e-4
LAYOUTS = ("runs", "interleaved", "mixed")


def quat_of(R):
    """(x, y, z, w) of a rotation matrix, w >= 0"""
    w = math.sqrt(max(1 + R[0, 0] + R[1, 1] + R[2, 2], 0.0)) / 2
    return np.array([(R[2, 1] - R[1, 2]) / (4 * w), (R[0, 2] - R[2, 0]) / (4 * w), (R[1, 0] - R[0, 1]) / (4 * w), w])


def general_pose(rng):
    """[tx ty tz qx qy qz qw] f32: every quaternion component at least Q_MIN in size, every translation component 0.2 - 1"""
    while True:
        R = general_rotation(rng)
        if 1 + np.trace(R) < 0.2:
            continue
        q = quat_of(R)
        if np.abs(q).min() >= Q_MIN + 1e-3:
            break
    t = rng.uniform(0.2, 1.0, 3) * rng.choice([-1.0, 1.0], 3)
    return np.concatenate([t, q / np.linalg.norm(q)]).astype(np.float32)


# ---- deformation -----------------------------------------------------------------------------------------------------
def _counts(n):
    """slot -> (points with a valid depth, points on holes)"""
    if n >= 257:
        rest = n - 4
        if n >= 1000:
            each = rest // 6
            c = {ONE: (1, each - 1), K63: (63, each - 63), K64: (64, each - 64), HOLES: (0, each), CLEAN: (each // 2, each - each // 2)}
        else:
            c = {ONE: (1, 40), K63: (63, 2), K64: (64, 2), HOLES: (0, 41), CLEAN: (12, 8)}
        left = rest - sum(a + b for a, b in c.values())
        c[WIDE] = (left - left // 10 - 1, left // 10 + 1)
        return c
    if n == 1:
        return {WIDE: (1, 0)}
    c = {ONE: (1, 3), HOLES: (0, 5), CLEAN: (4, 2), K63: (n // 4, 2)}
    left = n - sum(a + b for a, b in c.values())
    c[WIDE] = (left - 3, 3)
    return c


def _log_uniform(rng, k, lo=-3.0, hi=3.0):
    return (10.0 ** rng.uniform(lo, hi, k)).astype(np.float32)


def _layout(vidx, oor, layout, rng):
    """an order of the points 0 .. n-1 (vidx: their slots, oor: the out-of-range points, kept out of the runs)"""
    n = len(vidx)
    inr = np.setdiff1d(np.arange(n), oor)
    runs = [inr[vidx[inr] == s] for s in SLOTS_WITH_POINTS if (vidx[inr] == s).any()]
    if layout == "interleaved":
        order = [r[k] for k in range(max(len(r) for r in runs)) for r in runs if k < len(r)]
        for m, p in enumerate(oor):                               # spread through the order
            order.insert((m + 1) * len(order) // (len(oor) + 1), p)
        return np.array(order)
    order = []
    for m, r in enumerate(runs):                                  # the out-of-range points sit between the runs
        order += list(r) + ([oor[m]] if m < len(oor) else [])
    order = np.array(order + list(oor[len(runs):]), dtype=np.int64)
    if layout == "runs":
        return order
    cuts, at = [], 0
    while at < n:
        step = int(rng.integers(1, 101))
        cuts.append(order[at:at + step])
        at += step
    return np.concatenate([cuts[k] for k in rng.permutation(len(cuts))])


def deform_scene(n, layout="runs", seed=None):
    """-> dict(poses [B,7], disps_up [B,H,W], valid [B,H,W], dirty [B], vidx, pj, pi [n] int64, prev [n] f32,
    ids [n] (the point held at each position: the layouts of one n are permutations of the same points),
    unit [..] / oor [4] (point ids of the prev == 1 hole points and of the out-of-range points), K, H, W, B)"""
    assert layout in LAYOUTS
    rng = np.random.default_rng(1000 + n if seed is None else seed)
    H, W, B = H_DEFORM, W_DEFORM, B_DEFORM
    poses = np.stack([general_pose(rng) for _ in range(B)])
    depth_map = _log_uniform(rng, B * H * W).reshape(B, H, W)
    valid = rng.uniform(size=(B, H, W)) > 0.3
    vidx, pj, pi, prev, unit = [], [], [], [], []
    for s, (n_valid, n_holes) in sorted(_counts(n).items()):
        k = n_valid + n_holes
        px = rng.permutation(H * W)[:k]
        j, i = px // W, px % W
        has = np.arange(k) < n_valid
        valid[s, j, i] = has
        p = _log_uniform(rng, k)
        if s in (K63, K64):                                         # a narrow band at a level of its own
            p[has] = (10.0 ** rng.uniform(-2.5, 2.5) * rng.uniform(1.0, 1.25, n_valid)).astype(np.float32)
        # the new depth of a point that has one is its previous depth times 0.7 .. 1.4, as an update of the tracker
        # leaves it: the two sums of the scale are then of one size (the premise test_deform_scenes.py checks)
        depth_map[s, j[has], i[has]] = p[has] * rng.uniform(0.7, 1.4, n_valid).astype(np.float32)
        if DIRTY[s] and n_holes and n >= 63:
            p[n_valid] = 1.0
            unit.append(len(vidx) + n_valid)
        vidx += [s] * k
        pj += list(j)
        pi += list(i)
        prev += list(p)
    oor = []
    if n >= 257:                                                    # one index out of range each, the others in WIDE
        for bad in ((-1, 3, 5), (B, 4, 6), (WIDE, H, 7), (WIDE, 8, -1)):
            oor.append(len(vidx))
            vidx.append(bad[0]), pj.append(bad[1]), pi.append(bad[2]), prev.append(float(_log_uniform(rng, 1)[0]))
    assert len(vidx) == n, (len(vidx), n)
    vidx, pj, pi = (np.array(x, np.int64) for x in (vidx, pj, pi))
    prev, oor = np.array(prev, np.float32), np.array(oor, np.int64)
    order = _layout(vidx, oor, layout, np.random.default_rng(7))
    assert np.array_equal(np.sort(order), np.arange(n))
    return dict(poses=poses, disps_up=(np.float32(1) / depth_map).astype(np.float32), valid=valid, dirty=DIRTY.copy(),
                vidx=vidx[order], pj=pj[order], pi=pi[order], prev=prev[order], ids=order, unit=np.array(unit, np.int64),
                oor=oor, K=INTRINSICS[(H, W)], H=H, W=W, B=B, n=n, layout=layout)


def in_range(c):
    """[n] bool: the points whose three indices are in range"""
    return (c["vidx"] >= 0) & (c["vidx"] < c["B"]) & (c["pj"] >= 0) & (c["pj"] < c["H"]) & (c["pi"] >= 0) & (c["pi"] < c["W"])


def ref_indices(c):
    """(vidx, pj, pi) for the restatement, which indexes with them: the out-of-range points belong to no keyframe"""
    ok = in_range(c)
    return np.where(ok, c["vidx"], -1), np.where(ok, c["pj"], 0), np.where(ok, c["pi"], 0)


def moved(c):
    """[n] bool: the points the kernel re-places (indices in range, keyframe dirty)"""
    ok = in_range(c)
    ok[ok] = c["dirty"][c["vidx"][ok]]
    return ok


def frame_terms(c, v):
    """(prev, d) float32 of the points of keyframe v that enter its scale, d = 1.0f / disps_up as the kernel reads it;
    and [n] bool: the moved points of v on holes"""
    mine = moved(c) & (c["vidx"] == v)
    j, i = c["pj"][mine], c["pi"][mine]
    has = c["valid"][v, j, i]
    d = np.float32(1) / c["disps_up"][v, j[has], i[has]]
    holes = mine.copy()
    holes[mine] = ~has
    return c["prev"][mine][has], d, holes


def exact_scale(prev, d):
    """sum(prev d) / sum(prev^2) as a Fraction over the float32 inputs; None without a term"""
    F = fractions.Fraction
    den = sum(F(float(p)) ** 2 for p in prev)
    return sum(F(float(p)) * F(float(x)) for p, x in zip(prev, d)) / den if den else None


def integer_scale(prev, d):
    """The quotient of the two integer sums deform_scale_kernel documents, carried out exactly: every term times 2^e,
    e = 61 - (largest binary exponent of a term) - (bit length of the count), rounded to the nearest integer (ties to
    even, as llrint).  -> (Fraction, bit length, the larger of the two sums)"""
    F = fractions.Fraction
    pd = [F(float(p)) * F(float(x)) for p, x in zip(prev, d)]
    pp = [F(float(p)) ** 2 for p in prev]
    top = max(math.frexp(float(t))[1] for t in pd + pp)
    bits = len(pd).bit_length()
    e = 61 - top - bits
    a, b = (sum(round(t * F(2) ** e) for t in ts) for ts in (pd, pp))
    return F(a, b), bits, max(a, b)


def sequential_f32_scale(prev, d):
    a = b = np.float32(0)
    for p, x in zip(prev, d):
        a, b = a + p * x, b + p * p
    return a / b


def f32_neighbours(q):
    """the two float32 values that enclose the Fraction q (equal when q is a float32)"""
    x = np.float32(float(q))
    if fractions.Fraction(float(x)) == q:
        return x, x
    lo = x if fractions.Fraction(float(x)) < q else np.nextafter(x, np.float32(-np.inf))
    return lo, np.nextafter(lo, np.float32(np.inf))


# ---- z-buffer --------------------------------------------------------------------------------------------------------
def _camera(R, t):
    c = np.eye(4)
    c[:3, :3], c[:3, 3] = R, t
    return c


def zbuf_scene(H, W, counter, seed=None):
    """-> dict(full_pcl [M,H,W,3] f32, full_mask [M,H,W] bool, counter, M = counter + 1, c2w / w2c [4,4] f32 (w2c: the
    float64 inverse of the rounded c2w, rounded once: what the C entry points are given and what the restatement reads),
    K, H, W, cleared (the share of set bits cleared for firmness), planted, mid_row).  Map `counter` lies behind the maps that are
    read: points 0.2 in front of the view camera with their bits set, the nearest of the scene had they been read.

    planted (counter >= 1), name -> dict(index: positions in the flattened maps, pixel: (row, column) of the view the
    point aims at, depth):
      behind                       aimed at a pixel from behind the camera
      left, right, above, below    2.5 px beyond a border
      u_neg, v_neg                 u = -0.5 / v = -0.5, nearer (0.3) than anything else in the scene
      dup                          one point stored twice
      pair_nf, pair_fn             two points in one pixel, 0.6 and 0.9 away: the nearer stored first / the farther first
                                   (with three maps pair_fn and the second dup lie in map 1)
      masked                       the nearest point of its pixel (0.4) with its bit clear, then the winner (0.7)
      inf, nan                     a non-finite coordinate, bit set
      row_first, row_last          the nearest point of its pixel (0.5), stored in row 0 / row H - 1 of map 0
    Ordinary points are at least 1 away."""
    rng = np.random.default_rng(100 * H + counter if seed is None else seed)
    K = ZK[(H, W)]
    G, centre = general_rotation(rng), rng.uniform(0.2, 1.0, 3) * rng.choice([-1.0, 1.0], 3)
    c2w = _camera(G, centre).astype(np.float32)
    w2c = np.linalg.inv(c2w.astype(np.float64)).astype(np.float32)
    view = c2w.astype(np.float64)
    M = counter + 1
    pcl = np.zeros((M, H, W, 3), np.float32)
    jj, ii = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")

    def aim(u, v, depth, cam=view):
        dc = pixel_dirs(np.atleast_1d(np.float64(u)), np.atleast_1d(np.float64(v)), K) * np.atleast_1d(depth)[:, None]
        return (cam[:3, 3] + dc @ cam[:3, :3].T).astype(np.float32)

    for m in range(counter):
        cam = _camera(G @ rotation(rng.standard_normal(3), rng.uniform(-0.15, 0.15)), centre + rng.uniform(-0.1, 0.1, 3))
        pcl[m] = aim((ii + rng.uniform(0.05, 0.95, (H, W))).ravel(), (jj + rng.uniform(0.05, 0.95, (H, W))).ravel(),
                     rng.uniform(1.5, 4.0, H * W), cam).reshape(H, W, 3)
    pcl[counter] = aim((ii + 0.5).ravel(), (jj + 0.5).ravel(), np.full(H * W, 0.2)).reshape(H, W, 3)
    mask = rng.uniform(size=(M, H, W)) < 0.85
    mask[counter] = True
    planted = {}
    if counter:
        flat, fmask = pcl.reshape(-1, 3), mask.reshape(-1)
        slots = list(W + rng.permutation((H - 2) * W)[:20])        # rows 0 and H - 1 are row_first's and row_last's
        second = (H * W if counter >= 3 else 0)                     # where pair_fn and the second dup are stored
        targets = [(int(p) // (W - 2) + 1, int(p) % (W - 2) + 1) for p in rng.permutation((H - 2) * (W - 2))[:14]]
        frac = lambda: float(rng.uniform(0.25, 0.75))

        def plant(name, pts, bits=True, base=0):
            pts = np.atleast_2d(pts)
            idx = sorted(int(slots.pop()) for _ in pts)
            idx = [k + base for k in idx]
            bits = [bits] * len(idx) if isinstance(bits, bool) else bits
            for k, p, b in zip(idx, pts, bits):
                flat[k], fmask[k] = p, b
            return idx

        def entry(name, pixel, uv, depths, bits=True, base=0):
            pts = np.concatenate([aim(uv[0], uv[1], d) for d in depths])
            planted[name] = dict(index=plant(name, pts, bits, base), pixel=pixel, depth=list(depths))

        r, c = targets.pop()
        entry("behind", (r, c), (c + frac(), r + frac()), [-1.5])
        mid_r, mid_c = H // 2, W // 2
        entry("left", (mid_r, 0), (-2.5, mid_r + frac()), [0.5])
        entry("right", (mid_r, W - 1), (W + 2.5, mid_r + frac()), [0.5])
        entry("above", (0, mid_c), (mid_c + frac(), -2.5), [0.5])
        entry("below", (H - 1, mid_c), (mid_c + frac(), H + 2.5), [0.5])
        r, c = targets.pop()
        entry("u_neg", (r, 0), (-0.5, r + frac()), [0.3])
        entry("v_neg", (0, c), (c + frac(), -0.5), [0.3])
        r, c = targets.pop()
        uv = (c + frac(), r + frac())
        entry("dup", (r, c), uv, [0.8])
        planted["dup"]["index"] += plant("dup", aim(uv[0], uv[1], 0.8), True, second)
        r, c = targets.pop()
        entry("pair_nf", (r, c), (c + frac(), r + frac()), [0.6, 0.9])
        r, c = targets.pop()
        entry("pair_fn", (r, c), (c + frac(), r + frac()), [0.9, 0.6], base=second)
        r, c = targets.pop()
        entry("masked", (r, c), (c + frac(), r + frac()), [0.4, 0.7], bits=[False, True])
        r, c = targets.pop()
        bad = aim(c + frac(), r + frac(), 0.5)
        planted["inf"] = dict(index=plant("inf", bad * np.float32([np.inf, 1, 1])), pixel=(r, c), depth=[0.5])
        planted["nan"] = dict(index=plant("nan", bad * np.float32([1, np.nan, 1])), pixel=(r, c), depth=[0.5])
        for name, row in (("row_first", 0), ("row_last", H - 1)):
            r, c = targets.pop()
            slots.append(row * W + int(rng.integers(0, W)))
            entry(name, (r, c), (c + frac(), r + frac()), [0.5])
    # firmness: float64 on the rounded inputs
    X = pcl[:counter].reshape(-1, 3).astype(np.float64)
    w = w2c.astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        Xc = X @ w[:3, :3].T + w[:3, 3]
        z = Xc[:, 2] + 1e-6
        u, v = (-K[0] * Xc[:, 0] + K[2] * Xc[:, 2]) / z, (K[1] * Xc[:, 1] + K[3] * Xc[:, 2]) / z
        near = lambda x, n: (np.abs(x - np.round(x)) < DELTA) & (x > -1 - DELTA) & (x < n + 1 + DELTA)
        soft = near(u, W) | near(v, H) | (np.abs(z) < Z_MIN)
    before = mask[:counter].reshape(-1).copy()
    mask[:counter].reshape(-1)[soft] = False
    cleared = float((before & soft).sum() / max(before.sum(), 1))
    # the middle row the tests leave out: the one that stores pair_nf's nearer point
    mid_row = planted["pair_nf"]["index"][0] // W if counter else H // 2
    return dict(full_pcl=pcl, full_mask=mask, counter=counter, M=M, c2w=c2w, w2c=w2c, K=K, H=H, W=W, cleared=cleared,
                planted=planted, mid_row=mid_row)


ZBUF_SCENES = [(H, W, counter) for H, W in ZK for counter in (0, 1, 3)]


def border_scene():
    """identity pose, fx = 32, fy = 16, cx = 16, cy = 8 at 16 x 32: points whose u or v is exactly (minus) zero in
    float32 and in float64 (the numerator fx (-a) + cx c cancels exactly), which lie inside the image, beside ordinary
    ones.  -> dict as zbuf_scene's with one map; planted "u_zero" (row 5, column 0) and "v_zero" (row 0, column 9)"""
    H, W, K = 16, 32, (32.0, 16.0, 16.0, 8.0)
    pcl = np.zeros((1, H, W, 3), np.float32)
    jj, ii = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    pcl[0] = (pixel_dirs(ii + 0.5, jj + 0.5, K) * 4.0).astype(np.float32)
    pcl[0, 3, 3] = pixel_dirs(np.float64(0.0), np.float64(5.5), K) * 2.0          # u = 0: a = cx c / fx = -1
    pcl[0, 3, 4] = pixel_dirs(np.float64(9.5), np.float64(0.0), K) * 2.0          # v = 0
    planted = dict(u_zero=dict(index=[3 * W + 3], pixel=(5, 0), depth=[2.0]),
                   v_zero=dict(index=[3 * W + 4], pixel=(0, 9), depth=[2.0]))
    return dict(full_pcl=pcl, full_mask=np.ones((1, H, W), bool), counter=1, M=1, c2w=np.eye(4, dtype=np.float32),
                w2c=np.eye(4, dtype=np.float32), K=K, H=H, W=W, cleared=0.0, planted=planted, mid_row=8)
