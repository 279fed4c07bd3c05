"""Numpy restatement of the block-sparse TSDF volume of glorie_slam_amd/tsdf.py (csrc/tsdf.hip): the block grid, the
allocation of one frame as a block set, the voxel update and marching tetrahedra on the Kuhn split with the canonical
output order.  float64 unless a dtype is given; the volume is held densely over the whole block grid with a boolean array
of allocated blocks, which is what the kernels' block table and pool describe.

Conventions (the contract of the kernels):
  grid      origin = bounds_min, blocks per axis = ceil((bounds_max - bounds_min) / (8 voxel_length)); the linear table
            index of block (bx, by, bz) is (bz * nby + by) * nbx + bx; arrays are indexed [z, y, x]
  voxel     (i, j, k) samples origin + (i + 0.5, j + 0.5, k + 0.5) * voxel_length
  camera    OpenCV pinhole, K = (fx, fy, cx, cy), c2w rigid; pixel (u, v) is centred on (u, v)
"""
import itertools

import numpy as np

BLOCK = 8
SLOTS = (1, 2, 4, 3, 5, 6, 7)                       # corner reached by the owned edge of a slot
SLOT_OF = {d: s for s, d in enumerate(SLOTS)}
ORDERS = tuple(itertools.permutations((1, 2, 4)))   # the six tetrahedra (0, a, a|b, 7)


def _bits(c):
    return c & 1, (c >> 1) & 1, (c >> 2) & 1


def _parity(p):
    p, s = list(p), 1
    for i in range(len(p)):
        while p[i] != i:
            j = p[i]
            p[i], p[j] = p[j], p[i]
            s = -s
    return s


def order_sign(order):
    """orientation of the tetrahedron (0, a, a|b, 7): the sign of the permutation (a, b, c) of the axes"""
    return _parity([{1: 0, 2: 1, 4: 2}[a] for a in order])


def tet_table():
    """inside mask (bit p: vertex p of the tetrahedron has tsdf < 0) -> triangles of a POSITIVELY oriented tetrahedron, each
    three edges (p, q), p < q, wound so that the normal points from the inside vertices to the outside ones; a negatively
    oriented tetrahedron swaps the last two vertices of every triangle"""
    even = {0: (0, 1, 2, 3), 1: (1, 0, 3, 2), 2: (2, 0, 1, 3), 3: (3, 0, 2, 1)}
    e = lambda p, q: (min(p, q), max(p, q))
    table = {0: [], 15: []}
    for i in range(4):
        _, j, k, l = even[i]
        table[1 << i] = [[e(i, j), e(i, k), e(i, l)]]
        table[15 ^ (1 << i)] = [[e(i, j), e(i, l), e(i, k)]]
    for i, j in itertools.combinations(range(4), 2):
        k, l = [m for m in range(4) if m not in (i, j)]
        if _parity([i, j, k, l]) < 0:
            k, l = l, k
        table[(1 << i) | (1 << j)] = [[e(i, k), e(i, l), e(j, l)], [e(i, k), e(j, l), e(j, k)]]
    return table


TET_TABLE = tet_table()


# ---- the grid --------------------------------------------------------------------------------------------------------
def block_grid(bounds_min, bounds_max, voxel_length):
    """-> (origin float64 [3], (nbx, nby, nbz)): the bound rounded outwards to whole blocks"""
    lo, hi = np.asarray(bounds_min, np.float64), np.asarray(bounds_max, np.float64)
    nb = np.maximum(1, np.ceil((hi - lo) / (BLOCK * float(voxel_length)) - 1e-6)).astype(np.int64)
    return lo, tuple(int(n) for n in nb)


def new_volume(origin, nb, voxel_length, dtype=np.float64):
    nbx, nby, nbz = nb
    shape = (nbz * BLOCK, nby * BLOCK, nbx * BLOCK)
    return {"tsdf": np.zeros(shape, dtype), "weight": np.zeros(shape, dtype), "rgb": np.zeros(shape + (3,), dtype),
            "alloc": np.zeros((nbz, nby, nbx), bool), "origin": np.asarray(origin, np.float64),
            "voxel_length": float(voxel_length)}


def backproject(depth, c2w, K, depth_trunc):
    """world points [n,3] of the pixels with 0 < depth <= depth_trunc"""
    fx, fy, cx, cy = K
    depth, c2w = np.asarray(depth, np.float64), np.asarray(c2w, np.float64)
    v, u = np.nonzero((depth > 0) & (depth <= depth_trunc))
    d = depth[v, u]
    cam = np.stack([(u - cx) / fx * d, (v - cy) / fy * d, d], 1)
    return cam @ c2w[:3, :3].T + c2w[:3, 3]


def allocate(depth, c2w, K, origin, nb, voxel_length, sdf_trunc, depth_trunc, half=None):
    """-> (bool [nbz,nby,nbx] of the blocks that overlap a pixel's box [p - half, p + half] (half = sdf_trunc unless
    given), the number of pixels whose box leaves the grid: those flag nothing)"""
    half = sdf_trunc if half is None else half
    p = backproject(depth, c2w, K, depth_trunc)
    size = BLOCK * voxel_length
    lo = np.floor((p - half - origin) / size).astype(np.int64)
    hi = np.floor((p + half - origin) / size).astype(np.int64)
    nbv = np.asarray(nb)
    inside = ((lo >= 0) & (hi < nbv)).all(1)
    flag = np.zeros((nb[2], nb[1], nb[0]), bool)
    for l, h in zip(lo[inside], hi[inside]):
        flag[l[2]:h[2] + 1, l[1]:h[1] + 1, l[0]:h[0] + 1] = True
    return flag, int((~inside).sum())


def integrate(vol, depth, color, c2w, K, sdf_trunc, depth_trunc, dtype=np.float64, borderline=False):
    """one frame into the allocated blocks of `vol` (in place), every operation in `dtype`.  With borderline also returns
    the voxels (bool, dense) whose accept / reject decisions or pixel choice hang on less than the margins of the GPU test:
    u_f or v_f within 1e-3 of an integer, |z| < 1e-4, |sdf + sdf_trunc| < 1e-4"""
    T = dtype
    fx, fy, cx, cy = (T(k) for k in K)
    depth, color = np.asarray(depth, T), np.asarray(color, T)
    c2w = np.asarray(c2w, T)
    H, W = depth.shape
    Z, Y, X = vol["tsdf"].shape
    vl, o = T(vol["voxel_length"]), vol["origin"].astype(T)
    xs = o[0] + (np.arange(X, dtype=T) + T(0.5)) * vl
    ys = o[1] + (np.arange(Y, dtype=T) + T(0.5)) * vl
    zs = o[2] + (np.arange(Z, dtype=T) + T(0.5)) * vl
    dz, dy, dx = np.meshgrid(zs - c2w[2, 3], ys - c2w[1, 3], xs - c2w[0, 3], indexing="ij")
    R = c2w[:3, :3]
    px = R[0, 0] * dx + R[1, 0] * dy + R[2, 0] * dz                  # p = R^T (X - t)
    py = R[0, 1] * dx + R[1, 1] * dy + R[2, 1] * dz
    pz = R[0, 2] * dx + R[1, 2] * dy + R[2, 2] * dz
    live = np.repeat(np.repeat(np.repeat(vol["alloc"], BLOCK, 0), BLOCK, 1), BLOCK, 2)
    front = live & (pz > 0)
    with np.errstate(divide="ignore", invalid="ignore"):
        u_f = fx * px / pz + cx + T(0.5)
        v_f = fy * py / pz + cy + T(0.5)
    eps = T(1e-4)
    inimg = front & (u_f >= eps) & (u_f < T(W) - eps) & (v_f >= eps) & (v_f < T(H) - eps)
    u = np.where(inimg, u_f, 0).astype(np.int64)
    v = np.where(inimg, v_f, 0).astype(np.int64)
    d = depth[v, u]
    seen = inimg & (d > 0) & (d <= T(depth_trunc))
    mult = np.sqrt(T(1) + ((u.astype(T) - cx) / fx) ** 2 + ((v.astype(T) - cy) / fy) ** 2)
    sdf = (d - pz) * mult
    trunc = T(sdf_trunc)
    upd = seen & ~(sdf <= -trunc)
    new = np.minimum(T(1), sdf / trunc)
    w = vol["weight"]
    vol["tsdf"][upd] = ((vol["tsdf"] * w + new) / (w + T(1)))[upd]
    c = np.floor(np.clip(color[v, u], T(0), T(1)) * T(255))
    vol["rgb"][upd] = ((vol["rgb"] * w[..., None] + c) / (w[..., None] + T(1)))[upd]
    w[upd] += T(1)
    if not borderline:
        return None
    with np.errstate(invalid="ignore"):
        near_int = lambda a: np.abs(a - np.round(a)) < 1e-3
        edge = live & (np.abs(pz) < 1e-4)
        edge |= front & (u_f > -1) & (u_f < W + 1) & (v_f > -1) & (v_f < H + 1) & (near_int(u_f) | near_int(v_f))
        edge |= seen & (np.abs(sdf + trunc) < 1e-4)
    return edge


# ---- extraction -----------------------------------------------------------------------------------------------------
def _shift(a, c, fill):
    """a[k + dz, j + dy, i + dx] for corner c, `fill` past the end"""
    dx, dy, dz = _bits(c)
    out = np.full(a.shape, fill, a.dtype)
    Z, Y, X = a.shape[:3]
    out[:Z - dz, :Y - dy, :X - dx] = a[dz:, dy:, dx:]
    return out


def cell_valid(vol):
    """[Z,Y,X] bool: all 8 corners of the cell are allocated with weight > 0"""
    ok = np.repeat(np.repeat(np.repeat(vol["alloc"], BLOCK, 0), BLOCK, 1), BLOCK, 2) & (vol["weight"] > 0)
    cv = ok.copy()
    for c in range(1, 8):
        cv &= _shift(ok, c, False)
    return cv


def cell_keys(shape):
    """[Z,Y,X] int64: block table index * 512 + cell index in the block (x fastest)"""
    Z, Y, X = shape
    k, j, i = np.meshgrid(np.arange(Z), np.arange(Y), np.arange(X), indexing="ij")
    blk = ((k // BLOCK) * (Y // BLOCK) + j // BLOCK) * (X // BLOCK) + i // BLOCK
    return blk * 512 + (k % BLOCK) * 64 + (j % BLOCK) * 8 + i % BLOCK


def extract(vol, details=False):
    """-> vertices float64 [V,3], colours float64 [V,3] in [0,1], faces int64 [F,3] in the canonical order; with details
    also {"vertex_key": cell key * 7 + slot of every vertex, "face_key": cell key * 12 + 2 tetrahedron + triangle}"""
    tsdf = np.asarray(vol["tsdf"], np.float64)
    rgb = np.asarray(vol["rgb"], np.float64)
    Z, Y, X = tsdf.shape
    inside = tsdf < 0
    cv = cell_valid(vol)
    cvp = np.zeros((Z + 1, Y + 1, X + 1), bool)
    cvp[1:, 1:, 1:] = cv
    keys = cell_keys(tsdf.shape)
    emit = np.zeros((7, Z, Y, X), bool)
    for s, d in enumerate(SLOTS):
        used = np.zeros((Z, Y, X), bool)
        for o in range(8):
            if o & d == 0:
                ox, oy, oz = _bits(o)
                used |= cvp[1 - oz:1 - oz + Z, 1 - oy:1 - oy + Y, 1 - ox:1 - ox + X]
        emit[s] = used & (inside != _shift(inside, d, False))
    s_i, k_i, j_i, i_i = np.nonzero(emit)
    vkey = keys[k_i, j_i, i_i] * 7 + s_i
    order = np.argsort(vkey, kind="stable")
    s_i, k_i, j_i, i_i, vkey = s_i[order], k_i[order], j_i[order], i_i[order], vkey[order]
    vid = np.full((7, Z, Y, X), -1, np.int64)
    vid[s_i, k_i, j_i, i_i] = np.arange(len(vkey))
    d = np.array(SLOTS)[s_i]
    dxyz = np.stack([d & 1, (d >> 1) & 1, (d >> 2) & 1], 1)
    ta = tsdf[k_i, j_i, i_i]
    tb = tsdf[k_i + dxyz[:, 2], j_i + dxyz[:, 1], i_i + dxyz[:, 0]]
    t = ta / (ta - tb)
    g = np.stack([i_i, j_i, k_i], 1).astype(np.float64)
    verts = vol["origin"] + vol["voxel_length"] * (g + 0.5 + t[:, None] * dxyz)
    ca = rgb[k_i, j_i, i_i]
    cb = rgb[k_i + dxyz[:, 2], j_i + dxyz[:, 1], i_i + dxyz[:, 0]]
    cols = (ca + t[:, None] * (cb - ca)) / 255.0
    faces, fkeys = [], []
    kc, jc, ic = np.nonzero(cv)
    ckey = keys[kc, jc, ic]
    for q, (a, b, _) in enumerate(ORDERS):
        corners = (0, a, a | b, 7)
        sign = order_sign(ORDERS[q])
        m = np.zeros(len(kc), np.int64)
        for p, c in enumerate(corners):
            cx, cy, cz = _bits(c)
            m |= inside[kc + cz, jc + cy, ic + cx].astype(np.int64) << p
        for mask in range(1, 15):
            sel = np.nonzero(m == mask)[0]
            if not len(sel):
                continue
            for n_tri, tri in enumerate(TET_TABLE[mask]):
                ids = []
                for p, r in tri:
                    cx, cy, cz = _bits(corners[p])
                    slot = SLOT_OF[corners[r] & ~corners[p]]
                    ids.append(vid[slot, kc[sel] + cz, jc[sel] + cy, ic[sel] + cx])
                if sign < 0:
                    ids[1], ids[2] = ids[2], ids[1]
                faces.append(np.stack(ids, 1))
                fkeys.append(ckey[sel] * 12 + 2 * q + n_tri)
    if faces:
        faces, fkeys = np.concatenate(faces), np.concatenate(fkeys)
        order = np.argsort(fkeys, kind="stable")
        faces, fkeys = faces[order], fkeys[order]
    else:
        faces, fkeys = np.zeros((0, 3), np.int64), np.zeros(0, np.int64)
    assert (faces >= 0).all(), "a face of a valid cell uses an edge without a vertex"
    if details:
        return verts, cols, faces, {"vertex_key": vkey, "face_key": fkeys}
    return verts, cols, faces


# ---- mesh facts ------------------------------------------------------------------------------------------------------
def mesh_facts(verts, faces):
    """V, E, F, the Euler characteristic, how many faces every undirected edge has (min, max), whether every directed edge
    appears exactly once, the number of boundary edges (one face only) and the signed volume"""
    e = np.concatenate([faces[:, [0, 1]], faces[:, [1, 2]], faces[:, [2, 0]]])
    und, counts = (np.unique(np.sort(e, 1), axis=0, return_counts=True) if len(e) else
                   (np.zeros((0, 2), np.int64), np.zeros(0, np.int64)))
    directed_once = len(np.unique(e, axis=0)) == len(e) if len(e) else True
    a, b, c = (verts[faces[:, i]] for i in range(3)) if len(faces) else (np.zeros((0, 3)),) * 3
    volume = float(np.einsum("ij,ij->i", a, np.cross(b, c)).sum() / 6.0)
    V, E, F = len(verts), len(und), len(faces)
    return {"V": V, "E": E, "F": F, "euler": V - E + F, "faces_per_edge": (int(counts.min()), int(counts.max())) if E else (0, 0),
            "directed_once": bool(directed_once), "boundary_edges": int((counts == 1).sum()), "volume": volume}


def crossing_counts(face_key, nb):
    """faces by the number of axes (0..3) in which their cell is the last of its block with a neighbouring block behind
    it: such a cell reads its corners across a block face (1), a block edge (2) or a block corner (3)"""
    nbx, nby, nbz = nb
    cell, blk = (face_key // 12) % 512, face_key // (12 * 512)
    bx, by, bz = blk % nbx, (blk // nbx) % nby, blk // (nbx * nby)
    n = (((cell % 8 == 7) & (bx < nbx - 1)).astype(np.int64) + (((cell // 8) % 8 == 7) & (by < nby - 1))
         + ((cell // 64 == 7) & (bz < nbz - 1)))
    return np.bincount(n, minlength=4)


def dense_volume(tsdf, weight=None, rgb=None, origin=(0.0, 0.0, 0.0), voxel_length=1.0):
    """a volume of a dense grid [Z,Y,X] (sides multiples of 8): blocks exist where any weight in them is positive"""
    tsdf = np.asarray(tsdf, np.float64)
    Z, Y, X = tsdf.shape
    assert Z % BLOCK == 0 and Y % BLOCK == 0 and X % BLOCK == 0
    vol = new_volume(origin, (X // BLOCK, Y // BLOCK, Z // BLOCK), voxel_length)
    vol["tsdf"][:] = tsdf
    vol["weight"][:] = 1.0 if weight is None else weight
    if rgb is not None:
        vol["rgb"][:] = rgb
    w = vol["weight"].reshape(Z // BLOCK, BLOCK, Y // BLOCK, BLOCK, X // BLOCK, BLOCK)
    vol["alloc"][:] = (w > 0).any(axis=(1, 3, 5))
    return vol


# ---- the fields of the extraction tests (24^3 voxels over [-0.5, 0.5]^3) ---------------------------------------------
N = 24


def field_points(n=N):
    c = (np.arange(n) + 0.5) / n - 0.5
    return np.meshgrid(c, c, c, indexing="ij")                    # z, y, x


def sphere_field(radius=0.3, centre=(0.0, 0.0, 0.0), n=N):
    z, y, x = field_points(n)
    return np.sqrt((x - centre[0]) ** 2 + (y - centre[1]) ** 2 + (z - centre[2]) ** 2) - radius


def torus_field(R=0.3, r=0.12, n=N):
    z, y, x = field_points(n)
    return np.sqrt((np.sqrt(x * x + y * y) - R) ** 2 + z * z) - r


def two_spheres_field(n=N):
    return np.minimum(sphere_field(0.15, (-0.22, 0.0, 0.0), n), sphere_field(0.15, (0.22, 0.0, 0.0), n))


def zero_corner_field(n=N):
    """the sphere with the corner values closest to the surface forced to exactly 0 (576 of them)"""
    f = sphere_field(n=n)
    idx = np.argsort(np.abs(f), axis=None, kind="stable")[:576]
    f.reshape(-1)[idx] = 0.0
    return f


def pocket_weight(n=N):
    """weight 1 with a 3 x 3 x 3 pocket of weight 0 on the sphere's surface (around +x)"""
    w = np.ones((n, n, n))
    w[11:14, 11:14, 18:21] = 0.0
    return w


def colour_field(n=N):
    z, y, x = field_points(n)
    return np.stack([(x + 0.5) * 255.0, (y + 0.5) * 255.0, (z + 0.5) * 255.0], -1)


def field_volume(tsdf, weight=None, rgb=None):
    n = tsdf.shape[0]
    return dense_volume(tsdf, weight, colour_field(n) if rgb is None else rgb, origin=(-0.5, -0.5, -0.5), voxel_length=1.0 / n)


# ---- scene S of the GPU tests: a sphere seen by 8 cameras ------------------------------------------------------------
def look_at(eye, target=(0.0, 0.0, 0.0)):
    """camera-to-world of an OpenCV camera (x right, y down, z forward) at `eye` looking at `target`"""
    eye, target = np.asarray(eye, np.float64), np.asarray(target, np.float64)
    z = target - eye
    z /= np.linalg.norm(z)
    up = np.array([0.0, 0.0, 1.0]) if abs(z[2]) < 0.9 else np.array([0.0, 1.0, 0.0])
    x = np.cross(z, up)
    x /= np.linalg.norm(x)
    y = np.cross(z, x)
    c2w = np.eye(4)
    c2w[:3, 0], c2w[:3, 1], c2w[:3, 2], c2w[:3, 3] = x, y, z, eye
    return c2w


def sphere_depth(c2w, K, H, W, radius=0.3):
    """exact z-depth of the sphere of `radius` at the origin, 0 off the sphere; colour = a smooth function of the hit point"""
    fx, fy, cx, cy = K
    v, u = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    ray = np.stack([(u - cx) / fx, (v - cy) / fy, np.ones_like(u)], -1) @ c2w[:3, :3].T      # z component 1 in the camera
    o = c2w[:3, 3]
    a = (ray * ray).sum(-1)
    b = 2.0 * (ray @ o)
    c = o @ o - radius * radius
    disc = b * b - 4 * a * c
    hit = disc > 0
    s = np.where(hit, (-b - np.sqrt(np.where(hit, disc, 0.0))) / (2 * a), 0.0)
    hit &= s > 0
    depth = np.where(hit, s, 0.0)
    p = o + ray * s[..., None]
    color = np.where(hit[..., None], 0.5 + 0.5 * np.sin(7.0 * p + np.array([0.0, 1.0, 2.0])), 0.0)
    return depth.astype(np.float32), color.astype(np.float32)


SCENE_H, SCENE_W, SCENE_K = 48, 64, (60.0, 60.0, 31.5, 23.5)
SCENE_BOUND, SCENE_VOXEL, SCENE_TRUNC = 0.48, 0.02, 0.08


def sphere_scene():
    """8 cameras at distance about 1 along the six axes and two oblique directions, each nudged by a few millimetres:
    [(depth f32 [48,64], color f32 [48,64,3], c2w float64 [4,4])]"""
    dirs = [(1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1), (1, 1, 1), (-1, 1, -1)]
    rng = np.random.default_rng(11)
    frames = []
    for d in dirs:
        eye = np.asarray(d, np.float64) / np.linalg.norm(d) + rng.uniform(-4e-3, 4e-3, 3)
        c2w = look_at(eye, rng.uniform(-4e-3, 4e-3, 3))
        depth, color = sphere_depth(c2w, SCENE_K, SCENE_H, SCENE_W)
        frames.append((depth, color, c2w))
    return frames
