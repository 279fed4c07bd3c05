"""The numpy float64 restatement of the mesh-culling rules of include/glorie_hip.h (glorie_mesh_visibility,
glorie_mesh_select_faces, glorie_mesh_compact_*, glorie_mesh_components) and the scenes the tests run them on.

The restatement forms every number in float64 from the float32 inputs, one operation at a time in the order the header
writes, so that only the order of operations inside one expression could separate it from the kernels; a vertex whose
decision in a view hangs on the last bits (`unfirm`) is reported and left out by the tests.

`mutate` switches one deliberate mistake on; tests/test_cull_ref.py shows that every one of them changes a result on the
scenes, i.e. that the scenes would catch it in the kernels.
"""
import numpy as np

# the classes of (view, vertex): what the rule decided and why
SEEN, BEHIND, BEYOND, LEFT, RIGHT, TOP, BOTTOM, OCCLUDED, HOLE = range(9)
CLASS_NAMES = ("seen", "behind", "beyond z_far", "left of the border", "right of the border", "above the border",
               "below the border", "occluded", "depth hole")
FIRM_REL = 1e-9


def project(vertices, w2c):
    """p = ((R0 x + R1 y) + R2 z) + t per row, float64 from the float32 inputs -> px, py, pz [V]"""
    X = np.asarray(vertices, np.float32).astype(np.float64)
    w = np.asarray(w2c, np.float32).astype(np.float64)
    x, y, z = X[:, 0], X[:, 1], X[:, 2]
    return tuple(((w[a, 0] * x + w[a, 1] * y) + w[a, 2] * z) + w[a, 3] for a in range(3))


def visibility_classes(vertices, w2cs, K, H, W, depths=None, eps=0.03, edge=0, z_near=0.01, z_far=30.0,
                       depth_missing_sees=False, mutate=None):
    """-> (cls int8 [M,V] one of the classes above, sees bool [M,V], unfirm bool [M,V]).  w2cs float32 [M,4,4]; K =
    (fx, fy, cx, cy); depths: None or M maps [H,W] (an entry None: frustum only for that view)"""
    fx, fy, cx, cy = (float(np.float32(k)) for k in K)
    z_near, z_far, eps = float(np.float32(z_near)), float(np.float32(z_far)), float(np.float32(eps))
    M, V = len(w2cs), len(vertices)
    cls = np.zeros((M, V), np.int8)
    sees = np.zeros((M, V), bool)
    unfirm = np.zeros((M, V), bool)
    near = lambda a, b: np.abs(a - b) <= FIRM_REL * np.maximum(np.abs(a), np.abs(b))
    for m in range(M):
        px, py, pz = project(vertices, w2cs[m])
        with np.errstate(divide="ignore", invalid="ignore"):
            u = fx * px / pz + cx
            v = fy * py / pz + cy
        if mutate == "floor":
            ui, vi = np.floor(u), np.floor(v)
        else:
            ui, vi = np.floor(u + 0.5), np.floor(v + 0.5)
        lo = edge + 1 if mutate == "edge" else edge
        c = np.full(V, SEEN, np.int8)
        # the last assignment wins: the order below is the reverse of the rule's order of tests
        c[vi >= H - edge] = BOTTOM
        c[vi < lo] = TOP
        c[ui >= W - edge] = RIGHT
        c[ui < lo] = LEFT
        c[~np.isfinite(u) | ~np.isfinite(v)] = LEFT
        c[pz > z_far] = BEYOND
        c[~(pz > z_near)] = BEHIND
        inside = c == SEEN
        uf = unfirm[m]
        front = pz > z_near
        uf |= near(pz, z_near) | near(pz, z_far)
        with np.errstate(invalid="ignore"):
            for t in (u, v):
                frac = np.abs((t + 0.5) - np.rint(t + 0.5))
                uf |= front & (pz <= z_far) & (frac <= FIRM_REL * np.maximum(1.0, np.abs(t)))
        if depths is not None and depths[m] is not None:
            dm = np.asarray(depths[m], np.float32).astype(np.float64)
            idx = np.nonzero(inside)[0]
            d = dm[vi[idx].astype(np.int64), ui[idx].astype(np.int64)]
            hole = ~(d > 0.0)
            bound = d - eps if mutate == "eps" else d + eps
            occluded = ~hole & ~(pz[idx] <= bound)
            c[idx[occluded]] = OCCLUDED
            c[idx[hole]] = HOLE
            uf[idx[~hole]] |= near(pz[idx[~hole]], (d + eps)[~hole])
        cls[m] = c
        hole_sees = bool(depth_missing_sees) or mutate == "hole"
        sees[m] = (c == SEEN) | ((c == HOLE) & hole_sees)
    return cls, sees, unfirm


def visibility(vertices, w2cs, K, H, W, **kw):
    """-> (count int32 [V], unfirm bool [V]: the vertex is unfirm in some view)"""
    _, sees, unfirm = visibility_classes(vertices, w2cs, K, H, W, **kw)
    return sees.sum(0).astype(np.int32), unfirm.any(0)


def valid_faces(faces, V):
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    return ((f >= 0) & (f < V)).all(1)


def select_faces(faces, count, min_views=1, rule="all", mutate=None):
    """keep_face uint8 [F]"""
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    ok = valid_faces(f, len(count))
    seen = np.zeros(f.shape, bool)
    seen[ok] = np.asarray(count)[f[ok]] >= min_views
    if mutate == "rule":
        rule = "any" if rule == "all" else "all"
    keep = seen.all(1) if rule == "all" else seen.any(1)
    return (keep & ok).astype(np.uint8)


def compact(vertices, faces, keep_face, colors=None, mutate=None):
    """-> (vertices', faces' int32, colors' or None)"""
    vertices = np.asarray(vertices)
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    V = len(vertices)
    keep = (np.asarray(keep_face) != 0) & valid_faces(f, V)
    used = np.zeros(V, bool)
    used[f[keep].reshape(-1)] = True
    if mutate == "keepvertex" and not used.all():
        used[np.nonzero(~used)[0][0]] = True
    new_index = np.cumsum(used) - 1
    out_f = new_index[f[keep]].astype(np.int32).reshape(-1, 3)
    return vertices[used], out_f, (None if colors is None else np.asarray(colors)[used])


def components(faces, V, mutate=None):
    """-> (label int32 [V] = the smallest vertex index of the component, faces_of int32 [V] = the valid faces of the
    component at its label vertex).  A plain union-find with path compression"""
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    ok = valid_faces(f, V)
    parent = list(range(V))

    def find(x):
        r = x
        while parent[r] != r:
            r = parent[r]
        while parent[x] != r:
            parent[x], x = r, parent[x]
        return r

    def union(a, b):
        a, b = find(a), find(b)
        if a != b:
            lo, hi = (a, b) if (a < b) != (mutate == "maxlabel") else (b, a)
            parent[hi] = lo
    for a, b, c in f[ok].tolist():
        union(a, b)
        union(b, c)
    label = np.array([find(i) for i in range(V)], np.int32)
    faces_of = np.zeros(V, np.int32)
    np.add.at(faces_of, label[f[ok][:, 0]], 1)
    return label, faces_of


def component_mask(faces, label, faces_of, min_faces=0, keep_largest=False):
    """keep_face uint8 [F] of glorie_mesh_components"""
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    ok = valid_faces(f, len(label))
    lab = np.zeros(len(f), np.int64)
    lab[ok] = label[f[ok][:, 0]]
    keep = ok & (faces_of[lab] >= min_faces)
    if keep_largest:
        top = int(faces_of.max())
        best = int(np.nonzero(faces_of == top)[0][0]) if top > 0 else -1       # ties: the lower label
        keep &= lab == best
    return keep.astype(np.uint8)


# ---- scenes ----------------------------------------------------------------------------------------------------------------
ROOM = np.array([2.0, 1.5, 1.1])                       # half extents of the 4 x 3 x 2.2 m room
K = (41.3, 37.9, 25.2, 18.7)
H, W = 37, 53
EPS = 0.03
Z_FAR = 3.2                                            # shorter than the room's diagonal: some vertices lie beyond it


def _grid(origin, e1, e2, n1, n2):
    """a rectangle origin + a e1 + b e2 as (n1 x n2) cells with their own vertices -> (vertices [(n1+1)(n2+1),3], faces)"""
    a, b = np.meshgrid(np.arange(n1 + 1) / n1, np.arange(n2 + 1) / n2, indexing="ij")
    v = origin[None] + a.reshape(-1, 1) * e1[None] + b.reshape(-1, 1) * e2[None]
    idx = lambda i, j: i * (n2 + 1) + j
    f = [t for i in range(n1) for j in range(n2)
         for t in ((idx(i, j), idx(i + 1, j), idx(i + 1, j + 1)), (idx(i, j), idx(i + 1, j + 1), idx(i, j + 1)))]
    return v, np.array(f, np.int64)


def room_rectangles():
    """the six walls and the slab as (origin, e1, e2)"""
    x, y, z = ROOM
    o = lambda *p: np.array(p, np.float64)
    walls = [(o(-x, -y, -z), o(0, 2 * y, 0), o(0, 0, 2 * z)), (o(x, -y, -z), o(0, 2 * y, 0), o(0, 0, 2 * z)),
             (o(-x, -y, -z), o(2 * x, 0, 0), o(0, 0, 2 * z)), (o(-x, y, -z), o(2 * x, 0, 0), o(0, 0, 2 * z)),
             (o(-x, -y, -z), o(2 * x, 0, 0), o(0, 2 * y, 0)), (o(-x, -y, z), o(2 * x, 0, 0), o(0, 2 * y, 0))]
    slab = (o(0.6, -0.9, -0.7), o(0.25, 1.4, 0.0), o(0.0, 0.0, 1.0))
    return walls + [slab]


def room_mesh(walls=13, slab=(7, 5)):
    """-> (vertices f32 [1224,3], faces int32 [2098,3]): 7 components, the walls of 338 faces and the slab of 70"""
    vs, fs, base = [], [], 0
    rects = room_rectangles()
    for k, (o, e1, e2) in enumerate(rects):
        n1, n2 = (walls, walls) if k < 6 else slab
        v, f = _grid(o, e1, e2, n1, n2)
        vs.append(v)
        fs.append(f + base)
        base += len(v)
    return np.concatenate(vs).astype(np.float32), np.concatenate(fs).astype(np.int32)


def look_at(eye, target, roll=0.0, up=(0.0, 0.0, 1.0)):
    """OpenCV camera-to-world float64 [4,4]: z towards the target, y down, rolled about z"""
    eye, target = np.asarray(eye, np.float64), np.asarray(target, np.float64)
    z = target - eye
    z /= np.linalg.norm(z)
    x = np.cross(z, np.asarray(up, np.float64))
    x /= np.linalg.norm(x)
    y = np.cross(z, x)
    c, s = np.cos(roll), np.sin(roll)
    c2w = np.eye(4)
    c2w[:3, 0], c2w[:3, 1], c2w[:3, 2], c2w[:3, 3] = c * x + s * y, -s * x + c * y, z, eye
    return c2w


# (eye, target, roll) of the five cameras
CAMERAS = [((-1.31, -0.62, 0.13), (1.9, 0.41, -0.23), 0.11), ((-0.87, 0.93, -0.37), (1.7, -1.1, 0.52), -0.23),
           ((1.43, 0.21, 0.44), (-1.8, -0.73, -0.61), 0.31), ((-1.52, 0.05, -0.58), (0.9, 0.37, 0.85), -0.07),
           ((0.11, -1.07, 0.29), (1.2, 1.4, -0.33), 0.19)]


def room_cameras():
    """five general cameras inside the room -> c2ws float64 [5,4,4]"""
    return np.stack([look_at(e, t, r) for e, t, r in CAMERAS])


def jittered_cameras(n, seed=5):
    """n cameras: the five of room_cameras with jittered eyes, targets and rolls -> c2ws float64 [n,4,4]"""
    rng = np.random.default_rng(seed)
    out = []
    for i in range(n):
        e, t, r = CAMERAS[i % 5]
        out.append(look_at(np.array(e) + rng.uniform(-0.15, 0.15, 3), np.array(t) + rng.uniform(-0.4, 0.4, 3),
                           r + rng.uniform(-0.2, 0.2)))
    return np.stack(out)


def w2cs_of(c2ws):
    """what cull_mesh.vertex_visibility hands to the kernel: the float64 inverses rounded to float32"""
    return np.linalg.inv(np.asarray(c2ws, np.float64)).astype(np.float32)


def ray_cast_depth(c2w, rectangles=None):
    """the exact depth map float32 [H,W] of the rectangles from the camera: the smallest camera-frame z > 0 per pixel"""
    rectangles = room_rectangles() if rectangles is None else rectangles
    fx, fy, cx, cy = K
    u, v = np.meshgrid(np.arange(W, dtype=np.float64), np.arange(H, dtype=np.float64))
    d_cam = np.stack([(u - cx) / fx, (v - cy) / fy, np.ones_like(u)], -1)
    d = d_cam @ c2w[:3, :3].T
    eye = c2w[:3, 3]
    depth = np.full((H, W), np.inf)
    for o, e1, e2 in rectangles:
        n = np.cross(e1, e2)
        with np.errstate(divide="ignore", invalid="ignore"):
            t = (n @ (o - eye)) / (d @ n)
            hit = eye + t[..., None] * d - o
            a, b = hit @ e1 / (e1 @ e1), hit @ e2 / (e2 @ e2)
            ok = (t > 0) & (a >= 0) & (a <= 1) & (b >= 0) & (b <= 1)
        depth = np.where(ok & (t < depth), t, depth)
    return np.where(np.isfinite(depth), depth, 0.0).astype(np.float32)


HOLE_VIEW, HOLE_ROWS, HOLE_COLS = 0, slice(9, 21), slice(14, 31)


def room_depths(c2ws, hole=True):
    """the ray-cast maps of the views; with `hole` a rectangle of zeros is planted in the map of view HOLE_VIEW"""
    maps = [ray_cast_depth(c) for c in c2ws]
    if hole:
        maps[HOLE_VIEW][HOLE_ROWS, HOLE_COLS] = 0.0
    return maps


def room_scene(n_views=5):
    """the scene of the visibility tests -> dict(vertices, faces, c2ws, w2cs, depths, K, H, W, eps, z_far)"""
    v, f = room_mesh()
    c2ws = room_cameras() if n_views == 5 else jittered_cameras(n_views)
    return {"vertices": v, "faces": f, "c2ws": c2ws, "w2cs": w2cs_of(c2ws), "depths": room_depths(c2ws), "K": K, "H": H,
            "W": W, "eps": EPS, "z_far": Z_FAR, "z_near": 0.01}


SCENES = {"room5": lambda: room_scene(5), "room70": lambda: room_scene(70)}


def floaters(base_vertices, n_triangles=4, n_quads=3, seed=2):
    """single triangles and two-triangle quads of their own vertices, indexed after `base_vertices` vertices -> (vertices
    f32, faces int32, the number of faces added)"""
    rng = np.random.default_rng(seed)
    vs, fs, base = [], [], base_vertices
    for _ in range(n_triangles):
        vs.append(rng.uniform(-1, 1, (3, 3)))
        fs.append([base, base + 1, base + 2])
        base += 3
    for _ in range(n_quads):
        vs.append(rng.uniform(-1, 1, (4, 3)))
        fs += [[base, base + 1, base + 2], [base, base + 2, base + 3]]
        base += 4
    return np.concatenate(vs).astype(np.float32), np.array(fs, np.int32), len(fs)


def strip_mesh(n_triangles=3000, seed=3):
    """one strip of n triangles over n + 2 vertices whose numbering is a fixed random permutation with the smallest index
    in the middle of the strip: labels have to travel half the strip in both directions"""
    rng = np.random.default_rng(seed)
    n_v = n_triangles + 2
    perm = rng.permutation(n_v)
    mid = n_v // 2
    j = int(np.nonzero(perm == 0)[0][0])
    perm[[mid, j]] = perm[[j, mid]]
    pos = np.stack([np.arange(n_v) * 0.01, (np.arange(n_v) % 2) * 0.01, np.zeros(n_v)], 1)
    vertices = np.zeros((n_v, 3), np.float32)
    vertices[perm] = pos
    faces = np.stack([perm[:-2], perm[1:-1], perm[2:]], 1).astype(np.int32)
    return vertices, faces
