"""numpy float64 restatement of the probe march of glorie_ray_samples_near (include/glorie_hip.h): probe depths, the
distance from every probe to its nearest cloud point, occupancy, bracket and z-values, and the firmness precondition
under which the fp32 kernel must take the same decisions.

Probe k of n sits at depth float32(linspace(near, far, n)[k]) (float64 linspace, far = the float32 the kernel reads) and
at position o + dir * z_k; it is occupied iff its nearest cloud point is closer than r (d2 < r2, r2 = float32(r) squared
in float32).  A ray with two occupied probes is bracketed by the first two: z = float32(linspace(lo, hi, S)) of their
float64 depths; any other ray is invalid and spans linspace(near, far, S).

Firmness: the kernel forms the probe position and the squared distance in float32, which moves d2 by about 1e-5 * r2 at
the coordinates of the box scene (|x| <= 3.2, r = 0.08: an ulp of a coordinate is 2.4e-7, d2' ~ 2 r * 3 ulp = 1.1e-7
against r2 = 6.4e-3).  A ray is firm if no probe has |d2_min - r2| <= 1e-3 * r2 - two orders of margin; only firm rays
are compared exactly."""
import numpy as np

NEAR = 0.3
RADIUS = 0.08
FIRM_REL = 1e-3
N_RAYS = 64 * 11 + 9
N_MISS = 7
# (far, n): the reference's 25 probes at two far ends, one chunk exactly, one probe past a chunk, three chunks, brackets
# that cross a chunk boundary, first hits in the second and third chunk (chunk = 64 probes)
CASES = ((6.0, 25), (float(np.float32(3.6)), 25), (6.0, 64), (6.0, 65), (6.0, 130), (5.0, 160), (6.0, 300))
MAX_NON_FIRM_SHARE = 0.03

_SCENE = {}


def scene():
    """the 120 000-point box cloud and the first 713 rays of its 24 x 32 view, the first 7 turned away from the cloud
    -> dict(cloud [N,3] f32, rays_o [R,3] f32, rays_d [R,3] f32, depth [R] f32, radius [R] f32, c2w [4,4] f32)"""
    if not _SCENE:
        import glorie_slam_amd.synth as synth
        cloud, geo, col = synth.box_cloud(n_hits=40000)
        ro, rd, depth, radius, c2w = synth.box_rays(24, 32, fx=16.0, fy=16.0, cx=15.5, cy=11.5)
        ro, rd = ro[:N_RAYS].copy(), rd[:N_RAYS].copy()
        rd[:N_MISS] = np.array([0.0, 0.0, 1e-3], np.float32)
        _SCENE.update(cloud=cloud, geo=geo, col=col, rays_o=ro, rays_d=rd, depth=depth[:N_RAYS].copy(),
                      radius=radius[:N_RAYS].copy(), c2w=c2w)
    return _SCENE


def probe_depths(near, far, n):
    """float64 depths of the n probes (the bracket ends) and their float32 roundings (where the probes sit)"""
    z64 = np.linspace(float(near), float(np.float32(far)), int(n))
    return z64, z64.astype(np.float32)


def probe_points(rays_o, rays_d, z32):
    """[R,n,3] float64 positions o + dir * z of the probes"""
    o, d = rays_o.astype(np.float64), rays_d.astype(np.float64)
    return o[:, None, :] + d[:, None, :] * z32.astype(np.float64)[None, :, None]


_TREES = {}


def nearest_d2(cloud, pts):
    """squared distance from every point of pts [..., 3] to its nearest cloud point, float64 (inf for an empty cloud)"""
    if cloud.shape[0] == 0:
        return np.full(pts.shape[:-1], np.inf)
    key = (cloud.shape[0], float(cloud.astype(np.float64).sum()))
    if key not in _TREES:
        from scipy.spatial import cKDTree
        _TREES[key] = cKDTree(cloud.astype(np.float64))
    d, _ = _TREES[key].query(pts.reshape(-1, 3), k=1)
    return (d * d).reshape(pts.shape[:-1])


def r2_of(radius):
    return float(np.float32(radius) * np.float32(radius))


_D2 = {}


def scene_march(far, n, S):
    """march() of the scene's rays (all of them marched), the nearest distances computed once per (far, n)"""
    sc = scene()
    key = (float(np.float32(far)), int(n))
    if key not in _D2:
        _D2[key] = nearest_d2(sc["cloud"], probe_points(sc["rays_o"], sc["rays_d"], probe_depths(NEAR, far, n)[1]))
    return march(sc["cloud"], sc["rays_o"], sc["rays_d"], NEAR, far, n, S, d2=_D2[key])


def march(cloud, rays_o, rays_d, near, far, n, S, radius=RADIUS, d2=None):
    """-> dict(bracket [R,2] int32, near_mask [R] bool, z [R,S] f32, lo / hi [R] f64, occ [R,n] bool, firm [R] bool,
    d2 [R,n] f64)"""
    z64, z32 = probe_depths(near, far, n)
    if d2 is None:
        d2 = nearest_d2(cloud, probe_points(rays_o, rays_d, z32))
    r2 = r2_of(radius)
    occ = d2 < r2
    firm = ~(np.abs(d2 - r2) <= FIRM_REL * r2).any(-1)
    R = rays_o.shape[0]
    bracket = np.full((R, 2), -1, np.int32)
    far64 = float(np.float32(far))
    lo, hi = np.full(R, float(near)), np.full(R, far64)
    for r in range(R):
        idx = np.flatnonzero(occ[r])
        if idx.size >= 1:
            bracket[r, 0] = idx[0]
        if idx.size >= 2:
            bracket[r, 1] = idx[1]
            lo[r], hi[r] = z64[idx[0]], z64[idx[1]]
    z = np.stack([np.linspace(lo[r], hi[r], S) for r in range(R)]).astype(np.float32) if R else np.zeros((0, S), np.float32)
    return dict(bracket=bracket, near_mask=bracket[:, 1] >= 0, z=z, lo=lo, hi=hi, occ=occ, firm=firm, d2=d2)


def crosses_chunk(bracket, chunk):
    """rays whose two bracket probes lie in different chunks of `chunk` probes"""
    b = bracket
    return (b[:, 1] >= 0) & (b[:, 0] // chunk != b[:, 1] // chunk)
