"""The claims of tests/recon_ref.py itself (no GPU): the numpy restatement of the mesh evaluation that test_gpu_recon.py and
test_gpu_eval_recon.py hold the kernels to, and that the inputs those tests use keep the reference inside their caps."""
import numpy as np
import pytest

import recon_ref as R
import tsdf_ref

MAX_UNFIRM = 0.02                 # share of a scene's pixels whose depth may hang on the rounding of an edge test
FACTOR = 4.0                      # the yardstick of the GPU tests: error <= 4 x that of the float32 numpy composition
uniforms = R.uniforms


def test_samples_lie_in_their_triangles():
    v, f = R.sampling_mesh()
    u = uniforms(4099)
    p, face, near = R.sample_surface(v, f, u)
    tri = v.astype(np.float64)[f[face]]
    e1, e2, d = tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0], p - tri[:, 0]
    n = np.cross(e1, e2)
    scale = np.linalg.norm(e1, axis=1) * np.linalg.norm(e2, axis=1) * np.maximum(np.linalg.norm(d, axis=1), 1e-30)
    assert (np.abs(np.einsum("ij,ij->i", n, d)) <= 1e-12 * scale + 1e-300).all(), "in the plane"
    # barycentric coordinates from the normal equations
    g11, g12, g22 = (e1 * e1).sum(1), (e1 * e2).sum(1), (e2 * e2).sum(1)
    r1, r2 = (d * e1).sum(1), (d * e2).sum(1)
    det = g11 * g22 - g12 * g12
    a, b = (g22 * r1 - g12 * r2) / det, (g11 * r2 - g12 * r1) / det
    assert (a >= -1e-9).all() and (b >= -1e-9).all() and (a + b <= 1 + 1e-9).all(), "inside"
    assert not (face == 12).any(), "the face without area is never drawn"
    assert not near.any(), "the fixed seed puts no draw within 1e-12 of a CDF entry"
    for n_small in (1, 255):
        assert not R.sample_surface(v, f, uniforms(n_small))[2].any()


@pytest.mark.parametrize("n", R.SAMPLE_SIZES)
def test_sampling_yardstick_admits_one_rounding(n):
    """the best a float32 output can do is the float64 point rounded once; the draws of the GPU test are such that this
    is inside FACTOR x the error of the float32 composition (for a single draw that is not a matter of course)"""
    v, f = R.sampling_mesh()
    u = uniforms(n)
    p64, face, _ = R.sample_surface(v, f, u)
    best = np.abs(p64.astype(np.float32).astype(np.float64) - p64).max()
    e32 = np.abs(R.barycentric_points(v, f, face, u, np.float32).astype(np.float64) - p64).max()
    print(f"n {n}: one rounding {best:.3e}, float32 composition {e32:.3e}")
    assert best <= FACTOR * e32


def test_face_frequencies_follow_the_areas():
    v, f = R.sampling_mesh()
    n = 200000
    _, face, _ = R.sample_surface(v, f, uniforms(n, 7))
    areas = R.face_areas(v, f)
    p = areas / areas.sum()
    counts = np.bincount(face, minlength=len(f))
    sigma = np.sqrt(n * p * (1 - p))
    print("largest deviation in sigmas", (np.abs(counts - n * p) / np.maximum(sigma, 1e-30))[sigma > 0].max())
    assert (np.abs(counts - n * p) <= 5 * sigma + 1).all()
    assert counts[12] == 0 and areas[12] == 0
    assert np.isclose(areas[14] / areas[13], 1e6, rtol=1e-3)


def test_fine_sphere_against_the_analytic_depth():
    """a sphere of 96 x 48 facets is inscribed: a facet spans at most pi / 48 of arc, so it sags by at most r (1 - cos(pi /
    48)) below the sphere, and along a ray that meets the surface at an angle with cosine >= 0.5 by twice that"""
    r, stacks, slices = 0.3, 48, 96
    v, f = R.uv_sphere(r, stacks, slices)
    H, W, K = 30, 40, (38.0, 38.0, 19.5, 14.5)
    c2w = tsdf_ref.look_at((0.7, 0.5, 0.4), (0.01, 0.0, -0.01))
    depth = R.rasterise(v, f, np.linalg.inv(c2w), K, H, W)
    exact, _ = tsdf_ref.sphere_depth(c2w, K, H, W, r)
    exact = exact.astype(np.float64)
    vv, uu = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    ray = np.stack([(uu - K[2]) / K[0], (vv - K[3]) / K[1], np.ones_like(uu)], -1) @ c2w[:3, :3].T
    hit = c2w[:3, 3] + ray * exact[..., None]
    cosine = -(hit * ray).sum(-1) / (np.linalg.norm(hit, axis=-1) * np.linalg.norm(ray, axis=-1))
    steep = (exact > 0) & (cosine >= 0.5)
    assert steep.sum() > 100 and np.isfinite(depth[steep]).all()
    sag = r * (1 - np.cos(np.pi / stacks))
    err = np.abs(depth - exact)[steep] / np.linalg.norm(ray, axis=-1)[steep]
    print("fine sphere: depth error", err.max(), "allowed", 2 * sag + 1e-6)
    assert err.max() <= 2 * sag + 1e-6                   # 1e-6: the fp32 rounding of sphere_depth and of the vertices
    assert (depth[steep] >= exact[steep] - 1e-6).all(), "an inscribed mesh is never in front of the sphere"


def test_icp_returns_a_known_motion():
    sv, _ = R.uv_sphere()
    gv, _ = R.grid_mesh(16)
    src = np.concatenate([sv, gv + np.float32(0.1)])
    M = R.rigid((0.3, -0.5, 0.8), 2.0, (0.012, -0.01, 0.0125))
    assert np.isclose(np.linalg.norm(M[:3, 3]), 0.02, atol=1e-4)
    tgt = R.transform_points(M, src).astype(np.float32)
    T, info = R.icp(src, tgt)
    print("icp:", info, "difference from the motion", np.abs(T - M).max())
    assert info["fitness"] == 1.0 and info["iterations"] < 30
    assert np.abs(T - M).max() <= 1e-6                   # the fp32 rounding of the target, 6e-8 x 0.4, through a well-posed fit
    T32, _ = R.icp(src, tgt, round_f32=True)
    assert np.abs(T32 - M).max() <= 1e-6


def test_accuracy_of_a_shifted_sphere():
    """every point of a sphere shifted by delta is ||p| - r| from the sphere, whose mean over the sphere is delta / 2.  The
    mesh is inscribed (sag r (1 - cos(pi / 48))), and the nearest of n samples of density rho = n / area is farther than
    the surface by less than the distance to it within the surface, 1 / (2 sqrt(rho)) on average: twice that is allowed;
    the mean of n draws of spread <= delta is within 4 delta / sqrt(12 n)"""
    r, delta, n = 0.3, 0.05, 20000
    v, f = R.uv_sphere(r, 48, 96)
    gt, _, _ = R.sample_surface(v, f, uniforms(n, 3))
    rec, _, _ = R.sample_surface(v + np.float32([delta, 0, 0]), f, uniforms(n, 4))
    acc = R.accuracy(gt, rec)
    sag = r * (1 - np.cos(np.pi / 48))
    spacing = 1.0 / np.sqrt(n / R.face_areas(v, f).sum())
    mc = 4 * delta / np.sqrt(12 * n)
    print("accuracy", acc, "closed form", delta / 2, "allowed -", sag + mc, "+", sag + spacing + mc)
    assert delta / 2 - sag - mc <= acc <= delta / 2 + sag + spacing + mc


def test_bruteforce_equals_kdtree():
    rng = np.random.default_rng(5)
    pts = rng.uniform(0, 1, (3000, 3)).astype(np.float32)
    q = rng.uniform(-5, 6, (1000, 3)).astype(np.float32)
    d_b, i_b = R.nn_bruteforce(q, pts)
    d_k, i_k = R.nn_kdtree(q, pts)
    assert np.array_equal(i_b, i_k)
    np.testing.assert_allclose(d_b, d_k, rtol=1e-14)


def test_moments_give_the_kabsch_step():
    rng = np.random.default_rng(9)
    p = rng.normal(size=(50, 3)).astype(np.float32)
    M = R.rigid((1.0, 2.0, -1.0), 11.0, (0.3, -0.2, 0.1))
    q = R.transform_points(M, p).astype(np.float32)
    mom, _ = R.icp_moments(p, q, np.arange(50), np.zeros(50, np.float32), 1.0)
    assert mom[0] == 50 and mom[16] > 0
    np.testing.assert_allclose(R.kabsch_from_moments(mom), M, atol=1e-6)


@pytest.mark.parametrize("scene", R.raster_scenes(), ids=lambda s: s[0])
def test_raster_scenes_are_firm(scene):
    name, v, f, w2c, expected = scene
    grown, shrunk, exact, firm = R.firm_depth(v, f, w2c, R.RASTER_K, R.RASTER_H, R.RASTER_W, R.RASTER_NEAR, R.RASTER_FAR)
    share = 1.0 - firm.mean()
    covered = np.isfinite(exact).sum()
    print(f"{name}: {covered} covered pixels of {firm.size}, share that is not firm {share:.4f}")
    assert share <= MAX_UNFIRM
    assert (grown <= exact).all() and (exact <= shrunk).all()
    if expected == "none":
        assert covered == 0 and not np.isfinite(grown).any()
    else:
        assert covered > 60
    if name.startswith("wall"):
        cam = v.astype(np.float64) @ w2c[:3, :3].T + w2c[:3, 3]
        behind = cam[f][:, :, 2] <= R.RASTER_NEAR
        assert (behind.any(1) & ~behind.all(1)).all(), "both triangles cross the near plane: what is covered was clipped"
    if name == "grid":
        box = np.argwhere(np.isfinite(exact))
        size = box.max(0) - box.min(0) + 1
        print("grid: pixel box", size)
        assert (size >= 15).all() and (size <= 26).all()
        inner = exact[box[:, 0].min() + 2:box[:, 0].max() - 1, box[:, 1].min() + 2:box[:, 1].max() - 1]
        assert np.isfinite(inner).all(), "shared edges leave no holes"


def test_numpy_pipeline_is_within_a_voxel_on_the_sphere_scene():
    """the fused sphere of tsdf_ref.sphere_scene() (voxel 0.02) against the UV sphere of radius 0.3: the accuracy of 5,000
    samples is at most one voxel"""
    K, voxel, trunc, bound = tsdf_ref.SCENE_K, tsdf_ref.SCENE_VOXEL, tsdf_ref.SCENE_TRUNC, tsdf_ref.SCENE_BOUND
    origin, nb = tsdf_ref.block_grid((-bound,) * 3, (bound,) * 3, voxel)
    vol = tsdf_ref.new_volume(origin, nb, voxel)
    for depth, color, c2w in tsdf_ref.sphere_scene():
        vol["alloc"] |= tsdf_ref.allocate(depth, c2w, K, origin, nb, voxel, trunc, 30.0)[0]
        tsdf_ref.integrate(vol, depth, color, c2w, K, trunc, 30.0)
    rv, _, rf = tsdf_ref.extract(vol)
    assert len(rf) > 1000
    gv, gf = R.uv_sphere()
    rec, _, _ = R.sample_surface(rv.astype(np.float32), rf, uniforms(5000, 21))
    gt, _, _ = R.sample_surface(gv, gf, uniforms(5000, 22))
    acc = R.accuracy(gt, rec)
    print("numpy pipeline: accuracy", acc, "voxel", voxel)
    assert acc <= voxel
