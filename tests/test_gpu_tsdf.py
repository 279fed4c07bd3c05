"""The TSDF kernels (csrc/tsdf.hip through glorie_slam_amd/tsdf.py) against the numpy restatement of tests/tsdf_ref.py:
allocation as a block set, the voxel update against float64 on the GPU's own blocks with the error of the float32 numpy
composition as the yardstick, marching tetrahedra face by face, determinism and the wrappers' argument checks.

Scene S: the sphere of radius 0.3 seen by 8 cameras of 64 x 48 pixels, bound [-0.48, 0.48]^3, voxel 0.02, truncation 0.08
(216 blocks in the table, about 35,000 touched voxels)."""
import numpy as np
import pytest
import torch

import tsdf_ref as R

pytestmark = pytest.mark.gpu

FACTOR = 4.0                      # GPU error against float64 <= 4 x the error of the float32 numpy composition
MAX_EXCLUDED = 0.05               # share of the touched voxels that may be borderline
BOX = 1e-4                        # the allocation is compared with boxes shrunk and grown by this


def _dev(a, gpu, dtype=torch.float32):
    return torch.from_numpy(np.ascontiguousarray(a)).to(gpu, dtype)


def _dense(vol):
    """the GPU volume as the dense dict of tsdf_ref (float64 copies of the fp32 voxels) and the block ids [nbz,nby,nbx]"""
    coords, tsdf, weight, rgb = (t.cpu().numpy() for t in vol.blocks())
    ref = R.new_volume(vol.origin, vol.blocks_per_axis, vol.voxel_length)
    for (bx, by, bz), t, w, c in zip(coords, tsdf, weight, rgb):
        sl = (slice(bz * 8, bz * 8 + 8), slice(by * 8, by * 8 + 8), slice(bx * 8, bx * 8 + 8))
        ref["tsdf"][sl], ref["weight"][sl], ref["rgb"][sl] = t, w, c
        ref["alloc"][bz, by, bx] = True
    return ref, vol.table.cpu().numpy()


def _fuse(gpu, frames, K, lo, hi, voxel, trunc, depth_trunc=30.0, max_blocks=400):
    """integrate the frames on the GPU; -> (volume, blocks in use after every frame)"""
    from glorie_slam_amd.tsdf import TSDFVolume
    vol = TSDFVolume(voxel, trunc, lo, hi, max_blocks, gpu, depth_trunc=depth_trunc)
    used = []
    for depth, color, c2w in frames:
        vol.integrate(_dev(depth, gpu), _dev(color, gpu), _dev(c2w, gpu), K)
        used.append(vol.n_blocks)
    torch.cuda.synchronize()
    return vol, used


def _check_fusion(gpu, frames, K, lo, hi, voxel, trunc, depth_trunc=30.0, tag=""):
    """allocation and integration of `frames` against the reference; -> (volume, dense GPU copy, float64 reference)"""
    # the kernels take fp32 poses: every side gets the rounded matrix
    frames = [(d, c, np.asarray(p, np.float32).astype(np.float64)) for d, c, p in frames]
    vol, used = _fuse(gpu, frames, K, lo, hi, voxel, trunc, depth_trunc)
    got, table = _dense(vol)
    origin, nb = R.block_grid(lo, hi, voxel)
    assert nb == vol.blocks_per_axis and table.shape == (nb[2], nb[1], nb[0])
    index = vol.block_index[:vol.n_blocks].cpu().numpy()
    assert np.array_equal(table.reshape(-1)[index], np.arange(vol.n_blocks)), "table and block_index are inverse"
    assert (table >= 0).sum() == vol.n_blocks
    ref64, ref32 = R.new_volume(origin, nb, voxel), R.new_volume(origin, nb, voxel, np.float32)
    edge = np.zeros(ref64["tsdf"].shape, bool)
    out_lo = out_hi = 0
    grown_all, shrunk_all = np.zeros_like(ref64["alloc"]), np.zeros_like(ref64["alloc"])
    for f, (depth, color, c2w) in enumerate(frames):
        first = used[f - 1] if f else 0
        have = (table >= 0) & (table < used[f])
        new = have & (table >= first)
        shrunk, o_lo = R.allocate(depth, c2w, K, origin, nb, voxel, trunc, depth_trunc, half=trunc - BOX)
        grown, o_hi = R.allocate(depth, c2w, K, origin, nb, voxel, trunc, depth_trunc, half=trunc + BOX)
        shrunk_all |= shrunk
        grown_all |= grown
        assert not (shrunk & ~have).any(), f"{tag} frame {f}: a block the frame needs is missing"
        assert not (new & ~grown).any(), f"{tag} frame {f}: a block the frame does not touch was allocated"
        assert (np.diff(index[first:used[f]]) > 0).all(), f"{tag} frame {f}: ids must ascend with the table index"
        out_lo, out_hi = out_lo + o_lo, out_hi + o_hi
        ref64["alloc"] = ref32["alloc"] = have
        edge |= R.integrate(ref64, depth, color, c2w, K, trunc, depth_trunc, borderline=True)
        R.integrate(ref32, depth, color, np.asarray(c2w, np.float32), K, trunc, depth_trunc, dtype=np.float32)
    assert not (shrunk_all & ~(table >= 0)).any() and not ((table >= 0) & ~grown_all).any()
    stats = vol.stats
    assert stats["blocks"] == vol.n_blocks == used[-1] and stats["frames"] == len(frames)
    assert out_lo <= stats["pixels_outside"] <= out_hi, (out_lo, stats["pixels_outside"], out_hi)
    touched = ref64["weight"] > 0
    share = (edge & touched).sum() / max(touched.sum(), 1)
    ok = ~edge
    err = lambda a, key: float(np.abs(np.asarray(a[key], np.float64) - ref64[key])[ok].max())
    e_t, e_c, f_t, f_c = err(got, "tsdf"), err(got, "rgb"), err(ref32, "tsdf"), err(ref32, "rgb")
    print(f"{tag}: {vol.n_blocks} blocks, {int(touched.sum())} touched voxels, excluded share {share:.4f}, "
          f"pixels outside {stats['pixels_outside']}; tsdf error gpu {e_t:.3e} / float32 numpy {f_t:.3e} = "
          f"{e_t / max(f_t, 1e-30):.3f}; rgb error gpu {e_c:.3e} / float32 numpy {f_c:.3e} = {e_c / max(f_c, 1e-30):.3f}")
    assert share <= MAX_EXCLUDED
    assert touched.sum() > 0
    assert np.array_equal(got["weight"][ok], ref64["weight"][ok]), f"{tag}: weights differ outside the borderline voxels"
    assert np.array_equal(ref32["weight"][ok], ref64["weight"][ok])
    assert e_t <= FACTOR * f_t and e_c <= FACTOR * f_c
    return vol, got, ref64


def _close_mesh(got, ref, voxel):
    """GPU mesh (device tensors) against the reference's (float64): faces equal as arrays, positions to 1e-6 of a voxel,
    colours to 1e-6"""
    v, c, f = (t.cpu().numpy() for t in got)
    rv, rc, rf = ref
    assert v.dtype == np.float32 and c.dtype == np.float32 and f.dtype == np.int32
    assert v.shape == rv.shape and c.shape == rc.shape and f.shape == rf.shape, (v.shape, rv.shape, f.shape, rf.shape)
    assert np.array_equal(f, rf)
    if len(v):
        e_v, e_c = np.abs(v - rv).max() / voxel, np.abs(c - rc).max()
        print(f"mesh V {len(v)} F {len(f)}: position error {e_v:.2e} voxels, colour error {e_c:.2e}")
        assert e_v <= 1e-6 and e_c <= 1e-6


S_LO, S_HI = (-R.SCENE_BOUND,) * 3, (R.SCENE_BOUND,) * 3


@pytest.fixture(scope="module")
def scene():
    return R.sphere_scene()


@pytest.fixture(scope="module")
def fused(gpu, scene):
    return _check_fusion(gpu, scene, R.SCENE_K, S_LO, S_HI, R.SCENE_VOXEL, R.SCENE_TRUNC, tag="scene S")


def test_scene_allocation_and_integration(fused):
    vol, got, ref = fused
    assert vol.table.numel() == 216
    assert 30000 < (ref["weight"] > 0).sum() < 40000


def test_scene_extraction(fused):
    vol, got, _ = fused
    rv, rc, rf, det = R.extract(got, details=True)
    mesh = vol.extract()
    _close_mesh(mesh, (rv, rc, rf), vol.voxel_length)
    facts = R.mesh_facts(rv, rf)
    print("scene S mesh", facts)
    assert facts["F"] > 1000 and facts["directed_once"]
    assert R.crossing_counts(det["face_key"], vol.blocks_per_axis)[1:3].min() > 0       # block faces and edges
    # the vertices lie as close to the sphere as the reference's own mesh of the same voxels
    worst = np.abs(np.linalg.norm(rv, axis=1) - 0.3).max()
    dist = np.abs(np.linalg.norm(mesh[0].double().cpu().numpy(), axis=1) - 0.3)
    print(f"distance of the vertices from the sphere: gpu {dist.max():.3e}, reference {worst:.3e}")
    assert dist.max() <= worst + 1e-5


def test_two_runs_are_bitwise_equal(gpu, scene, fused):
    vol, _, _ = fused
    again, _ = _fuse(gpu, scene, R.SCENE_K, S_LO, S_HI, R.SCENE_VOXEL, R.SCENE_TRUNC)
    assert again.n_blocks == vol.n_blocks and torch.equal(again.table, vol.table)
    for a, b in zip(again.blocks(), vol.blocks()):
        assert torch.equal(a, b)
    for a, b in zip(again.extract(), vol.extract()):
        assert torch.equal(a, b)


# ---- kernel edge cases: allocation and integration -------------------------------------------------------------------
def _tilted(H, W, K, base, slope, holes=True):
    """a depth image base + slope . (x, y) of the pixel's ray, with a band of zeros and a band beyond depth_trunc"""
    fx, fy, cx, cy = K
    v, u = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    depth = base + slope[0] * (u - cx) / fx + slope[1] * (v - cy) / fy
    color = np.stack([u / W, v / H, 0.5 + 0.4 * np.sin(0.3 * u + 0.2 * v)], -1)
    color[:2] = 1.7                                                 # clamped to 1
    color[2:4] = -0.3                                               # clamped to 0
    if holes:
        depth[5:9] = 0.0
        depth[:, 11:14] = 5.0                                       # beyond depth_trunc of the cases below
        depth[20, 20] = -1.0
    return depth.astype(np.float32), color.astype(np.float32)


def test_ragged_image_with_invalid_depths(gpu):
    H, W, K = 37, 53, (48.0, 47.0, 25.25, 17.875)
    frames = []
    for eye in ((0.02, -0.01, -0.55), (0.3, 0.05, -0.5)):
        c2w = R.look_at(eye, (0.0, 0.0, 0.1))
        depth, color = _tilted(H, W, K, 0.6, (0.1, -0.05))
        frames.append((depth, color, c2w))
    vol, got, ref = _check_fusion(gpu, frames, K, (-0.6, -0.5, -0.25), (0.6, 0.5, 0.45), 0.02, 0.06, depth_trunc=2.0,
                                  tag="ragged 53 x 37")
    assert (ref["weight"] == 2).any()


def test_camera_inside_the_bound(gpu):
    """two cameras back to back inside the bound: each one's surface lies behind the other, so on the third frame (the
    first camera again) allocated voxels have p.z <= 0 and keep their values"""
    H, W, K = 48, 64, R.SCENE_K
    # (nudged off the lattice's axes, like the cameras of scene S: an axis-aligned camera projects whole rows of voxels
    # onto pixel borders)
    a = R.look_at((0.003, -0.002, -0.05), (0.017, 0.011, 1.0))
    b = R.look_at((-0.004, 0.001, 0.05), (0.013, -0.019, -1.0))
    da, ca = _tilted(H, W, K, 0.3, (0.05, 0.02), holes=False)
    db, cb = _tilted(H, W, K, 0.28, (-0.03, 0.04), holes=False)
    frames = [(da, ca, a), (db, cb, b), (da, ca, a)]
    vol, got, ref = _check_fusion(gpu, frames, K, (-0.48, -0.4, -0.48), (0.48, 0.4, 0.48), 0.02, 0.06, tag="camera inside")
    z = vol.origin[2] + (np.arange(ref["weight"].shape[0]) + 0.5) * vol.voxel_length
    assert (ref["weight"][z < -0.06] == 1).any() and (ref["weight"][z > 0.06] == 2).any()
    assert vol.stats["blocks_visited"] < vol.n_blocks, "the blocks behind the camera are culled"


def test_blocks_on_the_faces_of_the_bound_and_pixels_outside(gpu, scene):
    """the bound [-0.40, 0.40]^3 still holds every box of the sphere (0.3 + 0.08 < 0.40) and its outermost blocks
    [0.24, 0.40] carry surface; with [-0.32, 0.32]^3 the boxes around the poles leave the bound and are counted"""
    vol, got, ref = _check_fusion(gpu, scene, R.SCENE_K, (-0.4,) * 3, (0.4,) * 3, R.SCENE_VOXEL, R.SCENE_TRUNC,
                                  tag="blocks on the faces")
    assert vol.blocks_per_axis == (5, 5, 5) and vol.stats["pixels_outside"] == 0
    coords = vol.blocks()[0].cpu().numpy()
    w = ref["weight"]
    for axis in range(3):
        assert coords[:, axis].min() == 0 and coords[:, axis].max() == 4
        assert (np.take(w, 0, axis) > 0).any() and (np.take(w, -1, axis) > 0).any(), "the outermost voxel layers are touched"
    vol, _, _ = _check_fusion(gpu, scene[:3], R.SCENE_K, (-0.32,) * 3, (0.32,) * 3, R.SCENE_VOXEL, R.SCENE_TRUNC,
                              tag="pixels outside")
    assert vol.stats["pixels_outside"] > 100


def test_a_frame_that_sees_nothing_changes_nothing(gpu, scene):
    vol, _ = _fuse(gpu, scene[:2], R.SCENE_K, S_LO, S_HI, R.SCENE_VOXEL, R.SCENE_TRUNC)
    before = [t.clone() for t in (vol.table, vol.block_index, vol.tsdf, vol.weight, vol.rgb)]
    n = vol.n_blocks
    depth, color, c2w = scene[2]
    blind = [np.zeros_like(depth), np.full_like(depth, 31.0)]       # nothing, and everything beyond depth_trunc
    away = R.look_at((0.0, 0.0, 5.0), (0.0, 0.0, 9.0))              # a valid image that looks away from the volume
    for d, pose in ((blind[0], c2w), (blind[1], c2w), (np.full_like(depth, 0.5), away)):
        vol.integrate(_dev(d, gpu), _dev(color, gpu), _dev(pose, gpu), R.SCENE_K)
    torch.cuda.synchronize()
    assert vol.n_blocks == n and vol.stats["frames"] == 5
    for a, b in zip(before, (vol.table, vol.block_index, vol.tsdf, vol.weight, vol.rgb)):
        assert torch.equal(a, b)
    assert vol.stats["pixels_outside"] == depth.size, "the pixels of the frame that looks away are all outside"


def test_pool_one_block_short(gpu, scene):
    from glorie_slam_amd._lib import GlorieError
    from glorie_slam_amd.tsdf import TSDFVolume
    full, used = _fuse(gpu, scene[:2], R.SCENE_K, S_LO, S_HI, R.SCENE_VOXEL, R.SCENE_TRUNC)
    need = used[1]
    assert used[0] < need
    vol = TSDFVolume(R.SCENE_VOXEL, R.SCENE_TRUNC, S_LO, S_HI, need - 1, gpu)
    args = [(_dev(d, gpu), _dev(c, gpu), _dev(p, gpu)) for d, c, p in scene[:2]]
    vol.integrate(*args[0], R.SCENE_K)
    before = [t.clone() for t in (vol.table, vol.block_index, vol.tsdf, vol.weight, vol.rgb)]
    with pytest.raises(GlorieError, match="GLORIE_ENOMEM"):
        vol.integrate(*args[1], R.SCENE_K)
    torch.cuda.synchronize()
    assert vol.n_blocks == used[0] == vol.stats["blocks"] and vol.stats["frames"] == 1
    for a, b in zip(before, (vol.table, vol.block_index, vol.tsdf, vol.weight, vol.rgb)):
        assert torch.equal(a, b)
    exact, used2 = _fuse(gpu, scene[:2], R.SCENE_K, S_LO, S_HI, R.SCENE_VOXEL, R.SCENE_TRUNC, max_blocks=need)
    assert used2 == used and torch.equal(exact.table, full.table)
    for a, b in zip(exact.blocks(), full.blocks()):
        assert torch.equal(a, b)


# ---- extraction through from_dense -----------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["sphere", "torus", "two_spheres", "zero_corners", "pocket", "empty"])
def test_extraction_of_dense_grids(gpu, name):
    from glorie_slam_amd.tsdf import TSDFVolume
    n = R.N
    field = {"sphere": R.sphere_field, "torus": R.torus_field, "two_spheres": R.two_spheres_field,
             "zero_corners": R.zero_corner_field, "pocket": R.sphere_field, "empty": R.sphere_field}[name]()
    weight = {"pocket": R.pocket_weight(), "empty": np.zeros((n,) * 3)}.get(name, np.ones((n,) * 3))
    # what the kernel reads is fp32: the reference gets the same values
    tsdf32, rgb32 = field.astype(np.float32), R.colour_field(n).astype(np.float32)
    ref = R.field_volume(tsdf32.astype(np.float64), weight, rgb32.astype(np.float64))
    rv, rc, rf, det = R.extract(ref, details=True)
    vol = TSDFVolume.from_dense(_dev(tsdf32, gpu), _dev(weight, gpu), _dev(rgb32, gpu), (-0.5,) * 3, 1.0 / n, 0.1)
    assert vol.blocks_per_axis == (3, 3, 3) and vol.n_blocks == (0 if name == "empty" else 27)
    _close_mesh(vol.extract(), (rv, rc, rf), 1.0 / n)
    facts = R.mesh_facts(rv, rf)
    expect = {"sphere": (2906, 5808, 2), "torus": (3716, 7432, 0), "two_spheres": (None, None, 4),
              "zero_corners": (None, None, 2), "pocket": (None, None, 1), "empty": (0, 0, 0)}[name]
    assert facts["euler"] == expect[2] and (expect[0] is None or (facts["V"], facts["F"]) == expect[:2])
    if name in ("sphere", "torus"):
        assert R.crossing_counts(det["face_key"], (3, 3, 3))[1:3].min() > 0
    if name == "sphere":
        assert R.crossing_counts(det["face_key"], (3, 3, 3))[3] > 0, "cells at a block corner carry faces"


def test_extraction_does_not_depend_on_the_allocation_order(gpu):
    """the same grid with its block ids permuted gives the same mesh; a ragged grid (20 x 17 x 13) is padded"""
    from glorie_slam_amd.tsdf import TSDFVolume
    n = R.N
    tsdf32, rgb32 = R.torus_field().astype(np.float32), R.colour_field(n).astype(np.float32)
    vol = TSDFVolume.from_dense(_dev(tsdf32, gpu), torch.ones(n, n, n, device=gpu), _dev(rgb32, gpu), (-0.5,) * 3, 1.0 / n, 0.1)
    mesh = vol.extract()
    perm = torch.randperm(27, generator=torch.Generator().manual_seed(1)).to(gpu)
    inv = torch.argsort(perm)
    vol.tsdf[:27], vol.weight[:27], vol.rgb[:27] = vol.tsdf[:27][inv].clone(), vol.weight[:27][inv].clone(), vol.rgb[:27][inv].clone()
    vol.table.view(-1)[:] = perm.to(torch.int32)
    vol.block_index[:27] = inv.to(torch.int32)
    for a, b in zip(vol.extract(), mesh):
        assert torch.equal(a, b)
    cut = (slice(0, 13), slice(0, 17), slice(0, 20))
    ref = R.field_volume(tsdf32.astype(np.float64), None, rgb32.astype(np.float64))
    ref["weight"][:] = 0.0
    ref["weight"][cut] = 1.0
    ragged = TSDFVolume.from_dense(_dev(tsdf32[cut], gpu), torch.ones(13, 17, 20, device=gpu), _dev(rgb32[cut], gpu),
                                   (-0.5,) * 3, 1.0 / n, 0.1)
    assert ragged.blocks_per_axis == (3, 3, 2)
    ref = {k: (v[:16] if k in ("tsdf", "weight", "rgb") else v) for k, v in ref.items()}
    ref["alloc"] = ref["alloc"][:2]
    _close_mesh(ragged.extract(), R.extract(ref), 1.0 / n)


def test_empty_volume_and_cpu_tensors(gpu, scene):
    from glorie_slam_amd._lib import GlorieError
    from glorie_slam_amd.tsdf import TSDFVolume, depth_bounds
    vol = TSDFVolume(R.SCENE_VOXEL, R.SCENE_TRUNC, S_LO, S_HI, 8, gpu)
    v, c, f = vol.extract()
    assert v.shape == (0, 3) and c.shape == (0, 3) and f.shape == (0, 3) and f.dtype == torch.int32
    assert vol.stats == {"blocks": 0, "pixels_outside": 0, "frames": 0, "blocks_visited": 0}
    depth, color, c2w = scene[0]
    cpu = [torch.from_numpy(depth), torch.from_numpy(color), torch.from_numpy(c2w).float()]
    for k in range(3):
        args = [t.to(gpu) for t in cpu]
        args[k] = cpu[k]
        with pytest.raises(GlorieError):
            vol.integrate(*args, R.SCENE_K)
    with pytest.raises(GlorieError):
        TSDFVolume(R.SCENE_VOXEL, R.SCENE_TRUNC, S_LO, S_HI, 8, "cpu")
    with pytest.raises(GlorieError):
        TSDFVolume.from_dense(torch.zeros(8, 8, 8), torch.ones(8, 8, 8), torch.zeros(8, 8, 8, 3), (0, 0, 0), 0.1, 0.3)
    assert vol.n_blocks == 0
    # depth_bounds encloses the sphere's visible surface; "opengl" negates columns 1 and 2 first
    lo, hi = depth_bounds([(d, p) for d, _, p in scene], R.SCENE_K, 0.1)
    assert (lo < -0.39).all() and (lo > -0.41).all() and (hi > 0.39).all() and (hi < 0.41).all()
    a = TSDFVolume(R.SCENE_VOXEL, R.SCENE_TRUNC, S_LO, S_HI, 200, gpu)
    b = TSDFVolume(R.SCENE_VOXEL, R.SCENE_TRUNC, S_LO, S_HI, 200, gpu)
    gl = c2w.copy()
    gl[:3, 1:3] *= -1
    a.integrate(_dev(depth, gpu), _dev(color, gpu), _dev(c2w, gpu), R.SCENE_K)
    b.integrate(_dev(depth, gpu), _dev(color, gpu), _dev(gl, gpu), torch.tensor(R.SCENE_K), convention="opengl")
    assert a.n_blocks == b.n_blocks > 0
    for x, y in zip(a.blocks(), b.blocks()):
        assert torch.equal(x, y)
