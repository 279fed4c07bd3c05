"""The Python layer of the mesh evaluation (glorie_slam_amd/eval_recon.py, SequenceRunner.recon) against the numpy
restatement of tests/recon_ref.py: the 3D scores on the GPU's own sample points, ICP against the float64 loop with the
float32-rounded loop as the yardstick, depth L1 over views inside a box room, the runner end to end and the argument checks.

Scene: the UV sphere of radius 0.3 (480 triangles) as the ground truth and the mesh fused from tsdf_ref.sphere_scene()
(8 cameras of 64 x 48, voxel 0.02) as the reconstruction."""
import os

import numpy as np
import pytest
import torch

import recon_ref as R
import tsdf_ref

pytestmark = pytest.mark.gpu

FACTOR = 4.0
MAX_UNFIRM = 0.02
N_SAMPLES = 5000
MOTION = R.rigid((0.3, -0.5, 0.8), 2.0, (0.012, -0.01, 0.0125))       # 2 degrees about a skew axis, 2 cm


def _dev(a, gpu, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a)).to(gpu)
    return t if dtype is None else t.to(dtype)


@pytest.fixture(scope="module")
def meshes(gpu):
    """(rec vertices, rec faces, gt vertices, gt faces) on the device"""
    from glorie_slam_amd.generate_mesh import fuse_frames
    frames = [(_dev(d, gpu), _dev(c, gpu), p) for d, c, p in tsdf_ref.sphere_scene()]
    v, _, f, _ = fuse_frames(frames, tsdf_ref.SCENE_K, gpu, voxel_length=tsdf_ref.SCENE_VOXEL, sdf_trunc=tsdf_ref.SCENE_TRUNC)
    gv, gf = R.uv_sphere()
    assert len(f) > 1000
    return v, f, _dev(gv, gpu), _dev(gf, gpu)


def test_3d_metrics(gpu, meshes):
    from glorie_slam_amd import eval_recon as E
    rv, rf, gv, gf = meshes
    th = 0.05
    out, rec_pts, gt_pts = E.calc_3d_metric((rv, rf), (gv, gf), align=False, n_samples=N_SAMPLES, dist_th=th,
                                            return_samples=True)
    rec_pts, gt_pts = rec_pts.double().cpu().numpy(), gt_pts.double().cpu().numpy()
    assert rec_pts.shape == gt_pts.shape == (N_SAMPLES, 3)
    to_gt, to_rec = R.nn_kdtree(rec_pts, gt_pts)[0], R.nn_kdtree(gt_pts, rec_pts)[0]
    print("3d metrics:", out, "restated accuracy / completion (cm):", to_gt.mean() * 100, to_rec.mean() * 100)
    # identical fp32 inputs; the squared distance is three products and two sums in fp32: 3 x 2^-24 relative at most
    np.testing.assert_allclose(out["accuracy"], to_gt.mean() * 100, rtol=1e-6)
    np.testing.assert_allclose(out["completion"], to_rec.mean() * 100, rtol=1e-6)
    between = lambda d, x: (d < th * (1 - 1e-6)).mean() * 100 <= x <= (d < th * (1 + 1e-6)).mean() * 100
    assert between(to_rec, out["completion_ratio"]) and between(to_rec, out["recall"]) and between(to_gt, out["precision"])
    p, r = out["precision"], out["recall"]
    np.testing.assert_allclose(out["f-score"], 2 * p * r / (p + r), rtol=1e-12)
    assert out["accuracy"] <= tsdf_ref.SCENE_VOXEL * 100, "the fused sphere lies within a voxel of the sphere"
    # the three functions of eval_recon.py:25-43 on the same points
    d_rec, d_gt = _dev(rec_pts, gpu, torch.float32), _dev(gt_pts, gpu, torch.float32)
    np.testing.assert_allclose(E.accuracy(d_gt, d_rec) * 100, out["accuracy"], rtol=1e-12)
    np.testing.assert_allclose(E.completion(d_gt, d_rec) * 100, out["completion"], rtol=1e-12)
    np.testing.assert_allclose(E.completion_ratio(d_gt, d_rec, th) * 100, out["completion_ratio"], rtol=1e-12)


def test_icp(gpu, meshes):
    from glorie_slam_amd import eval_recon as E
    rv, rf, _, _ = meshes
    tgt = rv.cpu().numpy()
    moved = E.transform_points(MOTION, rv)
    src = moved.cpu().numpy()
    T, info = E.icp_align(moved, rv)
    T64, info64 = R.icp(src, tgt)
    T32, info32 = R.icp(src, tgt, round_f32=True)
    d_gpu, yard = np.abs(T - T64).max(), np.abs(T32 - T64).max()
    back = np.abs(T64 @ MOTION - np.eye(4)).max()
    print(f"icp on {len(src)} vertices: gpu {info}, float64 {info64}, float32-rounded {info32}")
    print(f"icp: |T gpu - T float64| {d_gpu:.3e} / |T rounded - T float64| {yard:.3e} = {d_gpu / max(yard, 1e-300):.3f}; "
          f"|T float64 . motion - 1| {back:.3e}")
    assert info["iterations"] == info64["iterations"] and info["fitness"] == info64["fitness"] == 1.0
    assert back <= 1e-6, "the restatement itself undoes the motion"
    assert d_gpu == 0.0 if yard == 0.0 else d_gpu <= FACTOR * yard
    # the scores of the moved mesh, aligned by the GPU's ICP and by the restatement's matrix
    gen = lambda: torch.Generator(device=gpu).manual_seed(5)
    a_gpu = E.calc_3d_metric((moved, rf), (rv, rf), align=True, n_samples=N_SAMPLES, generator=gen())
    a_ref = E.calc_3d_metric((moved, rf), (rv, rf), align=T64, n_samples=N_SAMPLES, generator=gen())
    # a sample moves by at most sqrt(3) (3 max|p| + 1) times the largest difference of the matrices, its fp32 rounding after
    # the transform by sqrt(3) 2^-24 max|p| on either side; the nearest-neighbour distance is 1-Lipschitz in the sample and
    # its fp32 evaluation is off by at most 2^-23 relative on either side
    pmax = float(np.abs(src).max()) + 0.03
    bound = 100 * (np.sqrt(3) * (3 * pmax + 1) * FACTOR * yard + 2 * np.sqrt(3) * 2.0 ** -24 * pmax
                   + 2 * 2.0 ** -23 * a_ref["accuracy"] / 100)
    print(f"accuracy (cm) of the moved mesh aligned by the gpu's icp {a_gpu['accuracy']:.9f}, by the restatement's matrix "
          f"{a_ref['accuracy']:.9f}; difference {abs(a_gpu['accuracy'] - a_ref['accuracy']):.3e}, allowed {bound:.3e}")
    assert abs(a_gpu["accuracy"] - a_ref["accuracy"]) <= bound
    # fewer than 3 correspondences: the current transform comes back
    far = rv + 50.0
    T_far, info_far = E.icp_align(far, rv, init=MOTION)
    assert np.array_equal(T_far, MOTION) and info_far["iterations"] == 0 and info_far["fitness"] == 0.0


# ---- depth L1 in a box room ------------------------------------------------------------------------------------------------
ROOM_H = ROOM_W = 64
ROOM_FOCAL = 40.0
ROOM_K = (ROOM_FOCAL, ROOM_FOCAL, ROOM_W / 2 - 0.5, ROOM_H / 2 - 0.5)
ROOM_SEED = 3


def _room():
    gv, gf = R.box_room()
    rv, rf = R.box_room((-0.97, -1.46, -0.78), (1.17, 1.43, 0.88))         # every wall a few centimetres inside
    return gv, gf, rv, rf


def _firm_views(views, meshes_np):
    """per view and mesh: (grown, shrunk, exact, firm, float32 composition)"""
    out = []
    for c2w in views:
        w2c = R._w2c32(c2w)
        per = []
        for v, f in meshes_np:
            args = (v, f, w2c, ROOM_K, ROOM_H, ROOM_W, 0.01, 20.0)
            per.append(R.firm_depth(*args) + (R.rasterise(*args, 0.0, np.float32),))
        out.append((w2c, per))
    return out


def test_depth_l1_in_a_box_room(gpu):
    from glorie_slam_amd import eval_recon as E
    gv, gf, rv, rf = _room()
    gt, rec = (_dev(gv, gpu), _dev(gf, gpu)), (_dev(rv, gpu), _dev(rf, gpu))
    kw = dict(align=False, n_imgs=6, H=ROOM_H, W=ROOM_W, focal=ROOM_FOCAL, seed=ROOM_SEED, return_details=True)
    out, det = E.calc_2d_metric(rec, gt, **kw)
    views = det["views"]
    assert np.array_equal(views, E.sample_views(gv.min(0).astype(np.float64), gv.max(0).astype(np.float64), 6, ROOM_SEED))
    assert (det["valid"] > 0).all()
    np.testing.assert_allclose(out["depth l1"], det["errors"].mean() * 100, rtol=1e-12)
    unfirm = total = 0
    sums = np.zeros(2)
    for i, (w2c, per) in enumerate(_firm_views(views, ((gv, gf), (rv, rf)))):
        w2c_d = _dev(w2c, gpu, torch.float32)
        g = [E.render_depth(*m, None, ROOM_K, ROOM_H, ROOM_W, w2c=w2c_d).double().cpu().numpy() for m in (gt, rec)]
        mean, count = R.depth_l1(g[0], g[1])
        assert det["valid"][i] == count and abs(det["errors"][i] - mean) <= 1e-12 * mean, "the metric is that of the renders"
        firm = per[0][3] & per[1][3]
        unfirm, total = unfirm + (~firm).sum(), total + firm.size
        tol = 0.0
        for depth, (grown, shrunk, exact, _, single) in zip(g, per):
            depth = np.where(depth > 0, depth, np.inf)
            assert (np.isfinite(depth) == np.isfinite(exact))[firm].all()
            both = firm & np.isfinite(exact) & np.isfinite(single)
            with np.errstate(invalid="ignore"):          # inf - inf on the pixels nothing covers
                yard = np.abs(single.astype(np.float64) - exact)[both].max()
                err = np.abs(depth - exact)[firm & np.isfinite(exact)].max()
            assert err <= FACTOR * yard
            tol += FACTOR * yard
        m = firm & np.isfinite(per[1][2])
        ref_mean = np.abs(R.to_zero(per[0][2]) - per[1][2])[m].mean()
        gpu_mean = np.abs(g[0] - g[1])[m].mean()
        assert abs(gpu_mean - ref_mean) <= tol
        sums += (gpu_mean, ref_mean)
    share = unfirm / total
    print(f"depth l1 {out['depth l1']:.6f} cm over 6 views; on the firm pixels gpu {sums[0] / 6 * 100:.9f} cm, reference "
          f"{sums[1] / 6 * 100:.9f} cm; share of pixels that are not firm in both meshes {share:.4f}")
    assert share <= MAX_UNFIRM
    assert 1.0 < out["depth l1"] < 15.0, "walls a few centimetres inside the room"


def test_depth_l1_skips_empty_views_and_redraws_unseen(gpu):
    from glorie_slam_amd import eval_recon as E
    gv, gf, rv, rf = _room()
    gt = (_dev(gv, gpu), _dev(gf, gpu))
    kw = dict(align=False, H=ROOM_H, W=ROOM_W, focal=ROOM_FOCAL, return_details=True)
    # a reconstruction of one wall (x = hi): a camera that looks at it and one that looks away
    wall = (_dev(rv, gpu), _dev(rf[2:4], gpu))
    at = tsdf_ref.look_at((0.1, 0.05, 0.02), (1.17, 0.1, 0.0))
    away = tsdf_ref.look_at((0.1, 0.05, 0.02), (-0.97, 0.1, 0.0))
    out, det = E.calc_2d_metric(wall, gt, views=[at, away, at], **kw)
    assert det["valid"][0] > 0 and det["valid"][1] == 0 and det["valid"][2] == det["valid"][0]
    np.testing.assert_allclose(out["depth l1"], det["errors"][0] * 100, rtol=1e-12)
    assert 2.0 < out["depth l1"] < 4.5, "the wall is 3 cm inside the room"
    # points behind the wall x = hi: every draw of the seeded stream that sees one of them is drawn again
    rng = np.random.default_rng(8)
    unseen = np.stack([np.full(200, 1.5), rng.uniform(-1.4, 1.3, 200), rng.uniform(-0.7, 0.8, 200)], 1).astype(np.float32)
    lo, hi = gv.min(0).astype(np.float64), gv.max(0).astype(np.float64)
    stream = E.sample_views(lo, hi, 60, ROOM_SEED)
    sees = []
    for c2w in stream:
        w2c = R._w2c32(c2w)
        a, b = (R.points_in_view(unseen, w2c, ROOM_K, ROOM_H, ROOM_W, 10.0 + s) for s in (1e-3, -1e-3))
        assert a == b or a > 0, "no draw hangs on the rounding of the border"
        sees.append(b > 0)
    sees = np.array(sees)
    expected = stream[~sees][:6]
    assert sees[:6].any() and len(expected) == 6
    rec = (_dev(rv, gpu), _dev(rf, gpu))
    _, det = E.calc_2d_metric(rec, gt, n_imgs=6, seed=ROOM_SEED, unseen_points=_dev(unseen, gpu), **kw)
    assert np.array_equal(det["views"], expected)
    _, det0 = E.calc_2d_metric(rec, gt, n_imgs=6, seed=ROOM_SEED, **kw)
    assert np.array_equal(det0["views"], stream[:6]) and not np.array_equal(det0["views"], expected)


# ---- the runner --------------------------------------------------------------------------------------------------------------
def _snapshot(run):
    npc = run.npc
    return ({k: v.clone() for k, v in run.images.items()}, npc.cloud_pos().clone(), npc.geo_feats.clone(),
            npc.col_feats.clone(), run.video.poses.clone(), run.video.disps_up.clone(), run.mapped, list(run.skipped))


def _unchanged(run, snap):
    images, pos, geo, col, poses, disps_up, mapped, skipped = snap
    assert sorted(images) == sorted(run.images) and all(torch.equal(images[k], run.images[k]) for k in images)
    npc = run.npc
    assert torch.equal(pos, npc.cloud_pos()) and torch.equal(geo, npc.geo_feats) and torch.equal(col, npc.col_feats)
    assert torch.equal(poses, run.video.poses) and torch.equal(disps_up, run.video.disps_up)
    assert run.mapped == mapped and list(run.skipped) == skipped


def test_runner_recon(gpu, tmp_path):
    from glorie_slam_amd.pipeline import synthetic_images, synthetic_runner
    K, H, W = 10, 168, 224
    run, c = synthetic_runner(gpu, K, zero_flow_head=True, map_iters=4, map_rays=600, H=H, W=W)
    imgs = synthetic_images(K, H, W)
    run.run(((k, imgs[k:k + 1]) for k in range(K)), c["intrinsics"], final_ba_steps=2)
    snap = _snapshot(run)
    mesh_kwargs = dict(voxel_length=0.04, sdf_trunc=0.16)
    v, _, f = run.mesh(**mesh_kwargs)
    assert len(f) > 1000
    lo, hi = v.min(0).values.cpu().numpy() - 0.3, v.max(0).values.cpu().numpy() + 0.3
    gv, gf = R.box_room(lo, hi)
    out = str(tmp_path / "run")
    res = run.recon(_dev(gv, gpu), _dev(gf, gpu), output=out, mesh_kwargs=mesh_kwargs, kwargs_3d=dict(n_samples=2000),
                    kwargs_2d=dict(n_imgs=8, H=64, W=64, focal=40.0))
    torch.cuda.synchronize()
    _unchanged(run, snap)
    print("runner recon:", res)
    assert sorted(res) == ["accuracy", "completion", "completion_ratio", "depth l1", "f-score", "precision", "recall"]
    assert all(np.isfinite(x) for x in res.values())
    lines = open(os.path.join(out, "metrics_recon.txt")).read().splitlines()
    assert [l.split(":")[0] for l in lines] == list(res) and float(lines[0].split(":")[1]) == res["accuracy"]
    assert os.path.exists(os.path.join(out, "mesh", "scene_kf.ply"))


# ---- arguments ---------------------------------------------------------------------------------------------------------------
def test_argument_checks(gpu, tmp_path):
    from glorie_slam_amd import eval_recon as E
    from glorie_slam_amd._lib import GlorieError
    from glorie_slam_amd.generate_mesh import write_ply
    v, f = R.box_room()
    dv, df = _dev(v, gpu), _dev(f, gpu)
    cpu_v, cpu_f = torch.from_numpy(v), torch.from_numpy(f)
    for call in (lambda: E.sample_surface(cpu_v, cpu_f, 4), lambda: E.calc_3d_metric((cpu_v, cpu_f), (dv, df)),
                 lambda: E.render_depth(dv, cpu_f, np.eye(4), ROOM_K, 8, 8), lambda: E.nn_distances(cpu_v, dv),
                 lambda: E.icp_align(dv, cpu_v), lambda: E.nn_stats(torch.zeros(4), 0.1)):
        with pytest.raises(GlorieError):
            call()
    for call in (lambda: E.sample_surface(dv, df.float(), 4), lambda: E.sample_surface(dv.int(), df, 4),
                 lambda: E.sample_surface(dv[:0], df, 4), lambda: E.sample_surface(dv, df[:0], 4),
                 lambda: E.calc_2d_metric((dv, df[:0]), (dv, df)), lambda: E.render_depth(dv, df, np.eye(3), ROOM_K, 8, 8),
                 lambda: E.render_depth(dv, df, np.eye(4), (1.0, 2.0), 8, 8), lambda: E.sample_surface(dv[:, :2], df, 4)):
        with pytest.raises(ValueError):
            call()
    with pytest.raises(GlorieError, match="GLORIE_EINVAL"):
        E.render_depth(dv, df, np.eye(4), ROOM_K, 8, 8, z_near=0.0)
    # paths of PLYs in the layout of generate_mesh.write_ply
    path = str(tmp_path / "room.ply")
    write_ply(path, v, f, np.zeros_like(v))
    res = E.eval_recon(path, (dv, df), eval_2d=False, align=False, device=gpu, kwargs_3d=dict(n_samples=500))
    assert sorted(res) == ["accuracy", "completion", "completion_ratio", "f-score", "precision", "recall"]
    assert all(np.isfinite(x) for x in res.values()) and res["accuracy"] < 50.0
