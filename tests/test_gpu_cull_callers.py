"""The callers of the mesh culling (SequenceRunner.mesh, generate_mesh_kf, eval_recon.eval_recon): the defaults leave every
output as it was, cull and clean do what they say on the mesh of the synthetic run, and culling the ground truth to the
views lifts the completion ratio by the unseen room's share of the area."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

H, W = 168, 224
VOXEL, TRUNC = 0.04, 0.16


@pytest.fixture(scope="module")
def run(gpu):
    """the synthetic runner of tests/test_gpu_generate_mesh.py after its run"""
    from glorie_slam_amd.pipeline import synthetic_images, synthetic_runner
    K = 10
    runner, c = synthetic_runner(gpu, K, zero_flow_head=True, map_iters=4, map_rays=600, H=H, W=W)
    imgs = synthetic_images(K, H, W)
    summary = runner.run(((k, imgs[k:k + 1]) for k in range(K)), c["intrinsics"], final_ba_steps=2)
    assert summary["mapped"] > 3
    return runner, c


def test_runner_defaults_are_bitwise_what_they_were(gpu, run, tmp_path):
    runner, _ = run
    a, b = str(tmp_path / "a"), str(tmp_path / "b")
    v0, c0, f0 = runner.mesh(output=a, voxel_length=VOXEL, sdf_trunc=TRUNC)
    v1, c1, f1 = runner.mesh(output=b, voxel_length=VOXEL, sdf_trunc=TRUNC, cull=None, clean=None)
    assert len(f0) > 1000
    assert torch.equal(v0, v1) and torch.equal(c0, c1) and torch.equal(f0, f1)
    for name in ("scene_kf.ply", "vertices_pos_kf.npy"):
        assert open(os.path.join(a, "mesh", name), "rb").read() == open(os.path.join(b, "mesh", name), "rb").read()
    assert sorted(os.listdir(os.path.join(b, "mesh"))) == ["scene_kf.ply", "vertices_pos_kf.npy"]


def test_runner_cull_and_clean(gpu, run, tmp_path):
    from glorie_slam_amd import cull_mesh as C
    from glorie_slam_amd.eval_render import eval_kf_imgs
    from glorie_slam_amd.generate_mesh import generate_mesh_kf, read_ply
    runner, c = run
    ren = runner.renderer
    K = (ren.fx, ren.fy, ren.cx, ren.cy)
    min_faces = 50
    cull = {"method": "occlusion", "rule": "all", "min_views": 1, "eps": 0.05, "edge": 4, "z_far": 20.0}
    raw_v, _, raw_f = runner.mesh(voxel_length=VOXEL, sdf_trunc=TRUNC)
    out = str(tmp_path / "culled")
    v, col, f = runner.mesh(output=out, voxel_length=VOXEL, sdf_trunc=TRUNC, cull=cull, clean={"min_faces": min_faces})
    print(f"raw mesh {len(raw_v)} vertices / {len(raw_f)} faces -> culled and cleaned {len(v)} / {len(f)}")
    assert 0 < len(f) < len(raw_f) and 0 < len(v) < len(raw_v), "an edge of 4 pixels cuts the rim of the fused surface"
    assert v.dtype == torch.float32 and col.dtype == torch.float32 and f.dtype == torch.int32 and col.shape == v.shape
    assert int(f.min()) == 0 and int(f.max()) == len(v) - 1
    # every vertex is seen by a keyframe: re-checked with the views and depths mesh() used
    frames = eval_kf_imgs(runner, keep_renders=True)["frames"]
    c2ws = np.stack([runner.video.get_pose(fr["video_idx"], "cpu").double().numpy() for fr in frames])
    depths = [torch.where(fr["render"]["mask"], fr["render"]["depth"].float(),
                          torch.zeros_like(fr["render"]["depth"], dtype=torch.float32)) for fr in frames]
    seen = C.vertex_visibility(v, c2ws, K, H, W, depths=depths, eps=0.05, edge=4, z_far=20.0)
    assert int(seen.min()) >= 1
    raw_seen = C.vertex_visibility(raw_v, c2ws, K, H, W, depths=depths, eps=0.05, edge=4, z_far=20.0)
    assert int(raw_seen.min()) == 0
    # no component is below min_faces
    _, faces_of = C.mesh_components(v, f)
    assert int(faces_of[faces_of > 0].min()) >= min_faces
    # the file holds the culled mesh
    pv, pf, _ = read_ply(os.path.join(out, "mesh", "scene_kf.ply"))
    assert np.array_equal(pv, v.cpu().numpy()) and np.array_equal(pf, f.cpu().numpy())
    # the same from files
    files = str(tmp_path / "files")
    runner.evaluate(output=files)
    runner.video.save_video(os.path.join(files, "video.npz"))
    fv, fcol, ff = generate_mesh_kf(files, c["intrinsics"], voxel_length=VOXEL, sdf_trunc=TRUNC, device=gpu, cull=cull,
                                    clean={"min_faces": min_faces})
    assert torch.equal(fv, v) and torch.equal(fcol, col) and torch.equal(ff, f)
    gv, gcol, gf = generate_mesh_kf(files, c["intrinsics"], voxel_length=VOXEL, sdf_trunc=TRUNC, device=gpu,
                                    mesh_name_suffix="raw")
    assert torch.equal(gv, raw_v) and torch.equal(gf, raw_f)


# ---- eval_recon ----------------------------------------------------------------------------------------------------------
ROOM = np.array([2.5, 1.5, 2.5])
SIZE, FOCAL = 320, 128.0
VIEW_K = (FOCAL, FOCAL, SIZE / 2 - 0.5, SIZE / 2 - 0.5)


def _box(half, centre=(0.0, 0.0, 0.0)):
    v = np.array([[(-half, half)[(c >> a) & 1][a] for a in range(3)] for c in range(8)], np.float32)
    quads = [(0, 2, 6, 4), (1, 5, 7, 3), (0, 4, 5, 1), (2, 3, 7, 6), (0, 1, 3, 2), (4, 6, 7, 5)]
    return v + np.asarray(centre, np.float32), np.array([t for a, b, c, d in quads for t in ((a, b, c), (a, c, d))], np.int32)


def _area(v, f):
    p = v.astype(np.float64)[f]
    return 0.5 * np.linalg.norm(np.cross(p[:, 1] - p[:, 0], p[:, 2] - p[:, 0]), axis=1).sum()


def _views():
    """cameras near the centre of the room: along the six axes and along four horizontal diagonals"""
    import cull_ref
    eye = np.array([0.2, 0.1, -0.15])
    level = [(1, 0, 0), (-1, 0, 0), (0, 0, 1), (0, 0, -1), (1, 0, 1), (-1, 0, 1), (1, 0, -1), (-1, 0, -1)]
    views = [cull_ref.look_at(eye, eye + np.array(d, np.float64), up=(0.0, -1.0, 0.0)) for d in level]
    views += [cull_ref.look_at(eye, eye + np.array(d, np.float64), up=(0.0, 0.0, 1.0)) for d in ((0, 1, 0), (0, -1, 0))]
    return np.stack(views)


def _room_depth(c2w):
    """the exact depth of the inside of the box ROOM from a camera inside it (the ray's exit, in camera-frame z)"""
    v, u = np.meshgrid(np.arange(SIZE, dtype=np.float64), np.arange(SIZE, dtype=np.float64), indexing="ij")
    ray = np.stack([(u - VIEW_K[2]) / FOCAL, (v - VIEW_K[3]) / FOCAL, np.ones_like(u)], -1) @ c2w[:3, :3].T
    safe = np.where(np.abs(ray) < 1e-12, 1e-12, ray)
    t = np.where(safe > 0, (ROOM - c2w[:3, 3]) / safe, (-ROOM - c2w[:3, 3]) / safe).min(-1)
    return t.astype(np.float32)


def test_eval_recon_with_cull(gpu):
    from glorie_slam_amd import eval_recon as E
    from glorie_slam_amd.tsdf import TSDFVolume
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(gpu)
    views = _views()
    # the reconstruction: the room fused from the views' exact depth, as tools/time_eval_recon.py builds its fine mesh
    vol = TSDFVolume(VOXEL, TRUNC, -ROOM - 0.3, ROOM + 0.3, 16000, gpu)
    for c2w in views:
        d = dev(_room_depth(c2w))
        vol.integrate(d, torch.full((SIZE, SIZE, 3), 0.5, device=gpu), dev(c2w.astype(np.float32)), VIEW_K)
    rec_v, _, rec_f = vol.extract()
    del vol
    assert len(rec_f) > 10000
    # the ground truth: that room and a second one the cameras never entered, behind the first one's wall
    seen_v, seen_f = _box(ROOM)
    far_v, far_f = _box(0.5 * ROOM, centre=(9.0, 0.0, 0.0))
    gt_v, gt_f = np.concatenate([seen_v, far_v]), np.concatenate([seen_f, far_f + len(seen_v)])
    share = _area(seen_v, seen_f) / (_area(seen_v, seen_f) + _area(far_v, far_f))
    assert abs(share - 0.8) < 1e-6
    n = 20000
    kw = dict(eval_2d=False, align=False, kwargs_3d={"n_samples": n, "dist_th": 0.1})
    cull = {"c2ws": views, "K": VIEW_K, "H": SIZE, "W": SIZE, "method": "occlusion", "eps": 0.1}
    rec, gt = (rec_v, rec_f), (dev(gt_v), dev(gt_f))
    # what the cut leaves: the seen room of the ground truth, whole, and the reconstruction but for rim faces
    (cut_rec_v, cut_rec_f), (cut_gt_v, cut_gt_f) = E._cull_pair(rec, gt, cull)
    assert np.array_equal(cut_gt_v.cpu().numpy(), seen_v) and np.array_equal(cut_gt_f.cpu().numpy(), seen_f)
    assert len(cut_rec_f) >= 0.99 * len(rec_f)
    plain = E.eval_recon(rec, gt, **kw)
    assert plain == E.eval_recon(rec, gt, cull=None, **kw)
    assert plain == E.calc_3d_metric(rec, gt, align=False, n_samples=n, dist_th=0.1), "cull=None is the path as it was"
    culled = E.eval_recon(rec, gt, cull=cull, **kw)
    print("without cull:", plain, "\nwith cull:   ", culled, "\nseen share of the ground truth's area:", share)
    # Of n samples of the uncut ground truth Binomial(n, share) fall on the seen room, and each of those has a
    # reconstructed point within dist_th with the probability r that the cut ground truth measures: the uncut ratio is
    # Binomial(n, share r) / n, the cut one Binomial(n, r) / n from other draws.  Their combination
    # plain - share * culled has mean 0 and variance share r (1 - share r) / n + share^2 r (1 - r) / n <=
    # (1 + share^2) / (4 n); 5 standard deviations of that, in percent.  (dist_th is 0.1: the room fused at a voxel of 0.04
    # from 320 x 320 maps lies up to a voxel off the walls, which is not what this test is about.)
    bound = 100.0 * 5.0 * np.sqrt((1.0 + share * share) / (4.0 * n))
    gap = plain["completion_ratio"] - share * culled["completion_ratio"]
    print(f"completion ratio {plain['completion_ratio']:.3f} -> {culled['completion_ratio']:.3f}; "
          f"plain - share * culled = {gap:.3f} (bound {bound:.3f})")
    assert abs(gap) <= bound
    lift = culled["completion_ratio"] - plain["completion_ratio"]
    assert abs(lift - (1.0 - share) * culled["completion_ratio"]) <= bound, "the lift is the unseen room's share"
    assert lift > bound, "and it stands clear of the sampling noise"
    assert culled["completion"] < plain["completion"], "the unseen room no longer counts as missing surface"
