"""The mesh of a run end to end (glorie_slam_amd/generate_mesh.py, SequenceRunner.mesh) on the synthetic stream at
168 x 224: the path through the files of evaluate(output) and save_video against the in-memory path, the PLY round trip,
the scaled trajectory, and the runner left as it was.  The scene's depths are around 2, a pixel covers about 0.018: a
voxel of 0.04 with a truncation of 0.16 keeps the pool at a few hundred blocks."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

H, W = 168, 224
VOXEL, TRUNC = 0.04, 0.16


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


def test_mesh_from_files_equals_mesh_from_memory(gpu, tmp_path):
    from glorie_slam_amd.generate_mesh import generate_mesh_kf, read_ply
    from glorie_slam_amd.pipeline import synthetic_images, synthetic_runner
    K = 10
    run, c = synthetic_runner(gpu, K, zero_flow_head=True, map_iters=4, map_rays=600, H=H, W=W)
    imgs = synthetic_images(K, H, W)
    summary = run.run(((k, imgs[k:k + 1]) for k in range(K)), c["intrinsics"], final_ba_steps=2)
    assert summary["mapped"] == run.mapped > 3
    snap = _snapshot(run)
    out = str(tmp_path / "run")
    res = run.evaluate(output=out)
    run.video.save_video(os.path.join(out, "video.npz"))
    intr = c["intrinsics"]
    v, col, f = generate_mesh_kf(out, intr, voxel_length=VOXEL, sdf_trunc=TRUNC, device=gpu)
    torch.cuda.synchronize()
    _unchanged(run, snap)
    assert res["frame_cnt"] > 3 and len(f) > 1000 and len(v) > 500, "the mesh must see the scene"
    assert v.dtype == torch.float32 and col.dtype == torch.float32 and f.dtype == torch.int32
    assert int(f.min()) == 0 and int(f.max()) == len(v) - 1
    assert float(col.min()) >= 0.0 and float(col.max()) <= 1.0 and bool(torch.isfinite(v).all())
    # the in-memory path: identical, and it writes the same two files
    mem_out = str(tmp_path / "mem")
    mv, mcol, mf = run.mesh(output=mem_out, voxel_length=VOXEL, sdf_trunc=TRUNC)
    torch.cuda.synchronize()
    _unchanged(run, snap)
    assert torch.equal(mv, v) and torch.equal(mcol, col) and torch.equal(mf, f)
    for root in (out, mem_out):
        assert sorted(os.listdir(os.path.join(root, "mesh"))) == ["scene_kf.ply", "vertices_pos_kf.npy"]
    assert open(os.path.join(out, "mesh", "scene_kf.ply"), "rb").read() == \
        open(os.path.join(mem_out, "mesh", "scene_kf.ply"), "rb").read()
    # the PLY round trip and the saved vertex positions
    pv, pf, pc = read_ply(os.path.join(out, "mesh", "scene_kf.ply"))
    assert np.array_equal(pv, v.cpu().numpy()) and np.array_equal(pf, f.cpu().numpy())
    assert pc.dtype == np.uint8 and np.array_equal(pc, np.rint(col.double().cpu().numpy() * 255.0).astype(np.uint8))
    saved = np.load(os.path.join(out, "mesh", "vertices_pos_kf.npy"))
    assert saved.dtype == np.float32 and np.array_equal(saved, v.cpu().numpy())
    # a scale of 2 (depths and translations doubled, the identity as the alignment, voxel and truncation doubled) is the
    # same volume twice as large: the same faces, vertices twice as far within the rounding of fp32
    sv, scol, sf = generate_mesh_kf(out, intr, scale=2.0, transform=np.eye(4), voxel_length=2 * VOXEL, sdf_trunc=2 * TRUNC,
                                    device=gpu, mesh_name_suffix="x2", scene="seq")
    assert torch.equal(sf, f)
    np.testing.assert_allclose(sv.cpu().numpy(), 2.0 * v.cpu().numpy(), rtol=1e-6, atol=1e-6 * VOXEL)
    np.testing.assert_allclose(scol.cpu().numpy(), col.cpu().numpy(), rtol=0, atol=1e-6)
    assert sorted(os.listdir(os.path.join(out, "mesh"))) == ["scene_kf.ply", "seq_x2.ply", "vertices_pos_kf.npy",
                                                            "vertices_pos_x2.npy"]
    # a rigid alignment moves the mesh with it: both paths again agree bit for bit.  The lattice is a new one, so against
    # the unmoved mesh only the place is compared: the centroid of the vertices.  Vertices sit on lattice edges, so the two
    # lattices' phase moves it by up to a voxel, and the few fragments at the rim by far less: 2 voxels are allowed (a
    # transform applied on the wrong side would move it by the size of the translation, 12 voxels and more)
    T = np.eye(4)
    T[:3, :3] = [[0.0, -1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0]]
    T[:3, 3] = [0.5, -0.25, 1.0]
    tv, tcol, tf = generate_mesh_kf(out, intr, transform=T, voxel_length=VOXEL, sdf_trunc=TRUNC, device=gpu,
                                    mesh_name_suffix="moved")
    mtv, mtcol, mtf = run.mesh(transform=T, voxel_length=VOXEL, sdf_trunc=TRUNC)
    assert torch.equal(mtv, tv) and torch.equal(mtcol, tcol) and torch.equal(mtf, tf) and len(tf) > 1000
    back = (tv.double().cpu().numpy() - T[:3, 3]) @ T[:3, :3]
    shift = np.abs(back.mean(0) - v.double().cpu().numpy().mean(0))
    print("centroid of the moved mesh, brought back, against the unmoved one (voxels):", shift / VOXEL)
    assert (shift < 2 * VOXEL).all()
    _unchanged(run, snap)
    # a map without a keyframe is an error
    np.save(os.path.join(out, "rendered_every_keyframe", "depth_00077.npy"), np.zeros((H, W), np.float32))
    with pytest.raises(ValueError):
        generate_mesh_kf(out, intr, voxel_length=VOXEL, sdf_trunc=TRUNC, device=gpu)
