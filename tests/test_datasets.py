"""glorie_slam_amd.datasets against the recording of the reference's loaders (tests/golden/datasets.npz, written by
tests/golden/make_datasets.py over the trees of tests/dataset_trees.py): the same trees are rebuilt in tmp_path and the
package's classes are compared with the recording field by field.  No GPU: nothing here calls __getitem__ or get_color,
which ingest on the device; the recorded depth tensor is compared with the numpy restatement of the depth path."""
import os

import numpy as np
import pytest
import torch

import dataset_trees as T
import ingest_ref as R

HERE = os.path.dirname(os.path.abspath(__file__))
REC = np.load(os.path.join(HERE, "golden", "datasets.npz"))


@pytest.fixture(scope="module")
def roots(tmp_path_factory):
    base = tmp_path_factory.mktemp("trees")
    out = {}
    for name, write in T.WRITERS.items():
        out[name] = (str(base / name), write(base / name))
    return out


def _dataset(name, roots, cam, stride=1, max_frames=-1):
    from glorie_slam_amd.datasets import get_dataset
    return get_dataset(T.cfg_for(name, roots[name][0], cam, stride, max_frames), device="cuda:0")


@pytest.mark.parametrize("name", sorted(T.SHIPPED_CAMS))
def test_get_intrinsic_of_the_shipped_camera_blocks(name, roots):
    got = _dataset(name, roots, T.SHIPPED_CAMS[name]).get_intrinsic()
    assert got.dtype == torch.float32 and np.array_equal(got.numpy(), REC[f"intrinsic_{name}"])
    assert np.array_equal(R.intrinsic(T.SHIPPED_CAMS[name]), REC[f"intrinsic_{name}"])


def test_dataset_dict_and_surface():
    from glorie_slam_amd import datasets as D
    assert D.dataset_dict == {"replica": D.Replica, "scannet": D.ScanNet, "tumrgbd": D.TUM_RGBD, "7scenes": D.SevenScenes}
    for cls in list(D.dataset_dict.values()) + [D.ArrayDataset]:
        assert issubclass(cls, D.BaseDataset)
    for attr in ("__len__", "get_color", "get_intrinsic", "depthloader", "__getitem__"):
        assert callable(getattr(D.BaseDataset, attr))
    assert not hasattr(D, "load_mono_depth")                   # stays in motion_filter.py
    src = open(D.__file__).read()
    assert "import cv2" not in src and "import PIL" not in src.split("def _read_image")[0]      # PIL only when a file is read


@pytest.mark.parametrize("name", sorted(T.WRITERS))
@pytest.mark.parametrize("stride,max_frames", T.SLICES)
def test_paths_slicing_and_poses(name, stride, max_frames, roots):
    ds = _dataset(name, roots, T.small_cam(), stride, max_frames)
    key = f"{name}_{stride}_{max_frames}"
    root = roots[name][0]
    assert [os.path.relpath(p, root) for p in ds.color_paths] == REC[key + "_color"].tolist()
    assert [os.path.relpath(p, root) for p in ds.depth_paths] == REC[key + "_depth"].tolist()
    want = REC[key + "_poses"]
    assert len(ds) == ds.n_img == len(want) == len(ds.poses)
    got = np.stack(ds.poses).astype(np.float64)
    if name == "tumrgbd":
        # the rotation of a unit quaternion, an inverse and a product in float64: entries of magnitude <= a few units, each
        # a handful of roundings at 2^-53 relative -> 1e-13 is hundreds of ulps of slack and far below any real difference
        np.testing.assert_allclose(got, want, rtol=0, atol=1e-13)
        if len(got):
            assert np.array_equal(got[0], np.eye(4))               # the first pose is the origin
    else:
        assert np.array_equal(got, want)


def test_tum_association_and_thinning(roots):
    ds = _dataset("tumrgbd", roots, T.small_cam(), 1, 100)
    assert np.array_equal(np.array(ds.associations, np.int64), REC["tum_assoc"])
    assert np.array_equal(np.array(ds.kept, np.int64), REC["tum_kept"])
    ti, td = np.array(T.TUM_T_IMAGE), np.array(T.TUM_T_DEPTH)
    assert np.array_equal(np.array(ds.associate_frames(ti, td, None), np.int64), REC["tum_assoc_no_pose"])
    assert len(REC["tum_assoc"]) < len(ti) and len(REC["tum_kept"]) < len(REC["tum_assoc"])    # both rules did bite


@pytest.mark.parametrize("name", sorted(T.WRITERS))
def test_recorded_depth_is_the_restatement_of_the_depth_path(name, roots):
    """the reference's __getitem__ depth (edges 2 / 3, png_depth_scale 5000) == tests/ingest_ref.depth of the written
    array: what the GPU tests hold the kernel to is what the reference computes"""
    ds = _dataset(name, roots, T.small_cam(), 1, 100)
    col, dep = roots[name][1]
    first = os.path.relpath(ds.depth_paths[0], roots[name][0])
    k = 0 if name != "tumrgbd" else T.TUM_T_DEPTH.index(float(os.path.basename(first)[:-4]))
    assert np.array_equal(R.depth(dep[k], T.small_cam())[0], REC[f"{name}_depth0"])
    assert np.array_equal(np.asarray(ds.poses[0], np.float64).astype(np.float32), REC[f"{name}_pose0"])
    raw = ds._raw_depth(0)                                          # the PIL decode returns what was written
    assert raw.dtype == np.uint16 and np.array_equal(raw, dep[k])
    host = ds.depthloader(0, ds.depth_paths, 5000.0)
    assert host.dtype == np.float32 and np.array_equal(host, dep[k].astype(np.float32) / 5000.0)
    if not ds.color_paths[0].endswith(".jpg"):
        assert np.array_equal(ds._raw_color(0), col[0])            # TUM: image 0 is the first kept frame


def test_array_dataset_checks_its_arrays():
    from glorie_slam_amd.datasets import ArrayDataset
    col, dep = T.frames(3)
    cfg = {"cam": T.small_cam()}
    ds = ArrayDataset(cfg, col, dep, T.poses(3))
    assert len(ds) == 3 and ds.poses.shape == (3, 4, 4) and ds.color_paths is None
    assert torch.equal(ds.get_intrinsic(), torch.from_numpy(R.intrinsic(T.small_cam())))
    with pytest.raises(ValueError):
        ArrayDataset(cfg, col.astype(np.float32))
    with pytest.raises(ValueError):
        ArrayDataset(cfg, col[:, :-1])
    with pytest.raises(ValueError):
        ArrayDataset(cfg, col, dep[:2])
    with pytest.raises(ValueError):
        ArrayDataset(cfg, col, dep, T.poses(2))


def test_align_full_traj_skips_frames_without_ground_truth():
    from glorie_slam_amd.traj_eval import align_full_traj
    rng = np.random.default_rng(0)
    gt = np.stack(T.poses(8))
    q, _ = np.linalg.qr(rng.standard_normal((3, 3)))
    q *= np.sign(np.linalg.det(q))
    est = gt.copy()
    est[:, :3, 3] = (gt[:, :3, 3] - np.array([0.3, -0.2, 0.1])) @ q / 1.7       # gt = 1.7 q est + t
    gt[2] = np.nan
    gt[5, 0, 3] = np.inf
    r_a, t_a, s, aligned, ref = align_full_traj(est, gt)
    assert aligned.shape == ref.shape == (6, 4, 4) and abs(s - 1.7) < 1e-9
    np.testing.assert_allclose(aligned[:, :3, 3], ref[:, :3, 3], atol=1e-9)
    with pytest.raises(ValueError):
        align_full_traj(est[:3], gt)
