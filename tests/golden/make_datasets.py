"""Pins of the dataset loaders against the imported reference (needs a checkout of it, GLORIE_REFERENCE; the tests do
not):

    python tests/golden/make_datasets.py

  datasets.npz   the reference's src/utils/datasets.py run over the tiny trees of tests/dataset_trees.py:
                 - intrinsic_<name>: get_intrinsic() for the four shipped camera blocks
                 - tum_assoc, tum_kept: associate_frames over the hand-made rgb.txt / depth.txt / groundtruth.txt (gaps
                   larger than max_dt, frames closer than 1/32 s) and the indices the frame_rate=32 thinning keeps
                 - <name>_<stride>_<max_frames>_color / _depth: the path lists relative to the tree (ordering, numeric
                   sort of ScanNet, slicing), _poses: the poses (TUM: origin-normalised)
                 - <name>_depth0: the depth tensor of __getitem__(0) with edges 2 / 3

What is recorded never passes through cv2's pixel arithmetic.  cv2 is absent here: a stand-in decodes with PIL
(imread), leaves the image as it is (undistort) and resizes by nearest neighbour (resize) - the colour it yields is not
recorded.  Under NumPy 2, np.unicode_ = np.str_ for parse_list.  The archive holds results only and is written with
fixed zip timestamps: re-running the script reproduces it bit for bit.
"""
import importlib.util
import os
import sys
import tempfile
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import dataset_trees as T  # noqa: E402
from make_pix_warp import REF, save_npz  # noqa: E402


def register_cv2():
    from PIL import Image
    cv2 = types.ModuleType("cv2")
    cv2.IMREAD_UNCHANGED = -1

    def imread(path, flag=1):
        with Image.open(path) as im:
            if flag == cv2.IMREAD_UNCHANGED:
                return np.array(im)
            return np.ascontiguousarray(np.array(im.convert("RGB"))[..., ::-1])

    def resize(img, size):
        w, h = size
        yi = np.minimum((np.arange(h) * img.shape[0]) // h, img.shape[0] - 1)
        xi = np.minimum((np.arange(w) * img.shape[1]) // w, img.shape[1] - 1)
        return np.ascontiguousarray(img[yi][:, xi])

    cv2.imread, cv2.resize, cv2.undistort = imread, resize, lambda img, K, dist: img
    sys.modules["cv2"] = cv2


def import_reference():
    register_cv2()
    if not hasattr(np, "unicode_"):
        np.unicode_ = np.str_
    spec = importlib.util.spec_from_file_location("ref_datasets", os.path.join(REF, "src", "utils", "datasets.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def rel(paths, root):
    return np.array([os.path.relpath(p, root) for p in paths])


def main():
    ref = import_reference()
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        roots = {}
        for name, write in T.WRITERS.items():
            roots[name] = os.path.join(tmp, name)
            write(roots[name])
        for name, cam in T.SHIPPED_CAMS.items():
            ds = ref.get_dataset(T.cfg_for(name, roots[name], cam), device="cpu")
            out[f"intrinsic_{name}"] = ds.get_intrinsic().numpy()
        for name in T.WRITERS:
            for stride, max_frames in T.SLICES:
                ds = ref.get_dataset(T.cfg_for(name, roots[name], T.small_cam(), stride, max_frames), device="cpu")
                key = f"{name}_{stride}_{max_frames}"
                out[key + "_color"], out[key + "_depth"] = rel(ds.color_paths, roots[name]), rel(ds.depth_paths, roots[name])
                out[key + "_poses"] = np.stack(ds.poses).astype(np.float64)
                assert len(ds) == len(ds.color_paths) == len(ds.depth_paths) == len(ds.poses)
            ds = ref.get_dataset(T.cfg_for(name, roots[name], T.small_cam(), 1, 100), device="cpu")
            index, color, depth, pose = ds[0]
            assert color.shape == (1, 3, 24, 40) and depth.shape == (24, 40)
            out[f"{name}_depth0"] = depth.numpy()
            out[f"{name}_pose0"] = pose.numpy()
        # TUM: the association and the thinning on their own
        tum = ref.TUM_RGBD(T.cfg_for("tumrgbd", roots["tumrgbd"], T.small_cam(), 1, 100), device="cpu")
        ti, td, tp = (np.array(t, np.float64) for t in (T.TUM_T_IMAGE, T.TUM_T_DEPTH, [round(t, 4) for t in T.TUM_T_POSE]))
        assoc = tum.associate_frames(ti, td, tp)
        out["tum_assoc"] = np.array(assoc, np.int64)
        out["tum_assoc_no_pose"] = np.array(tum.associate_frames(ti, td, None), np.int64)
        # which associations loadtum's thinning kept: recovered from its paths
        names =[os.path.basename(p) for p in tum.color_paths]
        kept = [k for k, a in enumerate(assoc) if f"{T.TUM_T_IMAGE[a[0]]:.6f}.png" in names]
        out["tum_kept"] = np.array(kept, np.int64)
        assert len(assoc) < len(ti) and len(kept) < len(assoc), (len(assoc), len(kept))
    path = os.path.join(HERE, "datasets.npz")
    save_npz(path, out)
    print("associations", len(out["tum_assoc"]), "of", len(T.TUM_T_IMAGE), "kept", out["tum_kept"].tolist())
    print(path, os.path.getsize(path), "bytes,", len(out), "arrays")


if __name__ == "__main__":
    main()
