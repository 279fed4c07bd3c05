"""Tiny dataset trees on disk, written with PIL, for tests/golden/make_datasets.py (which runs the reference's loaders over
them and records the results), tests/test_datasets.py and tests/test_gpu_datasets.py (which rebuild the same trees and
run the package's loaders).  Not a test module.  Everything is seeded: two calls write the same files."""
import os

import numpy as np

H, W, N = 37, 53, 6                      # frame size (odd width), frames per tree
TUM_FR1 = [0.2624, -0.9531, -0.0054, 0.0026, 1.1633]

# the four shipped camera blocks (configs/Replica, configs/TUM_RGBD freiburg1, configs/Scannet, configs/7scenes)
SHIPPED_CAMS = {
    "replica": dict(H=680, W=1200, fx=600.0, fy=600.0, cx=599.5, cy=339.5, png_depth_scale=6553.5, H_edge=0, W_edge=0,
                    H_out=320, W_out=640),
    "tumrgbd": dict(H=480, W=640, fx=517.3, fy=516.5, cx=318.6, cy=255.3, distortion=TUM_FR1, png_depth_scale=5000.0,
                    H_edge=8, W_edge=8, H_out=384, W_out=512),
    "scannet": dict(H=480, W=640, fx=577.590698, fy=578.729797, cx=318.905426, cy=242.683609, png_depth_scale=1000.0,
                    H_edge=8, W_edge=16, H_out=240, W_out=320),
    "7scenes": dict(H=480, W=640, fx=532.57, fy=531.54, cx=319.5, cy=239.5, png_depth_scale=1000.0, H_edge=8, W_edge=8,
                    H_out=384, W_out=512),
}


def small_cam(distortion=None, png_depth_scale=5000.0):
    cam = dict(H=H, W=W, fx=45.0, fy=44.0, cx=25.7, cy=18.2, png_depth_scale=png_depth_scale, H_edge=2, W_edge=3,
               H_out=24, W_out=40)
    if distortion is not None:
        cam["distortion"] = list(distortion)
    return cam


def cfg_for(name, folder, cam, stride=1, max_frames=-1):
    return {"dataset": name, "cam": cam, "data": {"input_folder": str(folder)}, "stride": stride, "max_frames": max_frames}


def frames(n=N, seed=11):
    """(colour uint8 [n,H,W,3] RGB, depth uint16 [n,H,W])"""
    rng = np.random.default_rng(seed)
    return (rng.integers(0, 256, (n, H, W, 3), dtype=np.uint8),
            rng.integers(0, 65536, (n, H, W)).astype(np.uint16))


def poses(n, seed=12):
    """n rigid 4x4 float64 camera-to-world matrices"""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(n):
        q, _ = np.linalg.qr(rng.standard_normal((3, 3)))
        if np.linalg.det(q) < 0:
            q[:, 0] = -q[:, 0]
        m = np.eye(4)
        m[:3, :3], m[:3, 3] = q, rng.uniform(-1, 1, 3)
        out.append(m)
    return out


def _save_png(path, arr):
    from PIL import Image
    os.makedirs(os.path.dirname(path), exist_ok=True)
    Image.fromarray(arr).save(path)


def _save_depth(path, arr):
    from PIL import Image
    os.makedirs(os.path.dirname(path), exist_ok=True)
    Image.fromarray(arr.astype(np.uint16)).save(path)             # mode I;16: a 16-bit PNG


# ---- TUM RGB-D --------------------------------------------------------------------------------------------------------
# image timestamps: 1 is closer than 1/32 s to 0 and 6 to 5 (thinned out); 4 has no depth within max_dt = 0.08;
# 7 has no pose within max_dt
TUM_T_IMAGE = [100.000, 100.020, 100.060, 100.120, 100.500, 100.620, 100.645, 100.900, 101.000, 101.050]
TUM_T_DEPTH = [100.010, 100.055, 100.130, 100.200, 100.300, 100.610, 100.650, 100.910, 101.010, 101.045]
TUM_T_POSE = [99.995 + 0.01 * k for k in range(70)] + [101.000 + 0.01 * k for k in range(8)]     # a gap 100.685 .. 101.0


def write_tum(root, seed=21):
    """-> (colour [n_img,H,W,3], depth [n_depth,H,W]) as written; files rgb/<t>.png, depth/<t>.png"""
    root = str(root)
    rng = np.random.default_rng(seed)
    col = rng.integers(0, 256, (len(TUM_T_IMAGE), H, W, 3), dtype=np.uint8)
    dep = rng.integers(0, 65536, (len(TUM_T_DEPTH), H, W)).astype(np.uint16)
    os.makedirs(root, exist_ok=True)
    with open(os.path.join(root, "rgb.txt"), "w") as f:
        f.write("# color images\n# file: 'hand made'\n# timestamp filename\n")
        for k, t in enumerate(TUM_T_IMAGE):
            f.write(f"{t:.6f} rgb/{t:.6f}.png\n")
            _save_png(os.path.join(root, "rgb", f"{t:.6f}.png"), col[k])
    with open(os.path.join(root, "depth.txt"), "w") as f:
        f.write("# depth maps\n# file: 'hand made'\n# timestamp filename\n")
        for k, t in enumerate(TUM_T_DEPTH):
            f.write(f"{t:.6f} depth/{t:.6f}.png\n")
            _save_depth(os.path.join(root, "depth", f"{t:.6f}.png"), dep[k])
    with open(os.path.join(root, "groundtruth.txt"), "w") as f:
        f.write("timestamp tx ty tz qx qy qz qw\n")               # the one row that skiprows=1 drops
        for t in TUM_T_POSE:
            q = rng.standard_normal(4)
            q /= np.linalg.norm(q)
            p = rng.uniform(-1, 1, 3)
            f.write(f"{t:.4f} " + " ".join(f"{v:.6f}" for v in list(p) + list(q)) + "\n")
    return col, dep


# ---- 7-Scenes, ScanNet, Replica ---------------------------------------------------------------------------------------
def write_7scenes(root, n=N, seed=31):
    root = str(root)
    col, dep = frames(n, seed)
    for k, m in enumerate(poses(n, seed + 1)):
        _save_png(os.path.join(root, f"frame-{k:06d}.color.png"), col[k])
        _save_depth(os.path.join(root, f"frame-{k:06d}.depth.png"), dep[k])
        np.savetxt(os.path.join(root, f"frame-{k:06d}.pose.txt"), m)
    return col, dep


def write_scannet(root, n=12, seed=41):
    """frame numbers 0 .. n-1 without zero padding: the numeric sort differs from the alphabetical one past 9"""
    root = str(root)
    col, dep = frames(n, seed)
    os.makedirs(os.path.join(root, "pose"), exist_ok=True)
    for k, m in enumerate(poses(n, seed + 1)):
        _save_png(os.path.join(root, "color", f"{k}.jpg"), col[k])
        _save_depth(os.path.join(root, "depth", f"{k}.png"), dep[k])
        with open(os.path.join(root, "pose", f"{k}.txt"), "w") as f:
            f.write("\n".join(" ".join(f"{v:.8f}" for v in row) for row in m))
    return col, dep


def write_replica(root, n=N, seed=51):
    root = str(root)
    col, dep = frames(n, seed)
    os.makedirs(os.path.join(root, "results"), exist_ok=True)
    with open(os.path.join(root, "traj.txt"), "w") as f:
        for k, m in enumerate(poses(n, seed + 1)):
            _save_png(os.path.join(root, "results", f"frame{k:06d}.jpg"), col[k])
            _save_depth(os.path.join(root, "results", f"depth{k:06d}.png"), dep[k])
            f.write(" ".join(f"{v:.10e}" for v in m.reshape(-1)) + "\n")
    return col, dep


WRITERS = {"tumrgbd": write_tum, "7scenes": write_7scenes, "scannet": write_scannet, "replica": write_replica}
# (stride, max_frames) cases recorded per dataset
SLICES = [(1, -1), (2, -1), (1, 4), (2, 5)]
