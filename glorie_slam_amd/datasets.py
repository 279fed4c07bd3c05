"""Dataset streams (reference: src/utils/datasets.py:17-336): Replica, ScanNet, 7-Scenes and TUM RGB-D sequences on disk,
and `ArrayDataset` for frames held in memory (no reference counterpart: tests, tools and synthetic runs use it).

A stream is what the drivers were written against: `len(stream)`, `stream[i] -> (index, color [1,3,h,w], depth [h,w],
pose)`, iteration in index order, `get_color(i)`, `get_intrinsic()` and the attributes `poses`, `color_paths`,
`depth_paths`, `n_img` (PoseTrajectoryFiller.__call__, SequenceRunner.run_stream, traj_eval.full_traj_eval).

Where the reference decodes with cv2 and then undistorts, resizes and converts on the host, files are decoded here with
PIL (imported when the first file is read) and the raw uint8 / uint16 arrays go to the device as they are:
`ingest.IngestPlan` turns them into the working-size float tensors there, one launch each.  Colour and depth therefore
come out on `device`; there is no host path.  PIL decodes RGB, so no channel swap is needed (cv2 arrays are BGR: pass
them through `IngestPlan.color(..., swap_rb=True)`).  Poses, path lists and the association of TUM's three timestamp
lists are host work and follow the reference line by line.
"""
import glob
import os

import numpy as np
import torch
from torch.utils.data import Dataset

from .ingest import IngestPlan, working_intrinsic


def _read_image(path, mode=None):
    from PIL import Image                                   # only when a file is actually read
    with Image.open(path) as im:
        return np.array(im.convert(mode) if mode else im)


def _read_depth_png(depth_path):
    """uint16 [H,W] as the file stores it (src/utils/datasets.py:52-55: anything but a PNG is a TypeError)"""
    if '.png' not in depth_path:
        raise TypeError(depth_path)
    raw = _read_image(depth_path)
    if raw.dtype != np.uint16:                                # some PIL versions open 16-bit PNGs as 32-bit integers
        if raw.ndim != 2 or raw.min() < 0 or raw.max() > 65535:
            raise TypeError(f"{depth_path}: not a 16-bit depth map")
        raw = raw.astype(np.uint16)
    return raw


class BaseDataset(Dataset):
    """src/utils/datasets.py:17-137.  cfg: 'dataset', 'cam' (see IngestPlan) and 'data' -> 'input_folder'"""

    def __init__(self, cfg, device='cuda:0'):
        super().__init__()
        cam = cfg['cam']
        self.name = cfg.get('dataset')
        self.device = device
        self.cam = cam
        self.png_depth_scale = cam.get('png_depth_scale', 1.0)
        self.n_img = -1
        self.depth_paths = None
        self.color_paths = None
        self.poses = None
        self.image_timestamps = None
        self.H, self.W, self.fx, self.fy, self.cx, self.cy = (cam[k] for k in ('H', 'W', 'fx', 'fy', 'cx', 'cy'))
        self.H_out, self.W_out = cam['H_out'], cam['W_out']
        self.H_edge, self.W_edge = cam.get('H_edge', 0), cam.get('W_edge', 0)
        self.distortion = np.array(cam['distortion']) if 'distortion' in cam else None
        folder = cfg.get('data', {}).get('input_folder')
        self.input_folder = os.path.expandvars(folder) if folder is not None else None
        self._plan = None

    @property
    def plan(self):
        """the IngestPlan of this camera, built (and its tables uploaded) on first use"""
        if self._plan is None:
            self._plan = IngestPlan(self.cam, self.device)
        return self._plan

    def __len__(self):
        return self.n_img

    def __iter__(self):
        for index in range(len(self)):
            yield self[index]

    # ---- raw frames: what a subclass may replace (ArrayDataset does) ---------------------------------------------------
    def _raw_color(self, index):
        """uint8 [H,W,3] RGB, numpy or tensor"""
        return _read_image(self.color_paths[index], "RGB")

    def _raw_depth(self, index):
        """[H,W] uint16 or float32 as stored, numpy or tensor; None without depth"""
        return _read_depth_png(self.depth_paths[index]) if self.depth_paths is not None else None

    def _upload(self, a):
        t = a if torch.is_tensor(a) else torch.from_numpy(np.ascontiguousarray(a))
        return t.to(self.plan.device).contiguous()

    # ---- the reference's surface ---------------------------------------------------------------------------------------
    def depthloader(self, index, depth_paths, depth_scale):
        """src/utils/datasets.py:48-58: the full-size depth of a file list on the host, float32 numpy [H,W] = raw /
        depth_scale (for callers that want ground-truth depth outside the stream; __getitem__ does not come through here)"""
        if depth_paths is None:
            return None
        return _read_depth_png(depth_paths[index]).astype(np.float32) / depth_scale

    def get_color(self, index):
        """src/utils/datasets.py:60-83 -> float32 [1,3,H_out,W_out] in [0,1] on the device"""
        return self.plan.color(self._upload(self._raw_color(index)))

    def get_colors(self, indices):
        """the frames `indices` in one launch -> float32 [B,3,H_out,W_out]"""
        return self.plan.color(torch.stack([self._upload(self._raw_color(int(i))) for i in indices]))

    def get_intrinsic(self):
        """src/utils/datasets.py:85-96 -> float32 [4] (fx, fy, cx, cy) of the working size, on the host"""
        return working_intrinsic(self.cam)

    def __getitem__(self, index):
        """src/utils/datasets.py:98-137 -> (index, color [1,3,h,w], depth [h,w] or None, pose float32 [4,4] or None)"""
        index = int(index)
        if not 0 <= index < len(self):
            raise IndexError(index)
        color = self.get_color(index)
        raw = self._raw_depth(index)
        depth = self.plan.depth(self._upload(raw))[0] if raw is not None else None
        pose = torch.from_numpy(np.asarray(self.poses[index])).float() if self.poses is not None else None
        return index, color, depth, pose

    def _slice(self, cfg, clamp):
        """[:max_frames][::stride] of the three lists; clamp: a negative max_frames means every frame (the reference does
        this for every dataset but TUM, where max_frames = -1 drops the last frame)"""
        stride, max_frames = cfg['stride'], cfg['max_frames']
        if clamp and max_frames < 0:
            max_frames = self.n_img
        self.color_paths = self.color_paths[:max_frames][::stride]
        self.depth_paths = self.depth_paths[:max_frames][::stride]
        self.poses = self.poses[:max_frames][::stride]
        self.n_img = len(self.color_paths)


class Replica(BaseDataset):
    """src/utils/datasets.py:140-168: results/frame*.jpg, results/depth*.png, traj.txt (one 4x4 per line)"""

    def __init__(self, cfg, device='cuda:0'):
        super().__init__(cfg, device)
        self.color_paths = sorted(glob.glob(f'{self.input_folder}/results/frame*.jpg'))
        self.depth_paths = sorted(glob.glob(f'{self.input_folder}/results/depth*.png'))
        self.n_img = len(self.color_paths)
        self.load_poses(f'{self.input_folder}/traj.txt')
        self._slice(cfg, clamp=True)

    def load_poses(self, path):
        self.poses = []
        with open(path, "r") as f:
            lines = f.readlines()
        for i in range(self.n_img):
            self.poses.append(np.array(list(map(float, lines[i].split()))).reshape(4, 4))


class ScanNet(BaseDataset):
    """src/utils/datasets.py:170-202: color/N.jpg, depth/N.png, pose/N.txt in numeric order"""

    def __init__(self, cfg, device='cuda:0'):
        super().__init__(cfg, device)
        number = lambda x: int(os.path.basename(x)[:-4])
        self.color_paths = sorted(glob.glob(os.path.join(self.input_folder, 'color', '*.jpg')), key=number)
        self.depth_paths = sorted(glob.glob(os.path.join(self.input_folder, 'depth', '*.png')), key=number)
        self.n_img = len(self.color_paths)
        self.load_poses(os.path.join(self.input_folder, 'pose'))
        self._slice(cfg, clamp=True)

    def load_poses(self, path):
        self.poses = []
        pose_paths = sorted(glob.glob(os.path.join(path, '*.txt')), key=lambda x: int(os.path.basename(x)[:-4]))
        for pose_path in pose_paths:
            with open(pose_path, "r") as f:
                lines = f.readlines()
            self.poses.append(np.array([list(map(float, line.split(' '))) for line in lines]).reshape(4, 4))


class SevenScenes(BaseDataset):
    """src/utils/datasets.py:204-229: *.color.png, *.depth.png, *.txt (float32 poses)"""

    def __init__(self, cfg, device='cuda:0'):
        super().__init__(cfg, device)
        self.color_paths = sorted(glob.glob(os.path.join(self.input_folder, '*.color.png')))
        self.depth_paths = sorted(glob.glob(os.path.join(self.input_folder, '*.depth.png')))
        self.n_img = len(self.color_paths)
        self.load_poses(self.input_folder)
        self._slice(cfg, clamp=True)

    def load_poses(self, path):
        self.poses = [np.loadtxt(p).astype(np.float32) for p in sorted(glob.glob(os.path.join(path, '*.txt')))]


class TUM_RGBD(BaseDataset):
    """src/utils/datasets.py:231-326: rgb.txt, depth.txt and groundtruth.txt (or pose.txt) associated by timestamp,
    thinned to at most 32 frames a second, the first kept pose taken as the origin"""

    def __init__(self, cfg, device='cuda:0'):
        super().__init__(cfg, device)
        self.color_paths, self.depth_paths, self.poses = self.loadtum(self.input_folder, frame_rate=32)
        self.n_img = len(self.color_paths)
        self._slice(cfg, clamp=False)

    def parse_list(self, filepath, skiprows=0):
        """ read list data """
        return np.loadtxt(filepath, delimiter=' ', dtype=str, skiprows=skiprows)

    def associate_frames(self, tstamp_image, tstamp_depth, tstamp_pose, max_dt=0.08):
        """ pair images, depths, and poses: the nearest depth (and pose) of every image, kept when closer than max_dt """
        associations = []
        for i, t in enumerate(tstamp_image):
            j = np.argmin(np.abs(tstamp_depth - t))
            if tstamp_pose is None:
                if np.abs(tstamp_depth[j] - t) < max_dt:
                    associations.append((i, j))
            else:
                k = np.argmin(np.abs(tstamp_pose - t))
                if (np.abs(tstamp_depth[j] - t) < max_dt) and (np.abs(tstamp_pose[k] - t) < max_dt):
                    associations.append((i, j, k))
        return associations

    def thin(self, tstamp_image, associations, frame_rate):
        """indices into `associations`: the first, then every one more than 1 / frame_rate after the last kept"""
        indicies = [0]
        for i in range(1, len(associations)):
            t0 = tstamp_image[associations[indicies[-1]][0]]
            t1 = tstamp_image[associations[i][0]]
            if t1 - t0 > 1.0 / frame_rate:
                indicies += [i]
        return indicies

    def loadtum(self, datapath, frame_rate=-1):
        """ read video data in tum-rgbd format """
        if os.path.isfile(os.path.join(datapath, 'groundtruth.txt')):
            pose_list = os.path.join(datapath, 'groundtruth.txt')
        elif os.path.isfile(os.path.join(datapath, 'pose.txt')):
            pose_list = os.path.join(datapath, 'pose.txt')
        else:
            raise FileNotFoundError(f"{datapath}: neither groundtruth.txt nor pose.txt")
        image_data = self.parse_list(os.path.join(datapath, 'rgb.txt'))
        depth_data = self.parse_list(os.path.join(datapath, 'depth.txt'))
        pose_data = self.parse_list(pose_list, skiprows=1)
        pose_vecs = pose_data[:, 1:].astype(np.float64)
        tstamp_image = image_data[:, 0].astype(np.float64)
        tstamp_depth = depth_data[:, 0].astype(np.float64)
        tstamp_pose = pose_data[:, 0].astype(np.float64)
        self.associations = self.associate_frames(tstamp_image, tstamp_depth, tstamp_pose)
        self.kept = self.thin(tstamp_image, self.associations, frame_rate)

        images, poses, depths = [], [], []
        inv_pose = None
        for ix in self.kept:
            (i, j, k) = self.associations[ix]
            images += [os.path.join(datapath, image_data[i, 1])]
            depths += [os.path.join(datapath, depth_data[j, 1])]
            c2w = self.pose_matrix_from_quaternion(pose_vecs[k])            # timestamp tx ty tz qx qy qz qw
            if inv_pose is None:
                inv_pose = np.linalg.inv(c2w)
                c2w = np.eye(4)
            else:
                c2w = inv_pose @ c2w
            poses += [c2w]
        return images, depths, poses

    def pose_matrix_from_quaternion(self, pvec):
        """ (t, q = qx qy qz qw) -> 4x4; the quaternion is normalised first, as scipy's Rotation.from_quat does """
        x, y, z, w = np.asarray(pvec[3:], np.float64) / np.linalg.norm(pvec[3:])
        x2, y2, z2, w2 = x * x, y * y, z * z, w * w
        xy, zw, xz, yw, yz, xw = x * y, z * w, x * z, y * w, y * z, x * w
        pose = np.eye(4)
        pose[:3, :3] = [[x2 - y2 - z2 + w2, 2 * (xy - zw), 2 * (xz + yw)],
                        [2 * (xy + zw), -x2 + y2 - z2 + w2, 2 * (yz - xw)],
                        [2 * (xz - yw), 2 * (yz + xw), -x2 - y2 + z2 + w2]]
        pose[:3, 3] = pvec[:3]
        return pose


class ArrayDataset(BaseDataset):
    """frames held in memory: frames_u8 uint8 [N,H,W,3] RGB, depths None or [N,H,W] uint16 / float32 (raw: divided by
    cam.png_depth_scale on ingest), poses None or [N,4,4]; numpy arrays or tensors (device tensors are not copied)"""

    def __init__(self, cfg, frames_u8, depths=None, poses=None, device=None):
        super().__init__(cfg, device if device is not None else cfg.get('device', 'cuda:0'))
        if (frames_u8.ndim != 4 or tuple(frames_u8.shape[1:]) != (self.H, self.W, 3)
                or frames_u8.dtype not in (np.uint8, torch.uint8)):
            raise ValueError(f"frames must be uint8 [N,{self.H},{self.W},3], got {frames_u8.dtype} "
                             f"{tuple(frames_u8.shape)}")
        n = frames_u8.shape[0]
        if depths is not None and (depths.ndim != 3 or tuple(depths.shape) != (n, self.H, self.W)):
            raise ValueError(f"depths must be [{n},{self.H},{self.W}], got {tuple(depths.shape)}")
        if poses is not None and tuple(np.shape(poses)) != (n, 4, 4):
            raise ValueError(f"poses must be [{n},4,4], got {tuple(np.shape(poses))}")
        self.frames, self.depths = frames_u8, depths
        self.poses = np.asarray(poses.cpu() if torch.is_tensor(poses) else poses, np.float64) if poses is not None else None
        self.n_img = n

    def _raw_color(self, index):
        return self.frames[index]

    def _raw_depth(self, index):
        return self.depths[index] if self.depths is not None else None

    def get_colors(self, indices):
        idx = [int(i) for i in indices]
        frames = self.frames[idx] if not torch.is_tensor(self.frames) else self.frames[torch.as_tensor(idx)]
        return self.plan.color(self._upload(frames))


dataset_dict = {
    "replica": Replica,
    "scannet": ScanNet,
    "tumrgbd": TUM_RGBD,
    "7scenes": SevenScenes,
}


def get_dataset(cfg, device='cuda:0') -> BaseDataset:
    """src/utils/datasets.py:335-336"""
    return dataset_dict[cfg['dataset']](cfg, device=device)
