"""Pins of the cloud deformation and the proxy depth against the imported reference (this container only; the reference
never travels):

    python tests/golden/make_deform.py

  deform.npz   one video of 8 slots, 6 keyframes at 48x64 (poses, disps_up, valid_depth_mask) and 4 input-point runs per
               keyframe, interleaved in the point arrays (keyframe order 0 1 2 3 4 5 0 1 ... ).  The valid masks have holes
               (those points take the get_scale fallback); every point of keyframe 5 lies on a hole, where the reference's
               0/0 scale writes NaN.  Keyframes 0 1 3 5 are dirty.
    deform_*   NeuralPointCloud.update_points_pos (src/neural_point.py:378-438) called unbound with a namespace `self`,
               driven by the module's update_points_pos(npc, video) (:509-537) with a namespace `video` whose
               get_depth_and_pose / get_pose are DepthVideo's own methods (src/depth_video.py:313-324, lietorch.SE3 a
               matrix stand-in) and an `add_points` recorder: input positions, depths, cloud rows, the keyframes
               add_points received.  Three variants: N_add 3, N_add 5, N_add 3 with fix_interval_when_add_along_ray.
    proxy_*    get_proxy_render_depth (:539-575) with proj_depth_map (:446-506) over a namespace npc whose full_pcl holds
               the iproj of keyframes 0-2 (float64 stand-in of droid_backends.iproj), for counter 3 (row -2: wraps to
               H-2) and counter 9 (row 4) with mapping_window_size 5, use_mono_to_complete on and off; the projected
               depth alone as well.
    c2w_*      Mapper.get_c2w_and_depth (src/mapper.py:246-279) unbound for keyframes 0-4: c2w, the aligned mono prior,
               the masked tracker depth.
  Points whose projection lies within 1e-2 px of a pixel border (in float64) are masked out of full_pcl, so fp32 cannot
  move a point to another pixel; no two points that land in one pixel are within 1e-4 in depth.

Stand-ins used while importing: as in make_pix_warp.py, every module of src.mapper's import chain that this environment
lacks becomes a module of MagicMocks; lietorch.SE3 is replaced by a rotation-matrix stand-in for get_pose.
The archive is written with fixed zip timestamps: re-running the script reproduces it bit for bit.
"""
import os
import sys
import types

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from make_pix_warp import import_mapper, rot, save_npz  # noqa: E402

OUT = os.path.dirname(os.path.abspath(__file__))

B, K, H, W = 8, 6, 48, 64
FX, FY, CX, CY = 40.0, 40.0, 31.5, 23.5
RUNS, MARGIN = 4, 1e-2
DIRTY = (0, 1, 3, 5)
ALL_HOLES = 5


def quat_xyzw(R):
    w = np.sqrt(max(1 + R[0, 0] + R[1, 1] + R[2, 2], 1e-12)) / 2
    return np.array([(R[2, 1] - R[1, 2]) / (4 * w), (R[0, 2] - R[2, 0]) / (4 * w), (R[1, 0] - R[0, 1]) / (4 * w), w])


def rot_of_quat(q):
    x, y, z, w = q.unbind(-1)
    return torch.stack([torch.stack([1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)]),
                        torch.stack([2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)]),
                        torch.stack([2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)])])


class SE3Standin:
    """lietorch.SE3 as DepthVideo.get_pose uses it: SE3(pose).to(device).inv().matrix()"""

    def __init__(self, data, inverse=False):
        self.data, self.inverse = data, inverse

    def to(self, device):
        return self

    def inv(self):
        return SE3Standin(self.data, not self.inverse)

    def matrix(self):
        R, t = rot_of_quat(self.data[3:]), self.data[:3]
        M = torch.eye(4, dtype=self.data.dtype)
        if self.inverse:
            M[:3, :3], M[:3, 3] = R.t(), -(R.t() @ t)
        else:
            M[:3, :3], M[:3, 3] = R, t
        return M


def make_video(rng):
    """w2c poses [B,7] (keyframes 0..K-1 along a short arc), disps_up [B,H,W], valid [B,H,W]"""
    poses = np.zeros((B, 7), np.float32)
    poses[:, 6] = 1
    for k in range(K):
        R = rot(0.04 * k - 0.1, 0.02 * k)
        c = np.array([0.05 * k, -0.02 * k, 0.03 * k])                # camera centre
        poses[k, :3] = -(R.T @ c)
        poses[k, 3:] = quat_xyzw(R.T)
    jj, ii = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    disps = np.zeros((B, H, W), np.float32)
    for k in range(K):
        depth = 2.0 + 0.5 * np.sin(0.11 * ii + 0.3 * k) + 0.3 * np.cos(0.17 * jj) + rng.uniform(0, 0.05, (H, W))
        disps[k] = 1.0 / depth
    valid = rng.uniform(0, 1, (B, H, W)) > 0.15
    valid[K:] = False
    return poses, disps, valid


def make_points(rng, valid):
    """RUNS interleaved runs per keyframe: (video_idx, j, i, previous depth); keyframe ALL_HOLES only on holes"""
    vidx, pj, pi = [], [], []
    for r in range(RUNS):
        for k in range(K):
            n = int(rng.integers(20, 60))
            if k == ALL_HOLES:
                hj, hi = np.nonzero(~valid[k])
                sel = rng.choice(len(hj), n, replace=False)
                j, i = hj[sel], hi[sel]
            else:
                j, i = rng.integers(0, H, n), rng.integers(0, W, n)
            vidx.append(np.full(n, k)), pj.append(j), pi.append(i)
    vidx, pj, pi = (np.concatenate(x).astype(np.int64) for x in (vidx, pj, pi))
    prev = rng.uniform(1.2, 3.0, len(vidx)).astype(np.float32)
    return vidx, pj, pi, prev


def run_deform(np_mod, dv_mod, video_np, pts, N_add, fix):
    poses, disps, valid = video_np
    vidx, pj, pi, prev = pts
    cfg = {"cam": {"H": H, "W": W, "fx": FX, "fy": FY, "cx": CX, "cy": CY, "H_out": H, "W_out": W, "H_edge": 0, "W_edge": 0},
           "mapping": {"render_depth": "proxy"}}
    video = types.SimpleNamespace(poses=torch.from_numpy(poses), disps_up=torch.from_numpy(disps),
                                  valid_depth_mask=torch.from_numpy(valid), cfg=cfg,
                                  npc_dirty=torch.zeros(B, dtype=torch.bool))
    video.npc_dirty[list(DIRTY)] = True

    class Lock:
        def __enter__(self):
            return None

        def __exit__(self, *a):
            return False
    video.get_lock = lambda: Lock()
    video.get_pose = types.MethodType(dv_mod.DepthVideo.get_pose, video)
    video.get_depth_and_pose = types.MethodType(dv_mod.DepthVideo.get_depth_and_pose, video)
    n = len(vidx)
    npc = types.SimpleNamespace(device="cpu", N_add=N_add, near_end_surface=0.95, far_end_surface=1.05,
                                fix_interval_when_add_along_ray=fix,
                                _input_video_idx=torch.from_numpy(vidx), _input_j=torch.from_numpy(pj),
                                _input_i=torch.from_numpy(pi), _input_depth=torch.from_numpy(prev.copy()),
                                _input_pos=torch.zeros(n, 3), _cloud_pos=torch.zeros(n * N_add, 3))
    added = []
    npc.pts_num = lambda: n * N_add
    npc.get_device = lambda: "cpu"
    npc.add_points = lambda idx: added.append(idx.clone())
    npc.retrain_updated_points = lambda: None
    npc.update_points_pos = types.MethodType(np_mod.NeuralPointCloud.update_points_pos, npc)
    np_mod.update_points_pos(npc, video)
    return (npc._input_pos.numpy(), npc._input_depth.numpy(), npc._cloud_pos.numpy(), added[0].numpy(),
            video.npc_dirty.numpy())


def iproj64(poses, disps):
    """full-resolution unprojection of every slot (droid_backends.iproj of SE3(poses).inv()), float64"""
    pcl = np.zeros((B, H, W, 3))
    jj, ii = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    for b in range(B):
        q = torch.from_numpy(poses[b, 3:].astype(np.float64))
        R = rot_of_quat(q).numpy()
        t = poses[b, :3].astype(np.float64)
        d = 1.0 / np.maximum(disps[b].astype(np.float64), 1e-9)
        Xc = np.stack([(ii - CX) / FX * d, (jj - CY) / FY * d, d], -1)
        pcl[b] = (Xc - t) @ R                                        # R^T (Xc - t)
    return pcl


def view_c2w():
    """the proxy view: OpenGL c2w near keyframe 2"""
    R = rot(-0.02, 0.03)
    M = np.eye(4)
    M[:3, :3] = R @ np.diag([1.0, -1.0, -1.0])
    M[:3, 3] = [0.08, -0.03, 0.05]
    return M


def border_safe_mask(pcl, mask, c2w):
    """drop the points whose float64 projection into c2w is within MARGIN px of a pixel border, or whose depth ties
    another point of the same pixel within 1e-4"""
    w2c = np.linalg.inv(c2w)
    X = pcl.reshape(-1, 3)
    Xc = X @ w2c[:3, :3].T + w2c[:3, 3]
    z = Xc[:, 2] + 1e-6
    u = (FX * -Xc[:, 0] + CX * Xc[:, 2]) / z
    v = (FY * Xc[:, 1] + CY * Xc[:, 2]) / z
    near = lambda a: np.abs(a - np.round(a)) < MARGIN
    m = mask.reshape(-1) & ~near(u) & ~near(v)
    inside = m & (u >= 0) & (u < W) & (v >= 0) & (v < H) & (-z > 0)
    px = np.where(inside, np.floor(v).astype(np.int64) * W + np.floor(np.maximum(u, 0)).astype(np.int64), -1)
    order = np.lexsort((-z, px))
    zs, ps = -z[order], px[order]
    tie = (ps[1:] == ps[:-1]) & (ps[1:] >= 0) & (np.abs(zs[1:] - zs[:-1]) < 1e-4)
    bad = np.zeros(len(m), bool)
    bad[order[1:][tie]] = True
    bad[order[:-1][tie]] = True
    return (m & ~bad).reshape(mask.shape)


def main():
    mapper = import_mapper()
    import src.depth_video as dv_mod
    import src.neural_point as np_mod
    dv_mod.lietorch = types.SimpleNamespace(SE3=SE3Standin)
    torch.manual_seed(0)
    rng = np.random.default_rng(20261016)
    poses, disps, valid = make_video(rng)
    pts = make_points(rng, valid)
    out = dict(hw=np.array([H, W]), intrinsics=np.array([FX, FY, CX, CY]), poses=poses, disps_up=disps, valid=valid,
               dirty=np.isin(np.arange(B), DIRTY), input_video_idx=pts[0], input_j=pts[1], input_i=pts[2],
               input_depth=pts[3], near_far=np.array([0.95, 1.05]))
    for name, N_add, fix in (("n3", 3, False), ("n5", 5, False), ("fix", 3, True)):
        pos, depth, cloud, added, flags = run_deform(np_mod, dv_mod, (poses, disps, valid), pts, N_add, fix)
        out.update({f"deform_{name}_pos": pos, f"deform_{name}_depth": depth, f"deform_{name}_cloud": cloud,
                    f"deform_{name}_added": added, f"deform_{name}_flags_after": flags,
                    f"deform_{name}_args": np.array([N_add, int(fix)])})

    # proxy depth over a namespace npc
    c2w = view_c2w()
    pcl = iproj64(poses, disps)
    fmask = valid.copy()
    fmask[3:] = False                                                # keyframes 0-2 unprojected
    fmask = border_safe_mask(pcl, fmask, c2w)
    droid = (1.0 / disps[2]).astype(np.float32)
    droid[~valid[2]] = 0
    droid[:, : W // 3] = 0                                           # a band of tracker holes
    mono = (1.7 + 0.01 * np.arange(H * W).reshape(H, W) / (H * W)).astype(np.float32)
    out.update(full_pcl=pcl.astype(np.float32), full_mask=fmask, proxy_c2w=c2w.astype(np.float32), proxy_droid=droid,
               proxy_mono=mono, mapping_window_size=np.array(5))
    for counter in (3, 9):
        for use_mono in (True, False):
            npc = types.SimpleNamespace(full_pcl=lambda: torch.from_numpy(pcl.astype(np.float32)),
                                        full_mask=lambda: torch.from_numpy(fmask),
                                        video=types.SimpleNamespace(counter=types.SimpleNamespace(value=counter)))
            cfg = {"cam": {"H": H, "W": W, "fx": FX, "fy": FY, "cx": CX, "cy": CY, "H_out": H, "W_out": W, "H_edge": 0, "W_edge": 0},
                   "mapping": {"mapping_window_size": 5, "save_depth": False}}
            proxy = np_mod.get_proxy_render_depth(npc, cfg, torch.from_numpy(c2w.astype(np.float32)),
                                                  torch.from_numpy(droid), torch.from_numpy(mono), "cpu",
                                                  use_mono_to_complete=use_mono)
            out[f"proxy_c{counter}_m{int(use_mono)}"] = proxy.numpy()
        out[f"proj_c{counter}"] = np_mod.proj_depth_map(torch.from_numpy(c2w.astype(np.float32)), npc, "cpu",
                                                        cfg).numpy()

    # Mapper.get_c2w_and_depth of keyframes 0-4 with an affine-distorted, partly inflated mono prior
    video = types.SimpleNamespace(poses=torch.from_numpy(poses), disps_up=torch.from_numpy(disps),
                                  valid_depth_mask=torch.from_numpy(valid), depth_scale=torch.zeros(B),
                                  depth_shift=torch.zeros(B))

    class Lock:
        def __enter__(self):
            return None

        def __exit__(self, *a):
            return False
    video.get_lock = lambda: Lock()
    video.get_pose = types.MethodType(dv_mod.DepthVideo.get_pose, video)
    video.get_depth_and_pose = types.MethodType(dv_mod.DepthVideo.get_depth_and_pose, video)
    video.get_depth_scale_and_shift = types.MethodType(dv_mod.DepthVideo.get_depth_scale_and_shift, video)
    me = types.SimpleNamespace(video=video, device="cpu", printer=types.SimpleNamespace(print=lambda *a, **k: None))
    monos, c2ws, wqs, droids = [], [], [], []
    for k in range(K - 1):
        m = (1.0 / disps[k]) * (0.8 + 0.1 * k) + 0.2
        m[5:9, 10:20] *= 20                                          # outliers beyond 3 x mean: no weight
        m = m.astype(np.float32)
        c, wq, dr = mapper.Mapper.get_c2w_and_depth(me, k, k, torch.from_numpy(m))
        monos.append(m), c2ws.append(c.numpy()), wqs.append(wq.numpy()), droids.append(dr.numpy())
    out.update(c2w_mono=np.stack(monos), c2w_c2w=np.stack(c2ws), c2w_mono_wq=np.stack(wqs), c2w_droid=np.stack(droids))
    save_npz(os.path.join(OUT, "deform.npz"), out)
    print("wrote", os.path.join(OUT, "deform.npz"), {k: np.asarray(v).shape for k, v in out.items()})


if __name__ == "__main__":
    main()
