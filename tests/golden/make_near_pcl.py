"""Generates tests/golden/near_pcl.npz: the reference's own NeuralPointCloud.sample_near_pcl (src/neural_point.py:315-375,
borrowed as an unbound method - its class needs faiss to construct) on the rays of tests/near_pcl_ref.scene(), on CPU.

    python tests/golden/make_near_pcl.py

The neighbour search behind it is exact: candidates from a k-d tree, the squared distance ((dx*dx + dy*dy) + dz*dz) in
float32 as the build's KNN forms it, neighbor_num = how many lie inside radius_query (sample_near_pcl only asks whether
that is zero).  The fixture stores the rays, near, far, num and the two outputs (data, no reference source); the cloud
is regenerated from glorie_slam_amd.synth by the tests.
"""
import os
import sys

import numpy as np
import torch

OUT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, OUT)
sys.path.insert(0, os.path.dirname(OUT))
sys.path.insert(0, os.path.dirname(os.path.dirname(OUT)))
from make_golden import install_stubs  # noqa: E402
import near_pcl_ref as ref  # noqa: E402


class BallNPC:
    device = "cpu"

    def __init__(self, cloud, radius_query):
        from scipy.spatial import cKDTree
        self.cloud = cloud.astype(np.float32)
        self.tree = cKDTree(self.cloud.astype(np.float64))
        self.rq = radius_query

    def find_neighbors_faiss(self, pos, step='query', retrain=False, is_pts_grad=False, dynamic_radius=None):
        q = pos.numpy().astype(np.float32)
        r2 = np.float32(self.rq) * np.float32(self.rq)
        cand = self.tree.query_ball_point(q.astype(np.float64), 1.05 * self.rq)
        nn = np.zeros(q.shape[0], np.int32)
        for i, c in enumerate(cand):
            if c:
                d = q[i][None, :] - self.cloud[c]
                d2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
                nn[i] = min(int((d2 < r2).sum()), 8)
        D = torch.zeros(q.shape[0], 8)
        return D, torch.zeros(q.shape[0], 8, dtype=torch.int64), torch.from_numpy(nn)


def main():
    import types
    install_stubs()
    for name in ("faiss", "faiss.contrib", "faiss.contrib.torch_utils", "cv2"):
        sys.modules.setdefault(name, types.ModuleType(name))
    ds = types.ModuleType("src.utils.datasets")
    ds.load_mono_depth = None
    sys.modules.setdefault("src.utils.datasets", ds)
    from src.neural_point import NeuralPointCloud as RefNPC
    BallNPC.sample_near_pcl = RefNPC.sample_near_pcl
    sc = ref.scene()
    npc = BallNPC(sc["cloud"], ref.RADIUS)
    near, far, num = ref.NEAR, 6.0, 10
    z, invalid = npc.sample_near_pcl(torch.from_numpy(sc["rays_o"]), torch.from_numpy(sc["rays_d"]), near,
                                     torch.tensor(far, dtype=torch.float32), num)
    np.savez_compressed(os.path.join(OUT, "near_pcl.npz"), rays_o=sc["rays_o"], rays_d=sc["rays_d"],
                        near=np.float64(near), far=np.float32(far), num=np.int32(num), z_vals=z.numpy(),
                        invalid=invalid.numpy())
    print("near_pcl.npz: invalid rays", int(invalid.sum()), "/", invalid.numel())


if __name__ == "__main__":
    main()
