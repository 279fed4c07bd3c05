"""Timing of the mesh evaluation (glorie_slam_amd/eval_recon.py) on the synthetic box room of tools/time_tsdf.py: the room
fused at 5/512 m voxels (the fine mesh) against its 12-triangle ground truth.

    python tools/time_eval_recon.py [--frames 24] [--views 1000] [--samples 200000] [--json]

Reports device times (events around the calls, median of --repeats after a warm-up) of: sampling --samples points of the
fine mesh; the two nearest-neighbour passes between --samples points of either mesh (cell list build + query); one ICP
iteration at the meshes' vertex counts (transform, 1-NN, moments, the 136-byte read-back); mesh_depth at 500 x 500 for the
fine mesh (policy 0 and 1) and for the 12-triangle room (policy 0, 1 and 2) from the same camera; the full loop of --views
views.  Next to them the host composition of the same steps in the same process: scipy's cKDTree for the two passes and
the numpy rasteriser of tests/recon_ref.py on the 12-triangle room and on the first --host-triangles triangles of the fine
mesh.  Figures to report, not gates - except one: with policy 0 the 12-triangle room must not be slower than the fine mesh
of the same view, or the large-triangle path is not doing its job.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tools"), os.path.join(ROOT, "tests")]

from glorie_slam_amd import eval_recon as E  # noqa: E402
from glorie_slam_amd.tsdf import TSDFVolume  # noqa: E402
from time_tsdf import K as FRAME_K, ROOM, TRUNC, VOXEL, room_frame, timed  # noqa: E402

H = W = 500
FOCAL = 300.0
VIEW_K = (FOCAL, FOCAL, W / 2 - 0.5, H / 2 - 0.5)


def box_room(half):
    v = np.array([[(-half, half)[(c >> a) & 1][a] for a in range(3)] for c in range(8)], np.float32)
    quads = [(0, 2, 6, 4), (1, 5, 7, 3), (0, 4, 5, 1), (2, 3, 7, 6), (0, 1, 3, 2), (4, 6, 7, 5)]
    return v, np.array([t for a, b, c, d in quads for t in ((a, b, c), (a, c, d))], np.int32)


def median_ms(fn, repeats):
    fn()                                                              # loads the code objects, sizes the allocator's pools
    return float(np.median([timed(fn)[0] for _ in range(repeats)]) * 1e3)


def host_ms(fn):
    t = time.perf_counter()
    out = fn()
    return (time.perf_counter() - t) * 1e3, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=24)
    ap.add_argument("--views", type=int, default=1000)
    ap.add_argument("--samples", type=int, default=200000)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--host-triangles", type=int, default=20000)
    ap.add_argument("--max-blocks", type=int, default=120000)
    ap.add_argument("--json", action="store_true")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    vol = TSDFVolume(VOXEL, TRUNC, -ROOM - 0.1, ROOM + 0.1, args.max_blocks, dev)
    for i in range(args.frames):
        vol.integrate(*room_frame(i, args.frames, dev), FRAME_K)
    fine_v, _, fine_f = vol.extract()
    del vol
    gv, gf = box_room(ROOM)
    room_v, room_f = torch.from_numpy(gv).to(dev), torch.from_numpy(gf).to(dev)
    res = {"fine_vertices": int(fine_v.shape[0]), "fine_faces": int(fine_f.shape[0]), "samples": args.samples,
           "image": [H, W]}
    n, rep = args.samples, args.repeats
    gen = torch.Generator(device=dev).manual_seed(0)
    u = torch.rand(n, 3, generator=gen, device=dev)
    res["sample_ms"] = median_ms(lambda: E.sample_surface(fine_v, fine_f, n, u=u), rep)
    rec_pts, _ = E.sample_surface(fine_v, fine_f, n, u=u)
    gt_pts, _ = E.sample_surface(room_v, room_f, n, u=torch.rand(n, 3, generator=gen, device=dev))
    res["nn_rec_to_gt_ms"] = median_ms(lambda: E.nn_distances(rec_pts, gt_pts), rep)
    res["nn_gt_to_rec_ms"] = median_ms(lambda: E.nn_distances(gt_pts, rec_pts), rep)
    index = E._index(room_v)
    mom = torch.empty(17, dtype=torch.float64, device=dev)
    T = np.eye(4)
    T[:3, 3] = 0.01

    def icp_iteration():
        cur = E.transform_points(T, fine_v)
        D, I = E._search(index, cur)
        return E.icp_moments(cur, room_v, I, D, 0.01, out=mom).cpu()
    res["icp_iteration_ms"] = median_ms(icp_iteration, rep)
    c2w = np.eye(4)
    a = 0.6
    c2w[:3, 0], c2w[:3, 2], c2w[:3, 3] = (np.cos(a), 0.0, -np.sin(a)), (np.sin(a), 0.0, np.cos(a)), (0.3, 0.1, -0.2)
    fine_r = E._Rasteriser(fine_v, fine_f, VIEW_K, H, W, 0.01, 20.0)
    room_r = E._Rasteriser(room_v, room_f, VIEW_K, H, W, 0.01, 20.0)
    w2c = E._w2c(c2w, dev)
    for name, r, policies in (("fine", fine_r, (0, 1)), ("room", room_r, (0, 1, 2))):
        for policy in policies:
            res[f"mesh_depth_{name}_policy{policy}_ms"] = median_ms(lambda: r.render(w2c, policy), rep)
    covered = [float((r.render(w2c) > 0).float().mean()) for r in (fine_r, room_r)]
    res["covered_share_fine_room"] = covered
    res["room_not_slower_than_fine_policy0"] = res["mesh_depth_room_policy0_ms"] <= res["mesh_depth_fine_policy0_ms"]
    loop = lambda: E.calc_2d_metric((fine_v, fine_f), (room_v, room_f), align=False, n_imgs=args.views, H=H, W=W, focal=FOCAL)
    E.calc_2d_metric((fine_v, fine_f), (room_v, room_f), align=False, n_imgs=2, H=H, W=W, focal=FOCAL)
    t, out = timed(loop)
    res["views"], res["view_loop_ms"], res["depth_l1_cm"] = args.views, t * 1e3, out["depth l1"]
    # ---- the host composition ---------------------------------------------------------------------------------------
    from scipy.spatial import cKDTree
    import recon_ref as R
    rec_np, gt_np = rec_pts.double().cpu().numpy(), gt_pts.double().cpu().numpy()
    res["host_kdtree_rec_to_gt_ms"] = host_ms(lambda: cKDTree(gt_np).query(rec_np, workers=-1))[0]
    res["host_kdtree_gt_to_rec_ms"] = host_ms(lambda: cKDTree(rec_np).query(gt_np, workers=-1))[0]
    w2c_np = w2c.double().cpu().numpy()
    res["host_raster_room_ms"] = host_ms(lambda: R.rasterise(gv, gf, w2c_np, VIEW_K, H, W))[0]
    k = min(args.host_triangles, int(fine_f.shape[0]))
    res["host_raster_fine_triangles"] = k
    res["host_raster_fine_ms"] = host_ms(lambda: R.rasterise(fine_v.cpu().numpy(), fine_f[:k].cpu().numpy(), w2c_np, VIEW_K,
                                                             H, W))[0]
    if not args.json:
        for key, val in res.items():
            print(f"{key:40s} {val}")
    print(json.dumps(res))
    if not res["room_not_slower_than_fine_policy0"]:
        sys.exit("with policy 0 the 12-triangle room is slower than the fine mesh of the same view")


if __name__ == "__main__":
    main()
