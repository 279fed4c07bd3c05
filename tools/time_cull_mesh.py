"""Timing of the mesh culling (glorie_slam_amd/cull_mesh.py, csrc/cull.hip) on the synthetic box room of
tools/time_tsdf.py: the room fused at 5/512 m voxels (the fine mesh) and the 640 x 480 cameras that turn in it.

    python tools/time_cull_mesh.py [--frames 24] [--views 64 200] [--repeats 5] [--json profiles/cull_mesh_time.json]

Reports device times (events around the calls, median of --repeats after a warm-up):
  visibility   the one launch over all views at every --views count: frustum only, against the views' own ray-cast depth
               maps, and against the maps the rasteriser made of the mesh itself (the launch alone, and the whole
               self-occlusion loop with its rasteriser calls); with the achieved bytes/s on the algorithmic bytes (12 B
               per vertex read, 4 B per count written, 64 B per view, 4 B of depth per (view, vertex) pair inside the
               frustum) and the (view, vertex) pairs per second
  select, compaction, components, clean_mesh   on the fine mesh
  torch        the composition of the same rules from torch ops in the same process: per view a float64 matmul, the
               tests and an indexed depth read; the compaction from a scatter, a cumsum and gathers; the labels from
               scatter_reduce(amin) over the edges with pointer jumping until nothing changes (one read-back per round)
  mesh()       SequenceRunner.mesh of the synthetic run with cull and clean off and on
Figures to report, not gates; the torch composition is the yardstick because there is no earlier path.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tools")]

from glorie_slam_amd import cull_mesh as C, eval_recon as E  # noqa: E402
from glorie_slam_amd.tsdf import TSDFVolume  # noqa: E402
from time_tsdf import H, K, ROOM, TRUNC, VOXEL, W, room_frame, timed  # noqa: E402

EPS, Z_NEAR, Z_FAR = 0.03, 0.01, 30.0


def median_ms(fn, repeats):
    fn()                                                              # loads the code objects, sizes the allocator's pools
    return float(np.median([timed(fn)[0] for _ in range(repeats)]) * 1e3)


def torch_visibility(vertices, w2cs, maps):
    """the rule of glorie_mesh_visibility from torch ops, one view at a time (float64)"""
    X = vertices.double()
    count = torch.zeros(X.shape[0], dtype=torch.int32, device=X.device)
    for m in range(w2cs.shape[0]):
        w = w2cs[m].double()
        p = X @ w[:3, :3].T + w[:3, 3]
        z = p[:, 2]
        u = torch.floor(K[0] * p[:, 0] / z + K[2] + 0.5)
        v = torch.floor(K[1] * p[:, 1] / z + K[3] + 0.5)
        ok = (z > Z_NEAR) & (z <= Z_FAR) & (u >= 0) & (u < W) & (v >= 0) & (v < H)
        if maps is not None:
            ui, vi = torch.where(ok, u, 0.0).long(), torch.where(ok, v, 0.0).long()
            d = maps[m][vi, ui].double()
            ok &= (d > 0) & (z <= d + EPS)
        count += ok.int()
    return count


def torch_compact(vertices, faces, keep):
    f = faces[keep.bool()].long()
    used = torch.zeros(vertices.shape[0], dtype=torch.bool, device=vertices.device)
    used[f.reshape(-1)] = True
    new_index = torch.cumsum(used.int(), 0) - 1
    return vertices[used], new_index[f].int()


def torch_components(faces, V, max_rounds=100000):
    """min-label propagation over the edges with pointer jumping; -> (label, rounds)"""
    f = faces.long()
    a = torch.cat([f[:, 0], f[:, 1]])
    b = torch.cat([f[:, 1], f[:, 2]])
    label = torch.arange(V, device=faces.device)
    for rounds in range(1, max_rounds + 1):
        before = label
        m = torch.minimum(label[a], label[b])
        label = label.scatter_reduce(0, a, m, "amin").scatter_reduce(0, b, m, "amin")
        label = label[label]
        if torch.equal(label, before):                                # the read-back of the round
            break
    return label.int(), rounds


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=24)
    ap.add_argument("--views", type=int, nargs="+", default=[64, 200])
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--max-blocks", type=int, default=120000)
    ap.add_argument("--skip-mesh", action="store_true", help="leave out the SequenceRunner.mesh timing")
    ap.add_argument("--json", default=os.path.join(ROOT, "profiles", "cull_mesh_time.json"))
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    vol = TSDFVolume(VOXEL, TRUNC, -ROOM - 0.1, ROOM + 0.1, args.max_blocks, dev)
    for i in range(args.frames):
        vol.integrate(*room_frame(i, args.frames, dev), K)
    fine_v, fine_c, fine_f = vol.extract()
    del vol
    V, F, rep = int(fine_v.shape[0]), int(fine_f.shape[0]), args.repeats
    res = {"device": torch.cuda.get_device_name(0), "vertices": V, "faces": F, "image": [H, W], "repeats": rep, "views": {}}
    count = torch.empty(V, dtype=torch.int32, device=dev)
    for M in args.views:
        frames = [room_frame(i, M, dev) for i in range(M)]
        maps = [d for d, _, _ in frames]
        c2ws = np.stack([c.double().cpu().numpy() for _, _, c in frames])
        w2cs = C._w2cs(c2ws, dev)
        given = C._depth_table(maps, dev)
        launch = lambda table: C._visibility_launch(fine_v, w2cs, K, H, W, Z_NEAR, Z_FAR, 0, table, EPS, False, False, count)
        row = {}
        row["frustum_ms"] = median_ms(lambda: launch(None), rep)
        pairs_inside = int(count.sum(dtype=torch.int64))
        row["given_depths_ms"] = median_ms(lambda: launch(given), rep)
        seen_given = int((count > 0).sum())
        r = E._Rasteriser(fine_v, fine_f, K, H, W, Z_NEAR, Z_FAR)
        own = [r.render(w2cs[m]) for m in range(M)]
        own_table = C._depth_table(own, dev)
        row["self_occlusion_launch_ms"] = median_ms(lambda: launch(own_table), rep)
        seen_self = int((count > 0).sum())
        del own, own_table
        row["self_occlusion_loop_ms"] = median_ms(
            lambda: C.self_occlusion_visibility(fine_v, fine_f, c2ws, K, H, W, eps=EPS, z_near=Z_NEAR, z_far=Z_FAR), rep)
        base = V * 16 + M * 64
        row["pairs"], row["pairs_inside_frustum"] = V * M, pairs_inside
        row["vertices_seen_given_self"] = [seen_given, seen_self]
        for key, nbytes in (("frustum", base), ("given_depths", base + 4 * pairs_inside),
                            ("self_occlusion_launch", base + 4 * pairs_inside)):
            row[key + "_bytes"] = nbytes
            row[key + "_GBps"] = nbytes / row[key + "_ms"] * 1e-6
            row[key + "_Gpairs_per_s"] = V * M / row[key + "_ms"] * 1e-6
        row["torch_frustum_ms"] = median_ms(lambda: torch_visibility(fine_v, w2cs, None), 2)
        row["torch_given_depths_ms"] = median_ms(lambda: torch_visibility(fine_v, w2cs, maps), 2)
        launch(given)
        row["torch_differing_counts"] = int((torch_visibility(fine_v, w2cs, maps) != count).sum())
        res["views"][str(M)] = row
        print(M, "views:", json.dumps(row), flush=True)
        last = (c2ws, maps)
    # ---- selection, compaction, components on the counts of the last view set ----------------------------------------------
    c2ws, maps = last
    count = C.vertex_visibility(fine_v, c2ws, K, H, W, depths=maps, eps=EPS, edge=8)
    res["select_ms"] = median_ms(lambda: C.select_faces(fine_f, count, 1, "all"), rep)
    keep = C.select_faces(fine_f, count, 1, "all")
    res["kept_faces"] = int(keep.sum(dtype=torch.int64))
    res["compact_ms"] = median_ms(lambda: C.compact_mesh(fine_v, fine_f, keep, fine_c), rep)
    res["torch_compact_ms"] = median_ms(lambda: torch_compact(fine_v, fine_f, keep), rep)
    cv, cf, _ = C.compact_mesh(fine_v, fine_f, keep, fine_c)
    tv, tf = torch_compact(fine_v, fine_f, keep)
    res["torch_compact_equals_kernel"] = bool(torch.equal(cv, tv) and torch.equal(cf, tf))
    res["components_ms"] = median_ms(lambda: C.mesh_components(fine_v, fine_f), rep)
    label, faces_of = C.mesh_components(fine_v, fine_f)
    res["components"] = int((faces_of > 0).sum())
    res["largest_component_faces"] = int(faces_of.max())
    res["clean_mesh_ms"] = median_ms(lambda: C.clean_mesh(fine_v, fine_f, fine_c, min_faces=100), rep)
    t, (tlabel, rounds) = timed(lambda: torch_components(fine_f, V))
    res["torch_components_ms"], res["torch_components_rounds"] = t * 1e3, rounds
    res["torch_components_equal_kernel"] = bool(torch.equal(tlabel, label))
    # ---- SequenceRunner.mesh ------------------------------------------------------------------------------------------------
    if not args.skip_mesh:
        from glorie_slam_amd.pipeline import synthetic_images, synthetic_runner
        n, h, w = 10, 168, 224
        run, c = synthetic_runner(dev, n, zero_flow_head=True, map_iters=4, map_rays=600, H=h, W=w)
        imgs = synthetic_images(n, h, w)
        run.run(((k, imgs[k:k + 1]) for k in range(n)), c["intrinsics"], final_ba_steps=2)
        kw = dict(voxel_length=0.04, sdf_trunc=0.16)
        on = dict(cull={"method": "occlusion", "eps": 0.05, "edge": 4}, clean={"min_faces": 50})
        res["runner_mesh_off_ms"] = median_ms(lambda: run.mesh(**kw), rep)
        res["runner_mesh_on_ms"] = median_ms(lambda: run.mesh(**kw, **on), rep)
        res["runner_mesh_faces_off_on"] = [int(run.mesh(**kw)[2].shape[0]), int(run.mesh(**kw, **on)[2].shape[0])]
    print(json.dumps(res))
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as fp:
            json.dump(res, fp, indent=1)
            fp.write("\n")


if __name__ == "__main__":
    main()
