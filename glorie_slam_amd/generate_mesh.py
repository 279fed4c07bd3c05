"""The triangle mesh of a run (reference: src/utils/generate_mesh.py:55-123 generate_mesh_kf): the masked depth and colour
maps the re-render evaluation saved for every mapped keyframe are fused into a TSDF volume (tsdf.py, csrc/tsdf.hip) with
the keyframe poses of video.npz, and the surface is extracted.

  generate_mesh_kf(output, intrinsics, ...)   from the files under `output`; writes mesh/{scene}_{suffix}.ply and
                                              mesh/vertices_pos_{suffix}.npy
  fuse_frames(frames, intrinsics, ...)        the same fusion from maps in device memory (SequenceRunner.mesh)
  write_ply / read_ply                        binary little-endian PLY with uchar vertex colours

A monocular map has no metric scale: `scale` multiplies the depths and the pose translations and `transform` (4x4, the
alignment of traj_eval.align_kf_traj: se3(r_a, t_a)) is applied on the left, as the reference's scaled and transformed
trajectory; the default voxel of 5/512 m and the truncation of 0.04 m mean something only after that alignment.

The reference's `compensate_vector` is not applied: it corrects the half-voxel offset between Open3D's sampling and its
extraction, which this volume does not have (voxel (i,j,k) samples origin + (i + 0.5, j + 0.5, k + 0.5) * voxel_length
and the vertices are placed on that lattice).  The mid-run meshes and the printer are out of scope.
"""
import os
import re

import numpy as np
import torch

from . import _lib as L
from .tsdf import BLOCK, TSDFVolume, _intrinsics, depth_bounds


def _placed(c2w, scale, transform):
    """the pose of the scaled and aligned trajectory: translation * scale, then transform on the left (float64)"""
    c2w = np.array(c2w, np.float64, copy=True)
    c2w[:3, 3] *= float(scale)
    if transform is not None:
        c2w = np.asarray(transform, np.float64) @ c2w
    return c2w


def fuse_frames(frames, intrinsics, device, scale=1.0, transform=None, voxel_length=5.0 / 512.0, sdf_trunc=0.04,
                max_blocks=None):
    """frames: list of (depth f32 [H,W] with 0 where there is nothing, color f32 [H,W,3], c2w [4,4] OpenCV convention) -
    depth and colour on `device`, c2w anywhere.  -> (vertices f32 [V,3], colors f32 [V,3], faces int32 [F,3], volume).
    The bound encloses the back-projected pixels; max_blocks (default: an estimate from the area the pixels cover) is
    doubled and the fusion repeated when a frame does not fit"""
    scale = float(scale)
    placed = []
    for depth, color, c2w in frames:
        L.need_cuda(depth, color)
        c2w = c2w.detach().cpu().numpy() if torch.is_tensor(c2w) else c2w
        pose = torch.from_numpy(_placed(c2w, scale, transform)).to(device, torch.float32)
        placed.append((L.f32(depth) * scale if scale != 1.0 else L.f32(depth), L.f32(color), pose))
    fx, fy, cx, cy = _intrinsics(intrinsics)
    empty = (torch.zeros(0, 3, device=device), torch.zeros(0, 3, device=device),
             torch.zeros(0, 3, dtype=torch.int32, device=device), None)
    if not placed:
        return empty
    try:
        lo, hi = depth_bounds([(d, p) for d, _, p in placed], (fx, fy, cx, cy), sdf_trunc + voxel_length)
    except ValueError:
        return empty
    n_table = int(np.prod(np.maximum(1, np.ceil((hi - lo) / (BLOCK * voxel_length) - 1e-6))))
    if max_blocks is None:
        # the surface patch of a pixel is about (d / fx) x (d / fy); a block face is (8 voxel)^2 and the truncation
        # band is 2 sdf_trunc / (8 voxel) + 1 blocks deep; a factor 2 for slanted surfaces
        side = BLOCK * voxel_length
        area = sum(float(((d * d) * ((d > 0) & (d <= 30.0))).sum()) for d, _, _ in placed) / (fx * fy)
        max_blocks = int(2.0 * area / (side * side) * (2.0 * sdf_trunc / side + 1.0)) + 64
    max_blocks = max(1, min(int(max_blocks), n_table))
    while True:
        vol = TSDFVolume(voxel_length, sdf_trunc, lo, hi, max_blocks, device)
        try:
            for depth, color, pose in placed:
                vol.integrate(depth, color, pose, (fx, fy, cx, cy))
            break
        except L.GlorieError as e:
            if "GLORIE_ENOMEM" not in str(e) or max_blocks >= n_table:
                raise
            max_blocks = min(2 * max_blocks, n_table)
    return vol.extract() + (vol,)


def cull_and_clean(vertices, colors, faces, frames, intrinsics, scale=1.0, transform=None, cull=None, clean=None):
    """the post-processing of a fused mesh (cull_mesh.py).  cull: a dict of cull_mesh keywords - the views are the poses of
    `frames` placed as fuse_frames places them, and for method "occlusion" without depths of its own the depths are the
    frames' depths times `scale`; clean: a dict of clean_mesh keywords.  None leaves the mesh as it is"""
    if (cull is None and clean is None) or faces.shape[0] == 0:
        return vertices, colors, faces
    from . import cull_mesh as C
    if cull is not None and frames:
        cull = dict(cull)
        c2ws = np.stack([_placed(c.detach().cpu().numpy() if torch.is_tensor(c) else c, scale, transform)
                         for _, _, c in frames])
        H, W = frames[0][0].shape[-2:]
        if cull.get("method") == "occlusion" and cull.get("depths") is None:
            cull["depths"] = [L.f32(d) * float(scale) if float(scale) != 1.0 else L.f32(d) for d, _, _ in frames]
        vertices, faces, colors, _ = C.cull_mesh(vertices, faces, c2ws, _intrinsics(intrinsics), H, W, colors=colors, **cull)
    if clean is not None and faces.shape[0] > 0:
        vertices, faces, colors = C.clean_mesh(vertices, faces, colors, **clean)
    return vertices, colors, faces


# ---- PLY -------------------------------------------------------------------------------------------------------------
_VERTEX = np.dtype([("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("red", "u1"), ("green", "u1"), ("blue", "u1")])
_FACE = np.dtype([("n", "u1"), ("v", "<i4", (3,))])


def write_ply(path, vertices, faces, colors):
    """binary little-endian PLY: vertices float x y z with uchar red green blue (colors in [0,1], rounded to nearest),
    faces as lists of 3 int vertex_indices"""
    to_np = lambda t: t.detach().cpu().numpy() if torch.is_tensor(t) else np.asarray(t)
    vertices, faces, colors = to_np(vertices), to_np(faces), to_np(colors)
    v = np.zeros(len(vertices), _VERTEX)
    v["x"], v["y"], v["z"] = vertices[:, 0], vertices[:, 1], vertices[:, 2]
    rgb = np.clip(np.rint(colors.astype(np.float64) * 255.0), 0, 255).astype(np.uint8)
    v["red"], v["green"], v["blue"] = rgb[:, 0], rgb[:, 1], rgb[:, 2]
    f = np.zeros(len(faces), _FACE)
    f["n"] = 3
    f["v"] = faces
    header = ("ply\nformat binary_little_endian 1.0\n"
              f"element vertex {len(v)}\nproperty float x\nproperty float y\nproperty float z\n"
              "property uchar red\nproperty uchar green\nproperty uchar blue\n"
              f"element face {len(f)}\nproperty list uchar int vertex_indices\nend_header\n")
    with open(path, "wb") as fp:
        fp.write(header.encode("ascii"))
        fp.write(v.tobytes())
        fp.write(f.tobytes())


def read_ply(path):
    """what write_ply wrote -> (vertices f32 [V,3], faces int32 [F,3], colors uint8 [V,3])"""
    with open(path, "rb") as fp:
        data = fp.read()
    end = data.index(b"end_header\n") + len(b"end_header\n")
    header = data[:end].decode("ascii")
    if "format binary_little_endian 1.0" not in header:
        raise ValueError("not a binary little-endian PLY")
    n_v = int(re.search(r"element vertex (\d+)", header).group(1))
    n_f = int(re.search(r"element face (\d+)", header).group(1))
    v = np.frombuffer(data, _VERTEX, n_v, end)
    f = np.frombuffer(data, _FACE, n_f, end + n_v * _VERTEX.itemsize)
    if end + n_v * _VERTEX.itemsize + n_f * _FACE.itemsize != len(data) or (n_f and (f["n"] != 3).any()):
        raise ValueError("unexpected PLY layout")
    return (np.stack([v["x"], v["y"], v["z"]], 1).astype(np.float32), f["v"].astype(np.int32),
            np.stack([v["red"], v["green"], v["blue"]], 1))


def save_mesh(output, vertices, colors, faces, mesh_name_suffix="kf", scene="scene"):
    """mesh/{scene}_{suffix}.ply and mesh/vertices_pos_{suffix}.npy under `output`; -> the path of the PLY"""
    mesh_dir = os.path.join(str(output), "mesh")
    os.makedirs(mesh_dir, exist_ok=True)
    np.save(os.path.join(mesh_dir, f"vertices_pos_{mesh_name_suffix}.npy"), vertices.detach().cpu().numpy())
    path = os.path.join(mesh_dir, f"{scene}_{mesh_name_suffix}.ply")
    write_ply(path, vertices, faces, colors)
    return path


def generate_mesh_kf(output, intrinsics, scale=1.0, transform=None, rendered_path="rendered_every_keyframe",
                     mesh_name_suffix="kf", scene="scene", voxel_length=5.0 / 512.0, sdf_trunc=0.04, device="cuda",
                     max_blocks=None, cull=None, clean=None):
    """Reads output/{rendered_path}/{depth,color}_%05d.npy and output/video.npz; every map is matched to the keyframe
    pose with its timestamp (the reference's warm-up offset loop walks to the same pairs; a map without a keyframe is an
    error); depth and pose translation are multiplied by `scale`, then `transform` is applied (see the module text).
    cull / clean: dicts of cull_mesh / clean_mesh keywords (cull_and_clean; off by default: the raw extraction).
    Writes mesh/{scene}_{suffix}.ply and mesh/vertices_pos_{suffix}.npy; -> (vertices, colors, faces) on the device"""
    maps_dir = os.path.join(str(output), rendered_path)
    stamps = sorted(int(m.group(1)) for m in (re.fullmatch(r"depth_(\d{5,})\.npy", f) for f in os.listdir(maps_dir)) if m)
    video = np.load(os.path.join(str(output), "video.npz"))
    by_stamp = {int(t): i for i, t in enumerate(video["timestamps"])}
    frames = []
    for ts in stamps:
        if ts not in by_stamp:
            raise ValueError(f"no keyframe of video.npz has the timestamp {ts} of depth_{ts:05d}.npy")
        depth = torch.from_numpy(np.load(os.path.join(maps_dir, f"depth_{ts:05d}.npy"))).to(device, torch.float32)
        color = torch.from_numpy(np.load(os.path.join(maps_dir, f"color_{ts:05d}.npy"))).to(device, torch.float32)
        frames.append((depth, color, video["poses"][by_stamp[ts]]))
    vertices, colors, faces, _ = fuse_frames(frames, intrinsics, device, scale=scale, transform=transform,
                                             voxel_length=voxel_length, sdf_trunc=sdf_trunc, max_blocks=max_blocks)
    vertices, colors, faces = cull_and_clean(vertices, colors, faces, frames, intrinsics, scale, transform, cull, clean)
    save_mesh(output, vertices, colors, faces, mesh_name_suffix, scene)
    return vertices, colors, faces
