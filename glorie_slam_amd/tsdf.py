"""Block-sparse TSDF fusion and mesh extraction on HIP kernels (csrc/tsdf.hip; reference: src/utils/generate_mesh.py,
which hands the re-rendered keyframes to Open3D's TSDF integration and mesh extraction).

  TSDFVolume             the volume: integrate(depth, color, c2w, intrinsics) per frame, extract() -> the triangle mesh
  TSDFVolume.from_dense  a volume over a grid the caller already holds
  depth_bounds           a bound that encloses the back-projected valid pixels of a list of frames

The volume is a dense int32 block table over a caller-given bound (rounded outwards to whole blocks of 8 x 8 x 8 voxels)
and a pool of max_blocks blocks; voxel (i,j,k) samples origin + (i + 0.5, j + 0.5, k + 0.5) * voxel_length.  The update
rule and the extraction (marching tetrahedra on the Kuhn split of every cell, indexed output in a canonical order) are
stated in include/glorie_hip.h.  One thread owns one voxel and every index comes from integer scans: repeated runs are
bitwise equal whatever the order the blocks were allocated in.

Deviation from Open3D: the update is the uniform-volume rule as the reference drives it (RGB8 colour, depth_trunc 30) on
blocks allocated around the back-projected pixels, and the surface comes from marching tetrahedra, not marching cubes -
parity with Open3D's own output is not pinned.  Vertices lie on the voxel-centre lattice this volume samples, so the
half-voxel compensation the reference adds after Open3D's extraction has no counterpart here.
"""
import ctypes

import numpy as np
import torch

from . import _lib as L

BLOCK = 8
BLOCK_VOXELS = BLOCK ** 3


def _intrinsics(intrinsics):
    if torch.is_tensor(intrinsics):
        intrinsics = intrinsics.detach().cpu().tolist()
    # rounded to fp32, what the kernels take: the bound of depth_bounds must not depend on how the caller held them
    fx, fy, cx, cy = (float(np.float32(v)) for v in intrinsics)
    return fx, fy, cx, cy


def depth_bounds(frames, intrinsics, margin, depth_trunc=30.0):
    """frames: iterable of (depth [H,W], c2w [4,4], OpenCV convention) tensors or arrays -> (bounds_min, bounds_max), two
    float64 [3] arrays that enclose the back-projected pixels with 0 < depth <= depth_trunc, grown by `margin` (at least
    the truncation distance, so that no pixel's box leaves the bound)"""
    fx, fy, cx, cy = _intrinsics(intrinsics)
    lo, hi = np.full(3, np.inf), np.full(3, -np.inf)
    for depth, c2w in frames:
        depth = torch.as_tensor(depth).detach().double()
        c2w = torch.as_tensor(c2w).detach().double().to(depth.device)
        H, W = depth.shape
        v, u = torch.meshgrid(torch.arange(H, device=depth.device, dtype=torch.float64),
                              torch.arange(W, device=depth.device, dtype=torch.float64), indexing="ij")
        keep = (depth > 0) & (depth <= depth_trunc)
        if not bool(keep.any()):
            continue
        d = depth[keep]
        cam = torch.stack([(u[keep] - cx) / fx * d, (v[keep] - cy) / fy * d, d], 1)
        p = cam @ c2w[:3, :3].T + c2w[:3, 3]
        lo = np.minimum(lo, p.min(0).values.cpu().numpy())
        hi = np.maximum(hi, p.max(0).values.cpu().numpy())
    if not np.isfinite(lo).all():
        raise ValueError("no frame has a pixel with 0 < depth <= depth_trunc")
    return lo - float(margin), hi + float(margin)


class TSDFVolume:
    """voxel_length, sdf_trunc in the unit of the poses; bounds_min, bounds_max: the axis-aligned bound (3 numbers each),
    rounded outwards to whole blocks from bounds_min; max_blocks: the capacity of the pool (20 B per voxel: 10 KiB per
    block)."""

    def __init__(self, voxel_length, sdf_trunc, bounds_min, bounds_max, max_blocks, device, depth_trunc=30.0):
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise L.GlorieError("TSDFVolume lives on the device (there is no CPU fallback on the product path)")
        self.voxel_length, self.sdf_trunc, self.depth_trunc = float(voxel_length), float(sdf_trunc), float(depth_trunc)
        if not (self.voxel_length > 0 and self.sdf_trunc > 0 and int(max_blocks) > 0):
            raise ValueError("voxel_length, sdf_trunc and max_blocks must be positive")
        lo, hi = np.asarray(bounds_min, np.float64), np.asarray(bounds_max, np.float64)
        if lo.shape != (3,) or hi.shape != (3,) or not (hi > lo).all():
            raise ValueError("bounds_min and bounds_max must be 3 numbers each with bounds_max > bounds_min")
        nb = np.maximum(1, np.ceil((hi - lo) / (BLOCK * self.voxel_length) - 1e-6)).astype(np.int64)
        if int(nb.prod()) > 2 ** 31 - 1024:
            raise ValueError(f"the block table would have {int(nb.prod())} entries: enlarge voxel_length or shrink the bound")
        self.origin = lo
        self.blocks_per_axis = tuple(int(n) for n in nb)                      # nbx, nby, nbz
        self.max_blocks = int(max_blocks)
        dev = self.device
        self.table = torch.full((self.blocks_per_axis[2], self.blocks_per_axis[1], self.blocks_per_axis[0]), -1,
                                dtype=torch.int32, device=dev)
        self.block_index = torch.zeros(self.max_blocks, dtype=torch.int32, device=dev)
        self.tsdf = torch.zeros(self.max_blocks, BLOCK_VOXELS, dtype=torch.float32, device=dev)
        self.weight = torch.zeros(self.max_blocks, BLOCK_VOXELS, dtype=torch.float32, device=dev)
        self.rgb = torch.zeros(self.max_blocks, BLOCK_VOXELS, 3, dtype=torch.float32, device=dev)
        self.counters = torch.zeros(8, dtype=torch.int32, device=dev)
        self.n_blocks = 0
        self.frames = 0
        self._origin_f = (ctypes.c_float * 3)(*[float(v) for v in lo])
        self._origin_d = (ctypes.c_double * 3)(*[float(v) for v in lo])
        self._nb = (ctypes.c_int * 3)(*self.blocks_per_axis)
        self._alloc_ws = None

    # ---- fusion -------------------------------------------------------------------------------------------------------
    def integrate(self, depth, color, c2w, intrinsics, convention="opencv"):
        """depth f32 [H,W], color f32 [H,W,3] in [0,1], c2w [4,4] or [3,4] rigid camera-to-world, intrinsics (fx, fy, cx,
        cy), all tensors on the volume's device.  convention "opengl": columns 1 and 2 of c2w are negated first (a copy).
        Allocates the blocks around the frame's pixels, then updates every allocated block the frame can see.  A frame
        that needs more blocks than the pool has left raises GlorieError (GLORIE_ENOMEM) and changes nothing"""
        L.need_cuda(depth, color, c2w)
        if convention not in ("opencv", "opengl"):
            raise ValueError(f"convention must be 'opencv' or 'opengl', got {convention!r}")
        depth, color = L.f32(depth), L.f32(color)
        if depth.dim() != 2 or tuple(color.shape) != tuple(depth.shape) + (3,):
            raise ValueError(f"depth must be [H,W] and color [H,W,3], got {tuple(depth.shape)} and {tuple(color.shape)}")
        c2w = L.homogeneous(c2w)
        if c2w.dim() != 2:
            raise ValueError(f"c2w must be one matrix, got {tuple(c2w.shape)}")
        if convention == "opengl":
            c2w = c2w.clone()
            c2w[:3, 1:3] *= -1
        fx, fy, cx, cy = _intrinsics(intrinsics)
        H, W = depth.shape
        dev = self.device
        lib = L.load()
        if self._alloc_ws is None:
            self._alloc_ws = L.workspace(lib.glorie_tsdf_allocate_workspace(self.table.numel()), dev)
        n = ctypes.c_int(0)
        L.check(lib.glorie_tsdf_allocate(L.ptr(depth), int(H), int(W), L.ptr(c2w), fx, fy, cx, cy, self.depth_trunc,
                                         self.sdf_trunc, self._origin_f, self.voxel_length, self._nb, L.ptr(self.table),
                                         L.ptr(self.block_index), self.max_blocks, L.ptr(self.counters),
                                         L.ptr(self._alloc_ws), ctypes.byref(n), L.stream_ptr(dev)),
                "glorie_tsdf_allocate")
        self.n_blocks = int(n.value)
        L.check(lib.glorie_tsdf_integrate(L.ptr(depth), L.ptr(color), int(H), int(W), L.ptr(c2w), fx, fy, cx, cy,
                                          self.depth_trunc, self.sdf_trunc, self._origin_f, self.voxel_length, self._nb,
                                          L.ptr(self.block_index), self.n_blocks, L.ptr(self.tsdf), L.ptr(self.weight),
                                          L.ptr(self.rgb), L.ptr(self.counters), L.stream_ptr(dev)),
                "glorie_tsdf_integrate")
        self.frames += 1

    @property
    def stats(self):
        """{"blocks": blocks in use, "pixels_outside": pixels whose box left the bound (all frames), "frames": frames
        integrated, "blocks_visited": blocks that passed the culling of the last frame} (one read-back)"""
        c = self.counters.cpu().tolist()
        return {"blocks": c[0], "pixels_outside": c[1], "frames": self.frames, "blocks_visited": c[3]}

    # ---- read-out -----------------------------------------------------------------------------------------------------
    def blocks(self):
        """-> (coords int32 [n,3] = (bx, by, bz) of every block in id order, tsdf [n,8,8,8], weight [n,8,8,8], rgb
        [n,8,8,8,3]; the 8 x 8 x 8 axes are z, y, x) as views of the pool"""
        n = self.n_blocks
        nbx, nby, _ = self.blocks_per_axis
        idx = self.block_index[:n]
        coords = torch.stack([idx % nbx, (idx // nbx) % nby, idx // (nbx * nby)], 1).to(torch.int32)
        return (coords, self.tsdf[:n].view(n, BLOCK, BLOCK, BLOCK), self.weight[:n].view(n, BLOCK, BLOCK, BLOCK),
                self.rgb[:n].view(n, BLOCK, BLOCK, BLOCK, 3))

    def extract(self):
        """-> (vertices f32 [V,3], colors f32 [V,3] in [0,1], faces int32 [F,3]) on the device: marching tetrahedra over
        every cell whose 8 corners carry weight; a count pass, one read-back of (V, F), an emit pass"""
        dev = self.device
        lib = L.load()
        ws = L.workspace(lib.glorie_tsdf_extract_workspace(self.table.numel(), self.n_blocks), dev)
        counts = (ctypes.c_int * 2)()
        L.check(lib.glorie_tsdf_extract_count(self._origin_f, self.voxel_length, self._nb, L.ptr(self.table),
                                              self.n_blocks, L.ptr(self.tsdf), L.ptr(self.weight), L.ptr(ws), counts,
                                              L.stream_ptr(dev)), "glorie_tsdf_extract_count")
        V, F = int(counts[0]), int(counts[1])
        vertices = torch.empty(V, 3, dtype=torch.float32, device=dev)
        colors = torch.empty(V, 3, dtype=torch.float32, device=dev)
        faces = torch.empty(F, 3, dtype=torch.int32, device=dev)
        if V or F:
            L.check(lib.glorie_tsdf_extract_emit(self._origin_d, self.voxel_length, self._nb, L.ptr(self.table),
                                                 self.n_blocks, L.ptr(self.tsdf), L.ptr(self.weight), L.ptr(self.rgb),
                                                 L.ptr(ws), L.ptr(vertices), L.ptr(colors), L.ptr(faces),
                                                 L.stream_ptr(dev)), "glorie_tsdf_extract_emit")
        return vertices, colors, faces

    # ---- a grid the caller already holds ------------------------------------------------------------------------------
    @classmethod
    def from_dense(cls, tsdf, weight, rgb, origin, voxel_length, sdf_trunc):
        """tsdf, weight [Z,Y,X], rgb [Z,Y,X,3] (0..255) device tensors; voxel (i,j,k) = tsdf[k,j,i] samples
        origin + (i + 0.5, j + 0.5, k + 0.5) * voxel_length.  The grid is padded with weight 0 to whole blocks; blocks
        exist where any weight in them is positive, with ids ascending in the table index"""
        L.need_cuda(tsdf, weight, rgb)
        tsdf, weight, rgb = L.f32(tsdf), L.f32(weight), L.f32(rgb)
        if tsdf.dim() != 3 or weight.shape != tsdf.shape or tuple(rgb.shape) != tuple(tsdf.shape) + (3,):
            raise ValueError("tsdf and weight must be [Z,Y,X] and rgb [Z,Y,X,3]")
        Z, Y, X = tsdf.shape
        nb = [-(-s // BLOCK) for s in (X, Y, Z)]
        pad = (0, nb[0] * BLOCK - X, 0, nb[1] * BLOCK - Y, 0, nb[2] * BLOCK - Z)
        F = torch.nn.functional

        def blocked(t, channels):
            t = F.pad(t, ((0, 0) if channels else ()) + pad)
            t = t.view(nb[2], BLOCK, nb[1], BLOCK, nb[0], BLOCK, *((3,) if channels else ()))
            return t.permute(0, 2, 4, 1, 3, 5, *((6,) if channels else ())).reshape(-1, BLOCK_VOXELS, *((3,) if channels else ()))
        b_tsdf, b_weight, b_rgb = blocked(tsdf, False), blocked(weight, False), blocked(rgb, True)
        live = torch.nonzero((b_weight > 0).any(1))[:, 0]
        n = int(live.numel())
        origin = np.asarray(origin, np.float64)
        hi = origin + np.array(nb, np.float64) * BLOCK * float(voxel_length)
        vol = cls(voxel_length, sdf_trunc, origin, hi, max(n, 1), tsdf.device)
        assert vol.blocks_per_axis == tuple(nb)
        vol.table.view(-1)[live] = torch.arange(n, dtype=torch.int32, device=tsdf.device)
        vol.block_index[:n] = live.to(torch.int32)
        vol.tsdf[:n], vol.weight[:n], vol.rgb[:n] = b_tsdf[live], b_weight[live], b_rgb[live]
        vol.counters[0] = n
        vol.n_blocks = n
        return vol
