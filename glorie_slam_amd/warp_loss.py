"""Pixel-warping loss of the mapper on HIP kernels (csrc/warp.hip; reference: src/mapper.py:326-388, projection
src/utils/common.py:324-350).

`pix_warping_loss` has the reference method's argument list and return (the scalar loss, differentiable with respect to
`depth` only).  Forward: glorie_pix_warp_fwd (two launches: per-ray loss, kept count and raw gradient; one workgroup
reducing the partials in a fixed order).  Backward: glorie_pix_warp_bwd (one launch: raw gradient x g_out / (3 count)).
The kept-entry count never leaves the device and no output is sized by the data, so the term records into the mapping
iteration's hipGraph.

Images: a [M,H,W,3] tensor (the reference layout), a [M,3,H,W] tensor with channels_first=True, or a `FrameTable` of
per-frame images (SequenceRunner's [3,H,W] keyframe images, no stack or transpose per iteration).
"""
import torch

from . import _lib as L

MAX_FRAMES = 64


class FrameTable:
    """device table of per-frame image pointers: images is a sequence of M float32 tensors, each [3,H,W]
    (channels_first) or [H,W,3].  Holds references to the images; build it once per window (one host-to-device copy)."""

    def __init__(self, images, channels_first=True):
        if not images:
            raise ValueError("FrameTable needs at least one image")
        self.images = [L.f32(im) for im in images]
        shape = self.images[0].shape
        for im in self.images:
            L.need_cuda(im)
            if im.shape != shape or im.dim() != 3:
                raise ValueError(f"FrameTable images must share one 3-d shape, got {tuple(im.shape)} and {tuple(shape)}")
        self.channels_first = bool(channels_first)
        self.H, self.W = (shape[1], shape[2]) if channels_first else (shape[0], shape[1])
        dev = self.images[0].device
        self.table = torch.tensor([im.data_ptr() for im in self.images], dtype=torch.int64).to(dev)

    def __len__(self):
        return len(self.images)


class PixWarpLoss(torch.autograd.Function):
    """(depth, meta) -> (loss, count); gradient with respect to depth only"""

    @staticmethod
    def forward(ctx, depth, meta):
        rays_o, rays_d, ray_frame, c2ws, frame_indices, images, table, chw, H, W, K, gt, nan_to_zero = meta
        dev = depth.device
        N, M = depth.shape[0], c2ws.shape[0]
        lib = L.load()
        depth_c = L.f32(depth)
        ws = L.workspace(lib.glorie_pix_warp_workspace(N), dev)
        loss = torch.empty((), dtype=torch.float32, device=dev)
        scale = torch.empty(1, dtype=torch.float32, device=dev)
        count = torch.empty(1, dtype=torch.int32, device=dev)
        raw = torch.empty(N, dtype=torch.float32, device=dev)
        L.check(lib.glorie_pix_warp_fwd(L.ptr(rays_o), L.ptr(rays_d), L.ptr(depth_c), L.ptr(ray_frame), N, L.ptr(c2ws),
                                        L.ptr(frame_indices), M, L.ptr(images), L.ptr(table), int(chw), H, W,
                                        *(float(k) for k in K), L.ptr(gt), int(nan_to_zero), L.ptr(ws), L.ptr(loss),
                                        L.ptr(raw), L.ptr(scale), L.ptr(count), L.stream_ptr(dev)),
                "glorie_pix_warp_fwd")
        ctx.save_for_backward(raw, scale)
        ctx.depth_dtype = depth.dtype
        ctx.mark_non_differentiable(count)
        return loss, count

    @staticmethod
    def backward(ctx, g_loss, g_count):
        raw, scale = ctx.saved_tensors
        g = g_loss.reshape(1).float().contiguous()
        grad = torch.empty_like(raw)
        L.check(L.load().glorie_pix_warp_bwd(L.ptr(raw), L.ptr(scale), L.ptr(g), raw.shape[0], L.ptr(grad),
                                             L.stream_ptr(raw.device)), "glorie_pix_warp_bwd")
        return grad.to(ctx.depth_dtype), None


def pix_warping_loss(batch_rays_o, batch_rays_d, depth, c2ws, fx, fy, cx, cy, W, H, frame_indices, indices_tensor,
                     img_gt_colors, batch_gt_color, nan_to_zero=False, channels_first=False, return_count=False):
    """Mapper.pix_warping_loss (mapper.py:326-388) on the HIP kernels.
    batch_rays_o, batch_rays_d [N,3]; depth [N] (the rendered depth: the gradient flows into it); c2ws [M,4,4] or
    [M,3,4]; frame_indices [M] and indices_tensor [N] (the ray's own frame) int64; img_gt_colors [M,H,W,3] (or
    [M,3,H,W] with channels_first, or a FrameTable); batch_gt_color [N,3].
    Returns the scalar loss: NaN for an empty selection as in the reference, 0 with nan_to_zero (the gradient is zero
    either way).  return_count: also the number of kept (ray, frame) entries as a [1] int32 device tensor."""
    L.need_cuda(batch_rays_o, batch_rays_d, depth, c2ws, frame_indices, indices_tensor, batch_gt_color)
    N, M = depth.shape[0], c2ws.shape[0]
    if not 0 <= M <= MAX_FRAMES:
        raise ValueError(f"pix_warping_loss supports up to {MAX_FRAMES} frames, got {M}")
    if batch_rays_o.shape != (N, 3) or batch_rays_d.shape != (N, 3) or batch_gt_color.shape != (N, 3) \
            or indices_tensor.shape != (N,) or frame_indices.shape != (M,):
        raise ValueError("pix_warping_loss: inconsistent ray / frame shapes")
    if isinstance(img_gt_colors, FrameTable):
        if len(img_gt_colors) != M or (img_gt_colors.H, img_gt_colors.W) != (H, W):
            raise ValueError("FrameTable does not match the frames / image size")
        images, table, chw = None, img_gt_colors.table, img_gt_colors.channels_first
    else:
        L.need_cuda(img_gt_colors)
        want = (M, 3, H, W) if channels_first else (M, H, W, 3)
        if tuple(img_gt_colors.shape) != want:
            raise ValueError(f"img_gt_colors must be {want}, got {tuple(img_gt_colors.shape)}")
        images, table, chw = L.f32(img_gt_colors), None, channels_first
    meta = (L.f32(batch_rays_o), L.f32(batch_rays_d), indices_tensor.long().contiguous(), L.homogeneous(c2ws),
            frame_indices.long().contiguous(), images, table, chw, int(H), int(W), (fx, fy, cx, cy),
            L.f32(batch_gt_color), nan_to_zero)
    loss, count = PixWarpLoss.apply(depth, meta)
    return (loss, count) if return_count else loss
