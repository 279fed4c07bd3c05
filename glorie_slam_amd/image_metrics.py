"""Image-quality metrics of the re-render evaluation on HIP kernels (csrc/metrics.hip; reference:
src/utils/eval_render.py:59-89, which calls pytorch_msssim.ms_ssim and torch's mse_loss).

  ms_ssim        MS-SSIM of two images with the defaults of pytorch_msssim (glorie_ms_ssim: levels + 1 launches)
  psnr           -10 log10 of the mean squared difference, over the frame or over a mask (glorie_frame_reduce: 2 launches)
  frame_metrics  everything eval_kf_imgs reports for one frame: psnr, ms_ssim, their masked forms, depth L1 and the masked
                 maps (glorie_frame_reduce, glorie_mask_apply, glorie_ms_ssim twice); with an lpips.Lpips also lpips
                 and masked_lpips (glorie_lpips twice)

Every sum is accumulated in fp64 from per-workgroup partials in a fixed order: repeated calls are bitwise equal, nothing
reads the device back, and every call records into a hipGraph.  Results are 0-dim float32 device tensors.

LPIPS is lpips.Lpips, built from weights the caller hands in (torchmetrics fetches AlexNet's from the network, this
package fetches nothing); without one the LPIPS values are left out.  Out of scope: the PNG copies of the renders (cv2).
"""
import torch

from . import _lib as L
from .color_grad import _layout

MS_SSIM_WEIGHTS = (0.0448, 0.2856, 0.3001, 0.2363, 0.1333)
WIN_SIZE = 11


def _pair(x, y):
    L.need_cuda(x, y)
    if tuple(x.shape) != tuple(y.shape):
        raise ValueError(f"images must have the same shape, got {tuple(x.shape)} and {tuple(y.shape)}")
    return L.f32(x), L.f32(y)


def ms_ssim(x, y, channels_first=False, levels=5, return_levels=False):
    """x, y f32 in [0,1], [H,W,3] (or [3,H,W] with channels_first) on the device -> the MS-SSIM as a 0-dim f32 tensor;
    with return_levels also [levels,2] f32: the channel means of (ssim, cs) of every level.  A non-contiguous or
    non-float32 input is copied first.  Like the library, 5 levels need a smaller side above 160; fewer levels (the
    first `levels` weights) need every level to keep 11 pixels"""
    x, y = _pair(x, y)
    if x.dim() != 3 or x.shape[0 if channels_first else 2] != 3:
        raise ValueError(f"images must be {'[3,H,W]' if channels_first else '[H,W,3]'}, got {tuple(x.shape)}")
    H, W = (x.shape[1], x.shape[2]) if channels_first else (x.shape[0], x.shape[1])
    levels = int(levels)
    if not 1 <= levels <= len(MS_SSIM_WEIGHTS):
        raise ValueError(f"levels must be in [1, {len(MS_SSIM_WEIGHTS)}], got {levels}")
    if min(H, W) <= (WIN_SIZE - 1) * 2 ** (levels - 1):
        # pytorch_msssim: "Image size should be larger than 160 due to the 4 downsamplings in ms-ssim"
        raise ValueError(f"image size should be larger than {(WIN_SIZE - 1) * 2 ** (levels - 1)} for {levels} levels, "
                         f"got {H}x{W}")
    dev = x.device
    lib = L.load()
    ws = L.workspace(lib.glorie_ms_ssim_workspace(int(H), int(W), levels), dev)
    out = torch.empty(1 + 2 * levels, dtype=torch.float32, device=dev)
    L.check(lib.glorie_ms_ssim(L.ptr(x), L.ptr(y), int(H), int(W), 1 if channels_first else 0, levels, L.ptr(ws),
                               L.ptr(out), L.stream_ptr(dev)), "glorie_ms_ssim")
    return (out[0], out[1:].view(levels, 2)) if return_levels else out[0]


def _hwc(x, name):
    if x.dim() != 3 or x.shape[2] != 3:
        raise ValueError(f"{name} must be [H,W,3], got {tuple(x.shape)}")


def _frame_reduce(a, b, mask, depth, gt_depth):
    """a, b [H,W,3] contiguous f32; mask u8 [H,W] or None -> (f32 [3] = psnr, masked_psnr, depth_l1; int32 [1] = count)"""
    H, W = a.shape[0], a.shape[1]
    dev = a.device
    lib = L.load()
    ws = L.workspace(lib.glorie_frame_reduce_workspace(int(H), int(W)), dev)
    out = torch.empty(3, dtype=torch.float32, device=dev)
    count = torch.empty(1, dtype=torch.int32, device=dev)
    L.check(lib.glorie_frame_reduce(L.ptr(a), L.ptr(b), int(H), int(W), L.ptr(mask), L.ptr(depth), L.ptr(gt_depth),
                                    L.ptr(ws), L.ptr(out), L.ptr(count), L.stream_ptr(dev)), "glorie_frame_reduce")
    return out, count


def _mask_u8(mask, H, W):
    if tuple(mask.shape) != (H, W):
        raise ValueError(f"mask must be [{H},{W}], got {tuple(mask.shape)}")
    return (mask if mask.dtype == torch.bool else mask != 0).contiguous().view(torch.uint8)


def psnr(x, y, mask=None):
    """x, y f32 [H,W,3] on the device -> -10 log10(mean((x - y)^2)) as a 0-dim f32 tensor; with mask [H,W] the mean is
    over its pixels (NaN on an empty mask, as mse_loss of an empty selection)"""
    x, y = _pair(x, y)
    _hwc(x, "images")
    L.need_cuda(mask)
    m = _mask_u8(mask, x.shape[0], x.shape[1]) if mask is not None else None
    out, _ = _frame_reduce(x, y, m, None, None)
    return out[1] if mask is not None else out[0]


def mask_apply(mask, depth=None, color_a=None, color_b=None):
    """copies of depth [H,W] and the colour images [H,W,3] with 0 where mask [H,W] is False (x[~mask] = 0 on a clone);
    None stays None"""
    L.need_cuda(mask, depth, color_a, color_b)
    H, W = mask.shape
    m = _mask_u8(mask, H, W)
    src = [L.f32(t) if t is not None else None for t in (depth, color_a, color_b)]
    for t, shape in zip(src, ((H, W), (H, W, 3), (H, W, 3))):
        if t is not None and tuple(t.shape) != shape:
            raise ValueError(f"expected {shape}, got {tuple(t.shape)}")
    dst = [torch.empty_like(t) if t is not None else None for t in src]
    L.check(L.load().glorie_mask_apply(L.ptr(m), int(H), int(W), *[L.ptr(t) for t in src], *[L.ptr(t) for t in dst],
                                       L.stream_ptr(mask.device)), "glorie_mask_apply")
    return tuple(dst)


def frame_metrics(render_color, render_depth, gt_color, mask, gt_depth=None, lpips=None):
    """What eval_kf_imgs computes for one frame (eval_render.py:59-89).  render_color, gt_color [H,W,3], render_depth
    [H,W], mask [H,W] bool, gt_depth [H,W] or None, all on the device; the inputs are not modified.
    -> dict of 0-dim f32 device tensors psnr, ms_ssim, masked_psnr, masked_ms_ssim, depth_l1 (only with gt_depth: the
    mean |render_depth - gt_depth| over the mask), the int32 [1] mask_count, and the masked maps depth [H,W] and
    color, gt_color [H,W,3] (0 outside the mask).  masked_ms_ssim is, as in the reference, the full-frame MS-SSIM of
    the two masked images, not a mean over the mask.  lpips: an lpips.Lpips adds lpips and masked_lpips (eval_render.py:64-65,
    :85-86), the latter likewise of the two masked images; None leaves both out and launches nothing more"""
    render_color, gt_color = _pair(render_color, gt_color)
    _hwc(render_color, "render_color")
    L.need_cuda(render_depth, mask, gt_depth)
    H, W = render_color.shape[0], render_color.shape[1]
    m = _mask_u8(mask, H, W)
    depth = L.f32(render_depth)
    gt_d = L.f32(gt_depth) if gt_depth is not None else None
    for name, d in (("render_depth", depth), ("gt_depth", gt_d)):
        if d is not None and tuple(d.shape) != (H, W):
            raise ValueError(f"{name} must be [{H},{W}], got {tuple(d.shape)}")
    sums, count = _frame_reduce(gt_color, render_color, m, depth if gt_d is not None else None, gt_d)
    out = {"psnr": sums[0], "ms_ssim": ms_ssim(gt_color, render_color), "masked_psnr": sums[1]}
    m_depth, m_color, m_gt = mask_apply(mask, depth, render_color, gt_color)
    out["masked_ms_ssim"] = ms_ssim(m_gt, m_color)
    if gt_d is not None:
        out["depth_l1"] = sums[2]
    if lpips is not None:
        out["lpips"] = lpips(gt_color, render_color)
        out["masked_lpips"] = lpips(m_gt, m_color)
    out.update(mask_count=count, depth=m_depth, color=m_color, gt_color=m_gt)
    return out
