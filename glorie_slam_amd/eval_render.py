"""Re-render evaluation at the end of a run (reference: src/utils/eval_render.py:18-124 eval_kf_imgs, :126-247 eval_imgs,
bound to Mapper at src/mapper.py:858-859): every mapped keyframe - or every `every_frame`-th frame of the stream with its
estimated pose - is rendered through the full renderer and scored against the input image with the kernels of
image_metrics.py; the masked depth and colour maps that meshing reads and the metrics file are written under `output`.

  eval_kf_imgs(runner)                                   the keyframes, on the view the mapper trained on
  eval_imgs(runner, frames, est_c2ws, every_frame)       arbitrary frames with given poses, on the projected cloud depth

Both return {"frames": [{"video_idx", "tstamp", "psnr", "ms_ssim", "masked_psnr", "masked_ms_ssim"[, "depth_l1"][, "lpips",
"masked_lpips"]}],
"avg_psnr", "avg_ms_ssim", "avg_masked_psnr", "avg_masked_ms_ssim", "avg_depth_l1" (None without gt depth), "frame_cnt"}.
The per-frame values stay on the device and are read back once at the end; the runner, its images and the cloud are only
read.

With save_png the unmasked render of every frame is also written as a PNG, as the reference does through cv2
(eval_render.py:54-57, :178-181): rerendered_keyframe_image/frame_%05d.png for the keyframes, rerendered_image/frame_%05d.png
for eval_imgs, the bytes of visualizer.to_rgb8 (saturate(rint(255 x)), RGB), written with PIL.

LPIPS (eval_render.py:27-28, :64-65, :85-86) needs AlexNet's weights, which torchmetrics fetches from the network and this
package does not: with lpips = an lpips.Lpips built from the caller's weights every frame also carries "lpips" and
"masked_lpips", the result "avg_lpips" and "avg_masked_lpips", and the metrics files the reference's avg_masked_lpips /
avg_lpips lines in its line order.  Without it (the default) they keep the reference's names and order minus those
lines.  The mesh that reads the saved maps: generate_mesh.py.
"""
import os
import shutil

import numpy as np
import torch

from .color_grad import color_grad_maps
from .common import align_scale_and_shift
from .image_metrics import frame_metrics
from .neural_point import proj_depth_map

_KEYS = ("psnr", "ms_ssim", "masked_psnr", "masked_ms_ssim", "depth_l1")
_LPIPS_KEYS = ("lpips", "masked_lpips")


def _constant_radius(runner, like):
    """the radius every training ray carries when the colour-gradient radii are off (SequenceRunner._keyframe_rays)"""
    npc = runner.npc
    if not npc.use_dynamic_radius:
        return None
    return torch.full_like(like, 0.5 * (npc.radius_add + npc.radius_query))


def _score(runner, c2w, render_depth, r_query, gt_color, gt_depth, lpips=None):
    """render one view and score it: (metrics of frame_metrics, unmasked render colour, render depth, mask)"""
    ren, npc = runner.renderer, runner.npc
    depth, _, color, valid_ray_mask, _ = ren.render_img(npc, runner.decoders, c2w, runner.device, stage="color",
                                                        gt_depth=render_depth, npc_geo_feats=npc.get_geo_feats(),
                                                        npc_col_feats=npc.get_col_feats(), dynamic_r_query=r_query,
                                                        cloud_pos=npc.cloud_pos())
    mask = (valid_ray_mask > 0) & (render_depth > 0)
    if gt_depth is not None:
        mask = mask & (gt_depth > 0)
    return frame_metrics(color, depth, gt_color, mask, gt_depth=gt_depth, lpips=lpips), color, depth, mask


def _evaluate(runner, views, output, subdir, log_name, ssim_label, gt_depth_fn, keep_renders, png_subdir=None, lpips=None):
    """views: iterable of (video_idx or None, tstamp, gt_color [H,W,3], c2w, render_depth [H,W], r_query [H,W] or None);
    png_subdir: with `output`, the directory under it that receives frame_%05d.png of every unmasked render"""
    dev = runner.device
    png_dir = None
    if output is not None and png_subdir is not None:
        from .visualizer import save_image, to_rgb8
        png_dir = os.path.join(str(output), png_subdir)
        os.makedirs(png_dir, exist_ok=True)
    if output is not None:
        maps_dir = os.path.join(str(output), subdir)
        if os.path.exists(maps_dir):
            shutil.rmtree(maps_dir)
        os.makedirs(maps_dir)
        os.makedirs(os.path.join(str(output), "logs"), exist_ok=True)
    keys = _KEYS if gt_depth_fn is not None else _KEYS[:4]
    if lpips is not None:
        keys = keys + _LPIPS_KEYS
    frames, rows = [], []
    with torch.no_grad():
        for video_idx, tstamp, gt_color, c2w, render_depth, r_query in views:
            gt_depth = gt_depth_fn(tstamp).to(dev, torch.float32) if gt_depth_fn is not None else None
            m, color, depth, mask = _score(runner, c2w, render_depth, r_query, gt_color, gt_depth, lpips)
            rows.append(torch.stack([m[k] for k in keys]))
            frame = {"video_idx": video_idx, "tstamp": tstamp}
            if keep_renders:
                frame["render"] = {"color": color, "depth": depth, "mask": mask}
            frames.append(frame)
            if output is not None:
                np.save(os.path.join(maps_dir, f"depth_{int(tstamp):05d}"), m["depth"].cpu().numpy())
                np.save(os.path.join(maps_dir, f"color_{int(tstamp):05d}"), m["color"].cpu().numpy())
            if png_dir is not None:
                save_image(os.path.join(png_dir, f"frame_{int(tstamp):05d}.png"), to_rgb8(color))
    values = torch.stack(rows).double().cpu().numpy() if rows else np.zeros((0, len(keys)))      # the one read-back
    for frame, row in zip(frames, values):
        frame.update({k: float(v) for k, v in zip(keys, row)})
    out = {"frames": frames, "frame_cnt": len(frames), "avg_depth_l1": None}
    with np.errstate(invalid="ignore"):
        for j, k in enumerate(keys):
            out[f"avg_{k}"] = float(values[:, j].sum() / len(frames)) if frames else float("nan")
    if output is not None:
        masked_lpips = f"avg_masked_lpips: {out['avg_masked_lpips']}\n" if lpips is not None else ""
        full_lpips = f"avg_lpips: {out['avg_lpips']}\n" if lpips is not None else ""
        text = (f"avg_masked_{ssim_label}: {out['avg_masked_ms_ssim']}\navg_masked_psnr: {out['avg_masked_psnr']}\n"
                f"{masked_lpips}###############\navg_{ssim_label}: {out['avg_ms_ssim']}\navg_psnr: {out['avg_psnr']}\n"
                f"{full_lpips}###############\n")
        with open(os.path.join(str(output), "logs", log_name), "w+") as fp:
            fp.write(text)
    return out


def eval_kf_imgs(runner, output=None, gt_depth_fn=None, keep_renders=False, save_png=False, lpips=None):
    """eval_kf_imgs (eval_render.py:18-124) over the mapped keyframes of a SequenceRunner that were not skipped.  Each is
    rendered on the view the mapper trained it on - with render_depth its proxy / aligned mono depth, else the tracker's
    depth - with its own dynamic_r_query / 3 * render_depth when the colour-gradient radii are on.  The mask is
    valid_ray_mask > 0 & render_depth > 0 (& gt_depth > 0 when gt_depth_fn(tstamp) -> [H,W] is given; without it
    depth_l1 is left out).  output: writes rendered_every_keyframe/{depth,color}_%05d.npy (the masked maps, by
    timestamp) and logs/metrics_render_kf.txt.  keep_renders: every frame also carries "render" = the unmasked colour,
    the depth and the mask as device tensors.  save_png with output: rerendered_keyframe_image/frame_%05d.png, the
    unmasked render colour of every keyframe (by timestamp).  lpips: an lpips.Lpips adds the LPIPS values and lines"""
    def views():
        for k in range(runner.mapped):
            if k in runner.skipped:
                continue
            if runner.render_depth is not None:
                got = runner._frame_depths(k)
                if got is None:
                    continue
                c2w, render_depth = got[0], runner._render_depth_of(*got)
            else:
                render_depth, c2w = runner._keyframe_view(k)
            if runner.color_grad is not None:
                r_query = runner._radius_maps(k, (render_depth, c2w), add=False)[1]
            else:
                r_query = _constant_radius(runner, render_depth)
            gt_color = runner.images[k].permute(1, 2, 0).contiguous()
            yield k, float(runner.video.timestamp[k]), gt_color, c2w, render_depth, r_query

    return _evaluate(runner, views(), output, "rendered_every_keyframe", "metrics_render_kf.txt", "ssim", gt_depth_fn,
                     keep_renders, "rerendered_keyframe_image" if save_png else None, lpips=lpips)


def eval_imgs(runner, frames, est_c2ws, every_frame, output=None, gt_depth_fn=None, keep_renders=False, save_png=False,
              lpips=None):
    """eval_imgs (eval_render.py:126-247): frames is an iterable of (idx, image [1,3,H,W] or [3,H,W] in [0,1]), est_c2ws[idx]
    the estimated camera-to-world matrix [4,4] (OpenCV convention, flipped to OpenGL here); every `every_frame`-th frame
    is rendered on the depth of the projected cloud (proj_depth_map; the neural points when the runner keeps no
    unprojected keyframe maps), its holes filled from the mono prior aligned on the projected pixels
    (align_scale_and_shift), with the query radii of the frame's own colour gradients.  output: writes
    rendered_every_frame/{depth,color}_%05d.npy and logs/metrics_render_every.txt, and with save_png
    rerendered_image/frame_%05d.png, the unmasked render colour of every rendered frame.  lpips: an lpips.Lpips adds the
    LPIPS values and lines"""
    dev = runner.device
    cfg = runner._mono_cfg()
    cfg["mapping"] = dict(cfg["mapping"], mapping_window_size=runner.mapping_window_size)
    npc = runner.npc

    def views():
        for idx, image in frames:
            if int(idx) % int(every_frame) != 0:
                continue
            image = image.to(dev, torch.float32)
            image = image[0] if image.dim() == 4 else image
            c2w = torch.as_tensor(est_c2ws[int(idx)]).detach().to(dev, torch.float32).clone()    # (the caller's stays)
            c2w[:3, 1:3] *= -1
            mono = runner.mono_depth_fn(idx, image).to(dev, torch.float32)
            if npc.full_pcl() is not None and npc.video is not None:
                proj = proj_depth_map(c2w, npc, dev, cfg)
            else:
                proj = proj_depth_map(c2w, npc, dev, cfg, neural_pcl=True)
            proj_valid = proj > 0
            scale, shift, _ = align_scale_and_shift(mono, proj, proj_valid)
            render_depth = torch.where(proj_valid, proj, scale * mono + shift)
            if runner.color_grad is not None:
                r_query = color_grad_maps(image, depth_query=render_depth, outputs=("r_query",),
                                          **runner.color_grad)["r_query"]
            else:
                r_query = _constant_radius(runner, render_depth)
            yield None, float(idx), image.permute(1, 2, 0).contiguous(), c2w, render_depth, r_query

    return _evaluate(runner, views(), output, "rendered_every_frame", "metrics_render_every.txt", "msssim", gt_depth_fn,
                     keep_renders, "rerendered_image" if save_png else None, lpips=lpips)
