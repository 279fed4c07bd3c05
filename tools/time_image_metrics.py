"""Device time of the image-metric kernels (glorie_slam_amd/image_metrics.py) against the torch composition of the same
formula in the same process, and of one keyframe's re-render evaluation split into render and metrics.

    python tools/time_image_metrics.py [--reps 100]

  ms_ssim, frame_metrics   at 640x480 and 1200x680: eager calls and replays of one hipGraph, device time per call from
                           events around `reps` back-to-back calls; the bar is `torch composition` on the same line: MS-SSIM
                           as depthwise conv2d + avg_pool2d in float32 on the device (what pytorch_msssim launches)
  eval_kf_imgs             one keyframe of the synthetic 640x480 stream: render_img alone, frame_metrics alone
"""
import argparse
import os
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

WEIGHTS = (0.0448, 0.2856, 0.3001, 0.2363, 0.1333)


def _time(fn, reps):
    for _ in range(5):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return 1e3 * e0.elapsed_time(e1) / reps


def _graphed(fn):
    """fn recorded into a hipGraph (after a warm-up on a side stream); returns the replay callable"""
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        fn()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        keep = fn()
    graph.keep = keep
    return graph.replay


def torch_ms_ssim(x, y, win, wts):
    """x, y [1,3,H,W] float32 on the device, win [3,1,1,11], wts [5,1,1]: the composition pytorch_msssim runs"""
    C1, C2 = 0.01 ** 2, 0.03 ** 2
    wt = win.transpose(2, 3)

    def filt(t):
        return F.conv2d(F.conv2d(t, win, groups=3), wt, groups=3)

    mcs = []
    for l in range(5):
        mu1, mu2 = filt(x), filt(y)
        s1, s2, s12 = filt(x * x) - mu1 * mu1, filt(y * y) - mu2 * mu2, filt(x * y) - mu1 * mu2
        cs_map = (2 * s12 + C2) / (s1 + s2 + C2)
        ssim_map = ((2 * mu1 * mu2 + C1) / (mu1 * mu1 + mu2 * mu2 + C1)) * cs_map
        if l < 4:
            mcs.append(torch.relu(cs_map.flatten(2).mean(-1)))
            pad = [s % 2 for s in x.shape[2:]]
            x, y = F.avg_pool2d(x, 2, padding=pad), F.avg_pool2d(y, 2, padding=pad)
    vals = torch.stack(mcs + [torch.relu(ssim_map.flatten(2).mean(-1))], dim=0)
    return torch.prod(vals ** wts, dim=0).mean()


def torch_frame_metrics(color, depth, gt, mask, gt_depth, win, wts):
    """eval_render.py:59-89 as torch launches it (mse_loss, indexing, two ms_ssim)"""
    chw = lambda t: t.permute(2, 0, 1)[None]
    out = [-10.0 * torch.log10(F.mse_loss(gt, color)), torch_ms_ssim(chw(gt), chw(color), win, wts)]
    depth, gt, color = depth.clone(), gt.clone(), color.clone()
    depth[~mask] = 0.0
    gt[~mask] = 0.0
    color[~mask] = 0.0
    out += [-10.0 * torch.log10(F.mse_loss(gt[mask], color[mask])), torch_ms_ssim(chw(gt), chw(color), win, wts),
            (depth - gt_depth).abs()[mask].mean()]
    return out


def time_kernels(dev, reps):
    from glorie_slam_amd.image_metrics import frame_metrics, ms_ssim
    from glorie_slam_amd.pipeline import synthetic_images
    g = torch.exp(-((torch.arange(11, dtype=torch.float32) - 5) ** 2) / (2 * 1.5 ** 2))
    win = (g / g.sum()).view(1, 1, 1, 11).repeat(3, 1, 1, 1).to(dev)
    wts = torch.tensor(WEIGHTS, device=dev).view(-1, 1, 1)
    for H, W in ((480, 640), (680, 1200)):
        gt = synthetic_images(1, H, W)[0].permute(1, 2, 0).contiguous().to(dev)
        color = (gt + 0.05 * torch.randn_like(gt)).clamp(0, 1)
        depth = 1.0 + torch.rand(H, W, device=dev)
        gt_depth = depth + 0.05 * torch.randn_like(depth)
        mask = torch.rand(H, W, device=dev) > 0.3
        x, y = gt.permute(2, 0, 1)[None].contiguous(), color.permute(2, 0, 1)[None].contiguous()
        ours, theirs = float(ms_ssim(gt, color)), float(torch_ms_ssim(x, y, win, wts))
        rows = {
            "ms_ssim": (lambda: ms_ssim(gt, color), lambda: torch_ms_ssim(x, y, win, wts)),
            "frame_metrics": (lambda: frame_metrics(color, depth, gt, mask, gt_depth=gt_depth),
                              lambda: torch_frame_metrics(color, depth, gt, mask, gt_depth, win, wts)),
        }
        print(f"{W}x{H}: ms_ssim {ours:.7f}, torch composition {theirs:.7f}")
        for name, (fn, ref) in rows.items():
            eager, ref_eager = _time(fn, reps), _time(ref, reps)
            replay = _time(_graphed(fn), reps)
            # the masked half of the torch form indexes with a boolean mask (a host read): it cannot be recorded
            ref_replay = _time(_graphed(ref), reps) if name == "ms_ssim" else float("nan")
            print(f"  {name}: kernels {eager:.1f} us eager, {replay:.1f} us replayed; torch composition {ref_eager:.1f} us "
                  f"eager, {ref_replay:.1f} us replayed")


def time_eval(dev, reps, K=6):
    import glorie_slam_amd.pipeline as P
    from glorie_slam_amd.eval_render import _constant_radius, _score
    from glorie_slam_amd.image_metrics import frame_metrics
    run, c = P.synthetic_runner(dev, K, zero_flow_head=True, map_iters=10, map_rays=1000)
    video, imgs = c["video"], P.synthetic_images(K)
    for k in range(K):
        run.init_state(k)
        video.timestamp[k] = k
        run.images[k] = imgs[k].to(dev)
    video.counter.value = K
    for k in range(K):
        run.map_keyframe(k)
        run.mapped += 1
    k = K - 1
    depth, c2w = run._keyframe_view(k)
    rq = _constant_radius(run, depth)
    gt = run.images[k].permute(1, 2, 0).contiguous()
    with torch.no_grad():
        m, color, r_depth, mask = _score(run, c2w, depth, rq, gt, None)
        npc = run.npc
        render = _time(lambda: run.renderer.render_img(npc, run.decoders, c2w, run.device, stage="color", gt_depth=depth,
                                                       npc_geo_feats=npc.get_geo_feats(), npc_col_feats=npc.get_col_feats(),
                                                       dynamic_r_query=rq, cloud_pos=npc.cloud_pos()), max(reps // 10, 5))
        metrics = _time(lambda: frame_metrics(color, r_depth, gt, mask), reps)
    print(f"eval_kf_imgs, one 640x480 keyframe ({int(run.npc.pts_num())} points): render_img {render:.1f} us, frame_metrics "
          f"{metrics:.1f} us; psnr {float(m['psnr']):.2f} ms_ssim {float(m['ms_ssim']):.4f}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=100)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    time_kernels(dev, a.reps)
    time_eval(dev, a.reps)


if __name__ == "__main__":
    main()
