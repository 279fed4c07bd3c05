"""The pixel-warping loss on the HIP kernels (glorie_slam_amd/warp_loss.py, csrc/warp.hip) and the multi-keyframe mapping
window of SequenceRunner that uses it (reference: src/mapper.py:326-388 and :437-509, src/utils/common.py:324-350).

  * against the reference's own values (tests/golden/pix_warp.npz, tests/golden/make_pix_warp.py);
  * against the float64 restatement (tests/pix_warp_ref.py) at the product shape: 640x480, a window of 5, 5000 rays,
    in all three image layouts;
  * repeated calls bitwise equal; finite differences of the restatement against the kernel's gradient;
  * SequenceRunner with pix_warping on: the term is active from the 5th keyframe on, the first iteration's loss is the
    restatement's, the iteration records into a hipGraph and its replays follow an eager run."""
import numpy as np
import pytest
import torch

from pix_warp_ref import pix_warp_loss as ref_loss, project as ref_project
from test_pix_warp_oracle import load_case

pytestmark = pytest.mark.gpu


def _hip(c, dev, depth=None, nan_to_zero=False, layout="hwc"):
    from glorie_slam_amd.warp_loss import FrameTable, pix_warping_loss
    t = lambda x: (x if torch.is_tensor(x) else torch.from_numpy(np.ascontiguousarray(x))).to(dev)
    dep = (t(c["depth"]) if depth is None else t(depth)).float().detach().clone().requires_grad_(True)
    imgs = t(c["images"]).float()
    if layout == "table":
        imgs = FrameTable([im.permute(2, 0, 1).contiguous() for im in imgs], channels_first=True)
    elif layout == "chw":
        imgs = imgs.permute(0, 3, 1, 2).contiguous()
    loss = pix_warping_loss(t(c["rays_o"]), t(c["rays_d"]), dep, t(c["c2ws"]), c["fx"], c["fy"], c["cx"], c["cy"],
                            c["W"], c["H"], t(c["frame_indices"]), t(c["indices"]), imgs, t(c["gt"]),
                            nan_to_zero=nan_to_zero, channels_first=layout == "chw")
    loss.backward()
    torch.cuda.synchronize()
    return loss.detach().cpu(), dep.grad.cpu()


def _ref(c, dev, depth=None):
    t = lambda x: (x if torch.is_tensor(x) else torch.from_numpy(np.ascontiguousarray(x))).to(dev)
    dep = (t(c["depth"]) if depth is None else t(depth)).double().detach().clone().requires_grad_(True)
    loss, mask = ref_loss(t(c["rays_o"]), t(c["rays_d"]), dep, t(c["c2ws"]), c["fx"], c["fy"], c["cx"], c["cy"], c["W"],
                          c["H"], t(c["frame_indices"]), t(c["indices"]), t(c["images"]), t(c["gt"]))
    loss.backward()
    return loss.detach().cpu(), dep.grad.cpu(), mask.cpu()


def _close(loss, grad, ref_l, ref_g):
    assert abs(float(loss) - float(ref_l)) <= 1e-5 * abs(float(ref_l)), (float(loss), float(ref_l))
    g = np.asarray(ref_g, dtype=np.float64)
    err = np.abs(grad.double().numpy() - g).max()
    assert err <= 1e-4 * np.abs(g).max(), (err, np.abs(g).max())


@pytest.mark.parametrize("name", ["a", "b"])
def test_hip_matches_the_reference(gpu, name):
    c = load_case(name)
    for layout in ("hwc", "chw", "table"):
        loss, grad = _hip(c, gpu, layout=layout)
        _close(loss, grad, c["loss"], c["grad"])


def test_hip_single_frame_is_nan_with_zero_gradient(gpu):
    c = load_case("c")
    loss, grad = _hip(c, gpu)
    assert torch.isnan(loss) and (grad == 0).all()
    loss0, grad0 = _hip(c, gpu, nan_to_zero=True)
    assert float(loss0) == 0.0 and (grad0 == 0).all()


def product_case(seed=0, N=5000, M=5, H=480, W=640):
    """a 5-frame window of 640x480 cameras on a short arc, 5000 rays drawn from every frame; rays with a sample within
    1e-2 px of a mask threshold or a texel boundary are redrawn (fp32 cannot flip a decision or a bilinear cell)"""
    g = torch.Generator().manual_seed(seed)
    fx = fy = 320.0
    cx, cy = 319.5, 239.5
    c2ws = torch.zeros(M, 4, 4, dtype=torch.float64)
    for m in range(M):
        a = 0.03 * (m - 2)
        c2ws[m, :3, :3] = torch.tensor([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]])
        c2ws[m, :3, 3] = torch.tensor([0.12 * (m - 2), 0.03 * (m % 2), 0.04 * m])
        c2ws[m, 3, 3] = 1
    c2ws = c2ws.float().double()
    low = torch.rand(M, 3, H // 16, W // 16, generator=g, dtype=torch.float64)
    images = torch.nn.functional.interpolate(low, size=(H, W), mode="bilinear", align_corners=False)
    images = images.permute(0, 2, 3, 1).float().contiguous()
    o, d, dep, own = [], [], [], []
    per = N // M
    for m in range(M):
        got = 0
        while got < per:
            n = 2 * per
            i, j = torch.rand(n, generator=g, dtype=torch.float64) * W, torch.rand(n, generator=g, dtype=torch.float64) * H
            dc = torch.stack([(i - cx) / fx, -(j - cy) / fy, -torch.ones_like(i)], -1)
            dw = (dc @ c2ws[m, :3, :3].T).float().double()
            z = (2.0 + 2.0 * torch.rand(n, generator=g, dtype=torch.float64)).float().double()
            ow = c2ws[m, :3, 3].expand(n, 3).float().double()
            X = (ow + dw * z[:, None]).float().double()
            u, v, zc = ref_project(c2ws, X, fx, fy, cx, cy)
            near = lambda x, t: (x - t).abs() < 1e-2
            bad = near(u, 5) | near(u, W - 5) | near(v, 5) | near(v, H - 5) | (zc.abs() < 1e-2)
            for q in (u - 0.5, v - 0.5):
                f = q - torch.floor(q)
                bad |= (f < 1e-2) | (f > 1 - 1e-2)
            ok = ~bad.any(1)
            k = min(int(ok.sum()), per - got)
            o.append(ow[ok][:k]), d.append(dw[ok][:k]), dep.append(z[ok][:k]), own.append(torch.full((k,), m))
            got += k
    own = torch.cat(own)
    frame_indices = torch.tensor([3, 4, 6, 7, 8])
    gt = images[own, 240, 320] + 0.1 * torch.randn(N, 3, generator=g)
    return dict(rays_o=torch.cat(o).float(), rays_d=torch.cat(d).float(), depth=torch.cat(dep).float(),
                c2ws=c2ws.float(), frame_indices=frame_indices, indices=frame_indices[own], images=images, gt=gt.float(),
                fx=fx, fy=fy, cx=cx, cy=cy, H=H, W=W)


def test_hip_matches_the_restatement_at_the_product_shape(gpu):
    c = product_case()
    ref_l, ref_g, mask = _ref(c, gpu)
    n = mask.sum(1)
    assert (n >= 4).sum() > 1000 and (n == 0).sum() > 100, n.bincount()     # both kinds of rays are there
    out = [_hip(c, gpu, layout=lay) for lay in ("hwc", "chw", "table")]
    _close(*out[0], ref_l, ref_g)
    for loss, grad in out[1:]:                                                 # the layouts read the same texels
        assert torch.equal(loss, out[0][0]) and torch.equal(grad, out[0][1])


def test_repeated_calls_are_bitwise_equal(gpu):
    c = product_case(seed=1)
    first = _hip(c, gpu, layout="table")
    for _ in range(3):
        again = _hip(c, gpu, layout="table")
        assert torch.equal(again[0], first[0]) and torch.equal(again[1], first[1])


def test_gradient_against_finite_differences(gpu):
    """central differences of the float64 restatement in depth, one ray at a time, against the kernel's gradient"""
    c = product_case(seed=2, N=500)
    _, grad = _hip(c, gpu)
    ref_l, _, mask = _ref(c, gpu)
    rays = torch.nonzero(mask.sum(1) >= 4).flatten()[:6].tolist() + torch.nonzero(mask.sum(1) == 0).flatten()[:2].tolist()
    assert len(rays) == 8
    dep = torch.from_numpy(np.asarray(c["depth"])) if not torch.is_tensor(c["depth"]) else c["depth"]
    h = 1e-6
    for r in rays:
        lp, lm = dep.double().clone(), dep.double().clone()
        lp[r] += h
        lm[r] -= h
        fd = (float(_ref(c, gpu, lp)[0]) - float(_ref(c, gpu, lm)[0])) / (2 * h)
        assert abs(float(grad[r]) - fd) <= 1e-3 * max(abs(fd), 1e-3 * float(grad.abs().max())), (r, float(grad[r]), fd)


def test_non_finite_depth_gets_zero_gradient(gpu):
    c = product_case(seed=3, N=1000)
    dep = c["depth"].clone()
    dep[:5] = float("nan")
    dep[5:8] = float("inf")
    loss, grad = _hip(c, gpu, depth=dep)
    ref_l, ref_g, _ = _ref(c, gpu, dep)
    assert torch.isfinite(grad).all() and (grad[:8] == 0).all()
    _close(loss, grad, ref_l, ref_g)


# ---- SequenceRunner with the pixel-warping window ------------------------------------------------------------------
K_RUN, ITERS, RAYS = 6, 6, 1000


def _window_run(gpu, graphs, probe=None):
    """K_RUN keyframes mapped with a 5-frame window (the setup of test_gpu_sequence's recorded-iteration test: generating
    poses and depth maps written into the video, no tracking); probe(run, k, tensors) sees every eager iteration"""
    from glorie_slam_amd.pipeline import synthetic_images, synthetic_runner
    run, c = synthetic_runner(gpu, K_RUN, zero_flow_head=True, map_iters=ITERS, map_rays=RAYS)
    run.pix_warping, run.mapping_window_size, run.w_pix_warp_loss = True, 5, 1000.0
    run.map_graph = graphs
    if probe is not None:
        run.map_probe = lambda k, t: probe(run, k, t)
    video, imgs = c["video"], synthetic_images(K_RUN)
    video.poses[:K_RUN] = c["poses"][:K_RUN]
    video.disps[:K_RUN] = c["disps"][:K_RUN]
    video.disps_up[:K_RUN] = torch.nn.functional.interpolate(c["disps"][:K_RUN, None], scale_factor=8, mode="bilinear",
                                                             align_corners=False)[:, 0]
    video.counter.value = K_RUN
    losses = []
    for k in range(K_RUN):
        run.images[k] = imgs[k].to(gpu)
        losses.append(run.map_keyframe(k))
    torch.cuda.synchronize()
    return run, losses


def test_runner_window_records_and_follows_the_restatement(gpu):
    probes = {}

    def probe(run, k, t):
        """the first (eager) iteration of keyframe k recomputed from its rendered depth: L1 sums + restatement"""
        if k in probes:
            return
        w, ren = t["warp"], run.renderer
        imgs = torch.stack([run.images[f] for f in w["window"]]).permute(0, 2, 3, 1)
        wr, _ = ref_loss(t["ro"], t["rd"], t["depth"], w["c2ws"], ren.fx, ren.fy, ren.cx, ren.cy, run.video.wd,
                         run.video.ht, w["frame_ids"], w["ray_frame"], imgs, t["gt_col"])
        wr = 0.0 if torch.isnan(wr) else float(wr)
        seen = t["seen"].double()
        l1 = (torch.abs(t["d"] - t["depth"]).double() * seen).sum() + \
            0.5 * (torch.abs(t["gt_col"] - t["colour"]).double() * seen[:, None]).sum()
        probes[k] = (float(t["loss"]), float((l1 + 1000.0 * wr) / seen.sum().clamp_min(1)), float(w["value"]), wr,
                     len(w["window"]), int(t["ro"].shape[0]))

    eager, le = _window_run(gpu, False, probe)
    eager2, l2 = _window_run(gpu, False)
    graph, lg = _window_run(gpu, True)

    for k in range(K_RUN):
        got, want, warp_got, warp_want, n_win, n_rays = probes[k]
        assert n_win == min(k + 1, 5) and n_rays == (RAYS // n_win) * n_win
        assert abs(got - want) <= 2e-3 * abs(want), (k, got, want)
        assert abs(warp_got - warp_want) <= 2e-3 * max(abs(warp_want), 1e-6), (k, warp_got, warp_want)
    for run in (eager, graph):
        w = np.array(run.warp_losses)
        assert (w[:4] == 0).all(), w                       # fewer than 4 other frames in the window
        assert (w[4:] > 0).all() and np.isfinite(w).all(), w
    assert graph.map_graph_stats["captures"] >= 1 and eager.map_graph_stats["captures"] == 0
    le, l2, lg = np.array(le), np.array(l2), np.array(lg)
    noise = np.abs(l2 - le).max()
    print("loss noise eager2-eager", noise, " graph-eager", np.abs(lg - le).max(), " scale", np.abs(le).max())
    print("warp terms (first, last) per keyframe:", graph.warp_losses)
    assert np.abs(lg - le).max() <= max(4.0 * noise, 3e-2 * np.abs(le).max()), (lg, le, noise)
    wg, we = np.array(graph.warp_losses), np.array(eager.warp_losses)
    assert np.abs(wg - we).max() <= 3e-2 * np.abs(we).max(), (wg, we)


def test_runner_flag_off_leaves_the_loss_alone(gpu):
    """pix_warping off (the default) - no window, no warp term, no probe of it"""
    from glorie_slam_amd.pipeline import synthetic_runner
    run, _ = synthetic_runner(gpu, 2, map_iters=2, map_rays=100)
    assert run.pix_warping is False and run.mapping_window_size == 1 and run.warp_losses == []
    cfg = {**run.cfg, "mapping": {"pix_warping": True, "w_pix_warp_loss": 1000.0, "mapping_window_size": 5}}
    from glorie_slam_amd.pipeline import SequenceRunner
    r2 = SequenceRunner(run.net, run.video, cfg, run.npc, run.decoders, run.renderer, lambda *a: None)
    assert r2.pix_warping and r2.mapping_window_size == 5 and r2.w_pix_warp_loss == 1000.0
