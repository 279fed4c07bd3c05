"""The frame-ingest kernels (csrc/ingest.hip through glorie_slam_amd.ingest.IngestPlan) against the numpy restatement
tests/ingest_ref.py, bit for bit (torch.equal).  Shapes are the smallest at which the kernel can still go wrong: an odd
width (3-byte pixels never aligned), outputs that are no multiple of the 64 x 4 tile and span several workgroups, a
distortion that sends border taps outside the image, up- and down-scaling, one edge without the other."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import ingest_ref as R

pytestmark = pytest.mark.gpu

TUM_FR1 = [0.2624, -0.9531, -0.0054, 0.0026, 1.1633]
EIGHT = TUM_FR1 + [0.05, -0.02, 0.01]

# name -> (B, cam)
CASES = {
    "distorted_37x53_edges": (3, R.cam_block(37, 53, 24, 40, H_edge=2, W_edge=3, distortion=TUM_FR1)),
    "plain_37x53_edges": (3, R.cam_block(37, 53, 24, 40, H_edge=2, W_edge=3)),
    "upscale_20x28": (2, R.cam_block(20, 28, 33, 47)),
    "equal_24x40": (2, R.cam_block(24, 40, 24, 40)),
    "halving_48x64": (2, R.cam_block(48, 64, 24, 32)),
    "w_edge_only": (2, R.cam_block(37, 53, 28, 40, H_edge=0, W_edge=3, distortion=TUM_FR1)),
    "h_edge_only": (2, R.cam_block(37, 53, 24, 46, H_edge=2, W_edge=0)),
    "batch_5": (5, R.cam_block(37, 53, 24, 40, H_edge=2, W_edge=3, distortion=TUM_FR1)),
    "eight_coefficients": (2, R.cam_block(37, 53, 24, 40, H_edge=2, W_edge=3, distortion=EIGHT)),
    "four_coefficients": (1, R.cam_block(37, 53, 24, 40, H_edge=2, W_edge=3, distortion=TUM_FR1[:4])),
    "wide_output_130x70": (1, R.cam_block(37, 53, 70, 130, H_edge=1, W_edge=1, distortion=TUM_FR1)),   # 3 x 18 workgroups
}


def _frames(B, cam, seed=0):
    return np.random.default_rng(seed).integers(0, 256, (B, cam["H"], cam["W"], 3), dtype=np.uint8)


def _plan(cam, gpu):
    from glorie_slam_amd.ingest import IngestPlan
    return IngestPlan(cam, gpu)


@pytest.mark.parametrize("swap_rb", [False, True])
@pytest.mark.parametrize("name", sorted(CASES))
def test_color_equals_the_restatement(name, swap_rb, gpu):
    B, cam = CASES[name]
    frames = _frames(B, cam)
    got = _plan(cam, gpu).color(torch.from_numpy(frames).to(gpu), swap_rb=swap_rb)
    want = torch.from_numpy(R.color(frames, cam, swap_rb=swap_rb))
    assert got.dtype == torch.float32 and got.shape == (B, 3, cam["H_out"], cam["W_out"]) and got.is_contiguous()
    assert torch.equal(got.cpu(), want)
    if name == "equal_24x40" and not swap_rb:
        assert torch.equal(got.cpu(), torch.from_numpy(frames).permute(0, 3, 1, 2).float() / 255.0)
    if name == "halving_48x64" and not swap_rb:
        f = frames.astype(np.int64)
        mean = (f[:, 0::2, 0::2] + f[:, 0::2, 1::2] + f[:, 1::2, 0::2] + f[:, 1::2, 1::2] + 2) >> 2
        assert torch.equal(got.cpu(), torch.from_numpy(mean.astype(np.float32) / np.float32(255)).permute(0, 3, 1, 2))


def test_single_frame_is_a_batch_of_one(gpu):
    B, cam = CASES["distorted_37x53_edges"]
    frames = _frames(1, cam, seed=1)
    plan = _plan(cam, gpu)
    got = plan.color(torch.from_numpy(frames[0]).to(gpu))
    assert got.shape == (1, 3, 24, 40) and torch.equal(got.cpu(), torch.from_numpy(R.color(frames[0], cam)))
    raw = np.random.default_rng(2).integers(0, 65536, (37, 53)).astype(np.uint16)
    d = plan.depth(torch.from_numpy(raw).to(gpu))
    assert d.shape == (1, 24, 40) and torch.equal(d.cpu(), torch.from_numpy(R.depth(raw, cam)))


def test_constant_255_checks_the_zero_border(gpu):
    """every tap inside -> exactly 1.0; a border pixel whose taps leave the image mixes in zeros -> below 1.0 (a clamp to
    the border would give 1.0 everywhere).  No edges here, so the output keeps the border pixels"""
    cam = R.cam_block(37, 53, 37, 53, distortion=TUM_FR1)
    frames = np.full((1, 37, 53, 3), 255, np.uint8)
    got = _plan(cam, gpu).color(torch.from_numpy(frames).to(gpu)).cpu()
    assert torch.equal(got, torch.from_numpy(R.color(frames, cam)))
    assert bool((got[:, :, 8:-8, 8:-8] == 1.0).all())
    border = torch.cat([got[:, :, 0].flatten(), got[:, :, -1].flatten(), got[:, :, :, 0].flatten(), got[:, :, :, -1].flatten()])
    assert float(border.min()) < 1.0 and float(got.max()) == 1.0
    # the same through the distorted case of the list above (edges 2 / 3 crop part of the border away)
    B, cam = CASES["distorted_37x53_edges"]
    got = _plan(cam, gpu).color(torch.from_numpy(frames).to(gpu)).cpu()
    assert torch.equal(got, torch.from_numpy(R.color(frames, cam)))
    assert bool((got[:, :, 6:-6, 6:-6] == 1.0).all())


@pytest.mark.parametrize("dtype", [np.uint16, np.float32])
@pytest.mark.parametrize("name", ["distorted_37x53_edges", "upscale_20x28", "equal_24x40", "halving_48x64", "w_edge_only",
                                  "h_edge_only", "batch_5", "wide_output_130x70"])
def test_depth_equals_the_restatement_and_torch_nearest(name, dtype, gpu):
    B, cam = CASES[name]
    cam = dict(cam, png_depth_scale=5000.0 if dtype == np.uint16 else 6553.5)
    rng = np.random.default_rng(3)
    raw = rng.integers(0, 65536, (B, cam["H"], cam["W"])).astype(dtype)
    if dtype == np.float32:
        raw += rng.uniform(0, 1, raw.shape).astype(np.float32)
    got = _plan(cam, gpu).depth(torch.from_numpy(raw).to(gpu)).cpu()
    assert got.shape == (B, cam["H_out"], cam["W_out"]) and torch.equal(got, torch.from_numpy(R.depth(raw, cam)))
    he, we = cam["H_edge"], cam["W_edge"]
    H_res, W_res = cam["H_out"] + 2 * he, cam["W_out"] + 2 * we
    full = torch.from_numpy(raw.astype(np.float32) / np.float32(cam["png_depth_scale"]))
    ref = F.interpolate(full[:, None], (H_res, W_res), mode="nearest")[:, 0][:, he:H_res - he, we:W_res - we]
    assert torch.equal(got, ref)


def test_depth_division_is_correctly_rounded_for_every_uint16(gpu):
    cam = R.cam_block(256, 256, 256, 256, png_depth_scale=6553.5)
    v = np.arange(65536, dtype=np.uint16).reshape(1, 256, 256)
    got = _plan(cam, gpu).depth(torch.from_numpy(v).to(gpu)).cpu().numpy()
    exact = np.arange(65536, dtype=np.float64) / np.float64(np.float32(6553.5))
    assert np.array_equal(got.reshape(-1), exact.astype(np.float32))


def test_capture_and_replay_in_a_graph(gpu):
    B, cam = CASES["distorted_37x53_edges"]
    cam = dict(cam, png_depth_scale=5000.0)
    plan = _plan(cam, gpu)
    rng = np.random.default_rng(4)
    frames = torch.from_numpy(_frames(B, cam, seed=5)).to(gpu)
    raw = torch.from_numpy(rng.integers(0, 65536, (B, 37, 53)).astype(np.uint16)).to(gpu)
    eager_c, eager_d = plan.color(frames), plan.depth(raw)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        plan.color(frames), plan.depth(raw)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out_c, out_d = plan.color(frames), plan.depth(raw)
    out_c.zero_(), out_d.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out_c, eager_c) and torch.equal(out_d, eager_d)
    # new contents in the same buffers: the replay reads them
    frames.copy_(torch.from_numpy(_frames(B, cam, seed=6)).to(gpu))
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out_c.cpu(), torch.from_numpy(R.color(frames.cpu().numpy(), cam)))


def test_error_cases(gpu):
    from glorie_slam_amd import _lib
    from glorie_slam_amd.ingest import IngestPlan
    B, cam = CASES["plain_37x53_edges"]
    plan = _plan(cam, gpu)
    frames = torch.from_numpy(_frames(2, cam)).to(gpu)
    with pytest.raises(_lib.GlorieError):
        plan.color(frames.cpu())
    with pytest.raises(_lib.GlorieError):
        plan.depth(torch.zeros(37, 53))
    with pytest.raises(ValueError):
        plan.color(frames.float())
    with pytest.raises(ValueError):
        plan.depth(torch.zeros(37, 53, dtype=torch.float64, device=gpu))
    with pytest.raises(ValueError):
        plan.color(frames.permute(0, 2, 1, 3))                             # right dtype, wrong shape
    wide = torch.zeros(2, 37, 106, 3, dtype=torch.uint8, device=gpu)
    with pytest.raises(ValueError):
        plan.color(wide[:, :, ::2])                                        # right shape, not contiguous
    with pytest.raises(ValueError):
        plan.depth(torch.zeros(37, 106, device=gpu)[:, ::2])
    with pytest.raises(ValueError):
        IngestPlan(dict(cam, distortion=[0.0] * 14), gpu)
