"""The contact-sheet kernels (glorie_slam_amd/csrc/vis.hip through glorie_slam_amd/visualizer.py) against the float32
restatement of tests/vis_ref.py, bit for bit: ranges, sheets at ragged sizes and scales, to_rgb8, replay from a captured
graph, and the bytes around a caller's `out`.  Every comparison is exact."""
import numpy as np
import pytest
import torch

import vis_ref as R

pytestmark = pytest.mark.gpu

F = np.float32
N_SURFACE = 10


def scene(H, W, seed=0, dmax=4.0, droid_zero=False):
    """maps that meet every rule of the sheet: holes in render_depth, a mono prior above dmax, depths on exact multiples of
    dmax / 256 (dmax a power of two), NaN and inf in depth, colours outside [0, 1] and half an ulp above k / 255"""
    rng = np.random.default_rng(seed)
    grid = lambda: (rng.integers(0, 257, (H, W)).astype(F) * F(dmax / 256))       # 256 t lands on the integers
    rd = (rng.random((H, W)) * dmax).astype(F)
    rd[rng.random((H, W)) < 0.15] = 0                                             # holes
    on = rng.random((H, W)) < 0.2
    rd[on] = grid()[on]
    depth = (rd + (rng.random((H, W)).astype(F) - F(0.5)) * F(0.5)).astype(F)
    depth[rng.random((H, W)) < 0.05] = np.nan
    depth[rng.random((H, W)) < 0.02] = np.inf
    droid = grid()
    if H * W > 2:
        droid.flat[0] = dmax                                                      # the range's end is met
        droid.flat[-1] = np.nan                                                   # and what is no number is skipped
    if droid_zero:
        droid[:] = 0
    k = rng.integers(0, 256, (H, W, 3)).astype(F)
    color = np.where(rng.random((H, W, 3)) < 0.5, np.nextafter(k / F(255), F(2)),
                     (rng.random((H, W, 3)) * 1.6 - 0.3).astype(F)).astype(F)
    tie = rng.random((H, W, 3)) < 0.05
    color[tie] = ((k + F(0.5)) / F(255))[tie]
    gt = (rng.random((H, W, 3)) * 1.6 - 0.3).astype(F)
    proj = np.where(rng.random((H, W)) < 0.6, grid(), F(0)).astype(F)
    sparse = np.where(rng.random((H, W)) < 0.2, (rng.random((H, W)) * dmax).astype(F), F(0)).astype(F)
    counts = rng.integers(0, N_SURFACE + 1, (H, W)).astype(F)
    mono = (rng.random((H, W)) * dmax * 1.5 + 0.1).astype(F)                      # above dmax
    return dict(render_depth=rd, depth=depth, color=color, gt_color=gt, droid_depth=droid, proj_depth=proj,
                valid_ray_count=counts, sparse_proj_depth=sparse, mono_depth=mono)


def on_device(maps, gpu):
    return {k: torch.from_numpy(v).to(gpu) for k, v in maps.items()}


def differing(sheet, ref):
    got = sheet.cpu().numpy()
    assert got.shape == ref.shape and got.dtype == np.uint8
    bad = np.argwhere(got != ref)
    return len(bad), (bad[:5].tolist(), got[tuple(bad[:5].T)].tolist(), ref[tuple(bad[:5].T)].tolist()) if len(bad) else None


# 37 x 53 at every scale; one pixel; a row longer than a workgroup's span with fewer rows than panels; a sheet whose
# pitch is a multiple of four pixels (the dword-store path) at a small size
CASES = [(37, 53, 1), (37, 53, 2), (37, 53, 3), (37, 53, 5), (1, 1, 1), (2, 130, 1), (2, 1300, 1), (6, 52, 1), (37, 56, 2)]


@pytest.mark.parametrize("H,W,scale", CASES)
def test_sheet_is_the_restatement(gpu, H, W, scale):
    from glorie_slam_amd.visualizer import PLASMA, contact_sheet, sheet_ranges
    for seed, droid_zero in ((1, False), (2, True)):
        maps = scene(H, W, seed, droid_zero=droid_zero)
        dev = on_device(maps, gpu)
        ranges = torch.full((4,), -1.0, device=gpu)
        sheet = contact_sheet(dev, N_SURFACE, scale=scale, ranges=ranges)
        want = R.ranges(maps)
        assert np.array_equal(ranges.cpu().numpy().view(np.uint32), want.view(np.uint32)), (ranges.tolist(), want.tolist())
        assert torch.equal(sheet_ranges(dev), ranges)
        n, first = differing(sheet, R.contact_sheet(maps, N_SURFACE, PLASMA, scale=scale))
        assert n == 0, first
        if droid_zero:
            assert want[0] == 0                                                   # the degenerate range [0, 0]
    # another gutter and title, none at all
    for gutter, title in ((1, 7), (0, 0)):
        sheet = contact_sheet(dev, N_SURFACE, scale=scale, gutter=gutter, title=title)
        n, first = differing(sheet, R.contact_sheet(maps, N_SURFACE, PLASMA, scale=scale, gutter=gutter, title=title))
        assert n == 0, first


def test_sheet_at_640x480(gpu):
    from glorie_slam_amd.visualizer import PLASMA, contact_sheet, panel_boxes
    maps = scene(480, 640, 3)
    sheet = contact_sheet(on_device(maps, gpu), N_SURFACE, scale=2)
    assert tuple(sheet.shape) == (1028, 976, 3)
    n, first = differing(sheet, R.contact_sheet(maps, N_SURFACE, PLASMA, scale=2))
    assert n == 0, first
    assert panel_boxes(480, 640, 2, 4, 12) == R.panel_boxes(480, 640, 2, 4, 12)


def test_ranges(gpu):
    from glorie_slam_amd.visualizer import sheet_ranges
    rng = np.random.default_rng(7)
    cases = []
    for n in (1, 3, 4, 5, 1023, 1025, 37 * 53, 300001):                          # below, at and past a lane's four values
        m = dict(render_depth=(rng.random(n) * 3).astype(F), depth=(rng.random(n) * 3).astype(F),
                 droid_depth=(rng.standard_normal(n) * 3).astype(F))
        m["render_depth"][rng.random(n) < 0.1] = 0
        m["depth"][rng.random(n) < 0.1] = np.nan
        m["droid_depth"][rng.random(n) < 0.1] = np.inf
        cases.append(m)
    cases.append(dict(render_depth=np.full(9, np.nan, F), depth=np.ones(9, F), droid_depth=np.full(9, -np.inf, F)))
    cases.append(dict(render_depth=np.zeros(9, F), depth=np.full(9, np.nan, F), droid_depth=-np.zeros(9, F)))
    cases.append(dict(render_depth=np.ones(9, F), depth=np.full(9, 1.1, F), droid_depth=np.full(9, -2.5, F)))   # dmax < 0
    for m in cases:
        got = sheet_ranges(on_device(m, gpu)).cpu().numpy()
        want = R.ranges(m)
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (got.tolist(), want.tolist())
    # a view that does not start on 16 bytes takes the scalar loads
    m = cases[5]
    dev = {k: torch.from_numpy(np.concatenate([np.zeros(1, F), v])).to(gpu)[1:] for k, v in m.items()}
    assert np.array_equal(sheet_ranges(dev).cpu().numpy().view(np.uint32), R.ranges(m).view(np.uint32))


def test_to_rgb8(gpu):
    from glorie_slam_amd.visualizer import to_rgb8
    k = np.arange(255, dtype=F)
    rng = np.random.default_rng(5)
    x = np.concatenate([((k + F(0.5)) / F(255)).astype(F), np.array([-1.0, -0.0, 0.0, 1.0, 1.5, 300.0, np.nan, np.inf, -np.inf], F),
                        (rng.random(2000) * 1.4 - 0.2).astype(F), np.nextafter(k / F(255), F(2)), k / F(255)])
    for n in (len(x), 7, 2, 1):                                                   # with and without a tail of fewer than four
        got = to_rgb8(torch.from_numpy(x[:n]).to(gpu))
        assert got.dtype == torch.uint8 and np.array_equal(got.cpu().numpy(), R.to_rgb8(x[:n]))
    ties = (x[:255] * F(255)) == k + F(0.5)                                       # where 255 x is an exact tie: the even level
    assert ties.any() and np.array_equal(R.to_rgb8(x[:255])[ties], (k + k % 2).astype(np.uint8)[ties])
    img = (rng.random((5, 7, 3)) * 1.4 - 0.2).astype(F)
    got = to_rgb8(torch.from_numpy(img).to(gpu))
    assert tuple(got.shape) == (5, 7, 3) and np.array_equal(got.cpu().numpy(), R.to_rgb8(img))
    off = torch.from_numpy(np.concatenate([np.zeros(1, F), x])).to(gpu)[1:]       # not on 16 bytes
    assert np.array_equal(to_rgb8(off).cpu().numpy(), R.to_rgb8(x))


def test_replay_from_a_captured_graph(gpu):
    from glorie_slam_amd.visualizer import PLASMA, contact_sheet, sheet_size
    H, W, scale = 37, 53, 2
    first, second = scene(H, W, 11), scene(H, W, 12, dmax=8.0)
    bufs = on_device(first, gpu)
    out = torch.zeros(*sheet_size(H, W, scale), 3, dtype=torch.uint8, device=gpu)
    ranges = torch.zeros(4, device=gpu)
    contact_sheet(bufs, N_SURFACE, scale=scale, out=out, ranges=ranges)           # eager: the table is on the device
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream(gpu)
    side.wait_stream(torch.cuda.current_stream(gpu))
    with torch.cuda.stream(side):
        graph.capture_begin()
        try:
            contact_sheet(bufs, N_SURFACE, scale=scale, out=out, ranges=ranges)
        finally:
            graph.capture_end()
    torch.cuda.current_stream(gpu).wait_stream(side)
    for maps in (second, first):
        for key, t in bufs.items():
            t.copy_(torch.from_numpy(maps[key]))
        out.zero_()
        ranges.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert np.array_equal(ranges.cpu().numpy().view(np.uint32), R.ranges(maps).view(np.uint32))
        n, where = differing(out, R.contact_sheet(maps, N_SURFACE, PLASMA, scale=scale))
        assert n == 0, where
    assert R.ranges(first)[0] != R.ranges(second)[0]


@pytest.mark.parametrize("H,W,scale", [(37, 53, 1), (6, 52, 1), (2, 130, 3)])
def test_out_is_all_that_is_written(gpu, H, W, scale):
    from glorie_slam_amd.visualizer import PLASMA, contact_sheet, sheet_size
    maps = scene(H, W, 21)
    SH, SW = sheet_size(H, W, scale)
    guard = 3
    for shift in (0, 1):                                                          # the sheet on and off a dword boundary
        flat = torch.full((shift + (SH + 2 * guard) * SW * 3,), 0x5a, dtype=torch.uint8, device=gpu)
        rows = flat[shift:].view(SH + 2 * guard, SW, 3)
        out = rows[guard:guard + SH]
        assert contact_sheet(on_device(maps, gpu), N_SURFACE, scale=scale, out=out) is out
        n, where = differing(out, R.contact_sheet(maps, N_SURFACE, PLASMA, scale=scale))
        assert n == 0, where
        assert bool((rows[:guard] == 0x5a).all()) and bool((rows[guard + SH:] == 0x5a).all())
        assert bool((flat[:shift] == 0x5a).all())
    with pytest.raises(ValueError):
        contact_sheet(on_device(maps, gpu), N_SURFACE, scale=scale, out=torch.zeros(SH, SW + 1, 3, dtype=torch.uint8, device=gpu))
