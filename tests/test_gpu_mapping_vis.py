"""SequenceRunner(mapping_vis=..., save_rendered_image=...) and eval_kf_imgs(save_png=True) on the synthetic runner at the
smallest size the runner tests use (glorie_slam_amd/pipeline.py, visualizer.py, eval_render.py; reference
src/mapper.py:664-673, src/utils/Visualizer.py, src/utils/eval_render.py:54-57): the files and their names, the PNG's
bytes, the composed sheet against the restatement fed with the runner's own maps, and that the sheet only reads - a run
with it is bitwise the run without it.  Every comparison is exact."""
import functools
import os

import numpy as np
import pytest
import torch

import vis_ref as R

pytestmark = pytest.mark.gpu

H, W, RAYS, ITERS = 168, 224, 600, 3
K = 3
SCHEDULE = dict(iters_first=4, iters=3, geo_iter_first=1, geo_iter_ratio=0.3, min_iter_ratio=0.95)


def _runner(gpu, mapping=None, pointcloud=None, few_valid=(), **ctor):
    """keyframes [0, K) of the synthetic stream as init_state sets them up, each with a rectangle of missing depth; ctor:
    SequenceRunner's keyword arguments (none: the runner as synthetic_runner builds it); few_valid: keyframes whose
    tracker mask leaves 50 pixels (skipped with render_depth)"""
    import glorie_slam_amd.pipeline as P
    import glorie_slam_amd.visualizer  # noqa: F401  (what every test here is about)
    orig_cfg, orig_cls = P.synthetic_cfg, P.SequenceRunner

    def cfg(*a, **k):
        c = orig_cfg(*a, **k)
        c["mapping"].update(mapping or {})
        c["pointcloud"].update(pointcloud or {})
        return c
    P.synthetic_cfg = cfg
    if ctor:
        P.SequenceRunner = functools.partial(orig_cls, **ctor)
    try:
        run, c = P.synthetic_runner(gpu, K, map_iters=ITERS, map_rays=RAYS, H=H, W=W)
    finally:
        P.synthetic_cfg, P.SequenceRunner = orig_cfg, orig_cls
    video, imgs = c["video"], P.synthetic_images(K, H, W)
    prior = run.mono_depth_fn
    run.mono_depth_fn = lambda tstamp, image: prior(int(tstamp) // 2, image)     # (timestamps are 2 k below)
    for k in range(K):
        run.init_state(k)
        video.timestamp[k] = 2 * k                                      # the files carry the timestamp, not the slot
        run.images[k] = imgs[k].to(gpu)
        video.disps_up[k][20 + 10 * k:70 + 10 * k, 30 + 20 * k:100 + 20 * k] = 0
        m = video.disps_up[k] > 0
        if k in few_valid:
            m = torch.zeros_like(m)
            m[:5, :10] = True
        video.valid_depth_mask[k] = m
    video.intrinsics[:K] = c["intrinsics"].to(gpu) / 8.0
    video.counter.value = K
    return run, c


def _state(run):
    npc = run.npc
    return dict(geo=npc.geo_feats.clone(), col=npc.col_feats.clone(), cloud=npc.cloud_pos().clone(),
                dec=[p.detach().clone() for p in run.decoders.parameters()], gen=run.gen.get_state().clone(),
                losses=list(run.losses))


def _same(a, b):
    return (torch.equal(a["geo"], b["geo"]) and torch.equal(a["col"], b["col"]) and torch.equal(a["cloud"], b["cloud"])
            and all(torch.equal(p, q) for p, q in zip(a["dec"], b["dec"])) and torch.equal(a["gen"], b["gen"])
            and a["losses"] == b["losses"])


def _listing(root):
    return sorted(os.path.relpath(os.path.join(dp, f), root) for dp, _, fs in os.walk(root) for f in fs)


@pytest.fixture(scope="module")
def runs(gpu, tmp_path_factory):
    root = tmp_path_factory.mktemp("mapping_vis")
    off, _ = _runner(gpu)
    off.output = str(root / "off")
    os.makedirs(off.output)
    for k in range(K):
        off.map_keyframe(k)
    on, _ = _runner(gpu, mapping_vis=str(root / "on" / "mapping_vis"), save_rendered_image=True)
    on.vis_options = dict(keep=True)
    for k in range(K):
        on.map_keyframe(k)
    off.mapped = on.mapped = K                                          # (what map_pending counts)
    return dict(off=off, on=on, root=root)


def test_files_and_names(runs):
    from PIL import Image

    from glorie_slam_amd.visualizer import sheet_size
    on, root = runs["on"], runs["root"]
    assert on.mapping_vis is not None and on.save_rendered_image and runs["off"].mapping_vis is None
    want = sorted([f"mapping_vis/{2 * k:05d}_{ITERS - 1:04d}.jpg" for k in range(K)]
                  + [f"rendered_image/frame_{2 * k:05d}.png" for k in range(K)])
    assert _listing(root / "on") == want
    assert [os.path.relpath(p, root / "on") for p in on.visualizer.written] == \
        [n for k in range(K) for n in (f"rendered_image/frame_{2 * k:05d}.png", f"mapping_vis/{2 * k:05d}_{ITERS - 1:04d}.jpg")]
    SH, SW = sheet_size(H, W, 2, 4, 12)
    for k in range(K):
        with Image.open(root / "on" / f"mapping_vis/{2 * k:05d}_{ITERS - 1:04d}.jpg") as im:
            assert im.size == (SW, SH) and im.mode == "RGB"
            im.load()
    # the off run wrote nothing
    assert _listing(runs["off"].output) == [] and runs["off"].visualizer is None


def test_png_is_the_render(runs):
    from PIL import Image

    from glorie_slam_amd.visualizer import to_rgb8
    on, root = runs["on"], runs["root"]
    for k, kept in enumerate(on.visualizer.kept):
        assert kept["idx"] == 2 * k and kept["iter"] == ITERS - 1
        with Image.open(root / "on" / f"rendered_image/frame_{2 * k:05d}.png") as im:
            png = np.asarray(im.convert("RGB"))
        color = kept["maps"]["color"]
        assert np.array_equal(png, to_rgb8(color).cpu().numpy())
        assert np.array_equal(png, R.to_rgb8(color.float().cpu().numpy()))
        assert png.shape == (H, W, 3) and png.std() > 0


def test_sheet_is_the_restatement_of_the_runners_maps(runs):
    from glorie_slam_amd.visualizer import PLASMA
    on = runs["on"]
    assert len(on.visualizer.kept) == K
    n_surface = on.cfg["rendering"]["N_surface"]
    boxes = R.panel_boxes(H, W, 2, 4, 12)
    for k, kept in enumerate(on.visualizer.kept):
        maps = {key: t.float().cpu().numpy() for key, t in kept["maps"].items()}
        # the maps are the keyframe's own: the view it trained on, its image, holes where the tracker had none
        view = on._keyframe_view(k)
        assert torch.equal(kept["maps"]["render_depth"], view[0]) and torch.equal(kept["c2w"], view[1])
        assert torch.equal(kept["maps"]["gt_color"], on.images[k].permute(1, 2, 0))
        assert (maps["render_depth"] == 0).sum() == 50 * 70 and (maps["proj_depth"] > 0).any()
        assert (maps["sparse_proj_depth"] > 0).any() and maps["valid_ray_count"].max() > 0
        want = R.contact_sheet(maps, n_surface, PLASMA, scale=2, gutter=4, title=12)
        got = kept["sheet"].cpu().numpy()
        assert got.shape == want.shape
        for p, (y0, x0, ph, pw) in enumerate(boxes):
            assert np.array_equal(got[y0:y0 + ph, x0:x0 + pw], want[y0:y0 + ph, x0:x0 + pw]), (k, p)
        assert np.array_equal(got, want)                                  # and the white around them


def test_the_sheet_only_reads(runs):
    assert _same(_state(runs["off"]), _state(runs["on"]))
    assert len(runs["on"].losses) == K


def test_schedule_path_writes_its_sheets(gpu, tmp_path):
    base, _ = _runner(gpu, mapping=SCHEDULE, mapping_schedule=True)
    for k in range(2):
        base.map_keyframe(k)
    run, _ = _runner(gpu, mapping=SCHEDULE, mapping_schedule=True, mapping_vis=True)
    run.output = str(tmp_path)
    for k in range(2):
        run.map_keyframe(k)
    assert run.schedules == base.schedules and len(run.schedules) == 2
    assert _listing(tmp_path) == [f"mapping_vis/{2 * k:05d}_{run.schedules[k][0] - 1:04d}.jpg" for k in range(2)]
    # (two scheduled runs without sheets do not repeat each other's feature tables bit for bit, so the bitwise comparison
    # is test_the_sheet_only_reads on the plain path; what a scheduled run does repeat must not move either)
    a, b = _state(base), _state(run)
    assert torch.equal(a["gen"], b["gen"]) and torch.equal(a["cloud"], b["cloud"]) and len(b["losses"]) == 2
    # True without an output directory is an error, not a silent skip
    lost, _ = _runner(gpu, mapping=SCHEDULE, mapping_schedule=True, mapping_vis=True)
    with pytest.raises(ValueError):
        lost.map_keyframe(0)


def test_config_key_and_skipped_keyframes(gpu, tmp_path):
    """mapping.save_rendered_image of the config, and with render_depth a keyframe without enough tracker depth is
    skipped and gets no sheet; the sheet's tracker depth and prior are the render-depth path's"""
    run, _ = _runner(gpu, mapping=dict(render_depth="proxy", save_rendered_image=True),
                     pointcloud=dict(bind_npc_with_pose=True), few_valid=(1,), mapping_vis=str(tmp_path / "vis"))
    run.vis_options = dict(keep=True, titles=False)
    inner, first = run._frame_depths, {}

    def frame_depths(f):
        got = inner(f)
        if got is not None:
            first.setdefault(f, got)
        return got
    run._frame_depths = frame_depths
    for k in range(K):
        run.map_keyframe(k)
    assert run.skipped == [1] and run.save_rendered_image
    assert _listing(tmp_path) == sorted([f"vis/{2 * k:05d}_{ITERS - 1:04d}.jpg" for k in (0, 2)]
                                        + [f"rendered_image/frame_{2 * k:05d}.png" for k in (0, 2)])
    kept = run.visualizer.kept
    assert [e["idx"] for e in kept] == [0, 4]
    for e, k in zip(kept, (0, 2)):
        c2w, m_wq, droid = first[k]                                       # what the keyframe was prepared with
        assert torch.equal(e["maps"]["droid_depth"], droid) and torch.equal(e["maps"]["mono_depth"], m_wq)
        assert torch.equal(droid > 0, run.video.valid_depth_mask[k]) and not torch.equal(m_wq, run.mono_priors[k])
        assert bool((e["maps"]["render_depth"] > 0).all()) and torch.equal(e["c2w"], c2w)


def test_eval_png_copies(runs, tmp_path):
    from PIL import Image

    from glorie_slam_amd.eval_render import eval_kf_imgs
    on = runs["on"]
    before = _state(on)
    plain = eval_kf_imgs(on, output=str(tmp_path / "plain"))
    assert not os.path.exists(tmp_path / "plain" / "rerendered_keyframe_image")
    res = eval_kf_imgs(on, output=str(tmp_path / "png"), save_png=True, keep_renders=True)
    assert sorted(os.listdir(tmp_path / "png" / "rerendered_keyframe_image")) == [f"frame_{2 * k:05d}.png" for k in range(K)]
    assert plain["frame_cnt"] == res["frame_cnt"] == K
    for k, f in enumerate(res["frames"]):
        with Image.open(tmp_path / "png" / "rerendered_keyframe_image" / f"frame_{2 * k:05d}.png") as im:
            png = np.asarray(im.convert("RGB"))
        assert np.array_equal(png, R.to_rgb8(f["render"]["color"].float().cpu().numpy()))
    assert eval_kf_imgs(on, save_png=True)["frame_cnt"] == K              # without an output nothing is written
    assert _same(before, _state(on))
