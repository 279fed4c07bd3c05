"""Renderer.near_pcl_path = "device" (rays without a depth prior marched inside the sampling launch) against the host
route, and Renderer.render_view / SequenceRunner.render_view (novel views without any depth prior), on the 24 x 32 box
view with seed-43 POINT decoders."""
import numpy as np
import pytest
import torch

import near_pcl_ref as ref

pytestmark = pytest.mark.gpu
H, W = 24, 32
_STATE = {}


def _cfg(dev, sample_near_pcl=True):
    return {"device": str(dev),
            "pointcloud": {"nn_weighting": "distance", "use_dynamic_radius": True, "min_nn_num": 2,
                           "nn_num": 8, "radius_query": ref.RADIUS, "radius_add": 0.04, "radius_min": 0.02},
            "rendering": {"N_surface": 10, "near_end_surface": 0.95, "far_end_surface": 1.05,
                          "sample_near_pcl": sample_near_pcl, "sigmoid_coef": 0.1, "near_end": ref.NEAR},
            "model": {"encode_rel_pos_in_col": True, "encode_viewd": True, "c_dim": 32}}


class Cam:
    H, W, fx, fy, cx, cy = H, W, 16.0, 16.0, 15.5, 11.5


def _scene(gpu):
    if not _STATE:
        import glorie_slam_amd.synth as synth
        from glorie_slam_amd.decoder import POINT
        from glorie_slam_amd.neural_point import NeuralPointCloud
        sc = ref.scene()
        ro, rd, depth, radius, c2w = synth.box_rays(H, W, fx=16.0, fy=16.0, cx=15.5, cy=11.5)
        t = lambda x: torch.from_numpy(x).to(gpu)
        cfg = _cfg(gpu)
        npc = NeuralPointCloud(cfg)
        npc.add_points(t(sc["cloud"]), t(sc["geo"]), t(sc["col"]))
        torch.manual_seed(43)
        dec = POINT(cfg, use_view_direction=True).eval().to(gpu)
        gt0 = depth.copy()
        gt0[::5] = 0.0
        _STATE.update(npc=npc, dec=dec, ro=t(ro), rd=t(rd), depth=t(depth), gt0=t(gt0), radius=t(radius * 2.5), c2w=t(c2w),
                      ro_np=ro, rd_np=rd, cloud=sc["cloud"])
    return _STATE


def _renderer(gpu, path, sample_near_pcl=True):
    from glorie_slam_amd.renderer import Renderer
    ren = Renderer(_cfg(gpu, sample_near_pcl), Cam())
    ren.near_pcl_path = path
    return ren


def _kw(st):
    npc = st["npc"]
    return dict(npc_geo_feats=npc.geo_feats, npc_col_feats=npc.col_feats, cloud_pos=npc.cloud_pos())


def test_device_route_equals_host_route_on_mixed_batch(gpu):
    """every fifth depth zeroed, 25 probes: the valid-ray masks and counts are equal on firm rays, the floats agree within
    what test_render_fast_path_equals_general_path grants the fused decoders against the op-by-op ones"""
    st = _scene(gpu)
    npc, dec = st["npc"], st["dec"]
    outs = {}
    with torch.no_grad():
        for path in ("host", "device"):
            ren = _renderer(gpu, path)
            outs[path] = ren.render_batch_ray(npc, dec, st["rd"], st["ro"], gpu, "color", gt_depth=st["gt0"],
                                              dynamic_r_query=st["radius"], **_kw(st))
    gt0 = st["gt0"]
    far = float(torch.minimum(5 * gt0.mean(), torch.max(gt0 * 1.2)).cpu())
    m = ref.march(st["cloud"], st["ro_np"], st["rd_np"], ref.NEAR, far, 25, 10)
    marched = (gt0 <= 0).cpu().numpy()
    firm = torch.from_numpy(m["firm"] | ~marched).to(gpu)
    assert (~m["firm"] & marched).sum() <= ref.MAX_NON_FIRM_SHARE * marched.sum()
    assert int((outs["device"][3] & torch.from_numpy(marched).to(gpu)).sum()) > 50        # marched rays do render
    for a, b in zip(outs["device"], outs["host"]):
        assert a.dtype == b.dtype and a.shape == b.shape
        if a.dtype.is_floating_point:
            torch.testing.assert_close(a[firm], b[firm], rtol=1e-6, atol=1e-7)
        else:
            assert torch.equal(a[firm], b[firm])


def test_default_route_is_host_and_unchanged(gpu):
    """near_pcl_path defaults to "host": a batch with depth-less rays still returns the general path's bits"""
    st = _scene(gpu)
    from glorie_slam_amd.renderer import Renderer
    ren = Renderer(_cfg(gpu), Cam())
    assert ren.near_pcl_path == "host"
    with torch.no_grad():
        a = ren.render_batch_ray(st["npc"], st["dec"], st["rd"], st["ro"], gpu, "color", gt_depth=st["gt0"],
                                 dynamic_r_query=st["radius"], **_kw(st))
        ren.use_fast_path = False
        b = ren.render_batch_ray(st["npc"], st["dec"], st["rd"], st["ro"], gpu, "color", gt_depth=st["gt0"],
                                 dynamic_r_query=st["radius"], **_kw(st))
    for x, y in zip(a, b):
        assert torch.equal(x, y)
    with pytest.raises(ValueError):
        ren.near_pcl_path = "gpu"
    assert ren.near_pcl_path == "host"


def test_without_sample_near_pcl_device_mode_takes_the_host_route(gpu):
    st = _scene(gpu)
    with torch.no_grad():
        a, b = [_renderer(gpu, path, sample_near_pcl=False).render_batch_ray(
            st["npc"], st["dec"], st["rd"], st["ro"], gpu, "color", gt_depth=st["gt0"], dynamic_r_query=st["radius"],
            **_kw(st)) for path in ("device", "host")]
    for x, y in zip(a, b):
        assert torch.equal(x, y)


@pytest.fixture(scope="module")
def view(gpu):
    """render_view of the box from its centre, far = 6: ceil(5.7 / 0.08) + 1 = 73 probes (two chunks)"""
    st = _scene(gpu)
    ren = _renderer(gpu, "host")                      # render_view marches on the device whatever the switch says
    out = ren.render_view(st["npc"], st["dec"], st["c2w"], gpu, far=6.0)
    assert ren.near_pcl_path == "host"
    return ren, out


def test_render_view_equals_render_batch_ray_in_device_mode(gpu, view):
    st = _scene(gpu)
    ren, out = view
    dev = _renderer(gpu, "device")
    const = torch.full((H * W,), 0.5 * (0.04 + ref.RADIUS), device=gpu)
    with torch.no_grad():
        ref_out = dev.render_batch_ray(st["npc"], st["dec"], st["rd"], st["ro"], gpu, "color", gt_depth=None,
                                       dynamic_r_query=const, near=(6.0, 73), **_kw(st))
    assert out[0].dtype == torch.float64 and out[0].shape == (H, W) and out[2].shape == (H, W, 3)
    for k, (a, b) in enumerate(zip(out, ref_out)):
        b = b.reshape(H, W, 3) if k == 2 else b.double().reshape(H, W)
        assert torch.equal(a, b)
    # the same frame through render_img in device mode with the reference's far = 10 and 25 probes is another march
    img = dev.render_img(st["npc"], st["dec"], st["c2w"], gpu, "color", gt_depth=None, dynamic_r_query=const.reshape(H, W),
                         **_kw(st))
    with torch.no_grad():
        b10 = dev.render_batch_ray(st["npc"], st["dec"], st["rd"], st["ro"], gpu, "color", gt_depth=None,
                                   dynamic_r_query=const, **_kw(st))
    assert torch.equal(img[0], b10[0].double().reshape(H, W)) and torch.equal(img[3], b10[3].double().reshape(H, W))


def test_render_view_depth_lies_in_the_bracket(gpu, view):
    """a valid ray's depth is a convex combination of its samples, which span the restatement's [lo, hi]; a ray with fewer
    than two occupied probes is not valid"""
    st = _scene(gpu)
    _, out = view
    m = ref.march(st["cloud"], st["ro_np"], st["rd_np"], ref.NEAR, 6.0, 73, 10)
    assert (~m["firm"]).mean() <= ref.MAX_NON_FIRM_SHARE
    depth = out[0].reshape(-1).cpu().numpy()
    valid = out[3].reshape(-1).cpu().numpy() > 0
    firm = m["firm"]
    assert not valid[firm & ~m["near_mask"]].any()
    sel = firm & valid
    assert sel.sum() > 0.8 * H * W
    lo, hi = m["lo"].astype(np.float32).astype(np.float64), m["hi"].astype(np.float32).astype(np.float64)
    print("render_view depth margins: min(depth - lo) %.3e  min(hi - depth) %.3e  bracket width %.3e" % (
        (depth - lo)[sel].min(), (hi - depth)[sel].min(), (hi - lo)[sel].min()))
    assert np.all(depth[sel] >= lo[sel]) and np.all(depth[sel] <= hi[sel])


def test_render_view_rejects_what_the_march_does_not_cover(gpu):
    st = _scene(gpu)
    ren = _renderer(gpu, "device", sample_near_pcl=False)
    with pytest.raises(RuntimeError):
        ren.render_view(st["npc"], st["dec"], st["c2w"], gpu, far=6.0)
    with pytest.raises(ValueError):
        _renderer(gpu, "device").render_view(st["npc"], st["dec"], st["c2w"], gpu, far=6.0, intervals=1)


def test_sequence_runner_render_view(gpu):
    """SequenceRunner.render_view on the synthetic runner: one mapped keyframe seen from a pose beside it"""
    import glorie_slam_amd.pipeline as P
    h, w, K = 168, 224, 2
    with pytest.raises(ValueError):
        P.SequenceRunner(None, None, {"device": str(gpu), "tracking": {}}, None, None, _renderer(gpu, "host"), None,
                         near_pcl_path="gpu")
    run, c = P.synthetic_runner(gpu, K, map_iters=2, map_rays=600, H=h, W=w)
    assert run.renderer.near_pcl_path == "host"
    video, imgs = c["video"], P.synthetic_images(K, h, w)
    for k in range(K):
        run.init_state(k)
        video.timestamp[k] = k
        run.images[k] = imgs[k].to(gpu)
        video.valid_depth_mask[k] = video.disps_up[k] > 0
    video.intrinsics[:K] = c["intrinsics"].to(gpu) / 8.0
    video.counter.value = K
    run.add_stride = 2                                  # a cloud dense enough for the 8 cm probe balls to meet it
    run.map_keyframe(0)
    assert run.npc.pts_num() > 0
    c2w = run._keyframe_view(0)[1].clone()
    c2w[:3, 3] += 0.02
    depth, unc, color, vmask, vcount = run.render_view(c2w)
    assert depth.shape == (h, w) and color.shape == (h, w, 3) and depth.dtype == torch.float64
    valid = vmask > 0
    print("SequenceRunner.render_view: valid pixels", int(valid.sum()), "of", h * w)
    assert int(valid.sum()) > 0
    assert bool(torch.isfinite(color[valid]).all()) and bool(torch.isfinite(depth[valid]).all())
    assert bool((depth[valid] > 0).all())
