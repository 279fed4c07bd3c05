"""glorie_window_rays (glorie_slam_amd/window_rays.py) on the GPU: every output bit-equal to the numpy restatement
(tests/window_rays_ref.py); against the per-frame torch composition on the device the gathers and rays_o bit-equal and
rays_d within five roundings a side.  General rotations with translation, non-integer intrinsics; shapes of less than a
wave (A), more than 64 frames with a ray count that is no multiple of 64 or 256 (B), several workgroups per frame with
a ragged tail in both image layouts (C), and no ray at all."""
import numpy as np
import pytest
import torch

from window_rays_ref import EPS32, rays_d_f64, scene, torch_composition, window_rays_ref

pytestmark = pytest.mark.gpu

_SCENES = {}


def _scene(name):
    """the scene and its numpy reference in the three radius modes, computed once"""
    if name not in _SCENES:
        s = scene(name)
        a = (s["depths"], s["images"], s["c2ws"], s["ii"], s["jj"], s["per"]) + s["K"]
        _SCENES[name] = (s, {"maps": window_rays_ref(*a, radius_maps=s["radius_maps"]),
                             "const": window_rays_ref(*a, const_radius=0.06), "none": window_rays_ref(*a)})
    return _SCENES[name]


def _table(s, gpu, mode, channels_first=True):
    from glorie_slam_amd.window_rays import WindowTable
    t = lambda x: torch.from_numpy(x).to(gpu)
    images = s["images"] if channels_first else np.ascontiguousarray(s["images"].transpose(0, 2, 3, 1))
    return WindowTable(list(t(s["depths"])), list(t(images)), t(s["c2ws"]),
                       list(t(s["radius_maps"])) if mode == "maps" else None, channels_first=channels_first)


def _call(s, table, gpu, mode):
    from glorie_slam_amd.window_rays import window_rays
    ii, jj = torch.from_numpy(s["ii"]).to(gpu), torch.from_numpy(s["jj"]).to(gpu)
    assert int(ii.min()) >= 0 and int(ii.max()) < s["W"] and int(jj.min()) >= 0 and int(jj.max()) < s["H"]
    return window_rays(table, ii, jj, s["per"], *s["K"], const_radius=0.06 if mode == "const" else None)


def _equal_bits(got, ref):
    for g, r in zip(got, ref):
        assert (g is None) == (r is None)
        if g is not None:
            g = g.cpu().numpy()
            assert g.dtype == r.dtype and g.shape == r.shape
            assert np.array_equal(g.view(np.uint32), np.ascontiguousarray(r).view(np.uint32))


@pytest.mark.parametrize("mode", ["maps", "const", "none"])
@pytest.mark.parametrize("name", ["A", "B", "C"])
def test_bits_of_the_restatement(gpu, name, mode):
    s, refs = _scene(name)
    table = _table(s, gpu, mode)
    got = _call(s, table, gpu, mode)
    _equal_bits(got, refs[mode])
    again = _call(s, table, gpu, mode)                          # a repeated call is bitwise equal
    for a, b in zip(got, again):
        assert (a is None and b is None) or torch.equal(a, b)


def test_channels_last_images(gpu):
    s, refs = _scene("C")
    _equal_bits(_call(s, _table(s, gpu, "maps", channels_first=False), gpu, "maps"), refs["maps"])


@pytest.mark.parametrize("name", ["A", "B", "C"])
def test_against_the_torch_composition(gpu, name):
    s, _ = _scene(name)
    t = lambda x: torch.from_numpy(x).to(gpu)
    ro, rd, d, col, rad = _call(s, _table(s, gpu, "maps"), gpu, "maps")
    tro, trd, td, tcol, trad = torch_composition(t(s["depths"]), t(s["images"]), t(s["c2ws"]), t(s["ii"]), t(s["jj"]),
                                                 s["per"], *s["K"], gpu, radius_maps=t(s["radius_maps"]))
    assert torch.equal(ro, tro) and torch.equal(d, td) and torch.equal(col, tcol) and torch.equal(rad, trad)
    _, S = rays_d_f64(s["c2ws"], s["ii"], s["jj"], s["per"], *s["K"])
    err = (rd.double() - trd.double()).abs().cpu().numpy()
    print("max err / bound", float((err / (5 * EPS32 * S)).max()))
    assert (err <= 5 * EPS32 * S).all()


def test_no_rays(gpu):
    from glorie_slam_amd.window_rays import window_rays
    s, _ = _scene("A")
    empty = torch.zeros(0, dtype=torch.int64, device=gpu)
    out = window_rays(_table(s, gpu, "maps"), empty, empty, 0, *s["K"])
    assert [tuple(o.shape) for o in out] == [(0, 3), (0, 3), (0,), (0, 3), (0,)]
    torch.cuda.synchronize()


def test_non_contiguous_inputs(gpu):
    """maps that are views (a transposed depth, a permuted image, float64 matrices) go through the table's copies"""
    from glorie_slam_amd.window_rays import WindowTable, window_rays
    s, refs = _scene("A")
    t = lambda x: torch.from_numpy(x).to(gpu)
    depths = [t(np.ascontiguousarray(d.T)).t() for d in s["depths"]]
    images = [t(np.ascontiguousarray(im.transpose(1, 2, 0))).permute(2, 0, 1) for im in s["images"]]
    radius = [t(np.ascontiguousarray(r.T)).t() for r in s["radius_maps"]]
    assert not depths[0].is_contiguous() and not images[0].is_contiguous()
    table = WindowTable(depths, images, t(s["c2ws"]).double()[:, :3, :], radius)
    ii, jj = t(s["ii"]), t(s["jj"])
    got = window_rays(table, ii.repeat_interleave(2)[::2], jj.repeat_interleave(2)[::2], s["per"], *s["K"])
    _equal_bits(got, refs["maps"])


def test_table_errors(gpu):
    from glorie_slam_amd.window_rays import WindowTable, window_rays
    s, _ = _scene("A")
    t = lambda x: torch.from_numpy(x).to(gpu)
    d, im, c, r = list(t(s["depths"])), list(t(s["images"])), t(s["c2ws"]), list(t(s["radius_maps"]))
    with pytest.raises(ValueError):
        WindowTable([], [], c[:0])
    with pytest.raises(ValueError):
        WindowTable(d, im[:2], c)                                           # counts differ
    with pytest.raises(ValueError):
        WindowTable(d, im, c, r[:1])
    with pytest.raises(ValueError):
        WindowTable(d, im, c[:2])
    with pytest.raises(ValueError):
        WindowTable(d, im, c[:, :2, :])                                     # not [M,4,4] / [M,3,4]
    with pytest.raises(ValueError):
        WindowTable(d[:2] + [d[2][:, :-1]], im, c)                          # a depth map of another size
    with pytest.raises(ValueError):
        WindowTable(d, im, c, channels_first=False)                         # [3,H,W] images read as [H,W,3]
    with pytest.raises(ValueError):
        WindowTable(d, im[:2] + [im[2].cpu()], c)                           # a map on the host
    with pytest.raises(ValueError):
        WindowTable(d, im, c, [x.long() for x in r])                        # integer maps
    table = WindowTable(d, im, c)
    ii, jj = t(s["ii"]), t(s["jj"])
    with pytest.raises(ValueError):
        window_rays(table, ii[:-1], jj[:-1], s["per"], *s["K"])             # N != M * per
    with pytest.raises(ValueError):
        window_rays(table, ii.int(), jj.int(), s["per"], *s["K"])           # not int64
