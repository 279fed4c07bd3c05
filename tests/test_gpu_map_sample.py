"""glorie_valid_index_build, glorie_sample_window_rays and glorie_depth_gate (glorie_slam_amd/map_sample.py) on the GPU:
tables, pixels, rays and gate bit-equal to the numpy restatement (tests/map_sample_ref.py) on every scene and gate vector -
everything is integer, compare or select except the ray direction, whose operation order window_rays pins - and the
sampled rays bit-equal to window_rays fed the returned pixels.  Both image layouts, radius maps, a constant radius and
none; no ray and no frame; argument errors; no host synchronisation; a second stream."""
import numpy as np
import pytest
import torch

from map_sample_ref import (GATE_KINDS, GATE_SIZES, depth_gate_ref, gate_vector, sample_window_rays_ref, scene,
                            valid_index_ref)

pytestmark = pytest.mark.gpu

NAMES = ["A", "B", "C", "D"]
_SCENES = {}


def _scene(name):
    """the scene, its tables in both modes and the reference of every draw set in the three radius modes, computed once"""
    if name not in _SCENES:
        s = scene(name)
        a = (s["depths"], s["images"], s["c2ws"])
        refs = []
        for draws in s["draws"]:
            b = (draws, s["per"]) + s["K"]
            refs.append({"maps": sample_window_rays_ref(*a, *b, radius_maps=s["radius_maps"]),
                         "const": sample_window_rays_ref(*a, *b, const_radius=0.06),
                         "none": sample_window_rays_ref(*a, *b),
                         "all": sample_window_rays_ref(*a, *b, mode="all", radius_maps=s["radius_maps"])})
        _SCENES[name] = (s, {m: valid_index_ref(s["depths"], m) for m in ("depth", "all")}, refs)
    return _SCENES[name]


def _table(s, gpu, mode, channels_first=True):
    from glorie_slam_amd.window_rays import WindowTable
    t = lambda x: torch.from_numpy(x).to(gpu)
    images = s["images"] if channels_first else np.ascontiguousarray(s["images"].transpose(0, 2, 3, 1))
    return WindowTable(list(t(s["depths"])), list(t(images)), t(s["c2ws"]),
                       list(t(s["radius_maps"])) if mode in ("maps", "all") else None, channels_first=channels_first)


def _bits(x):
    x = np.ascontiguousarray(x)
    return x.view({4: np.uint32, 8: np.uint64}[x.dtype.itemsize])


def _equal_bits(got, ref):
    assert len(got) == len(ref)
    for g, r in zip(got, ref):
        assert (g is None) == (r is None)
        if g is not None:
            g = g.cpu().numpy()
            assert g.dtype == r.dtype and g.shape == r.shape
            assert np.array_equal(_bits(g), _bits(r))


@pytest.mark.parametrize("mode", ["depth", "all"])
@pytest.mark.parametrize("name", NAMES)
def test_tables(gpu, name, mode):
    from glorie_slam_amd.map_sample import ValidIndex
    s, tables, _ = _scene(name)
    index = ValidIndex(_table(s, gpu, "none"), mode)
    words, prefix = tables[mode]
    assert index.words.dtype == torch.int64 and index.prefix.dtype == torch.int32
    assert np.array_equal(index.words.cpu().numpy().view(np.uint64), words)
    assert np.array_equal(index.prefix.cpu().numpy(), prefix)
    assert np.array_equal(index.counts.cpu().numpy(), prefix[:, -1])


@pytest.mark.parametrize("mode", ["maps", "const", "none", "all"])
@pytest.mark.parametrize("name", NAMES)
def test_bits_of_the_restatement(gpu, name, mode):
    from glorie_slam_amd.map_sample import ValidIndex, sample_window_rays
    from glorie_slam_amd.window_rays import window_rays
    s, tables, refs = _scene(name)
    table = _table(s, gpu, mode)
    index = ValidIndex(table, "all" if mode == "all" else "depth")
    const = 0.06 if mode == "const" else None
    for draws, ref in zip(s["draws"], refs):
        dr = torch.from_numpy(draws).to(gpu)
        got = sample_window_rays(table, index, dr, s["per"], *s["K"], const_radius=const)
        _equal_bits(got, ref[mode])
        # window_rays on the returned pixels: the same bits, but for the depth 0 of a slot without a valid pixel
        again = window_rays(table, got[5], got[6], s["per"], *s["K"], const_radius=const)
        empty = torch.from_numpy(np.repeat(tables["all" if mode == "all" else "depth"][1][:, -1] == 0, s["per"])).to(gpu)
        for q, (a, b) in enumerate(zip(got[:5], again)):
            assert (a is None) == (b is None)
            if a is None:
                continue
            if q == 2:
                assert not bool(a[empty].any()) and not bool((b[empty] > 0).any())
                a, b = a[~empty], b[~empty]
            assert torch.equal(a.view(torch.int32), b.view(torch.int32))
        if mode != "all":
            assert bool((got[2][~empty] > 0).all())                     # every sampled depth is valid


def test_channels_last_images(gpu):
    from glorie_slam_amd.map_sample import ValidIndex, sample_window_rays
    s, _, refs = _scene("C")
    table = _table(s, gpu, "maps", channels_first=False)
    got = sample_window_rays(table, ValidIndex(table), torch.from_numpy(s["draws"][0]).to(gpu), s["per"], *s["K"])
    _equal_bits(got, refs[0]["maps"])


def test_no_rays_and_no_frames(gpu):
    from glorie_slam_amd import _lib as L
    from glorie_slam_amd.map_sample import ValidIndex, sample_window_rays, depth_gate
    s, _, _ = _scene("A")
    table = _table(s, gpu, "maps")
    index = ValidIndex(table)
    out = sample_window_rays(table, index, torch.zeros(0, dtype=torch.int64, device=gpu), 0, *s["K"])
    assert [tuple(o.shape) for o in out] == [(0, 3), (0, 3), (0,), (0, 3), (0,), (0,), (0,)]
    keep, stats = depth_gate(torch.zeros(0, device=gpu))
    assert keep.shape == (0,) and stats.tolist() == [0.0] * 4
    # M = 0 at the C ABI (a WindowTable has at least one frame): nothing is launched, no pointer is read
    lib, none = L.load(), L.ptr(None)
    assert lib.glorie_valid_index_build(none, 0, 5, 7, 0, none, none, L.stream_ptr(gpu)) == 0
    assert lib.glorie_sample_window_rays(none, none, none, none, 0, 4, 1, 5, 7, 1.0, 1.0, 0.0, 0.0, none, none, none, 0.0, 0,
                                         none, none, none, none, none, none, none, L.stream_ptr(gpu)) == 0
    assert lib.glorie_depth_gate(none, 0, none, L.ptr(stats), L.stream_ptr(gpu)) == 0
    assert lib.glorie_depth_gate(L.ptr(stats), (1 << 22) + 1, L.ptr(stats), L.ptr(stats), L.stream_ptr(gpu)) == -4
    assert lib.glorie_valid_index_build(none, 1, 5, 7, 0, L.ptr(index.words), L.ptr(index.prefix), L.stream_ptr(gpu)) == -1
    assert lib.glorie_valid_index_build(none, 1, 5, 7, 2, L.ptr(index.words), L.ptr(index.prefix), L.stream_ptr(gpu)) == -1
    torch.cuda.synchronize()


def test_argument_errors(gpu):
    from glorie_slam_amd._lib import GlorieError
    from glorie_slam_amd.map_sample import ValidIndex, depth_gate, sample_window_rays
    s, _, _ = _scene("A")
    table, other = _table(s, gpu, "maps"), _table(s, gpu, "maps")
    index = ValidIndex(table)
    draws = torch.from_numpy(s["draws"][0]).to(gpu)
    with pytest.raises(ValueError):
        ValidIndex(table, "mono")
    with pytest.raises(ValueError):
        ValidIndex(list(table.depths))
    with pytest.raises(ValueError):
        sample_window_rays(other, index, draws, s["per"], *s["K"])          # the index of another table
    with pytest.raises(ValueError):
        sample_window_rays(table, index, draws[:-1], s["per"], *s["K"])     # N != M * per
    with pytest.raises(ValueError):
        sample_window_rays(table, index, draws.int(), s["per"], *s["K"])    # not int64
    with pytest.raises(GlorieError):
        sample_window_rays(table, index, draws.cpu(), s["per"], *s["K"])    # a CPU tensor
    with pytest.raises(GlorieError):
        depth_gate(torch.ones(5))
    with pytest.raises(ValueError):
        depth_gate(torch.ones(5, 2, device=gpu))
    with pytest.raises(ValueError):
        depth_gate(torch.ones(5, device=gpu).double())


@pytest.mark.parametrize("kind", GATE_KINDS)
def test_gate_bits(gpu, kind):
    from glorie_slam_amd.map_sample import depth_gate
    for n in GATE_SIZES:
        d = gate_vector(kind, n)
        keep, stats = depth_gate(torch.from_numpy(d).to(gpu))
        _equal_bits((keep, stats), depth_gate_ref(d))


def test_gate_of_the_sampled_depths(gpu):
    """the gate on what the sampler returns (zero-depth slots among it), and a view that is not contiguous"""
    from glorie_slam_amd.map_sample import ValidIndex, depth_gate, sample_window_rays
    s, _, refs = _scene("B")
    table = _table(s, gpu, "none")
    d = sample_window_rays(table, ValidIndex(table), torch.from_numpy(s["draws"][0]).to(gpu), s["per"], *s["K"])[2]
    _equal_bits(depth_gate(d), depth_gate_ref(refs[0]["none"][2]))
    _equal_bits(depth_gate(d.repeat_interleave(2)[::2]), depth_gate_ref(refs[0]["none"][2]))


def test_no_host_synchronisation(gpu):
    from glorie_slam_amd.map_sample import ValidIndex, depth_gate, sample_window_rays
    s, _, refs = _scene("D")
    table = _table(s, gpu, "maps")
    draws = torch.from_numpy(s["draws"][0]).to(gpu)
    index = ValidIndex(table)                                        # (and once before: the library is loaded)
    sample_window_rays(table, index, draws, s["per"], *s["K"])
    torch.cuda.synchronize()
    before = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        index = ValidIndex(table)
        got = sample_window_rays(table, index, draws, s["per"], *s["K"])
        gate = depth_gate(got[2])
    finally:
        torch.cuda.set_sync_debug_mode(before)
    _equal_bits(got, refs[0]["maps"])
    _equal_bits(gate, depth_gate_ref(refs[0]["maps"][2]))


def test_second_stream(gpu):
    from glorie_slam_amd.map_sample import ValidIndex, depth_gate, sample_window_rays
    s, _, refs = _scene("C")
    table = _table(s, gpu, "maps")
    draws = torch.from_numpy(s["draws"][0]).to(gpu)
    side = torch.cuda.Stream(gpu)
    side.wait_stream(torch.cuda.current_stream(gpu))
    with torch.cuda.stream(side):
        got = sample_window_rays(table, ValidIndex(table), draws, s["per"], *s["K"])
        gate = depth_gate(got[2])
    side.synchronize()
    _equal_bits(got, refs[0]["maps"])
    _equal_bits(gate, depth_gate_ref(refs[0]["maps"][2]))
