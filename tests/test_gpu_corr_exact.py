"""The correlation kernels against exact references, bit for bit, on scenes where no summation order is free
(tests/corr_ref.py builds the scenes and proves the claims; tests/test_corr_ref.py checks the builders on the CPU).

No comparison in this file carries a tolerance except the alt-corr test on general fp32 data, whose bound is the
oracle's own fp32 error measured on the same inputs."""
import functools

import numpy as np
import pytest
import torch

import corr_ref as R
from oracle import corr as ocorr

pytestmark = pytest.mark.gpu


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint16)


def _same_bits(got, ref, what, names=None):
    """fp16 arrays equal bit for bit; `names` labels the slices of axis 0 in the message"""
    got, ref = np.asarray(got), np.asarray(ref)
    assert got.dtype == ref.dtype == np.float16 and got.shape == ref.shape, (what, got.dtype, got.shape, ref.shape)
    ne = _bits(got) != _bits(ref)
    if ne.any():
        per = ne.reshape(ne.shape[0], -1).mean(1)
        bad = [(names[i] if names else i, float(per[i])) for i in np.nonzero(per)[0]]
        idx = tuple(int(v) for v in np.argwhere(ne)[0])
        raise AssertionError(f"{what}: {int(ne.sum())} of {ne.size} values differ; share per slice {bad}; first at {idx}: "
                             f"got {got[idx]!r} want {ref[idx]!r}")


def _poisoned(N, C, h, w, dev):
    """a channels-last fp16 map [N, C, h, w] of a non-zero pattern"""
    t = ((torch.arange(N * h * w * C, device=dev) % 251) + 1).half().view(N, h, w, C).permute(0, 3, 1, 2)
    assert t.is_contiguous(memory_format=torch.channels_last) or h * w == 1
    return t


def _random_encoder(seed, dev):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(128, 196, 1, 1, generator=g) / 14).to(dev), torch.randn(128, generator=g).to(dev)


@functools.lru_cache(maxsize=None)
def _otf_scene(h, w):
    """order-free features, the coordinate scenes (a)-(g) for the four edges, and the oracle's lookup - computed once"""
    fm = R.order_free_features(h * 100 + w, 3, h, w)
    coords, ii, jj, names = R.otf_scene_coords(h, w)
    for n in names:
        R.check_plan(n, h, w)                                      # every scene reaches the branches it names
    vols = R.otf_volumes(fm, R.OTF_II, R.OTF_JJ)
    ref = R.otf_lookup([np.tile(v, (len(names), 1, 1, 1, 1)) for v in vols], coords)
    ref.setflags(write=False)
    labels = [f"{n}/edge{e}" for n in names for e in range(len(R.OTF_II))]
    return fm, coords, ii, jj, labels, ref


def _c5(coords, dev):
    """[N, 2, h, w] numpy -> [1, N, h, w, 2] device tensor (the blocks' call contract)"""
    return torch.from_numpy(coords).to(dev).permute(0, 2, 3, 1)[None].contiguous()


# ---- volume-free lookup ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("h,w", R.SIZES_ALL)
def test_otf_lookup_bit_exact_on_every_box_branch(gpu, h, w):
    """OtfCorrBlock == oracle.corr.corr_otf bit for bit on order-free features: shared boxes of exactly 320 targets, the
    first size that does not fit, blocks with fitting and non-fitting quadrants, single pixels at every level, levels that
    fall back in front of levels that share a box, boxes partly and wholly outside the map on every side, coordinates of
    huge magnitude (exact zeros); edges incl. ii == jj.  lookup_encode(want_corr=True) returns the same bits."""
    from glorie_slam_amd.droid_net import OtfCorrBlock
    fm, coords, ii, jj, labels, ref = _otf_scene(h, w)
    blk = OtfCorrBlock(torch.from_numpy(fm).to(gpu)[None])
    c5, it, jt = _c5(coords, gpu), torch.from_numpy(ii).to(gpu), torch.from_numpy(jj).to(gpu)
    got = blk(c5, it, jt)[0].cpu().numpy()
    _same_bits(got, ref, f"OtfCorrBlock {h}x{w}", labels)
    huge = [i for i, s in enumerate(labels) if s.startswith("huge/")]
    assert not _bits(got[huge]).any()
    wgt, bias = _random_encoder(1, gpu)
    enc = torch.zeros(len(ii), 128, h, w, dtype=torch.float16, device=gpu).contiguous(memory_format=torch.channels_last)
    corr = blk.lookup_encode(c5, it, jt, OtfCorrBlock.pack_encoder(wgt), bias, enc, want_corr=True)
    _same_bits(corr[0].cpu().numpy(), ref, f"lookup_encode(want_corr) {h}x{w}", labels)


@pytest.mark.parametrize("num_levels", [1, 2, 3])
@pytest.mark.parametrize("h,w", [(16, 24), (12, 16), (13, 22)])
def test_otf_lookup_fewer_levels_bit_exact(gpu, h, w, num_levels):
    """glorie_corr_otf with num_levels < 4: the first levels of the four-level lookup, bit for bit"""
    from glorie_slam_amd.droid_net import OtfCorrBlock
    fm, coords, ii, jj, labels, ref = _otf_scene(h, w)
    for n in R.OTF_SCENES:
        R.check_plan(n, h, w, num_levels)
    blk = OtfCorrBlock(torch.from_numpy(fm).to(gpu)[None], num_levels=num_levels)
    got = blk(_c5(coords, gpu), torch.from_numpy(ii).to(gpu), torch.from_numpy(jj).to(gpu))[0].cpu().numpy()
    _same_bits(got, ref[:, :49 * num_levels], f"glorie_corr_otf {num_levels} levels {h}x{w}", labels)


@pytest.mark.parametrize("h,w", [(16, 24), (13, 22)])
def test_otf_fused_encoder_bit_exact(gpu, h, w):
    """glorie_corr_otf_encode on the encoder-exact scene: relu(W corr + b) == the float64 reference rounded once to fp16, bit
    for bit, written into a 128-channel slice of a 320-channel map whose other channels keep their (non-zero) contents;
    the encoder-only form agrees"""
    from glorie_slam_amd.droid_net import OtfCorrBlock
    fm, coords = R.otf_integer_scene(7, 3, h, w)
    ii, jj = R.OTF_ENC_II, R.OTF_ENC_JJ
    ref_corr = R.otf_lookup(R.otf_volumes(fm, ii, jj), coords)
    wgt, bias = R.integer_encoder(2, -1, 1, density=0.5)
    ref_enc, _, _ = R.encoder_reference(ref_corr, wgt.reshape(128, 196), bias)        # proves the bound for THIS scene
    blk = OtfCorrBlock(torch.from_numpy(fm).to(gpu)[None])
    c5, it, jt = _c5(coords, gpu), torch.from_numpy(ii).to(gpu), torch.from_numpy(jj).to(gpu)
    N = len(ii)
    wide = _poisoned(N, 320, h, w, gpu)
    poison = wide.clone()
    pw, pb = OtfCorrBlock.pack_encoder(torch.from_numpy(wgt).to(gpu)), torch.from_numpy(bias).to(gpu)
    corr = blk.lookup_encode(c5, it, jt, pw, pb, wide[:, 128:256], want_corr=True)
    _same_bits(corr[0].cpu().numpy(), ref_corr, f"lookup of the encoder launch {h}x{w}")
    _same_bits(wide[:, 128:256].cpu().numpy(), ref_enc, f"fused encoder {h}x{w}")
    assert torch.equal(wide[:, :128], poison[:, :128]) and torch.equal(wide[:, 256:], poison[:, 256:])
    only = _poisoned(N, 128, h, w, gpu)
    assert blk.lookup_encode(c5, it, jt, pw, pb, only) is None
    _same_bits(only.cpu().numpy(), ref_enc, f"encoder-only form {h}x{w}")


# ---- displacement-major lookup --------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _dm_scene(h, w):
    coords, names = R.dm_scene_coords(h, w)
    levels = R.dm_volumes(h * 100 + w, len(names), h, w)
    ref = ocorr.corr_lookup_pyramid(levels, coords, 3)
    ref.setflags(write=False)
    return levels, coords, names, ref


def _dm_store(dm, N, dev, seed=0):
    """the edges stored in another order in N + 1 slots (one hole, filled with a non-zero pattern)"""
    perm = torch.randperm(N + 1, generator=torch.Generator().manual_seed(seed))[:N].to(dev)
    store = []
    for d in dm:
        t = torch.full((N + 1, d.shape[1]), 3.0, dtype=torch.float16, device=dev)
        t[perm] = d
        store.append(t)
    return store, perm.int()


@pytest.mark.parametrize("h,w", R.SIZES_ALL)
def test_dm_fused_lookup_bit_exact(gpu, monkeypatch, h, w):
    """corr_dm_encode_kernel<CORR = true> (the form the update step launches) == oracle.corr.corr_lookup_pyramid bit for bit:
    windows off every side of the map, huge coordinates, a map-wide displacement that wraps the cyclic shift both ways at
    every level, random coordinates with a margin of half a map; volumes with -0.0 and subnormal planes and isolated
    +-65504; planar and interleaved coordinates, implicit slots and a permuted slot list with a hole, one launch and runs of
    3 edges.  The encoder-only launch writes the same encoder output as the launch that also writes the lookup."""
    from glorie_slam_amd import droid_backends as db, update_ops as U
    levels, coords, names, ref = _dm_scene(h, w)
    N = len(names)
    vols = [torch.from_numpy(v).to(gpu) for v in levels]
    dm = [db.dm_corr_level(v, l) for l, v in enumerate(vols)]
    store, slots = _dm_store(dm, N, gpu)
    planar = torch.from_numpy(coords).to(gpu)
    xy = planar.permute(0, 2, 3, 1).contiguous()
    wgt, bias = _random_encoder(3, gpu)
    ew = U.pack_corr_encoder_dm(wgt)
    _same_bits(db.cl_to_planar(db.corr_dm_lookup(dm, planar, h, w)).cpu().numpy(), ref, f"plain lookup {h}x{w}", names)
    first = None
    for chunk in (None, "3"):
        if chunk is None:
            monkeypatch.delenv("GLORIE_CORR_DM_CHUNK", raising=False)
        else:
            monkeypatch.setenv("GLORIE_CORR_DM_CHUNK", chunk)
        for interleaved in (False, True):
            for lv, sl in ((dm, None), (store, slots)):
                what = f"{h}x{w} chunk={chunk} interleaved={interleaved} slots={'list' if sl is not None else 'none'}"
                ct = xy if interleaved else planar
                wide = _poisoned(N, 320, h, w, gpu)
                poison = wide.clone()
                cl = db.corr_dm_lookup(lv, ct, h, w, slots=sl, interleaved=interleaved, enc_w=ew, enc_b=bias,
                                       enc_out=wide[:, 128:256])
                v = cl.view(N, 4, 8, 8, h, w)
                assert not bool(v[:, :, 7].view(torch.int16).any()) and not bool(v[:, :, :, 7].view(torch.int16).any()), what
                _same_bits(db.cl_to_planar(cl).cpu().numpy(), ref, f"fused lookup {what}", names)
                assert torch.equal(wide[:, :128], poison[:, :128]) and torch.equal(wide[:, 256:], poison[:, 256:]), what
                enc = wide[:, 128:256].contiguous(memory_format=torch.channels_last)
                only = _poisoned(N, 128, h, w, gpu)
                assert db.corr_dm_lookup(lv, ct, h, w, slots=sl, interleaved=interleaved, want_corr=False, enc_w=ew,
                                         enc_b=bias, enc_out=only) is None
                assert torch.equal(only.view(torch.int16), enc.view(torch.int16)), f"encoder-only launch {what}"
                if first is None:
                    first = enc.clone()
                    assert float(first.float().abs().max()) > 0
                assert torch.equal(enc.view(torch.int16), first.view(torch.int16)), f"encoder output {what}"
    assert not _bits(db.cl_to_planar(cl).cpu().numpy()[names.index("huge")]).any()


@pytest.mark.parametrize("h,w", [(16, 24), (13, 22)])
def test_dm_fused_encoder_bit_exact(gpu, h, w):
    """the MFMA epilogue of corr_dm_encode_kernel on the encoder-exact scene (integer volumes, quarter coordinates, integer
    weights): == the float64 reference rounded once to fp16, bit for bit, with and without the lookup written"""
    from glorie_slam_amd import droid_backends as db, update_ops as U
    N = 3
    levels, coords = R.dm_integer_scene(5, N, h, w)
    ref_corr = ocorr.corr_lookup_pyramid(levels, coords, 3)
    wgt, bias = R.integer_encoder(1, -4, 4)
    ref_enc, _, _ = R.encoder_reference(ref_corr, wgt.reshape(128, 196), bias)        # proves the bound for THIS scene
    dm = [db.dm_corr_level(torch.from_numpy(v).to(gpu), l) for l, v in enumerate(levels)]
    ew, eb = U.pack_corr_encoder_dm(torch.from_numpy(wgt).to(gpu)), torch.from_numpy(bias).to(gpu)
    planar = torch.from_numpy(coords).to(gpu)
    for interleaved in (False, True):
        ct = planar.permute(0, 2, 3, 1).contiguous() if interleaved else planar
        wide = _poisoned(N, 320, h, w, gpu)
        poison = wide.clone()
        cl = db.corr_dm_lookup(dm, ct, h, w, interleaved=interleaved, enc_w=ew, enc_b=eb, enc_out=wide[:, 128:256])
        _same_bits(db.cl_to_planar(cl).cpu().numpy(), ref_corr, f"lookup {h}x{w}")
        _same_bits(wide[:, 128:256].cpu().numpy(), ref_enc, f"fused encoder {h}x{w} interleaved={interleaved}")
        assert torch.equal(wide[:, :128], poison[:, :128]) and torch.equal(wide[:, 256:], poison[:, 256:])
        only = _poisoned(N, 128, h, w, gpu)
        db.corr_dm_lookup(dm, ct, h, w, interleaved=interleaved, want_corr=False, enc_w=ew, enc_b=eb, enc_out=only)
        _same_bits(only.cpu().numpy(), ref_enc, f"encoder-only launch {h}x{w} interleaved={interleaved}")


# ---- builder -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("h,w,layout", [(h, w, "dm") for h, w in [(16, 24)] + R.SIZES_RAGGED_LEVELS + R.SIZES_RAGGED] +
                         [(h, w, "tiled") for h, w in [(16, 24)] + R.SIZES_RAGGED_LEVELS])
def test_corr_arena_build_bit_exact(gpu, h, w, layout):
    """glorie_corr_build / glorie_corr_dm_build on order-free features: level 0 == the oracle's fp16 volume and levels 1-3 ==
    the oracle's pooled pyramid, bit for bit; the slot-recycling sequence (keep, then add into the freed slots) under the
    same comparison"""
    from glorie_slam_amd.droid_net import CorrArena
    from oracle import update_step as ostep
    F_ = 5
    fm = R.order_free_features(h * 100 + w + 1, F_, h, w)
    fcl = (torch.from_numpy(fm).to(gpu) / 4.0).permute(0, 2, 3, 1).reshape(F_, h * w, 128).contiguous()
    ii = np.array([0, 1, 2, 4, 3], np.int64)
    jj = np.array([1, 0, 4, 2, 3], np.int64)
    arena = CorrArena(h, w, gpu, capacity=4, layout=layout)         # 5 edges: grows once
    assert arena.layout == layout
    arena.add(fcl, torch.from_numpy(ii[:3]).to(gpu), torch.from_numpy(jj[:3]).to(gpu))
    arena.add(fcl, torch.from_numpy(ii[3:]).to(gpu), torch.from_numpy(jj[3:]).to(gpu))
    ref = ostep.corr_pyramid_fp16(fm[ii], fm[jj])
    for l in range(4):
        _same_bits(arena.level(l).cpu().numpy(), ref[l], f"{layout} {h}x{w} level {l}")
    before = {s_: arena.views()[0].view(arena.capacity, -1)[s_].clone() for s_ in arena._host_slots}
    freed = [arena._host_slots[1], arena._host_slots[3]]
    arena.keep([True, False, True, False, True])
    arena.add(fcl, torch.tensor([3, 0], device=gpu), torch.tensor([1, 2], device=gpu))
    assert sorted(arena._host_slots[3:]) == sorted(freed)
    for s_ in arena._host_slots[:3]:
        assert torch.equal(arena.views()[0].view(arena.capacity, -1)[s_], before[s_])
    ii2, jj2 = np.array([0, 2, 3, 3, 0]), np.array([1, 4, 3, 1, 2])
    ref2 = ostep.corr_pyramid_fp16(fm[ii2], fm[jj2])
    for l in range(4):
        _same_bits(arena.level(l).cpu().numpy(), ref2[l], f"{layout} {h}x{w} level {l} after recycling")


# ---- alt-corr ----------------------------------------------------------------------------------------------------------------
def _altcorr(gpu, f1, f2, c, radius):
    from glorie_slam_amd import droid_backends as db
    out, = db.altcorr_forward(torch.from_numpy(f1).to(gpu), torch.from_numpy(f2).to(gpu), torch.from_numpy(c).to(gpu), radius)
    return out.cpu().numpy()


@pytest.mark.parametrize("case", R.ALT_CASES, ids=lambda c: f"r{c[0]}-C{c[1]}-S{c[2]}-{c[3][0]}x{c[3][1]}-{c[4][0]}x{c[4][1]}-{c[5]}")
def test_altcorr_exact_on_integer_scenes(gpu, case):
    """glorie_altcorr_fwd == the oracle's loop nest in float64, EXACTLY, where every product and sum is exact in fp32:
    altcorr_r3_kernel with full and tail channel chunks, altcorr_generic_kernel (other radii, C % 4 != 0), S = 1 and 3, fewer
    and more pixels than a workgroup, target maps down to 1 x 1, windows off the map and huge coordinates"""
    f1, f2, c = R.altcorr_case(case)
    R.altcorr_exact_bound(f1, f2, c)
    ref = R.altcorr_f64(f1, f2, c, case[0])
    got = _altcorr(gpu, f1, f2, c, case[0])
    assert got.dtype == np.float32 and got.shape == ref.shape
    ne = got.astype(np.float64) != ref
    assert not ne.any(), f"{int(ne.sum())} of {ne.size} differ, first at {np.argwhere(ne)[0]}"


ALT_GENERAL = [(3, 128, 2, (9, 13), (4, 6)), (3, 40, 1, (8, 8), (8, 8)), (2, 128, 3, (9, 13), (4, 6)), (1, 130, 1, (5, 7), (2, 3)),
               (4, 32, 2, (8, 8), (4, 4)), (3, 6, 1, (9, 13), (9, 13))]


@pytest.mark.parametrize("radius,C,S,hw,hw2", ALT_GENERAL)
def test_altcorr_general_data_within_twice_the_oracles_fp32_error(gpu, radius, C, S, hw, hw2):
    """general fp32 data: max |kernel - f64| <= 2 max |oracle_fp32 - f64| on the same inputs (the margin covers the FMA
    contraction of the kernel's `o += s * w`); the ratio is printed (profiles/corr_exact_error.txt records it)"""
    rng = np.random.default_rng(40 + C + radius)
    B, (H, W), (H2, W2) = 2, hw, hw2
    f1 = (rng.standard_normal((B, H, W, C)) * 0.25).astype(np.float32)
    f2 = (rng.standard_normal((B, H2, W2, C)) * 0.25).astype(np.float32)
    c = np.stack([rng.uniform(-3, W2 + 3, (B, S, H, W)), rng.uniform(-3, H2 + 3, (B, S, H, W))], -1).astype(np.float32)
    ref = R.altcorr_f64(f1, f2, c, radius)
    e_oracle = np.abs(ocorr.altcorr_forward(f1, f2, c, radius).astype(np.float64) - ref).max()
    e_kernel = np.abs(_altcorr(gpu, f1, f2, c, radius).astype(np.float64) - ref).max()
    print(f"altcorr general r={radius} C={C} S={S} {H}x{W} -> {H2}x{W2}: kernel {e_kernel:.3e} oracle {e_oracle:.3e} "
          f"ratio {e_kernel / e_oracle:.3f}")
    assert e_oracle > 0
    assert e_kernel <= 2.0 * e_oracle, (e_kernel, e_oracle)


@pytest.mark.parametrize("S", [None, 3])
def test_altcorr_block_exact_and_agrees_with_otf(gpu, S):
    """AltCorrBlock as a whole (pyramid, S axis, permutes) == the float64 four-level reference, exactly, on the integer
    scene; with integer coordinates (the fp16 blend of OtfCorrBlock is exact there) both blocks return the same numbers"""
    from glorie_slam_amd.droid_net import AltCorrBlock, OtfCorrBlock
    h, w = 16, 24
    it, jt = torch.from_numpy(R.OTF_II).to(gpu), torch.from_numpy(R.OTF_JJ).to(gpu)
    for integer in (False, True):
        fm, coords = R.altcorr_block_scene(11, h, w, S or 1, integer)
        ref, inputs = R.altcorr_block_f64(fm.astype(np.float32), coords, R.OTF_II, R.OTF_JJ)
        for f1, f2, c in inputs:
            R.altcorr_exact_bound(f1, f2, c)
        fmt = torch.from_numpy(fm).to(gpu)
        ct = torch.from_numpy(coords).to(gpu)[None]                   # [1, N, h, w, S, 2]
        if S is None:
            ct, ref = ct[..., 0, :].contiguous(), ref[..., 0]
        got = AltCorrBlock(fmt.float()[None])(ct, it, jt)[0].cpu().numpy()
        assert got.shape == ref.shape and got.dtype == np.float32
        assert np.array_equal(got.astype(np.float64), ref), f"S={S} integer={integer}"
        if integer and S is None:
            otf = OtfCorrBlock(fmt[None])(ct, it, jt)[0].cpu().numpy()
            assert np.array_equal(otf.astype(np.float64), ref)
