"""The update operator's kernels (csrc/gru.hip, the epilogues of csrc/conv.hip, csrc/flowenc.hip, the motion kernels of
csrc/geom.hip) one by one against the numpy reference of tests/update_op_ref.py.

Linear paths run integer scenes and must give the reference's bits; kernels that are one IEEE chain must equal their numpy
float32 twin; the non-linear paths are held to update_op_ref.tol(), a per-element bound derived from the float64
reference's own summands, one fp16 ulp and four times the measured error of the float32 formulations.  Every operand is
a channel slice of a wider buffer with its own row stride, every output buffer is filled with a sentinel first.
test_update_op_ref.py holds the reference and the scenes' preconditions on the CPU."""
import ctypes

import numpy as np
import pytest
import torch

import update_op_ref as R

pytestmark = pytest.mark.gpu

SENT = -1234.0                                   # exact in fp16 and fp32, outside every scene's range of results


# ---- plumbing ---------------------------------------------------------------------------------------------------------------
def wide_map(dev, n, c, h, w, total=None, off=0, data=None):
    """fp16 channels-last map [n, c, h, w] = channels off .. off + c of a [n, h, w, total] buffer that holds SENT
    -> (view, buffer); data (exactly representable in fp16) is copied into the view"""
    total = total or c
    buf = torch.full((n, h, w, total), SENT, dtype=torch.float16, device=dev)
    view = buf.permute(0, 3, 1, 2)[:, off:off + c]
    if data is not None:
        d16 = np.asarray(data).astype(np.float16)
        assert np.array_equal(d16.astype(np.float64), np.asarray(data, np.float64)), "scene value is not an fp16 number"
        view.copy_(torch.from_numpy(np.ascontiguousarray(d16)).to(dev))
    return view, buf


def dv(a, dev, dtype=np.float32):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a).astype(dtype))).to(dev)


def host(t):
    return t.detach().float().cpu().numpy().astype(np.float64) if t.dtype != torch.float32 \
        else t.detach().cpu().numpy().astype(np.float64)


def untouched(buf, off, c):
    """the channels of the wide buffer outside [off, off + c) still hold the sentinel"""
    b = buf.float()
    return bool((b[..., :off] == SENT).all()) and bool((b[..., off + c:] == SENT).all())


def same(name, got, ref):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    assert got.shape == ref.shape, (name, got.shape, ref.shape)
    bad = got != ref
    if bad.any():
        i = tuple(int(v) for v in np.argwhere(bad)[0])
        raise AssertionError(f"{name}: {int(bad.sum())} of {bad.size} values differ, first at {i}: got {got[i]!r}, "
                             f"reference {ref[i]!r}; largest difference {np.abs(got - ref).max()!r}")


def close(name, got, ref, bound):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    bound = np.broadcast_to(np.asarray(bound, np.float64), ref.shape)
    assert got.shape == ref.shape, (name, got.shape, ref.shape)
    err = np.abs(got - ref)
    ratio = err / np.maximum(bound, 1e-300)
    print(f"{name}: max |error| {err.max():.3e}, max error / bound {ratio.max():.3f}")
    bad = ~(err <= bound)
    if bad.any():
        i = tuple(int(v) for v in np.unravel_index(np.argmax(np.where(bad, ratio, 0)), ref.shape))
        raise AssertionError(f"{name}: {int(bad.sum())} of {bad.size} values beyond the bound, worst at {i}: got {got[i]!r}, "
                             f"reference {ref[i]!r}, bound {bound[i]:.3e}")


def h16(rng, shape, scale=1.0):
    """random fp16 values as float64, with exact zeros and a few large entries"""
    v = (scale * rng.standard_normal(shape)).astype(np.float16)
    f = v.reshape(-1)
    f[0::17], f[5::29], f[6::31] = np.float16(0), np.float16(20), np.float16(-20)
    return v.astype(np.float64)


def terms_table(rng, n, dev):
    """float32 [n, 392]: columns 4 .. 388 are the z | r | q gate terms, a column slice with distinct rows per edge"""
    t = np.full((n, 392), SENT, np.float32)
    t[:, 4:388] = R.gate_terms(rng, n, 384)
    return t, dv(t, dev)


# ---- bias_act ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", [8, 24, 64, 128, 256, 384, 448])
def test_bias_act(gpu, C):
    """the <8>, <16>, <48> and generic instantiations, every act, with and without bias, out of place between slices of
    two buffers with different row strides and in place; NONE / RELU equal numpy float32, the channels around the slices
    keep the sentinel"""
    from glorie_slam_amd import update_ops as U
    for n, h, w in ((1, 1, 1), (2, 3, 5), (2, 1, 127)):
        rng = np.random.default_rng([C, n, h, w])
        x = h16(rng, (n, C, h, w), 2.0)
        bias = R.gate_terms(rng, 1, C)[0]
        for act in (U.ACT_NONE, U.ACT_RELU, U.ACT_SIGMOID):
            for b in (bias, None):
                name = f"bias_act C={C} {n}x{h}x{w} act={act} bias={b is not None}"
                bt = dv(b, gpu) if b is not None else None
                ref, bound = R.bias_act(x, b, act)
                xin, xbuf = wide_map(gpu, n, C, h, w, C + 24, 8, x)
                out, obuf = wide_map(gpu, n, C, h, w, C + 40, 16)
                U.bias_act(xin, bt, act, out=out)
                for tag, res in (("", out), (" in place", U.bias_act(xin, bt, act))):
                    if act == U.ACT_SIGMOID:
                        close(name + tag, host(res), ref, bound)
                    else:
                        same(name + tag, host(res), R.bias_act_f32(x, b, act).astype(np.float64))
                assert untouched(obuf, 16, C) and untouched(xbuf, 8, C), name


# ---- global-context terms ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M", [1, 100, 128, 384])
@pytest.mark.parametrize("parts", [1, 5, 16, 300])
def test_gru_glo_terms(gpu, parts, M):
    """the two-launch form on a stored map: every split of the pixels (300 parts > HW: empty slices), every width of the
    [128 x M] product, operands as slices, and the same bits on a repeat call"""
    from glorie_slam_amd import update_ops as U
    for n, h, w in ((1, 1, 1), (2, 3, 5), (3, 7, 10)):
        rng = np.random.default_rng([parts, M, n, h, w])
        wn, net = h16(rng, (n, 128, h, w), 2.0), np.tanh(h16(rng, (n, 128, h, w))).astype(np.float16).astype(np.float64)
        bw = R.gate_terms(rng, 1, 128)[0]
        G, Gb = (rng.standard_normal((128, M)) / 11).astype(np.float32), rng.standard_normal(M).astype(np.float32)
        wn_t, _ = wide_map(gpu, n, 128, h, w, 192, 64, wn)
        net_t, _ = wide_map(gpu, n, 128, h, w, 136, 8, net)
        args = (wn_t, dv(bw, gpu), net_t, dv(G, gpu), dv(Gb, gpu))
        g = U.gru_glo_terms(*args, parts=parts)
        arg = wn + bw.astype(np.float64).reshape(1, -1, 1, 1)
        ref, bound = R.glo_terms(arg, R.EPS * (np.abs(wn) + np.abs(bw).reshape(1, -1, 1, 1)), net, G, Gb)
        close(f"glo_terms parts={parts} M={M} {n}x{h}x{w}", host(g), ref, bound)
        assert torch.equal(g, U.gru_glo_terms(*args, parts=parts))


@pytest.mark.parametrize("n,h,w", R.MAPS)
def test_gru_glo_terms_fused(gpu, n, h, w):
    """the 1x1 convolution with the reduction as its epilogue + glorie_gru_glo_from_tiles against float64: the linear part
    is an exact scene, so the bound is the sigmoid's and the sums' alone; maps of one pixel, of 127, 128, 129 and 153 pixels
    (one and two tiles per map)"""
    from glorie_slam_amd import update_ops as U
    sc = R.conv_scene(n, h, w, 128, 128, 1, R.GATE_UNIT, R.GATE_DENSITY)
    rng = np.random.default_rng([3, n, h, w])
    bw = R.gate_terms(rng, 1, 128)[0]
    net_t, _ = wide_map(gpu, n, 128, h, w, 192, 32, sc["x"])
    wp = U.pack_conv_igemm(dv(sc["w"], gpu))
    arg = sc["acc"] + bw.astype(np.float64).reshape(1, -1, 1, 1)
    arg_err = R.EPS * (np.abs(sc["acc"]) + np.abs(bw).reshape(1, -1, 1, 1))
    for M in (100, 384):
        G, Gb = (rng.standard_normal((128, M)) / 11).astype(np.float32), rng.standard_normal(M).astype(np.float32)
        g = U.gru_glo_terms_fused(net_t, wp, dv(bw, gpu), dv(G, gpu), dv(Gb, gpu))
        ref, bound = R.glo_terms(arg, arg_err, sc["x"], G, Gb)
        close(f"glo_terms_fused M={M} {n}x{h}x{w}", host(g), ref, bound)
        assert torch.equal(g, U.gru_glo_terms_fused(net_t, wp, dv(bw, gpu), dv(G, gpu), dv(Gb, gpu)))


# ---- stand-alone gate kernels -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,h,w", [(3, 1, 1), (2, 1, 2), (2, 3, 5), (3, 7, 10)])
def test_gru_gate_kernels(gpu, n, h, w):
    """gru_gate_zr / gru_gate_q with a row stride of its own on every operand, the terms as column slices of one [N, 392]
    table with distinct rows per edge, out2 present and absent, maps of one pixel"""
    from glorie_slam_amd import update_ops as U
    rng = np.random.default_rng([4, n, h, w])
    zr, qc = h16(rng, (n, 256, h, w), 2.0), h16(rng, (n, 128, h, w), 2.0)
    net = np.tanh(h16(rng, (n, 128, h, w))).astype(np.float16).astype(np.float64)
    z0 = R.unit_interval16(rng, (n, 128, h, w)).astype(np.float64)
    tab, tab_t = terms_table(rng, n, gpu)
    zr_t, _ = wide_map(gpu, n, 256, h, w, 320, 32, zr)
    qc_t, _ = wide_map(gpu, n, 128, h, w, 144, 16, qc)
    net_t, _ = wide_map(gpu, n, 128, h, w, 448, 0, net)
    z0_t, _ = wide_map(gpu, n, 128, h, w, 136, 8, z0)
    z_t, zbuf = wide_map(gpu, n, 128, h, w, 160, 24)
    r_t, rbuf = wide_map(gpu, n, 128, h, w, 448, 128)
    U.gru_gate_zr(zr_t, tab_t[:, 4:260], net_t, z_t, r_t)
    z, zb, r, rb = R.gate_zr(zr, tab[:, 4:260], net)
    close(f"gate_zr z {n}x{h}x{w}", host(z_t), z, zb)
    close(f"gate_zr rnet {n}x{h}x{w}", host(r_t), r, rb)
    assert untouched(zbuf, 24, 128) and untouched(rbuf, 128, 128)
    ref, bound = R.gate_q(qc, tab[:, 260:388], z0, net)
    for with_out2 in (True, False):
        o_t, obuf = wide_map(gpu, n, 128, h, w, 200, 40)
        o2_t, o2buf = wide_map(gpu, n, 128, h, w, 448, 64)
        U.gru_gate_q(qc_t, tab_t[:, 260:388], z0_t, net_t, o_t, out2=o2_t if with_out2 else None)
        close(f"gate_q {n}x{h}x{w} out2={with_out2}", host(o_t), ref, bound)
        assert untouched(obuf, 40, 128) and untouched(o2buf, 64, 128)
        if with_out2:
            assert torch.equal(o2_t, o_t)
        else:
            assert bool((o2buf == SENT).all())
    assert bool((host(tab_t)[:, :4] == SENT).all())


# ---- segment mean -----------------------------------------------------------------------------------------------------------
def _segment_patterns(N, rng):
    """edge -> group tables over 5 groups; group 1 is always empty"""
    base = rng.choice([0, 3, 4], N)
    pats = {"random": base.copy()}
    if N > 256:
        second = base.copy()
        second[second == 3] = 0
        second[256:min(N, 512):7] = 2                       # group 2 lives in the second batch of 256 edges only
        pats["second batch only"] = second
    if N >= 256:
        full = base.copy()
        full[full == 3] = 4
        full[N - 256 - (N - 256) % 256:][:256] = 3          # all 256 edges of one batch in one group
        pats["a whole batch"] = full
    return pats


@pytest.mark.parametrize("h,w", [(1, 1), (3, 5), (1, 17)])
@pytest.mark.parametrize("N", [1, 7, 255, 256, 257, 600])
def test_segment_mean(gpu, N, h, w):
    """the ballot compaction over batches of 256 edges: edge counts around the batch size, empty groups, a group whose edges
    all lie in the second batch, a batch that belongs to one group entirely; x a slice, bias + ReLU on and off"""
    from glorie_slam_amd import update_ops as U
    rng = np.random.default_rng([5, N, h, w])
    x = h16(rng, (N, 128, h, w))
    x_t, _ = wide_map(gpu, N, 128, h, w, 192, 64, x)
    bias = rng.standard_normal(128).astype(np.float32)
    for pname, ix in _segment_patterns(N, rng).items():
        for b, relu in ((None, False), (bias, True)):
            out = U.segment_mean(x_t, dv(ix, gpu, np.int64), 5, bias=dv(b, gpu) if b is not None else None, relu=relu)
            ref, bound = R.segment_mean(x, ix, 5, b, relu)
            close(f"segment_mean N={N} {h}x{w} {pname} relu={relu}", host(out), ref, bound)
            assert float(out[1].abs().max()) == 0.0                      # the empty group
            counts = np.bincount(ix, minlength=5)
            assert counts[1] == 0 and (pname != "a whole batch" or counts[3] == 256)


# ---- conv3x3_small / conv_stencil -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("groups", [1, 2, 4])
@pytest.mark.parametrize("K", [1, 2, 3])
def test_conv3x3_small_integer_scenes(gpu, K, groups):
    """both tap-GEMM instantiations (9K <= 16 and > 16) and the row-major stencil bit for bit, on ragged maps and maps
    narrower than the stencil, x with channels beyond 128 * groups, with and without the input transform"""
    from glorie_slam_amd import update_ops as U
    acts = [U.ACT_NONE, U.ACT_RELU, U.ACT_RELU, U.ACT_NONE][:groups]
    for n, h, w in R.SMALL_MAPS:
        sc = R.small_scene(n, h, w, K, groups)
        x_t, _ = wide_map(gpu, n, 128 * groups + 64, h, w, 128 * groups + 96, 0, sc["x"])
        wp = U.pack_conv3x3_small([dv(wt, gpu) for wt in sc["ws"]])
        for transform in (False, True):
            ib = sc["in_bias"] if transform else None
            ref, _, _ = R.small_heads(sc["x"], sc["ws"], sc["out_bias"], acts, 0.5, ib, transform)
            out = U.conv3x3_small(x_t, wp, dv(sc["out_bias"], gpu), K, acts, scale=0.5,
                                  in_bias=dv(ib, gpu) if transform else None, in_relu=transform)
            same(f"conv3x3_small K={K} groups={groups} {n}x{h}x{w} transform={transform}", host(out), ref)


@pytest.mark.parametrize("n,h,w", R.SMALL_MAPS)
def test_conv3x3_small_activations(gpu, n, h, w):
    """sigmoid / softplus / ReLU / none of four heads on an exact linear part, fractional and saturating output biases,
    a scale that is no power of two"""
    from glorie_slam_amd import update_ops as U
    sc = R.small_scene(n, h, w, 2, 4, R.GATE_UNIT, R.GATE_DENSITY)
    rng = np.random.default_rng([6, n, h, w])
    ob = rng.standard_normal(8).astype(np.float32)
    ob[1], ob[2], ob[4], ob[5] = 20.0, -90.0, -20.0, 90.0
    acts = [U.ACT_NONE, U.ACT_SIGMOID, U.ACT_SOFTPLUS, U.ACT_RELU]
    x_t, _ = wide_map(gpu, n, 576, h, w, 584, 8, sc["x"])
    out = U.conv3x3_small(x_t, U.pack_conv3x3_small([dv(wt, gpu) for wt in sc["ws"]]), dv(ob, gpu), 2, acts, scale=0.01,
                          in_bias=dv(sc["in_bias"], gpu), in_relu=True)
    ref, bound, _ = R.small_heads(sc["x"], sc["ws"], ob, acts, np.float64(np.float32(0.01)), sc["in_bias"], True)
    for g in range(4):
        close(f"conv3x3_small act={acts[g]} {n}x{h}x{w}", host(out[g]), ref[g], bound[g])


@pytest.mark.parametrize("K", [1, 2, 3])
@pytest.mark.parametrize("n,h,w", R.SMALL_MAPS)
def test_conv_stencil_on_tap_planes(gpu, n, h, w, K):
    """the planar stencil on given tap planes: exact for none / ReLU, the derived bound for sigmoid / softplus; out_last
    takes the last group and leaves the rest of the result as it is"""
    from glorie_slam_amd import update_ops as U
    rng = np.random.default_rng([7, n, h, w, K])
    groups, P = 4, n * h * w
    rows = rng.integers(-8, 9, (groups * 9 * K, P)).astype(np.float64) * R.GATE_UNIT
    ob = rng.standard_normal(groups * K).astype(np.float32)
    ob[0], ob[-1] = 20.0, -90.0
    conv_out, abs_out = R.taps_to_conv(rows, n, h, w, groups, K), R.taps_to_conv(np.abs(rows), n, h, w, groups, K)
    rows_t = dv(rows, gpu)
    acts = [U.ACT_RELU, U.ACT_SIGMOID, U.ACT_NONE, U.ACT_SOFTPLUS]
    ref, bound = R.stencil(conv_out, abs_out, ob, acts, np.float64(np.float32(0.01)), K)
    out = U.conv_stencil(rows_t, dv(ob, gpu), n, h, w, groups, K, acts, scale=0.01)
    last = torch.full((P, K), SENT, device=gpu)
    out2 = U.conv_stencil(rows_t, dv(ob, gpu), n, h, w, groups, K, acts, scale=0.01, out_last=last)
    for g in range(groups):
        close(f"conv_stencil act={acts[g]} K={K} {n}x{h}x{w}", host(out[g]), ref[g], bound[g])
    assert torch.equal(out2[:3], out[:3]) and torch.equal(last.view(n, h, w, K), out[3])
    # integer biases, scale 1/2: every partial sum is exact
    ib = R.int_bias(rng, groups * K, R.GATE_UNIT)
    ref, _ = R.stencil(conv_out, abs_out, ib, [U.ACT_NONE, U.ACT_RELU] * 2, 0.5, K)
    same(f"conv_stencil exact K={K} {n}x{h}x{w}",
         host(U.conv_stencil(rows_t, dv(ib, gpu), n, h, w, groups, K, [U.ACT_NONE, U.ACT_RELU] * 2, scale=0.5)), ref)


# ---- implicit-GEMM convolution ----------------------------------------------------------------------------------------------
def _conv_inputs(dev, x, ca, cb):
    """segment A as a whole buffer with padding channels, segment B as a slice 64 channels into a wider one"""
    n, _, h, w = x.shape
    xa = wide_map(dev, n, ca, h, w, ca + 8, 0, x[:, :ca])[0] if ca else None
    xb = wide_map(dev, n, cb, h, w, cb + 64, 64, x[:, ca:])[0] if cb else None
    return xa, xb


def _must_refuse(policy, nout, epilogue):
    """the fit rules of csrc/conv.hip: the 256-channel ping-pong tile takes nout % 256 == 0 with the bias or the z|r
    epilogue, the 128-channel one nout % 128 == 0 with the bias or the q epilogue; every other policy takes every layer"""
    from glorie_slam_amd import update_ops as U
    if policy == "pp":
        return nout % 256 != 0 or epilogue not in (U.EPI_BIAS_ACT, U.EPI_GRU_ZR)
    if policy == "ppw":
        return nout % 128 != 0 or epilogue not in (U.EPI_BIAS_ACT, U.EPI_GRU_Q)
    return False


def _run_linear(dev, name, sc, ca, cb, nout, taps, policies, relu_only=False):
    """every policy x row pairing x (no bias, bias, bias + ReLU) of one layer: the reference's bits, or a refusal that
    leaves the output alone - and exactly the refusals of _must_refuse"""
    from glorie_slam_amd import update_ops as U
    n, _, h, w = sc["x"].shape
    xa, xb = _conv_inputs(dev, sc["x"], ca, cb)
    wt, bias, acc = dv(sc["w"][:nout], dev), sc["bias"][:nout], sc["acc"][:, :nout]
    packs = {pair: U.pack_conv_igemm(wt, pair=pair) for pair in (False, True)}
    bias_t = dv(bias, dev)
    with_bias = acc + bias.reshape(1, -1, 1, 1)
    cases = ((None, U.ACT_NONE, acc), (bias_t, U.ACT_NONE, with_bias), (bias_t, U.ACT_RELU, np.maximum(with_bias, 0.0)))
    cases = cases[2:] if relu_only else cases
    refused = set()
    for policy in policies:
        for pair in (False, True):
            for terms, act, ref in cases:
                out, obuf = wide_map(dev, n, nout, h, w, nout + 8, 0)
                try:
                    U.conv_igemm(xa, xb, packs[pair], taps, nout, out, terms=terms, act=act, policy=policy)
                except RuntimeError:
                    refused.add((policy, pair))
                    torch.cuda.synchronize()
                    assert bool((obuf == SENT).all()), f"{name}: refused policy {policy} pair={pair} wrote to the output"
                    continue
                same(f"{name} policy={policy} pair={pair} act={act} bias={terms is not None}", host(out), ref)
                assert untouched(obuf, 0, nout)
    expected = {(p, pair) for p in policies for pair in (False, True) if _must_refuse(p, nout, U.EPI_BIAS_ACT)}
    assert refused == expected, (name, sorted(refused, key=str), sorted(expected, key=str))


@pytest.mark.parametrize("nout", R.CONV_NOUT)
@pytest.mark.parametrize("ca,cb", R.CONV_CHANNELS)
@pytest.mark.parametrize("taps", [1, 9])
def test_conv_igemm_integer_scenes(gpu, taps, ca, cb, nout):
    """1x1 and 3x3 layers over one and two input segments (the second a slice), 64 .. 576 output channels, under every tile
    policy and both row packings: the int-exact reference's bits.  A policy that does not fit the layer must raise - those
    of _must_refuse and no other - and never return other values.  (On this map "split" has no whole round and "pp" /
    "ppw" one round of full-size tiles: test_conv_igemm_whole_rounds.)"""
    from glorie_slam_amd import update_ops as U
    n, h, w = R.POLICY_MAP
    sc = R.conv_scene(n, h, w, ca + cb, 576, 3 if taps == 9 else 1)
    _run_linear(gpu, f"conv_igemm {ca}+{cb}->{nout} taps={taps}", sc, ca, cb, nout, taps, list(U.CONV_POLICY))


@pytest.mark.parametrize("taps", [1, 9])
def test_conv_igemm_whole_rounds(gpu, taps):
    """64 -> 512 channels on 33,280 pixels, the smallest shape at which the launch logic of three policies leaves its
    single-launch form: "split" runs one whole round of 128-pixel tiles and a second launch of 64-pixel tiles that starts
    at a pixel offset; "pp" and "ppw" end in a partial round of smaller tiles.  The reference's bits under every policy."""
    from glorie_slam_amd import update_ops as U
    n, h, w = R.BIG_MAP
    c, nout = R.BIG_LAYER
    P, cus = n * h * w, torch.cuda.get_device_properties(gpu).multi_processor_count
    tiles128, ntn = (P + 127) // 128, nout // 128
    whole = tiles128 * ntn // 768 * 768 // ntn                                   # pixel tiles of the whole rounds of "split"
    assert tiles128 * ntn >= 768 and 0 < whole * 128 < P
    for px, tn in ((256, nout // 256), (512, nout // 128)):                      # pp, ppw: full tiles, then a smaller tile
        full = (P + px - 1) // px * tn // cus * cus // tn
        full -= full % 8
        rest = P - full * px
        assert full > 0 and rest > 0 and (rest * tn + cus - 1) // cus <= 3 * (px // 4), (px, full, rest)
    sc = R.conv_scene(n, h, w, c, nout, 3 if taps == 9 else 1)
    _run_linear(gpu, f"conv_igemm {c}->{nout} taps={taps} {n}x{h}x{w}", sc, c, 0, nout, taps, list(U.CONV_POLICY), relu_only=True)


@pytest.mark.parametrize("n,h,w", R.MAPS)
def test_conv_igemm_map_sizes(gpu, n, h, w):
    """a 3x3 two-segment 128-channel layer and a 1x1 64-channel layer on maps of one pixel, one row, ragged and exact
    128-pixel tiles, under every policy"""
    from glorie_slam_amd import update_ops as U
    _run_linear(gpu, f"conv_igemm 128+192->128 3x3 {n}x{h}x{w}", R.conv_scene(n, h, w, 320, 128, 3), 128, 192, 128, 9,
                list(U.CONV_POLICY))
    _run_linear(gpu, f"conv_igemm 64+64->64 1x1 {n}x{h}x{w}", R.conv_scene(n, h, w, 128, 64, 1), 64, 64, 64, 1,
                list(U.CONV_POLICY))


@pytest.mark.parametrize("n,h,w", R.GATE_MAPS)
def test_conv_igemm_gate_epilogues(gpu, n, h, w):
    """EPI_GRU_ZR and EPI_GRU_Q on an exact linear part: without a context term, with one map of it per edge, and through a
    pre_map with repeated and out-of-order entries into a larger table; terms as column slices with distinct rows, every
    operand with its own stride; under the policies that take a gate epilogue and both row packings"""
    from glorie_slam_amd import update_ops as U
    rng = np.random.default_rng([8, n, h, w])
    szr, sq = (R.conv_scene(n, h, w, 320, m, 3, R.GATE_UNIT, R.GATE_DENSITY) for m in (256, 128))
    net = np.tanh(h16(rng, (n, 128, h, w))).astype(np.float16).astype(np.float64)
    z0 = R.unit_interval16(rng, (n, 128, h, w)).astype(np.float64)
    table = h16(rng, (n + 2, 384, h, w))
    pmap = np.array([n + 1, 0, n + 1, 2][:n], np.int32)
    tab, tab_t = terms_table(rng, n, gpu)
    net_t, _ = wide_map(gpu, n, 128, h, w, 136, 8, net)
    z0_t, _ = wide_map(gpu, n, 128, h, w, 160, 32, z0)
    table_t, _ = wide_map(gpu, n + 2, 384, h, w, 400, 16, table)
    pres = {"none": (None, None, None), "per edge": (table[:n], None, table_t[:n]), "mapped": (table, pmap, table_t)}
    policies = [None, "128", "64", "split", "wide", "nohalo", "pp", "ppw"]
    for kind, sc, nout in (("zr", szr, 256), ("q", sq, 128)):
        xa, xb = _conv_inputs(gpu, sc["x"], 128, 192)
        packs = {pair: U.pack_conv_igemm(dv(sc["w"], gpu), pair=pair) for pair in (False, True)}
        lo, epi = (0, U.EPI_GRU_ZR) if kind == "zr" else (256, U.EPI_GRU_Q)
        terms, terms_t = tab[:, 4 + lo:4 + lo + nout], tab_t[:, 4 + lo:4 + lo + nout]
        for pname, (pre, pre_map, pre_t) in pres.items():
            pre_c = None if pre is None else pre[:, lo:lo + nout]
            pre_ct = None if pre_t is None else pre_t[:, lo:lo + nout]
            pm_t = None if pre_map is None else dv(pre_map, gpu, np.int32)
            if kind == "zr":
                z, zb, r, rb = R.gate_zr(sc["acc"], terms, net, pre_c, pre_map)
            else:
                q, qb = R.gate_q(sc["acc"], terms, z0, net, pre_c, pre_map)
            for policy in policies:
                for pair in (False, True):
                    name = f"conv_igemm {kind} {n}x{h}x{w} pre={pname} policy={policy} pair={pair}"
                    o_t, obuf = wide_map(gpu, n, 128, h, w, 144, 8)
                    o2_t, o2buf = wide_map(gpu, n, 128, h, w, 448, 128)
                    try:
                        if kind == "zr":
                            U.conv_igemm(xa, xb, packs[pair], 9, 256, o_t, epilogue=U.EPI_GRU_ZR, terms=terms_t, net=net_t,
                                         out2=o2_t, pre=pre_ct, pre_map=pm_t, policy=policy)
                        else:
                            U.conv_igemm(xa, xb, packs[pair], 9, 128, o_t, epilogue=U.EPI_GRU_Q, terms=terms_t, net=net_t,
                                         z=z0_t, pre=pre_ct, pre_map=pm_t, policy=policy)
                    except RuntimeError:
                        torch.cuda.synchronize()
                        assert _must_refuse(policy, nout, epi) and bool((obuf == SENT).all()) and bool((o2buf == SENT).all()), name
                        continue
                    assert not _must_refuse(policy, nout, epi), name
                    if kind == "zr":
                        close(name + " z", host(o_t), z, zb)
                        close(name + " rnet", host(o2_t), r, rb)
                        assert untouched(o2buf, 128, 128), name
                    else:
                        close(name, host(o_t), q, qb)
                        assert bool((o2buf == SENT).all()), name
                    assert untouched(obuf, 8, 128), name


# ---- heads ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,h,w", R.MAPS)
def test_conv_igemm_heads_and_stencil(gpu, n, h, w, monkeypatch):
    """hidden 3x3 convolution + ReLU (rounded to fp16) -> tap GEMM in the epilogue -> planar stencil, bit for bit on an
    integer scene: K = 1 .. 3, with and without the trailing stored channels, out_last, and GLORIE_CONV_PPW unset / 0 / 1"""
    from glorie_slam_amd import update_ops as U
    sc = R.conv_scene(n, h, w, 128, 384, 3)
    rng = np.random.default_rng([9, n, h, w])
    x_t, _ = wide_map(gpu, n, 128, h, w, 192, 64, sc["x"])
    b2 = R.int_bias(rng, 6)
    acts = (U.ACT_NONE, U.ACT_RELU)
    for K in (1, 2, 3):
        w2 = [R.int_weight(rng, K, 128, 3) for _ in range(2)]
        tap_w = U.pack_head_taps([dv(t, gpu) for t in w2])
        for nout in (384, 256):
            ref, _, hidden = R.heads(sc["x"], sc["w"][:nout], sc["bias"][:nout], w2, b2[:2 * K], acts, 0.5)
            wp = U.pack_conv_igemm(dv(sc["w"][:nout], gpu))
            for env in ((None, "0", "1") if K == 2 else (None,)):
                name = f"heads {n}x{h}x{w} K={K} nout={nout} PPW={env}"
                if env is None:
                    monkeypatch.delenv("GLORIE_CONV_PPW", raising=False)
                else:
                    monkeypatch.setenv("GLORIE_CONV_PPW", env)
                rest, rbuf = wide_map(gpu, n, 128, h, w, 160, 24)
                rows = U.conv_igemm_heads(x_t, wp, 9, nout, dv(sc["bias"][:nout], gpu), tap_w, K,
                                          out=rest if nout == 384 else None)
                monkeypatch.delenv("GLORIE_CONV_PPW", raising=False)
                last = torch.full((n * h * w, K), SENT, device=gpu)
                out = U.conv_stencil(rows, dv(b2[:2 * K], gpu), n, h, w, 2, K, acts, scale=0.5)
                out2 = U.conv_stencil(rows, dv(b2[:2 * K], gpu), n, h, w, 2, K, acts, scale=0.5, out_last=last)
                same(name, host(out), ref)
                same(name + " out_last", host(last).reshape(n, h, w, K), ref[1])
                assert torch.equal(out2[0], out[0])
                if nout == 384:
                    same(name + " stored channels", host(rest), hidden[:, 256:])
                    assert untouched(rbuf, 24, 128), name
                else:
                    assert bool((rbuf == SENT).all()), name


# ---- flow encoder -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,h,w", R.MAPS + R.NARROW)
def test_flow_conv7_integer_scenes(gpu, n, h, w):
    """the 7x7 layer on the fp32 map and on the zero-padded fp16 map, bit for bit, on maps narrower than the halo and ragged
    16-pixel tiles; output into a slice; the padded buffer equals the numpy twin before and after (borders still zero)"""
    from glorie_slam_amd import update_ops as U
    sc = R.flow_scene(n, h, w)
    ref = R.flow_conv7(sc["flow"], sc["w"], sc["bias"])
    flow_t, wp, bias_t = dv(sc["flow"], gpu), U.pack_flow_conv7(dv(sc["w"], gpu)), dv(sc["bias"], gpu)
    out, obuf = wide_map(gpu, n, 128, h, w, 192, 64)
    U.flow_conv7(flow_t, wp, bias_t, out)
    same(f"flow_conv7 {n}x{h}x{w}", host(out), ref)
    assert untouched(obuf, 64, 128)
    pf = U.flow_pad(flow_t, U.PaddedFlow(n, h, w, gpu))
    padded = R.flow_pad_f32(sc["flow"]).astype(np.float64)
    same(f"flow_pad {n}x{h}x{w}", host(pf.buf), padded)
    out, obuf = wide_map(gpu, n, 128, h, w, 200, 72)
    U.flow_conv7_padded(pf, wp, bias_t, out)
    same(f"flow_conv7_padded {n}x{h}x{w}", host(out), ref)
    assert untouched(obuf, 72, 128)
    same(f"padded map after the convolution {n}x{h}x{w}", host(pf.buf), padded)
    # the rounding of flow_pad on values that are not fp16 numbers
    rnd = (8.0 * np.random.default_rng([10, n, h, w]).standard_normal((n, h, w, 4))).astype(np.float32)
    same(f"flow_pad rounding {n}x{h}x{w}", host(U.flow_pad(dv(rnd, gpu), U.PaddedFlow(n, h, w, gpu)).buf),
         R.flow_pad_f32(rnd).astype(np.float64))


# ---- motion features --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,h,w", [(3, 1, 1), (3, 3, 5), (4, 7, 10)])
def test_motion_kernels(gpu, n, h, w):
    """differences below, at and above +-limit in all four channels, coords0 broadcast over n >= 3 maps: glorie_motion equals
    the numpy float32 chain, glorie_motion_padded its fp16 rounding inside zero borders"""
    from glorie_slam_amd import droid_backends as db, update_ops as U
    rng = np.random.default_rng([11, n, h, w])
    lim = 64.0
    steps = np.array([0.0, 63.5, 64.0, 64.0 + 2.0 ** -10, 64.0 - 2.0 ** -10, 65.0, 200.0])
    pick = lambda shape: rng.choice(steps, shape) * rng.choice([-1.0, 1.0], shape)
    ys, xs = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    c0 = np.stack([xs, ys], -1).astype(np.float32)                      # integers: c0 + step is exact
    c1 = (c0[None] + pick((n, h, w, 2))).astype(np.float32)
    tg = (c1 + pick((n, h, w, 2))).astype(np.float32)
    c1[n - 1] = (c0 + 40 * rng.standard_normal((h, w, 2))).astype(np.float32)      # and one map of general values
    tg[n - 1] = (c1[n - 1] + 40 * rng.standard_normal((h, w, 2))).astype(np.float32)
    raw = np.concatenate([c1 - c0[None], tg - c1], -1)
    if h * w > 1:
        assert (np.abs(raw) == lim).any() and (np.abs(raw) > lim).any() and ((np.abs(raw) < lim) & (np.abs(raw) > 63)).any()
    ref = R.motion_f32(c1, c0, tg, lim)
    got = db.motion(dv(c1, gpu), dv(c0, gpu), dv(tg, gpu), limit=lim)
    same(f"motion {n}x{h}x{w}", host(got), ref.astype(np.float64))
    pm = db.motion_padded(dv(c1, gpu), dv(c0, gpu), dv(tg, gpu), U.PaddedFlow(n, h, w, gpu), limit=lim)
    same(f"motion_padded {n}x{h}x{w}", host(pm.buf), R.flow_pad_f32(ref).astype(np.float64))


# ---- bookkeeping ------------------------------------------------------------------------------------------------------------
BOOKKEEPING = [   # G, HW, n_target, n_edges, age
    dict(G=3, HW=12, nt=200, ne=5, age=True),        # n_target above G * HW
    dict(G=3, HW=12, nt=20, ne=5, age=True),         # below
    dict(G=3, HW=12, nt=20, ne=5, age=False),        # no ages
    dict(G=3, HW=1, nt=7, ne=2, age=True),           # maps of one pixel
    dict(G=0, HW=12, nt=30, ne=4, age=True),         # no frames
    dict(G=2, HW=300, nt=1000, ne=3, age=True),      # several blocks
    dict(G=1, HW=4, nt=6, ne=700, age=True),         # more edges than either other job: every age is incremented
    dict(G=0, HW=12, nt=0, ne=300, age=True),        # ages alone
]


@pytest.mark.parametrize("case", BOOKKEEPING, ids=lambda c: "G{G}_HW{HW}_nt{nt}_ne{ne}_age{age}".format(**c))
def test_update_bookkeeping(gpu, case):
    """glorie_update_bookkeeping through the C ABI: frames unsorted and not contiguous, the rows of the damping table that
    they do not name keep a sentinel, ages present and absent, and the contract of include/glorie_hip.h that the launch
    covers the longest of its three jobs - all n_edges ages are incremented whatever n_target and G * HW are"""
    from glorie_slam_amd import _lib as L
    G, HW, nt, ne = case["G"], case["HW"], case["nt"], case["ne"]
    rng = np.random.default_rng([12, G, HW, nt, ne])
    B = 7
    frames = np.array([5, 1, 3][:G], np.int64)
    c1, dl = (40 * rng.standard_normal(nt)).astype(np.float32), rng.standard_normal(nt).astype(np.float32)
    eta = rng.random((G, HW)).astype(np.float32)
    table = np.full((B, HW), SENT, np.float32)
    age = rng.integers(0, 50, ne) if case["age"] else None
    ep = 1e-7
    c1_t, dl_t, eta_t, fr_t, table_t = dv(c1, gpu), dv(dl, gpu), dv(eta, gpu), dv(frames, gpu, np.int64), dv(table, gpu)
    target_t = torch.full((nt + 3,), SENT, device=gpu)
    ba_t = torch.full((G * HW + 3,), SENT, device=gpu)
    age_t = dv(np.concatenate([age, [-9, -9]]), gpu, np.int64) if age is not None else None
    opt = lambda t, cnt: L.ptr(t if cnt else None)
    L.check(L.load().glorie_update_bookkeeping(opt(c1_t, nt), opt(dl_t, nt), opt(target_t, nt), nt, opt(eta_t, G), opt(fr_t, G),
                                               L.ptr(table_t), opt(ba_t, G), G, HW, ctypes.c_float(ep), L.ptr(age_t), ne,
                                               L.stream_ptr()), "glorie_update_bookkeeping")
    torch.cuda.synchronize()
    target, tab, ba, aged = R.bookkeeping_f32(c1, dl, eta, frames, table, ep, age)
    same("target", host(target_t[:nt]), target.astype(np.float64))
    same("damping table", host(table_t), tab.astype(np.float64))
    same("damping_ba", host(ba_t[:G * HW]), ba.reshape(-1).astype(np.float64))
    assert bool((target_t[nt:] == SENT).all()) and bool((ba_t[G * HW:] == SENT).all())
    if age is not None:
        assert np.array_equal(age_t.cpu().numpy(), np.concatenate([aged, [-9, -9]]))
