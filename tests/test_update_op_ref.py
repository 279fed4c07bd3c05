"""The numpy reference of tests/update_op_ref.py against torch in float64 on the CPU, and the preconditions of
test_gpu_update_kernels.py: the exactness cap of every integer scene and the recorded float32-formulation errors."""
import numpy as np
import pytest
import torch
import torch.nn.functional as TF

import update_op_ref as R

T64 = lambda a: torch.from_numpy(np.ascontiguousarray(np.asarray(a, np.float64)))
CLOSE = dict(rtol=1e-12, atol=1e-12)              # float64 against float64, sums of a few thousand O(1) terms


@pytest.mark.parametrize("k", [1, 3, 7])
def test_conv_equals_torch_conv2d(k):
    rng = np.random.default_rng(k)
    x, w = rng.standard_normal((2, 12, 5, 9)), rng.standard_normal((7, 12, k, k))
    np.testing.assert_allclose(R.conv2d(x, w), TF.conv2d(T64(x), T64(w), padding=k // 2).numpy(), **CLOSE)
    b = rng.standard_normal(7)
    got = R.conv(x[:, :4], x[:, 4:], w, b, R.ACT_RELU)
    np.testing.assert_allclose(got, TF.relu(TF.conv2d(T64(x), T64(w), T64(b), padding=k // 2)).numpy(), **CLOSE)


def test_flow_conv7_equals_torch_conv2d():
    rng = np.random.default_rng(2)
    flow = (8 * rng.standard_normal((2, 6, 9, 4))).astype(np.float32)
    w, b = rng.standard_normal((128, 4, 7, 7)), rng.standard_normal(128)
    ref = TF.relu(TF.conv2d(torch.from_numpy(flow).half().double().permute(0, 3, 1, 2), T64(w), T64(b), padding=3))
    np.testing.assert_allclose(R.flow_conv7(flow, w, b), ref.numpy(), **CLOSE)


def test_heads_equal_torch_conv2d():
    rng = np.random.default_rng(3)
    n, h, w = 2, 5, 6
    x = R.int_map(rng, n, 128, h, w)
    w1, b1 = R.int_weight(rng, 384, 128, 3), R.int_bias(rng, 384)
    w2 = [R.int_weight(rng, 2, 128, 3) for _ in range(2)]
    b2 = rng.standard_normal(4)
    acts = (R.ACT_NONE, R.ACT_SIGMOID)
    v, t, hidden = R.heads(x, w1, b1, w2, b2, acts, scale=0.5)
    hid = TF.relu(TF.conv2d(T64(x), T64(w1), T64(b1), padding=1))
    np.testing.assert_array_equal(hidden, hid.numpy())
    for g in range(2):
        o = TF.conv2d(hid[:, 128 * g:128 * g + 128], T64(w2[g]), T64(b2[2 * g:2 * g + 2]), padding=1)
        o = (torch.sigmoid(o) if g else o) * 0.5
        np.testing.assert_allclose(v[g], o.permute(0, 2, 3, 1).numpy(), **CLOSE)
    assert (t > 0).all() and t.max() < 1e-2        # 9 roundings of taps of a few thousand
    # the stencil half on tap planes: the 9-point sum of the per-tap products is the convolution
    planes = np.stack([R.conv2d(hidden[:, 128 * g:128 * g + 128], w2[g][:, :, ky:ky + 1, kx:kx + 1]).transpose(1, 0, 2, 3)
                       for g in range(2) for ky in range(3) for kx in range(3)]).reshape(2 * 9 * 2, -1)
    for g, o in enumerate(R.taps_to_conv(planes, n, h, w, 2, 2)):
        np.testing.assert_array_equal(o, R.conv2d(hidden[:, 128 * g:128 * g + 128], w2[g]))
    v2, _, ops = R.small_heads(x, w2[:1], b2[:2], [R.ACT_SOFTPLUS], in_bias=R.int_bias(rng, 128), in_relu=True)
    o = TF.softplus(TF.conv2d(T64(ops[0]), T64(w2[0]), T64(b2[:2]), padding=1), threshold=700)    # no linear shortcut above 20
    np.testing.assert_allclose(v2[0], o.permute(0, 2, 3, 1).numpy(), **CLOSE)


def test_gates_glo_and_segment_mean_equal_the_module_formulas():
    """ConvGRU.forward / GraphAgg.forward of glorie_slam_amd/droid_net.py in float64 with the gate convolutions' outputs
    given: the reference functions are the same formulas"""
    from glorie_slam_amd.droid_net import ConvGRU, segment_mean
    rng = np.random.default_rng(4)
    n, h, w = 3, 4, 5
    gru = ConvGRU(128, 320).double()
    net = torch.tanh(T64(rng.standard_normal((n, 128, h, w))))
    inp = T64(rng.standard_normal((n, 320, h, w)))
    with torch.no_grad():
        hx = torch.cat([net, inp], 1)
        wn = gru.w(net)
        glo = (torch.sigmoid(wn) * net).view(n, 128, h * w).mean(-1).view(n, 128, 1, 1)
        zc, rc = TF.conv2d(hx, gru.convz.weight, None, padding=1), TF.conv2d(hx, gru.convr.weight, None, padding=1)
        z = torch.sigmoid(gru.convz(hx) + gru.convz_glo(glo))
        r = torch.sigmoid(gru.convr(hx) + gru.convr_glo(glo))
        hq = torch.cat([r * net, inp], 1)
        qc = TF.conv2d(hq, gru.convq.weight, None, padding=1)
        new = gru(net, inp)
        # the packed form of FusedUpdate: G = [convz_glo | convr_glo | convq_glo]^T, the conv biases folded into Gb
        G = torch.cat([m.weight.view(128, 128) for m in (gru.convz_glo, gru.convr_glo, gru.convq_glo)], 0).t()
        Gb = torch.cat([a.bias + b.bias for a, b in ((gru.convz, gru.convz_glo), (gru.convr, gru.convr_glo),
                                                     (gru.convq, gru.convq_glo))])
    g, gt = R.glo_terms(wn.numpy(), 0.0, net.numpy(), G.numpy(), Gb.numpy())
    want = torch.cat([gru.convz_glo(glo) + gru.convz.bias.view(1, -1, 1, 1), gru.convr_glo(glo) + gru.convr.bias.view(1, -1, 1, 1),
                      gru.convq_glo(glo) + gru.convq.bias.view(1, -1, 1, 1)], 1).view(n, 384)
    np.testing.assert_allclose(g, want.detach().numpy(), **CLOSE)
    assert (gt > 0).all() and gt.max() < 1e-4
    zz, zt, rr, rt = R.gate_zr(torch.cat([zc, rc], 1).numpy(), g[:, :256], net.numpy())
    np.testing.assert_allclose(zz, z.numpy(), **CLOSE)
    np.testing.assert_allclose(rr, (r * net).numpy(), **CLOSE)
    out, ot = R.gate_q(qc.numpy(), g[:, 256:], zz, net.numpy())
    np.testing.assert_allclose(out, new.numpy(), **CLOSE)
    # the context term and its map table: pre[pre_map] is added before the non-linearity
    pre = rng.standard_normal((2, 128, h, w))
    a, _ = R.gate_q(qc.numpy(), g[:, 256:], zz, net.numpy(), pre=pre, pre_map=[1, 0, 1])
    b, _ = R.gate_q(qc.numpy() + pre[[1, 0, 1]], g[:, 256:], zz, net.numpy())
    np.testing.assert_allclose(a, b, **CLOSE)
    # scatter_mean of GraphAgg
    x = T64(rng.standard_normal((1, 7, 128, h, w)))
    ix = torch.tensor([0, 2, 2, 0, 3, 2, 0])
    bias = rng.standard_normal(128)
    v, t = R.segment_mean(x[0].numpy(), ix.numpy(), 4, bias=bias, relu=True)
    want = segment_mean(TF.relu(x + T64(bias).view(1, 1, -1, 1, 1)), ix, 4)[0]
    np.testing.assert_allclose(v, want.numpy(), **CLOSE)
    assert (v[1] == 0).all()


def test_exact_twins_of_the_single_chain_kernels():
    rng = np.random.default_rng(5)
    x = rng.standard_normal((2, 16, 3, 4)).astype(np.float16)
    b = rng.standard_normal(16).astype(np.float32)
    want = TF.relu(torch.from_numpy(x).float() + torch.from_numpy(b).view(1, -1, 1, 1)).half().numpy()
    np.testing.assert_array_equal(R.bias_act_f32(x, b, R.ACT_RELU), want)
    c0 = rng.standard_normal((3, 4, 2)).astype(np.float32)
    c1 = (c0 + 50 * rng.standard_normal((2, 3, 4, 2))).astype(np.float32)
    tg = (c1 + 50 * rng.standard_normal((2, 3, 4, 2))).astype(np.float32)
    want = torch.cat([torch.from_numpy(c1) - torch.from_numpy(c0), torch.from_numpy(tg) - torch.from_numpy(c1)], -1).clamp(-64, 64)
    m = R.motion_f32(c1, c0, tg, 64.0)
    np.testing.assert_array_equal(m, want.numpy())
    assert (np.abs(m) == 64).any()
    p = R.flow_pad_f32(m)
    assert p.shape == (2, 9, 12, 4) and float(np.abs(p.astype(np.float64)).sum()) == float(np.abs(m.astype(np.float16).astype(np.float64)).sum())
    eta = rng.random((2, 12)).astype(np.float32)
    tgt, table, ba, age = R.bookkeeping_f32(c1, tg, eta, [3, 1], np.full((5, 12), -7, np.float32), 1e-7, np.arange(4))
    np.testing.assert_array_equal(ba, (0.2 * torch.from_numpy(eta) + 1e-7).numpy())
    np.testing.assert_array_equal(table[[3, 1]], eta)
    assert (table[[0, 2, 4]] == -7).all() and list(age) == [1, 2, 3, 4]
    np.testing.assert_array_equal(tgt, (torch.from_numpy(c1) + torch.from_numpy(tg)).numpy())


def test_integer_scenes_hold_the_exactness_cap():
    """every integer scene test_gpu_update_kernels.py runs bit-exactly: sum |x||w| + |bias| <= 2048 units (asserted by the
    generator on the reference alone, re-checked here), the heads' hidden map times the tap weights far below 2^24, and
    non-zero values on every border pixel of every map"""
    count = 0
    for name, scene in R.integer_scenes():
        count += 1
        assert 0 < scene["worst"] <= R.CAP, name
        x = scene["x"]
        assert (np.abs(x).sum(1)[:, R.border_mask(*x.shape[2:])] > 0).all(), name
        if "w" in scene and x.size < 10 ** 6:                # (the whole-rounds scenes: the generator's own assertion)
            assert R.check_cap(x, scene["w"], scene.get("unit", 1.0), scene["bias"]) == scene["worst"], name
        if name.startswith("heads"):
            hidden = R.conv(x, None, scene["w"], scene["bias"], R.ACT_RELU)
            assert hidden.max() <= R.CAP and 9 * 128 * hidden.max() < 2.0 ** 24, name
    assert count > 100
    with pytest.raises(AssertionError):
        rng = np.random.default_rng(0)
        R.check_cap(8 * R.int_map(rng, 2, 448, 3, 3), R.int_weight(rng, 8, 448, 3))


def test_recorded_activation_errors_hold():
    got = R.measure_e_act()
    for act, e in got.items():
        # numpy dispatches its float32 exp / log1p to the SIMD code of the CPU it runs on; a build whose exp rounds the other
        # way moves a result near 1 by one float32 ulp, so the record is held with that much room: 2^-23.  The record itself
        # (numpy 2.2.6, x86-64 AVX-512 / AVX2 loops) is what the GPU bound uses.
        assert e <= R.E_ACT[act] + 2.0 ** -23, (act, e)
        assert e >= 0.5 * R.E_ACT[act], (act, e)            # the record is a measurement, not a generous guess
    # the bound helper: one fp16 ulp, subnormal spacing below 2^-14
    assert R.ulp16(1.0) == 2.0 ** -10 and R.ulp16(0.75) == 2.0 ** -11 and R.ulp16(0.0) == 2.0 ** -24 and R.ulp16(-2048.0) == 2.0
