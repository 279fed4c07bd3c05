"""The one-launch flow encoder (csrc/flowenc.hip: flow_encoder_kernel, update_ops.flow_encoder) against the two launches it
replaces, bit for bit, and against a float64 evaluation of the two layers on an integer scene.

The kernel works on 8 x 16 output tiles with a 10 x 18 hidden tile; the shapes are the smallest that exercise each way that
tiling can go wrong (one exact tile, whole tiles on two maps, narrower than a tile, ragged in both directions, narrower than
the 7-wide stencil, the quarter-resolution map).  Every output is the channel slice [256:320] of a 320-channel buffer that
holds a sentinel."""
import functools

import numpy as np
import pytest
import torch

import update_op_ref as R

pytestmark = pytest.mark.gpu

SENT = -1234.0                                   # exact in fp16, outside every result's range

SHAPES = [(1, 8, 16), (2, 16, 32), (3, 9, 11), (2, 13, 21), (1, 5, 5), (2, 30, 40)]


def _slice(dev, n, h, w, total=320, off=256, c=64):
    buf = torch.full((n, h, w, total), SENT, dtype=torch.float16, device=dev)
    return buf.permute(0, 3, 1, 2)[:, off:off + c], buf


def _untouched(buf, off=256, c=64):
    return bool((buf[..., :off] == SENT).all()) and bool((buf[..., off + c:] == SENT).all())


@pytest.mark.parametrize("n,h,w", SHAPES)
def test_fused_equals_two_launches(gpu, n, h, w):
    """random motion maps, weights and biases: torch.equal to flow_conv7_padded + conv_igemm on the same packed operands,
    the other 256 channels of the buffer untouched, the padded motion map unchanged"""
    from glorie_slam_amd import update_ops as U
    g = torch.Generator(device="cpu").manual_seed(1000 * n + 10 * h + w)
    r = lambda *s: torch.randn(*s, generator=g)
    flow = torch.clamp(4.0 * r(n, h, w, 4), -64, 64).to(gpu)
    w7, b7 = U.pack_flow_conv7((r(128, 4, 7, 7) / 14).to(gpu)), r(128).to(gpu)
    w3, b3 = U.pack_conv_igemm((r(64, 128, 3, 3) / 34).to(gpu), pair=True), r(64).to(gpu)
    pf = U.flow_pad(flow, U.PaddedFlow(n, h, w, gpu))
    before = pf.buf.clone()

    f1 = torch.empty((n, 128, h, w), dtype=torch.float16, device=gpu).contiguous(memory_format=torch.channels_last)
    U.flow_conv7_padded(pf, w7, b7, f1)
    ref, rbuf = _slice(gpu, n, h, w)
    U.conv_igemm(f1, None, w3, 9, 64, ref, terms=b3, act=U.ACT_RELU)

    out, obuf = _slice(gpu, n, h, w)
    assert U.flow_encoder(pf, w7, b7, w3, b3, out) is True
    torch.cuda.synchronize()
    assert _untouched(rbuf) and _untouched(obuf)
    assert bool((ref != SENT).all()) and float(ref.float().abs().max()) > 0.0       # the reference did compute something
    diff = (out != ref)
    assert torch.equal(out, ref), f"{int(diff.sum())} of {diff.numel()} values differ, first at " \
                                  f"{tuple(int(v) for v in diff.nonzero()[0])} (map, channel, y, x)"
    assert torch.equal(pf.buf, before)


@functools.lru_cache(maxsize=None)
def _integer_scene(n, h, w):
    """the motion map and 7x7 layer of update_op_ref.flow_scene plus a sparse 3x3 layer in {-1, 0, 1} with integer bias.
    The hidden map relu(conv7 + b7) then holds integers <= 2048 (flow_scene's own cap): fp16 numbers.  Every output is an
    integer whose sum of |hidden| |w3| + |b3| stays <= 2048 (asserted here, on the reference alone), so the fp32 sums are
    exact in any order and the result is an fp16 number: the kernel must give the float64 value itself."""
    sc = R.flow_scene(n, h, w)
    hidden = R.flow_conv7(sc["flow"], sc["w"], sc["bias"])                      # float64 [n,128,h,w], exact
    assert np.array_equal(hidden, np.rint(hidden)) and hidden.max() <= R.CAP
    rng = np.random.default_rng([11, n, h, w])
    w3 = R.int_weight(rng, 64, 128, 3, density=1.0 / 16.0)
    b3 = R.int_bias(rng, 64)
    worst = R.check_cap(hidden, w3, 1.0, b3)
    out = np.maximum(R.conv2d(hidden, w3) + b3.reshape(1, -1, 1, 1), 0.0)
    assert out.max() > 0.0
    return dict(flow=sc["flow"], w7=sc["w"], b7=sc["bias"], w3=w3, b3=b3, out=out, worst=worst)


@pytest.mark.parametrize("n,h,w", [(2, 9, 11), (1, 13, 21)])
def test_fused_integer_scene_equals_float64(gpu, n, h, w):
    """relu(conv3x3_zero_padded(relu(conv7x7_zero_padded(x) + b7)) + b3) in float64 numpy on a scene where every hidden
    value and every output is an fp16 number: equality.  The scene's border pixels are non-zero and its biases are too, so
    a hidden halo pixel evaluated as relu(b7 + conv7 over the padding) instead of zero changes the border outputs."""
    from glorie_slam_amd import update_ops as U
    sc = _integer_scene(n, h, w)
    dv = lambda a: torch.from_numpy(np.array(a, np.float32)).to(gpu)      # (a copy: the scene's arrays are read-only)
    w7, b7 = U.pack_flow_conv7(dv(sc["w7"])), dv(sc["b7"])
    w3, b3 = U.pack_conv_igemm(dv(sc["w3"]), pair=True), dv(sc["b3"])
    pf = U.flow_pad(dv(sc["flow"]), U.PaddedFlow(n, h, w, gpu))
    out, obuf = _slice(gpu, n, h, w)
    U.flow_encoder(pf, w7, b7, w3, b3, out)
    got = out.float().cpu().numpy().astype(np.float64)
    bad = got != sc["out"]
    assert not bad.any(), f"{int(bad.sum())} of {bad.size} values differ, first at {tuple(int(v) for v in np.argwhere(bad)[0])}" \
                          f": largest difference {np.abs(got - sc['out']).max()}"
    assert _untouched(obuf)


def test_unsupported_row_stride_writes_nothing(gpu):
    """an output whose row stride is not a multiple of 8 halfs: GLORIE_EUNSUPPORTED as a GlorieError (strict) or False
    (strict=False), and not one element of the buffer written"""
    from glorie_slam_amd import _lib as L, update_ops as U
    n, h, w = 2, 9, 11
    g = torch.Generator(device="cpu").manual_seed(3)
    r = lambda *s: torch.randn(*s, generator=g)
    w7, b7 = U.pack_flow_conv7((r(128, 4, 7, 7) / 14).to(gpu)), r(128).to(gpu)
    w3, b3 = U.pack_conv_igemm((r(64, 128, 3, 3) / 34).to(gpu), pair=True), r(64).to(gpu)
    pf = U.flow_pad(r(n, h, w, 4).to(gpu), U.PaddedFlow(n, h, w, gpu))
    out, obuf = _slice(gpu, n, h, w, total=76, off=8)
    with pytest.raises(L.GlorieError, match="GLORIE_EUNSUPPORTED"):
        U.flow_encoder(pf, w7, b7, w3, b3, out)
    assert U.flow_encoder(pf, w7, b7, w3, b3, out, strict=False) is False
    torch.cuda.synchronize()
    assert bool((obuf == SENT).all())


def _step_inputs(dev, n, h, w, seed):
    g = torch.Generator(device=dev).manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g, device=dev)
    return (torch.tanh(r(1, n, 128, h, w)), torch.relu(r(1, n, 128, h, w)), 2.0 * r(1, n, 196, h, w),
            torch.clamp(4.0 * r(1, n, 4, h, w), -64, 64))


@pytest.mark.parametrize("n,h,w", [(3, 9, 11), (36, 60, 80)])
def test_step_equal_with_and_without_fusion(gpu, n, h, w):
    """FusedUpdate with fuse_flow on and off (one call each) on the same inputs: net, delta, weight, eta and the evaluated
    upmask are torch.equal"""
    from glorie_slam_amd.droid_net import UpdateModule, FusedUpdate
    torch.manual_seed(13)
    mod = UpdateModule().to(gpu).eval()
    net, inp, corr, flow = _step_inputs(gpu, n, h, w, seed=17)
    ii = torch.tensor([i // 5 for i in range(n)], device=gpu)
    outs = []
    for fuse in (True, False):
        f = FusedUpdate(mod)
        f.fuse_flow = fuse
        o = f(net, inp, corr, flow, ii, None)
        outs.append([t.evaluate() if hasattr(t, "evaluate") else t for t in o])
    for name, a, b in zip(("net", "delta", "weight", "eta", "upmask"), *outs):
        assert a is not None and torch.equal(a, b), name
