"""Reference of the update operator's kernels (csrc/gru.hip, the epilogues of csrc/conv.hip, csrc/flowenc.hip, the motion
kernels of csrc/geom.hip) in plain numpy, the scenes that make them observable and the one tolerance helper of
test_gpu_update_kernels.py (test infrastructure).

Nothing is shared with the kernels or with update_ops.py: maps are logical [N, C, h, w] arrays, weights are the unpacked
[Nout, C, k, k] tensors of the reference's droid_net.py / gru.py, so the packers of update_ops.py are under test too.  Every
function evaluates in float64 on the fp16 / fp32 values exactly as the kernel receives them.

Two kinds of scenes.
  Integer scenes (int_map / int_weight) for every linear path: activations in {-2..2} * unit, about a quarter non-zero,
  weights in {-1, 0, 1}, integer biases, and sum |x||w| <= CAP * unit over every receptive field (check_cap).  Every partial
  sum in any order is then exact in fp32 and every result exact in fp16: the kernel must give the reference's bits.  Every
  border pixel of every map carries a non-zero value and scenes have N >= 2 maps, so a read across a map edge shows.
  Non-linear paths (sigmoid, tanh blend, softplus, means) keep the linear part exact (unit = 1/8, sparse weights: arguments of
  a few units) and draw the non-linear operands at random: gate terms with saturating rows (+-20, +-90), arguments next to 0,
  z at exactly 0 and 1.  Their bounds come from tol(): per element and derived, never tuned.
      length-n fp32 sum                 n * 2^-24 * sum |summands|        (of the float64 reference's own summands)
      activation                        slope * (error of its argument) + MARGIN * E_ACT
      fp16 output                       + one fp16 ulp of the reference value (rounding costs half an ulp, the fp32 error
                                        decides which neighbour)
  E_ACT is the measured error of the kernels' float32 formulations evaluated in numpy float32 against float64 over the
  scenes' argument range (profiles/update_op_error.txt; `python tests/update_op_ref.py` prints it); the kernel is allowed
  MARGIN times as much, which covers the GPU's __expf / v_rcp_f32 against libm's expf and the IEEE division.

Kernels whose whole arithmetic is one IEEE chain (bias_act NONE / RELU, motion, motion_padded, flow_pad,
update_bookkeeping) have float32 / float16 numpy twins here (the *_f32 functions) and are compared for equality.
"""
import functools

import numpy as np

F, H16 = np.float32, np.float16
EPS = 2.0 ** -24
CAP = 2048
MARGIN = 4.0
ACT_NONE, ACT_RELU, ACT_SIGMOID, ACT_SOFTPLUS, ACT_TANH = 0, 1, 2, 3, 4
# measured by measure_e_act() (profiles/update_op_error.txt), rounded up in the third digit; test_update_op_ref.py holds
# the float32 formulations to them.  sigmoid, tanh: absolute; softplus: relative to max(1, |value|).
E_ACT = {ACT_SIGMOID: 8.92e-08, ACT_TANH: 1.10e-07, ACT_SOFTPLUS: 1.48e-07}
SLOPE = {ACT_NONE: 1.0, ACT_RELU: 1.0, ACT_SIGMOID: 0.25, ACT_TANH: 1.0, ACT_SOFTPLUS: 1.0}       # largest derivative
ARG_RANGE = 100.0                      # |argument| of every activation in the scenes (terms up to +-90 plus a few units)

MAPS = ((1, 1, 1), (2, 1, 2), (2, 3, 5), (3, 7, 10), (2, 9, 17), (2, 1, 127), (1, 8, 16), (3, 3, 43))
NARROW = tuple((2, h, w) for h, w in ((1, 1), (1, 7), (2, 3), (3, 2), (6, 1), (7, 6), (3, 7), (6, 6)))   # below the 7x7 halo


# ---- activations ------------------------------------------------------------------------------------------------------------
def act64(v, act):
    v = np.asarray(v, np.float64)
    if act == ACT_RELU:
        return np.maximum(v, 0.0)
    if act == ACT_SIGMOID:
        e = np.exp(-np.abs(v))
        return np.where(v >= 0, 1.0 / (1.0 + e), e / (1.0 + e))
    if act == ACT_SOFTPLUS:
        return np.logaddexp(0.0, v)
    if act == ACT_TANH:
        return np.tanh(v)
    return v


def act32(x, act):
    """the kernels' float32 formulations (gru.hip sigmoidf_, tanhf_, softplusf_) in numpy float32"""
    x = np.asarray(x, F)
    with np.errstate(over="ignore", under="ignore"):
        if act == ACT_SIGMOID:
            return (F(1) / (F(1) + np.exp(-x))).astype(F)
        if act == ACT_TANH:
            e = np.exp(F(-2) * np.abs(x))
            return np.copysign((F(1) - e) / (F(1) + e), x).astype(F)
        if act == ACT_SOFTPLUS:
            return np.where(x > F(20), x, np.log1p(np.exp(np.minimum(x, F(20))))).astype(F)
    raise ValueError(act)


def act_arguments():
    """the argument range of the scenes: a dense sweep, the neighbourhood of 0 and of the softplus switch, the saturating
    terms"""
    k = np.arange(-40, 7, dtype=np.float64)
    near0 = np.concatenate([2.0 ** k, -(2.0 ** k), [0.0]])
    sweep = np.linspace(-ARG_RANGE, ARG_RANGE, 800001)
    fine = np.linspace(-8.0, 8.0, 400001)
    edge = 20.0 + np.linspace(-1e-3, 1e-3, 2001)
    return np.concatenate([sweep, fine, near0, edge, [20.0, -20.0, 90.0, -90.0]]).astype(F)


def measure_e_act():
    x = act_arguments()
    out = {}
    for act in (ACT_SIGMOID, ACT_TANH, ACT_SOFTPLUS):
        ref = act64(x.astype(np.float64), act)
        err = np.abs(act32(x, act).astype(np.float64) - ref)
        if act == ACT_SOFTPLUS:
            err = err / np.maximum(1.0, np.abs(ref))
        out[act] = float(err.max())
    return out


# ---- the tolerance helper ---------------------------------------------------------------------------------------------------
def ulp16(v):
    a = np.maximum(np.abs(np.asarray(v, np.float64)), 2.0 ** -14)          # below: the subnormal spacing 2^-24
    return 2.0 ** (np.floor(np.log2(a)) - 10)


def tol(ref, n=0, abssum=0.0, act=None, arg_err=0.0, gain=1.0, fp16=False):
    """per-element bound of a kernel result against the float64 value `ref`:
    gain * (n * 2^-24 * abssum  +  [slope * arg_err + MARGIN * E_ACT]) + [one fp16 ulp of ref]
    n, abssum: length and sum of |summands| of the fp32 sum that forms the value (or, with `act`, pass the error of the
    activation's argument as arg_err); gain: |factor| the activation is multiplied with afterwards."""
    ref = np.asarray(ref, np.float64)
    t = n * EPS * np.asarray(abssum, np.float64) + np.zeros_like(ref)
    if act is not None:
        scale = np.maximum(1.0, np.abs(ref)) if act == ACT_SOFTPLUS else 1.0
        t = t + SLOPE[act] * np.asarray(arg_err, np.float64) + MARGIN * E_ACT.get(act, 0.0) * scale
    t = t * np.abs(gain)
    if fp16:
        t = t + ulp16(ref)
    return t


# ---- scenes -----------------------------------------------------------------------------------------------------------------
def border_mask(h, w):
    m = np.zeros((h, w), bool)
    m[0], m[-1], m[:, 0], m[:, -1] = True, True, True, True
    return m


def int_map(rng, n, c, h, w, unit=1.0, density=0.25):
    """[n, c, h, w] float64 holding {-2..2} * unit, `density` non-zero, every border pixel with at least one non-zero"""
    v = rng.integers(1, 3, (n, c, h, w)) * rng.choice([-1, 1], (n, c, h, w)) * (rng.random((n, c, h, w)) < density)
    ys, xs = np.nonzero(border_mask(h, w))
    for m in range(n):
        ch = rng.integers(0, c, len(ys))
        v[m, ch, ys, xs] = rng.choice([-2, -1, 1, 2], len(ys))
    return v.astype(np.float64) * unit


def int_weight(rng, nout, c, k, density=2.0 / 3.0):
    return (rng.choice([-1, 1], (nout, c, k, k)) * (rng.random((nout, c, k, k)) < density)).astype(np.float64)


def int_bias(rng, n, unit=1.0, span=3):
    return rng.integers(-span, span + 1, n).astype(np.float64) * unit


def check_cap(x, w, unit=1.0, bias=None):
    """the condition of the integer scenes, asserted on the reference alone: sum |x||w| (+ |bias|) <= CAP * unit over every
    output's receptive field; returns the largest sum in units"""
    # in units the summands are non-negative integers and c * k * k * 2 < 2^24: float32 sums them exactly, at half the cost
    xu = np.abs(np.asarray(x, np.float64)) / unit
    assert np.array_equal(xu, np.rint(xu)) and x.shape[1] * w.shape[2] * w.shape[3] * 2 < 2 ** 24
    s = conv2d(xu, np.abs(w), np.float32).astype(np.float64)
    if bias is not None:
        s = s + np.abs(bias).reshape(1, -1, 1, 1) / unit
    worst = float(s.max())
    assert worst <= CAP, f"integer scene exceeds the exactness cap: {worst} > {CAP}"
    return worst


def gate_terms(rng, n, m):
    """float32 [n, m] gate terms: N(0, 1), some next to 0, saturating entries in every row and one saturating row"""
    t = rng.standard_normal((n, m)).astype(F)
    t[:, 0::16] = F(2.0 ** -12) * t[:, 0::16]
    t[:, 1::32], t[:, 2::32], t[:, 3::32], t[:, 4::32] = F(20), F(-20), F(90), F(-90)
    if n > 1:
        t[n - 1, 5::2] = F(90) * np.sign(t[n - 1, 5::2])
    return t


def unit_interval16(rng, shape):
    """fp16 values of z: uniform in [0, 1] with exact zeros and ones"""
    z = rng.random(shape).astype(H16)
    z.reshape(-1)[0::7], z.reshape(-1)[3::11] = H16(0), H16(1)
    return z


# ---- float64 reference ------------------------------------------------------------------------------------------------------
def conv2d(x, w, dtype=np.float64):
    """zero-padded k x k correlation, x [N,C,h,w], w [O,C,k,k] -> [N,O,h,w] in float64 (dtype: see check_cap)"""
    x, w = np.asarray(x, dtype), np.asarray(w, dtype)
    n, c, h, wd = x.shape
    o, c2, k, _ = w.shape
    assert c == c2
    r = k // 2
    xp = np.zeros((n, c, h + 2 * r, wd + 2 * r), dtype)
    xp[:, :, r:r + h, r:r + wd] = x
    out = np.zeros((n, o, h, wd), dtype)
    for ky in range(k):
        for kx in range(k):
            out += np.einsum("oc,nchw->nohw", w[:, :, ky, kx], xp[:, :, ky:ky + h, kx:kx + wd], optimize=True)
    return out


def conv(xa, xb, weight, bias=None, act=ACT_NONE):
    """the convolution over the two input segments with epilogue 0 (bias + NONE / RELU) -> float64"""
    x = np.concatenate([np.asarray(t, np.float64) for t in (xa, xb) if t is not None], 1)
    v = conv2d(x, weight)
    if bias is not None:
        v = v + np.asarray(bias, np.float64).reshape(1, -1, 1, 1)
    return act64(v, act)


def bias_act(x, bias, act):
    """-> (value, bound); the bound is for ACT_SIGMOID, NONE / RELU are exact (bias_act_f32)"""
    x = np.asarray(x, np.float64)
    b = np.zeros(x.shape[1]) if bias is None else np.asarray(bias, np.float64)
    arg = x + b.reshape(1, -1, 1, 1)
    v = act64(arg, act)
    arg_err = EPS * (np.abs(x) + np.abs(b).reshape(1, -1, 1, 1))
    return v, tol(v, act=act, arg_err=arg_err, fp16=True)


def bias_act_f32(x, bias, act):
    """ACT_NONE / ACT_RELU as the kernel's IEEE chain: fp16 -> fp32, one add, max, round to fp16"""
    f = np.asarray(x, H16).astype(F)
    if bias is not None:
        f = f + np.asarray(bias, F).reshape(1, -1, 1, 1)
    if act == ACT_RELU:
        f = np.maximum(f, F(0))
    return f.astype(H16)


def _arg(acc, terms, pre, pre_map, roundings):
    """acc [N,C,h,w] + pre[pre_map] + terms[n] -> (argument, its fp32 error)"""
    acc = np.asarray(acc, np.float64)
    t = np.asarray(terms, np.float64)[:, :, None, None]
    mag = np.abs(acc) + np.abs(t)
    arg = acc + t
    if pre is not None:
        p = np.asarray(pre, np.float64)
        if pre_map is not None:
            p = p[np.asarray(pre_map)]
        arg, mag = arg + p, mag + np.abs(p)
    return arg, roundings * EPS * mag


def gate_zr(acc, terms, net, pre=None, pre_map=None):
    """z = sigmoid(acc[:, :128] + ...), rnet = sigmoid(acc[:, 128:] + ...) * net (gru.py:28-30); acc: the stored fp16 map of
    the stand-alone kernel or the convolution's (exact) accumulators -> (z, bound, rnet, bound)"""
    arg, err = _arg(acc, terms, pre, pre_map, 1 if pre is None else 2)
    s = act64(arg, ACT_SIGMOID)
    net = np.asarray(net, np.float64)
    z, r = s[:, :128], s[:, 128:] * net
    zt = tol(z, act=ACT_SIGMOID, arg_err=err[:, :128], fp16=True)
    rt = tol(s[:, 128:], act=ACT_SIGMOID, arg_err=err[:, 128:], gain=net) + EPS * np.abs(r) + ulp16(r)
    return z, zt, r, rt


def gate_q(acc, terms, z, net, pre=None, pre_map=None):
    """(1 - z) * net + z * tanh(acc + ...)   (gru.py:31-33) -> (value, bound)"""
    arg, err = _arg(acc, terms, pre, pre_map, 1 if pre is None else 2)
    q = act64(arg, ACT_TANH)
    z, net = np.asarray(z, np.float64), np.asarray(net, np.float64)
    a, b = (1.0 - z) * net, z * q
    v = a + b
    t = tol(q, act=ACT_TANH, arg_err=err, gain=z) + 3 * EPS * (np.abs(a) + np.abs(b)) + ulp16(v)
    return v, t


def glo_terms(arg, arg_err, net, G, Gb):
    """glo[n][c] = mean_p sigmoid(arg) * net; g = Gb + glo @ G (gru.py:25-31) -> (g [N,M], bound)"""
    net = np.asarray(net, np.float64)
    n, c, h, w = net.shape
    hw = h * w
    s = act64(arg, ACT_SIGMOID)
    prod = s * net
    glo = prod.reshape(n, c, hw).sum(2) / hw
    each = tol(s, act=ACT_SIGMOID, arg_err=arg_err, gain=net) + EPS * np.abs(prod)
    glo_err = (each.reshape(n, c, hw).sum(2) + (hw + 1) * EPS * np.abs(prod).reshape(n, c, hw).sum(2)) / hw
    G, Gb = np.asarray(G, np.float64), np.asarray(Gb, np.float64)
    g = glo @ G + Gb
    t = glo_err @ np.abs(G) + tol(g, n=129, abssum=np.abs(glo) @ np.abs(G) + np.abs(Gb))
    return g, t


def segment_mean(x, ix, groups, bias=None, relu=False):
    """out[g] = mean over e with ix[e] == g of act(x[e] + bias), zeros for an empty group (droid_net.py:53-59)"""
    x = np.asarray(x, np.float64)
    f = x if bias is None else x + np.asarray(bias, np.float64).reshape(1, -1, 1, 1)
    if relu:
        f = np.maximum(f, 0.0)
    ix = np.asarray(ix)
    v = np.zeros((groups,) + x.shape[1:])
    t = np.zeros_like(v)
    for g in range(groups):
        m = ix == g
        cnt = int(m.sum())
        if cnt:
            v[g] = f[m].sum(0) / cnt
            # cnt additions of summands that are one rounded add each, the reciprocal and the product with it
            t[g] = (cnt + 3) * EPS * np.abs(f[m]).sum(0) / cnt
    return v, t + ulp16(v)


def stencil(conv_out, abs_out, out_bias, acts, scale, K):
    """second half of the heads: conv_out [groups][N, K, h, w] (exact) + bias -> activation -> * scale; abs_out: the sums of
    the nine |taps| (or a bound on them) -> (value [groups, N, h, w, K], bound)"""
    vals, tols = [], []
    for g, (c, a, act) in enumerate(zip(conv_out, abs_out, acts)):
        b = np.zeros(K) if out_bias is None else np.asarray(out_bias, np.float64)[g * K:(g + 1) * K]
        arg = c + b.reshape(1, -1, 1, 1)
        v = act64(arg, act) * scale
        # bias + nine taps summed in fp32 (exact while everything is a multiple of the unit), then the product with scale
        err = 9 * EPS * (a + np.abs(b).reshape(1, -1, 1, 1))
        t = tol(v / scale, act=act, arg_err=err, gain=scale) + EPS * np.abs(v)
        vals.append(v.transpose(0, 2, 3, 1))
        tols.append(t.transpose(0, 2, 3, 1))
    return np.stack(vals), np.stack(tols)


def taps_to_conv(rows, n, h, w, groups, K):
    """tap planes [groups*9K, n*h*w] (row g*9K + d*K + j = tap d = 3 ky + kx of output j of head g at every pixel) -> the
    zero-padded 9-point sums [groups][n, K, h, w]: output pixel (y, x) takes tap d from pixel (y + ky - 1, x + kx - 1)"""
    rows = np.asarray(rows, np.float64).reshape(groups, 9, K, n, h, w)
    outs = []
    for g in range(groups):
        pad = np.zeros((9, K, n, h + 2, w + 2))
        pad[..., 1:1 + h, 1:1 + w] = rows[g]
        o = sum(pad[3 * ky + kx, :, :, ky:ky + h, kx:kx + w] for ky in range(3) for kx in range(3))
        outs.append(o.transpose(1, 0, 2, 3))
    return outs


def small_heads(x, ws, out_bias, acts, scale=1.0, in_bias=None, in_relu=False):
    """conv3x3_small: group g reads channels 128 g .. 128 g + 127 of x; the operand act_in(x + in_bias) is rounded to fp16
    (exact in the integer scenes) -> (value [groups, N, h, w, K], bound, per-group operands)"""
    x = np.asarray(x, np.float64)
    outs, ops, mags = [], [], []
    for g, wgt in enumerate(ws):
        xin = x[:, 128 * g:128 * (g + 1)]
        if in_bias is not None:
            xin = xin + np.asarray(in_bias, np.float64)[128 * g:128 * (g + 1)].reshape(1, -1, 1, 1)
        if in_relu:
            xin = np.maximum(xin, 0.0)
        assert np.array_equal(xin.astype(H16).astype(np.float64), xin)
        ops.append(xin)
        outs.append(conv2d(xin, wgt))
        mags.append(conv2d(np.abs(xin), np.abs(wgt)))                      # >= the sum of the nine |taps|
    v, t = stencil(outs, mags, out_bias, acts, scale, ws[0].shape[0])
    return v, t, ops


def heads(x, w1, b1, w2s, b2, acts, scale=1.0):
    """hidden = relu(conv3x3(x, w1) + b1) rounded to fp16; head g = 3x3 conv of hidden[:, 128 g : 128 g + 128] with w2s[g]
    -> K taps and stencil, activation, scale; the channels past 128 * groups are the stored `rest`
    -> (value [groups, N, h, w, K], bound, hidden float64)"""
    hidden = conv(x, None, w1, b1, ACT_RELU)
    assert np.array_equal(hidden.astype(H16).astype(np.float64), hidden)      # exact in fp16 (integer scenes)
    outs = [conv2d(hidden[:, 128 * g:128 * (g + 1)], w2) for g, w2 in enumerate(w2s)]
    mags = [conv2d(hidden[:, 128 * g:128 * (g + 1)], np.abs(w2)) for g, w2 in enumerate(w2s)]
    v, t = stencil(outs, mags, b2, acts, scale, w2s[0].shape[0])
    return v, t, hidden


def flow_conv7(flow, weight, bias):
    """relu(conv7x7(fp16(flow)) + bias): flow [N,h,w,4] float32 (droid_net.py:79-81) -> float64 [N,128,h,w]"""
    x = np.asarray(flow, F).astype(H16).astype(np.float64).transpose(0, 3, 1, 2)
    return act64(conv2d(x, weight) + np.asarray(bias, np.float64).reshape(1, -1, 1, 1), ACT_RELU)


def motion_f32(coords1, coords0, target, limit):
    """clamp([coords1 - coords0, target - coords1], +-limit) as the kernel's IEEE chain -> float32 [N,h,w,4]"""
    c1, c0, t = np.asarray(coords1, F), np.asarray(coords0, F), np.asarray(target, F)
    lim = F(limit)
    m = np.concatenate([c1 - c0[None], t - c1], -1).astype(F)
    return np.minimum(np.maximum(m, -lim), lim)


def flow_pad_f32(flow):
    """[N,h,w,4] float32 -> the zero-padded fp16 map [N,h+6,w+8,4], interior at row 3, pixel 3"""
    n, h, w, _ = flow.shape
    p = np.zeros((n, h + 6, w + 8, 4), H16)
    p[:, 3:3 + h, 3:3 + w] = np.asarray(flow, F).astype(H16)
    return p


def bookkeeping_f32(coords1, delta, eta, frames, table, ep, age):
    """factor_graph.py:219-223,248,256: target = coords1 + delta; table[frames] = eta; damping_ba = 0.2 * eta + ep (each
    operation rounded on its own); age += 1 -> (target, table, damping_ba, age)"""
    target = (np.asarray(coords1, F) + np.asarray(delta, F)).astype(F)
    table = np.array(table, F)
    eta = np.asarray(eta, F)
    if len(frames):
        table[np.asarray(frames)] = eta
    ba = ((eta * F(0.2)).astype(F) + F(ep)).astype(F)
    return target, table, ba, None if age is None else np.asarray(age, np.int64) + 1


# ---- the scenes of test_gpu_update_kernels.py (built once, shared, read-only) ------------------------------------------------
CONV_CHANNELS = ((128, 320), (0, 128), (128, 0), (64, 64), (128, 192))
CONV_NOUT = (64, 128, 256, 384, 576)
POLICY_MAP = (3, 7, 10)
GATE_MAPS = ((2, 1, 2), (3, 7, 10), (2, 9, 17), (3, 3, 43))
GATE_UNIT, GATE_DENSITY = 0.125, 1.0 / 16.0          # arguments of a few units in front of the non-linearities
SMALL_MAPS = MAPS + NARROW
# 33,280 pixels = 260 tiles of 128: with 512 output channels the "split" policy has one whole round of 768 tile slots and a
# remainder launch, and the ping-pong policies a partial last round of smaller tiles on a 256-CU device
BIG_MAP, BIG_LAYER = (2, 128, 130), (64, 512)


def _freeze(d):
    for v in d.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return d


@functools.lru_cache(maxsize=None)
def conv_scene(n, h, w, c, nout, k, unit=1.0, wdensity=2.0 / 3.0):
    """integer scene of a k x k layer c -> nout on n maps of h x w: x, w, bias, acc = conv2d(x, w) (exact), worst = the
    largest sum |x||w| + |bias| in units (asserted <= CAP)"""
    rng = np.random.default_rng([n, h, w, c, nout, k, int(1 / unit), int(1 / wdensity)])
    x, wt, bias = int_map(rng, n, c, h, w, unit), int_weight(rng, nout, c, k, wdensity), int_bias(rng, nout, unit)
    return _freeze(dict(x=x, w=wt, bias=bias, unit=unit, worst=check_cap(x, wt, unit, bias), acc=conv2d(x, wt)))


@functools.lru_cache(maxsize=None)
def small_scene(n, h, w, K, groups, unit=1.0, wdensity=2.0 / 3.0):
    """integer scene of conv3x3_small: x with 64 channels beyond 128 * groups, one [K,128,3,3] weight per group, input bias"""
    rng = np.random.default_rng([n, h, w, K, groups, int(1 / unit), int(1 / wdensity)])
    x = int_map(rng, n, 128 * groups + 64, h, w, unit)
    ws = tuple(int_weight(rng, K, 128, 3, wdensity) for _ in range(groups))
    in_bias = int_bias(rng, 128 * groups, unit, span=1)
    worst = 0.0
    for g, wt in enumerate(ws):
        xin = np.abs(x[:, 128 * g:128 * g + 128]) + np.abs(in_bias[128 * g:128 * g + 128]).reshape(1, -1, 1, 1)
        worst = max(worst, check_cap(xin, wt, unit, np.full(K, 3 * unit)))
    return _freeze(dict(x=x, ws=ws, in_bias=in_bias, out_bias=int_bias(rng, K * groups, unit), unit=unit, worst=worst))


@functools.lru_cache(maxsize=None)
def flow_scene(n, h, w):
    """integer motion map [n,h,w,4] float32 in {-2..2}, flow_encoder[0] weight [128,4,7,7] in {-1,0,1}, integer bias"""
    rng = np.random.default_rng([7, n, h, w])
    x = int_map(rng, n, 4, h, w, density=0.5)
    wt, bias = int_weight(rng, 128, 4, 7), int_bias(rng, 128)
    worst = check_cap(x, wt, 1.0, bias)
    return _freeze(dict(flow=np.ascontiguousarray(x.transpose(0, 2, 3, 1)).astype(F), x=x, w=wt, bias=bias, worst=worst))


def integer_scenes():
    """(name, scene) of every integer scene the GPU tests run"""
    n, h, w = POLICY_MAP
    for k in (1, 3):
        for c in sorted({a + b for a, b in CONV_CHANNELS}):
            yield f"conv {c}->576 k{k}", conv_scene(n, h, w, c, 576, k)
    for k in (1, 3):
        yield f"conv 64->512 k{k} whole rounds", conv_scene(*BIG_MAP, *BIG_LAYER, k)
    for n, h, w in MAPS:
        yield f"conv 320->128 k3 {n}x{h}x{w}", conv_scene(n, h, w, 320, 128, 3)
        yield f"conv 128->64 k1 {n}x{h}x{w}", conv_scene(n, h, w, 128, 64, 1)
        yield f"heads 128->384 {n}x{h}x{w}", conv_scene(n, h, w, 128, 384, 3)
        yield f"glo 128->128 {n}x{h}x{w}", conv_scene(n, h, w, 128, 128, 1, GATE_UNIT, GATE_DENSITY)
    for n, h, w in GATE_MAPS:
        yield f"gate 320->256 {n}x{h}x{w}", conv_scene(n, h, w, 320, 256, 3, GATE_UNIT, GATE_DENSITY)
        yield f"gate 320->128 {n}x{h}x{w}", conv_scene(n, h, w, 320, 128, 3, GATE_UNIT, GATE_DENSITY)
    for n, h, w in MAPS + NARROW:
        yield f"flow {n}x{h}x{w}", flow_scene(n, h, w)
    for n, h, w in SMALL_MAPS:
        for K in (1, 2, 3):
            for groups in (1, 2, 4):
                yield f"small K{K} g{groups} {n}x{h}x{w}", small_scene(n, h, w, K, groups)
        yield f"small act {n}x{h}x{w}", small_scene(n, h, w, 2, 4, GATE_UNIT, GATE_DENSITY)


if __name__ == "__main__":
    names = {ACT_SIGMOID: "sigmoid 1/(1+exp(-x))", ACT_TANH: "tanh (1-e)/(1+e), e = exp(-2|x|)",
             ACT_SOFTPLUS: "softplus x > 20 ? x : log1p(exp(x))"}
    print("# float32 formulations of csrc/gru.hip in numpy float32 against float64, %d arguments in [-%g, %g]"
          % (len(act_arguments()), ARG_RANGE, ARG_RANGE))
    print("# command: python tests/update_op_ref.py     (numpy %s, x86-64, AVX-512 / AVX2 float32 loops)" % np.__version__)
    print("# another numpy build may round exp / log1p the other way: tests/test_update_op_ref.py holds these records with 2^-23 of room")
    for a, e in measure_e_act().items():
        kind = "relative to max(1, |value|)" if a == ACT_SOFTPLUS else "absolute"
        print("%-40s max error %.4e  (%s)   recorded E_ACT %.3e, kernels allowed x %g" % (names[a], e, kind, E_ACT[a], MARGIN))
