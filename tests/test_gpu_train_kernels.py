"""The training kernels of csrc/train.hip against the float64 reference of tests/train_ref.py, at ragged sizes.

`render_train.RenderTrain` is driven with synthetic, already-placed samples (no KNN, no sampling kernel), so the number
of rays and samples and the neighbour pattern are free; `glorie_composite_bwd` and the Adam entry points are called on
their own.  Every comparison forms two errors against the float64 result - `e_hip` of the kernels and `e_f32` of the same
reference code run in float32 on the CPU - and asserts

    e_hip <= M * max(e_f32, ulp_floor),        ulp_floor = 2^-23 of the tensor's largest reference magnitude

per tensor and over ALL its elements.  Cases whose points are scene-sized (|x| up to 2: float32 Fourier phases move ReLU
pre-activations by ~2e-4 and a few units change side in float32 and in the kernels alike) use the relative Frobenius
error, with the floor scaled to it (every element off by 2^-23 of the largest one); the small cases (Q <= 257, points
within 0.05 of the origin) carry a seed for which no ReLU pre-activation of the float64 reference lies within 16 times the
float32 error of a kink - asserted, not assumed - and use the element-wise maximum error.

M = 32.  profiles/train_kernels_error_ratios.txt lists every case with its worst tensor and ratio (three runs on an
MI355X, identical to three digits).  The worst ratio that is not above 16 is 11.6 (4097x1 saturated colour, grad[20]); M is
twice that, rounded up to a power of two.  The margin is for the order of the fp32 atomics, which changes from run to run,
and for the hardware exp2 / log2 against libm.  Each test prints its ratios (`RATIO ...` lines, pytest -s).

Two ratios are above 16 and were followed up as a finding instead of being folded into M: 28.3 for grad[22], the bias of
the occupancy output, and 16.4 for grad[20], the bias of the last geometry fc_c layer, both in `13x5-saturated-color`
(e_hip 6.1e-7 against e_f32 2.2e-8 at a gradient of -0.121).  Both tensors are (a constant times) the ONE number
sum_q d loss / d occ[q]; every other tensor of every case stays below 7.2.  On the dumped kernel outputs: the compositing
backward itself is off by 1.8e-8 in that sum (float64 autograd at the kernels' own `raw`); the rest is the forward pass's
float32 error carried into the gradient, which per sample has the same spread in the kernels and in the float32 yardstick
(standard deviation 8.06e-4 against 8.20e-4 at 4097x1) - but for a single number e_f32 is one draw from that spread (0.02
standard deviations of the sum at 4097x1, 0.35 for the kernels), and the ratio of two such draws has a heavy tail.  Nothing
in csrc/train.hip was found to change for it.
"""
import ctypes
import math

import pytest
import torch

import train_ref as tr

pytestmark = pytest.mark.gpu
M = 32.0
_ULP = 2.0 ** -23


# ---------------------------------------------------------------------------------------------------------------------
# decoders
# ---------------------------------------------------------------------------------------------------------------------
_DEC = {}
_SAT_SCALE = 1.5


def _decoder(variant):
    """the 52 decoder tensors (CPU, float32): POINT under seed 43, or the same with every weight matrix scaled by 1.5 - softplus
    pre-activations then reach both saturated sides - and three units of every geometry layer dead (weights 0, bias -1)"""
    if variant not in _DEC:
        from glorie_slam_amd.decoder import POINT
        from glorie_slam_amd.render_train import decoder_tensors
        from test_golden import _decoder_cfg
        torch.manual_seed(43)
        dec = POINT(_decoder_cfg(), c_dim=32, hidden_size=128, use_view_direction=True).eval()
        ts = [t.detach().clone().float() for t in decoder_tensors(dec)]
        if variant == "saturated":
            for i, t in enumerate(ts):
                if t.dim() == 2 and i not in (tr.G_B, tr.N_B, tr.C_BP, tr.C_BV):
                    t.mul_(_SAT_SCALE)
            for i in range(5):                      # z = -1 whatever the input: the unit is dead for every sample
                ts[tr.G_W + i][:3] = 0.0
                ts[tr.G_b + i][:3] = -1.0
        _DEC[variant] = ts
    return _DEC[variant]


# ---------------------------------------------------------------------------------------------------------------------
# cases
# ---------------------------------------------------------------------------------------------------------------------
class Case:
    pass


def make_case(R, S, Np, seed, coef=None, unnormalised=False):
    """R rays x S samples on a cloud of Np points; every neighbour pattern is dealt round-robin over a random permutation of
    the samples, so each appears as soon as Q allows:
      full 8 neighbours | 2..7 valid, the rest I = -1, w = 0 | has == 0 with w and I left in place | duplicate indices
    plus (R >= 2) one ray all of whose samples have has == 0, and (Q >= 2) one zero-length view vector.  Row 0 of the cloud
    is referenced only through the clamped -1 entries.
    unnormalised (the inference tests): the same case - no draw of it changes - in which Q // 9 of the rows with has == 1 then
    get all eight weights zero and as many get their weights halved (sum 0.5); `c.wsum` names them (0: untouched, 1: zero,
    2: half) and `c.kind` the pattern each row was dealt."""
    c = Case()
    g = torch.Generator().manual_seed(seed)
    Q = R * S
    if coef is None:
        # A ray of ONE sample renders depth = z alpha / (alpha + 1e-10): at the renderer's coef = 0.1 alpha is ~0.5, the true
        # gradient is ~1e-10 and any float32 evaluation returns rounding noise in its place.  With coef = 10 the occupancies
        # of these decoders (-3 .. 2) put alpha around 1e-10 for part of the samples, and the gradient is O(1) there.
        coef = 10.0 if S == 1 else 0.1
    c.R, c.S, c.Q, c.Np, c.coef, c.small = R, S, Q, Np, coef, Q <= 257
    box = 0.1 if c.small else 4.0
    c.pts = (torch.rand(Q, 3, generator=g) - 0.5) * box
    c.views = torch.randn(Q, 3, generator=g)
    c.cloud = (torch.rand(Np, 3, generator=g) - 0.5) * box
    c.geo = torch.randn(Np, 32, generator=g) * 0.3
    c.col = torch.randn(Np, 32, generator=g) * 0.3
    I = torch.randint(1, Np, (Q, 8), generator=g)
    w = torch.rand(Q, 8, generator=g) + 0.05
    kind = torch.tensor([0, 1, 2, 3, 1, 0, 1])[torch.arange(Q) % 7][torch.randperm(Q, generator=g)]
    nvalid = torch.randint(2, 8, (Q,), generator=g)
    missing = (kind == 1)[:, None] & (torch.arange(8)[None, :] >= nvalid[:, None])
    I[missing] = -1
    w[missing] = 0.0
    dup = kind == 3
    I[dup, 1] = I[dup, 0]
    I[dup, 5] = I[dup, 2]
    I[dup, 6] = I[dup, 2]
    w = w / w.sum(1, keepdim=True)
    has = kind != 2
    if R >= 2:
        has.view(R, S)[R // 2] = False
    if Q >= 2:
        c.views[Q // 2] = 0.0
    assert int(I.min()) >= -1 and int(I.max()) < Np and not bool(((I == 0)).any())
    c.I, c.w, c.has = I, w.contiguous(), has
    c.z = torch.sort(torch.rand(R, S, generator=g) + 0.5, dim=1).values.contiguous()
    # cotangents of one sign: depth and colour are normalised weighted means, so the gradients of a ray's samples already
    # cancel within the ray; cotangents of random sign make the sums over rays cancel as well (the float64 gradient of the
    # occupancy bias at 5000 x 10 is then 1/1100 of the sum of its terms' magnitudes, and two float32 evaluations of it
    # differ by their summation order alone by more than either differs from float64)
    c.cd = torch.randn(R, generator=g).abs() + 0.5
    c.cc = torch.randn(R, 3, generator=g).abs() + 0.5
    c.kind, c.wsum = kind, torch.zeros(Q, dtype=torch.int64)
    if unnormalised:
        g2 = torch.Generator().manual_seed(seed + 7919)          # a stream of its own: the draws above stay what they were
        live = torch.nonzero(has).flatten()
        live = live[torch.randperm(live.numel(), generator=g2)]
        n = Q // 9
        c.wsum[live[:n]] = 1
        c.wsum[live[n:2 * n]] = 2
        w = c.w
        w[c.wsum == 1] = 0.0
        w[c.wsum == 2] *= 0.5
    used = torch.zeros(Np, dtype=torch.bool)
    ref = has[:, None] & (w != 0) & (I >= 0)
    used[I[ref]] = True
    c.used = used
    return c


# name: (R, S, Np, seed for the seed-43 decoders, seed for the saturated ones or None)
# The seeds of the small cases (Q <= 257) satisfy the kink condition of `_kink_margin` (searched on the CPU from seed 0 up).
CASES = {
    "1x1": (1, 1, 5, 1, None),                  # (and its one sample has alpha ~ 1e-10: see make_case on single-sample rays)
    "1x3": (1, 3, 40, 0, None),
    "3x5": (3, 5, 5, 0, 0),
    "7x9": (7, 9, 300, 0, None),
    "13x5": (13, 5, 5, 1, 0),
    "2x32": (2, 32, 400, 0, None),
    "17x10": (17, 10, 5, 2, None),
    "51x5": (51, 5, 2000, 8, None),
    "32x8": (32, 8, 5, 1, None),
    "257x1": (257, 1, 900, 13, 5),
    "33x31": (33, 31, 5, 11, 11),
    "4097x1": (4097, 1, 30000, 12, 12),
    "5000x10": (5000, 10, 20000, 13, None),
}
_BIG = ("262221x1", 262221, 1, 100000, 14)
_RUNS = [(n, v, s) for n, spec in CASES.items() for v in (("seed43", "saturated") if spec[4] is not None else ("seed43",))
         for s in ("geometry", "color")]


def _case(name, variant):
    R, S, Np, s43, ssat = CASES[name] if name != _BIG[0] else (_BIG[1], _BIG[2], _BIG[3], _BIG[4], None)
    return make_case(R, S, Np, s43 if variant == "seed43" else ssat)


def _reference(c, P, color, dtype):
    chunk = None if c.Q <= 20000 else max(1, 5000 // c.S)
    return tr.forward_backward(P, c.pts, c.views, c.cloud, c.geo, c.col, c.I, c.w, c.has, c.z, c.coef, color,
                               tr.linear_loss(c.cd, c.cc), dtype=dtype, chunk_rays=chunk)


_REF = {}


def _references(name, variant, stage):
    """(case, float64 result, float32 result), computed once per process"""
    key = (name, variant, stage)
    if key not in _REF:
        c = _case(name, variant)
        P = _decoder(variant)
        r64, r32 = _reference(c, P, stage == "color", torch.float64), _reference(c, P, stage == "color", torch.float32)
        if not c.small:
            r64.pop("pre"), r32.pop("pre")
        _REF[key] = (c, r64, r32)
    return _REF[key]


def _kink_margin(r64, r32):
    """(min |z| over every ReLU pre-activation of the float64 reference, max |z_f32 - z_f64|)"""
    return float(r64["pre"].abs().min()), float((r32["pre"].double() - r64["pre"]).abs().max())


# ---------------------------------------------------------------------------------------------------------------------
# the kernels
# ---------------------------------------------------------------------------------------------------------------------
def _run_hip(c, P, color, gpu):
    """forward + backward through the shipped glue on the CURRENT stream -> dict of device tensors"""
    from glorie_slam_amd.render_train import RenderTrain
    d = lambda t: t.to(gpu).contiguous()
    leaves = [d(t).clone().requires_grad_(True) for t in P]
    geo, col = d(c.geo).requires_grad_(True), d(c.col).requires_grad_(True)
    meta = (d(c.pts), d(c.views), d(c.cloud), d(c.I), d(c.w), d(c.has.to(torch.uint8)), d(c.z), c.coef, color)
    depth, var, rgb = RenderTrain.apply(meta, geo, col, *leaves)
    raw = depth.grad_fn.saved[4]
    loss = (d(c.cd) * depth).sum() + (d(c.cc) * rgb).sum()
    loss.backward()
    return dict(raw=raw, depth=depth.detach(), rgb=rgb.detach(), d_geo=geo.grad, d_col=col.grad,
                grads=[p.grad for p in leaves])


class Ratios:
    def __init__(self, label, frobenius, m=None):
        self.label, self.frob, self.rows, self.bad, self.m = label, frobenius, [], [], (M if m is None else float(m))

    def check(self, name, hip, r64, r32):
        """e_hip <= M max(e_f32, floor) over every element of the tensor; an identically zero reference must be met exactly"""
        hip = hip.detach().double().cpu().reshape(r64.shape)
        r32 = r32.double()
        assert bool(torch.isfinite(hip).all()), f"{self.label} {name}: not finite"
        top = float(r64.abs().max()) if r64.numel() else 0.0
        if top == 0.0:
            if r64.numel() and float(hip.abs().max()) != 0.0:
                self.bad.append(f"{name}: reference identically zero, kernel max |x| {float(hip.abs().max()):.3e}")
            return
        if self.frob:
            nrm = float(r64.norm())
            e_hip, e_f32 = float((hip - r64).norm()) / nrm, float((r32 - r64).norm()) / nrm
            floor = _ULP * top * math.sqrt(r64.numel()) / nrm
        else:
            e_hip, e_f32 = float((hip - r64).abs().max()), float((r32 - r64).abs().max())
            floor = _ULP * top
        ratio = e_hip / max(e_f32, floor)
        self.rows.append((ratio, name))
        print(f"RATIO {self.label} {name} e_hip {e_hip:.3e} e_f32 {e_f32:.3e} floor {floor:.3e} ratio {ratio:.3f}")
        if not e_hip <= self.m * max(e_f32, floor):
            self.bad.append(f"{name}: e_hip {e_hip:.3e} > {self.m} * max(e_f32 {e_f32:.3e}, floor {floor:.3e})")

    def finish(self):
        if self.rows:
            worst = max(self.rows)
            print(f"WORST {self.label} {worst[1]} {worst[0]:.3f}")
        assert not self.bad, f"{self.label}:\n  " + "\n  ".join(self.bad)


def _compare(rt, c, out, r64, r32, color):
    """everything a pass produces, against the reference"""
    has = c.has
    raw = out["raw"].detach().cpu()
    rt.check("raw.rgb", raw[:, :3], r64["raw"][:, :3], r32["raw"][:, :3])
    rt.check("raw.occ", raw[:, 3], r64["raw"][:, 3], r32["raw"][:, 3])
    # the -100 placeholders set the floor of the line above: the computed occupancies once more on their own
    assert bool((raw[~has, 3] == -100.0).all())
    if bool(has.any()):
        rt.check("raw.occ[has]", raw[has, 3], r64["raw"][has, 3], r32["raw"][has, 3])
    rt.check("depth", out["depth"], r64["depth"], r32["depth"])
    rt.check("rgb", out["rgb"], r64["rgb"], r32["rgb"])
    rt.check("d_geo_feats", out["d_geo"], r64["d_geo"], r32["d_geo"])
    d_col = out["d_col"] if out["d_col"] is not None else torch.zeros_like(c.col)
    rt.check("d_col_feats", d_col, r64["d_col"], r32["d_col"])
    # rows no valid (has, w != 0, I >= 0) entry references - row 0 among them - get exactly nothing
    assert not bool(c.used[0])
    assert bool((out["d_geo"].cpu()[~c.used] == 0.0).all()), "d_geo_feats: an unreferenced row is not exactly zero"
    assert bool((d_col.cpu()[~c.used] == 0.0).all()), "d_col_feats: an unreferenced row is not exactly zero"
    for i in range(52):
        g = out["grads"][i]
        if i in tr.FIXED:
            assert g is None, f"tensor {i}: the fixed Fourier matrices have no gradient"
            continue
        if not color and i in tr.COLOR_ONLY:
            assert g is None or float(g.abs().max()) == 0.0, f"tensor {i}: colour-only parameter touched by the geometry stage"
            continue
        assert g is not None, f"tensor {i}: no gradient"
        rt.check(f"grad[{i}]", g, r64["grads"][i], r32["grads"][i])
    if not color:
        assert float(raw[:, :3].abs().max()) == 0.0 and float(d_col.abs().max()) == 0.0


def _assert_case_is_what_it_claims(c, variant, r64, r32, name):
    kinds = int(c.has.sum()), int((~c.has).sum()), int((c.I < 0).sum())
    if c.Q >= 7:
        assert min(kinds) > 0, kinds
        assert bool((~c.has.view(c.R, c.S)).all(1).any())
    if c.small:
        zmin, dz = _kink_margin(r64, r32)
        print(f"KINK {name}/{variant} min|z| {zmin:.3e} max|z32-z64| {dz:.3e}")
        assert zmin >= 16 * dz, f"seed of {name}/{variant}: a ReLU pre-activation {zmin:.3e} from its kink, float32 moves it {dz:.3e}"
        if variant == "saturated":
            assert int((r64["pre"] < 0).all(0).sum()) >= 15          # units dead for every sample


@pytest.mark.parametrize("name,variant,stage", _RUNS, ids=[f"{n}-{v}-{s}" for n, v, s in _RUNS])
def test_training_pass_matches_float64(gpu, name, variant, stage):
    c, r64, r32 = _references(name, variant, stage)
    _assert_case_is_what_it_claims(c, variant, r64, r32, name)
    out = _run_hip(c, _decoder(variant), stage == "color", gpu)
    torch.cuda.synchronize()
    rt = Ratios(f"{name}/{variant}/{stage}", not c.small)
    _compare(rt, c, out, r64, r32, stage == "color")
    rt.finish()


def test_saturated_decoders_reach_both_sides_of_softplus():
    c = _case("33x31", "saturated")
    soft = []
    with torch.no_grad():
        tr.decode([t.double() for t in _decoder("saturated")], c.pts.double(), c.views.double(), c.cloud.double(),
                  c.geo.double(), c.col.double(), c.I, c.w.double(), c.has, True, soft=soft)
    z = torch.cat(soft, -1) * 100.0
    assert float((z > 20).float().mean()) > 0.05 and float((z < -20).float().mean()) > 0.05


def test_trunk_weight_gradients_beyond_256_rows_per_workgroup(gpu):
    """Q > 262144: wgrad() gives the trunk layers 288 rows per workgroup (geometry stage: the colour stage's workspace at this
    size is 8 times the mapper's)"""
    from glorie_slam_amd import _lib as L
    name = _BIG[0]
    need = int(L.load().glorie_render_train_workspace(_BIG[1])) + (2 << 30)
    free = torch.cuda.mem_get_info(gpu)[0]
    if free < need:
        pytest.skip(f"{free >> 20} MiB of device memory free, the case needs {need >> 20} MiB")
    assert ((_BIG[1] + 1023) // 1024 + 31) // 32 * 32 == 288
    c, r64, r32 = _references(name, "seed43", "geometry")
    out = _run_hip(c, _decoder("seed43"), False, gpu)
    torch.cuda.synchronize()
    rt = Ratios(f"{name}/seed43/geometry", True)
    _compare(rt, c, out, r64, r32, False)
    rt.finish()
    _REF.pop((name, "seed43", "geometry"))


@pytest.mark.parametrize("name,stage", [("17x10", "color"), ("33x31", "color"), ("33x31", "geometry"), ("5000x10", "color")])
def test_training_pass_on_a_side_stream(gpu, name, stage):
    """the weight gradients run on the library's second stream and must be joined back into the caller's: the whole pass on a
    non-default stream, its results consumed there with no device synchronisation in between"""
    c, r64, r32 = _references(name, "seed43", stage)
    s = torch.cuda.Stream(gpu)
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        out = _run_hip(c, _decoder("seed43"), stage == "color", gpu)
        # consumed on `s`: a copy that is enqueued right behind the backward pass
        got = {k: (v.clone() if torch.is_tensor(v) else v) for k, v in out.items()}
        got["grads"] = [g.clone() if g is not None else None for g in out["grads"]]
    s.synchronize()
    rt = Ratios(f"{name}/seed43/{stage}/side-stream", not c.small)
    _compare(rt, c, got, r64, r32, stage == "color")
    rt.finish()


@pytest.mark.parametrize("name", ["3x5", "33x31"])
def test_backward_accumulates_into_the_gradient_buffers(gpu, name):
    """glorie_render_train_bwd ADDS to what the gradient buffers hold: a second backward into buffers preset to X (|X| up to
    half the tensor's largest gradient, so that X costs at most one more rounding at the floor's magnitude) gives X + gradient"""
    from glorie_slam_amd import _lib as L
    from glorie_slam_amd.render_train import _ptr_struct
    c, r64, r32 = _references(name, "seed43", "color")
    lib = L.load()
    d = lambda t: t.to(gpu).contiguous()
    P = [d(t) for t in _decoder("seed43")]
    pts, views, cloud, I, w, has8, z = (d(t) for t in (c.pts, c.views, c.cloud, c.I, c.w, c.has.to(torch.uint8), c.z))
    geo, col = d(c.geo), d(c.col)
    Q = c.Q
    ws = torch.empty(int(lib.glorie_render_train_workspace(Q)) // 4, dtype=torch.float32, device=gpu)
    raw = torch.empty(Q, 4, dtype=torch.float32, device=gpu)
    ps = _ptr_struct(P)
    L.check(lib.glorie_render_train_fwd(ctypes.byref(ps), L.ptr(pts), L.ptr(views), L.ptr(cloud), L.ptr(geo), L.ptr(col),
                                        L.ptr(I), L.ptr(w), L.ptr(has8), Q, 1, L.ptr(ws), L.ptr(raw), L.stream_ptr()), "fwd")
    d_raw = torch.empty(Q, 4, dtype=torch.float32, device=gpu)
    cd, cc = d(c.cd), d(c.cc)
    L.check(lib.glorie_composite_bwd(L.ptr(raw), L.ptr(z), c.R, c.S, float(c.coef), L.ptr(cd), L.ptr(cc), L.ptr(d_raw),
                                     L.stream_ptr()), "composite_bwd")
    g = torch.Generator().manual_seed(7)

    def preset(ref):
        return ((torch.rand(ref.shape, generator=g) - 0.5) * float(ref.abs().max())).float().to(gpu)

    X = [None if i in tr.FIXED else preset(r64["grads"][i]) for i in range(52)]
    Xg, Xc = preset(r64["d_geo"]), preset(r64["d_col"])
    G = [x.clone() if x is not None else None for x in X]
    Gg, Gc = Xg.clone(), Xc.clone()
    gs = _ptr_struct(G)
    L.check(lib.glorie_render_train_bwd(ctypes.byref(ps), ctypes.byref(gs), L.ptr(pts), L.ptr(views), L.ptr(cloud), L.ptr(geo),
                                        L.ptr(col), L.ptr(I), L.ptr(w), L.ptr(has8), Q, 1, L.ptr(ws), L.ptr(d_raw), L.ptr(Gg),
                                        L.ptr(Gc), L.stream_ptr()), "bwd")
    torch.cuda.synchronize()
    rt = Ratios(f"{name}/seed43/color/accumulate", not c.small)
    rt.check("d_geo_feats", Gg.double() - Xg.double(), r64["d_geo"], r32["d_geo"])
    rt.check("d_col_feats", Gc.double() - Xc.double(), r64["d_col"], r32["d_col"])
    for i in range(52):
        if i not in tr.FIXED:
            assert float(X[i].abs().max()) > 0
            rt.check(f"grad[{i}]", G[i].double() - X[i].double(), r64["grads"][i], r32["grads"][i])
    rt.finish()


# ---------------------------------------------------------------------------------------------------------------------
# glorie_composite_bwd on its own
# ---------------------------------------------------------------------------------------------------------------------
def _composite_inputs(R, S, seed):
    g = torch.Generator().manual_seed(seed)
    table = torch.tensor([-100.0, -30.0, -1.0, 0.0, 1.0, 30.0, 1e3])
    occ = torch.where(torch.rand(R, S, generator=g) < 0.5, table[torch.randint(0, 7, (R, S), generator=g)],
                      torch.randn(R, S, generator=g) * 3.0)
    occ[0] = -100.0                                    # a ray of placeholders only
    if R > 1:
        occ[1, 0] = 1e3                                # a ray whose first sample is opaque: alpha == 1 exactly
        occ[R - 1, S - 1] = 1e3
    raw = torch.cat([torch.rand(R, S, 3, generator=g), occ[..., None]], -1).contiguous()
    z = torch.sort(torch.rand(R, S, generator=g) + 0.5, dim=1).values.contiguous()
    return raw, z, torch.randn(R, generator=g), torch.randn(R, 3, generator=g)


@pytest.mark.parametrize("coef", [0.1, 10.0])
@pytest.mark.parametrize("S", [1, 2, 10, 32])
@pytest.mark.parametrize("R", [1, 255, 257])
def test_composite_bwd_matches_float64(gpu, R, S, coef):
    from glorie_slam_amd import _lib as L
    lib = L.load()
    raw, z, gd, gc = _composite_inputs(R, S, 100 * R + S)
    if R > 1:
        a32 = torch.sigmoid(torch.tensor(coef, dtype=torch.float32) * raw[..., 3])
        assert bool((a32 == 1.0).any()) and (coef < 1 or bool((a32 == 0.0).any()))
    rawd, zd = raw.to(gpu), z.to(gpu)
    rt = Ratios(f"composite_bwd/{R}x{S}/coef{coef}", False)
    for mode, (a, b) in (("both", (gd, gc)), ("depth", (gd, None)), ("rgb", (None, gc))):
        out = torch.full((R, S, 4), float("nan"), device=gpu)
        ad, bd = (a.to(gpu) if a is not None else None), (b.to(gpu) if b is not None else None)
        L.check(lib.glorie_composite_bwd(L.ptr(rawd), L.ptr(zd), R, S, coef, L.ptr(ad), L.ptr(bd), L.ptr(out),
                                         L.stream_ptr()), mode)
        torch.cuda.synchronize()
        r64 = tr.composite_grad(raw, z, coef, a, b)
        r32 = tr.composite_grad(raw, z, coef, a, b, dtype=torch.float32)
        assert bool(torch.isfinite(r64).all())
        rt.check(f"{mode}.d_rgb", out[..., :3], r64[..., :3], r32[..., :3])
        rt.check(f"{mode}.d_occ", out[..., 3], r64[..., 3], r32[..., 3])
    rt.finish()


@pytest.mark.parametrize("S", [0, 33])
def test_composite_bwd_rejects_sample_counts_it_cannot_hold(gpu, S):
    from glorie_slam_amd import _lib as L
    buf = torch.zeros(4 * 40 * 4, device=gpu)
    out = torch.full((4 * 40 * 4,), 7.0, device=gpu)
    st = L.load().glorie_composite_bwd(L.ptr(buf), L.ptr(buf), 4, S, 0.1, L.ptr(buf), L.ptr(buf), L.ptr(out), L.stream_ptr())
    torch.cuda.synchronize()
    assert st == -1                                    # GLORIE_EINVAL
    assert bool((out == 7.0).all())                    # and nothing was launched


# ---------------------------------------------------------------------------------------------------------------------
# Adam
# ---------------------------------------------------------------------------------------------------------------------
_ADAM_SIZES = [1, 255, 256, 257, 1023, 1024, 1025, 65535, 65536, 65537]
_LR, _B1, _B2, _EPS = 3e-3, 0.9, 0.999, 1e-8
_MASK_ROWS = 33


def _adam_grad(shape, g):
    """magnitudes from 1e-8 to 1e3, both signs, one element in ten exactly zero"""
    mag = 10.0 ** (torch.rand(shape, generator=g) * 11.0 - 8.0)
    sign = torch.where(torch.rand(shape, generator=g) < 0.5, -1.0, 1.0)
    return (mag * sign * (torch.rand(shape, generator=g) >= 0.1)).float()


def _adam_setup(gpu, capturable):
    from glorie_slam_amd.render_train import FeatureAdam
    g = torch.Generator().manual_seed(21)
    params = [torch.zeros(n, device=gpu).requires_grad_(True) for n in _ADAM_SIZES]
    params.append(torch.zeros(_MASK_ROWS, 32, device=gpu).requires_grad_(True))       # the row-masked table
    for p in params:
        p.grad = torch.zeros_like(p)
    opt = FeatureAdam([{"params": params, "lr": _LR, "betas": (_B1, _B2), "eps": _EPS}], capturable=capturable)
    mask = (torch.rand(_MASK_ROWS, generator=g) < 0.6).to(gpu)
    assert 0 < int(mask.sum()) < _MASK_ROWS
    return opt, params, mask, g


def _adam_fill(params, g, gpu):
    """new gradients IN PLACE, and parameter values that make the update visible: even elements start from exactly 0 (the
    update is then the whole new value - nothing of it is lost to the rounding of p), odd ones from N(0,1)"""
    for p in params:
        p.grad.copy_(_adam_grad(p.shape, g).to(gpu))
        v = torch.randn(p.shape, generator=g)
        v.view(-1)[0::2] = 0.0
        with torch.no_grad():
            p.copy_(v.to(gpu))


def _adam_snapshot(opt, params):
    return [(p.detach().clone(), p.grad.clone(),
             opt.state[id(p)]["m"].clone() if id(p) in opt.state else torch.zeros_like(p),
             opt.state[id(p)]["v"].clone() if id(p) in opt.state else torch.zeros_like(p)) for p in params]


def _adam_check(rt, tag, before, opt, params, step, mask):
    """the update p_after - p_before and both moments of every tensor against adam_ref started from the same state"""
    for k, (p, (p0, g0, m0, v0)) in enumerate(zip(params, before)):
        rm = mask if k == len(params) - 1 else None
        r64 = tr.adam_ref(p0, g0, m0, v0, step, _LR, _B1, _B2, _EPS, rm)
        r32 = tr.adam_ref(p0, g0, m0, v0, step, _LR, _B1, _B2, _EPS, rm, dtype=torch.float32)
        st = opt.state[id(p)]
        p0c = p0.double().cpu()
        upd, u64, u32 = p.detach().double().cpu() - p0c, r64[0] - p0c, r32[0].double() - p0c
        name = f"{tag}.n{p.numel()}"
        zero = (p0c == 0).reshape(-1)
        for sel, what in ((zero, "update[p=0]"), (~zero, "update[p~1]")):
            if bool(sel.any()):
                rt.check(f"{name}.{what}", upd.reshape(-1)[sel], u64.reshape(-1)[sel], u32.reshape(-1)[sel])
        rt.check(f"{name}.m", st["m"], r64[1], r32[1])
        rt.check(f"{name}.v", st["v"], r64[2], r32[2])
        if rm is not None:
            out = ~rm
            assert torch.equal(p.detach()[out], p0[out]) and torch.equal(st["m"][out], m0[out]) and \
                torch.equal(st["v"][out], v0[out]), f"{name}: a masked-out row changed"
            assert not torch.equal(p.detach()[rm], p0[rm])


def _set_step(opt, params, n):
    for p in params:
        opt.state[id(p)]["step"] = n
    if opt.capturable:
        opt._step_dev.fill_(n)


@pytest.mark.parametrize("capturable", [False, True], ids=["by-value", "device-step"])
def test_adam_update_matches_float64(gpu, capturable):
    """glorie_adam_multi (sizes up to 65536), glorie_adam_step (65537 and the row-masked table) and their device-step
    variants, eager, at steps 1..12, 999..1001 and 4999..5001"""
    opt, params, mask, g = _adam_setup(gpu, capturable)
    assert params[-3].numel() == opt.MULTI_MAX and params[-2].numel() == opt.MULTI_MAX + 1
    rt = Ratios("adam/" + ("device-step" if capturable else "by-value"), False)
    steps = list(range(1, 13)) + [999, 1000, 1001, 4999, 5000, 5001]
    for step in steps:
        if step in (999, 4999):
            _set_step(opt, params, step - 1)
        _adam_fill(params, g, gpu)
        before = _adam_snapshot(opt, params)
        opt.step(row_masks={id(params[-1]): mask})
        torch.cuda.synchronize()
        assert all(opt.state[id(p)]["step"] == step for p in params)
        if capturable:
            assert int(opt._step_dev) == step
        _adam_check(rt, f"step{step}", before, opt, params, step, mask)
    rt.finish()


def test_adam_recorded_step_matches_float64(gpu):
    """as the mapper runs it: one eager step, step() recorded on a side stream, replayed 7 times with the gradients rewritten
    in place, the host's counts brought up with advance(), then back to eager steps by value"""
    opt, params, mask, g = _adam_setup(gpu, True)
    masks = {id(params[-1]): mask.to(torch.uint8)}
    rt = Ratios("adam/recorded", False)
    _adam_fill(params, g, gpu)
    before = _adam_snapshot(opt, params)
    opt.step(row_masks=masks)
    torch.cuda.synchronize()
    _adam_check(rt, "eager1", before, opt, params, 1, mask)
    graph = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream(gpu)
    with torch.cuda.graph(graph, stream=side):
        opt.step(row_masks=masks)
    torch.cuda.synchronize()
    n = 7
    for k in range(n):
        _adam_fill(params, g, gpu)
        before = _adam_snapshot(opt, params)
        graph.replay()
        torch.cuda.synchronize()
        assert int(opt._step_dev) == 2 + k
        _adam_check(rt, f"replay{k + 1}", before, opt, params, 2 + k, mask)
    opt.advance(n - 1)
    assert all(opt.state[id(p)]["step"] == int(opt._step_dev) == 1 + n for p in params)
    opt.capturable_fallback()
    _adam_fill(params, g, gpu)
    before = _adam_snapshot(opt, params)
    opt.step(row_masks=masks)
    torch.cuda.synchronize()
    _adam_check(rt, "eager-after", before, opt, params, 2 + n, mask)
    rt.finish()
