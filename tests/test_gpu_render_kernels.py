"""The inference kernels of the renderer against float64: the seven MFMA decoder kernels of csrc/mlp.hip (through
point_ops.render_mlp) against tests/train_ref.py::decode, and idw_gather / idw_gather2 / the weights-only launch, composite
and ray_counts of csrc/render.hip against tests/render_ref.py.  Everything is driven with synthetic, already-placed samples
(the case generator of test_gpu_train_kernels.py, extended by rows whose weights are all zero or sum to 0.5): no KNN, no
golden fixture.

Every floating comparison forms two errors against the float64 result - `e_hip` of the kernels and `e_f32` of the same
reference code run in float32 on the CPU - and asserts, per tensor and over ALL its elements (element-wise maximum error: a
ReLU pre-activation that changes side costs a forward pass no more than the rounding that moved it, so no kink condition),

    e_hip <= M * max(e_f32, 2^-23 * max|ref|)

Masks, placeholders (-100), the zeros of the geometry stage and everything the reference gives as exactly zero are compared
exactly; a second identical decoder call must return identical bits, and the fp16 range flag must stay zero.

M_DECODER = 8 for the decoder outputs, M_LIBM = 8 for IDW and compositing.
profiles/render_kernels_error_ratios.txt lists every case with its worst tensor and ratio (three runs on an MI355X, identical
in every digit: nothing on this path adds atomically).  Each M is twice the worst ratio of its family, rounded up to a power
of two - the margin is for the hardware transcendentals (mlp.hip evaluates the Fourier features with v_sin_f32 / v_cos_f32 on
v_fract_f32 and the sigmoid with __expf; render.hip uses libm) on inputs the cases do not hold:
  decoders          worst 2.172 (3x5/seed43, precise kernels, occ[has])   2 * 2.172 = 4.3 -> 8
  IDW, compositing  worst 2.408 (composite 1x33 at coef 0.1, rgb)         2 * 2.408 = 4.8 -> 8
No ratio stands apart from its family (decoders 0.28 .. 2.17, the split and the precise kernels alike; IDW 0.63 .. 1.23;
compositing 0.18 .. 2.41), so there is no finding to follow up: against a float32 libm evaluation of the same networks the
hardware sin / cos / exp do not show.  The absolute bounds M * max(e_f32, floor) the cases end up with are at most 7.7e-5 on
colours and 2.8e-5 on occupancy logits for the seed-43 decoders at points within 0.05 of the origin (4.7e-4 / 1.5e-4 with the
saturated decoders); at scene-sized points (|x| <= 2) the float32 yardstick itself is off by 2.7e-5 / 2.1e-4 and the bounds
are 2.1e-4 / 1.6e-3 (1.8e-3 / 8.1e-3 saturated) - the kernels' own error there is 1.2e-4 on occupancy.
Each test prints its ratios (`RATIO ...`), the relative Frobenius error beside them (`FROB ...`) and the absolute bound it
ends up with (`BOUND ...`), pytest -s.
"""
import pytest
import torch

import render_ref as rr
import train_ref as tr
from test_gpu_train_kernels import CASES, Ratios, _composite_inputs, _decoder, make_case

pytestmark = pytest.mark.gpu
M_DECODER = 8.0
M_LIBM = 8.0
_ULP = 2.0 ** -23


class _Ratios(Ratios):
    """Ratios with the element-wise maximum error; prints the relative Frobenius error and the absolute bound as well"""

    def __init__(self, label, m):
        super().__init__(label, False, m)

    def check(self, name, hip, r64, r32):
        super().check(name, hip, r64, r32)
        top = float(r64.abs().max()) if r64.numel() else 0.0
        if top == 0.0:
            return
        h = hip.detach().double().cpu().reshape(r64.shape)
        nrm = float(r64.norm())
        e_f32 = float((r32.double() - r64).abs().max())
        print(f"FROB {self.label} {name} hip {float((h - r64).norm()) / nrm:.3e} f32 {float((r32.double() - r64).norm()) / nrm:.3e}")
        print(f"BOUND {self.label} {name} {self.m * max(e_f32, _ULP * top):.3e}")


# ---------------------------------------------------------------------------------------------------------------------
# decoders
# ---------------------------------------------------------------------------------------------------------------------
# name: (R, S, Np, seed for the seed-43 decoders, seed for the saturated ones or None), as in CASES
_NEW_CASES = {
    "127x1": (127, 1, 5, 101, None),             # one below the 128-sample tile
    "129x1": (129, 1, 600, 102, 103),            # one past it: a second workgroup with one live sample
    "65665x1": (65665, 1, 30000, 104, None),     # 512 * 128 + 129: the grid stride of mlp_geo_v4 and a ragged last tile
}
_ALL_CASES = dict(CASES, **_NEW_CASES)
_LARGE = ("5000x10", "65665x1")
# at the two largest sizes one colour and one geometry run per kernel family, both feature modes between them
_LARGE_MODES = {("color", False): ("c_geo",), ("geometry", False): ("in-kernel",),
                ("color", True): ("in-kernel",), ("geometry", True): ("c_geo",)}
_RUNS = [(n, v, s, p) for n, spec in _ALL_CASES.items() for v in (("seed43", "saturated") if spec[4] is not None else ("seed43",))
         for s in ("color", "geometry") for p in (False, True)]


def _case(name, variant):
    R, S, Np, s43, ssat = _ALL_CASES[name]
    return make_case(R, S, Np, s43 if variant == "seed43" else ssat, unnormalised=True)


def _decode(c, P, dtype, chunk=16384):
    """raw [Q,4] (rgb of the colour stage, occupancy with its placeholders) and the interpolated geometry feature"""
    f = lambda t: t.to(dtype)
    P = [f(t) for t in P]
    pts, views, cloud, geo, col, w = (f(t) for t in (c.pts, c.views, c.cloud, c.geo, c.col, c.w))
    occ, rgb = [], []
    with torch.no_grad():
        for lo in range(0, c.Q, chunk):
            q = slice(lo, lo + chunk)
            o, r, _ = tr.decode(P, pts[q], views[q], cloud, geo, col, c.I[q], w[q], c.has[q], True)
            occ.append(o), rgb.append(r)
        occ = torch.where(c.has, torch.cat(occ), torch.full((), tr.PLACEHOLDER, dtype=dtype))
        return torch.cat([torch.cat(rgb), occ[:, None]], -1), rr.idw_features(geo, c.I, w, c.has)


_REF = {}


def _references(name, variant):
    """(case, float64 raw, float32 raw, float64 geometry feature), computed once per process and left unchanged"""
    key = (name, variant)
    if key not in _REF:
        c = _case(name, variant)
        raw64, cgeo64 = _decode(c, _decoder(variant), torch.float64)
        raw32, _ = _decode(c, _decoder(variant), torch.float32)
        _REF[key] = (c, raw64, raw32, cgeo64)
    return _REF[key]


def load_decoder_tensors(tensors):
    """the 52-tensor list back in a POINT module (what pack_decoders takes)"""
    from glorie_slam_amd.decoder import POINT
    from glorie_slam_amd.render_train import decoder_tensors
    from test_golden import _decoder_cfg
    dec = POINT(_decoder_cfg(), c_dim=32, hidden_size=128, use_view_direction=True).eval()
    with torch.no_grad():
        for dst, src in zip(decoder_tensors(dec), tensors):
            assert dst.shape == src.shape
            dst.copy_(src)
    after = decoder_tensors(dec)
    assert len(after) == len(tensors) == 52 and all(torch.equal(a.detach(), b) for a, b in zip(after, tensors))
    return dec


_PACKED, _DEV = {}, {}


def _packed(variant, gpu):
    if variant not in _PACKED:
        from glorie_slam_amd import point_ops
        _PACKED[variant] = point_ops.pack_decoders(load_decoder_tensors(_decoder(variant)).to(gpu))
    return _PACKED[variant]


def _on_device(name, variant, gpu):
    key = (name, variant)
    if key not in _DEV:
        c, _, _, cgeo64 = _references(name, variant)
        d = lambda t: t.to(gpu).contiguous()
        _DEV[key] = dict(pts=d(c.pts), views=d(c.views), cloud=d(c.cloud), geo=d(c.geo), col=d(c.col), I=d(c.I), w=d(c.w),
                         has=d(c.has.to(torch.uint8)), c_geo=d(cgeo64.float()))
    return _DEV[key]


def _render(t, packed, stage, precise, mode, flag):
    from glorie_slam_amd import point_ops
    in_kernel = mode == "in-kernel"
    return point_ops.render_mlp(packed, t["pts"], t["views"], t["cloud"], t["col"], None if in_kernel else t["c_geo"], t["I"],
                                t["w"], t["has"], stage=stage, geo_feats=t["geo"] if in_kernel else None, precise=precise,
                                range_flag=None if precise else flag)


def _patterns(c):
    """rows of every neighbour pattern among the samples whose occupancy is computed (has == 1), and the has == 0 rows"""
    live, plain = c.has, c.wsum == 0
    return {"full": live & plain & (c.I >= 0).all(1) & (c.kind != 3),
            "missing": live & plain & (c.I < 0).any(1),
            "duplicates": live & plain & (c.kind == 3),
            "weights all zero": live & (c.wsum == 1),
            "weights sum to 0.5": live & (c.wsum == 2),
            "has == 0 with live weights": ~live & (c.w.sum(1) > 0.4)}


def _assert_case_is_what_it_claims(c):
    n = {k: int(v.sum()) for k, v in _patterns(c).items()}
    zero, half = c.wsum == 1, c.wsum == 2
    assert bool((c.w[zero] == 0).all()) and bool(c.has[zero].all()) and bool(c.has[half].all())
    if bool(half.any()):
        assert float((c.w[half].sum(1) - 0.5).abs().max()) < 1e-6
    assert bool((c.w[c.I < 0] == 0).all())
    d = c.I[_patterns(c)["duplicates"]]
    assert bool(((d[:, 1] == d[:, 0]) & (d[:, 5] == d[:, 2]) & (d[:, 6] == d[:, 2])).all())
    if c.Q >= 2:
        assert float(c.views[c.Q // 2].abs().max()) == 0.0
    if c.R >= 2:
        assert bool((~c.has.view(c.R, c.S)).all(1).any())
    if c.Q >= 7:
        assert n["has == 0 with live weights"] > 0 and n["missing"] > 0
    if c.Q >= 9:
        assert n["weights all zero"] == n["weights sum to 0.5"] == c.Q // 9
    if c.Q >= 63:
        assert min(n.values()) > 0, n
    return n


def test_decoder_cases_cover_the_sizes_and_the_neighbour_patterns():
    sizes, seen = set(), {}
    for name, spec in _ALL_CASES.items():
        for variant in ("seed43", "saturated") if spec[4] is not None else ("seed43",):
            c = _case(name, variant)
            sizes.add(c.Q)
            for k, v in _assert_case_is_what_it_claims(c).items():
                seen[k] = seen.get(k, 0) + v
    assert {1, 127, 129, 257} <= sizes and (128 in sizes or 256 in sizes) and max(sizes) > 65536
    assert 512 * 128 + 129 in sizes
    assert min(seen.values()) > 0, seen
    assert {(n, v) for n, v, _, _ in _RUNS} >= {("129x1", "saturated"), ("33x31", "saturated"), ("65665x1", "seed43")}


@pytest.mark.parametrize("name,variant,stage,precise", _RUNS,
                         ids=[f"{n}-{v}-{s}-{'precise' if p else 'split'}" for n, v, s, p in _RUNS])
def test_decoders_match_float64(gpu, name, variant, stage, precise):
    """mlp_geo_v4 / mlp_nb_v4 / mlp_col_v5 (split) or mlp_geo_v3 / mlp_nb_v3 / mlp_col_v3 (precise), with the geometry feature
    handed in (the float64 interpolation rounded to float32) and interpolated inside the geometry kernel"""
    c, raw64, raw32, _ = _references(name, variant)
    _assert_case_is_what_it_claims(c)
    t, packed = _on_device(name, variant, gpu), _packed(variant, gpu)
    flag = torch.zeros(1, dtype=torch.int32, device=gpu)
    color, has = stage == "color", c.has
    modes = _LARGE_MODES[(stage, precise)] if name in _LARGE else ("c_geo", "in-kernel")
    rt = _Ratios(f"{name}/{variant}/{stage}/{'precise' if precise else 'split'}", M_DECODER)
    for mode in modes:
        raw = _render(t, packed, stage, precise, mode, flag)
        again = _render(t, packed, stage, precise, mode, flag)
        torch.cuda.synchronize()
        assert int(flag.item()) == 0, f"{mode}: the fp16 range flag is raised"
        assert torch.equal(raw, again), f"{mode}: two identical calls differ"
        raw = raw.cpu()
        assert raw.shape == (c.Q, 4) and bool(torch.isfinite(raw).all())
        assert bool((raw[~has, 3] == tr.PLACEHOLDER).all()), f"{mode}: a has == 0 row without the -100 placeholder"
        if bool(has.any()):
            rt.check(f"{mode}.occ[has]", raw[has, 3], raw64[has, 3], raw32[has, 3])
        if color:
            rt.check(f"{mode}.rgb", raw[:, :3], raw64[:, :3], raw32[:, :3])
            if bool((~has).any()):            # still the network's value at c = 0, on their own
                rt.check(f"{mode}.rgb[~has]", raw[~has, :3], raw64[~has, :3], raw32[~has, :3])
        else:
            assert float(raw[:, :3].abs().max()) == 0.0, f"{mode}: the geometry stage wrote colours"
    rt.finish()


@pytest.mark.parametrize("name", ["1x1", "129x1", "65665x1"])
def test_gather_phase_only_is_the_interpolated_feature(gpu, name):
    """stage_flags & 4 (mlp_geo_v4<GO>, what bench.py times as the feature pull): the kernel's own interpolation with the
    network dropped - column 3 is (f0 + f1) + (f18 + f19) of the interpolated geometry feature, by the IDW family's rule;
    129 samples give the second workgroup one live sample, 65665 the grid stride and the ragged tail"""
    from glorie_slam_amd import point_ops
    c, _, _, cgeo64 = _references(name, "seed43")
    t, packed = _on_device(name, "seed43", gpu), _packed("seed43", gpu)
    run = lambda: point_ops.render_mlp(packed, t["pts"], t["views"], t["cloud"], t["col"], None, t["I"], t["w"], t["has"],
                                       stage="geometry", geo_feats=t["geo"], gather_phase_only=True)
    raw, again = run(), run()
    torch.cuda.synchronize()
    assert torch.equal(raw, again), "two identical calls differ"
    raw = raw.cpu()
    assert raw.shape == (c.Q, 4) and bool(torch.isfinite(raw).all())
    assert float(raw[:, :3].abs().max()) == 0.0, "the geometry stage wrote colours"
    assert bool((raw[~c.has, 3] == 0).all()), "a has == 0 row with a feature"
    pick = lambda f: (f[:, 0] + f[:, 1]) + (f[:, 18] + f[:, 19])
    cgeo32 = rr.idw_features(c.geo.float(), c.I, c.w.float(), c.has)
    assert cgeo64.dtype == torch.float64 and cgeo32.dtype == torch.float32
    rt = _Ratios(f"gather-only/{name}", M_LIBM)
    rt.check("f0+f1+f18+f19", raw[:, 3], pick(cgeo64), pick(cgeo32))
    rt.finish()


# ---------------------------------------------------------------------------------------------------------------------
# inverse-distance weights and features
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("per_query", [False, True], ids=["fixed-radius", "radius-per-query"])
@pytest.mark.parametrize("Q", [1, 7, 8, 9, 31, 33, 257, 2049])
def test_idw_kernels_match_float64(gpu, Q, per_query):
    """idw_gather, idw_gather2 and the weights-only launch: masks exact, the three launches bit-equal, weights and features by
    the ratio rule - for min_nn 1..3 and both weightings"""
    from glorie_slam_amd import point_ops
    Np = 50
    D, I, nn, r, kind = rr.make_idw_case(Q, Np, 1000 + Q, per_query)
    if Q >= 7:
        assert sorted(set(kind.tolist())) == list(range(7))
    g = torch.Generator().manual_seed(Q)
    fa, fb = torch.randn(Np, 32, generator=g) * 0.3, torch.randn(Np, 32, generator=g) * 0.3
    d = lambda t: t.to(gpu)
    Dd, Id, nnd, fad, fbd = d(D), d(I), d(nn), d(fa), d(fb)
    rq = dict(radius_per_query=r) if per_query else dict(radius=r)
    rqd = dict(radius_per_query=d(r)) if per_query else dict(radius=r)
    rt = _Ratios(f"idw/{Q}/{'per-query' if per_query else 'fixed'}", M_LIBM)
    for min_nn in (1, 2, 3):
        for expo in (False, True):
            kw = dict(min_nn=min_nn, expo=expo)
            ca, has, w = point_ops.idw_gather(Dd, Id, nnd, fad, return_weights=True, **rqd, **kw)
            cb, hasb = point_ops.idw_gather(Dd, Id, nnd, fbd, **rqd, **kw)
            c2a, c2b, has2, w2 = point_ops.idw_gather2(Dd, Id, nnd, fad, fbd, **rqd, **kw)
            none, has0, w0 = point_ops.idw_gather(Dd, Id, nnd, None, return_weights=True, **rqd, **kw)
            torch.cuda.synchronize()
            assert none is None
            assert torch.equal(c2a, ca) and torch.equal(c2b, cb) and torch.equal(has2, has) and torch.equal(hasb, has)
            assert torch.equal(w2, w) and torch.equal(w0, w) and torch.equal(has0, has)
            w64, has64 = rr.idw_weights(D, I, nn, **rq, **kw)
            w32, has32 = rr.idw_weights(D, I, nn, dtype=torch.float32, **rq, **kw)
            w, has = w.cpu(), has.cpu()
            assert torch.equal(has, has64) and torch.equal(has32, has64)
            assert torch.equal(w == 0, w64 == 0) and torch.equal(w32 == 0, w64 == 0), "the radius / index mask differs"
            tag = f"min_nn{min_nn}.{'expo' if expo else 'inverse'}"
            rt.check(f"{tag}.w", w, w64, w32)
            for nm, got, f in (("c_a", ca, fa), ("c_b", cb, fb)):
                c64 = rr.idw_features(f.double(), I, w64, has64)
                c32 = rr.idw_features(f, I, w32, has64)
                rt.check(f"{tag}.{nm}", got, c64, c32)
                assert torch.equal(got.cpu() == 0, c64 == 0), f"{nm}: exact zeros differ"
            k = lambda nm: kind == rr.IDW_KINDS.index(nm)
            assert bool(has[k("all outside")].all()) and bool((w[k("all outside")] == 0).all())
            assert bool((ca.cpu()[k("all outside") | k("too few")] == 0).all())
            assert not bool(has[k("too few")].any()) and bool((w[k("too few")].sum(1) > 0.99).all())
            assert bool((w[k("tie"), 2] > 0).all()) and bool((w[k("tie"), 3] == 0).all())
            assert bool((w[I < 0] == 0).all())
    rt.finish()


# ---------------------------------------------------------------------------------------------------------------------
# compositing
# ---------------------------------------------------------------------------------------------------------------------
def _composite_case(R, S):
    """`_composite_inputs` with ray 0 all placeholders and ray 1 saturated at +100 in its first sample; R == 1 gets three
    rays (placeholders, saturated, ordinary) that are composited one launch each"""
    raw, z, _, _ = _composite_inputs(3 if R == 1 else R, S, 100 * R + S)
    assert bool((raw[0, :, 3] == -100.0).all())
    raw[1, 0, 3] = 100.0
    return raw, z


@pytest.mark.parametrize("coef", [0.1, 10.0])
@pytest.mark.parametrize("S", [1, 2, 10, 32, 33])
@pytest.mark.parametrize("R", [1, 255, 256, 257])
def test_composite_matches_float64(gpu, R, S, coef):
    from glorie_slam_amd import point_ops
    raw, z = _composite_case(R, S)
    batches = [slice(i, i + 1) for i in range(3)] if R == 1 else [slice(0, R)]
    rt = _Ratios(f"composite/{R}x{S}/coef{coef}", M_LIBM)
    for b in batches:
        rw, zz = raw[b].contiguous(), z[b].contiguous()
        got = point_ops.composite(rw.to(gpu), zz.to(gpu), coef)
        bare = point_ops.composite(rw.to(gpu), zz.to(gpu), coef, return_weights=False)
        torch.cuda.synchronize()
        assert bare[3] is None and all(torch.equal(x, y) for x, y in zip(got[:3], bare[:3]))
        r64 = rr.composite_full(rw.double(), zz.double(), coef)
        r32 = rr.composite_full(rw, zz, coef)
        assert all(bool(torch.isfinite(x).all()) for x in r64)
        tag = f"ray{b.start}." if R == 1 else ""
        for nm, x, y64, y32 in zip(("depth", "var", "rgb", "weights"), got, r64, r32):
            assert x.shape == y64.shape
            rt.check(tag + nm, x, y64, y32)
        if b.start == 0 and coef == 10.0:               # sigmoid(-1000) == 0: the placeholder ray leaves exactly nothing
            assert all(float(x[0].abs().max()) == 0.0 for x in got)
            assert all(float(x[0].abs().max()) == 0.0 for x in r64)
        sat = 1 - b.start                               # the saturated ray, where this launch holds it
        if 0 <= sat < rw.shape[0] and coef == 10.0:     # sigmoid(1000) == 1: the first sample takes everything
            assert float(got[3][sat, 0]) == 1.0 and float(r64[3][sat, 0]) == 1.0
    rt.finish()


# ---------------------------------------------------------------------------------------------------------------------
# sample counts
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("min_samples", [1, 3])
@pytest.mark.parametrize("S", [1, 10, 32])
@pytest.mark.parametrize("R", [1, 255, 257])
def test_ray_counts_exact(gpu, R, S, min_samples):
    from glorie_slam_amd import point_ops
    g = torch.Generator().manual_seed(10 * R + S)
    masks = [torch.rand(R * S, generator=g) < 0.5, torch.rand(R * S, generator=g) < 0.1,
             torch.zeros(R * S, dtype=torch.bool), torch.ones(R * S, dtype=torch.bool)]
    if R > 2:
        masks[0].view(R, S)[1] = False                  # an all-zero and an all-one ray among random ones
        masks[0].view(R, S)[R - 1] = True
    for has in masks:
        for h in (has, has.to(torch.uint8)):
            counts, valid = point_ops.ray_counts(h.to(gpu), S, min_samples)
            torch.cuda.synchronize()
            rc, rv = rr.ray_counts(has, S, min_samples)
            assert counts.dtype == torch.int64 and valid.dtype == torch.bool
            assert torch.equal(counts.cpu(), rc) and torch.equal(valid.cpu(), rv)


# ---------------------------------------------------------------------------------------------------------------------
# the chain
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precise", [False, True], ids=["split", "precise"])
def test_chain_of_kernels_matches_the_chain_of_references(gpu, precise):
    """33 rays x 10 samples from synthetic search results: idw_gather2 -> render_mlp on the kernel's own weights and
    feature -> ray_counts -> composite, against the same chain in float64 (yardstick: the same chain in float32)"""
    from glorie_slam_amd import point_ops
    R, S, Np, coef = 33, 10, 50, 0.1
    Q = R * S
    D, I, nn, r, kind = rr.make_idw_case(Q, Np, 77, True)
    g = torch.Generator().manual_seed(78)
    pts, views = (torch.rand(Q, 3, generator=g) - 0.5) * 0.1, torch.randn(Q, 3, generator=g)
    cloud = (torch.rand(Np, 3, generator=g) - 0.5) * 0.1
    geo, col = torch.randn(Np, 32, generator=g) * 0.3, torch.randn(Np, 32, generator=g) * 0.3
    z = torch.sort(torch.rand(R, S, generator=g) + 0.5, dim=1).values.contiguous()
    P = _decoder("seed43")
    d = lambda t: t.to(gpu)
    c_geo, c_col, has, w = point_ops.idw_gather2(d(D), d(I), d(nn), d(geo), d(col), radius_per_query=d(r), min_nn=2)
    flag = torch.zeros(1, dtype=torch.int32, device=gpu)
    raw = point_ops.render_mlp(_packed("seed43", gpu), d(pts), d(views), d(cloud), d(col), c_geo, d(I), w, has, stage="color",
                               precise=precise, range_flag=None if precise else flag)
    counts, valid = point_ops.ray_counts(has, S, 3)
    depth, var, rgb, weights = point_ops.composite(raw.reshape(R, S, 4), d(z), coef)
    torch.cuda.synchronize()
    assert int(flag.item()) == 0

    def chain(dtype):
        f = lambda t: t.to(dtype)
        wr, hr = rr.idw_weights(D, I, nn, radius_per_query=r, min_nn=2, dtype=dtype)
        with torch.no_grad():
            occ, col_, _ = tr.decode([f(t) for t in P], f(pts), f(views), f(cloud), f(geo), f(col), I, wr, hr, True)
        occ = torch.where(hr, occ, torch.full((), tr.PLACEHOLDER, dtype=dtype))
        rw = torch.cat([col_, occ[:, None]], -1)
        return (wr, hr, rw) + rr.composite_full(rw.reshape(R, S, 4), f(z), coef)

    w64, has64, raw64, d64, v64, c64, cw64 = chain(torch.float64)
    w32, has32, raw32, d32, v32, c32, cw32 = chain(torch.float32)
    assert torch.equal(has.cpu(), has64) and torch.equal(has32, has64) and 0 < int(has64.sum()) < Q
    rc, rv = rr.ray_counts(has64, S, 3)
    assert torch.equal(counts.cpu(), rc) and torch.equal(valid.cpu(), rv) and 0 < int(rv.sum())
    raw = raw.cpu()
    assert bool((raw[~has64, 3] == tr.PLACEHOLDER).all())
    lib = _Ratios(f"chain/{'precise' if precise else 'split'}/idw", M_LIBM)
    lib.check("w", w, w64, w32)
    lib.check("c_geo", c_geo, rr.idw_features(geo.double(), I, w64, has64), rr.idw_features(geo, I, w32, has64))
    lib.finish()
    rt = _Ratios(f"chain/{'precise' if precise else 'split'}", M_DECODER)
    rt.check("raw.rgb", raw[:, :3], raw64[:, :3], raw32[:, :3])
    rt.check("raw.occ[has]", raw[has64, 3], raw64[has64, 3], raw32[has64, 3])
    for nm, x, y64, y32 in (("depth", depth, d64, d32), ("var", var, v64, v32), ("rgb", rgb, c64, c32),
                            ("weights", weights, cw64, cw32)):
        rt.check(nm, x, y64, y32)
    rt.finish()
