"""Reference of the depth_scale preparation (csrc/dspo_prep.hip) in plain numpy, and the scenes that make it observable
(test infrastructure).

The reference restates DepthVideo.update_valid_depth_mask (depth_video.py:326-361), common.align_scale_and_shift and the
mono_thres rule of dspo._prepare_torch.  It shares nothing with the kernels: the medians come from a sort, the alignment is
solved in float64, the consistent-neighbour count is oracle.geom.depth_filter (the kernel under it is held to that oracle bit
for bit in test_gpu_geom.py).  The depths are float32(1) / disparity: the kernels divide with correct rounding, so numpy's
IEEE division is the same function and the masks can be compared for equality.

select_scene builds one frame of each kind in KINDS.  Called with visible_num = 0 every non-NaN depth is a key whatever the
depth filter counts, so the scenes isolate the two median selects from the geometry.  coupled_scene is a multi-view
consistent map stack (geom_ref.plane_graph with a far plane) whose frames carry mono priors of different quality.
"""
import functools

import numpy as np

import geom_ref
import glorie_slam_amd.synth as synth
from oracle import geom as ogeom

F = np.float32
EPS = 2.0 ** -24
KINDS = ("heavy_tail", "constant", "two_values", "low_byte", "wide_exponent", "scattered_nan", "one_valid", "two_valid",
         "no_valid")
SENSITIVE = ("heavy_tail", "two_values", "low_byte")         # a median one distinct depth off must change the mask
FLAT_TARGET = ("constant", "two_values", "low_byte")         # the masked disparities are (nearly) one value: scale ~ 0
NO_FIT = ("one_valid", "two_valid", "no_valid")              # fewer than two masked pixels: the 2 x 2 system is singular
PREPARE_SIZES = ((2, 2), (3, 5), (7, 9), (5, 13), (16, 16), (11, 93), (25, 41), (43, 47), (160, 240))
VMASK_SIZES = ((3, 5), (15, 17), (257, 1), (23, 89), (29, 71), (96, 128))
COUPLED_SIZES = ((24, 32), (33, 31))
FILL_DISP, FILL_MONO = F(1e-3), F(777.0)                     # frames beyond n: reading one would move every result

# Largest error of common.align_scale_and_shift evaluated in float32 on the CPU against align64, in units of
# kappa * 2^-24, over all frames of the class (profiles/dspo_prepare_error.txt; test_dspo_prep_ref.py holds the float32
# formulation to them).  The kernel is allowed MARGIN times as much.
MARGIN = 4.0
F32_ERROR = {                      # class: (scale, shift)
    "select": (4.366, 4.383),      # the select scenes' frames with a fit, PREPARE_SIZES; kappa 1.04 .. 1.8e4
    "select_flat": (4.607, 4.586),   # their frames whose masked target is one value (scale ~ 0), see align_errors
    "coupled": (4.411, 3.974),     # coupled_scene, COUPLED_RUNS; kappa 1.04 .. 1.4e3
}


# ---- reference --------------------------------------------------------------------------------------------------------------
def depths(disps):
    with np.errstate(divide="ignore", invalid="ignore"):
        return (F(1) / np.asarray(disps, F)).astype(F)


def thresholds(disps_sel, mv_thresh):
    z = depths(disps_sel).reshape(len(disps_sel), -1).astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        return (F(mv_thresh) * z.mean(1).astype(F)).astype(F)


def lower_median(z, valid):
    v = np.sort(z[valid])
    return v[(len(v) - 1) // 2] if len(v) else F(np.nan)


def mask_for(z, valid, med):
    with np.errstate(invalid="ignore", over="ignore"):
        return valid & (z < (F(3) * F(med)).astype(F))


def distinct_neighbours(z, valid, med):
    """nearest distinct valid depth below and above `med` (None where there is none)"""
    v = z[valid]
    lo, hi = v[v < med], v[v > med]
    return (lo.max() if len(lo) else None), (hi.min() if len(hi) else None)


def valid_mask(poses, disps, intrinsics, ix, mv_thresh, visible_num):
    """-> dict thresh [num], count, z, valid, mask [num,h,w], median [num]"""
    disps = np.asarray(disps, F)
    ix = np.asarray(ix, np.int64)
    thresh = thresholds(disps[ix], mv_thresh)
    count = ogeom.depth_filter(poses, disps, intrinsics, ix, thresh)
    z = depths(disps[ix])
    valid = (count >= visible_num) & ~np.isnan(z)
    median = np.array([lower_median(z[b], valid[b]) for b in range(len(ix))], F)
    mask = np.stack([mask_for(z[b], valid[b], median[b]) for b in range(len(ix))]) if len(ix) else valid
    return dict(thresh=thresh, count=count, z=z, valid=valid, median=median, mask=mask)


def align64(mono, disps, mask):
    """float64 least squares disps ~ scale * mono + shift over mask, per frame -> dict scale, shift, err (mean absolute
    residual), kappa = a00 a11 / det, lever = a01 / a11, pmean = mean |mono| over the mask, nmask"""
    n = len(mono)
    out = {k: np.full(n, np.nan) for k in ("scale", "shift", "err", "kappa", "lever", "pmean")}
    out["nmask"] = np.zeros(n, np.int64)
    for f in range(n):
        m = mask[f].reshape(-1)
        p = np.asarray(mono[f], np.float64).reshape(-1)[m]
        t = np.asarray(disps[f], np.float64).reshape(-1)[m]
        a00, a01, a11, b0, b1 = (p * p).sum(), p.sum(), float(len(p)), (p * t).sum(), t.sum()
        out["nmask"][f] = len(p)
        det = a00 * a11 - a01 * a01
        if len(p) == 0 or det == 0:
            continue
        s, q = (a11 * b0 - a01 * b1) / det, (-a01 * b0 + a00 * b1) / det
        out["scale"][f], out["shift"][f] = s, q
        out["err"][f] = np.abs(s * p + q - t).mean()
        out["kappa"][f] = a00 * a11 / det
        out["lever"][f] = a01 / a11
        out["pmean"][f] = np.abs(p).mean()
    return out


def align32(mono, disps, mask):
    """the reference's own formulation, common.align_scale_and_shift, on float32 CPU tensors (unmasked pixels zeroed)"""
    import torch
    from glorie_slam_amd.common import align_scale_and_shift
    mask = np.asarray(mask, bool)
    t = lambda x: torch.from_numpy(np.where(mask, x, 0).astype(F))       # weight 0 times NaN is NaN: keep NaN out
    threads = torch.get_num_threads()
    torch.set_num_threads(1)                                             # one summation order on every machine
    try:
        s, q, e = align_scale_and_shift(t(mono), t(disps), torch.from_numpy(mask.copy()))
    finally:
        torch.set_num_threads(threads)
    return s.numpy(), q.numpy(), e.numpy()


def align_errors(scale, shift, a, flat=False):
    """errors of a float32 result against align64's `a` in units of kappa * 2^-24 -> (scale [n], shift [n]).
    |ds| / |s|, |dq| / (|q| + |s| lever); where the masked target is one value (flat) the scale is ~0 and its error is
    taken against the magnitude it is the difference of, |s| + |q| / lever.  NaN where there is no fit."""
    with np.errstate(invalid="ignore", divide="ignore"):
        unit = a["kappa"] * EPS
        den_s = np.abs(a["scale"]) + (np.abs(a["shift"]) / np.abs(a["lever"]) if flat else 0.0)
        den_q = np.abs(a["shift"]) + np.abs(a["scale"] * a["lever"])
        return (np.abs(np.asarray(scale, np.float64) - a["scale"]) / den_s / unit,
                np.abs(np.asarray(shift, np.float64) - a["shift"]) / den_q / unit)


def bad_frames(a, avg, hw, mono_thres, rel_bound=(0.0, 0.0), flat=False):
    """the mono_thres rule -> bad [n] bool, margins dict.  margins: `err` = |err / avg - mono_thres| in units of the
    error that a relative error rel_bound = (scale, shift) of the fit can cause in err / avg; `count` = |nmask - hw / 2|
    (pixels); `scale` = |scale| in units of its own possible error (flat: measured as align_errors does).  inf where a quantity is not finite (NaN decides the
    rule by itself) or rel_bound is 0."""
    n = len(a["scale"])
    bad = np.zeros(n, bool)
    margins = dict(err=np.full(n, np.inf), count=np.abs(a["nmask"] - 0.5 * hw), scale=np.full(n, np.inf))
    if not mono_thres or mono_thres <= 0:
        return bad, margins
    with np.errstate(invalid="ignore", divide="ignore"):
        ratio = a["err"] / np.asarray(avg, np.float64)
        bad = (ratio > mono_thres) | np.isnan(a["err"]) | (a["scale"] < 0) | (a["nmask"] < 0.5 * hw)
        ds = (np.abs(a["scale"]) + (np.abs(a["shift"] / a["lever"]) if flat else 0.0)) * rel_bound[0]
        dq = (np.abs(a["shift"]) + np.abs(a["scale"] * a["lever"])) * rel_bound[1]
        derr = (ds * a["pmean"] + dq) / np.abs(avg)
        ok = np.isfinite(ratio) & (derr > 0)
        margins["err"][ok] = (np.abs(ratio - mono_thres) / derr)[ok]
        ok = np.isfinite(a["scale"]) & (ds > 0)
        margins["scale"][ok] = (np.abs(a["scale"]) / ds)[ok]
    return bad, margins


def edges(bad, ii, jj, n):
    ii, jj = np.asarray(ii, np.int64), np.asarray(jj, np.int64)
    look = lambda k: np.array([bool(bad[i]) if 0 <= i < n else False for i in k], bool)
    edge_on = ~(look(ii) | look(jj))
    return edge_on, int(edge_on.any())


def prepare(poses, disps, intrinsics, mono, n, mv_thresh, visible_num, mono_thres, ii, jj, bound=(0.0, 0.0), flat=False):
    """glorie_dspo_prepare on the first n frames of the stack -> the dict of valid_mask plus the alignment (`fit`), avg,
    bad, margins, edge_on, any_on.  bound = (scale, shift): the alignment error, in units of kappa * 2^-24, that the
    margins are measured in"""
    disps = np.asarray(disps, F)
    r = valid_mask(poses, disps, intrinsics, np.arange(n), mv_thresh, visible_num)
    r["fit"] = align64(mono[:n], disps[:n], r["mask"])
    with np.errstate(invalid="ignore"):
        r["avg"] = disps[:n].reshape(n, -1).astype(np.float64).mean(1).astype(F) if n else np.zeros(0, F)
    with np.errstate(invalid="ignore"):
        unit = np.nan_to_num(r["fit"]["kappa"] * EPS, nan=0.0, posinf=0.0)
    r["bad"], r["margins"] = bad_frames(r["fit"], r["avg"], disps.shape[1] * disps.shape[2], mono_thres,
                                        (bound[0] * unit, bound[1] * unit), flat)
    r["edge_on"], r["any_on"] = edges(r["bad"], ii, jj, n)
    return r


# ---- select scenes ----------------------------------------------------------------------------------------------------------
def _ulps(x, k):
    """the float32 k steps from x (positive finite x)"""
    return (np.asarray(x, F).view(np.int32) + np.int32(k)).view(F)


def disparity_of(z):
    """a float32 disparity d with float32(1) / d == z exactly (searched +-8 floats around 1 / z)"""
    z = F(z)
    c = _ulps(F(1) / z, np.arange(-8, 9))
    hit = c[F(1) / c == z]
    assert len(hit), "no disparity gives depth %r" % z
    return hit[len(hit) // 2]


def plant(d):
    """Overwrite the two deepest valid pixels of the flat disparity map d (NaN = no key) with one depth just below and one
    just above 3 * median, so that a median one distinct depth lower drops the first and one distinct depth higher admits
    the second -> their indices.  The pixels of rank <= k keep their rank, so the median stays."""
    z = depths(d)
    valid = ~np.isnan(z)
    n = int(valid.sum())
    assert n >= 4
    med = lower_median(z, valid)
    order = np.argsort(np.where(valid, z, -np.inf), kind="stable")
    ia, ib = order[-2], order[-1]
    keep = valid.copy()
    keep[[ia, ib]] = False
    lo, hi = distinct_neighbours(z, keep, med)
    assert lo is not None and lower_median(z, keep) <= med
    lim = F(3) * med
    zc = F(1) / _ulps(F(1) / lim, np.arange(-8, 9))
    below = zc[(zc < lim) & (zc >= F(3) * lo) & (zc > med)]
    above = zc[(zc >= lim) & ((zc < F(3) * hi) if hi is not None else True)]
    assert len(below) and len(above), "no disparity within 8 floats falls between the two limits"
    d[ia], d[ib] = disparity_of(below.max()), disparity_of(above.min())
    zz = depths(d)
    assert lower_median(zz, ~np.isnan(zz)) == med
    return int(ia), int(ib)


def _log_uniform(rng, hw, lo, hi):
    return (F(1) / np.exp(rng.uniform(np.log(lo), np.log(hi), hw)).astype(F)).astype(F)


def _frame(kind, hw, rng):
    """-> flat disparities [hw], planted pixel indices or None"""
    nan = F(np.nan)
    if kind == "heavy_tail":
        d = _log_uniform(rng, hw, 0.5, 50.0)
        return d, plant(d)
    if kind == "constant":
        return np.full(hw, F(0.4), F), None
    if kind == "two_values":
        d = np.full(hw, nan, F)
        perm = rng.permutation(hw)[:hw - hw % 2]
        d[perm[:len(perm) // 2]] = F(1.0)
        d[perm[len(perm) // 2:]] = F(0.25)
        return d, None
    if kind == "low_byte":
        steps = 8 * (rng.permutation(max(hw, 26)) % 26)[:hw]          # 2.0 + 0..200 floats: keys 0x400000xx
        table = {int(s): disparity_of(_ulps(F(2.0), int(s))) for s in np.unique(steps)}
        d = np.array([table[int(s)] for s in steps], F)
        return d, plant(d)
    if kind == "wide_exponent":
        d = (10.0 ** rng.uniform(-30, 3, hw)).astype(F)
        d[rng.permutation(hw)[:2]] = (F(0.0), F(1e-30))              # depth +inf is a valid key
        return d, None
    if kind == "scattered_nan":
        d = _log_uniform(rng, hw, 0.5, 50.0)
        d[rng.uniform(size=hw) < 0.3] = nan
        if np.isnan(d).all():
            d[0] = F(0.7)
        return d, None
    d = np.full(hw, nan, F)
    if kind == "one_valid":
        d[rng.integers(hw)] = F(0.5)
    elif kind == "two_valid":
        d[rng.permutation(hw)[:2]] = (F(0.25), F(1.0))               # the lower median 1.0 masks depth 4.0 out
    return d, None


@functools.lru_cache(maxsize=None)
def select_scene(h, w, seed=0, repeat=1, extra=2):
    """repeat x one frame of each kind (different seeds), then `extra` filler frames.  dict poses (identity), disps,
    mono [B,h,w], intrinsics [4], n, kinds [n], planted {frame: (ia, ib)}"""
    hw = h * w
    rng = np.random.default_rng(1000 * seed + hw)
    kinds = list(KINDS) * repeat
    n, B = len(kinds), len(kinds) + extra
    disps, mono = np.full((B, hw), FILL_DISP, F), np.full((B, hw), FILL_MONO, F)
    planted = {}
    for f, kind in enumerate(kinds):
        d, pl = _frame(kind, hw, rng)
        disps[f] = d
        if pl is not None:
            planted[f] = pl
        if kind in FLAT_TARGET:
            mono[f] = rng.uniform(0.5, 1.5, hw).astype(F)
        else:
            with np.errstate(invalid="ignore"):
                t = np.where(np.isfinite(d), d, rng.uniform(0.1, 1.0, hw)).astype(np.float64)
            mono[f] = ((t - rng.uniform(-0.05, 0.05)) / rng.uniform(0.5, 2.0)
                       * (1 + 0.02 * rng.standard_normal(hw))).astype(F)
    poses = np.zeros((B, 7), F)
    poses[:, 6] = 1
    for a in (disps, mono, poses):
        a.setflags(write=False)
    return dict(poses=poses, disps=disps.reshape(B, h, w), mono=mono.reshape(B, h, w), intrinsics=synth.camera(h, w),
                n=n, kinds=kinds, planted=planted, h=h, w=w)


@functools.lru_cache(maxsize=None)
def select_reference(h, w, seed=0, repeat=1, mono_thres=0.1):
    """the reference of glorie_dspo_prepare on select_scene (visible_num = 0, a self-pair edge per frame)"""
    s = select_scene(h, w, seed, repeat)
    ii = np.arange(s["n"], dtype=np.int64)
    return prepare(s["poses"], s["disps"], s["intrinsics"], s["mono"], s["n"], 0.05, 0, mono_thres, ii, ii,
                   tuple(max(a, b) for a, b in zip(kernel_bound("select"), kernel_bound("select_flat"))), flat=True)


def vmask_indices(s, seed=0):
    """one frame of every kind of a select_scene built with repeat >= 2, out of order and with the first named twice; the
    other copies and the filler frames are holes"""
    rng = np.random.default_rng(seed)
    rep = s["n"] // len(KINDS)
    assert rep >= 2
    ix = rng.permutation([k + len(KINDS) * int(rng.integers(rep)) for k in range(len(KINDS))]).astype(np.int64)
    return np.concatenate([ix, ix[:1]])


# ---- coupled scene ----------------------------------------------------------------------------------------------------------
# a slanted near plane that leaves the view on the left (Z = 1 / (1 + A x/z)) in front of a far plane at depth 7
COUPLED_PLANES = ((np.array([1.1, 0.05, 1.0]), 1.0), (np.array([0.0, 0.0, 1.0]), 7.0))
COUPLED_MONO_THRES = 0.06
COUPLED_N = 9                     # every frame of the stack is prepared; edges also name frames 9 and 11
PRIORS = ("half_cut", "clean", "anti", "structured", "noise2", "clean", "near_constant", "clean", "no_neighbour")
STRIPE = 0.62                     # frame 0: the columns from STRIPE * w on are scaled and fail the two-view filter


@functools.lru_cache(maxsize=None)
def coupled_scene(h, w, all_bad=False):
    """plane_graph(9, h, w) with the far plane; frame f carries the mono prior PRIORS[f].  Frame 0 loses a stripe of its
    near pixels to the two-view filter (their disparity is scaled), so that without the far pixels that 3 * median cuts
    away fewer than half remain; frame 8 is scaled as a whole and has no consistent neighbour.  all_bad: every prior is
    anti-correlated."""
    g = geom_ref.plane_graph(9, h, w, planes=COUPLED_PLANES)
    rng = np.random.default_rng(h * w)
    disps = g["disps"].copy()
    x = np.arange(w)[None, :].repeat(h, 0)
    disps[0][x >= int(STRIPE * w)] *= F(1.6)
    disps[8] *= F(1.7)
    yy, xx = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    mono = np.zeros_like(disps)
    for f in range(9):
        d = disps[f].astype(np.float64)
        kind = "anti" if all_bad else PRIORS[f]
        p = (d - 0.03 * (f - 3)) / (0.6 + 0.2 * f)
        if kind == "noise2":
            p = p * (1 + 0.02 * rng.standard_normal(d.shape))
        elif kind == "anti":
            p = 1.5 - p
        elif kind == "structured":
            p = p + 0.5 * d.mean() * np.sin(0.9 * xx + 0.4 * yy)
        elif kind == "near_constant":
            p = 1.0 + 0.03 * (0.5 * (d - d.mean()) / d.std() + 0.87 * rng.standard_normal(d.shape))
        mono[f] = p.astype(F)
    # every frame by itself, the graph's own pairs and - unless every frame is to be bad - frames beyond n (never bad)
    beyond = ([], []) if all_bad else ([9, 11, 1, 9], [9, 9, 11, 2])
    ii = np.concatenate([np.arange(COUPLED_N), beyond[0], g["ii"]]).astype(np.int64)
    jj = np.concatenate([np.arange(COUPLED_N), beyond[1], g["jj"]]).astype(np.int64)
    for a in (disps, mono):
        a.setflags(write=False)
    return dict(poses=g["poses"], disps=disps, mono=mono, intrinsics=g["intrinsics"][0].copy(), n=COUPLED_N, ii=ii, jj=jj,
                h=h, w=w)


def kernel_bound(cls):
    """the alignment error allowed to the kernel in scenes of class cls, (scale, shift) in units of kappa * 2^-24"""
    return tuple(MARGIN * b for b in F32_ERROR[cls])


@functools.lru_cache(maxsize=None)
def coupled_reference(h, w, mv_thresh, mono_thres=COUPLED_MONO_THRES, all_bad=False):
    s = coupled_scene(h, w, all_bad)
    return prepare(s["poses"], s["disps"], s["intrinsics"], s["mono"], s["n"], mv_thresh, 2, mono_thres, s["ii"], s["jj"],
                   kernel_bound("coupled"))


def threshold_band(s, r, mv_thresh):
    """pixels of the n prepared frames whose two-view count hangs on a depth difference within geom_ref.REL_BAND of the
    threshold (geom_ref.depth_filter64's float64 quantities)"""
    n = s["n"]
    _, edge = geom_ref.depth_filter64(s["poses"], s["disps"], s["intrinsics"], np.arange(n), r["thresh"].astype(np.float64))
    return edge


# ---- the float32 formulation's own error --------------------------------------------------------------------------------
COUPLED_RUNS = tuple((h, w, mv, all_bad) for (h, w) in COUPLED_SIZES for mv in (0.01, 0.05) for all_bad in (False, True)
                     if not (all_bad and mv == 0.01))


def class_errors(results):
    """results(scene, reference) -> (scale [n], shift [n]) of some float32 evaluation.  -> {class: (max scale error, max
    shift error, smallest kappa, largest kappa)} in units of kappa * 2^-24 over every frame the GPU tests compare"""
    acc = {}

    def add(cls, es, eq, kappa, sel):
        sel = sel & np.isfinite(kappa)
        if sel.any():
            a = acc.setdefault(cls, [0.0, 0.0, np.inf, 0.0])
            a[0], a[1] = max(a[0], np.nanmax(es[sel])), max(a[1], np.nanmax(eq[sel]))
            a[2], a[3] = min(a[2], kappa[sel].min()), max(a[3], kappa[sel].max())

    for (h, w) in PREPARE_SIZES:
        s, r = select_scene(h, w), select_reference(h, w)
        sc, sh = results(s, r)
        kinds = np.array(s["kinds"])
        for cls, flat in (("select", False), ("select_flat", True)):
            es, eq = align_errors(sc, sh, r["fit"], flat)
            sel = np.isin(kinds, FLAT_TARGET) if flat else ~np.isin(kinds, FLAT_TARGET + NO_FIT)
            add(cls, es, eq, r["fit"]["kappa"], sel)
    for (h, w, mv, all_bad) in COUPLED_RUNS:
        s, r = coupled_scene(h, w, all_bad), coupled_reference(h, w, mv, COUPLED_MONO_THRES, all_bad)
        es, eq = align_errors(*results(s, r), r["fit"])
        add("coupled", es, eq, r["fit"]["kappa"], np.ones(s["n"], bool))
    return {k: tuple(float(x) for x in v) for k, v in acc.items()}


def f32_errors():
    return class_errors(lambda s, r: align32(s["mono"][:s["n"]], s["disps"][:s["n"]], r["mask"])[:2])


def error_report(kernel=None):
    """the lines of profiles/dspo_prepare_error.txt; kernel = class_errors of the HIP entry (for the record only)"""
    lines = ["alignment error of common.align_scale_and_shift in float32 (CPU) against the float64 reference, max over the",
             "frames of the class, in units of kappa * 2^-24 (kappa = a00 a11 / det); bound = %g x that" % MARGIN]
    for cls, (es, eq, k0, k1) in f32_errors().items():
        for name, e, i in (("scale", es, 0), ("shift", eq, 1)):
            line = "%-12s %-5s kappa %8.3g .. %-8.3g float32 %6.3f  bound %7.3f" % (cls, name, k0, k1, e, MARGIN * F32_ERROR[cls][i])
            if kernel is not None:
                line += "  kernel %6.3f" % kernel[cls][i]
            lines.append(line)
    return lines


if __name__ == "__main__":
    print("\n".join(error_report()))
