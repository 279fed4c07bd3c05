"""Float64 restatement of one DSPO stage-2 iteration, per frame, and the scenes it is tested on (test infrastructure).

glorie_dspo_scale_shift (csrc/dspo.hip) optimises the disparities of every frame with outgoing edges together with that
frame's scale and shift of the mono prior.  oracle/dspo.py restates the reference's DENSE formulation (one 2M x 2M
Cholesky) in numpy; this module restates the same step from the formulas in the block-diagonal form, in float64 from the
fp32 inputs, with the projection of tests/geom_ref.py (4 x 4 matrices, scipy rotations - no quaternion formula):

  per edge n = (i -> j), pixel p     X1 = Tij (ray_i(p), d_i(p)),  Z = X1.z,  coords = K_j (X1.xy / (Z < 0.1 ? 1 : Z))
                                     valid = Z > 0.2,  w = 0.001 valid weight,  r = target - coords
                                     Jz = d coords / d disparity = K_j ((t.xy - X1.xy t.z / Z) / Z),  t = Tij[:3, 3]
  per frame k (slot s), pixel p      Cp = sum_n w Jz^2, Wp = sum_n w r Jz over the ENABLED edges leaving k
                                     prior: sa = sqrt(alpha) (vmask ? 10 : 1), invalid = mono < 1e-6 (decided in fp32)
                                            Jd = invalid and vmask ? 0 : sa,  Js = invalid ? 0 : -mono sa,  Jq = invalid ? 0 : -sa
                                            rd = sqrt(alpha) (d - (scale mono + shift))
                                     C = Cp + Jd^2 + eta[s],  W = Wp - Jd rd,  Q = 1 / C,  e = (Js Jd, Jq Jd)
  ten sums over p                    H = [Js^2, Js Jq, Jq^2],  G = e Q e^T,  u = -(Js, Jq) rd,  g = e Q W
  2 x 2 system                       S = H (1 + lm) + ep (diagonal only, BEFORE the Schur complement) - G,  b = u - g
                                     positive definite  <=>  S11 > 0 and S22 - S12^2 / S11 > 0
  step                               (ds, dq) = S^-1 b, or 0 for EVERY frame if any enabled frame's S is not positive definite
                                     dz = Q (W - e . (ds, dq)),  d <- max(d + dz, 0)

The slots are kx = sorted(unique(ii)) over all edges, enabled or not; eta[s] belongs to slot s; a frame without an
enabled outgoing edge is skipped and keeps its state.  The functions prefixed with an underscore are the places where a
kernel can go wrong; tests/test_dspo_ref.py replaces them one at a time in a copy of this module to show that the
comparison would notice.
"""
import functools
from collections import namedtuple

import numpy as np

import geom_ref
from geom_ref import REL_BAND, STEREO, near, relative_matrix, reproject64

F = np.float32
VALID_Z = 0.2                # a transformed point counts where Z > VALID_Z
CLAMP_Z = 0.1                # Z < CLAMP_Z is replaced by 1 before the division (inside reproject64)

Step = namedtuple("Step", "disps scales shifts raw dz systems failed enabled kx")


# ---- one iteration ----------------------------------------------------------------------------------------------------------
def _project(poses, disps, intr, ii, jj):
    """-> coords [N,HW,2], Z [N,HW], t [N,3] (translation of the edge's transform)"""
    coords, Z = reproject64(poses, disps, intr, ii, jj)
    t = np.array([(STEREO if int(i) == int(j) else relative_matrix(poses, int(i), int(j)))[:3, 3] for i, j in zip(ii, jj)])
    N = len(ii)
    return coords.reshape(N, -1, 2), Z.reshape(N, -1), t.reshape(N, 3)


def _prior_jacobians(mono32, vd, sa0):
    invalid = mono32 < F(1e-6)                                  # taken on the fp32 value, as the kernel does
    m = mono32.astype(np.float64)
    sa = sa0 * np.where(vd, 10.0, 1.0)
    Jd = np.where(invalid & vd, 0.0, sa)
    Js = np.where(invalid, 0.0, -m * sa)
    Jq = np.where(invalid, 0.0, -sa)
    return Jd, Js, Jq


def _eta_row(eta, s, k):
    return eta[s]


def _reduce(v, lm, ep):
    """ten sums -> S11, S12, S22, b1, b2 (damping before the Schur complement)"""
    H11, H22 = v[0] * (1.0 + lm) + ep, v[2] * (1.0 + lm) + ep
    return np.array([H11 - v[3], v[1] - v[4], H22 - v[5], v[6] - v[8], v[7] - v[9]])


def _resolve_failure(dx, bad):
    """bad [M]: enabled frames whose system is not positive definite.  One of them zeroes every frame's step."""
    return np.zeros_like(dx) if bad.any() else dx


def _clamp(d):
    return np.maximum(d, 0.0)


def stage2_iteration(target, weight, eta, poses, disps, intr, ii, jj, mono, scales, shifts, vmask, edge_on=None,
                     lm=1e-4, ep=0.1, alpha=0.01):
    """target / weight [N,h,w,2], eta [M,h,w], poses [B,7], disps / mono / vmask [B,h,w], intr [B,4], scales / shifts [B].
    -> Step(disps, scales, shifts [float64, same shapes], raw = disps + dz before the clamp, dz [M,HW] (0 in the rows of
    skipped frames), systems [M,5] = S11 S12 S22 b1 b2 (nan where skipped), failed, enabled [M], kx [M])"""
    lm, ep, sa0 = float(F(lm)), float(F(ep)), float(np.sqrt(np.float64(F(alpha))))     # the entry point takes C floats
    ii, jj = np.asarray(ii, np.int64), np.asarray(jj, np.int64)
    B, h, w = np.shape(disps)
    HW, N = h * w, len(ii)
    on = np.ones(N, bool) if edge_on is None else np.asarray(edge_on).astype(bool)
    kx = np.array(sorted(set(ii.tolist())), np.int64)
    M = len(kx)
    eta = np.asarray(eta, np.float64).reshape(len(eta), HW)
    d0 = np.asarray(disps, np.float64).reshape(B, HW)
    s0, q0 = np.asarray(scales, np.float64), np.asarray(shifts, np.float64)
    mono32 = np.asarray(mono, F).reshape(B, HW)
    vm = np.asarray(vmask).astype(bool).reshape(B, HW)
    tg = np.asarray(target, np.float64).reshape(N, HW, 2)
    wg = np.asarray(weight, np.float64).reshape(N, HW, 2)
    intr = np.asarray(intr, F)

    coords, Z, t = _project(poses, np.asarray(disps, F), intr, ii, jj)
    Zc = np.where(Z < CLAMP_Z, 1.0, Z)
    valid = (Z > VALID_Z).astype(np.float64)
    kj = intr[jj].astype(np.float64)                            # the TARGET frame's fx fy cx cy
    r = tg - coords
    Jz = np.stack([(kj[:, None, 0] * t[:, None, 0] - (coords[..., 0] - kj[:, None, 2]) * t[:, None, 2]) / Zc,
                   (kj[:, None, 1] * t[:, None, 1] - (coords[..., 1] - kj[:, None, 3]) * t[:, None, 2]) / Zc], -1)
    wgt = 0.001 * valid[..., None] * wg
    Cn = (wgt * Jz * Jz).sum(-1)
    Wn = (wgt * r * Jz).sum(-1)

    enabled = np.zeros(M, bool)
    systems = np.full((M, 5), np.nan)
    dx = np.zeros((M, 2))
    Qs, Ws, es = np.zeros((M, HW)), np.zeros((M, HW)), np.zeros((M, HW, 2))
    bad = np.zeros(M, bool)
    for s, k in enumerate(kx):
        mine = on & (ii == k)
        if not mine.any():
            continue
        enabled[s] = True
        Jd, Js, Jq = _prior_jacobians(mono32[k], vm[k], sa0)
        rd = sa0 * (d0[k] - (s0[k] * mono32[k].astype(np.float64) + q0[k]))
        C = Cn[mine].sum(0) + Jd * Jd + _eta_row(eta, s, k)
        W = Wn[mine].sum(0) - Jd * rd
        Q = 1.0 / C
        e1, e2 = Js * Jd, Jq * Jd
        v = np.array([(Js * Js).sum(), (Js * Jq).sum(), (Jq * Jq).sum(),
                      (e1 * Q * e1).sum(), (e1 * Q * e2).sum(), (e2 * Q * e2).sum(),
                      -(Js * rd).sum(), -(Jq * rd).sum(), (e1 * Q * W).sum(), (e2 * Q * W).sum()])
        S11, S12, S22, b1, b2 = systems[s] = _reduce(v, lm, ep)
        if S11 > 0.0 and S22 - S12 * S12 / S11 > 0.0:
            det = S11 * S22 - S12 * S12
            dx[s] = (S22 * b1 - S12 * b2) / det, (S11 * b2 - S12 * b1) / det
        else:
            bad[s] = True
        Qs[s], Ws[s], es[s] = Q, W, np.stack([e1, e2], -1)
    dx = _resolve_failure(dx, bad)

    dz = np.zeros((M, HW))
    d1, raw, s1, q1 = d0.copy(), d0.copy(), s0.copy(), q0.copy()
    for s, k in enumerate(kx):
        if not enabled[s]:
            continue
        dz[s] = Qs[s] * (Ws[s] - es[s] @ dx[s])
        raw[k] = d0[k] + dz[s]
        d1[k] = _clamp(raw[k])
        s1[k] += dx[s, 0]
        q1[k] += dx[s, 1]
    return Step(d1.reshape(B, h, w), s1, q1, raw.reshape(B, h, w), dz, systems, bool(bad.any()), enabled, kx)


def scene_args(g):
    """the positional arguments of stage2_iteration (and of oracle.dspo.ba_with_scale_shift) from a scene"""
    return (g["target"], g["weight_hw2"], g["eta"], g["poses"], g["disps"], g["intrinsics"], g["ii"], g["jj"], g["mono"],
            g["scales"], g["shifts"], g["vmask"])


def chain(n_iters, g, edge_on=None, lm=1e-4, ep=0.1, alpha=0.01):
    """n_iters iterations with the state rounded to fp32 in between, which is what the kernel's state is.
    -> list of Step, one per iteration; the last one's disps / scales / shifts are the float64 values before rounding"""
    d, s, q = g["disps"], g["scales"], g["shifts"]
    steps = []
    for _ in range(n_iters):
        st = stage2_iteration(g["target"], g["weight_hw2"], g["eta"], g["poses"], d, g["intrinsics"], g["ii"], g["jj"],
                              g["mono"], s, q, g["vmask"], edge_on=edge_on, lm=lm, ep=ep, alpha=alpha)
        steps.append(st)
        d, s, q = st.disps.astype(F), st.scales.astype(F), st.shifts.astype(F)
    return steps


# ---- the dense oracle on the same scene ------------------------------------------------------------------------------------
def filtered(g, edge_on):
    """the scene with the disabled edges physically removed and eta restricted to the slots that remain"""
    keep = np.asarray(edge_on).astype(bool)
    g2 = dict(g)
    for key in ("ii", "jj", "target", "weight_hw2", "noise_hw2"):
        g2[key] = g[key][keep]
    kx_all = sorted(set(g["ii"].tolist()))
    g2["eta"] = g["eta"][[kx_all.index(f) for f in sorted(set(g2["ii"].tolist()))]]
    return g2


def oracle_chain(n_iters, g, dtype, edge_on=None, lm=1e-4, ep=0.1, alpha=0.01):
    """oracle.dspo.ba_with_scale_shift n_iters times (dense formulation; it has no edge mask, so masked edges are removed)
    -> disps, scales, shifts, dz of the last iteration [M',HW] (M' = frames with enabled edges)"""
    from oracle import dspo as odspo
    if edge_on is not None:
        g = filtered(g, edge_on)
    d, s, q = g["disps"], g["scales"], g["shifts"]
    dz = None
    for _ in range(n_iters):
        d, s, q, dz = odspo.ba_with_scale_shift(g["target"], g["weight_hw2"], g["eta"], g["poses"], d, g["intrinsics"],
                                                g["ii"], g["jj"], g["mono"], s, q, g["vmask"], lm=lm, ep=ep, alpha=alpha,
                                                dtype=dtype)
    return np.asarray(d, np.float64), np.asarray(s, np.float64), np.asarray(q, np.float64), np.asarray(dz, np.float64)


# ---- scenes -----------------------------------------------------------------------------------------------------------------
def retarget(g):
    """targets = float64 reprojection of the scene's own state + its noise"""
    coords, _ = reproject64(g["poses"], g["disps"], g["intrinsics"], g["ii"], g["jj"])
    g["target"] = (coords + g["noise_hw2"]).astype(F)
    return g


def build_scene(kind, K, h, w, radius=2, seed=None, drop=(), stereo=(), perm_seed=None):
    """kind "general" | "plane": geom_ref.general_graph | plane_graph with their default seeds unless one is given.
    drop: frames that lose every outgoing edge (B > M, eta keeps the remaining slots); stereo: frames that get an
    ii == jj edge appended; perm_seed: the edge list shuffled.  Mono prior, start scale / shift and vmask as problem():
    10 % zero mono, 70 % vmask."""
    gen = {"general": geom_ref.general_graph, "plane": geom_ref.plane_graph}[kind]
    g = dict(gen(K, h, w, radius=radius) if seed is None else gen(K, h, w, seed=seed, radius=radius))
    seed = 0 if seed is None else seed
    rng = np.random.default_rng(seed)
    ii, jj = g["ii"], g["jj"]
    weight = g.pop("weight").transpose(0, 2, 3, 1)
    noise = g.pop("noise").transpose(0, 2, 3, 1)
    if len(stereo):
        extra = np.asarray(stereo, np.int64)
        ers = np.random.default_rng(seed + 77)
        ii, jj = np.concatenate([ii, extra]), np.concatenate([jj, extra])
        weight = np.concatenate([weight, ers.uniform(0.0, 1.0, (len(extra), h, w, 2)).astype(F)])
        noise = np.concatenate([noise, ers.normal(0.0, 0.5, (len(extra), h, w, 2)).astype(F)])
    order = np.flatnonzero(~np.isin(ii, np.asarray(drop, np.int64)))
    if perm_seed is not None:
        order = np.random.default_rng(perm_seed).permutation(order)
    g["ii"], g["jj"] = np.ascontiguousarray(ii[order]), np.ascontiguousarray(jj[order])
    g["weight_hw2"] = np.ascontiguousarray(weight[order])
    g["noise_hw2"] = np.ascontiguousarray(noise[order])
    g["eta"] = np.ascontiguousarray(g["eta"][sorted(set(g["ii"].tolist()))])
    retarget(g)
    s = rng.uniform(0.5, 2.0, K).astype(F)
    q = rng.uniform(-0.05, 0.05, K).astype(F)
    mono = (g["disps"] - q[:, None, None]) / s[:, None, None] * (1 + 0.02 * rng.standard_normal(g["disps"].shape))
    mono[rng.uniform(size=mono.shape) < 0.1] = 0.0
    g["mono"] = mono.astype(F)
    g["scales"] = (s * rng.uniform(0.9, 1.1, K)).astype(F)
    g["shifts"] = (q + rng.uniform(-0.01, 0.01, K)).astype(F)
    g["vmask"] = rng.uniform(size=g["disps"].shape) < 0.7
    return g


def clamp_scene():
    """plane_graph(6,7,9): rows 2..3 of frame 3 sit at disparity 1e-3 without a mono prior and outside vmask, so the prior
    pulls them to the frame's shift and the reprojection decides the rest; most of the 18 pixels end below zero"""
    g = build_scene("plane", 6, 7, 9)
    for key, val in (("disps", 1e-3), ("mono", 0.0), ("vmask", False)):
        g[key] = g[key].copy()
        g[key][3, 2:4] = val
    return retarget(g)


def bad_frame_scene(K, h, w, frame):
    """mono == 0 on one frame: its Js vanishes, so with ep = 0 its S11 is an exact 0.0 and the factorisation fails"""
    g = build_scene("plane", K, h, w)
    g["mono"] = g["mono"].copy()
    g["mono"][frame] = 0.0
    return g


SIZES = ((6, 7, 9), (7, 16, 20), (5, 17, 15))      # one ragged chunk of 256 pixels, two chunks, two chunks and odd sizes


def gap_frames(K):
    return (2, K - 1)                               # an interior frame and the last one


def touching(g, frame):
    """edge mask: off for every edge that starts or ends at `frame`"""
    return (g["ii"] != frame) & (g["jj"] != frame)


# name -> (builder, iterations, kwargs of stage2_iteration): every scene that tests/test_gpu_dspo_stage2.py runs, and
# "gapped-*" (gap and stereo edges together) for the comparison with the oracle in tests/test_dspo_ref.py
SCENES = {}
for _K, _h, _w in SIZES:
    for _kind in ("general", "plane"):
        SCENES[f"{_kind}-{_K}x{_h}x{_w}"] = (functools.partial(build_scene, _kind, _K, _h, _w), 3, {})
    SCENES[f"gapped-{_K}x{_h}x{_w}"] = (functools.partial(build_scene, "general", _K, _h, _w, drop=gap_frames(_K),
                                                         stereo=(1, 3)), 2, {})
    SCENES[f"gap-{_K}x{_h}x{_w}"] = (functools.partial(build_scene, "general", _K, _h, _w, drop=gap_frames(_K)), 2, {})
SCENES["stereo-7x16x20"] = (functools.partial(build_scene, "general", 7, 16, 20, stereo=(1, 3)), 2, {})
SCENES["stereo-perm-7x16x20"] = (functools.partial(build_scene, "general", 7, 16, 20, stereo=(1, 3), perm_seed=5), 2, {})
SCENES["clamp"] = (clamp_scene, 1, {})
for _K, _h, _w in ((6, 7, 9), (27, 5, 6)):
    for _ep in (0.0, 0.1):
        SCENES[f"badframe-K{_K}-ep{_ep}"] = (functools.partial(bad_frame_scene, _K, _h, _w, 2), 1, dict(ep=_ep))
SCENES["long-300x3x4"] = (functools.partial(build_scene, "plane", 300, 3, 4, radius=1), 1, {})


def _mask_general(g):
    return touching(g, 2)


SCENES["masked-7x16x20"] = (functools.partial(build_scene, "general", 7, 16, 20), 1, dict(edge_on=_mask_general))


@functools.lru_cache(maxsize=None)
def get(name):
    """-> (scene, kwargs, list of Step).  Built once per process and shared: treat everything in it as read-only."""
    builder, iters, kw = SCENES[name]
    g = builder()
    kw = dict(kw)
    if callable(kw.get("edge_on")):
        kw["edge_on"] = kw["edge_on"](g)
    return g, kw, chain(iters, g, **kw)


def firm(g, steps=(), edge_on=None):
    """No transformed point lies within REL_BAND (relative) of the Z thresholds 0.1 and 0.2, in the scene's own state and in
    the input state of every further iteration of `steps` (a chain): every validity decision of the kernel is then the
    reference's.  A single flipped validity changes a frame's sums, so the allowed share in the band is zero; a scene
    that violates it needs another seed, not a narrower band.  -> the shares of the first iteration's points below 0.1,
    in (0.1, 0.2) and behind the camera."""
    on = np.ones(len(g["ii"]), bool) if edge_on is None else np.asarray(edge_on).astype(bool)
    shares = None
    for d in [g["disps"]] + [st.disps.astype(F) for st in list(steps)[:-1]]:
        _, Z = reproject64(g["poses"], np.asarray(d, F), g["intrinsics"], g["ii"][on], g["jj"][on])
        for thr in (CLAMP_Z, VALID_Z):
            n = int(near(Z, thr).sum())
            assert n == 0, f"{n} transformed points within {REL_BAND} (relative) of Z = {thr}"
        if shares is None:
            shares = dict(below=float((Z < CLAMP_Z).mean()), between=float(((Z > CLAMP_Z) & (Z < VALID_Z)).mean()),
                          behind=float((Z < 0).mean()))
    return shares
