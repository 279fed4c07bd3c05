"""Pins tests/dspo_ref.py (the float64 per-frame restatement of DSPO stage 2) without a GPU: agreement with the dense
oracle, the failure decision, firmness of every scene the GPU tests use, and - on copies of the reference with one
deliberate error each - that the GPU comparison would notice such an error in the kernel."""
import importlib.util

import numpy as np
import pytest

import dspo_ref as R
from geom_ref import _rays, reproject64

ATOL = 2e-5                   # test_stage2_matches_dense_oracle_at_long_graph_shapes: scales, shifts and disparities
ORACLE_TOL = 2e-6             # reference against the float64 oracle; what is left is the oracle's fp32 relative pose


@pytest.fixture(scope="module")
def oracle():
    """name -> {dtype: (disps, scales, shifts, dz)} of the dense oracle, computed once per scene"""
    cache = {}

    def run(name, dtype):
        if (name, dtype) not in cache:
            g, kw, steps = R.get(name)
            cache[(name, dtype)] = R.oracle_chain(len(steps), g, dtype, **kw)
        return cache[(name, dtype)]
    return run


def gpu_bounds(name, oracle):
    """the bound the GPU test holds the kernel to on this scene: max(1.5 e_ref, atol) for disps, scales, shifts"""
    g, kw, steps = R.get(name)
    last = steps[-1]
    o32 = oracle(name, np.float32)
    return [max(1.5 * float(np.abs(a - b).max()), ATOL) for a, b in zip((last.disps, last.scales, last.shifts), o32)]


@pytest.mark.parametrize("name", sorted(R.SCENES))
def test_reference_matches_float64_oracle(name, oracle):
    g, kw, steps = R.get(name)
    last = steps[-1]
    od, os_, oq, odz = oracle(name, np.float64)
    for what, a, b in (("disps", last.disps, od), ("scales", last.scales, os_), ("shifts", last.shifts, oq),
                       ("dz", last.dz[last.enabled], odz)):
        err = float(np.abs(a - b).max())
        assert err <= ORACLE_TOL, (name, what, err)


def test_reference_matches_float64_oracle_on_the_arc():
    """the friendly scene of tests/test_gpu_dspo.py::problem, two iterations"""
    from test_gpu_dspo import problem
    g = problem()
    steps = R.chain(2, g)
    o = R.oracle_chain(2, g, np.float64)
    for a, b in zip((steps[-1].disps, steps[-1].scales, steps[-1].shifts), o):
        assert float(np.abs(a - b).max()) <= ORACLE_TOL


@pytest.mark.parametrize("name", [n for n in sorted(R.SCENES) if n.startswith("badframe")])
def test_failure_decision_is_the_oracles(name, oracle):
    g, kw, steps = R.get(name)
    st = steps[0]
    for dtype in (np.float32, np.float64):
        od, os_, oq, _ = oracle(name, dtype)
        oracle_failed = np.array_equal(os_, g["scales"]) and np.array_equal(oq, g["shifts"])
        assert st.failed == oracle_failed == (kw["ep"] == 0.0)
    bad = int(np.flatnonzero(st.kx == 2)[0])
    if st.failed:
        assert st.systems[bad, 0] == 0.0 and int((~(st.systems[:, 0] > 0)).sum()) == 1      # one frame, an exact zero
        assert np.array_equal(st.scales, g["scales"]) and np.array_equal(st.shifts, g["shifts"])
        assert float(np.abs(st.disps - g["disps"]).max()) > 1e-3                               # dz = Q W is applied
    else:
        assert st.scales[2] == g["scales"][2] and st.shifts[2] == g["shifts"][2]               # b = 0: an exact zero step
        others = st.kx != 2
        assert (np.abs(st.scales - g["scales"])[st.kx[others]] > 1e-4).all()


@pytest.mark.parametrize("name", sorted(R.SCENES))
def test_scenes_are_firm(name):
    g, kw, steps = R.get(name)
    shares = R.firm(g, steps, kw.get("edge_on"))
    if name.startswith(("general", "gap", "stereo", "masked")):
        assert shares["below"] > 0.01 and shares["between"] > 0.002 and shares["behind"] > 0.01, shares


def test_gapped_and_masked_frames_keep_their_state():
    for name in ("gap-6x7x9", "gapped-7x16x20"):
        g, kw, steps = R.get(name)
        last = steps[-1]
        assert len(last.kx) == g["K"] - 2 and g["eta"].shape[0] == g["K"] - 2
        for f in R.gap_frames(g["K"]):
            assert np.array_equal(last.disps[f], g["disps"][f]) and last.scales[f] == g["scales"][f]
    g, kw, steps = R.get("masked-7x16x20")
    st = steps[0]
    assert not st.enabled[2] and st.enabled.sum() == 6 and np.array_equal(st.disps[2], g["disps"][2])
    # the mask is the physically filtered graph; eta keeps the unmasked slot order
    g2 = R.filtered(g, kw["edge_on"])
    assert g2["eta"].shape[0] == 6 and np.array_equal(g2["eta"][2], g["eta"][3])
    st2 = R.chain(1, g2)[0]
    for a, b in zip((st.disps, st.scales, st.shifts), (st2.disps, st2.scales, st2.shifts)):
        assert np.array_equal(a, b)
    off = R.chain(1, g, edge_on=np.zeros(len(g["ii"]), bool))[0]
    assert not off.failed and np.array_equal(off.disps, g["disps"]) and np.array_equal(off.scales, g["scales"])


def test_edge_order_does_not_matter_to_the_reference():
    a, b = R.get("stereo-7x16x20")[2][-1], R.get("stereo-perm-7x16x20")[2][-1]
    assert float(np.abs(a.disps - b.disps).max()) < 1e-12 and float(np.abs(a.scales - b.scales).max()) < 1e-12


def test_clamp_scene_clamps():
    g, kw, steps = R.get("clamp")
    raw = steps[0].raw[3, 2:4].reshape(-1)
    assert raw.size == 18 and (g["disps"][3, 2:4] == np.float32(1e-3)).all()
    assert int((raw < -1e-4).sum()) >= 5 and int((raw > 1e-4).sum()) >= 1
    assert float((np.abs(raw) <= 1e-4).mean()) <= 0.2
    assert (steps[0].disps[3, 2:4].reshape(-1)[raw < 0] == 0.0).all()


# ---- mutations: one deliberate error each, in a copy of the reference ------------------------------------------------------
def _copy():
    spec = importlib.util.spec_from_file_location("dspo_ref_mutant", R.__file__)
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def _damping_after_schur(m):
    def reduce(v, lm, ep):
        return np.array([(v[0] - v[3]) * (1.0 + lm) + ep, v[1] - v[4], (v[2] - v[5]) * (1.0 + lm) + ep,
                         v[6] - v[8], v[7] - v[9]])
    m._reduce = reduce


def _valid_above_clamp(m):
    m.VALID_Z = m.CLAMP_Z


def _stereo_without_baseline(m):
    def project(poses, disps, intr, ii, jj):
        coords, Z, t = R._project(poses, disps, intr, ii, jj)
        _, h, w = disps.shape
        for n in np.flatnonzero(np.asarray(ii) == np.asarray(jj)):
            _, x, y = _rays(h, w, intr[ii[n]], disps[ii[n]])
            coords[n, :, 0], coords[n, :, 1], Z[n], t[n] = x.reshape(-1), y.reshape(-1), 1.0, 0.0
        return coords, Z, t
    m._project = project


def _jd_kept_for_invalid_masked(m):
    def prior(mono32, vd, sa0):
        _, Js, Jq = R._prior_jacobians(mono32, vd, sa0)
        return sa0 * np.where(vd, 10.0, 1.0), Js, Jq
    m._prior_jacobians = prior


def _eta_by_frame(m):
    m._eta_row = lambda eta, s, k: eta[min(k, len(eta) - 1)]


def _source_intrinsics(m):
    def project(poses, disps, intr, ii, jj):
        coords, Z, t = R._project(poses, disps, intr, ii, jj)
        for n, (i, j) in enumerate(zip(ii, jj)):
            swapped = np.array(intr)
            swapped[j] = intr[i]
            coords[n] = reproject64(poses, disps, swapped, [i], [j])[0].reshape(-1, 2)
        return coords, Z, t
    m._project = project


def _no_clamp(m):
    m._clamp = lambda d: d


def _local_failure(m):
    m._resolve_failure = lambda dx, bad: dx


MUTATIONS = {
    "damping-after-schur": (_damping_after_schur, ("plane-7x16x20", "general-7x16x20", "long-300x3x4")),
    "valid-at-0.1": (_valid_above_clamp, ("general-7x16x20", "general-5x17x15")),
    "stereo-zero-baseline": (_stereo_without_baseline, ("stereo-7x16x20",)),
    "jd-not-zeroed": (_jd_kept_for_invalid_masked, ("general-6x7x9", "plane-7x16x20")),
    "eta-by-frame": (_eta_by_frame, ("gap-6x7x9", "gap-7x16x20")),
    "source-intrinsics": (_source_intrinsics, ("general-6x7x9", "general-7x16x20")),
    "no-clamp": (_no_clamp, ("clamp",)),
    "local-failure": (_local_failure, ("badframe-K6-ep0.0", "badframe-K27-ep0.0")),
}


@pytest.mark.parametrize("mutation", sorted(MUTATIONS))
def test_reference_tells_a_wrong_kernel(mutation, oracle):
    """each mutation moves disparities, scales or shifts of at least one GPU-test scene by more than ten times the bound
    that the GPU test applies to that quantity on that scene"""
    mutate, names = MUTATIONS[mutation]
    m = _copy()
    mutate(m)
    factors = {}
    for name in names:
        g, kw, steps = R.get(name)
        wrong = m.chain(len(steps), g, **kw)[-1]
        right = steps[-1]
        bounds = gpu_bounds(name, oracle)
        factors[name] = max(float(np.abs(a - b).max()) / bound for a, b, bound in
                            zip((wrong.disps, wrong.scales, wrong.shifts), (right.disps, right.scales, right.shifts), bounds))
    print(mutation, {k: round(v, 1) for k, v in factors.items()})
    assert max(factors.values()) > 10.0, (mutation, factors)
