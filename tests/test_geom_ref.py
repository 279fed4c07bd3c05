"""tests/geom_ref.py on the CPU: its two scenes reach the branches that the synthetic graphs of synth.py leave out, and the
float32 oracle of the geometry kernels (oracle/geom.py, oracle/se3.py: quaternion formulas, the ones the kernels restate)
agrees with geom_ref's float64 matrix reference, which states the same operations without them.

`PYTHONPATH=. python tests/test_geom_ref.py` prints the measured oracle-against-float64 errors (profiles/geom_oracle_error.txt)."""
import functools

import numpy as np
import pytest

import geom_ref
from oracle import geom as ogeom

# map sizes of tests/test_gpu_geom.py: 1 pixel, one ragged row, odd h*w below one workgroup, exactly one workgroup,
# one workgroup + 4 pixels, several workgroups
SHAPES = ((1, 1), (1, 7), (7, 9), (16, 16), (13, 20), (30, 40))
PLANE_SHAPES = ((7, 9), (13, 20), (24, 32))
K_GENERAL, K_PLANE = 6, 9

# worst |oracle32 - ref64| / max(1, |ref64|) over both scenes at all the shapes above, as measured here
# (profiles/geom_oracle_error.txt); the assertions allow 4x, for other seeds and another libm
MEASURED = dict(coords=1.212e-5, frame_distance=4.04e-7, iproj=2.25e-7)
MARGIN = 4.0
MAX_EXCLUDED = 0.005       # share of pixels that may sit within geom_ref.REL_BAND of a threshold


@functools.lru_cache(maxsize=None)
def scene(kind, h, w):
    g = geom_ref.general_graph(K_GENERAL, h, w) if kind == "general" else geom_ref.plane_graph(K_PLANE, h, w)
    K = g["K"]
    ii, jj = np.meshgrid(np.arange(K), np.arange(K), indexing="ij")
    g["all_ii"], g["all_jj"] = ii.reshape(-1).astype(np.int64), jj.reshape(-1).astype(np.int64)
    return g


SCENES = [("general", h, w) for h, w in SHAPES] + [("plane", h, w) for h, w in PLANE_SHAPES]


def rel_err(got, ref):
    return np.abs(got - ref) / np.maximum(1.0, np.abs(ref))


# ---- the comparisons: each returns (worst relative error, mismatches of the thresholded output, excluded share) ----------
@functools.lru_cache(maxsize=None)
def reproject_stats(kind, h, w):
    g = scene(kind, h, w)
    ii = np.concatenate([g["ii"], [1, 4]])            # + two stereo edges
    jj = np.concatenate([g["jj"], [1, 4]])
    c, v = ogeom.reproject(g["poses"], g["disps"], g["intrinsics"], ii, jj)
    c64, Z = geom_ref.reproject64(g["poses"], g["disps"], g["intrinsics"], ii, jj)
    on_clamp, on_valid = geom_ref.near(Z, 0.1), geom_ref.near(Z, 0.2)
    err = rel_err(c, c64)[~on_clamp]
    bad = ((v[..., 0] > 0) != (Z > 0.2)) & ~on_valid
    return dict(err=float(err.max()) if err.size else 0.0, mismatches=int(bad.sum()),
                excluded=float((on_clamp | on_valid).mean()), valid=v[..., 0], Z=Z)


@functools.lru_cache(maxsize=None)
def frame_distance_stats(kind, h, w, beta):
    g = scene(kind, h, w)
    got = ogeom.frame_distance(g["poses"], g["disps"], g["intrinsics"][0], g["all_ii"], g["all_jj"], beta)
    ref, ratio, Z = geom_ref.frame_distance64(g["poses"], g["disps"], g["intrinsics"][0], g["all_ii"], g["all_jj"], beta)
    on_z = geom_ref.near(Z, 0.25)
    # a term that flips at Z = 0.25 moves V / T and A / V of its pair: the pair is compared without it
    pair_ok = ~on_z.any((1, 2)) & ~geom_ref.near(ratio, 0.75)
    bad = ((got == 1000.0) != (ref == 1000.0)) & pair_ok
    both = pair_ok & (got != 1000.0) & (ref != 1000.0)
    err = rel_err(got, ref)[both]
    return dict(err=float(err.max()) if err.size else 0.0, mismatches=int(bad.sum()), excluded=float(on_z.mean()),
                excluded_pairs=int((~pair_ok).sum()), got=got)


@functools.lru_cache(maxsize=None)
def iproj_stats(kind, h, w):
    g = scene(kind, h, w)
    got = ogeom.iproj(g["poses"], g["disps"], g["intrinsics"][0])
    ref = geom_ref.iproj64(g["poses"], g["disps"], g["intrinsics"][0])
    return dict(err=float(rel_err(got, ref).max()), mismatches=0, excluded=0.0)


def depth_filter_inputs(g):
    ix = np.arange(g["K"], dtype=np.int64)           # every frame: both ends of the +-5 window are clipped
    thresh = (0.01 * (1.0 / g["disps"][ix]).mean((1, 2))).astype(np.float32) * 4
    return ix, thresh


@functools.lru_cache(maxsize=None)
def depth_filter_stats(kind, h, w):
    g = scene(kind, h, w)
    ix, thresh = depth_filter_inputs(g)
    got = ogeom.depth_filter(g["poses"], g["disps"], g["intrinsics"][0], ix, thresh)
    ref, edge = geom_ref.depth_filter64(g["poses"], g["disps"], g["intrinsics"][0], ix, thresh)
    return dict(err=0.0, mismatches=int(((got != ref) & ~edge).sum()), excluded=float(edge.mean()), got=got)


# ---- scene conditions -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("h,w", SHAPES[2:])
def test_general_graph_reaches_the_untested_branches(h, w):
    g = scene("general", h, w)
    q = g["poses"][:, 3:]
    assert np.all(q != 0) and (q[:, 3] < 0).any() and (q[:, 3] > 0).any()
    assert np.allclose(np.linalg.norm(q, axis=1), 1.0, atol=1e-6)
    intr = g["intrinsics"]
    assert all(np.all(intr[a] != intr[b]) for a in range(g["K"]) for b in range(a))
    s = reproject_stats("general", h, w)
    valid = s["valid"][:len(g["ii"])]                  # without the stereo edges
    assert 0.85 <= valid.mean() <= 0.98
    assert valid.mean((1, 2)).min() < 0.8
    assert (s["Z"][:len(g["ii"])] < 0.1).mean() >= 0.02


@pytest.mark.parametrize("beta", [0.3, 0.75])
def test_general_graph_frame_distance_is_mixed(beta):
    got = frame_distance_stats("general", 30, 40, beta)["got"]
    assert (got == 1000.0).any() and (got < 1000.0).any()


def test_plane_graph_depth_filter_counts_cover_0_to_6():
    got = depth_filter_stats("plane", 24, 32)["got"]
    assert set(np.unique(got).tolist()) == set(range(7))
    assert (got >= 2).mean() > 0.5
    g = scene("plane", 24, 32)
    assert g["intrinsics"][0, 0] != g["intrinsics"][0, 1] and np.all(g["intrinsics"] == g["intrinsics"][0])


# ---- the float32 oracle against the float64 matrix reference ------------------------------------------------------------------
def _check(s, bound):
    print(s["err"], s["mismatches"], s["excluded"])
    assert s["err"] <= bound
    assert s["mismatches"] == 0
    assert s["excluded"] <= MAX_EXCLUDED


@pytest.mark.parametrize("kind,h,w", SCENES)
def test_oracle_reproject_matches_float64(kind, h, w):
    _check(reproject_stats(kind, h, w), MARGIN * MEASURED["coords"])


@pytest.mark.parametrize("beta", [0.3, 0.75])
@pytest.mark.parametrize("kind,h,w", SCENES)
def test_oracle_frame_distance_matches_float64(kind, h, w, beta):
    s = frame_distance_stats(kind, h, w, beta)
    _check(s, MARGIN * MEASURED["frame_distance"])
    assert s["excluded_pairs"] <= 1


@pytest.mark.parametrize("kind,h,w", SCENES)
def test_oracle_iproj_matches_float64(kind, h, w):
    _check(iproj_stats(kind, h, w), MARGIN * MEASURED["iproj"])


@pytest.mark.parametrize("kind,h,w", SCENES[2:])
def test_oracle_depth_filter_matches_float64(kind, h, w):
    _check(depth_filter_stats(kind, h, w), 0.0)


def main():
    print("float32 oracle (oracle/geom.py) against the float64 matrix reference (tests/geom_ref.py)")
    print("err = max |oracle32 - ref64| / max(1, |ref64|); mismatches of the thresholded output outside the band;")
    print(f"excluded = share of pixels within {geom_ref.REL_BAND:g} (relative) of a threshold")
    worst = {}
    rows = [("coords", reproject_stats, ()), ("frame_distance", frame_distance_stats, (0.3,)),
            ("frame_distance", frame_distance_stats, (0.75,)), ("iproj", iproj_stats, ()),
            ("depth_filter", depth_filter_stats, ())]
    for name, fn, extra in rows:
        for kind, h, w in SCENES:
            if name == "depth_filter" and h * w < 63:
                continue
            s = fn(kind, h, w, *extra)
            worst[name] = max(worst.get(name, 0.0), s["err"])
            print(f"{name:15s} {kind:8s} {h:2d}x{w:<2d} {'beta=%g' % extra[0] if extra else '':10s} err {s['err']:.3e}  "
                  f"mismatches {s['mismatches']}  excluded {s['excluded']:.2e}")
    for name, e in worst.items():
        print(f"worst {name:15s} {e:.3e}")


if __name__ == "__main__":
    main()
