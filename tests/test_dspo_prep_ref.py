"""The reference of the depth_scale preparation (tests/dspo_prep_ref.py) and the preconditions that the GPU tests of
csrc/dspo_prep.hip rest on: the scenes make the median observable, no frame decides the edge filter by rounding, and the
alignment bound is the float32 formulation's own error."""
import os

import numpy as np
import pytest
import torch

import dspo_prep_ref as R
import geom_ref

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SELECT_SCENES = [(h, w, 1) for (h, w) in R.PREPARE_SIZES] + [(h, w, 2) for (h, w) in R.VMASK_SIZES] + [(7, 9, 8)]


@pytest.mark.parametrize("h,w,repeat", SELECT_SCENES)
def test_median_is_torch_nanmedian_and_scenes_are_what_they_claim(h, w, repeat):
    s, r = R.select_scene(h, w, 0, repeat), R.select_reference(h, w, 0, repeat)
    hw = h * w
    z = torch.from_numpy(np.where(r["valid"], r["z"], np.float32(np.nan)).reshape(s["n"], hw))
    want = torch.nanmedian(z, dim=1).values.numpy()
    assert np.array_equal(r["median"], want, equal_nan=True)
    assert r["count"].min() >= 0                       # visible_num = 0: every non-NaN depth is a key
    assert np.array_equal(r["valid"], ~np.isnan(r["z"]))
    for f, kind in enumerate(s["kinds"]):
        m, nv = r["mask"][f], int(r["valid"][f].sum())
        d = s["disps"][f]
        if kind == "constant":
            assert m.all() and len(np.unique(d)) == 1
        elif kind == "two_values":
            assert nv % 2 == 0 and nv >= hw - 1 and r["median"][f] == 1.0
            assert np.array_equal(m, d == 1.0) and (d == 0.25).sum() == nv // 2
        elif kind == "low_byte":
            rest = np.delete(r["z"][f].reshape(-1), s["planted"][f]).view(np.uint32)
            assert ((rest >> 8) == (0x40000000 >> 8)).all()          # the keys differ in the lowest byte only
        elif kind == "wide_exponent":
            assert (d == 0).sum() >= 1 and np.isinf(r["z"][f]).any() and not m[d == 0].any()
            assert r["z"][f][np.isfinite(r["z"][f])].max() > 1e29
        elif kind == "scattered_nan":
            assert 0 < nv < hw or hw <= 4
        elif kind == "one_valid":
            assert nv == 1 and m.sum() == 1
        elif kind == "two_valid":
            assert nv == 2 and m.sum() == 1 and r["median"][f] == 1.0
        elif kind == "no_valid":
            assert nv == 0 and not m.any() and np.isnan(r["median"][f]) and np.isnan(r["fit"]["scale"][f])
            assert r["bad"][f]
    # the filler frames would move every result
    assert (s["disps"][s["n"]:] == R.FILL_DISP).all() and (s["mono"][s["n"]:] == R.FILL_MONO).all()


@pytest.mark.parametrize("h,w,repeat", SELECT_SCENES)
def test_a_median_one_distinct_depth_off_changes_the_mask(h, w, repeat):
    """the sensitivity precondition: with the nearest distinct valid depth below or above in the median's place the mask
    differs - so the minimum, the maximum, the upper median or a select that narrows the wrong byte cannot pass.  The two
    value frame holds nothing below its median (the lower of its two depths); there only the upper neighbour exists."""
    s, r = R.select_scene(h, w, 0, repeat), R.select_reference(h, w, 0, repeat)
    seen = 0
    for f, kind in enumerate(s["kinds"]):
        if kind not in R.SENSITIVE:
            continue
        z, valid, med = r["z"][f], r["valid"][f], r["median"][f]
        lo, hi = R.distinct_neighbours(z, valid, med)
        assert hi is not None and not np.array_equal(R.mask_for(z, valid, hi), r["mask"][f]), (kind, "above")
        if kind == "two_values":
            assert lo is None
        else:
            assert lo is not None and not np.array_equal(R.mask_for(z, valid, lo), r["mask"][f]), (kind, "below")
            ia, ib = s["planted"][f]                      # the planted pixels are the ones that move
            assert r["mask"][f].reshape(-1)[ia] and not r["mask"][f].reshape(-1)[ib]
            assert not R.mask_for(z, valid, lo).reshape(-1)[ia] and R.mask_for(z, valid, hi).reshape(-1)[ib]
        # with an even count the upper median is another depth (the low-byte frame is full of ties: not there)
        v = np.sort(z[valid])
        assert kind == "low_byte" or len(v) % 2 == 1 or v[len(v) // 2] != med
        seen += 1
    assert seen == 3 * repeat


def test_alignment_matches_the_recorded_result():
    f = np.load(os.path.join(GOLD, "align.npz"))
    a = R.align64(f["pred"], f["tgt"], f["wts"])
    np.testing.assert_allclose(a["scale"], f["scale"], rtol=1e-5)
    np.testing.assert_allclose(a["shift"], f["shift"], rtol=1e-4, atol=1e-6)
    np.testing.assert_allclose(a["err"], f["err"], rtol=1e-4)
    s32, q32, e32 = R.align32(f["pred"], f["tgt"], f["wts"])
    np.testing.assert_allclose(s32, f["scale"], rtol=1e-5)
    np.testing.assert_allclose(e32, f["err"], rtol=1e-4)


def test_threshold_and_mask_restate_the_oracle_stage():
    """the same validity mask as oracle/update_step.py's restatement of update_valid_depth_mask on a consistent scene"""
    from oracle import update_step as ostep
    s = R.coupled_scene(24, 32)
    ix = np.array([4, 1, 7, 1])
    r = R.valid_mask(s["poses"], s["disps"], s["intrinsics"], ix, 0.05, 2)
    want = ostep.valid_depth_mask(s["poses"], s["disps"], s["intrinsics"], ix, 0.05, 2)
    assert np.array_equal(r["mask"], want) and 0 < want.mean() < 1


def test_alignment_bound_is_the_float32_formulation_s_own_error():
    """F32_ERROR holds the measured error of common.align_scale_and_shift in float32 per scene class (the kernel is
    allowed MARGIN times as much).  Another CPU may sum in another order, so the measurement here must agree with the
    record within a quarter, not to the digit.  The classes span both ends of the conditioning."""
    got = R.f32_errors()
    assert set(got) == set(R.F32_ERROR)
    for cls, (es, eq, k0, k1) in got.items():
        print(cls, es, eq, k0, k1)
        for measured, recorded in zip((es, eq), R.F32_ERROR[cls]):
            assert 0.75 * recorded <= measured <= 1.25 * recorded, (cls, measured, recorded)
    assert got["coupled"][2] < 50 and got["coupled"][3] > 1000
    assert got["select"][2] < 50 and got["select"][3] > 1000
    assert R.MARGIN == 4.0


@pytest.mark.parametrize("h,w", R.COUPLED_SIZES)
@pytest.mark.parametrize("mv_thresh", [0.01, 0.05])
def test_coupled_scene_preconditions(h, w, mv_thresh):
    s, r = R.coupled_scene(h, w), R.coupled_reference(h, w, mv_thresh)
    n, hw, fit = s["n"], h * w, r["fit"]
    cut = (r["valid"] & ~r["mask"]).reshape(n, -1).sum(1)
    assert (cut > 0).sum() >= 2                           # depths beyond 3 * median that passed the two-view filter
    assert (r["count"] >= 2).reshape(n, -1).sum(1)[:8].min() > 0
    # no frame decides the edge filter by rounding: every margin is ten times what the kernel's alignment may be off
    assert r["margins"]["err"].min() > 10 and r["margins"]["scale"].min() > 10, r["margins"]
    assert r["margins"]["count"].min() >= 1
    # the threshold band: the float64 counts give the same mask, so the GPU test asserts plain equality
    c64, edge = geom_ref.depth_filter64(s["poses"], s["disps"], s["intrinsics"], np.arange(n),
                                        r["thresh"].astype(np.float64))
    assert edge.reshape(n, -1).mean(1).max() <= 0.005
    assert np.array_equal(c64, r["count"])
    # the edge list shows every frame by itself and names frames beyond n
    assert np.array_equal(s["ii"][:n], np.arange(n)) and np.array_equal(s["jj"][:n], np.arange(n))
    assert (s["ii"] >= n).any() and (s["jj"] >= n).any() and r["edge_on"][n] and r["any_on"] == 1
    assert np.array_equal(r["edge_on"][:n], ~r["bad"])
    kind = {k: R.PRIORS.index(k) for k in R.PRIORS}
    assert np.isnan(r["median"][kind["no_neighbour"]]) and r["bad"][kind["no_neighbour"]]
    assert fit["kappa"][kind["near_constant"]] > 1000 and np.nanmin(fit["kappa"]) < 50
    if mv_thresh == 0.05:
        # every rule decides one frame alone
        ratio = fit["err"] / r["avg"]
        half = fit["nmask"] >= 0.5 * hw
        f = kind["anti"]
        assert fit["scale"][f] < 0 and half[f] and ratio[f] < R.COUPLED_MONO_THRES
        f = kind["structured"]
        assert fit["scale"][f] > 0 and half[f] and ratio[f] > 2 * R.COUPLED_MONO_THRES
        f = kind["half_cut"]                              # 3 * median, not the two-view filter, takes it below one half
        assert fit["scale"][f] > 0 and ratio[f] < R.COUPLED_MONO_THRES and not half[f]
        assert r["valid"][f].sum() >= 0.5 * hw
        for f in (kind["clean"], kind["noise2"]):
            assert not r["bad"][f]
        assert r["bad"].sum() >= 5


@pytest.mark.parametrize("h,w", R.COUPLED_SIZES)
def test_coupled_scene_with_every_frame_bad(h, w):
    s, r = R.coupled_scene(h, w, True), R.coupled_reference(h, w, 0.05, all_bad=True)
    assert r["bad"].all() and r["any_on"] == 0 and not r["edge_on"].any() and (s["ii"] < s["n"]).all()
    assert r["margins"]["scale"].min() > 10
    off = R.coupled_reference(h, w, 0.05, 0.0)
    assert not off["bad"].any() and off["edge_on"].all()
