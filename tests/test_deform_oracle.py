"""The float64 restatement (tests/deform_ref.py) reproduces the reference's deformation, proxy depth and
get_c2w_and_depth pinned in tests/golden/deform.npz (tests/golden/make_deform.py).  CPU only."""
import os

import numpy as np
import pytest

from deform_ref import c2w_and_depth_ref, deform_ref, proj_depth_ref, proxy_depth_ref, skip_row

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "deform.npz")


def load():
    z = np.load(GOLDEN)
    c = {k: z[k] for k in z.files}
    c["fx"], c["fy"], c["cx"], c["cy"] = (float(x) for x in z["intrinsics"])
    c["H"], c["W"] = (int(x) for x in z["hw"])
    return c


def deform_case(c, name, nan_scale=False):
    N_add, fix = (int(x) for x in c[f"deform_{name}_args"])
    near, far = (float(x) for x in c["near_far"])
    return deform_ref(c["poses"], c["disps_up"], c["valid"], c["dirty"], c["input_video_idx"], c["input_j"],
                      c["input_i"], c["input_depth"], N_add, near, far, bool(fix), c["fx"], c["fy"], c["cx"], c["cy"],
                      nan_scale=nan_scale)


@pytest.mark.parametrize("name", ["n3", "n5", "fix"])
def test_deformation_restated(name):
    c = load()
    pos, depth, cloud = deform_case(c, name, nan_scale=True)
    N_add = int(c[f"deform_{name}_args"][0])
    dirty = c["dirty"][c["input_video_idx"]]
    holes = c["input_video_idx"] == 5
    # the keyframe without a valid depth: NaN in the reference and here (0/0)
    assert np.isnan(c[f"deform_{name}_pos"][holes]).all() and np.isnan(pos[holes]).all()
    keep = dirty & ~holes
    np.testing.assert_allclose(c[f"deform_{name}_pos"][keep], pos[keep], rtol=1e-5, atol=1e-5)
    np.testing.assert_allclose(c[f"deform_{name}_depth"][keep], depth[keep], rtol=1e-5)
    rows = np.repeat(keep, N_add)
    np.testing.assert_allclose(c[f"deform_{name}_cloud"][rows], cloud[rows], rtol=1e-5, atol=1e-5)
    # clean keyframes keep their previous depth and the zero-initialised rows of the namespace
    assert np.array_equal(c[f"deform_{name}_depth"][~dirty], c["input_depth"][~dirty])
    assert not c[f"deform_{name}_pos"][~dirty].any()
    # add_points received the dirty keyframes, the flags are cleared
    assert np.array_equal(c[f"deform_{name}_added"], np.nonzero(c["dirty"])[0])
    assert not c[f"deform_{name}_flags_after"].any()
    # some points used the scale fallback
    fb = keep & ~c["valid"][c["input_video_idx"], c["input_j"], c["input_i"]]
    assert fb.sum() > 20


def test_all_holes_rule():
    c = load()
    pos, depth, _ = deform_case(c, "n3")                # the port: scale 1 -> the previous depth, new pose
    holes = c["input_video_idx"] == 5
    assert np.isfinite(pos[holes]).all() and np.array_equal(depth[holes], c["input_depth"][holes].astype(np.float64))


@pytest.mark.parametrize("counter", [3, 9])
def test_proxy_depth_restated(counter):
    c = load()
    H = c["H"]
    assert skip_row(3, 5, H) == H - 2 and skip_row(9, 5, H) == 4 and skip_row(5 + H, 5, H) == -1
    proj = proj_depth_ref(c["full_pcl"], c["full_mask"], counter, int(c["mapping_window_size"]), c["proxy_c2w"],
                          c["fx"], c["fy"], c["cx"], c["cy"])
    np.testing.assert_allclose(c[f"proj_c{counter}"], proj, rtol=1e-5, atol=0)
    for use_mono in (1, 0):
        want = proxy_depth_ref(proj, c["proxy_droid"], c["proxy_mono"], bool(use_mono))
        np.testing.assert_allclose(c[f"proxy_c{counter}_m{use_mono}"], want, rtol=1e-5, atol=0)
    # the zeroed row differs between the two counters
    assert not np.array_equal(c["proj_c3"], c["proj_c9"])


def test_c2w_and_depth_restated():
    c = load()
    for k in range(len(c["c2w_mono"])):
        c2w, wq, droid = c2w_and_depth_ref(c["poses"][k], c["disps_up"][k], c["valid"][k], c["c2w_mono"][k])
        np.testing.assert_allclose(c["c2w_c2w"][k], c2w, rtol=1e-5, atol=1e-6)
        np.testing.assert_allclose(c["c2w_droid"][k], droid, rtol=1e-6)
        np.testing.assert_allclose(c["c2w_mono_wq"][k], wq, rtol=2e-5, atol=1e-5)
