"""The float64 restatement of the mapper's keyframe selection (tests/keyframe_select_ref.py) against the reference's own
Mapper.get_mask_from_c2w and Mapper.keyframe_selection_overlap, pinned in tests/golden/keyframe_select.npz
(tests/golden/make_keyframe_select.py), and the C ABI of the HIP kernels that implement them."""
import os

import numpy as np
import pytest

from keyframe_select_ref import frustum_ref, overlap_ref, project

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "keyframe_select.npz")


def load():
    z = np.load(GOLDEN)
    c = {k: z[k] for k in z.files}
    c["fx"], c["fy"], c["cx"], c["cy"] = (float(x) for x in z["intrinsics"])
    c["H"], c["W"] = (int(x) for x in z["hw"])
    return c


def _frustum(c, edge):
    return frustum_ref(c["frustum_points"], c["frustum_c2w"], c["frustum_depth"], c["fx"], c["fy"], c["cx"], c["cy"],
                       c["H"], c["W"], edge)


@pytest.mark.parametrize("edge", [-4, 6])
def test_frustum_restatement_matches_the_reference(edge):
    c = load()
    mask, _ = _frustum(c, edge)
    assert np.array_equal(mask.astype(np.uint8), c[f"frustum_mask_{edge}"])


def test_frustum_fixture_covers_every_branch():
    c = load()
    mask, d = _frustum(c, -4)
    W, H = c["W"], c["H"]
    assert (d["negz"] < 0).any() and ((d["negz"] > d["depth"] + 0.5) & (d["u"] > 0) & (d["u"] < W)).any()
    assert (d["u"] < -4).any() and (d["u"] > W + 4).any() and (d["v"] < -4).any() and (d["v"] > H + 4).any()
    band = ((d["u"] > -4) & (d["u"] < 0)) | ((d["u"] > W) & (d["u"] < W + 4)) | ((d["v"] > -4) & (d["v"] < 0)) | \
        ((d["v"] > H) & (d["v"] < H + 4))
    assert (band & mask).any()                                       # kept only because the -4 edge enlarges the image
    zero = d["sample"] == 0
    assert (zero & mask & (d["negz"] > 0.5)).any()                   # kept only through the maximum replacement
    assert mask.sum() > 100 and (~mask).sum() > 100
    mask6, _ = _frustum(c, 6)
    assert (mask & ~mask6).any() and not (mask6 & ~mask).any()


def test_overlap_restatement_matches_the_reference():
    c = load()
    S = int(c["overlap_samples"])
    inside, total = overlap_ref(c["overlap_rays_o"], c["overlap_rays_d"], c["overlap_ray_depth"], c["overlap_c2ws"],
                                c["fx"], c["fy"], c["cx"], c["cy"], c["H"], c["W"], n_samples=S)
    assert total == len(c["overlap_ray_depth"]) * S and len(c["overlap_ray_depth"]) < int(c["overlap_pixels"])
    assert np.array_equal(inside / total, c["overlap_percent"])
    order = sorted(range(len(inside)), key=lambda i: inside[i], reverse=True)
    cand = [i for i in order if inside[i] > 0]
    assert cand[:int(c["overlap_k"])] == c["overlap_selected"].tolist()
    assert inside[3] == 0 and inside[5] == 0


def test_overlap_restatement_draws_through_the_reference_ray_convention():
    c = load()
    # the recorded rays leave the current camera's centre and land on its image plane at integer pixels
    u, v, z = project(c["overlap_c2w"], c["overlap_rays_o"] + c["overlap_rays_d"], c["fx"], c["fy"], c["cx"], c["cy"])
    assert (z < 0).all()
    assert np.abs(u - np.round(u)).max() < 5e-3 and np.abs(v - np.round(v)).max() < 5e-3     # (the 1e-5 in z)


def test_selection_symbols_are_bound_and_exported():
    """the two kernels are in the binding table and the built library exports them"""
    import ctypes

    import glorie_slam_amd.build as b
    from glorie_slam_amd import _lib
    for name in ("glorie_frustum_select", "glorie_frustum_select_workspace", "glorie_keyframe_overlap"):
        assert name in _lib.SIGNATURES, name
    lib = ctypes.CDLL(b.build())
    for name in ("glorie_frustum_select", "glorie_frustum_select_workspace", "glorie_keyframe_overlap"):
        assert hasattr(lib, name), name
