"""The float64 restatement of the colour-gradient radii and the gradient-ranked pixel draw (tests/color_grad_ref.py)
against the reference's own Mapper.run radius block, get_sample_uv_with_grad and get_samples_with_pixel_grad, pinned in
tests/golden/color_grad.npz (tests/golden/make_color_grad.py), and the C ABI of the HIP kernels that implement them."""
import os

import numpy as np

from color_grad_ref import color_grad_maps_ref, top_indices_ref

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "color_grad.npz")


def load():
    z = np.load(GOLDEN)
    c = {k: z[k] for k in z.files}
    c["image"] = c["image_u8"].astype(np.float32) / np.float32(255)
    c["H"], c["W"] = (int(x) for x in c["hw"])
    thr, rmax, rmin, ratio = (float(x) for x in c["cfg"])
    c["args"] = dict(color_grad_threshold=thr, radius_add_max=rmax, radius_add_min=rmin, radius_query_ratio=ratio)
    return c


def test_restated_maps_match_the_reference():
    c = load()
    m = color_grad_maps_ref(c["image"], valid=c["valid"].astype(bool), **c["args"])
    # the reference's gray values and magnitudes are fp32 (about 1e-7 from float64), the slope of r_add is -0.43
    np.testing.assert_allclose(m["r_add"], c["r_add"], rtol=5e-6)
    np.testing.assert_allclose(m["r_query"], c["r_query"], rtol=5e-6)
    np.testing.assert_allclose(m["grad"], c["grad"], rtol=1e-6, atol=5e-7)


def test_fixture_covers_every_segment_and_the_border():
    c = load()
    thr = c["args"]["color_grad_threshold"]
    g = color_grad_maps_ref(c["image"], **c["args"])["grad"]
    assert (g <= 0.01).sum() > 100 and ((g > 0.01) & (g < thr)).sum() > 100 and (g > thr).sum() > 100
    for edge in (g[0], g[-1], g[:, 0], g[:, -1]):
        assert (edge > 0.01).any()
    assert (c["valid"] == 0).sum() > 100


def test_restated_candidates_match_the_reference():
    c = load()
    n = int(c["n"])
    grad = color_grad_maps_ref(c["image"], valid=c["valid"].astype(bool))["grad"]
    idx, valid = top_indices_ref(grad, 5 * n)
    assert np.array_equal(idx, c["candidates"]) and valid == 5 * n
    # the pixels of get_samples_with_pixel_grad: the first n candidates with a depth
    first = c["candidates"][:n]
    keep = first[c["depth"].reshape(-1)[first] > 0]
    assert np.array_equal(keep, c["s_j"] * c["W"] + c["s_i"])


def test_top_rule_takes_the_lowest_index_of_a_tie():
    keys = np.array([0.5, 1.0, 0.5, 0.5, -1.0, 2.0, 0.5], np.float32)
    assert top_indices_ref(keys, 4)[0].tolist() == [0, 1, 2, 5]
    idx, valid = top_indices_ref(keys, 7)
    assert idx.tolist() == list(range(7)) and valid == 6


def test_color_grad_symbols_are_bound_and_exported():
    """the kernels are in the binding table and the built library exports them"""
    import ctypes

    import glorie_slam_amd.build as b
    from glorie_slam_amd import _lib
    names = ("glorie_color_grad_maps", "glorie_topm", "glorie_topm_workspace")
    for name in names:
        assert name in _lib.SIGNATURES, name
    lib = ctypes.CDLL(b.build())
    for name in names:
        assert hasattr(lib, name), name
    import glorie_slam_amd.color_grad as cg
    for name in ("color_grad_maps", "dynamic_radius_maps", "get_sample_uv_with_grad", "get_samples_with_pixel_grad"):
        assert callable(getattr(cg, name)), name
