"""The float64 restatement of the on-device probe march (tests/near_pcl_ref.py) against a recording of the reference's
own sample_near_pcl, and the properties of the test cases the GPU tests rely on (no GPU)."""
import os

import numpy as np
import pytest

import near_pcl_ref as ref

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CHUNK = 64          # test_gpu_near_pcl asserts that this is the kernel's chunk width


def test_restatement_equals_reference_recording():
    """n = 25 probes, far = 6: same invalid rays and the same z-values bit for bit as the reference's sample_near_pcl on
    every firm ray (the reference places its probes with a float32 linspace, at most an ulp from the float64 one rounded
    to float32 - which cannot change the occupancy of a firm ray)"""
    f = np.load(os.path.join(GOLD, "near_pcl.npz"))
    sc = ref.scene()
    assert np.array_equal(f["rays_o"], sc["rays_o"]) and np.array_equal(f["rays_d"], sc["rays_d"])
    assert float(f["near"]) == ref.NEAR
    m = ref.march(sc["cloud"], sc["rays_o"], sc["rays_d"], float(f["near"]), float(f["far"]), 25, int(f["num"]))
    firm = m["firm"]
    assert (~firm).mean() <= ref.MAX_NON_FIRM_SHARE
    assert np.array_equal(~m["near_mask"][firm], f["invalid"][firm])
    assert np.array_equal(m["z"][firm].view(np.uint32), f["z_vals"][firm].view(np.uint32))
    assert int(f["invalid"].sum()) == 74 and f["z_vals"].shape == (ref.N_RAYS, 10)


def test_probe_depths_are_numpy_linspace():
    z64, z32 = ref.probe_depths(0.3, np.float32(3.6), 25)
    assert z64[0] == 0.3 and z64[-1] == float(np.float32(3.6)) and z64.dtype == np.float64
    assert np.array_equal(z64, 0.3 + np.arange(25) * ((float(np.float32(3.6)) - 0.3) / 24))
    assert np.array_equal(z32, z64.astype(np.float32))


# (far, n) -> non-firm rays, rays with one occupied probe, rays with none, brackets that cross a 64-probe chunk
EXPECTED = {(6.0, 25): (0, 67, 7, 0), (float(np.float32(3.6)), 25): (4, 5, 7, 0), (6.0, 64): (1, 0, 7, 0),
            (6.0, 65): (2, 0, 7, 0), (6.0, 130): (5, 0, 7, 0), (5.0, 160): (9, 0, 7, 30), (6.0, 300): (10, 0, 7, 0)}


@pytest.mark.parametrize("far,n", ref.CASES)
def test_case_properties(far, n):
    """the share of rays left out of the exact comparisons stays under 3 %, both kinds of invalid ray occur, and the
    cases that are there for the chunked march do what they are there for"""
    m = ref.scene_march(far, n, 10)
    occ_n = m["occ"].sum(-1)
    cross = ref.crosses_chunk(m["bracket"], CHUNK)
    got = (int((~m["firm"]).sum()), int((occ_n == 1).sum()), int((occ_n == 0).sum()), int(cross.sum()))
    assert got == EXPECTED[(far, n)]
    assert got[0] <= ref.MAX_NON_FIRM_SHARE * ref.N_RAYS
    assert np.array_equal(np.flatnonzero(occ_n == 0), np.arange(ref.N_MISS))        # the rays turned away from the cloud
    if (far, n) == (5.0, 160):
        assert int((cross & m["firm"]).sum()) == 30
    if (far, n) == (6.0, 300):
        first = m["bracket"][ref.N_MISS:, 0] // CHUNK
        assert set(first.tolist()) == {1, 2}                                        # no first hit in the first chunk
    # invalid rays span [near, far]; valid ones their bracket
    inv = ~m["near_mask"]
    assert np.all(m["z"][inv, 0] == np.float32(ref.NEAR)) and np.all(m["z"][inv, -1] == np.float32(far))
    z64 = ref.probe_depths(ref.NEAR, far, n)[0]
    v = np.flatnonzero(m["near_mask"])
    assert np.array_equal(m["z"][v, 0], z64[m["bracket"][v, 0]].astype(np.float32))
    assert np.array_equal(m["z"][v, -1], z64[m["bracket"][v, 1]].astype(np.float32))
