"""Every glorie_*_workspace function whose layout is written with the shared carver (or whose grid goes through the
shared reduce_blocks) still reports the size it reported before that refactor.  Python callers allocate by these
numbers and the entry points carve by the same layout, so a size that moves is a layout that moved.

The constants were recorded by calling the same functions of a library built from the commit before the refactor
(876a0a7) with the hand-written size formulas.  Host arithmetic only: no GPU."""
import pytest

N = (0, 1, 255, 256, 257, 70001)
PAIRS = ((0, 0), (1, 1), (255, 257), (256, 256), (257, 255), (70001, 1), (1, 70001))

ONE_ARG = {
    # n points
    "glorie_frustum_select_workspace": (8, 32, 2064, 2072, 2080, 562208),
    # n keys
    "glorie_topm_workspace": (1040, 1064, 1064, 1064, 1064, 4328),
    # N rays
    "glorie_pix_warp_workspace": (0, 16, 16, 16, 32, 4384),
    # F faces
    "glorie_mesh_area_cdf_workspace": (0, 32, 32, 32, 40, 2216),
    "glorie_mesh_depth_workspace": (0, 16, 1032, 1032, 1040, 280016),
    # n source points, Q queries
    "glorie_icp_moments_workspace": (0, 136, 136, 136, 272, 37264),
    "glorie_nn_stats_workspace": (0, 24, 24, 24, 48, 6576),
    # n_table entries of the block table
    "glorie_tsdf_allocate_workspace": (0, 32, 280, 280, 288, 72208),
}

TWO_ARGS = {
    # (V, F)
    "glorie_mesh_compact_workspace": (0, 56, 2088, 2088, 2104, 562232, 2232),
    # (H, W)
    "glorie_depth_l1_workspace": (0, 16, 4096, 4096, 4096, 4384, 4384),
    "glorie_frame_reduce_workspace": (0, 32, 8192, 8192, 8192, 8768, 8768),
    # (n_table, n_blocks)
    "glorie_tsdf_extract_workspace": (0, 1608, 400968, 399384, 397848, 3784, 109201608),
}


# the two with arguments of their own: (H, W, levels) and (H, W); 0 where the size is refused
MS_SSIM = {(0, 0, 1): 0, (11, 11, 1): 48, (10, 11, 1): 0, (37, 53, 2): 12560, (161, 177, 5): 235968, (160, 177, 5): 0,
           (255, 257, 4): 529632, (480, 640, 5): 2486352, (257, 70001, 5): 146619264, (11, 11, 6): 0}
LPIPS = {(0, 0): 0, (30, 31): 0, (31, 31): 52752, (35, 47): 94064, (63, 95): 468384, (255, 257): 5968896,
         (256, 256): 5968896, (257, 255): 5968896, (480, 640): 29087744}


@pytest.fixture(scope="module")
def lib():
    from glorie_slam_amd import _lib
    return _lib.load()


@pytest.mark.parametrize("name", sorted(ONE_ARG))
def test_one_argument_sizes(lib, name):
    got = tuple(getattr(lib, name)(n) for n in N)
    assert got == ONE_ARG[name]


@pytest.mark.parametrize("name", sorted(TWO_ARGS))
def test_two_argument_sizes(lib, name):
    got = tuple(getattr(lib, name)(a, b) for a, b in PAIRS)
    assert got == TWO_ARGS[name]


def test_ms_ssim_and_lpips_sizes(lib):
    assert {a: lib.glorie_ms_ssim_workspace(*a) for a in MS_SSIM} == MS_SSIM
    assert {a: lib.glorie_lpips_workspace(*a) for a in LPIPS} == LPIPS


def test_negative_sizes_report_nothing(lib):
    for name in ONE_ARG:
        assert getattr(lib, name)(-1) == 0, name
