"""The numpy restatement of the masked sampler and the depth gate (tests/map_sample_ref.py) against
np.flatnonzero(mask)[rank], against the reference's torch formulation on the CPU given the same ranks, and against
torch.median / torch.max and the reference's gate expression; and the preconditions of the shared scenes.  No GPU."""
import numpy as np
import pytest
import torch

from map_sample_ref import (DRAW_RANGE, DRAW_SETS, FRAME_PATTERNS, GATE_KINDS, GATE_SIZES, PATTERNS, SHAPES, depth_gate_ref,
                            gate_vector, kth_set_bit, rank_of, sample_pixels_ref, sample_window_rays_ref, scene,
                            torch_masked_samples, valid_index_ref, valid_mask)
from window_rays_ref import EPS32, rays_d_f64

NAMES = ["A", "B", "C", "D"]


@pytest.fixture(scope="module", params=NAMES)
def case(request):
    s = scene(request.param)
    return s, valid_index_ref(s["depths"])


def test_tables(case):
    s, (words, prefix) = case
    mask = valid_mask(s["depths"])
    M, HW = mask.shape
    nw = (HW + 63) // 64
    assert words.shape == (M, nw) and words.dtype == np.uint64 and prefix.shape == (M, nw + 1) and prefix.dtype == np.int32
    for m in range(M):
        bits = [(int(words[m, p // 64]) >> (p % 64)) & 1 for p in range(nw * 64)]
        assert bits[:HW] == mask[m].astype(int).tolist() and not any(bits[HW:])        # tail bits are zero
        assert prefix[m, 0] == 0 and prefix[m, nw] == mask[m].sum()
        assert np.array_equal(np.diff(prefix[m]), [bin(int(w)).count("1") for w in words[m]])


@pytest.mark.parametrize("mode", ["depth", "all"])
def test_pixels_against_flatnonzero(case, mode):
    s, _ = case
    words, prefix = valid_index_ref(s["depths"], mode)
    mask = valid_mask(s["depths"], mode)
    per, W = s["per"], s["W"]
    for draws in s["draws"]:
        ii, jj = sample_pixels_ref(words, prefix, draws, per, s["H"], W)
        for m in range(s["M"]):
            sl = slice(m * per, (m + 1) * per)
            count = int(mask[m].sum())
            if count == 0:
                assert not ii[sl].any() and not jj[sl].any()
                continue
            rank = rank_of(draws[sl], count)
            assert rank.min() >= 0 and rank.max() < count
            assert np.array_equal(jj[sl] * W + ii[sl], np.flatnonzero(mask[m])[rank])


def test_kth_set_bit():
    rng = np.random.default_rng(5)
    for word in [1, 1 << 63, (1 << 64) - 1, 0x8000000000000001] + [int(x) for x in rng.integers(1, 2 ** 63, 50)]:
        ones = [b for b in range(64) if (word >> b) & 1]
        assert [kth_set_bit(word, k) for k in range(len(ones))] == ones


def test_rays_against_the_torch_formulation(case):
    """the reference's get_samples with mask on the CPU, its randint replaced by the restatement's ranks: the same
    pixels, depths and colours, and directions within five roundings a side; a slot's invalid-depth draws cannot occur
    (every sampled depth is > 0), so its depth filter drops nothing"""
    s, _ = case
    t = torch.from_numpy
    mask = valid_mask(s["depths"]).reshape(s["M"], s["H"], s["W"])
    per = s["per"]
    draws = s["draws"][0]
    ro, rd, d, col, _, ii, jj = sample_window_rays_ref(s["depths"], s["images"], s["c2ws"], draws, per, *s["K"])
    _, S = rays_d_f64(s["c2ws"], ii, jj, per, *s["K"])
    for m in range(s["M"]):
        sl = slice(m * per, (m + 1) * per)
        count = int(mask[m].sum())
        if count == 0:
            assert not d[sl].any()
            continue
        sample = t(rank_of(draws[sl], count))
        image = t(np.ascontiguousarray(s["images"][m].transpose(1, 2, 0)))
        tro, trd, td, tcol, ti, tj = torch_masked_samples(t(s["depths"][m]), image, t(s["c2ws"][m]), t(mask[m]), sample,
                                                          *s["K"], "cpu")
        assert td.shape[0] == per and bool((td > 0).all())
        assert np.array_equal(ti.numpy(), ii[sl]) and np.array_equal(tj.numpy(), jj[sl])
        assert np.array_equal(td.numpy(), d[sl]) and np.array_equal(tcol.numpy(), col[sl])
        assert np.array_equal(tro.numpy(), ro[sl])
        err = np.abs(trd.numpy().astype(np.float64) - rd[sl].astype(np.float64))
        assert (err <= 5 * EPS32 * S[sl]).all()


def test_scene_preconditions():
    assert SHAPES == {"A": (3, 5, 7, 4), "B": (67, 9, 13, 5), "C": (2, 16, 24, 300), "D": (2, 48, 64, 130)}
    used = set()
    for name in NAMES:
        s = scene(name)
        M, H, W, per = SHAPES[name]
        used |= set(s["patterns"])
        assert s["draws"].shape == (DRAW_SETS[name], M * per) and s["draws"].dtype == np.int64
        assert s["draws"].min() == 0 and s["draws"].max() == DRAW_RANGE - 1
        counts = valid_mask(s["depths"]).sum(1)
        for m, pat in enumerate(s["patterns"]):
            flat = s["depths"][m].reshape(-1)
            if pat == "all":
                assert counts[m] == H * W
            elif pat == "none":
                assert counts[m] == 0
            elif pat == "last":
                assert counts[m] == 1 and flat[-1] > 0
            elif pat == "tail":
                assert counts[m] >= 1 and not (flat[:(H * W - 1) // 64 * 64] > 0).any() and flat[-1] > 0
            elif pat == "bad":
                assert np.isnan(flat).any() and (flat < 0).any() and 0 < counts[m] < H * W
            else:
                assert 0.3 * H * W < counts[m] < 0.7 * H * W
        finite = s["depths"][np.isfinite(s["depths"]) & (s["depths"] != 0)]
        assert np.abs(finite).min() > 1e-3                                   # no denormal depths
    assert used == set(PATTERNS)
    assert (5 * 7 < 64) and (64 < 9 * 13 < 128) and 16 * 24 == 6 * 64 and 48 * 64 == 48 * 64 and 130 % 64 and 300 > 4 * 64


def test_every_rank_is_hit_in_A():
    s = scene("A")
    words, prefix = valid_index_ref(s["depths"])
    mask = valid_mask(s["depths"])
    per = s["per"]
    hit = [set() for _ in range(s["M"])]
    for draws in s["draws"]:
        ii, jj = sample_pixels_ref(words, prefix, draws, per, s["H"], s["W"])
        for m in range(s["M"]):
            hit[m] |= set((jj[m * per:(m + 1) * per] * s["W"] + ii[m * per:(m + 1) * per]).tolist())
    for m in range(s["M"]):
        assert hit[m] == set(np.flatnonzero(mask[m]).tolist()) and len(hit[m]) > 0


@pytest.mark.parametrize("count", [1, 35, 640 * 480, 2 ** 31 - 1])
def test_rank_map_stays_inside(count):
    draws = np.array([0, 1, DRAW_RANGE // 2, DRAW_RANGE - 2, DRAW_RANGE - 1], np.int64)
    rank = rank_of(draws, count)
    exact = [(int(q) * count) >> 31 for q in draws]                          # python integers: no overflow
    assert rank.tolist() == exact and rank.min() >= 0 and rank.max() < count
    assert rank[0] == 0 and rank[-1] == count - 1


# ---- the gate -------------------------------------------------------------------------------------------------------
def _torch_gate(d):
    """the reference's expression (src/mapper.py:474-476) on the positive depths, on the CPU"""
    pos = d[d > 0]
    if pos.numel() == 0:
        return None
    thr = torch.minimum(10 * pos.median(), 1.2 * torch.max(pos))
    return pos.median(), torch.max(pos), thr, (d > 0) & (d <= thr)


@pytest.mark.parametrize("kind", GATE_KINDS)
@pytest.mark.parametrize("n", GATE_SIZES)
def test_gate_against_torch(kind, n):
    d = gate_vector(kind, n)
    keep, stats = depth_gate_ref(d)
    assert keep.dtype == np.float32 and stats.dtype == np.float32 and stats.shape == (4,)
    got = _torch_gate(torch.from_numpy(d))
    if got is None:
        assert not keep.any() and not stats.any()
        return
    median, dmax, thr, inside = got
    assert stats[0] == median.item() and stats[1] == dmax.item() and stats[2] == thr.item()
    assert np.array_equal(keep, inside.numpy().astype(np.float32)) and stats[3] == inside.sum().item()


def test_gate_vector_preconditions():
    binds = set()
    for n in GATE_SIZES:
        for kind in GATE_KINDS:
            d = gate_vector(kind, n)
            keep, (median, dmax, thr, kept) = depth_gate_ref(d)
            with np.errstate(invalid="ignore"):
                n_pos = int((d > 0).sum())
            if n_pos:
                binds.add("median" if np.float32(10) * median < np.float32(1.2) * dmax else "max")
            if kind == "outlier" and n >= 63:
                assert 1 <= n_pos - kept <= 0.2 * n_pos and keep[n // 2] == 0
                assert np.float32(10) * median < np.float32(1.2) * dmax
            if kind == "max_binds":
                assert np.float32(1.2) * dmax <= np.float32(10) * median and kept == n_pos
            if kind == "quantised" and n >= 1000:
                assert (d == median).sum() > n // 32                          # many ties at the median
            if kind == "mantissa" and n >= 63:
                assert len(np.unique(d)) > 1 and (np.unique(d.view(np.uint32)) >> 3 == np.float32(2).view(np.uint32) >> 3).all()
            if kind == "zeros_nan" and n >= 63:
                assert np.isnan(d).any() and (d == 0).any() and 0 < n_pos < n
            if kind == "all_zero":
                assert n_pos == 0
    assert binds == {"median", "max"}                                         # both branches of the min occur
