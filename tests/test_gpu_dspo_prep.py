"""csrc/dspo_prep.hip against the numpy reference of tests/dspo_prep_ref.py: the two exact median selects (in LDS inside
glorie_dspo_prepare, over global keys in glorie_valid_depth_mask) on scenes where every order statistic gives another mask,
the least-squares alignment within four times the float32 formulation's own error, the bad-frame rule and the edge filter
exactly, and the publishing tail of the edge kernel.  test_dspo_prep_ref.py holds the preconditions on the CPU."""
import numpy as np
import pytest
import torch

import dspo_prep_ref as R

pytestmark = pytest.mark.gpu

PATTERN_SCALE, PATTERN_SHIFT = 7.5, -3.25


def _t(x, dev):
    return torch.from_numpy(np.ascontiguousarray(x)).to(dev)


def _pattern(shape):
    return np.random.default_rng(5).uniform(size=shape) < 0.5


def run_prepare(s, dev, n, mv_thresh, visible_num, mono_thres, ii, jj, publish=None, calls=1):
    """droid_backends.dspo_prepare on the scene s -> mask [B,h,w], scale [B], shift [B], edge_on [N], any_on; the outputs
    hold a pattern before the call"""
    from glorie_slam_amd import droid_backends as db
    disps = _t(s["disps"], dev)
    B = disps.shape[0]
    vm = _t(_pattern(disps.shape), dev)
    sc = torch.full((B,), PATTERN_SCALE, device=dev)
    sh = torch.full((B,), PATTERN_SHIFT, device=dev)
    args = (_t(s["poses"], dev), disps, _t(np.asarray(s["intrinsics"], np.float32), dev), _t(s["mono"], dev))
    ii_t, jj_t = _t(np.asarray(ii, np.int64), dev), _t(np.asarray(jj, np.int64), dev)
    for _ in range(calls):
        eo, any_on = db.dspo_prepare(*args, n, mv_thresh, visible_num, mono_thres, ii_t, jj_t, vm, sc, sh, publish=publish)
    torch.cuda.current_stream().synchronize()
    return vm.cpu().numpy(), sc.cpu().numpy(), sh.cpu().numpy(), eo.cpu().numpy().astype(bool), int(any_on.item())


def check_untouched(s, n, vm, sc, sh):
    assert np.array_equal(vm[n:], _pattern(vm.shape)[n:])
    assert (sc[n:] == PATTERN_SCALE).all() and (sh[n:] == PATTERN_SHIFT).all()


def check_alignment(tag, kinds, fit, sc, sh, n):
    """scale and shift of the first n frames against align64's `fit`; kinds[f] None = a coupled frame.  Prints the
    largest error per class in units of kappa * 2^-24 before it asserts."""
    worst = {}
    fails = []
    for f in range(n):
        kind = kinds[f]
        if kind == "no_valid" or (kind is None and fit["nmask"][f] == 0):
            assert not np.isfinite(sc[f]) and not np.isfinite(sh[f]), (tag, f, sc[f], sh[f])
            continue
        if kind in R.NO_FIT or not np.isfinite(fit["kappa"][f]):
            continue                                   # one masked pixel: the system is singular, any value goes
        cls = "coupled" if kind is None else "select_flat" if kind in R.FLAT_TARGET else "select"
        one = {k: v[f:f + 1] for k, v in fit.items()}
        es, eq = R.align_errors(sc[f:f + 1], sh[f:f + 1], one, flat=cls == "select_flat")
        w = worst.setdefault(cls, [0.0, 0.0])
        w[0], w[1] = max(w[0], float(es[0])), max(w[1], float(eq[0]))
        bs, bq = R.kernel_bound(cls)
        if not (es[0] <= bs and eq[0] <= bq):
            fails.append((f, kind, float(es[0]), bs, float(eq[0]), bq, float(fit["kappa"][f])))
    for cls, (es, eq) in worst.items():
        print("alignment %s %s: scale %.3f shift %.3f (bounds %.3f %.3f)" % ((tag, cls, es, eq) + R.kernel_bound(cls)))
    assert not fails, (tag, fails)


def robust(r, f):
    """frame f's bad flag does not hang on the rounding of the alignment"""
    m = r["margins"]
    return m["err"][f] > 10 and m["scale"][f] > 10


# ---- the select in LDS ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("h,w", R.PREPARE_SIZES)
def test_prepare_on_select_scenes(gpu, h, w):
    s, r = R.select_scene(h, w), R.select_reference(h, w)
    n = s["n"]
    ii = np.arange(n, dtype=np.int64)
    vm, sc, sh, eo, any_on = run_prepare(s, gpu, n, 0.05, 0, 0.1, ii, ii)
    bad = [(f, s["kinds"][f], int((vm[f] != r["mask"][f]).sum())) for f in range(n) if not np.array_equal(vm[f], r["mask"][f])]
    assert not bad, bad
    check_untouched(s, n, vm, sc, sh)
    check_alignment("%dx%d" % (h, w), s["kinds"], r["fit"], sc, sh, n)
    sure = [f for f in range(n) if robust(r, f)]
    assert len(sure) >= 4
    assert np.array_equal(eo[sure], ~r["bad"][sure]), (eo, r["bad"], sure)
    assert s["kinds"].index("no_valid") in sure and not eo[s["kinds"].index("no_valid")]
    if len(sure) == n:
        assert any_on == r["any_on"]
    elif (~r["bad"][sure]).any():
        assert any_on == 1


def test_prepare_refuses_a_map_beyond_its_limit(gpu):
    from glorie_slam_amd import _lib as L
    s = dict(poses=np.tile(np.array([0, 0, 0, 0, 0, 0, 1], np.float32), (2, 1)), disps=np.full((2, 1, 38401), 0.5, np.float32),
             mono=np.full((2, 1, 38401), 0.5, np.float32), intrinsics=R.synth.camera(1, 38401))
    from glorie_slam_amd import droid_backends as db
    disps = _t(s["disps"], gpu)
    vm, sc, sh = _t(_pattern(disps.shape), gpu), torch.full((2,), PATTERN_SCALE, device=gpu), torch.full((2,), PATTERN_SHIFT, device=gpu)
    ii = torch.zeros(1, dtype=torch.int64, device=gpu)
    with pytest.raises(L.GlorieError, match="GLORIE_EUNSUPPORTED"):
        db.dspo_prepare(_t(s["poses"], gpu), disps, _t(s["intrinsics"], gpu), _t(s["mono"], gpu), 2, 0.05, 0, 0.1, ii, ii,
                        vm, sc, sh)
    torch.cuda.synchronize()
    check_untouched(s, 0, vm.cpu().numpy(), sc.cpu().numpy(), sh.cpu().numpy())


# ---- the select over global keys --------------------------------------------------------------------------------------------
def run_vmask(s, dev, ix, mv_thresh, visible_num):
    from glorie_slam_amd import droid_backends as db
    m = db.valid_depth_mask(_t(s["poses"], dev), _t(s["disps"], dev), _t(np.asarray(s["intrinsics"], np.float32), dev),
                            _t(np.asarray(ix, np.int64), dev), mv_thresh, visible_num)
    torch.cuda.synchronize()
    return m.cpu().numpy()


@pytest.mark.parametrize("h,w", R.VMASK_SIZES)
def test_valid_depth_mask_on_select_scenes(gpu, h, w):
    s = R.select_scene(h, w, 0, 2)
    ix = R.vmask_indices(s, seed=h)
    assert len(set(ix.tolist())) == 9 and len(ix) == 10 and list(ix) != sorted(ix)
    assert {s["kinds"][i] for i in ix} == set(R.KINDS) and ix.max() < s["n"]
    want = R.valid_mask(s["poses"], s["disps"], s["intrinsics"], ix, 0.05, 0)["mask"]
    got = run_vmask(s, gpu, ix, 0.05, 0)
    bad = [(b, s["kinds"][ix[b]], int((got[b] != want[b]).sum())) for b in range(len(ix)) if not np.array_equal(got[b], want[b])]
    assert not bad, bad


def test_valid_depth_mask_with_seventy_frames(gpu):
    """one thread per frame in blocks of 64: 70 frames span two blocks of vmask_pick_kernel"""
    s = R.select_scene(7, 9, 0, 8)
    ix = np.random.default_rng(3).permutation(s["n"])[:70].astype(np.int64)
    want = R.valid_mask(s["poses"], s["disps"], s["intrinsics"], ix, 0.05, 0)["mask"]
    got = run_vmask(s, gpu, ix, 0.05, 0)
    bad = [(b, s["kinds"][ix[b]]) for b in range(70) if not np.array_equal(got[b], want[b])]
    assert not bad, bad
    assert len({s["kinds"][i] for i in ix[64:]} & set(R.SENSITIVE)) >= 1      # the second block decides something


# ---- geometry, alignment and edge filter together ---------------------------------------------------------------------------
@pytest.mark.parametrize("h,w", R.COUPLED_SIZES)
@pytest.mark.parametrize("mv_thresh", [0.01, 0.05])
def test_prepare_and_mask_on_the_coupled_scene(gpu, h, w, mv_thresh):
    s, r = R.coupled_scene(h, w), R.coupled_reference(h, w, mv_thresh)
    n = s["n"]
    vm, sc, sh, eo, any_on = run_prepare(s, gpu, n, mv_thresh, 2, R.COUPLED_MONO_THRES, s["ii"], s["jj"])
    assert np.array_equal(vm, r["mask"]), [(f, int((vm[f] != r["mask"][f]).sum())) for f in range(n)]
    check_alignment("%dx%d mv %g" % (h, w, mv_thresh), [None] * n, r["fit"], sc, sh, n)
    assert np.array_equal(eo, r["edge_on"]), (eo[:n], r["bad"])
    assert any_on == r["any_on"] == 1
    ix = np.array([4, 0, 7, 2, 8, 2, 5], np.int64)                  # unordered, with holes and a repeat
    got = run_vmask(s, gpu, ix, mv_thresh, 2)
    assert np.array_equal(got, r["mask"][ix])


@pytest.mark.parametrize("h,w", R.COUPLED_SIZES)
def test_edge_filter_all_bad_off_and_empty(gpu, h, w):
    s, r = R.coupled_scene(h, w, True), R.coupled_reference(h, w, 0.05, all_bad=True)
    n = s["n"]
    vm, sc, sh, eo, any_on = run_prepare(s, gpu, n, 0.05, 2, R.COUPLED_MONO_THRES, s["ii"], s["jj"])
    assert np.array_equal(vm, r["mask"])
    check_alignment("%dx%d all bad" % (h, w), [None] * n, r["fit"], sc, sh, n)
    assert not eo.any() and any_on == 0 and r["any_on"] == 0
    # mono_thres = 0: no frame is bad
    s, r = R.coupled_scene(h, w), R.coupled_reference(h, w, 0.05, 0.0)
    vm, sc, sh, eo, any_on = run_prepare(s, gpu, n, 0.05, 2, 0.0, s["ii"], s["jj"])
    assert np.array_equal(vm, r["mask"]) and eo.all() and any_on == 1 and r["edge_on"].all()
    # no edge at all
    none = np.zeros(0, np.int64)
    vm, sc2, sh2, eo, any_on = run_prepare(s, gpu, n, 0.05, 2, R.COUPLED_MONO_THRES, none, none)
    assert np.array_equal(vm, r["mask"]) and len(eo) == 0 and any_on == 0
    assert np.array_equal(sc2, sc, equal_nan=True) and np.array_equal(sh2, sh, equal_nan=True)


# ---- the last workgroup publishes -------------------------------------------------------------------------------------------
def _publish_buffers(dev):
    """as DepthVideo.deferred_flag_init: a pinned host word, the device's launch count and arrival counter"""
    host = torch.zeros(1, dtype=torch.int32).pin_memory()
    state = torch.zeros(2, dtype=torch.int32, device=dev)
    return host, state


@pytest.mark.parametrize("N", [600, 40])
def test_edge_kernel_publishes_count_and_flag(gpu, N):
    """N = 600 is three workgroups: the last to arrive publishes and resets the arrival counter, so a second call on the
    same stream publishes again (count 2)"""
    for all_bad in (False, True):
        s, r = R.coupled_scene(24, 32, all_bad), R.coupled_reference(24, 32, 0.05, all_bad=all_bad)
        reps = -(-N // len(s["ii"]))
        ii, jj = np.tile(s["ii"], reps)[:N], np.tile(s["jj"], reps)[:N]
        host, state = _publish_buffers(gpu)
        vm, sc, sh, eo, any_on = run_prepare(s, gpu, s["n"], 0.05, 2, R.COUPLED_MONO_THRES, ii, jj,
                                             publish=(state, host.data_ptr()), calls=2)
        want = int(np.tile(r["edge_on"], reps)[:N].any())
        assert want == (0 if all_bad else 1) and any_on == want
        assert np.array_equal(eo, np.tile(r["edge_on"], reps)[:N])
        assert int(host[0]) == (2 << 1) | want, (int(host[0]), want)
        assert state.cpu().tolist() == [2, 0]


def test_publish_without_frames(gpu):
    """n = 0: nothing to prepare, publish_flag_kernel stores the count and a cleared flag"""
    s = R.coupled_scene(24, 32)
    host, state = _publish_buffers(gpu)
    vm, sc, sh, eo, any_on = run_prepare(s, gpu, 0, 0.05, 2, R.COUPLED_MONO_THRES, s["ii"], s["jj"],
                                         publish=(state, host.data_ptr()), calls=2)
    assert any_on == 0 and int(host[0]) == (2 << 1) and state.cpu().tolist() == [2, 0]
    check_untouched(s, 0, vm, sc, sh)
