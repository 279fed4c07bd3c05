"""The LPIPS kernels (csrc/lpips.hip through glorie_slam_amd/lpips.py) against the float64 reference of tests/lpips_ref.py.

Feature bound: for every tap the kernel's largest absolute error against float64 is at most 4 times the largest absolute
error of the torch float32 composition (on the CPU) against float64 on the same inputs - the yardstick and factor of
tests/test_gpu_image_metrics.py; a maximum over thousands of elements, so it needs no floor.
Value bound: for the per-layer values and the total the error against float64 is at most max(4 e32, 8 * 2^-24 |v|), e32
the float32 composition's error of the same value; the floor of eight half-ulps covers the float32 store of six outputs.
The kernel sums the score in fp64.  The ratios are printed under -s."""
import functools

import numpy as np
import pytest
import torch

import lpips_ref as R

pytestmark = pytest.mark.gpu

FACTOR = 4.0
HALF_ULP = 2.0 ** -24


@functools.lru_cache(maxsize=None)
def _metric(gpu, fold=False):
    from glorie_slam_amd.lpips import Lpips
    wts = R.weights()
    return Lpips([(torch.tensor(np.array(w)), torch.tensor(np.array(b))) for w, b in wts["conv"]],
                 [torch.tensor(np.array(l)) for l in wts["lin"]], device=gpu, fold_pools=fold)


def _dev(a, gpu, channels_first=False):
    t = torch.tensor(np.array(a)).to(gpu)
    return t.permute(2, 0, 1).contiguous() if channels_first else t


def _bits(t):
    return t.view(torch.int32)


def _check(gpu, H, W, channels_first, fold, tag):
    x, y, (v, per, maps), (v32, per32, maps32) = R.case(H, W)
    L = _metric(gpu, fold)
    tx, ty = _dev(x, gpu, channels_first), _dev(y, gpu, channels_first)
    got_v, got_per = L(tx, ty, channels_first=channels_first, return_layers=True)
    got_maps = L.features(tx, ty, channels_first=channels_first)
    assert got_v.shape == () and got_v.dtype == torch.float32 and got_per.shape == (5,)
    assert [tuple(m.shape) for m in got_maps] == [m.shape for m in maps]
    ratios = []
    for l, (g, ref, f32) in enumerate(zip(got_maps, maps, maps32)):
        err = np.abs(g.double().cpu().numpy() - ref).max()
        e32 = np.abs(f32 - ref).max()
        ratios.append(err / e32)
        print(f"{tag} tap {l + 1}: largest feature error {err:.2e}, float32 composition {e32:.2e}, ratio {err / e32:.3f}")
    want = np.concatenate([[v], per])
    got = np.concatenate([[float(got_v)], got_per.double().cpu().numpy()])
    e32 = np.abs(np.concatenate([[v32], per32]) - want)
    bound = np.maximum(FACTOR * e32, 8 * HALF_ULP * np.abs(want))
    err = np.abs(got - want)
    print(f"{tag} values {got}: errors {err}, float32 composition {e32}, largest ratio to the bound {(err / bound).max():.3f}")
    assert all(r <= FACTOR for r in ratios), ratios
    assert np.all(err <= bound), (err, bound)


@pytest.mark.parametrize("channels_first", [False, True])
@pytest.mark.parametrize("H,W", R.SIZES)
def test_features_and_values_against_float64(gpu, H, W, channels_first):
    """31 x 31 is the smallest legal size: one pixel in the last three taps"""
    _check(gpu, H, W, channels_first, False, f"{H}x{W} {'CHW' if channels_first else 'HWC'}")


@pytest.mark.parametrize("fold", [False, True])
@pytest.mark.parametrize("H,W", R.TILE_CASES)
def test_tile_edges_against_float64(gpu, H, W, fold):
    """tap sizes around the pixel tile of a workgroup (one short, exactly one, one over, two, two and a ragged one), for
    conv1's output (64 pixels) and for the 3x3 layers' (32); with the pools as launches of their own and folded into the
    staging"""
    _check(gpu, H, W, bool((H + W) & 2), fold, f"{H}x{W} {'folded' if fold else 'pool launches'}")


def test_folded_pools_give_the_same_bits(gpu):
    x, y = (_dev(a, gpu) for a in R.case(97, 130)[:2])
    a, b = _metric(gpu, False), _metric(gpu, True)
    assert all(torch.equal(_bits(p), _bits(q)) for p, q in zip(a.features(x, y), b.features(x, y)))
    assert torch.equal(_bits(a(x, y, return_layers=True)[1]), _bits(b(x, y, return_layers=True)[1]))


# ---- exact cases -----------------------------------------------------------------------------------------------------------
def test_exact_cases(gpu):
    L = _metric(gpu)
    for H, W, cf in ((63, 95, False), (35, 47, True)):
        x, y = (_dev(a, gpu, cf) for a in R.case(H, W)[:2])
        v, per = L(x, x.clone(), channels_first=cf, return_layers=True)
        assert float(v) == 0.0 and bool((per == 0.0).all())
        fx = L.features(x, x.clone(), channels_first=cf)
        assert all(torch.equal(_bits(m[0]), _bits(m[1])) for m in fx), "identical images give bit-identical features"
        a, b = L(x, y, channels_first=cf, return_layers=True), L(y, x, channels_first=cf, return_layers=True)
        assert float(a[0]) > 0.05
        assert torch.equal(_bits(a[0]), _bits(b[0])) and torch.equal(_bits(a[1]), _bits(b[1]))
        wild = 3.0 * x - 1.0
        assert float(wild.min()) < 0.0 and float(wild.max()) > 1.0
        a, b = L(wild, y, channels_first=cf, return_layers=True), L(wild.clamp(0.0, 1.0), y, channels_first=cf,
                                                                     return_layers=True)
        assert torch.equal(_bits(a[0]), _bits(b[0])) and torch.equal(_bits(a[1]), _bits(b[1]))


def test_repeated_calls_are_bitwise_equal_and_record_into_a_graph(gpu):
    L = _metric(gpu)
    x, y = (_dev(a, gpu) for a in R.case(63, 95)[:2])

    def run(a, b):
        v, per = L(a, b, return_layers=True)
        return [v, per] + L.features(a, b)

    first = [o.clone() for o in run(x, y)]
    for _ in range(3):
        assert all(torch.equal(_bits(a), _bits(b)) for a, b in zip(first, run(x, y)))
    # recorded on one pair of images, replayed on another of the same shape
    static = [x.clone(), y.clone()]
    side = torch.cuda.Stream(gpu)
    side.wait_stream(torch.cuda.current_stream(gpu))
    with torch.cuda.stream(side):
        run(*static)
    torch.cuda.current_stream(gpu).wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        recorded = run(*static)
    x2, y2 = (_dev(a, gpu) for a in R.scene(63, 95, seed=77))
    static[0].copy_(x2)
    static[1].copy_(y2)
    graph.replay()
    torch.cuda.synchronize()
    eager = run(x2, y2)
    assert all(torch.equal(_bits(a), _bits(b)) for a, b in zip(recorded, eager))
    assert not torch.equal(eager[0], first[0])


# ---- copies and rejections ---------------------------------------------------------------------------------------------------
def test_non_contiguous_and_float64_inputs_are_copied(gpu):
    L = _metric(gpu)
    x, y = R.case(35, 47)[:2]
    tx, ty = _dev(x, gpu), _dev(y, gpu)
    want = L(tx, ty)
    xc = _dev(x, gpu, True).permute(1, 2, 0)                   # [H,W,3] view of [3,H,W] storage
    assert not xc.is_contiguous()
    assert torch.equal(L(xc, ty.double()), want)
    wide = torch.zeros(35, 47, 6, device=gpu)
    wide[..., ::2] = ty
    assert torch.equal(L(tx, wide[..., ::2]), want)


def test_sizes_and_shapes_are_rejected(gpu):
    from glorie_slam_amd import _lib
    L = _metric(gpu)
    z = torch.zeros(30, 40, 3, device=gpu)
    with pytest.raises(ValueError):
        L(z, z)
    with pytest.raises(ValueError):
        L(z.permute(2, 0, 1).contiguous(), z.permute(2, 0, 1).contiguous(), channels_first=True)
    ok = torch.zeros(40, 40, 3, device=gpu)
    with pytest.raises(ValueError):
        L(ok, ok[:35])
    with pytest.raises(ValueError):
        L(ok[:, :, :2], ok[:, :, :2])
    with pytest.raises(_lib.GlorieError):
        L(ok.cpu(), ok.cpu())
    lib = _lib.load()
    assert lib.glorie_lpips_workspace(30, 40) == 0 and lib.glorie_lpips_workspace(40, 30) == 0
    assert lib.glorie_lpips_workspace(31, 31) > 0
    ws = _lib.workspace(lib.glorie_lpips_workspace(40, 40), gpu)
    out = torch.zeros(6, device=gpu)
    args = (_lib.ptr(L.weights), _lib.ptr(ws), _lib.ptr(out), _lib.ptr(None), 0, _lib.stream_ptr(gpu))
    assert lib.glorie_lpips(_lib.ptr(ok), _lib.ptr(ok), 30, 40, 0, *args) == -1         # GLORIE_EINVAL
    assert lib.glorie_lpips(_lib.ptr(ok), _lib.ptr(ok), 40, 40, 0, *args[:4], 2, args[5]) == -1   # an unknown flag
    assert lib.glorie_lpips(_lib.ptr(ok), _lib.ptr(ok), 40, 40, 0, *args) == 0


def test_weight_shapes_are_validated(gpu):
    from glorie_slam_amd.lpips import Lpips
    wts = R.weights()
    conv = [(torch.tensor(np.array(w)), torch.tensor(np.array(b))) for w, b in wts["conv"]]
    lin = [torch.tensor(np.array(l)) for l in wts["lin"]]
    with pytest.raises(ValueError):
        Lpips(conv[:4], lin, device=gpu)
    with pytest.raises(ValueError):
        Lpips([conv[0], conv[1], conv[3], conv[3], conv[4]], lin, device=gpu)
    with pytest.raises(ValueError):
        Lpips(conv, lin[:4] + [lin[4][:100]], device=gpu)
    # [1,C,1,1] heads are the same heads
    x, y = (_dev(a, gpu) for a in R.case(35, 47)[:2])
    shaped = Lpips(conv, [l.view(1, -1, 1, 1) for l in lin], device=gpu)
    assert torch.equal(shaped(x, y), _metric(gpu)(x, y))


# ---- loading ---------------------------------------------------------------------------------------------------------------
def _state_dicts():
    from glorie_slam_amd.lpips import FEATURE_INDEX
    wts = R.weights()
    conv = [(torch.tensor(np.array(w)), torch.tensor(np.array(b))) for w, b in wts["conv"]]
    lin = {f"lin{l}.model.1.weight": torch.tensor(np.array(w)).view(1, -1, 1, 1) for l, w in enumerate(wts["lin"])}
    torchvision = {}
    package = dict(lin)
    for l, (idx, (w, b)) in enumerate(zip(FEATURE_INDEX, conv)):
        torchvision[f"features.{idx}.weight"], torchvision[f"features.{idx}.bias"] = w, b
        package[f"net.slice{l + 1}.{idx}.weight"], package[f"net.slice{l + 1}.{idx}.bias"] = w, b
    torchvision["classifier.1.weight"] = torch.zeros(4, 4)                  # what else such a file holds
    package["scaling_layer.shift"] = torch.tensor(R.SHIFT).view(1, 3, 1, 1)
    metric = {"net." + k: v for k, v in package.items()}
    metric.update({f"net.lins.{l}.model.1.weight": lin[f"lin{l}.model.1.weight"] for l in range(5)})   # held twice
    return torchvision, lin, package, metric


def test_from_state_dict_and_load(gpu, tmp_path):
    from glorie_slam_amd.lpips import Lpips
    torchvision, lin, package, metric = _state_dicts()
    x, y = (_dev(a, gpu) for a in R.case(35, 47)[:2])
    want = _metric(gpu)(x, y, return_layers=True)
    loaded = [Lpips.from_state_dict(torchvision, lin, device=gpu), Lpips.from_state_dict(package, device=gpu),
              Lpips.from_state_dict(metric, device=gpu)]
    torch.save(torchvision, tmp_path / "alexnet.pth")
    torch.save(lin, tmp_path / "lin.pth")
    torch.save(package, tmp_path / "package.pth")
    loaded += [Lpips.load(str(tmp_path / "alexnet.pth"), str(tmp_path / "lin.pth"), device=gpu),
               Lpips.load(str(tmp_path / "package.pth"), device=gpu)]
    for L in loaded:
        assert torch.equal(L.weights, _metric(gpu).weights)
        got = L(x, y, return_layers=True)
        assert torch.equal(_bits(got[0]), _bits(want[0])) and torch.equal(_bits(got[1]), _bits(want[1]))
    missing = {k: v for k, v in package.items() if not k.startswith("lin3.")}
    with pytest.raises(KeyError, match="lin3"):
        Lpips.from_state_dict(missing, device=gpu)
    with pytest.raises(KeyError):
        Lpips.from_state_dict(torchvision, device=gpu)                        # no lin heads at all
    twice = dict(package)
    twice["other.lin0.model.1.weight"] = package["lin0.model.1.weight"] + 1.0   # two different candidates
    with pytest.raises(KeyError, match="ambiguous"):
        Lpips.from_state_dict(twice, device=gpu)
