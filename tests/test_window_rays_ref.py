"""The numpy restatement of glorie_window_rays against a float64 formulation and against the torch composition on the
CPU, and the host rule of the final refinement's window (keyframe_select.final_refine_window).  No GPU."""
import numpy as np
import pytest
import torch

from window_rays_ref import EPS32, rays_d_f64, scene, torch_composition, window_rays_ref


@pytest.fixture(scope="module", params=["A", "B", "C"])
def case(request):
    s = scene(request.param)
    ref = window_rays_ref(s["depths"], s["images"], s["c2ws"], s["ii"], s["jj"], s["per"], *s["K"],
                          radius_maps=s["radius_maps"])
    return s, ref


def test_restatement_against_float64(case):
    s, (ro, rd, d, col, rad) = case
    rd64, S = rays_d_f64(s["c2ws"], s["ii"], s["jj"], s["per"], *s["K"])
    err = np.abs(rd.astype(np.float64) - rd64)
    # two divisions' worth of roundings on a term (subtraction, division), its product and the two sums: five roundings
    # of relative size EPS32 / 2 on the way of any term
    bound = 5 * EPS32 / 2 * S
    print("max err / bound", float((err / bound).max()))
    assert (err <= bound).all()


def test_restatement_against_torch_cpu(case):
    s, (ro, rd, d, col, rad) = case
    t = lambda x: torch.from_numpy(x)
    tro, trd, td, tcol, trad = torch_composition(t(s["depths"]), t(s["images"]), t(s["c2ws"]), t(s["ii"]), t(s["jj"]),
                                                 s["per"], *s["K"], "cpu", radius_maps=t(s["radius_maps"]))
    assert np.array_equal(tro.numpy(), ro)
    assert np.array_equal(td.numpy(), d)
    assert np.array_equal(tcol.numpy(), col)
    assert np.array_equal(trad.numpy(), rad)
    _, S = rays_d_f64(s["c2ws"], s["ii"], s["jj"], s["per"], *s["K"])
    err = np.abs(trd.numpy().astype(np.float64) - rd.astype(np.float64))
    print("max err / bound", float((err / (5 * EPS32 * S)).max()))
    assert (err <= 5 * EPS32 * S).all()              # at most five roundings of EPS32 / 2 on each side


def test_restatement_modes():
    s = scene("A")
    a = (s["depths"], s["images"], s["c2ws"], s["ii"], s["jj"], s["per"]) + s["K"]
    assert window_rays_ref(*a)[4] is None
    const = window_rays_ref(*a, const_radius=0.06)[4]
    assert const.dtype == np.float32 and (const == np.float32(0.06)).all()
    hwc = window_rays_ref(s["depths"], np.ascontiguousarray(s["images"].transpose(0, 2, 3, 1)), *a[2:],
                          channels_first=False)
    assert np.array_equal(hwc[3], window_rays_ref(*a)[3])
    # the corners of shape A are among the draws
    pairs = set(zip(s["ii"].tolist(), s["jj"].tolist()))
    assert {(0, 0), (s["W"] - 1, 0), (0, s["H"] - 1), (s["W"] - 1, s["H"] - 1)} <= pairs


# ---- keyframe_select.final_refine_window ----------------------------------------------------------------------------------
def _gen(seed=3):
    return torch.Generator(device="cpu").manual_seed(seed)


@pytest.mark.parametrize("mapped,skipped,counter,map_rays", [(8, [], 8, 1000), (8, [7, 2], 8, 1000), (12, [3], 9, 1000),
                                                             (1, [], 1, 1000), (2, [], 2, 10), (3, [], 3, 7),
                                                             (200, [5, 199], 200, 1000), (200, [], 200, 100)])
def test_final_refine_window(mapped, skipped, counter, map_rays):
    from glorie_slam_amd.keyframe_select import final_refine_window
    window, per = final_refine_window(mapped, skipped, counter, map_rays, _gen())
    frames = [f for f in range(mapped) if f not in skipped]
    last, cand = frames[-1], frames[:-1]
    assert window[-1] == last
    sel = window[:-1]
    assert len(set(sel)) == len(sel) and set(sel) <= set(cand)
    assert not set(window) & set(skipped) and last not in sel
    assert len(sel) == min(len(cand), max(counter - 3, 0))
    assert per == max(1, map_rays // (len(window) + 1))
    again = final_refine_window(mapped, skipped, counter, map_rays, _gen())
    assert again == (window, per)


def test_final_refine_window_per_floor_and_seed():
    from glorie_slam_amd.keyframe_select import final_refine_window
    window, per = final_refine_window(200, [], 200, 100, _gen())
    assert len(window) == 198 and per == 1                      # 100 // 199 = 0: the floor
    assert final_refine_window(8, [], 8, 1000, _gen())[1] == 1000 // 7
    other = [final_refine_window(40, [], 40, 1000, _gen(s))[0] for s in (3, 4)]
    assert other[0] != other[1]                                 # the draw comes from the generator


def test_final_refine_window_errors():
    from glorie_slam_amd.keyframe_select import final_refine_window
    from glorie_slam_amd.warp_loss import MAX_FRAMES
    with pytest.raises(ValueError):
        final_refine_window(0, [], 0, 1000, _gen())
    with pytest.raises(ValueError):
        final_refine_window(2, [0, 1], 2, 1000, _gen())
    n = MAX_FRAMES + 3                                          # window: n - 3 selected + the last = MAX_FRAMES + 1
    with pytest.raises(ValueError):
        final_refine_window(n, [], n, 1000, _gen(), pix_warping=True)
    g = _gen()
    state = g.get_state()
    with pytest.raises(ValueError):
        final_refine_window(n, [], n, 1000, g, pix_warping=True)
    assert torch.equal(g.get_state(), state)                    # raised before anything was drawn
    assert len(final_refine_window(n, [], n, 1000, _gen(), pix_warping=None)[0]) == MAX_FRAMES + 1
    assert len(final_refine_window(n - 1, [], n - 1, 1000, _gen(), pix_warping=True)[0]) == MAX_FRAMES
