"""The float64 restatement of the pixel-warping loss (tests/pix_warp_ref.py) against the reference's own
Mapper.pix_warping_loss, pinned in tests/golden/pix_warp.npz (tests/golden/make_pix_warp.py): loss and d loss / d depth of
three cases - rays from every frame of a 5-frame window (a), rays behind cameras / outside the border / with fewer than 4 other
frames (b), a single frame (c: NaN loss, zero gradient)."""
import os

import numpy as np
import pytest
import torch

from pix_warp_ref import pix_warp_loss

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pix_warp.npz")


def load_case(name):
    z = np.load(GOLDEN)
    fx, fy, cx, cy = (float(x) for x in z["intrinsics"])
    H, W = (int(x) for x in z["hw"])
    c = {k[len(name) + 1:]: z[k] for k in z.files if k.startswith(name + "_")}
    c["images"] = z["images"][c["bank"]]
    c.update(fx=fx, fy=fy, cx=cx, cy=cy, H=H, W=W)
    return c


def ref_call(c, depth=None):
    t = torch.from_numpy
    dep = t(c["depth"]).double() if depth is None else depth
    dep = dep.detach().clone().requires_grad_(True)
    loss, mask = pix_warp_loss(t(c["rays_o"]), t(c["rays_d"]), dep, t(c["c2ws"]), c["fx"], c["fy"], c["cx"], c["cy"],
                               c["W"], c["H"], t(c["frame_indices"]), t(c["indices"]), t(c["images"]), t(c["gt"]))
    loss.backward()
    return loss.detach(), dep.grad, mask


@pytest.mark.parametrize("name", ["a", "b"])
def test_restatement_matches_the_reference(name):
    c = load_case(name)
    loss, grad, mask = ref_call(c)
    assert abs(float(loss) - float(c["loss"])) <= 1e-5 * abs(float(c["loss"]))
    g = c["grad"].astype(np.float64)
    assert np.abs(grad.numpy() - g).max() <= 1e-4 * np.abs(g).max()
    assert ((grad.numpy() != 0) == (g != 0)).all()


def test_case_b_covers_every_exclusion():
    c = load_case("b")
    t = torch.from_numpy
    from pix_warp_ref import project
    X = t(c["rays_o"]).double() + t(c["rays_d"]).double() * t(c["depth"]).double()[:, None]
    u, v, zc = project(t(c["c2ws"]).double(), X, c["fx"], c["fy"], c["cx"], c["cy"])
    inside = (u > 5) & (u < c["W"] - 5) & (v > 5) & (v < c["H"] - 5)
    other = t(c["frame_indices"])[None, :] != t(c["indices"])[:, None]
    ok = inside & (zc < 0) & other
    assert (zc > 0).any() and (~inside & (zc < 0)).any()             # behind a camera; in front but outside the border
    n = ok.sum(1)
    assert ((n > 0) & (n < 4)).any() and (n >= 4).any()               # rays dropped by the 4-frame rule, rays kept
    _, _, mask = ref_call(c)
    assert (mask.sum(1) == torch.where(n >= 4, n, torch.zeros_like(n))).all()


def test_single_frame_is_empty():
    c = load_case("c")
    assert np.isnan(c["loss"]) and not c["grad"].any()
    loss, grad, mask = ref_call(c)
    assert torch.isnan(loss) and not mask.any() and (grad == 0).all()


def test_non_finite_depth_is_masked_out():
    c = load_case("a")
    dep = torch.from_numpy(c["depth"]).double()
    dep[:3] = float("nan")
    dep[3] = float("inf")
    loss, grad, mask = ref_call(c, dep)
    assert torch.isfinite(loss) and not mask[:4].any()
    assert torch.isfinite(grad).all() and (grad[:4] == 0).all()
