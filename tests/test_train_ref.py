"""tests/train_ref.py - the float64 reference of the training kernels - pinned on the CPU: against the outputs recorded
from the reference project (tests/golden/decoders.npz, raw2outputs.npz), against finite differences, and against float64
autograd over the project's plain torch modules (an independent statement of the same formulas)."""
import numpy as np
import torch

import train_ref as tr
from test_golden import BruteNPC, _decoder_cfg, gold


def _decoders(seed=43):
    from glorie_slam_amd.decoder import POINT
    torch.manual_seed(seed)
    return POINT(_decoder_cfg(), c_dim=32, hidden_size=128, use_view_direction=True).eval()


def _tensors(dec):
    from glorie_slam_amd.render_train import decoder_tensors
    return [t.detach() for t in decoder_tensors(dec)]


def _golden_inputs(dec):
    f = gold("decoders.npz")
    dec.load_state_dict({k[4:]: torch.from_numpy(f[k]) for k in f.files if k.startswith("sd__")})
    cloud, p, rad = torch.from_numpy(f["cloud"]), torch.from_numpy(f["p"]), torch.from_numpy(f["radius"])
    npc = BruteNPC(cloud)
    D, I, nn = npc.find_neighbors_faiss(p, dynamic_radius=rad)
    g = dec.geo_decoder
    w, has = g._weights(npc, D, nn, rad, False, cloud, I, p)
    return f, cloud, p, I, w.squeeze(-1), has


def test_reference_decoders_match_the_recorded_outputs():
    dec = _decoders()
    f, cloud, p, I, w, has = _golden_inputs(dec)
    pm = f["point_mask"]
    assert np.array_equal(has.numpy(), pm)
    # The outputs were recorded from a float32 evaluation: the float32 run of the reference is held to the tolerance of
    # test_golden.test_decoders_match_reference.  The float64 run of the same code differs from the recording by the
    # recording's own rounding: Fourier phases 2 pi x B reach ~400 rad at these points (|x| ~ 1, B ~ 25 N(0,1), 3 terms),
    # one float32 ulp there is 3e-5, and the 93 / 80 embedding inputs pass through five layers of gain O(1).
    for dtype, rtol, atol in ((torch.float32, 1e-4, 1e-5), (torch.float64, 1e-4, 2e-4)):
        c = lambda t: t.to(dtype)
        with torch.no_grad():
            occ, rgb, pre = tr.decode([c(t) for t in _tensors(dec)], c(p), c(torch.from_numpy(f["views"])), c(cloud),
                                      c(torch.from_numpy(f["geo"])), c(torch.from_numpy(f["col"])), I, c(w), has, True)
        assert pre.shape == (p.shape[0], 160)
        np.testing.assert_allclose(occ[pm].numpy(), f["occ"][pm], rtol=rtol, atol=atol)
        np.testing.assert_allclose(rgb[pm].numpy(), f["rgb"][pm], rtol=rtol, atol=atol)


def test_reference_compositing_matches_the_recorded_outputs():
    f = gold("raw2outputs.npz")
    for dtype in (torch.float64, torch.float32):
        d, c, w = tr.composite(torch.from_numpy(f["raw"]).to(dtype), torch.from_numpy(f["z"]).to(dtype), 0.1)
        for got, key in ((d, "depth"), (c, "rgb"), (w, "weights")):
            np.testing.assert_allclose(got.numpy(), f[key], rtol=1e-5, atol=1e-6)


def _small_case(seed=5, R=2, S=3, Np=7):
    g = torch.Generator().manual_seed(seed)
    Q = R * S
    pts = (torch.rand(Q, 3, generator=g, dtype=torch.float64) - 0.5) * 0.1
    views = torch.randn(Q, 3, generator=g, dtype=torch.float64)
    cloud = (torch.rand(Np, 3, generator=g, dtype=torch.float64) - 0.5) * 0.1
    geo = torch.randn(Np, 32, generator=g, dtype=torch.float64) * 0.3
    col = torch.randn(Np, 32, generator=g, dtype=torch.float64) * 0.3
    I = torch.randint(0, Np, (Q, 8), generator=g)
    w = torch.rand(Q, 8, generator=g, dtype=torch.float64)
    I[1, 5] = -1                                   # a missing neighbour: weight zero, index clamped to row 0
    w[1, 5] = 0.0
    w = w / w.sum(1, keepdim=True)
    has = torch.ones(Q, dtype=torch.bool)
    has[4] = False                                 # a sample without neighbours (its w and I stay in place)
    z = torch.sort(torch.rand(R, S, generator=g, dtype=torch.float64) + 0.5, dim=1).values
    cd = torch.randn(R, generator=g, dtype=torch.float64)
    cc = torch.randn(R, 3, generator=g, dtype=torch.float64)
    return pts, views, cloud, geo, col, I, w, has, z, cd, cc


def test_reference_autograd_passes_gradcheck():
    dec = _decoders()
    P0 = [t.double() for t in _tensors(dec)]
    pts, views, cloud, geo, col, I, w, has, z, cd, cc = _small_case()
    with torch.no_grad():
        occ, _, _ = tr.decode(P0, pts, views, cloud, geo, col, I, w, has, True)
        shift = tr.placeholder_shift(occ, has)     # the -100 assignment as the constant it is for autograd
    assert float(shift[4]) != 0.0 and float(shift.abs().sum()) == abs(float(shift[4]))
    train = [i for i in range(52) if i not in tr.FIXED]

    def fn(gf, cf, *ps):
        P = list(P0)
        for i, p in zip(train, ps):
            P[i] = p
        _, depth, rgb, _ = tr.render(P, pts, views, cloud, gf, cf, I, w, has, z, 0.1, True, shift=shift)
        return depth, rgb

    inputs = [geo.clone().requires_grad_(True), col.clone().requires_grad_(True)] + \
             [P0[i].clone().requires_grad_(True) for i in train]
    assert torch.autograd.gradcheck(fn, inputs, eps=1e-6, atol=1e-6, rtol=1e-4, fast_mode=True)
    # the straight-through form used everywhere else has the same gradient
    a = tr.forward_backward(P0, pts, views, cloud, geo, col, I, w, has, z, 0.1, True, tr.linear_loss(cd, cc))
    depth, rgb = fn(*inputs)
    ((cd * depth).sum() + (cc * rgb).sum()).backward()
    assert torch.equal(a["d_geo"], inputs[0].grad) and torch.equal(a["d_col"], inputs[1].grad)
    for i, t in zip(train, inputs[2:]):
        assert torch.equal(a["grads"][i], t.grad), i
    assert float(a["raw"][4, 3]) == -100.0


def test_reference_gradients_match_autograd_over_the_plain_modules():
    """two independent statements of the same formulas: tests/train_ref.py and glorie_slam_amd.decoder (float64, CPU)"""
    from glorie_slam_amd.common import raw2outputs_nerf_color
    dec = _decoders()
    f, cloud, p, I, w, has = _golden_inputs(dec)
    dec = dec.double()
    dec.use_fused = False
    c = dec.color_decoder
    c.embedder._B, c.embedder_view_direction._B = c.embedder._B.double(), c.embedder_view_direction._B.double()
    # the modules embed `p.float()`: the fixture's points are float32 values, so casting them back loses nothing
    for emb in (dec.geo_decoder.embedder, c.embedder):
        emb.register_forward_pre_hook(lambda mod, args: (args[0].double(),))
    R, S = 12, 10
    views, rad = torch.from_numpy(f["views"]).double(), torch.from_numpy(f["radius"])
    g = torch.Generator().manual_seed(1)
    z = torch.sort(torch.rand(R, S, generator=g, dtype=torch.float64) + 0.5, dim=1).values
    cd = torch.randn(R, generator=g, dtype=torch.float64)
    cc = torch.randn(R, 3, generator=g, dtype=torch.float64)
    geo = torch.from_numpy(f["geo"]).double().requires_grad_(True)
    col = torch.from_numpy(f["col"]).double().requires_grad_(True)

    class NPC(BruteNPC):
        def find_neighbors_faiss(self, q, **kw):
            D, I, nn = super().find_neighbors_faiss(q.float(), **kw)
            return D.double(), I, nn

    raw, _, point_mask, _ = dec(p.double()[None], NPC(cloud), "color", geo, col, pts_num=S, cloud_pos=cloud.double(),
                                pts_views_d=views, dynamic_r_query=rad.double())
    assert torch.equal(point_mask, has) and int((~has).sum()) >= 10
    with torch.no_grad():
        raw[torch.nonzero(~point_mask).flatten(), -1] = -100.0
    depth, _, rgb, _ = raw2outputs_nerf_color(raw.reshape(R, S, 4), z, None, device="cpu", coef=0.1)
    ((cd * depth).sum() + (cc * rgb).sum()).backward()

    from glorie_slam_amd.render_train import decoder_tensors
    ts = decoder_tensors(dec)
    # the modules form the weights in float64 from the float32 distances; hand the reference the same ones
    D, _, nn = NPC(cloud).find_neighbors_faiss(p, dynamic_radius=rad)
    w64, _ = dec.geo_decoder._weights(NPC(cloud), D, nn, rad.double(), False, cloud.double(), I, p.double())
    a = tr.forward_backward(ts, p.double(), views, cloud.double(), geo, col, I, w64.squeeze(-1), has, z, 0.1, True,
                            tr.linear_loss(cd, cc))

    def close(x, y, name):
        scale = float(y.abs().max())
        assert scale > 0, name
        assert float((x - y).abs().max()) <= 1e-10 * scale, name

    close(a["raw"], raw.detach(), "raw")
    close(a["depth"], depth.detach(), "depth")
    close(a["rgb"], rgb.detach(), "rgb")
    close(a["d_geo"], geo.grad, "d_geo")
    close(a["d_col"], col.grad, "d_col")
    n = 0
    for i, t in enumerate(ts):
        if i in tr.FIXED:
            assert a["grads"][i] is None
            continue
        close(a["grads"][i], t.grad, f"tensor {i}")
        n += 1
    assert n == 50


def test_adam_ref_matches_torch_adam_in_float64():
    g = torch.Generator().manual_seed(0)
    p = torch.randn(9, 32, generator=g, dtype=torch.float64)
    lr, b1, b2, eps = (float(np.float32(x)) for x in (3e-3, 0.9, 0.999, 1e-8))
    q = p.clone().requires_grad_(True)
    opt = torch.optim.Adam([q], lr=lr, betas=(b1, b2), eps=eps)
    m, v = torch.zeros_like(p), torch.zeros_like(p)
    for step in range(1, 8):
        grad = torch.randn(9, 32, generator=g, dtype=torch.float64) * step
        q.grad = grad.clone()
        opt.step()
        p, m, v = tr.adam_ref(p, grad, m, v, step, 3e-3, 0.9, 0.999, 1e-8)
        torch.testing.assert_close(p, q.detach(), rtol=1e-12, atol=1e-14)
    mask = torch.arange(9) % 2 == 0
    p2, m2, v2 = tr.adam_ref(p, grad, m, v, 8, 3e-3, 0.9, 0.999, 1e-8, row_mask=mask)
    assert torch.equal(p2[~mask], p[~mask]) and torch.equal(m2[~mask], m[~mask]) and torch.equal(v2[~mask], v[~mask])
    assert not torch.equal(p2[mask], p[mask])
