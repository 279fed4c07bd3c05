"""Pins of the pixel-warping loss (the mapper's third term) against the imported reference (this container only; the
reference never travels):

    python tests/golden/make_pix_warp.py

  pix_warp.npz   Mapper.pix_warping_loss (src/mapper.py:326-388, projection src/utils/common.py:324-350) called unbound
                 on CPU with a namespace `self` carrying device="cpu"; its loss and the gradient with respect to `depth`
                 (loss.backward()).  Three cases over one bank of 7 smooth 48x64 colour images:
                   a  M=5 frames, rays from every frame (two thirds of them seen by all four others);
                   b  M=7 frames: one camera turned round (points behind it), one moved aside (points outside the 5-px
                      border), rays with fewer than 4 other frames;
                   c  M=1: every ray is excluded from its own frame -> NaN loss, zero gradient.
                 Every sample keeps >= 1e-2 px from the mask thresholds and from a texel boundary in float64, so fp32
                 rounding cannot flip a mask decision or a bilinear cell.

Stand-ins used while importing (absent third-party packages, never executed by the loss): every module the import chain
of src.mapper names and this environment lacks (cv2, open3d, colorama, wandb, faiss, torchmetrics, pytorch_msssim,
torchvision, skimage, droid_backends, lietorch, torch_scatter) becomes a module whose attributes are MagicMocks.
The archive is written with fixed zip timestamps: re-running the script reproduces it bit for bit.
"""
import io
import os
import sys
import types
import zipfile
from unittest import mock

import numpy as np
import torch

OUT = os.path.dirname(os.path.abspath(__file__))
REF = os.environ.get("GLORIE_REFERENCE", "/root/reference")

H, W = 48, 64
FX, FY, CX, CY = 40.0, 40.0, 31.5, 23.5
EDGE, MARGIN = 5, 1e-2


class _Stub(types.ModuleType):
    __path__ = []

    def __getattr__(self, k):
        if k.startswith("__"):
            raise AttributeError(k)
        v = mock.MagicMock(name=f"{self.__name__}.{k}")
        setattr(self, k, v)
        return v


def import_mapper():
    """src.mapper with every missing third-party module stubbed"""
    if REF not in sys.path:
        sys.path.insert(0, REF)
    for _ in range(64):
        try:
            import src.mapper as m
            return m
        except ModuleNotFoundError as e:
            if e.name.startswith("src"):
                raise
            sys.modules[e.name] = _Stub(e.name)
            for k in [k for k in sys.modules if k == "src" or k.startswith("src.")]:
                del sys.modules[k]
    raise RuntimeError("could not import src.mapper")


def rot(yaw, pitch=0.0):
    cy_, sy_, cp, sp = np.cos(yaw), np.sin(yaw), np.cos(pitch), np.sin(pitch)
    Ry = np.array([[cy_, 0, sy_], [0, 1, 0], [-sy_, 0, cy_]])
    Rx = np.array([[1, 0, 0], [0, cp, -sp], [0, sp, cp]])
    return Ry @ Rx


def c2w(R, t):
    M = np.eye(4)
    M[:3, :3], M[:3, 3] = R, t
    return M


def image_bank(rng, K):
    """smooth colours in [0, 1], quantised to 1/255 (the archive stays small)"""
    low = torch.from_numpy(rng.uniform(0, 1, (K, 3, H // 8, W // 8)))
    img = torch.nn.functional.interpolate(low, size=(H, W), mode="bilinear", align_corners=False)
    return (np.round(img.permute(0, 2, 3, 1).numpy() * 255) / 255).astype(np.float32)


def project(c2ws, X):
    """float64 common.py:324-350: -> u, v, zc [N,M]"""
    w2c = np.linalg.inv(c2ws)
    p = np.einsum("mij,nj->nmi", w2c[:, :3, :3], X) + w2c[None, :, :3, 3]
    a, b, c = p[..., 0], p[..., 1], p[..., 2]
    zc = c + 1e-5
    return (-FX * a + CX * c) / zc, (FY * b + CY * c) / zc, zc


def safe(u, v, zc):
    """no sample near a mask threshold or a texel boundary of its bilinear read"""
    near = lambda x, t: np.abs(x - t) < MARGIN
    bad = near(u, EDGE) | near(u, W - EDGE) | near(v, EDGE) | near(v, H - EDGE) | (np.abs(zc) < MARGIN)
    for q in (u - 0.5, v - 0.5):
        f = q - np.floor(q)
        bad |= np.isfinite(q) & ((f < MARGIN) | (f > 1 - MARGIN))
    return ~bad.any(axis=1)


def draw_rays(rng, c2ws, frames, per_frame, depth_range):
    """rays of the frames `frames` (positions in c2ws) through random pixels (common.py:39-54 direction convention)"""
    o, d, dep, own = [], [], [], []
    for m in frames:
        n = 0
        while n < per_frame:
            i, j = rng.uniform(0, W), rng.uniform(0, H)
            dc = np.array([(i - CX) / FX, -(j - CY) / FY, -1.0])
            dw = c2ws[m, :3, :3] @ dc
            z = rng.uniform(*depth_range)
            X = c2ws[m, :3, 3] + dw * z
            u, v, zc = project(c2ws, X[None].astype(np.float32).astype(np.float64))
            if not safe(u, v, zc)[0]:
                continue
            o.append(c2ws[m, :3, 3])
            d.append(dw)
            dep.append(z)
            own.append(m)
            n += 1
    f32 = lambda x: np.asarray(x, dtype=np.float32)
    return f32(o), f32(d), f32(dep), np.asarray(own)


def run_reference(Mapper, rays_o, rays_d, depth, c2ws, frame_indices, indices, images, gt):
    self = types.SimpleNamespace(device="cpu")
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x))
    dep = t(depth).requires_grad_(True)
    loss = Mapper.pix_warping_loss(self, t(rays_o), t(rays_d), dep, t(c2ws.astype(np.float32)), FX, FY, CX, CY, W, H,
                                   t(frame_indices), t(indices), t(images), t(gt))
    loss.backward()
    return np.float32(loss.detach().numpy()), dep.grad.numpy().astype(np.float32)


def make_case(Mapper, rng, bank, c2ws, frame_indices, per_frame, depth_range, bank_sel):
    M = len(c2ws)
    o, d, dep, own = draw_rays(rng, c2ws, range(M), per_frame, depth_range)
    images = bank[bank_sel]
    # the ray's colour: its own frame at the (nearest) pixel plus noise on both sides of the smooth-L1 knee
    X = o.astype(np.float64) + d.astype(np.float64) * dep[:, None].astype(np.float64)
    u, v, _ = project(c2ws, X)
    pu = np.clip(np.round(u[np.arange(len(own)), own] - 0.5).astype(int), 0, W - 1)
    pv = np.clip(np.round(v[np.arange(len(own)), own] - 0.5).astype(int), 0, H - 1)
    gt = (images[own, pv, pu] + rng.normal(0, 0.1, (len(own), 3))).astype(np.float32)
    indices = frame_indices[own]
    loss, grad = run_reference(Mapper, o, d, dep, c2ws, frame_indices, indices, images, gt)
    return dict(rays_o=o, rays_d=d, depth=dep, c2ws=c2ws.astype(np.float32), frame_indices=frame_indices,
                indices=indices, bank=np.asarray(bank_sel), gt=gt, loss=loss, grad=grad)


def save_npz(path, arrays):
    """np.savez_compressed with fixed zip timestamps"""
    with zipfile.ZipFile(path, "w", compression=zipfile.ZIP_DEFLATED) as z:
        for k, v in arrays.items():
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asarray(v), allow_pickle=False)
            info = zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            z.writestr(info, buf.getvalue())


def main():
    Mapper = import_mapper().Mapper
    torch.manual_seed(0)
    rng = np.random.default_rng(20261016)
    bank = image_bank(rng, 7)
    cases = {}
    # (a) five cameras a short step apart, all facing the same wall
    ca = np.stack([c2w(rot(0.04 * k - 0.08, 0.02 * (k % 2)), [0.15 * k - 0.3, 0.05 * (k % 3), 0.05 * k]) for k in range(5)])
    cases["a"] = make_case(Mapper, rng, bank, ca, np.array([2, 5, 6, 9, 11]), 40, (2.5, 4.0), [0, 1, 2, 3, 4])
    # (b) seven cameras: 0-3 close, 4 turned round, 5 moved far aside, 6 moved aside and up
    cb = [c2w(rot(0.05 * k), [0.2 * k, 0.0, 0.0]) for k in range(4)]
    cb += [c2w(rot(np.pi), [0.3, 0.0, -0.5]), c2w(rot(0.0), [2.6, 0.0, 0.0]), c2w(rot(-0.1, 0.1), [1.2, 1.0, 0.3])]
    cases["b"] = make_case(Mapper, rng, bank, np.stack(cb), np.array([10, 11, 12, 13, 14, 15, 16]), 40, (1.5, 6.0),
                           [6, 5, 4, 3, 2, 1, 0])
    # (c) one frame
    cases["c"] = make_case(Mapper, rng, bank, ca[:1], np.array([3]), 30, (2.5, 4.0), [0])
    assert np.isfinite(cases["a"]["loss"]) and np.isfinite(cases["b"]["loss"])
    assert np.isnan(cases["c"]["loss"]) and not cases["c"]["grad"].any()
    out = dict(images=bank, intrinsics=np.array([FX, FY, CX, CY], np.float32), hw=np.array([H, W]))
    for name, c in cases.items():
        out.update({f"{name}_{k}": v for k, v in c.items()})
    path = os.path.join(OUT, "pix_warp.npz")
    save_npz(path, out)
    for name, c in cases.items():
        print(name, "rays", len(c["depth"]), "loss", c["loss"], "rays with gradient", int((c["grad"] != 0).sum()))
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
