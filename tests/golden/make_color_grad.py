"""Pins of the colour-gradient radii and the gradient-ranked pixel draw against the imported reference (this container
only; the reference never travels):

    python tests/golden/make_color_grad.py

  color_grad.npz  one 96x128 image (flat, smooth and sharp regions: every segment of the radius map, border rows and
                  columns included), stored as uint8 and read as float32 u / 255.
                  - Mapper.run's radius block (src/mapper.py:767-784), Mapper.run called unbound with a namespace `self`
                    whose pipe yields one frame then `end`, whose mapping_keyframe records self.dynamic_r_add /
                    self.dynamic_r_query and returns False; torch.save replaced.  r_add, r_query (float64 -> float32).
                  - get_sample_uv_with_grad (src/utils/common.py:96-118) with a holed valid mask: the magnitude map it
                    ranks (-1 off the mask) and its 5n candidates, np.argpartition wrapped so that its tail comes back
                    sorted (that order is unspecified).  The 5n-th and (5n+1)-th magnitudes differ by >= 1e-5.
                  - get_samples_with_pixel_grad (common.py:121-186) end to end with np.random.choice the identity and the
                    same argpartition: the first n candidates in index order, their rays, depth and colour, the pixels
                    without depth dropped.

Stand-ins: scikit-image is absent here, so `skimage.color.rgb2gray` and `skimage.filters.sobel_h / sobel_v` are restated
as scikit-image 0.20 has them on scipy.ndimage (rgb . [0.2125, 0.7154, 0.0721] in the image's float type;
ndi.convolve with [1,0,-1] x [1,2,1]/4, mode='reflect').  The one assumption is the border: without a mask 0.20 does not
zero the border pixels (0.19 stopped doing so).  Under NumPy 2 the float32 magnitude clipped at float32(thr) compares
above the float64 node thr in interp1d's bounds check, which NumPy 1.23 (the reference's) did in float32; interp1d is
therefore built with fill_value="extrapolate", which evaluates every point exactly as the in-range branch of 1.23 does.
Every other module the import chain of src.mapper lacks becomes a module of MagicMocks (make_pix_warp.import_mapper).
The archive is written with fixed zip timestamps: re-running the script reproduces it bit for bit.
"""
import functools
import os
import sys
import types
from unittest import mock

import numpy as np
import scipy.interpolate
import scipy.ndimage as ndi
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from make_pix_warp import import_mapper, save_npz  # noqa: E402

OUT = os.path.dirname(os.path.abspath(__file__))
H, W = 96, 128
FX, FY, CX, CY = 100.0, 100.0, 63.5, 47.5
CFG = dict(radius_add_max=0.08, radius_add_min=0.02, radius_query_ratio=2, color_grad_threshold=0.15)
N_GRAD = 120                     # get_sample_uv_with_grad's n (600 candidates)


def register_skimage():
    """skimage.color.rgb2gray and skimage.filters.sobel_h / sobel_v of scikit-image 0.20, on scipy.ndimage"""
    def rgb2gray(rgb):
        rgb = np.asarray(rgb)
        return rgb @ np.array([0.2125, 0.7154, 0.0721], dtype=rgb.dtype)

    def _edge(image, axis):
        image = np.asarray(image)
        edge = np.array([1, 0, -1]).reshape((3, 1) if axis == 0 else (1, 3))
        smooth = (np.array([1, 2, 1]) / 4).reshape((1, 3) if axis == 0 else (3, 1))
        return ndi.convolve(image, edge * smooth, mode="reflect")

    sk, color, filters = (types.ModuleType(n) for n in ("skimage", "skimage.color", "skimage.filters"))
    color.rgb2gray = rgb2gray
    filters.sobel_h = lambda image, mask=None: _edge(image, 0)
    filters.sobel_v = lambda image, mask=None: _edge(image, 1)
    sk.color, sk.filters = color, filters
    sys.modules.update({"skimage": sk, "skimage.color": color, "skimage.filters": filters})


def make_image(rng):
    """uint8 [H,W,3]: a flat band on the left, smooth ramps and blobs, a sharp band of steps and noise on the right"""
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)
    img = np.empty((H, W, 3))
    for c in range(3):
        img[..., c] = 0.5 + 0.18 * np.sin(x / (9.0 + 2 * c)) * np.cos(y / (11.0 + c)) + 0.002 * x
    img[:, 8:40] = 0.4                                                       # flat
    band = (x >= 96)
    noise = rng.uniform(0, 1, (H, W, 3))
    img[band] = noise[band]                                                  # sharp
    img[(x >= 70) & (x < 80) & (y > 40)] = 0.9                               # a step
    return np.round(np.clip(img, 0, 1) * 255).astype(np.uint8)


def sorted_argpartition(orig):
    seen = []

    def argpartition(a, kth, axis=-1, **kw):
        idx = orig(a, kth, axis=axis, **kw)
        idx = np.concatenate([idx[:kth], np.sort(idx[kth:])])
        seen.append((np.array(a, copy=True), idx[kth:]))
        return idx
    return argpartition, seen


def radius_block(m, color):
    """Mapper.run up to its first mapping_keyframe -> (dynamic_r_add, dynamic_r_query) float64 [H,W]"""
    frames = iter([{"timestamp": 0, "video_idx": 0, "end": False}, {"timestamp": 1, "video_idx": 0, "end": True}])
    got = {}

    def mapping_keyframe(*a, **k):
        got["r_add"], got["r_query"] = self.dynamic_r_add.clone(), self.dynamic_r_query.clone()
        return False

    gt = torch.from_numpy(color).permute(2, 0, 1)[None]
    self = types.SimpleNamespace(
        pipe=types.SimpleNamespace(recv=lambda: next(frames), send=lambda *_: None), verbose=False, cfg={},
        frame_reader={0: (None, gt, torch.zeros(1, H, W), None)}, device="cpu", use_dynamic_radius=True,
        radius_add_max=CFG["radius_add_max"], radius_add_min=CFG["radius_add_min"],
        radius_query_ratio=CFG["radius_query_ratio"], color_grad_threshold=CFG["color_grad_threshold"], output="-",
        iters_first=1, n_img=1, keyframe_list=[], keyframe_dict=[], mapping_keyframe=mapping_keyframe)
    with mock.patch.object(m, "load_mono_depth", lambda idx, cfg: torch.zeros(H, W)), \
            mock.patch.object(m.torch, "save", lambda *a, **k: None), \
            mock.patch.object(m, "interp1d", functools.partial(scipy.interpolate.interp1d, fill_value="extrapolate")):
        m.Mapper.run(self)
    return got["r_add"].numpy(), got["r_query"].numpy()


def main():
    register_skimage()
    m = import_mapper()
    from src.utils import common
    rng = np.random.default_rng(20261016)
    u8 = make_image(rng)
    color = u8.astype(np.float32) / np.float32(255)
    r_add, r_query = radius_block(m, color)
    g = np.clip(np.sqrt(common.filters.sobel_h(common.rgb2gray(color)) ** 2 +
                        common.filters.sobel_v(common.rgb2gray(color)) ** 2), 0, np.float32(CFG["color_grad_threshold"]))
    segs = [(g <= 0.01).sum(), ((g > 0.01) & (g < np.float32(0.15))).sum(), (g >= np.float32(0.15)).sum()]
    assert min(segs) > 100, segs

    # a holed valid mask, and a depth map with its own holes (picks there are dropped by the depth filter)
    y, x = np.mgrid[0:H, 0:W]
    valid = ~(((y - 30) ** 2 + (x - 100) ** 2 < 12 ** 2) | ((y > 70) & (x > 110)))
    depth = (2.0 + 0.01 * y + 0.005 * x).astype(np.float32)
    depth[(x % 17 == 3) | ((y > 10) & (y < 14))] = 0.0
    c2w = np.eye(4, dtype=np.float32)
    c2w[:3, 3] = [0.1, -0.2, 0.3]
    argp, seen = sorted_argpartition(np.argpartition)
    with mock.patch.object(np, "argpartition", argp):
        cand = common.get_sample_uv_with_grad(0, H, 0, W, N_GRAD, torch.from_numpy(color), torch.from_numpy(valid))
    grad, cand = seen[0]
    assert len(cand) == 5 * N_GRAD
    ranked = np.sort(grad.reshape(-1))[::-1]
    gap = ranked[5 * N_GRAD - 1] - ranked[5 * N_GRAD]
    assert gap >= 1e-5, gap
    seen.clear()
    with mock.patch.object(np, "argpartition", argp), \
            mock.patch.object(np.random, "choice", lambda a, size, replace=True: np.arange(size)):
        ro, rd, d, col, i, j = common.get_samples_with_pixel_grad(
            0, H, 0, W, N_GRAD, H, W, FX, FY, CX, CY, torch.from_numpy(c2w), torch.from_numpy(depth),
            torch.from_numpy(color), "cpu", torch.from_numpy(valid))
    assert np.array_equal(seen[0][0], grad) and np.array_equal(seen[0][1], cand)
    assert np.array_equal(np.sort(j.numpy() * W + i.numpy()), j.numpy() * W + i.numpy())
    out = dict(image_u8=u8, hw=np.array([H, W]), cfg=np.array([CFG[k] for k in ("color_grad_threshold",
                                                                                  "radius_add_max", "radius_add_min",
                                                                                  "radius_query_ratio")]),
               r_add=r_add.astype(np.float32), r_query=r_query.astype(np.float32), valid=valid.astype(np.uint8),
               grad=grad.astype(np.float32), n=np.array(N_GRAD), candidates=cand.astype(np.int64), depth=depth,
               c2w=c2w, intrinsics=np.array([FX, FY, CX, CY], np.float32), s_rays_o=ro.numpy(), s_rays_d=rd.numpy(),
               s_depth=d.numpy(), s_color=col.numpy(), s_i=i.numpy(), s_j=j.numpy())
    path = os.path.join(OUT, "color_grad.npz")
    save_npz(path, out)
    print("segments", segs, "gap", gap, "samples", len(d), "of", N_GRAD)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
