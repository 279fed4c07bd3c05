"""LPIPS of the re-render evaluation on HIP kernels (csrc/lpips.hip; reference: src/utils/eval_render.py:27-28, :64-65,
:85-86, which calls torchmetrics' LearnedPerceptualImagePatchSimilarity(net_type='alex', normalize=True)).

torchmetrics fetches the AlexNet weights from the network; here the caller hands in the weights they already have:

  L = Lpips.load("alexnet.pth", "lpips_alex.pth")        # or Lpips.from_state_dict(sd, lin_sd), or Lpips(conv, lin)
  v = L(x, y)                                            # 0-dim f32 device tensor

The formula (torchmetrics' _LPIPS, version 0.1, eval mode): clamp to [0,1], 2 v - 1, (v - SHIFT) / SCALE, AlexNet's
`features` tapped after each of the five ReLUs, per pixel f / sqrt(NORM_EPS + sum_c f^2) of both images, the lin-weighted
squared difference, the mean over the pixels, the sum over the taps.  f32 features on the exact-f32 MFMA, the score in
fp64 from per-workgroup partials added in a fixed order: repeated calls are bitwise equal, nothing reads the device back,
and every call records into a hipGraph (the workspace is allocated by the caller's allocator before the launches)."""
import ctypes
import re

import torch

from . import _lib as L

SHIFT = (-0.030, -0.088, -0.188)
SCALE = (0.458, 0.448, 0.450)
# torchmetrics' form of the channel normalisation, f / sqrt(NORM_EPS + sum_c f^2) with the eps inside the root; the original
# lpips package divides by sqrt(sum_c f^2) + 1e-10.  The kernel's copy of the constant: kNormEps in csrc/lpips.hip
NORM_EPS = 1e-8
# (Ci, Co, kernel, stride, padding) of AlexNet's features 0, 3, 6, 8, 10; max_pool2d(3, 2) stands before the 2nd and 3rd
LAYERS = ((3, 64, 11, 4, 2), (64, 192, 5, 1, 2), (192, 384, 3, 1, 1), (384, 256, 3, 1, 1), (256, 256, 3, 1, 1))
FEATURE_INDEX = (0, 3, 6, 8, 10)
K_STEP = 4                     # the MFMA's K: conv1's 363 taps are padded to 364
MIN_SIDE = 31                  # conv1 gives 7, the first pool 3, the second 1
FOLD_POOLS = 1                 # GLORIE_LPIPS_FOLD_POOLS (include/glorie_hip.h)


def tap_shapes(H, W):
    """the (h, w) of the five taps of an H x W image (ValueError below 31 x 31)"""
    hw = (ctypes.c_int * 10)()
    if L.load().glorie_lpips_shapes(int(H), int(W), hw) != 0:
        raise ValueError(f"LPIPS needs an image of at least {MIN_SIDE}x{MIN_SIDE} (and at most 16384 a side), got {H}x{W}")
    return [(hw[2 * l], hw[2 * l + 1]) for l in range(5)]


def _find(sd, patterns, what, looked):
    """the one entry of sd whose key ends with one of `patterns` (regular expressions anchored at a name boundary)"""
    hits = [k for k in sd if any(re.search(r"(^|\.)" + p + "$", k) for p in patterns)]
    looked.append(f"{what}: " + " | ".join(p.replace("\\", "") for p in patterns))
    if len(hits) == 1:
        return sd[hits[0]]
    if len(hits) > 1:
        tensors = [sd[k] for k in hits]
        if all(t.shape == tensors[0].shape and torch.equal(t, tensors[0]) for t in tensors[1:]):
            return tensors[0]           # the same tensor under two names (a metric that holds the net twice)
    return hits


class Lpips:
    """LPIPS with the caller's AlexNet and lin weights, packed once and held on `device`.

    conv: five (weight [Co,Ci,k,k], bias [Co]) pairs of AlexNet's features 0, 3, 6, 8, 10; lin: five [C] (or [1,C,1,1])
    weights of the 1x1 heads."""

    def __init__(self, conv, lin, device="cuda", fold_pools=False):
        conv, lin = list(conv), list(lin)
        if len(conv) != 5 or len(lin) != 5:
            raise ValueError(f"expected five convolutions and five lin weights, got {len(conv)} and {len(lin)}")
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise L.GlorieError("Lpips runs on HIP kernels: it needs a GPU device (there is no CPU fallback)")
        packed, biases, lins = [], [], []
        for l, ((w, b), head, (ci, co, k, _, _)) in enumerate(zip(conv, lin, LAYERS)):
            w, b, head = (torch.as_tensor(t).detach().to(torch.float32).cpu() for t in (w, b, head))
            if tuple(w.shape) != (co, ci, k, k) or tuple(b.shape) != (co,):
                raise ValueError(f"convolution {l}: expected weight {(co, ci, k, k)} and bias {(co,)}, got "
                                 f"{tuple(w.shape)} and {tuple(b.shape)}")
            if head.numel() != co or tuple(head.shape) not in ((co,), (1, co, 1, 1)):
                raise ValueError(f"lin {l}: expected [{co}] or [1,{co},1,1], got {tuple(head.shape)}")
            rows = w.permute(2, 3, 1, 0).reshape(k * k * ci, co)            # row (ky k + kx) Ci + c, column = output channel
            kpad = -(-rows.shape[0] // K_STEP) * K_STEP
            packed.append(torch.cat([rows, rows.new_zeros(kpad - rows.shape[0], co)]).reshape(-1))
            biases.append(b)
            lins.append(head.reshape(-1))
        flat = torch.cat(packed + biases + lins).contiguous()
        want = L.load().glorie_lpips_weight_floats()
        if flat.numel() != want:
            raise L.GlorieError(f"packed LPIPS weights hold {flat.numel()} floats, the library expects {want}")
        self.weights = flat.to(self.device)
        self.flags = FOLD_POOLS if fold_pools else 0

    # ---- loading ------------------------------------------------------------------------------------------------------------
    @classmethod
    def from_state_dict(cls, sd, lin_sd=None, device="cuda", **kw):
        """sd (and lin_sd, when the lin heads come in a file of their own) with keys matched by suffix:
        torchvision's features.{0,3,6,8,10}.{weight,bias}, the lpips package's net.slice{1..5}.{0,3,6,8,10}.{weight,bias}
        and lin{0..4}.model.1.weight, or a torchmetrics metric's state dict (the same names under a further prefix).
        A missing or ambiguous key raises KeyError with the list of what was looked for"""
        merged = dict(sd)
        if lin_sd is not None:
            merged.update(lin_sd)
        conv, lin, looked, bad = [], [], [], []
        for l, idx in enumerate(FEATURE_INDEX):
            pair = []
            for part in ("weight", "bias"):
                got = _find(merged, [rf"features\.{idx}\.{part}", rf"slice{l + 1}\.{idx}\.{part}"],
                            f"convolution {l} {part}", looked)
                if isinstance(got, list):
                    bad.append((looked[-1], got))
                pair.append(got)
            conv.append(tuple(pair))
        for l in range(5):
            got = _find(merged, [rf"lin{l}\.model\.1\.weight", rf"lins\.{l}\.model\.1\.weight"], f"lin {l}", looked)
            if isinstance(got, list):
                bad.append((looked[-1], got))
            lin.append(got)
        if bad:
            lines = [f"  {what} -> {'missing' if not hits else 'ambiguous: ' + ', '.join(hits)}" for what, hits in bad]
            raise KeyError("LPIPS weights not found in the state dict (keys are matched by suffix):\n" + "\n".join(lines)
                           + "\nlooked for:\n  " + "\n  ".join(looked))
        return cls(conv, lin, device=device, **kw)

    @classmethod
    def load(cls, path, lin_path=None, device="cuda", **kw):
        """from one torch.save'd state dict that holds everything, or two: AlexNet's and the lin heads'"""
        sd = torch.load(path, map_location="cpu")
        lin_sd = torch.load(lin_path, map_location="cpu") if lin_path is not None else None
        return cls.from_state_dict(sd, lin_sd, device=device, **kw)

    # ---- evaluation ---------------------------------------------------------------------------------------------------------
    def _run(self, x, y, channels_first, want_features):
        L.need_cuda(x, y)
        if tuple(x.shape) != tuple(y.shape):
            raise ValueError(f"images must have the same shape, got {tuple(x.shape)} and {tuple(y.shape)}")
        if x.dim() != 3 or x.shape[0 if channels_first else 2] != 3:
            raise ValueError(f"images must be {'[3,H,W]' if channels_first else '[H,W,3]'}, got {tuple(x.shape)}")
        if x.device != self.weights.device:
            raise ValueError(f"the images are on {x.device}, the weights on {self.weights.device}")
        x, y = L.f32(x), L.f32(y)
        H, W = (x.shape[1], x.shape[2]) if channels_first else (x.shape[0], x.shape[1])
        shapes = tap_shapes(H, W)
        dev = x.device
        lib = L.load()
        ws = L.workspace(lib.glorie_lpips_workspace(int(H), int(W)), dev)
        out = torch.empty(6, dtype=torch.float32, device=dev)
        feats = None
        if want_features:
            sizes = [2 * h * w * co for (h, w), (_, co, _, _, _) in zip(shapes, LAYERS)]
            feats = torch.empty(sum(sizes), dtype=torch.float32, device=dev)
        L.check(lib.glorie_lpips(L.ptr(x), L.ptr(y), int(H), int(W), 1 if channels_first else 0, L.ptr(self.weights),
                                 L.ptr(ws), L.ptr(out), L.ptr(feats), self.flags, L.stream_ptr(dev)), "glorie_lpips")
        if not want_features:
            return out, None
        maps, at = [], 0
        for n, (h, w), (_, co, _, _, _) in zip(sizes, shapes, LAYERS):
            maps.append(feats[at:at + n].view(2, h, w, co))
            at += n
        return out, maps

    def __call__(self, x, y, channels_first=False, return_layers=False):
        """x, y f32 [H,W,3] (or [3,H,W] with channels_first) on the device, at least 31 x 31; values outside [0,1] are
        clamped -> the LPIPS as a 0-dim f32 tensor; with return_layers also [5] f32, the share of every tap.  A
        non-contiguous or non-float32 input is copied first"""
        out, _ = self._run(x, y, channels_first, False)
        return (out[0], out[1:]) if return_layers else out[0]

    def features(self, x, y, channels_first=False):
        """the five ReLU feature maps as f32 [2,h,w,C] (image x, then y), channels innermost"""
        return self._run(x, y, channels_first, True)[1]
