"""Frame ingest: raw dataset frames -> the working-size tensors of the tracker, on the device (csrc/ingest.hip; reference:
src/utils/datasets.py:60-83 get_color, :85-96 get_intrinsic, :98-137 __getitem__).

The reference undistorts, resizes and converts every frame on the host (cv2.undistort, cv2.resize) and uploads float32.
Here the uint8 frame is uploaded and one launch per batch produces the float images.  `IngestPlan` holds what depends
only on the camera, computed once in numpy and uploaded as small tables:

  map          int32 [H,W,2]: the source position of every undistorted pixel in 1/32 pixel (only with `distortion`)
  xtab, ytab   int32 [W_out,4], [H_out,4]: the two source indices and 11-bit weights of every output column / row of the
               bilinear resize to (H_out + 2 H_edge) x (W_out + 2 W_edge), cropped by the edges
  lut          float32 [256]: level / 255
  ysrc, xsrc   int32 [H_out], [W_out]: the nearest-neighbour source indices of the depth path, cropped

The arithmetic of the kernel is integer and is stated in include/glorie_hip.h; tests/ingest_ref.py restates it in numpy.
"""
import numpy as np
import torch

from . import _lib as L

_REQUIRED = ("H", "W", "fx", "fy", "cx", "cy", "H_out", "W_out")
INTER_BITS, COEF_BITS = 5, 11                        # 1/32-pixel remap positions, 11-bit resize coefficients


def undistort_table(H, W, fx, fy, cx, cy, distortion):
    """int32 [H,W,2] = (ix, iy): rint(32 x) of the distorted position of every pixel, float64 (k1 k2 p1 p2 [k3 [k4 k5 k6]])"""
    d = np.asarray(distortion, np.float64).reshape(-1)
    if d.size not in (4, 5, 8):
        raise ValueError(f"distortion must hold 4, 5 or 8 coefficients (k1 k2 p1 p2 [k3 [k4 k5 k6]]), got {d.size}")
    k1, k2, p1, p2, k3, k4, k5, k6 = np.concatenate([d, np.zeros(8 - d.size)])
    v, u = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    x, y = (u - cx) / fx, (v - cy) / fy
    r2 = x * x + y * y
    kr = (1 + ((k3 * r2 + k2) * r2 + k1) * r2) / (1 + ((k6 * r2 + k5) * r2 + k4) * r2)
    xd = x * kr + 2 * p1 * x * y + p2 * (r2 + 2 * x * x)
    yd = y * kr + p1 * (r2 + 2 * y * y) + 2 * p2 * x * y
    pos = np.stack([xd * fx + cx, yd * fy + cy], -1) * (1 << INTER_BITS)
    # far outside the frame every tap is outside it: the clip changes no pixel and keeps the table in int32
    pos = np.clip(np.nan_to_num(np.rint(pos), nan=-2.0 ** 30), -2.0 ** 30, 2.0 ** 30)
    return np.ascontiguousarray(pos.astype(np.int32))


def resize_table(n_src, n_dst):
    """int32 [n_dst,4] = (s0, s1, a0, a1) of a bilinear resize n_src -> n_dst (pixel centres, 11-bit weights)"""
    f = ((np.arange(n_dst, dtype=np.float64) + 0.5) * (n_src / n_dst) - 0.5).astype(np.float32)
    s = np.floor(f).astype(np.int64)
    f = f - s.astype(np.float32)
    f[s < 0] = 0.0
    s[s < 0] = 0
    f[s >= n_src - 1] = 0.0
    s[s >= n_src - 1] = n_src - 1
    scale = np.float32(1 << COEF_BITS)
    a1 = np.rint(f * scale).astype(np.int64)
    a0 = np.rint((np.float32(1.0) - f) * scale).astype(np.int64)
    return np.stack([s, np.minimum(s + 1, n_src - 1), a0, a1], 1).astype(np.int32)


def nearest_table(n_src, n_dst):
    """int32 [n_dst]: min(int(floorf(dst * (float32(n_src) / float32(n_dst)))), n_src - 1), F.interpolate's 'nearest'"""
    scale = np.float32(n_src) / np.float32(n_dst)
    src = np.floor(np.arange(n_dst, dtype=np.float32) * scale).astype(np.int64)
    return np.minimum(src, n_src - 1).astype(np.int32)


def working_intrinsic(cam):
    """get_intrinsic of src/utils/datasets.py:85-96 for a cam block -> float32 [4] (fx, fy, cx, cy) on the host: scaled to
    the resized frame, the principal point shifted by the crop; the reference's expression, float32 like there"""
    H_edge, W_edge = int(cam.get("H_edge", 0)), int(cam.get("W_edge", 0))
    H_res, W_res = int(cam["H_out"]) + 2 * H_edge, int(cam["W_out"]) + 2 * W_edge
    intrinsic = torch.as_tensor([cam["fx"], cam["fy"], cam["cx"], cam["cy"]]).float()
    intrinsic[0] *= W_res / cam["W"]
    intrinsic[1] *= H_res / cam["H"]
    intrinsic[2] *= W_res / cam["W"]
    intrinsic[3] *= H_res / cam["H"]
    if W_edge > 0:
        intrinsic[2] -= W_edge
    if H_edge > 0:
        intrinsic[3] -= H_edge
    return intrinsic


class IngestPlan:
    """the ingest of one camera block: cam is cfg['cam'] (H, W, fx, fy, cx, cy, H_out, W_out; optional H_edge, W_edge,
    distortion, png_depth_scale).  The tables are built here, once, and live on `device`."""

    def __init__(self, cam, device):
        missing = [k for k in _REQUIRED if k not in cam]
        if missing:
            raise ValueError(f"IngestPlan: cam lacks {missing}")
        self.H, self.W, self.H_out, self.W_out = (int(cam[k]) for k in ("H", "W", "H_out", "W_out"))
        self.fx, self.fy, self.cx, self.cy = (float(cam[k]) for k in ("fx", "fy", "cx", "cy"))
        self.H_edge, self.W_edge = int(cam.get("H_edge", 0)), int(cam.get("W_edge", 0))
        self.png_depth_scale = float(cam.get("png_depth_scale", 1.0))
        if min(self.H, self.W, self.H_out, self.W_out) < 1 or min(self.H_edge, self.W_edge) < 0:
            raise ValueError("IngestPlan: sizes must be positive and edges non-negative")
        self.cam = dict(cam)
        self.device = torch.device(device)
        if self.device.type == "cuda" and self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        distortion = cam.get("distortion")
        H_res, W_res = self.H_out + 2 * self.H_edge, self.W_out + 2 * self.W_edge
        he, we = self.H_edge, self.W_edge
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(self.device)
        self.map = None
        if distortion is not None:
            self.map = up(undistort_table(self.H, self.W, self.fx, self.fy, self.cx, self.cy, distortion))
        self.xtab = up(resize_table(self.W, W_res)[we:we + self.W_out])
        self.ytab = up(resize_table(self.H, H_res)[he:he + self.H_out])
        self.lut = up(np.arange(256, dtype=np.float32) / np.float32(255))
        self.xsrc = up(nearest_table(self.W, W_res)[we:we + self.W_out])
        self.ysrc = up(nearest_table(self.H, H_res)[he:he + self.H_out])

    def _batch(self, t, tail, what):
        if not torch.is_tensor(t):
            raise ValueError(f"{what} must be a tensor")
        L.need_cuda(t)
        if t.dim() == len(tail):
            t = t[None]
        if t.dim() != len(tail) + 1 or tuple(t.shape[1:]) != tail:
            raise ValueError(f"{what} must be [B,{','.join(map(str, tail))}] or one frame of it, got {tuple(t.shape)}")
        if not t.is_contiguous():
            raise ValueError(f"{what} must be contiguous")
        if t.device != self.device:
            raise ValueError(f"{what} lives on {t.device}, the plan on {self.device}")
        return t

    def color(self, frames_u8, swap_rb=False):
        """uint8 [B,H,W,3] (or [H,W,3]) on the device -> float32 [B,3,H_out,W_out] in [0,1].  swap_rb: the frames are BGR"""
        if torch.is_tensor(frames_u8) and frames_u8.dtype != torch.uint8:
            raise ValueError(f"color frames must be uint8, got {frames_u8.dtype}")
        t = self._batch(frames_u8, (self.H, self.W, 3), "color frames")
        B = t.shape[0]
        out = torch.empty(B, 3, self.H_out, self.W_out, dtype=torch.float32, device=self.device)
        L.check(L.load().glorie_ingest_color(L.ptr(t), B, self.H, self.W, L.ptr(self.map), L.ptr(self.xtab),
                                             L.ptr(self.ytab), L.ptr(self.lut), self.H_out, self.W_out, int(bool(swap_rb)),
                                             L.ptr(out), L.stream_ptr(self.device)), "glorie_ingest_color")
        return out

    def depth(self, raw):
        """raw depth [B,H,W] (or [H,W]) uint16 or float32 on the device -> float32 [B,H_out,W_out] = raw / png_depth_scale"""
        codes = {torch.uint16: 0, torch.float32: 1}
        if torch.is_tensor(raw) and raw.dtype not in codes:
            raise ValueError(f"raw depth must be uint16 or float32, got {raw.dtype}")
        t = self._batch(raw, (self.H, self.W), "raw depth")
        B = t.shape[0]
        out = torch.empty(B, self.H_out, self.W_out, dtype=torch.float32, device=self.device)
        L.check(L.load().glorie_ingest_depth(L.ptr(t), codes[t.dtype], B, self.H, self.W, L.ptr(self.ysrc), L.ptr(self.xsrc),
                                             self.png_depth_scale, self.H_out, self.W_out, L.ptr(out),
                                             L.stream_ptr(self.device)), "glorie_ingest_depth")
        return out

    def intrinsic(self):
        """float32 [4] (fx, fy, cx, cy) of the working size: get_intrinsic of src/utils/datasets.py:85-96"""
        return working_intrinsic(self.cam)
