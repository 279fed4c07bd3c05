"""The mapper's per-keyframe visualisation (csrc/vis.hip; reference: src/utils/Visualizer.py, called from
src/mapper.py:664-673): a 4 x 3 contact sheet per mapped keyframe, `{vis_dir}/{idx:05d}_{iter:04d}.jpg`, and with
save_rendered_image the rendered colour as `{img_dir}/frame_{idx:05d}.png`.

The reference copies twelve full-size maps to the host and draws a matplotlib figure at 300 dpi.  Here everything the sheet
needs already is a device tensor; three launches write the sheet as bytes and one device-to-host copy per file takes it
to PIL (imported when the first file is written, as in datasets.py).

  contact_sheet(maps, n_surface, scale, gutter, title)   uint8 [SH,SW,3] on the device
  sheet_ranges(maps)                                     float32 [4] = (dmax, residual min, residual max, 0)
  panel_boxes(H, W, scale, gutter, title)                the twelve panel rectangles (y0, x0, ph, pw)
  to_rgb8(color)                                         saturate(rint(255 x)): what cv2.imwrite stores of a float image
  Visualizer                                             the reference's class: vis_value_only, vis

`maps` holds float [H,W] tensors render_depth, depth, droid_depth, proj_depth, valid_ray_count, sparse_proj_depth,
mono_depth and float [H,W,3] tensors color and gt_color.  The layout and the arithmetic of every byte are stated in
include/glorie_hip.h; tests/vis_ref.py restates them in numpy.  Scalar panels use matplotlib's `plasma` table (PLASMA
below, matplotlib's own data as bytes).
"""
import ctypes
import os

import numpy as np
import torch

from . import _lib as L

MAP_KEYS = ("render_depth", "depth", "color", "gt_color", "droid_depth", "proj_depth", "valid_ray_count",
            "sparse_proj_depth", "mono_depth")
TITLES = ("Input Depth", "Rendered Depth", "Depth Residual", "Input RGB", "Rendered RGB", "RGB Residual", "Droid depth",
          "Pointcloud depth", "Pointcloud mask", "valid counts", "Sparse Pointcloud depth", "Monocular depth")

# (matplotlib.colormaps["plasma"].colors * 255).astype(uint8): 256 entries of r g b
PLASMA = np.frombuffer(bytes.fromhex(
    "0c078610078713068915068a18068b1b068c1d068d1f058e21058f2305902505912705922905932b05942d04942f0495"
    "3104963304973404983604983804993a049a3b039a3d039b3f039c40039c42039d44039e45039e47029f49029f4a02a0"
    "4c02a14e02a14f02a25101a25201a35401a35601a35701a45901a45a00a55c00a55e00a55f00a66100a66200a66400a7"
    "6500a76700a76800a76a00a76c00a86d00a86f00a87000a87200a87300a87500a87601a87801a87901a87b02a87c02a7"
    "7e03a77f03a78104a78204a78405a68506a68607a68807a58908a58b09a48c0aa48e0ca48f0da3900ea3920fa29310a1"
    "9511a19612a09713a099149f9a159e9b179e9d189d9e199c9f1a9ba01b9ba21c9aa31d99a41e98a51f97a72197a82296"
    "a92395aa2494ac2593ad2692ae2791af2890b02a8fb12b8fb22c8eb42d8db52e8cb62f8bb7308ab83289b93388ba3487"
    "bb3586bc3685bd3784be3883bf3982c03b81c13c80c23d80c33e7fc43f7ec5407dc6417cc7427bc8447ac94579ca4678"
    "cb4777cc4876cd4975ce4a75cf4b74d04d73d14e72d14f71d25070d3516fd4526ed5536dd6556dd7566cd7576bd8586a"
    "d95969da5a68db5b67dc5d66dc5e66dd5f65de6064df6163df6262e06461e16560e26660e3675fe3685ee46a5de56b5c"
    "e56c5be66d5ae76e5ae87059e87158e97257ea7356ea7455eb7654ec7754ec7853ed7952ed7b51ee7c50ef7d4fef7e4e"
    "f0804df0814df1824cf2844bf2854af38649f38748f48947f48a47f58b46f58d45f68e44f68f43f69142f79241f79341"
    "f89540f8963ff8983ef9993df99a3cfa9c3bfa9d3afa9f3afaa039fba238fba337fba436fca635fca735fca934fcaa33"
    "fcac32fcad31fdaf31fdb030fdb22ffdb32efdb52dfdb62dfdb82cfdb92bfdbb2bfdbc2afdbe29fdc029fdc128fdc328"
    "fdc427fdc626fcc726fcc926fccb25fccc25fcce25fbd024fbd124fbd324fad524fad624fad824f9d924f9db24f8dd24"
    "f8df24f7e024f7e225f6e425f6e525f5e726f5e926f4ea26f3ec26f3ee26f2f026f2f126f1f326f0f525f0f623eff821"),
    dtype=np.uint8).reshape(256, 3)

_tables = {}          # device -> PLASMA there
_workspaces = {}      # device -> the range pass's partials


def _device_of(t):
    dev = t.device
    return torch.device("cuda", torch.cuda.current_device()) if dev.index is None else dev


def _table(dev):
    if dev not in _tables:
        _tables[dev] = torch.from_numpy(PLASMA.copy()).to(dev)
    return _tables[dev]


def _workspace(dev):
    if dev not in _workspaces:
        _workspaces[dev] = L.workspace(L.load().glorie_vis_ranges_workspace(), dev)
    return _workspaces[dev]


def sheet_size(H, W, scale=2, gutter=4, title=12):
    """(SH, SW) of the sheet of H x W maps"""
    sh, sw = ctypes.c_int(), ctypes.c_int()
    L.check(L.load().glorie_vis_sheet_size(int(H), int(W), int(scale), int(gutter), int(title), ctypes.byref(sh),
                                           ctypes.byref(sw)), "glorie_vis_sheet_size")
    return sh.value, sw.value


def panel_boxes(H, W, scale=2, gutter=4, title=12):
    """the rectangle (y0, x0, ph, pw) of each of the twelve panels on the sheet, row-major; the `title` rows above y0
    belong to the panel's title"""
    if min(H, W, scale) < 1 or min(gutter, title) < 0:
        raise ValueError("panel_boxes: H, W, scale must be positive, gutter and title non-negative")
    ph, pw = -(-H // scale), -(-W // scale)
    return [(gutter + r * (title + ph + gutter) + title, gutter + c * (pw + gutter), ph, pw)
            for r in range(4) for c in range(3)]


def _maps(maps):
    """the nine maps as contiguous float32 device tensors of one size -> (dict, H, W)"""
    missing = [k for k in MAP_KEYS if k not in maps]
    if missing:
        raise ValueError(f"contact sheet: maps lacks {missing}")
    out = {k: L.f32(maps[k]) for k in MAP_KEYS}
    L.need_cuda(*out.values())
    H, W = out["render_depth"].shape if out["render_depth"].dim() == 2 else (0, 0)
    for k, t in out.items():
        want = (H, W, 3) if k in ("color", "gt_color") else (H, W)
        if H < 1 or W < 1 or tuple(t.shape) != want:
            raise ValueError(f"contact sheet: {k} must be {list(want)}, got {list(t.shape)}")
        if t.device != out["render_depth"].device:
            raise ValueError("contact sheet: the maps live on different devices")
    return out, H, W


def _ranges(m, out=None):
    dev = _device_of(m["render_depth"])
    if out is None:
        out = torch.empty(4, dtype=torch.float32, device=dev)
    elif out.dtype != torch.float32 or out.numel() != 4 or not out.is_contiguous() or not out.is_cuda:
        raise ValueError("ranges must be a contiguous float32 device tensor of 4 values")
    L.check(L.load().glorie_vis_ranges(L.ptr(m["render_depth"]), L.ptr(m["depth"]), L.ptr(m["droid_depth"]),
                                       m["render_depth"].numel(), L.ptr(out), L.ptr(_workspace(dev)), L.stream_ptr(dev)),
            "glorie_vis_ranges")
    return out


def sheet_ranges(maps, out=None):
    """float32 [4] on the device: (max droid_depth, min and max of the depth residual, 0), non-finite values skipped.
    Only render_depth, depth and droid_depth are read"""
    m = {k: L.f32(maps[k]) for k in ("render_depth", "depth", "droid_depth")}
    L.need_cuda(*m.values())
    if not (m["render_depth"].shape == m["depth"].shape == m["droid_depth"].shape):
        raise ValueError("sheet_ranges: render_depth, depth and droid_depth must have one shape")
    return _ranges(m, out)


def contact_sheet(maps, n_surface, scale=2, gutter=4, title=12, out=None, ranges=None):
    """the 4 x 3 sheet of `maps` as uint8 [SH,SW,3] (RGB) on the device: the range pass, then one compose launch; no host
    read, so a call can be recorded into a hipGraph (after one eager call, which uploads the colour table).  Panels are
    the maps decimated by `scale`, `gutter` white pixels apart with `title` white rows above each (panel_boxes).
    out: a contiguous uint8 [SH,SW,3] tensor to write into; ranges: a float32 [4] tensor that receives sheet_ranges"""
    m, H, W = _maps(maps)
    dev = _device_of(m["render_depth"])
    SH, SW = sheet_size(H, W, scale, gutter, title)
    if out is None:
        out = torch.empty(SH, SW, 3, dtype=torch.uint8, device=dev)
    elif out.dtype != torch.uint8 or tuple(out.shape) != (SH, SW, 3) or not out.is_contiguous() or out.device != dev:
        raise ValueError(f"out must be a contiguous uint8 [{SH},{SW},3] tensor on {dev}")
    ranges = _ranges(m, ranges)
    L.check(L.load().glorie_vis_compose(*(L.ptr(m[k]) for k in MAP_KEYS), H, W, L.ptr(ranges), float(n_surface),
                                        L.ptr(_table(dev)), int(scale), int(gutter), int(title), L.ptr(out),
                                        L.stream_ptr(dev)), "glorie_vis_compose")
    return out


def to_rgb8(color):
    """float colour (any shape) -> uint8 of that shape on the device: saturate(rint(255 x)), ties to even, NaN -> 0"""
    c = L.f32(color)
    L.need_cuda(c)
    out = torch.empty(c.shape, dtype=torch.uint8, device=c.device)
    L.check(L.load().glorie_vis_rgb8(L.ptr(c), c.numel(), L.ptr(out), L.stream_ptr(_device_of(c))), "glorie_vis_rgb8")
    return out


def save_image(path, rgb8):
    """uint8 [H,W,3] (RGB) on the device -> the file `path` (its suffix picks the format): one device-to-host copy"""
    from PIL import Image                                   # only when a file is actually written
    Image.fromarray(rgb8.cpu().numpy()).save(path)


def draw_titles(image, boxes, titles=TITLES, title=12):
    """write the panel titles into the title strips of a PIL image of the sheet, PIL's built-in font, centred, clipped to
    the panel's width"""
    from PIL import Image, ImageDraw, ImageFont
    font = ImageFont.load_default()
    for (y0, x0, _, pw), text in zip(boxes, titles):
        if title < 1 or pw < 1:
            continue
        left, top, right, bottom = font.getbbox(text)
        strip = Image.new("RGB", (pw, title), (255, 255, 255))
        ImageDraw.Draw(strip).text((max((pw - (right - left)) // 2, 0) - left, max((title - bottom) // 2, 0)), text,
                                   fill=(0, 0, 0), font=font)
        image.paste(strip, (x0, y0 - title))
    return image


def camera_matrix(c2w_or_camera_tensor, device):
    """a [4,4] (or [3,4]) camera-to-world matrix as it is; a camera tensor [qw qx qy qz tx ty tz] as its 4 x 4 matrix"""
    t = c2w_or_camera_tensor
    if t.dim() != 1:
        return t
    q, trans = t[:4].detach().to(device, torch.float32), t[4:7].detach().to(device, torch.float32)
    w, x, y, z = q.unbind(-1)
    s = 2.0 / (q * q).sum()
    c2w = torch.eye(4, dtype=torch.float32, device=device)
    c2w[:3, :3] = torch.stack([
        torch.stack([1 - s * (y * y + z * z), s * (x * y - z * w), s * (x * z + y * w)]),
        torch.stack([s * (x * y + z * w), 1 - s * (x * x + z * z), s * (y * z - x * w)]),
        torch.stack([s * (x * z - y * w), s * (y * z + x * w), 1 - s * (x * x + y * y)])])
    c2w[:3, 3] = trans
    return c2w


class Visualizer(object):
    """Visualizer of src/utils/Visualizer.py:12-219 with its constructor and method signatures.  scale, gutter, title:
    the layout of the sheet; titles=False leaves the title strips white; keep=True appends every composed sheet with
    its maps, as device tensors, to `kept`."""

    def __init__(self, vis_dir, renderer, verbose, device='cuda:0', logger=None, total_iters=None, img_dir=None,
                 scale=2, gutter=4, title=12, titles=True, keep=False):
        self.device = device
        self.vis_dir = vis_dir
        self.verbose = verbose
        self.renderer = renderer
        self.logger = logger
        self.total_iters = total_iters
        self.img_dir = img_dir
        self.scale, self.gutter, self.title, self.titles = int(scale), int(gutter), int(title), bool(titles)
        self.keep, self.kept = bool(keep), []
        self.written = []                                    # the files written, in order
        os.makedirs(f'{vis_dir}', exist_ok=True)

    @torch.no_grad()
    def vis_value_only(self, render_depth, c2w_or_camera_tensor, npc, decoders, npc_geo_feats, npc_col_feats,
                       dynamic_r_query=None, cloud_pos=None):
        """the rendered depth, colour, valid ray mask and valid sample counts of one view (Visualizer.py:30-54)"""
        c2w = camera_matrix(c2w_or_camera_tensor, self.device)
        depth, _, color, valid_ray_mask, valid_ray_count = self.renderer.render_img(
            npc, decoders, c2w, self.device, stage='color', gt_depth=render_depth, npc_geo_feats=npc_geo_feats,
            npc_col_feats=npc_col_feats, dynamic_r_query=dynamic_r_query, cloud_pos=cloud_pos)
        return depth, color, valid_ray_mask, valid_ray_count

    @torch.no_grad()
    def vis(self, idx, iter, gt_depth, render_depth, droid_depth, mono_depth, gt_color, c2w_or_camera_tensor, npc,
            decoders, npc_geo_feats, npc_col_feats, cfg, printer, freq_override=False, dynamic_r_query=None,
            cloud_pos=None, cur_total_iters=None, save_rendered_image=False):
        """Visualizer.vis (Visualizer.py:57-219): when (idx > 0 and iter == cur_total_iters - 1) or freq_override, render
        the view, project the cloud twice, compose the sheet and write `{vis_dir}/{idx:05d}_{iter:04d}.jpg`; with
        save_rendered_image and an img_dir also `{img_dir}/frame_{idx:05d}.png` of the rendered colour.  gt_depth is
        accepted and unused, as in the reference.  cfg: cam (or the renderer's camera), mapping.mapping_window_size and
        rendering.N_surface are read.  Pointcloud depth is the projection of the unprojected keyframe maps where the
        cloud keeps them, else of the neural points.  -> the sheet (device uint8 [SH,SW,3], titles not drawn) or None"""
        from .neural_point import proj_depth_map
        if not ((idx > 0 and (cur_total_iters is not None and iter == cur_total_iters - 1)) or freq_override):
            return None
        dev = self.device
        c2w = camera_matrix(c2w_or_camera_tensor, dev)
        depth, color, _, valid_ray_count = self.vis_value_only(render_depth, c2w, npc, decoders, npc_geo_feats,
                                                               npc_col_feats, dynamic_r_query, cloud_pos)
        if save_rendered_image and self.img_dir is not None:
            os.makedirs(f'{self.img_dir}', exist_ok=True)
            path = os.path.join(f'{self.img_dir}', f'frame_{idx:05d}.png')
            save_image(path, to_rgb8(color))
            self.written.append(path)
        dense = npc.full_pcl() is not None and getattr(npc, "video", None) is not None
        proj_depth = proj_depth_map(c2w.clone(), npc, dev, cfg, neural_pcl=not dense)
        s_proj_depth = proj_depth_map(c2w, npc, dev, cfg, neural_pcl=True)
        maps = dict(render_depth=render_depth, depth=depth, color=color, gt_color=gt_color, droid_depth=droid_depth,
                    proj_depth=proj_depth, valid_ray_count=valid_ray_count, sparse_proj_depth=s_proj_depth,
                    mono_depth=mono_depth)
        sheet = contact_sheet(maps, cfg["rendering"]["N_surface"], self.scale, self.gutter, self.title)
        fig_name = f'{self.vis_dir}/{idx:05d}_{iter:04d}.jpg'
        self._write_sheet(fig_name, sheet, tuple(render_depth.shape))
        if self.keep:
            self.kept.append(dict(idx=idx, iter=iter, sheet=sheet, maps=maps, c2w=c2w))
        if 'mapping' in str(self.vis_dir) and self.logger is not None and hasattr(self.logger, "log"):
            self.logger.log({f'Mapping_{idx:05d}_{iter:04d}': fig_name})
        if self.verbose and printer is not None:
            printer.print(f'Saved rendering visualization of color/depth image at {self.vis_dir}/'
                          f'{idx:05d}_{iter if cur_total_iters is None else cur_total_iters:04d}.jpg')
        return sheet

    def _write_sheet(self, path, sheet, shape):
        from PIL import Image
        image = Image.fromarray(sheet.cpu().numpy())         # the one device-to-host copy of this file
        if self.titles:
            draw_titles(image, panel_boxes(shape[0], shape[1], self.scale, self.gutter, self.title), title=self.title)
        image.save(path, quality=90)
        self.written.append(path)
