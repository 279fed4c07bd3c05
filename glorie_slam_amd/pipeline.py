"""Tracking + mapping composed on one stream of frames (BASELINE config 3: a full sequence on one GPU).

The reference runs a tracker process and a mapper process around shared memory (src/slam.py:119-126 spawns them;
src/tracker.py:33-77 is the per-frame loop `MotionFilter.track -> Frontend() -> periodic Backend.dense_ba`;
src/mapper.py:517-684 is the per-keyframe loop `add_neural_points -> optimise features + decoders against the keyframe's
depth and colour`; slam.py / tracker.py end with a final global BA).  Process orchestration, the mono-depth network, pose
evaluation and the mapper's keyframe-selection heuristics are out of scope; what is in scope are the
callers' CALL SHAPES, because they decide whether the hot-path pieces compose: the frontend's local graph with its
hipGraph replays and slot arena, the backend's throw-away low-memory graphs over the same video buffers, the cloud's cell
list being rebuilt under the renderer, the training path feeding FeatureAdam with tables that grow between keyframes.
`SequenceRunner` is that composition in one process, in the order the reference's two loops interleave when the mapper
keeps up with the tracker (every kept keyframe is mapped before the next frame is tracked).
"""
import time
import types

import torch

from .backend import Backend
from .color_grad import (COLOR_GRAD_THRESHOLD, RADIUS_ADD_MAX, RADIUS_ADD_MIN, RADIUS_QUERY_RATIO, color_grad_maps,
                         get_samples_with_pixel_grad)
from .common import get_rays_from_uv
from .frontend import Frontend
from .keyframe_select import final_refine_window, frustum_feature_mask, keyframe_selection_overlap, random_select
from .map_sample import DRAW_RANGE, ValidIndex, depth_gate, sample_window_rays
from .motion_filter import MotionFilter
from .neural_point import deform_points, proxy_render_depth, se3_inv, update_points_pos
from .render_train import FeatureAdam
from .warp_loss import MAX_FRAMES as MAX_WARP_FRAMES
from .warp_loss import FrameTable, pix_warping_loss
from .window_rays import WindowTable, window_rays

# the master config's learning rates of the mapping stages (cfg['mapping'][init | stage][geometry | color])
MAPPING_RATES = {"geometry": {"decoders_lr": 0.001, "geometry_lr": 0.03, "color_lr": 0.0},
                 "color": {"decoders_lr": 0.005, "geometry_lr": 0.005, "color_lr": 0.005}}


class _CfgVideo:
    """a DepthVideo seen with another cfg (the torch deformation driver reads the render depth mode and the camera from
    video.cfg); everything else is the video's own"""

    def __init__(self, video, cfg):
        self._video, self.cfg = video, cfg

    def __getattr__(self, name):
        return getattr(self._video, name)


def pose_matrix(pose7):
    """[tx ty tz qx qy qz qw] -> 4x4"""
    t, q = pose7[:3], pose7[3:]
    x, y, z, w = q.unbind(-1)
    R = torch.stack([torch.stack([1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)]),
                     torch.stack([2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)]),
                     torch.stack([2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)])])
    M = torch.eye(4, device=pose7.device, dtype=pose7.dtype)
    M[:3, :3] = R
    M[:3, 3] = t
    return M


class SequenceRunner:
    """net: DroidNet-like (fnet, cnet, update); video: DepthVideo; npc / decoders / renderer: the neural point cloud side.
    mono_depth_fn(tstamp, image) -> [H,W] depth prior (the reference reads it from the estimator's output directory)."""

    def __init__(self, net, video, cfg, npc, decoders, renderer, mono_depth_fn, use_graphs=True, ba_every=4, ba_steps=2,
                 map_iters=20, map_rays=1000, add_stride=8, seed=43, pix_warping=None, w_pix_warp_loss=None,
                 mapping_window_size=None, keyframe_selection_method=None, frustum_feature_selection=None,
                 frustum_edge=None, color_grad_radius=None, pixels_based_on_color_grad=None, bind_npc_with_pose=None,
                 render_depth=None, use_mono_to_complete=None, mapping_schedule=False, mapping_vis=None,
                 save_rendered_image=None, near_pcl_path="host"):
        self.net, self.video, self.cfg = net, video, cfg
        self.npc, self.decoders, self.renderer = npc, decoders, renderer
        # rays without a depth prior (Renderer.near_pcl_path): "device" keeps the renders of evaluate(), of the contact
        # sheets and of final_refine on the HIP path when a frame's depth has holes; "host" is the reference's route
        renderer.near_pcl_path = near_pcl_path              # (anything else is a ValueError)
        dev = cfg["device"]
        self.device = dev
        self.filter = MotionFilter(net, video, cfg, thresh=cfg["tracking"].get("motion_filter", {}).get("thresh", 0.0),
                                   device=dev, mono_depth_fn=mono_depth_fn)
        self.frontend = Frontend(net, video, cfg, use_graphs=use_graphs)
        self.backend = Backend(net, video, cfg)
        self.ba_every, self.ba_steps = ba_every, ba_steps
        self.map_iters, self.map_rays, self.add_stride = map_iters, map_rays, add_stride
        self.gen = torch.Generator(device="cpu").manual_seed(seed)
        self.images = {}                      # keyframe index -> [3,H,W] colour image (what video.images stores in the reference)
        self.mapped = 0                       # keyframes [0, mapped) are in the cloud
        self.last_ba = 0
        self.losses = []                      # per mapped keyframe: (first, last) loss of its mapping iterations
        self.timing = {"track_ms": [], "map_iter_ms": [], "ba_ms": [], "kept": []}
        # record the mapping iteration into a hipGraph per keyframe (map_keyframe).  Off by default: built and measured in
        # round 5 (tools/prof_map_graph.py) - recording 3.3 ms per keyframe, a replay 2.26 ms against 2.0-2.5 ms for an eager
        # iteration at 1000 rays: the iteration is ~110 small launches whose device-side latency a replay does not shorten
        # (the sum of its kernel durations IS its wall time, profiles/r04_train_kernel_stats.csv), not host-bound as the
        # round-4 notes had it.  What would shorten it is fewer launches (fused layers in csrc/train.hip).
        self.map_graph = False
        self.map_graph_stats = {"captures": 0, "replays": 0}
        self.init_state = None                # callable(k, tstamp): the tracker's initial guess for a new keyframe (tests)
        # the pixel-warping term (mapper.py:326-388, :502-507) over a window of keyframes: cfg["mapping"] keys of the
        # reference config or the constructor arguments; off by default (window 1, the loss of map_keyframe unchanged)
        mp = cfg.get("mapping", {})
        self.pix_warping = bool(mp.get("pix_warping", False) if pix_warping is None else pix_warping)
        self.w_pix_warp_loss = float(mp.get("w_pix_warp_loss", 1000.0) if w_pix_warp_loss is None else w_pix_warp_loss)
        self.mapping_window_size = int(mp.get("mapping_window_size", 1) if mapping_window_size is None
                                       else mapping_window_size)
        self.warp_losses = []                 # per mapped keyframe with pix_warping: (first, last) value of the warp term
        # keyframe selection (mapper.py:541-554) and frustum feature selection (:591-595, :675-677): cfg["mapping"] keys
        # or the constructor arguments (keyframe_selection_method=False: off whatever the config says).  Without a
        # method the window is k alone, or k and the most recent keyframes with pix_warping; with one it is the selected
        # keyframes of [0, k-1), then k-1, then k
        method = mp.get("keyframe_selection_method") if keyframe_selection_method is None else keyframe_selection_method
        if method not in (None, False, "", "overlap", "global"):
            raise ValueError(f"keyframe_selection_method must be 'overlap' or 'global', got {method!r}")
        self.keyframe_selection_method = method or None
        self.frustum_feature_selection = bool(mp.get("frustum_feature_selection", False)
                                              if frustum_feature_selection is None else frustum_feature_selection)
        self.frustum_edge = float(mp.get("frustum_edge", -4) if frustum_edge is None else frustum_edge)
        self.windows = []                     # per mapped keyframe: its mapping window (keyframe ids, k last)
        self.frustum_counts = []              # per mapped keyframe with frustum selection: the number of trained points
        self.map_probe = None                 # callable(k, dict of the iteration's tensors), eager iterations only (tests)
        # colour-gradient search radii (mapper.py:767-784): on when the cloud uses dynamic radii and cfg["pointcloud"] has
        # the four keys, or by the constructor argument (True without the keys: the master config's values).  Insertion
        # rays then take dynamic_r_add / 3 * depth of their pixel, training rays their frame's dynamic_r_query / 3 * depth;
        # off, every ray keeps the constant 0.5 * (radius_add + radius_query)
        pc = cfg.get("pointcloud", {})
        keys = ("radius_add_max", "radius_add_min", "radius_query_ratio", "color_grad_threshold")
        on = (bool(getattr(npc, "use_dynamic_radius", False)) and all(k in pc for k in keys)) \
            if color_grad_radius is None else bool(color_grad_radius)
        if on and not getattr(npc, "use_dynamic_radius", False):
            raise ValueError("color_grad_radius needs a point cloud with use_dynamic_radius")
        self.color_grad = dict(color_grad_threshold=float(pc.get("color_grad_threshold", COLOR_GRAD_THRESHOLD)),
                               radius_add_max=float(pc.get("radius_add_max", RADIUS_ADD_MAX)),
                               radius_add_min=float(pc.get("radius_add_min", RADIUS_ADD_MIN)),
                               radius_query_ratio=float(pc.get("radius_query_ratio", RADIUS_QUERY_RATIO))) if on else None
        # the second anchoring pass on the pixels of highest colour gradient (mapper.py:312-322): cfg["mapping"] key or
        # the constructor argument; 0 is off
        self.pixels_based_on_color_grad = int(mp.get("pixels_based_on_color_grad", 0)
                                              if pixels_based_on_color_grad is None else pixels_based_on_color_grad)
        # deformation of the cloud after tracker updates (mapper.py:705-707) and the depth the mapper trains on
        # (mapper.py:246-279, :557-573, :713-730): cfg["pointcloud"]["bind_npc_with_pose"], cfg["mapping"]["render_depth"]
        # ("proxy" / "mono") and ["use_mono_to_complete"], or the constructor arguments.  Off, the view depth stays
        # 1 / disps_up and nothing is deformed
        self.bind_npc_with_pose = bool(pc.get("bind_npc_with_pose", False) if bind_npc_with_pose is None
                                       else bind_npc_with_pose)
        mode = mp.get("render_depth") if render_depth is None else render_depth
        if mode not in (None, False, "", "proxy", "mono"):
            raise ValueError(f"render_depth must be 'proxy' or 'mono', got {mode!r}")
        self.render_depth = mode or None
        self.use_mono_to_complete = bool(mp.get("use_mono_to_complete", True) if use_mono_to_complete is None
                                         else use_mono_to_complete)
        self.mono_depth_fn = mono_depth_fn
        self.mono_priors = {}                 # keyframe -> its mono prior (keyframe_dict['mono_depth'])
        self._mono_by_tstamp = {}             # timestamp -> mono prior (device, [H,W] f32: 1.2 MB at 640x480)
        self.skipped = []                     # keyframes not mapped: fewer than 100 valid tracker depths
        self.deform_stats = {"calls": 0, "dirty_keyframes": 0, "points_moved": 0}
        self._deform_counts = None            # device int64 [dirty keyframes, points moved], read once per keyframe
        self._render_views = None             # inside map_keyframe with render_depth: frame -> (depth, c2w) or None
        self.refine_losses = []               # final_refine: (first, last) loss per outer pass
        self.refine_windows = []              # final_refine: the window of every outer pass (keyframe ids)
        # the reference's mapping schedule (mapper.py:390-515, :598-638), opt-in: every window frame's rays drawn among
        # its valid pixels and gated by min(10 median, 1.2 max) (map_sample.py), a geometry stage before the colour stage
        # with the stage's learning rates, and the iteration count scaled by the inserted points.  Off, map_keyframe
        # runs its one-stage loop unchanged
        self.mapping_schedule = bool(mapping_schedule)
        stages = {s: {sub: dict(MAPPING_RATES[sub], **mp.get(s, {}).get(sub, {})) for sub in ("geometry", "color")}
                  for s in ("init", "stage")}
        self.schedule = dict(rates=stages, geo_iter_first=int(mp.get("geo_iter_first", 400)),
                             geo_iter_ratio=float(mp.get("geo_iter_ratio", 0.3)),
                             min_iter_ratio=float(mp.get("min_iter_ratio", 0.95)),
                             fix_geo_decoder=bool(mp.get("fix_geo_decoder", True)),
                             fix_color_decoder=bool(mp.get("fix_color_decoder", False)),
                             iters_first=int(mp.get("iters_first", map_iters)), iters=int(mp.get("iters", map_iters)),
                             w_geo_loss=float(mp.get("w_geo_loss", 1.0)), w_color_loss=float(mp.get("w_color_loss", 0.5)),
                             pixels_adding=int(mp["pixels_adding"]) if mp.get("pixels_adding") else None)
        self.schedules = []                   # per keyframe mapped on the schedule: (iterations, of them geometry stage)
        # the per-keyframe contact sheet (mapper.py:664-673, visualizer.py), opt-in: mapping_vis is a directory, or True
        # for <output>/mapping_vis with `output` the run's directory (run(output=...) or the attribute); with
        # save_rendered_image (the argument, else cfg["mapping"]["save_rendered_image"]) the rendered colour goes to
        # rendered_image/ next to it.  Off, nothing below is touched
        self.mapping_vis = None if mapping_vis in (None, False) else mapping_vis
        self.save_rendered_image = bool(mp.get("save_rendered_image", False) if save_rendered_image is None
                                        else save_rendered_image)
        self.output = None
        self.visualizer = None                # created with the first sheet
        self.vis_options = {}                 # Visualizer keywords (scale, gutter, title, titles, keep, logger)
        self._vis_depths = None               # with render_depth: (aligned mono prior, tracker depth) of the keyframe

    # ---- tracker.py:33-77 ------------------------------------------------------------------------------------------
    @torch.no_grad()
    def track(self, tstamp, image, intrinsics):
        """one frame: motion filter, local BA-update iterations, periodic global BA.  Returns True if the frame was kept"""
        t0 = time.perf_counter()
        n_before = self.video.counter.value
        self.filter.track(tstamp, image, intrinsics)
        appended = self.video.counter.value > n_before
        if appended:
            self.images[n_before] = image[0].to(self.device)
            if self.init_state is not None:
                self.init_state(n_before, tstamp)
        self.frontend()
        kept = appended and self.video.counter.value > n_before
        cur = self.video.counter.value
        torch.cuda.synchronize()
        self.timing["track_ms"].append(1e3 * (time.perf_counter() - t0))      # motion filter + frontend of this frame
        self.timing["kept"].append(bool(kept))
        if self.frontend.is_initialized and cur - self.last_ba >= self.ba_every and self.ba_every > 0:
            tb = time.perf_counter()
            self.backend.dense_ba(self.ba_steps)
            torch.cuda.synchronize()
            self.timing["ba_ms"].append(1e3 * (time.perf_counter() - tb))
            self.last_ba = cur
        return kept

    # ---- mapper.py:517-684 (one keyframe) ---------------------------------------------------------------------------
    def _keyframe_view(self, k):
        """depth map and camera-to-world matrix of keyframe k (constant while the keyframe is mapped); with render_depth,
        inside map_keyframe, the render depth of the frames computed for it (_render_view)"""
        if self._render_views is not None and self._render_views.get(k) is not None:
            return self._render_views[k]
        v = self.video
        depth = torch.where(v.disps_up[k] > 0, 1.0 / v.disps_up[k].clamp_min(1e-6), torch.zeros_like(v.disps_up[k]))
        c2w = pose_matrix(se3_inv(v.poses[k]))
        # the neural point cloud lives in the OpenGL camera convention of the renderer (common.py:302-322)
        c2w = c2w.clone()
        c2w[:3, 1] *= -1
        c2w[:3, 2] *= -1
        return depth, c2w

    def _keyframe_rays(self, k, stride=1, count=None, view=None, pix=None, radius_map=None):
        """pixels of keyframe k with a valid depth -> rays, depth, colour, pixel ids (common.py:39-54 ray convention).
        view: `_keyframe_view(k)` computed by the caller; pix: the (ii, jj) pixel draw of this call, already on the device
        (the mapping loop draws all its iterations at once: a per-iteration host-to-device copy from pageable memory blocks
        the host until the stream has drained); radius_map: a per-pixel [H,W] radius of keyframe k (_radius_maps) the rays
        gather from, else the constant one"""
        v = self.video
        H, W = v.ht, v.wd
        cam = self.renderer
        depth, c2w = view if view is not None else self._keyframe_view(k)
        if pix is not None:
            ii, jj = pix
        elif count is None:
            jj, ii = torch.meshgrid(torch.arange(stride // 2, H, stride, device=self.device),
                                    torch.arange(stride // 2, W, stride, device=self.device), indexing="ij")
            ii, jj = ii.reshape(-1), jj.reshape(-1)
        else:
            ii = torch.randint(0, W, (count,), generator=self.gen).to(self.device)
            jj = torch.randint(0, H, (count,), generator=self.gen).to(self.device)
        ro, rd = get_rays_from_uv(ii.float(), jj.float(), c2w, cam.fx, cam.fy, cam.cx, cam.cy, self.device)
        d = depth[jj, ii]
        col = self.images[k][:, jj, ii].t().contiguous()
        radius = None
        if radius_map is not None:
            radius = radius_map[jj, ii]
        elif self.npc.use_dynamic_radius:
            radius = torch.full_like(d, self._const_radius())
        return ro.reshape(-1, 3).contiguous(), rd.reshape(-1, 3).contiguous(), d, col, ii, jj, radius

    def map_keyframe(self, k):
        """seed the keyframe's points, then `map_iters` iterations on `map_rays` of its pixels (depth + colour L1,
        mapper.py:497-505; learning rates of the colour stage, mapper.py:412-414).  With pix_warping on or a
        keyframe_selection_method, the rays are split over a window of keyframes (_map_window); with pix_warping the
        pixel-warping term joins the loss (warp_loss.py).  With frustum_feature_selection only the feature rows inside
        the keyframe's frustum are trained (keyframe_select.py; FeatureAdam's row masks).  With bind_npc_with_pose the
        cloud is deformed first; with render_depth the keyframe is inserted on its anchor depth and every window frame
        trains on its render depth (proxy or aligned mono), and a frame with too few tracker depths is skipped.  With
        mapping_schedule the iterations follow the reference's schedule instead (_optimize_scheduled).  With mapping_vis
        the keyframe's contact sheet is written after its last iteration (_visualize)"""
        npc = self.npc
        self._render_views = None
        self._vis_depths = None
        try:
            with torch.no_grad():
                if self.bind_npc_with_pose and npc.pts_num() > 0:
                    self._deform()
                anchor = None
                if self.render_depth is not None:
                    anchor = self._prepare_render(k)
                    if anchor is None:
                        self.skipped.append(k)
                        return None
                # colour-gradient radii of k scaled by its depth: (r_add, r_query) [H,W], or None
                ins_view = anchor if anchor is not None else self._keyframe_view(k)
                query_depth = self._keyframe_view(k)[0] if anchor is not None else None
                rmaps = self._radius_maps(k, ins_view, query_depth=query_depth) if self.color_grad is not None else None
                if self.mapping_schedule and self.schedule["pixels_adding"]:
                    # pixels_adding pixels drawn among the anchor depth's valid ones (mapper.py:297-303)
                    ro, rd, d, col, radius, ii, jj = self._insertion_samples(k, ins_view, rmaps)
                else:
                    ro, rd, d, col, ii, jj, radius = self._keyframe_rays(k, stride=self.add_stride, view=ins_view,
                                                                         radius_map=rmaps[0] if rmaps else None)
                added = [npc.add_neural_points(ro, rd, d, col, k, ii, jj, dynamic_radius=radius)]
                if self.pixels_based_on_color_grad > 0:
                    added.append(self._anchor_grad_points(k, rmaps, view=ins_view))
            if npc.pts_num() == 0:
                return None
            # frame_pts_add (mapper.py:305-324): one host read per keyframe on the schedule
            return self._optimize_keyframe(k, rmaps, sum(int(a) for a in added) if self.mapping_schedule else None)
        finally:
            self._render_views = None
            self._read_deform_stats()

    def _mapping_loss(self, ro, rd, d, gt_col, radius, geo, col_f, warp=None, *, stage="color", gate=None, w_geo=None,
                      w_color=None):
        """the loss of one mapping iteration (mapper.py:497-507) on the feature tables geo / col_f: depth and colour L1
        over the rays that carry a depth and met the cloud, plus the pixel-warping term of the window `warp` (its value is
        left in warp["value"]), per seen ray -> (loss, rendered depth, rendered colour, seen [N] as float).
        stage "geometry": rendered without the colour decoder, no colour term (mapper.py:483, :500).  gate: 1 / 0 weights
        [N] of the depth gate (map_sample.depth_gate), multiplied into `seen`.  w_geo, w_color: the weights of the two L1
        sums (None: 1 and 0.5)"""
        npc, ren = self.npc, self.renderer
        depth, _, colour, _, counts = ren.render_batch_ray(npc, self.decoders, rd, ro, self.device, stage, gt_depth=d,
                                                           npc_geo_feats=geo, npc_col_feats=col_f,
                                                           cloud_pos=npc.cloud_pos(), dynamic_r_query=radius)
        # (masked sums instead of `x[seen].sum()`: boolean indexing sizes its result on the host - one device round trip
        # in the forward and one in the backward pass of every iteration)
        seen = ((counts > 0) & (d > 0)).to(depth.dtype)
        if gate is not None:
            seen = seen * gate
        loss = (torch.abs(d - depth) * seen).sum()
        if w_geo is not None:
            loss = w_geo * loss
        if stage == "color":
            loss = loss + (0.5 if w_color is None else w_color) * (torch.abs(gt_col - colour) * seen[:, None]).sum()
        if warp is not None:
            # inside the numerator: its weight relative to the L1 sums is the reference's (mapper.py:497-507)
            w = pix_warping_loss(ro, rd, depth, warp["c2ws"], ren.fx, ren.fy, ren.cx, ren.cy, self.video.wd,
                                 self.video.ht, warp["frame_ids"], warp["ray_frame"], warp["table"], gt_col,
                                 nan_to_zero=True)
            loss = loss + self.w_pix_warp_loss * w
            warp["value"].copy_(w.detach())
        return loss / seen.sum().clamp_min(1), depth, colour, seen

    def _map_setup(self, k, rmaps=None, final=None, table=False):
        """what the iterations of keyframe k - or, with final = (window, views, per, pix_warping) and k None, of one pass
        of final_refine - hold fixed, as a namespace: geo, col_f (the clones of the two feature tables that are trained);
        view (of k), window, views, per, and `win`, the dict of the last three with frame_ids and ray_frame (None for k
        alone); warp (win plus the window's c2ws and the device table of its images, with pix_warping); rq (frame -> its
        query radius map, with colour-gradient radii) and const_r (the constant radius otherwise); with `table` the
        WindowTable of the window (also win["table"]); frustum and row_masks (keyframes with frustum selection)"""
        npc, ren = self.npc, self.renderer
        s = types.SimpleNamespace(geo=npc.geo_feats.detach().clone().requires_grad_(True),
                                  col_f=npc.col_feats.detach().clone().requires_grad_(True), view=None, win=None,
                                  warp=None, rq=None, table=None, frustum=None, row_masks=None)
        with torch.no_grad():
            if final is None:
                s.view = self._keyframe_view(k)
                windowed, pix_warping = bool(self.pix_warping or self.keyframe_selection_method), self.pix_warping
                window = self._map_window(k, s.view) if windowed else [k]
                s.per = self.map_rays // len(window)      # (frames skipped below still count, mapper.py:584)
                s.window, s.views = self._window_views(window, {k: s.view})
                if self.frustum_feature_selection:
                    # the rows the iterations may change: inside the frustum of this view, against the depth the iteration
                    # reads (get_mask_from_c2w, mapper.py:591-595); the count stays on the device until the keyframe is done
                    s.frustum = frustum_feature_mask(npc.cloud_pos(), s.view[1], s.view[0], ren.fx, ren.fy, ren.cx, ren.cy,
                                                     self.video.ht, self.video.wd, self.frustum_edge)
                    s.row_masks = {id(s.geo): s.frustum[0], id(s.col_f): s.frustum[0]}
            else:
                (s.window, s.views, s.per, pix_warping), windowed = final, True
            window, views = s.window, s.views
            # every window frame's own query radius map, built once per keyframe; the iteration gathers from them
            if self.color_grad is not None:
                s.rq = {f: (rmaps[1] if rmaps is not None and f == k else self._radius_maps(f, views[f], add=False)[1])
                        for f in window}
            s.const_r = None if s.rq is not None else self._const_radius()
            if pix_warping or table:
                c2ws = torch.stack([views[f][1] for f in window]).float().contiguous()
            if table:
                s.table = WindowTable([views[f][0] for f in window], [self.images[f] for f in window], c2ws,
                                      [s.rq[f] for f in window] if s.rq else None, channels_first=True)
            if windowed:
                frame_ids = torch.tensor(window, dtype=torch.int64).to(self.device)
                s.win = {"window": window, "views": views, "per": s.per, "frame_ids": frame_ids,
                         "ray_frame": frame_ids.repeat_interleave(s.per)}
                if table:
                    s.win["table"] = s.table
                if pix_warping:
                    s.warp = dict(s.win, c2ws=c2ws, table=FrameTable([self.images[f] for f in window], channels_first=True),
                                  value=torch.zeros((), device=self.device), first=None)
        return s

    def _all_depth(self, s):
        """one look at the window's depth maps (a host round trip per KEYFRAME): if every pixel carries a depth, no
        iteration needs the host - the renderer skips its per-batch zero-depth check and the iteration can be recorded"""
        return bool(torch.stack([(s.views[f][0] > 0).all() for f in s.window]).all())

    def _train(self, s, n_it, opt, rays, all_depth, probe_k, before=None, record=False, probe_extra=None):
        """`n_it` mapping iterations on the setup `s` (_map_setup) with the optimizer `opt`, then the trained tables go
        back into the cloud.  An iteration is before(it) (the caller's switches), rays(it) under no_grad -> ((ro, rd, d,
        gt_col, radius), keywords of _mapping_loss, further entries of the probe's dict), zero_grad, the loss, map_probe
        under the id `probe_k`, backward, step.  record: iteration 1 is recorded into a hipGraph and replayed for itself and
        every later one (rays must not read `it` then).  -> (seconds between the two synchronisations, (first, last) loss,
        NaN for no iteration); the pixel-warping term's pair is left in s.warp["first"] / ["value"]"""
        npc, ren, warp = self.npc, self.renderer, s.warp
        frustum = s.frustum[0] if s.frustum is not None else None
        self.last_optimizer = opt                            # (tests: step bookkeeping)

        def iteration(it):
            with torch.no_grad():
                (ro, rd, d, gt_col, radius), loss_kw, extra = rays(it)
            opt.zero_grad()
            # the colour decoder is not run in the geometry stage: no gradient is formed for its table there
            col_f = s.col_f.detach() if loss_kw.get("stage") == "geometry" else s.col_f
            loss, depth, colour, seen = self._mapping_loss(ro, rd, d, gt_col, radius, s.geo, col_f, warp, **loss_kw)
            if self.map_probe is not None and not torch.cuda.is_current_stream_capturing():
                self.map_probe(probe_k, dict(ro=ro, rd=rd, d=d, gt_col=gt_col, depth=depth.detach(),
                                             colour=colour.detach(), seen=seen, loss=loss.detach(), warp=warp, window=s.win,
                                             frustum=frustum, radius=radius, **extra, **(probe_extra or {})))
            loss.backward()
            opt.step(row_masks=s.row_masks)
            return loss.detach()

        first = last = graph = None
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ren.assume_depth = all_depth
        try:
            for it in range(n_it):
                if before is not None:
                    before(it)
                if record and it == 1:
                    # Iteration 0 ran eagerly (it sizes the scratch arenas, creates the Adam moments and sends the pointer
                    # table); iteration 1 is RECORDED - forward, masked loss, backward (incl. its second stream for the weight
                    # gradients), Adam with the step count in device memory - and replayed for itself and every later one
                    # (mapper.py:586-624 runs 150-1500 of them per keyframe on the same tensors).
                    try:
                        graph, last = self._capture_iteration(lambda: iteration(it))
                    except Exception as exc:      # a failed recording must not take the mapper down
                        import warnings
                        warnings.warn(f"hipGraph capture of the mapping iteration failed ({exc!r}); running eagerly")
                        record = False
                        opt.capturable_fallback()
                if graph is not None:
                    graph.replay()
                    continue
                last = iteration(it)
                if first is None:
                    first = last.clone()
                    if warp is not None:
                        warp["first"] = warp["value"].clone()
            if graph is not None:
                # host bookkeeping: the eager iteration and the recording itself each counted one step, the device did
                # 1 + (n_it - 1)
                opt.advance(n_it - 2)
                last = last.clone()
                self.map_graph_stats["captures"] += 1
                self.map_graph_stats["replays"] += n_it - 1
        finally:
            ren.assume_depth = False
        torch.cuda.synchronize()
        elapsed = time.perf_counter() - t0
        with torch.no_grad():
            npc.update_geo_feats(s.geo.detach())
            npc.update_col_feats(s.col_f.detach())
        return elapsed, (float(first), float(last)) if n_it else (float("nan"), float("nan"))

    def _optimize_keyframe(self, k, rmaps, frame_pts_add=None):
        """the mapping iterations of map_keyframe (after the insertion) and their bookkeeping: the one-stage loop
        (_optimize_default) or, with mapping_schedule, the reference's schedule for `frame_pts_add` inserted points
        (_optimize_scheduled)"""
        s = self._map_setup(k, rmaps, table=self.mapping_schedule)
        self.decoders.train()
        if self.mapping_schedule:
            n_it, elapsed, losses = self._optimize_scheduled(k, s, frame_pts_add)
        else:
            n_it, elapsed, losses = self._optimize_default(k, s)
        self.decoders.eval()
        self.timing["map_iter_ms"].append(1e3 * elapsed / max(n_it, 1))
        self.losses.append(losses)
        self.windows.append(s.window)
        if s.warp is not None and n_it:
            self.warp_losses.append((float(s.warp["first"]), float(s.warp["value"])))
        if s.frustum is not None:
            self.frustum_counts.append(int(s.frustum[1]))
        if self.mapping_vis is not None:
            self._visualize(k, s.view, s.rq[k] if s.rq else None, n_it)
        return losses

    def _optimize_default(self, k, s):
        """map_iters iterations in the colour stage on uniform pixel draws, every decoder trained at 0.005; recorded into a
        hipGraph when map_graph is set and every window pixel carries a depth -> (iterations, seconds, (first, last))"""
        dec, n_it, W, H = self.decoders, self.map_iters, self.video.wd, self.video.ht
        for p in dec.parameters():
            p.requires_grad_(True)
        # map_rays // len(window) pixels of every window frame per iteration (pixs_per_image, mapper.py:584), all
        # iterations drawn up front in one transfer: [iteration][ii | jj][frame-major rays], in the generator's order per
        # iteration and frame
        draws = torch.stack([torch.stack([torch.cat(c) for c in zip(*[
            (torch.randint(0, W, (s.per,), generator=self.gen), torch.randint(0, H, (s.per,), generator=self.gen))
            for _ in s.window])]) for _ in range(n_it)]).to(self.device) if n_it else None
        all_depth = self._all_depth(s)
        record = bool(getattr(self, "map_graph", True)) and all_depth and n_it >= 4 and \
            str(self.device).startswith("cuda") and getattr(self.renderer, "use_train_path", True)
        opt = FeatureAdam([{"params": list(dec.parameters()), "lr": 0.005}, {"params": [s.geo], "lr": 0.005},
                           {"params": [s.col_f], "lr": 0.005}], capturable=record)
        pix = draws[0].clone() if n_it else None             # the iteration reads its pixels from this buffer

        def before(it):
            if it:
                pix.copy_(draws[it])

        def rays(it):
            if s.win is None:
                ro, rd, d, gt_col, _, _, radius = self._keyframe_rays(k, view=s.view, pix=(pix[0], pix[1]),
                                                                      radius_map=s.rq[k] if s.rq else None)
            else:
                ro, rd, d, gt_col, radius = self._window_rays(s.win, pix, s.rq)
            return (ro, rd, d, gt_col, radius), {}, dict(pix=pix)

        return (n_it,) + self._train(s, n_it, opt, rays, all_depth, k, before=before, record=record)

    # ---- the reference's schedule (mapper.py:390-515, :598-638), mapping_schedule=True ------------------------------
    def _const_radius(self):
        return 0.5 * (self.npc.radius_add + self.npc.radius_query) if self.npc.use_dynamic_radius else None

    def _insertion_samples(self, k, view, rmaps):
        """cfg pixels_adding pixels of keyframe k drawn among the valid pixels of its insertion depth, one launch ->
        (rays_o, rays_d, depth, colour, radius, ii, jj)"""
        ren = self.renderer
        table = WindowTable([view[0]], [self.images[k]], view[1][None].float(), [rmaps[0]] if rmaps else None)
        draws = torch.randint(0, DRAW_RANGE, (self.schedule["pixels_adding"],), generator=self.gen).to(self.device)
        return sample_window_rays(table, ValidIndex(table), draws, draws.shape[0], ren.fx, ren.fy, ren.cx, ren.cy,
                                  const_radius=None if rmaps else self._const_radius())

    def schedule_of(self, init, frame_pts_add):
        """(iterations, of them in the geometry stage) of a keyframe (mapper.py:613-629): iters_first for the first mapped
        keyframe, else iters scaled by the inserted points over 300, clipped to [min_iter_ratio iters, 2 iters];
        iteration t is a geometry iteration iff t <= geo_iter_first (first keyframe) or int(n geo_iter_ratio)"""
        sc = self.schedule
        if init:
            n, bound = sc["iters_first"], sc["geo_iter_first"]
        else:
            n = min(max(int(sc["iters"] * frame_pts_add / 300), int(sc["min_iter_ratio"] * sc["iters"])), 2 * sc["iters"])
            bound = int(n * sc["geo_iter_ratio"])
        return n, min(n, bound + 1)

    def _optimize_scheduled(self, k, s, frame_pts_add):
        """the mapping iterations of map_keyframe on the reference's schedule.  One WindowTable and ValidIndex per
        keyframe over its window; every iteration is one sampling launch and one gate launch in front of the loss, its
        stage and learning rates by schedule_of.  Runs eagerly -> (iterations, seconds, (first, last))"""
        dec, ren, sc = self.decoders, self.renderer, self.schedule
        init = not self.schedules
        n_it, n_geo = self.schedule_of(init, frame_pts_add)
        rates = sc["rates"]["init" if init else "stage"]
        geo_params, col_params = list(dec.geo_decoder.parameters()), list(dec.color_decoder.parameters())
        flags = [(p, p.requires_grad) for p in dec.parameters()]
        index = ValidIndex(s.table, "all" if self.render_depth == "mono" else "depth")
        # every iteration's draws in one transfer
        draws = torch.randint(0, DRAW_RANGE, (n_it, len(s.window) * s.per), generator=self.gen).to(self.device)
        # one look per keyframe: when every drawn ray is sure to carry a depth the renderer needs no host check
        all_depth = bool((index.counts > 0).all()) if index.mode == "depth" else self._all_depth(s)
        trained = ([] if sc["fix_geo_decoder"] else geo_params) + ([] if sc["fix_color_decoder"] else col_params)
        opt = FeatureAdam([{"params": trained, "lr": 0.0}, {"params": [s.geo], "lr": 0.0}, {"params": [s.col_f], "lr": 0.0}])
        stage_of = lambda it: "geometry" if it < n_geo else "color"

        def before(it):
            if it in (0, n_geo):
                # the colour decoder is not run in the geometry stage: no gradient is formed for it there
                for p in col_params:
                    p.requires_grad_(stage_of(it) == "color" and not sc["fix_color_decoder"])
            for group, key in zip(opt.param_groups, ("decoders_lr", "geometry_lr", "color_lr")):
                group["lr"] = float(rates[stage_of(it)][key])

        def rays(it):
            stage = stage_of(it)
            ro, rd, d, gt_col, radius, ii, jj = sample_window_rays(s.table, index, draws[it], s.per, ren.fx, ren.fy, ren.cx,
                                                                   ren.cy, const_radius=s.const_r)
            gate, gate_stats = depth_gate(d)
            extra = dict(pix=torch.stack([ii, jj]), stage=stage, gate=gate, gate_stats=gate_stats, ii=ii, jj=jj,
                         lrs=dict(rates[stage])) if self.map_probe is not None else {}
            return (ro, rd, d, gt_col, radius), dict(stage=stage, gate=gate, w_geo=sc["w_geo_loss"],
                                                     w_color=sc["w_color_loss"]), extra

        try:
            for p in geo_params:
                p.requires_grad_(not sc["fix_geo_decoder"])
            elapsed, losses = self._train(s, n_it, opt, rays, all_depth, k, before=before)
        finally:
            for p, req in flags:
                p.requires_grad_(req)
        self.schedules.append((n_it, n_geo))
        return n_it, elapsed, losses

    # ---- the per-keyframe contact sheet (mapper.py:664-673) --------------------------------------------------------
    def _visualize(self, k, view, r_query, n_it):
        """Visualizer.vis for keyframe k after its last iteration: the view it trained on, its query radii and the
        trained feature tables (already back in the cloud); the tracker depth and the mono prior are the render-depth
        path's (aligned prior) or, without render_depth, the view depth itself and the raw prior.  Only reads"""
        import os

        from .visualizer import Visualizer
        npc = self.npc
        if self.visualizer is None:
            vis_dir = self.mapping_vis
            if vis_dir is True:
                if self.output is None:
                    raise ValueError("mapping_vis=True needs the run's output directory (run(output=...) or .output)")
                vis_dir = os.path.join(str(self.output), "mapping_vis")
            base = str(self.output) if self.output is not None else os.path.dirname(os.path.abspath(str(vis_dir)))
            self.visualizer = Visualizer(str(vis_dir), self.renderer, False, device=self.device,
                                         img_dir=os.path.join(base, "rendered_image"), **self.vis_options)
        with torch.no_grad():
            render_depth, c2w = view
            if self._vis_depths is not None:
                mono, droid = self._vis_depths
            else:
                mono, droid = self._mono_prior(k), render_depth
            if r_query is None and npc.use_dynamic_radius:
                r_query = torch.full_like(render_depth, self._const_radius())
            cfg = self._mono_cfg()
            cfg["mapping"] = dict(cfg["mapping"], mapping_window_size=self.mapping_window_size)
            self.visualizer.vis(int(self.video.timestamp[k]), n_it - 1, None, render_depth, droid, mono,
                                self.images[k].permute(1, 2, 0).contiguous(), c2w, npc, self.decoders,
                                npc.get_geo_feats(), npc.get_col_feats(), cfg, None, freq_override=(k == 0),
                                dynamic_r_query=r_query, cloud_pos=npc.cloud_pos(), cur_total_iters=n_it,
                                save_rendered_image=self.save_rendered_image)

    # ---- deformation and render depth (mapper.py:246-279, :557-573, :705-730) -------------------------------------
    def _deform(self):
        """update_points_pos(npc, video) of the reference: on HIP (deform_points) unless render_depth is "mono", where the
        torch driver re-places the points with the mono priors of the dirty keyframes (computed first where missing).
        Like the reference, nothing happens when no flag is set (one host read of the flags: no index rebuild then)"""
        npc, v, ren = self.npc, self.video, self.renderer
        if npc.video is None:
            npc.video = v
        if not bool(v.npc_dirty.any()):
            return
        if self._deform_counts is None:
            self._deform_counts = torch.zeros(2, dtype=torch.int64, device=self.device)
        if self.render_depth == "mono":
            dirty, = torch.where(v.npc_dirty)
            # the driver asks for every dirty keyframe's prior by dataset index, the ones without points included
            priors = {int(v.timestamp[f]): self._mono_prior(f) for f in dirty.tolist()}
            self._deform_counts[0] += dirty.numel()
            if npc._input_video_idx is not None:
                self._deform_counts[1] += torch.isin(npc._input_video_idx, dirty).sum()
            update_points_pos(npc, _CfgVideo(v, self._mono_cfg()), priors.__getitem__)
            self.deform_stats["calls"] += 1
            return
        if deform_points(npc, v, ren.fx, ren.fy, ren.cx, ren.cy, stats=self._deform_counts):
            self.deform_stats["calls"] += 1

    def _mono_cfg(self):
        """the runner's cfg with what the torch deformation driver reads from video.cfg: the render depth mode and the
        renderer's camera as update_cam expects it"""
        v, ren = self.video, self.renderer
        cam = dict(self.cfg.get("cam", {}))
        cam.update(H=v.ht, W=v.wd, H_out=v.ht, W_out=v.wd, H_edge=0, W_edge=0, fx=ren.fx, fy=ren.fy, cx=ren.cx, cy=ren.cy)
        return dict(self.cfg, cam=cam, mapping=dict(self.cfg.get("mapping", {}), render_depth="mono"))

    def _read_deform_stats(self):
        if self._deform_counts is not None:
            dirty, moved = self._deform_counts.tolist()
            self.deform_stats.update(dirty_keyframes=int(dirty), points_moved=int(moved))

    def _mono_prior(self, f):
        """the mono prior of keyframe f, computed when it is first needed and kept (keyframe_dict['mono_depth']).  Kept by
        timestamp: a keyframe of the tracker's window may still be culled and its slot reused by the next frame"""
        ts = float(self.video.timestamp[f])
        if ts not in self._mono_by_tstamp:
            self._mono_by_tstamp[ts] = self.mono_depth_fn(ts, self.images.get(f)).to(self.device, torch.float32)
        self.mono_priors[f] = self._mono_by_tstamp[ts]
        return self.mono_priors[f]

    def _frame_depths(self, f):
        """Mapper.get_c2w_and_depth (mapper.py:246-279): (c2w in the OpenGL convention, aligned mono prior m_wq, tracker
        depth with 0 outside valid_depth_mask), or None for fewer than 100 valid tracker depths (the reference means to
        skip the frame there)"""
        v = self.video
        droid, valid, c2w = v.get_depth_and_pose(f, self.device)
        if int(valid.sum()) < 100:
            return None
        droid[~valid] = 0
        c2w[:3, 1:3] *= -1
        m = self._mono_prior(f)
        scale, shift = v.get_depth_scale_and_shift(f, m, droid, (m < m.mean() * 3) & valid)
        return c2w, m * scale + shift, droid

    def _render_depth_of(self, c2w, m_wq, droid):
        if self.render_depth == "mono":
            return m_wq
        ren = self.renderer
        return proxy_render_depth(self.npc, self.video, c2w, droid, m_wq, self.mapping_window_size, ren.fx, ren.fy,
                                  ren.cx, ren.cy, use_mono_to_complete=self.use_mono_to_complete)

    def _render_view(self, f):
        """(render depth, c2w) of window frame f, None if it is skipped"""
        rv = self._render_views
        if f not in rv:
            got = self._frame_depths(f)
            rv[f] = None if got is None else (self._render_depth_of(*got), got[0])
        return rv[f]

    def _prepare_render(self, k):
        """keyframe k with render_depth: its anchor view (insertion depth, c2w) - the tracker depth with holes from m_wq
        in proxy mode, m_wq in mono mode - after add_points(k); its render view goes to _render_views.  None: skipped"""
        got = self._frame_depths(k)
        if got is None:
            return None
        c2w, m_wq, droid = got
        if self.mapping_vis is not None:
            self._vis_depths = (m_wq, droid)
        anchor = torch.where(droid == 0, m_wq, droid) if self.render_depth == "proxy" else m_wq.clone()
        if self.npc.video is None:
            self.npc.video = self.video
        self.npc.add_points(k)                          # full_pcl holds k before the projection (mapper.py:306)
        self._render_views = {k: (self._render_depth_of(c2w, m_wq, droid), c2w)}
        return anchor, c2w

    def _select_keyframes(self, k, view):
        """the keyframes of [0, k-1) that join k-1 and k in the window of keyframe k: up to mapping_window_size - 2 of
        them (mapper.py:541-549: the candidates are keyframe_dict[:-1]), by overlap with k's view or at random"""
        num, n_cand = max(self.mapping_window_size - 2, 0), max(k - 1, 0)
        if num == 0 or n_cand == 0:
            return []
        if self.keyframe_selection_method == "global":
            return random_select(n_cand, num, generator=self.gen)
        ren = self.renderer
        c2ws = torch.stack([self._keyframe_view(f)[1] for f in range(n_cand)])
        return keyframe_selection_overlap(self.images.get(k), view[0], view[1], c2ws, num, ren.fx, ren.fy, ren.cx, ren.cy,
                                          generator=self.gen)

    def _map_window(self, k, view):
        """the mapping window of keyframe k (keyframe ids, k last).  Without a keyframe_selection_method: k and the
        mapping_window_size - 1 most recent earlier keyframes; with one: the selected keyframes, k-1, k"""
        if self.keyframe_selection_method:
            return self._select_keyframes(k, view) + ([k - 1] if k > 0 else []) + [k]
        return list(range(max(0, k - self.mapping_window_size + 1), k + 1))

    def _window_views(self, window, known=()):
        """(the frames of `window` that are not skipped, frame -> (depth, c2w)): `known` views as given, the others their
        render view with render_depth (None: skipped), else their keyframe view"""
        fetch = self._render_view if self.render_depth is not None else self._keyframe_view
        with torch.no_grad():
            views = {f: (known[f] if f in known else fetch(f)) for f in window}
        window = [f for f in window if views[f] is not None]
        return window, {f: views[f] for f in window}

    def _window_rays(self, win, pix, rq=None):
        """the rays of one iteration over the window: frame f's slice of `pix` through its own view, depth and image
        (and its own query radius map of `rq`, frame -> [H,W], when given)"""
        per, parts = win["per"], []
        for i, f in enumerate(win["window"]):
            sl = slice(i * per, (i + 1) * per)
            parts.append(self._keyframe_rays(f, view=win["views"][f], pix=(pix[0, sl], pix[1, sl]),
                                             radius_map=rq[f] if rq else None))
        ro, rd, d, col = (torch.cat([p[j] for p in parts]) for j in range(4))
        radius = torch.cat([p[6] for p in parts]) if parts[0][6] is not None else None
        return ro, rd, d, col, radius

    def _radius_maps(self, f, view, add=True, query_depth=None):
        """(dynamic_r_add / 3 * depth or None, dynamic_r_query / 3 * depth) [H,W] of keyframe f from its image and the
        depth of `view` (mapper.py:538, :719, :767-784), the query radius from `query_depth` when given: one launch"""
        m = color_grad_maps(self.images[f], depth_add=view[0] if add else None,
                            depth_query=view[0] if query_depth is None else query_depth,
                            outputs=("r_add", "r_query") if add else ("r_query",), **self.color_grad)
        return m.get("r_add"), m["r_query"]

    def _anchor_grad_points(self, k, rmaps, view=None):
        """the second anchoring pass (mapper.py:312-322): pixels_based_on_color_grad pixels drawn from the 5x as many of
        highest colour gradient where the keyframe has depth, inserted with is_pts_grad=True (view: the anchor view)"""
        ren, H, W = self.renderer, self.video.ht, self.video.wd
        depth, c2w = view if view is not None else self._keyframe_view(k)
        color = self.images[k].permute(1, 2, 0)
        ro, rd, d, col, ii, jj = get_samples_with_pixel_grad(0, H, 0, W, self.pixels_based_on_color_grad, H, W, ren.fx,
                                                             ren.fy, ren.cx, ren.cy, c2w, depth, color, self.device,
                                                             depth > 0, generator=self.gen)
        if rmaps is not None:
            radius = rmaps[0][jj, ii]
        elif self.npc.use_dynamic_radius:
            radius = torch.full_like(d, self._const_radius())
        else:
            radius = None
        return self.npc.add_neural_points(ro.reshape(-1, 3).contiguous(), rd.reshape(-1, 3).contiguous(), d,
                                          col.contiguous(), k, ii, jj, is_pts_grad=True, dynamic_radius=radius)

    def _capture_iteration(self, iteration):
        """record one mapping iteration into a hipGraph (one memory pool for all keyframes of this runner, kept open by a
        one-node keeper graph as in FactorGraph._capture); returns (graph, the iteration's loss tensor inside the pool)"""
        dev = torch.device(self.device)
        cap = getattr(self, "_map_capture_stream", None)
        if cap is None:
            cap = self._map_capture_stream = torch.cuda.Stream(dev)
            self._map_pool = torch.cuda.graph_pool_handle()
            self._map_keeper = torch.cuda.CUDAGraph()
            with torch.cuda.stream(cap):
                self._map_keeper.capture_begin(pool=self._map_pool)
                self._map_keeper_buf = torch.zeros(1, device=dev)
                self._map_keeper.capture_end()
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        cap.wait_stream(torch.cuda.current_stream(dev))
        # no automatic garbage collection while the capture is open: the iteration runs its backward on the autograd thread, and a
        # collection that starts there finalises whatever cyclic garbage earlier work left behind (graphs, events, contexts) -
        # device calls from another thread inside a global-mode capture, which end the process.  Nothing is collected here
        # either (FactorGraph._capture says why); the collector is only held off for the few milliseconds of the recording.
        import gc
        gc_was_on = gc.isenabled()
        gc.disable()
        try:
            with torch.cuda.stream(cap):
                graph.capture_begin(pool=self._map_pool)
                try:
                    loss = iteration()
                finally:
                    graph.capture_end()
        finally:
            if gc_was_on:
                gc.enable()
        torch.cuda.current_stream(dev).wait_stream(cap)
        return graph, loss

    def map_pending(self):
        """map every keyframe the frontend has finished with (its redundancy test culls a frame inside the same call that
        appended it, tracker.py:56-69: what is below the window's end afterwards is final)"""
        done = self.frontend.t1 if self.frontend.is_initialized else 0
        while self.mapped < done:
            self.map_keyframe(self.mapped)
            self.mapped += 1

    # ---- mapper.py:816-855 ------------------------------------------------------------------------------------------
    def final_refine(self, outer_iters=5, iters=None, pix_warping=None, save_final_pcl=False, output=None):
        """Mapper.final_refine: after the last global BA the point features are trained once more over all keyframes
        (mapping_keyframe with color_refine=True: the cloud is deformed, no point is inserted, the decoders are frozen,
        no frustum selection).  `outer_iters` passes; each selects its window (keyframe_select.final_refine_window:
        the 'global' method over every mapped keyframe), recomputes its views and radius maps, and runs 2 * map_iters
        iterations (`iters` when given) with a fresh FeatureAdam on the two feature tables.  An iteration's rays come
        from one launch (window_rays.py) whatever the window's size, its loss is map_keyframe's (_mapping_loss), in the
        colour stage at the runner's learning rate throughout.  pix_warping: None is the runner's setting while the
        window fits the pixel-warping kernel (warp_loss.MAX_FRAMES frames), off beyond; True beyond it is an error.
        Runs eagerly.  save_final_pcl with `output`: final_point_cloud.npy, npc_cloud.npy and final_point_cloud.ply
        there (mapper.py:838-849).  The passes' (first, last) losses go to refine_losses, their windows to
        refine_windows; the bookkeeping of map_keyframe is not touched.
        -> dict(window_sizes, per, losses, pix_warping, ms_per_iter)"""
        npc, dec, ren, v = self.npc, self.decoders, self.renderer, self.video
        n_it = 2 * self.map_iters if iters is None else int(iters)
        self.refine_losses, self.refine_windows = [], []
        sizes, pers, warped, elapsed, steps = [], [], [], 0.0, 0
        frozen = [(p, p.requires_grad) for p in dec.parameters()]
        # the first window before anything runs on the GPU: an empty map or an impossible pix_warping ends the call here
        first_window = final_refine_window(self.mapped, self.skipped, int(v.counter.value), self.map_rays, self.gen,
                                           pix_warping=pix_warping)
        if npc.pts_num() == 0:
            raise ValueError("final refinement needs a point cloud")
        self._render_views = None
        try:
            if self.bind_npc_with_pose:
                with torch.no_grad():
                    self._deform()
            for p, _ in frozen:                    # fix_geo_decoder and fix_color_decoder: no decoder gradient is formed
                p.requires_grad_(False)
            dec.train()
            for o in range(int(outer_iters)):
                window, per = first_window if o == 0 else final_refine_window(
                    self.mapped, self.skipped, int(v.counter.value), self.map_rays, self.gen, pix_warping=pix_warping)
                if self.render_depth is not None:
                    self._render_views = {}
                window, views = self._window_views(window)                       # (per stays, mapper.py:564, :584)
                if not window:
                    raise ValueError("final refinement: every window frame was skipped")
                warp_on = (self.pix_warping if pix_warping is None else bool(pix_warping)) \
                    and len(window) <= MAX_WARP_FRAMES
                s = self._map_setup(None, final=(window, views, per, warp_on), table=True)
                # every iteration's draw in one transfer: [iteration][ii | jj][frame-major rays]
                n_rays = per * len(window)
                draws = torch.stack([torch.randint(0, v.wd, (n_it, n_rays), generator=self.gen),
                                     torch.randint(0, v.ht, (n_it, n_rays), generator=self.gen)], 1).to(self.device)
                opt = FeatureAdam([{"params": [s.geo], "lr": 0.005}, {"params": [s.col_f], "lr": 0.005}])

                def rays(it):
                    pix = draws[it]
                    return window_rays(s.table, pix[0], pix[1], per, ren.fx, ren.fy, ren.cx, ren.cy,
                                       const_radius=s.const_r), {}, dict(pix=pix)

                dt, losses = self._train(s, n_it, opt, rays, self._all_depth(s), window[-1], probe_extra=dict(refine=o))
                elapsed += dt
                steps += n_it
                self.refine_losses.append(losses)
                self.refine_windows.append(list(window))
                sizes.append(len(window))
                pers.append(per)
                warped.append(s.warp is not None)
        finally:
            for p, req in frozen:
                p.requires_grad_(req)
            dec.eval()
            self._render_views = None
            self._read_deform_stats()
        if save_final_pcl and output is not None:
            self.save_final_pcl(output)
        return {"window_sizes": sizes, "per": pers[0] if pers else first_window[1], "losses": list(self.refine_losses),
                "pix_warping": bool(warped) and all(warped), "ms_per_iter": 1e3 * elapsed / max(steps, 1)}

    def save_final_pcl(self, output):
        """final_point_cloud.npy ([n,6]: input_pos | input_rgb), npc_cloud.npy ([n,3]: cloud_pos) and
        final_point_cloud.ply (the input points, colours input_rgb / 255: add_neural_points stores 0..255 as the
        reference does) under `output` (mapper.py:838-849)"""
        import os

        import numpy as np

        from .generate_mesh import write_ply
        os.makedirs(str(output), exist_ok=True)
        pos = self.npc.input_pos().detach().cpu().numpy()
        rgb = self.npc.input_rgb().detach().cpu().numpy()
        np.save(os.path.join(str(output), "final_point_cloud"), np.hstack((pos, rgb)))
        np.save(os.path.join(str(output), "npc_cloud"), self.npc.cloud_pos().detach().cpu().numpy())
        write_ply(os.path.join(str(output), "final_point_cloud.ply"), pos, np.zeros((0, 3), np.int32),
                  rgb.astype(np.float64) / 255.0)

    # ---- the stream -------------------------------------------------------------------------------------------------
    def run(self, frames, intrinsics, final_ba_steps=7, final_refine=False, output=None):
        """frames: iterable of (tstamp, image [1,3,H,W] in [0,1]).  final_refine: the final refinement of the map
        (final_refine() with its defaults) after the final BA.  output: the run's directory, where mapping_vis=True puts
        mapping_vis/ and rendered_image/.  Returns a summary dict."""
        if output is not None:
            self.output = output
        for tstamp, image in frames:
            self.track(tstamp, image, intrinsics)
            self.map_pending()
        with torch.no_grad():
            n, n_edges = self.backend.dense_ba(final_ba_steps)             # the final global BA of slam.py / tracker.py
        self.map_pending()
        if self.bind_npc_with_pose and self.npc.pts_num() > 0:
            with torch.no_grad():                                           # the cloud follows the final trajectory
                self._deform()
            self._read_deform_stats()
        if final_refine:
            self.final_refine()
        torch.cuda.synchronize()
        return {"keyframes": int(self.video.counter.value), "final_ba_edges": int(n_edges), "mapped": self.mapped,
                "points": int(self.npc.pts_num()), "losses": list(self.losses), "timing": self.timing}

    def run_stream(self, stream, **kwargs):
        """run() over a dataset stream (datasets.BaseDataset: items (index, color [1,3,H,W], depth, pose) and
        get_intrinsic()): the frame index is the timestamp, as in the reference's tracker loop (src/tracker.py:48-51)"""
        return self.run(((item[0], item[1]) for item in stream), stream.get_intrinsic(), **kwargs)

    # ---- eval_render.py:18-124 ------------------------------------------------------------------------------------------
    def evaluate(self, output=None, gt_depth_fn=None, **kwargs):
        """re-render every mapped keyframe and score it against its image (eval_render.eval_kf_imgs: PSNR, MS-SSIM, their
        masked forms, depth L1 with gt_depth_fn; the masked maps and the metrics file under `output`).  Not part of run()"""
        from .eval_render import eval_kf_imgs
        return eval_kf_imgs(self, output=output, gt_depth_fn=gt_depth_fn, **kwargs)

    def render_view(self, c2w, **kwargs):
        """the map seen from the pose c2w [4,4], which need not be a keyframe's (Renderer.render_view: no depth prior, every
        ray marched on the device); kwargs: stage, far, intervals, dynamic_r_query.  -> depth, uncertainty, color [H,W,3],
        valid_ray_mask, valid_ray_counts as render_img returns them.  Not part of run()"""
        npc = self.npc
        c2w = torch.as_tensor(c2w, dtype=torch.float32).to(self.device)
        return self.renderer.render_view(npc, self.decoders, c2w, self.device, npc_geo_feats=npc.get_geo_feats(),
                                         npc_col_feats=npc.get_col_feats(), cloud_pos=npc.cloud_pos(), **kwargs)

    # ---- generate_mesh.py:55-123 ----------------------------------------------------------------------------------------
    def mesh(self, output=None, mesh_name_suffix="kf", scene="scene", cull=None, clean=None, **kwargs):
        """the triangle mesh of the run (generate_mesh.fuse_frames): every mapped keyframe is re-rendered (eval_kf_imgs)
        and its masked depth and colour are fused from device memory into a TSDF volume with the keyframe's own pose;
        kwargs: scale, transform, voxel_length, sdf_trunc, max_blocks.  cull: a dict of cull_mesh.cull_mesh keywords - the
        mesh is cut to what the mapped keyframes saw from their placed poses, for method "occlusion" against the masked
        re-rendered depths; clean: a dict of cull_mesh.clean_mesh keywords (both off by default).  -> (vertices f32 [V,3],
        colors f32 [V,3], faces int32 [F,3]) on the device; with `output` also mesh/{scene}_{suffix}.ply and
        mesh/vertices_pos_{suffix}.npy, as generate_mesh_kf writes from the files of evaluate(output) and save_video.  Not
        part of run()"""
        from .eval_render import eval_kf_imgs
        from .generate_mesh import cull_and_clean, fuse_frames, save_mesh
        res = eval_kf_imgs(self, keep_renders=True)
        frames = []
        for f in res["frames"]:
            r = f["render"]
            depth = torch.where(r["mask"], r["depth"].float(), torch.zeros_like(r["depth"], dtype=torch.float32))
            color = torch.where(r["mask"][..., None], r["color"].float(), torch.zeros_like(r["color"], dtype=torch.float32))
            frames.append((depth, color, self.video.get_pose(f["video_idx"], "cpu")))
        ren = self.renderer
        intrinsics = (ren.fx, ren.fy, ren.cx, ren.cy)
        vertices, colors, faces, _ = fuse_frames(frames, intrinsics, self.device, **kwargs)
        vertices, colors, faces = cull_and_clean(vertices, colors, faces, frames, intrinsics, kwargs.get("scale", 1.0),
                                                 kwargs.get("transform"), cull, clean)
        if output is not None:
            save_mesh(output, vertices, colors, faces, mesh_name_suffix, scene)
        return vertices, colors, faces

    # ---- eval_recon.py:229-248 ------------------------------------------------------------------------------------------
    def recon(self, gt_vertices, gt_faces, output=None, mesh_kwargs=None, **kwargs):
        """the reconstruction scores of the run (eval_recon.eval_recon): the mesh of mesh(output=output, **mesh_kwargs)
        against the ground-truth mesh (device tensors); kwargs: eval_2d, eval_3d, align, kwargs_3d, kwargs_2d, cull (views in
        the ground truth's frame that both meshes are cut to before scoring).  -> the
        dict of accuracy, completion, completion_ratio, precision, recall, f-score and depth l1; with `output` also
        metrics_recon.txt next to the mesh folder.  Not part of run()"""
        from .eval_recon import eval_recon
        vertices, _, faces = self.mesh(output=output, **(mesh_kwargs or {}))
        return eval_recon((vertices, faces), (gt_vertices, gt_faces), output=output, **kwargs)


# ---- the synthetic 640x480 stream of the config-3 test and of bench.py's `sequence` entry --------------------------------
def synthetic_cfg(device, buffer, H=480, W=640):
    return {
        "cam": {"H_out": H, "W_out": W}, "device": str(device), "setting": "t", "scene": "seq", "data": {"output": "/tmp"},
        "mono_prior": {"predict_online": False}, "mapping": {"every_frame": 5},
        "tracking": {
            "buffer": buffer, "beta": 0.75, "warmup": 8, "max_age": 50, "mono_thres": 0.1,
            "multiview_filter": {"thresh": 0.25, "visible_num": 2}, "store_images": False,
            "motion_filter": {"thresh": -1.0},     # every frame becomes a keyframe (a zeroed flow head predicts no motion)
            "frontend": {"enable_loop": False, "keyframe_thresh": 0.0, "thresh": 16.0, "window": 25, "radius": 1,
                         "nms": 1, "max_factors": 75},
            "backend": {"BA_type": "DSPO", "thresh": 25.0, "radius": 1, "nms": 5, "normalize": False,
                        "loop_window": 25, "loop_thresh": 25.0, "loop_radius": 1, "loop_nms": 12}},
        "pointcloud": {"nn_weighting": "distance", "use_dynamic_radius": True, "min_nn_num": 2, "nn_num": 8,
                       "radius_query": 0.08, "radius_add": 0.04, "radius_min": 0.02},
        "rendering": {"N_surface": 10, "near_end_surface": 0.95, "far_end_surface": 1.05, "sample_near_pcl": True,
                      "sigmoid_coef": 0.1, "near_end": 0.3},
        "model": {"encode_rel_pos_in_col": True, "encode_viewd": True, "c_dim": 32}}


def synthetic_images(K, H=480, W=640, seed=5):
    """smooth random textures in [0, 1] (low-resolution noise, bilinearly upsampled): [K,3,H,W]"""
    g = torch.Generator().manual_seed(seed)
    low = torch.rand(K, 3, H // 16, W // 16, generator=g)
    return torch.nn.functional.interpolate(low, size=(H, W), mode="bilinear", align_corners=False).clamp(0, 1)


def synthetic_runner(device, K, zero_flow_head=True, map_iters=20, map_rays=1000, use_graphs=True, H=480, W=640,
                     buffer=None):
    """SequenceRunner over the keyframe arc of synth.keyframe_graph (the bench's graph G8 continued to K frames): seed-43
    default-init DroidNet and decoders, the mono prior = the true depth under an affine distortion, the tracker's initial
    guess of a new keyframe = its generating pose and disparity.  zero_flow_head: the last layer of the flow head is
    zeroed, which makes the generating trajectory a fixed point of the tracking loop (there are no trained weights
    here).  -> (runner, dict(poses, disps, cfg, video, npc, intrinsics))"""
    import numpy as np

    from . import synth
    from .decoder import POINT
    from .depth_video import DepthVideo
    from .droid_net import DroidNet
    from .neural_point import NeuralPointCloud
    from .renderer import Renderer
    h, w = H // 8, W // 8
    cfg = synthetic_cfg(device, max(K + 2, buffer or 0), H, W)    # buffer: tracking.buffer of the shipped configs is 400-600
    g = synth.keyframe_graph(K=K, h=h, w=w, radius=3)
    torch.manual_seed(43)
    net = DroidNet().to(device).eval()
    if zero_flow_head:
        with torch.no_grad():
            net.update.delta[2].weight.zero_()
            net.update.delta[2].bias.zero_()
    video = DepthVideo(cfg)
    npc = NeuralPointCloud(cfg)
    torch.manual_seed(43)
    dec = POINT(cfg, use_view_direction=True).eval().to(device)
    sx, sy = W / 640.0, H / 480.0
    cam = types.SimpleNamespace(H=H, W=W, fx=320.0 * sx, fy=320.0 * sy, cx=319.5 * sx, cy=239.5 * sy)
    ren = Renderer(cfg, cam)
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(device)
    disps = t(g["disps"])                                        # [K,h,w] generating disparities
    full = torch.nn.functional.interpolate(1.0 / disps[:, None], size=(H, W), mode="bilinear", align_corners=False)[:, 0]

    def mono(tstamp, image):
        return (full[int(tstamp)] * 1.25 + 0.1).to(device)

    run = SequenceRunner(net, video, cfg, npc, dec, ren, mono, use_graphs=use_graphs, ba_every=4, ba_steps=2,
                         map_iters=map_iters, map_rays=map_rays, add_stride=8)
    poses = t(g["poses"])

    def init_state(k, tstamp=None):
        video.poses[k] = poses[k]
        video.disps[k] = disps[k]
        video.disps_up[k] = 1.0 / full[k]
    run.init_state = init_state
    intr = torch.tensor([cam.fx, cam.fy, cam.cx, cam.cy])
    return run, dict(poses=poses, disps=disps, cfg=cfg, video=video, npc=npc, intrinsics=intr)


def synthetic_long_runner(device, n_frames=220, leg=60, repeat_every=9, map_iters=20, map_rays=1000, buffer=512, ba_every=20,
                          H=480, W=640):
    """Config 3 beyond the 13-frame miniature: a stream of `n_frames` 640x480 frames whose camera walks the arc of
    synth.keyframe_graph forth and back (a triangle wave of period 2 * leg: frame 2 * leg stands where frame 0 stood, so the
    loop-closure search finds pairs more than 20 keyframes apart), with every `repeat_every`-th frame a repeat of its
    predecessor (zero induced flow: the frontend's redundancy test culls it, rm_keyframe shifts the buffers), loop closure
    enabled, a global BA every `ba_every` keyframes, `map_iters` mapping iterations per kept keyframe, a 512-frame buffer.
    Flow head zeroed: the generating trajectory is a fixed point.  -> (runner, dict(...), frames iterator factory)"""
    import numpy as np

    from . import synth
    from .decoder import POINT
    from .depth_video import DepthVideo
    from .droid_net import DroidNet
    from .neural_point import NeuralPointCloud
    from .renderer import Renderer
    h, w = H // 8, W // 8
    cfg = synthetic_cfg(device, buffer, H, W)
    cfg["tracking"]["frontend"].update({"enable_loop": True, "keyframe_thresh": 0.5})
    g = synth.keyframe_graph(K=leg + 1, h=h, w=w, radius=3)
    # arc position of stream frame f: triangle wave; every repeat_every-th frame repeats its predecessor
    pos, u = [], 0
    for f in range(n_frames):
        if f and f % repeat_every == 0:
            pos.append(pos[-1])
            continue
        k = u % (2 * leg)
        pos.append(k if k <= leg else 2 * leg - k)
        u += 1
    torch.manual_seed(43)
    net = DroidNet().to(device).eval()
    with torch.no_grad():
        net.update.delta[2].weight.zero_()
        net.update.delta[2].bias.zero_()
    video = DepthVideo(cfg)
    npc = NeuralPointCloud(cfg)
    torch.manual_seed(43)
    dec = POINT(cfg, use_view_direction=True).eval().to(device)
    cam = types.SimpleNamespace(H=H, W=W, fx=320.0 * W / 640.0, fy=320.0 * H / 480.0, cx=319.5 * W / 640.0, cy=239.5 * H / 480.0)
    ren = Renderer(cfg, cam)
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(device)
    disps, poses = t(g["disps"]), t(g["poses"])
    full = torch.nn.functional.interpolate(1.0 / disps[:, None], size=(H, W), mode="bilinear", align_corners=False)[:, 0]
    run = SequenceRunner(net, video, cfg, npc, dec, ren, lambda ts, im: (full[pos[int(ts)]] * 1.25 + 0.1), use_graphs=True,
                         ba_every=ba_every, ba_steps=2, map_iters=map_iters, map_rays=map_rays, add_stride=8)

    def init_state(k, tstamp):
        a = pos[int(tstamp)]
        video.poses[k] = poses[a]
        video.disps[k] = disps[a]
        video.disps_up[k] = 1.0 / full[a]
    run.init_state = init_state
    bank = synthetic_images(leg + 1, H, W)                                  # one texture per arc position

    def frames():
        for f in range(n_frames):
            yield f, bank[pos[f]:pos[f] + 1]
    intr = torch.tensor([cam.fx, cam.fy, cam.cx, cam.cy])
    return run, dict(poses=poses, disps=disps, cfg=cfg, video=video, npc=npc, intrinsics=intr, pos=pos), frames
