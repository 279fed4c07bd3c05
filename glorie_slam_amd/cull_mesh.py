"""Mesh culling to the region the cameras saw and removal of small connected components, on HIP kernels (csrc/cull.hip).

  vertex_visibility   per vertex, the number of views that see it: inside the frustum and, with depth maps, not behind the
                      surface the view measured
  cull_mesh           drops the faces whose vertices too few views saw; method "frustum", or "occlusion" against given
                      depth maps or against the mesh's own rasterised depth
  mesh_components     connected components over shared vertex indices
  clean_mesh          drops the components below min_faces, or all but the largest
  compact_mesh        the mesh under any face mask, order kept, indices remapped
  cull_mesh_file      the same on a PLY in the layout generate_mesh.write_ply writes

The reference scores against meshes somebody else culled (cull_replica_mesh/<scene>.ply in its Replica configs) and has no
such step of its own; the rules are stated in include/glorie_hip.h.  Device tensors throughout, no CPU fallback; numpy
float64 on the host only for the 4x4 inverses.  Cameras are OpenCV pinholes whose pixel (u, v) samples image coordinates
(u, v), as in eval_recon.py and tsdf.py.
"""
import ctypes

import numpy as np
import torch

from . import _lib as L
from .eval_recon import _Rasteriser, _intrinsics, _mesh, _points

RING = 16           # depth maps alive at once in the self-occlusion loop, and views per visibility launch there
_RULES = {"all": 0, "any": 1}


def _w2cs(c2ws, device):
    """c2ws [M,4,4] host or device -> w2cs f32 [M,4,4] on the device, inverted on the host in float64"""
    c2ws = np.asarray(c2ws.detach().cpu() if torch.is_tensor(c2ws) else c2ws, np.float64)
    if c2ws.ndim != 3 or c2ws.shape[1:] != (4, 4):
        raise ValueError(f"c2ws must be [M,4,4], got {c2ws.shape}")
    inv = np.linalg.inv(c2ws) if len(c2ws) else c2ws
    return torch.from_numpy(np.ascontiguousarray(inv.astype(np.float32))).to(device)


def _depth_list(depths, M, H, W, device):
    """a list of M device maps f32 [H,W] from a list or an [M,H,W] tensor"""
    if torch.is_tensor(depths):
        L.need_cuda(depths)
        if depths.dim() != 3:
            raise ValueError(f"depths must be [M,H,W] or a list of [H,W] maps, got {tuple(depths.shape)}")
        depths = L.f32(depths)
        depths = [depths[m] for m in range(depths.shape[0])]
    depths = list(depths)
    if len(depths) != M:
        raise ValueError(f"{len(depths)} depth maps for {M} views")
    out = []
    for d in depths:
        if not torch.is_tensor(d):
            raise ValueError(f"a depth map must be a device tensor, got {type(d).__name__}")
        L.need_cuda(d)
        if tuple(d.shape) != (H, W):
            raise ValueError(f"a depth map must be [{H},{W}], got {tuple(d.shape)}")
        out.append(L.f32(d.to(device)))
    return out


def _depth_table(maps, device):
    """the device array of the maps' addresses, as glorie_mesh_visibility takes it; None without maps"""
    if maps is None:
        return None
    return torch.tensor([m.data_ptr() for m in maps], dtype=torch.int64).to(device)


def _visibility_launch(vertices, w2cs, K, H, W, z_near, z_far, edge, table, eps, depth_missing_sees, accumulate, count):
    dev = vertices.device
    with torch.cuda.device(dev):
        L.check(L.load().glorie_mesh_visibility(L.ptr(vertices), vertices.shape[0], L.ptr(w2cs), w2cs.shape[0], *K, H, W,
                                                float(z_near), float(z_far), int(edge), L.ptr(table), float(eps),
                                                int(bool(depth_missing_sees)), int(bool(accumulate)), L.ptr(count),
                                                L.stream_ptr(dev)), "glorie_mesh_visibility")


def vertex_visibility(vertices, c2ws, K, H, W, depths=None, eps=0.03, edge=0, z_near=0.01, z_far=30.0,
                      depth_missing_sees=False, out=None):
    """count int32 [V]: the views of c2ws [M,4,4] (OpenCV, host or device) that see every vertex.  A view sees a vertex
    with z_near < z <= z_far whose nearest pixel lies at least `edge` pixels inside the H x W image and, with depths (a list
    of M device maps [H,W] or an [M,H,W] tensor), whose z is at most the map's depth there + eps; where the map has no
    depth (<= 0) it sees the vertex only if depth_missing_sees.  One launch for all views; with `out` (int32 [V]) the counts
    are added to it"""
    vertices = _points(vertices, "vertices")
    dev = vertices.device
    if vertices.shape[0] == 0:
        raise ValueError("there are no vertices")
    H, W, K = int(H), int(W), _intrinsics(K)
    w2cs = _w2cs(c2ws, dev)
    maps = _depth_list(depths, w2cs.shape[0], H, W, dev) if depths is not None else None
    if out is not None:
        L.need_cuda(out)
        if out.dtype != torch.int32 or tuple(out.shape) != (vertices.shape[0],) or not out.is_contiguous():
            raise ValueError("out must be a contiguous int32 [V] tensor")
    count = out if out is not None else torch.empty(vertices.shape[0], dtype=torch.int32, device=dev)
    _visibility_launch(vertices, w2cs, K, H, W, z_near, z_far, edge, _depth_table(maps, dev), eps, depth_missing_sees,
                       out is not None, count)
    return count


def self_occlusion_visibility(vertices, faces, c2ws, K, H, W, eps=0.03, edge=0, z_near=0.01, z_far=30.0,
                              depth_missing_sees=False, test_vertices=None):
    """the counts of vertex_visibility against the depth of the mesh (vertices, faces) itself: every view is rasterised with
    glorie_mesh_depth into a ring of at most RING maps, and every chunk of RING views is one accumulating visibility
    launch, so memory stays bounded at any number of views.  test_vertices: lists of vertices to test against those maps
    (default: the mesh's own) -> one count per list"""
    r = _Rasteriser(vertices, faces, K, H, W, z_near, z_far)
    dev = r.vertices.device
    tested = [r.vertices] if test_vertices is None else [_points(t, "vertices") for t in test_vertices]
    w2cs = _w2cs(c2ws, dev)
    counts = [torch.zeros(t.shape[0], dtype=torch.int32, device=dev) for t in tested]
    ring = [torch.empty(r.H, r.W, dtype=torch.float32, device=dev) for _ in range(min(RING, max(w2cs.shape[0], 1)))]
    for m0 in range(0, w2cs.shape[0], RING):
        chunk = w2cs[m0:m0 + RING]
        for j in range(chunk.shape[0]):
            r.render(chunk[j], out=ring[j])
        table = _depth_table(ring[:chunk.shape[0]], dev)
        for t, c in zip(tested, counts):
            # stream order: the next chunk's rasteriser calls overwrite the ring only after this launch has read it
            _visibility_launch(t, chunk, r.K, r.H, r.W, z_near, z_far, edge, table, eps, depth_missing_sees, True, c)
    return counts[0] if test_vertices is None else counts


def select_faces(faces, count, min_views=1, rule="all"):
    """keep_face uint8 [F]: all (rule "all") or any ("any") of the face's vertices have count >= min_views; a face with an
    index outside [0, V) is dropped"""
    if rule not in _RULES:
        raise ValueError(f"rule must be 'all' or 'any', got {rule!r}")
    L.need_cuda(faces, count)
    faces = faces.to(torch.int32).contiguous()
    keep = torch.empty(faces.shape[0], dtype=torch.uint8, device=faces.device)
    with torch.cuda.device(faces.device):
        L.check(L.load().glorie_mesh_select_faces(L.ptr(faces), faces.shape[0], count.shape[0], L.ptr(count), int(min_views),
                                                  _RULES[rule], L.ptr(keep), L.stream_ptr(faces.device)),
                "glorie_mesh_select_faces")
    return keep


def _colors(colors, vertices):
    if colors is None:
        return None
    colors = _points(colors, "colors")
    if colors.shape != vertices.shape or colors.device != vertices.device:
        raise ValueError("colors must be [V,3] on the vertices' device")
    return colors


def compact_mesh(vertices, faces, keep_face, colors=None):
    """the mesh under the face mask keep_face (uint8 or bool [F]): kept faces and the vertices they refer to, both in their
    order, indices remapped, colours carried -> (vertices, faces) or (vertices, faces, colors).  One read-back (V', F')"""
    vertices, faces = _mesh(vertices, faces)
    colors = _colors(colors, vertices)
    L.need_cuda(keep_face)
    if keep_face.dtype not in (torch.uint8, torch.bool) or tuple(keep_face.shape) != (faces.shape[0],):
        raise ValueError("keep_face must be uint8 or bool [F]")
    keep = keep_face.to(torch.uint8).contiguous()
    lib, dev = L.load(), vertices.device
    V, F = vertices.shape[0], faces.shape[0]
    ws = L.workspace(lib.glorie_mesh_compact_workspace(V, F), dev)
    n = (ctypes.c_int * 2)()
    with torch.cuda.device(dev):
        L.check(lib.glorie_mesh_compact_count(L.ptr(faces), F, V, L.ptr(keep), L.ptr(ws), n, L.stream_ptr(dev)),
                "glorie_mesh_compact_count")
        out_v = torch.empty(n[0], 3, dtype=torch.float32, device=dev)
        out_f = torch.empty(n[1], 3, dtype=torch.int32, device=dev)
        out_c = torch.empty(n[0], 3, dtype=torch.float32, device=dev) if colors is not None else None
        L.check(lib.glorie_mesh_compact_emit(L.ptr(vertices), L.ptr(colors), L.ptr(faces), F, V, L.ptr(keep), L.ptr(ws),
                                             n[0], n[1], L.ptr(out_v), L.ptr(out_c), L.ptr(out_f), L.stream_ptr(dev)),
                "glorie_mesh_compact_emit")
    return (out_v, out_f) if colors is None else (out_v, out_f, out_c)


def cull_mesh(vertices, faces, c2ws, K, H, W, colors=None, method="frustum", depths=None, rule="all", min_views=1,
              eps=0.03, edge=0, z_near=0.01, z_far=30.0, depth_missing_sees=False):
    """The mesh cut to what the views c2ws [M,4,4] saw -> (vertices, faces[, colors], count), count int32 over the
    vertices that came in.  method "frustum": a vertex is seen by the views whose frustum holds it; "occlusion": also not
    behind `depths` (as vertex_visibility takes them), or with depths=None not behind the mesh's own depth
    (self_occlusion_visibility).  A face stays when all (rule "all") or any ("any") of its vertices were seen by at least
    min_views views"""
    if method not in ("frustum", "occlusion"):
        raise ValueError(f"method must be 'frustum' or 'occlusion', got {method!r}")
    if rule not in _RULES:
        raise ValueError(f"rule must be 'all' or 'any', got {rule!r}")
    vertices, faces = _mesh(vertices, faces)
    kw = dict(eps=eps, edge=edge, z_near=z_near, z_far=z_far, depth_missing_sees=depth_missing_sees)
    if method == "occlusion" and depths is None:
        count = self_occlusion_visibility(vertices, faces, c2ws, K, H, W, **kw)
    else:
        count = vertex_visibility(vertices, c2ws, K, H, W, depths=depths if method == "occlusion" else None, **kw)
    keep = select_faces(faces, count, min_views, rule)
    return compact_mesh(vertices, faces, keep, colors) + (count,)


def _components(vertices, faces, min_faces=0, keep_largest=False, want_mask=False):
    vertices, faces = _mesh(vertices, faces)
    lib, dev = L.load(), vertices.device
    V, F = vertices.shape[0], faces.shape[0]
    label = torch.empty(V, dtype=torch.int32, device=dev)
    faces_of = torch.empty(V, dtype=torch.int32, device=dev)
    keep = torch.empty(F, dtype=torch.uint8, device=dev) if want_mask else None
    ws = L.workspace(lib.glorie_mesh_components_workspace(), dev)
    with torch.cuda.device(dev):
        L.check(lib.glorie_mesh_components(L.ptr(faces), F, V, int(min_faces), int(bool(keep_largest)), L.ptr(ws),
                                           L.ptr(label), L.ptr(faces_of), L.ptr(keep), L.stream_ptr(dev)),
                "glorie_mesh_components")
    return vertices, faces, label, faces_of, keep


def mesh_components(vertices, faces):
    """-> (label int32 [V] = the smallest vertex index of the vertex's component, faces_of int32 [V] = the number of
    faces of the component at its label vertex, 0 elsewhere).  No host synchronisation"""
    return _components(vertices, faces)[2:4]


def clean_mesh(vertices, faces, colors=None, min_faces=0, keep_largest=False):
    """the mesh without the connected components of fewer than min_faces faces; keep_largest: only the component with the
    most faces (ties: the one with the lowest vertex index) -> (vertices, faces) or (vertices, faces, colors)"""
    vertices, faces, _, _, keep = _components(vertices, faces, min_faces, keep_largest, want_mask=True)
    return compact_mesh(vertices, faces, keep, colors)


def cull_mesh_file(src_ply, dst_ply, c2ws, K, H, W, device="cuda", clean=None, **kwargs):
    """read_ply(src_ply) -> cull_mesh(**kwargs) -> clean_mesh(**clean) when `clean` is a dict -> write_ply(dst_ply);
    -> (vertices, faces, colors) on the device"""
    from .generate_mesh import read_ply, write_ply
    v, f, c = read_ply(src_ply)
    v, f = torch.from_numpy(v).to(device), torch.from_numpy(f).to(device)
    c = torch.from_numpy(c.astype(np.float32) / np.float32(255.0)).to(device)
    v, f, c, _ = cull_mesh(v, f, c2ws, K, H, W, colors=c, **kwargs)
    if clean is not None and f.shape[0] > 0:
        v, f, c = clean_mesh(v, f, c, **clean)
    write_ply(dst_ply, v, f, c)
    return v, f, c
