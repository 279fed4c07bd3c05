"""The mesh-culling kernels (csrc/cull.hip) through glorie_slam_amd/cull_mesh.py against the float64 restatement of
tests/cull_ref.py: exact visibility counts on firm vertices, selection and compaction bit for bit, component labels and face
counts bit for bit, and the argument checks.

Scene: the 4 x 3 x 2.2 m box room of cull_ref.room_mesh (six walls of 13 x 13 cells with their own vertices and a slab of
7 x 5 cells inside: 1224 vertices, 2098 faces), five general cameras of 37 x 53 pixels, depth from an exact ray cast with a
rectangle of zeros planted in the first map, eps = 0.03, z_far = 3.2.  The restatement has no unfirm vertex on it, 438
vertices seen by at least one view and 786 by none, and 32 to 111 occluded vertices per view (tests/test_cull_ref.py)."""
import numpy as np
import pytest
import torch

import cull_ref as R

pytestmark = pytest.mark.gpu

MAX_UNFIRM = 1e-3       # the share of a scene's vertices that may be left out as unfirm


def _dev(a, gpu, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a)).to(gpu)
    return t if dtype is None else t.to(dtype)


@pytest.fixture(scope="module")
def scenes():
    return {name: make() for name, make in R.SCENES.items()}


def _check_counts(what, got, vertices, w2cs, s, **kw):
    """got (device int32) equals the restatement on every firm vertex; at most MAX_UNFIRM of them may be unfirm"""
    ref, unfirm = R.visibility(vertices, w2cs, s["K"], s["H"], s["W"], **kw)
    got = got.cpu().numpy()
    share = unfirm.mean()
    wrong = int((got[~unfirm] != ref[~unfirm]).sum())
    print(f"{what}: {len(ref)} vertices, unfirm share {share:.5f}, seen by a view {int((ref > 0).sum())}, "
          f"differing firm counts {wrong}")
    assert got.dtype == np.int32 and got.shape == ref.shape
    assert share <= MAX_UNFIRM
    assert wrong == 0
    return ref


def _kw(s, **over):
    kw = dict(eps=s["eps"], z_near=s["z_near"], z_far=s["z_far"])
    kw.update(over)
    return kw


@pytest.mark.parametrize("use_depths", [False, True])
@pytest.mark.parametrize("edge", [0, 3])
@pytest.mark.parametrize("missing", [False, True])
def test_visibility_room(gpu, scenes, use_depths, edge, missing):
    from glorie_slam_amd import cull_mesh as C
    s = scenes["room5"]
    depths = [_dev(d, gpu) for d in s["depths"]] if use_depths else None
    got = C.vertex_visibility(_dev(s["vertices"], gpu), s["c2ws"], s["K"], s["H"], s["W"], depths=depths,
                              **_kw(s, edge=edge, depth_missing_sees=missing))
    ref = _check_counts(f"room depths={use_depths} edge={edge} missing={missing}", got, s["vertices"], s["w2cs"], s,
                        depths=s["depths"] if use_depths else None, **_kw(s, edge=edge, depth_missing_sees=missing))
    assert 0 < (ref > 0).sum() < len(ref)


def test_visibility_depths_as_one_tensor_and_device_poses(gpu, scenes):
    from glorie_slam_amd import cull_mesh as C
    s = scenes["room5"]
    v = _dev(s["vertices"], gpu)
    a = C.vertex_visibility(v, s["c2ws"], s["K"], s["H"], s["W"], depths=[_dev(d, gpu) for d in s["depths"]], **_kw(s))
    b = C.vertex_visibility(v, _dev(s["c2ws"], gpu), s["K"], s["H"], s["W"], depths=_dev(np.stack(s["depths"]), gpu), **_kw(s))
    assert torch.equal(a, b)


def test_visibility_accumulates_over_chunks(gpu, scenes):
    from glorie_slam_amd import cull_mesh as C
    s = scenes["room5"]
    v = _dev(s["vertices"], gpu)
    depths = [_dev(d, gpu) for d in s["depths"]]
    whole = C.vertex_visibility(v, s["c2ws"], s["K"], s["H"], s["W"], depths=depths, **_kw(s))
    acc = torch.zeros(len(s["vertices"]), dtype=torch.int32, device=gpu)
    for lo, hi in ((0, 1), (1, 5)):
        out = C.vertex_visibility(v, s["c2ws"][lo:hi], s["K"], s["H"], s["W"], depths=depths[lo:hi], out=acc, **_kw(s))
        assert out is acc
    assert torch.equal(acc, whole)
    # one view, and none
    one = C.vertex_visibility(v, s["c2ws"][:1], s["K"], s["H"], s["W"], depths=depths[:1], **_kw(s))
    _check_counts("room M=1", one, s["vertices"], s["w2cs"][:1], s, depths=s["depths"][:1], **_kw(s))
    none = C.vertex_visibility(v, np.zeros((0, 4, 4)), s["K"], s["H"], s["W"], **_kw(s))
    assert int(none.abs().sum()) == 0


def test_visibility_seventy_views(gpu, scenes):
    """more views than nothing in particular but fewer than the LDS stage holds at once, then more than it holds"""
    from glorie_slam_amd import cull_mesh as C
    s = scenes["room70"]
    v = _dev(s["vertices"], gpu)
    depths = [_dev(d, gpu) for d in s["depths"]]
    got = C.vertex_visibility(v, s["c2ws"], s["K"], s["H"], s["W"], depths=depths, **_kw(s, edge=3))
    ref = _check_counts("room M=70", got, s["vertices"], s["w2cs"], s, depths=s["depths"], **_kw(s, edge=3))
    assert ref.max() > 16
    # 140 views in one launch: the staging loop takes a second, ragged chunk (128 + 12)
    twice = C.vertex_visibility(v, np.concatenate([s["c2ws"], s["c2ws"]]), s["K"], s["H"], s["W"], depths=depths + depths,
                                **_kw(s, edge=3))
    assert torch.equal(twice, 2 * got)


@pytest.mark.parametrize("n", [1, 63, 65, 70001])
def test_visibility_ragged_sizes(gpu, scenes, n):
    from glorie_slam_amd import cull_mesh as C
    s = scenes["room5"]
    rng = np.random.default_rng(n)
    pts = (rng.uniform(-1.05, 1.05, (n, 3)) * R.ROOM).astype(np.float32)
    got = C.vertex_visibility(_dev(pts, gpu), s["c2ws"], s["K"], s["H"], s["W"], depths=[_dev(d, gpu) for d in s["depths"]],
                              **_kw(s, edge=1))
    _check_counts(f"{n} random points", got, pts, s["w2cs"], s, depths=s["depths"], **_kw(s, edge=1))


@pytest.mark.parametrize("n_views", [5, 20])
def test_self_occlusion_through_cull_mesh(gpu, scenes, n_views):
    """the counts against the rasteriser's own maps (read back: the rasteriser is not re-tested here); 20 views take two
    chunks of the ring"""
    from glorie_slam_amd import cull_mesh as C, eval_recon as E
    s = scenes["room5"]
    c2ws = s["c2ws"] if n_views == 5 else R.jittered_cameras(n_views)
    w2cs = R.w2cs_of(c2ws)
    v, f = _dev(s["vertices"], gpu), _dev(s["faces"], gpu)
    colors = _dev(np.abs(s["vertices"][:, ::-1]) * 0.2, gpu)
    out_v, out_f, out_c, count = C.cull_mesh(v, f, c2ws, s["K"], s["H"], s["W"], colors=colors, method="occlusion",
                                             rule="any", min_views=2, **_kw(s, edge=2))
    maps = [E.render_depth(v, f, None, s["K"], s["H"], s["W"], z_near=s["z_near"], z_far=s["z_far"],
                           w2c=_dev(w, gpu)).cpu().numpy() for w in w2cs]
    assert all((m > 0).any() for m in maps)
    ref = _check_counts(f"self-occlusion M={n_views}", count, s["vertices"], w2cs, s, depths=maps, **_kw(s, edge=2))
    keep = R.select_faces(s["faces"], ref, 2, "any")
    rv, rf, rc = R.compact(s["vertices"], s["faces"], keep, colors.cpu().numpy())
    assert 0 < len(rf) < len(s["faces"])
    assert np.array_equal(out_v.cpu().numpy(), rv) and np.array_equal(out_f.cpu().numpy(), rf)
    assert np.array_equal(out_c.cpu().numpy(), rc)


# ---- selection and compaction ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def counted(scenes):
    s = scenes["room5"]
    count, unfirm = R.visibility(s["vertices"], s["w2cs"], s["K"], s["H"], s["W"], depths=s["depths"], **_kw(s))
    assert not unfirm.any()
    return count


@pytest.mark.parametrize("rule", ["all", "any"])
@pytest.mark.parametrize("min_views", [1, 2])
def test_select_and_compact(gpu, scenes, counted, rule, min_views):
    from glorie_slam_amd import cull_mesh as C
    s = scenes["room5"]
    V = len(s["vertices"])
    faces = np.concatenate([s["faces"][:900], [[0, 1, V]], s["faces"][900:], [[-1, 2, 3]]]).astype(np.int32)
    colors = (np.abs(s["vertices"]) * 0.25).astype(np.float32)
    keep = C.select_faces(_dev(faces, gpu), _dev(counted, gpu), min_views, rule)
    ref_keep = R.select_faces(faces, counted, min_views, rule)
    assert keep.dtype == torch.uint8 and np.array_equal(keep.cpu().numpy(), ref_keep)
    assert ref_keep[900] == 0 and ref_keep[-1] == 0 and 0 < ref_keep.sum() < len(faces)
    out_v, out_f, out_c = C.compact_mesh(_dev(s["vertices"], gpu), _dev(faces, gpu), keep, _dev(colors, gpu))
    rv, rf, rc = R.compact(s["vertices"], faces, ref_keep, colors)
    assert out_f.dtype == torch.int32 and out_v.dtype == torch.float32
    assert np.array_equal(out_v.cpu().numpy(), rv) and np.array_equal(out_f.cpu().numpy(), rf)
    assert np.array_equal(out_c.cpu().numpy(), rc)
    # without colours, and a bool mask
    out_v2, out_f2 = C.compact_mesh(_dev(s["vertices"], gpu), _dev(faces, gpu), keep.bool())
    assert torch.equal(out_v2, out_v) and torch.equal(out_f2, out_f)


def test_compact_nothing_and_everything(gpu, scenes):
    from glorie_slam_amd import cull_mesh as C
    s = scenes["room5"]
    V = len(s["vertices"])
    v, f = _dev(s["vertices"], gpu), _dev(s["faces"], gpu)
    out_v, out_f, out_c = C.compact_mesh(v, f, torch.zeros(len(s["faces"]), dtype=torch.uint8, device=gpu), v)
    assert tuple(out_v.shape) == (0, 3) and tuple(out_f.shape) == (0, 3) and tuple(out_c.shape) == (0, 3)
    out_v, out_f = C.compact_mesh(v, f, torch.ones(len(s["faces"]), dtype=torch.uint8, device=gpu))
    assert torch.equal(out_v, v) and torch.equal(out_f, f)
    # a kept face with an index outside [0, V) is dropped, and only it
    bad = np.concatenate([s["faces"], [[0, 1, V], [-1, 0, 1]]]).astype(np.int32)
    out_v, out_f = C.compact_mesh(v, _dev(bad, gpu), torch.full((len(bad),), 7, dtype=torch.uint8, device=gpu))
    assert torch.equal(out_v, v) and torch.equal(out_f, f)
    # nobody is seen: cull_mesh returns an empty mesh without an error
    away = s["c2ws"].copy()
    away[:, :3, 3] += 100.0
    out_v, out_f, count = C.cull_mesh(v, f, away, s["K"], s["H"], s["W"], **_kw(s))
    assert tuple(out_v.shape) == (0, 3) and tuple(out_f.shape) == (0, 3) and int(count.sum()) == 0


# ---- components --------------------------------------------------------------------------------------------------------------
def _component_scenes():
    v, f = R.room_mesh()
    fv, ff, _ = R.floaters(len(v))
    v2 = np.concatenate([v, fv])
    isolated = np.zeros((6, 3), np.float32)
    degenerate = np.array([[5, 5, 9], [len(v2) + 6, 0, 1], [-1, 2, 3], [7, 7, 7]], np.int32)
    sv, sf = R.strip_mesh()
    return {"room": (v, f), "floaters": (v2, np.concatenate([f, ff])),
            "degenerate": (np.concatenate([v2, isolated]), np.concatenate([f, ff, degenerate])),
            "strip": (sv, sf), "one face": (np.eye(3, dtype=np.float32), np.array([[2, 0, 1]], np.int32))}


@pytest.mark.parametrize("name", ["room", "floaters", "degenerate", "strip", "one face"])
def test_components(gpu, name):
    from glorie_slam_amd import cull_mesh as C
    v, f = _component_scenes()[name]
    label, faces_of = C.mesh_components(_dev(v, gpu), _dev(f, gpu))
    again, faces_again = C.mesh_components(_dev(v, gpu), _dev(f, gpu))
    ref_label, ref_faces_of = R.components(f, len(v))
    print(f"{name}: {len(v)} vertices, {len(f)} faces, {len(np.unique(ref_label))} components")
    assert label.dtype == torch.int32 and faces_of.dtype == torch.int32
    assert np.array_equal(label.cpu().numpy(), ref_label) and np.array_equal(faces_of.cpu().numpy(), ref_faces_of)
    assert torch.equal(label, again) and torch.equal(faces_of, faces_again)
    if name == "room":
        assert faces_of[faces_of > 0].tolist() == [338] * 6 + [70]
    if name == "strip":
        assert int(label.max()) == 0 and int(faces_of[0]) == 3000


def test_clean_mesh(gpu):
    from glorie_slam_amd import cull_mesh as C
    v, f = R.room_mesh()
    fv, ff, n_added = R.floaters(len(v))
    v2, f2 = np.concatenate([v, fv]), np.concatenate([f, ff])
    colors = (np.abs(v2) * 0.25).astype(np.float32)
    out_v, out_f, out_c = C.clean_mesh(_dev(v2, gpu), _dev(f2, gpu), _dev(colors, gpu), min_faces=3)
    assert n_added == 10
    assert np.array_equal(out_v.cpu().numpy(), v) and np.array_equal(out_f.cpu().numpy(), f), "exactly the floaters go"
    assert np.array_equal(out_c.cpu().numpy(), colors[:len(v)])
    # min_faces = 2 keeps the quads, 1 everything
    label, faces_of = R.components(f2, len(v2))
    for min_faces in (1, 2, 71, 339):
        keep = R.component_mask(f2, label, faces_of, min_faces)
        rv, rf, _ = R.compact(v2, f2, keep)
        out_v, out_f = C.clean_mesh(_dev(v2, gpu), _dev(f2, gpu), min_faces=min_faces)
        assert np.array_equal(out_v.cpu().numpy(), rv) and np.array_equal(out_f.cpu().numpy(), rf), min_faces
    # the six walls tie on 338 faces: the one with the lowest label stays
    out_v, out_f = C.clean_mesh(_dev(v2, gpu), _dev(f2, gpu), keep_largest=True)
    assert np.array_equal(out_v.cpu().numpy(), v[:196]) and np.array_equal(out_f.cpu().numpy(), f[:338])
    # with the first wall's faces moved to the end and one of them taken away the second wall is the largest
    f3 = np.concatenate([f[338:], f[1:338]])
    out_v, out_f = C.clean_mesh(_dev(v, gpu), _dev(f3, gpu), keep_largest=True)
    assert np.array_equal(out_v.cpu().numpy(), v[196:392]) and np.array_equal(out_f.cpu().numpy(), f[338:676] - 196)


# ---- arguments ---------------------------------------------------------------------------------------------------------------
def test_argument_checks(gpu, scenes):
    from glorie_slam_amd import _lib, cull_mesh as C
    s = scenes["room5"]
    v, f = _dev(s["vertices"], gpu), _dev(s["faces"], gpu)
    args = (s["c2ws"], s["K"], s["H"], s["W"])
    with pytest.raises(_lib.GlorieError):
        C.cull_mesh(v.cpu(), f, *args)
    with pytest.raises(_lib.GlorieError):
        C.vertex_visibility(v.cpu(), *args)
    with pytest.raises(_lib.GlorieError):
        C.mesh_components(v, f.cpu())
    with pytest.raises(ValueError):
        C.cull_mesh(v[:, :2], f, *args)
    with pytest.raises(ValueError):
        C.clean_mesh(v, f.to(torch.int16))
    with pytest.raises(ValueError):
        C.mesh_components(v, f[:0])
    with pytest.raises(ValueError):
        C.cull_mesh(v[:0], f, *args)
    with pytest.raises(ValueError):
        C.cull_mesh(v, f, *args, method="zbuffer")
    with pytest.raises(ValueError):
        C.cull_mesh(v, f, *args, rule="most")
    with pytest.raises(ValueError):
        C.vertex_visibility(v, s["c2ws"][0], s["K"], s["H"], s["W"])
    with pytest.raises(ValueError):
        C.vertex_visibility(v, *args, depths=[_dev(d, gpu) for d in s["depths"][:2]])
    with pytest.raises(ValueError):
        C.compact_mesh(v, f, torch.ones(3, dtype=torch.uint8, device=gpu))
    # bad sizes are refused by the entry points themselves, before any launch
    with pytest.raises(_lib.GlorieError, match="GLORIE_EINVAL"):
        C.vertex_visibility(v, *args, edge=-1)
    with pytest.raises(_lib.GlorieError, match="GLORIE_EINVAL"):
        C.vertex_visibility(v, *args, z_near=2.0, z_far=1.0)
    lib = _lib.load()
    assert lib.glorie_mesh_components(_lib.ptr(f), -1, 5, 0, 0, None, None, None, None, None) == -1
    assert lib.glorie_mesh_compact_count(_lib.ptr(f), 0, 5, None, None, None, None) == -1
    assert lib.glorie_mesh_select_faces(_lib.ptr(f), 4, 0, None, 1, 0, None, None) == -1
    assert lib.glorie_mesh_compact_workspace(0, 5) == 0
