"""Pins tests/cull_ref.py, the float64 restatement the GPU tests of the mesh-culling kernels compare against, and its
scenes (no GPU): the components against scipy, the visibility rule against an independent formulation, every branch of
the rule populated in every scene, and every deliberate mistake (`mutate`) caught by at least one scene."""
import numpy as np
import pytest

import cull_ref as R

SCENES = {name: make() for name, make in R.SCENES.items()}


def _vis_kw(s, **over):
    kw = dict(depths=s["depths"], eps=s["eps"], z_near=s["z_near"], z_far=s["z_far"])
    kw.update(over)
    return kw


def test_room_mesh_is_the_documented_one():
    v, f = R.room_mesh()
    assert v.shape == (1224, 3) and v.dtype == np.float32 and f.shape == (2098, 3) and f.dtype == np.int32
    label, faces_of = R.components(f, len(v))
    assert np.unique(label).tolist() == [0, 196, 392, 588, 784, 980, 1176]
    assert faces_of[faces_of > 0].tolist() == [338] * 6 + [70]


def _scipy_labels(faces, V):
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import connected_components
    f = np.asarray(faces, np.int64)
    f = f[R.valid_faces(f, V)]
    rows = np.concatenate([f[:, 0], f[:, 1]])
    cols = np.concatenate([f[:, 1], f[:, 2]])
    g = coo_matrix((np.ones(len(rows)), (rows, cols)), shape=(V, V))
    _, comp = connected_components(g, directed=False)
    smallest = np.full(comp.max() + 1, V, np.int64)
    np.minimum.at(smallest, comp, np.arange(V))
    return smallest[comp].astype(np.int32)


def _component_cases():
    v, f = R.room_mesh()
    fv, ff, _ = R.floaters(len(v))
    degenerate = np.array([[5, 5, 9], [len(v) + len(fv), 0, 1], [-1, 2, 3], [7, 7, 7]], np.int32)
    sv, sf = R.strip_mesh()
    return {"room": (f, len(v)), "floaters": (np.concatenate([f, ff]), len(v) + len(fv)),
            "degenerate": (np.concatenate([f, ff, degenerate]), len(v) + len(fv) + 6), "strip": (sf, len(sv)),
            "one face": (np.array([[2, 0, 1]], np.int32), 3)}


@pytest.mark.parametrize("name", ["room", "floaters", "degenerate", "strip", "one face"])
def test_components_equal_scipy(name):
    faces, V = _component_cases()[name]
    label, faces_of = R.components(faces, V)
    assert np.array_equal(label, _scipy_labels(faces, V))
    ok = R.valid_faces(faces, V)
    assert faces_of.sum() == ok.sum() and (faces_of[label != np.arange(V)] == 0).all()
    assert np.array_equal(faces_of[np.unique(label)], np.bincount(label[np.asarray(faces)[ok][:, 0]], minlength=V)[np.unique(label)])


def test_strip_has_its_smallest_index_in_the_middle():
    v, f = R.strip_mesh()
    assert len(f) == 3000 and len(v) == 3002
    where = int(np.nonzero(f[:, 0] == 0)[0][0])
    assert 1400 < where < 1600
    label, faces_of = R.components(f, len(v))
    assert (label == 0).all() and faces_of[0] == 3000
    assert not np.array_equal(np.sort(f[:, 0]), f[:, 0])


def _independent_counts(s, edge, depth_missing_sees, use_depths):
    """homogeneous 3x4 projection, rounding without rint or floor(x + 0.5)"""
    fx, fy, cx, cy = s["K"]
    Kmat = np.array([[fx, 0, cx], [0, fy, cy], [0, 0, 1]], np.float64)
    Kmat = Kmat.astype(np.float32).astype(np.float64)
    Xh = np.concatenate([s["vertices"].astype(np.float64), np.ones((len(s["vertices"]), 1))], 1)
    count = np.zeros(len(Xh), np.int64)
    for m, w2c in enumerate(s["w2cs"]):
        x = Xh @ (Kmat @ w2c.astype(np.float64)[:3]).T
        zc = x[:, 2]
        with np.errstate(divide="ignore", invalid="ignore"):
            ui, vi = np.ceil(x[:, 0] / zc - 0.5), np.ceil(x[:, 1] / zc - 0.5)
        ok = (zc > np.float32(s["z_near"])) & (zc <= np.float32(s["z_far"]))
        ok &= (ui >= edge) & (ui <= s["W"] - edge - 1) & (vi >= edge) & (vi <= s["H"] - edge - 1)
        if use_depths:
            idx = np.nonzero(ok)[0]
            d = s["depths"][m][vi[idx].astype(int), ui[idx].astype(int)].astype(np.float64)
            ok[idx] = np.where(d > 0, zc[idx] - d <= np.float64(np.float32(s["eps"])), depth_missing_sees)
        count += ok
    return count


@pytest.mark.parametrize("name", sorted(SCENES))
@pytest.mark.parametrize("edge,missing,use_depths", [(0, False, True), (3, True, True), (0, False, False)])
def test_visibility_equals_independent_formulation(name, edge, missing, use_depths):
    s = SCENES[name]
    count, unfirm = R.visibility(s["vertices"], s["w2cs"], s["K"], s["H"], s["W"],
                                 **_vis_kw(s, edge=edge, depth_missing_sees=missing, depths=s["depths"] if use_depths else None))
    assert unfirm.sum() == 0, "the scenes are built to have no vertex on a decision boundary"
    assert np.array_equal(count, _independent_counts(s, edge, missing, use_depths))


def test_room_counts_are_pinned():
    s = SCENES["room5"]
    cls, sees, unfirm = R.visibility_classes(s["vertices"], s["w2cs"], s["K"], s["H"], s["W"], **_vis_kw(s))
    count = sees.sum(0)
    assert not unfirm.any()
    assert ((count >= 1).sum(), (count == 0).sum()) == (438, 786)
    assert (cls == R.OCCLUDED).sum(1).tolist() == [77, 66, 94, 32, 111]
    assert (cls == R.HOLE).sum(1).tolist() == [12, 0, 0, 0, 0]


@pytest.mark.parametrize("name", sorted(SCENES))
@pytest.mark.parametrize("edge", [0, 3])
def test_every_branch_is_populated(name, edge):
    s = SCENES[name]
    cls, sees, _ = R.visibility_classes(s["vertices"], s["w2cs"], s["K"], s["H"], s["W"], **_vis_kw(s, edge=edge))
    for k, what in enumerate(R.CLASS_NAMES):
        assert (cls == k).sum() >= 5, f"{name}: no vertex is {what}"
    count = sees.sum(0)
    min_views = 2
    assert (count == min_views - 1).sum() >= 5, "no vertex is seen by exactly min_views - 1 views"
    for mv in (1, min_views):
        per_face = (count[s["faces"]] >= mv).sum(1)
        assert (np.bincount(per_face, minlength=4) >= 5).all(), "faces with 0 / 1 / 2 / 3 seen vertices are needed"


def _pipeline(s, vis_mutate=None, sel_mutate=None, compact_mutate=None, rule="all", min_views=1, edge=3, missing=False):
    count, _ = R.visibility(s["vertices"], s["w2cs"], s["K"], s["H"], s["W"],
                            **_vis_kw(s, edge=edge, depth_missing_sees=missing, mutate=vis_mutate))
    keep = R.select_faces(s["faces"], count, min_views, rule, mutate=sel_mutate)
    colors = s["vertices"][:, ::-1] * 0.1
    return (count, keep) + R.compact(s["vertices"], s["faces"], keep, colors, mutate=compact_mutate)


def _differs(a, b):
    return any(x.shape != y.shape or not np.array_equal(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize("mutation", ["edge", "floor", "eps", "hole", "rule", "keepvertex", "maxlabel"])
def test_mutations_are_caught(mutation):
    caught = []
    for name, s in SCENES.items():
        if mutation == "maxlabel":
            label, _ = R.components(s["faces"], len(s["vertices"]))
            wrong, _ = R.components(s["faces"], len(s["vertices"]), mutate="maxlabel")
            caught.append(not np.array_equal(label, wrong))
            continue
        kw = {"vis_mutate": mutation} if mutation in ("edge", "floor", "eps", "hole") else \
            {"sel_mutate": mutation} if mutation == "rule" else {"compact_mutate": mutation}
        caught.append(_differs(_pipeline(s), _pipeline(s, **kw)))
    assert any(caught), f"no scene catches the mutation {mutation!r}"
    if mutation in ("edge", "floor", "eps", "hole"):
        # these change the counts themselves, in every scene
        for s in SCENES.values():
            assert not np.array_equal(_pipeline(s)[0], _pipeline(s, vis_mutate=mutation)[0])


def test_compaction_properties():
    s = SCENES["room5"]
    count, keep, v, f, c = _pipeline(s)
    assert 0 < keep.sum() < len(keep) and len(f) == keep.sum()
    assert f.min() == 0 and f.max() == len(v) - 1 and len(np.unique(f)) == len(v)
    # kept faces in their order, referring to the same positions and colours
    src = s["faces"][keep != 0]
    assert np.array_equal(v[f], s["vertices"][src]) and np.array_equal(c[f], (s["vertices"][:, ::-1] * 0.1)[src])
    # nothing kept and everything kept
    v0, f0, _ = R.compact(s["vertices"], s["faces"], np.zeros(len(keep), np.uint8))
    assert v0.shape == (0, 3) and f0.shape == (0, 3)
    v1, f1, _ = R.compact(s["vertices"], s["faces"], np.ones(len(keep), np.uint8))
    assert np.array_equal(v1, s["vertices"]) and np.array_equal(f1, s["faces"])
    # a face with an index outside [0, V) is dropped whatever the mask says
    bad = np.concatenate([s["faces"], [[0, 1, len(s["vertices"])], [-1, 0, 1]]]).astype(np.int32)
    v2, f2, _ = R.compact(s["vertices"], bad, np.ones(len(bad), np.uint8))
    assert np.array_equal(f2, s["faces"]) and np.array_equal(v2, s["vertices"])
    assert R.select_faces(bad, np.ones(len(s["vertices"]), np.int32), 1, "any")[-2:].tolist() == [0, 0]


def test_component_mask():
    v, f = R.room_mesh()
    fv, ff, n_added = R.floaters(len(v))
    faces = np.concatenate([f, ff])
    label, faces_of = R.components(faces, len(v) + len(fv))
    keep = R.component_mask(faces, label, faces_of, min_faces=3)
    assert keep[:len(f)].all() and not keep[len(f):].any() and n_added == 10
    largest = R.component_mask(faces, label, faces_of, keep_largest=True)
    assert largest.sum() == 338 and largest[:338].all(), "six walls tie on 338 faces: the lowest label wins"
