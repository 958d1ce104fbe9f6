"""The numpy restatement of connected components and the floater filter (tests/mesh_components_ref.py) against known
answers and scipy, on meshes of the numpy marching cubes (tests/mesh_ref.py).  No GPU."""
import numpy as np
import pytest

from tests import mesh_components_ref as cref
from tests import mesh_ref

_meshes = {}


def mesh_of(name):
    """(vertices, normals, triangles) of a fixture grid at threshold 2.5, computed once"""
    if name not in _meshes:
        grid = {"snake": cref.snake_grid, "corner": lambda: cref.touching_cubes(False), "edge": lambda: cref.touching_cubes(True),
                "crowd": lambda: cref.crowd_grid(48, 120)}[name]()
        _meshes[name] = mesh_ref.marching_cubes(grid, threshold=2.5)
    return _meshes[name]


def test_snake_has_its_known_answer():
    v, n, t = mesh_of("snake")
    assert (len(v), len(t)) == (4590, 8692)
    c = cref.components(v, t)
    nt = c["n_triangles"]
    assert len(nt) == 122 and int(nt.max()) == 7724 and sorted(nt.tolist())[:-1] == [8] * 121
    big = int(np.argmax(nt))
    assert c["n_vertices"].sum() == len(v) and nt.sum() == len(t)
    assert np.array_equal(c["first_vertex"], np.sort(c["first_vertex"]))  # ranked by smallest vertex
    for k in (0, big, 121):  # the label is the smallest vertex id of the set, the box is the set's
        members = np.flatnonzero(c["vertex_component"] == k)
        assert members[0] == c["first_vertex"][k] and len(members) == c["n_vertices"][k]
        assert np.array_equal(c["lo"][k], v[members].min(axis=0)) and np.array_equal(c["hi"][k], v[members].max(axis=0))
    # the filter: the big piece alone is the closed tube; keep_largest=3 adds the two floaters with the lowest ids
    for kw in (dict(keep_largest=1), dict(min_triangles=9)):
        fv, fn, fc, ft = cref.filter_mesh(v, n, np.zeros((len(v), 3), np.uint8), t, **kw)
        assert len(ft) == 7724 and mesh_ref.is_closed_manifold(ft) and int(ft.max()) == len(fv) - 1
        assert np.array_equal(fv, v[c["vertex_component"] == big])
    keep = cref.keep_mask(c, keep_largest=3)
    floaters = [k for k in range(122) if k != big]
    assert np.flatnonzero(keep).tolist() == sorted([big] + floaters[:2])
    assert cref.keep_mask(c).all() and not cref.keep_mask(c, min_triangles=7725).any()
    # diagonals: a floater's box is a cell and a half across (0.14 of the unit cube at most); the tube spans the grid
    assert np.array_equal(cref.keep_mask(c, min_diagonal=0.5), np.arange(122) == big)
    fv, fn, fc, ft = cref.filter_mesh(v, n, np.zeros((len(v), 3), np.uint8), t)
    assert np.array_equal(fv, v) and np.array_equal(ft, t)


@pytest.mark.parametrize("name", ["corner", "edge"])
def test_touching_cubes_are_two_components(name):
    v, n, t = mesh_of(name)
    c = cref.components(v, t)
    assert c["n_triangles"].tolist() == [44, 44] and c["n_vertices"].tolist() == [24, 24]
    assert c["first_vertex"][0] == 0 and (c["vertex_component"][t] == c["triangle_component"][:, None]).all()


def test_unused_vertices_are_components_of_their_own():
    v = np.arange(18, dtype=np.float32).reshape(6, 3) * np.float32(-1)  # negative coordinates: lo / hi are not swapped
    t = np.array([[4, 2, 5]], np.uint32)
    c = cref.components(v, t)
    assert c["first_vertex"].tolist() == [0, 1, 2, 3] and c["n_triangles"].tolist() == [0, 0, 1, 0]
    assert c["vertex_component"].tolist() == [0, 1, 2, 3, 2, 2] and c["n_vertices"].tolist() == [1, 1, 3, 1]
    assert np.array_equal(c["lo"][2], v[5]) and np.array_equal(c["hi"][2], v[2])
    z = cref.components(np.array([[0.0, -0.0, 1.0], [-0.0, 0.0, 1.0]], np.float32), np.array([[0, 1, 1]]))
    assert np.signbit(z["lo"][0]).tolist() == [True, True, False] and np.signbit(z["hi"][0]).tolist() == [False, False, False]
    e = cref.components(np.zeros((0, 3), np.float32), np.zeros((0, 3), np.uint32))
    assert len(e["first_vertex"]) == 0 and len(cref.keep_mask(e)) == 0
    assert [len(a) for a in cref.compact(e, cref.keep_mask(e), *[np.zeros((0, 3))] * 4)] == [0, 0, 0, 0]


def test_keep_rule_ties_go_to_the_lower_id():
    c = dict(n_triangles=np.array([8, 20, 8, 20, 8], np.uint64), lo=np.zeros((5, 3), np.float32),
             hi=np.array([[3, 4, 0]] * 4 + [[3, 4, 12]], np.float32))
    assert cref.keep_mask(c, keep_largest=1).tolist() == [False, True, False, False, False]
    assert cref.keep_mask(c, keep_largest=3).tolist() == [True, True, False, True, False]
    assert cref.keep_mask(c, min_triangles=9, keep_largest=3).tolist() == [False, True, False, True, False]
    assert cref.keep_mask(c, min_diagonal=5.0).all() and cref.keep_mask(c, min_diagonal=5.5).tolist() == [False] * 4 + [True]
    assert cref.keep_mask(c, keep_largest=2, min_diagonal=5.5).tolist() == [False] * 5  # in the order of the rule


@pytest.mark.parametrize("name", ["snake", "corner", "edge", "crowd"] + ["closed_%02d" % k for k in range(20)] +
                         [g[0] for g in mesh_ref.edge_grids()])
def test_partition_agrees_with_scipy(name):
    sparse = pytest.importorskip("scipy.sparse")
    from scipy.sparse.csgraph import connected_components

    if name.startswith("closed_"):
        sigma, thr = mesh_ref.adversarial_grids()[int(name[7:])]
        v, n, t = mesh_ref.marching_cubes(sigma, threshold=thr)
    elif name in ("snake", "corner", "edge", "crowd"):
        v, n, t = mesh_of(name)
    else:
        sigma, thr = {g[0]: g[1:] for g in mesh_ref.edge_grids()}[name]
        v, n, t = mesh_ref.marching_cubes(sigma, threshold=thr)
    c = cref.components(v, t)
    e = np.concatenate([t[:, [0, 1]], t[:, [1, 2]]]).astype(np.int64)
    g = sparse.coo_matrix((np.ones(len(e)), (e[:, 0], e[:, 1])), shape=(len(v), len(v)))
    n_sp, lab = connected_components(g, directed=False) if len(v) else (0, np.zeros(0, np.int64))
    assert n_sp == len(c["first_vertex"])
    # the same partition: scipy's label is a function of ours and there are as many of each
    pairs = np.unique(np.stack([lab, c["vertex_component"].astype(np.int64)], 1), axis=0)
    assert len(pairs) == n_sp
    if len(t):
        assert (c["vertex_component"][t] == c["triangle_component"][:, None]).all()
