"""Connected components and floater removal on the GPU (prv_components.hip through the C ABI) against the numpy restatement
(tests/mesh_components_ref.py): labels, table (boxes as raw float bits) and the filtered arrays, all by equality."""
import ctypes as C

import numpy as np
import pytest

from nerf_prv_amd import _lib as L
from nerf_prv_amd import api
from tests import mesh_components_ref as cref
from tests import mesh_ref, util
from tests.test_mesh_tables import parse_ply

pytestmark = pytest.mark.gpu

SLOT = 46  # slots of their own: the session context is shared with the other GPU modules
TABLE = ("first_vertex", "n_vertices", "n_triangles", "lo", "hi")
ARRAYS = ("vertices", "normals", "colors", "triangles")

GRIDS = {"snake": lambda: (cref.snake_grid(), 2.5), "cubes_corner": lambda: (cref.touching_cubes(False), 2.5),
         "cubes_edge": lambda: (cref.touching_cubes(True), 2.5), "crowd": lambda: (cref.crowd_grid(), 2.5)}
GRIDS.update({"closed_%02d" % k: (lambda g=g: g) for k, g in enumerate(mesh_ref.adversarial_grids())})
GRIDS.update({name: (lambda s=sigma, t=thr: (s, t)) for name, sigma, thr in mesh_ref.edge_grids()})
_cache = {}


def extract(ctx, name):
    """(mesh of the grid, the restatement's components of that mesh); the grid and the restatement are computed once"""
    if name not in _cache:
        _cache[name] = GRIDS[name]()
    sigma, thr = _cache[name][:2]
    m = ctx.marching_cubes_grid(ctx.torch.from_numpy(sigma).to(ctx.device), threshold=thr)
    if len(_cache[name]) == 2:
        _cache[name] += (cref.components(m.vertices, m.triangles),)
    return m, _cache[name][2]


def assert_components_equal(got, want):
    for k in TABLE + ("vertex_component", "triangle_component"):
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, k
        g, w = (got[k].view(np.uint32), want[k].view(np.uint32)) if k in ("lo", "hi") else (got[k], want[k])
        assert np.array_equal(g, w), k


def assert_filter_equal(m, comp, **kw):
    """m.filter(**kw) equals the restatement's compaction; -> the filtered mesh"""
    f = m.filter(**kw)
    want = cref.compact(comp, cref.keep_mask(comp, **kw), m.vertices, m.normals, m.colors, m.triangles)
    assert f.counts() == (len(want[0]), len(want[3])), kw
    for a, w in zip(ARRAYS, want):
        assert getattr(f, a).tobytes() == w.tobytes(), (a, kw)
    return f


def test_snake_with_floaters(ctx):
    m, want = extract(ctx, "snake")
    assert m.counts() == (4590, 8692)
    got = m.components()
    print(f"snake: {len(got['first_vertex'])} components in {m.component_rounds()} rounds")
    assert 1 <= m.component_rounds() <= 64
    assert_components_equal(got, want)
    nt = got["n_triangles"]
    assert len(nt) == 122 and int(nt.max()) == 7724 and int((nt == 8).sum()) == 121
    big = int(np.argmax(nt))
    for kw in (dict(keep_largest=1), dict(min_triangles=9)):
        f = assert_filter_equal(m, want, **kw)
        assert f.counts()[1] == 7724 and mesh_ref.is_closed_manifold(f.triangles)
        one = f.components()  # the filtered mesh is a full mesh: it labels too
        assert len(one["first_vertex"]) == 1 and one["n_triangles"].tolist() == [7724]
        f.close()
    f = assert_filter_equal(m, want, keep_largest=3)
    kept = f.components()
    floaters = [k for k in range(122) if k != big][:2]
    assert sorted(kept["n_triangles"].tolist()) == [8, 8, 7724]
    assert f.counts()[0] == int(got["n_vertices"][[big] + floaters].sum())
    first = np.sort(got["first_vertex"][[big] + floaters])  # order kept: the new components start where the old ones did
    assert np.array_equal(f.vertices[kept["first_vertex"]], m.vertices[first])
    f.close()
    assert_filter_equal(m, want, min_diagonal=0.5).close()
    assert_filter_equal(m, want, min_triangles=8, keep_largest=40, min_diagonal=0.1).close()
    f = m.filter()
    for a in ARRAYS:
        assert getattr(f, a).tobytes() == getattr(m, a).tobytes(), a
    f.close()
    m.close()


@pytest.mark.parametrize("name", ["cubes_corner", "cubes_edge"])
def test_touching_cubes(ctx, name):
    m, want = extract(ctx, name)
    got = m.components()
    assert_components_equal(got, want)
    assert got["n_triangles"].tolist() == [44, 44] and got["n_vertices"].tolist() == [24, 24]
    f = assert_filter_equal(m, want, keep_largest=1)
    assert mesh_ref.is_closed_manifold(f.triangles)
    f.close()
    m.close()


@pytest.mark.parametrize("name", [n for n in GRIDS if n.startswith("closed_")] + [g[0] for g in mesh_ref.edge_grids()])
def test_hard_grids(ctx, name):
    m, want = extract(ctx, name)
    got = m.components()
    assert_components_equal(got, want)
    used = np.zeros(len(m.vertices), bool)
    used[m.triangles.reshape(-1)] = True
    lone = got["vertex_component"][~used]  # vertices that no triangle uses: components of their own with 0 triangles
    assert len(np.unique(lone)) == len(lone) and (got["n_triangles"][lone] == 0).all() and (got["n_vertices"][lone] == 1).all()
    assert int((got["n_triangles"] == 0).sum()) == len(lone)
    if len(got["first_vertex"]):
        assert m.component_rounds() <= 64
        median = int(np.median(got["n_triangles"]))
        assert_filter_equal(m, want, min_triangles=median + 1).close()
        assert_filter_equal(m, want, keep_largest=2).close()
    m.close()


def test_crowd_and_determinism(ctx):
    m, want = extract(ctx, "crowd")
    again, _ = extract(ctx, "crowd")
    got, got2 = m.components(), again.components()
    print(f"crowd: {m.counts()} vertices / triangles, {len(got['first_vertex'])} components in {m.component_rounds()} rounds")
    assert len(got["first_vertex"]) > 500 and m.counts()[0] % 64 != 0
    assert_components_equal(got, want)
    for k in got:
        assert got[k].tobytes() == got2[k].tobytes(), k
    kw = dict(min_triangles=200, keep_largest=300, min_diagonal=0.03)
    f, f2 = assert_filter_equal(m, want, **kw), again.filter(**kw)
    assert 0 < f.counts()[1] < m.counts()[1]
    for a in ARRAYS:
        assert getattr(f, a).tobytes() == getattr(f2, a).tobytes(), a
    for x in (f, f2, m, again):
        x.close()


def test_empty_mesh(ctx):
    m = ctx.marching_cubes_grid(ctx.torch.zeros((9, 8, 7), dtype=ctx.torch.float32, device=ctx.device))
    got = m.components()
    assert all(len(got[k]) == 0 for k in got) and got["lo"].shape == (0, 3) and m.component_rounds() == 0
    f = m.filter(keep_largest=1)
    assert f.counts() == (0, 0) and f.vertices.shape == (0, 3) and f.triangles.shape == (0, 3)
    assert len(f.components()["first_vertex"]) == 0
    f.close()
    m.close()


def test_bad_arguments_and_inert_meshes(ctx):
    lib = ctx.lib
    m, want = extract(ctx, "cubes_corner")

    def message(of_ctx=True):
        return (lib.prv_last_error(ctx.handle if of_ctx else None) or b"").decode()

    n, h, r = C.c_uint64(), C.c_void_p(), C.c_int()
    assert lib.prv_debug_mesh_component_rounds(m.handle, C.byref(r)) == L.PRV_E_STATE and "not been labelled" in message()
    assert lib.prv_mesh_components(m.handle, None) == L.PRV_E_INVALID and "n_components is NULL" in message()
    assert lib.prv_mesh_components(None, C.byref(n)) == L.PRV_E_INVALID and "mesh is NULL" in message(False)
    assert lib.prv_mesh_labels(None, None, None) == L.PRV_E_INVALID and "mesh is NULL" in message(False)
    assert lib.prv_mesh_component_info(m.handle, 2, None) == L.PRV_E_INVALID and "out_host is NULL" in message()
    table = (L.MeshComponent * 2)()
    assert lib.prv_mesh_component_info(m.handle, 1, table) == L.PRV_E_INVALID and "capacity 1 is below the mesh's 2" in message()
    assert lib.prv_mesh_component_info(m.handle, 2, table) == L.PRV_OK and table[1].n_triangles == 44
    assert lib.prv_mesh_labels(m.handle, None, None) == L.PRV_OK
    assert lib.prv_debug_mesh_component_rounds(m.handle, None) == L.PRV_E_INVALID and "rounds is NULL" in message()
    assert lib.prv_debug_mesh_component_rounds(m.handle, C.byref(r)) == L.PRV_OK and 1 <= r.value <= 64
    o = L.MeshFilterOpts()
    assert lib.prv_mesh_filter_default_opts(None) == L.PRV_E_INVALID and "NULL" in message(False)
    assert lib.prv_mesh_filter_default_opts(C.byref(o)) == L.PRV_OK and (o.min_triangles, o.keep_largest, o.min_diagonal) == (0, 0, 0.0)
    assert lib.prv_mesh_filter(m.handle, None, C.byref(h)) == L.PRV_E_INVALID and "options are NULL" in message()
    assert lib.prv_mesh_filter(m.handle, C.byref(o), None) == L.PRV_E_INVALID and "out is NULL" in message()
    assert lib.prv_mesh_filter(None, C.byref(o), C.byref(h)) == L.PRV_E_INVALID and "mesh is NULL" in message(False)
    for bad in (-1.0, float("nan"), float("inf")):
        with pytest.raises(api.PrvError) as e:
            m.filter(min_diagonal=bad)
        assert e.value.code == L.PRV_E_INVALID and "min_diagonal" in str(e.value), bad
    m.close()
    # meshes that outlive their context are inert: errors, no crash -- the filtered one too
    other = api.Context(0)
    sigma = other.torch.from_numpy(cref.touching_cubes(True)).to(other.device)
    m = other.marching_cubes_grid(sigma, threshold=2.5)
    f = m.filter(keep_largest=1)
    assert f.counts() == (24, 44)
    other.close()
    for x in (m, f):
        for call in (x.components, x.filter, x.component_rounds, x.counts):
            with pytest.raises(api.PrvError) as e:
                call()
            assert e.value.code == L.PRV_E_STATE and "context has been destroyed" in str(e.value)
        x.close()


def test_coloured_mesh_from_a_field(ctx, tmp_path):
    ctx.synthetic_model(SLOT, api.field_desc(**util.SMALL), util.SEED_A)
    thr = float(np.percentile(ctx.density_grid(SLOT, 40).cpu().numpy(), 80))
    m = ctx.marching_cubes(SLOT, 40, threshold=thr)
    got = m.components()
    want = cref.components(m.vertices, m.triangles)
    assert_components_equal(got, want)
    assert len(got["first_vertex"]) > 1 and len(np.unique(m.colors, axis=0)) > 10
    big = int(np.argmax(got["n_triangles"]))  # argmax: the first of equals, the tie rule
    f = assert_filter_equal(m, want, keep_largest=1)
    mask = got["vertex_component"] == big
    assert np.array_equal(f.colors, m.colors[mask]) and np.array_equal(f.normals.view(np.uint32), m.normals[mask].view(np.uint32))
    pts = f.sample(4096, 3).cpu().numpy()
    assert pts.shape == (4096, 3) and np.isfinite(pts).all()
    assert (pts >= got["lo"][big]).all() and (pts <= got["hi"][big]).all()
    f.save(tmp_path / "kept.ply", 1.0, (0, 0, 0))
    pv, pn, pc, pt = parse_ply(tmp_path / "kept.ply")
    assert (len(pv), len(pt)) == f.counts() and np.array_equal(pc, f.colors) and np.array_equal(pt, f.triangles.astype(np.int64))
    f.close()
    m.close()


def test_testbed_saves_and_measures_without_floaters(ctx, tmp_path):
    tb = api.Testbed(0)
    try:
        tb.synthetic_model(api.field_desc(**util.SMALL), util.SEED_A)
        tb.scale, tb.offset = 0.6, [0.4, 0.55, 0.3]
        thr = float(np.percentile(tb.ctx.density_grid(0, 40).cpu().numpy(), 80))
        m = tb.ctx.marching_cubes(0, 40, threshold=thr)
        comp = m.components()
        assert len(comp["first_vertex"]) > 1
        # the defaults: today's file, byte for byte
        m.save(tmp_path / "plain.ply", tb.scale, tb.offset)
        tb.compute_and_save_marching_cubes_mesh(str(tmp_path / "tb.ply"), (40, 40, 40), thresh=thr)
        assert (tmp_path / "tb.ply").read_bytes() == (tmp_path / "plain.ply").read_bytes()
        tb.compute_and_save_marching_cubes_mesh(str(tmp_path / "one.ply"), (40, 40, 40), thresh=thr, keep_largest=1)
        pv, pn, pc, pt = parse_ply(tmp_path / "one.ply")
        one = cref.components(pv, pt)
        assert len(one["first_vertex"]) == 1 and one["n_triangles"][0] == comp["n_triangles"].max()
        f = m.filter(keep_largest=1)
        f.save(tmp_path / "want.ply", tb.scale, tb.offset)
        assert (tmp_path / "one.ply").read_bytes() == (tmp_path / "want.ply").read_bytes()
        # metrics: the filtered mesh's own samples as the reference -> the filtered run is exact, the unfiltered one is not
        ref = api.engine_to_dataset(f.sample(20000, 0).cpu().numpy(), tb.scale, tb.offset)
        kw = dict(resolution=(40, 40, 40), n_samples=20000, thresh=thr, tau=0.01)
        clean = tb.compute_geometry_metrics(ref, keep_largest=1, **kw)
        plain = tb.compute_geometry_metrics(ref, **kw)
        assert clean["hausdorff_rec"] < 1e-6 and plain["hausdorff_rec"] > 100 * max(clean["hausdorff_rec"], 1e-6)
        f.close()
        m.close()
    finally:
        tb.ctx.close()
