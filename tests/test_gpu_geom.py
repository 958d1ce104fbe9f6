"""The geometric evaluation on the GPU, through the C ABI (api.py): nearest neighbours bit for bit against the numpy brute force
(tests/geom_ref.py) and against the on-device brute-force twin, the mesh sampler against its restatement, the metrics, known
geometry end to end, and the error paths."""
import numpy as np
import pytest

from nerf_prv_amd import _lib as L
from nerf_prv_amd import api
from tests import geom_ref, instances, util
from tests.test_geom_host import R0, RES, linear_sphere_grid

pytestmark = pytest.mark.gpu

SLOT = 44  # slots of their own: the session context is shared with the other GPU modules


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def field_mesh(ctx, kw, res, seed=util.SEED_A, slot=SLOT):
    ctx.synthetic_model(slot, api.field_desc(**kw), seed)
    thr = float(np.median(ctx.density_grid(slot, min(res, 64)).cpu().numpy()))
    return ctx.marching_cubes(slot, res, threshold=thr, colors=False)


def clustered(rng, n, lo=0.0, ext=1.0):
    """95 % of the points in 0.1 % of the box volume (a cube of a tenth of the side), the rest uniform"""
    k = int(0.95 * n)
    a = (0.63 + 0.1 * rng.random((k, 3))) * ext + lo
    b = rng.random((n - k, 3)) * ext + lo
    return rng.permutation(np.concatenate([a, b]).astype(np.float32))


def families(ctx):
    rng = np.random.default_rng(7)
    u = lambda n: rng.random((n, 3), dtype=np.float32)
    m = field_mesh(ctx, util.SMALL, 48)
    on_mesh = m.sample(20011, seed=3).cpu().numpy()
    on_mesh_q = m.sample(19997, seed=4).cpu().numpy()
    m.close()
    plane = u(20000)
    plane[:, 1] = np.float32(0.375)
    dup = np.repeat(u(10007), 2, axis=0)
    far = (np.array([40, -7, 3], np.float32) + (u(20001) - np.float32(0.5)) * np.float32(0.1)).astype(np.float32)
    far_q = (np.array([40, -7, 3], np.float32) + (u(19999) - np.float32(0.5)) * np.float32(0.12)).astype(np.float32)
    outside = np.concatenate([u(7000) + np.float32(1.5), u(7000) * np.float32(0.2) - np.float32(3.0),
                              (u(6001) * np.array([1, 1, 0.01], np.float32) + np.array([0, 0, 1.001], np.float32))]).astype(np.float32)
    line = np.zeros((5000, 3), np.float32)
    line[:, 2] = rng.random(5000, dtype=np.float32)
    return {
        "uniform": (u(20000), u(20000)),
        "mesh": (on_mesh_q, on_mesh),
        "clustered": (clustered(rng, 19999), clustered(rng, 20003)),
        "clustered_uniform_queries": (u(8191), clustered(rng, 20003)),
        "planar": (u(9999), plane),
        "planar_on_plane": (plane[::3] + np.array([0.001, 0, 0.002], np.float32), plane),
        "duplicated": (u(10001), dup),
        "far_from_origin": (far_q, far),
        "outside_the_box": (outside, u(20000)),
        "one_reference": (u(1000), u(1)),
        "one_repeated_point": (u(777), np.tile(u(1), (300, 1))),
        "line": (u(3001), line),
        "odd_sizes": (u(65), u(257)),
        "tiny": (u(1), u(3)),
        "63_by_4097": (u(63), u(4097)),
    }


@pytest.fixture(scope="module")
def nn_inputs(ctx):
    return families(ctx)


@pytest.mark.parametrize("family", ["uniform", "mesh", "clustered", "clustered_uniform_queries", "planar", "planar_on_plane", "duplicated",
                                    "far_from_origin", "outside_the_box", "one_reference", "one_repeated_point", "line", "odd_sizes",
                                    "tiny", "63_by_4097"])
def test_nearest_neighbours_equal_the_brute_force_reference_bit_for_bit(ctx, nn_inputs, family):
    q, p = nn_inputs[family]
    want_d2, want_id = geom_ref.nearest(q, p)
    for algorithm in (L.NN_GRID, L.NN_BRUTE):
        idx = ctx.nn_index(p, algorithm)
        d2, ids = idx.query(q)
        d2, ids = d2.cpu().numpy(), ids.cpu().numpy()
        print(family, algorithm, idx.info(), "tests", idx.tests(), "of", len(q) * len(p), "d2 mismatches",
              int((bits(d2) != bits(want_d2)).sum()), "id mismatches", int((ids != want_id).sum()))
        assert np.array_equal(bits(d2), bits(want_d2)), (family, algorithm)
        assert np.array_equal(ids.astype(np.int64), want_id), (family, algorithm)
        if algorithm == L.NN_GRID:
            d2b, idsb = idx.query(q)  # the order inside a cell may vary from run to run: the results must not
            assert d2b.cpu().numpy().tobytes() == d2.tobytes() and idsb.cpu().numpy().tobytes() == ids.tobytes()
            assert idx.info()["n"] == len(p)
        else:
            assert idx.tests() == len(q) * len(p)
        idx.close()


def test_grid_equals_brute_force_on_the_device_at_a_million_points(ctx):
    """2^20 x 2^20 on mesh samples of the FIELD_256 synthetic model, and on the clustered set: identical bytes, and the grid forms
    strictly fewer distances than brute force (a counter of candidate tests, not a timer)"""
    n = 1 << 20
    m = field_mesh(ctx, api.FIELD_256, 256)
    a, b = m.sample(n, seed=1), m.sample(n, seed=2)
    m.close()
    rng = np.random.default_rng(9)
    t = ctx.torch
    sets = {"mesh": (a, b), "clustered": (t.from_numpy(clustered(rng, n)).to(ctx.device), t.from_numpy(clustered(rng, n)).to(ctx.device))}
    grid = {}
    for name, (q, p) in sets.items():
        idx = ctx.nn_index(p)
        d2, ids = idx.query(q)
        grid[name] = (d2.cpu().numpy(), ids.cpu().numpy(), idx.tests(), idx.info())
        idx.close()
        print(name, "grid", grid[name][3], "tests", grid[name][2], "brute", n * n, "ratio", n * n / max(1, grid[name][2]))
    assert grid["mesh"][2] < n * n // 100  # strictly less distance work, by a wide margin on a surface
    assert grid["clustered"][2] < n * n
    for name, (q, p) in sets.items():
        idx = ctx.nn_index(p, L.NN_BRUTE)
        d2, ids = idx.query(q)
        idx.close()
        assert d2.cpu().numpy().tobytes() == grid[name][0].tobytes(), name
        assert ids.cpu().numpy().tobytes() == grid[name][1].tobytes(), name


def sphere_mesh(ctx, res=RES):
    return ctx.marching_cubes_grid(ctx.torch.from_numpy(linear_sphere_grid(res)).to(ctx.device), threshold=2.5)


def strata_triangles(v, t, n):
    """first and last triangle each of the n strata can reach, from the restated weights"""
    w = geom_ref.triangle_weights(v, t)
    W = sum(w)
    scan = np.concatenate([[0], np.cumsum(np.array(w, np.uint64))[:-1]]).astype(np.uint64)
    lo = np.array([k * W // n for k in range(n)], np.uint64)
    hi = np.array([max((k + 1) * W // n - 1, k * W // n) for k in range(n)], np.uint64)
    return np.searchsorted(scan, lo, side="right") - 1, np.searchsorted(scan, hi, side="right") - 1


@pytest.mark.parametrize("which", ["F4_5", "F2_10", "sphere"])
def test_mesh_sample_equals_the_reference(ctx, which):
    m = sphere_mesh(ctx, 48) if which == "sphere" else field_mesh(ctx, instances.MATRIX[which].kw, 40)
    v, t = m.vertices, m.triangles
    assert len(t) > 1000
    for n, seed in ((5000, 0), (4099, 0xFEEDFACE12345678)):
        xyz, tri = m.sample(n, seed, want_triangles=True)
        want_xyz, want_tri = geom_ref.sample_mesh(v, t, n, seed)
        assert np.array_equal(tri.cpu().numpy().astype(np.int64), want_tri)
        assert np.array_equal(bits(xyz.cpu().numpy()), bits(want_xyz))
    a = m.sample(3000, 5)
    b, tb = m.sample(3000, 5, want_triangles=True)
    c, tc = m.sample(3000, 6, want_triangles=True)
    assert a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes()  # a pure function of (mesh, n, seed)
    assert c.cpu().numpy().tobytes() != b.cpu().numpy().tobytes()
    # another seed: other points, each inside the same stratum's run of triangles
    first, last = strata_triangles(v, t, 3000)
    for ids in (tb.cpu().numpy(), tc.cpu().numpy()):
        assert (ids >= first).all() and (ids <= last).all()
    m.close()


def test_metrics_equal_the_reference(ctx):
    rng = np.random.default_rng(12)
    rec = rng.random((15000, 3), dtype=np.float32)
    ref = (rng.random((11003, 3), dtype=np.float32) * np.float32(0.9) + np.float32(0.02)).astype(np.float32)
    tau = 0.02
    want = geom_ref.metrics(rec, ref, tau)
    got = ctx.geometry_metrics(rec, ref, tau)
    again = ctx.geometry_metrics(rec, ref, tau)
    print(got)
    assert got == again  # deterministic run to run
    for k in ("n_rec", "n_ref", "precision", "recall", "fscore", "hausdorff_rec", "hausdorff_ref"):
        assert got[k] == want[k], k
    assert 0 < got["precision"] < 1 and 0 < got["recall"] < 1
    rel = max(len(rec), len(ref)) * 2.0 ** -53  # the worst-case error of an fp64 sum of non-negative terms in any order
    for k in ("accuracy", "completeness", "accuracy_sq", "completeness_sq", "chamfer"):
        assert abs(got[k] - want[k]) <= rel * want[k], (k, got[k], want[k])
    same = ctx.geometry_metrics(rec, rec, 0.0)
    assert same["chamfer"] == 0 and same["fscore"] == 1.0 and same["hausdorff_rec"] == 0


def test_known_geometry_end_to_end(ctx):
    """the mesh of an analytic sphere (sigma linear in the radius, res 96), sampled, against points placed on the same sphere:
    accuracy and completeness below one grid step; against the sphere shrunk by four steps both move to that offset within one
    step (tests/test_geom_host.py checks the same bounds on the numpy pipeline alone)"""
    step = 1.0 / (RES - 1)
    m = sphere_mesh(ctx)
    rec = m.sample(200000, seed=5)
    m.close()
    same = ctx.geometry_metrics(rec, geom_ref.sphere_points(200000, R0), step)
    print(same)
    assert same["accuracy"] < step and same["completeness"] < step
    assert same["fscore"] == 1.0
    delta = 4 * step
    shrunk = ctx.geometry_metrics(rec, geom_ref.sphere_points(200000, R0 - delta), step)
    print(shrunk)
    assert abs(shrunk["accuracy"] - delta) < step and abs(shrunk["completeness"] - delta) < step
    assert shrunk["fscore"] == 0.0


def test_errors_are_codes_and_messages(ctx):
    t = ctx.torch
    good = t.rand((100, 3), device=ctx.device)
    for bad_value in (float("nan"), float("inf")):
        bad = good.clone()
        bad[37, 1] = bad_value
        with pytest.raises(api.PrvError) as e:
            ctx.nn_index(bad)
        assert e.value.code == L.PRV_E_INVALID and "non-finite" in str(e.value)
        idx = ctx.nn_index(good)
        with pytest.raises(api.PrvError) as e:
            idx.query(bad)
        assert e.value.code == L.PRV_E_INVALID and "non-finite" in str(e.value)
        idx.close()
        with pytest.raises(api.PrvError) as e:
            ctx.geometry_metrics(good, bad, 0.1)
        assert e.value.code == L.PRV_E_INVALID
    with pytest.raises(api.PrvError) as e:
        ctx.nn_index(t.zeros((0, 3), device=ctx.device))
    assert e.value.code == L.PRV_E_INVALID
    import ctypes as C

    lib, h = ctx.lib, C.c_void_p()
    host = np.zeros((10, 3), np.float32)
    assert lib.prv_nn_index_create(ctx.handle, None, 10, None, C.byref(h)) == L.PRV_E_INVALID  # NULL points
    assert lib.prv_nn_index_create(ctx.handle, api._ptr(host), 10, None, C.byref(h)) == L.PRV_E_INVALID  # a host pointer
    assert b"not a device pointer" in lib.prv_last_error(ctx.handle)
    assert lib.prv_nn_index_create(ctx.handle, api._ptr(good), 100, C.byref(L.NNOpts(algorithm=9)), C.byref(h)) == L.PRV_E_INVALID
    idx = ctx.nn_index(good)
    d2 = t.empty(10, device=ctx.device)
    ids = t.empty(10, dtype=t.int32, device=ctx.device)
    assert lib.prv_nn_query(idx.handle, api._ptr(host), 10, api._ptr(d2), api._ptr(ids)) == L.PRV_E_INVALID
    assert lib.prv_nn_query(idx.handle, api._ptr(good), 10, None, api._ptr(ids)) == L.PRV_E_INVALID
    assert lib.prv_nn_query(idx.handle, api._ptr(good), 0, api._ptr(d2), api._ptr(ids)) == L.PRV_E_INVALID
    idx.close()
    out = L.GeomMetrics()
    assert lib.prv_geometry_metrics(ctx.handle, api._ptr(good), 100, api._ptr(host), 10, 0.1, C.byref(out)) == L.PRV_E_INVALID
    assert lib.prv_geometry_metrics(ctx.handle, api._ptr(good), 100, api._ptr(good), 100, float("nan"), C.byref(out)) == L.PRV_E_INVALID
    # an empty mesh, n = 0, a host pointer for the samples
    empty = ctx.marching_cubes_grid(t.zeros((9, 8, 7), dtype=t.float32, device=ctx.device))
    with pytest.raises(api.PrvError) as e:
        empty.sample(10)
    assert e.value.code == L.PRV_E_STATE and "no triangles" in str(e.value)
    empty.close()
    m = sphere_mesh(ctx, 24)
    with pytest.raises(api.PrvError) as e:
        m.sample(0)
    assert e.value.code == L.PRV_E_INVALID
    assert lib.prv_mesh_sample(m.handle, 10, 0, api._ptr(host), None) == L.PRV_E_INVALID
    assert lib.prv_mesh_sample(m.handle, 10, 0, None, None) == L.PRV_E_INVALID
    m.close()
    # an index that outlives its context is inert: errors, no crash
    other = api.Context(0)
    idx = other.nn_index(np.random.default_rng(1).random((50, 3), dtype=np.float32))
    assert idx.info()["n"] == 50
    other.close()
    with pytest.raises(api.PrvError) as e:
        idx.info()
    assert e.value.code == L.PRV_E_STATE
    assert lib.prv_nn_query(idx.handle, api._ptr(good), 10, api._ptr(d2), api._ptr(ids)) == L.PRV_E_STATE
    idx.close()


def test_testbed_compute_geometry_metrics(ctx):
    """a synthetic model against samples of its own mesh: Chamfer below one grid step, in dataset units"""
    tb = api.Testbed(0)
    try:
        tb.synthetic_model(api.field_desc(**util.SMALL), util.SEED_A)
        res, n = 96, 1 << 20
        thr = float(np.median(tb.ctx.density_grid(tb._slot, 48).cpu().numpy()))
        m = tb.ctx.marching_cubes(tb._slot, res, threshold=thr, colors=False)
        assert len(m.triangles) > 1000
        ref = api.engine_to_dataset(m.sample(n, seed=77).cpu().numpy(), tb.scale, tb.offset)
        m.close()
        out = tb.compute_geometry_metrics(ref, resolution=(res, res, res), n_samples=n, thresh=thr)
        print(out)
        step = 1.0 / (res - 1) / tb.scale  # dataset units
        assert out["n_rec"] == n and out["n_ref"] == n
        assert 0 < out["chamfer"] < step and all(np.isfinite(v) for v in out.values())
    finally:
        tb.ctx.close()


def test_metrics_with_an_existing_reference_index_are_the_same(ctx):
    rng = np.random.default_rng(21)
    rec, ref = rng.random((9001, 3), dtype=np.float32), rng.random((7003, 3), dtype=np.float32)
    ref_dev = ctx._points(ref)
    want = ctx.geometry_metrics(rec, ref_dev, 0.03)
    for algorithm in (L.NN_GRID, L.NN_BRUTE):
        idx = ctx.nn_index(ref_dev, algorithm)
        assert ctx.geometry_metrics(rec, ref_dev, 0.03, ref_index=idx) == want
        assert ctx.geometry_metrics(rec, ref_dev, 0.03, ref_index=idx) == want  # the index is reusable
        with pytest.raises(api.PrvError) as e:
            ctx.geometry_metrics(rec, ref_dev[:100], 0.03, ref_index=idx)
        assert e.value.code == L.PRV_E_INVALID
        idx.close()


def test_a_sliver_thin_reference_box_still_finds_every_neighbour(ctx):
    """an axis whose extent is so small that cells per unit length would overflow gets one layer of cells"""
    rng = np.random.default_rng(22)
    p = rng.random((3000, 3), dtype=np.float32)
    p[:, 2] = np.where(rng.random(3000) < 0.5, np.float32(0), np.float32(1e-44))  # a subnormal extent
    q = rng.random((1000, 3), dtype=np.float32) * np.float32(1e-3)
    q[:, :2] = rng.random((1000, 2), dtype=np.float32)
    want_d2, want_id = geom_ref.nearest(q, p)
    idx = ctx.nn_index(p)
    d2, ids = idx.query(q)
    assert idx.info()["dims"][2] == 1
    assert np.array_equal(bits(d2.cpu().numpy()), bits(want_d2)) and np.array_equal(ids.cpu().numpy().astype(np.int64), want_id)
    idx.close()


# ---- the planner (prv_planner, `evaluate_geometry: 1`)
def _planner(tmp_path, name, extra, timeout=600):
    import os
    import subprocess

    from tests.test_gpu_planner import GOLD, ROOT, YAML

    exe = os.path.join(ROOT, "nerf_prv_amd", "prv_planner")
    assert os.path.exists(exe), "prv_planner missing: run __graft_entry__.build()"
    pre = tmp_path / name
    pre.mkdir()
    cfg = pre / "cfg.yaml"
    cfg.write_text(YAML.format(pre=pre, vs=os.path.join(GOLD, "hemisphere"), method=7,
                               model_source="train_steps: 300\ntrain_rays: 1024\ntrain_width: 64\ntrain_height: 36\nground_truth_seed: 4242\n"
                                            "train_deterministic: 1\nsave_members: 1\ndump_scores: 1\nevaluate: 1\nevaluate_views: 5\n" + extra))
    out = subprocess.run([exe, str(cfg)], input="21\nobjA\n-1\n", text=True, capture_output=True, timeout=timeout)
    return out, pre / "Compare" / "ShapeNet" / "objA_m7_v1_t0"


def _tree(save, skip=("train_time", "infer_time", "run_time.txt")):
    """relative path -> bytes of every file of an output tree except the wall-clock ones and the geometry files"""
    out = {}
    for p in sorted(save.rglob("*")):
        rel = str(p.relative_to(save))
        if p.is_file() and not rel.startswith(skip) and not rel.endswith("_geometry.txt"):
            out[rel] = p.read_bytes()
    return out


def test_planner_writes_a_geometry_file_beside_every_metrics_file(ctx, tmp_path):
    """the small train-in-loop configuration with deterministic training: with `evaluate_geometry: 1` every metrics/<it>.txt has a
    metrics/<it>_geometry.txt with finite values and n_ref == geometry_samples; without the key none is written and every other
    output is byte for byte the same; a run whose reference is unusable stops with a message before it trains anything"""
    samples = 30000
    on, save_on = _planner(tmp_path, "on", f"evaluate_geometry: 1\ngeometry_mc_res: 64\ngeometry_samples: {samples}\n")
    assert on.returncode == 0, on.stdout + on.stderr
    metrics = sorted(p for p in (save_on / "metrics").iterdir() if not p.name.endswith("_geometry.txt"))
    assert metrics, "the run evaluated nothing"
    for p in metrics:
        g = p.with_name(p.stem + "_geometry.txt")
        assert g.exists(), g
        m = api.read_geometry_metrics(g)
        print(g.name, m)
        assert list(m) == list(geom_ref.FIELDS)
        assert m["n_ref"] == samples and m["n_rec"] == samples
        assert all(np.isfinite(v) for v in m.values())
        assert 0 <= m["accuracy"] <= 0.35 and 0 <= m["completeness"] <= 0.35  # dataset units: the unit cube's diagonal is sqrt(3) / scale = 0.346
        assert m["chamfer"] == (m["accuracy"] + m["completeness"]) / 2 and 0 <= m["fscore"] <= 1
    off, save_off = _planner(tmp_path, "off", "")
    assert off.returncode == 0, off.stdout + off.stderr
    assert not list(save_off.rglob("*_geometry.txt"))
    a, b = _tree(save_on), _tree(save_off)
    assert sorted(a) == sorted(b) and len(a) > 10
    assert [k for k in a if a[k].replace(str(tmp_path / "on").encode(), b"") != b[k].replace(str(tmp_path / "off").encode(), b"")] == []
    bad, save_bad = _planner(tmp_path, "bad", f"evaluate_geometry: 1\ngeometry_reference: \"{tmp_path}/missing.pcd\"\n")
    assert bad.returncode != 0 and "geometry_reference" in bad.stderr and "nothing was trained" in bad.stderr
    assert "train_members:" not in bad.stderr and not (save_bad / "metrics").exists()


def test_planner_takes_a_pcd_cloud_as_the_reference(ctx, tmp_path):
    """geometry_reference: an ASCII .pcd in the dataset frame, brought to the engine frame with the run's scale and offset"""
    pts = geom_ref.sphere_points(4000, 0.03, centre=(0.0, 0.0, 0.0)).astype(np.float32)
    pcd = tmp_path / "ref.pcd"
    head = ("# .PCD v0.7 - Point Cloud Data file format\nVERSION 0.7\nFIELDS x y z rgb\nSIZE 4 4 4 4\nTYPE F F F U\nCOUNT 1 1 1 1\n"
            f"WIDTH {len(pts)}\nHEIGHT 1\nVIEWPOINT 0 0 0 1 0 0 0\nPOINTS {len(pts)}\nDATA ascii\n")
    pcd.write_text(head + "".join(f"{x:.9g} {y:.9g} {z:.9g} 8421504\n" for x, y, z in pts))
    out, save = _planner(tmp_path, "pcd", f"evaluate_geometry: 1\ngeometry_mc_res: 64\ngeometry_samples: 20000\ngeometry_reference: \"{pcd}\"\n")
    assert out.returncode == 0, out.stdout + out.stderr
    files = list((save / "metrics").glob("*_geometry.txt"))
    assert files
    for g in files:
        m = api.read_geometry_metrics(g)
        print(g.name, m)
        assert m["n_ref"] == len(pts) and m["n_rec"] == 20000 and all(np.isfinite(v) for v in m.values())
