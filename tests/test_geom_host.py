"""The geometric evaluation without a GPU: the numpy restatement (tests/geom_ref.py) against hand-known answers, the
sampling rule on a two-triangle mesh, the ABI bindings, the metrics file, and the reference pipeline on an analytic sphere."""
import ctypes as C
import os
import subprocess

import numpy as np

from nerf_prv_amd import _lib as L
from nerf_prv_amd import api
from tests import geom_ref, mesh_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def lattice(z, n=12, step=0.05):
    i = np.arange(n, dtype=np.float32) * np.float32(step)
    x, y = np.meshgrid(i, i)
    return np.stack([x.ravel(), y.ravel(), np.full(x.size, z, np.float32)], 1).astype(np.float32)


def test_parallel_lattices_are_their_distance_apart():
    d = 0.25  # exact in float32, and less than the lattice step's multiples that could compete: the nearest point is the one above
    a, b = lattice(0.0), lattice(d)
    for tau, f in ((d, 1.0), (np.nextafter(np.float32(d), np.float32(0)), 0.0)):
        m = geom_ref.metrics(a, b, tau)
        for k in ("accuracy", "completeness", "chamfer", "hausdorff_rec", "hausdorff_ref"):
            assert m[k] == d, k
        assert m["accuracy_sq"] == d * d and m["completeness_sq"] == d * d
        assert m["fscore"] == f and m["precision"] == f and m["recall"] == f


def test_a_set_against_itself_is_all_zeros():
    rng = np.random.default_rng(1)
    a = rng.random((500, 3), dtype=np.float32)
    d2, ids = geom_ref.nearest(a, a)
    assert (d2 == 0).all() and np.array_equal(ids, np.arange(500))
    m = geom_ref.metrics(a, a, 0.0)
    assert all(m[k] == 0 for k in ("accuracy", "completeness", "chamfer", "hausdorff_rec", "hausdorff_ref", "accuracy_sq"))
    assert m["fscore"] == 1.0 and m["n_rec"] == 500 and m["n_ref"] == 500


def test_ties_resolve_to_the_smallest_id():
    rng = np.random.default_rng(2)
    base = rng.random((100, 3), dtype=np.float32)
    ref = np.concatenate([base, base, base[::-1]])  # every point three times
    d2, ids = geom_ref.nearest(base, ref)
    assert (d2 == 0).all() and np.array_equal(ids, np.arange(100))
    d2, ids = geom_ref.nearest(np.array([[0.0, 0.0, 0.0]], np.float32), np.array([[1, 0, 0], [0, 1, 0], [0, 0, -1], [2, 0, 0]], np.float32))
    assert d2[0] == 1.0 and ids[0] == 0


def test_counter_rng_vector_form_equals_the_scalar_form():
    for seed, stream in ((0, 0x5A0), (0xDEADBEEFCAFEF00D, 0x5A3)):
        v = geom_ref.rng_u24_array(seed, stream, 50)
        assert [int(x) for x in v] == [geom_ref.rng_u24(seed, stream, i) for i in range(50)]
        assert v.max() < (1 << 24)


def two_triangles():
    """areas 3 : 1 in the plane z = 0.25, then a zero-area triangle (a repeated vertex) and a collinear one"""
    v = np.array([[0, 0, 0.25], [3, 0, 0.25], [0, 1, 0.25], [5, 5, 0.25], [6, 5, 0.25], [5, 6, 0.25], [9, 9, 9], [10, 10, 10]], np.float32)
    t = np.array([[6, 6, 7], [0, 1, 2], [6, 7, 6], [3, 4, 5], [0, 1, 1]], np.uint32)
    return v, t


def inside(p, a, b, c, eps=1e-5):
    m = np.stack([b - a, c - a], 1).astype(np.float64)
    uv, *_ = np.linalg.lstsq(m, (p - a).astype(np.float64), rcond=None)
    return uv[0] >= -eps and uv[1] >= -eps and uv[0] + uv[1] <= 1 + eps


def test_sampling_reference_on_two_triangles():
    v, t = two_triangles()
    w = geom_ref.triangle_weights(v, t)
    assert w[0] == 0 and w[2] == 0 and w[4] == 0 and w[1] == 3 * w[3] == 3 * (1 << 39)
    for n in (1, 7, 64, 1000, 4001):
        xyz, tri = geom_ref.sample_mesh(v, t, n, seed=11)
        assert xyz.dtype == np.float32 and xyz.shape == (n, 3)
        counts = np.bincount(tri, minlength=5)
        assert counts[0] == counts[2] == counts[4] == 0
        assert abs(counts[1] - 3 * n / 4) <= 1 and abs(counts[3] - n / 4) <= 1, (n, counts)
        assert (xyz[:, 2] == np.float32(0.25)).all()  # in the plane
        for p, k in zip(xyz[:200], tri[:200]):
            assert inside(p, *v[t[k]]), (p, k)
        assert (np.diff(tri) >= 0).all()  # stratified: the strata walk the triangles in order
    a, _ = geom_ref.sample_mesh(v, t, 500, seed=11)
    b, _ = geom_ref.sample_mesh(v, t, 500, seed=11)
    c, tc = geom_ref.sample_mesh(v, t, 500, seed=12)
    assert a.tobytes() == b.tobytes() and a.tobytes() != c.tobytes()


def test_bindings_and_struct_sizes(tmp_path):
    names = ["prv_mesh_sample", "prv_nn_default_opts", "prv_nn_index_create", "prv_nn_query", "prv_nn_index_info", "prv_debug_nn_tests",
             "prv_nn_index_destroy", "prv_geometry_metrics"]
    assert all(n in L.SIGNATURES for n in names)
    lib = L.load()
    o = L.NNOpts(algorithm=7)
    assert lib.prv_nn_default_opts(C.byref(o)) == L.PRV_OK and o.algorithm == L.NN_GRID
    # handles are checked before any GPU work: NULL is an error code and a message, not a crash
    assert lib.prv_nn_query(None, None, 1, None, None) == L.PRV_E_INVALID and b"NULL" in lib.prv_last_error(None)
    assert lib.prv_mesh_sample(None, 1, 0, None, None) == L.PRV_E_INVALID
    assert lib.prv_geometry_metrics(None, None, 1, None, 1, 0.1, None) == L.PRV_E_INVALID
    lib.prv_nn_index_destroy(None)
    src = tmp_path / "sizes.c"
    src.write_text('#include "prv.h"\n#include <stdio.h>\nint main(void) { printf("%zu %zu %d %d\\n", sizeof(prv_geom_metrics), '
                   "sizeof(prv_nn_opts), PRV_NN_GRID, PRV_NN_BRUTE); return 0; }\n")
    exe = tmp_path / "sizes"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)], text=True).split()]
    assert got == [C.sizeof(L.GeomMetrics), C.sizeof(L.NNOpts), L.NN_GRID, L.NN_BRUTE] and got[0] == 96
    assert api.GEOMETRY_FIELDS == geom_ref.FIELDS


def test_metrics_file_round_trips(tmp_path):
    rng = np.random.default_rng(3)
    m = geom_ref.metrics(rng.random((300, 3), dtype=np.float32), rng.random((200, 3), dtype=np.float32), 0.05)
    path = tmp_path / "0_geometry.txt"
    api.write_geometry_metrics(path, m)
    lines = open(path).read().splitlines()
    assert [l.split("\t")[0] for l in lines] == list(geom_ref.FIELDS) and lines[0] == "n_rec\t300"
    back = api.read_geometry_metrics(path)
    assert back == {k: m[k] for k in geom_ref.FIELDS}  # 17 significant digits: exact


def test_frame_conversions_are_inverses():
    rng = np.random.default_rng(4)
    p = rng.normal(size=(50, 3))
    e = api.dataset_to_engine(p, 0.33, (0.5, 0.4, 0.6))
    np.testing.assert_allclose(api.engine_to_dataset(e, 0.33, (0.5, 0.4, 0.6)), p, atol=1e-14)
    assert np.allclose(api.dataset_to_engine([[0, 0, 0]], 0.33, (0.5, 0.4, 0.6)), [[0.4, 0.6, 0.5]])


RES, R0 = 96, 0.3


def linear_sphere_grid(res=RES, r=R0, k=10.0):
    """sigma linear in the radius: the 2.5 iso-surface is the sphere of radius r exactly, and linear interpolation along an
    edge is exact up to the edge's own curvature"""
    ax = mesh_ref.grid_axes((res, res, res), (0, 0, 0), (1, 1, 1))
    z, y, x = np.meshgrid(ax[2], ax[1], ax[0], indexing="ij")
    d = np.sqrt((x - 0.5) ** 2 + (y - 0.5) ** 2 + (z - 0.5) ** 2)
    return (2.5 + k * (r - d)).astype(np.float32)


def test_reference_pipeline_on_an_analytic_sphere():
    """marching cubes (mesh_ref) -> sampling -> metrics, all in numpy: accuracy and completeness against points on the same
    sphere are below one grid step, and against a sphere shrunk by four grid steps both move to that offset within one step"""
    step = 1.0 / (RES - 1)
    v, _, t = mesh_ref.marching_cubes(linear_sphere_grid(), threshold=2.5)
    rec, _ = geom_ref.sample_mesh(v, t, 6000, seed=5)
    same = geom_ref.metrics(rec, geom_ref.sphere_points(6000, R0), tau=step)
    assert same["accuracy"] < step and same["completeness"] < step, same
    delta = 4 * step
    shrunk = geom_ref.metrics(rec, geom_ref.sphere_points(6000, R0 - delta), tau=step)
    assert abs(shrunk["accuracy"] - delta) < step and abs(shrunk["completeness"] - delta) < step, shrunk


# ---- the planner's side (nerf_prv_amd/host/geometry_eval.hpp; prv_planner-private, so it is compiled into a probe here)
PROBE = r"""
#include "geometry_eval.hpp"
#include <iostream>
using namespace prvhost;
int main(int argc, char** argv) {
  FileStorage fs;
  if (!fs.open(argv[1])) return 2;
  const GeometryEvalConfig g = geometry_eval_config(fs);
  std::cout << "on " << g.on << "\nmc_res " << g.mc_res << "\nsamples " << g.samples << "\ntau " << g.tau_for(0.1) << "\nreference [" << g.reference
            << "]\nproblem [" << geometry_eval_problem(g) << "]\n";
  prv_geom_metrics m{};
  m.n_rec = 7; m.n_ref = 9; m.accuracy = 0.5; m.completeness = 0.25; m.accuracy_sq = 1.0; m.completeness_sq = 4.0; m.chamfer = 0.375;
  m.precision = 1.0 / 3.0; m.recall = 0.5; m.fscore = 0.4; m.hausdorff_rec = 2.0; m.hausdorff_ref = 3.0;
  if (argc > 2) { FILE* f = fopen(argv[2], "w"); const std::string t = geometry_metrics_text(m, 5.0); fwrite(t.data(), 1, t.size(), f); fclose(f); }
  std::vector<float> p = {0.01f, -0.02f, 0.03f};
  const double off[3] = {0.5, 0.4, 0.6};
  geometry_to_engine(p, 5.0, off);
  printf("engine %.9g %.9g %.9g\n", p[0], p[1], p[2]);
  return 0;
}
"""


def run_probe(tmp_path, yaml_text, metrics_path=None):
    exe = tmp_path / "probe"
    if not exe.exists():
        (tmp_path / "probe.cpp").write_text(PROBE)
        subprocess.check_call(["g++", "-std=c++17", "-Wall", "-I", os.path.join(ROOT, "nerf_prv_amd", "host"),
                               str(tmp_path / "probe.cpp"), "-o", str(exe)])
    cfg = tmp_path / "cfg.yaml"
    cfg.write_text("%YAML:1.0\nname_of_pcd: \"objA\"\n" + yaml_text)
    out = subprocess.check_output([str(exe), str(cfg)] + ([str(metrics_path)] if metrics_path else []), text=True)
    return dict(l.split(" ", 1) for l in out.splitlines())


def test_planner_yaml_keys_parse_and_absent_keys_mean_off(tmp_path):
    off = run_probe(tmp_path, "evaluate: 1\n")
    assert off["on"] == "0" and off["mc_res"] == "256" and off["samples"] == str(1 << 20) and off["reference"] == "[]" and off["problem"] == "[]"
    assert float(off["tau"]) == 0.01 * 0.1  # 1 % of the object size
    on = run_probe(tmp_path, "evaluate_geometry: 1\ngeometry_mc_res: 96\ngeometry_samples: 5000\ngeometry_tau: 0.002   # dataset units\n"
                             "geometry_reference: \"/data/objA.pcd\"\n")
    assert on == dict(on="1", mc_res="96", samples="5000", tau="0.002", reference="[/data/objA.pcd]", problem="[]", engine=on["engine"])
    assert run_probe(tmp_path, "evaluate_geometry: 0\n")["on"] == "0"
    assert "pcd" in run_probe(tmp_path, "evaluate_geometry: 1\ngeometry_reference: \"mesh.ply\"\n")["problem"]
    assert "geometry_mc_res" in run_probe(tmp_path, "evaluate_geometry: 1\ngeometry_mc_res: 1\n")["problem"]
    assert "geometry_samples" in run_probe(tmp_path, "evaluate_geometry: 1\ngeometry_samples: 0\n")["problem"]
    # no config in the tree turns it on: existing runs are what they were
    for name in os.listdir(os.path.join(ROOT, "configs")):
        assert "evaluate_geometry" not in open(os.path.join(ROOT, "configs", name)).read(), name


def test_planner_metrics_writer_and_frame_change(tmp_path):
    path = tmp_path / "3_geometry.txt"
    out = run_probe(tmp_path, "", path)
    got = api.read_geometry_metrics(path)
    assert list(got) == list(geom_ref.FIELDS)  # struct order, the python writer's format
    assert got == dict(n_rec=7, n_ref=9, accuracy=0.1, completeness=0.05, accuracy_sq=1.0 / 25, completeness_sq=4.0 / 25, chamfer=0.375 / 5.0,
                       precision=1.0 / 3.0, recall=0.5, fscore=0.4, hausdorff_rec=0.4, hausdorff_ref=0.6)  # dataset units: / scale
    api.write_geometry_metrics(tmp_path / "again.txt", got)
    assert api.read_geometry_metrics(tmp_path / "again.txt") == got
    want = api.dataset_to_engine([[0.01, -0.02, 0.03]], 5.0, (0.5, 0.4, 0.6))[0]
    np.testing.assert_allclose([float(x) for x in out["engine"].split()], want, rtol=1e-6)
