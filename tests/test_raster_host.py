"""The triangle rasteriser without a GPU: the CPU reference (tests/raster_ref.py) gives the answers one can work out by hand and
holds a tessellated sphere's depth against the analytic one; the planner's `coverage_occluder` key parses and is policed; the C
ABI's new symbols are declared, exported and bound."""
import os
import re
import subprocess

import numpy as np
import pytest

from nerf_prv_amd import _lib, api
from tests import coverage_ref, raster_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32
W = H = 8
# at the origin, looking along +z, focal length 8, principal point (0, 0): a point (x, y, z) lands on u = 8 x / z, v = 8 y / z
CAM = coverage_ref.Cam([[1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 1, 0]], 8, 8, 0, 0)


def at_pixels(uv, d):
    """engine points that project onto the pixel coordinates uv at depth d (exact where uv * d / 8 is)"""
    uv = np.asarray(uv, np.float64)
    return np.concatenate([uv * d / 8.0, np.full((len(uv), 1), d)], axis=1).astype(np.float32)


# vertices ON the centres of pixels (1, 1), (5, 1) and (1, 5), depth 2: every coordinate is exact in float32
CORNER = at_pixels([[1.5, 1.5], [5.5, 1.5], [1.5, 5.5]], 2.0)
CORNER_PIXELS = {(x, y) for y in range(1, 6) for x in range(1, 6) if (x - 1) + (y - 1) <= 4}


def filled(depth):
    return {(int(x), int(y)) for y, x in zip(*np.nonzero(depth))}


def test_vertices_and_edges_on_pixel_centres_are_inside():
    """the legs run through the centres of row 1 and column 1, the hypotenuse through (5,1) (4,2) (3,3) (2,4) (1,5): 5 + 4 + 3 + 2
    + 1 = 15 pixels, vertices and edges included, each at exactly depth 2 (the triangle is parallel to the image)"""
    d = ref.depth(CAM, CORNER, [[0, 1, 2]], W, H)
    assert filled(d) == CORNER_PIXELS and len(CORNER_PIXELS) == 15
    assert set(np.unique(d).tolist()) == {0.0, 2.0}


def test_the_mirror_wound_twin_gives_the_same_bytes():
    a = ref.depth(CAM, CORNER, [[0, 1, 2]], W, H)
    for twin in ([0, 2, 1], [2, 1, 0], [1, 0, 2], [1, 2, 0]):
        assert ref.depth(CAM, CORNER, [twin], W, H).tobytes() == a.tobytes()


def test_triangles_without_area_write_nothing():
    line = at_pixels([[1.5, 1.5], [3.5, 3.5], [5.5, 5.5]], 2.0)  # three centres on one diagonal
    assert not ref.depth(CAM, line, [[0, 1, 2]], W, H).any()
    assert not ref.depth(CAM, CORNER, [[0, 0, 1], [2, 1, 2], [1, 1, 1]], W, H).any()  # a repeated id
    assert not ref.depth(CAM, CORNER, np.zeros((0, 3), np.uint32), W, H).any()  # no triangle at all
    assert not ref.depth(CAM, np.zeros((0, 3), np.float32), np.zeros((0, 3), np.uint32), W, H).any()


def test_two_triangles_sharing_an_edge_leave_no_empty_pixel_along_it():
    """the square of centres (1,1)..(5,5) cut along either diagonal: all 25 pixels, the diagonal's included; and a skew quad with
    vertices off the grid fills the same pixels whichever diagonal cuts it"""
    sq = at_pixels([[1.5, 1.5], [5.5, 1.5], [5.5, 5.5], [1.5, 5.5]], 2.0)
    want = {(x, y) for y in range(1, 6) for x in range(1, 6)}
    assert filled(ref.depth(CAM, sq, [[0, 1, 2], [0, 2, 3]], W, H)) == want
    assert filled(ref.depth(CAM, sq, [[0, 1, 3], [1, 2, 3]], W, H)) == want
    quad = at_pixels([[0.7, 1.1], [6.9, 0.3], [7.4, 6.2], [1.9, 7.6]], 3.0)
    a = ref.depth(CAM, quad, [[0, 1, 2], [0, 2, 3]], W, H)
    b = ref.depth(CAM, quad, [[0, 1, 3], [1, 2, 3]], W, H)
    assert filled(a) == filled(b) and len(filled(a)) > 25
    assert set(np.unique(a).tolist()) == {0.0, 3.0} and a.tobytes() == b.tobytes()


@pytest.mark.parametrize("d", [1.7, 0.001, 12345.678, 1.0000001])
def test_a_fronto_parallel_triangle_gives_exactly_its_depth(d):
    """every vertex at depth (float)d: the interpolated inverse depth is 1 / d to a few float64 roundings, far inside the float32
    rounding interval of d"""
    tri = at_pixels([[0.3, 0.2], [7.9, 1.1], [3.3, 7.7]], d)
    out = ref.depth(CAM, tri, [[0, 1, 2]], W, H)
    assert len(filled(out)) > 10 and set(np.unique(out).view(np.uint32).tolist()) == {0, int(f32(d).view(np.uint32))}


def test_a_triangle_with_a_vertex_behind_or_far_outside_is_dropped_whole():
    tri = CORNER.copy()
    tri[2, 2] = -1.0
    assert not ref.depth(CAM, tri, [[0, 1, 2]], W, H).any()
    tri = CORNER.copy()
    tri[1, 0] = f32(2.0 * 32768 / 8)  # u = 32768 exactly: refused; one float below it: kept
    assert not ref.depth(CAM, tri, [[0, 1, 2]], W, H).any()
    tri[1, 0] = np.nextafter(tri[1, 0], f32(0))
    assert ref.depth(CAM, tri, [[0, 1, 2]], W, H).any()
    tri[0, 1] = np.nan
    assert not ref.depth(CAM, tri, [[0, 1, 2]], W, H).any()


def test_the_nearer_of_two_triangles_wins_and_a_point_behind_it_is_hidden():
    near, far = CORNER, at_pixels([[0.5, 0.5], [7.5, 0.5], [0.5, 7.5]], 4.0)
    v = np.concatenate([far, near])
    keys = ref.depth_keys(CAM, v, [[0, 1, 2], [3, 4, 5]], W, H)
    d = np.where(keys == ref.NEVER, 0, keys).view(np.float32)
    assert d[2, 2] == 2.0 and d[0, 0] == 4.0 and d[7, 7] == 0.0
    pts = np.concatenate([at_pixels([[2.5, 2.5]], 1.0), at_pixels([[2.5, 2.5]], 2.0), at_pixels([[2.5, 2.5]], 3.0),
                          at_pixels([[7.5, 7.5]], 9.0), at_pixels([[9.5, 2.5]], 1.0)])
    # in front of the mesh; exactly on it (visible at tolerance 0); behind it; a pixel no triangle covers; outside the image
    assert ref.visible(CAM, pts, keys, W, H, 0.0).tolist() == [True, True, False, True, False]
    assert ref.visible(CAM, pts, keys, W, H, 0.5).tolist() == [True, True, True, True, False]  # 3 <= 2 * 1.5


# ---- a tessellated sphere against the analytic depth
def uv_sphere(centre, radius, n_lat, n_lon):
    """vertices ON the sphere (float64 -> float32), triangles: two fans at the poles, quads cut in two between"""
    th = np.linspace(0, np.pi, n_lat + 1)[1:-1]
    ph = np.linspace(0, 2 * np.pi, n_lon, endpoint=False)
    ring = np.stack([np.outer(np.sin(th), np.cos(ph)), np.outer(np.sin(th), np.sin(ph)), np.outer(np.cos(th), np.ones(n_lon))], axis=-1)
    v = np.concatenate([[[0, 0, 1.0]], ring.reshape(-1, 3), [[0, 0, -1.0]]]) * radius + np.asarray(centre, np.float64)
    idx = lambda i, j: 1 + i * n_lon + j % n_lon
    tri = []
    for j in range(n_lon):
        tri.append([0, idx(0, j), idx(0, j + 1)])
        tri.append([len(v) - 1, idx(n_lat - 2, j + 1), idx(n_lat - 2, j)])
        for i in range(n_lat - 2):
            tri += [[idx(i, j), idx(i + 1, j), idx(i + 1, j + 1)], [idx(i, j), idx(i + 1, j + 1), idx(i, j + 1)]]
    return v.astype(np.float32), np.asarray(tri, np.uint32)


def test_the_depth_of_a_tessellated_sphere_against_the_analytic_ray_sphere_depth():
    """a sphere of radius R = 0.5 at distance D = 2 on the optical axis, 64 x 64 pixels, focal length 64.

    THE BOUND.  The mesh's vertices lie on the sphere, so a facet with circumradius r_c lies in the shell between radius
    R - s and R, with the sagitta s = R - sqrt(R^2 - r_c^2); s is taken for the largest r_c of the mesh.  Along a ray whose
    closest approach to the centre is b, the sphere of radius r is met at t(r) = m - sqrt(r^2 - b^2) (m: the distance to the
    closest approach), so the mesh is met between t(R) and t(R - s): the error in t is at most
        sqrt(R^2 - b^2) - sqrt((R - s)^2 - b^2),
    which grows with b; the test looks at the pixels with b <= 0.8 R and takes the value at b = 0.8 R.  The depth is z = t * dir_z
    with dir_z <= 1: the same bound holds for z.  The snap moves a projected vertex by at most 1/512 pixel per axis, i.e. the
    surface sideways by at most (sqrt(2) / 512) * D / f; at b <= 0.8 R the depth changes by at most b / sqrt(R^2 - b^2) = 4 / 3 per
    unit of sideways motion: 4/3 * sqrt(2) / 512 * D / f.  float32 roundings of the vertices and of the result (2^-24 relative each,
    at depth <= D) are below 1e-6 together; the bound carries 2e-6 for them."""
    R, D, f, n = 0.5, 2.0, 64.0, 64
    cam = coverage_ref.Cam([[1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 1, 0]], f, f, n / 2, n / 2)
    v, tri = uv_sphere((0, 0, D), R, 24, 48)
    got = ref.depth(cam, v, tri, n, n).astype(np.float64)
    p = v.astype(np.float64)[tri.astype(np.int64)]
    a, b, c = (np.linalg.norm(p[:, i] - p[:, (i + 1) % 3], axis=1) for i in range(3))
    area = 0.5 * np.linalg.norm(np.cross(p[:, 1] - p[:, 0], p[:, 2] - p[:, 0]), axis=1)
    r_c = float((a * b * c / (4 * area)).max())
    s = R - np.sqrt(R * R - r_c * r_c)
    b_max = 0.8 * R
    bound = (np.sqrt(R * R - b_max ** 2) - np.sqrt((R - s) ** 2 - b_max ** 2)) + 4 / 3 * np.sqrt(2) / 512 * D / f + 2e-6
    ys, xs = np.mgrid[0:n, 0:n]
    d = np.stack([(xs + 0.5 - n / 2) / f, (ys + 0.5 - n / 2) / f, np.ones((n, n))], axis=-1)
    d /= np.linalg.norm(d, axis=-1, keepdims=True)
    m = d[..., 2] * D  # the centre is (0, 0, D)
    b2 = D * D - m * m
    inner = b2 <= b_max ** 2
    want = (m - np.sqrt(np.where(inner, R * R - b2, 0))) * d[..., 2]
    err = np.abs(got - want)[inner]
    print(f"sagitta {s:.3g} (r_c {r_c:.3g}), bound {bound:.3g}, worst error {err.max():.3g} over {inner.sum()} pixels")
    assert inner.sum() > 400 and (got[inner] > 0).all()
    assert err.max() <= bound
    assert not got[b2 > (1.02 * R) ** 2].any()  # nothing beside the silhouette
    # the far side never shows: every depth is on the near half
    assert got[got > 0].max() <= D + 1e-6


# ---- the planner's key
PROBE = r"""
#include <iostream>
#include "coverage_eval.hpp"
int main(int argc, char** argv) {
  prvhost::FileStorage fs;
  if (!fs.open(argv[1])) return 2;
  const prvhost::CoverageEvalConfig c = prvhost::coverage_eval_config(fs);
  std::cout << "occluder=" << c.occluder << "\nmesh=" << c.mesh_occluder() << "\nproblem=" << prvhost::coverage_eval_problem(c, fs.has("geometry_reference"))
            << "\n" << prvhost::coverage_text(10, 8, 2, 4, 6, c.mesh_occluder());
  return 0;
}
"""


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    d = tmp_path_factory.mktemp("probe")
    (d / "probe.cpp").write_text(PROBE)
    exe = d / "probe"
    subprocess.check_call(["g++", "-std=c++17", "-O0", "-I", os.path.join(ROOT, "nerf_prv_amd", "host"), "-o", str(exe), str(d / "probe.cpp")])

    def run(text):
        (d / "cfg.yaml").write_text(text)
        return subprocess.check_output([str(exe), str(d / "cfg.yaml")], text=True)

    return run


POINT_FILE = "n_points\t10\nn_coverable\t8\nn_views\t2\ncovered\t4\ncoverage\t0.5\ngreedy_covered\t6\nefficiency\t0.66666666666666663\n"


def test_the_occluder_key_parses_defaults_to_points_and_is_policed(probe):
    assert probe("evaluate_coverage: 1\n") == "occluder=points\nmesh=0\nproblem=\n" + POINT_FILE
    assert probe("evaluate_coverage: 1\ncoverage_occluder: points\n") == "occluder=points\nmesh=0\nproblem=\n" + POINT_FILE
    assert probe("evaluate_coverage: 1\ncoverage_occluder: mesh\n") == "occluder=mesh\nmesh=1\nproblem=\n" + POINT_FILE + "occluder\tmesh\n"
    out = probe("evaluate_coverage: 1\ncoverage_occluder: mesh\ngeometry_reference: \"ref.pcd\"\n")
    assert "problem=coverage_occluder: mesh needs the ground-truth field's mesh, and geometry_reference names a cloud" in out
    out = probe("evaluate_coverage: 1\ncoverage_occluder: triangles\n")
    assert "problem=coverage_occluder must be points or mesh, got \"triangles\"\n" in out
    out = probe("evaluate_coverage: 1\ncoverage_occluder: points\ngeometry_reference: \"ref.pcd\"\n")  # a cloud and the point path: fine
    assert "problem=\n" in out
    assert probe("coverage_occluder: mesh\n").startswith("occluder=mesh\nmesh=0\nproblem=\n" + POINT_FILE[:10])  # evaluate_coverage off: nothing asks


def test_mesh_config_is_the_default_plus_the_keys():
    strip = lambda t: [l for l in t.splitlines() if l.strip() and not l.lstrip().startswith("#")]
    a = strip(open(os.path.join(ROOT, "configs", "DefaultConfiguration.yaml")).read())
    b = strip(open(os.path.join(ROOT, "configs", "CoverageEvalMesh.yaml")).read())
    assert b[: len(a)] == a and b[len(a)] == "evaluate_coverage: 1" and "coverage_occluder: mesh" in b[len(a):]
    assert not any(l.startswith("geometry_reference") for l in b)


# ---- the ABI and the documents
NEW = (("prv_mesh_from_arrays", 6), ("prv_mesh_depth", 8), ("prv_coverage_create_occluded", 12))


def header_text():
    return open(os.path.join(ROOT, "include", "prv.h")).read()


def test_new_symbols_declared_exported_and_bound():
    text = re.sub(r"/\*.*?\*/", "", header_text(), flags=re.S)
    out = subprocess.check_output(["nm", "-D", "--defined-only", os.path.join(ROOT, "nerf_prv_amd", "libprv_hip.so")], text=True)
    exported = {l.split()[-1] for l in out.splitlines() if " T " in l}
    for name, n_args in NEW:
        m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*)\)\s*;", text)
        assert m, f"{name} is not declared in prv.h"
        assert len([a for a in m.group(1).split(",") if a.strip()]) == n_args
        assert name in exported
        assert len(_lib.SIGNATURES[name][1]) == n_args
    lib = _lib.load()
    assert lib.prv_abi_version() == 5
    assert re.search(r"#define\s+PRV_ABI_VERSION\s+5\b.*prv_coverage_create_occluded.*additive", header_text())
    for attr in ("mesh_from_arrays", "mesh_depth", "coverage"):
        assert hasattr(api.Context, attr)
    import inspect
    assert "occluder" in inspect.signature(api.Context.coverage).parameters
    assert "occluder" in inspect.signature(api.Testbed.compute_coverage).parameters


def test_null_arguments_are_e_invalid_without_a_context():
    import ctypes as C
    lib = _lib.load()
    h = C.c_void_p()
    assert lib.prv_mesh_from_arrays(None, None, 0, None, 0, C.byref(h)) == _lib.PRV_E_INVALID and "context is NULL" in lib.prv_last_error(None).decode()
    assert lib.prv_mesh_depth(None, None, None, None, 1, 8, 8, None) == _lib.PRV_E_INVALID
    o = _lib.CoverageOpts(1, -1.0)
    rc = lib.prv_coverage_create_occluded(None, None, 0, None, None, None, 1, 8, 8, C.byref(o), None, C.byref(h))
    assert rc == _lib.PRV_E_INVALID and "depth_tol" in lib.prv_last_error(None).decode() and not h.value
    o = _lib.CoverageOpts(0, 0.02)  # point_size is ignored: the context is what is missing
    rc = lib.prv_coverage_create_occluded(None, None, 0, None, None, None, 1, 8, 8, C.byref(o), None, C.byref(h))
    assert rc == _lib.PRV_E_INVALID and "context is NULL" in lib.prv_last_error(None).decode()


def test_header_states_the_contract_and_the_limits():
    text = re.sub(r"\s*\n\s*\*\s*", " ", header_text())
    text = re.sub(r"\s+", " ", text)
    for phrase in ("X = (int64)rintf(u * 256.0f)", "Px = 256 x + 128, Py = 256 y + 128", "E_ab(P) = (Xb - Xa)(Py - Ya) - (Yb - Ya)(Px - Xa)",
                   "A2 = E_ab(c)", "w_a = E_bc(P) >= 0, w_b = E_ca(P) >= 0 and w_c = E_ab(P) >= 0", "i_k = 1.0 / (double)z_k",
                   "iz = ((double)w_a * i_a + (double)w_b * i_b) + (double)w_c * i_c", "z = (float)((double)A2 / iz)",
                   "|u| >= 32768.0f", "NO NEAR-PLANE CLIPPING", "stand outside the object", "The answer to that is the mesh occluder",
                   "PRV_RASTER_LIST_ENTRIES", "PRV_RASTER_SMALL_PIXELS"):
        assert phrase in text, phrase
