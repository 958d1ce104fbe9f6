"""Marching-cubes case table (generated), the CPU reference's meshes, and the mesh file writer (no GPU needed)."""
import os

import numpy as np
import pytest

from tests import mesh_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_generator_reproduces_the_committed_header():
    gen = mesh_ref.generator()
    with open(os.path.join(ROOT, "nerf_prv_amd", "csrc", "prv_mc_tables.hpp")) as fh:
        assert fh.read() == gen.render_header()


def test_every_case_uses_its_crossing_edges_once_per_loop():
    masks, tri, ntri = mesh_ref.tables()
    gen = mesh_ref.generator()
    for case in range(256):
        crossing = {e for e in range(12) if (masks[case] >> e) & 1}
        assert masks[case] == sum(1 << e for e, (a, b) in enumerate(gen.EDGES) if ((case >> a) & 1) != ((case >> b) & 1))
        t = [tuple(x) for x in tri[case, :ntri[case]]]
        assert {e for x in t for e in x} == crossing, case
        # directed mesh edges: fan diagonals appear in both directions, the loops' segments once -- and every crossing edge
        # has exactly one segment out and one in (it lies on exactly one loop, once)
        use = {}
        for x in t:
            assert len(set(x)) == 3, (case, x)
            for k in range(3):
                d = (x[k], x[(k + 1) % 3])
                use[d] = use.get(d, 0) + 1
        boundary = [d for d, n in use.items() if n == 1 and (d[1], d[0]) not in use]
        assert all(n == 1 for n in use.values()), case
        outs = sorted(d[0] for d in boundary)
        ins = sorted(d[1] for d in boundary)
        assert outs == sorted(crossing) and ins == sorted(crossing), case
        assert len(t) == len(crossing) - 2 * len(gen.case_loops(case)[0]), case
    assert max(ntri) == tri.shape[1]


@pytest.mark.parametrize("k", range(20))
def test_reference_meshes_are_closed_manifolds(k):
    sigma, thr = mesh_ref.adversarial_grids()[k]
    v, n, t = mesh_ref.marching_cubes(sigma, threshold=thr)
    assert len(t) > 0
    assert mesh_ref.is_closed_manifold(t)  # every edge in two triangles, with opposite winding
    assert np.isfinite(v).all() and (v >= 0).all() and (v <= 1).all()
    assert len(np.unique(t)) == len(v)  # every vertex is used


EDGE_GRIDS = {name: (sigma, thr) for name, sigma, thr in mesh_ref.edge_grids()}


@pytest.mark.parametrize("name", list(EDGE_GRIDS))
def test_reference_on_the_edge_grids_is_finite_and_on_its_edges(name):
    sigma, thr = EDGE_GRIDS[name]
    assert sigma.dtype == np.float32 and sigma.size <= 266240
    v, n, t = mesh_ref.marching_cubes(sigma, threshold=thr)
    rz, ry, rx = sigma.shape
    _, _, ia, ib = mesh_ref.crossing_edges(sigma, thr)
    axes = mesh_ref.grid_axes((rx, ry, rz), (0, 0, 0), (1, 1, 1))
    pa = np.stack([axes[a][ia[:, a]] for a in range(3)], 1)
    pb = np.stack([axes[a][ib[:, a]] for a in range(3)], 1)
    assert len(v) == len(pa) and (len(v) > 0 or name == "huge_thr3e38")  # nothing is above 3e38: the one empty mesh
    assert np.isfinite(v).all()
    assert ((v >= pa) & (v <= pb)).all()  # exactly: pa <= pb, equal off the edge's axis, and fp32 rounding is monotonic
    assert np.isfinite(n).all()
    length = np.linalg.norm(n.astype(np.float64), axis=1)
    assert ((length == 0) | (np.abs(length - 1) <= 1e-5)).all()
    assert t.dtype == np.uint32 and (len(t) == 0 or int(t.max()) < len(v))
    # every vertex is used, with no exception for thin grids: res >= 2 on every axis, so every grid edge belongs to a cell,
    # and a cell's triangles use all of its crossing edges (test_every_case_uses_its_crossing_edges_once_per_loop)
    assert len(np.unique(t)) == len(v)


def test_edge_grids_hold_what_they_are_for():
    """so that the GPU tests on these grids cannot be hollow"""
    _, _, ntri = mesh_ref.tables()
    sigma, thr = EDGE_GRIDS["noise_ragged_scan"]
    inside, vid, _, _ = mesh_ref.crossing_edges(sigma, thr)
    hist = np.bincount(mesh_ref.cell_cases(inside).ravel(), minlength=256)
    assert (hist > 0).all()  # all 256 cases
    assert ntri.max() == 5 and (hist[ntri >= 4] >= 10).all()
    assert sigma.size == 4160 * 64  # waves of 64 points: one scan chunk of 4096 and a ragged one of 64
    per_wave = np.diff(vid.reshape(-1, 3 * 64)[:, -1], prepend=-1)  # crossings per wave
    assert per_wave.min() > 0 and per_wave.mean() > 90
    sigma, thr = EDGE_GRIDS["noise_4097_waves"]
    assert 4096 * 64 < sigma.size <= 4097 * 64 and sigma.size % 64 == 63  # 4097 waves, the last one lane short
    sigma, thr = EDGE_GRIDS["noise_ragged_cells"]
    rz, ry, rx = sigma.shape
    assert (rz - 2) * ry * rx > 4096 * 64 + 64  # cells (and their triangles) in waves past the first scan chunk
    assert EDGE_GRIDS["thin_2x2x15"][0].size < 64 < EDGE_GRIDS["thin_2x2x31"][0].size < 128 and EDGE_GRIDS["thin_9x9x2"][0].shape[2] == 2
    for name in ("plateau_thr1", "plateau_thr2"):
        sigma, thr = EDGE_GRIDS[name]
        v, _, t = mesh_ref.marching_cubes(sigma, threshold=thr)
        assert (sigma == thr).mean() > 0.2
        assert len(np.unique(v, axis=0)) < len(v)  # coincident vertices (t = 0 on every edge of an on-threshold corner)
        a, b, c = (v[t[:, k]].astype(np.float64) for k in range(3))
        assert (np.linalg.norm(np.cross(b - a, c - a), axis=1) == 0).any()  # zero-area triangles
    sigma = EDGE_GRIDS["signed_thr0"][0]
    assert (np.signbit(sigma) & (sigma == 0)).any() and (sigma < 0).any() and (sigma > 0).any()
    sigma = EDGE_GRIDS["subnormal"][0]
    assert (sigma == 0).mean() > 0.2 and sigma.max() < np.finfo(np.float32).tiny and (sigma > 0).mean() > 0.7
    sigma = EDGE_GRIDS["huge_thr0"][0]
    with np.errstate(over="ignore"):
        assert np.isinf(sigma.max() - sigma.min()) and np.isinf(np.float32(1e38) - sigma.min())
    for name in ("nonfinite", "nonfinite_block"):
        sigma = EDGE_GRIDS[name][0]
        for kind in (np.isposinf, np.isneginf, np.isnan):
            assert 0.02 < kind(sigma).mean() < 0.05
        for ax in range(3):
            lo, hi = np.moveaxis(sigma, ax, 0)[:-1], np.moveaxis(sigma, ax, 0)[1:]
            fin_lo, fin_hi = np.isfinite(lo), np.isfinite(hi)
            assert (np.isposinf(lo) & fin_hi & (hi <= 0.5)).any()  # (+inf, finite outside)
            assert (fin_lo & (lo > 0.5) & np.isneginf(hi)).any()   # (finite inside, -inf)
            assert (np.isnan(lo) & fin_hi & (hi > 0.5)).any()      # (NaN, finite inside)
            assert (np.isposinf(lo) & np.isnan(hi)).any()          # (+inf, NaN)
            assert (np.isposinf(lo) & np.isneginf(hi)).any()       # (+inf, -inf)
    block = np.isposinf(EDGE_GRIDS["nonfinite_block"][0][5:8, 6:9, 9:12])
    assert block.all()


def test_reference_sphere_is_oriented_outwards():
    r = 40
    ax = np.linspace(0, 1, r).astype(np.float32)
    z, y, x = np.meshgrid(ax, ax, ax, indexing="ij")
    d = np.sqrt((x - 0.5) ** 2 + (y - 0.5) ** 2 + (z - 0.5) ** 2)
    sigma = np.exp(8.0 * (0.3 - d)).astype(np.float32)
    v, n, t = mesh_ref.marching_cubes(sigma, threshold=2.5)
    r_iso = 0.3 - np.log(2.5) / 8.0
    assert mesh_ref.euler_characteristic(len(v), t) == (2, True)
    assert abs(mesh_ref.signed_volume(v, t) / (4 / 3 * np.pi * r_iso ** 3) - 1) < 0.01
    radial = (v - 0.5) / np.linalg.norm(v - 0.5, axis=1, keepdims=True)
    assert (np.einsum("ij,ij->i", radial, n) > 0.99).all()  # -grad sigma points outwards


# ---------------------------------------------------------------- the file writer (host only)
def parse_ply(path):
    data = open(path, "rb").read()
    end = data.index(b"end_header\n") + len(b"end_header\n")
    header = data[:end].decode().splitlines()
    assert header[0] == "ply" and header[1] == "format binary_little_endian 1.0"
    nv = int([l for l in header if l.startswith("element vertex")][0].split()[-1])
    nf = int([l for l in header if l.startswith("element face")][0].split()[-1])
    props = [l.split()[1:] for l in header if l.startswith("property")]
    assert props == [["float", "x"], ["float", "y"], ["float", "z"], ["float", "nx"], ["float", "ny"], ["float", "nz"],
                     ["uchar", "red"], ["uchar", "green"], ["uchar", "blue"], ["list", "uchar", "int", "vertex_indices"]]
    vt = np.dtype([("p", "<f4", 3), ("n", "<f4", 3), ("c", "u1", 3)])
    verts = np.frombuffer(data, vt, nv, end)
    ft = np.dtype([("k", "u1"), ("i", "<i4", 3)])
    faces = np.frombuffer(data, ft, nf, end + nv * vt.itemsize)
    assert end + nv * vt.itemsize + nf * ft.itemsize == len(data)
    assert (faces["k"] == 3).all()
    return verts["p"], verts["n"], verts["c"], faces["i"]


def parse_obj(path):
    v, vn, f = [], [], []
    for line in open(path):
        p = line.split()
        if not p or p[0].startswith("#"):
            continue
        if p[0] == "v":
            v.append([float(x) for x in p[1:7]])
        elif p[0] == "vn":
            vn.append([float(x) for x in p[1:4]])
        elif p[0] == "f":
            ids = [x.split("//") for x in p[1:]]
            assert all(a == b for a, b in ids)
            f.append([int(a) - 1 for a, _ in ids])
    v = np.array(v, np.float64).reshape(-1, 6)
    return (v[:, :3].astype(np.float32), np.array(vn, np.float32).reshape(-1, 3), np.rint(v[:, 3:] * 255).astype(np.uint8),
            np.array(f, np.int64).reshape(-1, 3))


def _sample_mesh():
    rng = np.random.default_rng(7)
    v = rng.random((50, 3)).astype(np.float32)
    n = rng.standard_normal((50, 3)).astype(np.float32)
    c = rng.integers(0, 256, (50, 3)).astype(np.uint8)
    t = rng.integers(0, 50, (80, 3)).astype(np.uint32)
    return v, n, c, t


@pytest.mark.parametrize("ext", [".ply", ".obj", ".PLY"])
def test_mesh_files_parse_back_in_the_dataset_frame(tmp_path, ext):
    from nerf_prv_amd import api

    v, n, c, t = _sample_mesh()
    scale, offset = 0.8, (0.5, 0.25, -0.125)
    path = tmp_path / ("mesh" + ext)
    api.write_mesh(path, v, t, n, c, scale, offset)
    pv, pn, pc, pt = (parse_ply if ext.lower() == ".ply" else parse_obj)(path)
    want = api.engine_to_dataset(v, scale, offset).astype(np.float32)  # q = (e2, e0, e1); (q - offset) / scale
    assert np.array_equal(pv, want)
    assert np.array_equal(pn, n[:, [2, 0, 1]])
    assert np.array_equal(pc, c)
    assert np.array_equal(pt, t.astype(np.int64))


@pytest.mark.parametrize("ext", [".ply", ".obj"])
def test_empty_mesh_file_is_valid(tmp_path, ext):
    from nerf_prv_amd import api

    path = tmp_path / ("empty" + ext)
    api.write_mesh(path, np.zeros((0, 3)), np.zeros((0, 3)), None, None, 1.0, (0, 0, 0))
    pv, pn, pc, pt = (parse_ply if ext == ".ply" else parse_obj)(path)
    assert len(pv) == len(pn) == len(pc) == len(pt) == 0


def test_mesh_file_rejects_bad_arguments(tmp_path):
    from nerf_prv_amd import _lib as L
    from nerf_prv_amd import api

    v, n, c, t = _sample_mesh()
    for bad in ("mesh.stl", "mesh", "mesh.ply.txt"):
        with pytest.raises(api.PrvError) as e:
            api.write_mesh(tmp_path / bad, v, t, n, c)
        assert e.value.code == L.PRV_E_INVALID and ".ply or .obj" in str(e.value)
        assert not (tmp_path / bad).exists()
    with pytest.raises(api.PrvError) as e:
        api.write_mesh(tmp_path / "m.ply", v, np.array([[0, 1, 50]]), n, c)  # vertex id out of range
    assert e.value.code == L.PRV_E_INVALID
    with pytest.raises(api.PrvError) as e:
        api.write_mesh(tmp_path / "m.ply", v, t, n, c, scale=0.0)
    assert e.value.code == L.PRV_E_INVALID
    with pytest.raises(api.PrvError) as e:
        api.write_mesh(tmp_path / "no_such_dir" / "m.obj", v, t, n, c)
    assert e.value.code == L.PRV_E_IO
