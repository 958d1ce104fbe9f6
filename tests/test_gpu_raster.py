"""The triangle rasteriser on the GPU, through the C ABI (api.py): prv_mesh_depth's buffers (raster_small_kernel,
raster_large_kernel) equal the restatement of tests/raster_ref.py bit for bit, whatever the threshold between the two paths, the
list's capacity and the view batches; coverage with a mesh occluder (raster_visible_kernel) equals the reference's bit matrix,
counts and depth, and sees nothing of a sphere nested in a closed one where the point path sees through; the error paths, empty
inputs, handles that outlive their context, prv_mesh_from_arrays as an ordinary mesh; and prv_planner with `coverage_occluder:
mesh`.  No tolerance anywhere: every comparison is of bytes or integers."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from nerf_prv_amd import _lib as L
from nerf_prv_amd import api
from tests import coverage_ref, raster_ref as ref
from tests import util
from tests.test_gpu_planner import GOLD, ROOT, YAML

pytestmark = pytest.mark.gpu

SLOT = 49  # a slot of its own: the session context is shared with the other GPU modules
N_VIEWS = 8
CENTRE = np.array([0.5, 0.5, 0.5], np.float32)  # where the hemisphere's cameras look (engine frame)
SHAPES = [(1, (16, 16)), (3, (33, 17)), (8, (80, 45))]
ENV = ("PRV_RASTER_SMALL_PIXELS", "PRV_RASTER_LIST_ENTRIES", "PRV_COVERAGE_ZBUF_BYTES")


def view_ids(n_views):
    return [0, 3, 6][:n_views] if n_views <= 3 else list(range(N_VIEWS))


def sphere(rng, n, radius, centre=CENTRE):
    d = rng.normal(size=(n, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    return (np.asarray(centre, np.float64) + radius * d).astype(np.float32)


@pytest.fixture(scope="module")
def cams(ctx, oracle):
    """eight pinhole views of the hemisphere (fov-at-centre intrinsics, rescaled to whatever size a call asks for)"""
    tms, scale, offset = util.hemisphere_transforms(oracle, util.fibonacci_hemisphere(N_VIEWS))
    cs = ctx.cameras_from_matrices(tms, util.FOV_X, 80, 45, scale, offset)
    yield cs
    cs.close()


def box_mesh(lo, hi):
    lo, hi = np.asarray(lo, np.float64), np.asarray(hi, np.float64)
    v = np.array([[(hi if (k >> a) & 1 else lo)[a] for a in range(3)] for k in range(8)], np.float32)
    quads = [(0, 1, 3, 2), (4, 6, 7, 5), (0, 4, 5, 1), (2, 3, 7, 6), (0, 2, 6, 4), (1, 5, 7, 3)]
    return v, np.array([t for a, b, c, d in quads for t in ((a, b, c), (a, c, d))], np.uint32)


@pytest.fixture(scope="module")
def meshes(ctx, cams):
    """name -> (vertices (n, 3) float32, triangles (m, 3) uint32), engine frame"""
    ctx.synthetic_model(SLOT, api.field_desc(**util.SMALL), util.SEED_A)
    thr = float(np.median(ctx.density_grid(SLOT, 48).cpu().numpy()))
    out = {}
    for res in (24, 48):
        m = ctx.marching_cubes(SLOT, res, threshold=thr, colors=False)
        out[f"mc{res}"] = (m.vertices.copy(), m.triangles.copy())
        m.close()
    c2w = cams.get(0)[0]
    eye, right, up, fwd = c2w[:, 3].astype(np.float64), c2w[:, 0].astype(np.float64), c2w[:, 1].astype(np.float64), c2w[:, 2].astype(np.float64)
    sign = 1.0 if np.dot(CENTRE - eye, fwd) > 0 else -1.0  # which way the camera looks along its z column
    # the hand-made families of the host test, placed in front of view 0: a triangle, its mirror-wound twin, a zero-area one, a
    # repeated id, a quad cut in two, a slanted triangle
    plane = lambda x, y, z: (eye + x * right + y * up + sign * z * fwd)
    v = np.array([plane(-0.3, -0.2, 1.2), plane(0.4, -0.25, 1.2), plane(-0.1, 0.3, 1.2), plane(0.0, 0.0, 1.0), plane(0.1, 0.1, 1.1), plane(0.2, 0.2, 1.2),
                  plane(-0.5, -0.4, 1.6), plane(0.5, -0.4, 1.6), plane(0.5, 0.4, 1.6), plane(-0.5, 0.4, 1.6), plane(-0.2, 0.1, 0.8), plane(0.3, 0.2, 1.5),
                  plane(0.0, -0.3, 2.0)], np.float32)
    out["hand_made"] = (v, np.array([[0, 1, 2], [0, 2, 1], [3, 4, 5], [0, 0, 1], [6, 7, 8], [6, 8, 9], [10, 11, 12]], np.uint32))
    # a box that fills every image and runs past all four borders; its corner 0 is moved behind view 0's eye
    bv, bt = box_mesh(CENTRE - 0.8, CENTRE + 0.8)  # (0.8 < 1.5 / sqrt(3): every camera of the hemisphere stands outside it)
    bv[0] = (eye - sign * 0.5 * fwd).astype(np.float32)
    out["box"] = (bv, bt)
    return out


def cam_list(camset, ids, w, h):
    return [coverage_ref.cam_at(camset, v, w, h) for v in ids]


_want = {}


def want_depth(cams, meshes, name, n_views, size):
    """the reference's buffers, computed once per input and shared by the tests that need them"""
    key = (name, n_views, size)
    if key not in _want:
        v, t = meshes[name]
        _want[key] = np.stack([ref.depth(c, v, t, size[0], size[1]) for c in cam_list(cams, view_ids(n_views), size[0], size[1])])
    return _want[key]


# ---- 1. prv_mesh_depth == the reference's bits
@pytest.mark.parametrize("n_views,size", SHAPES, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v))
@pytest.mark.parametrize("name", ["mc24", "mc48", "hand_made", "box"])
def test_mesh_depth_equals_the_reference_bit_for_bit(ctx, cams, meshes, name, n_views, size):
    v, t = meshes[name]
    want = want_depth(cams, meshes, name, n_views, size)
    with ctx.mesh_from_arrays(v, t) as m:
        got = ctx.mesh_depth(m, cams, view_ids(n_views), size[0], size[1]).cpu().numpy()
        stats = ctx.raster_stats()
    bad = int((got.view(np.uint32) != want.view(np.uint32)).sum())
    print(f"{name} {len(t)} triangles, {n_views} views {size}: filled {int((want > 0).sum())} of {want.size}, mismatches {bad}, {stats}")
    assert got.shape == want.shape and bad == 0
    assert stats["pairs"] == len(t) * n_views
    assert (want > 0).any()
    if name == "box":  # corner 0 is behind view 0: its six triangles are dropped there, the other six still fill the image
        cam0 = cam_list(cams, [0], size[0], size[1])[0]
        assert not coverage_ref.project(cam0, v[:1])[0][0] and coverage_ref.project(cam0, v[1:])[0].all()
        s0 = ref.Setup(cam0, v, t, size[0], size[1])
        assert len(s0.ids) > 0 and not any(0 in t[i] for i in s0.ids)  # (a face whose box misses a flat image is not in the setup either)
        assert ((s0.x0 == 0) & (s0.y0 == 0) & (s0.x1 == size[0] - 1) & (s0.y1 == size[1] - 1)).any()  # past all four borders
        assert stats["large"] > 0 and (want[0] > 0).all()
    if name.startswith("mc"):
        assert (want == 0).any()


# ---- 2. the threshold, the capacity and the batches change no byte
def test_threshold_capacity_and_batches_change_no_byte(ctx, cams, meshes, monkeypatch):
    """mc24 at 33 x 17 (sub-pixel to few-pixel boxes) and the hand-made set at 80 x 45; the box size of a chosen triangle comes from
    the reference's own setup"""
    for name, n_views, size in (("mc24", 3, (33, 17)), ("hand_made", 8, (80, 45)), ("box", 3, (33, 17))):
        v, t = meshes[name]
        ids = view_ids(n_views)
        want = want_depth(cams, meshes, name, n_views, size)
        s = ref.Setup(cam_list(cams, ids[:1], *size)[0] if name != "box" else cam_list(cams, ids[1:2], *size)[0], v, t, *size)
        sizes = np.unique(s.box_pixels())
        sizes = sizes[sizes >= 2]
        px = int(sizes[len(sizes) // 2])  # a box size that some triangle of the view has, with triangles on both sides of it
        pts = sphere(np.random.default_rng(2), 300, 0.25)
        with ctx.mesh_from_arrays(v, t) as m:
            with ctx.coverage(pts, cams, ids, *size, depth_tol=0.02, occluder=m) as cov:
                want_bits = [cov.bits(j) for j in range(len(ids))]
            tried = [dict(PRV_RASTER_SMALL_PIXELS=str(k)) for k in (1, px, px - 1, 0, 10 ** 9)]
            tried += [dict(PRV_RASTER_LIST_ENTRIES=str(k), PRV_RASTER_SMALL_PIXELS=str(max(px - 1, 0))) for k in (1, 64)] if name != "mc24" else \
                     [dict(PRV_RASTER_LIST_ENTRIES="64", PRV_RASTER_SMALL_PIXELS=str(max(px - 1, 0)))]
            tried += [dict(PRV_COVERAGE_ZBUF_BYTES="1"), dict(PRV_COVERAGE_ZBUF_BYTES="1", PRV_RASTER_LIST_ENTRIES="64", PRV_RASTER_SMALL_PIXELS="1")]
            large = []
            for env in tried:
                for k in ENV:
                    monkeypatch.delenv(k, raising=False)
                for k, val in env.items():
                    monkeypatch.setenv(k, val)
                got = ctx.mesh_depth(m, cams, ids, *size).cpu().numpy()
                large.append(ctx.raster_stats()["large"])
                assert got.tobytes() == want.tobytes(), env
                with ctx.coverage(pts, cams, ids, *size, depth_tol=0.02, occluder=m, want_depth=True) as cov:
                    assert all(np.array_equal(cov.bits(j), want_bits[j]) for j in range(len(ids))), env
                    assert cov.depth.cpu().numpy().tobytes() == want.tobytes(), env
            for k in ENV:
                monkeypatch.delenv(k, raising=False)
            print(name, "deferred pairs per setting", large)
            # 0: every pair with a box; 1 >= px - 1 > px (the chosen triangle changes path there); huge: none
            assert large[3] >= large[0] >= large[2] > large[1] >= large[4] == 0


# ---- 3. coverage with the mesh as the occluder == the reference
@pytest.fixture(scope="module")
def clouds(ctx, meshes):
    rng = np.random.default_rng(11)
    v, t = meshes["mc48"]
    with ctx.mesh_from_arrays(v, t) as m:
        samples = m.sample(4097, seed=5).cpu().numpy()
    return {"mesh_samples": samples, "wide_box": rng.uniform(-2.0, 3.0, (4097, 3)).astype(np.float32)}


def assert_coverage_matches(ctx, cams, ids, pts, mesh_arrays, m, w, h, tol):
    want_vis, want_d = ref.matrix(cam_list(cams, ids, w, h), pts, mesh_arrays[0], mesh_arrays[1], w, h, tol)
    cov = ctx.coverage(pts, cams, ids, w, h, point_size=7, depth_tol=tol, want_depth=True, occluder=m)
    got_d = cov.depth.cpu().numpy()
    print(f"n {len(pts)} views {len(ids)} {w}x{h} tol {tol}: visible {cov.visible().tolist()} want {want_vis.sum(axis=1).tolist()}")
    assert np.array_equal(got_d.view(np.uint32), want_d.view(np.uint32))
    for j in range(len(ids)):
        got, want = cov.bits(j), coverage_ref.pack(want_vis[j])
        assert got.shape == want.shape and np.array_equal(got, want), (j, int((got != want).sum()))
    assert cov.visible().tolist() == want_vis.sum(axis=1).tolist()
    assert cov.info() == dict(n_points=len(pts), n_views=len(ids), n_coverable=int(want_vis.any(axis=0).sum()))
    return want_vis, cov


@pytest.mark.parametrize("n", [1, 63, 64, 65, 4097])
@pytest.mark.parametrize("family", ["mesh_samples", "wide_box"])
def test_occluded_coverage_equals_the_reference_at_every_word_edge(ctx, cams, meshes, clouds, family, n):
    pts = clouds[family][:n]
    with ctx.mesh_from_arrays(*meshes["mc48"]) as m:
        want, cov = assert_coverage_matches(ctx, cams, [0, 3, 6], pts, meshes["mc48"], m, 33, 17, 0.02)
        if n == 4097:
            assert want.any() and not want.all()
        cov.close()


def test_curve_and_greedy_on_an_occluded_handle_equal_the_reference(ctx, cams, meshes, clouds):
    ids = list(range(N_VIEWS))
    with ctx.mesh_from_arrays(*meshes["mc48"]) as m:
        want, cov = assert_coverage_matches(ctx, cams, ids, clouds["mesh_samples"], meshes["mc48"], m, 80, 45, 0.02)
    for order in (ids, ids[::-1], [5, 5, 2, 0]):  # (the mesh is gone: the handle keeps the bit matrix)
        covered, first = cov.curve(order, want_first_seen=True)
        want_covered, want_first = coverage_ref.curve(want, order)
        assert covered.tolist() == want_covered and np.array_equal(first.cpu().numpy().view(np.uint32), want_first)
    for k in (1, 3, N_VIEWS):
        chosen, covered = cov.greedy(k)
        assert (chosen.tolist(), covered.tolist()) == coverage_ref.greedy(want, k)
    cov.close()


# ---- 4. the point of the feature
def test_a_closed_mesh_hides_the_sphere_inside_it_where_the_point_path_sees_through(ctx, cams):
    """a closed sphere of radius 0.3 (marching cubes on an analytic grid) around 4011 points of a radius-0.15 sphere: the mesh
    occluder sees 0 of them in every view -- from the reference alone, then from the GPU -- while the point path, given the inner
    points plus 500 points of the outer sphere at point_size 1, sees some: the holes between 500 points let the inside through"""
    t = ctx.torch
    g = t.linspace(0, 1, 48, dtype=t.float64, device=ctx.device)
    z, y, x = t.meshgrid(g, g, g, indexing="ij")
    sigma = (0.3 - t.sqrt((x - 0.5) ** 2 + (y - 0.5) ** 2 + (z - 0.5) ** 2)).to(t.float32)
    rng = np.random.default_rng(7)
    inner, outer = sphere(rng, 4011, 0.15), sphere(rng, 500, 0.3)
    ids = list(range(N_VIEWS))
    camsl = cam_list(cams, ids, 80, 45)
    with ctx.marching_cubes_grid(sigma, threshold=0.0) as m:
        assert len(m.triangles) > 1000
        r = np.linalg.norm(m.vertices.astype(np.float64) - 0.5, axis=1)
        assert 0.29 < r.min() and r.max() < 0.31
        want_vis, _ = ref.matrix(camsl, inner, m.vertices, m.triangles, 80, 45, 0.02)
        assert want_vis.sum(axis=1).tolist() == [0] * N_VIEWS  # the reference alone
        with ctx.coverage(inner, cams, ids, 80, 45, depth_tol=0.02, occluder=m) as cov:
            assert cov.visible().tolist() == [0] * N_VIEWS and cov.info()["n_coverable"] == 0
    both = np.concatenate([inner, outer])
    want_pts, _ = coverage_ref.matrix(camsl, both, 80, 45, 1, 0.02)
    assert want_pts[:, :4011].sum() > 0
    with ctx.coverage(both, cams, ids, 80, 45, point_size=1, depth_tol=0.02) as cov:
        seen = sum(int(np.unpackbits(cov.bits(j).view(np.uint8), bitorder="little")[:4011].sum()) for j in range(N_VIEWS))
    print("inner points seen through the 500-point shell, summed over the views:", seen)
    assert seen == int(want_pts[:, :4011].sum()) > 0


# ---- 5. in front, beside, and exactly on
def test_points_in_front_of_beside_and_exactly_on_the_mesh(ctx):
    """a camera at the engine frame's origin looking along +z, a triangle parallel to the image at depth 2 with its vertices on
    pixel centres: every coordinate is exact, so the hand-worked answer of the host test holds on the GPU"""
    cam = coverage_ref.Cam([[1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 1, 0]], 8, 8, 4, 4)
    uv = np.array([[1.5, 1.5], [5.5, 1.5], [1.5, 5.5]])
    tri = np.concatenate([(uv - 4) * 2.0 / 8.0, np.full((3, 1), 2.0)], axis=1).astype(np.float32)
    at = lambda u, v, d: [(u - 4) * d / 8.0, (v - 4) * d / 8.0, d]
    pts = np.array([at(2.5, 2.5, 1.0), at(2.5, 2.5, 2.0), at(2.5, 2.5, 3.0), at(7.5, 7.5, 9.0), at(9.5, 2.5, 1.0)], np.float32)
    keys = ref.depth_keys(cam, tri, [[0, 1, 2]], 8, 8)
    assert ref.visible(cam, pts, keys, 8, 8, 0.0).tolist() == [True, True, False, True, False]
    # the same camera as a camset: the engine's c2w row r is the dataset matrix's row (1, 2, 0)[r] with columns 1 and 2 negated
    tm = np.array([[0, 0, -1, 0], [1, 0, 0, 0], [0, -1, 0, 0], [0, 0, 0, 1]], np.float64)
    cs = ctx.cameras_from_matrices_intr(tm[None], dict(fl_x=8.0, fl_y=8.0, cx=4.0, cy=4.0, w=8, h=8), 1.0, [0.0, 0.0, 0.0])
    got_cam = coverage_ref.cam_at(cs, 0, 8, 8, dataset=True)
    assert np.array_equal(got_cam.c2w, cam.c2w) and (got_cam.fx, got_cam.fy, got_cam.cx, got_cam.cy) == (8, 8, 4, 4)
    with ctx.mesh_from_arrays(tri, [[0, 1, 2]]) as m, ctx.coverage(pts, cs, None, 8, 8, depth_tol=0.0, occluder=m, want_depth=True) as cov:
        got = np.unpackbits(cov.bits(0).view(np.uint8), bitorder="little")[:5].astype(bool)
        # in front of the mesh; exactly on it; behind it; a pixel that holds no triangle; outside the image
        assert got.tolist() == [True, True, False, True, False]
        assert float(cov.depth[0, 2, 2]) == 2.0 and float(cov.depth[0, 7, 7]) == 0.0
    cs.close()


# ---- 6. errors
def test_every_error_path_is_e_invalid_with_a_message(ctx, oracle, cams, meshes):
    v, t = meshes["hand_made"]
    pts = sphere(np.random.default_rng(1), 100, 0.2)
    lib, tt = ctx.lib, ctx.torch

    def invalid(call, text):
        with pytest.raises(api.PrvError) as e:
            call()
        assert e.value.code == L.PRV_E_INVALID and text in str(e.value), str(e.value)

    bad = t.copy()
    bad[2, 1] = len(v)
    invalid(lambda: ctx.mesh_from_arrays(v, bad), "out of range")
    nan = v.copy()
    nan[3, 2] = np.nan
    invalid(lambda: ctx.mesh_from_arrays(nan, t), "not finite")
    inf = v.copy()
    inf[0, 0] = np.inf
    invalid(lambda: ctx.mesh_from_arrays(inf, t), "not finite")
    h = C.c_void_p()
    assert lib.prv_mesh_from_arrays(ctx.handle, None, 3, api._ptr(t), 1, C.byref(h)) == L.PRV_E_INVALID
    assert "xyz_host is NULL" in lib.prv_last_error(ctx.handle).decode() and not h.value
    assert lib.prv_mesh_from_arrays(ctx.handle, api._ptr(v), len(v), None, 1, C.byref(h)) == L.PRV_E_INVALID
    assert "tri_host is NULL" in lib.prv_last_error(ctx.handle).decode() and not h.value
    assert lib.prv_mesh_from_arrays(ctx.handle, api._ptr(v), (1 << 31) + 1, api._ptr(t), 1, C.byref(h)) == L.PRV_E_INVALID
    assert "2^31" in lib.prv_last_error(ctx.handle).decode()
    tms, scale, offset = util.hemisphere_transforms(oracle, util.fibonacci_hemisphere(3))
    intr = dict(fl_x=60.0, fl_y=58.0, cx=41.0, cy=21.5, w=80, h=45, k1=0.12, k2=-0.05, p1=0.01, p2=-0.008)
    lens = ctx.cameras_from_matrices_intr(tms[[1]], intr, scale, offset)
    with ctx.mesh_from_arrays(v, t) as m:
        invalid(lambda: ctx.mesh_depth(m, lens, None, 16, 16), "lens")
        invalid(lambda: ctx.coverage(pts, lens, None, 16, 16, occluder=m), "lens")
        invalid(lambda: ctx.mesh_depth(m, cams, [0, N_VIEWS], 16, 16), "out of range")
        invalid(lambda: ctx.mesh_depth(m, cams, None, 0, 16), "image size")
        invalid(lambda: ctx.coverage(pts, cams, None, 16, 16, depth_tol=-1.0, occluder=m), "depth_tol")
        host_depth = np.zeros((N_VIEWS, 16, 16), np.float32)
        assert lib.prv_mesh_depth(ctx.handle, m.handle, cams.handle, None, N_VIEWS, 16, 16, api._ptr(host_depth)) == L.PRV_E_INVALID
        assert "depth_out_dev is not a device pointer" in lib.prv_last_error(ctx.handle).decode()
        assert lib.prv_mesh_depth(ctx.handle, m.handle, cams.handle, None, N_VIEWS, 16, 16, None) == L.PRV_E_INVALID
        assert "depth_out_dev is NULL" in lib.prv_last_error(ctx.handle).decode()
        o, dev = L.CoverageOpts(1, 0.02), tt.from_numpy(pts).to(ctx.device)
        for xyz, depth, text in ((api._ptr(pts), None, "xyz_dev is not a device pointer"), (None, None, "xyz_dev is NULL"),
                                 (api._ptr(dev), api._ptr(host_depth), "depth_out_dev is not a device pointer")):
            rc = lib.prv_coverage_create_occluded(ctx.handle, xyz, len(pts), m.handle, cams.handle, None, N_VIEWS, 16, 16, C.byref(o), depth, C.byref(h))
            assert rc == L.PRV_E_INVALID and text in lib.prv_last_error(ctx.handle).decode() and not h.value
        rc = lib.prv_coverage_create_occluded(ctx.handle, api._ptr(dev), len(pts), None, cams.handle, None, N_VIEWS, 16, 16, C.byref(o), None, C.byref(h))
        assert rc == L.PRV_E_INVALID and "occluder is NULL" in lib.prv_last_error(ctx.handle).decode() and not h.value
        depth = tt.empty((N_VIEWS, 16, 16), dtype=tt.float32, device=ctx.device)
        assert lib.prv_mesh_depth(ctx.handle, None, cams.handle, None, N_VIEWS, 16, 16, api._ptr(depth)) == L.PRV_E_INVALID
        assert "mesh is NULL" in lib.prv_last_error(ctx.handle).decode()
        assert ctx.mesh_depth(m, cams, None, 16, 16).shape == (N_VIEWS, 16, 16)  # the mesh is as good as before
    lens.close()


# ---- 7, 8. empty inputs
def test_an_empty_mesh_and_an_empty_cloud_are_not_errors(ctx, cams, meshes):
    pts = sphere(np.random.default_rng(1), 1000, 0.2)
    ids = list(range(N_VIEWS))
    for v, t in ((np.zeros((0, 3), np.float32), np.zeros((0, 3), np.uint32)), (meshes["hand_made"][0], np.zeros((0, 3), np.uint32))):
        with ctx.mesh_from_arrays(v, t) as m:
            assert m.counts() == (len(v), 0)
            assert not ctx.mesh_depth(m, cams, ids, 33, 17).any()
            want = np.stack([ref.visible(c, pts, np.full((17, 33), ref.NEVER, np.uint32), 33, 17, 0.02) for c in cam_list(cams, ids, 33, 17)])
            with ctx.coverage(pts, cams, ids, 33, 17, occluder=m, want_depth=True) as cov:
                assert cov.visible().tolist() == want.sum(axis=1).tolist() and want.sum() > 0  # every in-image point
                assert all(np.array_equal(cov.bits(j), coverage_ref.pack(want[j])) for j in ids) and not cov.depth.any()
    with ctx.mesh_from_arrays(*meshes["hand_made"]) as m, ctx.coverage(np.zeros((0, 3), np.float32), cams, ids, 33, 17, occluder=m, want_depth=True) as cov:
        assert cov.info() == dict(n_points=0, n_views=N_VIEWS, n_coverable=0) and cov.visible().tolist() == [0] * N_VIEWS
        assert cov.depth.cpu().numpy().tobytes() == want_depth(cams, meshes, "hand_made", 8, (33, 17)).tobytes()
        assert cov.greedy(2)[1].tolist() == [0, 0]


# ---- 9. lifetimes
def test_a_mesh_or_handle_that_outlives_its_context_is_inert(oracle, meshes):
    tms, scale, offset = util.hemisphere_transforms(oracle, util.fibonacci_hemisphere(3))
    c = api.Context(0)
    cs = c.cameras_from_matrices(tms, util.FOV_X, 80, 45, scale, offset)
    m = c.mesh_from_arrays(*meshes["hand_made"])
    cov = c.coverage(sphere(np.random.default_rng(1), 100, 0.2), cs, None, 16, 16, occluder=m)
    assert cov.info()["n_views"] == 3
    other = api.Context(0)
    cs2 = other.cameras_from_matrices(tms, util.FOV_X, 80, 45, scale, offset)
    with pytest.raises(api.PrvError) as e:  # a mesh of another context
        other.mesh_depth(m, cs2, None, 16, 16)
    assert e.value.code == L.PRV_E_INVALID and "another context" in str(e.value)
    cs.close()
    c.close()
    for call in (cov.info, cov.visible, lambda: cov.greedy(1), m.counts, lambda: m.filter(keep_largest=1), lambda: m.sample(10)):
        with pytest.raises(api.PrvError) as e:
            call()
        assert e.value.code == L.PRV_E_STATE and "destroyed" in str(e.value)
    depth = other.torch.empty((3, 16, 16), dtype=other.torch.float32, device=other.device)
    assert other.lib.prv_mesh_depth(other.handle, m.handle, cs2.handle, None, 3, 16, 16, api._ptr(depth)) == L.PRV_E_STATE
    cov.close()
    m.close()
    cs2.close()
    other.close()


# ---- 10. an ordinary mesh
def test_a_mesh_from_arrays_round_trips_labels_and_filters(ctx, tmp_path):
    a, b = box_mesh([0.1, 0.1, 0.1], [0.3, 0.3, 0.3]), box_mesh([0.6, 0.6, 0.6], [0.7, 0.7, 0.7])
    v = np.concatenate([a[0], b[0], [[0.9, 0.9, 0.9]]]).astype(np.float32)  # two boxes and a vertex no triangle uses
    t = np.concatenate([a[1], b[1] + 8, a[1][:0]]).astype(np.uint32)
    with ctx.mesh_from_arrays(v, t) as m:
        assert m.counts() == (17, 24)
        assert m.vertices.tobytes() == v.tobytes() and m.triangles.tobytes() == t.tobytes()
        assert not m.normals.any() and not m.colors.any()
        comp = m.components()
        assert comp["n_vertices"].tolist() == [8, 8, 1] and comp["n_triangles"].tolist() == [12, 12, 0]
        assert comp["vertex_component"].tolist() == [0] * 8 + [1] * 8 + [2] and comp["triangle_component"].tolist() == [0] * 12 + [1] * 12
        assert np.array_equal(comp["lo"][0], v[:8].min(axis=0)) and np.array_equal(comp["hi"][1], v[8:16].max(axis=0))
        with m.filter(min_triangles=1, min_diagonal=0.2) as f:  # the small box's diagonal is 0.17
            assert f.counts() == (8, 12) and f.vertices.tobytes() == v[:8].tobytes() and f.triangles.tobytes() == t[:12].tobytes()
        s = m.sample(2000, seed=3).cpu().numpy()
        in_a = ((s >= 0.1 - 1e-6) & (s <= 0.3 + 1e-6)).all(axis=1)
        in_b = ((s >= 0.6 - 1e-6) & (s <= 0.7 + 1e-6)).all(axis=1)
        assert (in_a | in_b).all() and 0.7 < in_a.mean() < 0.9  # area-weighted: 4 : 1
        m.save(tmp_path / "m.ply", 1.0, (0.0, 0.0, 0.0))
        assert (tmp_path / "m.ply").stat().st_size > 17 * 27 + 24 * 13


# ---- 11. the planner
SOURCE = ("train_steps: 20\ntrain_rays: 1024\ntrain_width: 64\ntrain_height: 36\nground_truth_seed: 4242\n"
          "geometry_mc_res: 64\ngeometry_samples: 5000")


def run_planner(pre, extra):
    exe = os.path.join(ROOT, "nerf_prv_amd", "prv_planner")
    pre.mkdir()
    cfg = pre / "cfg.yaml"
    text = YAML.format(pre=pre, vs=os.path.join(GOLD, "hemisphere"), method=0, model_source=SOURCE + extra)
    cfg.write_text(text.replace("num_of_max_iteration: 3", "num_of_max_iteration: 2"))
    out = subprocess.run([exe, str(cfg)], input="21\nobjA\n-1\n", text=True, capture_output=True, timeout=300)
    return out, pre / "Compare" / "ShapeNet" / "objA_m0_v1_t0"


def coverage_files(save):
    return sorted((save / "metrics").glob("*_coverage.txt"), key=lambda p: int(p.name.split("_")[0]))


def test_planner_with_the_mesh_occluder_writes_the_line_and_the_counts_of_the_python_path(tmp_path):
    out, save = run_planner(tmp_path / "mesh", "\nevaluate_coverage: 1\ncoverage_occluder: mesh")
    assert out.returncode == 0, out.stdout + out.stderr
    files = coverage_files(save)
    assert [p.name for p in files] == ["0_coverage.txt", "1_coverage.txt", "2_coverage.txt"]
    rows = []
    for p in files:
        lines = p.read_text().splitlines()
        assert lines[-1] == "occluder\tmesh" and [l.split("\t")[0] for l in lines[:-1]] == ["n_points", "n_coverable", "n_views", "covered", "coverage",
                                                                                             "greedy_covered", "efficiency"]
        rows.append({l.split("\t")[0]: l.split("\t")[1] for l in lines[:-1]})
    # the same inputs through Python: the ground-truth field, its mesh at the planner's resolution, the planner's samples (seed 1)
    # and the view space's cameras; a Testbed with scale 1 and offset 0 takes dataset points that are a cycle of the engine's
    all_json = [p for p in (tmp_path / "mesh").rglob("*_coverage.json")]
    assert len(all_json) == 1
    order = [int((save / "movement" / f"{i}.txt").read_text().split()[0]) for i in (-1, 0, 1)]  # the first view, then each iteration's choice
    tb = api.Testbed(0)
    tb.scale, tb.offset = 1.0, [0.0, 0.0, 0.0]
    c = tb.ctx
    c.synthetic_model(6, api.field_desc(**dict(util.SMALL, density_bias=3.0, table_amp=4.0, per_level_scale=0.0)), 4242)  # the planner's field_* keys
    cs = c.cameras_from_json(str(all_json[0]))
    m = c.marching_cubes(6, 64, colors=False)
    pts = m.sample(5000, seed=1).cpu().numpy()
    n_sets = [int(r["n_views"]) for r in rows]
    assert n_sets == [1, 2, 3]
    for r in rows:  # iteration it is judged on the first view and the choices of the iterations before it
        k = int(r["n_views"])
        ids = order[:k]
        res = tb.compute_coverage(pts[:, [2, 0, 1]], cs, ids, occluder=m)
        print(k, ids, r, res)
        assert res["n_points"] == int(r["n_points"]) == 5000 and res["n_coverable"] == int(r["n_coverable"])
        assert res["covered"][-1] == int(r["covered"]) and res["greedy_covered"][-1] == int(r["greedy_covered"])
    m.close()
    cs.close()
    c.close()


def test_planner_without_the_key_writes_the_point_path_s_bytes_and_refuses_a_cloud_with_the_mesh(tmp_path):
    pts = sphere(np.random.default_rng(4), 20000, 0.035, centre=(0.0, 0.0, 0.0))
    pcd = tmp_path / "ref.pcd"
    head = ("# .PCD v0.7 - Point Cloud Data file format\nVERSION 0.7\nFIELDS x y z rgb\nSIZE 4 4 4 4\nTYPE F F F U\nCOUNT 1 1 1 1\n"
            f"WIDTH {len(pts)}\nHEIGHT 1\nVIEWPOINT 0 0 0 1 0 0 0\nPOINTS {len(pts)}\nDATA ascii\n")
    pcd.write_text(head + "".join(f"{x:.9g} {y:.9g} {z:.9g} 8421504\n" for x, y, z in pts))
    keys = f"\nevaluate_coverage: 1\ncoverage_point_size: 2\ngeometry_reference: \"{pcd}\""  # the existing planner test's configuration
    a, save_a = run_planner(tmp_path / "absent", keys)
    b, save_b = run_planner(tmp_path / "points", keys + "\ncoverage_occluder: points")
    assert a.returncode == 0 and b.returncode == 0, a.stderr + b.stderr
    fa, fb = coverage_files(save_a), coverage_files(save_b)
    assert len(fa) == 3 and [p.read_bytes() for p in fa] == [p.read_bytes() for p in fb]
    assert all(b"occluder" not in p.read_bytes() and len(p.read_text().splitlines()) == 7 for p in fa)
    bad, save = run_planner(tmp_path / "bad", keys + "\ncoverage_occluder: mesh")
    assert bad.returncode != 0 and "coverage_occluder: mesh needs the ground-truth field's mesh" in bad.stderr and "nothing was trained" in bad.stderr
    assert not (save / "metrics").exists()
    bad, save = run_planner(tmp_path / "worse", "\nevaluate_coverage: 1\ncoverage_occluder: triangles")
    assert bad.returncode != 0 and "coverage_occluder must be points or mesh" in bad.stderr and not (save / "metrics").exists()
