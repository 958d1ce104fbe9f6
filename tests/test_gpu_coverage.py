"""Surface coverage on the GPU, through the C ABI (api.py): the visibility bit matrix, the per-view counts and the depth buffers
(coverage_depth_kernel, coverage_visible_kernel) equal the float32 restatement of tests/coverage_ref.py bit for bit; the depth
buffers cover the pixels the point splat fills; curve, first_seen and greedy (coverage_gain_kernel, coverage_mark_kernel) equal
the exact-integer restatement; batches of views, the error paths, a handle that outlives its context, an empty cloud; and
prv_planner with `evaluate_coverage: 1`.  No tolerance anywhere: every comparison is of bytes or integers."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from nerf_prv_amd import _lib as L
from nerf_prv_amd import api
from tests import coverage_ref as ref
from tests import util
from tests.test_gpu_planner import GOLD, ROOT, YAML

pytestmark = pytest.mark.gpu

SLOT = 48  # a slot of its own: the session context is shared with the other GPU modules
N_VIEWS = 8
CENTRE = np.array([0.5, 0.5, 0.5], np.float32)  # where the hemisphere's cameras look (engine frame), 1.5 away


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


@pytest.fixture(scope="module")
def clouds(ctx, cams):
    """the point families, engine frame: name -> (n, 3) float32"""
    rng = np.random.default_rng(11)
    ctx.synthetic_model(SLOT, api.field_desc(**util.SMALL), util.SEED_A)
    thr = float(np.median(ctx.density_grid(SLOT, 48).cpu().numpy()))
    m = ctx.marching_cubes(SLOT, 48, threshold=thr, colors=False)
    mesh = m.sample(20011, seed=5).cpu().numpy()
    m.close()
    c2w = cams.get(0)[0]
    eye, right = c2w[:, 3], c2w[:, 0]
    ball = sphere(rng, 4097, 0.3)
    bad = mesh[:4097].copy()
    bad[::7, 0] = np.nan
    bad[1::7, 1] = np.inf
    bad[2::7, 2] = -np.inf
    bad[3::7] = np.float32(3e38)
    bad[4::7, 1] = np.float32(-3e38)
    return {
        "mesh": mesh,
        "nested_spheres": np.concatenate([sphere(rng, 16000, 0.3), sphere(rng, 4011, 0.15)]),
        "behind_view_0": (eye + (eye - ball)).astype(np.float32),  # the ball mirrored through camera 0
        "beside_view_0": (ball + np.float32(4.0) * right).astype(np.float32),  # far off view 0's image, still in front of it
        "wide_box": rng.uniform(-2.0, 3.0, (20011, 3)).astype(np.float32),  # around, beside and behind every camera
        "duplicated": np.repeat(mesh[:5000], 2, axis=0),
        "not_finite": bad,
    }


def cam_list(camset, ids, w, h, dataset=False):
    return [ref.cam_at(camset, v, w, h, dataset) for v in ids]


def assert_matches_reference(ctx, camset, ids, pts, w, h, ps, tol, dataset=False):
    """the handle's bit matrix, counts and depth buffers == the reference's; -> (want_vis, handle)"""
    want_vis, want_depth = ref.matrix(cam_list(camset, ids, w, h, dataset), pts, w, h, ps, tol)
    cov = ctx.coverage(pts, camset, ids, w, h, point_size=ps, depth_tol=tol, want_depth=True)
    info = cov.info()
    got_depth = cov.depth.cpu().numpy()
    print(f"n {len(pts)} views {len(ids)} {w}x{h} ps {ps} tol {tol}: visible {cov.visible().tolist()} coverable {info['n_coverable']}; "
          f"depth mismatches {int((got_depth.view(np.uint32) != want_depth.view(np.uint32)).sum())}")
    assert np.array_equal(got_depth.view(np.uint32), want_depth.view(np.uint32))
    for j in range(len(ids)):
        got, want = cov.bits(j), ref.pack(want_vis[j])
        assert got.shape == want.shape == ((len(pts) + 63) // 64,)
        assert np.array_equal(got, want), (j, int((got != want).sum()))
    assert cov.visible().tolist() == want_vis.sum(axis=1).tolist()
    assert info == dict(n_points=len(pts), n_views=len(ids), n_coverable=int(want_vis.any(axis=0).sum()))
    return want_vis, cov


# ---- the bit matrix, visible() and depth: exact
@pytest.mark.parametrize("n", [1, 63, 64, 65, 4097, 20011])
def test_bits_counts_and_depth_equal_the_reference_at_every_word_edge(ctx, cams, clouds, n):
    """the ballot's tail (n % 64 != 0), exactly one word, one word and a bit, several blocks"""
    want, cov = assert_matches_reference(ctx, cams, [0, 3, 6], clouds["mesh"][:n], 33, 17, 2, 0.02)
    assert want.any()
    cov.close()


@pytest.mark.parametrize("n_views,size,ps,tol", [(1, (16, 16), 1, 0.0), (3, (33, 17), 2, 0.02), (8, (80, 45), 5, 0.02), (3, (80, 45), 1, 0.0),
                                                 (8, (16, 16), 5, 0.0), (1, (33, 17), 5, 0.02), (8, (33, 17), 1, 0.02), (3, (16, 16), 2, 0.0)],
                         ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_bits_counts_and_depth_equal_the_reference_over_views_sizes_and_options(ctx, cams, clouds, n_views, size, ps, tol):
    ids = [0, 3, 6][:n_views] if n_views <= 3 else list(range(N_VIEWS))
    want, cov = assert_matches_reference(ctx, cams, ids, clouds["mesh"], size[0], size[1], ps, tol)
    assert want.any() and not want.all()
    cov.close()


@pytest.mark.parametrize("family,n_views,size,ps,tol", [("nested_spheres", 8, (80, 45), 2, 0.02), ("behind_view_0", 1, (33, 17), 2, 0.02),
                                                        ("beside_view_0", 1, (80, 45), 5, 0.02), ("wide_box", 8, (33, 17), 5, 0.0),
                                                        ("duplicated", 3, (80, 45), 1, 0.0), ("not_finite", 3, (33, 17), 2, 0.02)])
def test_point_families_equal_the_reference(ctx, cams, clouds, family, n_views, size, ps, tol):
    pts = clouds[family]
    ids = list(range(n_views))
    want, cov = assert_matches_reference(ctx, cams, ids, pts, size[0], size[1], ps, tol)
    if family == "nested_spheres":  # the inner sphere is wholly hidden, from every view
        assert want[:, :16000].any(axis=0).sum() > 4000 and not want[:, 16000:].any()
    if family in ("behind_view_0", "beside_view_0"):
        assert not want.any() and cov.info()["n_coverable"] == 0 and not cov.depth.any()
    if family == "wide_box":
        assert want.any()
    if family == "duplicated":  # equal depths: both copies or neither
        assert want.any() and np.array_equal(want[:, 0::2], want[:, 1::2])
    if family == "not_finite":
        ordinary = np.isfinite(pts).all(axis=1) & (np.abs(pts) < 1e30).all(axis=1)  # (the 3e38 rows overflow on the way: no claim)
        assert want[:, ordinary].any() and not want[:, ~np.isfinite(pts).all(axis=1)].any()
    cov.close()


def test_a_cloud_far_from_the_origin_equals_the_reference(ctx, oracle, cams, clouds):
    """cameras and cloud moved together to (40.5, -6.5, 3.5): the same code at coordinates with 6 fewer mantissa bits to spare"""
    tms, scale, offset = util.hemisphere_transforms(oracle, util.fibonacci_hemisphere(3))
    far = ctx.cameras_from_matrices(tms, util.FOV_X, 80, 45, scale, offset + np.array([3.0, 40.0, -7.0]))
    # (a dataset offset (o0, o1, o2) moves the engine frame by (o1, o2, o0); view 0 is the pole of either hemisphere)
    assert np.allclose(far.get(0)[0][:, 3] - cams.get(0)[0][:, 3], [40.0, -7.0, 3.0], atol=1e-4)
    pts = (clouds["mesh"] + np.array([40.0, -7.0, 3.0], np.float32)).astype(np.float32)
    want, cov = assert_matches_reference(ctx, far, [0, 1, 2], pts, 80, 45, 2, 0.02)
    assert want.any(axis=0).sum() > 1000
    cov.close()
    far.close()


# ---- a cross-check that needs no reference: the depth buffers cover what the splat fills
def test_depth_is_positive_exactly_where_the_splat_is_opaque(ctx, oracle, cams, clouds):
    pts = clouds["mesh"]
    rgb = np.full((len(pts), 3), 90, np.uint8)  # never white
    dataset_pts = pts[:, [2, 0, 1]]  # e = (q1, q2, q0) with scale 1 and offset 0
    tms, scale, offset = util.hemisphere_transforms(oracle, util.fibonacci_hemisphere(3))
    intr = dict(fl_x=60.0, fl_y=58.0, cx=41.0, cy=21.5, w=80, h=45, k1=0.12, k2=-0.05, p1=0.01, p2=-0.008)
    lens = ctx.cameras_from_matrices_intr(tms[[1]], intr, scale, offset)
    assert np.any(lens.lens(0) != 0)
    for camset, ids, ps in ((cams, [0, 5], 1), (cams, [2, 7], 5), (lens, [0], 2)):
        with ctx.coverage(pts, camset, ids, 80, 45, point_size=ps, want_depth=True) as cov:
            img = ctx.splat_points(dataset_pts, rgb, 1.0, [0.0, 0.0, 0.0], camset, ids, 80, 45, point_size=ps, flip180=False)
            opaque = (img[..., 3] == 255).cpu().numpy()
            filled = (cov.depth > 0).cpu().numpy()
            assert opaque.any() and np.array_equal(filled, opaque)
            assert cov.info()["n_coverable"] > 0
    lens.close()


# ---- curve, first_seen and greedy: exact
def test_curve_first_seen_and_greedy_equal_the_reference(ctx, cams, clouds):
    ids = list(range(N_VIEWS))
    want, cov = assert_matches_reference(ctx, cams, ids, clouds["mesh"], 80, 45, 2, 0.02)
    n_coverable = cov.info()["n_coverable"]
    for order in (ids, ids[::-1], [5, 5, 2, 5, 2, 0], [3]):
        covered, first = cov.curve(order, want_first_seen=True)
        want_covered, want_first = ref.curve(want, order)
        assert covered.tolist() == want_covered and np.array_equal(first.cpu().numpy().view(np.uint32), want_first)
        assert all(a <= b for a, b in zip(want_covered, want_covered[1:]))
    assert cov.curve(ids).tolist()[-1] == n_coverable and cov.curve(ids[::-1]).tolist()[-1] == n_coverable
    assert cov.curve([5, 5, 2]).tolist()[1] == cov.curve([5]).tolist()[0]  # the repeat gains 0
    assert cov.curve([]).tolist() == []
    visible = cov.visible()
    for k in (1, 3, N_VIEWS):
        chosen, covered = cov.greedy(k)
        want_chosen, want_covered = ref.greedy(want, k)
        assert chosen.tolist() == want_chosen and covered.tolist() == want_covered
        assert chosen[0] == int(np.argmax(visible)) and covered[0] == visible.max()
    chosen, covered = cov.greedy(N_VIEWS)
    assert sorted(chosen.tolist()) == ids and covered[-1] == n_coverable
    again = cov.greedy(N_VIEWS)
    assert again[0].tobytes() == chosen.tobytes() and again[1].tobytes() == covered.tobytes()
    a, fa = cov.curve(ids, want_first_seen=True)
    b, fb = cov.curve(ids, want_first_seen=True)
    assert a.tobytes() == b.tobytes() and fa.cpu().numpy().tobytes() == fb.cpu().numpy().tobytes()
    cov.close()


def test_greedy_ties_and_zero_gain_rounds_on_views_that_see_the_same(ctx, cams, clouds):
    """views 1 and 2 of the list are the same camera: they tie, the smaller position wins, and the copy is taken last at gain 0"""
    ids = [4, 0, 0, 4]
    want, cov = assert_matches_reference(ctx, cams, ids, clouds["mesh"][:4097], 33, 17, 2, 0.02)
    chosen, covered = cov.greedy(4)
    assert (chosen.tolist(), covered.tolist()) == ref.greedy(want, 4)
    assert chosen[0] == (0 if want[0].sum() >= want[1].sum() else 1) and sorted(chosen.tolist()[:2]) == [0, 1]
    assert chosen.tolist()[2:] == [2, 3] and covered[1] > covered[0] and covered[2] == covered[1] and covered[3] == covered[1]
    cov.close()


def test_greedy_beats_the_first_four_views_of_the_hemisphere(ctx, oracle):
    """a sphere under the 64-view hemisphere: the first four views in file order crowd the pole, four greedy ones spread out"""
    tms, scale, offset = util.hemisphere_transforms(oracle, util.fibonacci_hemisphere(64))
    cs = ctx.cameras_from_matrices(tms, util.FOV_X, 80, 45, scale, offset)
    pts = sphere(np.random.default_rng(3), 20000, 0.3)
    with ctx.coverage(pts, cs, None, 80, 45, point_size=2) as cov:
        chosen, covered = cov.greedy(4)
        in_order = cov.curve([0, 1, 2, 3])
        print("greedy", chosen.tolist(), covered.tolist(), "file order", in_order.tolist(), "coverable", cov.info()["n_coverable"])
        assert covered[-1] > in_order[-1] and covered[0] >= in_order[0]
    cs.close()


# ---- batches, errors, lifetime, the empty cloud
def test_views_in_several_depth_buffer_batches_give_the_bytes_of_one_batch(ctx, cams, clouds, monkeypatch):
    """33 x 17 x 4 = 2244 bytes per view: a 5000-byte budget takes two views per batch (8 views: four batches; 3 views: 2 + 1), a
    budget of 1 byte one view per batch"""
    pts = clouds["mesh"]
    for ids in (list(range(N_VIEWS)), [6, 1, 3]):
        with ctx.coverage(pts, cams, ids, 33, 17, point_size=2, want_depth=True) as one:
            want_bits = [one.bits(j) for j in range(len(ids))]
            want_depth, want_visible, want_info = one.depth.cpu().numpy(), one.visible(), one.info()
        for budget in ("5000", "1"):
            monkeypatch.setenv("PRV_COVERAGE_ZBUF_BYTES", budget)
            with ctx.coverage(pts, cams, ids, 33, 17, point_size=2, want_depth=True) as cov:
                assert all(np.array_equal(cov.bits(j), want_bits[j]) for j in range(len(ids)))
                assert cov.depth.cpu().numpy().tobytes() == want_depth.tobytes()
                assert cov.visible().tolist() == want_visible.tolist() and cov.info() == want_info
            monkeypatch.delenv("PRV_COVERAGE_ZBUF_BYTES")


def test_every_error_path_is_e_invalid_with_a_message(ctx, cams, clouds):
    pts = clouds["mesh"][:1000]
    t = ctx.torch

    def invalid(call, text):
        with pytest.raises(api.PrvError) as e:
            call()
        assert e.value.code == L.PRV_E_INVALID and text in str(e.value), str(e.value)

    invalid(lambda: ctx.coverage(pts, cams, None, 16, 16, point_size=0), "point_size")
    invalid(lambda: ctx.coverage(pts, cams, None, 16, 16, point_size=65), "point_size")
    invalid(lambda: ctx.coverage(pts, cams, None, 16, 16, depth_tol=-1e-3), "depth_tol")
    invalid(lambda: ctx.coverage(pts, cams, None, 16, 16, depth_tol=float("nan")), "depth_tol")
    invalid(lambda: ctx.coverage(pts, cams, None, 16, 16, depth_tol=float("inf")), "depth_tol")
    invalid(lambda: ctx.coverage(pts, cams, None, 0, 16), "image size")
    invalid(lambda: ctx.coverage(pts, cams, [0, N_VIEWS], 16, 16), "out of range")
    # a host pointer, or NULL, where a device pointer is required
    lib, h, o = ctx.lib, C.c_void_p(), L.CoverageOpts(1, 0.02)
    dev = t.from_numpy(pts).to(ctx.device)
    host_depth = np.zeros((N_VIEWS, 16, 16), np.float32)
    for xyz, depth, text in ((api._ptr(pts), None, "xyz_dev is not a device pointer"), (None, None, "xyz_dev is NULL"),
                             (api._ptr(dev), api._ptr(host_depth), "depth_out_dev is not a device pointer")):
        rc = lib.prv_coverage_create(ctx.handle, xyz, len(pts), cams.handle, None, N_VIEWS, 16, 16, C.byref(o), depth, C.byref(h))
        assert rc == L.PRV_E_INVALID and text in lib.prv_last_error(ctx.handle).decode() and not h.value
    rc = lib.prv_coverage_create(ctx.handle, api._ptr(dev), len(pts), cams.handle, None, N_VIEWS, 16, 16, C.byref(o), None, None)
    assert rc == L.PRV_E_INVALID and "out is NULL" in lib.prv_last_error(ctx.handle).decode()
    with ctx.coverage(pts, cams, None, 16, 16) as cov:
        invalid(lambda: cov.greedy(0), "k must be at least 1")
        invalid(lambda: cov.greedy(-2), "k must be at least 1")
        invalid(lambda: cov.greedy(N_VIEWS + 1), f"k = {N_VIEWS + 1} views asked of {N_VIEWS}")
        invalid(lambda: cov.curve([0, N_VIEWS]), "order[1]")
        invalid(lambda: cov.curve([-1]), "order[0]")
        invalid(lambda: cov.bits(N_VIEWS), "out of range")
        covered, first = np.zeros(1, np.uint64), np.zeros(len(pts), np.uint32)
        order = np.zeros(1, np.int32)
        rc = lib.prv_coverage_curve(cov.handle, api._ptr(order), 1, api._ptr(covered), api._ptr(first))
        assert rc == L.PRV_E_INVALID and "first_seen_dev is not a device pointer" in lib.prv_last_error(ctx.handle).decode()
        assert lib.prv_coverage_greedy(cov.handle, 1, None, None) == L.PRV_E_INVALID
        assert cov.greedy(1)[1][0] == cov.visible().max()  # the handle is as good as before


def test_a_handle_that_outlives_its_context_is_inert(oracle, clouds):
    tms, scale, offset = util.hemisphere_transforms(oracle, util.fibonacci_hemisphere(3))
    c = api.Context(0)
    cs = c.cameras_from_matrices(tms, util.FOV_X, 80, 45, scale, offset)
    cov = c.coverage(clouds["mesh"][:1000], cs, None, 16, 16)
    assert cov.info()["n_views"] == 3
    cs.close()
    c.close()
    for call in (cov.info, cov.visible, lambda: cov.greedy(1), lambda: cov.curve([0])):
        with pytest.raises(api.PrvError) as e:
            call()
        assert e.value.code == L.PRV_E_STATE and "destroyed" in str(e.value)
    words = np.zeros(16, np.uint64)
    assert c.lib.prv_coverage_bits(cov.handle, 0, api._ptr(words)) == L.PRV_E_STATE
    cov.close()


def test_an_empty_cloud_is_not_an_error(ctx, cams):
    with ctx.coverage(np.zeros((0, 3), np.float32), cams, None, 33, 17, want_depth=True) as cov:
        assert cov.info() == dict(n_points=0, n_views=N_VIEWS, n_coverable=0)
        assert cov.visible().tolist() == [0] * N_VIEWS and cov.bits(2).shape == (0,)
        assert not cov.depth.any()
        covered, first = cov.curve([1, 0, 1], want_first_seen=True)
        assert covered.tolist() == [0, 0, 0] and first.shape == (0,)
        chosen, covered = cov.greedy(N_VIEWS)
        assert chosen.tolist() == list(range(N_VIEWS)) and covered.tolist() == [0] * N_VIEWS


# ---- the planner
COVERAGE_SOURCE = ("train_steps: 20\ntrain_rays: 1024\ntrain_width: 64\ntrain_height: 36\nground_truth_seed: 4242\n"
                   "geometry_mc_res: 64\ngeometry_samples: 5000")


def run_planner(pre, extra):
    exe = os.path.join(ROOT, "nerf_prv_amd", "prv_planner")
    pre.mkdir()
    cfg = pre / "cfg.yaml"
    text = YAML.format(pre=pre, vs=os.path.join(GOLD, "hemisphere"), method=0, model_source=COVERAGE_SOURCE + extra)
    cfg.write_text(text.replace("num_of_max_iteration: 3", "num_of_max_iteration: 2"))
    out = subprocess.run([exe, str(cfg)], input="21\nobjA\n-1\n", text=True, capture_output=True, timeout=300)
    return out, pre / "Compare" / "ShapeNet" / "objA_m0_v1_t0"


def read_coverage(path):
    out = {}
    for line in open(path).read().splitlines():
        k, v = line.split("\t")
        out[k] = float(v) if k in ("coverage", "efficiency") else int(v)
    return out


def test_planner_writes_a_coverage_file_per_iteration_and_none_without_the_key(ctx, tmp_path):
    """a two-iteration random loop (method 0: nothing is trained or scored) over the five-view hemisphere; the reference is a
    sphere cloud (an ASCII .pcd in the dataset frame, radius 0.035 around the object's centre): dense enough to hide its far side"""
    pts = sphere(np.random.default_rng(4), 20000, 0.035, centre=(0.0, 0.0, 0.0))
    pcd = tmp_path / "ref.pcd"
    head = ("# .PCD v0.7 - Point Cloud Data file format\nVERSION 0.7\nFIELDS x y z rgb\nSIZE 4 4 4 4\nTYPE F F F U\nCOUNT 1 1 1 1\n"
            f"WIDTH {len(pts)}\nHEIGHT 1\nVIEWPOINT 0 0 0 1 0 0 0\nPOINTS {len(pts)}\nDATA ascii\n")
    pcd.write_text(head + "".join(f"{x:.9g} {y:.9g} {z:.9g} 8421504\n" for x, y, z in pts))
    out, save = run_planner(tmp_path / "on", f"\nevaluate_coverage: 1\ncoverage_point_size: 2\ngeometry_reference: \"{pcd}\"")
    assert out.returncode == 0, out.stdout + out.stderr
    files = sorted((save / "metrics").glob("*_coverage.txt"), key=lambda p: int(p.name.split("_")[0]))
    assert [p.name for p in files] == ["0_coverage.txt", "1_coverage.txt", "2_coverage.txt"]
    rows = [read_coverage(p) for p in files]
    print(rows)
    for it, r in enumerate(rows):
        assert list(r) == ["n_points", "n_coverable", "n_views", "covered", "coverage", "greedy_covered", "efficiency"]
        assert r["n_points"] == 20000 and 0 < r["n_coverable"] <= 20000 and r["n_views"] == it + 1
        assert 0 < r["covered"] <= r["n_coverable"] and r["greedy_covered"] <= r["n_coverable"]
        assert r["coverage"] == r["covered"] / r["n_coverable"] and r["efficiency"] == r["covered"] / r["greedy_covered"]
    assert rows[0]["covered"] <= rows[1]["covered"] <= rows[2]["covered"]
    assert rows[0]["covered"] < rows[0]["n_coverable"] and rows[2]["covered"] > rows[0]["covered"]  # one view does not see it all
    assert rows[0]["covered"] <= rows[0]["greedy_covered"]  # at k = 1 greedy is the best single view
    assert len({(r["n_points"], r["n_coverable"]) for r in rows}) == 1  # one handle for the object
    out, save = run_planner(tmp_path / "off", "")
    assert out.returncode == 0, out.stdout + out.stderr
    assert (save / "metrics").is_dir() and not list(save.rglob("*_coverage*")) and not list((tmp_path / "off").rglob("*_coverage*"))
    out, save = run_planner(tmp_path / "bad", "\nevaluate_coverage: 1\ncoverage_point_size: 99")
    assert out.returncode != 0 and "coverage_point_size must be in [1, 64]" in out.stderr and "nothing was trained" in out.stderr
    assert not (save / "metrics").exists()
