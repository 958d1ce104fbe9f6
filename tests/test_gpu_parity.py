"""GPU parity tests proper: the HIP path (through the C ABI) against the CPU oracle on
the same seeded inputs.  Bars: bit-exact for rays, sample positions (via counts), grid
features (fp16 bit patterns), bytes and rankings; 1e-3 for MLP outputs and pixels (the
tolerance BASELINE.json's north_star states), written at each assert."""
import numpy as np
import pytest

from nerf_prv_amd import api
from tests import util

pytestmark = pytest.mark.gpu

RTOL = 1e-3  # north_star: "within 1e-3 relative"
PIX_ATOL = 1e-3  # pixels live in [0,1]: relative to full scale


@pytest.fixture(scope="module", params=["F4", "F2"])
def fields(request, ctx, oracle):
    kw = util.SMALL if request.param == "F4" else util.SMALL_F2
    d_o, d_p = oracle.desc(**kw), api.field_desc(**kw)
    f = oracle.OracleField(d_o, seed=util.SEED_A)
    ctx.synthetic_model(0, d_p, util.SEED_A)
    return d_o, d_p, f


@pytest.fixture(scope="module")
def cams(ctx, oracle):
    pts = util.fibonacci_hemisphere(6)
    tms, scale, offset = util.hemisphere_transforms(oracle, pts)
    w = h = 40
    cs = ctx.cameras_from_matrices(tms, util.FOV_X, w, h, scale, offset)
    ocams = oracle.cameras_from_transforms(tms, util.FOV_X, w, h, scale, offset)
    return cs, ocams, w, h


def test_synthetic_model_bit_exact(ctx, fields):
    d_o, d_p, f = fields
    t, m, o = ctx.export_model(0, d_p)
    to, mo, oo = f.params()
    assert np.array_equal(t, to) and np.array_equal(m, mo) and np.array_equal(o, oo)


def test_model_load_roundtrip(ctx, fields):
    d_o, d_p, f = fields
    ctx.load_model(1, d_p, *f.params())
    t, m, o = ctx.export_model(1, d_p)
    to, mo, oo = f.params()
    assert np.array_equal(t, to) and np.array_equal(m, mo) and np.array_equal(o, oo)


def test_camera_conversion_and_rays_bit_exact(ctx, oracle, cams):
    cs, ocams, w, h = cams
    for v in range(len(ocams)):
        c2w, intr = cs.get(v)
        assert np.array_equal(c2w.reshape(12), np.frombuffer(ocams[v].c2w, np.float32))
        o, d, t = ctx.debug_raygen(cs, v, w, h, 0)
        oo, od, ot = oracle.raygen(ocams[v], w, h, 0)
        assert np.array_equal(o, oo) and np.array_equal(d, od)
        assert np.array_equal(t, ot)  # inf == inf for misses
    o, d, t = ctx.debug_raygen(cs, 1, w, h, 3)  # jittered sub-sample
    oo, od, ot = oracle.raygen(ocams[1], w, h, 3)
    assert np.array_equal(o, oo) and np.array_equal(d, od) and np.array_equal(t, ot)


def test_hash_grid_features_bit_exact(ctx, fields):
    d_o, d_p, f = fields
    rng = np.random.default_rng(1)
    pos = rng.random((4096, 3), dtype=np.float32)
    pos[:8] = [[0, 0, 0], [1, 1, 1], [1, 0, 0], [0, 1, 0], [0, 0, 1], [0.5, 0.5, 0.5], [1, 1, 0], [-0.1, 1.2, 0.3]]
    got = ctx.debug_encode(0, pos)
    want = f.encode(pos)
    assert np.array_equal(got, want)  # fp16 bit patterns


def test_field_eval(ctx, fields):
    d_o, d_p, f = fields
    rng = np.random.default_rng(2)
    pos = rng.random((2048, 3), dtype=np.float32)
    dirs = rng.standard_normal((2048, 3)).astype(np.float32)
    dirs /= np.linalg.norm(dirs, axis=1, keepdims=True)
    got, gocc = ctx.debug_field(0, pos, dirs)
    want, wocc = f.eval(pos, dirs)
    assert np.array_equal(gocc, wocc)
    # raw MLP outputs: fp16 operands, fp32 accumulate on MFMA vs wide accumulate in the oracle
    np.testing.assert_allclose(got[:, 4:20], want[:, 4:20], rtol=RTOL, atol=2e-3)
    np.testing.assert_allclose(got[:, 20:23], want[:, 20:23], rtol=RTOL, atol=2e-3)
    np.testing.assert_allclose(got[:, 0], want[:, 0], rtol=3e-3)  # sigma = exp(logit): d(sigma)/sigma = d(logit)
    np.testing.assert_allclose(got[:, 1:4], want[:, 1:4], rtol=RTOL, atol=1e-4)


@pytest.mark.parametrize("S,spp", [(128, 1), (37, 1), (64, 2)])
def test_render_pixels_and_sample_counts(ctx, oracle, fields, cams, S, spp):
    d_o, d_p, f = fields
    cs, ocams, w, h = cams
    opts = api.render_opts(w, h, S, spp, 1e-4)
    img, st = ctx.render(0, cs, None, opts)
    img = img.cpu().numpy()
    n_eval = 0
    for v, oc in enumerate(ocams):
        want, ne = f.render(oc, w, h, S, spp, 1e-4)
        n_eval += ne
        err = np.abs(img[v] - want)
        assert err.max() <= PIX_ATOL, (v, err.max())
        assert (err <= RTOL * np.maximum(np.abs(want), 1e-1)).all()
    # identical occupancy-skip decisions; early termination compares T against min_T after a hardware
    # exp, so a ray may stop one sample earlier or later than the oracle when T lands within 1e-6 of it
    assert abs(int(st.samples_evaluated) - n_eval) <= max(2, n_eval // 100000)
    assert st.rays == len(ocams) * w * h * spp and st.samples_nominal == st.rays * S


def test_march_rejection_on_awkward_cameras(ctx, oracle, fields):
    """the march pass rejects rays with a reciprocal-only slab test against the occupied cells' (grown) bounding box
    before the exact set-up (prv_kernels.hip, march_compact_kernel): it may only ever err towards "hit".  Cameras that
    stress it: inside the object, exactly axis-aligned rays (zero direction components: 0 * inf in the slab test),
    300 units away, looking away, and a sweep of sideways offsets whose rays graze the box.  Pixels and the count of
    evaluated samples equal the oracle's, which knows no such test."""
    d_o, d_p, f = fields
    w = h = 33  # odd: the central pixel's ray is exactly the optical axis
    S = 64

    def tm(rot, t):
        m = np.eye(4)
        m[:3, :3] = rot
        m[:3, 3] = t
        return m

    eye, back = np.eye(3), np.diag([-1.0, 1.0, -1.0])
    ry = lambda a: np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]])
    cases = [("inside", tm(eye, [0, 0, 0]), util.FOV_X), ("axis", tm(eye, [0, 0, 0.3]), util.FOV_X), ("away", tm(back, [0, 0, 0.3]), util.FOV_X),
             ("far", tm(eye, [0, 0, 60.0]), 0.02), ("corner", tm(ry(0.6), [0.25, 0.07, 0.28]), 0.5)]
    cases += [(f"graze{i}", tm(eye, [0.04 * i, 0.02 * i, 0.3]), 0.6) for i in range(1, 8)]
    scale, offset = 5.0, np.array([0.5, 0.5, 0.5])
    live_views = 0
    for name, m, fov in cases:
        cs = ctx.cameras_from_matrices(m[None], fov, w, h, scale, offset)
        oc = oracle.cameras_from_transforms(m[None], fov, w, h, scale, offset)[0]
        img, st = ctx.render(0, cs, None, api.render_opts(w, h, S, 1, 1e-4))
        want, ne = f.render(oc, w, h, S, 1, 1e-4)
        util.assert_pixels_close(img[0].cpu().numpy(), want)
        assert abs(int(st.samples_evaluated) - ne) <= 2, (name, int(st.samples_evaluated), ne)
        live_views += ne > 0
        cs.close()
    assert live_views >= 6  # most of these views do see the object; "away" sees nothing


REF_INTR = {"fl_x": 915.60668945312500, "fl_y": 913.32666015625, "cx": 647.14532470703125, "cy": 372.51531982421875,
            "w": 1280, "h": 720, "k1": 0.12042199820280075, "k2": -0.21373499929904938, "p1": -0.0021210000850260258,
            "p2": 7.5e-4}


def test_dataset_cameras_lens_rays_bit_exact(ctx, oracle):
    """the dataset's own intrinsics (run.py:238-247: off-centre principal point, fl_y, OpenCV lens solved by 8
    Newton steps): rays bit-identical to the oracle at the json size and at a rescaled size; the golden rays
    of the independent numpy restatement reproduced on the device"""
    import json
    import os

    pts = util.fibonacci_hemisphere(3)
    tms, scale, offset = util.hemisphere_transforms(oracle, pts)
    cs = ctx.cameras_from_matrices_intr(tms, REF_INTR, scale, offset)
    assert cs.size == (1280, 720)
    np.testing.assert_array_equal(cs.lens(1), np.array([REF_INTR[k] for k in ("k1", "k2", "p1", "p2")], np.float32))
    import ctypes as C

    for (w, h) in ((160, 90), (100, 40)):
        ocams = oracle.cameras_from_dataset(tms, REF_INTR, scale, offset, w, h)
        for v in (0, 2):
            o, d, t = ctx.debug_raygen(cs, v, w, h, 0)
            oo, od, ot = oracle.raygen(ocams[v], w, h, 0)
            assert np.array_equal(o, oo) and np.array_equal(d, od) and np.array_equal(t, ot)
    # full size: 300 seeded pixels of one view, sub-sample 5
    w, h = 1280, 720
    ocam = oracle.cameras_from_dataset(tms, REF_INTR, scale, offset)[1]
    o, d, t = ctx.debug_raygen(cs, 1, w, h, 5)
    ox, oy = C.c_float(), C.c_float()
    oracle.lib().orc_spp_offset(5, C.byref(ox), C.byref(oy))
    rng = np.random.default_rng(11)
    for px, py in zip(rng.integers(0, w, 300), rng.integers(0, h, 300)):
        oo, od = np.zeros(3, np.float32), np.zeros(3, np.float32)
        oracle.lib().orc_raygen(C.byref(ocam), int(px), int(py), ox, oy, oracle._p(oo), oracle._p(od))
        i = int(py) * w + int(px)
        assert np.array_equal(o[i], oo) and np.array_equal(d[i], od), (px, py)
    # the golden rays of the numpy restatement: transform_matrix chosen so that the engine-frame camera IS the
    # fixture's c2w (rows cycle (y,z,x), columns 1,2 negate; scale 1, offset 0)
    with open(os.path.join(os.path.dirname(__file__), "golden", "golden_lens.json")) as f:
        g = json.load(f)
    k = dict(g["intr"], **dict(zip(("k1", "k2", "p1", "p2"), g["lens_rays"])))
    R = np.asarray(g["c2w"], np.float64).reshape(3, 4)
    tm = np.eye(4)
    for src, dst in ((2, 0), (0, 1), (1, 2)):
        tm[dst, :3] = R[src, :3] * [1, -1, -1]
        tm[dst, 3] = R[src, 3]
    one = ctx.cameras_from_matrices_intr(tm[None], k, 1.0, [0.0, 0.0, 0.0])
    c2w_dev, _ = one.get(0)
    assert np.array_equal(c2w_dev, R.astype(np.float32))
    o, d, _ = ctx.debug_raygen(one, 0, 1280, 720, 0)
    for r in g["rays"]:
        i = r["py"] * 1280 + r["px"]
        np.testing.assert_array_equal(o[i].astype(np.float64), r["o"])
        np.testing.assert_array_equal(d[i].astype(np.float64), r["d"])


def test_dataset_cameras_render_parity(ctx, oracle, fields):
    """pixels through the lens path against the oracle, 1e-3 (north_star)"""
    d_o, d_p, f = fields
    pts = util.fibonacci_hemisphere(4)
    tms, scale, offset = util.hemisphere_transforms(oracle, pts)
    cs = ctx.cameras_from_matrices_intr(tms, REF_INTR, scale, offset)
    w, h = 64, 36
    ocams = oracle.cameras_from_dataset(tms, REF_INTR, scale, offset, w, h)
    img, st = ctx.render(0, cs, None, api.render_opts(w, h, 64, 1, 1e-4))
    img = img.cpu().numpy()
    n_eval = 0
    for v, oc in enumerate(ocams):
        want, ne = f.render(oc, w, h, 64, 1, 1e-4)
        n_eval += ne
        assert np.abs(img[v] - want).max() <= PIX_ATOL
    assert abs(int(st.samples_evaluated) - n_eval) <= 2 and n_eval > 0
    # and the lens matters: the pinhole set of the same poses renders different pixels
    pin = ctx.cameras_from_matrices(tms, 2 * np.arctan(0.5 * 1280 / REF_INTR["fl_x"]), 1280, 720, scale, offset)
    img_pin, _ = ctx.render(0, pin, None, api.render_opts(w, h, 64, 1, 1e-4))
    assert float((img_pin.cpu().numpy() - img).__abs__().max()) > 0.05


def test_dataset_json_loader(ctx, oracle, tmp_path):
    """prv_cameras_from_dataset_json reads the intrinsics block the planner writes (main.cpp:1585-1602) by key,
    with the documented fall-backs; prv_cameras_from_json keeps the screenshot rule (fov at the centre)"""
    import json

    pts = util.fibonacci_hemisphere(2)
    tms, scale, offset = util.hemisphere_transforms(oracle, pts)
    k = REF_INTR
    root = {"camera_angle_x": 2 * np.arctan(0.5 * k["w"] / k["fl_x"]), "camera_angle_y": 2 * np.arctan(0.5 * k["h"] / k["fl_y"]),
            "fl_x": k["fl_x"], "fl_y": k["fl_y"], "k1": k["k1"], "k2": k["k2"], "k3": 0.005386, "p1": k["p1"], "p2": k["p2"],
            "cx": k["cx"], "cy": k["cy"], "w": k["w"], "h": k["h"], "aabb_scale": 1, "scale": scale, "offset": list(offset),
            "frames": [{"file_path": f"2/rgbaClip_{i}.png", "transform_matrix": np.asarray(tm).tolist()} for i, tm in enumerate(tms)]}
    path = tmp_path / "2.json"
    path.write_text(json.dumps(root))
    ds = ctx.cameras_from_dataset_json(path)
    ref = ctx.cameras_from_matrices_intr(tms, k, scale, offset)
    for v in range(2):
        for a, b in zip(ds.get(v), ref.get(v)):
            assert np.array_equal(a, b)
        assert np.array_equal(ds.lens(v), ref.lens(v))
    _, intr = ds.get(0)
    np.testing.assert_array_equal(intr, np.array([k["fl_x"], k["fl_y"], k["cx"], k["cy"]], np.float32))
    shot = ctx.cameras_from_json(path)  # screenshot rule: camera_angle_x, centre, no lens
    _, intr_s = shot.get(0)
    assert intr_s[2] == 640.0 and intr_s[3] == 360.0 and intr_s[0] == intr_s[1] and not shot.lens(0).any()
    # fall-backs: no fl_*/cx/cy/lens keys -> camera_angle_*, image centre, pinhole
    for key in ("fl_x", "fl_y", "cx", "cy", "k1", "k2", "p1", "p2"):
        root.pop(key)
    path.write_text(json.dumps(root))
    fb = ctx.cameras_from_dataset_json(path)
    _, intr_f = fb.get(1)
    np.testing.assert_allclose(intr_f, [k["fl_x"], k["fl_y"], 640.0, 360.0], rtol=1e-6)
    assert not fb.lens(1).any()
    root.pop("camera_angle_x"), root.pop("camera_angle_y")
    path.write_text(json.dumps(root))
    with pytest.raises(api.PrvError):
        ctx.cameras_from_dataset_json(path)
    with pytest.raises(api.PrvError):
        ctx.cameras_from_matrices_intr(tms, dict(k, fl_x=float("nan")), scale, offset)


def test_render_view_subset_and_order(ctx, fields, cams):
    cs, ocams, w, h = cams
    opts = api.render_opts(w, h, 64, 1, 1e-4)
    full, _ = ctx.render(0, cs, None, opts)
    sub, _ = ctx.render(0, cs, [4, 1], opts)
    assert bool((sub[0] == full[4]).all()) and bool((sub[1] == full[1]).all())
    again, _ = ctx.render(0, cs, None, opts)
    assert bool((again == full).all())  # run-to-run bit reproducible


def test_rgba8_bytes(ctx, oracle, fields, cams):
    cs, ocams, w, h = cams
    opts = api.render_opts(w, h, 64, 1, 1e-4, background=(0, 0, 0, 1))
    u8, _ = ctx.render_rgba8(0, cs, None, opts)
    f32, _ = ctx.render(0, cs, None, opts)
    # the byte rule itself is exact on identical float inputs
    want = oracle.quantize_rgba8(f32.cpu().numpy(), (0, 0, 0, 1))
    got = u8.cpu().numpy()
    diff = np.abs(got.astype(int) - want.astype(int))
    assert diff.max() <= 1 and (diff != 0).mean() < 1e-4  # powf ulp at a rounding boundary only
    # ... and "at a rounding boundary" is checked: a byte that differs has its float64 value within the band that
    # tests/image_ref.py derives for a float32 evaluation, and the device's bytes are the float64 bytes outside that band
    from tests import image_ref
    q = image_ref.quantize_exact(f32.cpu().numpy(), (0, 0, 0, 1))
    assert q.in_band[diff != 0].all()
    assert q.in_band[got != q.byte].all() and np.abs(got.astype(int) - q.byte.astype(int)).max() <= 1
    q = ctx.quantize_rgba8(f32, (0, 0, 0, 1)).cpu().numpy()
    assert np.array_equal(q, got)


@pytest.mark.parametrize("method,E", [(2, 2), (3, 5), (2, 3)])
def test_ensemble_scores_from_bytes(ctx, oracle, method, E):
    import torch

    rng = np.random.default_rng(method * 10 + E)
    n_views, npix = 5, 45 * 80  # the reference's candidate size (main.cpp:1805-1806)
    base = rng.integers(0, 256, (n_views, npix, 4), dtype=np.uint8)
    imgs = []
    for e in range(E):
        noise = rng.integers(-3, 4, base.shape)
        noise[rng.random(base.shape) < 0.5] = 0  # many zero-variance channels (the 1e-10 gate)
        imgs.append(np.clip(base.astype(int) + noise, 0, 255).astype(np.uint8))
    dev = [torch.from_numpy(i).cuda() for i in imgs]
    rec = ctx.score_ensemble_images(method, dev)
    fn = oracle.score_ensemble_rgb if method == 2 else oracle.score_ensemble_rgbdensity
    want = np.array([fn([i[v] for i in imgs]) for v in range(n_views)])
    # the device adds the per-pixel addends in the reference loop's order, one sequential double sum per view:
    # EnsembleRGBDensity is bit-identical; EnsembleRGB adds logs, where the two log implementations may differ
    # in the last bit of an addend
    if method == 3:
        assert np.array_equal(rec["score"], want)
    else:
        np.testing.assert_allclose(rec["score"], want, rtol=1e-13)
    ids = np.arange(n_views)
    assert np.array_equal(ctx.rank(rec, ids), oracle.rank(want, ids))
    assert ctx.argmax(rec, ids) == oracle.argmax(want, ids)
    # a duplicated view ties exactly and the lower id wins (strict '>' of main.cpp:2088)
    dup = [torch.cat([d, d[:1]]) for d in dev]
    rec2 = ctx.score_ensemble_images(method, dup)
    assert rec2["score"][0] == rec2["score"][n_views]
    order = list(ctx.rank(rec2, np.arange(n_views + 1)))
    assert order.index(0) + 1 == order.index(n_views)


def test_score_views_psnr_and_ranking(ctx, oracle, fields, cams):
    d_o, d_p, f = fields
    cs, ocams, w, h = cams
    ctx.synthetic_model(2, d_p, util.SEED_B)
    fb = oracle.OracleField(d_o, seed=util.SEED_B)
    opts = api.render_opts(w, h, 64, 1, 1e-4)
    gt, _ = ctx.render(2, cs, None, opts)
    rec, st = ctx.score_views(api.L.SCORE_PSNR_COVERAGE, [0], cs, None, opts, gt=gt, want_stats=True)
    want = []
    for oc in ocams:
        a, _ = f.render(oc, w, h, 64, 1, 1e-4)
        b, _ = fb.render(oc, w, h, 64, 1, 1e-4)
        want.append(oracle.score_view(a, b))  # (score, psnr, coverage), coverage weight 1
    want = np.array(want)
    np.testing.assert_allclose(rec["psnr"], want[:, 1], rtol=RTOL)
    np.testing.assert_allclose(rec["coverage"], want[:, 2], rtol=RTOL)
    np.testing.assert_allclose(rec["score"], want[:, 0], rtol=RTOL)
    ids = np.arange(len(ocams))
    assert np.array_equal(ctx.rank(rec, ids), oracle.rank(want[:, 0], ids))  # integer ranking exact
    # the documented weight: 0 ranks by PSNR alone, w adds w * mean((1 - alpha)^2) (main.cpp:2148's density term)
    ctx.set_coverage_weight(0.0)
    rec0, _ = ctx.score_views(api.L.SCORE_PSNR_COVERAGE, [0], cs, None, opts, gt=gt)
    ctx.set_coverage_weight(2.5)
    rec25, _ = ctx.score_views(api.L.SCORE_PSNR_COVERAGE, [0], cs, None, opts, gt=gt)
    ctx.set_coverage_weight(1.0)
    np.testing.assert_allclose(rec0["score"], -want[:, 1], rtol=RTOL)
    np.testing.assert_allclose(rec25["score"] - rec0["score"], 2.5 * (rec["score"] - rec0["score"]), rtol=1e-9, atol=1e-12)


@pytest.mark.parametrize("method,E", [(2, 2), (3, 5)])
def test_score_views_ensemble_and_ranking(ctx, oracle, fields, cams, method, E):
    d_o, d_p, f = fields
    cs, ocams, w, h = cams
    members = []
    for e in range(E):
        ctx.synthetic_model(3 + e, d_p, 1000 + e)
        members.append(oracle.OracleField(d_o, seed=1000 + e))
    bg = (0, 0, 0, 0)  # alpha carries opacity (the intent of main.cpp:2126-2127)
    opts = api.render_opts(w, h, 64, 1, 1e-4, background=bg)
    rec, _ = ctx.score_views(method, list(range(3, 3 + E)), cs, None, opts)
    want = []
    for oc in ocams:
        imgs = [oracle.quantize_rgba8(m.render(oc, w, h, 64, 1, 1e-4)[0], bg) for m in members]
        want.append((oracle.score_ensemble_rgb if method == 2 else oracle.score_ensemble_rgbdensity)(imgs))
    want = np.array(want)
    np.testing.assert_allclose(rec["score"], want, rtol=RTOL)
    ids = np.arange(len(ocams))
    assert np.array_equal(ctx.rank(rec, ids), oracle.rank(want, ids))


def test_first_hit_ray_cast_bit_exact(ctx, oracle, fields, cams):
    """a13: GPU twin of the reference's CPU ray-caster, integer voxel ids must match exactly"""
    d_o, d_p, f = fields
    cs, ocams, w, h = cams
    got = ctx.first_hit(0, cs, None, w, h).cpu().numpy()
    for v, oc in enumerate(ocams):
        want = oracle.first_hit_image(f, oc, w, h)
        assert np.array_equal(got[v], want)
        assert (want >= 0).sum() > 50 and (want < 0).sum() > 50  # both hits and misses are exercised
    near = ctx.first_hit(0, cs, [0], w, h, max_range=1.2).cpu().numpy()[0]  # main.cpp:258 passes a max range
    want = oracle.first_hit_image(f, ocams[0], w, h, max_range=1.2)
    assert np.array_equal(near, want) and (near >= 0).sum() < (got[0] >= 0).sum()


def test_precept_per_voxel_ray_cast_with_realsense_model(ctx, oracle, fields):
    """a13 + a14: the reference's CPU render path in full (main.cpp:98-284): every ground-truth voxel is
    projected through the inverse Brown-Conrady RealSense model of DefaultConfiguration.yaml, culled,
    snapped to an integer pixel, deprojected and ray-cast.  Integer voxel ids must match exactly."""
    import torch

    d_o, d_p, f = fields
    _, _, occ = f.params()
    R = d_o.occ_res
    bits = np.unpackbits(occ.view(np.uint8), bitorder="little")[: R ** 3]
    idx = np.nonzero(bits)[0]  # the "ground-truth leaves": centres of the occupied cells
    vox = np.stack([(idx % R + 0.5) / R, (idx // R % R + 0.5) / R, (idx // (R * R) + 0.5) / R], axis=1).astype(np.float32)
    # a camera 1.5 cube units from the centre, +Z looking at it, slightly rolled
    eye = np.array([0.5 + 1.2, 0.5 - 0.6, 0.5 + 0.7])
    z = (np.array([0.5, 0.5, 0.5]) - eye) / np.linalg.norm(np.array([0.5, 0.5, 0.5]) - eye)
    x = np.cross(z, [0.1, 0.2, 1.0]); x /= np.linalg.norm(x)
    y = np.cross(z, x)
    c2w = np.eye(4)
    c2w[:3, 0], c2w[:3, 1], c2w[:3, 2], c2w[:3, 3] = x, y, z, eye
    intr = api.L.Rs2Intrinsics(width=1280, height=720, ppx=647.14532470703125, ppy=372.51531982421875,
                               fx=915.60668945312500, fy=913.32666015625000, model=2)
    for i, v in enumerate([1.2042199820280075e-01, -2.1373499929904938e-01, 5.3860000334680080e-03,
                           -2.1210000850260258e-03, 0.0]):  # yaml color_k1,k2,k3,p1,p2 -> coeffs[0..4]
        intr.coeffs[i] = v
    got = ctx.precept(0, torch.from_numpy(vox).cuda(), c2w, intr, max_range=3.0).cpu().numpy()
    k9 = np.array([intr.ppx, intr.ppy, intr.fx, intr.fy] + list(intr.coeffs), np.float32)
    want = oracle.precept(f, vox, c2w, k9, 1280, 720, 2, 3.0)
    assert np.array_equal(got, want)
    hit = want >= 0
    assert hit.sum() > 100  # most leaves project into the image and are hit
    # a hit is never behind the voxel that generated the ray: the first occupied cell is at most as far
    cells = np.stack([want[hit] % R, want[hit] // R % R, want[hit] // (R * R)], axis=1)
    d_hit = np.linalg.norm((cells + 0.5) / R - eye, axis=1)
    d_vox = np.linalg.norm(vox[hit] - eye, axis=1)
    assert (d_hit <= d_vox + 2.0 * np.sqrt(3) / R).all()
    short = ctx.precept(0, torch.from_numpy(vox).cuda(), c2w, intr, max_range=1.0).cpu().numpy()  # main.cpp:258
    assert np.array_equal(short, oracle.precept(f, vox, c2w, k9, 1280, 720, 2, 1.0)) and (short >= 0).sum() < hit.sum()


def test_error_behaviour(ctx, fields, cams):
    cs, ocams, w, h = cams
    with pytest.raises(api.PrvError) as e:
        ctx.render(api.L.MAX_SLOTS, cs, None, api.render_opts(w, h))  # slot out of range (PRV_MAX_SLOTS)
    assert e.value.code == api.L.PRV_E_INVALID
    fresh = api.Context(0)
    cs2 = fresh.cameras_from_matrices(np.eye(4)[None], util.FOV_X, w, h, 1.0, [0.5, 0.5, 0.5])
    with pytest.raises(api.PrvError) as e:
        fresh.render(0, cs2, None, api.render_opts(w, h))  # empty slot
    assert e.value.code == api.L.PRV_E_STATE
    cs2.close()
    fresh.close()
    with pytest.raises(api.PrvError):
        ctx.render(0, cs, None, api.render_opts(w, h, samples_per_ray=129))
    with pytest.raises(api.PrvError):
        ctx.render(0, cs, [99], api.render_opts(w, h))
    with pytest.raises(api.PrvError):
        ctx.cameras_from_json("/nonexistent/transforms.json")
    img, st = ctx.render(0, cs, [], api.render_opts(w, h))  # empty view list is fine
    assert img.shape[0] == 0 and st.rays == 0
    # the runtime can not be shut down under a live context (and this process shares it with torch: never call it here)
    assert ctx.lib.prv_runtime_shutdown() == api.L.PRV_E_STATE
    assert b"still alive" in ctx.lib.prv_last_error(None)


def test_ground_truth_splats_byte_exact(ctx, oracle):
    """prv_splat_points (the rgbaClip images of get_coverage, main.cpp:1604-1618) against the oracle: a coloured
    sphere-shell cloud seen by lens cameras, 5-pixel points (yaml:18) -- identical bytes"""
    rng = np.random.default_rng(3)
    n = 20000
    d = rng.normal(size=(n, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    xyz = (0.04 * d + 1e-10).astype(np.float32)  # a 4 cm sphere at the origin, world units
    rgb = rng.integers(0, 256, size=(n, 3), dtype=np.uint8)
    rgb[:50] = 255  # some exactly-white points
    pts = util.fibonacci_hemisphere(3)
    tms, scale, offset = util.hemisphere_transforms(oracle, pts)
    cs = ctx.cameras_from_matrices_intr(tms, REF_INTR, scale, offset)
    for (w, h, size) in ((160, 90, 5), (64, 36, 1)):
        ocams = oracle.cameras_from_dataset(tms, REF_INTR, scale, offset, w, h)
        got = ctx.splat_points(xyz, rgb, scale, offset, cs, None, w, h, point_size=size).cpu().numpy()
        assert got.shape == (3, h, w, 4)
        for v in range(3):
            want = oracle.splat_points(xyz, rgb, scale, offset, ocams[v], w, h, point_size=size)
            assert np.array_equal(got[v], want), v
        cover = (got[..., 3] == 255).mean()
        assert 0.005 < cover < 0.6
    one = ctx.splat_points(xyz, rgb, scale, offset, cs, [2], 160, 90, 5, flip180=False).cpu().numpy()[0]
    assert np.array_equal(one[::-1, ::-1], got_last := ctx.splat_points(xyz, rgb, scale, offset, cs, [2], 160, 90, 5).cpu().numpy()[0])
    empty = ctx.splat_points(np.zeros((0, 3), np.float32), np.zeros((0, 3), np.uint8), scale, offset, cs, [0], 32, 18).cpu().numpy()
    assert (empty == np.array([255, 255, 255, 0], np.uint8)).all()
    with pytest.raises(api.PrvError):
        ctx.splat_points(xyz, rgb, scale, offset, cs, [0], 32, 18, point_size=0)
    del got_last


def test_host_pointers_are_refused_not_dereferenced(ctx, fields, cams):
    """a host buffer where the ABI wants device memory is an error code (PRV_E_INVALID), not a GPU page fault"""
    import ctypes as C

    cs, ocams, w, h = cams
    opts = api.render_opts(w, h, 16, 1, 1e-4)
    ids = np.arange(1, dtype=np.int32)
    host_out = np.zeros((1, h, w, 4), np.float32)
    rc = ctx.lib.prv_render(ctx.handle, 0, cs.handle, ids.ctypes.data_as(C.c_void_p), 1, C.byref(opts),
                            host_out.ctypes.data_as(C.c_void_p), None)
    assert rc == api.L.PRV_E_INVALID and b"device pointer" in ctx.lib.prv_last_error(ctx.handle)
    host_u8 = np.zeros((1, h, w, 4), np.uint8)
    rc = ctx.lib.prv_render_rgba8(ctx.handle, 0, cs.handle, ids.ctypes.data_as(C.c_void_p), 1, C.byref(opts),
                                  host_u8.ctypes.data_as(C.c_void_p), None)
    assert rc == api.L.PRV_E_INVALID
    img, _ = ctx.render(0, cs, [0], opts)  # the context is still healthy
    assert img.shape == (1, h, w, 4)
