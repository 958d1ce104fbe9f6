"""Depth rendering (prv_render_depth, render_planes_kernel in kRenderDepth mode) on the GPU: parity with the CPU restatement of the oracle's march
(tests/depth_ref.py), bit-identity of its colour with prv_render, a known answer independent of the oracle, invariance under
the render policies, errors, and the run.py surfaces (Testbed render_mode = Depth, the server's --screenshot_depth)."""
import ctypes as C
import json
import math
import os

import numpy as np
import pytest

from nerf_prv_amd import api
from tests import depth_ref, march_ref, util

pytestmark = pytest.mark.gpu

SLOT = 50  # slots of this file: 50.. (test_gpu_mesh.py uses 40+)
W, H = 24, 20


@pytest.fixture(scope="module", params=["F4", "F2"])
def field(request, ctx, oracle):
    kw = util.SMALL if request.param == "F4" else util.SMALL_F2
    f = oracle.OracleField(oracle.desc(**kw), seed=util.SEED_A)
    ctx.synthetic_model(SLOT, api.field_desc(**kw), util.SEED_A)
    yield f
    f.close()


@pytest.fixture(scope="module")
def cams(ctx, oracle):
    tms, scale, offset = util.hemisphere_transforms(oracle, util.fibonacci_hemisphere(6))
    tms = tms[[0, 3]]
    cs = ctx.cameras_from_matrices(tms, util.FOV_X, W, H, scale, offset)
    return cs, oracle.cameras_from_transforms(tms, util.FOV_X, W, H, scale, offset)


_both, _check_identity, _ref = depth_ref.both, depth_ref.check_identity, depth_ref.reference


CONFIGS = [(128, 1, 1e-4, 0), (37, 1, 1e-4, 0), (64, 2, 1e-4, 0), (0, 1, 1e-4, 1)]


@pytest.mark.parametrize("S,spp,min_T,mode", CONFIGS, ids=["S128", "S37", "S64spp2", "ngp"])
def test_depth_parity_and_identity(ctx, oracle, field, cams, S, spp, min_T, mode):
    cs, ocams = cams
    opts = api.render_opts(W, H, S if mode == 0 else 0, spp, min_T, step_mode=mode)
    rgba, depth, st, plain, st0 = _both(ctx, SLOT, cs, opts)
    _check_identity(rgba, st, plain, st0)
    assert depth.shape == (len(ocams), H, W) and depth.dtype == np.float32
    for v, oc in enumerate(ocams):
        want = _ref(oracle, field, oc, W, H, S, spp, min_T, mode)
        got = np.concatenate([rgba[v], depth[v][..., None]], axis=-1)
        util.assert_pixels_close(got, want)
        assert np.array_equal(depth[v] == 0, want[..., 4] == 0)  # misses and dead rays: exactly 0
    assert (depth > 0).any()


def test_depth_engine_rule_default_termination(ctx, oracle, field, cams):
    """min_T 0.01 (run.py:304): a ray may stop a sample either side of the threshold -- (r, g, b, a, z) together must match
    one of the termination variants"""
    cs, ocams = cams
    opts = api.engine_render_opts(W, H, 0, 1, 0.01)
    rgba, depth, st, plain, st0 = _both(ctx, SLOT, cs, opts)
    _check_identity(rgba, st, plain, st0)
    for v, oc in enumerate(ocams):
        wants = [_ref(oracle, field, oc, W, H, 0, 1, mt, 1) for mt in util.termination_variants(0.01)]
        got = np.concatenate([rgba[v], depth[v][..., None]], axis=-1)
        util.assert_pixels_close_any(got, wants)


def test_depth_lens_camera(ctx, oracle, field):
    from tests.test_gpu_parity import REF_INTR

    tms, scale, offset = util.hemisphere_transforms(oracle, util.fibonacci_hemisphere(4))
    cs = ctx.cameras_from_matrices_intr(tms[[1]], REF_INTR, scale, offset)
    w, h = 32, 18
    oc = oracle.cameras_from_dataset(tms[[1]], REF_INTR, scale, offset, w, h)[0]
    for S, mode in ((64, 0), (0, 1)):
        opts = api.render_opts(w, h, S, 1, 1e-4, step_mode=mode)
        rgba, depth, st, plain, st0 = _both(ctx, SLOT, cs, opts)
        _check_identity(rgba, st, plain, st0)
        want = _ref(oracle, field, oc, w, h, S, 1, 1e-4, mode)
        util.assert_pixels_close(np.concatenate([rgba[0], depth[0][..., None]], axis=-1), want)
        assert (depth[0] > 0).any()
    cs.close()


def _slab_model(ctx, slot):
    """zero table and MLP, density_bias 20: alpha = 1 at the first occupied sample; occupied = the cells below z = 0.5"""
    desc = api.field_desc(**dict(util.SMALL, density_bias=20.0))
    nt, nm, no = api.model_sizes(desc)
    R = desc.occ_res
    occ = np.zeros(no, np.uint32)
    occ[: (R * R * (R // 2)) // 32] = 0xFFFFFFFF  # bit x + R (y + R z) for z < R / 2
    ctx.load_model(slot, desc, np.zeros(nt, np.uint16), np.zeros(nm, np.uint16), occ)


def _top_camera(ctx, w, h):
    # engine c2w = [[1, 0, 0, .5], [0, -1, 0, .5], [0, 0, -1, 2]]: above the cube, looking along -z (scale 1, offset 0)
    tm = np.array([[[0, 0, 1, 2], [1, 0, 0, 0.5], [0, 1, 0, 0.5], [0, 0, 0, 1]]], np.float64)
    return ctx.cameras_from_matrices(tm, math.radians(60.0), w, h, 1.0, [0.0, 0.0, 0.0])


@pytest.mark.parametrize("mode", [0, 1], ids=["fixed_s", "ngp"])
def test_depth_known_answer_slab(ctx, mode):
    slot, w, h, S = SLOT + 2, 40, 40, 128
    _slab_model(ctx, slot)
    cs = _top_camera(ctx, w, h)
    c2w, _ = cs.get(0)
    assert np.array_equal(c2w, np.array([[1, 0, 0, 0.5], [0, -1, 0, 0.5], [0, 0, -1, 2]], np.float32))
    opts = api.render_opts(w, h, S if mode == 0 else 0, 1, 1e-4, step_mode=mode)
    rgba, depth, _ = ctx.render_depth(slot, cs, None, opts)
    rgba, z = rgba.cpu().numpy()[0], depth.cpu().numpy()[0]
    o, d, t = ctx.debug_raygen(cs, 0, w, h, 0)
    o, d, t = o.astype(np.float64), d.astype(np.float64), t.astype(np.float64)
    s = (0.5 - o[:, 2]) / d[:, 2]  # where the ray crosses the plane z = 0.5
    x, y = o[:, 0] + s * d[:, 0], o[:, 1] + s * d[:, 1]
    cos = -d[:, 2]
    dt = np.where(mode == 1, float(march_ref.NGP_DT), (t[:, 1] - t[:, 0]) / S)
    m = 0.02  # clear of the slab's edges by more than a step
    inside = ((x > m) & (x < 1 - m) & (y > m) & (y < 1 - m)).reshape(h, w)
    outside = ((x < -m) | (x > 1 + m) | (y < -m) | (y > 1 + m)).reshape(h, w)
    assert inside.sum() > 100 and outside.sum() > 100
    bound = (dt * cos).reshape(h, w) + 1e-5
    assert (rgba[..., 3][inside] == 1.0).all()
    assert (np.abs(z - 1.5)[inside] <= bound[inside]).all(), np.abs(z - 1.5)[inside].max()
    assert (z[outside] == 0).all() and (rgba[..., 3][outside] == 0).all()
    cs.close()


def _policy_scene(ctx, oracle, slot, kw=util.SMALL):
    ctx.synthetic_model(slot, api.field_desc(**kw), util.SEED_B)
    tms, scale, offset = util.hemisphere_transforms(oracle, util.fibonacci_hemisphere(6))
    return ctx.cameras_from_matrices(tms, util.FOV_X, 96, 80, scale, offset)


POLICY_ENVS = [{"PRV_MERGE_MAX": "0"}, {"PRV_MERGE_MAX": "6", "PRV_POOL": "1"}, {"PRV_MERGE_MAX": "31", "PRV_POOL": "0"},
               {"PRV_MERGE_MAX": "31", "PRV_POOL": "1"}, {"PRV_CELL_CACHE": "1"}, {"PRV_BLOCKS_PER_CU": "1"}, {"PRV_QUEUE_MB": "1"}]
_env_id = lambda e: ",".join(f"{k}={v}" for k, v in e.items())


def _check_policy_invariance(ctx, oracle, monkeypatch, env, kw, instance):
    no_pair = "PRV_NO_PAIR" in env
    for mode in (1, 0):
        opts = api.render_opts(96, 80, 0 if mode else 128, 1, 1e-4, step_mode=mode)
        cs = _policy_scene(ctx, oracle, SLOT + 3, kw)
        assert ctx.model_layout(SLOT + 3)["kernel_dense_levels"] == instance
        want_rgba, want_z, _ = ctx.render_depth(SLOT + 3, cs, None, opts)
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        c2 = api.Context(0)
        try:
            cs2 = _policy_scene(c2, oracle, 0, kw)
            assert c2.model_layout(0)["kernel_dense_levels"] == (0 if no_pair else instance)
            rgba, z, _ = c2.render_depth(0, cs2, None, opts)
            assert np.array_equal(rgba.cpu().numpy().view(np.uint32), want_rgba.cpu().numpy().view(np.uint32))
            assert np.array_equal(z.cpu().numpy().view(np.uint32), want_z.cpu().numpy().view(np.uint32))
            assert (want_z.cpu().numpy() > 0).any()
            cs2.close()
        finally:
            c2.close()
        for k in env:
            monkeypatch.delenv(k)
        # a subset of the views equals those views of the full render
        rgba, z, _ = ctx.render_depth(SLOT + 3, cs, [4, 1], opts)
        assert np.array_equal(z.cpu().numpy(), want_z.cpu().numpy()[[4, 1]])
        assert np.array_equal(rgba.cpu().numpy(), want_rgba.cpu().numpy()[[4, 1]])
        cs.close()


@pytest.mark.parametrize("env", POLICY_ENVS, ids=_env_id)
def test_depth_policy_invariance(ctx, oracle, monkeypatch, env):
    """util.SMALL: the generic instance <4,0>"""
    _check_policy_invariance(ctx, oracle, monkeypatch, env, util.SMALL, 0)


@pytest.mark.parametrize("env", POLICY_ENVS + [{"PRV_NO_PAIR": "1"}], ids=_env_id)
@pytest.mark.parametrize("which", ["F4_5", "F2_10"])
def test_depth_policy_invariance_on_the_fast_instances(ctx, oracle, monkeypatch, env, which):
    """the same on <4,5> and <2,10> (tests/instances.py), the instances the product's fields run, and the generic gather
    (PRV_NO_PAIR=1: <F,0>) against them: identical bits"""
    from tests import instances

    e = instances.MATRIX[which]
    _check_policy_invariance(ctx, oracle, monkeypatch, env, e.kw, e.instance)


def test_depth_spp_reduce_and_views(ctx, oracle, field, cams):
    """spp 4 with a subset of views, against the same views of the full render and the reference"""
    cs, ocams = cams
    opts = api.render_opts(W, H, 64, 4, 1e-4)
    rgba, z, st = ctx.render_depth(SLOT, cs, [1], opts)
    full_rgba, full_z, _ = ctx.render_depth(SLOT, cs, None, opts)
    assert np.array_equal(z.cpu().numpy()[0], full_z.cpu().numpy()[1])
    want = _ref(oracle, field, ocams[1], W, H, 64, 4, 1e-4, 0)
    util.assert_pixels_close(np.concatenate([rgba.cpu().numpy()[0], z.cpu().numpy()[0][..., None]], axis=-1), want)


def test_depth_errors(ctx, cams):
    cs, _ = cams
    lib = ctx.lib
    ctx.synthetic_model(SLOT + 5, api.field_desc(**util.SMALL), util.SEED_A)
    opts = api.render_opts(W, H, 64, 1, 1e-4)
    ids = np.array([0], np.int32)
    rgba = ctx.torch.empty((1, H, W, 4), dtype=ctx.torch.float32, device=ctx.device)
    z = ctx.torch.empty((1, H, W), dtype=ctx.torch.float32, device=ctx.device)

    def call(slot, ids_, n, out, outz):
        return lib.prv_render_depth(ctx.handle, slot, cs.handle, api._ptr(ids_), n, C.byref(opts), api._ptr(out), api._ptr(outz), None)

    def plain(slot, ids_, n, out):
        return lib.prv_render(ctx.handle, slot, cs.handle, api._ptr(ids_), n, C.byref(opts), api._ptr(out), None)

    assert call(SLOT + 5, ids, 1, rgba, None) == api.L.PRV_E_INVALID  # no depth output
    assert call(SLOT + 5, ids, 1, None, z) == 0  # no colour output: rendered into scratch
    assert call(SLOT + 5, ids, 0, None, None) == 0  # nothing to render
    assert call(SLOT + 9, ids, 1, rgba, z) == plain(SLOT + 9, ids, 1, rgba) != 0  # empty slot
    assert call(-1, ids, 1, rgba, z) == api.L.PRV_E_INVALID
    bad = np.array([99], np.int32)
    assert call(SLOT + 5, bad, 1, rgba, z) == plain(SLOT + 5, bad, 1, rgba) == api.L.PRV_E_INVALID
    host_z, host_rgba = np.zeros((1, H, W), np.float32), np.zeros((1, H, W, 4), np.float32)
    assert call(SLOT + 5, ids, 1, rgba, host_z) == api.L.PRV_E_INVALID
    assert call(SLOT + 5, ids, 1, host_rgba, z) == api.L.PRV_E_INVALID
    assert not host_z.any() and not host_rgba.any()
    # the context is usable afterwards
    r, d, _ = ctx.render_depth(SLOT + 5, cs, None, opts)
    assert (d.cpu().numpy() > 0).any()


def test_testbed_depth_mode(ctx, oracle, tmp_path):
    tb = api.Testbed(0)
    try:
        tb.synthetic_model(api.field_desc(**util.SMALL), util.SEED_A)
        assert tb.render_mode == api.RenderMode.Shade
        tms, scale, offset = util.hemisphere_transforms(oracle, util.fibonacci_hemisphere(6))
        tb.scale, tb.offset = scale, list(offset)
        tb.fov = math.degrees(util.FOV_X)
        tb.set_nerf_camera_matrix(tms[2][:-1, :])
        w, h = 48, 32
        shade = tb.render(w, h, 1, True)
        tb.render_mode = api.Depth
        img = tb.render(w, h, 1, True)
        assert img.shape == (h, w, 4) and img.dtype == np.float32
        cams = tb.ctx.cameras_from_matrices(tms[[2]], util.FOV_X, w, h, scale, offset)
        opts = api.engine_render_opts(w, h, 0, 1, tb.nerf.render_min_transmittance)
        rgba, z, _ = tb.ctx.render_depth(0, cams, None, opts, want_stats=False)
        rgba, z = rgba.cpu().numpy()[0], z.cpu().numpy()[0]
        for c in range(3):
            assert np.array_equal(img[..., c], z)
        assert np.array_equal(img[..., 3], rgba[..., 3])
        assert (z > 0).any() and not np.array_equal(img, shade)
        cams.close()
        # a training view: the dataset's own camera (intrinsics + lens)
        from tests.test_gpu_parity import REF_INTR

        k = REF_INTR
        meta = dict(fl_x=k["fl_x"], fl_y=k["fl_y"], cx=k["cx"], cy=k["cy"], w=64, h=36, k1=k["k1"], k2=k["k2"], p1=k["p1"], p2=k["p2"],
                    camera_angle_x=2 * math.atan(0.5 * 64 / k["fl_x"]), scale=scale, offset=list(offset), aabb_scale=1,
                    frames=[{"file_path": f"v{i}.png", "transform_matrix": tms[i].tolist()} for i in (1, 4)])
        meta["fl_x"], meta["fl_y"], meta["cx"], meta["cy"] = k["fl_x"] * 0.05, k["fl_y"] * 0.05, k["cx"] * 0.05, k["cy"] * 0.05
        path = tmp_path / "scene.json"
        path.write_text(json.dumps(meta))
        tb.load_training_data(str(path))
        tb.set_camera_to_training_view(1)
        img = tb.render(64, 36, 1, True)
        rgba, z, _ = tb.ctx.render_depth(0, tb._dataset_cams, [1], api.engine_render_opts(64, 36, 0, 1, tb.nerf.render_min_transmittance))
        rgba, z = rgba.cpu().numpy()[0], z.cpu().numpy()[0]
        assert np.array_equal(img[..., 0], z) and np.array_equal(img[..., 2], z) and np.array_equal(img[..., 3], rgba[..., 3])
        assert (z > 0).any()
        tb.render_ground_truth = True
        with pytest.raises(NotImplementedError):
            tb.render(64, 36, 1, True)
    finally:
        tb.ctx.close()


def test_server_screenshot_depth(ctx, oracle, tmp_path):
    from PIL import Image

    from nerf_prv_amd import compat_server

    tms, scale, offset = util.hemisphere_transforms(oracle, util.fibonacci_hemisphere(6))
    w, h = 40, 30
    shots = {"camera_angle_x": util.FOV_X, "w": w, "h": h, "scale": scale, "offset": list(offset),
             "frames": [{"file_path": f"./images/view_{i}", "transform_matrix": tms[i].tolist()} for i in (0, 2, 5)]}
    sj = tmp_path / "shots.json"
    sj.write_text(json.dumps(shots))
    out = tmp_path / "shots"
    cmd = f"python run.py --n_steps 0 --screenshot_transforms {sj} --screenshot_dir {out} --screenshot_depth"
    (tmp_path / "run_with_c++.py").write_text("import os\nos.system('" + cmd + "')\n")
    (tmp_path / "ready_c++.txt").write_text("")

    def load_model(sc, cx):
        cx.synthetic_model(SLOT + 6, api.field_desc(**util.SMALL), util.SEED_B)
        return SLOT + 6

    srv = compat_server.CompatServer(str(tmp_path), ctx, load_model, screenshot_spp=2)
    assert srv.poll_once()
    assert sorted(os.listdir(out)) == ["view_0.png", "view_2.png", "view_5.png"]
    cams = ctx.cameras_from_json(str(sj))
    _, z, _ = ctx.render_depth(SLOT + 6, cams, None, api.engine_render_opts(w, h, 0, 2, 0.01, background=(0.0, 0.0, 0.0, 1.0)))
    z = z.cpu().numpy()
    for i, name in enumerate(["view_0.png", "view_2.png", "view_5.png"]):
        got = Image.open(str(out / name))
        assert got.mode == "I;16"
        ref = tmp_path / "ref.png"
        api.write_image_depth(str(ref), z[i], scale)
        assert np.array_equal(np.asarray(got), np.asarray(Image.open(str(ref))))
    assert (z > 0).any()
    cams.close()
