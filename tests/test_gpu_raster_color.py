"""The colour images of a mesh on the GPU, through the C ABI (api.py): prv_mesh_render's three planes (the raster kernels on 64-bit
keys, raster_shade_kernel) equal the restatement of tests/raster_color_ref.py byte for byte on the shapes and meshes of the depth
tests; the depth plane is prv_mesh_depth's; coincident triangles take the lower id's colours; the threshold between the two
paths, the list's capacity, the view batches and the flip change nothing they should not; the alpha rule, an empty mesh, the error
paths and lifetimes; colours set from the host survive filter and save; prv_planner's mode 3 with `gt_surface: mesh` writes
exactly these images.  No tolerance anywhere: every comparison is of bytes or integers."""
import json
import os
import subprocess

import numpy as np
import pytest

from nerf_prv_amd import _lib as L
from nerf_prv_amd import api
from tests import raster_color_ref as ref
from tests import util
from tests.test_gpu_planner import GOLD, ROOT, YAML
from tests.test_gpu_raster import ENV, N_VIEWS, SHAPES, SLOT, cam_list, cams, meshes, view_ids  # noqa: F401 (cams, meshes: fixtures)
from tests.test_raster_host import uv_sphere

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def colored(ctx, meshes):
    """name -> (vertices, triangles, colors (n, 3) uint8): the depth tests' meshes; the marching-cubes ones with the colours the
    field gives them, the hand-made family and the box with a distinct colour per vertex"""
    thr = float(np.median(ctx.density_grid(SLOT, 48).cpu().numpy()))  # (the `meshes` fixture put the field in SLOT)
    out = {}
    for res in (24, 48):
        with ctx.marching_cubes(SLOT, res, threshold=thr, colors=True) as m:
            v, t = meshes[f"mc{res}"]
            assert m.vertices.tobytes() == v.tobytes() and m.triangles.tobytes() == t.tobytes()
            assert len(np.unique(m.colors, axis=0)) > 10
            out[f"mc{res}"] = (v, t, m.colors.copy())
    rng = np.random.default_rng(17)
    for name in ("hand_made", "box"):
        v, t = meshes[name]
        c = rng.permutation(254)[: len(v)]  # distinct per vertex, never white
        out[name] = (v, t, np.stack([c, 253 - c, (c * 7 + 3) % 251], axis=1).astype(np.uint8))
    return out


_want = {}


def want_planes(cams, colored, name, n_views, size):
    """the reference's (rgba, depth, triangle id), computed once per input and shared by the tests that need them"""
    key = (name, n_views, size)
    if key not in _want:
        v, t, c = colored[name]
        _want[key] = ref.render_views(cam_list(cams, view_ids(n_views), *size), v, t, c, *size)
    return _want[key]


def render(ctx, m, cams, ids, size, flip180=False):
    rgba, depth, tri = ctx.mesh_render(m, cams, ids, size[0], size[1], flip180=flip180, want_depth=True, want_triangles=True)
    return rgba.cpu().numpy(), depth.cpu().numpy(), tri.cpu().numpy().view(np.uint32)


# ---- 1, 2. the three planes == the reference's bytes; the depth plane == prv_mesh_depth
@pytest.mark.parametrize("n_views,size", SHAPES, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v))
@pytest.mark.parametrize("name", ["mc24", "mc48", "hand_made", "box"])
def test_mesh_render_equals_the_reference_byte_for_byte(ctx, cams, colored, name, n_views, size):
    v, t, c = colored[name]
    want_rgba, want_depth, want_tri = want_planes(cams, colored, name, n_views, size)
    ids = view_ids(n_views)
    with ctx.mesh_from_arrays(v, t, colors=c) as m:
        assert m.colors.tobytes() == c.tobytes()
        rgba, depth, tri = render(ctx, m, cams, ids, size)
        stats = ctx.raster_stats()
        alone = ctx.mesh_render(m, cams, ids, *size)
        assert alone.dtype == ctx.torch.uint8 and alone.cpu().numpy().tobytes() == rgba.tobytes()  # no planes asked for: the image alone
        depth_call = ctx.mesh_depth(m, cams, ids, *size).cpu().numpy()
    bad = [int((a != b).sum()) for a, b in ((rgba, want_rgba), (depth.view(np.uint32), want_depth.view(np.uint32)), (tri, want_tri))]
    print(f"{name} {len(t)} triangles, {n_views} views {size}: covered {int((want_depth > 0).sum())} of {want_depth.size}, "
          f"mismatching bytes / depths / ids {bad}, {stats}")
    assert rgba.shape == want_rgba.shape == (n_views, size[1], size[0], 4) and depth.shape == want_depth.shape and tri.shape == want_tri.shape
    assert bad == [0, 0, 0]
    assert depth.tobytes() == depth_call.tobytes()  # the depth plane is prv_mesh_depth's, bit for bit
    assert stats["pairs"] == len(t) * n_views
    covered = want_depth > 0
    assert covered.any() and (want_rgba[covered][:, 3] == 255).all() and len(np.unique(want_rgba[covered], axis=0)) > 3
    if name == "box":
        assert stats["large"] > 0 and covered[0].all()  # past all four borders: the large path, and view 0 is filled without corner 0
    if name.startswith("mc"):
        assert (~covered).any() and (want_rgba[~covered] == ref.BACKGROUND).all()


# ---- 3. the tie rule
def test_coincident_triangles_take_the_lower_id_s_colours_in_both_orders(ctx, cams, colored):
    """the hand-made family's first triangle twice, from duplicated vertices: equal depth bits at every pixel, so only the id in
    the key's low word decides; a key without it would leave the colour to the order of the atomics"""
    v = colored["hand_made"][0][:3]
    vv, tt = np.concatenate([v, v]), np.array([[0, 1, 2], [3, 4, 5]], np.uint32)
    red, blue = [[200, 10, 10]] * 3, [[10, 10, 200]] * 3
    cam0 = cam_list(cams, [0], 80, 45)
    for first, second in ((red, blue), (blue, red)):
        c = np.array(first + second, np.uint8)
        want = ref.render_views(cam0, vv, tt, c, 80, 45)
        with ctx.mesh_from_arrays(vv, tt, colors=c) as m:
            rgba, depth, tri = render(ctx, m, cams, [0], (80, 45))
        covered = want[1] > 0
        assert covered.sum() > 50 and (want[2][covered] == 0).all() and (want[0][covered] == tuple(first[0]) + (255,)).all()  # the reference alone
        assert rgba.tobytes() == want[0].tobytes() and depth.tobytes() == want[1].tobytes() and tri.tobytes() == want[2].tobytes()


# ---- 4. invariance
def test_threshold_capacity_batches_and_repetition_change_no_byte_and_the_flip_only_turns_the_image(ctx, cams, colored, monkeypatch):
    for name, n_views, size in (("mc24", 3, (33, 17)), ("hand_made", 8, (80, 45)), ("box", 3, (33, 17))):
        v, t, c = colored[name]
        ids = view_ids(n_views)
        want = want_planes(cams, colored, name, n_views, size)
        tried = [{}, {}, dict(PRV_RASTER_SMALL_PIXELS="0"), dict(PRV_RASTER_SMALL_PIXELS=str(10 ** 9)),
                 dict(PRV_RASTER_LIST_ENTRIES="64" if name == "mc24" else "1", PRV_RASTER_SMALL_PIXELS="1"), dict(PRV_COVERAGE_ZBUF_BYTES="1"),
                 dict(PRV_COVERAGE_ZBUF_BYTES="1", PRV_RASTER_LIST_ENTRIES="64", PRV_RASTER_SMALL_PIXELS="0")]
        large = []
        with ctx.mesh_from_arrays(v, t, colors=c) as m:
            for env in tried:
                for k in ENV:
                    monkeypatch.delenv(k, raising=False)
                for k, val in env.items():
                    monkeypatch.setenv(k, val)
                got = render(ctx, m, cams, ids, size)
                large.append(ctx.raster_stats()["large"])
                assert all(g.tobytes() == w.tobytes() for g, w in zip(got, want)), env
                turned = render(ctx, m, cams, ids, size, flip180=True)
                assert np.array_equal(turned[0], want[0][:, ::-1, ::-1]), env  # reversed on both axes
                assert turned[1].tobytes() == want[1].tobytes() and turned[2].tobytes() == want[2].tobytes(), env  # the planes stay
            for k in ENV:
                monkeypatch.delenv(k, raising=False)
        print(name, "deferred pairs per setting", large)
        assert large[2] >= large[0] >= large[3] == 0 and large[2] > 0  # 0: every pair with a box; huge: none


# ---- 5. the alpha rule; an empty mesh
def test_an_exactly_white_pixel_is_transparent_with_depth_and_id_set_and_an_empty_mesh_is_all_background(ctx, cams, colored):
    v, t, _ = colored["hand_made"]
    white = np.full((len(v), 3), 255, np.uint8)
    ids = view_ids(3)
    with ctx.mesh_from_arrays(v, t, colors=white) as m:
        rgba, depth, tri = render(ctx, m, cams, ids, (33, 17))
    _, want_depth, want_tri = want_planes(cams, colored, "hand_made", 3, (33, 17))
    assert (rgba == ref.BACKGROUND).all()
    assert (want_depth > 0).any() and depth.tobytes() == want_depth.tobytes() and tri.tobytes() == want_tri.tobytes()
    for vv, tt in ((np.zeros((0, 3), np.float32), np.zeros((0, 3), np.uint32)), (v, np.zeros((0, 3), np.uint32))):
        with ctx.mesh_from_arrays(vv, tt, colors=white[: len(vv)]) as m:
            for flip in (False, True):
                rgba, depth, tri = render(ctx, m, cams, ids, (33, 17), flip180=flip)
                assert (rgba == ref.BACKGROUND).all() and not depth.any() and (tri == ref.NO_TRIANGLE).all()
            assert ctx.raster_stats()["pairs"] == 0


# ---- 6. errors, lifetimes, and colours on an ordinary mesh
def test_every_error_path_has_its_code_and_message(ctx, oracle, cams, colored):
    v, t, c = colored["hand_made"]
    lib, tt = ctx.lib, ctx.torch

    def invalid(call, text):
        with pytest.raises(api.PrvError) as e:
            call()
        assert e.value.code == L.PRV_E_INVALID and text in str(e.value), str(e.value)

    tms, scale, offset = util.hemisphere_transforms(oracle, util.fibonacci_hemisphere(3))
    intr = dict(fl_x=60.0, fl_y=58.0, cx=41.0, cy=21.5, w=80, h=45, k1=0.12, k2=-0.05, p1=0.01, p2=-0.008)
    lens = ctx.cameras_from_matrices_intr(tms[[1]], intr, scale, offset)
    with ctx.mesh_from_arrays(v, t) as m:
        invalid(lambda: ctx.mesh_render(m, cams, None, 16, 16), "prv_mesh_set_colors")  # a mesh without colours
        invalid(lambda: m.set_colors(c[:-1]), "colours for a mesh of")
        invalid(lambda: m.set_colors(np.concatenate([c, c])), "colours for a mesh of")
        assert lib.prv_mesh_set_colors(m.handle, None, len(v)) == L.PRV_E_INVALID and "rgb_host is NULL" in lib.prv_last_error(ctx.handle).decode()
        assert not m.colors.any()
        invalid(lambda: ctx.mesh_render(m, cams, None, 16, 16), "prv_mesh_set_colors")  # (a refused set_colors gives it none)
        m.set_colors(c)
        assert m.colors.tobytes() == c.tobytes()
        invalid(lambda: ctx.mesh_render(m, lens, None, 16, 16), "lens")
        invalid(lambda: ctx.mesh_render(m, cams, [0, N_VIEWS], 16, 16), "out of range")
        invalid(lambda: ctx.mesh_render(m, cams, None, 0, 16), "image size")
        dev = dict(rgba=tt.empty((N_VIEWS, 16, 16, 4), dtype=tt.uint8, device=ctx.device), depth=tt.empty((N_VIEWS, 16, 16), dtype=tt.float32, device=ctx.device),
                   tri=tt.empty((N_VIEWS, 16, 16), dtype=tt.int32, device=ctx.device))
        host = dict(rgba=np.zeros((N_VIEWS, 16, 16, 4), np.uint8), depth=np.zeros((N_VIEWS, 16, 16), np.float32), tri=np.zeros((N_VIEWS, 16, 16), np.uint32))
        for which, text in (("rgba", "out_rgba8_dev is not a device pointer"), ("depth", "depth_out_dev is not a device pointer"),
                            ("tri", "tri_out_dev is not a device pointer")):
            args = [api._ptr(host[k] if k == which else dev[k]) for k in ("rgba", "depth", "tri")]
            assert lib.prv_mesh_render(ctx.handle, m.handle, cams.handle, None, N_VIEWS, 16, 16, 0, *args) == L.PRV_E_INVALID
            assert text in lib.prv_last_error(ctx.handle).decode()
        assert lib.prv_mesh_render(ctx.handle, m.handle, cams.handle, None, N_VIEWS, 16, 16, 0, None, None, None) == L.PRV_E_INVALID
        assert "out_rgba8_dev is NULL" in lib.prv_last_error(ctx.handle).decode()
        assert lib.prv_mesh_render(ctx.handle, None, cams.handle, None, N_VIEWS, 16, 16, 0, api._ptr(dev["rgba"]), None, None) == L.PRV_E_INVALID
        assert "mesh is NULL" in lib.prv_last_error(ctx.handle).decode()
        assert ctx.mesh_render(m, cams, None, 16, 16).shape == (N_VIEWS, 16, 16, 4)  # the mesh is as good as before
    lens.close()


def test_a_mesh_of_another_context_is_refused_and_one_that_outlives_its_context_is_inert(oracle, colored):
    v, t, c = colored["hand_made"]
    tms, scale, offset = util.hemisphere_transforms(oracle, util.fibonacci_hemisphere(3))
    first = api.Context(0)
    m = first.mesh_from_arrays(v, t, colors=c)
    other = api.Context(0)
    cs = other.cameras_from_matrices(tms, util.FOV_X, 80, 45, scale, offset)
    with pytest.raises(api.PrvError) as e:
        other.mesh_render(m, cs, None, 16, 16)
    assert e.value.code == L.PRV_E_INVALID and "another context" in str(e.value)
    first.close()
    with pytest.raises(api.PrvError) as e:
        m.set_colors(c)
    assert e.value.code == L.PRV_E_STATE and "destroyed" in str(e.value)
    out = other.torch.empty((3, 16, 16, 4), dtype=other.torch.uint8, device=other.device)
    assert other.lib.prv_mesh_render(other.handle, m.handle, cs.handle, None, 3, 16, 16, 0, api._ptr(out), None, None) == L.PRV_E_STATE
    m.close()
    cs.close()
    other.close()


def test_colours_set_from_the_host_survive_filter_and_save(ctx, colored, tmp_path):
    v, t, c = colored["hand_made"]  # its components: triangles {0, 1, 3} on vertices 0..2, {2} on 3..5, {4, 5} on 6..9, {6} on 10..12
    with ctx.mesh_from_arrays(v, t) as m:
        m.set_colors(c)
        with m.filter(keep_largest=1) as f:
            assert f.counts() == (3, 3) and f.colors.tobytes() == c[:3].tobytes()
        m.save(tmp_path / "m.ply", 1.0, (0.0, 0.0, 0.0))
    raw = (tmp_path / "m.ply").read_bytes()
    body = raw[raw.index(b"end_header\n") + len(b"end_header\n"):]
    rows = np.frombuffer(body[: len(v) * 27], np.dtype([("p", "<f4", (6,)), ("c", "u1", (3,))]))
    assert rows["c"].tobytes() == c.tobytes()


# ---- 7. the planner: mode 3 on a mesh
def planner_cfg(pre, extra):
    """the configuration of the existing mode-3 test (160 x 90 images, 5 views) plus `extra`"""
    text = YAML.format(pre=pre, vs=os.path.join(GOLD, "hemisphere"), method=2, model_source="train_steps: 40\ntrain_rays: 1024\npoints_size_cloud: 2" + extra)
    text = text.replace("color_width: 1280", "color_width: 160").replace("color_height: 720", "color_height: 90").replace(
        "9.1560668945312500e+02", "114.45").replace("9.1332666015625000e+02", "114.2").replace("6.4714532470703125e+02", "80.9").replace(
        "3.7251531982421875e+02", "46.6")
    (pre / "models").mkdir(parents=True, exist_ok=True)
    cfg = pre / "cfg.yaml"
    cfg.write_text(text)
    return cfg


def run_mode3(cfg, name):
    return subprocess.run([os.path.join(ROOT, "nerf_prv_amd", "prv_planner"), str(cfg)], input=f"3\n{name}\n-1\n", text=True, capture_output=True, timeout=300)


def ellipsoid():
    """an ellipsoid of semi-axes 0.6, 0.45, 0.3 m, off-centre, coloured by its normals (never white): (positions float32, triangles,
    colours)"""
    d, t = uv_sphere((0, 0, 0), 1.0, 16, 32)
    v = (np.array([0.6, 0.45, 0.3]) * d.astype(np.float64) + [3.0, -2.0, 1.0]).astype(np.float32)
    return v, t, np.clip(128 + 120 * d.astype(np.float64), 0, 254).astype(np.uint8)


def centred_and_scaled(p, size):
    """mode 3's rule for the points of an object, operation by operation: the centroid (a running float64 sum in file order), the
    float32 difference, radius = the largest float64 norm of those, 17/16 of it, and p * size / that in float64, rounded to float32"""
    c = np.array([np.cumsum(p[:, a].astype(np.float64))[-1] for a in range(3)]) / float(len(p))
    q = (p.astype(np.float64) - c).astype(np.float32)
    q64 = q.astype(np.float64)
    radius = np.sqrt(((0.0 + q64[:, 0] * q64[:, 0]) + q64[:, 1] * q64[:, 1]) + q64[:, 2] * q64[:, 2]).max()
    raw = radius * 17.0 / 16.0
    return (q64 * size / raw).astype(np.float32)


def test_planner_mode3_with_a_mesh_writes_the_images_of_mesh_render(ctx, tmp_path):
    from PIL import Image

    from tests import coverage_ref
    from tests.march_ref import fmaf

    pre = tmp_path / "mesh_flow"
    cfg = planner_cfg(pre, "\ngt_surface: mesh")
    v, t, c = ellipsoid()
    api.write_mesh(pre / "models" / "egg.ply", v[:, [1, 2, 0]], t, colors=c, scale=1.0, offset=(0.0, 0.0, 0.0))  # the file holds (e2, e0, e1) = v
    out = run_mode3(cfg, "egg")
    assert out.returncode == 0, out.stdout + out.stderr
    assert f"{len(v)} vertices, {len(t)} triangles" in out.stdout
    gt = pre / "Coverage_images" / "ShapeNet" / "egg"
    assert float((gt / "size.txt").read_text()) == 0.1
    meta = json.load(open(gt / "5.json"))
    assert len(meta["frames"]) == 5 and (meta["w"], meta["h"]) == (160, 90)
    # the same vertices through Python: centred and scaled by the rule, placed with the json's scale and offset, then the axis cycle
    p = centred_and_scaled(v, 0.1)
    s, o = np.float32(meta["scale"]), np.asarray(meta["offset"], np.float32)
    q = np.stack([fmaf(p[:, a], s, o[a]) for a in range(3)], axis=1).astype(np.float32)
    e = np.ascontiguousarray(q[:, [1, 2, 0]])
    cs = ctx.cameras_from_dataset_json(str(gt / "5.json"))
    # the covered fraction, from the CPU reference alone: view 1 looks down on an object of 0.1 m that the view space frames
    cam1 = coverage_ref.cam_at(cs, 1, 160, 90, dataset=True)
    want1 = ref.render(cam1, e, t, c, 160, 90, flip=True)[0]
    frac = float((want1[..., 3] > 0).mean())
    print("covered fraction of view 1 (CPU reference):", frac)
    assert 0.02 < frac < 0.6
    with ctx.mesh_from_arrays(e, t, colors=c) as m:
        want = ctx.mesh_render(m, cs, None, 160, 90, flip180=True).cpu().numpy()
    assert want[1].tobytes() == want1.tobytes()
    for i in range(5):
        img = np.asarray(Image.open(gt / "5" / f"rgbaClip_{i}.png"))
        assert img.shape == (90, 160, 4) and img.tobytes() == want[i].tobytes(), i
    assert float((np.asarray(Image.open(gt / "5" / "rgbaClip_1.png"))[..., 3] > 0).mean()) == frac
    cs.close()


def test_planner_mode3_points_is_the_default_and_a_bad_surface_or_file_is_refused_before_anything_is_written(tmp_path):
    import struct

    rng = np.random.default_rng(21)
    d = rng.normal(size=(4000, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    xyz = (np.array([0.6, 0.45, 0.3]) * d + [3.0, -2.0, 1.0]).astype(np.float32)
    rgb = np.clip(128 + 120 * d, 0, 254).astype(np.uint32)
    packed = (rgb[:, 0] << 16) | (rgb[:, 1] << 8) | rgb[:, 2]
    body = b"".join(struct.pack("<fffI", *p, int(k)) for p, k in zip(xyz, packed))
    head = (f"VERSION 0.7\nFIELDS x y z rgb\nSIZE 4 4 4 4\nTYPE F F F U\nCOUNT 1 1 1 1\nWIDTH {len(xyz)}\nHEIGHT 1\n"
            f"VIEWPOINT 0 0 0 1 0 0 0\nPOINTS {len(xyz)}\nDATA binary\n").encode()
    outputs = []
    for where, extra in (("absent", ""), ("points", "\ngt_surface: points")):
        pre = tmp_path / where
        cfg = planner_cfg(pre, extra)
        (pre / "models" / "shell.pcd").write_bytes(head + body)
        out = run_mode3(cfg, "shell")
        assert out.returncode == 0, out.stdout + out.stderr
        gt = pre / "Coverage_images" / "ShapeNet" / "shell"
        files = sorted(p.relative_to(gt).as_posix() for p in gt.rglob("*") if p.is_file())
        assert "5/rgbaClip_4.png" in files and "size.txt" in files and "4000 points" in out.stdout
        outputs.append({f: (gt / f).read_bytes() for f in files})
    assert outputs[0] == outputs[1]
    # refusals: a value that is neither, an ASCII ply, no ply at all
    pre = tmp_path / "bad"
    cfg = planner_cfg(pre, "\ngt_surface: voxels")
    (pre / "models" / "shell.pcd").write_bytes(head + body)
    out = run_mode3(cfg, "shell")
    assert out.returncode != 0 and 'gt_surface must be points or mesh, got "voxels"' in out.stderr
    assert not (pre / "Coverage_images" / "ShapeNet" / "shell" / "size.txt").exists()
    pre = tmp_path / "ascii"
    cfg = planner_cfg(pre, "\ngt_surface: mesh")
    (pre / "models" / "shell.ply").write_text("ply\nformat ascii 1.0\nelement vertex 0\nend_header\n")
    out = run_mode3(cfg, "shell")
    assert out.returncode != 0 and "binary_little_endian" in out.stderr and "nothing was written" in out.stderr
    out = run_mode3(cfg, "nothing_here")
    assert out.returncode != 0 and "cannot open" in out.stderr
    assert not list((pre / "Coverage_images").rglob("size.txt"))
