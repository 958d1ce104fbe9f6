"""Mesh extraction on the GPU (prv_mesh.hip through the C ABI): the density grid bit for bit against the field hook, the
marching cubes against the numpy reference (tests/mesh_ref.py) on the same sigma grid, the colours against the field hook,
and the run.py mirrors (Testbed, the flag-file server)."""
import numpy as np
import pytest

from nerf_prv_amd import _lib as L
from nerf_prv_amd import api, compat_server
from tests import mesh_ref, util
from tests.test_mesh_tables import parse_obj, parse_ply

pytestmark = pytest.mark.gpu

SLOT = 40  # slots of their own: the session context is shared with the other GPU modules
AABB = ((0.1, 0.2, 0.15), (0.8, 0.9, 0.7))


def grid_points(res, aabb=None):
    """(n, 3) fp32 positions of the grid points, x fastest -- lo + float32(i) * step, as the kernel computes them"""
    lo, hi = aabb if aabb is not None else ((0, 0, 0), (1, 1, 1))
    ax = mesh_ref.grid_axes(res, lo, hi)
    z, y, x = np.meshgrid(ax[2], ax[1], ax[0], indexing="ij")
    return np.stack([x.ravel(), y.ravel(), z.ravel()], 1).astype(np.float32)


@pytest.fixture(scope="module", params=["F4", "F2"])
def field(request, ctx, oracle):
    kw = util.SMALL if request.param == "F4" else util.SMALL_F2
    ctx.synthetic_model(SLOT, api.field_desc(**kw), util.SEED_A)
    return kw


@pytest.mark.parametrize("res,aabb", [((24, 24, 24), None), ((17, 23, 30), None), ((20, 16, 12), AABB)])
def test_density_grid_is_the_field_bit_for_bit(ctx, field, res, aabb):
    grid = ctx.density_grid(SLOT, res, aabb).cpu().numpy()
    assert grid.shape == (res[2], res[1], res[0]) and grid.dtype == np.float32
    pts = grid_points(res, aabb)
    want, occ = ctx.debug_field(SLOT, pts, np.tile([0.0, 0.0, 1.0], (len(pts), 1)))
    assert np.array_equal(grid.ravel().view(np.uint32), want[:, 0].view(np.uint32))
    with_occ = ctx.density_grid(SLOT, res, aabb, use_occupancy=True).cpu().numpy().ravel()
    assert np.array_equal(with_occ.view(np.uint32), (want[:, 0] * occ.astype(np.float32)).view(np.uint32))


def test_density_grid_matches_the_oracle(ctx, oracle, field):
    res = (13, 11, 9)
    grid = ctx.density_grid(SLOT, res, AABB).cpu().numpy().ravel()
    pts = grid_points(res, AABB)
    f = oracle.OracleField(oracle.desc(**field), seed=util.SEED_A)
    want, _ = f.eval(pts, np.tile([0.0, 0.0, 1.0], (len(pts), 1)).astype(np.float32))
    np.testing.assert_allclose(grid, want[:, 0], rtol=3e-3)  # test_gpu_parity.py::test_field_eval's bar


def sphere_grid(res, k=10.0, r=0.3, c=(0.5, 0.5, 0.5)):
    ax = mesh_ref.grid_axes(res, (0, 0, 0), (1, 1, 1))
    z, y, x = np.meshgrid(ax[2], ax[1], ax[0], indexing="ij")
    d = np.sqrt((x - c[0]) ** 2 + (y - c[1]) ** 2 + (z - c[2]) ** 2)
    return np.exp(k * (r - d)).astype(np.float32), r - np.log(2.5) / k


@pytest.mark.parametrize("res", [(64, 64, 64), (48, 64, 80)])
def test_marching_cubes_grid_on_an_analytic_sphere(ctx, res):
    sigma, r_iso = sphere_grid(res)
    m = ctx.marching_cubes_grid(ctx.torch.from_numpy(sigma).to(ctx.device), threshold=2.5)
    v, n, t = mesh_ref.marching_cubes(sigma, threshold=2.5)
    assert len(v) > 1000
    assert np.array_equal(m.triangles, t)
    assert np.array_equal(m.vertices.view(np.uint32), v.view(np.uint32))
    np.testing.assert_allclose(m.normals, n, atol=1e-5)
    assert (m.colors == 0).all()  # no field, no colours
    dist = np.linalg.norm(m.vertices.astype(np.float64) - 0.5, axis=1)
    assert np.abs(dist - r_iso).max() < 1e-3
    assert mesh_ref.euler_characteristic(len(m.vertices), m.triangles) == (2, True)
    vol = mesh_ref.signed_volume(m.vertices, m.triangles)
    assert vol > 0 and abs(vol / (4.0 / 3.0 * np.pi * r_iso ** 3) - 1.0) < 0.01
    m.close()


def test_marching_cubes_on_a_field_equals_the_reference(ctx, field):
    res = 128
    grid = ctx.density_grid(SLOT, res).cpu().numpy()
    thr = float(np.median(grid))
    m1 = ctx.marching_cubes(SLOT, res, threshold=thr)
    m2 = ctx.marching_cubes(SLOT, res, threshold=thr)
    v, n, t = mesh_ref.marching_cubes(grid, threshold=thr)
    assert len(t) > 10000
    assert np.array_equal(m1.triangles, t)
    assert np.array_equal(m1.vertices.view(np.uint32), v.view(np.uint32))
    np.testing.assert_allclose(m1.normals, n, atol=1e-5)
    for a in ("vertices", "normals", "colors", "triangles"):  # deterministic: identical bytes
        assert getattr(m1, a).tobytes() == getattr(m2, a).tobytes(), a
    # colours: the field at the vertex seen from outside, quantised as an opaque pixel
    out, _ = ctx.debug_field(SLOT, m1.vertices, -m1.normals)
    rgba = np.concatenate([out[:, 1:4], np.ones((len(out), 1), np.float32)], 1)
    want = ctx.quantize_rgba8(ctx.torch.from_numpy(rgba).to(ctx.device), (0, 0, 0, 0)).cpu().numpy()[:, :3]
    assert np.array_equal(m1.colors, want)
    assert len(np.unique(m1.colors.reshape(-1, 3), axis=0)) > 10
    stages = ctx.mesh_stage_ms()
    assert all(x >= 0 for x in stages.values()) and stages["grid"] > 0
    m1.close()
    m2.close()


# ---------------------------------------------------------------- adversarial and edge grids (tests/mesh_ref.py)
CLOSED_GRIDS = {"closed_%02d" % k: g for k, g in enumerate(mesh_ref.adversarial_grids())}
EDGE_GRIDS = {name: (sigma, thr) for name, sigma, thr in mesh_ref.edge_grids()}
_want = {}


def _reference(name):
    """the grid, its threshold and the reference's mesh, computed once"""
    if name not in _want:
        sigma, thr = (CLOSED_GRIDS.get(name) or EDGE_GRIDS[name])
        _want[name] = (sigma, thr) + mesh_ref.marching_cubes(sigma, threshold=thr)
    return _want[name]


def _extract_and_compare(ctx, name):
    """the mesh of a grid, equal to the reference's (ids and positions exactly, normals at the file's 1e-5), twice"""
    sigma, thr, v, n, t = _reference(name)
    dev = ctx.torch.from_numpy(sigma).to(ctx.device)
    m, again = ctx.marching_cubes_grid(dev, threshold=thr), ctx.marching_cubes_grid(dev, threshold=thr)
    try:
        assert m.counts() == (len(v), len(t))
        assert np.array_equal(m.triangles, t)
        assert np.array_equal(m.vertices.view(np.uint32), v.view(np.uint32))
        dev_n = float(np.abs(m.normals.astype(np.float64) - n).max()) if len(n) else 0.0
        print(f"{name}: {len(v)} vertices, {len(t)} triangles, normals off by at most {dev_n:.3g}")
        np.testing.assert_allclose(m.normals, n, atol=1e-5)
        for a in ("vertices", "normals", "colors", "triangles"):  # deterministic: identical bytes
            assert getattr(m, a).tobytes() == getattr(again, a).tobytes(), a
    except BaseException:
        m.close()
        raise
    finally:
        again.close()
    return m


@pytest.mark.parametrize("name", list(CLOSED_GRIDS))
def test_marching_cubes_grid_on_closed_adversarial_grids(ctx, name):
    m = _extract_and_compare(ctx, name)
    assert len(m.triangles) > 0 and mesh_ref.is_closed_manifold(m.triangles)
    m.close()


@pytest.mark.parametrize("name", list(EDGE_GRIDS))
def test_marching_cubes_grid_on_edge_grids(ctx, name, tmp_path):
    sigma = EDGE_GRIDS[name][0]
    if name == "noise_4097_waves":
        assert -(-sigma.size // 64) == 4097 and sigma.size % 64 != 0
    m = _extract_and_compare(ctx, name)
    assert np.isfinite(m.vertices).all() and np.isfinite(m.normals).all()
    if name.startswith("nonfinite"):
        assert not np.isfinite(sigma).all()
        pts = m.sample(1000, 5).cpu().numpy()
        assert pts.shape == (1000, 3) and np.isfinite(pts).all()
        m.save(tmp_path / "m.ply", 1.0, (0, 0, 0))
        pv, pn, _, pt = parse_ply(tmp_path / "m.ply")
        assert np.isfinite(pv).all() and np.isfinite(pn).all() and np.array_equal(pt, m.triangles.astype(np.int64))
        m.save(tmp_path / "m.obj", 1.0, (0, 0, 0))
        text = (tmp_path / "m.obj").read_text().lower()
        assert "nan" not in text and "inf" not in text
        assert len(parse_obj(tmp_path / "m.obj")[0]) == len(m.vertices)
    m.close()


def test_marching_cubes_with_occupancy_on_unequal_axes(ctx):
    """the field path: the occupancy mask makes exact-zero plateaus in a real field"""
    ctx.synthetic_model(SLOT + 5, api.field_desc(**util.SMALL), util.SEED_A)
    res = (17, 23, 30)
    grid = ctx.density_grid(SLOT + 5, res, use_occupancy=True).cpu().numpy()
    assert grid.shape == (30, 23, 17) and (grid == 0).any() and (grid > 0).any()
    thr = float(np.median(grid))
    m = ctx.marching_cubes(SLOT + 5, res, threshold=thr, use_occupancy=True)
    v, n, t = mesh_ref.marching_cubes(grid, threshold=thr)
    assert len(t) > 0 and m.counts() == (len(v), len(t))
    assert np.array_equal(m.triangles, t)
    assert np.array_equal(m.vertices.view(np.uint32), v.view(np.uint32))
    np.testing.assert_allclose(m.normals, n, atol=1e-5)
    m.close()


def test_empty_grid_bad_arguments_and_inert_meshes(ctx, tmp_path):
    m = ctx.marching_cubes_grid(ctx.torch.zeros((9, 8, 7), dtype=ctx.torch.float32, device=ctx.device))
    assert m.vertices.shape == (0, 3) and m.triangles.shape == (0, 3) and m.counts() == (0, 0)
    m.save(tmp_path / "empty.ply", 1.0, (0, 0, 0))
    assert all(len(a) == 0 for a in parse_ply(tmp_path / "empty.ply"))
    m.close()
    ctx.synthetic_model(SLOT + 1, api.field_desc(**util.SMALL), util.SEED_B)
    for kw in (dict(res=1), dict(res=(8, 8, 1025)), dict(res=8, aabb=((0.5, 0, 0), (0.5, 1, 1))),
               dict(res=8, aabb=((0, 0, 0), (1, 1.5, 1))), dict(res=8, aabb=((-0.1, 0, 0), (1, 1, 1))),
               dict(res=8, threshold=float("nan"))):
        with pytest.raises(api.PrvError) as e:
            ctx.marching_cubes(SLOT + 1, **kw)
        assert e.value.code == L.PRV_E_INVALID, kw
    with pytest.raises(api.PrvError) as e:
        ctx.density_grid(SLOT + 1, 0)
    assert e.value.code == L.PRV_E_INVALID
    with pytest.raises(api.PrvError) as e:
        ctx.marching_cubes(SLOT + 2, 8)  # empty slot
    assert e.value.code == L.PRV_E_STATE
    m = ctx.marching_cubes(SLOT + 1, 16, threshold=0.0)
    with pytest.raises(api.PrvError) as e:
        m.save(tmp_path / "mesh.stl")
    assert e.value.code == L.PRV_E_INVALID
    m.close()
    # a mesh that outlives its context is inert: errors, no crash
    other = api.Context(0)
    other.synthetic_model(0, api.field_desc(**util.SMALL), util.SEED_B)
    m = other.marching_cubes(0, 16, threshold=float(np.median(other.density_grid(0, 16).cpu().numpy())))
    assert m.counts()[0] > 0
    other.close()
    with pytest.raises(api.PrvError) as e:
        m.counts()
    assert e.value.code == L.PRV_E_STATE
    with pytest.raises(api.PrvError) as e:
        m.save(tmp_path / "late.ply")
    assert e.value.code == L.PRV_E_STATE and not (tmp_path / "late.ply").exists()
    m.close()


def test_res_512_on_the_512_field(ctx):
    ctx.synthetic_model(SLOT + 3, api.field_desc(**api.FIELD_512), util.SEED_A)
    thr = float(np.percentile(ctx.density_grid(SLOT + 3, 64).cpu().numpy(), 99))  # a surface, not a sponge
    a = ctx.marching_cubes(SLOT + 3, 512, threshold=thr, colors=False)
    b = ctx.marching_cubes(SLOT + 3, 512, threshold=thr, colors=False)
    assert a.counts() == b.counts() and a.counts()[1] > 0
    assert a.triangles.tobytes() == b.triangles.tobytes()
    assert int(a.triangles.max()) == len(a.vertices) - 1
    a.close()
    b.close()


def test_testbed_and_flag_file_server_save_meshes(ctx, tmp_path):
    tb = api.Testbed(0)
    try:
        tb.synthetic_model(api.field_desc(**util.SMALL), util.SEED_A)
        tb.scale, tb.offset = 0.6, [0.4, 0.55, 0.3]
        thr = float(np.median(tb.ctx.density_grid(0, 40).cpu().numpy()))
        tb.compute_and_save_marching_cubes_mesh(str(tmp_path / "tb.ply"), (40, 40, 40), thresh=thr)
        pv, pn, pc, pt = parse_ply(tmp_path / "tb.ply")
        want = tb.ctx.marching_cubes(0, 40, threshold=thr)
        q = pv.astype(np.float64) * tb.scale + np.asarray(tb.offset)  # dataset -> q, then e = (q1, q2, q0)
        np.testing.assert_allclose(q[:, [1, 2, 0]], want.vertices, rtol=1e-6, atol=1e-7)
        assert np.array_equal(pt, want.triangles.astype(np.int64)) and np.array_equal(pc, want.colors)
        d = tb.compute_marching_cubes_mesh((40, 40, 40), thresh=thr)
        assert np.array_equal(d["V"], pv) and np.array_equal(d["F"], pt) and np.array_equal(d["N"], pn)
        want.close()
    finally:
        tb.ctx.close()
    # run.py:279-282 through the flag-file server
    scene = tmp_path / "scene.json"
    scene.write_text('{"scale": 0.5, "offset": [0.5, 0.5, 0.5], "frames": []}')
    out = tmp_path / "meshes" / "m.obj"
    cmd = f"python run.py --scene {scene} --n_steps 0 --save_mesh {out} --marching_cubes_res 24"
    args = compat_server.parse_command("import os\nos.system('" + cmd + "')\n")

    def load_model(sc, cx):
        cx.synthetic_model(SLOT + 4, api.field_desc(**util.SMALL), util.SEED_B)
        return SLOT + 4

    compat_server.CompatServer(str(tmp_path), ctx, load_model).serve_one(args)
    pv, pn, pc, pt = parse_obj(out)
    want = ctx.marching_cubes(SLOT + 4, 24)  # run.py's default threshold
    assert len(pv) == len(want.vertices) and np.array_equal(pt, want.triangles.astype(np.int64))
    np.testing.assert_allclose(pv, api.engine_to_dataset(want.vertices, 0.5, [0.5, 0.5, 0.5]), rtol=1e-6, atol=1e-7)
    want.close()
