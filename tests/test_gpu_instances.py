"""Everything that is compiled once per (F, NDENSE) field instance -- the feature gather, the field hook
(debug_field64_kernel), the colour and depth renders (render_queue64_kernel, render_planes_kernel) and the mesh kernels
(mesh_density_kernel, mesh_color_kernel) -- on every instance and on every reason for falling back to the generic one:
the field matrix of tests/instances.py.  util.SMALL and util.SMALL_F2, which the other parity modules use, select the
generic instances <4,0> and <2,0>; the fast instances <4,5>, <4,3>, <2,10>, <2,6> (paired dense loads, shared hash
constants) are what api.FIELD_256 / FIELD_512 run.

Every test first asserts the layout the context reports against the matrix.  References and bars are the existing ones:
features bit for bit with the oracle, field outputs at test_gpu_parity.py::test_field_eval's bars, pixels at
util.assert_pixels_close against the oracle / tests/depth_ref.py, the density grid bit for bit against the field hook and
3e-3 against the oracle, marching cubes equal to tests/mesh_ref.py.  A fast instance and the generic one (PRV_NO_PAIR=1)
return identical bytes everywhere: no tolerance.

Slots 56..63 of the session context."""
import contextlib
import os

import numpy as np
import pytest

from nerf_prv_amd import api, planner
from tests import depth_ref, instances, march_ref, mesh_ref, util
from tests.test_gpu_mesh import AABB, grid_points
from tests.test_gpu_parity import RTOL

pytestmark = pytest.mark.gpu

SLOT = 56  # the matrix entry under test
SLOT_TWIN = 57  # fast == generic
SLOT_RELOC = 58  # relocation on the fast depth instances
SLOT_PRODUCT = 60  # FIELD_256 / FIELD_512
W, H = 24, 20
THREADS = 16
# (samples per ray, spp, stepping rule): fixed S, fixed S with an odd count and two sub-samples, the engine's own rule
CONFIGS = [(128, 1, 0), (37, 2, 0), (0, 1, 1)]
CONFIG_IDS = ["S128", "S37spp2", "ngp"]
MIN_T = 1e-4
UP = np.array([0.0, 0.0, 1.0], np.float32)


class Loaded:
    def __init__(self, name, entry, field):
        self.name, self.entry, self.kw, self.f = name, entry, entry.kw, field


@contextlib.contextmanager
def environment(env):
    """the switches are read when a context is created and when a model is installed"""
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def load(ctx, oracle, slot, name, entry, want_oracle=True):
    ctx.synthetic_model(slot, api.field_desc(**entry.kw), util.SEED_A)
    instances.assert_layout(ctx.model_layout(slot), entry)
    return Loaded(name, entry, oracle.OracleField(oracle.desc(**entry.kw), seed=util.SEED_A) if want_oracle else None)


@pytest.fixture(scope="module", params=list(instances.MATRIX))
def inst(request, ctx, oracle):
    m = load(ctx, oracle, SLOT, request.param, instances.MATRIX[request.param])
    yield m
    m.f.close()
    ctx.synthetic_model(SLOT, api.field_desc(**util.SMALL), util.SEED_A)  # the slot does not keep a 68 MiB table


@pytest.fixture(scope="module")
def cams(ctx, oracle):
    tms, scale, offset = util.hemisphere_transforms(oracle, util.fibonacci_hemisphere(6))
    tms = tms[[0, 3]]
    cs = ctx.cameras_from_matrices(tms, util.FOV_X, W, H, scale, offset)
    yield cs, oracle.cameras_from_transforms(tms, util.FOV_X, W, H, scale, offset)
    cs.close()


def _opts(w, h, S, spp, mode, min_T=MIN_T):
    return api.render_opts(w, h, S if mode == 0 else 0, spp, min_T, step_mode=mode)


def _positions(kw, seed, n_random):
    rng = np.random.default_rng(seed)
    return np.concatenate([rng.random((n_random, 3), dtype=np.float32), instances.cube_positions(),
                           instances.boundary_positions(kw, rng)])


def _unit(rng, n):
    d = rng.standard_normal((n, 3)).astype(np.float32)
    return d / np.linalg.norm(d, axis=1, keepdims=True)


# ---- the matrix itself
def test_matrix_reaches_every_instance():
    """(F, kernel_dense_levels) of the matrix = every instance the kernels are compiled for; the product's fields run two of them"""
    assert {(e.F, e.instance) for e in instances.MATRIX.values()} == instances.ALL_INSTANCES
    assert {(e.F, e.instance) for e in instances.PRODUCT.values()} == {(4, 5), (2, 10)}
    assert [k for k, e in instances.MATRIX.items() if e.wide] == ["F4_wide"]
    assert sorted(instances.FAST) == ["F2_10", "F2_6", "F4_3", "F4_5"]


def test_layout(ctx, inst):
    lay = ctx.model_layout(SLOT)
    instances.assert_layout(lay, inst.entry)
    assert lay["table_bytes_physical"] == instances.restated_layout(inst.kw)["table_bytes_physical"]
    assert lay["n_dense_levels"] + lay["n_hashed_levels"] == inst.kw["n_levels"]


def test_layout_of_an_imported_snapshot_shape(ctx):
    """instant-ngp's nerf/base.json shape (tests/test_gpu_ingp.py: NGP) has 5 dense and 11 hashed levels at F = 2: there is
    no <2,5> instance, an imported snapshot of that shape runs the generic one"""
    from tests.test_gpu_ingp import NGP

    ctx.synthetic_model(SLOT + 7, api.field_desc(**NGP), util.SEED_A)
    lay = ctx.model_layout(SLOT + 7)
    want = instances.restated_layout(NGP)
    assert (lay["kernel_features"], lay["kernel_dense_levels"], lay["n_dense_levels"], lay["n_hashed_levels"]) == (2, 0, 5, 11)
    assert all(lay[k] == want[k] for k in ("kernel_dense_levels", "n_dense_levels", "n_hashed_levels", "table_bytes_physical"))
    ctx.synthetic_model(SLOT + 7, api.field_desc(**util.SMALL), util.SEED_A)


def test_a_rejected_install_empties_its_slot_and_no_other(ctx, cams):
    """a descriptor the plan rejects (tests/test_field_plan_host.py: PAST_LIMIT, a level of 4097 vertices per axis), loaded over a
    valid model: the call fails with the plan's text, the slot is empty afterwards, and the context's other slots render what they
    rendered before"""
    from tests.test_field_plan_host import PAST_LIMIT

    victim, bystander = SLOT + 3, SLOT + 6
    small = api.field_desc(**util.SMALL)
    ctx.synthetic_model(victim, small, util.SEED_A)
    ctx.synthetic_model(bystander, small, util.SEED_B)
    opts = _opts(W, H, 128, 1, 0)
    before = ctx.render(bystander, cams[0], None, opts)[0].cpu().numpy().copy()
    assert (ctx.render(victim, cams[0], None, opts)[0].cpu().numpy()[..., 3] > 0).any()
    bad = api.field_desc(**PAST_LIMIT)
    t, m, o = api.model_sizes(bad)
    with pytest.raises(api.PrvError, match=r"level 1 has 4097 vertices per axis \(limit 4096\)") as e:
        ctx.load_model(victim, bad, np.zeros(t, np.uint16), np.zeros(m, np.uint16), np.zeros(o, np.uint32))
    assert e.value.code == api.L.PRV_E_INVALID
    with pytest.raises(api.PrvError, match=f"model slot {victim} is empty") as e:
        ctx.render(victim, cams[0], None, opts)
    assert e.value.code == api.L.PRV_E_STATE
    assert np.array_equal(ctx.render(bystander, cams[0], None, opts)[0].cpu().numpy(), before)
    ctx.synthetic_model(victim, small, util.SEED_A)  # the slot takes a model again
    instances.assert_layout(ctx.model_layout(victim), instances.MATRIX["F4_0"])


# ---- features, field
def test_features_bit_exact(ctx, inst):
    instances.assert_layout(ctx.model_layout(SLOT), inst.entry)
    pos = _positions(inst.kw, 11, 2048)
    pos[:3] = [[-0.1, 1.2, 0.3], [1.0, 1.0, 1.0], [0.0, 0.0, 0.0]]  # outside: clamped
    got, want = ctx.debug_encode(SLOT, pos), inst.f.encode(pos)
    bad = np.argwhere(got != want)
    assert len(bad) == 0, f"{len(bad)} feature words differ, first at position {pos[bad[0][0]]!r}, level {bad[0][1] // inst.entry.F}"
    assert len(np.unique(got)) > 100  # fp16 bit patterns of a real table


def test_field_eval(ctx, inst):
    instances.assert_layout(ctx.model_layout(SLOT), inst.entry)
    rng = np.random.default_rng(12)
    pos = _positions(inst.kw, 13, 1024)[:3072]
    dirs = _unit(rng, len(pos))
    got, gocc = ctx.debug_field(SLOT, pos, dirs)
    want, wocc = inst.f.eval(pos, dirs)
    assert np.array_equal(gocc, wocc)
    # test_gpu_parity.py::test_field_eval's four bars
    np.testing.assert_allclose(got[:, 4:20], want[:, 4:20], rtol=RTOL, atol=2e-3)
    np.testing.assert_allclose(got[:, 20:23], want[:, 20:23], rtol=RTOL, atol=2e-3)
    np.testing.assert_allclose(got[:, 0], want[:, 0], rtol=3e-3)
    np.testing.assert_allclose(got[:, 1:4], want[:, 1:4], rtol=RTOL, atol=1e-4)


# ---- colour, depth
def _check_counts(st, f, ocams, w, h, S, spp, mode, n_eval):
    live = sum(f.march_count(oc, w, h, S, spp, threads=THREADS, step_mode=mode) for oc in ocams)
    assert int(st.samples_live) == live > 0  # every step's occupancy decision, exactly
    # early termination compares T against min_T after a hardware exp: a ray may stop a sample either side of the oracle's
    assert abs(int(st.samples_evaluated) - n_eval) <= max(2, n_eval // 100000)
    assert st.rays == len(ocams) * w * h * spp
    assert st.samples_nominal == st.rays * (S if mode == 0 else api.L.NGP_MAX_STEPS)


@pytest.mark.parametrize("S,spp,mode", CONFIGS, ids=CONFIG_IDS)
def test_colour(ctx, inst, cams, S, spp, mode):
    instances.assert_layout(ctx.model_layout(SLOT), inst.entry)
    cs, ocams = cams
    img, st = ctx.render(SLOT, cs, None, _opts(W, H, S, spp, mode))
    img = img.cpu().numpy()
    n_eval = 0
    for v, oc in enumerate(ocams):
        want, ne = inst.f.render(oc, W, H, S, spp, MIN_T, threads=THREADS, step_mode=mode)
        n_eval += ne
        util.assert_pixels_close(img[v], want)
    _check_counts(st, inst.f, ocams, W, H, S, spp, mode, n_eval)
    assert (img[..., 3] > 0).any()


@pytest.mark.parametrize("S,spp,mode", CONFIGS, ids=CONFIG_IDS)
def test_depth(ctx, oracle, inst, cams, S, spp, mode):
    instances.assert_layout(ctx.model_layout(SLOT), inst.entry)
    cs, ocams = cams
    rgba, depth, st, plain, st0 = depth_ref.both(ctx, SLOT, cs, _opts(W, H, S, spp, mode))
    depth_ref.check_identity(rgba, st, plain, st0)
    assert depth.shape == (len(ocams), H, W) and depth.dtype == np.float32
    for v, oc in enumerate(ocams):
        want = depth_ref.reference(oracle, inst.f, oc, W, H, S, spp, MIN_T, mode)
        got = np.concatenate([rgba[v], depth[v][..., None]], axis=-1)
        util.assert_pixels_close(got, want)
        assert np.array_equal(depth[v] == 0, want[..., 4] == 0)  # misses and dead rays: exactly 0
    assert (depth > 0).any()


# ---- mesh
@pytest.mark.parametrize("res,aabb", [((17, 23, 30), None), ((20, 16, 12), AABB), ((24, 24, 24), None)], ids=["17x23x30", "aabb", "24"])
def test_density_grid_is_the_field_bit_for_bit(ctx, inst, res, aabb):
    instances.assert_layout(ctx.model_layout(SLOT), inst.entry)
    grid = ctx.density_grid(SLOT, res, aabb).cpu().numpy()
    assert grid.shape == (res[2], res[1], res[0]) and grid.dtype == np.float32
    pts = grid_points(res, aabb)
    want, occ = ctx.debug_field(SLOT, pts, np.tile(UP, (len(pts), 1)))
    assert np.array_equal(grid.ravel().view(np.uint32), want[:, 0].view(np.uint32))
    with_occ = ctx.density_grid(SLOT, res, aabb, use_occupancy=True).cpu().numpy().ravel()
    assert np.array_equal(with_occ.view(np.uint32), (want[:, 0] * occ.astype(np.float32)).view(np.uint32))


def test_density_grid_matches_the_oracle(ctx, inst):
    instances.assert_layout(ctx.model_layout(SLOT), inst.entry)
    res = (13, 11, 9)
    pts = np.concatenate([grid_points(res, AABB), grid_points((7, 6, 5), None)])  # inside, and with the cube's faces
    grid = np.concatenate([ctx.density_grid(SLOT, res, AABB).cpu().numpy().ravel(), ctx.density_grid(SLOT, (7, 6, 5)).cpu().numpy().ravel()])
    want, _ = inst.f.eval(pts, np.tile(UP, (len(pts), 1)))
    np.testing.assert_allclose(grid, want[:, 0], rtol=3e-3)  # test_gpu_mesh.py::test_density_grid_matches_the_oracle's bar


def _mesh_arrays(m):
    return {a: getattr(m, a).copy() for a in ("vertices", "normals", "colors", "triangles")}


def _check_mesh_against_reference(ctx, slot, res, thr, min_triangles):
    grid = ctx.density_grid(slot, res).cpu().numpy()
    m = ctx.marching_cubes(slot, res, threshold=thr)
    try:
        v, n, t = mesh_ref.marching_cubes(grid, threshold=thr)
        assert len(t) > min_triangles
        assert np.array_equal(m.triangles, t)
        assert np.array_equal(m.vertices.view(np.uint32), v.view(np.uint32))
        np.testing.assert_allclose(m.normals, n, atol=1e-5)
        # colours: the field at the vertex seen from outside, quantised as an opaque pixel
        out, _ = ctx.debug_field(slot, m.vertices, -m.normals)
        rgba = np.concatenate([out[:, 1:4], np.ones((len(out), 1), np.float32)], 1)
        want = ctx.quantize_rgba8(ctx.torch.from_numpy(rgba).to(ctx.device), (0, 0, 0, 0)).cpu().numpy()[:, :3]
        assert np.array_equal(m.colors, want)
        assert len(np.unique(m.colors.reshape(-1, 3), axis=0)) > 10
    finally:
        m.close()


def test_marching_cubes_equals_the_reference(ctx, inst):
    instances.assert_layout(ctx.model_layout(SLOT), inst.entry)
    thr = float(np.median(ctx.density_grid(SLOT, 64).cpu().numpy()))
    _check_mesh_against_reference(ctx, SLOT, 64, thr, 2000)


# ---- a fast instance and the generic one: identical bytes
@pytest.fixture(scope="module", params=instances.FAST)
def twin(request, ctx, oracle):
    entry = instances.MATRIX[request.param]
    load(ctx, oracle, SLOT_TWIN, request.param, entry, want_oracle=False)
    with environment({"PRV_NO_PAIR": "1"}):
        other = api.Context(0)
        other.synthetic_model(0, api.field_desc(**entry.kw), util.SEED_A)
    instances.assert_layout(other.model_layout(0), entry, no_pair=True)
    yield entry, other
    other.close()
    ctx.synthetic_model(SLOT_TWIN, api.field_desc(**util.SMALL), util.SEED_A)


def _assert_twin_layouts(ctx, twin):
    entry, other = twin
    instances.assert_layout(ctx.model_layout(SLOT_TWIN), entry)
    instances.assert_layout(other.model_layout(0), entry, no_pair=True)
    assert entry.instance != 0


def test_fast_equals_generic_features_and_field(ctx, twin):
    _assert_twin_layouts(ctx, twin)
    entry, other = twin
    pos = _positions(entry.kw, 21, 4096)
    dirs = _unit(np.random.default_rng(22), len(pos))
    a, b = ctx.debug_encode(SLOT_TWIN, pos), other.debug_encode(0, pos)
    bad = np.argwhere(a != b)
    assert len(bad) == 0, f"{len(bad)} feature words differ, first at position {pos[bad[0][0]]!r}, level {bad[0][1] // entry.F}"
    (fa, oa), (fb, ob) = ctx.debug_field(SLOT_TWIN, pos, dirs), other.debug_field(0, pos, dirs)
    assert np.array_equal(oa, ob)
    bad = np.argwhere(fa.view(np.uint32) != fb.view(np.uint32))
    assert len(bad) == 0, f"{len(bad)} field outputs differ, first at position {pos[bad[0][0]]!r}, output {bad[0][1]}: {fa[tuple(bad[0])]!r} / {fb[tuple(bad[0])]!r}"


@pytest.mark.parametrize("mode", [0, 1], ids=["fixed_s", "ngp"])
def test_fast_equals_generic_render_and_depth(ctx, oracle, twin, mode):
    _assert_twin_layouts(ctx, twin)
    entry, other = twin
    tms, scale, offset = util.hemisphere_transforms(oracle, util.fibonacci_hemisphere(5))
    w, h = 56, 44
    opts = _opts(w, h, 96, 1, mode)
    outs = []
    for c, slot in ((ctx, SLOT_TWIN), (other, 0)):
        cs = c.cameras_from_matrices(tms, util.FOV_X, w, h, scale, offset)
        rgba, depth, st, plain, st0 = depth_ref.both(c, slot, cs, opts)
        depth_ref.check_identity(rgba, st, plain, st0)
        outs.append((plain, depth, int(st.samples_evaluated), int(st.samples_live)))
        cs.close()
    a, b = outs
    assert np.array_equal(a[0].view(np.uint32), b[0].view(np.uint32))
    assert np.array_equal(a[1].view(np.uint32), b[1].view(np.uint32))
    assert a[2] == b[2] > 0 and a[3] == b[3] > 0
    assert (a[1] > 0).any()


def test_fast_equals_generic_mesh(ctx, twin):
    _assert_twin_layouts(ctx, twin)
    entry, other = twin
    for res, aabb in (((17, 23, 30), None), ((20, 16, 12), AABB)):
        for occ in (False, True):
            a = ctx.density_grid(SLOT_TWIN, res, aabb, use_occupancy=occ).cpu().numpy()
            b = other.density_grid(0, res, aabb, use_occupancy=occ).cpu().numpy()
            assert a.tobytes() == b.tobytes(), (res, occ)
    thr = float(np.median(ctx.density_grid(SLOT_TWIN, 64).cpu().numpy()))
    ma, mb = ctx.marching_cubes(SLOT_TWIN, 64, threshold=thr), other.marching_cubes(0, 64, threshold=thr)
    try:
        xa, xb = _mesh_arrays(ma), _mesh_arrays(mb)
        assert len(xa["triangles"]) > 2000
        for k in xa:
            assert xa[k].tobytes() == xb[k].tobytes(), k
    finally:
        ma.close()
        mb.close()


# ---- rays change lanes mid-flight (tail merge, tail pool): the depth kernels move a seventh word per ray
@pytest.mark.parametrize("env", [{"PRV_MERGE_MAX": "31", "PRV_POOL": "1"}, {"PRV_MERGE_MAX": "0"}], ids=["merge31_pool", "merge0"])
@pytest.mark.parametrize("name", ["F4_5", "F2_10"])
def test_depth_relocation_on_the_fast_instances(ctx, oracle, name, env):
    entry = instances.MATRIX[name]
    tms, scale, offset = util.hemisphere_transforms(oracle, util.fibonacci_hemisphere(6))
    w, h = 96, 80
    ctx.synthetic_model(SLOT_RELOC, api.field_desc(**entry.kw), util.SEED_B)
    instances.assert_layout(ctx.model_layout(SLOT_RELOC), entry)
    with environment(env):
        other = api.Context(0)
        other.synthetic_model(0, api.field_desc(**entry.kw), util.SEED_B)
    try:
        instances.assert_layout(other.model_layout(0), entry)
        for mode in (1, 0):
            opts = _opts(w, h, 128, 1, mode)
            outs = []
            for c, slot in ((ctx, SLOT_RELOC), (other, 0)):
                cs = c.cameras_from_matrices(tms, util.FOV_X, w, h, scale, offset)
                rgba, z, _ = c.render_depth(slot, cs, None, opts)
                outs.append((rgba.cpu().numpy(), z.cpu().numpy()))
                cs.close()
            (ra, za), (rb, zb) = outs
            assert np.array_equal(ra.view(np.uint32), rb.view(np.uint32))
            assert np.array_equal(za.view(np.uint32), zb.view(np.uint32))
            assert (za > 0).any()
    finally:
        other.close()


# ---- the product's fields at the product's shape
@pytest.fixture(scope="module", params=list(instances.PRODUCT))
def product(request, ctx, oracle):
    m = load(ctx, oracle, SLOT_PRODUCT, request.param, instances.PRODUCT[request.param])
    yield m
    m.f.close()
    ctx.synthetic_model(SLOT_PRODUCT, api.field_desc(**util.SMALL), util.SEED_A)


@pytest.fixture(scope="module")
def candidate(ctx, oracle):
    """one 80x45 view of bench.py's candidate set"""
    tms, scale, offset = planner.hemisphere_transforms(planner.hemisphere_generate(64), 0.3, 0.1, [1e-10] * 3)
    tms = tms[[20]]
    w, h = 80, 45
    cs = ctx.cameras_from_matrices(tms, util.FOV_X, w, h, scale, offset)
    yield cs, oracle.cameras_from_transforms(tms, util.FOV_X, w, h, scale, offset)[0], w, h
    cs.close()


def test_product_layout(ctx, product):
    instances.assert_layout(ctx.model_layout(SLOT_PRODUCT), product.entry)


# the engine's rule with the engine's min_T (0.01: a ray may stop a sample either side of the threshold, util.py) and fixed S.
# The reference is per-ray Python, three times over under the engine's rule: every third pixel of the view in row-major
# order, a fixed stride (80 = 3 * 26 + 2: the columns shift from row to row), no data-dependent selection
PRODUCT_STRIDE = 3


@pytest.mark.parametrize("S,min_T", [(0, 0.01), (128, 1e-4)], ids=["engine_rule", "S128"])
def test_product_depth(ctx, oracle, product, candidate, S, min_T):
    instances.assert_layout(ctx.model_layout(SLOT_PRODUCT), product.entry)
    cs, oc, w, h = candidate
    mode = 1 if S == 0 else 0
    opts = api.engine_render_opts(w, h, S, 1, min_T)
    assert opts.step_mode == (api.L.STEP_NGP if S == 0 else api.L.STEP_FIXED_S)
    rgba, depth, st, plain, st0 = depth_ref.both(ctx, SLOT_PRODUCT, cs, opts)
    depth_ref.check_identity(rgba, st, plain, st0)  # the whole view
    got = march_ref.strided(np.concatenate([rgba[0], depth[0][..., None]], axis=-1), PRODUCT_STRIDE)
    assert len(got) * 4 >= w * h  # at least one pixel in four

    def ref(mt):
        return march_ref.strided(depth_ref.reference(oracle, product.f, oc, w, h, S, 1, mt, mode, PRODUCT_STRIDE), PRODUCT_STRIDE)

    if min_T == 0.01:
        util.assert_pixels_close_any(got, [ref(mt) for mt in util.termination_variants(min_T)])
    else:
        want = ref(min_T)
        util.assert_pixels_close(got, want)
        assert np.array_equal(got[:, 4] == 0, want[:, 4] == 0)
    assert (got[:, 4] > 0).sum() > 50


def test_product_density_grid(ctx, product):
    instances.assert_layout(ctx.model_layout(SLOT_PRODUCT), product.entry)
    res = (64, 64, 64)
    grid = ctx.density_grid(SLOT_PRODUCT, res).cpu().numpy().ravel()
    pts = grid_points(res)
    want, _ = ctx.debug_field(SLOT_PRODUCT, pts, np.tile(UP, (len(pts), 1)))
    assert np.array_equal(grid.view(np.uint32), want[:, 0].view(np.uint32))
    pick = np.random.default_rng(31).choice(len(pts), 4096, replace=False)
    ref, _ = product.f.eval(pts[pick], np.tile(UP, (len(pick), 1)))
    np.testing.assert_allclose(grid[pick], ref[:, 0], rtol=3e-3)


def test_marching_cubes_on_the_512_field_equals_the_reference(ctx):
    """tests/test_gpu_mesh.py::test_res_512_on_the_512_field checks determinism at res 512; this is the same field and
    threshold at a size the numpy reference can do"""
    entry = instances.PRODUCT["FIELD_512"]
    ctx.synthetic_model(SLOT_PRODUCT + 1, api.field_desc(**entry.kw), util.SEED_A)
    instances.assert_layout(ctx.model_layout(SLOT_PRODUCT + 1), entry)
    thr = float(np.percentile(ctx.density_grid(SLOT_PRODUCT + 1, 64).cpu().numpy(), 99))  # a surface, not a sponge
    _check_mesh_against_reference(ctx, SLOT_PRODUCT + 1, 96, thr, 500)
    ctx.synthetic_model(SLOT_PRODUCT + 1, api.field_desc(**util.SMALL), util.SEED_A)
