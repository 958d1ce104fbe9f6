"""Dense replicas of the hashed levels of an F = 4 field that runs the <4, 5> instance (prv_device.hpp: ReplicaDev; prv_field_plan.hpp:
plan_replicas): a replica holds exactly the entries the hashed gather fetches, so everything a model computes with replicas
equals, BYTE FOR BYTE, what it computes without -- features, field outputs, pixels (float and RGBA8), evaluated-sample counts.
No comparison in this file has a tolerance.

PRV_REPLICA_LEVELS (0..3, 0 = off) and PRV_REPLICA_MB (the byte budget) are read when a model is installed, the render
policies when a context is created: every case builds its own contexts under `environment`.  The small field is the F4_5
entry of tests/instances.py (five dense levels, hashed levels of 48, 68 and 96 vertices per axis); the product's field is
api.FIELD_256 on bench.py's baseline scene."""
import numpy as np
import pytest

from nerf_prv_amd import api
from tests import instances, util
from tests.test_gpu_instances import environment

gpu = pytest.mark.gpu

# the replica counts a model can hold = the variants the library ships (render_queue64_replica_kernel<NGP, NREPL>; under the
# engine's rule the launch reads at most two of the levels a model holds: kReplicaLevelsNgp, prv_kernels.hpp)
VARIANTS = (1, 2, 3)
DEFAULT_LEVELS = 3    # what a model gets with nothing set, budget permitting (prv_field_plan.hpp: kReplicaBudgetDefault = 256 MiB)
F4_5 = instances.MATRIX["F4_5"]
BASELINE_256 = dict(api.FIELD_256, table_amp=0.1, density_bias=0.0)  # bench.py's field_kw("256", "baseline")
W, H = 48, 32
MIN_T = 1e-4
# small images under the engine's rule run the corner-cache instance by default (render_policy), which has no replica
# variant: the small-field contexts switch it off, so both stepping rules go through render_queue64_replica_kernel
PLAIN = {"PRV_CELL_CACHE": "0"}


# ---- the layout arithmetic, restated (no GPU)
def restated_replica(res, F=4):
    """a row of res + 1 entries rounded up to 8 entries, as many rows per plane, res + 1 planes, whole 4 KiB pages"""
    row = (res + 1 + 7) // 8 * 8
    mz = row * row * 2 * F
    return row, mz, (mz * (res + 1) + 4095) // 4096 * 4096


def hashed_res(kw):
    return [res for _, res, hashed, _ in instances.restated_levels(kw) if hashed]


def test_replica_layout_arithmetic():
    """strides and sizes against numbers written down here; every z stride below 2^24 (the gather multiplies with v_mul_u32_u24)"""
    assert hashed_res(api.FIELD_256) == [116, 173, 256]
    assert hashed_res(F4_5.kw) == [48, 68, 96]
    want = {116: (120, 115200, 13479936), 173: (176, 247808, 43118592), 256: (264, 557568, 143298560),
            48: (56, 25088, 1232896), 68: (72, 41472, 2863104), 96: (104, 86528, 8396800)}
    for res, w in want.items():
        assert restated_replica(res) == w
        assert api.replica_level(res, 4) == w
        assert w[1] < 1 << 24 and w[1] * res + w[0] * 8 * res + 8 * (res + 2) <= w[2]  # the last 16-byte load ends inside
    assert sum(want[r][2] for r in (116, 173, 256)) == 199897088 < 256 << 20  # FIELD_256: 190.6 MiB, inside the default budget
    assert sum(want[r][2] for r in (48, 68, 96)) == 12492800
    # power-of-two strides, for comparison: 16 MiB + 128 MiB + 1 GiB
    assert [8 << (3 * (r + 1 - 1).bit_length()) for r in (116, 173, 256)] == [16 << 20, 128 << 20, 1 << 30]
    # a level whose z stride would not fit 24 bits is not replicated
    assert api.replica_level(1448, 4)[2] == 0 and api.replica_level(1439, 4)[2] > 0


# ---- contexts
def fresh(env, kw, seed=util.SEED_A, slot=0):
    with environment(env):
        c = api.Context(0)
        c.synthetic_model(slot, api.field_desc(**kw), seed)
    return c


def expected_bytes(kw, n):
    return sum(restated_replica(r)[2] for r in hashed_res(kw)[:n])


@pytest.fixture(scope="module")
def small(oracle):
    """F4_5 in slot 0 of one context per variant; [0] = replicas off"""
    cs = {n: fresh(dict(PLAIN, PRV_REPLICA_LEVELS=str(n)), F4_5.kw) for n in (0,) + VARIANTS}
    for n, c in cs.items():
        instances.assert_layout(c.model_layout(0), F4_5)
        assert api.replica_layout(c, 0) == (n, expected_bytes(F4_5.kw, n))
    yield cs
    for c in cs.values():
        c.close()


@pytest.fixture(scope="module")
def views(oracle):
    tms, scale, offset = util.hemisphere_transforms(oracle, util.fibonacci_hemisphere(6))
    return tms[[0, 3, 5]], scale, offset


def render_all(c, views, w, h, slot=0):
    """-> {rule: (float image bytes, RGBA8 bytes, samples evaluated, samples live)} under both stepping rules, spp 1"""
    tms, scale, offset = views
    cams = c.cameras_from_matrices(tms, util.FOV_X, w, h, scale, offset)
    out = {}
    for rule, opts in (("fixed_s", api.render_opts(w, h, 128, 1, MIN_T)), ("ngp", api.engine_render_opts(w, h, 0, 1, MIN_T))):
        img, st = c.render(slot, cams, None, opts)
        u8, st8 = c.render_rgba8(slot, cams, None, opts)
        assert int(st.samples_evaluated) == int(st8.samples_evaluated) > 0
        out[rule] = (img.cpu().numpy().tobytes(), u8.cpu().numpy().tobytes(), int(st.samples_evaluated), int(st.samples_live))
    cams.close()
    return out


def assert_same(a, b, what):
    for rule in a:
        assert a[rule][2:] == b[rule][2:], (what, rule, "sample counts", a[rule][2:], b[rule][2:])
        assert a[rule][0] == b[rule][0], (what, rule, "float pixels differ")
        assert a[rule][1] == b[rule][1], (what, rule, "RGBA8 pixels differ")


# ---- features
def feature_positions(kw):
    """a few thousand positions: per level every combination, per axis, of 0, 1, the last cell's interior and nextafter(1, 0)
    (the clamp / duplicated-border cases); cell boundaries of every level; the cube's faces, edges and corners; random ones
    inside and beyond [0, 1] (clamp01)"""
    rng = np.random.default_rng(31)
    pos = [rng.random((2048, 3), dtype=np.float32), (rng.random((512, 3), dtype=np.float32) * 2.0 - 0.5).astype(np.float32),
           np.array([[-0.1, 1.2, 0.3], [1.5, -2.0, 7.0], [-1e-7, 1.0000001, 0.5]], np.float32),
           instances.cube_positions(), instances.boundary_positions(kw, rng)]
    for s, _res, _, _ in instances.restated_levels(kw):
        s = float(s)
        last = np.floor(np.float32(s) + np.float32(0.5))  # the cell of p = 1
        v = np.array([0.0, 1.0, min((last - 0.25) / s, 1.0), np.nextafter(np.float32(1), np.float32(0))], np.float32)
        x, y, z = np.meshgrid(v, v, v, indexing="ij")
        pos.append(np.stack([x.ravel(), y.ravel(), z.ravel()], 1))
    return np.ascontiguousarray(np.concatenate(pos), np.float32)


@gpu
def test_features_equal_off_and_oracle(small, oracle):
    pos = feature_positions(F4_5.kw)
    assert 3000 < len(pos) < 20000
    f = oracle.OracleField(oracle.desc(**F4_5.kw), seed=util.SEED_A)
    want = f.encode(pos)
    f.close()
    off = small[0].debug_encode(0, pos)
    assert np.array_equal(off, want)
    dirs = np.random.default_rng(32).standard_normal((len(pos), 3)).astype(np.float32)
    dirs /= np.linalg.norm(dirs, axis=1, keepdims=True)
    field_off = small[0].debug_field(0, pos, dirs)
    for n in VARIANTS:
        got = small[n].debug_encode(0, pos)
        bad = np.argwhere(got != off)
        assert len(bad) == 0, f"NREPL {n}: {len(bad)} feature words differ, first at position {pos[bad[0][0]]!r}, level {bad[0][1] // 4}"
        assert np.array_equal(got, want)
        out, occ = small[n].debug_field(0, pos, dirs)
        assert out.tobytes() == field_off[0].tobytes() and np.array_equal(occ, field_off[1])


# ---- images
@gpu
def test_images_equal_off(small, views):
    off = render_all(small[0], views, W, H)
    for n in VARIANTS:
        assert_same(render_all(small[n], views, W, H), off, f"NREPL {n}")


@gpu
def test_images_equal_off_with_relocation(small, views):
    """tail merge and the block's pool forced on by a small merge threshold: rays that change lanes re-read the right levels"""
    reloc = dict(PLAIN, PRV_MERGE_MAX="6", PRV_POOL="1")
    plain_off = render_all(small[0], views, W, H)
    c = fresh(dict(reloc, PRV_REPLICA_LEVELS="0"), F4_5.kw)
    off = render_all(c, views, W, H)
    c.close()
    assert_same(off, plain_off, "relocation, replicas off")
    for n in VARIANTS:
        c = fresh(dict(reloc, PRV_REPLICA_LEVELS=str(n)), F4_5.kw)
        assert api.replica_layout(c, 0)[0] == n
        got = render_all(c, views, W, H)
        c.close()
        assert_same(got, off, f"relocation, NREPL {n}")


# ---- the product's field
@gpu
def test_field_256_equal_off(views):
    """api.FIELD_256, baseline scene, two 80x45 views: what a model gets with nothing set against replicas off.  At this image
    size the engine's rule runs the corner-cache instance by default (render_policy), so a third context renders it with
    PRV_CELL_CACHE=0: the replica variant under both rules.  The only test that builds the 200 MB of replicas."""
    two = (views[0][:2], views[1], views[2])
    entry = instances.PRODUCT["FIELD_256"]
    off_c = fresh({"PRV_REPLICA_LEVELS": "0"}, BASELINE_256)
    lay_off = off_c.model_layout(0)
    assert api.replica_layout(off_c, 0) == (0, 0)
    off = render_all(off_c, two, 80, 45)
    off_c.close()
    for env in ({}, {"PRV_CELL_CACHE": "0"}):
        c = fresh(env, BASELINE_256)
        instances.assert_layout(c.model_layout(0), entry)
        assert c.model_layout(0) == lay_off
        assert api.replica_layout(c, 0) == (DEFAULT_LEVELS, expected_bytes(api.FIELD_256, DEFAULT_LEVELS))
        got = render_all(c, two, 80, 45)
        c.close()
        assert_same(got, off, f"FIELD_256 {env}")


# ---- republish
@gpu
def test_reinstall_rebuilds_replicas(views):
    """model A, render, model B into the same slot, render == a fresh context's render of B (stale replicas would show A's
    finest levels); a field without replica variants in the slot afterwards gives the buffer back"""
    env = dict(PLAIN, PRV_REPLICA_LEVELS="3")
    c = fresh(env, F4_5.kw, util.SEED_A)
    a = render_all(c, views, W, H)
    with environment(env):
        c.synthetic_model(0, api.field_desc(**F4_5.kw), util.SEED_B)
    assert api.replica_layout(c, 0) == (3, expected_bytes(F4_5.kw, 3))
    b = render_all(c, views, W, H)
    other = fresh(env, F4_5.kw, util.SEED_B)
    want = render_all(other, views, W, H)
    other.close()
    assert_same(b, want, "B after A")
    assert a["ngp"][0] != b["ngp"][0]
    off = fresh(dict(PLAIN, PRV_REPLICA_LEVELS="0"), F4_5.kw, util.SEED_B)
    assert_same(b, render_all(off, views, W, H), "B, replicas off")
    off.close()
    with environment(env):
        c.synthetic_model(0, api.field_desc(**instances.MATRIX["F4_3"].kw), util.SEED_A)  # <4, 3>: no replicas
    assert api.replica_layout(c, 0) == (0, 0)
    instances.assert_layout(c.model_layout(0), instances.MATRIX["F4_3"])
    c.close()


# ---- fallback
@gpu
@pytest.mark.parametrize("mb, want_levels", [(5, 2), (2, 1), (1, 0)])
def test_budget_falls_back_to_a_smaller_variant(small, views, mb, want_levels):
    """F4_5's replicas take 1.18 + 2.73 + 8.01 MiB: a budget the finest level does not fit runs the smaller variant, one the
    coarsest does not fit none; PRV_NO_PAIR=1 (the generic instance) composes: no replicas, same pixels"""
    c = fresh(dict(PLAIN, PRV_REPLICA_MB=str(mb)), F4_5.kw)
    assert api.replica_layout(c, 0) == (want_levels, expected_bytes(F4_5.kw, want_levels))
    got = render_all(c, views, W, H)
    c.close()
    off = render_all(small[0], views, W, H)
    assert_same(got, off, f"budget {mb} MiB")
    if mb == 1:
        g = fresh(dict(PLAIN, PRV_NO_PAIR="1", PRV_REPLICA_LEVELS="3"), F4_5.kw)
        instances.assert_layout(g.model_layout(0), F4_5, no_pair=True)
        assert api.replica_layout(g, 0) == (0, 0)
        assert_same(render_all(g, views, W, H), off, "PRV_NO_PAIR=1")
        g.close()
