"""What the parameter regimes of tests/field_cases.py contain, asserted with the CPU oracle alone (no GPU), and the float64
reference of tests/field_ref.py against the oracle on an ordinary field.  tests/test_gpu_field_regimes.py runs the kernels on
these regimes; a regime that did not reach the binary16 edge it is named after would make those tests pass for nothing."""
import ctypes as C

import numpy as np
import pytest

from tests import field_cases as fc
from tests import field_ref, instances, march_ref, util

RENDER_SHAPES = ["F4_5", "F2_10"]
W, H = 24, 20


@pytest.fixture(scope="module", params=fc.SHAPES)
def name(request):
    return request.param


def _field(oracle, c):
    return oracle.OracleField(oracle.desc(**c.kw), params=c.params)


def _outputs(oracle, regime, name):
    c = fc.case(oracle, regime, name)
    pos = fc.regime_positions(regime, c.kw)
    f = _field(oracle, c)
    out, occ = f.eval(pos, fc.directions(len(pos)))
    f.close()
    return c, pos, out, occ


def test_shapes_are_the_matrix_without_the_large_ones():
    assert set(fc.SHAPES) == {k for k, e in instances.MATRIX.items() if (e.F, e.instance) in instances.ALL_INSTANCES and not e.wide
                              and k not in ("F4_finer_than_table", "F2_all_dense")}
    assert {(instances.MATRIX[k].F, instances.MATRIX[k].instance) for k in fc.SHAPES} == instances.ALL_INSTANCES
    assert instances.MATRIX["F4_all_hashed"].n_dense == 0


@pytest.mark.parametrize("regime", fc.HOST_REGIMES)
def test_parameters_are_finite_seeded_and_of_the_models_size(oracle, name, regime):
    c = fc.case(oracle, regime, name)
    again = fc.GENERATORS[regime](oracle, name)
    want = oracle.OracleField(oracle.desc(**c.kw), seed=1).params()
    for a, b, w in zip(c.params, again.params, want):
        assert a.dtype == w.dtype and a.shape == w.shape
        assert np.array_equal(a, b)  # seeded
    assert fc.all_finite_params(c.params)  # the ABI defines nothing for Inf / NaN words
    assert np.isfinite(c.kw["density_bias"])


def test_positions_hold_every_kind_and_the_restated_layout_is_the_oracles(oracle, name):
    kw = fc.shape_kw(name)
    pos = fc.positions(kw)
    assert 2500 <= len(pos) <= fc.N_POSITIONS
    assert ((pos == 0) | (pos == 1)).any(axis=1).sum() >= 200  # the cube's surface
    lv, total = oracle.levels(oracle.desc(**kw))
    mine = fc.level_table(kw)
    assert total == mine[-1][3] + mine[-1][4]
    for a, b in zip(lv, mine):
        assert (a.scale, a.res, a.hashed, a.size, a.offset) == (b[0], b[1], int(b[2]), b[3], b[4])
    # corner_entries is orc_encode's addressing: a table that holds its own entry number in feature 0 blends to a value between
    # the smallest and the largest corner entry of every level (weights within one fp16 rounding of a partition of one)
    t, m, o = fc.case(oracle, "fresh", name).params
    F = kw["n_features"]
    ent = fc.corner_entries(kw, pos)
    for l, (_, _, _, size, off) in enumerate(mine):
        local = np.arange(t.size // F, dtype=np.float64) - off
        tab = np.zeros(t.size, np.float16)
        tab[::F] = (np.clip(local, 0, size) / size).astype(np.float16)  # in [0, 1]: monotone in the entry number
        f = oracle.OracleField(oracle.desc(**kw), params=(tab.view(np.uint16), m, o))
        got = f.encode(pos)[:, l * F].view(np.float16).astype(np.float64)
        f.close()
        vals = tab[::F].astype(np.float64)[ent[l]]
        assert (got >= vals.min(axis=1) - 2e-3).all() and (got <= vals.max(axis=1) + 2e-3).all(), l


# ---- fresh
def test_fresh_is_mostly_subnormal(oracle, name):
    c = fc.case(oracle, "fresh", name)
    assert c.kw["table_amp"] == 1e-4 and (c.params[2] == 0xFFFFFFFF).all()
    assert fc.is_subnormal_half(c.params[0]).mean() >= 0.5
    f = _field(oracle, c)
    feat = f.encode(fc.positions(c.kw))
    f.close()
    small = fc.is_subnormal_half(feat) | ((feat & 0x7FFF) == 0)
    assert small.mean() >= 0.25
    F = c.kw["n_features"]
    for l in range(c.kw["n_levels"]):
        assert (feat[:, l * F:(l + 1) * F] & 0x7FFF).any(), l  # no level's features are all zero


# ---- edges
def test_edges_reach_every_class_on_every_level_and_overflow_in_the_blend(oracle, name):
    c = fc.case(oracle, "edges", name)
    pos = fc.regime_positions("edges", c.kw)
    F = c.kw["n_features"]
    cls = fc.half_class(c.params[0]).reshape(-1, F)
    ent = fc.corner_entries(c.kw, pos)
    for l in range(c.kw["n_levels"]):
        seen = cls[ent[l]]  # (positions, 8 corners, F)
        assert set(seen.ravel()) == set(fc.EDGE_CLASSES) | {"ordinary"}, l
        # the eight corners of a cell mix the classes: most cells of the random positions (the first 1024) see three or more
        mixed = np.mean([len(set(cell.ravel())) >= 3 for cell in seen[:1024:8]])
        assert mixed > 0.75, (l, mixed)
    signs = c.params[0] >> 15
    assert 0.4 < signs.mean() < 0.6
    f = _field(oracle, c)
    feat = f.encode(pos)
    f.close()
    inf = fc.is_inf_half(feat)
    assert (feat[inf] == 0x7C00).any() and (feat[inf] == 0xFC00).any()  # +Inf and -Inf out of finite entries
    assert ((feat & 0x7C00) != 0x7C00).mean() >= 0.9
    assert not (((feat & 0x7C00) == 0x7C00) & ((feat & 0x03FF) != 0)).any()  # no NaN: the chain never subtracts infinities


# ---- saturated
def test_saturated_sigma_leaves_the_normal_floats_at_both_ends(oracle, name):
    c, pos, out, _ = _outputs(oracle, "saturated", name)
    logit = out[:, 4].astype(np.float64) + c.kw["density_bias"]
    assert (logit < fc.LOGIT_FLUSH).any() and (logit > fc.LOGIT_OVERFLOW).any()
    assert (np.abs(logit) < 30).mean() >= 0.3  # the middle third keeps ordinary logits
    sigma = out[:, 0]
    tiny = np.finfo(np.float32).tiny
    assert ((sigma >= 0) & (sigma < tiny)).any()  # an exact 0 or a subnormal float
    assert np.isposinf(sigma).any()
    assert (np.isfinite(sigma) & (sigma >= tiny)).mean() >= 1 / 3
    assert np.isfinite(out[:, 1:]).all()  # only sigma saturates


@pytest.mark.parametrize("shape", RENDER_SHAPES)
def test_saturated_rays_cross_infinite_and_flushed_samples(oracle, shape):
    """the (37, 2, fixed) render of tests/test_gpu_field_regimes.py, first sub-sample of the first view: per-sample sigma from the oracle"""
    c = fc.case(oracle, "saturated", shape)
    f = _field(oracle, c)
    tms, scale, offset = util.hemisphere_transforms(oracle, util.fibonacci_hemisphere(6))
    cam = oracle.cameras_from_transforms(tms[[0, 3]], util.FOV_X, W, H, scale, offset)[0]
    lib = oracle.lib()
    n_inf = n_flushed = n_rays = 0
    tiny = np.finfo(np.float32).tiny
    for _, y, x, o, d in march_ref.rays(lib, cam, W, H, 1):
        _, ts, alphas, _, _ = march_ref.ray_samples(lib, f, o, d, 0, 37, march_ref.f32(1e-4))
        if not ts:
            continue
        p = np.array([[march_ref.fmaf(t, d[k], o[k]) for k in range(3)] for t in ts], np.float32)
        sigma = f.eval(p, np.tile(d, (len(p), 1)))[0][:, 0]
        n_rays += 1
        n_inf += bool(np.isposinf(sigma).any())
        n_flushed += bool((sigma < tiny).any())
        assert all(a == 1 for a, s in zip(alphas, sigma) if np.isposinf(s)) and all(a == 0 for a, s in zip(alphas, sigma) if s < tiny)
    f.close()
    assert n_rays > 50 and n_inf >= 1 and n_flushed >= 1, (n_rays, n_inf, n_flushed)


# ---- wide_mlp
def test_wide_mlp_overflows_the_narrowing_on_some_positions_only(oracle, name):
    c, pos, out, _ = _outputs(oracle, "wide_mlp", name)
    bad = ~np.isfinite(out).all(axis=1)
    assert bad.any() and (~bad).mean() >= 0.8
    # it is the narrowing that overflows: in float64, with nothing rounded to binary16 between the layers, every output is finite
    f = _field(oracle, c)
    ref = field_ref.evaluate(f.encode(pos), fc.directions(len(pos)), c.params[1], c.kw["density_bias"])
    f.close()
    assert np.isfinite(ref[:, 1:]).all()
    unit0 = np.maximum(f_unit0(c, oracle, pos), 0.0)
    assert np.array_equal(unit0 >= 65520.0, bad)  # exactly the positions whose unit 0 rounds to +Inf as a half


def f_unit0(c, oracle, pos):
    f = _field(oracle, c)
    x = f.encode(pos).view(np.float16).astype(np.float64)
    f.close()
    return (x @ field_ref.layers(c.params[1])[0][:, 0]).astype(np.float32).astype(np.float64)


# ---- the float64 reference
@pytest.mark.parametrize("kw", [util.SMALL, util.SMALL_F2], ids=["F4", "F2"])
def test_float64_reference_agrees_with_the_oracle_on_the_ordinary_field(oracle, kw):
    """tests/test_gpu_parity.py::test_field_eval's four bars, on its field (+-0.5 table) and its positions"""
    kw = dict(kw, table_amp=0.5)
    f = oracle.OracleField(oracle.desc(**kw), seed=util.SEED_A)
    rng = np.random.default_rng(2)
    pos = rng.random((2048, 3), dtype=np.float32)
    dirs = rng.standard_normal((2048, 3)).astype(np.float32)
    dirs /= np.linalg.norm(dirs, axis=1, keepdims=True)
    want, _ = f.eval(pos, dirs)
    got = field_ref.evaluate(f.encode(pos), dirs, f.params()[1], f.desc.density_bias)
    f.close()
    np.testing.assert_allclose(got[:, 4:20], want[:, 4:20], rtol=1e-3, atol=2e-3)
    np.testing.assert_allclose(got[:, 20:23], want[:, 20:23], rtol=1e-3, atol=2e-3)
    np.testing.assert_allclose(got[:, 0], want[:, 0], rtol=3e-3)
    np.testing.assert_allclose(got[:, 1:4], want[:, 1:4], rtol=1e-3, atol=1e-4)
    fig = field_ref.group_figures(field_ref.column_figures(want, got))
    print("FIELD_REF_FIGURES ordinary", {k: f"{v:.2e}" for k, v in fig.items()})
    assert max(fig.values()) < 2e-3  # the oracle's fp16 narrowing between the layers: 2^-11 per activation


def test_sh4_is_the_oracles(oracle):
    d = fc.directions(64)
    want = np.zeros((64, 16), np.float32)
    for i in range(64):
        oracle.lib().orc_sh4(d[i].ctypes.data_as(C.c_void_p), want[i].ctypes.data_as(C.c_void_p))
    np.testing.assert_allclose(field_ref.sh4(d), want, rtol=0, atol=1e-6)
