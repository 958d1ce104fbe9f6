"""The inference field kernels -- feature gather and blend, the MFMA MLP, the activations, and the colour, depth, entropy and
density-grid kernels built on them -- on the parameter regimes of tests/field_cases.py: a fresh table (mostly subnormal binary16),
binary16 edge words, a field whose density logits leave expf's normal range at both ends, an MLP whose hidden activations overflow
the narrowing to binary16, and a field that api.Trainer produced.  What each regime contains is asserted without a GPU in
tests/test_field_cases_host.py.

Bars.  Features: bit for bit with the oracle, Inf words included.  A fast instance, the generic one and a model with dense replicas:
identical bytes.  Field outputs: per output column the largest |value - float64 reference| over the positions divided by the
column's largest |reference| (tests/field_ref.py), once for the oracle and once for the GPU; the GPU's figure may be FIGURE_FACTOR
times the oracle's.  Sigma: SIGMA_RTOL against the oracle where the oracle's sigma is a normal float (`saturated`: the logit's own
bar, see test_field_outputs), 0 or that where it is subnormal or 0, +Inf where it is +Inf; and against exp of the GPU's own logit
at (2 |logit| + 2) 2^-24.  Pixels, depth, entropy, density grid and mesh: the existing bars of
tests/test_gpu_instances.py and tests/test_gpu_entropy.py.

Slots 8 (the case under test) and 9 (the trainer's) of the session context."""
import numpy as np
import pytest

from nerf_prv_amd import api
from tests import depth_ref, entropy_ref, field_ref, instances, march_ref, mesh_ref, util
from tests import field_cases as fc
from tests.test_gpu_entropy import _assert_entropy
from tests.test_gpu_instances import _opts, environment
from tests.test_gpu_mesh import grid_points
from tests.test_gpu_replica import PLAIN, expected_bytes

pytestmark = pytest.mark.gpu

SLOT, SLOT_TRAIN = 8, 9
W, H = 24, 20
MIN_T = 1e-4
THREADS = 16
UP = np.array([0.0, 0.0, 1.0], np.float32)
FEATURE_REGIMES = ["fresh", "edges", "trained"]
FIELD_REGIMES = ["fresh", "trained", "saturated", "wide_mlp"]
PIXEL_REGIMES = ["fresh", "trained", "saturated"]
PIXEL_SHAPES = ["F4_5", "F2_10"]
PIXEL_CONFIGS = [(37, 2, 0), (0, 1, 1)]  # fixed S with an odd count and two sub-samples; the engine's own rule
TINY = np.finfo(np.float32).tiny

# The GPU's figure against the oracle's.  Both narrow every hidden layer to binary16, which is nearly all of either's distance from
# the float64 reference; the GPU adds fp32 MFMA accumulation in another order and two one-ulp hardware functions (v_exp_f32,
# v_rcp_f32), which can move a hidden value across a binary16 rounding boundary the oracle's stayed below: twice the oracle's figure.
# Measured (MI355X, `FIELD_REGIME_FIGURES` lines of pytest -s, worst column of each group over the seven shapes; the oracle's and the
# GPU's figures agree to the digits shown, the largest difference between them is 1e-5 of either):
#   regime      density outputs   colour outputs   rgb
#   fresh       1.25e-3           9.60e-4          7.9e-5
#   trained     6.09e-3           1.79e-3          4.6e-4
#   saturated   4.19e-4           1.53e-3          2.0e-3
#   wide_mlp    4.19e-4           9.14e-4          3.4e-4
# No column needs more than the oracle's own figure: the factor is headroom for a rounding flip, not something these inputs use.
# Sigma against the oracle, worst relative error: fresh 2.9e-7, trained 4.9e-4, wide_mlp 2.6e-4, saturated 2.1e-2 (bar there
# 0.13 to 0.17 = twice the oracle's own distance from the float64 logit; see test_field_outputs).  Where the oracle's sigma is
# subnormal (172 to 233 positions per shape) the GPU returns 0 on every one: v_exp_f32 flushes (include/prv.h, density_bias).
FIGURE_FACTOR = 2.0
SIGMA_RTOL = 3e-3  # tests/test_gpu_parity.py::test_field_eval's: d(sigma) / sigma = d(logit)


# ---- the cases
@pytest.fixture(scope="module")
def trained(ctx, oracle):
    """-> get(name): the `trained` regime of a shape, trained once: prv_model_fresh at table_amp 1e-4, TRAIN_STEPS steps of
    api.Trainer on tests/test_gpu_train.py's lens scene (its options, and deterministic = 1: the same field on every run), export_model"""
    tms, intr, scale, offset, imgs = fc.train_scene(oracle)
    cams = ctx.cameras_from_matrices_intr(tms, intr, scale, offset)
    done = {}

    def get(name):
        if name not in done:
            kw = dict(fc.shape_kw(name), table_amp=fc.FRESH_AMP)
            d = api.field_desc(**kw)
            ctx.fresh_model(SLOT_TRAIN, d, util.SEED_A)
            tr = api.Trainer(ctx, SLOT_TRAIN, cams, ctx.torch.from_numpy(imgs),
                             api.train_opts(n_rays=1024, n_samples=24, occ_every=16, occ_sigma_thresh=0.01 * 24 / 3 ** 0.5, deterministic=1))
            losses = tr.steps(fc.TRAIN_STEPS)
            assert np.isfinite(losses).all() and np.mean(losses[-20:]) < 0.5 * np.mean(losses[:5])  # it did train
            params = ctx.export_model(SLOT_TRAIN, d)
            tr.close()
            assert fc.all_finite_params(params) and 0 < np.unpackbits(params[2].view(np.uint8)).sum()
            done[name] = fc.Case(kw, params)
        return done[name]

    yield get
    cams.close()
    ctx.synthetic_model(SLOT_TRAIN, api.field_desc(**util.SMALL), util.SEED_A)


@pytest.fixture(scope="module")
def install(ctx, oracle, trained):
    """-> put(regime, name, context, slot): loads the case, asserts the layout, returns (case, oracle field of the same words)"""
    fields = []

    def put(regime, name, c=ctx, slot=SLOT, no_pair=False, want_oracle=True):
        case = trained(name) if regime == "trained" else fc.case(oracle, regime, name)
        c.load_model(slot, api.field_desc(**case.kw), *case.params)
        instances.assert_layout(c.model_layout(slot), instances.MATRIX[name], no_pair=no_pair)
        if not want_oracle:
            return case, None
        fields.append(oracle.OracleField(oracle.desc(**case.kw), params=case.params))
        return case, fields[-1]

    yield put
    for f in fields:
        f.close()
    ctx.synthetic_model(SLOT, api.field_desc(**util.SMALL), util.SEED_A)


def _first_difference(a, b, pos, F):
    bad = np.argwhere(a != b)
    return len(bad) == 0, (f"{len(bad)} feature words differ, first at position {pos[bad[0][0]]!r}, level {bad[0][1] // F}: "
                           f"{a[tuple(bad[0])]:#06x} / {b[tuple(bad[0])]:#06x}" if len(bad) else "")


# ---- a. features, bit for bit
@pytest.mark.parametrize("name", fc.SHAPES)
@pytest.mark.parametrize("regime", FEATURE_REGIMES)
def test_features_bit_exact(ctx, install, regime, name):
    case, f = install(regime, name)
    pos = fc.regime_positions(regime, case.kw)
    got, want = ctx.debug_encode(SLOT, pos), f.encode(pos)
    same, msg = _first_difference(got, want, pos, case.kw["n_features"])
    assert same, msg
    if regime == "fresh":
        assert (fc.is_subnormal_half(got) | ((got & 0x7FFF) == 0)).mean() >= 0.25
    if regime == "edges":
        assert (got == 0x7C00).any() and (got == 0xFC00).any()  # the same Inf


# ---- b. a fast instance, the generic one and dense replicas: identical bytes
@pytest.fixture(scope="module")
def generic_ctx():
    with environment({"PRV_NO_PAIR": "1"}):
        other = api.Context(0)
    yield other
    other.close()


@pytest.mark.parametrize("name", instances.FAST)
@pytest.mark.parametrize("regime", FEATURE_REGIMES)
def test_fast_equals_generic_features_and_field(ctx, install, generic_ctx, regime, name):
    case, _ = install(regime, name, want_oracle=False)
    with environment({"PRV_NO_PAIR": "1"}):
        install(regime, name, generic_ctx, 0, no_pair=True, want_oracle=False)
    assert instances.MATRIX[name].instance != 0
    pos = fc.regime_positions(regime, case.kw)
    dirs = fc.directions(len(pos))
    same, msg = _first_difference(ctx.debug_encode(SLOT, pos), generic_ctx.debug_encode(0, pos), pos, case.kw["n_features"])
    assert same, msg
    (fa, oa), (fb, ob) = ctx.debug_field(SLOT, pos, dirs), generic_ctx.debug_field(0, pos, dirs)
    assert np.array_equal(oa, ob)
    bad = np.argwhere(fa.view(np.uint32) != fb.view(np.uint32))
    assert len(bad) == 0, f"{len(bad)} field outputs differ, first at position {pos[bad[0][0]]!r}, output {bad[0][1]}: {fa[tuple(bad[0])]!r} / {fb[tuple(bad[0])]!r}"


@pytest.mark.parametrize("regime", ["fresh", "edges"])
def test_replicas_equal_the_hashed_levels(ctx, install, regime):
    """F4_5 with its three hashed levels read from dense replicas (PRV_REPLICA_LEVELS, read when the model is installed)"""
    name = "F4_5"
    case = None
    feats = {}
    for n in (0, 3):
        with environment(dict(PLAIN, PRV_REPLICA_LEVELS=str(n))):
            c = api.Context(0)
            try:
                case, _ = install(regime, name, c, 0, want_oracle=False)
                assert api.replica_layout(c, 0) == (n, expected_bytes(case.kw, n))
                pos = fc.regime_positions(regime, case.kw)
                feats[n] = c.debug_encode(0, pos)
            finally:
                c.close()
    same, msg = _first_difference(feats[3], feats[0], pos, 4)
    assert same, msg
    case, _ = install(regime, name, want_oracle=False)
    same, msg = _first_difference(feats[3], ctx.debug_encode(SLOT, pos), pos, 4)
    assert same, msg


# ---- c. field outputs
@pytest.mark.parametrize("name", fc.SHAPES)
@pytest.mark.parametrize("regime", FIELD_REGIMES)
def test_field_outputs(ctx, install, regime, name):
    case, f = install(regime, name)
    pos = fc.regime_positions(regime, case.kw)
    dirs = fc.directions(len(pos))
    got, gocc = ctx.debug_field(SLOT, pos, dirs)
    want, wocc = f.eval(pos, dirs)
    assert np.array_equal(gocc, wocc)
    # non-finite outputs: the same columns of the same positions
    cols = np.r_[0:23]
    for kind in (np.isnan, np.isposinf, np.isneginf):  # the same NaN, the same Inf of the same sign
        assert np.array_equal(kind(got[:, cols]), kind(want[:, cols])), kind.__name__
    rows = np.isfinite(want[:, 1:23]).all(axis=1)
    if regime == "wide_mlp":
        assert (~rows).any() and rows.mean() >= 0.8
    else:
        assert rows.all()
    ref = field_ref.evaluate(f.encode(pos), dirs, case.params[1], case.kw["density_bias"])
    fo, fg = field_ref.column_figures(want, ref, rows), field_ref.column_figures(got, ref, rows)
    go, gg = field_ref.group_figures(fo), field_ref.group_figures(fg)
    print(f"FIELD_REGIME_FIGURES {regime} {name}: " + "  ".join(f"{k} oracle {go[k]:.2e} gpu {gg[k]:.2e}" for k in go))
    # sigma
    ws, gs = want[rows, 0], got[rows, 0]
    normal, inf = np.isfinite(ws) & (ws >= TINY), np.isposinf(ws)
    with np.errstate(invalid="ignore"):
        rel = np.abs(gs[normal].astype(np.float64) - ws[normal]) / ws[normal]
    print(f"FIELD_REGIME_SIGMA {regime} {name}: worst relative error {rel.max():.2e} over {normal.sum()} normal, {inf.sum()} infinite, "
          f"{(~normal & ~inf).sum()} subnormal or zero (GPU zero on {(gs[~normal & ~inf] == 0).sum()})")
    for k in range(1, 23):
        assert fg[k] <= FIGURE_FACTOR * fo[k], f"output {k}: GPU {fg[k]:.3e} of the column's range from the float64 reference, oracle {fo[k]:.3e}"
    # d(sigma) / sigma = d(logit), and the logit is output 4, which the oracle itself has within fo[4] of its range from the float64
    # reference: where that is more than SIGMA_RTOL (saturated: the last layer's column is scaled ~100-fold, one binary16 step of
    # one hidden unit moves the logit by up to 2e-2) sigma cannot be held closer to the oracle than the logit is held
    sigma_rtol = max(SIGMA_RTOL, FIGURE_FACTOR * fo[4] * np.abs(ref[rows, 4]).max()) if regime == "saturated" else SIGMA_RTOL
    print(f"FIELD_REGIME_SIGMA {regime} {name}: bar {sigma_rtol:.2e}")
    # fast_exp alone, apart from the logit's noise: the GPU's sigma against exp of the GPU's OWN logit in float64.  The kernel rounds
    # out0 + bias and its product with log2(e) to float32 (2^-24 |logit| each, relative to sigma) and v_exp_f32 is good to one ulp
    logit = got[rows, 4].astype(np.float64) + np.float64(np.float32(case.kw["density_bias"]))
    mine = np.exp(logit[normal])
    ok = (mine >= 2 * TINY) & (mine <= np.finfo(np.float32).max / 2)  # (clear of the flush and of the overflow)
    own = np.abs(gs[normal][ok].astype(np.float64) - mine[ok]) / mine[ok] / ((2.0 * np.abs(logit[normal][ok]) + 2.0) * 2.0 ** -24)
    print(f"FIELD_REGIME_EXP {regime} {name}: sigma against exp(own logit), worst error {own.max():.2f} of (2 |logit| + 2) 2^-24 over {ok.sum()} positions")
    assert own.max() <= 1.0
    assert rel.max() <= sigma_rtol
    assert np.isposinf(gs[inf]).all()
    low = ~normal & ~inf
    assert ((gs[low] == 0) | (np.abs(gs[low].astype(np.float64) - ws[low]) <= sigma_rtol * ws[low])).all()
    if regime == "saturated":
        assert inf.any() and low.any() and normal.mean() >= 1 / 3


# ---- d. pixels
@pytest.fixture(scope="module")
def cams(ctx, oracle):
    tms, scale, offset = util.hemisphere_transforms(oracle, util.fibonacci_hemisphere(6))
    tms = tms[[0, 3]]
    cs = ctx.cameras_from_matrices(tms, util.FOV_X, W, H, scale, offset)
    yield cs, oracle.cameras_from_transforms(tms, util.FOV_X, W, H, scale, offset)
    cs.close()


# The finding of this module.  Training pushes empty space to sigma dt of about 2^-25, where
# alpha = 1 - exp(-sigma dt) is 0 or one ulp of 1 (2^-24) depending on the last bit of the exponential: v_exp_f32 and expf agree to one
# ulp and differ by a whole alpha on such a sample.  A pixel whose rays hold n live samples with an oracle alpha below FLOOR_ALPHA
# can therefore differ by n 2^-24 / spp in alpha for no fault of either side; where that alone is more than FLOOR_SHARE of the
# pixel's bar, or where EVERY live sample of the pixel is such a sample (it is exactly 0 or not by one ulp), the pixel is a FLOOR PIXEL
# (nearly transparent rays through trained empty space; found on the CPU from the oracle's per-sample alphas).  test_colour_and_depth holds every other pixel of a `trained` view to every check and the floor pixels to
# finiteness, identity and the sample counts; test_trained_floor_pixels holds the floor pixels to the pixel bars and the
# exact-zero depth mask, and is a strict xfail.  147 to 254 of a view's 480 pixels are floor pixels; the others meet colour within
# 1.3e-4 and depth within 1.9e-4 of the bar's 1e-3.  Measured on the MI355X over ALL pixels (deterministic training, first view):
#   trained-F4_5-S37spp2   7 pixels whose depth is exactly 0 on one side only (colour 7.6e-5, depth 9.6e-5 of the bar's 1e-3)
#   trained-F4_5-ngp       8 such pixels (colour 6.1e-4, depth 8.3e-4)
#   trained-F2_10-S37spp2  13 such pixels (colour 1.4e-4, depth 1.9e-4)
#   trained-F2_10-ngp      alpha 2.6464462e-05 against the oracle's 3.0517578e-05 at pixel (5, 16): 1.034e-3 relative to the floor
# The cure is alpha = -expm1(-sigma dt) in the kernels and the oracle together; it moves every pixel's last bits and the headline
# digests with them.  fresh and saturated have no floor pixel by definition and pass every check on every pixel.
FLOOR_ALPHA = 2.0 ** -20  # one ulp of 1 is a sixteenth of it or more
FLOOR_SHARE = 0.25
ALPHA_AT_ONE_ULP = ("alpha = 1 - exp(-sigma dt) at one ulp of 1 in trained empty space: v_exp_f32 and expf differ by a whole alpha per sample; "
                    "nearly transparent pixels with depth exactly 0 on one side only (7 to 13 per view), one alpha 1.034e-3 from the oracle's; "
                    "cure (-expm1 in kernels and oracle) moves the digests")
PIXEL_CASES = [pytest.param(r, n, *c, id=f"{r}-{n}-{i}") for r in PIXEL_REGIMES for n in PIXEL_SHAPES for c, i in zip(PIXEL_CONFIGS, ["S37spp2", "ngp"])]


def _floor_pixels(oracle, f, oc, S, spp, mode, alpha_image):
    """(H, W) bool: see above"""
    lib, n, n_live = oracle.lib(), np.zeros((H, W)), np.zeros((H, W))
    for _, y, x, o, d in march_ref.rays(lib, oc, W, H, spp):
        alphas = march_ref.ray_samples(lib, f, o, d, mode, S, march_ref.f32(MIN_T))[2]
        n[y, x] += sum(1 for a in alphas if a < FLOOR_ALPHA)
        n_live[y, x] += len(alphas)
    return (n * 2.0 ** -24 / spp > FLOOR_SHARE * util.PIX_RTOL * np.maximum(alpha_image, util.PIX_FLOOR)) | ((n == n_live) & (n > 0))


@pytest.fixture(scope="module")
def pixel_runs(ctx, oracle, install, cams):
    """-> run(regime, name, S, spp, mode): the render, and per view the GPU's (H, W, 5), the oracle's render, the depth reference and the
    floor pixels; every check that does not look at pixel values is made here.  Computed once per case."""
    done = {}

    def run(regime, name, S, spp, mode):
        key = (regime, name, S, spp, mode)
        if key not in done:
            case, f = install(regime, name)
            cs, ocams = cams
            rgba, depth, st, plain, st0 = depth_ref.both(ctx, SLOT, cs, _opts(W, H, S, spp, mode))
            depth_ref.check_identity(rgba, st, plain, st0)
            assert np.isfinite(rgba).all() and np.isfinite(depth).all()  # every output float
            assert depth.shape == (len(ocams), H, W) and depth.dtype == np.float32
            views, live = [], 0
            for v, oc in enumerate(ocams):
                want, _ = f.render(oc, W, H, S, spp, MIN_T, threads=THREADS, step_mode=mode)
                live += f.march_count(oc, W, H, S, spp, threads=THREADS, step_mode=mode)
                ref = depth_ref.reference(oracle, f, oc, W, H, S, spp, MIN_T, mode)  # (its colour is the oracle's render to 1e-6)
                floor = _floor_pixels(oracle, f, oc, S, spp, mode, want[..., 3]) if regime == "trained" else np.zeros((H, W), bool)
                views.append((np.concatenate([rgba[v], depth[v][..., None]], axis=-1), want, ref, floor))
            assert int(st.samples_live) == live > 0
            assert (rgba[..., 3] > 0).any() and (depth > 0).any()
            done[key] = views
        return done[key]

    return run


def _check_pixels(tag, got, want, ref, rows):
    """the pixels `rows` of one view: colour against the oracle's render, colour and depth against the restatement, the zero-depth mask"""
    one = ((got[..., 4] == 0) != (ref[..., 4] == 0)) & rows
    print(f"PIXEL_FIGURES {tag}: {int(rows.sum())} pixels; colour against the oracle, worst relative error {util.pixel_rel_err(got[rows][:, :4], want[rows]).max():.3e}; "
          f"depth against the restatement {util.pixel_rel_err(got[rows][:, 4], ref[rows][:, 4]).max():.3e}; depth 0 on one side only on {int(one.sum())}")
    util.assert_pixels_close(got[rows][:, :4], want[rows])
    util.assert_pixels_close(got[rows], ref[rows])
    assert not one.any()  # misses and dead rays: exactly 0


@pytest.mark.parametrize("regime,name,S,spp,mode", PIXEL_CASES)
def test_colour_and_depth(pixel_runs, regime, name, S, spp, mode):
    for v, (got, want, ref, floor) in enumerate(pixel_runs(regime, name, S, spp, mode)):
        keep = ~floor
        if regime == "trained":
            lit = want[..., 3] > util.PIX_FLOOR
            assert floor.any() and not (floor & (want[..., 3] > 0.1)).any()  # floor pixels are nearly transparent ones
            assert (keep & lit).sum() >= 20, "a trained view must keep pixels that show the object"
        else:
            assert keep.all()
        _check_pixels(f"{regime} {name} {S}/{spp}/{mode} view {v}", got, want, ref, keep)


@pytest.mark.xfail(strict=True, raises=AssertionError, reason=ALPHA_AT_ONE_ULP)
@pytest.mark.parametrize("name", PIXEL_SHAPES)
def test_trained_floor_pixels(pixel_runs, name):
    """the floor pixels of the `trained` views, both configurations of a shape together, at the bars every other pixel meets"""
    checked = 0
    for (S, spp, mode), cid in zip(PIXEL_CONFIGS, ["S37spp2", "ngp"]):
        for v, (got, want, ref, floor) in enumerate(pixel_runs("trained", name, S, spp, mode)):
            checked += int(floor.sum())
            if floor.any():
                _check_pixels(f"trained {name} {cid} view {v} FLOOR PIXELS", got, want, ref, floor)
    assert checked > 0


def test_entropy_of_the_saturated_field(ctx, oracle, install, cams):
    """weights that are exactly 0 (flushed sigma) and exactly T (infinite sigma): h(p) counts a denormal p as 0"""
    case, f = install("saturated", "F4_5")
    cs, ocams = cams
    S, spp, mode = 37, 2, 0
    ent, alpha, st = ctx.render_entropy(SLOT, cs, None, _opts(W, H, S, spp, mode))
    ent, alpha = ent.cpu().numpy(), alpha.cpu().numpy()
    assert np.isfinite(ent).all() and np.isfinite(alpha).all()
    for v, oc in enumerate(ocams):
        want = entropy_ref.reference(oracle, f, oc, W, H, S, spp, MIN_T, mode)
        _assert_entropy(f"saturated/F4_5/view{v}", ent[v], alpha[v], want)
    assert (ent > 0).any()


# ---- e. density grid and mesh
@pytest.mark.parametrize("name", fc.SHAPES)
@pytest.mark.parametrize("regime", ["saturated", "fresh"])
def test_density_grid_and_mesh(ctx, install, regime, name):
    case, _ = install(regime, name, want_oracle=False)
    res = (17, 23, 30)
    grid = ctx.density_grid(SLOT, res).cpu().numpy()
    assert grid.shape == (res[2], res[1], res[0]) and grid.dtype == np.float32
    pts = grid_points(res, None)
    want, _ = ctx.debug_field(SLOT, pts, np.tile(UP, (len(pts), 1)))
    assert np.array_equal(grid.ravel().view(np.uint32), want[:, 0].view(np.uint32))
    assert not np.isnan(grid).any()
    if regime == "saturated":
        assert np.isposinf(grid).any() and (grid == 0).any()
    thr = float(np.median(grid))
    assert np.isfinite(thr)
    m = ctx.marching_cubes(SLOT, res, threshold=thr)
    try:
        v, n, t = mesh_ref.marching_cubes(grid, threshold=thr)
        assert len(t) > 100
        assert np.isfinite(m.vertices).all()
        assert np.array_equal(m.triangles, t)
        assert np.array_equal(m.vertices.view(np.uint32), v.view(np.uint32))
    finally:
        m.close()
