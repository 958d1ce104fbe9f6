"""The trainer's own ray marcher (train_rays_kernel / train_rays_patch_kernel: slab test, step-range bound, occupancy walk through
ballots) and its density refresh (density_refresh_fast_kernel / density_refresh_kernel) at their edges, against the CPU oracle
(oracle/prv_train.c).  Inputs: tests/train_cases.py; that they exercise what they claim: tests/test_train_cases_host.py.

Bars.  The ray batch is integers: sample count, ray count and the set of table entries the gradient touches are EQUAL.  Loss and
gradients: test_random_training_case's (1e-3).  The refreshed bitfield is EQUAL word for word wherever no cell's density is within
1e-4 of the threshold (a hundred times the 1e-6 by which the two sides' sigma differ), and the render that follows counts the
oracle's live samples on it.  Every trainer here is the product path (deterministic = 0)."""
import numpy as np
import pytest

from nerf_prv_amd import api
from tests import train_cases as tc

pytestmark = pytest.mark.gpu

SLOT, SLOT_REFRESH = 10, 11  # this module's own (tests/test_gpu_train.py and test_gpu_sweep.py train in slot 3)
# per level of the table gradient / per layer of the MLP gradient, against the oracle.  Measured over the sixteen random cases on
# the MI355X: worst 4.5e-5 (a level; worst layer 2.5e-5).  Twice that, one digit, would be 1e-4; the worst is below
# 5e-4, so the bar is the project's 1e-3
BLOCK_BAR = 1e-3


def _both(ctx, oracle, params, kw, ds, imgs, slot=SLOT, **opts):
    """the same field, cameras, images and options on both sides -> (oracle trainer, HIP trainer, camera set)"""
    f = oracle.OracleField(oracle.desc(**kw), params=params)
    ctx.load_model(slot, api.field_desc(**kw), *params)
    cams = ctx.cameras_from_matrices_intr(ds["tms"], ds["intr"], ds["scale"], ds["offset"])
    otr = oracle.OracleTrainer(f, oracle.train_opts(**opts), tc.oracle_cameras(oracle, ds), imgs)
    gtr = api.Trainer(ctx, slot, cams, ctx.torch.from_numpy(imgs), api.train_opts(**opts))
    return otr, gtr, cams


def _check_batch(otr, gtr, what, guard=False):
    """the batch is the oracle's (integers: equal), loss and gradients within test_random_training_case's bars -> the gradients"""
    want_loss, want_tg, want_mg = otr.gradients()
    loss, tg, mg = gtr.gradients()
    info = gtr.info()
    print(what, "samples", info["samples_last"], otr.samples_last, "rays", info["active_rays"], otr.active_rays, "loss", loss, want_loss,
          "rel_l2 table", tc.rel_l2(tg, want_tg), "mlp", tc.rel_l2(mg, want_mg))
    assert info["samples_last"] == otr.samples_last, what
    assert info["active_rays"] == otr.active_rays, what
    # the only witness of WHICH samples were listed: the entries their corners touch
    assert np.array_equal(tg != 0, want_tg.astype(np.float32) != 0), (what, int((tg != 0).sum()), int((want_tg.astype(np.float32) != 0).sum()))
    assert loss == pytest.approx(want_loss, rel=1e-3, abs=1e-7), what
    if otr.samples_last == 0:
        assert not tg.any() and not mg.any(), what
    elif np.abs(want_mg).max() > 1e-9:
        assert tc.rel_l2(mg, want_mg) < 1e-3 and tc.rel_l2(tg, want_tg) < 1e-3, what
    else:
        assert guard, what  # test_random_training_case's escape for a vanishing gradient: only where the caller allows it
    return (tg, mg), (want_tg, want_mg)


def _check_steps(otr, gtr, what, n=3):
    got, want = gtr.steps(n), [otr.step() for _ in range(n)]
    print(what, "losses", got, want)
    np.testing.assert_allclose(got, want, rtol=5e-3, atol=1e-9, err_msg=str(what))


def _awkward(ctx, oracle, name, **opts):
    ds = tc.awkward_datasets(oracle)[name]
    _, params = tc.awkward_field(oracle, name, dense="step_mode" not in opts)  # the fixed rule (and patches): the denser grid
    imgs = tc.awkward_images(name, len(ds["tms"]))
    if name == "away":
        opts["l2_reg"] = 0.0  # nothing may move: not even the MLP's weight decay
    otr, gtr, cams = _both(ctx, oracle, params, tc.TINY, ds, imgs, n_rays=64, occ_every=0, seed=ds["seed"], **opts)
    _check_batch(otr, gtr, (name, opts))
    if name == "away":  # every ray misses the cube: no sample, no gradient, and two steps leave the masters alone
        assert otr.samples_last == 0
        before = gtr.master()
        gtr.steps(2)
        after = gtr.master()
        assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1])
    else:
        assert otr.samples_last > 0
        _check_steps(otr, gtr, (name, opts))
    gtr.close()
    cams.close()


def test_the_case_module_restates_the_training_tests_intrinsics():
    from tests import test_gpu_train

    assert tc.LENS_INTR == test_gpu_train.INTR and tc.TINY == test_gpu_train.TINY


@pytest.mark.parametrize("rule", list(tc.RULES))
@pytest.mark.parametrize("name", tc.AWKWARD)
def test_awkward_cameras(ctx, oracle, name, rule):
    """cameras inside the cube (t0 = 0), axis-parallel rays (two zero direction components in the slab test), a far camera (t ~ 300:
    the step range in units of a step that is 50 float ulps wide), a camera looking away, grazing rays (t1 - t0 of a few steps: the
    bound `inside` against the exact `t < t1`), all of them in one set: the same batch as the oracle under both sampling rules"""
    _awkward(ctx, oracle, name, **tc.RULES[rule])


@pytest.mark.parametrize("patch", tc.PATCHES, ids=lambda p: f"{p[0]}x{p[1]}")
@pytest.mark.parametrize("name", tc.AWKWARD)
def test_awkward_cameras_with_patches(ctx, oracle, name, patch):
    """train_rays_patch_kernel has a slab test and an occupancy walk of its own: the same sets, rays drawn as 4 x 2 and 1 x 3 patches"""
    _awkward(ctx, oracle, name, n_samples=24, patch_w=patch[0], patch_h=patch[1])


@pytest.mark.parametrize("case_id", range(tc.N_RANDOM))
def test_random_engine_marcher_case(ctx, oracle, case_id):
    """the product's default rule on random fields and option sets: step caps around the 64-step ballot round, occupancy grids with
    no coarse grid and with a partial last word, sparse and single-cell occupancy, hemisphere and awkward cameras.  Besides the
    whole-vector bars: rel_l2 per table level and per MLP layer, which a whole-vector norm can hide"""
    case = tc.random_ngp_case(case_id)
    params, ds, imgs = tc.realise(oracle, case)
    otr, gtr, cams = _both(ctx, oracle, params, case["field"], ds, imgs, **case["opts"])
    (tg, mg), (want_tg, want_mg) = _check_batch(otr, gtr, case, guard=True)
    if otr.samples_last and np.abs(want_mg).max() > 1e-9:
        lv, at_l = tc.block_rel_l2(tg, want_tg, tc.level_ranges(oracle, oracle.desc(**case["field"])))
        ly, at_m = tc.block_rel_l2(mg, want_mg, tc.MLP_LAYERS)
        print("case", case_id, "worst per-level rel_l2", lv, "level", at_l, "worst per-layer rel_l2", ly, "layer", at_m)
        assert lv < BLOCK_BAR and ly < BLOCK_BAR, (case, lv, at_l, ly, at_m)
    _check_steps(otr, gtr, case)
    gtr.close()
    cams.close()


# ------------------------------------------------------------------ density refresh

_thresholds = {}


def _refresh_start(oracle, occ_res, F):
    """field, its parameters, the oracle's cell densities and the threshold tests/test_train_cases_host.py asserts the empty band for"""
    if (occ_res, F) not in _thresholds:
        f, params = tc.refresh_field(oracle, occ_res, F)
        sigma = tc.cell_sigma(oracle, f)
        _thresholds[(occ_res, F)] = (params, sigma, tc.place_threshold(sigma))
    return _thresholds[(occ_res, F)]


def _fast_forward(monkeypatch, fast):
    """PRV_TRAIN_FAST_FWD as the case wants it, whatever the caller's environment holds (read when a trainer is created)"""
    if fast is None:
        monkeypatch.delenv("PRV_TRAIN_FAST_FWD", raising=False)
    else:
        monkeypatch.setenv("PRV_TRAIN_FAST_FWD", fast)


def _refresh_trainers(ctx, oracle, monkeypatch, occ_res, F, fast, **opts):
    params, sigma, thresh = _refresh_start(oracle, occ_res, F)
    kw = dict(tc.REFRESH_FIELD, n_levels=32 // F, n_features=F, occ_res=occ_res)
    ds = tc.awkward_datasets(oracle)["inside_off_centre"]
    imgs = tc.awkward_images("inside_off_centre", len(ds["tms"]))
    _fast_forward(monkeypatch, fast)
    otr, gtr, cams = _both(ctx, oracle, params, kw, ds, imgs, slot=SLOT_REFRESH, n_rays=32, n_samples=8, occ_sigma_thresh=thresh, **opts)
    monkeypatch.delenv("PRV_TRAIN_FAST_FWD", raising=False)
    return kw, ds, sigma, thresh, otr, gtr, cams


def _assert_words(occ, want, n_cells, what):
    assert np.array_equal(occ, want), (what, int(np.unpackbits((occ ^ want).view(np.uint8)).sum()), "bits differ")
    if n_cells % 32:
        assert int(occ[-1]) >> (n_cells % 32) == 0, what  # the unused bits of the last word


@pytest.mark.parametrize("occ_res,F,fast", tc.refresh_cases())
def test_refresh_is_exact(ctx, oracle, monkeypatch, occ_res, F, fast):
    """one refresh from the same field, a threshold no density comes near: the bitfield is the oracle's word for word (27 and 4913
    cells: a partial last word), by both kernels and both template instances; and the slot renders with it.  The slot was loaded with
    one occupied corner cell, so the coarse grid (12, 20, 32; none at 3, 17) and the occupied box that the render path derived from
    THAT grid cover next to nothing: only a render that derives them again from the refreshed grid counts the oracle's live samples"""
    kw, ds, sigma, thresh, otr, gtr, cams = _refresh_trainers(ctx, oracle, monkeypatch, occ_res, F, fast, occ_every=0)
    otr.refresh_occupancy()
    gtr.refresh_occupancy()
    t16, m16, occ = ctx.export_model(SLOT_REFRESH, api.field_desc(**kw))
    want = otr.params()[2]
    n_cells = occ_res ** 3
    assert np.array_equal(tc.bits_of(want, n_cells), sigma > np.float32(thresh)) and 0.2 * n_cells <= tc.bits_of(want, n_cells).sum() <= 0.8 * n_cells
    loaded = _refresh_start(oracle, occ_res, F)[0][2]
    assert tc.bits_of(loaded, n_cells).sum() == 1 and tc.bits_of(want & ~loaded, n_cells).sum() >= 0.2 * n_cells - 1  # the start grid holds none of it
    _assert_words(occ, want, n_cells, (occ_res, F, fast))
    f = oracle.OracleField(oracle.desc(**kw), params=(t16, m16, occ))
    _, st = ctx.render(SLOT_REFRESH, cams, [0], api.engine_render_opts(tc.W, tc.H, 0, 1, 1e-4))
    live = f.march_count(tc.oracle_cameras(oracle, ds)[0], tc.W, tc.H, 0, step_mode=oracle.STEP_NGP)
    stale = oracle.OracleField(oracle.desc(**kw), params=(t16, m16, loaded)).march_count(tc.oracle_cameras(oracle, ds)[0], tc.W, tc.H, 0, step_mode=oracle.STEP_NGP)
    assert live > 0 and 2 * stale < live  # what the loaded grid's one cell would let through
    assert int(st.samples_live) == live, (occ_res, F, fast, int(st.samples_live), live)
    gtr.close()
    cams.close()


@pytest.mark.parametrize("occ_res,F,fast", [(17, 4, None), (17, 2, "0"), (12, 2, None), (12, 4, "0"), (3, 4, None), (3, 2, "0")])
def test_refresh_is_a_fixed_point_while_nothing_moves(ctx, oracle, monkeypatch, occ_res, F, fast):
    """lr = 0, a refresh after every step, decay 0.5: ema = max(ema / 2, sigma) = sigma every time, so the first refresh gives the
    oracle's bits (sigma > thresh) and the fifth gives them again.  A decay applied AFTER the max halves the EMA: other bits."""
    kw, ds, sigma, thresh, otr, gtr, cams = _refresh_trainers(ctx, oracle, monkeypatch, occ_res, F, fast, occ_every=1, occ_decay=0.5, lr=0.0)
    d, n_cells = api.field_desc(**kw), occ_res ** 3
    want = np.packbits(np.pad(sigma > np.float32(thresh), (0, -n_cells % 32)), bitorder="little").view(np.uint32)
    gtr.steps(1)
    first = ctx.export_model(SLOT_REFRESH, d)[2]
    _assert_words(first, want, n_cells, (occ_res, F, fast, "first refresh"))
    gtr.steps(4)
    assert gtr.info()["steps"] == 5
    _assert_words(ctx.export_model(SLOT_REFRESH, d)[2], first, n_cells, (occ_res, F, fast, "fifth refresh"))
    for _ in range(5):
        otr.step()
    assert np.array_equal(otr.params()[2], want)  # the oracle's rule has the same fixed point
    gtr.close()
    cams.close()


def test_a_negative_learning_rate_is_still_refused(ctx, oracle, monkeypatch):
    """lr = 0 is a setting (the fixed-point test above: steps run, nothing moves); lr < 0 and NaN are not"""
    params, _, thresh = _refresh_start(oracle, 3, 4)
    kw = dict(tc.REFRESH_FIELD, n_levels=8, n_features=4, occ_res=3)
    ds = tc.awkward_datasets(oracle)["axis"]
    ctx.load_model(SLOT_REFRESH, api.field_desc(**kw), *params)
    cams = ctx.cameras_from_matrices_intr(ds["tms"], ds["intr"], ds["scale"], ds["offset"])
    imgs = ctx.torch.from_numpy(tc.awkward_images("axis", 1))
    for lr in (-1e-3, float("nan")):
        with pytest.raises(api.PrvError) as e:
            api.Trainer(ctx, SLOT_REFRESH, cams, imgs, api.train_opts(n_rays=8, n_samples=8, lr=lr))
        assert e.value.code == api.L.PRV_E_INVALID
    tr = api.Trainer(ctx, SLOT_REFRESH, cams, imgs, api.train_opts(n_rays=8, n_samples=8, lr=0.0))
    before = tr.master()
    assert np.isfinite(tr.steps(2)).all()
    after = tr.master()
    assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1])
    tr.close()
    cams.close()


@pytest.mark.parametrize("fast", [None, "0"])
def test_refresh_decay_holds_cells_on(ctx, oracle, monkeypatch, fast):
    """the EMA doing what it exists for: 12 steps, a refresh every second one, densities falling -- cells that are on although their
    current density is below the threshold.  The two trainings differ by the f32 atomics' order: delta = the largest relative difference
    of the cell densities (the oracle's evaluation of both sides' final parameters); outside a band of 2 delta around the threshold
    the GPU's bits are the oracle's, and at least 15 of the cells that the decay alone holds on lie outside it and are on"""
    params, ds, imgs, opts = tc.ema_case(oracle)
    kw = tc.EMA_CASE["field"]
    _fast_forward(monkeypatch, fast)
    otr, gtr, cams = _both(ctx, oracle, params, kw, ds, imgs, **opts)
    monkeypatch.delenv("PRV_TRAIN_FAST_FWD", raising=False)
    gtr.steps(tc.EMA_CASE["steps"])
    for _ in range(tc.EMA_CASE["steps"]):
        otr.step()
    n_cells, thresh = kw["occ_res"] ** 3, np.float32(opts["occ_sigma_thresh"])
    t16, m16, occ = ctx.export_model(SLOT, api.field_desc(**kw))
    sigma_g = tc.cell_sigma(oracle, oracle.OracleField(oracle.desc(**kw), params=(t16, m16, occ)))
    sigma_o, ema_o = tc.cell_sigma(oracle, otr.field()), otr.ema()
    delta = float(np.max(np.abs(sigma_g.astype(np.float64) - sigma_o) / sigma_o))
    band = tc.in_band(ema_o, float(thresh), 2.0 * delta)
    held = (ema_o > thresh) & (sigma_o < thresh)
    got, want = tc.bits_of(occ, n_cells), tc.bits_of(otr.params()[2], n_cells)
    print("fast", fast, "delta", delta, "cells in the band", int(band.sum()), "of", n_cells, "held by the decay", int(held.sum()), "outside the band",
          int((held & ~band).sum()), "bits that differ outside the band", int((got != want)[~band].sum()))
    assert band.sum() <= 0.05 * n_cells  # more: a badly chosen case
    assert np.array_equal(got[~band], want[~band])
    assert (held & ~band & got).sum() >= 15
    gtr.close()
    cams.close()
