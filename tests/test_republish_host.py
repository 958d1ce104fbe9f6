"""CPU checks of tests/republish_cases.py: the oracle alone shows that every change moves what it claims to move, before a GPU sees it.
These are conditions on the inputs, not tolerances on the code.

steps_shrink (64 steps, 192 rays x 24 samples, lr 1e-2, a refresh every 16 steps, threshold 2, decay 0.5) and refresh_grow (one corner
cell, one refresh at train_cases.place_threshold's threshold), per shape:
  * the occupied cells' box moves by a cell or more on an axis: it shrinks in steps_shrink, grows in refresh_grow;
  * a quarter of the occupancy words differ;
  * steps_shrink: half of the table scalars that received a gradient in step 0, 16, 32 or 48, and half of the MLP halfs, changed their fp16 bits;
  * of the pixels that are non-zero in either of the oracle's renders before and after (views 0 and 3 of the five, 37 samples a ray),
    10 % differ by more than the pixel bar 1e-3 max(|want|, 1/255).

Measured with the oracle (box as lo..hi in cells, x y z; the box before is 0..15 on every axis in steps_shrink, cell 0 in refresh_grow):
  steps_shrink   box after          words  table scalars with a gradient / of them changed   MLP changed   pixels
    F4_5         2..15 2..14 0..15  1.00   0.355 / 0.998                                     1.000         1.00
    F4_3         2..15 0..15 0..13  1.00   0.842 / 0.999                                     1.000         1.00
    F2_10        2..15 0..15 0..13  1.00   0.668 / 0.999                                     1.000         1.00
    F2_6         2..15 1..15 0..15  1.00   0.943 / 0.999                                     1.000         1.00
    F4_0         2..15 1..15 0..13  1.00   0.688 / 0.999                                     1.000         1.00
    F2_0         2..14 1..14 1..14  1.00   0.840 / 0.999                                     1.000         1.00
    F4_5, engine's marcher (40 rays, lr 2e-2, refreshes at 30 and 60, threshold 5): 3..13 2..13 1..12, words 1.00, table 0.999, MLP 1.000,
    pixels 1.00
  refresh_grow: box after 0..15 on every axis, pixels 1.00 for all eight; words 1.00 (R4: 0.98); cells on of 4096: F4_5 1318, F4_3 1012,
    F2_10 831, F2_6 931, F4_0 1055, F2_0 3233, R4 1018, R2 3203
The planes x = 0 and x = 1 go off in every shape (and under decay 0, and at 48 steps): the condition does not hang on one cell.

The consumer table is checked against nerf_prv_amd.api.Context: every public method with a `slot` or `slots` parameter, or whose
source calls a function of include/prv.h that takes a model slot (whatever the wrapper names its argument), is the method of a
consumer, or stands in republish_cases.EXEMPT with its reason (the installers, which are the reinstall changes themselves; the file
readers and writers, which end in load_model's and export_model's paths; model_desc, which returns what install stored)."""
import numpy as np
import pytest

from tests import republish_cases as rc, train_cases as tc, util

_cache = {}


def _train(oracle, name, spec):
    """-> (before, after, touched table scalars) of the oracle's steps_shrink"""
    key = (name, spec["opts"]["n_rays"])
    if key not in _cache:
        kw = rc.train_kw(name)
        ds, imgs = rc.training_scene(oracle, kw)
        before = rc.all_occupied(oracle, kw)
        f = oracle.OracleField(oracle.desc(**kw), params=before)
        otr = oracle.OracleTrainer(f, oracle.train_opts(**spec["opts"]), tc.oracle_cameras(oracle, ds), imgs)
        touched = np.zeros(len(before[0]), bool)
        for k in range(spec["steps"]):
            if k % 16 == 0:
                touched |= otr.gradients()[1] != 0  # the batch of the step to come; nothing moves
            otr.step()
        _cache[key] = (kw, before, otr.params(), touched)
    return _cache[key]


def _pixel_share(oracle, kw, before, after):
    ocams = rc.oracle_cameras(oracle)
    diff = live = 0
    for v in (0, 3):
        imgs = []
        for p in (before, after):
            f = oracle.OracleField(oracle.desc(**kw), params=p)
            imgs.append(f.render(ocams[v], rc.W, rc.H, rc.FIXED_S, 1, rc.MIN_T)[0])
            f.close()
        a, b = imgs
        nz = (a != 0).any(-1) | (b != 0).any(-1)
        diff += int((util.pixel_rel_err(b, a).max(-1)[nz] > util.PIX_RTOL).sum())
        live += int(nz.sum())
    assert live > 200
    return diff / live


@pytest.mark.parametrize("name", rc.SHAPES)
def test_steps_shrink_changes_everything(oracle, name):
    kw, before, after, touched = _train(oracle, name, rc.STEPS_SHRINK)
    b0, b1 = rc.assert_occupancy_preconditions(before[2], after[2], kw["occ_res"], "shrink")
    table_share = float(np.mean(before[0][touched] != after[0][touched]))
    mlp_share = float(np.mean(before[1] != after[1]))
    pix = _pixel_share(oracle, kw, before, after)
    print(name, "box", b1[0], b1[1], "words", rc.words_changed(before[2], after[2]), "touched", float(touched.mean()), "table", table_share, "mlp", mlp_share,
          "pixels", pix)
    assert touched.sum() > 1000 and table_share >= 0.5 and mlp_share >= 0.5
    assert pix >= 0.10


def test_steps_shrink_under_the_engines_marcher(oracle):
    kw, before, after, touched = _train(oracle, "F4_5", rc.STEPS_SHRINK_NGP)
    b0, b1 = rc.assert_occupancy_preconditions(before[2], after[2], kw["occ_res"], "shrink")
    table_share, mlp_share = float(np.mean(before[0][touched] != after[0][touched])), float(np.mean(before[1] != after[1]))
    pix = _pixel_share(oracle, kw, before, after)
    print("ngp box", b1[0], b1[1], "words", rc.words_changed(before[2], after[2]), "table", table_share, "mlp", mlp_share, "pixels", pix)
    assert table_share >= 0.5 and mlp_share >= 0.5
    assert pix >= 0.10


@pytest.mark.parametrize("name", rc.SHAPES + list(rc.REFRESH_OWN))
def test_refresh_grow_changes_the_occupancy_alone(oracle, name):
    kw, before, thresh = rc.refresh_start(oracle, name)
    f = oracle.OracleField(oracle.desc(**kw), params=before)
    ds, imgs = rc.training_scene(oracle, kw)
    otr = oracle.OracleTrainer(f, oracle.train_opts(**rc.refresh_opts(thresh)), tc.oracle_cameras(oracle, ds), imgs)
    otr.refresh_occupancy()
    after = otr.params()
    assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1])
    b0, b1 = rc.assert_occupancy_preconditions(before[2], after[2], kw["occ_res"], "grow")
    assert np.all(b0[1] == 0) and np.all(b1[1] - b1[0] >= 12)  # one cell -> most of the cube
    sigma = tc.cell_sigma(oracle, f)
    assert not tc.in_band(sigma, thresh, tc.BAND).any()  # no cell near the threshold: the GPU's bits are these
    pix = _pixel_share(oracle, kw, before, after)
    print(name, "box", b1[0], b1[1], "words", rc.words_changed(before[2], after[2]), "on", int(tc.bits_of(after[2], 4096).sum()), "pixels", pix)
    assert pix >= 0.10


@pytest.mark.parametrize("name", rc.SHAPES)
def test_reinstall_changes_everything(oracle, name):
    kw = rc.install_kw(name)
    before, after = rc.synthetic(oracle, kw, util.SEED_A), rc.synthetic(oracle, kw, util.SEED_B)
    after = (after[0], after[1], rc.upper_half(kw["occ_res"]))
    assert rc.occupied_box(before[2], kw["occ_res"])[0][2] < kw["occ_res"] // 2 == rc.occupied_box(after[2], kw["occ_res"])[0][2]
    assert rc.words_changed(before[2], after[2]) >= 0.25
    assert np.mean(before[0] != after[0]) >= 0.5 and np.mean(before[1] != after[1]) >= 0.5


def test_every_slot_method_of_the_context_is_a_consumer_or_exempt():
    from nerf_prv_amd import api

    methods = rc.slot_methods(api.Context)
    assert len(methods) >= 20 and {"render", "score_views", "marching_cubes", "load_model"} <= set(methods)
    consumed = {c.method for c in rc.CONSUMERS.values()}
    assert consumed <= set(methods), consumed - set(methods)  # a consumer names a method that exists and takes a slot
    assert not consumed & set(rc.EXEMPT)
    missing = [m for m in methods if m not in consumed and m not in rc.EXEMPT]
    assert not missing, f"api.Context.{missing} take a model slot: add them to republish_cases.CONSUMERS, or to EXEMPT with a reason"
    assert set(rc.EXEMPT) <= set(methods) and all(len(r) > 20 for r in rc.EXEMPT.values())
    assert all(set(c.reads) <= set("tmo") for c in rc.CONSUMERS.values())
    assert sorted(rc.SINGLE + rc.MEMBERS) == sorted(rc.CONSUMERS)
    assert rc.dirty_order(rc.SINGLE)[:2] == ["first_hit", "precept"] and sorted(rc.dirty_order(rc.SINGLE)) == sorted(rc.SINGLE)


def test_the_gpu_modules_cases_cover_the_table():
    """the case list of tests/test_gpu_republish.py (importing it needs no GPU): every shape under every change, every consumer"""
    from tests import instances, test_gpu_republish as g

    assert sorted(rc.SINGLE) == sorted(g.CASES[g.SINGLE_CASES[0]].consumers) and sorted(rc.MEMBERS) == sorted(g.CASES[g.MEMBER_CASES[0]].consumers)
    assert {c.shape for c in g.CASES.values() if c.change == "steps_shrink" and not c.env} == set(rc.SHAPES)
    assert {c.shape for c in g.CASES.values() if c.change == "refresh_grow"} == set(rc.SHAPES) | set(rc.REFRESH_OWN)
    assert {c.shape for c in g.CASES.values() if c.change == "reinstall_same_shape"} == set(rc.SHAPES)
    assert set(g._POLICY) == set(instances.FAST)
    assert {instances.MATRIX[k].instance != 0 for k in rc.ROUND_SHAPES} == {True, False}
