"""Every consumer of a model slot sees the slot's new state after it changed (tests/republish_cases.py: the shapes, the changes, the
consumer table).  Per (shape, change), in this order: the state before is installed, every consumer runs once on it (the context's
scratch buffers, cull rectangles, queues, interleaved occupancy and the slot's derived state now hold the old state), the change is
applied, every consumer runs again, the slot is exported, and a fresh api.Context loaded with the exported arrays runs every consumer.

  * after the change == the fresh context: identical bytes of every array a consumer returns (images, planes, records, samples_live and
    samples_evaluated, mesh arrays, features, voxel ids, chosen views and gains), no tolerance;
  * after the change != before it, for every consumer that reads an array the change wrote (republish_cases.CHANGED / Consumer.reads:
    refresh_grow writes the occupancy alone, so debug_encode and marching cubes without the occupancy must return the OLD bytes;
    model_layout is the descriptor's and moves with reinstall_other_shape only);
  * the export equals the trainer's masters rounded to fp16 and its own second call; the GPU's own arrays meet the box and word
    conditions of tests/test_republish_host.py (a failure, never a skip);
  * colour, and depth, after steps_shrink equal the oracle's render of the exported field at util.assert_pixels_close_any's bar: the two
    contexts cannot be wrong together.

In that order the first consumer after the change rebuilds the slot's derived state for all the others.  The `round` tests give every
consumer a change of its own instead (republish_cases.ROUND: a live trainer, four steps and a refresh before each consumer's second
run, on two fast and the two generic shapes, and on five members): each entry point meets a slot that is dirty when it is called.
Run once against a library whose density_grid, debug_encode and debug_field asked only whether the slot is loaded, these tests failed
for exactly those three on all four shapes, and the batched tests above did not.  first_hit and precept without the rebuild still pass,
and rightly: their kernel (first_hit_dda) reads the canonical occupancy words, which the trainer writes in place, and no derived state;
the same holds for export_model.

The render policies (PRV_MERGE_MAX, PRV_POOL, PRV_CELL_CACHE) and PRV_MARCH_MULTI are read when a context is created: those cases run in
a context of their own made under tests.test_gpu_instances.environment, and their fresh context is made under it too.

Slots of the session context: 38 (the slot under test) and 8, 9, 39, 47, 49 (the ensemble's members); they end as util.SMALL fields."""
import numpy as np
import pytest

from nerf_prv_amd import api
from tests import depth_ref, instances, march_ref, republish_cases as rc, util
from tests.test_gpu_instances import environment

pytestmark = pytest.mark.gpu

SLOT = 38
MEMBER_SLOTS = [8, 9, 39, 47, 49]
_scenes = {}


def _scene(oracle, kw):
    key = tuple(sorted(kw.items()))
    if key not in _scenes:
        _scenes[key] = rc.training_scene(oracle, kw)
    return _scenes[key]


class Trained:
    """a loaded slot with a live trainer on it"""

    def __init__(self, c, oracle, slot, kw, params, opts):
        ds, imgs = _scene(oracle, kw)
        self.c, self.slot, self.kw, self.params = c, slot, kw, params
        c.load_model(slot, api.field_desc(**kw), *params)
        self.cams = c.cameras_from_matrices_intr(ds["tms"], ds["intr"], ds["scale"], ds["offset"])
        self.tr = api.Trainer(c, slot, self.cams, c.torch.from_numpy(imgs), api.train_opts(**opts))

    def finish(self):
        self.master = self.tr.master()
        self.tr.close()
        self.cams.close()


# ---- the changes: before(c, oracle) installs the old state -> state; change(c, oracle, state) applies it
def _steps_before(name, spec, slot=SLOT, member=0):
    def before(c, oracle):
        kw = rc.train_kw(name)
        field_seed, train_seed = rc.member_seeds(member)
        return [Trained(c, oracle, slot, kw, rc.all_occupied(oracle, kw, field_seed), dict(spec["opts"], seed=train_seed))]
    return before


def _steps_change(spec):
    def change(c, oracle, state):
        if len(state) == 1:
            assert np.isfinite(state[0].tr.steps(spec["steps"])).all()
        else:
            assert np.isfinite(api.train_many([s.tr for s in state], spec["steps"])).all()
        for s in state:
            s.finish()
    return change


def _refresh_before(name):
    def before(c, oracle):
        kw, params, thresh = rc.refresh_start(oracle, name)
        return [Trained(c, oracle, SLOT, kw, params, rc.refresh_opts(thresh))]
    return before


def _refresh_change(c, oracle, state):
    state[0].tr.refresh_occupancy()
    state[0].finish()


def _install(c, oracle, kw, seed, occ=None):
    t, m, o = rc.synthetic(oracle, kw, seed)
    c.load_model(SLOT, api.field_desc(**kw), t, m, o if occ is None else occ)


def _reinstall_before(names, same):
    """names[:-1] in turn over the slot (its buffers carry that history), names[-1] is the change"""
    def before(c, oracle):
        for k, name in enumerate(names[:-1]):
            _install(c, oracle, rc.install_kw(name) if same else _reshape_kw(name), util.SEED_A + k)
        return []
    return before


def _reshape_kw(name):
    return rc.train_kw(name) if name == "F2_10" else rc.install_kw(name)  # the middle one with another occupancy resolution too


def _reinstall_change(names, same):
    def change(c, oracle, state):
        kw = rc.install_kw(names[-1]) if same else _reshape_kw(names[-1])
        _install(c, oracle, kw, util.SEED_B if same else util.SEED_A + len(names) - 1, rc.upper_half(kw["occ_res"]) if same else None)
        assert not same or kw == rc.install_kw(names[0])
    return change


class Case:
    def __init__(self, change, shape, before, apply, slots=(SLOT,), consumers=None, env=None, direction=None):
        self.change, self.shape, self.before, self.apply, self.slots, self.env, self.direction = change, shape, before, apply, list(slots), env or {}, direction
        self.consumers = consumers if consumers is not None else rc.SINGLE
        self.members = len(self.slots) > 1

    def ids(self):
        return self.slots if self.members else self.slots[0]


def _members_case(shape, n, env=None):
    slots = MEMBER_SLOTS[:n]
    befores = [_steps_before(shape, rc.STEPS_SHRINK, slot, e) for e, slot in enumerate(slots)]
    return Case("members", shape, lambda c, oracle: [b(c, oracle)[0] for b in befores], _steps_change(rc.STEPS_SHRINK), slots, rc.MEMBERS, env, "shrink")


CASES = {}
for _name in rc.SHAPES:
    CASES[f"{_name}-steps_shrink"] = Case("steps_shrink", _name, _steps_before(_name, rc.STEPS_SHRINK), _steps_change(rc.STEPS_SHRINK), direction="shrink")
    CASES[f"{_name}-refresh_grow"] = Case("refresh_grow", _name, _refresh_before(_name), _refresh_change, direction="grow")
    CASES[f"{_name}-reinstall_same_shape"] = Case("reinstall_same_shape", _name, _reinstall_before([_name, _name], True), _reinstall_change([_name, _name], True))
for _name in rc.REFRESH_OWN:
    CASES[f"{_name}-refresh_grow"] = Case("refresh_grow", _name, _refresh_before(_name), _refresh_change, direction="grow")
CASES["F4_5-steps_shrink_ngp"] = Case("steps_shrink_ngp", "F4_5", _steps_before("F4_5", rc.STEPS_SHRINK_NGP), _steps_change(rc.STEPS_SHRINK_NGP),
                                      direction="shrink")
for _k in (2, 3):
    CASES[f"{rc.RESHAPE[_k - 2]}-to-{rc.RESHAPE[_k - 1]}"] = Case("reinstall_other_shape", rc.RESHAPE[_k - 1], _reinstall_before(rc.RESHAPE[:_k], False),
                                                                   _reinstall_change(rc.RESHAPE[:_k], False))
# one (shape, change, consumer) per fast instance under other render policies, and colour on F4_5 under the engine's rule
_POLICY = {"F4_5": "render_ngp", "F4_3": "depth_fixed", "F2_10": "footprint_ngp", "F2_6": "render_fixed_spp4"}
for _name, _consumer in _POLICY.items():
    for _tag, _env in (("merge31_pool", {"PRV_MERGE_MAX": "31", "PRV_POOL": "1"}), ("cell_cache", {"PRV_CELL_CACHE": "1"})):
        CASES[f"{_name}-steps_shrink-{_tag}"] = Case("steps_shrink", _name, _steps_before(_name, rc.STEPS_SHRINK), _steps_change(rc.STEPS_SHRINK),
                                                     consumers=[_consumer], env=_env, direction="shrink")
# the ensemble: five members take the one-launch march by default, two take it under PRV_MARCH_MULTI=1
CASES["F4_5-members5"] = _members_case("F4_5", 5)
CASES["F2_10-members5"] = _members_case("F2_10", 5)
CASES["F4_5-members5-march_multi0"] = _members_case("F4_5", 5, {"PRV_MARCH_MULTI": "0"})
CASES["F4_5-members2"] = _members_case("F4_5", 2)
CASES["F4_5-members2-march_multi1"] = _members_case("F4_5", 2, {"PRV_MARCH_MULTI": "1"})

SINGLE_CASES = [k for k, c in CASES.items() if not c.members and not c.env]
MEMBER_CASES = [k for k, c in CASES.items() if c.members]
POLICY_CASES = [k for k, c in CASES.items() if not c.members and c.env]


def _run_consumers(c, rig, case):
    return {k: rc.CONSUMERS[k].run(c, rig, case.ids()) for k in case.consumers}


def _in_fresh_context(oracle, case, exports, descs):
    c = api.Context(0)
    try:
        rig = rc.Rig(c, oracle)
        for slot, d, arrays in zip(case.slots, descs, exports):
            c.load_model(slot, d, *arrays)
        out = _run_consumers(c, rig, case)
        layout = c.model_layout(case.slots[0])
        rig.close()
    finally:
        c.close()
    return out, layout


class Run:
    pass


def _protocol(c, oracle, case):
    r = Run()
    r.case = case
    rig = rc.Rig(c, oracle)
    r.state = case.before(c, oracle)
    r.occ_before = [c.export_model(s, c.model_desc(s))[2] for s in case.slots]
    r.warm = _run_consumers(c, rig, case)
    case.apply(c, oracle, r.state)
    r.after = _run_consumers(c, rig, case)
    r.descs = [c.model_desc(s) for s in case.slots]
    r.exports = [c.export_model(s, d) for s, d in zip(case.slots, r.descs)]
    r.exports_again = [c.export_model(s, d) for s, d in zip(case.slots, r.descs)]
    r.layout = c.model_layout(case.slots[0])
    rig.close()
    r.fresh, r.fresh_layout = _in_fresh_context(oracle, case, r.exports, r.descs)
    return r


_runs = {}  # the session context's runs, by case: a fixture that wants a subset of them does not run the protocol again


def _protocol_for(request, ctx, oracle):
    case = CASES[request.param]
    if not case.env:
        if request.param not in _runs:
            _runs[request.param] = _protocol(ctx, oracle, case)
        return _runs[request.param]
    with environment(case.env):  # restored on the way out; the session context never sees it
        c = api.Context(0)
        try:
            return _protocol(c, oracle, case)
        finally:
            c.close()


@pytest.fixture(scope="module", autouse=True)
def own_slots(ctx):
    yield
    _runs.clear()
    for s in [SLOT] + MEMBER_SLOTS:  # no trained table, no 32^3 grid stays behind
        ctx.synthetic_model(s, api.field_desc(**util.SMALL), util.SEED_A)


@pytest.fixture(scope="module", params=SINGLE_CASES)
def run(request, ctx, oracle):
    return _protocol_for(request, ctx, oracle)


@pytest.fixture(scope="module", params=[k for k in SINGLE_CASES if CASES[k].change == "steps_shrink"])
def shrunk(request, ctx, oracle):
    return _protocol_for(request, ctx, oracle)


@pytest.fixture(scope="module", params=MEMBER_CASES)
def ensemble(request, ctx, oracle):
    return _protocol_for(request, ctx, oracle)


@pytest.fixture(scope="module", params=POLICY_CASES)
def policy(request, ctx, oracle):
    return _protocol_for(request, ctx, oracle)


def _assert_consumer(r, name):
    consumer = rc.CONSUMERS[name]
    bad = rc.same_bytes(r.after[name], r.fresh[name])
    assert not bad, f"{name}: {bad} after the change differ from a fresh context loaded with the exported arrays"
    moved = consumer.reads & set(rc.CHANGED[r.case.change])
    if name == "model_layout":
        moved = "d" in rc.CHANGED[r.case.change]
    same_as_before = not rc.same_bytes(r.after[name], r.warm[name])
    assert same_as_before == (not moved), f"{name}: the change {'left' if moved else 'moved'} its output (reads {sorted(consumer.reads)})"


@pytest.mark.parametrize("name", rc.SINGLE)
def test_consumer_sees_the_new_state(run, name):
    _assert_consumer(run, name)


@pytest.mark.parametrize("name", rc.MEMBERS)
def test_ensemble_consumer_sees_the_new_state(ensemble, name):
    _assert_consumer(ensemble, name)


def test_consumer_sees_the_new_state_under_other_policies(policy):
    _assert_consumer(policy, policy.case.consumers[0])
    _check_export_and_preconditions(policy)


def _check_export_and_preconditions(r):
    for k, slot in enumerate(r.case.slots):
        assert all(np.array_equal(a, b) for a, b in zip(r.exports[k], r.exports_again[k]))
        t16, m16, occ = r.exports[k]
        if r.state:  # a trainer's: the fp16 copies of its masters
            mt, mm = r.state[k].master
            assert np.array_equal(t16, mt.astype(np.float16).view(np.uint16)) and np.array_equal(m16, mm.astype(np.float16).view(np.uint16))
            if r.case.direction == "grow":
                assert np.array_equal(t16, r.state[k].params[0]) and np.array_equal(m16, r.state[k].params[1])
        if r.case.direction:
            rc.assert_occupancy_preconditions(r.occ_before[k], occ, r.descs[k].occ_res, r.case.direction)
        else:
            assert r.case.change == "reinstall_other_shape" or rc.words_changed(r.occ_before[k], occ) >= 0.25
    if r.case.members:  # members that differ: the interleaved occupancy has more than one answer per cell
        occs = [e[2] for e in r.exports]
        assert all(rc.words_changed(occs[0], o) > 0.05 for o in occs[1:])


def test_export_and_preconditions(run):
    _check_export_and_preconditions(run)


def test_ensemble_export_and_preconditions(ensemble):
    _check_export_and_preconditions(ensemble)


def test_layout_follows_the_installed_shape(run):
    entry = instances.MATRIX.get(run.case.shape)
    assert run.layout == run.fresh_layout
    if entry is not None:
        instances.assert_layout(run.layout, entry)
        assert run.layout["table_bytes_physical"] == instances.restated_layout(entry.kw)["table_bytes_physical"]


def test_trained_renders_equal_the_oracles(shrunk, oracle):
    """colour (views 0 and 3, both rules) and depth (one view, every 13th pixel) after steps_shrink against the oracle on the exported
    field: the session context and the fresh one agree bit for bit, so this pins both"""
    run = shrunk
    kw = run.state[0].kw
    f = oracle.OracleField(oracle.desc(**kw), params=run.exports[0])
    ocams = rc.oracle_cameras(oracle)
    for rule, S, mode in (("fixed", rc.FIXED_S, 0), ("ngp", 0, 1)):
        got = run.after[f"render_{rule}"]["rgba"]
        for v, oc in ((0, ocams[0]), (3, ocams[3])):
            util.assert_pixels_close_any(got[v], [f.render(oc, rc.W, rc.H, S, 1, mt, step_mode=mode)[0] for mt in util.termination_variants(rc.MIN_T)])
        assert (got[..., 3] > 0.5).mean() > 0.02
    v, stride = 3, 13
    d = run.after["depth_fixed"]
    got = march_ref.strided(np.concatenate([d["rgba"][v], d["depth"][v][..., None]], axis=-1), stride)
    wants = [march_ref.strided(depth_ref.render(oracle.lib(), f, ocams[v], rc.W, rc.H, rc.FIXED_S, 1, mt, 0, stride), stride)
             for mt in util.termination_variants(rc.MIN_T)]
    util.assert_pixels_close_any(got, wants)
    f.close()


# ---- every consumer meets a DIRTY slot: a change of its own before its second run
class Rounds:
    pass


def _rounds(c, oracle, shape, slots, names):
    """a live trainer per slot; per consumer: run it (warm, clean slot), one round of steps ending in a refresh (the slot is dirty: nobody
    has used it since), run it again, export.  Then one fresh context loads each export in turn and runs that consumer."""
    r = Rounds()
    r.names, r.warm, r.after, r.fresh, r.exports = rc.dirty_order(names), {}, {}, {}, {}
    case = Case("round", shape, None, None, slots, names)
    state = [_steps_before(shape, rc.ROUND, slot, e)(c, oracle)[0] for e, slot in enumerate(slots)]
    descs = [api.field_desc(**s.kw) for s in state]
    rig = rc.Rig(c, oracle)
    for name in r.names:
        run = rc.CONSUMERS[name].run
        r.warm[name] = run(c, rig, case.ids())
        if len(state) == 1:
            state[0].tr.steps(rc.ROUND["steps"])
        else:
            api.train_many([s.tr for s in state], rc.ROUND["steps"])
        r.after[name] = run(c, rig, case.ids())  # the first use of the slot since the trainer published
        r.exports[name] = [c.export_model(s, d) for s, d in zip(slots, descs)]
    for s in state:
        s.finish()
    rig.close()
    f = api.Context(0)
    try:
        rig = rc.Rig(f, oracle)
        for name in r.names:
            for slot, d, arrays in zip(slots, descs, r.exports[name]):
                f.load_model(slot, d, *arrays)
            r.fresh[name] = rc.CONSUMERS[name].run(f, rig, case.ids())
        rig.close()
    finally:
        f.close()
    return r


@pytest.fixture(scope="module", params=rc.ROUND_SHAPES)
def rounds(request, ctx, oracle):
    return _rounds(ctx, oracle, request.param, [SLOT], rc.SINGLE)


@pytest.fixture(scope="module", params=["F4_5", "F2_0"])
def member_rounds(request, ctx, oracle):
    return _rounds(ctx, oracle, request.param, MEMBER_SLOTS, rc.MEMBERS)


def _assert_round(r, name):
    bad = rc.same_bytes(r.after[name], r.fresh[name])
    assert not bad, f"{name} on a dirty slot: {bad} differ from a fresh context loaded with the arrays exported right after it"
    moved = bool(rc.CONSUMERS[name].reads)  # a round writes table, MLP and occupancy; model_layout reads none of them
    assert (not rc.same_bytes(r.after[name], r.warm[name])) == (not moved), f"{name}: the round {'left' if moved else 'moved'} its output"
    k = r.names.index(name)
    if k:  # the round did move the arrays it reads: a condition on the input
        prev, now = r.exports[r.names[k - 1]], r.exports[name]
        for e in range(len(now)):
            assert not np.array_equal(prev[e][0], now[e][0]) and not np.array_equal(prev[e][1], now[e][1]) and not np.array_equal(prev[e][2], now[e][2])


@pytest.mark.parametrize("name", rc.SINGLE)
def test_consumer_rebuilds_a_dirty_slot_itself(rounds, name):
    """what test_consumer_sees_the_new_state cannot show: there the first consumer after the change rebuilds the slot for all the others.
    Here the trainer steps before EVERY consumer's second run, so an entry point that does not rebuild a dirty slot returns the bytes of
    the round before"""
    _assert_round(rounds, name)


@pytest.mark.parametrize("name", rc.MEMBERS)
def test_ensemble_consumer_rebuilds_dirty_members_itself(member_rounds, name):
    _assert_round(member_rounds, name)


def test_train_render_train_render_refresh_render(ctx, oracle):
    """one slot: train, render, train, render, refresh, render -- each render's bytes are those of a fresh context loaded with the export
    taken at that moment.  A dirty flag cleared too early, or not set by refresh_occupancy alone, fails the second or the third."""
    name = "F4_5"
    rig = rc.Rig(ctx, oracle)
    s = _steps_before(name, rc.STEPS_SHRINK)(ctx, oracle)[0]
    consumers = ["render_ngp", "depth_fixed", "first_hit"]
    case = Case("interleaved", name, None, None, consumers=consumers)
    got, exports = [], []
    d = api.field_desc(**s.kw)
    for stage in ("train", "train", "refresh"):
        if stage == "train":
            s.tr.steps(24 if not got else 20)  # refreshes at steps 16 and 32; the last one alone comes 12 steps after them
        else:
            s.tr.refresh_occupancy()
        k = len(got)  # each of the three is the first to use the slot once
        got.append(_run_consumers(ctx, rig, Case("interleaved", name, None, None, consumers=consumers[k:] + consumers[:k])))
        exports.append(ctx.export_model(SLOT, d))
    s.finish()
    rig.close()
    assert not np.array_equal(exports[0][0], exports[1][0]) and np.array_equal(exports[1][0], exports[2][0])
    assert rc.words_changed(exports[1][2], exports[2][2]) > 0  # the refresh alone moved the grid
    for k in range(3):
        fresh, _ = _in_fresh_context(oracle, case, [exports[k]], [d])
        for name in consumers:
            assert not rc.same_bytes(got[k][name], fresh[name]), (k, name)
            if k:
                assert rc.same_bytes(got[k][name], got[k - 1][name]), (k, name)
