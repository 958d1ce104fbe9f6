"""The HIP trainer's optimiser step (prv_train.hip: adam_table_kernel, adam_mlp_kernel, end_step; prv_train_api.inc: the step's
chain) pinned to tests/adam_ref.py, an independent float64 Adam -- not to the oracle, whose optimiser is the same three lines.

The step ladder: gradients() previews the batch the next step will use (same kernels, same launch shapes; deterministic = 1
makes its sums order-free), master() gives the weights before, steps(1) steps, master() gives the weights after.  The reference
gets the previewed gradient and must land within BAR = 2e-3 lr + 2^-23 |w| of every scalar (tests/test_adam_host.py: f32
rounding stays below 0.02 BAR, the weakest wrong rule lands 40 BAR away).  That the step used the previewed batch is asserted,
not assumed: two previews are byte-equal and the step's loss is the previewed loss bit for bit.

Then the things a per-step check cannot see: N steps in one call equal N calls of one step byte for byte (the next step's
rate, written by the closing kernel while the step is still in flight, must not leak; the next batch is listed ahead only
in the chained run), members stepping side by side equal their solo runs, and the product path (f32 atomics) keeps what
holds in any order of the atomics."""
import numpy as np
import pytest

from nerf_prv_amd import api
from tests import adam_ref, util
from tests.test_gpu_train import scene  # noqa: F401  (the TINY F4 / F2 scenes, built once per module as test_gpu_train.py builds them)

pytestmark = pytest.mark.gpu

# few rays per step: most table entries rest between visits (tests/test_adam_host.py runs the same batches on the oracle)
RULES = {"fixed_s": dict(n_rays=48, n_samples=24), "ngp": dict(step_mode=api.L.STEP_NGP, n_samples=1024, n_rays=8)}
REFRESH = dict(occ_every=4, occ_sigma_thresh=0.3)
SLOT = 3


def bits(a):
    return np.ascontiguousarray(a).view(np.uint8).tobytes()


def make(ctx, oracle, scene, slot=SLOT, field_seed=util.SEED_A, **opts):  # noqa: F811
    """an all-occupied seeded field in `slot` and a trainer on it"""
    kw, ocams, cams, imgs = scene
    t, m, o = oracle.OracleField(oracle.desc(**kw), seed=field_seed).params()
    ctx.load_model(slot, api.field_desc(**kw), t, m, np.full_like(o, 0xFFFFFFFF))
    base = dict(occ_every=0, deterministic=1)
    base.update(opts)
    return api.Trainer(ctx, slot, cams, ctx.torch.from_numpy(imgs), api.train_opts(**base))


def ladder(ctx, tr, kw, hp, n_steps, slot=SLOT):
    """n_steps single steps, each held to the reference -> (losses, masters, exported model, worst error / BAR, worst error / lr, coverage)"""
    d = api.field_desc(**kw)
    n_table = tr.info()["table_scalars"]
    ref = adam_ref.AdamRef(n_table, api.L.MLP_HALFS, **hp)
    cov, worst, worst_lr, losses = adam_ref.Coverage(n_table), 0.0, 0.0, []
    t16_before = ctx.export_model(slot, d)[0].copy()
    for k in range(n_steps):
        loss, tg, mg = tr.gradients()
        loss_b, tg_b, mg_b = tr.gradients()
        assert np.float32(loss).tobytes() == np.float32(loss_b).tobytes() and bits(tg) == bits(tg_b) and bits(mg) == bits(mg_b), k
        t0, m0 = tr.master()
        got_loss = tr.steps(1)
        assert got_loss.tobytes() == np.float32(loss).tobytes(), (k, got_loss, loss)  # the step used the previewed batch
        losses.append(got_loss[0])
        t1, m1 = tr.master()
        assert tr.info()["steps"] == k + 1
        want_t, want_m = ref.step(k + 1, t0, tg, m0, mg)
        e = max(adam_ref.excess(t1, want_t, hp["lr"]), adam_ref.excess(m1, want_m, hp["lr"]))
        worst = max(worst, e)
        worst_lr = max(worst_lr, np.abs(t1 - want_t).max() / hp["lr"], np.abs(m1 - want_m).max() / hp["lr"])
        assert e <= 1.0, f"step {k + 1}: a scalar is {e:.2f} BAR from the reference"
        t16, m16, _ = ctx.export_model(slot, d)
        still = tg == 0
        assert np.array_equal(t1[still].view(np.uint32), t0[still].view(np.uint32)), k  # untouched: master ...
        assert np.array_equal(t16[still], t16_before[still]), k  # ... and the fp16 table the renderer reads
        assert np.array_equal(t16, t1.astype(np.float16).view(np.uint16)) and np.array_equal(m16, m1.astype(np.float16).view(np.uint16)), k
        t16_before = t16.copy()
        cov.add(~still)
    assert cov.n_revisited >= 200, cov.n_revisited
    # F = 4: a group of four is one table entry, whose four features get their gradient together (test_adam_host.py)
    if kw["n_features"] == 2:
        assert cov.n_partial_groups >= 50, cov.n_partial_groups
    return np.array(losses, np.float32), (t1, m1), [a.copy() for a in ctx.export_model(slot, d)], worst, worst_lr, cov


LADDERS = {  # hyper-parameter set, rule, steps, extra options
    "default": ("default", "fixed_s", 120, {}),
    "slow": ("slow", "fixed_s", 40, {}),
    "fast": ("fast", "fixed_s", 40, {}),
    "default_ngp": ("default", "ngp", 40, {}),
    "default_refresh": ("default", "fixed_s", 40, REFRESH),  # a density refresh behind every fourth step: no batch listed ahead there
}


@pytest.mark.parametrize("case", list(LADDERS))
def test_step_ladder_against_the_reference(ctx, oracle, scene, case):  # noqa: F811
    hyper, rule, n_steps, extra = LADDERS[case]
    hp = adam_ref.HYPER[hyper]
    tr = make(ctx, oracle, scene, **hp, **RULES[rule], **extra)
    losses, _, _, worst, worst_lr, cov = ladder(ctx, tr, scene[0], hp, n_steps)
    tr.close()
    print(f"[F{scene[0]['n_features']} {case}] {n_steps} steps: worst |w_gpu - w_ref| = {worst:.4f} BAR = {worst_lr:.2e} lr; "
          f"revisited {cov.n_revisited}, partly touched groups {cov.n_partial_groups}")
    assert np.isfinite(losses).all() and worst <= 1.0


@pytest.mark.parametrize("env", [None, ("PRV_TRAIN_GRAPH", "0"), ("PRV_TRAIN_OWN_QUEUE", "0")], ids=["default", "no_graph", "pooled_queue"])
@pytest.mark.parametrize("hyper,extra", [("fast", REFRESH), ("slow", {})], ids=["fast_refresh", "slow"])
def test_chained_steps_equal_single_steps(ctx, oracle, scene, monkeypatch, env, hyper, extra):  # noqa: F811
    """steps(N) in one call: steps are opened by the previous step's closing kernel, batches are listed ahead beside the
    table's Adam pass, a graph is replayed -- none of it in the ladder's steps(1) calls.  Same bytes."""
    if env:
        monkeypatch.setenv(*env)  # read when a trainer is created
    N = 40
    hp = adam_ref.HYPER[hyper]
    opts = dict(**hp, **RULES["fixed_s"], **extra)
    tr = make(ctx, oracle, scene, **opts)
    losses, (t1, m1), model, worst, _, _ = ladder(ctx, tr, scene[0], hp, N)
    tr.close()
    tr = make(ctx, oracle, scene, **opts)
    chained = tr.steps(N)
    ct, cm = tr.master()
    cmodel = ctx.export_model(SLOT, api.field_desc(**scene[0]))
    assert tr.info()["steps"] == N
    tr.close()
    assert chained.tobytes() == losses.tobytes()
    assert bits(ct) == bits(t1) and bits(cm) == bits(m1)
    assert all(bits(a) == bits(b) for a, b in zip(cmodel, model))  # fp16 table, MLP, occupancy


def test_members_side_by_side_equal_their_solo_runs(ctx, oracle, scene, monkeypatch):  # noqa: F811
    """prv_train_steps_multi, two members with their own seeds on two slots.  A member stepping alone launches two backward
    blocks per CU and one per CU beside others; the block count is part of the order in which the MLP's weight gradient is
    summed (one partial slot per block), so it is pinned here with PRV_TRAIN_BWD_BLOCKS for both runs: what is compared is
    whether a member sees anything of its neighbour, not two summation orders."""
    monkeypatch.setenv("PRV_TRAIN_BWD_BLOCKS", "64")
    N = 30
    d = api.field_desc(**scene[0])
    opts = [dict(seed=900 + e, **adam_ref.HYPER["fast" if e else "default"], **RULES["fixed_s"], **REFRESH) for e in range(2)]
    alone = []
    for e in range(2):
        tr = make(ctx, oracle, scene, slot=e, field_seed=util.SEED_A + e, **opts[e])
        alone.append((tr.steps(N), tr.master(), [a.copy() for a in ctx.export_model(e, d)]))
        tr.close()
    trs = [make(ctx, oracle, scene, slot=e, field_seed=util.SEED_A + e, **opts[e]) for e in range(2)]
    together = api.train_many(trs, N)
    assert bits(alone[0][0]) != bits(alone[1][0])  # the members do differ
    for e, tr in enumerate(trs):
        assert tr.info()["steps"] == N
        t, m = tr.master()
        assert together[e].tobytes() == alone[e][0].tobytes()
        assert bits(t) == bits(alone[e][1][0]) and bits(m) == bits(alone[e][1][1])
        assert all(bits(a) == bits(b) for a, b in zip(ctx.export_model(e, d), alone[e][2]))
        tr.close()


def test_product_path_keeps_what_no_order_of_atomics_changes(ctx, oracle, scene):  # noqa: F811
    """deterministic = 0 (f32 atomics, what the product trains with), 20 steps.  The previewed gradient is the step's up to
    the order of the adds, so only order-free facts are asserted.  `untouched` is taken per table ENTRY (all F features zero
    in the preview): an entry no sample reaches is zero in any order, while a single feature of a reached entry could cancel
    to exactly zero in one order and not in another."""
    kw = scene[0]
    F, d, hp = kw["n_features"], api.field_desc(**kw), adam_ref.HYPER["default"]
    tr = make(ctx, oracle, scene, deterministic=0, **hp, **RULES["fixed_s"])
    lr = float(np.float32(hp["lr"]))
    n_still = 0
    for k in range(20):
        loss, tg, mg = tr.gradients()
        t0, m0 = tr.master()
        t16_0 = ctx.export_model(SLOT, d)[0].copy()
        tr.steps(1)
        t1, m1 = tr.master()
        t16, m16, _ = ctx.export_model(SLOT, d)
        still = np.repeat(~(tg.reshape(-1, F) != 0).any(axis=1), F)
        n_still += int(still.sum())
        assert np.array_equal(t1[still].view(np.uint32), t0[still].view(np.uint32)) and np.array_equal(t16[still], t16_0[still]), k
        assert np.array_equal(t16, t1.astype(np.float16).view(np.uint16)) and np.array_equal(m16, m1.astype(np.float16).view(np.uint16)), k
        if k == 0:  # zero moments: |m| / sqrt(v) = 1 after the bias corrections, whatever the betas
            for w0, w1, g in ((t0, t1, tg), (m0, m1, mg + np.float32(hp["l2_reg"]) * m0)):
                big = np.abs(g) > 1e-10
                assert big.sum() > 1000
                np.testing.assert_allclose((w1 - w0)[big], -lr * np.sign(g[big]), rtol=2e-3)
    assert n_still > 20 * 1000 and tr.info()["steps"] == 20
    tr.close()
