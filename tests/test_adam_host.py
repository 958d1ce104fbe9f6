"""The optimiser's bar, earned without a GPU, and the CPU oracle's optimiser pinned to something that is not itself.

tests/adam_ref.py states Adam with the sparse table rule in float64.  Here:

  * the same formula in float32 numpy, on seeded synthetic gradient sequences (200 steps, 60 % exact zeros per step, magnitudes
    over six decades, three hyper-parameter sets), stays within BAR = 2e-3 lr + 2^-23 |w| of it at every step -- so a correct
    float32 implementation passes -- while every wrong rule of adam_ref.MUTATIONS exceeds 10 BAR on some step of every set;
  * oracle/prv_train.c's own update, step by step on the TINY scenes under both sampling rules, is within BAR of the
    reference, leaves untouched table scalars bit-unchanged and keeps its fp16 copies equal to the rounded masters.

tests/test_gpu_adam.py holds the HIP trainer to the same bar.  CPU only."""
import numpy as np
import pytest

from tests import adam_ref, instances, util

TINY = dict(n_levels=8, n_features=4, log2_hashmap=10, base_res=4, finest_res=24, occ_res=16, density_bias=1.0, table_amp=0.5)
TINY_F2 = dict(TINY, n_levels=16, n_features=2)
INTR = {"fl_x": 20.0, "fl_y": 19.5, "cx": 12.3, "cy": 7.8, "w": 24, "h": 16, "k1": 0.05, "k2": -0.02, "p1": 0.001, "p2": -0.002}
N_TABLE, N_MLP, N_STEPS = 4096, 1024, 200


def synthetic(seed):
    """initial f32 weights and a gradient sequence: ~60 % exact zeros per step (whole idle stretches too: a scalar rests for
    a run of steps with probability 1/2 per run), |g| = 10^U(-9, -3)"""
    rng = np.random.default_rng(seed)
    w_t = rng.uniform(-0.5, 0.5, N_TABLE).astype(np.float32)
    w_m = rng.uniform(-0.5, 0.5, N_MLP).astype(np.float32)
    seq = []
    for k in range(N_STEPS):
        if k % 5 == 0:
            resting = [rng.random(n) < 0.5 for n in (N_TABLE, N_MLP)]
        out = []
        for n, rest in zip((N_TABLE, N_MLP), resting):
            g = rng.choice([-1.0, 1.0], n) * 10.0 ** rng.uniform(-9.0, -3.0, n)
            g[(rng.random(n) < 0.2) | rest] = 0.0
            out.append(g.astype(np.float32))
        seq.append(out)
    return w_t, w_m, seq


class AdamF32:
    """the reference's formula restated in float32 numpy (what a correct kernel computes, up to the order of its operations)"""

    def __init__(self, lr, beta1, beta2, eps, l2_reg):
        f = np.float32
        self.lr, self.b1, self.b2, self.eps, self.l2 = lr, f(beta1), f(beta2), f(eps), f(l2_reg)
        self.m = [np.zeros(N_TABLE, f), np.zeros(N_MLP, f)]
        self.v = [np.zeros(N_TABLE, f), np.zeros(N_MLP, f)]

    def step(self, n, w_t, g_t, w_m, g_m):
        f = np.float32
        rate = f(float(f(self.lr)) * np.sqrt(1.0 - float(self.b2) ** n) / (1.0 - float(self.b1) ** n))
        out = []
        for i, (w, g, on) in enumerate(((w_t, g_t, g_t != 0), (w_m, g_m + self.l2 * w_m, np.ones(N_MLP, bool)))):
            m, v = self.m[i], self.v[i]
            m[on] = self.b1 * m[on] + (f(1) - self.b1) * g[on]
            v[on] = self.b2 * v[on] + (f(1) - self.b2) * g[on] * g[on]
            out.append(np.where(on, w - rate * m / (np.sqrt(v) + self.eps), w).astype(f))
        return out


@pytest.fixture(scope="module", params=list(adam_ref.HYPER))
def synthetic_run(request):
    """the f32 trajectory, the reference's answer at each of its steps, and each mutation's"""
    hp = adam_ref.HYPER[request.param]
    w_t, w_m, seq = synthetic(7)
    ref, f32 = adam_ref.AdamRef(N_TABLE, N_MLP, **hp), AdamF32(**hp)
    wrong = {k: adam_ref.AdamRef(N_TABLE, N_MLP, rule=mu.rule, **hp) for k, mu in adam_ref.MUTATIONS.items()}
    gap, caught = 0.0, {k: 0.0 for k in wrong}
    cov = adam_ref.Coverage(N_TABLE)
    for k, (g_t, g_m) in enumerate(seq):
        n = k + 1
        want = ref.step(n, w_t, g_t, w_m, g_m)
        got = f32.step(n, w_t, g_t, w_m, g_m)
        gap = max(gap, max(adam_ref.excess(a, b, hp["lr"]) for a, b in zip(got, want)))
        for name, mu in wrong.items():
            bad = mu.step(n, w_t, g_t, w_m, g_m)
            caught[name] = max(caught[name], max(adam_ref.excess(a, b, hp["lr"]) for a, b in zip(bad, want)))
        cov.add(g_t != 0)
        assert np.array_equal(got[0][g_t == 0], w_t[g_t == 0])
        w_t, w_m = got  # the masters follow the f32 trajectory, as a trainer's do
    return request.param, hp, gap, caught, cov


def test_f32_arithmetic_stays_inside_the_bar(synthetic_run):
    name, hp, gap, caught, cov = synthetic_run
    print(f"[{name}] f32 restatement vs f64 reference over {N_STEPS} steps: worst error = {gap:.4f} BAR")
    cov.check()
    assert gap <= 1.0
    assert gap <= 0.1  # ... with room: the bar is not a fit to what f32 happens to give


@pytest.mark.parametrize("mutation", list(adam_ref.MUTATIONS))
def test_every_wrong_rule_lands_far_outside_the_bar(synthetic_run, mutation):
    name, hp, gap, caught, cov = synthetic_run
    if not adam_ref.MUTATIONS[mutation].applies(adam_ref.as_held(hp)):
        pytest.fail(f"{mutation} is no different rule under the set {name}: every listed set must tell it apart")
    print(f"[{name}] {mutation}: worst step is {caught[mutation]:.1f} BAR from the reference")
    assert caught[mutation] > 10.0


def test_mutation_list_is_the_agreed_one():
    assert set(adam_ref.MUTATIONS) >= {"betas_exchanged", "step_number_minus_one", "step_number_plus_one", "no_second_moment_correction",
                                       "eps_inside_the_root", "untouched_moments_decay", "l2_on_the_table_too", "l2_wrong_sign",
                                       "group_wise_skipping"}


def test_first_step_is_lr_against_the_sign():
    """a known answer of the reference itself: with zero moments the first step is lr * g / (|g| + eps sqrt(1 - b2))"""
    hp = adam_ref.HYPER["default"]
    ref = adam_ref.AdamRef(4, 4, **hp)
    g = np.array([1e-3, -2e-5, 0.0, 7.0])
    w = np.array([0.25, -0.5, 0.125, 1.0], np.float32)
    t, m = ref.step(1, w, g, w, np.zeros(4))
    lr = float(np.float32(hp["lr"]))
    np.testing.assert_allclose(t - w, [-lr, lr, 0.0, -lr], rtol=1e-9, atol=0)
    assert t[2] == w[2] and ref.table_m[2] == 0.0 and ref.table_v[2] == 0.0
    np.testing.assert_allclose(m - w, -lr * np.sign(w), rtol=1e-6)  # the MLP: l2_reg * w alone is a gradient


# ------------------------------------------------------------------ the oracle's optimiser


@pytest.fixture(scope="module", params=["F4", "F2"])
def scene(request, oracle):
    kw = TINY if request.param == "F4" else TINY_F2
    gt = oracle.OracleField(oracle.desc(**dict(kw, density_bias=3.0, table_amp=2.0)), seed=util.SEED_B)
    pts = util.fibonacci_hemisphere(8)
    tms, scale, offset = util.hemisphere_transforms(oracle, pts)
    cams = oracle.cameras_from_dataset(tms, INTR, scale, offset)
    imgs = np.stack([oracle.quantize_rgba8(gt.render(c, 24, 16, 32, 1, 1e-4)[0], (0, 0, 0, 0)) for c in cams])
    f = oracle.OracleField(oracle.desc(**kw), seed=util.SEED_A)
    t, m, o = f.params()
    return kw, oracle.OracleField(f.desc, params=(t, m, np.full_like(o, 0xFFFFFFFF))), cams, imgs


# few rays per step, so that most table entries rest between visits (192 rays touch 95 % of this table every step)
RULES = {"fixed_s": dict(n_rays=48, n_samples=24), "ngp": dict(step_mode=1, n_samples=1024, n_rays=8)}
ORACLE_STEPS = 40


@pytest.mark.parametrize("rule", list(RULES))
@pytest.mark.parametrize("hyper", list(adam_ref.HYPER))
def test_oracle_update_is_the_reference_update(oracle, scene, hyper, rule):
    kw, init, cams, imgs = scene
    hp = adam_ref.HYPER[hyper]
    tr = oracle.OracleTrainer(init, oracle.train_opts(occ_every=0, **hp, **RULES[rule]), cams, imgs)
    ref = adam_ref.AdamRef(tr.n_table, len(tr.master()[1]), **hp)
    cov, worst, worst_lr = adam_ref.Coverage(tr.n_table), 0.0, 0.0
    for k in range(ORACLE_STEPS):
        loss, tg, mg = tr.gradients()
        tg, mg = tg.astype(np.float32), mg.astype(np.float32)  # what the optimiser is handed
        t0, m0 = (a.copy() for a in tr.master())
        assert tr.step() == pytest.approx(loss, rel=1e-12)  # the step used the batch that was previewed
        t1, m1 = (a.copy() for a in tr.master())
        want_t, want_m = ref.step(k + 1, t0, tg, m0, mg)
        e = max(adam_ref.excess(t1, want_t, hp["lr"]), adam_ref.excess(m1, want_m, hp["lr"]))
        worst = max(worst, e)
        worst_lr = max(worst_lr, np.abs(t1 - want_t).max() / hp["lr"], np.abs(m1 - want_m).max() / hp["lr"])
        assert e <= 1.0, (k, e)
        still = tg == 0
        assert np.array_equal(t1[still].view(np.uint32), t0[still].view(np.uint32))
        assert (t1 != t0)[~still].mean() > 0.9  # ... and the touched ones do move
        t16, m16, _ = tr.params()
        assert np.array_equal(t16, t1.astype(np.float16).view(np.uint16)) and np.array_equal(m16, m1.astype(np.float16).view(np.uint16))
        cov.add(~still)
    print(f"[{kw['n_features']} features, {hyper}, {rule}] oracle vs reference: worst error = {worst:.4f} BAR = "
          f"{worst_lr:.2e} lr; revisited {cov.n_revisited}, partly touched groups {cov.n_partial_groups}")
    assert cov.n_revisited >= 200
    # F = 4: a group of four IS one table entry and the encoder's backward pass hands all four features of an entry their
    # gradient together, so its groups are touched whole; F = 2 packs two entries into a group and has to show the mix
    if kw["n_features"] == 2:
        assert cov.n_partial_groups >= 50


# ------------------------------------------------------------------ adam_table_kernel's partial last group


@pytest.mark.parametrize("name", list(instances.MATRIX) + list(instances.PRODUCT) + ["TINY", "TINY_F2", "SMALL", "SMALL_F2"])
def test_every_table_is_whole_groups_of_four(oracle, name):
    """prv_train.hip: adam_table_kernel keeps a path for a last group of fewer than four scalars (i4 + 4 > n).  No descriptor
    reaches it: a dense level is rounded up to a multiple of 8 entries, a hashed one has 2^log2_hashmap >= 16, and F is 2
    or 4 -- every level, hence every table, is a multiple of four scalars (of eight, even)."""
    kw = {"TINY": TINY, "TINY_F2": TINY_F2, "SMALL": util.SMALL, "SMALL_F2": util.SMALL_F2}.get(name)
    if kw is None:
        kw = {**instances.MATRIX, **instances.PRODUCT}[name].kw
    F = kw["n_features"]
    restated = instances.restated_levels(kw)
    assert all(entries % 8 == 0 for _, _, _, entries in restated) and F in (2, 4)
    lv, total = oracle.levels(oracle.desc(**kw))
    assert [a.size for a in lv] == [n for _, _, _, n in restated] and total == sum(a.size for a in lv)
    assert (total * F) % 4 == 0
