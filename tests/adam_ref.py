"""An independent statement of the trainer's optimiser (test infrastructure): Adam (Kingma and Ba, 2015, algorithm 1, in the
form with the two bias corrections folded into the rate) with instant-ngp's sparse rule for the hash table, in plain numpy
float64.  It imports neither the oracle nor the package and shares no line with either C source.

The rule, for step number n = 1, 2, ... (global: the count of optimiser steps taken so far, plus one):

  * a table scalar whose gradient is exactly zero this step keeps w, m and v exactly -- per scalar, not per group of four;
  * a touched scalar:  m = b1 m + (1 - b1) g,   v = b2 v + (1 - b2) g^2,
                       w = w - lr sqrt(1 - b2^n) / (1 - b1^n) * m / (sqrt(v) + eps);
  * an MLP weight is touched every step, with g = (batch gradient) + l2_reg * w; the table gets no l2_reg.

`AdamRef` keeps its own float64 m and v across steps and restarts w, at every step, from the float32 master weights it is
handed: rounding of w cannot pile up between the reference and the code under test, an error in how the moments are kept does.
The hyper-parameters are the float32 numbers a trainer holds (prv_train_opts), widened exactly.

`MUTATIONS` are wrong rules behind the same interface: what a test built on AdamRef must be able to tell from the right one
(tests/test_adam_host.py shows that it does, at ten times its bar).  `applies(hp)` says for which hyper-parameters a mutation
is a different rule at all.
"""
import numpy as np

# the three hyper-parameter sets of the optimiser tests: the library's defaults and two that move every knob
HYPER = {
    "default": dict(lr=1e-2, beta1=0.9, beta2=0.99, eps=1e-15, l2_reg=1e-6),
    "slow": dict(lr=1e-3, beta1=0.8, beta2=0.999, eps=1e-8, l2_reg=1e-4),
    "fast": dict(lr=5e-2, beta1=0.5, beta2=0.9, eps=1e-15, l2_reg=1e-6),
}


def as_held(hp):
    """the hyper-parameters as the float32 values a trainer holds"""
    return {k: float(np.float32(v)) for k, v in hp.items()}


def bar(lr, w):
    """per-scalar bound on |w_new - w_ref|: 0.2 % of one full-size step plus one unit in the last place of the f32 master.
    (tests/test_adam_host.py: f32 arithmetic stays 70x below it, the weakest wrong rule lands 40x above it.)"""
    return 2e-3 * float(np.float32(lr)) + 2.0 ** -23 * np.abs(np.asarray(w, np.float64))


class Rule:
    """the knobs a mutation turns; the defaults are the right rule"""

    def __init__(self, swap_betas=False, n_shift=0, correct_v=True, eps_inside=False, decay_untouched=False, l2_on_table=False,
                 l2_sign=1.0, skip_group=1):
        self.swap_betas, self.n_shift, self.correct_v, self.eps_inside = swap_betas, n_shift, correct_v, eps_inside
        self.decay_untouched, self.l2_on_table, self.l2_sign, self.skip_group = decay_untouched, l2_on_table, l2_sign, skip_group


class AdamRef:
    def __init__(self, n_table, n_mlp, lr, beta1, beta2, eps, l2_reg, rule=None):
        self.hp = as_held(dict(lr=lr, beta1=beta1, beta2=beta2, eps=eps, l2_reg=l2_reg))
        self.rule = rule if rule is not None else Rule()
        self.table_m, self.table_v = np.zeros(n_table), np.zeros(n_table)
        self.mlp_m, self.mlp_v = np.zeros(n_mlp), np.zeros(n_mlp)

    def _update(self, n, w, g, m, v, touched):
        """m and v are updated in place; returns the new w (float64)"""
        r, hp = self.rule, self.hp
        b1, b2 = (hp["beta2"], hp["beta1"]) if r.swap_betas else (hp["beta1"], hp["beta2"])
        n = n + r.n_shift
        if r.decay_untouched:
            m[~touched] *= b1
            v[~touched] *= b2
        m[touched] = b1 * m[touched] + (1.0 - b1) * g[touched]
        v[touched] = b2 * v[touched] + (1.0 - b2) * g[touched] ** 2
        with np.errstate(all="ignore"):  # (the n - 1 mutation divides by zero at the first step, as the bug would)
            rate = hp["lr"] * (np.sqrt(1.0 - b2 ** n) if r.correct_v else 1.0) / (1.0 - b1 ** n)
            root = np.sqrt(v + hp["eps"]) if r.eps_inside else np.sqrt(v) + hp["eps"]
            return np.where(touched, w - rate * m / root, w)

    def step(self, n, table_w, table_g, mlp_w, mlp_g):
        """one optimiser step, number n (1-based, global), from the given f32 masters and the gradients the optimiser
        was handed -> the new (table, mlp) weights in float64"""
        r, l2 = self.rule, self.hp["l2_reg"] * self.rule.l2_sign
        tw, tg = np.asarray(table_w, np.float64), np.asarray(table_g, np.float64)
        mw, mg = np.asarray(mlp_w, np.float64), np.asarray(mlp_g, np.float64)
        if r.l2_on_table:
            tg = tg + l2 * tw
        touched = tg != 0.0
        if r.skip_group > 1:  # a group of skip_group consecutive scalars is updated whole when any of them is touched
            touched = np.repeat(touched.reshape(-1, r.skip_group).any(axis=1), r.skip_group)
        new_t = self._update(n, tw, tg, self.table_m, self.table_v, touched)
        new_m = self._update(n, mw, mg + l2 * mw, self.mlp_m, self.mlp_v, np.ones(len(mw), bool))
        return new_t, new_m


class Mutation:
    def __init__(self, rule, applies=lambda hp: True):
        self.rule, self.applies = rule, applies


_has_l2 = lambda hp: hp["l2_reg"] != 0.0
MUTATIONS = {
    "betas_exchanged": Mutation(Rule(swap_betas=True), lambda hp: hp["beta1"] != hp["beta2"]),
    "step_number_minus_one": Mutation(Rule(n_shift=-1)),
    "step_number_plus_one": Mutation(Rule(n_shift=+1)),
    "no_second_moment_correction": Mutation(Rule(correct_v=False)),
    "eps_inside_the_root": Mutation(Rule(eps_inside=True)),
    "untouched_moments_decay": Mutation(Rule(decay_untouched=True)),
    "l2_on_the_table_too": Mutation(Rule(l2_on_table=True), _has_l2),
    "l2_wrong_sign": Mutation(Rule(l2_sign=-1.0), _has_l2),
    "group_wise_skipping": Mutation(Rule(skip_group=4)),
}


def excess(got, ref, lr):
    """max over scalars of |got - ref| / bar; a non-finite value counts as infinitely far"""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    with np.errstate(invalid="ignore"):
        d = np.abs(got - ref) / bar(lr, ref)
    return float(np.where(np.isfinite(d), d, np.inf).max()) if d.size else 0.0


class Coverage:
    """the two conditions that keep a run from being vacuous, accumulated from the table's per-step touched masks:
    scalars that were touched, then left alone for three or more steps, then touched again (their moments must have been kept),
    and groups of four of which some scalars were touched and others not (the per-scalar rule is exercised)"""

    def __init__(self, n_table):
        self.idle = np.full(n_table, -1, np.int64)  # steps since the last touch; -1: never touched
        self.revisited = np.zeros(n_table, bool)
        self.partial = np.zeros(n_table // 4, bool)

    def add(self, touched):
        touched = np.asarray(touched, bool)
        self.revisited |= touched & (self.idle >= 3)
        self.idle = np.where(touched, 0, np.where(self.idle >= 0, self.idle + 1, -1))
        k = touched[: len(self.partial) * 4].reshape(-1, 4).sum(axis=1)
        self.partial |= (k > 0) & (k < 4)

    @property
    def n_revisited(self):
        return int(self.revisited.sum())

    @property
    def n_partial_groups(self):
        return int(self.partial.sum())

    def check(self):
        assert self.n_revisited >= 200, f"only {self.n_revisited} table scalars were touched again after 3+ idle steps"
        assert self.n_partial_groups >= 50, f"only {self.n_partial_groups} groups of four were partly touched"
