"""Termination histograms and the Jensen-Shannon view score without a GPU: the CPU reference (tests/termination_ref.py) checks
itself against the oracle and gives the answers one can work out by hand, the C ABI's new symbols are declared, exported and
bound, and the planner shell knows method 9 and polices what it runs with."""
import os
import re
import subprocess

import numpy as np
import pytest

from nerf_prv_amd import _lib, planner
from tests import surface_ref, termination_ref as tr, util
from tests.test_host import GOLD, YAML

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32


@pytest.fixture()
def config(tmp_path):
    p = tmp_path / "DefaultConfiguration.yaml"
    p.write_text(YAML.format(pre=tmp_path, vs=os.path.join(GOLD, "hemisphere")))
    return p


# ---- the reference checks itself
@pytest.mark.parametrize("mode", [0, 1], ids=["fixed", "ngp"])
def test_reference_bins_and_escape_sum_to_one_and_alpha_is_the_oracles(oracle, mode):
    f = oracle.OracleField(oracle.desc(**dict(util.SMALL, density_bias=5.0)), seed=util.SEED_A)
    tms, scale, offset = surface_ref.case_transforms(oracle)
    w, h, K = 24, 16, 16
    ocam = oracle.cameras_from_transforms(tms, util.FOV_X, w, h, scale, offset)[1]
    try:
        want, live = tr.reference(oracle, f, ocam, w, h, K, 96, 1, 1e-4, mode)  # asserts its alpha against the oracle's own render
        px = want[0].astype(np.float64)
        total = px[..., :K].sum(axis=-1) + (1.0 - px[..., K])
        assert (px[..., K] > 0).sum() > 20 and np.abs(total - 1.0).max() <= (K + 1) * 2.0 ** -24
        assert not want[0][..., :K][~live].any() and (want[0][..., :K][live] > 0).any()
        # spp 2: the mean of two sub-samples still sums to 1 (one more rounding per plane for the sum, one for the scale)
        want2, _ = tr.reference(oracle, f, ocam, w, h, K, 96, 2, 1e-4, mode)
        px = want2[0].astype(np.float64)
        assert np.abs(px[..., :K].sum(axis=-1) + (1.0 - px[..., K]) - 1.0).max() <= 3 * (K + 1) * 2.0 ** -24
    finally:
        f.close()


def test_the_bin_formula_never_reaches_the_bin_count():
    for K in tr.BINS:
        for nmax in list(range(1, 129)) + [1024]:
            M = tr.bin_mul(K, nmax)
            assert tr.bin_of(nmax - 1, K, nmax) < K and (nmax - 1) * M < 1 << 32
            assert tr.bin_of(0, K, nmax) == 0
            bins = [tr.bin_of(i, K, nmax) for i in range(nmax)]
            assert bins == sorted(bins)  # depth order: a ray's bins never go back
        assert all(tr.bin_of(i, K, 1024) == i >> (10 - K.bit_length() + 1) for i in range(1024))  # the engine's rule: a plain shift


def test_histogram_by_hand():
    # S = 8, K = 4: two steps a bin; samples at steps 1, 2, 3, 6 with opacity 0.5 each
    bins, T, live = tr.histogram([1, 2, 3, 6], [0.5] * 4, 4, 8)
    assert bins.tolist() == [0.5, 0.375, 0.0, 0.0625] and T == f32(0.0625) and live.tolist() == [True, True, False, True]
    # the cut: T = 0.25 < 0.3 after the second sample, the rest is never composited
    bins, T, live = tr.histogram([1, 2, 3, 6], [0.5] * 4, 4, 8, min_T=0.3)
    assert bins.tolist() == [0.5, 0.25, 0.0, 0.0] and T == f32(0.25) and live.tolist() == [True, True, False, False]


# ---- the divergence on hand-made planes
def test_jsd_restatement_on_hand_made_planes():
    for name, bins, alphas, want in tr.hand_made_cases():
        J = tr.jsd(bins, alphas)
        assert J.shape == (1, 1, 1) and abs(float(J[0, 0, 0]) - want) <= 1e-12, name
        assert J.max() <= np.log2(bins.shape[0]) + 1e-12, name
    rng = np.random.default_rng(3)
    for E in (2, 3, 5, 8):  # no random case exceeds log2 E either, and identical members give 0
        p = rng.dirichlet(np.full(17, 0.2), size=(E, 50)).astype(np.float32)
        bins, alphas = np.moveaxis(p[..., :16], -1, 1), 1.0 - p[..., 16].astype(np.float64)
        J = tr.jsd(bins, alphas)
        assert (J >= 0).all() and J.max() <= np.log2(E)
        assert tr.jsd(np.repeat(bins[:1], E, axis=0), np.repeat(alphas[:1], E, axis=0)).max() <= 1e-14  # (float64 roundings of the mean; exactly 0 for E = 2)
        assert not tr.jsd(np.repeat(bins[:1], 2, axis=0), np.repeat(alphas[:1], 2, axis=0)).any()
    vj, vo = tr.view_scores(np.zeros((2, 4, 3, 2, 2)), np.zeros((2, 3, 2, 2)))
    assert vj.shape == vo.shape == (3,) and not vj.any() and not vo.any()


# ---- the ABI
def test_new_symbols_declared_exported_and_bound():
    header = open(os.path.join(ROOT, "include", "prv.h")).read()
    text = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    out = subprocess.check_output(["nm", "-D", "--defined-only", os.path.join(ROOT, "nerf_prv_amd", "libprv_hip.so")], text=True)
    exported = {l.split()[-1] for l in out.splitlines() if " T " in l}
    for name, n_args in (("prv_render_termination", 10), ("prv_termination_divergence", 11)):
        m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*)\)\s*;", text)
        assert m, f"{name} is not declared in prv.h"
        assert len([a for a in m.group(1).split(",") if a.strip()]) == n_args
        assert name in exported
        assert len(_lib.SIGNATURES[name][1]) == n_args
    assert re.search(r"#define\s+PRV_SCORE_TERMINATION_JSD\s+9\b", header) and _lib.SCORE_TERMINATION_JSD == 9
    assert re.search(r"#define\s+PRV_TERMINATION_BINS_DEFAULT\s+16\b", header) and _lib.TERMINATION_BINS_DEFAULT == 16
    assert _lib.load().prv_abi_version() == 5 and re.search(r"#define\s+PRV_ABI_VERSION\s+5\b", header)


# ---- the planner shell
def test_method_9_is_in_scope_and_8_is_not():
    assert planner.host().prvh_method_in_scope(9) == 1 and planner.host().prvh_method_in_scope(8) == 0


def test_method_9_takes_method_3s_ensemble(config):
    assert planner.ShareData(config, "", -1, -1, 9).number("ensemble_num") == 5 == planner.ShareData(config, "", -1, -1, 3).number("ensemble_num")


def test_termination_config_is_the_default_with_one_line_changed():
    a = open(os.path.join(ROOT, "configs", "DefaultConfiguration.yaml")).read().splitlines()
    b = open(os.path.join(ROOT, "configs", "EnsembleTermination.yaml")).read().splitlines()
    assert len(a) == len(b)
    assert [(x, y) for x, y in zip(a, b) if x != y] == [("method_of_IG : 3", "method_of_IG : 9")]


@pytest.mark.parametrize("extra,rc,text", [("score_path: png\n", -16, "score_path: fused"), ("views_per_iteration: 2\n", -14, "views_per_iteration 2")],
                         ids=["png", "batch"])
def test_method_9_outside_the_fused_single_view_loop_is_refused_and_nothing_is_written(config, capfd, extra, rc, text):
    cfg = config.parent / "refused.yaml"
    cfg.write_text(open(config).read() + extra)
    sd = planner.ShareData(cfg, "refused", -1, -1, 9)
    before = sorted(os.listdir(config.parent))
    with pytest.raises(RuntimeError, match=f"rc={rc}"):
        sd.nbv_loop([1e-10] * 3, 0.1, lambda *a: [0.0] * len(a[4]), first_view_id=1)
    err = capfd.readouterr().err
    assert text in err and "nothing was written" in err
    assert sorted(os.listdir(config.parent)) == before and not os.path.exists(sd.string("save_path") + "_v1_t0")


def test_method_9_runs_the_stub_scored_loop(config):
    """the fused single-view loop takes the method like 3 and 7: the stub-scored loop of tests/test_entropy_host.py, same plan"""
    table = {0: [0.25, 3.5, 3.5, 1.0], 1: [0.0, 6.0, 2.0], 2: [1e-9, 0.0]}
    seen = []

    def score(m, it, s, r, ids):
        seen.append(m)
        return table[it][: len(ids)]

    chosen = planner.ShareData(config, "m9", -1, -1, 9).nbv_loop([1e-10] * 3, 0.1, score, first_view_id=1)
    assert chosen == [1, 2, 3, 0] and set(seen) == {9}
