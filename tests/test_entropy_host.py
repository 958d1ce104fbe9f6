"""Ray entropy (method 7, PRV_SCORE_RAY_ENTROPY) without a GPU: the planner shell runs the method, the C ABI's new symbols are
declared, exported and bound, and the CPU reference of the GPU tests (tests/entropy_ref.py) gives the answers one can work
out by hand."""
import json
import os
import re
import subprocess

import numpy as np
import pytest

from nerf_prv_amd import planner
from tests import entropy_ref
from tests.test_host import GOLD, YAML

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture()
def config(tmp_path):
    p = tmp_path / "DefaultConfiguration.yaml"
    p.write_text(YAML.format(pre=tmp_path, vs=os.path.join(GOLD, "hemisphere")))
    return p


def test_method_7_is_in_scope_and_6_is_not():
    host = planner.host()
    assert host.prvh_method_in_scope(7) == 1
    assert [host.prvh_method_in_scope(m) for m in (5, 6, 8)] == [1, 0, 0]


def test_method_7_loop_with_a_stub_scorer_picks_the_argmax(config):
    """the shell treats RayEntropy like the other scored methods: every unchosen view goes to the scorer, the largest score is
    next (ties: the lowest id), the usual tree is written; `score_path: png` does not reroute it"""
    cfg = config.parent / "png.yaml"
    cfg.write_text(open(config).read() + "score_path: png\n")
    for path, name in ((config, ""), (cfg, "png")):
        sd = planner.ShareData(path, name, -1, -1, 7)
        calls = []

        def scorer(method, iteration, scene_json, render_json, ids):
            assert method == 7 and len(json.load(open(render_json))["frames"]) == len(ids)
            assert len(json.load(open(scene_json))["frames"]) == iteration + 1
            calls.append(list(ids))
            table = {0: [0.25, 3.5, 3.5, 1.0], 1: [0.0, 6.0, 2.0], 2: [1e-9, 0.0]}
            return table[iteration][: len(ids)]

        chosen = sd.nbv_loop([1e-10] * 3, 0.1, scorer, first_view_id=1)
        assert calls == [[0, 2, 3, 4], [0, 3, 4], [0, 4]]
        assert chosen == [1, 2, 3, 0]
        save = sd.string("save_path")
        assert save.endswith("_m7_v1_t0")
        for sub in ("json", "render_json", "metrics", "render", "train_time", "infer_time", "movement"):
            assert os.path.isdir(os.path.join(save, sub))
        assert sorted(os.listdir(os.path.join(save, "train_time"))) == ["0.txt", "1.txt", "2.txt"]
        assert float(open(os.path.join(save, "run_time.txt")).read()) >= 0
        assert sd.number("ensemble_num") == 5  # the yaml's: only methods 2 and 3 force theirs


def test_refusals_name_method_7(config, capfd):
    sd = planner.ShareData(config, "m6", -1, -1, 6)
    with pytest.raises(RuntimeError, match="rc=-10"):
        sd.nbv_loop([1e-10] * 3, 0.1, lambda *a: [0], first_view_id=1)
    assert "7 (RayEntropy)" in capfd.readouterr().err
    assert not os.path.exists(sd.string("save_path") + "_v1_t0")
    main = open(os.path.join(ROOT, "nerf_prv_amd", "host", "main.cpp")).read()
    assert "5 (PSNRCoverage) and 7 (RayEntropy)" in main


def test_ray_entropy_config_is_train_in_loop_with_method_7():
    strip = lambda t: [l for l in t.splitlines() if l.strip() and not l.lstrip().startswith("#")]
    a = strip(open(os.path.join(ROOT, "configs", "TrainInLoop.yaml")).read())
    b = strip(open(os.path.join(ROOT, "configs", "RayEntropy.yaml")).read())
    assert len(a) == len(b)
    assert [(x, y) for x, y in zip(a, b) if x != y] == [("method_of_IG : 3", "method_of_IG : 7")]


# ---- the reference, by hand
def test_reference_known_answers():
    H, T = entropy_ref.entropy_of_alphas([])  # an empty ray: it escapes for certain
    assert H == 0 and T == 1
    H, T = entropy_ref.entropy_of_alphas([1.0])  # one opaque sample: it stops there for certain
    assert H == 0 and T == 0
    H, T = entropy_ref.entropy_of_alphas([0.5, 1.0])  # two equal weights, no escape: one bit
    assert H == 1 and T == 0
    H, T = entropy_ref.entropy_of_alphas([0.5])  # stop or escape, even odds: one bit as well
    assert H == 1 and T == 0.5
    H, T = entropy_ref.entropy_of_alphas([0.25, 1.0 / 3.0, 0.5, 1.0])  # four equal weights: two bits (1/3 is not exact in fp32)
    assert abs(float(H) - 2.0) < 1e-6 and T == 0
    # the cut: with min_T 0.3 the ray stops after the second sample (T = 0.25) and the third never counts
    H, T = entropy_ref.entropy_of_alphas([0.5, 0.5, 0.5], min_T=0.3)
    assert T == 0.25 and H == 1.5  # weights 1/2, 1/4, escape 1/4
    # denormal weights count as 0, the smallest normal one does not
    assert entropy_ref.h_add(np.float32(1e-39), np.float32(0.75)) == np.float32(0.75)
    assert entropy_ref.h_add(np.float32(0.0), np.float32(0.75)) == np.float32(0.75)
    tiny = np.float32(2.0 ** -126)
    assert entropy_ref.h_add(tiny, np.float32(0.0)) == np.float32(126.0 * 2.0 ** -126)
    # H is at most log2(outcomes)
    rng = np.random.default_rng(3)
    for n in (3, 17, 128):
        H, _ = entropy_ref.entropy_of_alphas(rng.random(n) * 0.2)
        assert 0 < float(H) <= np.log2(n + 1) + 1e-5


# ---- the ABI
def test_new_symbols_declared_exported_and_bound():
    from nerf_prv_amd import _lib

    header = open(os.path.join(ROOT, "include", "prv.h")).read()
    text = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    m = re.search(r"\bint\s+prv_render_entropy\s*\(([^;]*)\)\s*;", text)
    assert m, "prv_render_entropy is not declared in prv.h"
    n_args = len([a for a in m.group(1).split(",") if a.strip()])
    assert n_args == 9
    out = subprocess.check_output(["nm", "-D", "--defined-only", os.path.join(ROOT, "nerf_prv_amd", "libprv_hip.so")], text=True)
    assert "prv_render_entropy" in {l.split()[-1] for l in out.splitlines() if " T " in l}
    res, args = _lib.SIGNATURES["prv_render_entropy"]
    assert len(args) == n_args
    assert _lib.load().prv_render_entropy.argtypes is not None
    assert re.search(r"#define\s+PRV_SCORE_RAY_ENTROPY\s+7\b", header)
    assert _lib.SCORE_RAY_ENTROPY == 7 and _lib.SCORE_PSNR_COVERAGE == 5
    # every function prv.h declares is bound (the new one included), and the ABI version did not move
    declared = set(re.findall(r"\b(prv_[a-z0-9_]+)\s*\(", text))
    missing = sorted(n for n in declared if n not in _lib.SIGNATURES)
    assert not missing, missing
    assert _lib.load().prv_abi_version() == 5
