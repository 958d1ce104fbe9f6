"""Several views per round without a GPU: the CPU reference of the selection stage (tests/select_ref.py) gives the answers one
can work out by hand, the C ABI's new symbols are declared, exported and bound, and the planner shell reads and polices the
new yaml key."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from nerf_prv_amd import _lib, api, planner
from tests import select_ref
from tests.test_host import GOLD, YAML

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = select_ref.UNLOCATED


@pytest.fixture()
def config(tmp_path):
    p = tmp_path / "DefaultConfiguration.yaml"
    p.write_text(YAML.format(pre=tmp_path, vs=os.path.join(GOLD, "hemisphere")))
    return p


# ---- the reference, by hand
def test_of_two_identical_views_the_second_is_chosen_last():
    a = np.array([0, 1, 2, 3], np.uint32)
    b = np.array([10, 11, U, U], np.uint32)
    vox = np.stack([a, a, b])
    q = np.array([[5, 5, 5, 5], [5, 5, 5, 5], [4, 4, 1, 1]], np.uint32)
    chosen, gains = select_ref.greedy(vox, q, 3, 16)
    assert chosen == [0, 2, 1] and gains == [20, 10, 0]  # the copy sees nothing new: gain 0, after the weaker view


def test_tie_order_follows_the_view_order():
    vox = np.array([[1, 2], [3, 4], [5, 6]], np.uint32)
    q = np.full((3, 2), 7, np.uint32)
    assert select_ref.greedy(vox, q, 3, 16) == ([0, 1, 2], [14, 14, 14])
    q[2] = 8
    assert select_ref.greedy(vox, q, 2, 16) == ([2, 0], [16, 14])


def test_k_equal_n_returns_a_permutation():
    rng = np.random.default_rng(5)
    vox = rng.integers(0, 16 ** 3, (6, 50)).astype(np.uint32)
    vox[rng.random((6, 50)) < 0.3] = U
    q = rng.integers(0, 1 << 20, (6, 50)).astype(np.uint32)
    chosen, gains = select_ref.greedy(vox, q, 6, 16)
    assert sorted(chosen) == list(range(6))
    assert gains[0] == max(int(q[i].astype(np.uint64).sum()) for i in range(6))  # round 1: nothing is covered yet


def test_unlocated_gain_is_never_discounted():
    vox = np.array([[7, 7, U], [7, U, U]], np.uint32)
    q = np.array([[100, 100, 1], [50, 30, 20]], np.uint32)
    chosen, gains = select_ref.greedy(vox, q, 2, 16)
    assert chosen == [0, 1] and gains == [201, 50]  # voxel 7 is covered; the two unlocated pixels still count in full
    assert select_ref.unlocated_sum(vox[1], q[1]) == 50
    big = np.full((1, 70000), 10 * 65536, np.uint32)  # a view's sum passes 2^32: exact all the same
    assert select_ref.greedy(np.full((1, 70000), U, np.uint32), big, 1, 16)[1] == [70000 * 10 * 65536]


def test_gain_words_and_voxels_by_hand():
    H = np.array([0.0, -1.0, np.nan, 1.0, 0.5 + 2.0 ** -17, 1e9, np.inf], np.float32)
    assert select_ref.gain_words(H).tolist() == [0, 0, 0, 65536, 32768, 4294967040, 4294967040]
    o = np.tile(np.array([0.5, 0.5, -1.0], np.float32), (6, 1))
    d = np.tile(np.array([0.0, 0.0, 1.0], np.float32), (6, 1))
    cos = np.ones(6, np.float32)
    alpha = np.array([1.0, 0.5, 0.4, 1.0, 1.0, 1.0], np.float32)
    z = np.array([1.5, 0.75, 0.6, 0.0, 0.5, 2.5], np.float32)  # premultiplied: z / alpha = 1.5 where located
    vox = select_ref.voxels_from_rays(o, d, cos, alpha, z, 16, 0.5)
    mid = 8 + 16 * (8 + 16 * 8)  # the point (0.5, 0.5, 0.5) at G = 16
    assert vox.tolist() == [mid, mid, U, U, U, U]  # alpha below the bar, z = 0, a point in front of the cube, one behind it


# ---- the ABI
def test_new_symbols_declared_exported_and_bound(capfd):
    header = open(os.path.join(ROOT, "include", "prv.h")).read()
    text = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    out = subprocess.check_output(["nm", "-D", "--defined-only", os.path.join(ROOT, "nerf_prv_amd", "libprv_hip.so")], text=True)
    exported = {l.split()[-1] for l in out.splitlines() if " T " in l}
    for name, n_args in (("prv_render_footprint", 10), ("prv_select_default_opts", 1), ("prv_select_from_images", 14), ("prv_select_views", 10)):
        m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*)\)\s*;", text)
        assert m, f"{name} is not declared in prv.h"
        assert len([a for a in m.group(1).split(",") if a.strip()]) == n_args
        assert name in exported
        assert len(_lib.SIGNATURES[name][1]) == n_args
    declared = set(re.findall(r"\b(prv_[a-z0-9_]+)\s*\(", text))
    assert not sorted(n for n in declared if n not in _lib.SIGNATURES)
    lib = _lib.load()
    assert lib.prv_abi_version() == 5 and re.search(r"#define\s+PRV_ABI_VERSION\s+5\b", header)
    o = api.select_opts()
    assert (o.k, o.grid_res, o.alpha_min) == (1, 64, 0.5)
    assert C.sizeof(_lib.SelectOpts) == 12
    o = api.select_opts(k=4, grid_res=128, alpha_min=0.25)
    assert (o.k, o.grid_res, o.alpha_min) == (4, 128, 0.25)
    assert lib.prv_select_default_opts(None) == _lib.PRV_E_INVALID


@pytest.mark.parametrize("kw,text", [(dict(k=0), "k must be at least 1"), (dict(k=-3), "k must be at least 1"), (dict(k=8), "k = 8 views asked of 7"),
                                     (dict(grid_res=48), "grid_res"), (dict(grid_res=8), "grid_res"), (dict(grid_res=512), "grid_res")])
def test_bad_options_give_e_invalid_with_a_message(kw, text):
    """the options are checked before anything else, so this needs no GPU: the message is the no-context one's"""
    lib = _lib.load()
    o = api.select_opts(**kw)
    chosen = np.zeros(8, np.int32)
    rc = lib.prv_select_from_images(None, None, None, 7, 8, 8, None, None, None, C.byref(o), api._ptr(chosen), None, None, None)
    assert rc == _lib.PRV_E_INVALID and text in lib.prv_last_error(None).decode()
    ro = api.render_opts(8, 8)
    rc = lib.prv_select_views(None, 0, None, None, 7, C.byref(ro), C.byref(o), api._ptr(chosen), None, None)
    assert rc == _lib.PRV_E_INVALID and text in lib.prv_last_error(None).decode()
    rc = lib.prv_select_views(None, 0, None, None, 7, C.byref(ro), None, api._ptr(chosen), None, None)
    assert rc == _lib.PRV_E_INVALID and "NULL" in lib.prv_last_error(None).decode()


# ---- the planner shell
def test_share_data_reads_views_per_iteration_and_defaults_it_to_1(config):
    assert planner.ShareData(config, "", -1, -1, 7).number("views_per_iteration") == 1
    cfg = config.parent / "batch.yaml"
    cfg.write_text(open(config).read() + "views_per_iteration: 4\n")
    assert planner.ShareData(cfg, "", -1, -1, 7).number("views_per_iteration") == 4
    bad = config.parent / "bad.yaml"
    bad.write_text(open(config).read() + "views_per_iteration: 0\n")
    with pytest.raises(Exception, match="views_per_iteration"):
        planner.ShareData(bad, "", -1, -1, 7)


@pytest.mark.parametrize("method,extra", [(3, ""), (5, ""), (0, ""), (7, "score_path: png\n")], ids=["m3", "m5", "m0", "m7_png"])
def test_views_per_iteration_above_1_is_refused_outside_method_7_fused_and_nothing_is_written(config, capfd, method, extra):
    cfg = config.parent / "batch.yaml"
    cfg.write_text(open(config).read() + "views_per_iteration: 3\n" + extra)
    sd = planner.ShareData(cfg, "refused", -1, -1, method)
    before = sorted(os.listdir(config.parent))
    with pytest.raises(RuntimeError, match="rc=-14"):
        sd.nbv_loop([1e-10] * 3, 0.1, lambda *a: [0.0] * len(a[4]), first_view_id=1)
    err = capfd.readouterr().err
    assert "views_per_iteration 3" in err and "7 (RayEntropy)" in err and "nothing was written" in err
    assert sorted(os.listdir(config.parent)) == before and not os.path.exists(sd.string("save_path") + "_v1_t0")


def test_views_per_iteration_1_is_the_loop_as_it_was(config):
    """the key set to 1 changes nothing: the stub-scored loop of tests/test_entropy_host.py, same calls, same plan"""
    cfg = config.parent / "one.yaml"
    cfg.write_text(open(config).read() + "views_per_iteration: 1\n")
    plans = []
    for path, name in ((config, "a"), (cfg, "b")):
        sd = planner.ShareData(path, name, -1, -1, 7)
        table = {0: [0.25, 3.5, 3.5, 1.0], 1: [0.0, 6.0, 2.0], 2: [1e-9, 0.0]}
        chosen = sd.nbv_loop([1e-10] * 3, 0.1, lambda m, it, s, r, ids: table[it][: len(ids)], first_view_id=1)
        save = sd.string("save_path")
        plans.append((chosen, [open(os.path.join(save, "movement", f"{i}.txt")).read() for i in (-1, 0, 1, 2)]))
    assert plans[0] == plans[1] and plans[0][0] == [1, 2, 3, 0]


def test_batch_config_is_ray_entropy_plus_the_key():
    strip = lambda t: [l for l in t.splitlines() if l.strip() and not l.lstrip().startswith("#")]
    a = strip(open(os.path.join(ROOT, "configs", "RayEntropy.yaml")).read())
    b = strip(open(os.path.join(ROOT, "configs", "RayEntropyBatch.yaml")).read())
    assert b[: len(a)] == a and b[len(a):] == ["views_per_iteration: 4"]
