"""Several next views per round on the GPU: the footprint render (prv_render_footprint, render_planes_kernel in
kRenderFootprint mode) is the entropy
render's and the depth render's bytes on every compiled field instance; the selection stage (prv_select_from_images,
prv_select_views: select_footprint_kernel, select_gain_kernel, select_mark_kernel) equals the float32 / exact-integer
restatement of tests/select_ref.py word for word; prv_planner with views_per_iteration > 1 takes several views per training
round and, with the key at 1, is the loop it was.  No tolerance anywhere: every comparison is of bytes or integers."""
import os
import subprocess

import numpy as np
import pytest

from nerf_prv_amd import api, planner
from tests import instances, select_ref, util
from tests.test_gpu_instances import load
from tests.test_gpu_planner import GOLD, ROOT, YAML

pytestmark = pytest.mark.gpu

SLOT, SLOT_SMALL = 20, 21  # slots of this file: 20..23
STAT_KEYS = ("rays", "samples_nominal", "samples_evaluated", "samples_live")
U = select_ref.UNLOCATED


def _u32(t):
    return t.cpu().numpy().view(np.uint32)


# ---- the footprint render: entropy's and depth's bytes, on every entry of tests/instances.py
FW, FH = 44, 30  # the width is no multiple of 64


@pytest.fixture(scope="module", params=list(instances.MATRIX) + list(instances.PRODUCT))
def inst(request, ctx, oracle):
    entry = instances.MATRIX.get(request.param) or instances.PRODUCT[request.param]
    m = load(ctx, oracle, SLOT, request.param, entry, want_oracle=False)
    yield m
    ctx.synthetic_model(SLOT, api.field_desc(**util.SMALL), util.SEED_A)


@pytest.fixture(scope="module")
def cams3(ctx, oracle):
    tms, scale, offset = util.hemisphere_transforms(oracle, util.fibonacci_hemisphere(6))
    cs = ctx.cameras_from_matrices(tms[[0, 2, 5]], util.FOV_X, FW, FH, scale, offset)
    yield cs
    cs.close()


@pytest.mark.parametrize("min_T", [1e-4, 0.01], ids=["T1e-4", "T0.01"])
@pytest.mark.parametrize("mode", [0, 1], ids=["fixed", "ngp"])
@pytest.mark.parametrize("spp", [1, 3], ids=["spp1", "spp3"])
def test_footprint_is_the_entropy_and_depth_renders_bit_for_bit(ctx, inst, cams3, spp, mode, min_T):
    instances.assert_layout(ctx.model_layout(SLOT), inst.entry)
    opts = api.render_opts(FW, FH, 96 if mode == 0 else 0, spp, min_T, step_mode=mode)
    ent, alpha, depth, st = ctx.render_footprint(SLOT, cams3, None, opts)
    ent0, alpha0, st_e = ctx.render_entropy(SLOT, cams3, None, opts)
    _, depth0, st_d = ctx.render_depth(SLOT, cams3, None, opts)
    assert ent.shape == (3, FH, FW) and depth.shape == (3, FH, FW)
    assert np.array_equal(_u32(ent), _u32(ent0))
    assert np.array_equal(_u32(alpha), _u32(alpha0))
    assert np.array_equal(_u32(depth), _u32(depth0))
    for k in STAT_KEYS:
        assert getattr(st, k) == getattr(st_e, k) == getattr(st_d, k), k
    assert (ent0.cpu().numpy() > 0).any() and (depth0.cpu().numpy() > 0).any()


@pytest.mark.parametrize("mode", [0, 1], ids=["fixed", "ngp"])
def test_footprint_batches_equal_one_batch(oracle, monkeypatch, mode):
    """A 1 MiB queue budget deals the three views to the queue in several batches: the engine's rule needs 1320 px x 3 x 208 B =
    823,680 B per view (one view per batch), the fixed rule 380,160 B (two views, then one).  Every plane then crosses a batch
    boundary at a non-zero first view, through its staging and its reduce: same bytes, same statistics."""
    opts = api.render_opts(FW, FH, 96 if mode == 0 else 0, 3, 1e-4, step_mode=mode)
    tms, scale, offset = util.hemisphere_transforms(oracle, util.fibonacci_hemisphere(6))

    def footprint():
        c = api.Context(0)
        try:
            c.synthetic_model(0, api.field_desc(**util.SMALL), util.SEED_A)
            cs = c.cameras_from_matrices(tms[[0, 2, 5]], util.FOV_X, FW, FH, scale, offset)
            ent, alpha, depth, st = c.render_footprint(0, cs, None, opts)
            cs.close()
            return [_u32(t).tobytes() for t in (ent, alpha, depth)], [getattr(st, k) for k in STAT_KEYS], ent.cpu().numpy(), depth.cpu().numpy()
        finally:
            c.close()

    monkeypatch.delenv("PRV_QUEUE_MB", raising=False)
    planes, stats, ent, depth = footprint()
    monkeypatch.setenv("PRV_QUEUE_MB", "1")
    planes1, stats1, _, _ = footprint()
    for name, a, b in zip(("entropy", "alpha", "depth"), planes, planes1):
        assert a == b, name
    assert stats == stats1
    assert all((ent[v] > 0).any() and (depth[v] > 0).any() for v in range(3))  # every batch rendered something


# ---- select_from_images on synthetic planes, no render
SW, SH, SN = 130, 70, 7  # a view's 9100 pixels straddle blocks and waves
DUP_FIRST, DUP_SECOND = 2, 4  # the same camera twice


@pytest.fixture(scope="module")
def cams7(ctx, oracle):
    tms, scale, offset = util.hemisphere_transforms(oracle, util.fibonacci_hemisphere(6))
    cs = ctx.cameras_from_matrices(tms[[0, 1, 2, 3, 2, 4, 5]], util.FOV_X, SW, SH, scale, offset)
    yield cs
    cs.close()


def _planes(variant):
    """(H, alpha, z), (7, 70, 130) float32 each.  The cameras sit 1.5 engine units from the cube's centre: expected depths of
    0.8..2.2 put points inside the cube, in front of it and behind it, and the outer pixels' rays miss it altogether."""
    rng = np.random.default_rng(11)
    shape = (SN, SH, SW)
    alpha = rng.uniform(0.2, 1.0, shape).astype(np.float32)  # alpha_min 0.5: a good third lies below
    z = (alpha * rng.uniform(0.8, 2.2, shape).astype(np.float32)).astype(np.float32)
    z[rng.random(shape) < 0.1] = 0.0
    H = rng.uniform(0.0, 6.0, shape).astype(np.float32)
    H[rng.random(shape) < 0.01] = np.nan
    H[rng.random(shape) < 0.01] = -1.0
    if variant == "ten":
        H[:] = 10.0  # 9100 pixels x 10 x 65536: a view's sum passes 2^32
    for p in (H, alpha, z):
        p[DUP_SECOND] = p[DUP_FIRST]
    return H, alpha, z


_want = {}


def _reference(ctx, cs, variant, G):
    """the planes and the reference's words of a (variant, grid) pair, computed once"""
    if (variant, G) not in _want:
        H, alpha, z = _planes(variant)
        words = [select_ref.footprint(ctx, cs, v, SW, SH, H[v], alpha[v], z[v], G, 0.5) for v in range(SN)]
        _want[(variant, G)] = (H, alpha, z, np.stack([w[0] for w in words]), np.stack([w[1] for w in words]))
    return _want[(variant, G)]


@pytest.mark.parametrize("variant", ["random", "ten"])
@pytest.mark.parametrize("G", [16, 128])
def test_select_from_images_equals_the_reference(ctx, cams7, G, variant):
    H, alpha, z, want_vox, want_q = _reference(ctx, cams7, variant, G)
    dev = [ctx.torch.from_numpy(p).to(ctx.device) for p in (H, alpha, z)]
    located = want_vox != U
    assert located.any() and (~located).any() and (want_vox[located] < G ** 3).all()
    assert ((alpha < 0.5) & (z > 0)).any() and (z == 0).any()  # below alpha_min, z = 0, and (the rest) outside the cube
    assert (~located & (alpha >= 0.5) & (z > 0)).any()
    if variant == "ten":
        assert int(want_q[0].astype(np.uint64).sum()) > 1 << 32
    for k in (1, 3, 7):
        so = api.select_opts(k=k, grid_res=G)
        chosen, gains, vox, q = ctx.select_from_images(cams7, None, *dev, so, want_words=True)
        assert np.array_equal(_u32(vox), want_vox) and np.array_equal(_u32(q), want_q)  # every pixel
        want_chosen, want_gains = select_ref.greedy(want_vox, want_q, k, G)
        print(f"SELECT_FIGURES {variant}/G{G}/k{k}: chosen {chosen.tolist()} gains {gains.tolist()}")
        assert chosen.tolist() == want_chosen and [int(g) for g in gains] == want_gains
        again = ctx.select_from_images(cams7, None, *dev, so, want_words=True)  # two runs: identical bytes
        assert again[0].tobytes() == chosen.tobytes() and again[1].tobytes() == gains.tobytes()
        assert _u32(again[2]).tobytes() == _u32(vox).tobytes() and _u32(again[3]).tobytes() == _u32(q).tobytes()
        if k == 7:
            assert sorted(chosen.tolist()) == list(range(SN))
            order = chosen.tolist()
            assert order.index(DUP_FIRST) < order.index(DUP_SECOND)
            # the second copy sees no voxel the first has not covered: what it still gains is its unlocated pixels'
            assert int(gains[order.index(DUP_SECOND)]) == select_ref.unlocated_sum(want_vox[DUP_SECOND], want_q[DUP_SECOND])
    # view_ids name the candidates and their order: ties go to the one listed first, the answer is in view ids
    ids = np.array([6, 4, 2, 0, 1, 3, 5], np.int32)
    so = api.select_opts(k=7, grid_res=G)
    chosen, gains = ctx.select_from_images(cams7, ids, *[d[ctx.torch.from_numpy(ids.astype(np.int64)).to(ctx.device)].contiguous() for d in dev], so)
    want_chosen, want_gains = select_ref.greedy(want_vox[ids], want_q[ids], 7, G)
    assert chosen.tolist() == [int(ids[i]) for i in want_chosen] and [int(g) for g in gains] == want_gains
    assert chosen.tolist().index(DUP_SECOND) < chosen.tolist().index(DUP_FIRST)  # listed first now


def test_select_misuse(ctx, cams7):
    H, alpha, z = (ctx.torch.zeros((SN, SH, SW), dtype=ctx.torch.float32, device=ctx.device) for _ in range(3))
    host = np.zeros((SN, SH, SW), np.float32)
    for so, planes, text in ((api.select_opts(k=8), (H, alpha, z), "k = 8"), (api.select_opts(k=0), (H, alpha, z), "at least 1"),
                             (api.select_opts(k=2, grid_res=100), (H, alpha, z), "grid_res"), (api.select_opts(k=2), (H, host, z), "device pointer")):
        with pytest.raises(api.PrvError) as e:
            ctx.select_from_images(cams7, None, *planes, so)
        assert e.value.code == api.L.PRV_E_INVALID and text in str(e.value)
    with pytest.raises(api.PrvError) as e:
        ctx.select_views(SLOT + 3, cams7, None, api.render_opts(SW, SH, 64), api.select_opts(k=2))  # an empty slot
    assert e.value.code == api.L.PRV_E_STATE
    chosen, gains = ctx.select_from_images(cams7, None, H, alpha, z, api.select_opts(k=3))  # usable afterwards; all-zero planes: ties
    assert chosen.tolist() == [0, 1, 2] and gains.tolist() == [0, 0, 0]


# ---- select_views: the render and the rounds in one call
@pytest.fixture(scope="module", params=["F4", "F2"])
def small(request, ctx):
    kw = util.SMALL if request.param == "F4" else util.SMALL_F2
    ctx.synthetic_model(SLOT_SMALL, api.field_desc(**kw), util.SEED_A)
    return request.param


@pytest.mark.parametrize("S,spp,mode", [(64, 1, 0), (0, 2, 1)], ids=["S64", "ngp_spp2"])
def test_select_views_is_the_footprint_render_then_the_rounds(ctx, small, S, spp, mode):
    w, h = 40, 30
    tms, scale, offset = planner.hemisphere_transforms(planner.hemisphere_generate(64), 0.3, 0.1, [1e-10] * 3)
    cs = ctx.cameras_from_matrices(tms[np.arange(12) * 5 + 2], util.FOV_X, w, h, scale, offset)
    opts = api.render_opts(w, h, S, spp, 0.01, step_mode=mode)
    so = api.select_opts(k=4)
    chosen, gains, st = ctx.select_views(SLOT_SMALL, cs, None, opts, so, want_stats=True)
    ent, alpha, depth, st0 = ctx.render_footprint(SLOT_SMALL, cs, None, opts)
    chosen2, gains2, vox, q = ctx.select_from_images(cs, None, ent, alpha, depth, so, want_words=True)
    assert chosen.tolist() == chosen2.tolist() and gains.tolist() == gains2.tolist()
    for k in STAT_KEYS:
        assert getattr(st, k) == getattr(st0, k), k
    ent, alpha, depth = (t.cpu().numpy() for t in (ent, alpha, depth))
    words = [select_ref.footprint(ctx, cs, v, w, h, ent[v], alpha[v], depth[v], so.grid_res, so.alpha_min) for v in range(12)]
    want_vox, want_q = np.stack([x[0] for x in words]), np.stack([x[1] for x in words])
    assert np.array_equal(_u32(vox), want_vox) and np.array_equal(_u32(q), want_q)
    assert (want_vox != U).sum() > 100 and (want_q > 0).any()  # the field is seen and located
    want_chosen, want_gains = select_ref.greedy(want_vox, want_q, 4, so.grid_res)
    print(f"SELECT_FIGURES {small}/{S}/{spp}/{mode}: chosen {chosen.tolist()} gains {gains.tolist()} located {(want_vox != U).sum()}")
    assert chosen.tolist() == want_chosen and [int(g) for g in gains] == want_gains
    assert len(set(chosen.tolist())) == 4
    cs.close()


# ---- the planner
TRAIN = ("train_steps: 40\ntrain_rays: 1024\ntrain_width: 64\ntrain_height: 36\nground_truth_seed: 4242\ntrain_deterministic: 1\n"
         "dump_scores: 1")


def _plan(tmp_path, name, extra):
    """prv_planner, mode 21, method 7 on the miniature object of tests/test_gpu_planner.py: five views, four to choose"""
    exe = os.path.join(ROOT, "nerf_prv_amd", "prv_planner")
    assert os.path.exists(exe), "prv_planner missing: run __graft_entry__.build()"
    pre = tmp_path / name
    pre.mkdir()
    cfg = pre / "cfg.yaml"
    text = YAML.format(pre=pre, vs=os.path.join(GOLD, "hemisphere"), method=7, model_source=TRAIN + extra)
    cfg.write_text(text.replace("num_of_max_iteration: 3", "num_of_max_iteration: 4"))
    out = subprocess.run([exe, str(cfg)], input="21\nobjA\n-1\n", text=True, capture_output=True, timeout=300, env=dict(os.environ, PRV_PLANNER_TIMING="1"))
    assert out.returncode == 0, out.stdout + out.stderr
    line = [l for l in out.stdout.splitlines() if l.startswith("chosen_nbvs:")][-1]
    chosen = [int(x) for x in line.split(":")[1].split()]
    trained = [int(l.split("views ")[1].split()[0]) for l in out.stderr.splitlines() if l.startswith("train_members:")]
    return pre / "Compare" / "ShapeNet" / "objA_m7_v1_t0", chosen, trained


def _tree(save, subs):
    return {f"{sub}/{f}": open(save / sub / f, "rb").read() for sub in subs for f in sorted(os.listdir(save / sub))}


def test_planner_takes_three_views_per_round(tmp_path):
    total, k = 5, 3
    save, chosen, trained = _plan(tmp_path, "batch", "\nviews_per_iteration: 3")
    assert len(chosen) == total and len(set(chosen)) == total and chosen[0] == 1
    rounds = -(-(total - 1) // k)  # ceil((total - 1) / 3) = 2: three views, then the one that is left
    moves = sorted(f for f in os.listdir(save / "movement") if f != "-1.txt")
    assert moves == [f"{i}.txt" for i in range(rounds)]
    assert trained == [1, 4]  # one training per round, on the views so far
    lines = [open(save / "movement" / f).read().splitlines() for f in moves]
    assert [len(l) for l in lines] == [3, 1]
    assert [int(l.split("\t")[0]) for ls in lines for l in ls] == chosen[1:]  # appended in selection order
    totals = [float(l.split("\t")[2]) for ls in lines for l in ls]
    legs = [float(l.split("\t")[1]) for ls in lines for l in ls]
    assert all(x > 0 for x in legs) and np.allclose(np.cumsum(legs), totals, atol=1e-5)  # the chain of legs through the chosen views
    assert sorted(os.listdir(save / "json")) == [f"{i}.json" for i in range(rounds + 1)]
    assert (save / "run_time.txt").exists() and sorted(os.listdir(save / "train_time")) == [f"{i}.txt" for i in range(rounds)]
    gains = np.frombuffer((save / "gains" / "0.bin").read_bytes(), np.uint64)
    assert len(gains) == 3 and gains[0] > 0 and gains[0] >= gains[1] >= gains[2]  # greedy gains never grow


def test_planner_with_the_key_at_1_is_the_loop_without_it(tmp_path):
    subs = ("json", "render_json", "movement", "scores", "records")
    save_a, chosen_a, trained_a = _plan(tmp_path, "plain", "")
    save_b, chosen_b, trained_b = _plan(tmp_path, "one", "\nviews_per_iteration: 1")
    assert chosen_a == chosen_b and len(chosen_a) == 5 and trained_a == trained_b == [1, 2, 3, 4]
    assert _tree(save_a, subs) == _tree(save_b, subs)
    assert not (save_b / "gains").exists()
