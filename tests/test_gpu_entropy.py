"""Ray entropy on the GPU (prv_render_entropy, render_planes_kernel in kRenderEntropy mode, PRV_SCORE_RAY_ENTROPY, prv_planner method 7): the opacity is
prv_render's bit for bit, the entropy is the CPU restatement's (tests/entropy_ref.py) on every compiled field instance, a fast
instance equals the generic one, calls are deterministic, the fused scoring round is the mean of the image, and the planner
picks the arg-max of those scores.

The entropy bar is |got - want| <= 1e-3 * max(|want|, entropy_ref.FLOOR); where the floor comes from, and what was measured,
is written next to it in tests/entropy_ref.py.  Every comparison prints its figures (pytest -s) before it asserts."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from nerf_prv_amd import api, planner
from tests import entropy_ref, instances, march_ref, util
from tests.test_gpu_comm import free_port
from tests.test_gpu_instances import CONFIG_IDS, CONFIGS, MIN_T, PRODUCT_STRIDE, environment, load
from tests.test_gpu_planner import GOLD, ROOT, YAML

pytestmark = pytest.mark.gpu

SLOT = 30  # slots of this file: 30..37
SLOT_TWIN, SLOT_SMALL, SLOT_PRODUCT, SLOT_ROUND = 31, 32, 33, 34
W, H = 24, 20
STAT_KEYS = ("rays", "samples_nominal", "samples_evaluated", "samples_live")


def _opts(w, h, S, spp, mode, min_T=MIN_T):
    return api.render_opts(w, h, S if mode == 0 else 0, spp, min_T, step_mode=mode)


def _both(c, slot, cs, opts, ids=None):
    """render_entropy and render of the same views -> entropy, alpha, stats, plain rgba, plain stats"""
    ent, alpha, st = c.render_entropy(slot, cs, ids, opts)
    plain, st0 = c.render(slot, cs, ids, opts)
    return ent.cpu().numpy(), alpha.cpu().numpy(), st, plain.cpu().numpy(), st0


def _check_identity(alpha, st, plain, st0):
    assert np.array_equal(alpha.view(np.uint32), plain[..., 3].view(np.uint32))  # bit for bit
    for k in STAT_KEYS:
        assert getattr(st, k) == getattr(st0, k), k


def _report(tag, got, want):
    dev, rel, need, floored = entropy_ref.stats(got, want)
    print(f"ENTROPY_FIGURES {tag}: max|got-want| {dev:.3e}  max rel (no floor) {rel:.3e}  floor a pure 1e-3 bar needs {need:.3e}  "
          f"max rel (floor {entropy_ref.FLOOR:g}) {floored:.3e}  max H {np.abs(want).max():.3f}")


def _assert_entropy(tag, got_h, got_a, want):
    """want: (..., 5) of entropy_ref (r, g, b, alpha, H).  Every pixel the reference computed is compared."""
    _report(tag, got_h, want[..., 4])
    util.assert_pixels_close(got_a, want[..., 3])
    err = entropy_ref.rel_err(got_h, want[..., 4])
    worst = np.unravel_index(np.argmax(err), err.shape)
    assert err.max() <= entropy_ref.RTOL, (f"{tag} pixel {worst}: got {np.asarray(got_h)[worst]!r}, want {want[..., 4][worst]!r}, relative error "
                                           f"{err.max():.3e} (floor {entropy_ref.FLOOR})")
    assert np.array_equal(np.asarray(got_h) == 0, want[..., 4] == 0)  # misses and dead rays: exactly 0


# ---- the matrix of compiled instances
@pytest.fixture(scope="module", params=list(instances.MATRIX))
def inst(request, ctx, oracle):
    m = load(ctx, oracle, SLOT, request.param, instances.MATRIX[request.param])
    yield m
    m.f.close()
    ctx.synthetic_model(SLOT, api.field_desc(**util.SMALL), util.SEED_A)


@pytest.fixture(scope="module")
def cams(ctx, oracle):
    tms, scale, offset = util.hemisphere_transforms(oracle, util.fibonacci_hemisphere(6))
    tms = tms[[0, 3]]
    cs = ctx.cameras_from_matrices(tms, util.FOV_X, W, H, scale, offset)
    yield cs, oracle.cameras_from_transforms(tms, util.FOV_X, W, H, scale, offset)
    cs.close()


@pytest.mark.parametrize("S,spp,mode", CONFIGS, ids=CONFIG_IDS)
def test_entropy_on_every_instance(ctx, oracle, inst, cams, S, spp, mode):
    instances.assert_layout(ctx.model_layout(SLOT), inst.entry)
    cs, ocams = cams
    ent, alpha, st, plain, st0 = _both(ctx, SLOT, cs, _opts(W, H, S, spp, mode))
    _check_identity(alpha, st, plain, st0)
    assert ent.shape == (len(ocams), H, W) and ent.dtype == np.float32
    for v, oc in enumerate(ocams):
        want = entropy_ref.reference(oracle, inst.f, oc, W, H, S, spp, MIN_T, mode)
        _assert_entropy(f"{inst.name}/{S}/{spp}/{mode}/view{v}", ent[v], alpha[v], want)
    assert (ent > 0).any()


# ---- util.SMALL, whole images (tests/test_gpu_depth.py's configurations)
@pytest.fixture(scope="module", params=["F4", "F2"])
def field(request, ctx, oracle):
    kw = util.SMALL if request.param == "F4" else util.SMALL_F2
    f = oracle.OracleField(oracle.desc(**kw), seed=util.SEED_A)
    ctx.synthetic_model(SLOT_SMALL, api.field_desc(**kw), util.SEED_A)
    yield f
    f.close()


SMALL_CONFIGS = [(128, 1, 1e-4, 0), (37, 1, 1e-4, 0), (64, 2, 1e-4, 0), (0, 1, 1e-4, 1), (64, 4, 1e-4, 0)]


@pytest.mark.parametrize("S,spp,min_T,mode", SMALL_CONFIGS, ids=["S128", "S37", "S64spp2", "ngp", "S64spp4"])
def test_entropy_whole_images(ctx, oracle, field, cams, S, spp, min_T, mode):
    cs, ocams = cams
    ent, alpha, st, plain, st0 = _both(ctx, SLOT_SMALL, cs, _opts(W, H, S, spp, mode, min_T))
    _check_identity(alpha, st, plain, st0)
    for v, oc in enumerate(ocams):
        want = entropy_ref.reference(oracle, field, oc, W, H, S, spp, min_T, mode)
        _assert_entropy(f"small/{S}/{spp}/{mode}/view{v}", ent[v], alpha[v], want)
    assert (ent > 0).any()


def test_entropy_engine_rule_default_termination(ctx, oracle, field, cams):
    """min_T 0.01 (run.py:304): a ray may stop a sample either side of the threshold -- (alpha, H) together must match one of
    the termination variants (util.assert_pixels_close_any's rule)"""
    cs, ocams = cams
    ent, alpha, st, plain, st0 = _both(ctx, SLOT_SMALL, cs, api.engine_render_opts(W, H, 0, 1, 0.01))
    _check_identity(alpha, st, plain, st0)
    for v, oc in enumerate(ocams):
        wants = [entropy_ref.reference(oracle, field, oc, W, H, 0, 1, mt, 1)[..., 3:5] for mt in util.termination_variants(0.01)]
        _report(f"small/engine/0.01/view{v}", ent[v], wants[0][..., 1])
        entropy_ref.assert_close_any(np.stack([alpha[v], ent[v]], axis=-1), wants)


# ---- the product's fields at the product's shape (tests/test_gpu_instances.py: test_product_depth's pixels)
@pytest.fixture(scope="module", params=list(instances.PRODUCT))
def product(request, ctx, oracle):
    m = load(ctx, oracle, SLOT_PRODUCT, request.param, instances.PRODUCT[request.param])
    yield m
    m.f.close()
    ctx.synthetic_model(SLOT_PRODUCT, api.field_desc(**util.SMALL), util.SEED_A)


@pytest.mark.parametrize("S,min_T", [(0, 0.01), (128, 1e-4)], ids=["engine_rule", "S128"])
def test_entropy_on_the_product_fields(ctx, oracle, product, S, min_T):
    instances.assert_layout(ctx.model_layout(SLOT_PRODUCT), product.entry)
    tms, scale, offset = planner.hemisphere_transforms(planner.hemisphere_generate(64), 0.3, 0.1, [1e-10] * 3)
    w, h = 80, 45
    cs = ctx.cameras_from_matrices(tms[[20]], util.FOV_X, w, h, scale, offset)
    oc = oracle.cameras_from_transforms(tms[[20]], util.FOV_X, w, h, scale, offset)[0]
    mode = 1 if S == 0 else 0
    ent, alpha, st, plain, st0 = _both(ctx, SLOT_PRODUCT, cs, api.engine_render_opts(w, h, S, 1, min_T))
    _check_identity(alpha, st, plain, st0)  # the whole view
    got_h, got_a = march_ref.strided(ent[0], PRODUCT_STRIDE)[:, 0], march_ref.strided(alpha[0], PRODUCT_STRIDE)[:, 0]
    assert len(got_h) * 4 >= w * h

    def ref(mt):
        return march_ref.strided(entropy_ref.reference(oracle, product.f, oc, w, h, S, 1, mt, mode, PRODUCT_STRIDE), PRODUCT_STRIDE)

    if min_T == 0.01:
        wants = [ref(mt)[:, 3:5] for mt in util.termination_variants(min_T)]
        _report(f"{product.name}/engine", got_h, wants[0][:, 1])
        entropy_ref.assert_close_any(np.stack([got_a, got_h], axis=-1), wants)
    else:
        _assert_entropy(f"{product.name}/S128", got_h, got_a, ref(min_T))
    assert (got_h > 0).sum() > 50
    cs.close()


# ---- opacity and statistics are prv_render's: both rules, spp 1 and 16, relocation on and off, a lens camera
@pytest.mark.parametrize("env", [{"PRV_MERGE_MAX": "31", "PRV_POOL": "1"}, {"PRV_MERGE_MAX": "0"}], ids=["merge31_pool", "merge0"])
@pytest.mark.parametrize("name", ["F4_5", "F2_10", "F4_0"])
def test_opacity_is_the_colour_kernels_bit_for_bit(ctx, oracle, name, env):
    from tests.test_gpu_parity import REF_INTR

    entry = instances.MATRIX[name]
    tms, scale, offset = util.hemisphere_transforms(oracle, util.fibonacci_hemisphere(6))
    with environment(env):
        c = api.Context(0)
        c.synthetic_model(0, api.field_desc(**entry.kw), util.SEED_B)
    try:
        instances.assert_layout(c.model_layout(0), entry)
        ctx.synthetic_model(SLOT_TWIN, api.field_desc(**entry.kw), util.SEED_B)  # the session context: its own relocation policy
        w, h = 96, 80
        cs = c.cameras_from_matrices(tms, util.FOV_X, w, h, scale, offset)
        cs0 = ctx.cameras_from_matrices(tms, util.FOV_X, w, h, scale, offset)
        lens = c.cameras_from_matrices_intr(tms[[1, 4]], REF_INTR, scale, offset)
        for mode in (1, 0):
            for spp in (1, 16):
                opts = _opts(w, h, 128, spp, mode)
                ent, alpha, st, plain, st0 = _both(c, 0, cs, opts)
                _check_identity(alpha, st, plain, st0)
                assert (ent > 0).any() and (ent[alpha == 0] == 0).all()
                assert (ent >= 0).all()
                # which lane composites a ray does not change its entropy: the session context's policy gives the same bytes
                ent0, alpha0, _ = ctx.render_entropy(SLOT_TWIN, cs0, None, opts)
                assert np.array_equal(ent0.cpu().numpy().view(np.uint32), ent.view(np.uint32))
                assert np.array_equal(alpha0.cpu().numpy().view(np.uint32), alpha.view(np.uint32))
            lo = _opts(64, 36, 96, 1, mode)
            ent, alpha, st, plain, st0 = _both(c, 0, lens, lo)
            _check_identity(alpha, st, plain, st0)
            assert (ent > 0).any()
        for x in (cs, lens):
            x.close()
        cs0.close()
    finally:
        c.close()


# ---- a fast instance and the generic one: identical bytes
@pytest.mark.parametrize("name", instances.FAST)
def test_fast_equals_generic_entropy(ctx, oracle, name):
    entry = instances.MATRIX[name]
    load(ctx, oracle, SLOT_TWIN, name, entry, want_oracle=False)
    with environment({"PRV_NO_PAIR": "1"}):
        other = api.Context(0)
        other.synthetic_model(0, api.field_desc(**entry.kw), util.SEED_A)
    try:
        instances.assert_layout(other.model_layout(0), entry, no_pair=True)
        tms, scale, offset = util.hemisphere_transforms(oracle, util.fibonacci_hemisphere(5))
        w, h = 56, 44
        for mode in (0, 1):
            outs = []
            for c, slot in ((ctx, SLOT_TWIN), (other, 0)):
                cs = c.cameras_from_matrices(tms, util.FOV_X, w, h, scale, offset)
                ent, alpha, st, plain, st0 = _both(c, slot, cs, _opts(w, h, 96, 1, mode))
                _check_identity(alpha, st, plain, st0)
                outs.append((ent, alpha, int(st.samples_evaluated), int(st.samples_live)))
                cs.close()
            a, b = outs
            assert np.array_equal(a[0].view(np.uint32), b[0].view(np.uint32))
            assert np.array_equal(a[1].view(np.uint32), b[1].view(np.uint32))
            assert a[2] == b[2] > 0 and a[3] == b[3] > 0 and (a[0] > 0).any()
    finally:
        other.close()
        ctx.synthetic_model(SLOT_TWIN, api.field_desc(**util.SMALL), util.SEED_A)


# ---- determinism
def _round_scene(c, slot=SLOT_ROUND, n_views=11, w=40, h=24):
    c.synthetic_model(slot, api.field_desc(**util.SMALL), 777)
    tms, scale, offset = planner.hemisphere_transforms(util.fibonacci_hemisphere(n_views), 0.3, 0.1, [1e-10] * 3)
    return c.cameras_from_matrices(tms, util.FOV_X, w, h, scale, offset)


@pytest.mark.parametrize("S,spp,mode", [(64, 1, 0), (0, 2, 1)], ids=["S64", "ngp_spp2"])
def test_entropy_is_deterministic_and_batches_equal_single_views(ctx, monkeypatch, S, spp, mode):
    cs = _round_scene(ctx)
    opts = _opts(40, 24, S, spp, mode, 0.01)
    a_h, a_a, _ = ctx.render_entropy(SLOT_ROUND, cs, None, opts)
    b_h, b_a, _ = ctx.render_entropy(SLOT_ROUND, cs, None, opts)
    a_h, a_a = a_h.cpu().numpy(), a_a.cpu().numpy()
    assert a_h.tobytes() == b_h.cpu().numpy().tobytes() and a_a.tobytes() == b_a.cpu().numpy().tobytes()
    for v in (0, 5, 10):
        h1, a1, _ = ctx.render_entropy(SLOT_ROUND, cs, [v], opts)
        assert h1.cpu().numpy()[0].tobytes() == a_h[v].tobytes() and a1.cpu().numpy()[0].tobytes() == a_a[v].tobytes()
    h2, a2, _ = ctx.render_entropy(SLOT_ROUND, cs, [7, 2], opts)
    assert np.array_equal(h2.cpu().numpy(), a_h[[7, 2]]) and np.array_equal(a2.cpu().numpy(), a_a[[7, 2]])
    # out_alpha may be NULL
    lib, ids = ctx.lib, np.arange(len(cs), dtype=np.int32)
    out = ctx.torch.empty((len(cs), 24, 40), dtype=ctx.torch.float32, device=ctx.device)
    assert lib.prv_render_entropy(ctx.handle, SLOT_ROUND, cs.handle, api._ptr(ids), len(ids), C.byref(opts), api._ptr(out), None, None) == 0
    assert out.cpu().numpy().tobytes() == a_h.tobytes()
    # a small queue budget deals the views to the queue in several batches: same bytes
    monkeypatch.setenv("PRV_QUEUE_MB", "1")
    c2 = api.Context(0)
    try:
        cs2 = _round_scene(c2, 0)
        h3, a3, _ = c2.render_entropy(0, cs2, None, opts)
        assert h3.cpu().numpy().tobytes() == a_h.tobytes() and a3.cpu().numpy().tobytes() == a_a.tobytes()
        cs2.close()
    finally:
        c2.close()
    assert (a_h > 0).any()
    cs.close()


# ---- the fused round
@pytest.mark.parametrize("S,spp,mode", [(64, 1, 0), (64, 2, 0), (0, 16, 1)], ids=["S64", "S64spp2", "ngp_spp16"])
def test_score_views_ray_entropy_is_the_mean_of_the_image(ctx, S, spp, mode):
    cs = _round_scene(ctx)
    opts = _opts(40, 24, S, spp, mode, 0.01)
    ent, alpha, st_img = ctx.render_entropy(SLOT_ROUND, cs, None, opts)
    ent, alpha = ent.cpu().numpy().astype(np.float64), alpha.cpu().numpy().astype(np.float64)
    rec, st = ctx.score_views(api.L.SCORE_RAY_ENTROPY, [SLOT_ROUND], cs, None, opts, want_stats=True)
    want = ent.reshape(len(cs), -1).mean(axis=1)
    # fp64 sums of 960 fp32 values in another order: equal to a few ulp of the double
    np.testing.assert_allclose(rec["score"], want, rtol=1e-13, atol=0)
    np.testing.assert_allclose(rec["coverage"], alpha.reshape(len(cs), -1).mean(axis=1).astype(np.float32), rtol=1e-6)
    assert (rec["psnr"] == 0).all() and (rec["score"] > 0).all() and len(set(rec["score"])) == len(cs)
    for k in STAT_KEYS:
        assert getattr(st, k) == getattr(st_img, k), k
    # larger is chosen first: the ranking is rank_host's on those scores; argmax is its head
    ids = np.arange(len(cs), dtype=np.int32)
    order = ctx.rank(rec, ids)
    assert list(order) == list(api.rank_host(rec, ids))
    assert list(order) == sorted(ids, key=lambda i: (-rec["score"][i], i)) and ctx.argmax(rec, ids) == order[0]
    # deterministic, a subset of the views gives those views' records, device records equal the host's
    rec2, _ = ctx.score_views(api.L.SCORE_RAY_ENTROPY, [SLOT_ROUND], cs, None, opts)
    assert rec2.tobytes() == rec.tobytes()
    sub, _ = ctx.score_views(api.L.SCORE_RAY_ENTROPY, [SLOT_ROUND], cs, [9, 0, 4], opts)
    assert sub.tobytes() == rec[[9, 0, 4]].tobytes()
    dev = ctx.torch.zeros((len(cs), 16), dtype=ctx.torch.uint8, device=ctx.device)
    ctx.score_views(api.L.SCORE_RAY_ENTROPY, [SLOT_ROUND], cs, None, opts, records_dev=dev, to_host=False)
    assert dev.cpu().numpy().tobytes() == rec.tobytes()
    # one rank without a communicator: the sharded entry point is the plain round
    one = np.zeros(len(cs), api.RECORD_DTYPE)
    slots = np.array([SLOT_ROUND], np.int32)
    assert ctx.lib.prv_score_views_sharded(ctx.handle, None, api.L.SCORE_RAY_ENTROPY, api._ptr(slots), 1, cs.handle, len(cs), 1, C.byref(opts),
                                           None, api._ptr(one), None) == 0
    assert one.tobytes() == rec.tobytes()
    cs.close()


def test_score_views_ray_entropy_misuse(ctx):
    cs = _round_scene(ctx)
    opts = _opts(40, 24, 64, 1, 0, 0.01)
    gt = ctx.torch.zeros((len(cs), 24, 40, 4), dtype=ctx.torch.float32, device=ctx.device)
    cases = [([SLOT_ROUND, SLOT_ROUND], None, api.L.PRV_E_INVALID, "one model"),  # n_models != 1
             ([SLOT_ROUND], gt, api.L.PRV_E_INVALID, "no reference images"),      # a non-NULL gt
             ([SLOT + 7], None, api.L.PRV_E_STATE, "")]                           # an empty slot
    for slots, g, code, text in cases:
        with pytest.raises(api.PrvError) as e:
            ctx.score_views(api.L.SCORE_RAY_ENTROPY, slots, cs, None, opts, gt=g)
        assert e.value.code == code and text in str(e.value) and len(str(e.value)) > 10, (slots, str(e.value))
    with pytest.raises(api.PrvError) as e:
        ctx.score_views(6, [SLOT_ROUND], cs, None, opts)  # 6 is no method
    assert e.value.code == api.L.PRV_E_INVALID
    ids = np.array([0], np.int32)
    host = np.zeros((1, 24, 40), np.float32)
    out = ctx.torch.empty((1, 24, 40), dtype=ctx.torch.float32, device=ctx.device)
    call = lambda slot, n, o, a: ctx.lib.prv_render_entropy(ctx.handle, slot, cs.handle, api._ptr(ids), n, C.byref(opts), api._ptr(o), api._ptr(a), None)
    assert call(SLOT_ROUND, 1, None, out) == api.L.PRV_E_INVALID  # no entropy output
    assert call(SLOT_ROUND, 0, None, None) == 0  # nothing to render
    assert call(SLOT + 7, 1, out, None) == api.L.PRV_E_STATE
    assert call(SLOT_ROUND, 1, host, None) == api.L.PRV_E_INVALID and call(SLOT_ROUND, 1, out, host) == api.L.PRV_E_INVALID
    assert not host.any()
    rec, _ = ctx.score_views(api.L.SCORE_RAY_ENTROPY, [SLOT_ROUND], cs, None, opts)  # the context is usable afterwards
    assert (rec["score"] > 0).all()
    cs.close()


def _entropy_comm_worker(rank, world, port, outdir):
    """one of two processes on the one GPU: own context, socket transport (tests/test_gpu_comm.py's pattern)"""
    c = api.Context(0)
    comm = api.Comm(c, rank, world, transport="socket", rendezvous=f"127.0.0.1:{port}")
    try:
        cs = _round_scene(c, 0)
        opts = _opts(40, 24, 64, 2, 0, 0.01)
        rec_i, st = comm.score_views(api.L.SCORE_RAY_ENTROPY, [0], cs, len(cs), opts, interleaved=True, want_stats=True)
        rec_b, _ = comm.score_views(api.L.SCORE_RAY_ENTROPY, [0], cs, len(cs), opts, interleaved=False)
        np.savez(os.path.join(outdir, f"rank{rank}.npz"), rec_i=rec_i.view(np.uint8), rec_b=rec_b.view(np.uint8), evaluated=st.samples_evaluated)
        comm.barrier()
    finally:
        comm.close()
        c.close()


def test_two_processes_on_one_gpu_score_ray_entropy(ctx, tmp_path):
    import torch.multiprocessing as mp

    port = free_port()
    mctx = mp.get_context("spawn")
    procs = [mctx.Process(target=_entropy_comm_worker, args=(r, 2, port, str(tmp_path))) for r in range(2)]
    for p in procs:
        p.start()
    for p in procs:
        p.join(timeout=300)
        assert p.exitcode == 0
    r0, r1 = (np.load(tmp_path / f"rank{r}.npz") for r in range(2))
    cs = _round_scene(ctx)
    want, st = ctx.score_views(api.L.SCORE_RAY_ENTROPY, [SLOT_ROUND], cs, None, _opts(40, 24, 64, 2, 0, 0.01), want_stats=True)
    for r in (r0, r1):
        assert r["rec_i"].tobytes() == want.tobytes() and r["rec_b"].tobytes() == want.tobytes()
    assert int(r0["evaluated"]) + int(r1["evaluated"]) == st.samples_evaluated
    cs.close()


# ---- the planner
def test_planner_method_7_trains_one_member_and_picks_the_largest_entropy(ctx, tmp_path):
    """prv_planner, mode 21, method_of_IG 7 on the miniature object of tests/test_gpu_planner.py with deterministic training:
    the loop completes and writes the usual tree; one member is trained per iteration and no reference image is made; every
    decision is the arg-max of Context.score_views(SCORE_RAY_ENTROPY) on the member that iteration saved.
    configs/RayEntropy.yaml is this loop at the reference's sizes (tests/test_entropy_host.py pins its keys)."""
    exe = os.path.join(ROOT, "nerf_prv_amd", "prv_planner")
    assert os.path.exists(exe), "prv_planner missing: run __graft_entry__.build()"
    pre = tmp_path / "m7"
    pre.mkdir()
    cfg = pre / "cfg.yaml"
    cfg.write_text(YAML.format(pre=pre, vs=os.path.join(GOLD, "hemisphere"), method=7,
                               model_source="train_steps: 40\ntrain_rays: 1024\ntrain_width: 64\ntrain_height: 36\nground_truth_seed: 4242\n"
                                            "train_deterministic: 1\nsave_members: 1\ndump_scores: 1"))
    env = dict(os.environ, PRV_PLANNER_TIMING="1")
    out = subprocess.run([exe, str(cfg)], input="21\nobjA\n-1\n", text=True, capture_output=True, timeout=300, env=env)
    assert out.returncode == 0, out.stdout + out.stderr
    line = [l for l in out.stdout.splitlines() if l.startswith("chosen_nbvs:")][-1]
    chosen = [int(x) for x in line.split(":")[1].split()]
    assert len(chosen) == 4 and len(set(chosen)) == 4 and chosen[0] == 1
    save = pre / "Compare" / "ShapeNet" / "objA_m7_v1_t0"
    for sub in ("json", "render_json", "metrics", "render", "train_time", "infer_time", "movement"):
        assert (save / sub).is_dir()
    assert (save / "run_time.txt").exists() and (save / "json" / "3.json").exists() and (save / "train_time" / "2.txt").exists()
    trained = [l for l in out.stderr.splitlines() if l.startswith("train_members:")]
    assert [int(l.split("views ")[1].split()[0]) for l in trained] == [1, 2, 3]  # one training per iteration, on the views so far
    assert not [p for p in pre.rglob("*_render.json")]  # method 5's reference-image set is not made
    opts = api.render_opts(80, 45, 64, 2, 0.01, background=(0, 0, 0, 1))
    for it in range(3):
        assert sorted(os.listdir(save / "members" / str(it))) == ["member_0.prvf"]
        ctx.load_model_file(SLOT_ROUND, save / "members" / str(it) / "member_0.prvf")
        cs = ctx.cameras_from_json(save / "render_json" / f"{it}.json")
        candidates = [v for v in range(5) if v not in chosen[: it + 1]]
        assert len(cs) == len(candidates)
        rec, _ = ctx.score_views(api.L.SCORE_RAY_ENTROPY, [SLOT_ROUND], cs, None, opts)
        dumped = np.frombuffer((save / "scores" / f"{it}.bin").read_bytes(), np.float64)
        assert dumped.tobytes() == rec["score"].tobytes()  # the loop scored this member, with these options
        records = np.frombuffer((save / "records" / f"{it}.bin").read_bytes(), api.RECORD_DTYPE)
        assert records.tobytes() == rec.tobytes()
        assert chosen[it + 1] == candidates[int(np.argmax(rec["score"]))] == ctx.argmax(rec, np.array(candidates, np.int32))
        assert (rec["score"] > 0).all()
        cs.close()
    # the same run again gives the same plan (deterministic training, deterministic scores)
    pre2 = tmp_path / "m7_again"
    pre2.mkdir()
    cfg2 = pre2 / "cfg.yaml"
    cfg2.write_text(cfg.read_text().replace(str(pre), str(pre2)))
    out2 = subprocess.run([exe, str(cfg2)], input="21\nobjA\n-1\n", text=True, capture_output=True, timeout=300)
    assert out2.returncode == 0, out2.stdout + out2.stderr
    assert [l for l in out2.stdout.splitlines() if l.startswith("chosen_nbvs:")][-1] == line
