"""Termination histograms and the Jensen-Shannon view score on the GPU: prv_render_termination (render_planes_kernel in
kRenderTermination mode) against the CPU reference of tests/termination_ref.py on every compiled field instance, its bin edges,
exact placement, independence of where a ray is composited, consistency with the entropy and footprint renders; the reduce
kernel (prv_termination_divergence) on synthetic planes; prv_score_views method 9 against the reference pipeline; misuse.

Against the reference: alpha and the statistics are prv_render_entropy's, byte for byte; every bin plane is within the project's
pixel bar of the reference at one of the thresholds of util.termination_variants(min_T) (a ray may stop one sample either side)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from nerf_prv_amd import api
from tests import instances, march_ref, surface_ref, termination_ref as tr, util
from tests.surface_ref import FH, FW
from tests.test_gpu_comm import free_port
from tests.test_gpu_instances import environment, load
from tests.test_gpu_planner import GOLD, ROOT, YAML
from tests.test_gpu_select import STAT_KEYS, _u32

pytestmark = pytest.mark.gpu

SLOT, SLOT_SMALL, SLOT_MEMBER = 12, 13, 14  # slots of this file: 12..19 (the ensemble's members: 14..18)
MIN_T = 1e-4
S_FIXED = surface_ref.S_FIXED
f32 = np.float32


def _opts(S, spp, mode, w=FW, h=FH, min_T=MIN_T):
    return api.render_opts(w, h, S if mode == 0 else 0, spp, min_T, step_mode=mode)


def _termination(c, slot, cs, opts, K, ids=None):
    bins, alpha, st = c.render_termination(slot, cs, ids, opts, K)
    return bins.cpu().numpy(), alpha.cpu().numpy(), st


def _views(ctx, oracle, w=FW, h=FH):
    tms, scale, offset = surface_ref.case_transforms(oracle)  # views 0 and 3 of the six-view hemisphere
    return (ctx.cameras_from_matrices(tms, util.FOV_X, w, h, scale, offset),
            oracle.cameras_from_transforms(tms, util.FOV_X, w, h, scale, offset))


def _assert_against_reference(got_bins, got_alpha, want, tag):
    """got_bins [K, h, w], got_alpha [h, w]; want [3, h, w, K + 1]: every pixel (all planes together) matches one variant"""
    got = np.concatenate([np.moveaxis(got_bins, 0, -1), got_alpha[..., None]], axis=-1)
    n_variant = util.assert_pixels_close_any(got, list(want))
    dev = np.abs(got.astype(np.float64) - want.astype(np.float64)).max(axis=-1).min(axis=0).max()
    rel = np.stack([util.pixel_rel_err(got, w).max(axis=-1) for w in want]).min(axis=0).max()
    print(f"TERMINATION_FIGURES {tag}: largest |got - want| {dev:.3e}, largest floored relative error {rel:.3e}, {n_variant} pixels match only a variant")


def _check_case(ctx, oracle, m, slot, cs, ocams, mode, S, K, spps):
    refs = {}
    for v, oc in enumerate(ocams):  # one march serves every spp: sub-sample k's offset does not depend on spp
        sub, live = tr.render_variants(oracle.lib(), m.f, oc, FW, FH, K, [f32(t) for t in util.termination_variants(MIN_T)], S, max(spps), mode)
        refs[v] = (sub, live)
    for spp in spps:
        opts = _opts(S, spp, mode)
        bins, alpha, st = _termination(ctx, slot, cs, opts, K)
        _, alpha0, st0 = ctx.render_entropy(slot, cs, None, opts)
        assert np.array_equal(alpha.view(np.uint32), _u32(alpha0))
        for k in STAT_KEYS:
            assert getattr(st, k) == getattr(st0, k), k
        for v, oc in enumerate(ocams):
            sub, live = refs[v]
            want = np.stack([tr.mean(sub[j, :spp]) for j in range(sub.shape[0])])
            march_ref.assert_alpha_is_the_oracles(m.f, oc, FW, FH, S, spp, MIN_T, mode, want[0][..., K])
            _assert_against_reference(bins[:, v], alpha[v], want, f"{m.name}/{'ngp' if mode else 'S%d' % S}/K{K}/spp{spp}/view{v}")
            untouched = ~live[:spp].any(axis=0)  # [h, w, K]: bins no live sample of any sub-sample falls in
            assert not np.moveaxis(bins[:, v], 0, -1)[untouched].any()
            dead = alpha[v] == 0
            assert dead.any() and not bins[:, v][:, dead].any()
        assert (bins > 0).any() and st.samples_evaluated > 0


# ---- 1. against the reference, on every compiled instance
@pytest.mark.parametrize("mode", [0, 1], ids=["fixed", "ngp"])
@pytest.mark.parametrize("name", list(instances.MATRIX))
def test_termination_against_the_reference(ctx, oracle, name, mode):
    m = load(ctx, oracle, SLOT, name, instances.MATRIX[name])
    cs, ocams = _views(ctx, oracle)
    try:
        _check_case(ctx, oracle, m, SLOT, cs, ocams, mode, S_FIXED, 16, (1, 3))
    finally:
        cs.close()
        m.f.close()
        ctx.synthetic_model(SLOT, api.field_desc(**util.SMALL), util.SEED_A)


# ---- 2. bin edges
@pytest.mark.parametrize("mode,S", [(0, 37), (0, 128), (1, 0)], ids=["S37", "S128", "ngp"])
@pytest.mark.parametrize("K", [4, 64])
@pytest.mark.parametrize("name", ["F4_5", "F2_10"])
def test_termination_bin_edges(ctx, oracle, name, K, mode, S):
    m = load(ctx, oracle, SLOT, name, instances.MATRIX[name])
    cs, ocams = _views(ctx, oracle)
    try:
        _check_case(ctx, oracle, m, SLOT, cs, ocams, mode, S, K, (1,))
    finally:
        cs.close()
        m.f.close()
        ctx.synthetic_model(SLOT, api.field_desc(**util.SMALL), util.SEED_A)


# ---- 3. exact placement: two slabs of occupancy, everything else exactly 0
@pytest.mark.parametrize("mode", [0, 1], ids=["fixed", "ngp"])
def test_termination_places_weights_in_the_bins_of_live_samples_only(ctx, oracle, mode):
    kw = dict(util.SMALL, density_bias=4.5)
    params = surface_ref.two_shell_params(oracle, kw, util.SEED_A)
    ctx.load_model(SLOT_SMALL, api.field_desc(**kw), *params)
    f = oracle.OracleField(oracle.desc(**kw), params=params)
    w, h, S, K = surface_ref.SHELL_W, surface_ref.SHELL_H, surface_ref.SHELL_S, 16
    tms, scale, offset = util.hemisphere_transforms(oracle, util.fibonacci_hemisphere(6))
    cs = ctx.cameras_from_matrices(tms[[0, 3]], util.FOV_X, w, h, scale, offset)
    ocams = oracle.cameras_from_transforms(tms[[0, 3]], util.FOV_X, w, h, scale, offset)
    try:
        bins, alpha, _ = _termination(ctx, SLOT_SMALL, cs, api.render_opts(w, h, S if mode == 0 else 0, 1, MIN_T, step_mode=mode), K)
        n_empty = 0
        for v, oc in enumerate(ocams):
            # min_T = 0 walks every live sample: a bin is live where ANY live sample falls in it, composited or cut
            _, live = tr.render_variants(oracle.lib(), f, oc, w, h, K, [f32(0)], S, 1, mode)
            live = live[0]
            got = np.moveaxis(bins[:, v], 0, -1)
            assert not got[~live].any()  # exactly 0.0
            dead = ~live.any(axis=-1)
            assert dead.any() and not got[dead].any() and not alpha[v][dead].any()
            n_empty += int((~live).sum())
            assert (got[live] > 0).any()
        print(f"TERMINATION_PLACEMENT_FIGURES mode {mode}: {n_empty} bins exactly 0")
        assert n_empty > K * w * h  # the slabs leave most bins of most pixels empty
    finally:
        cs.close()
        f.close()
        ctx.synthetic_model(SLOT_SMALL, api.field_desc(**util.SMALL), util.SEED_A)


# ---- 4. relocation and batching lose or duplicate no flush
@pytest.mark.parametrize("mode", [0, 1], ids=["fixed", "ngp"])
def test_termination_batches_and_relocation_change_no_byte(oracle, monkeypatch, mode):
    opts = _opts(96, 3, mode)
    tms, scale, offset = util.hemisphere_transforms(oracle, util.fibonacci_hemisphere(6))

    def render(views):
        c = api.Context(0)
        try:
            c.synthetic_model(0, api.field_desc(**util.SMALL), util.SEED_A)
            cs = c.cameras_from_matrices(tms[views], util.FOV_X, FW, FH, scale, offset)
            bins, alpha, st = _termination(c, 0, cs, opts, 16)
            cs.close()
            return bins, alpha, [getattr(st, k) for k in STAT_KEYS]
        finally:
            c.close()

    for k in ("PRV_QUEUE_MB", "PRV_MERGE_MAX", "PRV_POOL"):
        monkeypatch.delenv(k, raising=False)
    six = list(range(6))
    bins, alpha, stats = render(six)
    assert all((bins[:, v] > 0).any() for v in six)
    for env in ({"PRV_QUEUE_MB": "1"}, {"PRV_MERGE_MAX": "31", "PRV_POOL": "1"}, {"PRV_MERGE_MAX": "0", "PRV_POOL": "0"},
                {"PRV_QUEUE_MB": "1", "PRV_MERGE_MAX": "31", "PRV_POOL": "1"}):
        with environment(env):
            bins1, alpha1, stats1 = render(six)
        assert bins1.tobytes() == bins.tobytes() and alpha1.tobytes() == alpha.tobytes(), env
        assert stats1[:2] == stats[:2] and stats1[3] == stats[3], env
    for env in ({}, {"PRV_MERGE_MAX": "31", "PRV_POOL": "1"}):  # one view alone = its planes in the batch of six
        with environment(env):
            b1, a1, _ = render([4])
        assert b1[:, 0].tobytes() == bins[:, 4].tobytes() and a1[0].tobytes() == alpha[4].tobytes(), env


# ---- 5. consistency with what exists
def test_termination_is_consistent_with_entropy_and_footprint(ctx, oracle):
    ctx.synthetic_model(SLOT_SMALL, api.field_desc(**dict(util.SMALL, density_bias=6.0)), util.SEED_A)
    cs, ocams = _views(ctx, oracle)
    S, K = 128, 16
    try:
        for mode in (0, 1):
            opts = _opts(S, 1, mode)
            bins, alpha, _ = _termination(ctx, SLOT_SMALL, cs, opts, K)
            total = bins.astype(np.float64).sum(axis=0)
            worst = np.abs(total - alpha.astype(np.float64)).max()
            print(f"TERMINATION_SUM_FIGURES mode {mode}: largest |sum of bins - alpha| {worst:.3e}")
            assert worst <= (K + 1) * 2.0 ** -24 * 2
            _, alpha_f, depth, _ = ctx.render_footprint(SLOT_SMALL, cs, None, opts)
            assert np.array_equal(_u32(alpha_f), alpha.view(np.uint32))
            depth = depth.cpu().numpy()
            n = 0
            for v, oc in enumerate(ocams):
                o, d, t = ctx.debug_raygen(cs, v, FW, FH)
                t0, t1 = t[:, 0].reshape(FH, FW).astype(np.float64), t[:, 1].reshape(FH, FW).astype(np.float64)
                cos = np.array([march_ref.forward_cos(oc, di) for di in d], np.float64).reshape(FH, FW)
                # bin k holds steps [k n_max / K, (k + 1) n_max / K): its middle in t, and the width of a bin
                width = (t1 - t0) / K if mode == 0 else float(march_ref.NGP_DT) * march_ref.NGP_STEPS / K
                solid = alpha[v] >= 0.5
                assert solid.sum() > 20
                centre = (bins[:, v].astype(np.float64) * (np.arange(K) + 0.5)[:, None, None]).sum(axis=0)[solid] / total[v][solid]
                t_hist = t0[solid] + centre * (width[solid] if mode == 0 else width)
                t_foot = depth[v][solid].astype(np.float64) / alpha[v][solid] / cos[solid]
                assert (np.abs(t_hist - t_foot) <= (width[solid] if mode == 0 else width)).all()
                n += int(solid.sum())
            print(f"TERMINATION_DEPTH_FIGURES mode {mode}: {n} pixels, centroid within one bin of the footprint's expected depth")
    finally:
        cs.close()
        ctx.synthetic_model(SLOT_SMALL, api.field_desc(**util.SMALL), util.SEED_A)


# ---- 6. the reduce kernel on synthetic planes
def _dev(ctx, a):
    return ctx.torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(ctx.device)


def _divergence(ctx, bins, alphas):
    """bins [E, K, n, h, w], alphas [E, n, h, w] (numpy) -> (J [n, h, w], view J [n], view opacity [n])"""
    out, vj, vo = ctx.termination_divergence([_dev(ctx, b) for b in bins], [_dev(ctx, a) for a in alphas])
    return out.cpu().numpy(), vj, vo


def test_divergence_of_identical_members_is_exactly_zero(ctx):
    rng = np.random.default_rng(5)
    n, h, w, K = 2, 9, 31, 16
    p = rng.dirichlet(np.full(K + 1, 0.3), size=(n, h, w)).astype(np.float32)  # [n, h, w, K + 1]
    bins = np.moveaxis(p[..., :K], -1, 0)
    alpha = (f32(1) - p[..., K]).astype(np.float32)
    J, vj, vo = _divergence(ctx, [bins, bins.copy()], [alpha, alpha.copy()])
    assert not J.any() and not vj.any()
    assert np.allclose(vo, alpha.astype(np.float64).reshape(n, -1).mean(axis=1), rtol=1e-6)


def test_divergence_hand_made_cases(ctx):
    for name, bins, alphas, want in tr.hand_made_cases():
        E = bins.shape[0]
        J, vj, _ = _divergence(ctx, bins, alphas)
        assert abs(float(J[0, 0, 0]) - want) <= 1e-6 and abs(vj[0] - want) <= 1e-6, (name, J, want)
        assert J.max() <= np.log2(E) + 1e-6, name
        assert abs(float(tr.jsd(bins, alphas)[0, 0, 0]) - want) <= 1e-12, name


def test_divergence_against_the_float64_restatement(ctx):
    worst = 0.0
    for E in (2, 3, 5, 8):
        for K in (4, 16, 64):
            rng = np.random.default_rng(100 * E + K)
            n, h, w = 2, 17, 33  # more than one block's worth of lanes per view would need 256 x blocks pixels: 561 do for two
            p = rng.dirichlet(np.full(K + 1, 0.2), size=(E, n, h, w)).astype(np.float32)
            p[:, :, :2] = 0  # dead rows: every member empty, alpha 0
            bins = np.moveaxis(p[..., :K], -1, 1)  # [E, K, n, h, w]
            alphas = np.where(p.sum(axis=-1) > 0, f32(1) - p[..., K], f32(0)).astype(np.float32)
            J, vj, vo = _divergence(ctx, bins, alphas)
            want = tr.jsd(bins, alphas)
            dev = float(np.abs(J.astype(np.float64) - want).max())
            worst = max(worst, dev)
            print(f"TERMINATION_JSD_FIGURES E {E} K {K}: largest |J - float64| {dev:.3e} bits (largest J {want.max():.3f})")
            assert dev <= tr.JSD_ATOL
            assert want.max() <= np.log2(E) and J.max() <= np.log2(E) + tr.JSD_ATOL and not J[:, :2].any()
            wj, wo = tr.view_scores(bins, alphas)
            assert np.abs(vj - wj).max() <= tr.JSD_ATOL and np.abs(vo - wo).max() <= 1e-6
            J2, vj2, vo2 = _divergence(ctx, bins, alphas)  # deterministic sums
            assert J2.tobytes() == J.tobytes() and vj2.tobytes() == vj.tobytes() and vo2.tobytes() == vo.tobytes()
    print(f"TERMINATION_JSD_FIGURES all: largest |J - float64| {worst:.3e} bits, bar {tr.JSD_ATOL:.0e}")


# ---- 7. prv_score_views, method 9
N_SCORE = 6


@pytest.fixture(scope="module")
def ensemble(ctx, oracle):
    """five members that differ by seed, their oracle twins, six views, and per stepping rule the reference's sub-sample planes"""
    kw = dict(util.SMALL, density_bias=5.0)
    seeds = [util.SEED_A + 17 * e for e in range(5)]
    fields = []
    for e, seed in enumerate(seeds):
        ctx.synthetic_model(SLOT_MEMBER + e, api.field_desc(**kw), seed)
        fields.append(oracle.OracleField(oracle.desc(**kw), seed=seed))
    w, h = 20, 14
    tms, scale, offset = util.hemisphere_transforms(oracle, util.fibonacci_hemisphere(N_SCORE))
    cs = ctx.cameras_from_matrices(tms, util.FOV_X, w, h, scale, offset)
    ocams = oracle.cameras_from_transforms(tms, util.FOV_X, w, h, scale, offset)
    cache = {}

    def planes(mode):  # [E, n, 3 spp, h, w, K + 1], computed once per rule and shared
        if mode not in cache:
            cache[mode] = np.stack([np.stack([tr.render_variants(oracle.lib(), f, oc, w, h, 16, [f32(0.01)], 64, 3, mode)[0][0] for oc in ocams])
                                    for f in fields])
        return cache[mode]

    yield cs, w, h, planes
    cs.close()
    for f in fields:
        f.close()
    for e in range(5):
        ctx.synthetic_model(SLOT_MEMBER + e, api.field_desc(**util.SMALL), util.SEED_A)


@pytest.mark.parametrize("spp", [1, 3])
@pytest.mark.parametrize("mode", [0, 1], ids=["fixed", "ngp"])
@pytest.mark.parametrize("E", [3, 5])
def test_score_views_method_9_against_the_reference_pipeline(ctx, ensemble, E, mode, spp):
    cs, w, h, planes = ensemble
    opts = api.render_opts(w, h, 64 if mode == 0 else 0, spp, 0.01, step_mode=mode)
    slots = [SLOT_MEMBER + e for e in range(E)]
    rec, st = ctx.score_views(api.L.SCORE_TERMINATION_JSD, slots, cs, None, opts, want_stats=True)
    sub = planes(mode)[:E, :, :spp]  # [E, n, spp, h, w, K + 1]
    px = np.stack([np.stack([tr.mean(sub[e, v]) for v in range(N_SCORE)]) for e in range(E)])  # [E, n, h, w, K + 1]
    want, want_cov = tr.view_scores(np.moveaxis(px[..., :16], -1, 1), px[..., 16])
    diff = np.abs(rec["score"] - want)
    print(f"TERMINATION_SCORE_FIGURES E {E} mode {mode} spp {spp}: scores {rec['score'].tolist()}, reference {want.tolist()}, largest relative difference "
          f"{(diff / want).max():.3e}")
    assert (want > 0).all() and (diff <= util.PIX_RTOL * want).all()
    assert np.abs(rec["coverage"] - want_cov).max() <= util.PIX_RTOL * want_cov.max() and not rec["psnr"].any()
    ids = np.arange(N_SCORE, dtype=np.int32)
    ref_rec = np.zeros(N_SCORE, api.RECORD_DTYPE)
    ref_rec["score"] = want
    gaps = np.diff(np.sort(want))
    assert ctx.rank(rec, ids).tolist() == ctx.rank(ref_rec, ids).tolist(), (
        f"ranking differs; closest reference scores {gaps.min():.3e} apart, largest GPU-reference difference {diff.max():.3e}"
        + (" (closer than twice that: a tie within the bar)" if gaps.min() < 2 * diff.max() else ""))
    assert st.rays == E * N_SCORE * w * h * spp
    # the same members through the two calls the score is made of
    outs = [ctx.render_termination(s, cs, None, opts, api.L.TERMINATION_BINS_DEFAULT, want_stats=False)[:2] for s in slots]
    _, vj, vo = ctx.termination_divergence([o[0] for o in outs], [o[1] for o in outs], want_image=False)
    assert vj.tobytes() == rec["score"].tobytes() and np.array_equal(vo.astype(np.float32), rec["coverage"])
    # one rank without a communicator: the sharded entry point (what the planner calls) is the plain round
    one, sl = np.zeros(N_SCORE, api.RECORD_DTYPE), np.array(slots, np.int32)
    assert ctx.lib.prv_score_views_sharded(ctx.handle, None, api.L.SCORE_TERMINATION_JSD, api._ptr(sl), E, cs.handle, N_SCORE, 1, C.byref(opts),
                                           None, api._ptr(one), None) == 0
    assert one.tobytes() == rec.tobytes()
    sub_rec, _ = ctx.score_views(api.L.SCORE_TERMINATION_JSD, slots, cs, [4, 1], opts)  # a view's score does not depend on its batch
    assert sub_rec["score"].tolist() == [rec["score"][4], rec["score"][1]]


# ---- 7b. two socket ranks on one GPU: the sharded round gives one process's records
ENSEMBLE_KW = dict(util.SMALL, density_bias=5.0)


def _scene_cams(c):
    from nerf_prv_amd import planner

    tms, scale, offset = planner.hemisphere_transforms(util.fibonacci_hemisphere(11), 0.3, 0.1, [1e-10] * 3)
    return c.cameras_from_matrices(tms, util.FOV_X, 40, 24, scale, offset)


def _termination_comm_worker(rank, world, port, outdir):
    """one of two processes on the one GPU: own context, socket transport (tests/test_gpu_comm.py's pattern)"""
    c = api.Context(0)
    comm = api.Comm(c, rank, world, transport="socket", rendezvous=f"127.0.0.1:{port}")
    try:
        for e in range(3):
            c.synthetic_model(e, api.field_desc(**ENSEMBLE_KW), util.SEED_A + 17 * e)
        cs = _scene_cams(c)
        opts = api.render_opts(40, 24, 64, 2, 0.01)
        rec_i, st = comm.score_views(api.L.SCORE_TERMINATION_JSD, [0, 1, 2], cs, len(cs), opts, interleaved=True, want_stats=True)
        rec_b, _ = comm.score_views(api.L.SCORE_TERMINATION_JSD, [0, 1, 2], cs, len(cs), opts, interleaved=False)
        np.savez(os.path.join(outdir, f"rank{rank}.npz"), rec_i=rec_i.view(np.uint8), rec_b=rec_b.view(np.uint8), evaluated=st.samples_evaluated)
        comm.barrier()
    finally:
        comm.close()
        c.close()


def test_two_processes_on_one_gpu_score_termination_jsd(ctx, tmp_path):
    import torch.multiprocessing as mp

    port = free_port()
    mctx = mp.get_context("spawn")
    procs = [mctx.Process(target=_termination_comm_worker, args=(r, 2, port, str(tmp_path))) for r in range(2)]
    for p in procs:
        p.start()
    for p in procs:
        p.join(timeout=300)
        assert p.exitcode == 0
    r0, r1 = (np.load(tmp_path / f"rank{r}.npz") for r in range(2))
    for e in range(3):
        ctx.synthetic_model(SLOT_MEMBER + e, api.field_desc(**ENSEMBLE_KW), util.SEED_A + 17 * e)
    cs = _scene_cams(ctx)
    try:
        want, st = ctx.score_views(api.L.SCORE_TERMINATION_JSD, [SLOT_MEMBER + e for e in range(3)], cs, None, api.render_opts(40, 24, 64, 2, 0.01),
                                   want_stats=True)
        assert (want["score"] > 0).all()
        for r in (r0, r1):
            assert r["rec_i"].tobytes() == want.tobytes() and r["rec_b"].tobytes() == want.tobytes()  # both shard orders, every rank
        assert int(r0["evaluated"]) + int(r1["evaluated"]) == st.samples_evaluated  # the shards evaluate exactly the whole
    finally:
        cs.close()
        for e in range(3):
            ctx.synthetic_model(SLOT_MEMBER + e, api.field_desc(**util.SMALL), util.SEED_A)


# ---- 8. the planner
def test_planner_method_9_trains_five_members_and_picks_the_largest_divergence(ctx, tmp_path):
    """prv_planner, mode 21, method_of_IG 9 on the miniature object of tests/test_gpu_planner.py with deterministic training, three
    rounds: the loop completes, trains five members per iteration, and every decision is the arg-max of the reference score
    recomputed from the members that iteration saved -- tests/termination_ref.py's float64 divergence of the saved members'
    termination planes (the planes themselves are held to the CPU reference by the tests above) -- which the loop's own records
    match within the score's bar, and equal Context.score_views on the saved members byte for byte."""
    exe = os.path.join(ROOT, "nerf_prv_amd", "prv_planner")
    assert os.path.exists(exe), "prv_planner missing: run __graft_entry__.build()"
    pre = tmp_path / "m9"
    pre.mkdir()
    cfg = pre / "cfg.yaml"
    cfg.write_text(YAML.format(pre=pre, vs=os.path.join(GOLD, "hemisphere"), method=9,
                               model_source="train_steps: 40\ntrain_rays: 1024\ntrain_width: 64\ntrain_height: 36\nground_truth_seed: 4242\n"
                                            "train_deterministic: 1\nsave_members: 1\ndump_scores: 1"))
    out = subprocess.run([exe, str(cfg)], input="21\nobjA\n-1\n", text=True, capture_output=True, timeout=300, env=dict(os.environ, PRV_PLANNER_TIMING="1"))
    assert out.returncode == 0, out.stdout + out.stderr
    line = [l for l in out.stdout.splitlines() if l.startswith("chosen_nbvs:")][-1]
    chosen = [int(x) for x in line.split(":")[1].split()]
    assert len(chosen) == 4 and len(set(chosen)) == 4 and chosen[0] == 1
    save = pre / "Compare" / "ShapeNet" / "objA_m9_v1_t0"
    assert (save / "run_time.txt").exists() and (save / "json" / "3.json").exists()
    opts = api.render_opts(80, 45, 64, 2, 0.01, background=(0, 0, 0, 1))
    slots = [SLOT_MEMBER + e for e in range(5)]
    try:
        for it in range(3):
            assert sorted(os.listdir(save / "members" / str(it))) == [f"member_{e}.prvf" for e in range(5)]  # method 3's ensemble
            for e in range(5):
                ctx.load_model_file(slots[e], save / "members" / str(it) / f"member_{e}.prvf")
            cs = ctx.cameras_from_json(save / "render_json" / f"{it}.json")
            candidates = [v for v in range(5) if v not in chosen[: it + 1]]
            assert len(cs) == len(candidates)
            rec, _ = ctx.score_views(api.L.SCORE_TERMINATION_JSD, slots, cs, None, opts)
            records = np.frombuffer((save / "records" / f"{it}.bin").read_bytes(), api.RECORD_DTYPE)
            assert records.tobytes() == rec.tobytes()  # the loop scored these members, with these options
            dumped = np.frombuffer((save / "scores" / f"{it}.bin").read_bytes(), np.float64)
            assert dumped.tobytes() == rec["score"].tobytes()
            planes = [ctx.render_termination(s, cs, None, opts, api.L.TERMINATION_BINS_DEFAULT, want_stats=False)[:2] for s in slots]
            want, _ = tr.view_scores(np.stack([b.cpu().numpy() for b, _ in planes]), np.stack([a.cpu().numpy() for _, a in planes]))
            diff = np.abs(rec["score"] - want)
            print(f"TERMINATION_PLANNER_FIGURES iteration {it}: scores {rec['score'].tolist()}, reference {want.tolist()}")
            assert (want > 0).all() and (diff <= util.PIX_RTOL * want).all()
            gaps = np.diff(np.sort(want)) if len(want) > 1 else np.array([np.inf])
            assert chosen[it + 1] == candidates[int(np.argmax(want))] == ctx.argmax(rec, np.array(candidates, np.int32)), (
                f"closest reference scores {gaps.min():.3e} apart, largest GPU-reference difference {diff.max():.3e}")
            cs.close()
    finally:
        for s in slots:
            ctx.synthetic_model(s, api.field_desc(**util.SMALL), util.SEED_A)


def test_termination_misuse(ctx, oracle):
    w, h = 16, 12
    ctx.synthetic_model(SLOT_SMALL, api.field_desc(**util.SMALL), util.SEED_A)
    tms, scale, offset = util.hemisphere_transforms(oracle, util.fibonacci_hemisphere(3))
    cs = ctx.cameras_from_matrices(tms, util.FOV_X, w, h, scale, offset)
    opts = api.render_opts(w, h, 32, 1, 0.01)
    try:
        for K in (0, 2, 3, 12, 128, -16):
            with pytest.raises(api.PrvError) as e:
                ctx.render_termination(SLOT_SMALL, cs, None, opts, K)
            assert e.value.code == api.L.PRV_E_INVALID and "n_bins" in str(e.value)
        bins = ctx.torch.zeros((16, 3, h, w), dtype=ctx.torch.float32, device=ctx.device)
        alpha = ctx.torch.zeros((3, h, w), dtype=ctx.torch.float32, device=ctx.device)
        host = np.zeros((16, 3, h, w), np.float32)
        for b, a, text in ((None, alpha, "required"), (host, alpha, "device pointer"), (bins, host[0], "device pointer")):
            rc = ctx.lib.prv_render_termination(ctx.handle, SLOT_SMALL, cs.handle, None, 3, C.byref(opts), 16, api._ptr(b), api._ptr(a), None)
            assert rc == api.L.PRV_E_INVALID and text in ctx.lib.prv_last_error(ctx.handle).decode(), text
        # the reduce: member counts, bins, NULL and host planes
        arr = lambda xs: (C.c_void_p * len(xs))(*[x if isinstance(x, int) or x is None else x.data_ptr() for x in xs])
        vj = np.zeros(3)
        for n_models, K, bs, as_, text in ((1, 16, [bins], [alpha], "models"), (9, 16, [bins] * 9, [alpha] * 9, "models"),
                                           (2, 12, [bins] * 2, [alpha] * 2, "n_bins"), (2, 16, [bins, None], [alpha] * 2, "required"),
                                           (2, 16, [bins] * 2, [alpha, host.ctypes.data], "device pointer")):
            rc = ctx.lib.prv_termination_divergence(ctx.handle, arr(bs), arr(as_), n_models, 3, w, h, K, None, api._ptr(vj), None)
            assert rc == api.L.PRV_E_INVALID and text in ctx.lib.prv_last_error(ctx.handle).decode(), text
        # the score: one model, nine models, reference images
        gt = ctx.torch.zeros((3, h, w, 4), dtype=ctx.torch.float32, device=ctx.device)
        for slots, g in (([SLOT_SMALL], None), ([SLOT_SMALL] * 9, None), ([SLOT_SMALL] * 2, gt)):
            with pytest.raises(api.PrvError) as e:
                ctx.score_views(api.L.SCORE_TERMINATION_JSD, slots, cs, None, opts, gt=g)
            assert e.value.code == api.L.PRV_E_INVALID and "method 9" in str(e.value)
        rec, _ = ctx.score_views(api.L.SCORE_TERMINATION_JSD, [SLOT_SMALL] * 2, cs, None, opts)  # usable afterwards; identical members: exactly 0
        assert not rec["score"].any() and (rec["coverage"] > 0).any()
    finally:
        cs.close()
