"""The ray queue between the march kernels and render_queue64_body, attacked on purpose: the populations of tests/queue_cases.py
(tests/test_queue_cases_host.py asserts, without a GPU, which queue path each one forces) through the colour render, the plane
modes, every placement switch and the multi-member march.

  octant_high / octant_low   the octant's region overflows: waves move on, one reservation per sub-region straddles its end (the
                             drain renders min(count, seg_cap) - cut records), octant 7 wraps to region 0, idle XCDs walk on
  one_subregion              every live block appends to ONE counter, which overflows on its own
  counts0 .. counts65        batches of exactly 0, 1, 63, 64, 65 live rays
  skew                       one wave holds one-sample rays and 800-step rays: refill, tail merge and the pool around stragglers
  gaps                       whole empty extension chunks between two occupied stretches (next_chunk; take_ray into a later chunk
                             when relocation is on)
  opaque                     every ray ends at its first sample: a refill every round

Bars: none of its own.  Colour against the oracle with util.assert_pixels_close (min_T = 1e-4); the march count exact; the
evaluated count under tests/test_gpu_ngp_step.py's bar; the planes under entropy_ref's rule (every pixel within 1e-3 -- util's
floor, entropy_ref's for H -- of the reference at one of util.termination_variants); everything else is np.array_equal."""
import numpy as np
import pytest

from nerf_prv_amd import api
from tests import entropy_ref, instances, march_ref, queue_cases as qc, termination_ref, util
from tests.test_gpu_instances import environment

pytestmark = pytest.mark.gpu

SLOT = 62  # slots of this file: 62..63
SHAPES = {"F4_0": instances.MATRIX["F4_0"], "F4_5": instances.MATRIX["F4_5"]}  # util.SMALL (generic <4,0>) and the fast <4,5>
SWITCHES = [{"PRV_SPATIAL_REGIONS": "0"},  # block id % regions: never overflows -- the control
            {"PRV_QUEUE_SEGMENTS": "1"}, {"PRV_MERGE_MAX": "0"}, {"PRV_MERGE_MAX": "31", "PRV_POOL": "1"}, {"PRV_BLOCKS_PER_CU": "1"}]
RUNS = qc.runs()
_run_id = lambda r: f"{r[0]}-{'ngp' if r[1] else 'S128'}"
_env_id = lambda e: ",".join(f"{k}={v}" for k, v in e.items())
f32 = np.float32


def _S(mode):
    return qc.S_FIXED if mode == qc.FIXED else 0


def _load(c, oracle, slot, case, shape):
    f = case.load(c, oracle, slot, SHAPES[shape].kw)
    instances.assert_layout(c.model_layout(slot), SHAPES[shape])
    return f


def _render(c, oracle, slot, name, mode, shape):
    """-> (images [views, h, w, 4], samples_live, samples_evaluated) of the case in context c"""
    case = qc.get(name)
    _load(c, oracle, slot, case, shape).close()
    cs = case.cams(c)
    img, st = c.render(slot, cs, None, case.opts(mode))
    cs.close()
    assert st.rays == case.n_views * case.w * case.h * case.spp
    return img.cpu().numpy(), int(st.samples_live), int(st.samples_evaluated)


_default = {}


def _default_render(ctx, oracle, name, mode, shape):
    """the default context's render of a run, once per module"""
    key = (name, mode, shape)
    if key not in _default:
        _default[key] = _render(ctx, oracle, SLOT, name, mode, shape)
    return _default[key]


# ---- 1. against the oracle
@pytest.mark.parametrize("shape", list(SHAPES))
@pytest.mark.parametrize("run", RUNS, ids=_run_id)
def test_colour_and_counts_against_the_oracle(ctx, oracle, run, shape):
    name, mode = run
    case = qc.get(name)
    img, live, n_eval = _default_render(ctx, oracle, name, mode, shape)
    f = case.oracle_field(oracle, SHAPES[shape].kw)
    want_live = want_eval = 0
    for v, oc in enumerate(case.ocams(oracle)):
        want, ne = f.render(oc, case.w, case.h, _S(mode), case.spp, case.min_T, threads=16, step_mode=mode)
        want_eval += ne
        want_live += f.march_count(oc, case.w, case.h, _S(mode), case.spp, step_mode=mode)
        util.assert_pixels_close(img[v], want)
    f.close()
    print(f"QUEUE_GPU {name} {shape} mode {mode}: live {live} (oracle {want_live}), evaluated {n_eval} (oracle {want_eval})")
    assert live == want_live  # every step's occupancy decision of every record, exactly
    assert abs(n_eval - want_eval) <= max(4, want_eval // 20000)  # tests/test_gpu_ngp_step.py's bar
    if case.regime in (qc.TRANSPARENT, qc.OPAQUE):
        assert n_eval == want_eval  # no ray near the threshold: all of its samples, or exactly one


# ---- 2. the plane modes against folds over tests/march_ref.py's samples
def _pixels(p, v, per_view):
    """a few pixels of view v: live ones evenly spread over the view (the rays with the fewest and the most live samples among
    them), and two dead ones"""
    live = p.live[:, v].any(axis=0)
    ys, xs = np.nonzero(live)
    pick = set()
    if len(ys):
        idx = np.unique(np.linspace(0, len(ys) - 1, per_view).astype(int))
        pick |= {(int(ys[i]), int(xs[i])) for i in idx}
        cnt = np.where(live, p.count[:, v].sum(axis=0), -1)
        pick.add(tuple(int(a) for a in np.unravel_index(np.argmax(cnt), cnt.shape)))
        pick.add(tuple(int(a) for a in np.unravel_index(np.argmin(np.where(live, cnt, 1 << 30)), cnt.shape)))
    dy, dx = np.nonzero(~live)
    pick |= {(int(dy[i]), int(dx[i])) for i in (0, len(dy) // 2) if len(dy)}
    return sorted(pick)


def _plane_reference(oracle, f, case, ocam, mode, pixels, K):
    """-> [3 variants, len(pixels), K + 3] float32: the K termination bins, alpha, H, z of every chosen pixel (sub-samples averaged)
    at the thresholds of util.termination_variants(min_T); one march per ray serves the three planes and the histogram"""
    mts = [f32(t) for t in util.termination_variants(case.min_T)]
    sub = np.zeros((len(mts), case.spp, len(pixels), K + 3), np.float32)
    where = {px: i for i, px in enumerate(pixels)}
    nmax = termination_ref.n_max(mode, qc.S_FIXED)
    for k, y, x, o, d in march_ref.rays(oracle.lib(), ocam, case.w, case.h, case.spp, pixels=pixels):
        steps, ts, alphas, _, _ = march_ref.ray_samples(oracle.lib(), f, o, d, mode, qc.S_FIXED, min(mts))
        cos = march_ref.forward_cos(ocam, d)
        for j, mt in enumerate(mts):
            bins = termination_ref.histogram(steps, alphas, K, nmax, mt)[0] if K else ()
            n_used, Tc = 0, f32(1)
            for a in alphas:  # the samples this threshold composites
                n_used += 1
                Tc = f32(Tc * (f32(1) - a))
                if Tc < mt:
                    break
            (D,), T = march_ref.composite(alphas[:n_used], [(t,) for t in ts[:n_used]], 1)
            H = entropy_ref.entropy_of_alphas(alphas, mt)[0] if alphas else f32(0)
            sub[j, k, where[(y, x)]] = (*bins, f32(1) - T if alphas else f32(0), H, f32(D * cos))
    return np.stack([march_ref.mean(s) for s in sub])


def _assert_planes(got, wants, K, tag):
    """entropy_ref.assert_close_any's rule over (bins, alpha, z | H): every pixel, all of its values together, within the bar of one variant"""
    errs = []
    for w in wants:
        e = util.pixel_rel_err(np.delete(got, K + 1, axis=-1), np.delete(w, K + 1, axis=-1)).max(axis=-1)
        errs.append(np.maximum(e, entropy_ref.rel_err(got[..., K + 1], w[..., K + 1])))
    best = np.min(errs, axis=0)
    print(f"QUEUE_GPU planes {tag}: {best.size} pixels, largest relative error {best.max():.3e}")
    assert best.max() <= util.PIX_RTOL, (tag, int(np.argmax(best)), got[np.argmax(best)], wants[0][np.argmax(best)])


TERMINATION_CASES = ("octant_high", "gaps", "skew")


@pytest.mark.parametrize("shape", list(SHAPES))
@pytest.mark.parametrize("run", [r for r in RUNS if not r[0].startswith("counts")], ids=_run_id)
def test_plane_modes_against_the_march_reference(ctx, oracle, run, shape):
    """prv_render_footprint (entropy + opacity + depth in one launch) on every case, prv_render_termination at K = 4 on three"""
    name, mode = run
    case = qc.get(name)
    p = qc.population(oracle, case, mode)
    f = _load(ctx, oracle, SLOT, case, shape)
    cs = case.cams(ctx)
    opts = case.opts(mode)
    ent, alpha, depth, st = ctx.render_footprint(SLOT, cs, None, opts)
    ent, alpha, depth = (t.cpu().numpy() for t in (ent, alpha, depth))
    K = 4 if name in TERMINATION_CASES else 0
    if K:
        bins, alpha_t, st_t = ctx.render_termination(SLOT, cs, None, opts, K)
        bins = bins.cpu().numpy()
        assert np.array_equal(alpha_t.cpu().numpy().view(np.uint32), alpha.view(np.uint32))
        assert (st_t.samples_live, st_t.samples_evaluated) == (st.samples_live, st.samples_evaluated)
    cs.close()
    _, live, n_eval = _default_render(ctx, oracle, name, mode, shape)
    assert int(st.samples_live) == live and abs(int(st.samples_evaluated) - n_eval) <= max(4, n_eval // 20000)
    views = sorted({0, case.n_views // 2, case.n_views - 1})  # (a Python march per ray: three views, a few pixels each)
    per_view = max(2, 8 // case.spp) if case.n_views <= 3 else 2
    ocams = case.ocams(oracle)
    for v in views:
        oc = ocams[v]
        pixels = _pixels(p, v, per_view)
        ys, xs = np.array(pixels).T
        wants = _plane_reference(oracle, f, case, oc, mode, pixels, K)
        got = np.stack([bins[k, v, ys, xs] for k in range(K)] + [alpha[v, ys, xs], ent[v, ys, xs], depth[v, ys, xs]], axis=-1)
        _assert_planes(got, wants, K, f"{name}/{shape}/mode{mode}/view{v}")
        dead = ~p.live[:, v].any(axis=0)
        assert not alpha[v][dead].any() and not ent[v][dead].any() and not depth[v][dead].any()  # dead rays: exactly 0
        assert not K or not bins[:, v][:, dead].any()
    f.close()


# ---- 3. byte identity across placement
@pytest.fixture(scope="module", params=SWITCHES, ids=_env_id)
def switched(request):
    """one context per switch for the whole module (the switches are read when a context is created)"""
    with environment(request.param):
        c = api.Context(0)
    yield c
    c.close()


@pytest.mark.parametrize("run", RUNS, ids=_run_id)
def test_placement_switches_change_no_byte(ctx, oracle, switched, run):
    """where a record lies in the queue, which region overflowed into which, who drains it and whether a ray moves between slots
    changes neither a bit of the image nor a count"""
    name, mode = run
    for shape in SHAPES:
        img, live, n_eval = _default_render(ctx, oracle, name, mode, shape)
        img2, live2, n_eval2 = _render(switched, oracle, 0, name, mode, shape)
        assert live2 == live and n_eval2 == n_eval, (shape, live, live2, n_eval, n_eval2)
        assert np.array_equal(img2.view(np.uint32), img.view(np.uint32)), shape


@pytest.mark.parametrize("run", [r for r in RUNS if r[0] in ("skew", "gaps")], ids=_run_id)
def test_footprint_planes_do_not_depend_on_placement(ctx, oracle, switched, run):
    """the footprint mode's five moved words {record, next sample, T, H, D} through tail merge and pool (PRV_MERGE_MAX=31 PRV_POOL=1,
    and every other switch): the stragglers of `skew`, and `gaps`' rays taken over in a later chunk, leave the three planes and
    the counts what the default placement gives, bit for bit"""
    name, mode = run
    case = qc.get(name)
    for shape in SHAPES:
        outs = []
        for c, slot in ((ctx, SLOT), (switched, 0)):
            _load(c, oracle, slot, case, shape).close()
            cs = case.cams(c)
            ent, alpha, depth, st = c.render_footprint(slot, cs, None, case.opts(mode))
            cs.close()
            outs.append(([t.cpu().numpy() for t in (ent, alpha, depth)], (int(st.samples_live), int(st.samples_evaluated))))
        (want, n_want), (got, n_got) = outs
        assert n_got == n_want, (shape, n_want, n_got)
        for plane, g, w in zip(("entropy", "alpha", "depth"), got, want):
            assert np.array_equal(g.view(np.uint32), w.view(np.uint32)), (shape, plane)
        assert (want[1] > 0).any() and (want[2] > 0).any()


# ---- 4. counts
@pytest.mark.parametrize("shape", list(SHAPES))
@pytest.mark.parametrize("mode", [qc.FIXED, qc.NGP], ids=["S128", "ngp"])
@pytest.mark.parametrize("n", qc.COUNTS)
def test_counts_render_exactly_their_live_pixels(ctx, oracle, n, mode, shape):
    name = f"counts{n}"
    case = qc.get(name)
    p = qc.population(oracle, case, mode)
    assert p.n_rays == n
    img, live, n_eval = _default_render(ctx, oracle, name, mode, shape)
    assert np.array_equal(img[0, ..., 3] > 0, p.live[0, 0]) and int((img[0, ..., 3] > 0).sum()) == n
    assert not img[0][~p.live[0, 0]].any()  # every other pixel: exactly zero, all four channels
    assert live == sum(p.n_live_samples) and (n_eval > 0) == (n > 0)
    if n == 0:
        assert live == 0 and n_eval == 0 and not img.any()
        bg = (0.25, 0.5, 0.75, 1.0)
        _load(ctx, oracle, SLOT, case, shape).close()  # (the cached render above may be an earlier test's: the slot has moved on)
        cs = case.cams(ctx)
        u8, st = ctx.render_rgba8(SLOT, cs, None, case.opts(mode, background=bg))
        cs.close()
        assert np.array_equal(u8.cpu().numpy(), oracle.quantize_rgba8(np.zeros((1, case.h, case.w, 4), np.float32), bg))  # the background everywhere
        assert int(st.samples_live) == 0 and int(st.samples_evaluated) == 0


# ---- 5. the multi-member march
def _member_grids(case, E):
    """member 0 takes the case's grid; the others an all-occupied, an empty and a slab grid and the case's grid mirrored"""
    R = qc.R
    return [case.occ, np.ones((R, R, R), bool), np.zeros((R, R, R), bool), qc.slab_grid(), case.occ[::-1, ::-1, ::-1].copy()][:E]


@pytest.mark.parametrize("E,method", [(2, 2), (5, 3)])
@pytest.mark.parametrize("name", ["octant_high", "one_subregion", "gaps"])
def test_multi_member_march_fills_unevenly_full_regions_like_one_march_per_member(oracle, name, E, method):
    """march_multi_kernel reserves for the E members in one wave instruction, lane e on member e's counter: the members' regions
    are unevenly full (one overflows its octant's region, one is empty, one fills every region).  As
    test_one_march_launch_for_the_ensemble_gives_every_member_its_own_result: the same records, march count and evaluated count
    as one march launch per member"""
    case = qc.get(name)
    kw = case.kw(util.SMALL)
    got = {}
    for multi in ("0", "1"):
        with environment({"PRV_MARCH_MULTI": multi}):
            c = api.Context(0)
        try:
            for e, grid in enumerate(_member_grids(case, E)):
                f = oracle.OracleField(oracle.desc(**kw), seed=4242 + e)
                t, m, _ = f.params()
                f.close()
                words = np.frombuffer(np.packbits(grid.reshape(-1).astype(np.uint8), bitorder="little").tobytes(), np.uint32).copy()
                c.load_model(e, api.field_desc(**kw), t, m, words)
            cs = case.cams(c)
            opts = api.engine_render_opts(case.w, case.h, 0, case.spp, 0.01, background=(0, 0, 0, 1))
            rec, st = c.score_views(method, list(range(E)), cs, None, opts, want_stats=True)
            got[multi] = (rec.tobytes(), int(st.samples_live), int(st.samples_evaluated), rec)
            cs.close()
        finally:
            c.close()
    assert got["0"][1] == got["1"][1] > 0
    assert got["0"][2] == got["1"][2] > 0
    assert got["0"][0] == got["1"][0]
    assert np.all(np.isfinite(got["1"][3]["score"]))
