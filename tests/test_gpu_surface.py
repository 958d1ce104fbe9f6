"""The surface locator on the GPU: prv_render_surface (render_planes_kernel in kRenderSurface mode) against the CPU reference
of tests/surface_ref.py on every compiled field instance, its independence of where a ray is composited, the fast instances
against the generic one, prv_select_views_surface as the surface render followed by the rounds, misuse, and the planner with
select_locator: surface.

Against the reference: entropy, alpha and the statistics are prv_render_entropy's, byte for byte.  Where the reference's three
threshold variants agree (tests/test_surface_host.py caps where they do not), hit and z are the reference's bit for bit.  For
z the bar could have been 2 ulp -- t is bit-identical between kernel and reference and the product is one multiply, so only the
cosine's square root and division can differ -- but on the MI355X z is bit-equal in all 42 comparisons of the matrix (the
`SURFACE_FIGURES` lines of pytest -s: "z within 0 ulp" throughout), so equality is what is asserted.  Elsewhere
lo <= got <= hi, and at 1 spp got is one of the three variants' values."""
import numpy as np
import pytest

from nerf_prv_amd import api, planner
from tests import instances, select_ref, surface_ref, util
from tests.surface_ref import FH, FW
from tests.test_gpu_instances import environment, load
from tests.test_gpu_select import STAT_KEYS, _plan, _u32

pytestmark = pytest.mark.gpu

SLOT, SLOT_TWIN, SLOT_SMALL = 24, 25, 26  # slots of this file: 24..27
f32 = np.float32
Z_ULPS = 0  # z against the reference where the variants agree: bit-equal on the MI355X in every case of this file (see the docstring)


def _ulps(a, b):
    """distance in float32 steps between same-signed finite values"""
    return np.abs(np.asarray(a, np.float32).view(np.int32).astype(np.int64) - np.asarray(b, np.float32).view(np.int32).astype(np.int64))


def _surface(c, slot, cs, opts, level=0.5, ids=None):
    ent, alpha, depth, hit, st = c.render_surface(slot, cs, ids, opts, level)
    return [t.cpu().numpy() for t in (ent, alpha, depth, hit)], st


# ---- (a) against the reference, on every compiled instance
@pytest.fixture(scope="module", params=surface_ref.cases(), ids=[f"{n}-{'ngp' if m else 'fixed'}-L{l}" for n, m, l, _ in surface_ref.cases()])
def case(request, ctx, oracle):
    name, mode, level, min_T = request.param
    m = load(ctx, oracle, SLOT, name, surface_ref.case_entry(name, mode))
    tms, scale, offset = surface_ref.case_transforms(oracle)
    cs = ctx.cameras_from_matrices(tms, util.FOV_X, FW, FH, scale, offset)
    ocams = oracle.cameras_from_transforms(tms, util.FOV_X, FW, FH, scale, offset)
    want = surface_ref.case_bounds(oracle, m.f, ocams, mode, level, min_T)  # once, for both spp
    yield m, cs, mode, level, min_T, want
    cs.close()
    m.f.close()
    ctx.synthetic_model(SLOT, api.field_desc(**util.SMALL), util.SEED_A)


@pytest.mark.parametrize("spp", surface_ref.SPP, ids=["spp1", "spp3"])
def test_surface_against_the_reference(ctx, case, spp):
    m, cs, mode, level, min_T, want = case
    instances.assert_layout(ctx.model_layout(SLOT), m.entry)
    opts = api.render_opts(FW, FH, surface_ref.S_FIXED if mode == 0 else 0, spp, min_T, step_mode=mode)
    (ent, alpha, z, hit), st = _surface(ctx, SLOT, cs, opts, level)
    ent0, alpha0, st0 = ctx.render_entropy(SLOT, cs, None, opts)
    assert np.array_equal(ent.view(np.uint32), _u32(ent0)) and np.array_equal(alpha.view(np.uint32), _u32(alpha0))
    for k in STAT_KEYS:
        assert getattr(st, k) == getattr(st0, k), k
    n_exact = n_loose = worst = 0
    for v, b in enumerate(want[spp]):
        exact = ~b.loose
        assert np.array_equal(hit[v][exact].view(np.uint32), b.hit_lo[exact].view(np.uint32))
        ulps = _ulps(z[v][exact], b.z_lo[exact])
        worst = max(worst, int(ulps.max()))
        assert ulps.max() <= Z_ULPS, f"view {v}: z is {ulps.max()} ulp from the reference"
        loose = b.loose
        assert ((b.z_lo[loose] <= z[v][loose]) & (z[v][loose] <= b.z_hi[loose])).all()
        assert ((b.hit_lo[loose] <= hit[v][loose]) & (hit[v][loose] <= b.hit_hi[loose])).all()
        if spp == 1:  # the ray crossed where one of the variants crosses
            one_of = _ulps(z[v][None].repeat(3, 0), b.z_var).min(axis=0) <= Z_ULPS
            assert one_of.all() and (hit[v][None] == b.hit_var).any(axis=0).all()
        dead = alpha[v] == 0
        assert dead.any() and not ent[v][dead].any() and not z[v][dead].any() and not hit[v][dead].any()  # exactly 0 in all four
        n_exact += int((exact & b.hit_pixels).sum())
        n_loose += int((loose & b.hit_pixels).sum())
    print(f"SURFACE_FIGURES {m.name}/{mode}/L{level}/spp{spp}: {n_exact} hit pixels exact (z within {worst} ulp), {n_loose} between the variants")
    assert n_exact > 50 and (hit > 0).any() and (z > 0).any()


# ---- (b) placement changes nothing
@pytest.mark.parametrize("mode", [0, 1], ids=["fixed", "ngp"])
def test_surface_batches_and_relocation_change_no_byte(oracle, monkeypatch, mode):
    """One batch against several (a 1 MiB queue budget, as tests/test_gpu_select.py's footprint test shrinks it), with the tail
    merge and the pool on and off: which lane composites a ray, and in which launch, changes no byte of any plane."""
    opts = api.render_opts(FW, FH, 96 if mode == 0 else 0, 3, 1e-4, step_mode=mode)
    tms, scale, offset = util.hemisphere_transforms(oracle, util.fibonacci_hemisphere(6))

    def surface():
        c = api.Context(0)
        try:
            c.synthetic_model(0, api.field_desc(**util.SMALL), util.SEED_A)
            cs = c.cameras_from_matrices(tms[[0, 2, 5]], util.FOV_X, FW, FH, scale, offset)
            planes, st = _surface(c, 0, cs, opts)
            cs.close()
            return [p.tobytes() for p in planes], [getattr(st, k) for k in STAT_KEYS], planes
        finally:
            c.close()

    for k in ("PRV_QUEUE_MB", "PRV_MERGE_MAX", "PRV_POOL"):
        monkeypatch.delenv(k, raising=False)
    base, stats, planes = surface()
    assert all((planes[2][v] > 0).any() and (planes[3][v] > 0).any() for v in range(3))
    for env in ({"PRV_QUEUE_MB": "1"}, {"PRV_MERGE_MAX": "31", "PRV_POOL": "1"}, {"PRV_MERGE_MAX": "0", "PRV_POOL": "0"},
                {"PRV_QUEUE_MB": "1", "PRV_MERGE_MAX": "31", "PRV_POOL": "1"}):
        with environment(env):
            other, stats1, _ = surface()
        for name, a, b in zip(("entropy", "alpha", "depth", "hit"), base, other):
            assert a == b, (name, env)
        assert stats1[:2] == stats[:2] and stats1[3] == stats[3], env


# ---- (c) a fast instance and the generic one: identical bytes
@pytest.mark.parametrize("name", ["F4_5", "F2_10"])
def test_fast_equals_generic_surface(ctx, oracle, name):
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
                outs.append(_surface(c, slot, cs, api.render_opts(w, h, 96 if mode == 0 else 0, 1, 1e-4, step_mode=mode)))
                cs.close()
            (a, st_a), (b, st_b) = outs
            for p, q in zip(a, b):
                assert np.array_equal(p.view(np.uint32), q.view(np.uint32))
            assert int(st_a.samples_evaluated) == int(st_b.samples_evaluated) > 0 and (a[3] > 0).any()
    finally:
        other.close()
        ctx.synthetic_model(SLOT_TWIN, api.field_desc(**util.SMALL), util.SEED_A)


# ---- (d) select_views(locator="surface"): the surface render, then the rounds
@pytest.mark.parametrize("S,spp,mode", [(64, 1, 0), (0, 2, 1)], ids=["S64", "ngp_spp2"])
def test_select_views_surface_is_the_surface_render_then_the_rounds(ctx, S, spp, mode):
    w, h, n, k = 40, 30, 7, 3
    ctx.synthetic_model(SLOT_SMALL, api.field_desc(**util.SMALL), util.SEED_A)
    tms, scale, offset = planner.hemisphere_transforms(planner.hemisphere_generate(64), 0.3, 0.1, [1e-10] * 3)
    cs = ctx.cameras_from_matrices(tms[np.arange(n) * 9 + 2], util.FOV_X, w, h, scale, offset)
    opts = api.render_opts(w, h, S, spp, 0.01, step_mode=mode)
    so = api.select_opts(k=k)
    chosen, gains, st = ctx.select_views(SLOT_SMALL, cs, None, opts, so, want_stats=True, locator="surface", level=0.5)
    ent, alpha, depth, hit, st0 = ctx.render_surface(SLOT_SMALL, cs, None, opts, 0.5)
    chosen2, gains2, vox, q = ctx.select_from_images(cs, None, ent, hit, depth, so, want_words=True)
    assert chosen.tolist() == chosen2.tolist() and gains.tolist() == gains2.tolist()
    for key in STAT_KEYS:
        assert getattr(st, key) == getattr(st0, key), key
    ent, depth, hit = (t.cpu().numpy() for t in (ent, depth, hit))
    words = [select_ref.footprint(ctx, cs, v, w, h, ent[v], hit[v], depth[v], so.grid_res, so.alpha_min) for v in range(n)]
    want_vox, want_q = np.stack([x[0] for x in words]), np.stack([x[1] for x in words])
    assert np.array_equal(_u32(vox), want_vox) and np.array_equal(_u32(q), want_q)
    assert (want_vox != select_ref.UNLOCATED).sum() > 100 and (want_q > 0).any()
    want_chosen, want_gains = select_ref.greedy(want_vox, want_q, k, so.grid_res)
    print(f"SURFACE_SELECT_FIGURES {S}/{spp}/{mode}: chosen {chosen.tolist()} gains {gains.tolist()} located {(want_vox != select_ref.UNLOCATED).sum()}")
    assert chosen.tolist() == want_chosen and [int(g) for g in gains] == want_gains and len(set(chosen.tolist())) == k
    with pytest.raises(ValueError):
        ctx.select_views(SLOT_SMALL, cs, None, opts, so, locator="nonsense")
    cs.close()


# ---- (e) misuse
def test_surface_misuse(ctx, oracle):
    w, h = 16, 12
    ctx.synthetic_model(SLOT_SMALL, api.field_desc(**util.SMALL), util.SEED_A)
    tms, scale, offset = util.hemisphere_transforms(oracle, util.fibonacci_hemisphere(3))
    cs = ctx.cameras_from_matrices(tms, util.FOV_X, w, h, scale, offset)
    opts = api.render_opts(w, h, 32, 1, 0.01)
    so = api.select_opts(k=2)
    for level, text in ((0.0, "level"), (1.0, "level"), (float("nan"), "level"), (0.995, "min_transmittance")):
        with pytest.raises(api.PrvError) as e:
            ctx.render_surface(SLOT_SMALL, cs, None, opts, level)
        assert e.value.code == api.L.PRV_E_INVALID and text in str(e.value)
        with pytest.raises(api.PrvError) as e:
            ctx.select_views(SLOT_SMALL, cs, None, opts, so, locator="surface", level=level)
        assert e.value.code == api.L.PRV_E_INVALID and text in str(e.value)
    import ctypes as C

    dev = [ctx.torch.zeros((3, h, w), dtype=ctx.torch.float32, device=ctx.device) for _ in range(4)]
    host = np.zeros((3, h, w), np.float32)
    for i in range(4):
        for bad, text in ((None, "required"), (host, "device pointer")):
            ptrs = [api._ptr(bad) if j == i else api._ptr(dev[j]) for j in range(4)]
            rc = ctx.lib.prv_render_surface(ctx.handle, SLOT_SMALL, cs.handle, None, 3, C.byref(opts), 0.5, *ptrs, None)
            assert rc == api.L.PRV_E_INVALID and text in ctx.lib.prv_last_error(ctx.handle).decode(), (i, text)
    (ent, alpha, z, hit), _ = _surface(ctx, SLOT_SMALL, cs, opts)  # usable afterwards
    assert (hit > 0).any()
    cs.close()


# ---- (f) what the feature is for: a ray that meets two separated semi-opaque shells
def test_surface_sits_on_a_shell_where_the_expected_depth_falls_between_them(ctx, oracle):
    """util.SMALL's synthetic field at density bias 2.5, its occupancy replaced by two slabs of cells across z (load path), seen
    from straight above.  The oracle alone names the rays that leave the first shell with 0.2 < w1 < 0.5 of their opacity spent
    and reach the level in the second shell under every threshold variant.  On those pixels the surface depth / hit is within
    one step dt of a sample the reference marks as the crossing one, and the footprint render's z / alpha -- the default
    locator's point -- lies strictly between the shells, where there is nothing."""
    w, h, S, min_T = surface_ref.SHELL_W, surface_ref.SHELL_H, surface_ref.SHELL_S, 1e-4
    kw = dict(util.SMALL, density_bias=2.5)
    params = surface_ref.two_shell_params(oracle, kw, util.SEED_A)
    f = oracle.OracleField(oracle.desc(**kw), params=params)
    ctx.load_model(SLOT_SMALL, api.field_desc(**kw), *params)
    tms, scale, offset = util.hemisphere_transforms(oracle, util.fibonacci_hemisphere(6))
    ocam = oracle.cameras_from_transforms(tms[:1], util.FOV_X, w, h, scale, offset)[0]
    assert np.frombuffer(ocam.c2w, np.float32)[10] < -0.99  # the view from straight above: its axis goes through both slabs
    T_cross = [f32(v) for v in util.termination_variants(f32(1) - f32(0.5))]
    ref = surface_ref.shell_rays(oracle.lib(), f, ocam, w, h, S, min_T, T_cross)
    f.close()
    sel = (ref["t_gap1"] > 0) & (ref["w1"] > 0.2) & (ref["w1"] < 0.5) & (ref["t_cross"] >= ref["t_gap1"][None]).all(axis=0)
    print(f"SURFACE_SHELLS: {int(sel.sum())} rays with 0.2 < w1 < 0.5 that cross in the second shell, of {int((ref['t_gap1'] > 0).sum())} through both")
    assert sel.sum() >= 50  # (113 on the oracle)
    cs = ctx.cameras_from_matrices(tms[:1], util.FOV_X, w, h, scale, offset)
    opts = api.render_opts(w, h, S, 1, min_T)
    (_, _, z, hit), _ = _surface(ctx, SLOT_SMALL, cs, opts, 0.5)
    _, alpha_f, z_f, _ = ctx.render_footprint(SLOT_SMALL, cs, None, opts)
    cs.close()
    ctx.synthetic_model(SLOT_SMALL, api.field_desc(**util.SMALL), util.SEED_A)
    alpha_f, z_f = alpha_f.cpu().numpy()[0], z_f.cpu().numpy()[0]
    assert (hit[0][sel] == 1).all()
    cos, dt = ref["cos"][sel].astype(np.float64), ref["dt"][sel].astype(np.float64)
    t_surface = z[0][sel].astype(np.float64) / hit[0][sel] / cos
    t_expected = z_f[sel].astype(np.float64) / alpha_f[sel] / cos
    off = np.abs(t_surface[None] - ref["t_cross"][:, sel].astype(np.float64)).min(axis=0)
    print(f"SURFACE_SHELLS: surface depth off its crossing sample by at most {off.max():.3e} (dt {dt.mean():.3e}); expected depth "
          f"{(t_expected - ref['t_gap0'][sel]).min():.3e} behind the first shell, {(ref['t_gap1'][sel] - t_expected).min():.3e} before the second")
    assert (off <= dt).all()
    assert (t_surface >= ref["t_gap1"][sel] - dt).all()  # ... which lies in the second shell
    assert ((t_expected > ref["t_gap0"][sel]) & (t_expected < ref["t_gap1"][sel])).all()  # strictly between the shells


# ---- the matrix's own density under the engine's rule (the cases above are denser: tests/surface_ref.py DENSITY_BIAS)
def test_surface_at_the_matrix_density_under_the_engine_rule(ctx, oracle):
    """F4_5 as tests/instances.py has it (bias 3), one view, 1 spp.  About half the hit pixels lie between the variants here and
    are held to lo <= got <= hi and to being one variant's value; the rest are held to the reference itself, as in (a)."""
    m = load(ctx, oracle, SLOT, "F4_5", instances.MATRIX["F4_5"])
    tms, scale, offset = surface_ref.case_transforms(oracle)
    cs = ctx.cameras_from_matrices(tms[:1], util.FOV_X, FW, FH, scale, offset)
    ocam = oracle.cameras_from_transforms(tms[:1], util.FOV_X, FW, FH, scale, offset)[0]
    tc = [f32(v) for v in util.termination_variants(f32(1) - f32(0.5))]
    b = surface_ref.Bounds(surface_ref.render_variants(oracle.lib(), m.f, ocam, FW, FH, tc, 0, 1, 1e-4, 1))
    (_, _, z, hit), _ = _surface(ctx, SLOT, cs, api.render_opts(FW, FH, 0, 1, 1e-4, step_mode=1), 0.5)
    cs.close()
    m.f.close()
    ctx.synthetic_model(SLOT, api.field_desc(**util.SMALL), util.SEED_A)
    exact, loose = ~b.loose, b.loose
    assert np.array_equal(hit[0][exact].view(np.uint32), b.hit_lo[exact].view(np.uint32))
    assert _ulps(z[0][exact], b.z_lo[exact]).max() <= Z_ULPS
    assert ((b.z_lo[loose] <= z[0][loose]) & (z[0][loose] <= b.z_hi[loose])).all()
    assert ((b.hit_lo[loose] <= hit[0][loose]) & (hit[0][loose] <= b.hit_hi[loose])).all()
    assert (_ulps(z[0][None].repeat(3, 0), b.z_var).min(axis=0) <= Z_ULPS).all() and (hit[0][None] == b.hit_var).any(axis=0).all()
    print(f"SURFACE_FIGURES F4_5 at bias 3, engine's rule: {int((exact & b.hit_pixels).sum())} hit pixels exact, {int((loose & b.hit_pixels).sum())} between the variants")
    assert (exact & b.hit_pixels).sum() > 50 and (loose & b.hit_pixels).sum() > 50


# ---- (g) the planner
def test_planner_takes_three_views_per_round_with_the_surface_locator(tmp_path):
    import os

    total, k = 5, 3
    save, chosen, trained = _plan(tmp_path, "surface", "\nviews_per_iteration: 3\nselect_locator: surface\nselect_level: 0.5")
    assert len(chosen) == total and len(set(chosen)) == total and chosen[0] == 1
    moves = sorted(f for f in os.listdir(save / "movement") if f != "-1.txt")
    assert moves == ["0.txt", "1.txt"] and trained == [1, 4]
    lines = [open(save / "movement" / f).read().splitlines() for f in moves]
    assert [len(l) for l in lines] == [3, 1]  # three views in the first round, then the one that is left
    assert [int(l.split("\t")[0]) for ls in lines for l in ls] == chosen[1:]
    gains = np.frombuffer((save / "gains" / "0.bin").read_bytes(), np.uint64)
    assert len(gains) == k and gains[0] > 0 and gains[0] >= gains[1] >= gains[2]
