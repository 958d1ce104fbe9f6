"""Scoring rounds and hand-written tables on fields that hold dense replicas (tests/test_gpu_replica.py has the single-model
renders).  The field is the F4_5 entry of tests/instances.py throughout; the reference of every comparison is the same call
in a context whose models were all installed with PRV_REPLICA_LEVELS=0 -- the hashed gather, which tests/test_gpu_instances.py
pins to the oracle -- and every comparison is BYTE FOR BYTE: no tolerance appears in this file (the one oracle anchor of a
round uses the suite's pixel bar, util.PIX_RTOL, as it stands).

1. Ensemble rounds (Context.score_views, methods 3 and 2) whose members hold DIFFERENT replica counts, installed one by one
   under their own PRV_REPLICA_LEVELS: the one-march-launch round renders member e through launch_render(rp, m.rdev, ...), the
   member-by-member path through render_views; a member rendered through another member's ReplicaDev, a variant chosen by
   another member's count, or a member's spp > 1 staging image mixed up would change a record.
2. A table in which no two entries of a level are equal (within windows of 61 441 entries), queried exactly ON the vertices of
   the hashed levels, where the interpolated feature is the entry itself: a replica filled from a wrong source entry cannot
   hide behind two entries that happen to hold the same half.
3. One member of a mixed round against the oracle's render.

The switches are read when a context is created and when a model is installed: every case builds its own contexts."""
import math
from fractions import Fraction

import numpy as np
import pytest

from nerf_prv_amd import api
from tests import instances, util
from tests.test_gpu_instances import environment
from tests.test_gpu_ngp_step import _ensemble_with_own_occupancies
from tests.test_gpu_replica import F4_5, PLAIN, VARIANTS, expected_bytes, fresh, hashed_res, restated_replica  # noqa: F401

gpu = pytest.mark.gpu

SEED0 = 4242
# members, score method, the replica count each member is installed with
ENSEMBLES = {5: (api.L.SCORE_ENSEMBLE_RGB_DENSITY, (3, 0, 1, 2, 3)), 2: (api.L.SCORE_ENSEMBLE_RGB, (2, 3))}
SUBSET = [5, 2, 3]  # a view subset, in another order
SPARE_SLOT = 5      # of the reference contexts: test_rounds_can_see_a_mix_up's hybrid member
N_VIEWS = 7
MIN_T = 0.01
FIXED_S = 64


# ------------------------------------------------------------------ 1. rounds
class _InstallUnder:
    """what _ensemble_with_own_occupancies installs through: member e goes into slot e under ITS replica count"""

    def __init__(self, c, counts):
        self.c, self.counts = c, counts

    def load_model(self, slot, *arrays):
        with environment({"PRV_REPLICA_LEVELS": str(self.counts[slot])}):
            self.c.load_model(slot, *arrays)


def ensemble_context(oracle, env, counts):
    with environment(env):
        c = api.Context(0)
    _ensemble_with_own_occupancies(_InstallUnder(c, counts), oracle, F4_5.kw, len(counts), SEED0)
    for e, n in enumerate(counts):
        instances.assert_layout(c.model_layout(e), F4_5)
        assert api.replica_layout(c, e) == (n, expected_bytes(F4_5.kw, n)), (e, n)
    return c


@pytest.fixture(scope="module")
def contexts(oracle):
    """(members, environment) -> (the context whose members hold ENSEMBLES' counts, the reference context: every count 0),
    built on first use and kept for the module"""
    made = {}

    def get(n_members, env):
        key = (n_members, tuple(sorted(env.items())))
        if key not in made:
            counts = ENSEMBLES[n_members][1]
            made[key] = (ensemble_context(oracle, env, counts), ensemble_context(oracle, env, (0,) * n_members))
        return made[key]

    yield get
    for pair in made.values():
        for c in pair:
            c.close()


def round_opts(rule, w, h, spp):
    if rule == "ngp":
        return api.engine_render_opts(w, h, 0, spp, MIN_T, background=(0, 0, 0, 1))
    return api.render_opts(w, h, FIXED_S, spp, MIN_T, background=(0, 0, 0, 1))


def play_round(c, oracle, n_members, rule, spp, size, slots=None):
    """-> (records' bytes, samples live, samples evaluated) of the round over all views and over SUBSET, and the records"""
    tms, scale, offset = util.hemisphere_transforms(oracle, util.fibonacci_hemisphere(N_VIEWS))
    w, h = size
    cs = c.cameras_from_matrices(tms, util.FOV_X, w, h, scale, offset)
    opts = round_opts(rule, w, h, spp)
    slots = list(range(n_members)) if slots is None else slots
    out = []
    for ids in (None, SUBSET):
        rec, st = c.score_views(ENSEMBLES[n_members][0], slots, cs, ids, opts, want_stats=True)
        out.append((rec.tobytes(), int(st.samples_live), int(st.samples_evaluated)))
    cs.close()
    return out, rec


def assert_round_equals_reference(contexts, oracle, env, n_members, rule, spp, size):
    mixed, ref = contexts(n_members, env)
    got, _ = play_round(mixed, oracle, n_members, rule, spp, size)
    want, rec = play_round(ref, oracle, n_members, rule, spp, size)
    what = (env, n_members, rule, spp, size)
    for g, w_, views in zip(got, want, ("all views", SUBSET)):
        assert w_[1] > 0 and w_[2] > 0, (what, views)
        assert g[1:] == w_[1:], (what, views, "samples live / evaluated", g[1:], w_[1:])
        assert g[0] == w_[0], (what, views, "records differ from the reference context's")
    assert np.all(np.isfinite(rec["score"])) and len(set(rec["score"].tolist())) > 1


@gpu
@pytest.mark.parametrize("size", [(44, 36), (20, 16)])
@pytest.mark.parametrize("rule", ["ngp", "fixed"])
@pytest.mark.parametrize("spp", [1, 3])
@pytest.mark.parametrize("n_members", [5, 2])
def test_round_of_members_with_different_replica_counts(contexts, oracle, n_members, spp, rule, size):
    """PRV_CELL_CACHE=0: the engine's rule goes through the replica variant (at most kReplicaLevelsNgp levels of what a member
    holds), not through the corner-cache instance; five members take the one-march-launch round under the engine's rule, two
    members and the fixed rule go member by member"""
    assert_round_equals_reference(contexts, oracle, PLAIN, n_members, rule, spp, size)


@gpu
@pytest.mark.parametrize("multi", ["0", "1"])
@pytest.mark.parametrize("n_members", [5, 2])
def test_round_on_the_one_launch_and_the_member_by_member_path(contexts, oracle, n_members, multi):
    """the spp-3 round under the engine's rule, forced through one march launch for the ensemble (every member's own staging
    image, then spp_reduce) and through one march launch per member: both equal the reference context's"""
    assert_round_equals_reference(contexts, oracle, dict(PLAIN, PRV_MARCH_MULTI=multi), n_members, "ngp", 3, (44, 36))


@gpu
def test_round_with_nothing_set(contexts, oracle):
    """the default environment: at these image sizes the engine's rule runs the corner-cache instance (render_policy), which has
    no replica variant and reads the hashed table of members that hold replicas; the fixed rule runs <false, NREPL>"""
    for rule in ("ngp", "fixed"):
        assert_round_equals_reference(contexts, oracle, {}, 5, rule, 3, (44, 36))


@gpu
@pytest.mark.parametrize("n_members", [5, 2])
def test_rounds_can_see_a_mix_up(contexts, oracle, n_members):
    """What the comparisons above rest on, shown in the reference context (no replicas anywhere).
      * The members' images differ: scored one by one against the same reference image, no two members have the same score at
        any view.
      * The records follow the members' images: with one member's slot replaced by its neighbour's they change.
      * The records see the mix-up itself: member 1 with its hashed levels -- all three, or the coarsest alone -- taken from
        member 0's table, which is what member 1 rendered through member 0's ReplicaDev computes, gives other records.
      * A round over the same members in another slot ORDER cannot show anything: both scores are symmetric functions of the
        members' bytes (per pixel a mean and a variance over the members), so the permuted round renders the same images and
        scores them the same.  For two members that holds to the bit -- (a + b) / 2 and the deviations +-(a - b) / 2 of two
        bytes are exact in double, the variance is the same double in either order -- and is asserted; for five members the
        order could reach a record only through the rounding of the sums over the members (on an MI355X it does not: equal
        bytes), and only the counts are asserted."""
    _, ref = contexts(n_members, PLAIN)
    w, h = 44, 36
    tms, scale, offset = util.hemisphere_transforms(oracle, util.fibonacci_hemisphere(N_VIEWS))
    cs = ref.cameras_from_matrices(tms, util.FOV_X, w, h, scale, offset)
    opts = round_opts("ngp", w, h, 1)
    gt = np.random.default_rng(77).random((N_VIEWS, h, w, 4), dtype=np.float32)
    gt[..., :3] *= gt[..., 3:]
    gt = ref.torch.from_numpy(gt).to(ref.device).contiguous()
    scores = [ref.score_views(api.L.SCORE_PSNR_COVERAGE, [e], cs, None, opts, gt=gt)[0]["score"] for e in range(n_members)]
    cs.close()
    for a in range(n_members):
        assert np.all(np.isfinite(scores[a]))
        for b in range(a):
            assert np.all(scores[a] != scores[b]), (a, b, scores[a], scores[b])
    base, _ = play_round(ref, oracle, n_members, "ngp", 1, (w, h))
    again, _ = play_round(ref, oracle, n_members, "ngp", 1, (w, h))
    assert base == again  # (a round is deterministic: a difference below is the slots')
    replaced, _ = play_round(ref, oracle, n_members, "ngp", 1, (w, h), slots=[1] + list(range(1, n_members)))
    assert replaced[0][0] != base[0][0] and replaced[1][0] != base[1][0]
    d = api.field_desc(**F4_5.kw)
    (t0, _, _), (t1, m1, o1) = ref.export_model(0, d), ref.export_model(1, d)
    hashed = [(first, n) for _, _, is_hashed, n, first in level_offsets(F4_5.kw) if is_hashed]
    F = F4_5.kw["n_features"]
    for borrowed in (hashed, hashed[:1]):
        t = t1.copy()
        for first, n in borrowed:
            t[first * F:(first + n) * F] = t0[first * F:(first + n) * F]
        assert not np.array_equal(t, t1)
        with environment({"PRV_REPLICA_LEVELS": "0"}):
            ref.load_model(SPARE_SLOT, d, t, m1, o1)
        mixed_up, _ = play_round(ref, oracle, n_members, "ngp", 1, (w, h), slots=[0, SPARE_SLOT] + list(range(2, n_members)))
        assert mixed_up[0][1] == base[0][1]  # (the occupancy is member 1's: the same steps)
        assert mixed_up[0][0] != base[0][0] and mixed_up[1][0] != base[1][0], len(borrowed)
    permuted, _ = play_round(ref, oracle, n_members, "ngp", 1, (w, h), slots=list(range(n_members))[::-1])
    assert permuted[0][1:] == base[0][1:] and permuted[1][1:] == base[1][1:]  # the same rays, steps and samples, whatever the order
    if n_members == 2:
        assert permuted[0][0] == base[0][0] and permuted[1][0] == base[1][0]


# ------------------------------------------------------------------ 3. one oracle anchor for a round
@gpu
def test_member_of_a_mixed_round_against_the_oracle(contexts, oracle):
    """member 2 (one replica, the all-occupied grid) of the five-member context, engine's rule, spp 1, one 44x36 view, against
    the oracle's render of the same parameters at the suite's pixel bar: the byte-equal family hangs on something outside
    the library"""
    mixed, _ = contexts(5, PLAIN)
    assert api.replica_layout(mixed, 2)[0] == ENSEMBLES[5][1][2] == 1
    w, h, view = 44, 36, 4
    tms, scale, offset = util.hemisphere_transforms(oracle, util.fibonacci_hemisphere(N_VIEWS))
    cs = mixed.cameras_from_matrices(tms, util.FOV_X, w, h, scale, offset)
    img, _ = mixed.render(2, cs, [view], round_opts("ngp", w, h, 1))
    cs.close()
    d_o = oracle.desc(**F4_5.kw)
    seeded = oracle.OracleField(d_o, seed=SEED0 + 2)
    t, m, o = seeded.params()
    seeded.close()
    f = oracle.OracleField(d_o, params=(t, m, np.full_like(o, 0xFFFFFFFF)))  # _ensemble_with_own_occupancies' member 2
    oc = oracle.cameras_from_transforms(tms, util.FOV_X, w, h, scale, offset)[view]
    wants = [f.render(oc, w, h, 0, 1, mt, step_mode=oracle.STEP_NGP)[0] for mt in util.termination_variants(MIN_T)]
    f.close()
    got = img[0].cpu().numpy()
    util.assert_pixels_close_any(got, wants)
    assert (got[..., 3] > 0.5).mean() > 0.1


# ------------------------------------------------------------------ 2. a table in which no two entries are equal
HASH_Y, HASH_Z = 2654435761, 805459861
WINDOW = 61441          # entries i and j of a level hold different halfs in every feature unless i = j (mod WINDOW)
_h = np.arange(1 << 16, dtype=np.uint32)
FINITE = _h[((_h >> 10) & 31 != 31) & (_h & 0x7FFF != 0)].astype(np.uint16)  # every finite binary16 but the two zeros
assert len(FINITE) == 63486 >= WINDOW
STRIDE = 25013          # a unit modulo len(FINITE) = 2 * 3^2 * 3527: i -> i * STRIDE is a bijection, neighbours land far apart
assert math.gcd(STRIDE, len(FINITE)) == 1


def level_offsets(kw):
    """[(scale, res, hashed, entries, first entry)] of the canonical table (tests/instances.py: restated_levels)"""
    out, off = [], 0
    for s, res, hashed, n in instances.restated_levels(kw):
        out.append((s, res, hashed, n, off))
        off += n
    return out


def injective_table(kw):
    """the canonical table: entry i, feature k of level l = FINITE[((i mod WINDOW) * STRIDE + 15013 k + 4001 l) mod 63486].
    Within an aligned window of WINDOW entries the map i -> half is injective for every feature (a bijection of Z_63486
    restricted to WINDOW <= 63486 residues); the four features of an entry and the levels are offset against each other."""
    F = kw["n_features"]
    parts = []
    for l, (_, _, _, n, _) in enumerate(level_offsets(kw)):
        i = np.arange(n, dtype=np.int64)[:, None] % WINDOW
        k = np.arange(F, dtype=np.int64)[None, :]
        parts.append(FINITE[(i * STRIDE + 15013 * k + 4001 * l) % len(FINITE)].reshape(-1))
    return np.concatenate(parts)


def hash_index(x, y, z, entries):
    """the hashed levels' entry of vertex (x, y, z): prv_levels.hpp's hash, restated"""
    x, y, z = (np.asarray(v, np.uint64) for v in (x, y, z))
    return ((x ^ (y * np.uint64(HASH_Y)) ^ (z * np.uint64(HASH_Z))) & np.uint64(entries - 1)).astype(np.int64)


def _rounds_to(val, k):
    """the exact rational val rounds to the integer k in binary32, away from every tie"""
    e = k.bit_length() - 1
    up = Fraction(2) ** (e - 24)  # half the spacing above k
    return (-(up / 2 if k == 1 << e else up)) < val - k < up


def exact_vertex_coords(scale):
    """{k: p}: binary32 coordinates p in [0, 1] with fmaf(scale, p, 0.5) == k EXACTLY (checked in rational arithmetic), so that
    the cell is k, the weight of vertex k is 1 and that of k + 1 is 0.  k runs from 1 (the position is scale * p + 0.5 >= 0.5:
    vertex 0 always shares its weight) to the cell of p = 1, the last one; a k none of whose neighbouring p rounds to it is
    left out."""
    s32 = np.float32(scale)
    s = Fraction(float(s32))
    last = int(np.floor(s32 + np.float32(0.5)))
    out = {}
    for k in range(1, last + 1):
        p = np.float32((k - 0.5) / float(s32))
        cands = [p]
        for _ in range(3):
            cands = [np.nextafter(cands[0], np.float32(-1))] + cands + [np.nextafter(cands[-1], np.float32(2))]
        cands = [c for c in cands if 0.0 <= c <= 1.0]
        cands.sort(key=lambda c: abs(s * Fraction(float(c)) + Fraction(1, 2) - k))
        if cands and _rounds_to(s * Fraction(float(cands[0])) + Fraction(1, 2), k):
            out[k] = cands[0]
    return out, last


class VertexQueries:
    """positions on the vertices of the hashed levels of `kw`.  Per hashed level: one vertex per distinct table entry among the
    vertices that can be hit exactly, a seeded sample of them that reaches MORE than half of the distinct entries the level's
    replica covers (all of [0, res - 1]^3), the corners of the last cell, and p = 1 on each axis, pair of axes and all three
    with the other axes on vertices (the duplicated-border rows and planes of a replica where the scale is an integer)."""

    def __init__(self, kw, share=0.55, seed=5):
        rng = np.random.default_rng(seed)
        self.kw, self.levels = kw, []
        pos = []
        for l, (s, res, hashed, entries, first) in enumerate(level_offsets(kw)):
            if not hashed:
                continue
            coords, last = exact_vertex_coords(s)
            assert last in coords and len(coords) >= 0.75 * last, (l, last, len(coords))  # (assert_reach says what that reaches)
            ks = np.array(sorted(coords))
            g = np.arange(res)
            covered = np.unique(hash_index(g[:, None, None], g[None, :, None], g[None, None, :], entries))
            idx = hash_index(ks[:, None, None], ks[None, :, None], ks[None, None, :], entries).reshape(-1)
            _, firsts = np.unique(idx, return_index=True)
            pick = rng.permutation(firsts)[:int(math.ceil(share * len(covered)))]
            corner = [np.ravel_multi_index(tuple(len(ks) - 1 - b for b in bits), (len(ks),) * 3) for bits in np.ndindex(2, 2, 2)]
            pick = np.unique(np.concatenate([pick, corner]))
            kx, ky, kz = (ks[a] for a in np.unravel_index(pick, (len(ks),) * 3))
            lut = np.zeros(last + 1, np.float32)
            lut[ks] = [coords[k] for k in ks]
            p = np.stack([lut[kx], lut[ky], lut[kz]], 1)
            self.levels.append(dict(level=l, first=first, entries=entries, covered=covered, start=sum(len(q) for q in pos), n=len(p),
                                    vertex=np.stack([kx, ky, kz], 1), entry=hash_index(kx, ky, kz, entries)))
            pos.append(p)
            few = lut[np.unique(np.concatenate([ks[:2], ks[-2:], rng.choice(ks, 8)]))]
            for axes in ((0,), (1,), (2,), (0, 1), (0, 2), (1, 2), (0, 1, 2)):
                rest = [a for a in range(3) if a not in axes]
                grid = np.stack(np.meshgrid(*([few] * len(rest)), indexing="ij"), -1).reshape(-1, len(rest)) if rest else np.zeros((1, 0), np.float32)
                q = np.ones((len(grid), 3), np.float32)
                q[:, rest] = grid
                pos.append(q)
        self.n_vertex_and_border = sum(len(q) for q in pos)
        pos.append(rng.random((3000, 3), dtype=np.float32))  # interior: all eight corners contribute
        self.pos = np.ascontiguousarray(np.concatenate(pos), np.float32)

    def assert_reach(self):
        """the exact-vertex positions reach at least half of the distinct entries each replica covers"""
        for L in self.levels:
            reached = np.unique(L["entry"])
            assert np.isin(reached, L["covered"]).all()
            assert 2 * len(reached) >= len(L["covered"]) > 0.5 * L["entries"], (L["level"], len(reached), len(L["covered"]))

    def entries_expected(self, table, L):
        """(n, F): the table entries the level's vertex positions must return as they are"""
        F = self.kw["n_features"]
        return table.reshape(-1, F)[L["first"] + L["entry"]]


def injective_model(oracle, kw):
    seeded = oracle.OracleField(oracle.desc(**kw), seed=util.SEED_A)
    _, mlp, occ = seeded.params()
    seeded.close()
    return injective_table(kw), mlp, np.full_like(occ, 0xFFFFFFFF)


@gpu
def test_replica_of_a_table_without_equal_entries(oracle):
    kw = F4_5.kw
    assert [res for _, res, hashed, _, _ in level_offsets(kw) if hashed] == hashed_res(kw) == [48, 68, 96]
    q = VertexQueries(kw)
    q.assert_reach()
    params = injective_model(oracle, kw)
    f = oracle.OracleField(oracle.desc(**kw), params=params)
    want = f.encode(q.pos)
    f.close()
    F = kw["n_features"]
    for L in q.levels:  # the oracle agrees that these positions return entries
        got = want[L["start"]:L["start"] + L["n"], L["level"] * F:(L["level"] + 1) * F]
        assert np.array_equal(got, q.entries_expected(params[0], L)), L["level"]
    outs = {}
    for n in (0,) + VARIANTS:
        with environment(dict(PLAIN, PRV_REPLICA_LEVELS=str(n))):
            c = api.Context(0)
            c.load_model(0, api.field_desc(**kw), *params)
        instances.assert_layout(c.model_layout(0), F4_5)
        assert api.replica_layout(c, 0) == (n, expected_bytes(kw, n))
        outs[n] = c.debug_encode(0, q.pos)
        c.close()
    for n in VARIANTS:
        bad = np.argwhere(outs[n] != outs[0])
        assert len(bad) == 0, (f"NREPL {n}: {len(bad)} feature halfs differ from replicas off, first at position {q.pos[bad[0][0]]!r} "
                               f"(index {bad[0][0]} of {q.n_vertex_and_border} vertex and border positions), level {bad[0][1] // F}")
    for n in (0,) + VARIANTS:
        bad = np.argwhere(outs[n] != want)
        assert len(bad) == 0, f"NREPL {n}: {len(bad)} feature halfs differ from the oracle's, first at position {q.pos[bad[0][0]]!r}, level {bad[0][1] // F}"
