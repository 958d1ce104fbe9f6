"""The queue cases of tests/queue_cases.py force what they claim, from the oracle and the restated layout alone (no GPU): a
case that has silently stopped overflowing fails here, not on the GPU.

Two layouts: the context's default (8 octant regions x 8 sub-regions = 64 counters) and PRV_QUEUE_SEGMENTS=1.  Under the latter
n_seg = n_sub = 8, the octant drops out of (octant * n_sub + sub) % n_seg, every sub-region is preferred by at most
ceil(blocks / 8) blocks' rays and seg_cap = ceil(blocks / 8) * 256 + 64 holds them: the overflow conditions CANNOT hold there (the
pigeonhole bound n_sub * seg_cap exceeds the batch), so that layout is asserted to be what it is -- a second control beside
PRV_SPATIAL_REGIONS=0 -- and the conditions that do not depend on the layout (counts, skew, gaps, opaque) are asserted for both.

Run with -s for the figures (QUEUE_CASE lines)."""
import numpy as np
import pytest

from tests import queue_cases as qc
from tests import util

SEGMENTS = [8, 1]


def _figures(oracle, name, mode, segments):
    c = qc.get(name)
    p = qc.population(oracle, c, mode)
    L = qc.Layout(c.w, c.h, c.spp, segments)
    pref = p.preferred(L)
    print(f"QUEUE_CASE {name} {'ngp' if mode else 'S128'} segments={segments}: live rays {p.n_rays}, blocks {L.blocks(c.n_views)}, n_seg {L.n_seg}, "
          f"seg_cap {L.seg_cap(c.n_views)}, n_sub * seg_cap {L.n_sub * L.seg_cap(c.n_views)}, preferred per octant region "
          f"{pref.reshape(-1, L.n_sub).sum(axis=1).tolist()}, most preferred sub-region {int(pref.max())}")
    assert pref.sum() == p.n_rays
    assert L.invariant(c.n_views)
    return c, p, L, pref


def _assert_control(c, L, pref):
    """PRV_QUEUE_SEGMENTS=1: no sub-region can be asked for more than it holds"""
    assert L.n_seg == L.n_sub == qc.K_SUB
    assert pref.max() <= -(-L.blocks(c.n_views) // L.n_seg) * 256 <= L.seg_cap(c.n_views) - 64


@pytest.mark.parametrize("segments", SEGMENTS)
@pytest.mark.parametrize("mode", [qc.FIXED, qc.NGP], ids=["fixed", "ngp"])
@pytest.mark.parametrize("name,octant", [("octant_high", 7), ("octant_low", 0)])
def test_octant_cases_overflow_their_octants_region(oracle, name, octant, mode, segments):
    """the live rays that prefer the octant's region exceed its n_sub * seg_cap records by at least 25 %: some wave must move on,
    one reservation per sub-region must straddle; octant 7's overflow wraps to region 0, octant 0's own XCD finds the others empty"""
    c, p, L, pref = _figures(oracle, name, mode, segments)
    if segments == 1:
        return _assert_control(c, L, pref)
    per_oct = pref.reshape(8, L.n_sub).sum(axis=1)
    assert per_oct[octant] >= 1.25 * L.n_sub * L.seg_cap(c.n_views)
    assert per_oct[octant] == p.n_rays or per_oct[octant] >= 0.95 * p.n_rays  # (a few rays see the far cell only)
    assert p.n_rays <= L.n_seg * (L.seg_cap(c.n_views) - 63)
    # the block lies wholly inside the octant: the box's centre is outside it
    lo, hi = c.occ_box()
    mid = 0.5 * (lo + hi)
    z, y, x = np.nonzero(c.occ)
    block = (np.stack([x, y, z], 1) >= 4) & (np.stack([x, y, z], 1) < 28)
    cells = np.stack([x, y, z], 1)[block.all(axis=1)]
    assert len(cells) == 8 ** 3
    assert ((cells / qc.R > mid).all() if octant == 7 else ((cells + 1) / qc.R < mid).all())


@pytest.mark.parametrize("segments", SEGMENTS)
@pytest.mark.parametrize("mode", [qc.FIXED, qc.NGP], ids=["fixed", "ngp"])
def test_one_subregion_takes_every_live_ray(oracle, mode, segments):
    c, p, L, pref = _figures(oracle, "one_subregion", mode, segments)
    assert L.tiles_x == 8 and (L.tiles_x * L.tiles_y) % L.n_sub == 0  # lin % n_sub is the tile column, in every view
    cols = np.nonzero(p.live.any(axis=(0, 1, 2)))[0]
    assert cols.min() >= 16 * qc.ONE_SUB_COLUMN and cols.max() < 16 * qc.ONE_SUB_COLUMN + 16  # one tile column only
    assert p.live.any(axis=(0, 2, 3)).all()  # in every view
    if segments == 1:
        return _assert_control(c, L, pref)
    sub = pref.reshape(8, L.n_sub)
    o = int(np.argmax(sub.sum(axis=1)))
    assert sub[o, qc.ONE_SUB_COLUMN] == p.n_rays >= 1.25 * L.seg_cap(c.n_views)
    assert np.delete(sub[o], qc.ONE_SUB_COLUMN).sum() == 0  # its seven siblings are preferred by none


@pytest.mark.parametrize("mode", [qc.FIXED, qc.NGP], ids=["fixed", "ngp"])
@pytest.mark.parametrize("n", qc.COUNTS)
def test_counts_have_exactly_their_live_rays(oracle, n, mode):
    c = qc.get(f"counts{n}")
    p = qc.population(oracle, c, mode)  # (its masks' sum is the oracle's march count)
    assert p.n_rays == n
    f = c.oracle_field(oracle, util.SMALL)
    img, _ = f.render(c.ocams(oracle)[0], c.w, c.h, qc.S_FIXED if mode == qc.FIXED else 0, 1, c.min_T, step_mode=mode)
    f.close()
    assert int((img[..., 3] > 0).sum()) == n and np.array_equal(img[..., 3] > 0, p.live[0, 0])  # the oracle renders exactly those pixels
    if n:
        ys, xs = np.nonzero(p.live[0, 0])
        assert n < 63 or (xs.min() < 16 <= xs.max() and ys.min() < 16 <= ys.max())  # across the tiles' corner
    for segments in SEGMENTS:
        _figures(oracle, c.name, mode, segments)


@pytest.mark.parametrize("mode", [qc.FIXED, qc.NGP], ids=["fixed", "ngp"])
def test_skew_puts_the_shortest_and_the_longest_rays_in_one_wave(oracle, mode):
    c = qc.get("skew")
    p = qc.population(oracle, c, mode)
    for segments in SEGMENTS:
        _, _, L, _ = _figures(oracle, "skew", mode, segments)
        ex = p.wave_extremes(L, p.count)
        few, many = (2, 600) if mode == qc.NGP else (1, 100)
        both = [e for e in ex if e[0] <= few and e[1] >= many]
        print(f"QUEUE_CASE skew: {len(both)} of {len(ex)} live waves hold a ray with <= {few} and one with >= {many} live samples: {both[:4]}")
        assert both
    _assert_nothing_terminates(oracle, c, p, mode)


def _assert_nothing_terminates(oracle, c, p, mode):
    f = c.oracle_field(oracle, util.SMALL)
    for v, oc in enumerate(c.ocams(oracle)):
        _, n_eval = f.render(oc, c.w, c.h, qc.S_FIXED if mode == qc.FIXED else 0, c.spp, c.min_T, step_mode=mode)
        assert n_eval == p.n_live_samples[v] > 0
    f.close()


def test_gaps_leave_whole_extension_chunks_empty(oracle):
    c = qc.get("gaps")
    assert c.modes == (qc.NGP,)
    p = qc.population(oracle, c, qc.NGP, keep_masks=True)
    rep = qc.gap_report(p)
    assert len(rep) == p.n_rays > 0
    for chunks, breaks, base0 in rep:
        assert len(breaks) == 1  # two occupied stretches
        a, b = breaks[0]  # empty steps [a, b)
        assert b - a >= 128
        first_empty_chunk = -(-(a - base0) // 128)
        assert base0 + 128 * (first_empty_chunk + 1) <= b and first_empty_chunk >= 1  # a whole extension chunk without a live step
        assert chunks[0] == 0 and chunks[-1] >= 2 and (b - base0) // 128 == chunks[-1] <= 7
    print(f"QUEUE_CASE gaps: {len(rep)} live rays, chunks with live steps {sorted(set(tuple(r[0]) for r in rep))}, empty steps e.g. {rep[0][1]}")
    _assert_nothing_terminates(oracle, c, p, qc.NGP)
    for segments in SEGMENTS:
        _figures(oracle, "gaps", qc.NGP, segments)


@pytest.mark.parametrize("mode", [qc.FIXED, qc.NGP], ids=["fixed", "ngp"])
def test_opaque_stops_every_ray_at_its_first_sample(oracle, mode):
    c = qc.get("opaque")
    p = qc.population(oracle, c, mode)
    f = c.oracle_field(oracle, util.SMALL)
    n_eval = sum(f.render(oc, c.w, c.h, qc.S_FIXED if mode == qc.FIXED else 0, c.spp, c.min_T, step_mode=mode)[1] for oc in c.ocams(oracle))
    f.close()
    assert n_eval == p.n_rays > 1000
    for segments in SEGMENTS:
        _figures(oracle, "opaque", mode, segments)


def test_camera_matrix_is_the_engine_camera(oracle):
    eye, target = np.array([0.2, -0.7, 1.9]), np.array([0.5, 0.4, 0.6])
    c2w = oracle.nerf_to_ngp(qc.camera_matrix(eye, target), 1.0, np.zeros(3))
    fwd = (target - eye) / np.linalg.norm(target - eye)
    np.testing.assert_allclose(c2w[:, 3], eye, atol=1e-6)
    np.testing.assert_allclose(c2w[:, 2], fwd, atol=1e-6)
    np.testing.assert_allclose(c2w[:, :3].T @ c2w[:, :3], np.eye(3), atol=1e-6)


@pytest.mark.parametrize("segments,spatial", [(8, 1), (1, 1), (8, 0), (3, 1)])
@pytest.mark.parametrize("W,H,spp,views", [(1, 1, 1, 1), (32, 32, 1, 1), (64, 48, 1, 8), (64, 48, 4, 8), (128, 48, 1, 8), (44, 36, 3, 5), (80, 45, 16, 7),
                                           (80, 45, 6, 7), (800, 800, 1, 64), (33, 17, 64, 3), (33, 17, 128, 3)])
def test_capacity_invariant(W, H, spp, views, segments, spatial):
    """n_seg * (seg_cap - 63) > blocks * 256: with one straddling reservation of at most 64 per region, the regions that are closed
    hold at least seg_cap - 63 records each; if a wave found every region closed the queue would hold more records than the batch
    has rays.  The argument behind the `unreachable` on region_reserve's last line"""
    L = qc.Layout(W, H, spp, segments, spatial)
    assert L.blocks(views) * 256 >= W * H * spp * views  # every ray has a thread
    assert L.seg_cap(views) == -(-L.blocks(views) // L.n_seg) * 256 + 64
    assert L.invariant(views)
    ix, iy, kk = L.threads()
    assert len({(a, b, c) for a, b, c in zip(ix, iy, kk)}) == 256 and ix.max() < 1 << L.tile_w_log2 and iy.max() < 1 << L.tile_h_log2
