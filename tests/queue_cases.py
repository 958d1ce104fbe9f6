"""Adversarial ray populations for the render queue (test infrastructure, no GPU): tests/test_queue_cases_host.py asserts
what each one forces from the oracle alone, tests/test_gpu_queue.py runs them.

A case is a field shape's worth of inputs built by hand: an occupancy grid ([z, y, x] bool, loaded through load_model as
tests/test_gpu_ngp_step.py's _ensemble_with_own_occupancies does), a density regime (density_bias / table_amp), cameras (in the
engine's frame, far and narrow where near-parallel rays are wanted), image size, spp and the stepping rules it runs under.

Restated here, in Python:
  * `Layout`: MarchLayout of prv_api.cpp -- the tiles of a march launch, blocks() and seg_cap(), and which pixel / sub-sample
    every thread of a block is (march_ray_setup: Morton order inside the tile, sub-samples on adjacent lanes for a power-of-two
    spp, on grid.z otherwise);
  * the region rule of march_emit (prv_kernels.hip): the wave's first live lane picks the region; the octant is that of the
    ray's position at the middle of its live span, (first + last live step) >> 1, t = fmaf(i + 0.5, dt, t0) and
    fmaf(t, d, o) > 0.5f * (occ_lo + occ_hi) in float32, occ_lo / occ_hi the one-cell-grown box of the occupied cells
    (summarize_occupancy); the sub-region is `linear block id % n_sub`; the region is (octant * n_sub + sub) % n_seg.
The masks are the oracle's: rays and box intersection through its exported primitives (oracle.raygen), the steps
t_i = fmaf(i + 0.5, dt, t0), p = fmaf(t, d, o) and orc_occupied's cell rule vectorised with tests/march_ref.py's fmaf (float64
product and sum, rounded once to float32); `population` asserts their sum against OracleField.march_count.

The capacity invariant (why region_reserve always finds room): a reservation fails in a region only once that region is closed,
and a closed region holds at least seg_cap - 63 records (one reservation of <= 64 straddles its end); with
n_seg * (seg_cap - 63) > blocks * 256 >= the batch's live rays, all regions closed would mean more records than rays.
"""
import numpy as np

from tests import march_ref, util

f32 = np.float32
R = 32  # occ_res of util.SMALL and of instances.MATRIX["F4_5"]
FIXED, NGP = 0, 1
S_FIXED = 128
K_SUB = 8  # kSubRegions
TRANSPARENT = dict(table_amp=0.1, density_bias=0.0)  # no ray terminates early
DEFAULT = {}
OPAQUE = dict(table_amp=0.1, density_bias=14.0)  # sigma dt ~ 1e3: T = 0 after the first sample


# ---------------------------------------------------------------- the layout (prv_api.cpp: MarchLayout)
class Layout:
    def __init__(self, W, H, spp, queue_segments=8, spatial_regions=1):
        self.W, self.H, self.spp = W, H, spp
        self.n_sub = K_SUB if spatial_regions else 1
        self.n_seg = queue_segments * self.n_sub
        self.spatial_regions = spatial_regions
        self.spp_inner_log2 = 0
        if 1 < spp <= 64 and spp & (spp - 1) == 0:
            while (1 << self.spp_inner_log2) < spp:
                self.spp_inner_log2 += 1
        pix_log2 = 8 - self.spp_inner_log2
        self.tile_w_log2, self.tile_h_log2 = (pix_log2 + 1) // 2, pix_log2 // 2
        self.tiles_x = (W + (1 << self.tile_w_log2) - 1) >> self.tile_w_log2
        self.tiles_y = (H + (1 << self.tile_h_log2) - 1) >> self.tile_h_log2

    def grid_z(self):
        return 1 if self.spp_inner_log2 > 0 else self.spp

    def blocks(self, n_views):
        return self.tiles_x * self.tiles_y * n_views * self.grid_z()

    def seg_cap(self, n_views):
        return ((self.blocks(n_views) + self.n_seg - 1) // self.n_seg) * 256 + 64

    def invariant(self, n_views):
        """n_seg * (seg_cap - 63) > blocks * 256"""
        return self.n_seg * (self.seg_cap(n_views) - 63) > self.blocks(n_views) * 256

    def threads(self):
        """-> (ix, iy, kk) int arrays [256]: the thread's pixel inside its tile and its sub-sample (-1: the block's grid.z)"""
        t = np.arange(256)
        i = t >> self.spp_inner_log2
        ix = (i & 1) | ((i >> 1) & 2) | ((i >> 2) & 4) | ((i >> 3) & 8)
        iy = ((i >> 1) & 1) | ((i >> 2) & 2) | ((i >> 3) & 4) | ((i >> 4) & 8)
        kk = t & ((1 << self.spp_inner_log2) - 1) if self.spp_inner_log2 > 0 else np.full(256, -1)
        return ix, iy, kk


# ---------------------------------------------------------------- cameras, in the engine's frame
def camera_matrix(eye, target, up=(0.0, 0.0, 1.0)):
    """a transform_matrix (scale 1, offset 0) whose engine camera sits at `eye` and looks at `target`: the engine's c2w is
    [right, down, forward, eye]; nerf_matrix_to_ngp negates columns 1, 2 and cycles the axes (engine xyz = nerf yzx)"""
    eye, target, up = (np.asarray(v, np.float64) for v in (eye, target, up))
    fwd = target - eye
    fwd /= np.linalg.norm(fwd)
    right = np.cross(fwd, up)
    right /= np.linalg.norm(right)
    down = np.cross(fwd, right)
    eng = np.stack([right, -down, -fwd, eye], axis=1)  # columns 1, 2 negated back
    tm = np.eye(4)
    tm[:3, :] = eng[[2, 0, 1], :]
    return tm


def fov_for(span, dist):
    """the horizontal field of view under which `span` engine units at distance `dist` fill the image's width"""
    return 2.0 * np.arctan(0.5 * span / dist)


class Case:
    def __init__(self, name, occ, regime, tms, fov, w, h, spp=1, modes=(FIXED, NGP), min_T=1e-4):
        self.name, self.occ, self.regime = name, np.ascontiguousarray(occ, bool), dict(regime)
        self.tms, self.fov, self.w, self.h, self.spp, self.modes, self.min_T = np.asarray(tms), float(fov), w, h, spp, tuple(modes), min_T
        self.scale, self.offset = 1.0, np.zeros(3)

    @property
    def n_views(self):
        return len(self.tms)

    def words(self):
        bits = np.packbits(self.occ.reshape(-1).astype(np.uint8), bitorder="little")
        return np.frombuffer(bits.tobytes(), np.uint32).copy()

    def kw(self, shape_kw):
        return dict(shape_kw, **self.regime)

    def oracle_field(self, oracle, shape_kw, seed=util.SEED_A):
        """the synthetic field of this shape and regime with the case's occupancy grid in place of its own"""
        d = oracle.desc(**self.kw(shape_kw))
        f = oracle.OracleField(d, seed=seed)
        t, m, o = f.params()
        f.close()
        assert o.size == self.words().size
        return oracle.OracleField(d, params=(t, m, self.words()))

    def load(self, ctx, oracle, slot, shape_kw, seed=util.SEED_A):
        """the same field into a context's slot -> its OracleField"""
        from nerf_prv_amd import api

        f = self.oracle_field(oracle, shape_kw, seed)
        ctx.load_model(slot, api.field_desc(**self.kw(shape_kw)), *f.params())
        return f

    def ocams(self, oracle):
        return oracle.cameras_from_transforms(self.tms, self.fov, self.w, self.h, self.scale, self.offset)

    def cams(self, ctx):
        return ctx.cameras_from_matrices(self.tms, self.fov, self.w, self.h, self.scale, self.offset)

    def opts(self, mode, min_T=None, **kw):
        from nerf_prv_amd import api

        return api.render_opts(self.w, self.h, S_FIXED if mode == FIXED else 0, self.spp, self.min_T if min_T is None else min_T, step_mode=mode, **kw)

    def occ_box(self):
        """summarize_occupancy's occ_lo / occ_hi (prv_field_plan.hpp; float32)"""
        z, y, x = np.nonzero(self.occ)
        if x.size == 0:
            return np.full(3, 2.0, f32), np.full(3, -1.0, f32)
        lo = np.array([x.min(), y.min(), z.min()])
        hi = np.array([x.max(), y.max(), z.max()])
        return (lo - 1).astype(f32) / f32(R), (hi + 2).astype(f32) / f32(R)


# ---------------------------------------------------------------- the oracle's masks, vectorised
def _fma(a, b, c):
    return (np.asarray(a, np.float64) * np.asarray(b, np.float64) + np.asarray(c, np.float64)).astype(f32)


def view_masks(oracle, case, ocam, mode, k):
    """-> (mask [h * w, n] bool, o, d [h * w, 3], t0, dt [h * w]) of sub-sample k's rays of one view: step i is live"""
    o, d, t = oracle.raygen(ocam, case.w, case.h, k)
    t0, t1 = t[:, 0], t[:, 1]
    hit = t1 > t0
    if mode == NGP:
        n, dt = march_ref.NGP_STEPS, np.full(len(t0), march_ref.NGP_DT, f32)
    else:
        with np.errstate(invalid="ignore"):
            n, dt = S_FIXED, ((t1 - t0) / f32(S_FIXED)).astype(f32)
    i = (np.arange(n, dtype=f32) + f32(0.5))[None, :]
    ts = _fma(i, dt[:, None], t0[:, None])
    ok = hit[:, None] & np.isfinite(ts)
    if mode == NGP:
        ok &= ts < t1[:, None]  # (t grows with i: the oracle's break at the first t >= t1)
    cell = np.zeros(ts.shape, np.int64)
    for a, mul in ((0, 1), (1, R), (2, R * R)):
        with np.errstate(invalid="ignore"):
            p = _fma(ts, d[:, a:a + 1], o[:, a:a + 1])
            c = (np.clip(np.nan_to_num(p), f32(0), f32(1)) * f32(R)).astype(np.int64)
        cell += np.minimum(c, R - 1) * mul
    return case.occ.reshape(-1)[cell] & ok, o, d, t0, dt


class Population:
    """what the march of one batch (all views of the case) gives the queue under one layout"""

    def __init__(self, case, mode, live, first, last, o, d, t0, dt, n_live_samples):
        self.case, self.mode = case, mode
        self.live, self.first, self.last = live, first, last  # [spp, views, h, w]
        self.o, self.d, self.t0, self.dt = o, d, t0, dt
        self.n_rays = int(live.sum())
        self.n_live_samples = n_live_samples  # per view
        self.steps = np.where(live, last - first + 1, 0)  # the live SPAN (gaps included)

    def octants(self):
        """the octant of every ray's mid-span position (meaningful where live)"""
        lo, hi = self.case.occ_box()
        mid = (f32(0.5) * (lo + hi)).astype(f32)
        i0 = ((self.first + self.last) >> 1).astype(f32) + f32(0.5)
        t = _fma(i0, self.dt, self.t0)
        oct_ = np.zeros(self.live.shape, np.int64)
        for a in range(3):
            oct_ |= (_fma(t, self.d[..., a], self.o[..., a]) > mid[a]).astype(np.int64) << a
        return oct_

    def waves(self, layout):
        """yields (lin, [(k, v, y, x) of the wave's valid lanes, in lane order]) for every wave of the launch"""
        c = self.case
        ix, iy, kk = layout.threads()
        gx, gy = layout.tiles_x * layout.tiles_y, c.n_views
        for bz in range(layout.grid_z()):
            for v in range(gy):
                for bx in range(gx):
                    ty, tx = divmod(bx, layout.tiles_x)
                    px, py = (tx << layout.tile_w_log2) + ix, (ty << layout.tile_h_log2) + iy
                    k = np.where(kk < 0, bz, kk)
                    lin = bx + gx * (v + gy * bz)
                    for w in range(4):
                        s = slice(64 * w, 64 * w + 64)
                        yield lin, [(int(k_), v, int(y_), int(x_)) for k_, y_, x_ in zip(k[s], py[s], px[s]) if x_ < c.w and y_ < c.h]

    def preferred(self, layout):
        """-> int [n_seg]: the live rays whose wave prefers each region (march_emit's rule)"""
        oct_ = self.octants()
        out = np.zeros(layout.n_seg, np.int64)
        for lin, lanes in self.waves(layout):
            idx = tuple(np.array(lanes).T) if lanes else None
            if idx is None:
                continue
            lv = self.live[idx]
            if not lv.any():
                continue
            first = np.argmax(lv)
            pref = int(oct_[idx][first]) * layout.n_sub + lin % layout.n_sub if layout.spatial_regions else lin
            out[pref % layout.n_seg] += int(lv.sum())
        return out

    def wave_extremes(self, layout, counts):
        """-> [(fewest, most) of `counts` over the wave's live rays] for every wave with a live ray"""
        out = []
        for _, lanes in self.waves(layout):
            if not lanes:
                continue
            idx = tuple(np.array(lanes).T)
            lv = self.live[idx]
            if lv.any():
                out.append((int(counts[idx][lv].min()), int(counts[idx][lv].max())))
        return out


_populations = {}


def population(oracle, case, mode, shape_kw=util.SMALL, keep_masks=False):
    """the case's rays under one stepping rule; the masks' sum is asserted against the oracle's march count, view by view.
    Cached: the masks do not depend on the field's shape beyond occ_res"""
    key = (case.name, mode, keep_masks)
    if key in _populations:
        return _populations[key]
    f = case.oracle_field(oracle, shape_kw)
    shp = (case.spp, case.n_views, case.h, case.w)
    live, first, last = np.zeros(shp, bool), np.zeros(shp, np.int64), np.zeros(shp, np.int64)
    o, d = np.zeros(shp + (3,), f32), np.zeros(shp + (3,), f32)
    t0, dt = np.zeros(shp, f32), np.zeros(shp, f32)
    count = np.zeros(shp, np.int64)
    masks = {}
    per_view = []
    for v, oc in enumerate(case.ocams(oracle)):
        tot = 0
        for k in range(case.spp):
            m, o_, d_, t0_, dt_ = view_masks(oracle, case, oc, mode, k)
            any_ = m.any(axis=1)
            live[k, v] = any_.reshape(case.h, case.w)
            first[k, v] = np.argmax(m, axis=1).reshape(case.h, case.w)
            last[k, v] = (m.shape[1] - 1 - np.argmax(m[:, ::-1], axis=1)).reshape(case.h, case.w)
            count[k, v] = m.sum(axis=1).reshape(case.h, case.w)
            o[k, v], d[k, v] = o_.reshape(case.h, case.w, 3), d_.reshape(case.h, case.w, 3)
            t0[k, v], dt[k, v] = t0_.reshape(case.h, case.w), np.nan_to_num(dt_).reshape(case.h, case.w)
            tot += int(m.sum())
            if keep_masks:
                masks[(k, v)] = m.reshape(case.h, case.w, -1)
        want = f.march_count(oc, case.w, case.h, S_FIXED if mode == FIXED else 0, case.spp, step_mode=mode)
        assert tot == want, (case.name, mode, v, tot, want)
        per_view.append(tot)
    f.close()
    p = Population(case, mode, live, first, last, o, d, t0, dt, per_view)
    p.count, p.masks = count, masks
    _populations[key] = p
    return p


# ---------------------------------------------------------------- the cases
def _cells(*boxes):
    """[z, y, x] grid with the given ((x0, x1), (y0, y1), (z0, z1)) half-open cell boxes occupied"""
    g = np.zeros((R, R, R), bool)
    for (x0, x1), (y0, y1), (z0, z1) in boxes:
        g[z0:z1, y0:y1, x0:x1] = True
    return g


def _around(centre, dist, n=8):
    """n eyes at `dist` from `centre`, one along every diagonal"""
    c = np.asarray(centre, np.float64)
    dirs = [(sx, sy, sz) for sz in (1, -1) for sy in (1, -1) for sx in (1, -1)][:n]
    return [c + dist * np.asarray(s, np.float64) * np.array([1.0, 0.8, 0.6]) / np.linalg.norm([1.0, 0.8, 0.6]) for s in dirs]


def _octant_case(name, block, far, spp, n_views):
    """a solid block wholly inside one octant of the occupied box + one far cell that stretches the box, so that the box's centre
    lies outside the block: every ray through the block prefers that octant's region.  Close-up views"""
    (x0, x1) = block
    occ = _cells(((x0, x1),) * 3, ((far, far + 1),) * 3)
    centre = np.full(3, 0.5 * (x0 + x1) / R)
    tms = [camera_matrix(e, centre) for e in _around(centre, 0.42, n_views)]
    return Case(name, occ, DEFAULT, tms, util.FOV_X, 64, 48, spp=spp)


def octant_high():
    return _octant_case("octant_high", (20, 28), 2, 4, 4)  # octant 7: the overflow wraps to region 0; spp 4: sub-samples on adjacent lanes


def octant_low():
    return _octant_case("octant_low", (4, 12), 29, 1, 8)  # octant 0


ONE_SUB_COLUMN = 5  # the tile column the object is seen in


def one_subregion():
    """a thin tall block (2 x 2 x 10 cells, in octant 0 of a box stretched by a far cell the views do not see) that every view
    sees inside tile column 5 of its 8 x 3 tiles: every live block has lin % 8 == 5"""
    occ = _cells(((6, 8), (6, 8), (3, 13)), ((29, 30),) * 3)
    p = np.array([7.0 / R, 7.0 / R, 8.0 / R])
    w, h, dist = 128, 48, 3.0
    fov = fov_for(128 * (0.1 / 11.0), dist)  # 11 pixels per 0.1 engine units
    focal = 0.5 * w / np.tan(0.5 * fov)
    shift = (16 * ONE_SUB_COLUMN + 8 - 0.5 * w) * dist / focal  # the block's image sits in the middle of the column
    tms = []
    for j in range(8):
        a = 2.0 * np.pi * (j + 0.25) / 8.0
        fwd = np.array([np.cos(a), np.sin(a), 0.0])
        right = np.cross(fwd, [0.0, 0.0, 1.0])
        eye = p - dist * fwd - shift * right
        tms.append(camera_matrix(eye, eye + fwd))
    return Case("one_subregion", occ, DEFAULT, tms, fov, w, h)


COUNTS = (0, 1, 63, 64, 65)


def counts(n):
    """exactly n live rays: n single occupied cells in the plane z = 16, seen from far away along z by a 32 x 32 image whose
    pixel (x, y) looks down the middle of cell column (x, y).  The cells fill a 9-wide window that straddles the four tiles'
    and the waves' corners at (16, 16)"""
    occ = np.zeros((R, R, R), bool)
    for j in range(n):
        occ[16, 12 + j // 9, 11 + j % 9] = True
    dist = 60.0
    eye = np.array([0.5, 0.5, 0.5 - dist])
    tm = camera_matrix(eye, [0.5, 0.5, 0.5], up=(0.0, -1.0, 0.0))
    return Case(f"counts{n}", occ, DEFAULT, [tm], fov_for(1.0, dist), 32, 32)


def skew():
    """seen from far away along (1, 1, 0): a bar along that direction through the whole cube (rays inside it are live from entry
    to exit: 800+ steps of the engine's rule, all 128 samples of the fixed rule) under a one-cell-thick staircase sheet
    x + y = 32 (cells that touch at their corners only: rays through a corner have one or two live samples), transparent field"""
    z, y, x = np.meshgrid(np.arange(R), np.arange(R), np.arange(R), indexing="ij")
    lateral = np.abs(x - y)
    bar = (lateral <= 3) & (z >= 14) & (z < 17)  # (the boundary between the two is not a wave's edge: row 24 is z = 16 cells)
    sheet = (x + y == R) & (z >= 17) & (z < 23)
    fwd = np.array([1.0, 1.0, 0.0]) / np.sqrt(2.0)
    dist = 40.0
    c = np.array([0.5, 0.5, 0.5])
    tms = [camera_matrix(c - s * dist * fwd, c) for s in (1.0, -1.0)]
    return Case("skew", bar | sheet, TRANSPARENT, tms, fov_for(0.9, dist), 64, 48)


def gaps():
    """two slabs at opposite ends of the cube (z < 2 and z >= 30 cells), seen along z from either side and at a slant: every ray
    enters through one slab and leaves through the other, ~520 empty steps apart"""
    occ = _cells(((0, R), (0, R), (0, 2)), ((0, R), (0, R), (30, R)))
    c = np.array([0.5, 0.5, 0.5])
    dist = 30.0
    eyes = [c + dist * np.array(e) for e in ((0.0, 0.0, -1.0), (0.0, 0.0, 1.0), (0.05, 0.03, -1.0))]
    tms = [camera_matrix(e, c, up=(0.0, 1.0, 0.0)) for e in eyes]
    return Case("gaps", occ, TRANSPARENT, tms, fov_for(0.6, dist), 40, 30, modes=(NGP,))


def opaque():
    """a solid ball in a field so dense that every ray stops at its first sample: a refill every round"""
    z, y, x = np.meshgrid(np.arange(R), np.arange(R), np.arange(R), indexing="ij")
    ball = ((x + 0.5) / R - 0.5) ** 2 + ((y + 0.5) / R - 0.5) ** 2 + ((z + 0.5) / R - 0.5) ** 2 < 0.3 ** 2
    c = np.array([0.5, 0.5, 0.5])
    tms = [camera_matrix(e, c) for e in _around(c, 1.2, 4)]
    return Case("opaque", ball, OPAQUE, tms, util.FOV_X, 64, 48)


def slab_grid():
    z = np.arange(R)[:, None, None]
    return np.broadcast_to(np.abs((z + 0.5) / R - 0.4) < 0.12, (R, R, R)).copy()


CASES = {"octant_high": octant_high, "octant_low": octant_low, "one_subregion": one_subregion, "skew": skew, "gaps": gaps, "opaque": opaque}
CASES.update({f"counts{n}": (lambda n=n: counts(n)) for n in COUNTS})
_cases = {}


def get(name):
    if name not in _cases:
        _cases[name] = CASES[name]()
    return _cases[name]


def runs():
    """every (case name, stepping rule) the case allows"""
    return [(n, m) for n in CASES for m in get(n).modes]


# ---------------------------------------------------------------- what a case must force (asserted on the host, relied on by the GPU tests)
def gap_report(p):
    """gaps: per live ray the chunks (128 steps from the first non-empty 32-step word on) that hold live steps, from the masks"""
    out = []
    for (k, v), m in p.masks.items():
        for y in range(p.case.h):
            for x in range(p.case.w):
                if not p.live[k, v, y, x]:
                    continue
                idx = np.nonzero(m[y, x])[0]
                base0 = 32 * (idx[0] // 32)
                chunks = sorted(set(((idx - base0) // 128).tolist()))
                breaks = np.nonzero(np.diff(idx) > 1)[0]
                out.append((chunks, [(int(idx[b]) + 1, int(idx[b + 1])) for b in breaks], base0))
    return out
