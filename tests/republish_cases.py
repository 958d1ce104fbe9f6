"""Inputs of the republish tests, shared by tests/test_republish_host.py (CPU: the oracle alone shows that every input changes what it
claims to change) and tests/test_gpu_republish.py (every consumer of a model slot, on a slot that changed under a context whose buffers
hold the old state, against a fresh context loaded with the slot's exported arrays: identical bytes).  No GPU is needed to import this.

Shapes: the four fast instances and the two generic ones of tests/instances.py.  Under a trainer they have occ_res 16, density_bias 1,
table_amp 0.5 (tests/test_gpu_train.py's TINY); the scene is that module's: 8 lens views at 24 x 16 of a denser field of the same shape.

Ways a warm slot changes (CHANGES):
  steps_shrink          64 optimiser steps from an all-occupied grid (STEPS_SHRINK: lr 1e-2, a refresh every 16 steps = four refreshes,
                        threshold 2, decay 0.5).  Table, MLP, occupancy, coarse grid and box change: the densities part into an object and
                        next to nothing, and the planes x = 0, 1 of the grid, which every ray crosses on its way to a transparent pixel,
                        go off.  steps_shrink_ngp: the same under the engine's marcher (STEPS_SHRINK_NGP: 40 rays a step, lr 2e-2, threshold 5,
                        refreshes at steps 30 and 60 -- an earlier one finds no density above the threshold and empties the grid).
  refresh_grow          one occupied corner cell (train_cases.refresh_field's construction, on this module's shapes; its own two shapes
                        are REFRESH_OWN), then Trainer.refresh_occupancy() alone, at a threshold in the widest gap of the cell densities
                        (train_cases.place_threshold): the box grows from one cell to most of the cube, table and MLP stay.
  reinstall_same_shape  load_model of another seed's arrays with another occupancy (the upper half of the cube) over the loaded slot.
  reinstall_other_shape F4_5 -> F2_10 -> F4_0 over one slot (RESHAPE): buffers and instance change under a live context.
  round                 a live trainer and one ROUND per consumer (four steps, a refresh after the fourth: table, MLP and occupancy move
                        every time), so that EVERY consumer meets a slot that is dirty when it is called -- in the other changes the first
                        consumer of the table rebuilds the derived state and the rest run on a clean slot.  dirty_order(): the consumers
                        that read the occupancy alone come first, while the grid still loses whole regions per round.
  members               two and five slots trained side by side (api.train_many) with STEPS_SHRINK's settings, each with its own refresh.

CONSUMERS is the table name -> Consumer of everything in nerf_prv_amd.api.Context that reads a slot.  A consumer returns a dict of numpy
arrays; two runs agree when every array has the same bytes.  `reads` says which canonical arrays can reach the output: a change that
leaves all of them alone (refresh_grow: the occupancy only) cannot change it, and then the output must be the old one."""
import numpy as np

from tests import instances, train_cases as tc, util

SHAPES = ["F4_5", "F4_3", "F2_10", "F2_6", "F4_0", "F2_0"]
RESHAPE = ["F4_5", "F2_10", "F4_0"]
TRAIN_OVERRIDES = dict(occ_res=16, density_bias=1.0, table_amp=0.5)
W, H, N_VIEWS = 56, 44, 5
GRID = 32  # density and marching-cubes grids
MIN_T = 1e-4
FIXED_S = 37
TRAIN_W, TRAIN_H, TRAIN_VIEWS = tc.W, tc.H, 8
STEPS_SHRINK = dict(steps=64, opts=dict(n_rays=192, n_samples=24, lr=1e-2, occ_every=16, occ_sigma_thresh=2.0, occ_decay=0.5))
STEPS_SHRINK_NGP = dict(steps=64, opts=dict(n_rays=40, step_mode=1, n_samples=1024, lr=2e-2, occ_every=30, occ_sigma_thresh=5.0, occ_decay=0.5))
ROUND = dict(steps=4, opts=dict(STEPS_SHRINK["opts"], occ_every=4))
ROUND_SHAPES = ["F4_5", "F2_10", "F4_0", "F2_0"]  # two fast instances, the two generic ones
REFRESH_OWN = {"R4": 4, "R2": 2}  # train_cases.refresh_field(oracle, 16, F) itself


def train_kw(name):
    return dict(instances.MATRIX[name].kw, **TRAIN_OVERRIDES)


def install_kw(name):
    """the reinstall cases: the matrix entry as it is (occ_res 32: a row of the grid is one whole word)"""
    return dict(instances.MATRIX[name].kw)


# ------------------------------------------------------------------ occupancy: box and words
def occupied_box(occ, R):
    """(lo[3], hi[3]) of the occupied cells in cells, x first, or None for an empty grid"""
    idx = np.argwhere(tc.bits_of(occ, R ** 3).reshape(R, R, R))
    return None if len(idx) == 0 else (idx.min(0)[::-1].copy(), idx.max(0)[::-1].copy())


def box_shrank(before, after):
    """inside the old box, and at least one cell smaller on at least one axis"""
    return bool(np.all(after[0] >= before[0]) and np.all(after[1] <= before[1]) and (np.any(after[0] > before[0]) or np.any(after[1] < before[1])))


def words_changed(a, b):
    return float(np.mean(np.asarray(a) != np.asarray(b)))


def assert_occupancy_preconditions(before, after, R, direction):
    """section 2 of the issue, on anybody's arrays: the box moves by a cell or more on some axis the way the change says, and a quarter of
    the words differ"""
    b0, b1 = occupied_box(before, R), occupied_box(after, R)
    assert b0 is not None and b1 is not None, (b0, b1)
    assert box_shrank(b0, b1) if direction == "shrink" else box_shrank(b1, b0), (direction, b0, b1)
    assert words_changed(before, after) >= 0.25, words_changed(before, after)
    return b0, b1


def upper_half(R):
    bits = np.zeros((R, R, R), np.uint8)
    bits[R // 2:] = 1
    return np.packbits(bits.reshape(-1), bitorder="little").view(np.uint32).copy()


# ------------------------------------------------------------------ the states
def training_scene(oracle, kw):
    """tests/test_gpu_train.py's scene for a shape -> dict(tms, intr, scale, offset), images"""
    gt = oracle.OracleField(oracle.desc(**dict(kw, density_bias=3.0, table_amp=2.0)), seed=util.SEED_B)
    tms, scale, offset = util.hemisphere_transforms(oracle, util.fibonacci_hemisphere(TRAIN_VIEWS))
    ds = dict(tms=tms, intr=dict(tc.LENS_INTR), scale=scale, offset=offset)
    imgs = np.stack([oracle.quantize_rgba8(gt.render(c, TRAIN_W, TRAIN_H, 32, 1, 1e-4)[0], (0, 0, 0, 0)) for c in tc.oracle_cameras(oracle, ds)])
    gt.close()
    return ds, imgs


def all_occupied(oracle, kw, seed=util.SEED_A):
    f = oracle.OracleField(oracle.desc(**kw), seed=seed)
    t, m, o = f.params()
    f.close()
    return t, m, tc.mask_tail(np.full_like(o, 0xFFFFFFFF), kw["occ_res"])


def synthetic(oracle, kw, seed):
    f = oracle.OracleField(oracle.desc(**kw), seed=seed)
    p = f.params()
    f.close()
    return p


def refresh_start(oracle, name):
    """-> (kw, parameters with one occupied corner cell, threshold): train_cases.refresh_field for R4 / R2, its construction (densities
    over two orders of magnitude: table_amp 2) on a shape of SHAPES"""
    if name in REFRESH_OWN:
        F = REFRESH_OWN[name]
        f, params = tc.refresh_field(oracle, 16, F)
        kw = dict(tc.REFRESH_FIELD, n_levels=32 // F, n_features=F, occ_res=16)
    else:
        kw = dict(train_kw(name), table_amp=2.0)
        t, m, o = synthetic(oracle, kw, util.SEED_A)
        o = np.zeros_like(o)
        o[0] = 1
        params = (t, m, o)
        f = oracle.OracleField(oracle.desc(**kw), params=params)
    thresh = tc.place_threshold(tc.cell_sigma(oracle, f))
    f.close()
    return kw, params, thresh


def refresh_opts(thresh):
    return dict(n_rays=32, n_samples=8, occ_every=0, occ_sigma_thresh=thresh)


def member_seeds(e):
    return util.SEED_A + 16 * e, 900 + e  # field, trainer


# ------------------------------------------------------------------ what a consumer needs beside the slot, per context
def render_views(oracle):
    return util.hemisphere_transforms(oracle, util.fibonacci_hemisphere(N_VIEWS))


def oracle_cameras(oracle):
    tms, scale, offset = render_views(oracle)
    return oracle.cameras_from_transforms(tms, util.FOV_X, W, H, scale, offset)


def positions():
    rng = np.random.default_rng(0x9E9)
    pos = np.concatenate([rng.random((512, 3), dtype=np.float32), instances.cube_positions()])
    d = rng.standard_normal((len(pos), 3)).astype(np.float32)
    return pos, d / np.linalg.norm(d, axis=1, keepdims=True)


class Rig:
    """the cameras, reference images and points of the consumers, on one context"""

    def __init__(self, ctx, oracle):
        from nerf_prv_amd import api

        self.api, self.ctx = api, ctx
        tms, scale, offset = render_views(oracle)
        self.cams = ctx.cameras_from_matrices(tms, util.FOV_X, W, H, scale, offset)
        rng = np.random.default_rng(0x67)
        gt = rng.random((N_VIEWS, H, W, 4), dtype=np.float32)
        gt[..., :3] *= gt[..., 3:]
        self.gt = ctx.torch.from_numpy(gt).to(ctx.device).contiguous()
        self.pos, self.dirs = positions()
        g = (np.arange(16, dtype=np.float32) + 0.5) / 16
        z, y, x = np.meshgrid(g, g, g, indexing="ij")
        self.voxels = ctx.torch.from_numpy(np.stack([x.ravel(), y.ravel(), z.ravel()], 1)).to(ctx.device).contiguous()
        eye, centre = np.array([0.5 + 1.2, 0.5 - 0.6, 0.5 + 0.7]), np.array([0.5, 0.5, 0.5])  # tests/test_gpu_parity.py's precept camera
        zc = (centre - eye) / np.linalg.norm(centre - eye)
        xc = np.cross(zc, [0.1, 0.2, 1.0])
        xc /= np.linalg.norm(xc)
        self.c2w = np.eye(4)
        self.c2w[:3, 0], self.c2w[:3, 1], self.c2w[:3, 2], self.c2w[:3, 3] = xc, np.cross(zc, xc), zc, eye
        self.rs2 = api.L.Rs2Intrinsics(width=1280, height=720, ppx=647.14532470703125, ppy=372.51531982421875, fx=915.60668945312500,
                                       fy=913.32666015625000, model=2)
        for i, v in enumerate([1.2042199820280075e-01, -2.1373499929904938e-01, 5.3860000334680080e-03, -2.1210000850260258e-03, 0.0]):
            self.rs2.coeffs[i] = v

    def opts(self, rule, spp=1):
        if rule == "ngp":
            return self.api.engine_render_opts(W, H, 0, spp, MIN_T)
        return self.api.render_opts(W, H, FIXED_S, spp, MIN_T)

    def close(self):
        self.cams.close()


def _np(t):
    return t.cpu().numpy()


def _stats(st):
    return np.array([st.samples_live, st.samples_evaluated], np.uint64)


def _render(method, names):
    """a prv_render* wrapper of api.Context -> consumer(rule, spp)"""
    def make(rule, spp=1, **kw):
        def run(ctx, rig, slot):
            *planes, st = getattr(ctx, method)(slot, rig.cams, None, rig.opts(rule, spp), **kw)
            out = {n: _np(p) for n, p in zip(names, planes)}
            out["stats"] = _stats(st)
            return out
        return run
    return make


_colour = _render("render", ["rgba"])
_rgba8 = _render("render_rgba8", ["rgba8"])
_depth = _render("render_depth", ["rgba", "depth"])
_entropy = _render("render_entropy", ["entropy", "alpha"])
_footprint = _render("render_footprint", ["entropy", "alpha", "depth"])
_surface = _render("render_surface", ["entropy", "alpha", "depth", "hit"])
_termination = _render("render_termination", ["bins", "alpha"])


def _score(method, rule, spp=1):
    def run(ctx, rig, slots):
        one = method in (5, 7)
        rec, st = ctx.score_views(method, [slots[0]] if one else list(slots), rig.cams, None, rig.opts(rule, spp), gt=rig.gt if method == 5 else None,
                                  want_stats=True)
        return {"records": rec, "stats": _stats(st)}
    return run


def _single(run):
    return lambda ctx, rig, slot: run(ctx, rig, [slot])


def _evaluate(ctx, rig, slot):
    return {"psnr_ssim": np.array(ctx.evaluate(slot, rig.cams, None, rig.opts("fixed"), rig.gt), np.float64)}


def _select(locator):
    def run(ctx, rig, slot):
        chosen, gains, st = ctx.select_views(slot, rig.cams, None, rig.opts("ngp"), rig.api.select_opts(k=3, grid_res=32), want_stats=True, locator=locator)
        return {"chosen": chosen, "gains": gains, "stats": _stats(st)}
    return run


def _density_grid(ctx, rig, slot):
    return {"sigma": _np(ctx.density_grid(slot, GRID)), "sigma_occupied": _np(ctx.density_grid(slot, GRID, use_occupancy=True))}


def _marching_cubes(use_occupancy):
    def run(ctx, rig, slot):
        m = ctx.marching_cubes(slot, GRID, use_occupancy=use_occupancy, colors=True)
        out = {"vertices": m.vertices, "normals": m.normals, "colors": m.colors, "triangles": m.triangles}
        m.close()
        return out
    return run


def _debug_field(ctx, rig, slot):
    out, occ = ctx.debug_field(slot, rig.pos, rig.dirs)
    return {"field": out, "occupied": occ}


def _export(ctx, rig, slot):
    t, m, o = ctx.export_model(slot, ctx.model_desc(slot))
    return {"table": t, "mlp": m, "occ": o}


def _layout(ctx, rig, slot):
    lay = ctx.model_layout(slot)
    return {"layout": np.array([lay[k] for k in sorted(lay)], np.int64)}


class Consumer:
    """run(ctx, rig, slot) -> dict of arrays (members: slot is the list of the ensemble's slots); method: the api.Context method it drives;
    reads: the canonical arrays that can reach its output"""

    def __init__(self, method, run, reads="tmo", members=False):
        self.method, self.run, self.reads, self.members = method, run, set(reads), members


CONSUMERS = {
    "render_fixed": Consumer("render", _colour("fixed")),
    "render_ngp": Consumer("render", _colour("ngp")),
    "render_fixed_spp4": Consumer("render", _colour("fixed", 4)),
    "render_ngp_spp4": Consumer("render", _colour("ngp", 4)),
    "render_rgba8_fixed": Consumer("render_rgba8", _rgba8("fixed")),
    "render_rgba8_ngp": Consumer("render_rgba8", _rgba8("ngp")),
    "depth_fixed": Consumer("render_depth", _depth("fixed")),
    "depth_ngp": Consumer("render_depth", _depth("ngp")),
    "depth_ngp_spp4": Consumer("render_depth", _depth("ngp", 4)),
    "entropy_fixed": Consumer("render_entropy", _entropy("fixed")),
    "entropy_ngp": Consumer("render_entropy", _entropy("ngp")),
    "footprint_fixed": Consumer("render_footprint", _footprint("fixed")),
    "footprint_ngp": Consumer("render_footprint", _footprint("ngp")),
    "surface_fixed": Consumer("render_surface", _surface("fixed")),
    "surface_ngp": Consumer("render_surface", _surface("ngp")),
    "termination_fixed": Consumer("render_termination", _termination("fixed")),
    "termination_ngp": Consumer("render_termination", _termination("ngp")),
    "score5_fixed": Consumer("score_views", _single(_score(5, "fixed"))),
    "score5_ngp": Consumer("score_views", _single(_score(5, "ngp"))),
    "score7_fixed": Consumer("score_views", _single(_score(7, "fixed"))),
    "score7_ngp": Consumer("score_views", _single(_score(7, "ngp"))),
    "evaluate": Consumer("evaluate", _evaluate),
    "select_expected": Consumer("select_views", _select("expected")),
    "select_surface": Consumer("select_views", _select("surface")),
    "density_grid": Consumer("density_grid", _density_grid),
    "marching_cubes": Consumer("marching_cubes", _marching_cubes(False), reads="tm"),
    "marching_cubes_occupancy": Consumer("marching_cubes", _marching_cubes(True)),
    "debug_encode": Consumer("debug_encode", lambda ctx, rig, slot: {"features": ctx.debug_encode(slot, rig.pos)}, reads="t"),
    "debug_field": Consumer("debug_field", _debug_field),
    "first_hit": Consumer("first_hit", lambda ctx, rig, slot: {"cells": _np(ctx.first_hit(slot, rig.cams, None, W, H))}, reads="o"),
    "precept": Consumer("precept", lambda ctx, rig, slot: {"cells": _np(ctx.precept(slot, rig.voxels, rig.c2w, rig.rs2, max_range=3.0))}, reads="o"),
    "export_model": Consumer("export_model", _export),
    "model_layout": Consumer("model_layout", _layout, reads=""),  # the descriptor alone: it moves with reinstall_other_shape only
    # the ensemble's: every member's image enters the record
    "score2_ngp": Consumer("score_views", _score(2, "ngp"), members=True),
    "score3_ngp": Consumer("score_views", _score(3, "ngp"), members=True),
    "score3_ngp_spp4": Consumer("score_views", _score(3, "ngp", 4), members=True),
    "score2_fixed": Consumer("score_views", _score(2, "fixed"), members=True),
    "score9_ngp": Consumer("score_views", _score(9, "ngp"), members=True),
    "score9_fixed": Consumer("score_views", _score(9, "fixed"), members=True),
}
SINGLE = [k for k, c in CONSUMERS.items() if not c.members]
MEMBERS = [k for k, c in CONSUMERS.items() if c.members]

def dirty_order(names):
    return sorted(names, key=lambda k: (CONSUMERS[k].reads != {"o"}, names.index(k)))


# what each change writes: table, mlp, occupancy ("d": the descriptor)
CHANGED = {"steps_shrink": "tmo", "steps_shrink_ngp": "tmo", "refresh_grow": "o", "reinstall_same_shape": "tmo", "reinstall_other_shape": "tmod", "round": "tmo",
           "members": "tmo"}

# api.Context methods that take a slot and are no consumer of its derived state, each with its reason
EXEMPT = {
    "load_model": "installs a slot: it is reinstall_same_shape / reinstall_other_shape, the change itself",
    "synthetic_model": "installs a slot through the same install_model as load_model, from arrays made on the host",
    "fresh_model": "installs a slot through the same install_model as load_model, from arrays made on the host",
    "load_model_file": "reads a file, then load_model's path (tests/test_gpu_parity.py round-trips it)",
    "load_ingp": "reads a snapshot, then load_model's path (tests/test_gpu_ingp.py)",
    "save_model": "writes the canonical arrays that export_model returns, which is in the table",
    "save_ingp": "writes the canonical arrays that export_model returns, which is in the table",
    "model_desc": "returns the descriptor stored at install; no derived state, and every export_model consumer here calls it",
}
# (slot_methods finds a method by a parameter named slot / slots, the wrappers' convention, and by the slot-taking function of
# include/prv.h that its source calls, which holds whatever the wrapper names its arguments)


def slot_functions():
    """the functions of include/prv.h with a model slot among their parameters (`int slot`, `int model_slot`, `const int* model_slots`,
    `const int* slots`): the C header names its slots, whatever a Python wrapper calls its arguments"""
    import os
    import re

    with open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "prv.h")) as f:
        text = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    return sorted(name for name, params in re.findall(r"\b(prv_\w+)\s*\(([^;{]*?)\)\s*;", text, flags=re.S)
                  if re.search(r"\bint\s+(model_)?slot\b|\bconst\s+int\s*\*\s*(model_)?slots\b", params))


def slot_methods(cls):
    """the public methods of cls that take a model slot: a parameter named slot or slots, or a call of one of slot_functions() in the
    method's source (a wrapper that names its slot argument otherwise is found by the C function it drives)"""
    import inspect
    import re

    fns = slot_functions()
    out = []
    for name, fn in inspect.getmembers(cls, inspect.isfunction):
        if name.startswith("_"):
            continue
        calls = set(re.findall(r"\blib\.(prv_\w+)\(", inspect.getsource(fn)))
        if {"slot", "slots"} & set(inspect.signature(fn).parameters) or calls & set(fns):
            out.append(name)
    return sorted(out)


def same_bytes(a, b):
    """names of the arrays of two consumer outputs that differ in shape, type or bytes"""
    bad = [k for k in a if k not in b or a[k].shape != b[k].shape or a[k].dtype != b[k].dtype or a[k].tobytes() != b[k].tobytes()]
    return bad + [k for k in b if k not in a]
