"""PRV_REGION_CELLS: the render launch drains every octant region of the ray queue cell by cell (prv_queue_order.hpp: a
descriptor per march wave, a counting sort between march and render, one cursor per octant region).  The order in which records
are rendered changes no pixel and no count: everything here is np.array_equal / == between a context with PRV_REGION_CELLS=1
(the order of arrival, no descriptors) and contexts with 2, 4 and 8 cells per axis.  A descriptor the sort lost shows as pixels
that stay zero and a smaller evaluated count, one it doubled as a larger evaluated count.

  * F4_5 with its three replicas, F2_10 and the generic F4_0, both stepping rules, 44x36 and 20x16, spp 1 and 3 (3: sub-samples
    on grid.z), colour + RGBA8 + the march and evaluated counts;
  * a plane mode (the footprint launch) on F4_5;
  * a five-member method-3 round through march_multi_kernel (lane e reserves member e's descriptor);
  * the adversarial populations of tests/queue_cases.py under the default policy (the corner-cache instance under the engine's
    rule): an octant region that overflows (tail cut, waves that move on), one counter that takes every ray, every ray ending at
    its first sample, exact small counts, one live ray per wave, and a view that does not see the box at all."""
import numpy as np
import pytest

from nerf_prv_amd import api
from tests import instances, queue_cases as qc, region_cases, util
from tests.test_gpu_instances import environment

pytestmark = pytest.mark.gpu

CELLS = (1, 2, 4, 8)
PLAIN = {"PRV_CELL_CACHE": "0"}  # small images under the engine's rule: the replica / plain instances, not the corner cache
SHAPES = ("F4_5", "F2_10", "F4_0")
SIZES = ((44, 36), (20, 16))
MIN_T = 1e-4


def _contexts(env):
    out = {}
    for n in CELLS:
        with environment(dict(env, PRV_REGION_CELLS=str(n))):
            out[n] = api.Context(0)
    return out


@pytest.fixture(scope="module")
def plain():
    cs = _contexts(PLAIN)
    for c in cs.values():
        for slot, shape in enumerate(SHAPES):
            c.synthetic_model(slot, api.field_desc(**instances.MATRIX[shape].kw), util.SEED_A)
            instances.assert_layout(c.model_layout(slot), instances.MATRIX[shape])
        assert api.replica_layout(c, 0)[0] == 3
    yield cs
    for c in cs.values():
        c.close()


@pytest.fixture(scope="module")
def default_policy():
    cs = _contexts({})
    yield cs
    for c in cs.values():
        c.close()


@pytest.fixture(scope="module")
def views(oracle):
    tms, scale, offset = util.hemisphere_transforms(oracle, util.fibonacci_hemisphere(6))
    return tms[[0, 2, 3, 5]], scale, offset


def _rules(w, h, spp):
    return (("fixed_s", api.render_opts(w, h, 128, spp, MIN_T)), ("ngp", api.engine_render_opts(w, h, 0, spp, MIN_T)))


def _colour(c, slot, views, w, h, spp):
    tms, scale, offset = views
    cams = c.cameras_from_matrices(tms, util.FOV_X, w, h, scale, offset)
    out = {}
    for rule, opts in _rules(w, h, spp):
        img, st = c.render(slot, cams, None, opts)
        u8, st8 = c.render_rgba8(slot, cams, None, opts)
        out[rule] = (img.cpu().numpy().tobytes(), u8.cpu().numpy().tobytes(), int(st.samples_live), int(st.samples_evaluated), int(st8.samples_evaluated))
    cams.close()
    return out


def _assert_same(want, got, tag):
    for rule in want:
        assert got[rule][2:] == want[rule][2:], (tag, rule, "counts", want[rule][2:], got[rule][2:])
        assert want[rule][3] > 0, (tag, rule)
        assert got[rule][0] == want[rule][0], (tag, rule, "float pixels differ")
        assert got[rule][1] == want[rule][1], (tag, rule, "bytes differ")


# F4_5 (the replica instances) at both sizes and both spp; the other instances share the queue code: one size each
COLOUR_RUNS = [("F4_5", size, spp) for size in SIZES for spp in (1, 3)] + [("F2_10", SIZES[0], 1), ("F4_0", SIZES[0], 1)]


@pytest.mark.parametrize("shape,size,spp", COLOUR_RUNS, ids=lambda v: v if isinstance(v, str) else f"{v[0]}x{v[1]}" if isinstance(v, tuple) else f"spp{v}")
def test_colour_and_counts_do_not_depend_on_the_cells(plain, views, shape, size, spp):
    slot = SHAPES.index(shape)
    want = _colour(plain[1], slot, views, *size, spp)
    for n in CELLS[1:]:
        _assert_same(want, _colour(plain[n], slot, views, *size, spp), (shape, size, spp, n))


def test_footprint_planes_do_not_depend_on_the_cells(plain, views):
    tms, scale, offset = views
    w, h = SIZES[0]
    outs = {}
    for n, c in plain.items():
        cams = c.cameras_from_matrices(tms, util.FOV_X, w, h, scale, offset)
        outs[n] = {}
        for rule, opts in _rules(w, h, 1):
            ent, alpha, depth, st = c.render_footprint(0, cams, None, opts)
            outs[n][rule] = ([t.cpu().numpy().tobytes() for t in (ent, alpha, depth)], int(st.samples_live), int(st.samples_evaluated))
        cams.close()
    for n in CELLS[1:]:
        for rule in outs[1]:
            assert outs[n][rule][1:] == outs[1][rule][1:] and outs[1][rule][2] > 0, (n, rule)
            assert outs[n][rule][0] == outs[1][rule][0], (n, rule)


def test_method3_round_of_five_members_through_march_multi(views):
    """the ensemble's one march launch: five members' descriptors from one wave instruction, five ordering launches"""
    tms, scale, offset = views
    w, h = SIZES[0]
    got = {}
    for n in CELLS:
        with environment({"PRV_REGION_CELLS": str(n), "PRV_MARCH_MULTI": "1"}):
            c = api.Context(0)
        try:
            for e in range(5):
                c.synthetic_model(e, api.field_desc(**instances.MATRIX["F4_5"].kw), 4242 + e)
            cams = c.cameras_from_matrices(tms, util.FOV_X, w, h, scale, offset)
            rec, st = c.score_views(3, list(range(5)), cams, None, api.engine_render_opts(w, h, 0, 1, 0.01, background=(0, 0, 0, 1)), want_stats=True)
            got[n] = (rec.tobytes(), int(st.samples_live), int(st.samples_evaluated))
            cams.close()
        finally:
            c.close()
    assert got[1][1] > 0 and got[1][2] > 0
    for n in CELLS[1:]:
        assert got[n] == got[1], n


# ---- adversarial populations
ADVERSARIAL = {"octant_high": lambda: qc.get("octant_high"), "one_subregion": lambda: qc.get("one_subregion"), "opaque": lambda: qc.get("opaque"),
               "counts0": lambda: qc.get("counts0"), "counts1": lambda: qc.get("counts1"), "counts65": lambda: qc.get("counts65"),
               "one_ray_per_wave": region_cases.one_ray_per_wave, "blind_view": region_cases.with_a_blind_view,
               "one_cell": region_cases.one_cell}


@pytest.mark.parametrize("mode", [qc.FIXED, qc.NGP], ids=["S128", "ngp"])
@pytest.mark.parametrize("name", list(ADVERSARIAL))
def test_adversarial_populations_drain_completely(default_policy, oracle, name, mode):
    case = ADVERSARIAL[name]()
    got = {}
    for n, c in default_policy.items():
        case.load(c, oracle, 0, instances.MATRIX["F4_5"].kw).close()
        cs = case.cams(c)
        img, st = c.render(0, cs, None, case.opts(mode))
        cs.close()
        got[n] = (img.cpu().numpy(), int(st.samples_live), int(st.samples_evaluated))
    img, live, n_eval = got[1]
    if name == "one_ray_per_wave":
        assert int((img[0, ..., 3] > 0).sum()) == 16 and all((img[0, y:y + 8, x:x + 8, 3] > 0).sum() == 1 for y in range(0, 32, 8) for x in range(0, 32, 8))
    if name == "blind_view":
        assert not img[2].any() and img[1].any() and img[3].any()
    assert (live > 0) == (name != "counts0")
    for n in CELLS[1:]:
        assert got[n][1:] == (live, n_eval), (name, n, got[n][1:], (live, n_eval))
        assert np.array_equal(got[n][0].view(np.uint32), img.view(np.uint32)), (name, n)
