"""The field matrix of tests/instances.py without a GPU: the layout each entry is expected to produce equals what a Python
restatement of compute_levels (prv_levels.hpp) and of plan_field's physical-layout rules (prv_field_plan.hpp) gives, and the
restated level geometry is the oracle's.  (tests/test_field_plan_host.py holds the C++ rules against the restatement; on the GPU,
tests/test_gpu_instances.py asserts the context's own answer.)"""
import numpy as np
import pytest

from tests import instances, util

ENTRIES = {**instances.MATRIX, **instances.PRODUCT}


@pytest.mark.parametrize("name", list(ENTRIES))
def test_expected_layout_is_the_restated_one(oracle, name):
    e = ENTRIES[name]
    lay = instances.restated_layout(e.kw)
    assert (lay["kernel_dense_levels"], lay["n_dense_levels"], lay["n_hashed_levels"]) == (e.instance, e.n_dense, e.n_hashed)
    assert lay["wide_offsets"] == e.wide == instances.is_wide(e.kw)
    assert e.n_dense + e.n_hashed == e.kw["n_levels"] and e.kw["n_levels"] * e.F == 32
    lv, _ = oracle.levels(oracle.desc(**e.kw))
    mine = instances.restated_levels(e.kw)
    assert [(np.float32(a.scale), a.res, bool(a.hashed), a.size) for a in lv] == [(s, r, h, n) for s, r, h, n in mine]


def test_matrix_reaches_every_instance_and_the_usual_small_fields_only_the_generic_ones():
    assert {(e.F, e.instance) for e in instances.MATRIX.values()} == instances.ALL_INSTANCES
    assert instances.restated_layout(util.SMALL)["kernel_dense_levels"] == 0
    assert instances.restated_layout(util.SMALL_F2)["kernel_dense_levels"] == 0


def test_boundary_positions_sit_on_cell_boundaries():
    kw = instances.MATRIX["F4_5"].kw
    pos = instances.boundary_positions(kw, np.random.default_rng(0))
    assert pos.dtype == np.float32 and pos.min() >= 0.0 and pos.max() <= 1.0
    for s, res, _, _ in instances.restated_levels(kw):
        cell = np.floor(np.float32(s) * pos + np.float32(0.5))
        assert cell.max() >= res - 2  # the last cell of the level is visited
        frac = np.float64(s) * pos + 0.5
        assert (np.abs(frac - np.round(frac)) < 1e-5).any()  # and a position on (or one ulp off) a boundary
    cube = instances.cube_positions()
    assert len(cube) == 7 ** 3 - 5 ** 3 and ((cube == 0) | (cube == 1)).any(axis=1).all()
