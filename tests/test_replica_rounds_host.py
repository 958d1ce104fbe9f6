"""The inputs of tests/test_gpu_replica_rounds.py's table case, checked without a GPU: the table holds no two equal halfs within a
window, the vertex positions are vertices (the oracle returns the entries themselves there), they reach what they claim, and a
copy that reads a neighbouring entry is seen at every one of them."""
import numpy as np
import pytest

from tests import test_gpu_replica_rounds as rr

KW = rr.F4_5.kw


@pytest.fixture(scope="module")
def queries():
    return rr.VertexQueries(KW)


def test_table_is_injective_within_a_window_and_finite():
    table = rr.injective_table(KW).reshape(-1, KW["n_features"])
    assert np.all((table >> 10) & 31 != 31) and np.all(table & 0x7FFF != 0)  # no NaN, no infinity, neither zero
    for _, _, hashed, n, first in rr.level_offsets(KW):
        level = table[first:first + n]
        for lo in range(0, n, rr.WINDOW):
            for k in range(KW["n_features"]):
                w = level[lo:lo + rr.WINDOW, k]
                assert len(np.unique(w)) == len(w), (first, lo, k)
        assert np.all(level[:, 0] != level[:, 1]) and np.all(level[:, 2] != level[:, 3]) and np.all(level[:, 0] != level[:, 2])
        if hashed:  # what a copy of entry i ^ 1, i + 1 or i - 1 would hold differs in every feature
            for other in (np.arange(n) ^ 1, (np.arange(n) + 1) % n, (np.arange(n) - 1) % n):
                assert np.all(level != level[other])


def test_vertex_coordinates_are_exact():
    for s, res, hashed, _, _ in rr.level_offsets(KW):
        if not hashed:
            continue
        coords, last = rr.exact_vertex_coords(s)
        assert last in (res - 1, res - 2) and last in coords
        for k, p in coords.items():
            pos = float(np.float32(s)) * float(p) + 0.5  # (in double: within 2^-29 of the exact sum, far inside binary32's spacing)
            assert np.float32(pos) == k and 0.0 <= p <= 1.0


def test_positions_reach_half_of_every_replica(queries):
    queries.assert_reach()
    assert [L["level"] for L in queries.levels] == [5, 6, 7]
    assert 3000 <= len(queries.pos) - queries.n_vertex_and_border and len(queries.pos) < 120000


def test_oracle_returns_the_entries_and_sees_a_neighbouring_copy(oracle, queries):
    """at the vertex positions the oracle's features of a hashed level are the table's entries; with the hashed levels' entries
    swapped in pairs (what a replica filled from entry i ^ 1 holds) every one of those features changes, in all four halfs"""
    F = KW["n_features"]
    table, mlp, occ = rr.injective_model(oracle, KW)
    swapped = table.copy().reshape(-1, F)
    for _, _, hashed, n, first in rr.level_offsets(KW):
        if hashed:
            swapped[first:first + n] = swapped[first + (np.arange(n) ^ 1)]
    d = oracle.desc(**KW)
    outs = []
    for t in (table, swapped.reshape(-1)):
        f = oracle.OracleField(d, params=(t, mlp, occ))
        outs.append(np.concatenate([f.encode(queries.pos[L["start"]:L["start"] + L["n"]:7]) for L in queries.levels]))
        f.close()
    row = 0
    for L in queries.levels:
        n = len(range(0, L["n"], 7))
        cols = slice(L["level"] * F, (L["level"] + 1) * F)
        assert np.array_equal(outs[0][row:row + n, cols], queries.entries_expected(table, L)[::7])
        assert np.all(outs[0][row:row + n, cols] != outs[1][row:row + n, cols])
        row += n
