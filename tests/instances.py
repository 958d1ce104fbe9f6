"""The field matrix of the instance tests (test infrastructure): one small field per compiled (F, NDENSE) instance of the
field-evaluating kernels and one per reason for falling back to the generic instance <F, 0>, each with the layout it must
produce (prv_model_layout: kernel_dense_levels, n_dense_levels, n_hashed_levels).

The expectations are written down, not computed: `restated_layout` below restates compute_levels (prv_levels.hpp) and the
physical-layout rules of plan_field (prv_field_plan.hpp) in Python so that the table can be checked without a GPU
(tests/test_instances_host.py), and the C++ rules against the restatement (tests/test_field_plan_host.py); on the GPU every test
asserts the context's own answer against the table first, so a shape that does not select its instance fails loudly instead
of running on <F, 0> unnoticed.

    id                    dense / hashed   instance   why
    F4_5, F4_3            5 / 3, 3 / 5     5, 3       SMALL with a larger / smaller table
    F4_0                  4 / 4            0          SMALL itself: no instance for four dense levels
    F2_10, F2_6           10 / 6, 6 / 10   10, 6      SMALL_F2 with a larger / smaller table
    F2_0                  9 / 7            0          SMALL_F2 itself: no instance for nine dense levels
    F4_all_hashed         0 / 8            0          2 KiB hashed tables: level offsets not 4 KiB aligned, no dense level
    F4_finer_than_table   1 / 7            0          hashed levels with more vertices per axis than table entries
    F2_all_dense          16 / 0           0          no hashed level
    F4_wide               7 / 1            0, wide    one 32 MiB hashed level: 32-bit offsets (FieldDev::wide_offsets)
    FIELD_256, FIELD_512  5 / 3, 10 / 6    5, 10      the product's fields
"""
import math

import numpy as np

from nerf_prv_amd import api
from tests import util


class Entry:
    def __init__(self, kw, n_dense, n_hashed, instance, wide=False):
        self.kw, self.n_dense, self.n_hashed, self.instance, self.wide = dict(kw), n_dense, n_hashed, instance, wide

    @property
    def F(self):
        return self.kw["n_features"]


MATRIX = {
    "F4_5": Entry(dict(util.SMALL, log2_hashmap=16), 5, 3, 5),
    "F4_3": Entry(dict(util.SMALL, log2_hashmap=13), 3, 5, 3),
    "F4_0": Entry(util.SMALL, 4, 4, 0),
    "F2_10": Entry(dict(util.SMALL_F2, log2_hashmap=14), 10, 6, 10),
    "F2_6": Entry(dict(util.SMALL_F2, log2_hashmap=11), 6, 10, 6),
    "F2_0": Entry(util.SMALL_F2, 9, 7, 0),
    "F4_all_hashed": Entry(dict(util.SMALL, log2_hashmap=8), 0, 8, 0),
    "F4_finer_than_table": Entry(dict(n_levels=8, n_features=4, log2_hashmap=6, base_res=4, finest_res=96, occ_res=32), 1, 7, 0),
    "F2_all_dense": Entry(dict(util.SMALL_F2, log2_hashmap=19), 16, 0, 0),
    "F4_wide": Entry(dict(n_levels=8, n_features=4, log2_hashmap=22, base_res=8, finest_res=200, occ_res=32), 7, 1, 0, wide=True),
}
PRODUCT = {
    "FIELD_256": Entry(api.FIELD_256, 5, 3, 5),
    "FIELD_512": Entry(api.FIELD_512, 10, 6, 10),
}
FAST = [k for k, e in MATRIX.items() if e.instance != 0]  # the entries with a generic twin under PRV_NO_PAIR=1
ALL_INSTANCES = {(4, 5), (4, 3), (4, 0), (2, 10), (2, 6), (2, 0)}


def is_wide(kw):
    """plan_field's rule (prv_field_plan.hpp): a hashed level whose last byte offset does not fit 24 bits takes the 32-bit multiply path"""
    return restated_layout(kw)["n_hashed_levels"] >= 1 and ((1 << kw["log2_hashmap"]) - 1) * 2 * kw["n_features"] >= 1 << 24


def assert_layout(layout, entry, no_pair=False):
    """layout: Context.model_layout(slot).  Under PRV_NO_PAIR=1 every level goes through the generic gather: the context
    reports no dense level at all."""
    assert layout["kernel_features"] == entry.F
    assert layout["n_hashed_levels"] == entry.n_hashed
    if no_pair:
        assert layout["kernel_dense_levels"] == 0 and layout["n_dense_levels"] == 0
    else:
        assert layout["kernel_dense_levels"] == entry.instance, layout
        assert layout["n_dense_levels"] == entry.n_dense, layout
    assert is_wide(entry.kw) == entry.wide
    assert layout["table_bytes_physical"] == restated_layout(entry.kw)["table_bytes_physical"]  # (the same with and without PRV_NO_PAIR)


def restated_levels(kw):
    """compute_levels of prv_levels.hpp -> [(scale, res, hashed, entries)]"""
    n, T = kw["n_levels"], 1 << kw["log2_hashmap"]
    pls = np.float32(kw.get("per_level_scale", 0.0))
    growth = math.exp((math.log(kw["finest_res"]) - math.log(kw["base_res"])) / (n - 1)) if n > 1 else 1.0
    out = []
    for l in range(n):
        if pls > 0:
            s = np.float32(np.exp2(np.float32(l) * np.log2(pls))) * np.float32(kw["base_res"]) - np.float32(1.0)
        else:
            s = kw["base_res"] * growth ** l - 1.0
            if abs(s - math.floor(s + 0.5)) < 1e-9:
                s = math.floor(s + 0.5)
            s = np.float32(s)
        res = int(math.ceil(float(s))) + 1
        hashed = res ** 3 > T
        out.append((s, res, hashed, T if hashed else (res ** 3 + 7) & ~7))
    return out


def restated_layout(kw):
    """the instance plan_field + instance_dense_levels (prv_field_plan.hpp) pick for a descriptor, restated: power-of-two strides and
    sizes for the dense levels, levels placed largest first, the shared-hash conditions, the instance table"""
    lv = restated_levels(kw)
    F = kw["n_features"]
    ebytes = 2 * F
    ceil_log2 = lambda v: max(0, (v - 1).bit_length())
    sx = [0 if h else ceil_log2(res + 1) for _, res, h, _ in lv]
    psize = [size if h else 1 << ceil_log2((res + 1) << (2 * sx[i])) for i, (_, res, h, size) in enumerate(lv)]
    off, total = {}, 0
    for i in sorted(range(len(lv)), key=lambda i: -psize[i]):  # stable, like std::stable_sort
        off[i], total = total, total + psize[i]
    n_dense = 0
    while n_dense < len(lv) and not lv[n_dense][2]:
        n_dense += 1
    shared, wide = True, False
    for i, (_, res, hashed, size) in enumerate(lv):
        if hashed:
            if res > size or i < n_dense:
                shared = False
            if (size - 1) * ebytes >= 1 << 24:
                wide, shared = True, False
            if (off[i] * ebytes) & 4095 or res - 1 > 4095:
                shared = False
        elif (off[i] * ebytes) & 31 or sx[i] > 31:
            shared = False
    if not shared:
        inst = 0
    elif F == 4:
        inst = n_dense if n_dense in (5, 3) else 0
    else:
        inst = n_dense if n_dense in (10, 6) else 0
    return dict(kernel_dense_levels=inst, n_dense_levels=n_dense, n_hashed_levels=sum(1 for x in lv if x[2]), hash_shared=shared,
                wide_offsets=wide, table_bytes_physical=total * ebytes)


def boundary_positions(kw, rng, per_level=4):
    """positions exactly on cell boundaries of every level.  A level's cell index is floor(fma(scale, p, 0.5)): its cells
    change at p = (k - 0.5) / scale, and p = k / scale is the middle of a cell.  For a few vertices k of level l (the first
    cells, the last cell, random ones) the fp32 values k / scale_l and (k +- 0.5) / scale_l and the two fp32 neighbours of
    each, on one, two or three axes at once (the other axes random).  The last cell is where the paired layout's duplicated
    border and the generic path's min(c + 1, res - 1) clamp must agree."""
    out = []
    for s, res, _, _ in restated_levels(kw):
        s = float(s)
        ks = {0, 1, res - 2, res - 1} | set(int(k) for k in rng.integers(0, res, per_level))
        for k in sorted(k for k in ks if 0 <= k < res):
            for exact in (k / s, (k - 0.5) / s, (k + 0.5) / s):
                x = np.float32(min(max(exact, 0.0), 1.0))
                for v in (np.nextafter(x, np.float32(-1)), x, np.nextafter(x, np.float32(2))):
                    if not 0.0 <= v <= 1.0:
                        continue
                    for axes in ((0,), (1,), (2,), (0, 1), (0, 1, 2)):
                        p = rng.random(3, dtype=np.float32)
                        p[list(axes)] = v
                        out.append(p)
    return np.array(out, np.float32)


def cube_positions(n=7):
    """the cube's 8 corners, and points on its 6 faces, 12 edges: every position with a coordinate in {0, 1}"""
    g = np.linspace(0.0, 1.0, n, dtype=np.float32)
    x, y, z = np.meshgrid(g, g, g, indexing="ij")
    p = np.stack([x.ravel(), y.ravel(), z.ravel()], 1)
    on_surface = ((p == 0) | (p == 1)).any(axis=1)
    return np.ascontiguousarray(p[on_surface])
