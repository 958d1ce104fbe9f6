"""Ray populations for the cell-ordered drain of the queue (PRV_REGION_CELLS), beside those of tests/queue_cases.py: used by
tests/test_gpu_region_cells.py (GPU) and tests/test_queue_order_host.py (what each one forces, without a GPU)."""
import numpy as np

from tests import queue_cases as qc, util


def one_ray_per_wave():
    """qc.counts' far view down z, 32 x 32 pixels on the 32 x 32 cell columns: one occupied cell in the middle of every 8 x 8 pixel
    patch -- a march wave is one such patch, so every wave of the launch holds exactly one live ray"""
    base = qc.counts(1)
    occ = np.zeros((qc.R, qc.R, qc.R), bool)
    for y in range(4, 32, 8):
        for x in range(4, 32, 8):
            occ[16, y, x] = True
    return qc.Case("one_ray_per_wave", occ, qc.DEFAULT, base.tms, base.fov, 32, 32)


def with_a_blind_view():
    """octant_low and one more camera that looks away from the box: a whole view of the batch without a live ray"""
    base = qc.get("octant_low")
    away = qc.camera_matrix([0.5, 0.5, 3.0], [0.5, 0.5, 9.0], up=(0.0, 1.0, 0.0))
    return qc.Case("blind_view", base.occ, base.regime, list(base.tms[:2]) + [away] + list(base.tms[2:4]), base.fov, base.w, base.h)


ONE_CELL_BLOCK = 5  # the occupied grid cell [5, 6)^3


def one_cell():
    """every descriptor of a populated octant in ONE cell, at 2, 4 and 8 cells per axis: a single occupied grid cell [5, 6)^3 and a
    far cell [18, 19)^3 that stretches the one-cell-grown box to [4, 20) / 32 (middle 12).  Octant 0 is [4, 12) / 32; its cells are
    4, 2 and 1 grid cells wide and the block is cell 0, 0 and 1 of them on every axis (all the figures are exact in binary32).  The
    views look at the block from close by and from directions in which the far cell is not behind it, so the middle of the live
    span of a ray that sees the block lies inside the block: hundreds of blocks of records, one key"""
    b = ONE_CELL_BLOCK
    occ = qc._cells(((b, b + 1),) * 3, ((18, 19),) * 3)
    lo, hi = 4.0, 20.0  # the one-cell-grown box, in grid cells
    for cells in (2, 4, 8):
        width = 0.5 * (hi - lo) / cells
        assert int((b - lo) / width) == int((b + 1 - 1e-6 - lo) / width), cells  # both faces of the block in the same cell
    centre = np.full(3, (b + 0.5) / qc.R)
    tms = [qc.camera_matrix(e, centre) for e in qc._around(centre, 0.075, 8)]
    return qc.Case("one_cell", occ, qc.TRANSPARENT, tms, util.FOV_X, 128, 96)
