"""Mesh extraction timings (dev tool, not bench.py): per-stage milliseconds of prv_marching_cubes -- density grid,
classify + scans, emit, colours (HIP events inside the call) -- and grid points per second of the density pass, at res 256
and 512 on the BASELINE.md section 6 scene (FIELD_256, table U(-0.1, 0.1), no density bias) and the 512^3 field.

    python scripts/meshbench.py [--reps 5] [--res 256 512] [--json out.json]

Each configuration runs at the iso-level 2.5 (run.py's default) and at the grid's median (a large surface).  The density
grid is timed with the default row waves (64 consecutive points) and with 4x4x4-brick waves (PRV_MESH_BRICK=1)."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--res", type=int, nargs="+", default=[256, 512])
ap.add_argument("--json", default="")
args = ap.parse_args()

from nerf_prv_amd import api

ctx = api.Context(0)
scenes = {"baseline": dict(api.FIELD_256, table_amp=0.1, density_bias=0.0), "field512": dict(api.FIELD_512)}
rows = []
for si, (name, fd) in enumerate(scenes.items()):
    ctx.synthetic_model(si, api.L.FieldDesc(**fd), 0x5EED0001)
    for res in args.res:
        med = float(np.median(ctx.density_grid(si, res).cpu().numpy()))
        for thr_name, thr in (("2.5", 2.5), ("median", med)):
            for brick in ("0", "1"):
                os.environ["PRV_MESH_BRICK"] = brick
                stages, counts = [], None
                for r in range(args.reps + 1):  # the first is a warm-up
                    m = ctx.marching_cubes(si, res, threshold=thr)
                    counts = m.counts()
                    m.close()
                    if r:
                        stages.append(ctx.mesh_stage_ms())
                best = {k: min(s[k] for s in stages) for k in stages[0]}
                med_ms = {k: float(np.median([s[k] for s in stages])) for k in stages[0]}
                row = dict(scene=name, res=res, threshold=thr_name, threshold_value=thr, brick=int(brick), vertices=counts[0],
                           triangles=counts[1], stage_ms_median=med_ms, stage_ms_best=best,
                           grid_points_per_s=res ** 3 / (med_ms["grid"] * 1e-3) if med_ms["grid"] > 0 else None)
                rows.append(row)
                print(json.dumps(row), flush=True)
os.environ.pop("PRV_MESH_BRICK", None)
if args.json:
    with open(args.json, "w") as fh:
        json.dump(rows, fh, indent=1)
ctx.close()
