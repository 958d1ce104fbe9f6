"""Geometric-evaluation timings (dev tool, not bench.py): index build, nearest-neighbour query (grid and brute force), surface
sampling and the end-to-end prv_geometry_metrics, at 2^20 x 2^20 points -- on samples of the FIELD_256 synthetic model's mesh and
on a clustered, adversarial set (95 % of the points in 0.1 % of the box volume).  Host clock around calls that end in a device
synchronise (every entry point here synchronises).  Also the distances each algorithm formed (prv_debug_nn_tests).

    python scripts/geombench.py [--reps 5] [--log2n 20] [--no-brute] [--json out.json]
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--log2n", type=int, default=20)
ap.add_argument("--no-brute", action="store_true")
ap.add_argument("--json", default="")
args = ap.parse_args()

import torch

from nerf_prv_amd import api

L = api.L
ctx = api.Context(0)
n = 1 << args.log2n


def timed(fn, reps=args.reps):
    out, ms = None, []
    for r in range(reps + 1):  # the first round is a warm-up
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        if r:
            ms.append((time.perf_counter() - t0) * 1e3)
    return out, float(np.median(ms)), float(min(ms))


def clustered(rng, k):
    a = 0.63 + 0.1 * rng.random((int(0.95 * k), 3))
    b = rng.random((k - len(a), 3))
    return torch.from_numpy(rng.permutation(np.concatenate([a, b]).astype(np.float32))).to(ctx.device)


ctx.synthetic_model(0, api.field_desc(**api.FIELD_256), 0x5EED0001)
thr = float(np.median(ctx.density_grid(0, 64).cpu().numpy()))
mesh = ctx.marching_cubes(0, 256, threshold=thr, colors=False)
rows = []
_, med, best = timed(lambda: mesh.sample(n, 1))
rows.append(dict(case="sample", n=n, triangles=int(len(mesh.triangles)), ms_median=med, ms_best=best))
print(json.dumps(rows[-1]), flush=True)
rng = np.random.default_rng(9)
sets = {"mesh": (mesh.sample(n, 1), mesh.sample(n, 2)), "clustered": (clustered(rng, n), clustered(rng, n))}
mesh.close()
for name, (q, p) in sets.items():
    row = dict(case=name, n=n)
    for label, algorithm in (("grid", L.NN_GRID), ("brute", L.NN_BRUTE)):
        if algorithm == L.NN_BRUTE and args.no_brute:
            continue
        idx, med, best = timed(lambda: ctx.nn_index(p, algorithm))
        row[label + "_build_ms"] = dict(median=med, best=best)
        _, med, best = timed(lambda: idx.query(q), reps=args.reps if algorithm == L.NN_GRID else min(args.reps, 2))
        row[label + "_query_ms"] = dict(median=med, best=best)
        row[label + "_tests"] = idx.tests()
        if algorithm == L.NN_GRID:
            row["grid"] = idx.info()
        idx.close()
    if "brute_query_ms" in row:
        row["grid_speedup_over_brute"] = row["brute_query_ms"]["median"] / row["grid_query_ms"]["median"]
        row["tests_ratio"] = row["brute_tests"] / max(1, row["grid_tests"])
    _, med, best = timed(lambda: ctx.geometry_metrics(q, p, 0.01))
    row["geometry_metrics_ms"] = dict(median=med, best=best)
    rows.append(row)
    print(json.dumps(row), flush=True)
if args.json:
    with open(args.json, "w") as fh:
        json.dump(rows, fh, indent=1)
ctx.close()
