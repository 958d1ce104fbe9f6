"""Surface-coverage timings (dev tool, not bench.py): prv_coverage_create (depth buffers + visibility bit matrix + the counts),
prv_coverage_curve over every view and prv_coverage_greedy, on 2^20 samples of the FIELD_256 synthetic model's mesh -- at the
reference's candidate round (540 views of 80 x 45) and at 144 views of 800 x 800.  Host clock around calls that end in a device
synchronise (every entry point here synchronises).

    python scripts/coveragebench.py [--reps 5] [--log2n 20] [--greedy-k 20] [--point-size 1] [--json out.json]
"""
import argparse
import json
import os
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--log2n", type=int, default=20)
ap.add_argument("--greedy-k", type=int, default=20)
ap.add_argument("--point-size", type=int, default=1)
ap.add_argument("--json", default="")
args = ap.parse_args()

import torch

from nerf_prv_amd import api, planner

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


def hemisphere(k):
    """k unit vectors with z >= 0, the pole first (the view-space files' format)"""
    i = np.arange(1, k)
    z = 1.0 - i / float(k)
    r = np.sqrt(np.maximum(0.0, 1.0 - z * z))
    th = np.pi * (3.0 - np.sqrt(5.0)) * i
    return np.concatenate([[[0.0, 0.0, 1.0]], np.stack([r * np.cos(th), r * np.sin(th), z], axis=1)])


def cameras(k):
    c = [1e-10] * 3
    intr = planner.Intrinsics(width=1280, height=720, ppx=647.1, ppy=372.5, fx=915.60668945312500, fy=913.3)
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "views.json")
        planner.write_transforms(path, intr, planner.view_space(hemisphere(k), 0.3, c), c, 0.1, candidate=True)
        return ctx.cameras_from_json(path)


ctx.synthetic_model(0, api.field_desc(**api.FIELD_256), 0x5EED0001)
thr = float(np.median(ctx.density_grid(0, 64).cpu().numpy()))
mesh = ctx.marching_cubes(0, 256, threshold=thr, colors=False)
pts = mesh.sample(n, 1)
mesh.close()
rows = []
for n_views, (w, h) in ((540, (80, 45)), (144, (800, 800))):
    cs = cameras(n_views)
    cov, med, best = timed(lambda: ctx.coverage(pts, cs, None, w, h, point_size=args.point_size))
    row = dict(case=f"{n_views}x{w}x{h}", n=n, point_size=args.point_size, create_ms=dict(median=med, best=best), **cov.info())
    order = np.arange(n_views, dtype=np.int32)
    _, med, best = timed(lambda: cov.curve(order))
    row["curve_all_views_ms"] = dict(median=med, best=best)
    k = min(args.greedy_k, n_views)
    (chosen, covered), med, best = timed(lambda: cov.greedy(k))
    row["greedy_ms"] = dict(k=k, median=med, best=best)
    row["greedy_covered"] = int(covered[-1])
    row["file_order_covered"] = int(cov.curve(order[:k])[-1])
    cov.close()
    cs.close()
    rows.append(row)
    print(json.dumps(row), flush=True)
if args.json:
    with open(args.json, "w") as fh:
        json.dump(rows, fh, indent=1)
ctx.close()
