"""Mesh-occluder timings (dev tool, not bench.py): prv_coverage_create_occluded beside prv_coverage_create in the same run, on
scripts/coveragebench.py's two sizes (540 views of 80 x 45, 144 views of 800 x 800; 2^20 samples of the FIELD_256 synthetic
model's res-256 mesh, that mesh as the occluder), the share of (view, triangle) pairs the large path took, a sweep of
PRV_RASTER_SMALL_PIXELS on both, and prv_mesh_depth of one 12-triangle box at 144 x 800 x 800 (the large path alone).  Host clock
around calls that end in a device synchronise (every entry point here synchronises).
--color: prv_mesh_render (64-bit keys, then the shading pass) beside prv_mesh_depth on the same two sizes and nothing else; the
mesh then carries the field's colours.

    python scripts/rasterbench.py [--reps 5] [--log2n 20] [--sweep 1,4,16,64,256,1024] [--json out.json]
    python scripts/rasterbench.py --color --reps 3
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
ap.add_argument("--sweep", default="1,4,16,64,256,1024")
ap.add_argument("--json", default="")
ap.add_argument("--color", action="store_true")
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
        if hasattr(out, "close"):
            out.close()
    return dict(median=float(np.median(ms)), best=float(min(ms)))


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
mesh = ctx.marching_cubes(0, 256, threshold=thr, colors=args.color)
pts = None if args.color else mesh.sample(n, 1)
lo, hi = np.array([0.2, 0.2, 0.2]), np.array([0.8, 0.8, 0.8])
bv = np.array([[(hi if (k >> a) & 1 else lo)[a] for a in range(3)] for k in range(8)], np.float32)
quads = [(0, 1, 3, 2), (4, 6, 7, 5), (0, 4, 5, 1), (2, 3, 7, 6), (0, 2, 6, 4), (1, 5, 7, 3)]
box = ctx.mesh_from_arrays(bv, np.array([t for a, b, c, d in quads for t in ((a, b, c), (a, c, d))], np.uint32))
rows = []
for n_views, (w, h) in ((540, (80, 45)), (144, (800, 800))):
    cs = cameras(n_views)
    row = dict(case=f"{n_views}x{w}x{h}", n=n, triangles=int(mesh.counts()[1]))
    os.environ.pop("PRV_RASTER_SMALL_PIXELS", None)
    if args.color:
        row["mesh_depth_ms"] = timed(lambda: ctx.mesh_depth(mesh, cs, None, w, h))
        row["mesh_render_ms"] = timed(lambda: ctx.mesh_render(mesh, cs, None, w, h))
        row["mesh_render_planes_ms"] = timed(lambda: ctx.mesh_render(mesh, cs, None, w, h, want_depth=True, want_triangles=True))
        stats = ctx.raster_stats()
        row["pairs"], row["large_pairs"] = stats["pairs"], stats["large"]
        row["render_over_depth"] = row["mesh_render_ms"]["median"] / row["mesh_depth_ms"]["median"]
        cs.close()
        rows.append(row)
        print(json.dumps(row), flush=True)
        continue
    row["points_create_ms"] = timed(lambda: ctx.coverage(pts, cs, None, w, h, point_size=1))
    row["mesh_create_ms"] = timed(lambda: ctx.coverage(pts, cs, None, w, h, occluder=mesh))
    stats = ctx.raster_stats()
    row["pairs"], row["large_pairs"], row["large_share"] = stats["pairs"], stats["large"], stats["large"] / max(1, stats["pairs"])
    row["mesh_depth_ms"] = timed(lambda: ctx.mesh_depth(mesh, cs, None, w, h))
    row["sweep"] = {}
    for k in [int(x) for x in args.sweep.split(",")]:
        os.environ["PRV_RASTER_SMALL_PIXELS"] = str(k)
        t = timed(lambda: ctx.mesh_depth(mesh, cs, None, w, h))
        row["sweep"][str(k)] = dict(t, large_pairs=ctx.raster_stats()["large"])
    os.environ.pop("PRV_RASTER_SMALL_PIXELS", None)
    if (w, h) == (800, 800):
        row["box_depth_ms"] = timed(lambda: ctx.mesh_depth(box, cs, None, w, h))
        s = ctx.raster_stats()
        row["box_pairs"], row["box_large_pairs"] = s["pairs"], s["large"]
    cs.close()
    rows.append(row)
    print(json.dumps(row), flush=True)
if args.json:
    with open(args.json, "w") as fh:
        json.dump(rows, fh, indent=1)
box.close()
mesh.close()
ctx.close()
