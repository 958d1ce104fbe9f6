"""Depth-map fusion timings (dev tool, not bench.py): prv_tsdf_integrate of 64 views at 800 x 800 into a 256^3 volume -- the depth
and colour images are prv_mesh_render's of the FIELD_256 synthetic model's res-128 mesh -- with and without the colour volume,
then prv_tsdf_mesh.  HIP events on the context's stream around each call, after a warm-up call; one JSON line.

    python scripts/tsdfbench.py [--reps 5] [--res 256] [--views 64] [--size 800] [--json out.json]
"""
import argparse
import json
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--res", type=int, default=256)
ap.add_argument("--views", type=int, default=64)
ap.add_argument("--size", type=int, default=800)
ap.add_argument("--json", default="")
args = ap.parse_args()

import torch

from nerf_prv_amd import api, planner

ctx = api.Context(0)


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


def timed(fn):
    """-> dict(median, best) of the GPU milliseconds between two events around fn(), the first round a warm-up"""
    ms = []
    for r in range(args.reps + 1):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        out = fn()
        b.record()
        torch.cuda.synchronize()
        if r:
            ms.append(a.elapsed_time(b))
        if hasattr(out, "close"):
            out.close()
    return dict(median=float(np.median(ms)), best=float(min(ms)))


def kernel_resources():
    """VGPRs and waves per SIMD of the integrate kernel, from scripts/kernel_resources.py (None without a compiler)"""
    try:
        out = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "kernel_resources.py"), "prv_tsdf.hip", "tsdf_integrate"],
                             capture_output=True, text=True, timeout=600).stdout
        f = [l for l in out.splitlines() if "tsdf_integrate_kernel" in l][0].split()
        return dict(vgprs=int(f[1]), sgprs=int(f[3]), waves_per_simd=int(f[7]))
    except Exception:
        return None


ctx.synthetic_model(0, api.field_desc(**api.FIELD_256), 0x5EED0001)
thr = float(np.median(ctx.density_grid(0, 64).cpu().numpy()))
mesh = ctx.marching_cubes(0, 128, threshold=thr, colors=True)
cs = cameras(args.views)
w = h = args.size
rgba8, depth = ctx.mesh_render(mesh, cs, None, w, h, want_depth=True)
n = args.res ** 3
row = dict(case=f"{args.res}^3 x {args.views} views x {w}x{h}", points=n, point_views=n * args.views)
for name, colors in (("depth_only", False), ("depth_colour", True)):
    vol = ctx.tsdf_volume(args.res, colors=colors)
    t = timed(lambda: vol.integrate(cs, None, depth, None, rgba8 if colors else None))
    pv = n * args.views / (t["median"] * 1e-3)
    gather = 4 * (2 if colors else 1)  # bytes gathered per point-view that passes: depth, and the colour word
    chunks = -(-args.views // 32)      # launches per call: the state is read and written once per launch
    state = (48 if colors else 16) * n * chunks
    row[name] = dict(ms_per_call=t, point_views_per_s=pv, gather_bytes_per_s_at_most=pv * gather, state_bytes_per_call=state,
                     state_bytes_per_s=state / (t["median"] * 1e-3), info=vol.info())
    if colors:
        row["mesh_ms"] = timed(lambda: vol.mesh())
        with vol.mesh() as m:
            row["mesh_counts"] = m.counts()
    vol.close()
row["kernel"] = kernel_resources()
print(json.dumps(row), flush=True)
if args.json:
    with open(args.json, "w") as fh:
        json.dump(row, fh, indent=1)
cs.close()
mesh.close()
ctx.close()
