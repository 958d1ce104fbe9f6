"""Depth render timings (dev tool, not bench.py): prv_render_depth against prv_render of the same views -- the render launches'
milliseconds from HIP events (prv_profile_begin / end) and the ratio -- on the BASELINE.md section 6 scene (FIELD_256, table
U(-0.1, 0.1), no density bias; the 64-view hemisphere bench.py builds, 800x800, the engine's stepping rule) and on the 512^3 field.

    python scripts/depthbench.py [--reps 5] [--views 64] [--size 800] [--json out.json]
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--views", type=int, default=64)
ap.add_argument("--size", type=int, default=800)
ap.add_argument("--json", default="")
args = ap.parse_args()

import torch

from nerf_prv_amd import api, planner

ctx = api.Context(0)
pts = planner.hemisphere_generate(args.views)
tms, scale, offset = planner.hemisphere_transforms(pts, 0.3, 0.1, [1e-10] * 3)
fov_x = 2.0 * np.arctan(0.5 * 1280 / 915.60668945312500)
w = h = args.size
cams = ctx.cameras_from_matrices(tms, fov_x, w, h, scale, offset)
opts = api.engine_render_opts(w, h, 0, 1, 1e-4)
rgba = torch.empty((args.views, h, w, 4), dtype=torch.float32, device=ctx.device)
depth = torch.empty((args.views, h, w), dtype=torch.float32, device=ctx.device)
scenes = {"baseline": dict(api.FIELD_256, table_amp=0.1, density_bias=0.0), "field512": dict(api.FIELD_512)}
rows = []
for si, (name, fd) in enumerate(scenes.items()):
    ctx.synthetic_model(si, api.L.FieldDesc(**fd), 0x5EED0001)
    runs = {"colour": lambda: ctx.render(si, cams, None, opts, out=rgba, want_stats=False),
            "depth": lambda: ctx.render_depth(si, cams, None, opts, out=rgba, out_depth=depth, want_stats=False)}
    ms = {k: [] for k in runs}
    for r in range(args.reps + 1):  # the first round is a warm-up
        for k, fn in runs.items():  # interleaved, so clock drift hits both alike
            ctx.profile_begin()
            fn()
            torch.cuda.synchronize()
            prof = ctx.profile_end()
            if r:
                ms[k].append(prof["render_ms"])
    _, _, st = ctx.render_depth(si, cams, None, opts, out=rgba, out_depth=depth)
    med = {k: float(np.median(v)) for k, v in ms.items()}
    row = dict(scene=name, views=args.views, size=w, samples_evaluated=st.samples_evaluated, render_ms_median=med,
               render_ms_best={k: min(v) for k, v in ms.items()}, depth_over_colour=med["depth"] / med["colour"])
    rows.append(row)
    print(json.dumps(row), flush=True)
cams.close()
if args.json:
    with open(args.json, "w") as fh:
        json.dump(rows, fh, indent=1)
ctx.close()
