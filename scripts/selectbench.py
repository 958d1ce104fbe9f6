"""Selection-stage timings (dev tool, not bench.py), one bounded GPU step after another; the first failure ends the run.

  1. footprint launch: prv_render_footprint against prv_render_entropy of the same views, interleaved -- the render launches'
     milliseconds from HIP events (prv_profile_begin / end) and the ratio -- on the BASELINE.md section 6 scene (FIELD_256, table
     U(-0.1, 0.1), no density bias; 64 views, 800x800, 128 samples per ray) and on a scoring round of the reference's size (540
     candidates, 80x45, 16 sub-samples, the engine's stepping rule, min_T 0.01).  The entropy instances compile to the same
     registers, LDS and spills as before the footprint mode existed (scripts/kernel_resources.py), so this library's
     prv_render_entropy stands for the earlier one in the A/B.
  2. selection stage alone: prv_select_from_images at k = 4 on the planes of those two renders (host clock around the call,
     which ends in a device synchronise: it includes the per-round read-back of the views' sums).

  --locator surface|both adds prv_render_surface (level 0.5) to the interleaved launches of step 1, so one run times the
  footprint and the surface launch side by side on the same box (surface_over_footprint), and step 2 is run on its planes too.

    python scripts/selectbench.py [--reps 5] [--json out.json] [--locator expected|surface|both]
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
ap.add_argument("--json", default="")
ap.add_argument("--locator", choices=["expected", "surface", "both"], default="expected")
args = ap.parse_args()

import torch

from nerf_prv_amd import api, planner

ctx = api.Context(0)
fov_x = 2.0 * np.arctan(0.5 * 1280 / 915.60668945312500)
ctx.synthetic_model(0, api.L.FieldDesc(**dict(api.FIELD_256, table_amp=0.1, density_bias=0.0)), 0x5EED0001)
cases = {"section6_64x800x800_S128": (64, 800, 800, api.render_opts(800, 800, 128, 1, 1e-4)),
         "round_540x80x45_spp16_ngp": (540, 80, 45, api.engine_render_opts(80, 45, 0, 16, 0.01))}
rows = []
for name, (n, w, h, opts) in cases.items():
    tms, scale, offset = planner.hemisphere_transforms(planner.hemisphere_generate(n), 0.3, 0.1, [1e-10] * 3)
    cams = ctx.cameras_from_matrices(tms, fov_x, w, h, scale, offset)
    ent = torch.empty((n, h, w), dtype=torch.float32, device=ctx.device)
    alpha = torch.empty((n, h, w), dtype=torch.float32, device=ctx.device)
    runs = {"entropy": lambda: ctx.render_entropy(0, cams, None, opts, out=ent, out_alpha=alpha, want_stats=False),
            "footprint": lambda: ctx.render_footprint(0, cams, None, opts, want_stats=False)}
    if args.locator != "expected":
        runs["surface"] = lambda: ctx.render_surface(0, cams, None, opts, 0.5, want_stats=False)
    ms = {k: [] for k in runs}
    for r in range(args.reps + 1):  # the first round is a warm-up
        for k, fn in runs.items():  # interleaved, so clock drift hits both alike
            ctx.profile_begin()
            fn()
            torch.cuda.synchronize()
            prof = ctx.profile_end()
            if r:
                ms[k].append(prof["render_ms"])
    f_ent, f_alpha, f_depth, st = ctx.render_footprint(0, cams, None, opts)
    assert torch.equal(f_ent, ent) and torch.equal(f_alpha, alpha)  # faster and different is not faster
    med = {k: float(np.median(v)) for k, v in ms.items()}
    row = dict(case=name, samples_evaluated=st.samples_evaluated, render_ms_median=med, render_ms_best={k: min(v) for k, v in ms.items()},
               render_ms_all=ms, footprint_over_entropy=med["footprint"] / med["entropy"])
    if "surface" in med:
        s_ent, s_alpha, s_depth, s_hit, _ = ctx.render_surface(0, cams, None, opts, 0.5)
        assert torch.equal(s_ent, ent) and torch.equal(s_alpha, alpha)
        row.update(surface_over_footprint=med["surface"] / med["footprint"], surface_over_entropy=med["surface"] / med["entropy"])
    so = api.select_opts(k=4)
    sel = []
    for r in range(args.reps + 1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        chosen, gains = ctx.select_from_images(cams, None, f_ent, f_alpha, f_depth, so)
        if r:
            sel.append((time.perf_counter() - t0) * 1e3)
    row.update(select_k4_ms_median=float(np.median(sel)), select_k4_ms_best=min(sel), select_k4_ms_all=sel, chosen=chosen.tolist(),
               gains=[int(g) for g in gains])
    if "surface" in med:
        sel = []
        for r in range(args.reps + 1):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            chosen, gains = ctx.select_from_images(cams, None, s_ent, s_hit, s_depth, so)
            if r:
                sel.append((time.perf_counter() - t0) * 1e3)
        row.update(surface_select_k4_ms_median=float(np.median(sel)), surface_chosen=chosen.tolist(), surface_gains=[int(g) for g in gains])
    rows.append(row)
    print(json.dumps(row), flush=True)
    cams.close()
if args.json:
    with open(args.json, "w") as fh:
        json.dump(rows, fh, indent=1)
ctx.close()
