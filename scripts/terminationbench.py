"""Termination render and method-9 round timings (dev tool, not bench.py), in the manner of scripts/entropybench.py:
prv_render_termination (16 bins) against prv_render_entropy of the same views -- the render launches' milliseconds from HIP
events (prv_profile_begin / end) and the ratio --, and a prv_score_views round of method 9 (PRV_SCORE_TERMINATION_JSD) against
one of method 3 (PRV_SCORE_ENSEMBLE_RGB_DENSITY) over the same five members (wall clock around the synchronised call), on the
BASELINE.md section 6 scene (FIELD_256, table U(-0.1, 0.1), no density bias; 64 views, 800x800, 128 samples per ray) and on
a scoring round of the reference's size (540 candidates, 80x45, 16 sub-samples, the engine's stepping rule, min_T 0.01).

    python scripts/terminationbench.py [--reps 5] [--json out.json]
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
args = ap.parse_args()

import torch

from nerf_prv_amd import api, planner

E, K = 5, api.L.TERMINATION_BINS_DEFAULT
ctx = api.Context(0)
fov_x = 2.0 * np.arctan(0.5 * 1280 / 915.60668945312500)
for e in range(E):
    ctx.synthetic_model(e, api.L.FieldDesc(**dict(api.FIELD_256, table_amp=0.1, density_bias=0.0)), 0x5EED0001 + e)
slots = list(range(E))
cases = {"section6_64x800x800_S128": (64, 800, 800, api.render_opts(800, 800, 128, 1, 1e-4)),
         "round_540x80x45_spp16_ngp": (540, 80, 45, api.engine_render_opts(80, 45, 0, 16, 0.01))}
rows = []
for name, (n, w, h, opts) in cases.items():
    tms, scale, offset = planner.hemisphere_transforms(planner.hemisphere_generate(n), 0.3, 0.1, [1e-10] * 3)
    cams = ctx.cameras_from_matrices(tms, fov_x, w, h, scale, offset)
    ent = torch.empty((n, h, w), dtype=torch.float32, device=ctx.device)
    alpha = torch.empty((n, h, w), dtype=torch.float32, device=ctx.device)
    launches = {"entropy": lambda: ctx.render_entropy(0, cams, None, opts, out=ent, out_alpha=alpha, want_stats=False),
                "termination": lambda: ctx.render_termination(0, cams, None, opts, K, want_stats=False)}
    rounds = {"method3": lambda: ctx.score_views(api.L.SCORE_ENSEMBLE_RGB_DENSITY, slots, cams, None, opts),
              "method9": lambda: ctx.score_views(api.L.SCORE_TERMINATION_JSD, slots, cams, None, opts)}
    ms = {k: [] for k in list(launches) + list(rounds)}
    for r in range(args.reps + 1):  # the first round is a warm-up
        for k, fn in launches.items():  # interleaved, so clock drift hits both alike
            ctx.profile_begin()
            fn()
            torch.cuda.synchronize()
            prof = ctx.profile_end()
            if r:
                ms[k].append(prof["render_ms"])
        for k, fn in rounds.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()  # (records to the host: the call returns synchronised)
            if r:
                ms[k].append((time.perf_counter() - t0) * 1e3)
    rec, _ = rounds["method9"]()
    med = {k: float(np.median(v)) for k, v in ms.items()}
    row = dict(case=name, members=E, bins=K, ms_median=med, ms_best={k: min(v) for k, v in ms.items()}, ms_all=ms,
               termination_over_entropy=med["termination"] / med["entropy"], method9_over_method3=med["method9"] / med["method3"],
               mean_jsd_bits=float(rec["score"].mean()))
    rows.append(row)
    print(json.dumps(row), flush=True)
    cams.close()
if args.json:
    with open(args.json, "w") as fh:
        json.dump(rows, fh, indent=1)
ctx.close()
