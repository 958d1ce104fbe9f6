#!/usr/bin/env python3
"""bench.py -- the hot path of NeRF-PRV on MI355X: render + score candidate views.

One "step" = one scoring round of the planner over this rank's shard of the candidate set:
march + render every view (800x800, 128 samples/ray) of the synthetic 256^3 hash-grid field
BASELINE.md section 6 specifies (table U(-0.1,0.1), Xavier MLPs, analytic occupancy), reduce each to a
PSNR/coverage score against reference images already resident in HBM, all-gather the 16-byte records over
RCCL (N > 1: prv_score_views_sharded, the C ABI's own communicator -- what prv_planner runs), rank.
BASELINE.json configs[1].

    python bench.py --gpus N --steps K --warmup W

With N > 1 and no WORLD_SIZE in the environment this process only LAUNCHES: it starts
`python -m torch.distributed.run --nproc-per-node N bench.py ...` (one rank per GPU, RCCL),
never touches a GPU itself, forwards rank 0's JSON line and exits with the children's code.
Under torch.distributed.run (WORLD_SIZE set) it is one of the ranks.

    --mode weak    (default) --views-per-gpu views per rank, total grows with N
    --mode strong  --views-total views sharded over the ranks (BASELINE configs[3]: 1024 views, --field 512)

A plain run sets up, warms up, times the K steps and prints the headline line (its `roofline` comes from the timed
steps themselves).  Everything else the line can carry -- the CPU baseline, the side workloads (field512, field_hbm, the
other scene, the reference's round, ngp_step, first hit), training, the full loop, N > 1's configs[3] round and the
torch.distributed cross-check of the gathered records -- runs only with --full.

    --dump-outputs DIR   after the timed steps: the last step's gathered records and ranking as DIR/<name>.npy

Prints ONE JSON line on rank 0.  Parity status of every number here: the GPU path is checked
against this repository's own CPU oracle (tests/), which is NOT pinned to the reference binary
(instant-ngp is absent from the reference tree) -- stated in the line as "parity".
"""
import argparse
import hashlib
import json
import os
import socket
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

SEED_A, SEED_B = 0x5EED0001, 0x5EED0002
BYTES_PER_SAMPLE = 512   # L*8 corners*F*2 B = 8*8*4*2 = 16*8*2*2: hash-table gather per field evaluation
FLOP_PER_SAMPLE = 20480  # 10,240 MAC of the two MLPs
MFMA_PER_ROUND = 24      # v_mfma_f32_32x32x16_f16 per 32-slot round (prv_device.hpp: mlp_forward / mlp_forward2; the 64-slot
                         # kernel counts a wave iteration as two rounds)
# peaks, MI355X_MICROARCH.md
HBM_PEAK_GBS = 8000.0        # 8 TB/s spec
HBM_ACHIEVABLE_GBS = 6300.0  # what a streaming kernel reaches (MI355X_MICROARCH.md)
L2_PEAK_GBS = 34500.0        # aggregate L2, ~34.5 TB/s
MFMA_F16_PEAK_TFLOPS = 2500.0  # dense f16/bf16
N_SIMD, MAX_CLOCK_HZ = 1024, 2.4e9  # 256 CUs x 4 SIMDs
# What ONE SIMD spends per wave64 vector instruction, MEASURED on this chip (scripts/valu_rate.hip ->
# profiles/r04_valu_issue_rate.txt; grid 1, four waves per SIMD, the slowest wave of the launch -- the lowest figures of the
# table, so the peak below is the most any instruction stream of this mix can get).  gfx950 has THREE issue classes:
#   c2  2 cycles once two waves share the SIMD (one wave alone: 5): v_fma/mul/add/sub_f32, v_add/sub_u32, v_and/or/xor/mov_b32,
#       v_bitop3_b32, v_lshrrev_b32, v_ashrrev_i32, v_max_f16, v_accvgpr_*
#   c4  4 cycles whatever the occupancy: every packed-f16 / packed-f32 / f64 op, every conversion, v_lshlrev_b32, v_max/min_f32,
#       v_med3, v_fract, v_mad/mul_u32_u24, v_mul_lo_u32, v_add3/lshl_add/and_or/bfe/bfi/perm, v_cmp, v_cndmask, DPP / SDWA forms
#   c8  8 cycles: v_exp/rcp_f32 (and the other transcendentals), v_permlane32_swap, v_fma_f16, v_fma_mixlo_f16
# and an MFMA holds the SIMD's vector issue for 8 cycles of its 32 (the "v_mfma + k VALU" rows: 24 fillers + 1 MFMA = 108 cycles).
# The round-3 line assumed 4 cycles flat; the hardware guide says 2 with >= 2 waves per SIMD -- true for c2 only, and four
# fifths of this kernel's instructions are c4 (packed-f16 blend, f32 -> f16 conversions, ReLU).
ISSUE_CYCLES = {"c2": 2.08, "c4": 4.07, "c8": 8.07, "mfma": 8.0}
ISSUE_RATE_FILE = os.path.join("profiles", "r04_valu_issue_rate.txt")
# What bounds the trainer: the f32 adds into the table gradient are served by the memory side
# at one rate per 64-byte request whatever their shape (scripts/atomic_rate.hip), and the backward pass issues 26.4 of them
# per composited sample under the fixed sampling rule, 9.8 under the engine's marcher (TCC_EA0_ATOMIC of the backward tile kernel).
GATHER_CALIB_GBS = 3800.0  # random 64-byte gathers over a 64 MiB footprint (scripts/gather_calib.hip -> profiles/archive/r01_gather_calib.txt)
ATOMIC_REQ_PEAK_G = 20.5
ATOMIC_RATE_FILE = os.path.join("profiles", "r04_atomic_request_rate.txt")
# round 6, re-measured at upstream's batch (262 K composited samples per step) under both sampling rules of a training ray:
ATOMIC_REQ_PER_SAMPLE = {"ngp": 9.76, "fixed": 26.35}
ATOMIC_REQ_FILE = os.path.join("profiles", "r06_train_rules.txt")
ISSUE_PEAK_GCYC = N_SIMD * MAX_CLOCK_HZ / 1e9  # 2457.6 G SIMD issue-cycles/s at the 2.4 GHz maximum clock
VALU_PEAK_GINST = ISSUE_PEAK_GCYC / ISSUE_CYCLES["c4"]  # wave-instructions/s if every instruction were c4 (kept for the detail object)
ROUND_COST_FILE = os.path.join("profiles", "r06_round_cost.json")  # VALU instructions per wave-round, from the PMC pass
TRAFFIC_FILE = os.path.join("profiles", "r06_pmc_traffic.json")    # fabric-side bytes per launch, from the PMC passes
ISA_CLASSES_FILE = os.path.join("profiles", "r06_isa_classes.json")  # static issue-class histogram of the hot loop (scripts/isa_count.py)


# The algorithmic floor of the render kernel: wave-instructions one 64-sample wave iteration NEEDS for this algorithm
# (fp16 table and blend as tiny-cuda-nn defines them, fp16 activations between the MLP layers), counted from the ISA of
# render_queue64_kernel in DESIGN.md section 3 ("floor"), each with its issue class:
#   blend 128 v_pk_fma_f16 (c4) | per level: weights 3 v_fract + 3 v_cvt_pk_f16_f32 + 6 v_pk_mul_f16 (c4) + 3 v_sub_f32 (c2),
#   positions 3 v_fma_f32 (c2), cell indices 3 v_cvt_i32_f32 (c4) | addresses: 4 per dense level (2 v_mul_u32_u24 c4 + 2 v_add c2),
#   26 per hashed level (x shift + 2 multiplies + 3 clamps c4; 3 increments, 8 v_bitop3, 8 v_and / v_add c2 ... 6 c4 + 20 c2) |
#   accumulator -> next B operand 104 v_cvt_pk_f16_f32 + 96 v_pk_max_f16 (c4) | 8 v_permlane32_swap (c8) | sample position
#   8 v_fma_f32 (c2) | sample selection 8 (c4) | compositing 29 (2 v_exp + 1 v_rcp c8, 13 c2, 13 c4).
# MFMA: 10,240 MAC x 64 samples / 16,384 MAC per v_mfma_f32_32x32x16_f16 = 40 (48 are issued: the two 64 -> 16 layers fill
# half of their 32-row tiles).
def isa_floor(n_levels, n_dense):
    n_hashed = n_levels - n_dense
    c4 = 128 + 12 * n_levels + 3 * n_levels + 2 * n_dense + 6 * n_hashed + 200 + 8 + 13
    c2 = 3 * n_levels + 3 * n_levels + 2 * n_dense + 20 * n_hashed + 8 + 13
    c8 = 8 + 3
    cyc = c2 * ISSUE_CYCLES["c2"] + c4 * ISSUE_CYCLES["c4"] + c8 * ISSUE_CYCLES["c8"] + 40 * ISSUE_CYCLES["mfma"]
    return {"valu_per_64_samples": c2 + c4 + c8, "c2": c2, "c4": c4, "c8": c8, "mfma_per_64_samples": 40, "issue_cycles_per_64_samples": cyc}


def parse_args(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--mode", choices=["weak", "strong"], default="weak")
    ap.add_argument("--views-per-gpu", type=int, default=64)
    ap.add_argument("--views-total", type=int, default=1024, help="--mode strong: the fixed candidate set")
    ap.add_argument("--width", type=int, default=800)
    ap.add_argument("--height", type=int, default=800)
    ap.add_argument("--samples", type=int, default=128)
    ap.add_argument("--field", choices=["256", "512"], default="256")
    ap.add_argument("--scene", choices=["baseline", "dense"], default="baseline",
                    help="baseline = BASELINE.md section 6 literally: table U(-0.1,0.1), no density bias (the headline); "
                         "dense = table U(-4,4), density bias 3: an opaque object, early termination exercised")
    # side measurements: each acts in a --full run only, and giving any of them asks for that run (so that a command line
    # written when the full run was the default still runs what it ran then)
    side = ap.add_argument_group("side measurements", "each acts in a --full run only; giving any of them turns --full on")
    side_actions = []

    def side_opt(*names, **kw):
        side_actions.append(side.add_argument(*names, **kw))

    side_opt("--full-loop", action="store_true",
             help="BASELINE configs[4] at size (minutes): prv_planner configs/TrainInLoop.yaml semantics, 5 objects x 20 rounds (mode 21) + "
                  "the PSNR curve and stopping criterion (mode 4), end-to-end wall-clock in the full_loop sub-object.  Without it "
                  "a --full run does ONE object x 20 rounds (a few minutes at upstream's training batch) so that its line carries the figure")
    side_opt("--full-loop-objects", type=int, default=0, help="0 = 1 by default, 5 with --full-loop")
    side_opt("--no-full-loop", action="store_true")
    side_opt("--full-loop-small", action="store_true",
             help="full_loop on configs/TrainInLoop_small.yaml: the 4096-ray training cap of rounds 1-5, about 1/6.6 of upstream's batch "
                  "(reported as `reduced`; the default trains at the library default = upstream's 2^18-sample batch)")
    side_opt("--cpu-seconds", type=float, default=12.0)
    side_opt("--no-cpu-baseline", action="store_true")
    side_opt("--reference-round-fixed", action="store_true", help="reference_round: also the round with 128 uniform samples per ray (not the reference's rule)")
    side_opt("--no-training", action="store_true")
    side_opt("--no-extras", action="store_true", help="skip the field512 / baseline-scene / first-hit side measurements")
    side_opt("--train-steps", type=int, default=300)
    side_opt("--no-field-hbm", action="store_true", help="skip the field_hbm side workload (a 448 MiB table: the one HBM-bound line of the record)")
    side_opt("--no-config3", action="store_true", help="N > 1: skip the configs[3] sub-object (1024 views of the 512^3 field, strong scaling)")
    side_opt("--train-patch", default="", help="full_loop: WxH, training rays drawn as patches of adjacent pixels (yaml train_patch_w / "
                                               "train_patch_h; a speed / quality trade: profiles/r05_train_patch_study.txt)")
    ap.add_argument("--full", action="store_true",
                    help="also every side measurement and check beyond the headline (the side-measurement options refine it); "
                         "off: the run does what the headline figure needs and nothing else")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write the last timed step's records (score, psnr, coverage) and ranking as DIR/<name>.npy (float64 / float32)")
    unset = object()  # argparse fills in a default only where the namespace has no value yet: what stays `unset` was not given
    args = ap.parse_args(argv, argparse.Namespace(**{a.dest: unset for a in side_actions}))
    for a in side_actions:
        if getattr(args, a.dest) is unset:
            setattr(args, a.dest, a.default)
        else:
            args.full = True
    if args.steps < 1:
        ap.error("--steps must be at least 1")
    return args


def dump_outputs(directory, records, order):
    """what the timed path hands its caller after a step: the gathered 16-byte records, field by field, and the ranking
    (view ids, stored as float64: exact)"""
    import numpy as np

    os.makedirs(directory, exist_ok=True)
    arrays = {"records_score": np.asarray(records["score"], np.float64), "records_psnr": np.asarray(records["psnr"], np.float32),
              "records_coverage": np.asarray(records["coverage"], np.float32), "ranking": np.asarray(order, np.float64)}
    for name, a in arrays.items():
        np.save(os.path.join(directory, name + ".npy"), a)


# ------------------------------------------------------------------ launcher (N > 1, plain invocation)

def free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def launch_ranks(args, argv):
    """parent of a plain `python bench.py --gpus N`: N fresh rank processes under torch.distributed.run.
    Nothing here imports torch or touches a GPU; stdout of the children (rank 0's JSON line) is forwarded."""
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={args.gpus}",
           "--master-addr", "127.0.0.1", "--master-port", str(free_port()), os.path.abspath(__file__)] + list(argv)
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")  # RCCL needs dmabuf IPC on this pool
    env.setdefault("OMP_NUM_THREADS", "1")
    proc = subprocess.Popen(cmd, stdout=subprocess.PIPE, text=True, env=env, cwd=ROOT)
    line = None
    for out in proc.stdout:
        if out.startswith("{") and '"metric"' in out:
            line = out
        else:
            sys.stderr.write(out)  # launcher / rank chatter is not the result
    rc = proc.wait()
    if line is not None:
        sys.stdout.write(line)
        sys.stdout.flush()
    if rc == 0 and line is None:
        sys.stderr.write("bench.py: the ranks exited cleanly without a JSON line\n")
        rc = 1
    return rc


# ------------------------------------------------------------------ CPU side (rank 0, N = 1 only)

def usable_cores():
    """host cores this process may actually use: the affinity mask, capped by a cgroup CPU quota when there is one
    (the GPU boxes expose 256 logical CPUs behind a 16-CPU quota: 256 threads there are 16 cores' worth of time)"""
    n = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)
    try:
        quota, period = open("/sys/fs/cgroup/cpu.max").read().split()[:2]
        if quota != "max":
            n = min(n, max(1, -(-int(quota) // int(period))))
    except (OSError, ValueError):
        try:
            q = int(open("/sys/fs/cgroup/cpu/cpu.cfs_quota_us").read())
            per = int(open("/sys/fs/cgroup/cpu/cpu.cfs_period_us").read())
            if q > 0 and per > 0:
                n = min(n, max(1, -(-q // per)))
        except (OSError, ValueError):
            pass
    return max(1, n)


def cpu_baseline(args, fkw, tms, scale, offset, fov_x):
    """the oracle (a scalar C port of the same algorithm) on the host cores, bounded sample"""
    from oracle import oracle as orc

    threads = min(usable_cores(), 256)  # the oracle's pthread pool tops out there
    f = orc.OracleField(orc.desc(**fkw), seed=SEED_A)
    cams = orc.cameras_from_transforms(tms, fov_x, args.width, args.height, scale, offset)
    band = min(args.height, max(64, threads))  # one row per thread at least: every core the line claims has work
    rows = ((args.height - band) // 2, (args.height - band) // 2 + band)
    f.render(cams[0], args.width, args.height, args.samples, 1, 1e-4, threads=threads, rows=(rows[0], rows[0] + 1))
    n_eval, n_views, t0 = 0, 0, time.perf_counter()
    for v in range(len(cams)):
        _, ne = f.render(cams[v], args.width, args.height, args.samples, 1, 1e-4, threads=threads, rows=rows)
        n_eval += ne
        n_views += 1
        if time.perf_counter() - t0 > args.cpu_seconds:
            break
    dt = time.perf_counter() - t0
    cores = min(threads, band)
    fh_rate, fh_cores = first_hit_cpu(f, cams[0], args, cores)
    return {
        "value": n_eval / dt,
        "unit": "ray-samples/s",
        "cores": cores,
        "kind": "port",
        "sample": f"rows {rows[0]}-{rows[1]} of {n_views} views at {args.width}x{args.height}, "
                  f"{args.samples} samples/ray, {n_eval} samples evaluated in {dt:.1f} s "
                  f"(oracle/prv_oracle.c, pthreads over rows)",
        "first_hit_rays_per_s": fh_rate,
        "first_hit_cores": fh_cores,
    }


def first_hit_cpu(f, cam, args, cores):
    """the oracle's scalar first-hit DDA over one whole view, the rows dealt to `cores` threads (ctypes calls drop
    the GIL, so the bands run side by side) -- the same cores the marcher line claims, not one"""
    from concurrent.futures import ThreadPoolExecutor

    from oracle import oracle as orc

    cores = max(1, min(cores, args.height))
    edges = [args.height * k // cores for k in range(cores + 1)]
    bands = [(edges[k], edges[k + 1]) for k in range(cores) if edges[k + 1] > edges[k]]
    orc.first_hit_image(f, cam, args.width, args.height, rows=(0, 1))
    t0 = time.perf_counter()
    with ThreadPoolExecutor(max_workers=len(bands)) as pool:
        list(pool.map(lambda b: orc.first_hit_image(f, cam, args.width, args.height, rows=b), bands))
    return args.height * args.width / (time.perf_counter() - t0), len(bands)


def mapped_rccl():
    """distinct librccl files this process has mapped right now (/proc/self/maps)"""
    seen = []
    try:
        with open("/proc/self/maps") as fh:
            for line in fh:
                path = line.split(None, 5)[-1].strip() if line.count(" ") >= 5 else ""
                if os.path.basename(path).startswith("librccl.so") and path not in seen:
                    seen.append(path)
    except OSError:
        pass
    return seen


def load_json(rel):
    path = os.path.join(ROOT, rel)
    if not os.path.exists(path):
        return None
    with open(path) as fh:
        return json.load(fh)


# ------------------------------------------------------------------ one rank

class Round:
    """one workload (field, scene, view set) on this rank: reference images resident, a scoring round per step()"""

    def __init__(self, env, fkw, n_views, args, slots=(0, 1), comm=None):
        """comm: the C ABI's communicator (api.Comm) -- with it a step IS prv_score_views_sharded, the product's multi-GPU
        path; without it (one rank, or the torch.distributed fallback) the step scores the shard and gathers in Python"""
        api, planner, torch, np = env["api"], env["planner"], env["torch"], env["np"]
        self.env, self.args, self.n_views, self.comm = env, args, n_views, comm
        ctx, rank, world = env["ctx"], env["rank"], env["world"]
        self.desc = api.L.FieldDesc(**fkw)
        self.slot = slots[0]
        ctx.synthetic_model(slots[0], self.desc, SEED_A)  # the field being scored
        ctx.synthetic_model(slots[1], self.desc, SEED_B)  # the field the reference images come from
        # candidate set: generated hemisphere, radius 0.3 around the origin (+1e-10), object size 0.1
        # -> cameras at 1.5 cube units from the centre of the unit cube
        pts = planner.hemisphere_generate(n_views)
        self.fov_x = 2.0 * np.arctan(0.5 * 1280 / 915.60668945312500)  # the reference camera's 69.9 deg
        self.tms, self.scale, self.offset = planner.hemisphere_transforms(pts, 0.3, 0.1, [1e-10] * 3)
        self.cams = ctx.cameras_from_matrices(self.tms, self.fov_x, args.width, args.height, self.scale, self.offset)
        self.my_ids, self.per_rank = planner.shard_views(n_views, rank, world, interleaved=True)  # balances pole vs equator views
        self.opts = api.render_opts(args.width, args.height, args.samples, 1, 1e-4)
        # reference images of this rank's views, resident in HBM before any timed region
        self.gt, _ = ctx.render(slots[1], self.cams, self.my_ids, self.opts, want_stats=False)
        self.rec_dev = torch.zeros(max(1, self.per_rank) * 16, dtype=torch.uint8, device=env["device"])

    def step(self, want_stats=False):
        env = self.env
        api, planner, np = env["api"], env["planner"], env["np"]
        if self.comm is not None:
            # the product path (include/prv.h "several GPUs"; what prv_planner `shard: views` runs): shard -> render +
            # score -> ONE ncclAllGather of the 16-byte records on the context's stream -> view order, inside libprv_hip.so
            records, st = self.comm.score_views(api.L.SCORE_PSNR_COVERAGE, [self.slot], self.cams, self.n_views, self.opts,
                                                gt_shard=self.gt, interleaved=True, want_stats=want_stats)
        else:
            _, st = env["ctx"].score_views(api.L.SCORE_PSNR_COVERAGE, [self.slot], self.cams, self.my_ids, self.opts, gt=self.gt,
                                           records_dev=self.rec_dev, to_host=False, want_stats=want_stats)
            if env["use_dist"]:  # fallback only (the C ABI's communicator did not come up): torch.distributed's all-gather
                records = planner.gather_records(self._rec_for_gather(), self.per_rank, self.n_views, device=env["gather_device"], interleaved=True)
            else:  # one rank: its records are the round's records
                records = self.rec_dev.cpu().numpy().view(api.RECORD_DTYPE)[: self.n_views].copy()
        order = api.rank_host(records, np.arange(self.n_views, dtype=np.int32))
        return st, records, order

    def torch_gather_round(self):
        """the cross-check of the product path: the same shard scored into rec_dev, gathered by torch.distributed"""
        env = self.env
        api, planner = env["api"], env["planner"]
        env["ctx"].score_views(api.L.SCORE_PSNR_COVERAGE, [self.slot], self.cams, self.my_ids, self.opts, gt=self.gt,
                               records_dev=self.rec_dev, to_host=False)
        return planner.gather_records(self._rec_for_gather(), self.per_rank, self.n_views, device=env["gather_device"], interleaved=True)

    def _rec_for_gather(self):
        """the device tensor itself for RCCL; a host copy when torch.distributed runs on gloo (tests: ranks sharing a GPU)"""
        env = self.env
        if env.get("gather_device") is not None or not env["use_dist"]:
            return self.rec_dev
        return self.rec_dev.cpu().numpy().view(env["api"].RECORD_DTYPE)[: len(self.my_ids)].copy()

    def measure(self, steps, warmup):
        """W untimed steps, then EXACTLY `steps` timed ones between barriers; -> dict of raw measurements"""
        env = self.env
        torch, dist, ctx = env["torch"], env["dist"], env["ctx"]

        def barrier():
            torch.cuda.synchronize()
            if env["use_dist"]:
                dist.barrier()
            torch.cuda.synchronize()

        st, records, order = self.step(want_stats=True)  # also sizes every workspace
        for _ in range(max(0, warmup - 1)):
            self.step()
        import gc

        gc.collect()
        gc.disable()  # as timeit does: a generation-2 pass of the interpreter (tens of ms with torch loaded) is not the workload
        try:
            barrier()
            ctx.profile_begin()
            t0 = time.perf_counter()
            for _ in range(steps):
                _, records, order = self.step()
            barrier()
            elapsed = time.perf_counter() - t0
            prof = ctx.profile_end()
            prof["clock_ghz"] = ctx.render_clock_ghz()  # stamped inside the last step's render launch (prv_debug_render_clock)
        finally:
            gc.enable()
        tmax = torch.tensor([elapsed], dtype=torch.float64, device=env.get("red_device", env["device"]))
        tot = torch.tensor([float(st.samples_evaluated), float(st.samples_nominal), float(st.rays)], dtype=torch.float64,
                           device=env.get("red_device", env["device"]))
        if env["use_dist"]:
            dist.all_reduce(tmax, op=dist.ReduceOp.MAX)
            dist.all_reduce(tot, op=dist.ReduceOp.SUM)
        ev_all, nom_all, rays_all = (float(x) for x in tot.tolist())
        return dict(elapsed=float(tmax.item()), steps=steps, prof=prof, st=st, order=order, records=records, ev_all=ev_all,
                    nom_all=nom_all, rays_all=rays_all)

    def close(self):
        self.cams.close()
        self.gt = None


def lib_digest():
    """sha256 of the DEVICE code (the .hip_fatbin section) of the libprv_hip.so this run loads: the per-round instruction
    counts of the committed PMC pass are a property of the gfx950 code objects, so the profile file names the code it was
    taken from and the line says whether they match (host-side changes to the library do not break the binding)"""
    from nerf_prv_amd import _lib

    return _lib.device_code_digest()


def kernel_figures(m, variant, hbm_bound, scene, layout):
    """-> (roofline, detail) of the dominant kernel (render_queue64) from a Round.measure() result.

    `roofline` is flat and short, the contract's keys first (kernel, bound, frac, peak, achieved, unit, traffic, then the
    in-run measurements they come from): a parser that keeps the first couple of dozen scalar keys keeps all of it.  Everything
    else (the floor's composition, the issue occupancy, the per-clock readings, provenance of the PMC figures) is `detail`.

    In-run quantities: launch durations (HIP events on the launch stream), evaluated samples and wave-rounds (counted by the
    kernel itself), the shader clock (stamped inside the launch).  Per-round instruction counts are a property of the binary:
    they come from the committed PMC pass (SQ_INSTS_VALU / wave-rounds) and the static issue-class histogram of the hot loop,
    are labelled *_from_profile, and carry the digest of the device code they were measured on (profile_matches_binary)."""
    prof, st, k = m["prof"], m["st"], m["steps"]
    launches = max(1, prof["render_launches"])
    kernel_s = prof["render_ms"] * 1e-3 / launches
    samples = st.samples_evaluated * k / launches
    rounds = st.wave_rounds * k / launches
    alg_gbs = samples * BYTES_PER_SAMPLE / kernel_s / 1e9
    mfma_tflops = samples * FLOP_PER_SAMPLE / kernel_s / 1e12
    # the MFMA pipe's own occupancy: 24 instructions of 8 passes x 4 cycles per wave-round, padded slots included
    mfma_pipe_frac = rounds * MFMA_PER_ROUND * 32 / (kernel_s * N_SIMD * MAX_CLOCK_HZ)
    key = f"{variant} {scene}"
    digest = lib_digest()
    cost = (load_json(ROUND_COST_FILE) or {}).get(key)
    classes = (load_json(ISA_CLASSES_FILE) or {}).get(variant)
    traffic = (load_json(TRAFFIC_FILE) or {}).get(key)
    clock = prof.get("clock_ghz") or 0.0
    cycles_per_s = N_SIMD * MAX_CLOCK_HZ
    # the algorithmic floor: issue cycles this algorithm NEEDS per 64 samples at the measured per-class
    # costs -- a fatter kernel scores lower here, and higher on issue_busy
    floor = isa_floor(layout["n_levels"], layout["n_dense_levels"])
    floor_gcyc = samples / 64.0 * floor["issue_cycles_per_64_samples"] / kernel_s / 1e9
    floor_frac = floor_gcyc / ISSUE_PEAK_GCYC
    # the instructions actually ISSUED, priced the same way: the hot loop's static class histogram (two blocks, once per
    # 64-slot iteration = two wave-rounds) + whatever else the PMC pass counted per round, at the c4 price
    issued_cyc_per_iter = issued_busy = None
    if cost and classes:
        hot = classes["c2"] + classes["c4"] + classes["c8"]
        rest = max(0.0, 2.0 * cost["valu_insts_per_round"] - hot)
        issued_cyc_per_iter = (classes["c2"] * ISSUE_CYCLES["c2"] + classes["c4"] * ISSUE_CYCLES["c4"] + classes["c8"] * ISSUE_CYCLES["c8"]
                               + classes["mfma"] * ISSUE_CYCLES["mfma"] + rest * ISSUE_CYCLES["c4"])
        issued_busy = rounds / 2.0 * issued_cyc_per_iter / (kernel_s * cycles_per_s)
    traffic_bytes = None
    fabric_gbs = None
    if traffic:
        per_sample = (traffic["fetch_kib_per_launch"] + traffic["write_kib_per_launch"]) * 1024.0 / traffic["samples_evaluated_per_launch"]
        traffic_bytes = per_sample * samples
    if hbm_bound:
        # 64 MiB table: beyond the L2s, INSIDE the 256 MiB Infinity Cache (MI355X_MICROARCH.md: FETCH_SIZE counts its hits too) --
        # not an HBM-bandwidth workload.  What binds it is the fabric's rate of random 64-byte requests: the gather calibration
        # (scripts/gather_calib.hip) reaches 3.8 TB/s = 59 G requests/s with this access shape at this footprint.
        # (achieved = the algorithmic bytes, as the contract defines it; the fraction is taken on what reaches the fabric -- the
        # committed PMC pass's FETCH_SIZE + WRITE_SIZE, ~0.88 of the algorithmic bytes: rays of a cohort share lines in L1 / L2)
        fabric_gbs = traffic_bytes / kernel_s / 1e9 if traffic_bytes else alg_gbs
        # the peak in ALGORITHMIC bytes: the calibration's 3.8 TB/s of 64-B lines, times the algorithmic bytes this kernel gets out
        # of a fabric-side byte (1 / 0.88 from the committed PMC pass; 1 without one) -- so that frac = achieved / peak = the share
        # of the fabric's request rate the launch uses (= fabric_side_frac)
        peak_alg = GATHER_CALIB_GBS * (alg_gbs / fabric_gbs if fabric_gbs else 1.0)
        head = {"bound": "fabric_request_rate", "frac": alg_gbs / peak_alg, "peak": peak_alg, "achieved": alg_gbs,
                "unit": "GB/s of algorithmic gather bytes (peak = the 3.8 TB/s random-64-B-request calibration at this footprint x algorithmic bytes per fabric-side byte)"}
        note = ("64 MiB table: lives in the 256 MiB Infinity Cache, so neither this line nor any other in the record is HBM-bandwidth-bound "
                "(FETCH_SIZE includes Infinity-Cache hits); fabric-side reads ~= algorithmic bytes, random 64-B requests, against the "
                "3.8 TB/s the gather calibration (profiles/archive/r01_gather_calib.txt) reaches for this access shape; hbm_algorithmic_frac = the "
                "same bytes over the 8 TB/s HBM peak, kept for comparison with earlier rounds' `frac`.  A table that really leaves the caches "
                "needs > 256 MiB: the `field_hbm` side workload of this line (hashed levels beyond 16 MiB ride the generic gather with 32-bit offsets)")
    else:
        # cache-resident table: HBM is not the binding resource (hbm_algorithmic_frac > 1 is a cache effect, not a fraction of
        # anything).  Candidates: SIMD vector issue, the MFMA pipe, L2 bandwidth -- the largest fraction names the bound.
        cands = {"valu_issue": issued_busy if issued_busy is not None else floor_frac, "mfma": mfma_pipe_frac, "l2": alg_gbs / L2_PEAK_GBS}
        bound = max((v, n) for n, v in cands.items())[1]
        if bound == "valu_issue":
            head = {"bound": "valu_issue", "frac": floor_frac, "peak": ISSUE_PEAK_GCYC, "achieved": floor_gcyc,
                    "unit": "G SIMD issue-cycles/s (algorithmic floor at measured per-class issue costs)"}
        elif bound == "mfma":
            head = {"bound": "mfma", "frac": mfma_pipe_frac, "peak": ISSUE_PEAK_GCYC, "achieved": mfma_pipe_frac * ISSUE_PEAK_GCYC,
                    "unit": "G MFMA-pipe cycles/s"}
        else:
            head = {"bound": "l2", "frac": alg_gbs / L2_PEAK_GBS, "peak": L2_PEAK_GBS, "achieved": alg_gbs, "unit": "GB/s"}
        note = ("17.4 MiB table is L2 / Infinity-Cache resident, so HBM is not the bound (hbm_algorithmic_frac is a cache effect); "
                "the binding resource is SIMD vector issue.  frac = issue cycles the algorithm NEEDS per 64 samples (ISA floor, "
                "each instruction at its MEASURED issue class: 2 / 4 / 8 cycles, MFMA 8; " + ISSUE_RATE_FILE + ") x samples evaluated in "
                "this run / launch time, over 1024 SIMDs x 2.4 GHz.  issue_busy_at_measured_clock = the same for the instructions "
                "actually ISSUED at the clock the launch really held (stamped inside it): the share of SIMD cycles spent issuing")
    roof = {"kernel": "render_queue" + variant.replace("<", "_kernel<", 1)}
    roof.update(head)
    roof.update({
        "traffic": traffic_bytes,  # fabric-side bytes per launch (FETCH_SIZE + WRITE_SIZE of the committed PMC passes, scaled by this run's samples)
        "avg_launch_ms": kernel_s * 1e3,
        "units_per_launch": samples,
        "bytes_per_unit": BYTES_PER_SAMPLE,
        "launches": launches,
        "slot_utilisation": samples / max(1.0, 32.0 * rounds),
        "samples_per_s_in_kernel": samples / kernel_s,
        "shader_clock_ghz_measured": clock if clock > 0.0 else None,
        "issue_busy_at_measured_clock": issued_busy * MAX_CLOCK_HZ / (clock * 1e9) if issued_busy is not None and clock > 0.0 else None,
        "hbm_algorithmic_frac": alg_gbs / HBM_PEAK_GBS,
        "fabric_side_frac": (fabric_gbs / GATHER_CALIB_GBS) if hbm_bound else None,  # what reaches the fabric (PMC bytes of the committed pass) over the calibration
        "mfma_useful_frac": mfma_tflops / MFMA_F16_PEAK_TFLOPS,
        "mfma_pipe_frac": mfma_pipe_frac,
        "profile_matches_binary": bool(cost and cost.get("device_code_sha256") == digest),
        "note": note,
    })
    detail = {
        "kernel": roof["kernel"],
        "wave_rounds_per_launch": rounds,
        "march_avg_launch_ms": prof["march_ms"] / max(1, prof["march_launches"]),
        "algorithmic_gather_GBps": alg_gbs,
        "l2_algorithmic_frac": alg_gbs / L2_PEAK_GBS,
        "mfma_tflops": mfma_tflops,
        "issue_cycles_per_instruction": dict(ISSUE_CYCLES, source=ISSUE_RATE_FILE),
        "floor": dict(floor, frac=floor_frac,
                      mfma_pipe_frac=samples / 64.0 * floor["mfma_per_64_samples"] * 32 / (kernel_s * cycles_per_s),
                      note="instructions the algorithm needs per 64-sample wave iteration (ISA count, DESIGN.md section 3), by issue class"),
        "issued_from_profile": None,
        "this_device_code_sha256": digest,
        "traffic_from_profile": None,
    }
    if cost:
        detail["issued_from_profile"] = {
            "valu_insts_per_round": cost["valu_insts_per_round"], "hot_loop_classes": classes, "issue_cycles_per_64_slot_iteration": issued_cyc_per_iter,
            "issue_busy_at_max_clock": issued_busy, "device_code_sha256": cost.get("device_code_sha256"), "file": ROUND_COST_FILE,
            # what the SIMDs could evaluate if every issue cycle carried this kernel's instruction mix AND every ray slot held a
            # live ray; a leaner kernel RAISES this ceiling, so compare rounds by samples/s, not by a fraction alone
            "issue_bound_samples_per_s": cycles_per_s / (issued_cyc_per_iter / 64.0) if issued_cyc_per_iter else None}
    if clock > 0.0:
        detail["mfma_pipe_frac_at_measured_clock"] = mfma_pipe_frac * MAX_CLOCK_HZ / (clock * 1e9)
        detail["floor"]["frac_at_measured_clock"] = floor_frac * MAX_CLOCK_HZ / (clock * 1e9)
    if traffic:
        detail["traffic_from_profile"] = {"bytes_per_launch": traffic_bytes, "bytes_per_unit": traffic_bytes / samples, "file": TRAFFIC_FILE,
                                          "note": "FETCH_SIZE + WRITE_SIZE of the committed PMC passes scaled by this run's sample count; not measured in this run"}
    return roof, detail


class stdout_to_stderr:
    """RCCL prints a version banner on STDOUT when a communicator is created; rank 0's stdout carries the ONE JSON line,
    so while communicators come up the process's fd 1 points at fd 2"""

    def __enter__(self):
        sys.stdout.flush()
        self.saved = os.dup(1)
        os.dup2(2, 1)

    def __exit__(self, *exc):
        import ctypes

        sys.stdout.flush()
        ctypes.CDLL(None).fflush(None)  # the banner sits in C stdio's buffer (fd 1 is a pipe: fully buffered) until flushed
        os.dup2(self.saved, 1)
        os.close(self.saved)


def comm_up(env, timeout_s=150.0):
    """N > 1: bring up the C ABI's own communicator (prv_comm_create "rccl" -> TCP-star rendezvous + ncclCommInitRank; what
    prv_planner `shard: views` uses) on a watchdog thread: a failure or a hang here is REPORTED, and the ranks then agree
    (over torch.distributed) whether the timed region runs on it or on the torch.distributed fallback."""
    import threading

    api, ctx, rank, world = env["api"], env["ctx"], env["rank"], env["world"]
    result = {"ok": False, "stage": "create", "comm": None}

    def work():
        try:
            comm = api.Comm(ctx, rank, world, transport=os.environ.get("PRV_BENCH_COMM", "rccl"))
            result["comm"] = comm
            result["stage"] = "barrier"
            comm.barrier()
            result["transport"] = comm.transport
            result["stage"] = "done"
            result["ok"] = True
        except Exception as e:  # reported, not raised
            result["error"] = f"{type(e).__name__}: {e}"

    th = threading.Thread(target=work, daemon=True)
    th.start()
    th.join(timeout_s)
    if th.is_alive():
        result["error"] = f"no answer within {timeout_s:.0f} s (stage: {result['stage']})"
        result["hung"] = True
    return result


def full_loop(args):
    """BASELINE configs[4] at size on this GPU: the C++ planner executable on configs/TrainInLoop.yaml semantics -- per
    object 20 rounds of (train a fresh 5-member ensemble 2500 steps on the views chosen so far, render + score the
    remaining candidates of the 144-view set at 80x45 spp 16, EnsembleRGBDensity arg-max; main.cpp:1718-2277), then mode 4:
    the PSNR-vs-#views curve and the stopping criterion's label (NeRF_fit_curve.cpp:119-206).  A child process (the
    planner owns its own HIP context); wall-clock is the metric configs[4] names."""
    import re
    import tempfile

    exe = os.path.join(ROOT, "nerf_prv_amd", "prv_planner")
    if not os.path.exists(exe):
        return {"error": "prv_planner missing: run __graft_entry__.build()"}
    work = tempfile.mkdtemp(prefix="prv_full_loop_")
    # configs/TrainInLoop.yaml trains at the library default = upstream's batch (run.py:185-208 leaves the engine's batch alone:
    # a 2^18-sample target per step under a 2^16-ray cap); --full-loop-small = configs/TrainInLoop_small.yaml, the 4096-ray cap
    # of rounds 1-5 (about 1/6.6 of that batch), labelled as reduced wherever it is reported
    small = bool(getattr(args, "full_loop_small", False))
    cfg_name = "TrainInLoop_small.yaml" if small else "TrainInLoop.yaml"
    cfg = open(os.path.join(ROOT, "configs", cfg_name)).read()
    cfg = re.sub(r'pre_path: "[^"]*"', f'pre_path: "{work}/"', cfg)
    cfg = re.sub(r'model_path: "[^"]*"', f'model_path: "{work}/models/"', cfg)
    cfg = re.sub(r'viewspace_path: "[^"]*"', f'viewspace_path: "{os.path.join(ROOT, "tests", "golden", "hemisphere")}/"', cfg)
    # final evaluation and the curve's test set on the 64-view set (the reference's is its 100-view file, not shipped with
    # this repository); mode 4's curve at n = 3, 6, ..., 30 views + the 64-view upper bound
    cfg += "\nevaluate: 1\nevaluate_views: 64\ncoverage_view_num_max: 30\ncoverage_view_num_add: 3\ncoverage_view_num_full: 64\n"
    if getattr(args, "train_patch", ""):
        pw, ph = (int(x) for x in args.train_patch.split("x"))
        cfg += f"train_patch_w: {pw}\ntrain_patch_h: {ph}\n"

    def cfg_int(key, default):
        m = re.search(rf"^{key}\s*:\s*(\d+)", cfg, re.M)
        return int(m.group(1)) if m else default

    # what the planner will run with: method 3 -> five members (Share_Data.hpp:505-510), method 2 -> two; steps per member and round
    method = cfg_int("method_of_IG", 3)
    n_members = 5 if method == 3 else 2 if method == 2 else cfg_int("ensemble_num", 1)
    n_steps = cfg_int("train_steps", cfg_int("n_steps", 2500))
    path = os.path.join(work, "cfg.yaml")
    with open(path, "w") as fh:
        fh.write(cfg)
    names = [f"object_{k}" for k in range(args.full_loop_objects or (5 if args.full_loop else 1))]
    from nerf_prv_amd import api as _api  # the library's own defaults (no GPU touched: a struct filled by prv_train_default_opts)

    dflt = _api.train_opts()
    rays_cap = cfg_int("train_rays", int(dflt.n_rays))
    out = {"objects": len(names), "rounds_per_object": 20,
           "config": f"configs/{cfg_name} (144-view set, {n_members} members x {n_steps} steps per round, training batch: {int(dflt.target_samples)}-sample "
                     f"target per member-step under a {rays_cap}-ray cap" + (" = REDUCED, about 1/6.6 of upstream's batch" if small else " = the library default = upstream's")
                     + ", candidates 80x45 spp 16, engine stepping rule)",
           "train_rays_cap": rays_cap, "target_samples": int(dflt.target_samples), "training_batch": "reduced" if small else "library default (upstream's)",
           "work_dir": work}
    t_all = time.perf_counter()
    for mode, key in ((21, "view_planning_s"), (4, "psnr_curve_and_stopping_criterion_s")):
        t0 = time.perf_counter()
        # the planner's default exit (ordered shutdown, flush, _exit): its exit code is the planner's own
        r = subprocess.run([exe, path], input=f"{mode}\n" + "\n".join(names) + "\n-1\n", text=True, capture_output=True, timeout=(3600 if args.full_loop else 900),
                           env=dict(os.environ, PRV_PLANNER_TIMING="1"))  # one line per training call on stderr
        out[key] = time.perf_counter() - t0
        if os.environ.get("PRV_BENCH_KEEP_STDERR"):  # dev: the planner's timing lines, one file per mode
            with open(f"{os.environ['PRV_BENCH_KEEP_STDERR']}.mode{mode}.txt", "w") as fh:
                fh.write(r.stderr)
        if r.returncode != 0:
            out["error"] = f"mode {mode} exited {r.returncode}: {(r.stdout + r.stderr)[-400:]}"
            return out
        if mode == 21:
            # "train_members: views V gt G s, fresh F s, create C s, steps S s, total T s": S = prv_train_steps_multi of that
            # round (5 members x 2500 steps side by side)
            steps_s = [float(x) for x in re.findall(r"train_members: .*? steps ([0-9.eE+-]+) s", r.stderr)]
            train_s = [float(x) for x in re.findall(r"train_members: .*? total ([0-9.eE+-]+) s", r.stderr)]
            for key2, word in (("training_ground_truth_s", "gt"), ("training_fresh_models_s", "fresh"), ("training_create_s", "create")):
                vals = [float(x) for x in re.findall(rf"train_members: .*? {word} ([0-9.eE+-]+) s", r.stderr)]
                if vals:
                    out[key2] = sum(vals)  # where a training call's time outside its optimiser steps goes
            score_s = [float(x) for x in re.findall(r"score_round: .*? total ([0-9.eE+-]+) s", r.stderr)]
            if score_s:
                out["scoring_rounds"] = len(score_s)
                out["scoring_s"] = sum(score_s)  # render + score of the remaining candidates, every member (camera json included)
            last = [(int(a), int(b)) for a, b in re.findall(r"train_members: .*?: (\d+) samples, (\d+) rays", r.stderr)]
            if last:  # member 0's last batch of every training call: composited samples and rays cast
                out["samples_per_member_step"] = sum(a for a, _ in last) / len(last)
                out["rays_per_member_step"] = sum(b for _, b in last) / len(last)
            if steps_s:
                out["training_calls"] = len(steps_s)
                out["training_steps_s"] = sum(steps_s)
                out["training_total_s"] = sum(train_s)
                out["members"], out["steps_per_member_and_round"] = n_members, n_steps
                out["member_step_us"] = sum(steps_s) / (len(steps_s) * n_members * n_steps) * 1e6
                out["round_of_5_member_steps_ms"] = sum(steps_s) / (len(steps_s) * n_steps) * 1e3 * 5.0 / n_members
                if last:
                    out["trained_samples_per_s"] = out["samples_per_member_step"] / (out["member_step_us"] * 1e-6)
                if getattr(args, "train_patch", ""):
                    out["train_patch"] = args.train_patch
            chosen = [l for l in r.stdout.splitlines() if l.startswith("chosen_nbvs:")]
            out["views_chosen_last_object"] = [int(x) for x in chosen[-1].split(":")[1].split()] if chosen else None
        else:
            out["labels"] = sum(1 for l in r.stdout.splitlines() if l.startswith("label:"))
    out["wall_clock_s"] = time.perf_counter() - t_all
    out["seconds_per_object"] = out["wall_clock_s"] / max(1, len(names))
    return out


def run_rank(args):
    import numpy as np
    import torch
    import torch.distributed as dist

    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if world != args.gpus:
        raise SystemExit(f"--gpus {args.gpus} but WORLD_SIZE={world}")
    dry = os.environ.get("PRV_BENCH_DRY_RUN") == "1"
    if dry:
        return dry_run(args, rank, world, np, torch, dist)
    # tests only (tests/test_gpu_comm.py): PRV_BENCH_SHARED_GPU=1 runs N ranks on ONE GPU -- RCCL refuses ranks that share a
    # device, so torch.distributed comes up on gloo and the C ABI's communicator on its host-staged socket transport; the
    # code path (comm_up -> unanimous decision -> prv_score_views_sharded in the timed region -> cross-check) is the same
    shared_gpu = os.environ.get("PRV_BENCH_SHARED_GPU") == "1"
    if shared_gpu:
        local_rank = 0
        os.environ.setdefault("PRV_BENCH_COMM", "socket")
    torch.cuda.set_device(local_rank)
    device = torch.device("cuda", local_rank)
    red_device = torch.device("cpu") if shared_gpu else device  # where the small torch.distributed reductions live
    use_dist = world > 1 or os.environ.get("PRV_FORCE_DIST") == "1"  # the latter: exercise RCCL with one rank
    if use_dist:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29511")
        with stdout_to_stderr():
            if shared_gpu:
                dist.init_process_group("gloo", rank=rank, world_size=world)
            else:
                dist.init_process_group("nccl", rank=rank, world_size=world, device_id=device)
            dist.barrier()  # the communicator (and its banner) comes up here, not inside the timed region
            torch.cuda.synchronize()

    from nerf_prv_amd import api, planner

    ctx = api.Context(local_rank)  # raises when libprv_hip.so / the GPU is missing: no fallback
    env = dict(api=api, planner=planner, torch=torch, dist=dist, np=np, ctx=ctx, rank=rank, world=world, device=device,
               use_dist=use_dist, red_device=red_device, gather_device=None if shared_gpu else device)

    # N > 1: the timed region runs the PRODUCT's collective path -- the C ABI's communicator.  Every rank reports whether
    # its side came up; one all-reduce (torch.distributed, its own stream) makes the decision unanimous.
    comm, comm_info, any_hung = None, None, False
    if use_dist:
        with stdout_to_stderr():
            comm_info = comm_up(env)
        flags = torch.tensor([0.0 if comm_info.get("ok") else 1.0, 1.0 if comm_info.get("hung") else 0.0], device=red_device)
        dist.all_reduce(flags, op=dist.ReduceOp.SUM)
        n_failed, n_hung = (int(x) for x in flags.tolist())
        any_hung = n_hung > 0
        if n_failed == 0:
            comm = comm_info["comm"]
        elif comm_info.get("hung"):
            # this rank's context has a thread stuck inside a collective: it is abandoned; the fallback measures on a fresh one
            ctx = api.Context(local_rank)
            env["ctx"] = ctx

    def field_kw(field, scene):
        kw = dict(api.FIELD_256 if field == "256" else api.FIELD_512)
        if scene == "baseline":  # BASELINE.md section 6 literally
            kw.update(table_amp=0.1, density_bias=0.0)
        return kw

    def layout_of(slot):
        lay = ctx.model_layout(slot)
        lay["n_levels"] = lay["n_dense_levels"] + lay["n_hashed_levels"]
        return lay

    def variant_of(slot):
        lay = ctx.model_layout(slot)
        return f"64<{lay['kernel_features']}, {lay['kernel_dense_levels']}>"

    n_views = args.views_per_gpu * world if args.mode == "weak" else args.views_total
    fkw = field_kw(args.field, args.scene)
    main = Round(env, fkw, n_views, args, comm=comm)
    m = main.measure(args.steps, args.warmup)
    k, elapsed = args.steps, m["elapsed"]
    if args.dump_outputs and rank == 0:
        dump_outputs(args.dump_outputs, m["records"], m["order"])

    # cross-check, untimed (--full): the records the product path gathered == the records torch.distributed gathers
    collective = None
    if use_dist:
        same = None
        if comm is not None and args.full:
            other = main.torch_gather_round()
            same = other.tobytes() == m["records"].tobytes()
        collective = {"timed_path": "prv_score_views_sharded on prv_comm (C ABI, " + (comm.transport if comm else "-") + ")" if comm is not None
                      else "torch.distributed all-gather (FALLBACK: the C ABI's communicator did not come up)",
                      "ranks": comm.world if comm is not None else 0, "transport": comm.transport if comm is not None else None,
                      "records_identical_to_torch_gather": same,
                      "error": None if comm is not None else (comm_info or {}).get("error")}

    if collective is not None:
        # ONE RCCL per process: the library file the C ABI's communicator resolved (prv_comm_library) next to every librccl
        # this process has mapped (torch.distributed's "nccl" backend brought its own up first)
        mapped = mapped_rccl()
        lib = comm.library if comm is not None else None
        collective["librccl_mapped"] = mapped
        collective["librccl_prv_comm"] = lib
        collective["one_rccl_per_process"] = (len(mapped) <= 1 and (lib is None or not lib["path"] or not mapped or
                                                                    os.path.realpath(lib["path"]) == os.path.realpath(mapped[0])))

    # BASELINE configs[3] literally, in the SAME multi-GPU run, after the (weak) headline: 1024 candidate views of the
    # synthetic 512^3 field sharded 1024/N per GPU (128 at N = 8), one all-gather of the records per round, at the headline's
    # image size.  Timed like the headline (barriers, max over ranks), on the same communicator.
    config3 = None
    if args.full and world > 1 and not args.no_config3 and not (args.mode == "strong" and args.field == "512" and args.views_total == 1024):
        import threading

        box = {}

        def work3():
            try:
                torch.cuda.set_device(device)  # a new thread starts on device 0: the round's synchronisations must mean THIS rank's GPU
                r3 = Round(env, field_kw("512", args.scene), 1024, args, slots=(2, 3), comm=comm)
                k3 = max(2, min(5, args.steps))
                m3 = r3.measure(k3, 1)
                box["out"] = {
                    "workload": f"BASELINE configs[3]: 1024 hemisphere views sharded {-(-1024 // world)}/GPU over {world} GPUs, {args.width}x{args.height}, "
                                f"{args.samples} samples/ray, synthetic 512^3 field (L=16 F=2 log2T=21), one all-gather of 16-B records per round",
                    "scaling": "strong", "steps": k3, "ms_per_step": m3["elapsed"] / k3 * 1e3,
                    "views_per_s": 1024 * k3 / m3["elapsed"], "value": m3["ev_all"] * k3 / m3["elapsed"], "unit": "ray-samples/s",
                    "views_per_gpu": len(r3.my_ids), "timed_path": collective["timed_path"] if collective else None,
                    "comm_ranks": comm.world if comm is not None else 0,
                    "rccl_ranks": comm.world if comm is not None and comm.transport == "rccl" else 0,
                    "ranking_sha256": hashlib.sha256(np.asarray(m3["order"], np.int32).tobytes()).hexdigest()[:16],
                    "records_sha256": hashlib.sha256(m3["records"].tobytes()).hexdigest()[:16]}
                r3.close()
            except Exception as e:
                box["out"] = {"error": f"{type(e).__name__}: {e}"}

        # on a watchdog like the communicator's bring-up: the headline is measured already, and a rank that hangs (or fails
        # alone) in this side measurement must not cost the run its line -- the line goes out without `config3`, the job
        # then exits non-zero
        limit3 = float(os.environ.get("PRV_BENCH_CONFIG3_TIMEOUT", "240"))
        t_start3 = time.perf_counter()
        th = threading.Thread(target=work3, daemon=True)
        th.start()
        th.join(limit3)
        if th.is_alive():
            config3 = {"error": "no answer within the watchdog's limit"}
            any_hung = True
        else:
            config3 = box.get("out")
            if use_dist:
                # Did every rank get through?  The vote is a collective, and a rank that failed ALONE arrives here while the
                # others still sit in the round's barrier until their watchdog fires (they then skip the vote and leave): the
                # vote runs on a watchdog of its own -- what is left of the round's limit plus a margin -- so that this rank
                # (rank 0 included) still prints its line; the job then exits non-zero like any run with a hung rank.
                vote = {}

                def cast():
                    bad = torch.tensor([1.0 if (config3 is None or "error" in config3) else 0.0], device=red_device)
                    dist.all_reduce(bad, op=dist.ReduceOp.SUM)
                    vote["bad"] = bad.item()

                tv = threading.Thread(target=cast, daemon=True)
                tv.start()
                tv.join(max(0.0, limit3 - (time.perf_counter() - t_start3)) + 30.0)
                if tv.is_alive():
                    any_hung = True
                    if config3 is not None and "error" not in config3:
                        config3 = {"error": "the other ranks never reached the vote on the configs[3] round"}
                elif vote.get("bad", 0) > 0 and config3 is not None and "error" not in config3:
                    config3 = {"error": f"{int(vote['bad'])} rank(s) failed the configs[3] round"}

    extras = {}
    solo_ok = args.full and rank == 0 and world == 1 and not args.no_extras  # side measurements only in the N = 1 run
    if solo_ok:
        solo = dict(env, world=1, rank=0, use_dist=False)
        # (1) the HBM-bound configuration (BASELINE configs[3]'s field) timed in the SAME run
        if args.field == "256":
            r = Round(solo, field_kw("512", args.scene), args.views_per_gpu, args, slots=(2, 3))
            mm = r.measure(max(3, min(10, args.steps)), 2)
            roof512, detail512 = kernel_figures(mm, variant_of(2), True, args.scene, layout_of(2))
            extras["field512"] = {
                "workload": f"{args.views_per_gpu} views {args.width}x{args.height}, synthetic 512^3 field (L=16 F=2 log2T=21, 64 MiB table), scene {args.scene}",
                "value": mm["ev_all"] * mm["steps"] / mm["elapsed"], "unit": "ray-samples/s", "steps": mm["steps"],
                "ms_per_step": mm["elapsed"] / mm["steps"] * 1e3,
                "samples_evaluated_per_step": mm["st"].samples_evaluated,
                "roofline": roof512,
                "roofline_detail": detail512,
            }
            # lifted to top-level keys as well: a parser that keeps only scalars keeps these
            extras["field512_value"] = extras["field512"]["value"]
            extras["field512_frac"] = roof512["frac"]
            extras["field512_avg_launch_ms"] = roof512["avg_launch_ms"]
            r.close()
        # (1b) a table that really leaves the caches (round 6; the 512^3 field's 64 MiB sit in the 256 MiB Infinity Cache): seven
        #      hashed levels of 64 MiB = 448 MiB of random 4-byte gathers.  Render only (no reference images: a second such field is
        #      another gigabyte), 16 views; the roofline that binds THIS one is HBM: every 4-byte entry of a hashed level drags a
        #      64-byte line out of DRAM, so beside the algorithmic fraction the line carries the line-traffic estimate
        if args.field == "256" and not args.no_field_hbm:
            hkw = dict(api.FIELD_HBM)
            if args.scene == "baseline":
                hkw.update(table_amp=0.1, density_bias=0.0)
            ctx.synthetic_model(2, api.L.FieldDesc(**hkw), SEED_A)
            n_hv = min(16, args.views_per_gpu)
            # (a 16-view hemisphere of its own, generated as scripts/kbench.py --field hbm --views 16 generates it: the PMC pass behind
            # `traffic` is of exactly these views)
            htms, hscale, hoffset = planner.hemisphere_transforms(planner.hemisphere_generate(n_hv), 0.3, 0.1, [1e-10] * 3)
            hcams = ctx.cameras_from_matrices(htms, main.fov_x, args.width, args.height, hscale, hoffset)
            hopts = api.render_opts(args.width, args.height, args.samples, 1, 1e-4)
            himg = torch.empty((n_hv, args.height, args.width, 4), dtype=torch.float32, device=device)
            _, hst = ctx.render(2, hcams, None, hopts, out=himg)
            torch.cuda.synchronize()
            ctx.profile_begin()
            t_h = time.perf_counter()
            h_reps = 3
            for _ in range(h_reps):
                ctx.render(2, hcams, None, hopts, out=himg, want_stats=False)
            torch.cuda.synchronize()
            dt_h = (time.perf_counter() - t_h) / h_reps
            hprof = ctx.profile_end()
            lay = ctx.model_layout(2)
            k_s = hprof["render_ms"] * 1e-3 / max(1, hprof["render_launches"])
            alg_gbs = hst.samples_evaluated * BYTES_PER_SAMPLE / k_s / 1e9
            # lines per sample that cannot be cached: 8 corners of every hashed level, each its own 64-byte line (the table is
            # 448 MiB of uniformly hashed entries); the dense levels' lines are shared by neighbouring samples and mostly hit
            line_gbs = hst.samples_evaluated * lay["n_hashed_levels"] * 8 * 64 / k_s / 1e9
            # ... and what the counters say (FETCH_SIZE + WRITE_SIZE of the committed PMC pass of this workload, per sample):
            # neighbouring rays do share lines, even on the coarser hashed levels -- 18 lines per sample, not 56
            tr = (load_json(TRAFFIC_FILE) or {}).get("hbm " + args.scene)
            traffic_bytes = fabric_gbs_h = None
            same_launch = False
            if tr:
                traffic_bytes = (tr["fetch_kib_per_launch"] + tr["write_kib_per_launch"]) * 1024.0 / tr["samples_evaluated_per_launch"] * hst.samples_evaluated
                fabric_gbs_h = traffic_bytes / k_s / 1e9
                same_launch = n_hv == 16 and int(tr["samples_evaluated_per_launch"]) == int(hst.samples_evaluated)  # the PMC pass saw this very launch
            extras["field_hbm"] = {
                "workload": f"{n_hv} views {args.width}x{args.height} x {args.samples} samples, synthetic field L=16 F=2 log2T=24 finest 2048: "
                            f"{lay['n_hashed_levels']} hashed levels of 64 MiB (448 MiB of random gathers; canonical table "
                            f"{lay['table_bytes_canonical'] / 2**20:.0f} MiB), {lay['n_dense_levels']} dense; generic gather with 32-bit offsets; render only",
                "value": hst.samples_evaluated / dt_h, "unit": "ray-samples/s", "steps": h_reps, "ms_per_step": dt_h * 1e3,
                "samples_evaluated_per_step": int(hst.samples_evaluated),
                "roofline": {"kernel": "render_queue64_kernel<2, 0>", "bound": "hbm", "frac": alg_gbs / HBM_PEAK_GBS, "peak": HBM_PEAK_GBS,
                             "achieved": alg_gbs, "unit": "GB/s", "traffic": traffic_bytes, "avg_launch_ms": k_s * 1e3,
                             "memory_side_GBps": fabric_gbs_h, "traffic_is_of_this_launch": bool(tr) and same_launch, "memory_side_frac_of_peak": fabric_gbs_h / HBM_PEAK_GBS if fabric_gbs_h else None,
                             "memory_side_frac_of_achievable": fabric_gbs_h / HBM_ACHIEVABLE_GBS if fabric_gbs_h else None,
                             "memory_side_frac_of_random_request_calibration": fabric_gbs_h / 3600.0 if fabric_gbs_h else None,
                             "units_per_launch": float(hst.samples_evaluated), "bytes_per_unit": BYTES_PER_SAMPLE,
                             "line_traffic_estimate_GBps": line_gbs, "line_traffic_frac_of_peak": line_gbs / HBM_PEAK_GBS,
                             "line_traffic_frac_of_achievable": line_gbs / HBM_ACHIEVABLE_GBS,
                             "note": "the one workload of the record whose table (448 MiB of hashed levels) exceeds the 256 MiB Infinity Cache: HBM-bound.  "
                                     "frac = algorithmic gather bytes (512 B per sample) over the 8 TB/s peak; what the memory side moves is a 64-byte "
                                     "line per 4-byte entry: memory_side_* = FETCH_SIZE + WRITE_SIZE of the committed PMC pass (1,176 B = 18 lines per "
                                     "sample: neighbouring rays share lines even on the hashed levels; L2 hit 9 %) over the 8 TB/s peak, the guide's 6.3 "
                                     "TB/s achievable, and the 3.3-3.6 TB/s the random-64-B-request calibration reaches at 1-4 GiB footprints "
                                     "(profiles/archive/r01_gather_calib.txt) -- that last one, not the sequential peak, is this access shape's ceiling; "
                                     "line_traffic_* = the no-sharing estimate (7 levels x 8 corners x 64 B per sample)"}}
            extras["field_hbm_value"] = extras["field_hbm"]["value"]
            extras["field_hbm_frac"] = alg_gbs / HBM_PEAK_GBS
            extras["field_hbm_memory_side_frac"] = fabric_gbs_h / HBM_PEAK_GBS if fabric_gbs_h else None
            hcams.close()
            del himg
            ctx.synthetic_model(2, api.L.FieldDesc(**field_kw(args.field, args.scene)), SEED_A)  # (the slot gives the gigabyte back)
        # (2) the other scene: dense (table U(-4,4), density bias 3: an opaque object, rays terminate early) when the
        #     headline is BASELINE.md section 6's nearly transparent one, and the other way round
        other = "dense" if args.scene == "baseline" else "baseline"
        r = Round(solo, field_kw(args.field, other), args.views_per_gpu, args, slots=(2, 3))
        mm = r.measure(args.steps, 2)  # as many steps as the headline: a 5-step figure carried 0.2 ms of warm-up in round 3
        extras["scene_" + other] = {
            "workload": f"{args.views_per_gpu} views, " + ("table U(-4,4), density_bias 3 (opaque object, early termination)" if other == "dense"
                                                        else "table U(-0.1,0.1), density_bias 0 (BASELINE.md section 6)"),
            "value": mm["ev_all"] * mm["steps"] / mm["elapsed"], "unit": "ray-samples/s", "steps": mm["steps"],
            "ms_per_step": mm["elapsed"] / mm["steps"] * 1e3,
            "samples_evaluated_per_step": mm["st"].samples_evaluated,
            "samples_per_ray": mm["st"].samples_evaluated / max(1, mm["st"].rays),
        }
        extras["scene_" + other]["roofline"], extras["scene_" + other]["roofline_detail"] = kernel_figures(
            mm, variant_of(2), args.field == "512", other, layout_of(2))
        # where a step of this scene goes, kernel by kernel (HIP events on the launch stream) -- the round-3 verdict asked what
        # the 0.3 ms between the render launch and the step were
        pr = mm["prof"]
        extras["scene_" + other]["step_breakdown_ms"] = {
            "render": pr["render_ms"] / mm["steps"], "march": pr["march_ms"] / mm["steps"],
            "everything_else": mm["elapsed"] / mm["steps"] * 1e3 - (pr["render_ms"] + pr["march_ms"]) / mm["steps"],
            "note": "everything_else = PSNR / coverage reduce (~0.2 ms), record gather + finalize, launch gaps, host time per step"}
        r.close()
        # (3) the reference's OWN scoring round: 540 candidates at 80x45, spp 16, 5 members, EnsembleRGBDensity
        #     (main.cpp:1796-1806, run.py:48,304, Share_Data.hpp:505-510), in both stepping rules
        extras["reference_round"] = reference_round(env, field_kw(args.field, "dense"), layout_of, variant_of, args)
        # (4) the headline's views under the engine's own stepping rule
        extras["ngp_step"] = ngp_step_round(solo, fkw, args, layout_of, variant_of)

    # BASELINE config 1 analogue (the reference's CPU render path, main.cpp:98-284): first occupied voxel
    # per ray over the same views; GPU (prv_first_hit) here, the oracle's scalar DDA in cpu_baseline
    first_hit = None
    if solo_ok:
        cells = ctx.first_hit(0, main.cams, main.my_ids, args.width, args.height)
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        for _ in range(5):
            cells = ctx.first_hit(0, main.cams, main.my_ids, args.width, args.height)
        torch.cuda.synchronize()
        dt_fh = (time.perf_counter() - t1) / 5
        first_hit = {"gpu_rays_per_s": len(main.my_ids) * args.width * args.height / dt_fh,
                     "hit_fraction": float((cells >= 0).float().mean().item())}

    # the other half of an NBV iteration: in-process training of the field (run.py:185-208), outside the timed
    # region and not part of `value`: a fresh field trained on this rank's reference images
    training = None
    if args.full and rank == 0 and world == 1 and not args.no_training:
        tcams = ctx.cameras_from_matrices(np.asarray(main.tms)[main.my_ids], main.fov_x, args.width, args.height, main.scale,
                                          main.offset)
        ctx.synthetic_model(5, api.L.FieldDesc(**field_kw(args.field, "dense")), SEED_B)  # an opaque object to learn
        u8, _ = ctx.render_rgba8(5, tcams, None, api.render_opts(args.width, args.height, args.samples, 1, 1e-4,
                                                                background=(0, 0, 0, 0)))
        tdesc = api.L.FieldDesc(**dict(fkw, table_amp=1e-4, density_bias=0.0))

        def train_rate(rule):
            """a fresh field, 300 warm-up steps untimed (past the all-occupied start), then args.train_steps timed"""
            ctx.fresh_model(4, tdesc, 0x1234)
            tr = api.Trainer(ctx, 4, tcams, u8, api.train_opts(step_mode=api.L.STEP_NGP if rule == "ngp" else api.L.STEP_FIXED_S))
            tr.steps(300)
            torch.cuda.synchronize()
            t2 = time.perf_counter()
            losses = tr.steps(args.train_steps)
            torch.cuda.synchronize()
            dt_tr = time.perf_counter() - t2
            used = tr.info()["samples_last"]
            rate = used * args.train_steps / dt_tr
            res = {"sampling_rule": "PRV_STEP_NGP: the engine's marcher, dt = sqrt(3)/1024, per-ray random start (upstream's; the default)" if rule == "ngp"
                                    else "PRV_STEP_FIXED_S: 128 jittered uniform samples between the AABB hits (rounds 1-5)",
                   "steps_per_s": args.train_steps / dt_tr, "ms_per_step": dt_tr / args.train_steps * 1e3, "samples_per_s": rate,
                   "rays_per_step_cap": int(tr.opts.n_rays), "target_samples_per_step": int(tr.opts.target_samples),
                   "active_rays_last_batch": tr.info()["active_rays"], "steps_per_ray_cap": int(tr.opts.n_samples),
                   "used_samples_last_batch": used, "loss_last": float(losses[-1]),
                   "atomic_bound": {"bound": "memory-side atomic requests (table-gradient adds)", "peak_g_requests_per_s": ATOMIC_REQ_PEAK_G,
                                    "peak_source": ATOMIC_RATE_FILE, "requests_per_sample_from_profile": ATOMIC_REQ_PER_SAMPLE[rule],
                                    "requests_source": ATOMIC_REQ_FILE + " (section 1: TCC_EA0_ATOMIC of the backward launch at this batch, this rule)",
                                    "frac": rate * ATOMIC_REQ_PER_SAMPLE[rule] / (ATOMIC_REQ_PEAK_G * 1e9)}}
            tr.close()
            return res

        training = train_rate("ngp" if api.train_opts().step_mode == api.L.STEP_NGP else "fixed")
        training["note"] = ("fresh field; batch adapts to ~2^18 composited samples per step (upstream's batch); f16-MFMA forward (activations kept), backward dX chain "
                            "and dW on bf16-split MFMAs, merging table scatter, sparse Adam; samples_per_s uses the last batch's count.  Under the engine's "
                            "marcher the backward launch of a trainer alone takes 0.18 ms against 0.125 ms for its 2.6 M requests at the memory side's rate "
                            "(its blocks' own work is 0.09 ms; five members side by side run it at the request rate), under the fixed rule the request "
                            "rate binds outright (profiles/r06_train_rules.txt, sections 4 and 10)")
        training["fixed_rule"] = train_rate("fixed")
        tcams.close()

    if rank == 0:
        roof, roof_detail = kernel_figures(m, variant_of(0), args.field == "512", args.scene, layout_of(0))
        scene_words = ("BASELINE.md section 6 scene: table U(-0.1,0.1), Xavier MLPs, no density bias, analytic occupancy (4 spheres)"
                       if args.scene == "baseline" else "dense scene: table U(-4,4), density bias 3, analytic occupancy (4 spheres)")
        cpu = None
        if args.full and not args.no_cpu_baseline and world == 1:  # reported at N=1 only
            cpu = cpu_baseline(args, fkw, main.tms, main.scale, main.offset, main.fov_x)
        loop = None
        if args.full and world == 1 and not args.no_full_loop and not args.no_extras:
            try:
                loop = full_loop(args)
            except Exception as e:  # the side measurement must never cost the run its line
                loop = {"error": f"{type(e).__name__}: {e}"}
        out = {
            # scene in the metric's name: round 3 switched the default scene, and lines of different scenes do not compare
            "metric": f"ray-samples/s (field evaluations composited; candidate views rendered + scored; scene {args.scene}, field {args.field}^3)",
            "value": m["ev_all"] * k / elapsed,
            "unit": "ray-samples/s",
            "n_gpus": world,
            "steps": k,
            "warmup": args.warmup,
            "ms_per_step": elapsed / k * 1e3,
            "higher_is_better": True,
            "scaling": args.mode,
            "vs_baseline": None,
            "dtype": "f16",
            "data": "synthetic",
            "config": {
                "workload": f"render+score {len(main.my_ids)} hemisphere views/GPU, {args.width}x{args.height}, "
                            f"{args.samples} samples/ray, synthetic {args.field}^3 hash-grid field "
                            f"(L={fkw['n_levels']} F={fkw['n_features']} log2T={fkw['log2_hashmap']}; {scene_words}), "
                            "PSNR+coverage score vs resident reference images",
                "scene": args.scene,
                "samples_per_ray": args.samples,
                "views_total": n_views,
                "parallelism": (f"views sharded {args.views_per_gpu}/GPU" if args.mode == "weak" else
                                f"{n_views} views sharded over {world} GPUs") + ", interleaved; one all-gather of 16-B records",
            },
            "roofline": roof,
            "cpu_baseline": cpu,
        }
        # scalars a parser that drops nested objects still keeps
        lifted = {"roofline_frac": roof["frac"], "roofline_bound": roof["bound"]}
        for key in ("field512_value", "field512_frac", "field512_avg_launch_ms", "field_hbm_value", "field_hbm_frac", "field_hbm_memory_side_frac"):
            if key in extras:
                lifted[key] = extras.pop(key)
        rr = extras.get("reference_round")
        if rr:
            lifted.update({"reference_round_ms": rr["ngp_step"]["ms_per_round"], "reference_round_views_per_s": rr["ngp_step"]["views_per_s"],
                           })
            if "fixed_128" in rr:
                lifted["reference_round_fixed_128_ms"] = rr["fixed_128"]["ms_per_round"]
        if extras.get("ngp_step"):
            lifted["ngp_step_samples_per_s"] = extras["ngp_step"]["value"]
        if training:
            lifted["training_steps_per_s"] = training["steps_per_s"]
            lifted["training_samples_per_s"] = training["samples_per_s"]
        if config3 and "views_per_s" in config3:
            lifted["config3_views_per_s"] = config3["views_per_s"]
            lifted["config3_ms_per_step"] = config3["ms_per_step"]
        if loop and "seconds_per_object" in loop:
            lifted["full_loop_s_per_object"] = loop["seconds_per_object"]
            lifted["full_loop_member_step_us"] = loop.get("member_step_us")
            lifted["full_loop_training_batch"] = loop.get("training_batch")
            lifted["full_loop_samples_per_member_step"] = loop.get("samples_per_member_step")
            lifted["full_loop_trained_samples_per_s"] = loop.get("trained_samples_per_s")
        out.update(lifted)
        out.update({
            "dtype_note": "fp16 table, blend and MLP operands (MFMA f16 -> f32 accumulate); f32 rays, positions, compositing",
            "parity": "vs own CPU oracle (oracle/), unpinned: the reference's render arithmetic lives in instant-ngp, absent from its tree; "
                      "this workload is gated whole view by whole view in tests/test_gpu_wholeview.py",
            "rccl_ranks": (comm.world if comm is not None and comm.transport == "rccl" else (world if use_dist and comm is None and not shared_gpu else 0)),
            "comm_ranks": comm.world if comm is not None else 0,  # prv_comm_world of the communicator the timed region ran on
            "collective": collective,
            "nominal_ray_samples_per_s": m["nom_all"] * k / elapsed,
            "rays_per_s": m["rays_all"] * k / elapsed,
            "views_scored_per_s": n_views * k / elapsed,
            "samples_evaluated_per_step_per_gpu": m["st"].samples_evaluated,
            "samples_live_per_step_per_gpu": m["st"].samples_live,
            "samples_nominal_per_step_per_gpu": m["st"].samples_nominal,
            "evaluated_samples_per_ray": m["st"].samples_evaluated / max(1, m["st"].rays),
            "ranking_head": [int(x) for x in m["order"][:8]],
            "ranking_sha256": hashlib.sha256(np.asarray(m["order"], np.int32).tobytes()).hexdigest()[:16],  # the WHOLE integer ranking
            "records_sha256": hashlib.sha256(m["records"].tobytes()).hexdigest()[:16],  # every gathered 16-byte record of the last step
            "roofline_detail": roof_detail,
            "first_hit": first_hit,
            "training": training,
        })
        out.update(extras)
        if config3 is not None:
            out["config3"] = config3
        if loop is not None:
            out["full_loop"] = loop
        if cpu is None:
            del out["cpu_baseline"]
        print(json.dumps(out), flush=True)
    if any_hung:
        # a rank has a thread stuck inside a collective on an abandoned context: the line (measured on the fallback) is out;
        # nobody enters another barrier, and the job does not pretend to have ended cleanly
        sys.stdout.flush()
        sys.stderr.flush()
        os._exit(3)
    if comm is not None:
        comm.barrier()
        comm.close()
    if use_dist:
        dist.barrier()
        dist.destroy_process_group()
    main.close()
    ctx.close()
    return 0


def reference_round(env, fkw, layout_of, variant_of, args):
    """the reference's own scoring round on this GPU: 540 candidate views at 80x45, 16 sub-samples per pixel, a 5-member
    ensemble, EnsembleRGBDensity -- once with 128 uniform samples per ray, once with the engine's stepping rule; each with
    its own roofline of the render launches (one per member), measured in the run like the headline's"""
    api, planner, torch, np, ctx = env["api"], env["planner"], env["torch"], env["np"], env["ctx"]
    n_views, members = 540, 5
    desc = api.L.FieldDesc(**fkw)
    for e in range(members):
        ctx.synthetic_model(2 + e, desc, SEED_A + 16 + e)
    pts = planner.hemisphere_generate(n_views)
    fov_x = 2.0 * np.arctan(0.5 * 1280 / 915.60668945312500)
    tms, scale, offset = planner.hemisphere_transforms(pts, 0.3, 0.1, [1e-10] * 3)
    cams = ctx.cameras_from_matrices(tms, fov_x, 80, 45, scale, offset)
    slots = list(range(2, 2 + members))
    out = {"workload": "540 views x 80x45 x 16 spp x 5 members, EnsembleRGBDensity (main.cpp:1796-1806, 2099-2161; run.py:48,304), min_T 0.01"}
    reps = 5

    def per_member(prof, opts):
        """one render launch per member and round: its mean duration over the timed rounds, beside what that member's field makes
        a ray do -- samples evaluated before termination (a render of the member alone, untimed) -- and the rate the two give.
        The members are five different random fields behind ONE occupancy grid: their rays march the same steps and stop at
        different depths, which is the whole spread of the launch durations"""
        ms = prof.get("render_launch_ms") or []
        out_m = []
        for e in range(members):
            _, st_e = ctx.render(slots[e], cams, None, opts)
            mine = ms[e::members] if len(ms) == members * reps else []
            row = {"member": e, "samples_evaluated": int(st_e.samples_evaluated), "samples_live": int(st_e.samples_live)}
            if mine:
                row["launch_ms"] = sum(mine) / len(mine)
                row["samples_per_s_in_kernel"] = st_e.samples_evaluated / (row["launch_ms"] * 1e-3)
            out_m.append(row)
        return out_m

    # (the round with 128 uniform samples per ray is NOT the reference's rule -- it renders with the engine's stepping -- and left
    # the default line in round 6: --reference-round-fixed brings it back)
    for name, spr in ((("fixed_128", 128),) if args.reference_round_fixed else ()) + (("ngp_step", 0),):
        opts = api.engine_render_opts(80, 45, spr, 16, 0.01, background=(0, 0, 0, 1))
        rec, st = ctx.score_views(api.L.SCORE_ENSEMBLE_RGB_DENSITY, slots, cams, None, opts, want_stats=True)
        torch.cuda.synchronize()
        ctx.profile_begin()
        t0 = time.perf_counter()
        for _ in range(reps):
            rec, _ = ctx.score_views(api.L.SCORE_ENSEMBLE_RGB_DENSITY, slots, cams, None, opts)
        torch.cuda.synchronize()
        dt = (time.perf_counter() - t0) / reps
        prof = ctx.profile_end()
        prof["clock_ghz"] = ctx.render_clock_ghz()
        # st counts the whole round (all members); a "step" of the figures below is one round
        m = {"prof": prof, "st": st, "steps": reps}
        roof, _ = kernel_figures(m, variant_of(2), False, "dense", layout_of(2))
        out[name] = {"ms_per_round": dt * 1e3, "views_per_s": n_views / dt, "ray_samples_per_s": st.samples_evaluated / dt,
                     "evaluated_samples_per_ray": st.samples_evaluated / max(1, st.rays), "live_samples_per_ray": st.samples_live / max(1, st.rays),
                     "render_ms_per_round": prof["render_ms"] / reps, "march_ms_per_round": prof["march_ms"] / reps,
                     "render_launches_per_round": prof["render_launches"] // reps,
                     "per_member": per_member(prof, opts),
                     "best_view": int(ctx.argmax(rec, np.arange(n_views))),
                     "roofline": {k: roof[k] for k in ("kernel", "bound", "frac", "peak", "achieved", "unit", "avg_launch_ms", "units_per_launch",
                                                       "slot_utilisation", "samples_per_s_in_kernel", "shader_clock_ghz_measured")}}
    if "fixed_128" in out:
        out["fixed_128"]["note"] = ("not the reference's rule (it renders with the engine's stepping: ngp_step).  Slot utilisation stays ~0.68 here by "
                                "MEASUREMENT: relocation (tail merge + pool) lifts it to 0.92 and makes this round slower, 46.4 -> 48.8 ms -- 128 uniform "
                                "samples share no cell, so the corner cache that pays for relocation under the engine's rule has nothing to keep "
                                "(profiles/r05_march_multi.txt)")
    out["ngp_step"]["note"] = ("the five members' rays are marched in ONE launch (march_multi_kernel: one occupancy walk per ray answers every member), "
                               "then one render launch per member; per_member: each launch's mean duration beside the samples that member's field makes "
                               "the rays evaluate -- the members are random fields behind one occupancy grid, their rays stop at different depths: the "
                               "launches' spread is the spread of evaluated samples (DESIGN.md section 10, row 2: why the five launches were not fused)")
    cams.close()
    return out


def ngp_step_round(env, fkw, args, layout_of, variant_of):
    """the headline's 64 views at 800x800 under the ENGINE's stepping rule (dt = sqrt(3)/1024, every step tested against
    the occupancy grid, no per-ray cap; what run.py:245-247, 304 render with): render only, samples/s over wall time"""
    api, planner, torch, np, ctx = env["api"], env["planner"], env["torch"], env["np"], env["ctx"]
    ctx.synthetic_model(2, api.L.FieldDesc(**fkw), SEED_A)
    pts = planner.hemisphere_generate(args.views_per_gpu)
    fov_x = 2.0 * np.arctan(0.5 * 1280 / 915.60668945312500)
    tms, scale, offset = planner.hemisphere_transforms(pts, 0.3, 0.1, [1e-10] * 3)
    cams = ctx.cameras_from_matrices(tms, fov_x, args.width, args.height, scale, offset)
    opts = api.engine_render_opts(args.width, args.height, 0, 1, 1e-4)
    out_img = torch.empty((args.views_per_gpu, args.height, args.width, 4), dtype=torch.float32, device=env["device"])
    _, st = ctx.render(2, cams, None, opts, out=out_img)
    torch.cuda.synchronize()
    reps = 3
    ctx.profile_begin()
    t0 = time.perf_counter()
    for _ in range(reps):
        ctx.render(2, cams, None, opts, out=out_img, want_stats=False)
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) / reps
    prof = ctx.profile_end()
    prof["clock_ghz"] = ctx.render_clock_ghz()
    roof, _ = kernel_figures({"prof": prof, "st": st, "steps": reps}, variant_of(2), args.field == "512", args.scene, layout_of(2))
    cams.close()
    return {"workload": f"{args.views_per_gpu} views {args.width}x{args.height}, engine stepping rule (PRV_STEP_NGP), scene {args.scene}, render only",
            "value": st.samples_evaluated / dt, "unit": "ray-samples/s", "ms_per_render": dt * 1e3,
            "samples_evaluated": st.samples_evaluated, "samples_live_march_count": st.samples_live,
            "evaluated_samples_per_ray": st.samples_evaluated / max(1, st.rays),
            "roofline": {k: roof[k] for k in ("kernel", "bound", "frac", "avg_launch_ms", "units_per_launch", "slot_utilisation",
                                              "samples_per_s_in_kernel", "shader_clock_ghz_measured")}}


def dry_run(args, rank, world, np, torch, dist):
    """PRV_BENCH_DRY_RUN=1 (tests only): launcher -> rendezvous (gloo) -> shard -> gather -> identical ranking, with
    records that are a fixed function of the view id.  No GPU, no field, NO performance figure: value is null."""
    from nerf_prv_amd import api, planner

    if world > 1:
        dist.init_process_group("gloo", rank=rank, world_size=world)
    n_views = args.views_per_gpu * world if args.mode == "weak" else args.views_total
    ids, per = planner.shard_views(n_views, rank, world, interleaved=True)
    rec = np.zeros(len(ids), api.RECORD_DTYPE)
    rec["score"] = np.sin(ids.astype(np.float64) * 12.9898) * 43758.5453 % 1.0
    records = planner.gather_records(rec, per, n_views, interleaved=True)
    order = api.rank_host(records, np.arange(n_views, dtype=np.int32))
    digest = torch.tensor([int(np.frombuffer(records.tobytes(), np.uint8).astype(np.int64).sum()), int(order[0])])
    if world > 1:
        all_d = [torch.zeros_like(digest) for _ in range(world)]
        dist.all_gather(all_d, digest)
        assert all(bool((d == digest).all()) for d in all_d), "ranks disagree on the gathered records"
    config3 = None
    if args.full and world > 1 and not args.no_config3:  # the shape of the sub-object the real N > 1 run adds (with --full): configs[3]'s 1024 views, strong
        ids3, per3 = planner.shard_views(1024, rank, world, interleaved=True)
        rec3 = np.zeros(len(ids3), api.RECORD_DTYPE)
        rec3["score"] = np.sin(ids3.astype(np.float64) * 12.9898) * 43758.5453 % 1.0
        records3 = planner.gather_records(rec3, per3, 1024, interleaved=True)
        order3 = api.rank_host(records3, np.arange(1024, dtype=np.int32))
        config3 = {"scaling": "strong", "views_per_gpu": int(len(ids3)), "comm_ranks": world,
                   "records_checksum": int(np.frombuffer(records3.tobytes(), np.uint8).astype(np.int64).sum()),
                   "ranking_head": [int(x) for x in order3[:8]]}
    if rank == 0:
        print(json.dumps({"metric": "dry run (no GPU work, no performance figure)", "value": None, "dry_run": True, "n_gpus": world,
                          "scaling": args.mode, "views_total": n_views, "ranking_head": [int(x) for x in order[:8]],
                          "records_checksum": int(digest[0]), "config3": config3}), flush=True)
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()
    return 0


def main():
    argv = sys.argv[1:]
    args = parse_args(argv)
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        sys.exit(launch_ranks(args, argv))  # before anything touches a GPU
    rc = run_rank(args)
    # Everything is closed and the line is out.  The process leaves through an ordinary interpreter exit, so that every
    # exit handler runs -- a profiler's, or whatever else the host installed to record what the run loaded and did; an
    # _exit skips them all, and with them the record that this run executed the library's native code.  The price is the
    # rare crash profiles/NOTES.md ("prv_planner's exit") traces to the HIP runtime's own exit-time teardown, after the
    # line is out ("a host that must run its own exit handlers").  PRV_BENCH_EXIT=quick is
    # PRV_PLANNER_EXIT=quick's counterpart for a host that records nothing at exit and scores runs by exit code: flush,
    # then _exit.
    sys.stdout.flush()
    sys.stderr.flush()
    if os.environ.get("PRV_BENCH_EXIT") == "quick":
        os._exit(rc)
    sys.exit(rc)


if __name__ == "__main__":
    main()
