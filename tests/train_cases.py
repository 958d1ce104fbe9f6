"""Inputs of the trainer's edge tests, shared by tests/test_train_cases_host.py (CPU: the oracle alone shows that every input
exercises what it claims) and tests/test_gpu_train_edges.py (the HIP trainer against the oracle on the same inputs).

Three families: camera sets a training test had never seen (inside the cube, axis-parallel, far, looking away, grazing: the cameras of
test_ngp_step_awkward_cameras, as DATASETS), random option sets under the engine's marcher (step caps around the 64-step round,
occupancy grids with no coarse grid and with a partial last word, sparse and single-cell occupancy), and the density refresh's
shapes with a threshold that no cell's density comes near."""
import numpy as np

from tests import util

W, H = 24, 16
SCALE, OFFSET = 5.0, np.array([0.5, 0.5, 0.5])
# tests/test_gpu_train.py: INTR (the GPU module asserts that the two are the same dict)
LENS_INTR = {"fl_x": 20.0, "fl_y": 19.5, "cx": 12.3, "cy": 7.8, "w": W, "h": H, "k1": 0.05, "k2": -0.02, "p1": 0.001, "p2": -0.002}
TINY = dict(n_levels=8, n_features=4, log2_hashmap=10, base_res=4, finest_res=24, occ_res=16, density_bias=1.0, table_amp=0.5)
MLP_LAYERS = ((0, 2048), (2048, 3072), (3072, 5120), (5120, 9216), (9216, 10240))  # tests/test_oracle_train.py's five ranges


def pinhole(fov_x):
    """a principal point in the MIDDLE of pixel (12, 7): that pixel's ray is the camera's axis, exactly"""
    f = float(np.float32(0.5 * W / np.tan(0.5 * fov_x)))
    return {"fl_x": f, "fl_y": f, "cx": 12.5, "cy": 7.5, "w": W, "h": H}


def _tm(rot, t):
    m = np.eye(4)
    m[:3, :3] = rot
    m[:3, 3] = t
    return m


def _ry(a):
    return np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]])


def awkward_datasets(oracle=None):
    """name -> dict(tms [n, 4, 4], intr, scale, offset, seed): the poses of test_ngp_step_awkward_cameras as training sets of 24 x 16
    images.  Every second one has the lens of LENS_INTR, the others are pinhole cameras at the field of view of the render test;
    `mixed` holds one pose of each (a CamSet has one set of intrinsics: the lens).  `seed` is the trainer's: chosen so that the
    oracle's 64-ray batch meets tests/test_train_cases_host.py's conditions (for `axis`: the batch holds the axis pixel itself)."""
    eye, back = np.eye(3), np.diag([-1.0, 1.0, -1.0])
    sets = [("inside", [_tm(eye, [0, 0, 0]), _tm(_ry(0.6), [0, 0, 0])], util.FOV_X),
            ("inside_off_centre", [_tm(_ry(0.6), [0.05, -0.03, 0.06]), _tm(eye, [-0.07, 0.04, 0.02])], util.FOV_X),
            ("axis", [_tm(eye, [0, 0, 0.3])], util.FOV_X),
            ("away", [_tm(back, [0, 0, 0.3])], util.FOV_X),
            ("far", [_tm(eye, [0, 0, 60.0])], 0.006),
            ("corner", [_tm(_ry(0.6), [0.25, 0.07, 0.28])], 0.5),
            ("diag", [_tm(_ry(0.7853981), [0.2, 0.0, 0.2])], 0.3)]
    sets += [(f"graze{i}", [_tm(eye, [0.04 * i, 0.02 * i, 0.3])], 0.6) for i in range(1, 6)]
    lens = {"inside", "away", "corner", "graze1", "graze3", "graze5"}
    out = {}
    for k, (name, tms, fov) in enumerate(sets):
        out[name] = dict(tms=np.stack(tms), intr=dict(LENS_INTR) if name in lens else pinhole(fov), scale=SCALE, offset=OFFSET.copy(),
                         seed=0xA3C0 + k)
    out["axis"]["seed"] = AXIS_SEED
    out["mixed"] = dict(tms=np.stack([tms[0] for _, tms, _ in sets]), intr=dict(LENS_INTR), scale=SCALE, offset=OFFSET.copy(), seed=0xA3F0)
    return out


AXIS_SEED = 0xA3C2
AWKWARD = ["inside", "inside_off_centre", "axis", "away", "far", "corner", "diag"] + [f"graze{i}" for i in range(1, 6)] + ["mixed"]
RULES = {"fixed_s": dict(n_samples=24), "ngp": dict(step_mode=1, n_samples=1024)}
PATCHES = [(4, 2), (1, 3)]


def images(rng, n, h=H, w=W):
    """random bytes with the alpha mix of test_random_training_case: 30 % transparent, 35 % opaque, the rest anything"""
    imgs = rng.integers(0, 256, (n, h, w, 4), dtype=np.uint8)
    imgs[..., 3] = np.where(rng.random((n, h, w)) < 0.3, 0, np.where(rng.random((n, h, w)) < 0.5, 255, imgs[..., 3]))
    return imgs


def sparse_occupancy(rng, shape, occ_res):
    """the AND of two random words (test_random_first_hit_case), the unused bits of the last word zero as everywhere"""
    o = rng.integers(0, 1 << 32, shape, dtype=np.uint32) & rng.integers(0, 1 << 32, shape, dtype=np.uint32)
    return mask_tail(o, occ_res)


def mask_tail(o, occ_res):
    tail = occ_res ** 3 % 32
    if tail:
        o[-1] &= np.uint32((1 << tail) - 1)
    return o


def awkward_field(oracle, name, dense=False):
    """the awkward sets' field: TINY with a quarter of its cells occupied, so that a ray's live mask is ragged in every 64-step round.
    dense (the fixed rule's 24 samples per ray, where a grazing set has few rays that hit the cube at all): three quarters, the OR of
    two random words -- still ragged, and three times the samples"""
    f = oracle.OracleField(oracle.desc(**TINY), seed=util.SEED_A)
    t, m, o = f.params()
    rng = np.random.default_rng(0x0CC + AWKWARD.index(name))
    o = sparse_occupancy(rng, o.shape, TINY["occ_res"])
    if dense:
        o = rng.integers(0, 1 << 32, o.shape, dtype=np.uint32) | rng.integers(0, 1 << 32, o.shape, dtype=np.uint32)
    return oracle.OracleField(f.desc, params=(t, m, o)), (t, m, o)


def awkward_images(name, n):
    return images(np.random.default_rng(0x1A6 + AWKWARD.index(name)), n)


# ------------------------------------------------------------------ random cases under the engine's marcher

N_RANDOM = 16
STEP_CAPS = [1, 63, 64, 65, 200, 1023, 1024]  # around the 64-step ballot round, and the full cap and one less
OCC_RES = [1, 3, 4, 8, 12, 17, 20, 32]
RANDOM_SEED = 0x7EB12  # + case_id; chosen so that the sixteen cases meet tests/test_train_cases_host.py's conditions
SAMPLE_BUDGET = 30000  # samples the oracle lists per batch, about: a case's CPU side stays at a few seconds


def random_ngp_case(case_id):
    """what test_random_training_case draws, under the engine's marcher: a step cap from {1, 63, 64, 65, 200, 1023, 1024}, an
    occupancy resolution from {1, 3, 4, 8, 12, 17, 20, 32} (no coarse grid: 1, 3, 4, 17; coarse grids of 2^3, 3^3, 5^3, 8^3; 1, 27 and 4913
    cells: a partial last word), occupancy all on / sparse / one cell, hemisphere or awkward cameras"""
    rng = np.random.default_rng(RANDOM_SEED + case_id)
    F = int(rng.choice([2, 4]))
    base = int(rng.integers(2, 9))
    kw = dict(n_levels=32 // F, n_features=F, log2_hashmap=int(rng.integers(8, 13)), base_res=base,
              finest_res=int(rng.integers(base + 1, 64)), occ_res=int(rng.choice(OCC_RES)),
              density_bias=float(rng.uniform(0.0, 2.0)), table_amp=float(rng.uniform(0.05, 1.0)))
    cams = str(rng.choice(["hemisphere", "hemisphere"] + [n for n in AWKWARD if n != "away"]))
    if cams == "hemisphere":
        w, h, n_views = int(rng.integers(3, 33)), int(rng.integers(3, 25)), int(rng.integers(1, 7))
        intr = {"fl_x": 0.8 * w, "fl_y": 0.78 * w, "cx": 0.51 * w, "cy": 0.48 * h, "w": w, "h": h,
                "k1": float(rng.uniform(-0.1, 0.1)), "k2": float(rng.uniform(-0.1, 0.1)),
                "p1": float(rng.uniform(-0.005, 0.005)), "p2": float(rng.uniform(-0.005, 0.005))}
        camera = dict(kind="hemisphere", n_views=n_views, intr=intr, predicted_size=float(rng.choice([0.1, 0.3])))
    else:
        w, h = W, H
        camera = dict(kind=cams)
        n_views = len(awkward_datasets()[cams]["tms"])
    occupancy = str(rng.choice(["all", "sparse", "sparse", "cell"]))
    n_samples = int(rng.choice(STEP_CAPS))
    # the two lists are DEALT, not drawn (the draws above keep the stream as it is): sixteen draws from seven caps miss one more often than
    # not.  Case k takes cap k mod 7 and resolution k mod 8 of the lists as RANDOM_SEED shuffles them: every cap at least twice, every
    # resolution twice, in sixteen different pairs
    deal = np.random.default_rng(RANDOM_SEED)
    n_samples = int(deal.permutation(STEP_CAPS)[case_id % len(STEP_CAPS)])
    kw["occ_res"] = int(deal.permutation(OCC_RES)[case_id % len(OCC_RES)])
    # an upper estimate of a ray's listed samples: every step it may take, a quarter of them (and some) in a sparse grid
    per_ray = max(1.0, min(n_samples, 1024) * {"all": 1.0, "sparse": 0.3, "cell": 0.05}[occupancy])
    opts = dict(step_mode=1, n_samples=n_samples, n_rays=int(np.clip(rng.integers(1, 700), 1, max(1, SAMPLE_BUDGET // per_ray))), occ_every=0,
                random_bg=int(rng.integers(0, 2)), min_T=float(rng.choice([0.0, 1e-4, 1e-2])), seed=int(rng.integers(1, 1 << 40)),
                target_samples=int(rng.choice([0, 1 << 18])))
    return dict(id=case_id, field=kw, field_seed=int(rng.integers(1, 1 << 40)), occupancy=occupancy, occ_seed=int(rng.integers(1, 1 << 40)),
                camera=camera, w=w, h=h, n_views=n_views, img_seed=int(rng.integers(1, 1 << 40)), opts=opts)


def realise(oracle, case):
    """a case's arrays: (field parameters (t, m, o), dataset dict(tms, intr, scale, offset), images)"""
    f = oracle.OracleField(oracle.desc(**case["field"]), seed=case["field_seed"])
    t, m, o = f.params()
    R, rng = case["field"]["occ_res"], np.random.default_rng(case["occ_seed"])
    if case["occupancy"] == "all":
        o = mask_tail(np.full_like(o, 0xFFFFFFFF), R)
    elif case["occupancy"] == "sparse":
        o = sparse_occupancy(rng, o.shape, R)
    else:  # one cell, near the middle of the cube, where every camera set looks
        c = [int(np.clip(R // 2 + rng.integers(-1, 2), 0, R - 1)) for _ in range(3)]
        bit = c[0] + R * (c[1] + R * c[2])
        o = np.zeros_like(o)
        o[bit >> 5] = np.uint32(1 << (bit & 31))
    cam = case["camera"]
    if cam["kind"] == "hemisphere":
        tms, scale, offset = util.hemisphere_transforms(oracle, util.fibonacci_hemisphere(cam["n_views"]), predicted_size=cam["predicted_size"])
        ds = dict(tms=tms, intr=cam["intr"], scale=scale, offset=offset)
    else:
        ds = awkward_datasets()[cam["kind"]]
    imgs = images(np.random.default_rng(case["img_seed"]), case["n_views"], case["h"], case["w"])
    return (t, m, o), ds, imgs


def oracle_cameras(oracle, ds):
    return oracle.cameras_from_dataset(ds["tms"], ds["intr"], ds["scale"], ds["offset"])


def rel_l2(a, b):
    return np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30)


def level_ranges(oracle, d):
    """[lo, hi) of every level in the table's scalars"""
    lv, _ = oracle.levels(d)
    return [(int(L.offset) * d.n_features, (int(L.offset) + int(L.size)) * d.n_features) for L in lv]


def block_rel_l2(got, want, ranges):
    """rel_l2 per block, for the blocks whose oracle norm exceeds 1e-3 of the largest block's (a whole-vector norm hides a block that
    is wrong but small); the worst of them, and which"""
    norms = [np.linalg.norm(want[lo:hi]) for lo, hi in ranges]
    worst, at = 0.0, None
    for k, (lo, hi) in enumerate(ranges):
        if norms[k] > 1e-3 * max(norms) and norms[k] > 0:
            e = rel_l2(got[lo:hi], want[lo:hi])
            if e > worst:
                worst, at = e, k
    return worst, at


# ------------------------------------------------------------------ density refresh

REFRESH_FIELD = dict(log2_hashmap=10, base_res=4, finest_res=24, density_bias=1.0, table_amp=2.0)


def refresh_cases():
    """(occ_res, F, PRV_TRAIN_FAST_FWD): 27, 4913 cells -> a partial last word; 12, 20, 32 -> whole words; both refresh kernels
    (the MFMA one by default, the scalar one under PRV_TRAIN_FAST_FWD=0), both template instances"""
    return [(R, F, fast) for R in (3, 12, 17, 20, 32) for F in (4, 2) for fast in (None, "0")]


def refresh_field(oracle, occ_res, F, seed=util.SEED_A):
    """the refresh tests' field: densities spread over two orders of magnitude (table_amp = 2).  It is loaded with ONE occupied cell, in
    a corner: what the render path derives from that grid (coarse grid, occupied box) covers next to nothing, so a render that still
    used it after a refresh would lose nearly all of the refreshed grid's samples.  A refresh writes every word (the EMA starts at 0)."""
    f = oracle.OracleField(oracle.desc(n_levels=32 // F, n_features=F, occ_res=occ_res, **REFRESH_FIELD), seed=seed)
    t, m, o = f.params()
    o = np.zeros_like(o)
    o[0] = 1
    return oracle.OracleField(f.desc, params=(t, m, o)), (t, m, o)


def _dummy_dataset(oracle):
    ds = awkward_datasets()["axis"]
    return oracle_cameras(oracle, ds), np.zeros((1, H, W, 4), np.uint8)


def cell_sigma(oracle, field):
    """the oracle's density at every cell centre (x fastest): a new trainer's EMA starts at 0, so after ONE refresh it is sigma"""
    cams, imgs = _dummy_dataset(oracle)
    tr = oracle.OracleTrainer(field, oracle.train_opts(n_rays=1, n_samples=1, occ_every=0, occ_decay=0.0), cams, imgs)
    tr.refresh_occupancy()
    return tr.ema()


BAND = 1e-4  # no cell's density within this relative distance of the threshold: a hundred times the 1e-6 by which GPU and oracle differ


def place_threshold(sigma, lo=0.2, hi=0.8):
    """a float32 threshold in the middle of the widest gap between neighbouring densities that leaves between lo and hi of the cells on"""
    s = np.sort(sigma.astype(np.float64))
    n = len(s)
    k0, k1 = int(np.ceil((1.0 - hi) * n)), int(np.floor((1.0 - lo) * n))  # s[k] .. s[k + 1]: n - k - 1 cells above
    gaps = s[k0 + 1:k1 + 1] / s[k0:k1]
    k = k0 + int(np.argmax(gaps))
    return float(np.float32(np.sqrt(s[k] * s[k + 1])))


def in_band(values, thresh, rel):
    return np.abs(values.astype(np.float64) - thresh) <= rel * thresh


def bits_of(occ, n_cells):
    return np.unpackbits(np.ascontiguousarray(occ, np.uint32).view(np.uint8), bitorder="little")[:n_cells].astype(bool)


# the EMA case: densities that FALL while training, so that cells stay on through the decayed maximum alone.  lr = 1e-2 moves them
# enough (the oracle ends with some 770 such cells of 4096, 250 of them with an EMA within 5 % above the threshold, where a decay on the
# wrong side of the max would switch them off) while the two trainings stay within delta ~ 1e-3 of each other; at lr = 3e-2 the f32
# atomics' noise grows to delta = 0.12 in 12 steps and the band of 2 delta holds 9 % of the cells: a badly chosen case
EMA_CASE = dict(field=dict(TINY, density_bias=1.0, table_amp=1.0), seed=util.SEED_B, steps=12,
                opts=dict(n_rays=256, n_samples=24, occ_every=2, occ_decay=0.95, lr=1e-2, seed=0xE3A))


def ema_case(oracle):
    """-> (field parameters, dataset, images, train options with the threshold): the scene of tests/test_gpu_train.py (8 hemisphere
    views of a denser field, lens cameras) started from a field that is too dense nearly everywhere"""
    gt = oracle.OracleField(oracle.desc(**dict(TINY, density_bias=3.0, table_amp=2.0)), seed=util.SEED_B)
    tms, scale, offset = util.hemisphere_transforms(oracle, util.fibonacci_hemisphere(8))
    ds = dict(tms=tms, intr=dict(LENS_INTR), scale=scale, offset=offset)
    imgs = np.stack([oracle.quantize_rgba8(gt.render(c, W, H, 32, 1, 1e-4)[0], (0, 0, 0, 0)) for c in oracle_cameras(oracle, ds)])
    f = oracle.OracleField(oracle.desc(**EMA_CASE["field"]), seed=EMA_CASE["seed"])
    t, m, o = f.params()
    o = np.full_like(o, 0xFFFFFFFF)
    return (t, m, o), ds, imgs, dict(EMA_CASE["opts"], occ_sigma_thresh=EMA_THRESH)


EMA_THRESH = 2.0
