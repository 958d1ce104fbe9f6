"""Parameter regimes for the field kernels (test infrastructure; host code only: numpy and the CPU oracle).

Every other parity test loads what prv_model_synthetic generates: table values uniform in +-table_amp and a random MLP of one
amplitude.  The regimes here are what the product runs on and what binary16 allows:

    fresh      table uniform in +-1e-4 (prv_model_fresh's start): about 60 % of the words are subnormal halfs, and so are the
               weights' products and the partial sums of the blend.  Synthetic MLP, every cell occupied.
    edges      table words drawn, per word and with either sign, from EDGE_WORDS (zero, the smallest and the largest subnormal, the
               smallest normal, one, the largest finite half, and their neighbours), every second word an ordinary +-0.5 value.  The
               draw is by word index over the whole table, so every level, dense or hashed, holds every class and the eight corners
               of a cell mix them.  On every level the eight vertices of the cube's last cell hold +65504 in feature 0 and -65504
               in feature 1: positions there (`corner_positions`) blend eight equal entries under weights whose fp16 products sum a
               hair above 1 for some of them, and the chain ends in +-Inf.
    saturated  synthetic table and MLP; the density head's last-layer column 0 scaled and density_bias set (with the oracle, over
               the positions the tests use) so that the logit out0 + bias has its 1/3 and 2/3 quantiles at -+25 and its tails
               beyond -87.3 (expf leaves the normal floats) and +88.72 (expf overflows).
    wide_mlp   synthetic table and MLP; the first density layer's unit 0 scaled until its activation exceeds 65504, the largest
               finite half, on about one position in twenty (the narrowing between the layers then gives +Inf); the unit's
               outgoing weights are scaled down by 2^-16, so the field stays ordinary wherever the unit stays finite.
    trained    produced on the GPU by tests/test_gpu_field_regimes.py: prv_model_fresh at table_amp = 1e-4 on the shape under test,
               TRAIN_STEPS steps of api.Trainer on `train_scene`, export_model.

No parameter word is Inf or NaN.  What each regime contains is asserted with the oracle alone in tests/test_field_cases_host.py.
"""
import numpy as np

from tests import instances, util

SHAPES = ["F4_5", "F4_3", "F4_0", "F2_10", "F2_6", "F2_0", "F4_all_hashed"]  # one per compiled instance + the all-hashed fallback
HOST_REGIMES = ["fresh", "edges", "saturated", "wide_mlp"]
N_POSITIONS = 3000
TRAIN_STEPS = 250
FRESH_AMP = 1e-4
ORDINARY_AMP = 0.5
WIDE_AMP = 4.0  # wide_mlp's table: the product descriptors' amplitude, so that the scaled weights stay finite halfs
MLP_HALFS = 10240
# MLP layout (oracle/prv_oracle.c: eval_with_sh): layer l is W[k * n_out + o] at LAYER_OFFSET[l]
LAYER_OFFSET = (0, 2048, 3072, 5120, 9216)
LAYER_SHAPE = ((32, 64), (64, 16), (32, 64), (64, 64), (64, 16))
LOGIT_FLUSH, LOGIT_OVERFLOW = -87.3, 88.72

# magnitudes; the sign bit is drawn separately
EDGE_WORDS = np.array([0x0000, 0x0001, 0x0002, 0x03FE, 0x03FF, 0x0400, 0x0401, 0x3BFF, 0x3C00, 0x3C01, 0x7BFE, 0x7BFF], np.uint16)
# class of a magnitude: what the blend does with it differs per class, not per neighbour
EDGE_CLASSES = {"zero": (0x0000,), "min_subnormal": (0x0001, 0x0002), "max_subnormal": (0x03FE, 0x03FF), "min_normal": (0x0400, 0x0401),
                "one": (0x3BFF, 0x3C00, 0x3C01), "max_finite": (0x7BFE, 0x7BFF)}
HALF_MAX = 0x7BFF


class Case:
    """kw: the descriptor's keywords (api.field_desc(**kw) / oracle.desc(**kw)); params: (table u16, mlp u16, occ u32)"""

    def __init__(self, kw, params):
        self.kw, self.params = dict(kw), params


def shape_kw(name):
    return dict(instances.MATRIX[name].kw, table_amp=ORDINARY_AMP, density_bias=3.0)


def _seed(name, regime):
    return 0xF1E1D000 + 16 * SHAPES.index(name) + HOST_REGIMES.index(regime)


def positions(kw):
    """tests/test_gpu_instances.py's positions (random, cube surface, cell boundaries of every level), capped: 1024 random ones,
    the cube's surface, and of the boundary positions every k-th, so that every level keeps its share"""
    rng = np.random.default_rng(41)
    rnd, cube, bnd = rng.random((1024, 3), dtype=np.float32), instances.cube_positions(), instances.boundary_positions(kw, rng)
    room = N_POSITIONS - len(rnd) - len(cube)
    bnd = bnd[np.unique(np.linspace(0, len(bnd) - 1, min(room, len(bnd))).astype(np.int64))]
    return np.ascontiguousarray(np.concatenate([rnd, cube, bnd]))


def corner_positions(kw, per_level=24):
    """per level, positions in the half cell at the cube's corner (1, 1, 1): every axis has floor(scale p + 0.5) >= res - 2"""
    rng = np.random.default_rng(43)
    out = []
    for s, _, _, _ in instances.restated_levels(kw):
        out.append(1.0 - rng.random((per_level, 3)) * (0.5 / float(s)))
    return np.concatenate(out).astype(np.float32)


def directions(n):
    d = np.random.default_rng(42).standard_normal((n, 3)).astype(np.float32)
    return d / np.linalg.norm(d, axis=1, keepdims=True)


# ---- the oracle's table layout, restated (oracle/prv_oracle.c: orc_field_levels, orc_encode)
def level_table(kw):
    """-> [(scale f32, res, hashed, size, offset)], offsets in entries, levels in order"""
    out, off = [], 0
    for s, res, hashed, size in instances.restated_levels(kw):
        out.append((np.float32(s), res, hashed, size, off))
        off += size
    return out


def entry_index(level, cx, cy, cz):
    """table entry (in entries, from the table's start) of vertex (cx, cy, cz), arrays allowed"""
    _, res, hashed, size, off = level
    cx, cy, cz = (np.minimum(np.asarray(c, np.uint64), res - 1) for c in (cx, cy, cz))
    if hashed:
        idx = (cx ^ (cy * np.uint64(2654435761) & np.uint64(0xFFFFFFFF)) ^ (cz * np.uint64(805459861) & np.uint64(0xFFFFFFFF))) & np.uint64(size - 1)
    else:
        idx = cx + res * (cy + res * cz)
    return (idx + np.uint64(off)).astype(np.int64)


def corner_entries(kw, pos):
    """-> (n_levels, n_positions, 8) table entries of the eight corners the gather of every position reads"""
    p = np.clip(np.asarray(pos, np.float32), 0.0, 1.0).astype(np.float64)
    out = []
    for lv in level_table(kw):
        c0 = np.floor((np.float64(lv[0]) * p + 0.5).astype(np.float32)).astype(np.int64)  # fmaf: one rounding of the exact value
        out.append(np.stack([entry_index(lv, c0[:, 0] + (c & 1), c0[:, 1] + ((c >> 1) & 1), c0[:, 2] + (c >> 2)) for c in range(8)], axis=1))
    return np.stack(out)


def half_class(words):
    """class name per EDGE_CLASSES of every word, "ordinary" for the rest"""
    mag = np.asarray(words, np.uint16) & 0x7FFF
    out = np.full(mag.shape, "ordinary", dtype=object)
    for name, ws in EDGE_CLASSES.items():
        out[np.isin(mag, ws)] = name
    return out


def is_subnormal_half(words):
    w = np.asarray(words, np.uint16)
    return ((w & 0x7C00) == 0) & ((w & 0x03FF) != 0)


def is_inf_half(words):
    return (np.asarray(words, np.uint16) & 0x7FFF) == 0x7C00


def all_finite_params(params):
    return all(((np.asarray(a, np.uint16) & 0x7C00) != 0x7C00).all() for a in params[:2])


# ---- the regimes
def _synthetic(oracle, kw, seed):
    f = oracle.OracleField(oracle.desc(**kw), seed=seed)
    params = f.params()
    f.close()
    return params


def fresh(oracle, name):
    kw = dict(shape_kw(name), table_amp=FRESH_AMP)
    table, mlp, occ = _synthetic(oracle, kw, util.SEED_A)
    rng = np.random.default_rng(_seed(name, "fresh"))
    table = rng.uniform(-FRESH_AMP, FRESH_AMP, table.size).astype(np.float32).astype(np.float16).view(np.uint16)
    return Case(kw, (table, mlp, np.full_like(occ, 0xFFFFFFFF)))


def edges(oracle, name):
    kw = shape_kw(name)
    table, mlp, occ = _synthetic(oracle, kw, util.SEED_A)
    rng = np.random.default_rng(_seed(name, "edges"))
    n, F = table.size, kw["n_features"]
    words = EDGE_WORDS[rng.integers(0, len(EDGE_WORDS), n)] | (rng.integers(0, 2, n).astype(np.uint16) << 15)
    ordinary = rng.uniform(-ORDINARY_AMP, ORDINARY_AMP, n).astype(np.float32).astype(np.float16).view(np.uint16)
    table = np.where(rng.integers(0, 2, n) == 1, words, ordinary).astype(np.uint16)
    for lv in level_table(kw):  # the cube's last cell: +65504 in feature 0, -65504 in feature 1
        res = lv[1]
        c = np.array([[res - 2 + (k & 1), res - 2 + ((k >> 1) & 1), res - 2 + (k >> 2)] for k in range(8)])
        e = entry_index(lv, c[:, 0], c[:, 1], c[:, 2])
        table[e * F] = HALF_MAX
        table[e * F + 1] = HALF_MAX | 0x8000
    return Case(kw, (table, mlp, np.full_like(occ, 0xFFFFFFFF)))


def _with_bias(oracle, kw, params):
    return oracle.OracleField(oracle.desc(**kw), params=params)


def saturated(oracle, name):
    kw = shape_kw(name)
    table, mlp, occ = _synthetic(oracle, kw, util.SEED_A)
    pos = positions(kw)
    f = _with_bias(oracle, kw, (table, mlp, occ))
    out0 = f.eval(pos, directions(len(pos)))[0][:, 4].astype(np.float64)
    f.close()
    q1, q2 = np.quantile(out0, [1 / 3, 2 / 3])
    gain = 50.0 / (q2 - q1)
    w = mlp.copy()
    col = LAYER_OFFSET[1] + 16 * np.arange(64)
    scaled = (w[col].view(np.float16).astype(np.float64) * gain).astype(np.float16)
    assert np.isfinite(scaled).all()
    w[col] = scaled.view(np.uint16)
    kw = dict(kw, density_bias=float(np.float32(-25.0 - gain * q1)))
    return Case(kw, (table, w, occ))


def wide_mlp(oracle, name):
    kw = dict(shape_kw(name), table_amp=WIDE_AMP)
    table, mlp, occ = _synthetic(oracle, kw, util.SEED_A)
    pos = positions(kw)
    f = _with_bias(oracle, kw, (table, mlp, occ))
    feat = f.encode(pos).view(np.float16).astype(np.float64)
    f.close()
    w = mlp.copy()
    col = LAYER_OFFSET[0] + 64 * np.arange(32)  # unit 0 of the first density layer
    act = feat @ w[col].view(np.float16).astype(np.float64)
    gain = 65504.0 / np.quantile(act, 0.95)
    scaled = (w[col].view(np.float16).astype(np.float64) * gain).astype(np.float16)
    assert gain > 0 and np.isfinite(scaled).all()
    w[col] = scaled.view(np.uint16)
    row = LAYER_OFFSET[1] + np.arange(16)  # what unit 0 feeds
    w[row] = (w[row].view(np.float16).astype(np.float64) * 2.0 ** -16).astype(np.float16).view(np.uint16)
    return Case(kw, (table, w, occ))


GENERATORS = {"fresh": fresh, "edges": edges, "saturated": saturated, "wide_mlp": wide_mlp}
_cache = {}


def case(oracle, regime, name):
    """the regime on the shape, built once per process"""
    if (regime, name) not in _cache:
        c = GENERATORS[regime](oracle, name)
        assert all_finite_params(c.params)
        _cache[regime, name] = c
    return _cache[regime, name]


def regime_positions(regime, kw):
    """the positions a regime is evaluated at: `positions`, and for `edges` the cube's last cell of every level as well"""
    pos = positions(kw)
    return np.concatenate([pos, corner_positions(kw)]) if regime == "edges" else pos


# ---- the training scene of the `trained` regime: tests/test_gpu_train.py's 24x16 lens scene
def train_scene(oracle):
    """-> (transform matrices, intrinsics, scale, offset, images RGBA8 [8, 16, 24, 4])"""
    from tests.test_gpu_train import INTR, TINY

    gt = oracle.OracleField(oracle.desc(**dict(TINY, density_bias=3.0, table_amp=2.0)), seed=util.SEED_B)
    tms, scale, offset = util.hemisphere_transforms(oracle, util.fibonacci_hemisphere(8))
    ocams = oracle.cameras_from_dataset(tms, INTR, scale, offset)
    imgs = np.stack([oracle.quantize_rgba8(gt.render(c, 24, 16, 32, 1, 1e-4)[0], (0, 0, 0, 0)) for c in ocams])
    gt.close()
    return tms, INTR, scale, offset, imgs
