"""float64 evaluation of the field's two MLP heads (test infrastructure): the reference against which the oracle's own error
and the GPU's are measured (tests/test_field_cases_host.py, tests/test_gpu_field_regimes.py).

Input: the oracle's bit-exact binary16 features of the positions (OracleField.encode) and the view directions.  Everything after
them is plain double arithmetic: the spherical harmonics, the five layers, ReLU, exp and the logistic function.  The weights are the
binary16 words of the model, read exactly; NOTHING is rounded to binary16 or float32 between the layers (the oracle and the kernels
narrow every hidden layer and the colour head's inputs to binary16), and nothing overflows.

Output layout = prv_debug_field's: [0] sigma, [1:4] rgb, [4:20] density head outputs, [20:36] colour head outputs.
"""
import numpy as np

LAYER_OFFSET = (0, 2048, 3072, 5120, 9216)
LAYER_SHAPE = ((32, 64), (64, 16), (32, 64), (64, 64), (64, 16))
# the output columns the bars are stated for
GROUPS = {"density_out": slice(4, 20), "colour_out": slice(20, 23), "rgb": slice(1, 4)}


def sh4(d):
    """real spherical harmonics, degree 4, of float32 directions -- oracle/prv_oracle.c: orc_sh4's formulas in double"""
    x, y, z = (np.asarray(d, np.float32)[:, k].astype(np.float64) for k in range(3))
    xy, xz, yz, x2, y2, z2 = x * y, x * z, y * z, x * x, y * y, z * z
    return np.stack([
        np.full_like(x, 0.28209479177387814), -0.48860251190291987 * y, 0.48860251190291987 * z, -0.48860251190291987 * x,
        1.0925484305920792 * xy, -1.0925484305920792 * yz, 0.94617469575755997 * z2 - 0.31539156525251999, -1.0925484305920792 * xz,
        0.54627421529603959 * x2 - 0.54627421529603959 * y2, 0.59004358992664352 * y * (-3.0 * x2 + y2), 2.8906114426405538 * xy * z,
        0.45704579946446572 * y * (1.0 - 5.0 * z2), 0.3731763325901154 * z * (5.0 * z2 - 3.0), 0.45704579946446572 * x * (1.0 - 5.0 * z2),
        1.4453057213202769 * z * (x2 - y2), 0.59004358992664352 * x * (-x2 + 3.0 * y2)], axis=1)


def layers(mlp_words):
    w = np.asarray(mlp_words, np.uint16).view(np.float16).astype(np.float64)
    return [w[o:o + i * n].reshape(i, n) for o, (i, n) in zip(LAYER_OFFSET, LAYER_SHAPE)]


def evaluate(features_u16, dirs, mlp_words, density_bias):
    """-> (n, 36) float64"""
    W = layers(mlp_words)
    x = np.asarray(features_u16, np.uint16).view(np.float16).astype(np.float64)
    with np.errstate(over="ignore", invalid="ignore"):
        dens = np.maximum(x @ W[0], 0.0) @ W[1]
        h = np.maximum(np.concatenate([dens, sh4(dirs)], axis=1) @ W[2], 0.0)
        col = np.maximum(h @ W[3], 0.0) @ W[4]
        out = np.zeros((len(x), 36))
        out[:, 0] = np.exp(dens[:, 0] + np.float64(np.float32(density_bias)))
        out[:, 1:4] = 1.0 / (1.0 + np.exp(-col[:, :3]))
    out[:, 4:20], out[:, 20:36] = dens, col
    return out


def column_figures(values, ref, rows=None):
    """per output column: max over the positions (rows: a mask) of |value - ref|, divided by the column's max |ref| -> (36,)"""
    v, r = np.asarray(values, np.float64), np.asarray(ref, np.float64)
    if rows is not None:
        v, r = v[rows], r[rows]
    return np.abs(v - r).max(axis=0) / np.maximum(np.abs(r).max(axis=0), np.finfo(np.float64).tiny)


def group_figures(fig):
    return {g: float(fig[s].max()) for g, s in GROUPS.items()}
