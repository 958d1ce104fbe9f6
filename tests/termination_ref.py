"""CPU reference of the termination render and of the Jensen-Shannon view score (test infrastructure, in the manner of
tests/entropy_ref.py and tests/surface_ref.py).

The histogram (prv_render_termination, include/prv.h), a fold over tests/march_ref.py's samples, the one restatement of the
oracle's march:
  * the ray's live samples (i, alpha_i) are march_ref.ray_samples': i is the step index t_i = fmaf(i + 0.5, dt, t0) was formed
    from, the one the kernel forms t from;
  * bin(i) = (i * M) >> 16 in 32-bit unsigned arithmetic, M = floor(K * 65536 / n_max), n_max = S (fixed rule) or 1024;
  * w_i = alpha_i T_i is added to its bin in float32, in depth order; the escape is T_end, alpha = 1 - T_end;
  * per pixel the sub-samples are summed in order, then scaled by 1 / spp (march_ref.mean).
A GPU ray's T differs from this one's by rounding, so a ray whose T lands on min_T may stop one sample apart: `render_variants`
walks the thresholds of util.termination_variants(min_T) in one march.

The score (prv_termination_divergence): `jsd` restates J = H(mean of the members) - mean of the members' H in float64 from
given planes.
"""
import numpy as np

from tests import util
from tests.march_ref import NGP_STEPS, assert_alpha_is_the_oracles, f32, mean, ray_samples, rays

BINS = (4, 8, 16, 32, 64)


def n_max(step_mode, S):
    return NGP_STEPS if step_mode == 1 else int(S)


def bin_mul(K, nmax):
    """M of the bin formula, as the host forms it"""
    return (int(K) * 65536) // int(nmax)


def bin_of(i, K, nmax):
    """the sample's bin: 32-bit unsigned multiply, shift"""
    return ((int(i) * bin_mul(K, nmax)) & 0xFFFFFFFF) >> 16


def histogram(steps, alphas, K, nmax, min_T=0.0):
    """-> (bins [K] float32, T_end, live [K] bool) of a ray whose live samples have these step indices and opacities, in depth order,
    cut at the first sample after which T < min_T; live: the bins a composited sample falls in"""
    bins, live = np.zeros(K, np.float32), np.zeros(K, bool)
    T = f32(1)
    for i, a in zip(steps, alphas):
        a = f32(a)
        b = bin_of(i, K, nmax)
        bins[b] = f32(bins[b] + f32(a * T))
        live[b] = True
        T = f32(T * (f32(1) - a))
        if T < f32(min_T):
            break
    return bins, T, live


def render_variants(lib, field, cam, w, h, K, min_Ts, S=128, spp=1, step_mode=0):
    """-> (sub [n, spp, h, w, K + 1] float32 per SUB-SAMPLE and threshold of min_Ts: the K bins, then alpha;
    live [spp, h, w, K] bool: the bins any live sample of the ray falls in, cut or not)"""
    n = len(min_Ts)
    sub = np.zeros((n, spp, h, w, K + 1), np.float32)
    live = np.zeros((spp, h, w, K), bool)
    nmax = n_max(step_mode, S)
    lo = f32(min(min_Ts))
    for k, y, x, o, d in rays(lib, cam, w, h, spp):
        steps, _, alphas, _, _ = ray_samples(lib, field, o, d, step_mode, S, lo)  # the longest of the variants' walks
        for j, mt in enumerate(min_Ts):
            bins, T, lv = histogram(steps, alphas, K, nmax, mt)
            sub[j, k, y, x, :K] = bins
            sub[j, k, y, x, K] = f32(1) - T
            live[k, y, x] |= lv
    return sub, live


def render(lib, field, cam, w, h, K, S=128, spp=1, min_T=1e-4, step_mode=0):
    """-> (h, w, K + 1) float32: the pixel's K bins, then alpha"""
    sub, _ = render_variants(lib, field, cam, w, h, K, [f32(min_T)], S, spp, step_mode)
    return mean(sub[0])


def reference(oracle, f, ocam, w, h, K, S, spp, min_T, mode):
    """-> (variants [3, h, w, K + 1], live [h, w, K]) at the thresholds of util.termination_variants(min_T), for spp sub-samples"""
    sub, live = render_variants(oracle.lib(), f, ocam, w, h, K, [f32(v) for v in util.termination_variants(min_T)], S, spp, mode)
    want = np.stack([mean(sub[j]) for j in range(sub.shape[0])])
    assert_alpha_is_the_oracles(f, ocam, w, h, S, spp, min_T, mode, want[0][..., K])
    return want, live.any(axis=0)


# ---- the Jensen-Shannon divergence, float64, from given planes
def _h64(p):
    p = np.asarray(p, np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(p >= 2.0 ** -126, -p * np.log2(np.where(p > 0, p, 1.0)), 0.0)


def jsd(bins, alphas):
    """bins: [E, K, ...] member histograms, alphas: [E, ...] their opacities -> J [...] float64 in bits:
    H(mean_e p_e) - mean_e H(p_e) over the K bins and the escape 1 - alpha, clamped at 0 as the kernel clamps"""
    bins, alphas = np.asarray(bins, np.float64), np.asarray(alphas, np.float64)
    p = np.concatenate([bins, (1.0 - alphas)[:, None]], axis=1)  # [E, K + 1, ...]
    A = _h64(p.mean(axis=0)).sum(axis=0)
    B = _h64(p).sum(axis=1).mean(axis=0)
    return np.maximum(A - B, 0.0)


def view_scores(bins, alphas):
    """bins [E, K, n, h, w], alphas [E, n, h, w] -> (mean J per view [n], mean opacity over members and pixels per view [n])"""
    J = jsd(bins, alphas)
    return J.reshape(J.shape[0], -1).mean(axis=1), np.asarray(alphas, np.float64).mean(axis=0).reshape(J.shape[0], -1).mean(axis=1)


def hand_made_cases():
    """[(name, bins [E, K, 1, 1, 1], alphas [E, 1, 1, 1], J in bits)]"""
    K = 8

    def planes(rows):  # rows: per member {bin: weight}
        b = np.zeros((len(rows), K, 1, 1, 1), np.float32)
        for e, row in enumerate(rows):
            for k, w in row.items():
                b[e, k] = w
        return b, b.sum(axis=1)

    out = [("identical", *planes([{2: 0.25, 5: 0.5}] * 2), 0.0), ("two opaque members, different bins", *planes([{1: 1.0}, {6: 1.0}]), 1.0),
           # one member stops surely, the other escapes surely: two point masses
           ("one stops, one escapes", *planes([{3: 1.0}, {}]), 1.0),
           # one stops surely, the other half stops there: H((0.75, 0.25)) - 0.5 H((0.5, 0.5))
           ("one stops, one half escapes", *planes([{3: 1.0}, {3: 0.5}]), -(0.75 * np.log2(0.75) + 0.25 * np.log2(0.25)) - 0.5)]
    for E in (3, 5, 8):
        out.append((f"{E} members in {E} bins", *planes([{e: 1.0} for e in range(E)]), float(np.log2(E))))
    return out


# ---- the bar of the reduce kernel against `jsd` ON THE SAME INPUT PLANES (tests/test_gpu_termination.py: random Dirichlet planes,
# E = 2, 3, 5, 8 x K = 4, 16, 64).  The sources of deviation are the hardware log2 and the float32 sums of K + 1 terms, both
# input-dependent.  What they can add up to, term by term:
#   * a sum of K + 1 <= 65 terms h(p) >= 0 that ends at H <= log2(65) = 6.03 bits: every fmaf rounds to half an ulp of a value
#     below 8, 2^-22 / 2 = 2.4e-7 bits, so 65 of them at most 1.6e-5 bits;
#   * the hardware log2 is good to about one ulp of its result, which is at most 126 in magnitude: 2^-17 relative to p's own
#     term, i.e. sum_k p_k * 7.6e-6 <= 7.6e-6 bits for a distribution (the p_k sum to 1);
#   * J = A - mean_e B_e carries A's error and the mean of the B_e's: twice the above, (1.6e-5 + 7.6e-6) * 2 = 4.7e-5 bits, plus
#     the E - 1 adds and the scale of the mean, each half an ulp of a value below 64 (8 members x 6 bits... below 8 after the
#     scale): under 1e-5 together.
# So no input of this kind can deviate by more than about 6e-5 bits.  That is a worst case; the bar is set from what the hardware does.
# MEASURED on the MI355X over the twelve inputs (`TERMINATION_JSD_FIGURES` lines of pytest -s): largest |J_gpu - J_float64| =
# 2.6e-7 ... 4.3e-7 bits at K = 4, 9.1e-7 ... 9.9e-7 at K = 16, 2.2e-6 ... 2.9e-6 at K = 64 (it grows with the number of terms, not
# with E); the largest of all, JSD_MEASURED = 2.898e-6 bits, at E = 5, K = 64.  The bar is four times that, rounded up to one
# digit: 4 x 2.898e-6 = 1.16e-5 -> 2e-5 bits (a third of the worst case above).
JSD_MEASURED = 2.898e-6
JSD_ATOL = 2e-5
