"""CPU reference of the ray-entropy render (test infrastructure, in the manner of tests/depth_ref.py).

A fold over tests/march_ref.py's samples, the one restatement of the oracle's march, with the entropy sum of
prv_render_entropy (include/prv.h):
  * w_i = alpha_i T_i over exactly the samples, weights and early termination of the colour composite;
  * H = sum_i h(w_i) + h(T_end), h(p) = p >= 2^-126 ? -p log2(p) : 0, accumulated in depth order as H = fmaf(p, -log2 p, H),
    the escape term last; a ray that misses the box or has no live sample gives 0;
  * per pixel the sub-samples summed in order, then scaled by 1 / spp.
log2 is numpy's float32 one.
"""
import numpy as np

from tests.march_ref import assert_alpha_is_the_oracles, composite, f32, fmaf, mean, ray_samples, rays

FLT_MIN = f32(2.0 ** -126)


def h_add(p, H):
    """H + h(p) as the kernel accumulates it"""
    p = f32(p)
    if not p >= FLT_MIN:
        return f32(H)
    return fmaf(p, -f32(np.log2(p)), H)


def entropy_of_alphas(alphas, min_T=0.0):
    """-> (H, T_end) of a ray whose live samples have these opacities, in depth order: the sum march_ray takes, on its own"""
    T, H = f32(1), f32(0)
    for a in alphas:
        a = f32(a)
        H = h_add(f32(a * T), H)
        T = f32(T * (f32(1) - a))
        if T < f32(min_T):
            break
    return h_add(T, H), T


def march_ray(lib, field, o, d, step_mode, S, min_T):
    """-> (r, g, b, a, H) of one ray: the colour composite plus the entropy sum"""
    _, _, alphas, rgbs, _ = ray_samples(lib, field, o, d, step_mode, S, min_T)
    (r, g, b), T = composite(alphas, rgbs, 3)
    if T == f32(1):  # no live sample: exactly 0 (h(1) = 0 anyway)
        return np.array([r, g, b, f32(0), f32(0)], np.float32)
    H, T = entropy_of_alphas(alphas, min_T)
    return np.array([r, g, b, f32(1) - T, H], np.float32)


def render(lib, field, cam, w, h, S=128, spp=1, min_T=1e-4, step_mode=0, pixel_stride=1):
    """-> (h, w, 5) float32: r, g, b, alpha (as OracleField.render) and H (bits).
    pixel_stride n > 1: only the pixels whose row-major index is a multiple of n are computed (`march_ref.strided` picks the
    same ones out of an image); the others stay 0."""
    sub = np.zeros((spp, h, w, 5), np.float32)
    for k, y, x, o, d in rays(lib, cam, w, h, spp, pixel_stride):
        sub[k, y, x] = march_ray(lib, field, o, d, step_mode, S, f32(min_T))
    return mean(sub)


def reference(oracle, f, ocam, w, h, S, spp, min_T, mode, pixel_stride=1):
    want = render(oracle.lib(), f, ocam, w, h, S, spp, min_T, mode, pixel_stride)
    assert_alpha_is_the_oracles(f, ocam, w, h, S, spp, min_T, mode, want[..., :4], pixel_stride)  # its colour too
    return want


# ---- the bar of the GPU tests (tests/test_gpu_entropy.py): |got - want| <= RTOL * max(|want|, FLOOR), the project's form
# (util.PIX_RTOL with a floored denominator).
# MEASURED on the MI355X over every comparison of tests/test_gpu_entropy.py (88 images: the instance matrix x 3 configurations x
# 2 views, util.SMALL / SMALL_F2 whole images x 6 configurations, the product's two fields; `ENTROPY_FIGURES` lines of pytest -s):
#   largest |got - want| = 8.0e-5 bits, at H = 4.5 bits (F4_3, S = 128);
#   largest |got - want| / |want| with NO floor = 2.2e-5 (the same pixel); second 1.8e-5 (F4_wide, S = 37 spp 2);
#   no pixel of these inputs misses a pure 1e-3 relative bar: the floor these inputs NEED is 0.
# Why there is a floor all the same, and its size: alpha = 1 - exp(-sigma dt) is a difference from 1, so the hardware exp2 and
# the MFMA accumulation order (about 1 ulp each in the exponential) move alpha by up to one ulp of 1, 2^-24, ABSOLUTELY, however
# small alpha is.  A ray whose only samples are nearly transparent (w ~ 2^-24 ... 1e-5) then has H = h(w) + h(1 - w) off by
# 2^-24 * |dH/dw| = 2^-24 * (log2(1 / w) + 1 / ln 2) <= 2^-24 * (24 + 1.44) = 1.5e-6 bits while H itself is of that order: no
# relative bar can hold there.  1.5e-6 / RTOL = 1.5e-3 bits; FLOOR = 2^-9 = 1.95e-3 bits is the next power of two (margin 1.3).
# Below it the bar is an absolute 1.95e-6 bits; a view's score is a mean of values up to ~7 bits.
RTOL = 1e-3
FLOOR = 2.0 ** -9


def rel_err(got, want):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    return np.abs(got - want) / np.maximum(np.abs(want), FLOOR)


def stats(got, want):
    """the figures the bar was set from: (largest absolute deviation, largest unfloored relative error, the floor a pure RTOL
    bar would need, largest floored relative error)"""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    dev = np.abs(got - want)
    with np.errstate(divide="ignore", invalid="ignore"):
        rel = np.where(want != 0, dev / np.abs(want), np.where(dev == 0, 0.0, np.inf))
    miss = rel > RTOL
    need = (dev[miss] / RTOL).max() if miss.any() else 0.0
    return float(dev.max()), float(rel.max()), float(need), float(rel_err(got, want).max())


def assert_close_any(got, wants):
    """got: (..., 2) = (alpha, H) per pixel; wants: the references at the thresholds of util.termination_variants().  Every
    pixel (both values together) must match one of them (util.assert_pixels_close_any's rule: a ray may stop a sample
    either side of min_T)."""
    from tests import util

    got = np.asarray(got)
    errs = np.stack([np.maximum(util.pixel_rel_err(got[..., 0], w[..., 0]), rel_err(got[..., 1], w[..., 1])) for w in wants])
    best = errs.min(axis=0)
    worst = np.unravel_index(np.argmax(best), best.shape)
    assert best.max() <= RTOL, (f"pixel {worst}: got (alpha, H) {got[worst]!r}, want {np.asarray(wants[0])[worst]!r} (or its termination "
                                f"variants), relative error {best.max():.3e} (floor {FLOOR})")
