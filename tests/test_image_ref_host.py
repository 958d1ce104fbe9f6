"""tests/image_ref.py validated without a GPU: known answers of the float64 reference, then the oracle's float32 twin
(oracle/prv_oracle.c: orc_quantize_rgba8, orc_score_view, orc_ssim, the ensemble scores) against it on the input families of
tests/image_cases.py -- the inputs and bounds tests/test_gpu_image_scores.py then holds the kernels to.  Prints the share of
in-band bytes per family (cap 1 %) and the twin's SSIM deviations that image_ref.SSIM_TOL is four times the largest of."""
import math

import numpy as np
import pytest

from tests import image_cases as cases
from tests import image_ref as ref

f32 = np.float32
BAND_CAP = 0.01


def _const(h, w, rgb, a=1.0):
    img = np.empty((h, w, 4), f32)
    img[..., :3], img[..., 3] = rgb, a
    return img


# ---- known answers of the reference itself

def test_identical_images():
    a, _ = cases.random_pair(1, 1, 9, 11, 0.05)
    for bg in cases.BACKGROUNDS:
        assert ref.ssim(a[0], a[0], bg) == 1.0
        p = ref.psnr_coverage(a[0], a[0].copy(), bg)
        assert p.mse == 0.0 and p.psnr == math.inf and p.score == -math.inf
        # the rounding bound cannot promise this of a float32 evaluation; that both sides of the difference are the same
        # operations on the same bits does (the GPU test asserts +inf for that reason)
        assert p.psnr_tol == math.inf


def test_black_against_white():
    black, white = _const(7, 8, 0.0), _const(7, 8, 1.0)
    p = ref.psnr_coverage(black, white, (0, 0, 0, 0))
    # white is 1.055f - 0.055f = 1 - 5e-8 with the recipe's float32 constants: 0 dB to within 1e-6
    assert p.mse == pytest.approx(1.0, abs=2e-7) and abs(p.psnr) < 1e-6 and p.coverage == 1.0 and abs(p.score) < 1e-6
    s = ref.ssim(black, white, (0, 0, 0, 0))
    lw = sum(ref.K_LUM) * (ref.K_A - ref.K_B) ** ref.K_GAMMA * ref.K_TAP.sum() ** 2  # white's blurred luminance; black's is 0, the covariance term is c2 / c2
    assert s == pytest.approx(ref.C1 / (lw * lw + ref.C1), rel=1e-6) and 0 < s < 1.1e-4


def test_constant_images():
    for ga, gb in ((0.25, 0.5), (0.0, 0.1), (1.0, 0.9)):
        A, B = _const(8, 6, ga), _const(8, 6, gb)
        la, lb = ref.luminance(A, (0, 0, 0, 1))[0, 0], ref.luminance(B, (0, 0, 0, 1))[0, 0]
        want = (2 * la * lb + ref.C1) / (la * la + lb * lb + ref.C1)
        # the taps are float32 numbers and sum to 1 - 1.3e-8, not to 1: the "variances" of a constant are -2.6e-8 l^2, not 0
        assert ref.ssim(A, B, (0, 0, 0, 1)) == pytest.approx(want, rel=1e-6)
        assert la == pytest.approx(sum(ref.K_LUM) * ref.clip01(ref.srgb(np.float64(f32(ga)))) ** ref.K_GAMMA, rel=1e-12)


def test_hand_computed_window():
    """5 x 5, one window: A is black but for a white centre, B has a second white pixel in the corner.  With L = white's
    luminance, p = tap[2]^2 the centre's weight and q = tap[0]^2 the corner's, every blurred quantity is a weight times L or
    L^2, written out here term by term"""
    A, B = _const(5, 5, 0.0), _const(5, 5, 0.0)
    A[2, 2, :3] = 1.0
    B[2, 2, :3] = 1.0
    B[0, 0, :3] = 1.0
    t = [float(f32(x)) for x in (0.120078, 0.233881, 0.292082)]
    white = (float(f32(1.055)) - float(f32(0.055))) ** float(f32(0.4545454545))  # srgb(1) with the float32 constants, then the gamma
    L = (float(f32(0.2126)) + float(f32(0.7152)) + float(f32(0.0722))) * white
    p, q = t[2] * t[2], t[0] * t[0]
    mA, mB = p * L, (p + q) * L
    sA, sB, sAB = p * L * L - mA * mA, (p + q) * L * L - mB * mB, p * L * L - mA * mB
    want = (2 * mA * mB + 1e-4) / (mA * mA + mB * mB + 1e-4) * (2 * sAB + 9e-4) / (sA + sB + 9e-4)
    assert ref.ssim(A, B, (0, 0, 0, 0)) == pytest.approx(want, rel=1e-12)
    assert 0.5 < want < 1.0


def test_quantize_known_bytes():
    px = np.array([[0, 0, 0, 1], [1, 1, 1, 1], [0.5, 0.25, 0.0, 0.5], [0, 0, 0, 0], [0.2, 0.4, 0.6, 0.0]], f32)
    q = ref.quantize_exact(px, (0, 0, 0, 0))
    assert q.byte[0].tolist() == [0, 0, 0, 255] and q.byte[1].tolist() == [255, 255, 255, 255]
    assert q.byte[2].tolist() == [255, 188, 0, 128]  # un-premultiplied 1, 0.5, 0: 0.5 -> sRGB 0.7354 -> 188.03
    assert q.byte[3].tolist() == [0, 0, 0, 0]
    assert q.byte[4].tolist() == [124, 170, 203, 0]  # alpha 0 over alpha-0 background: the colours are NOT divided
    assert q.y[2, 1] == pytest.approx(255 * (1.055 * 0.5 ** (1 / 2.4) - 0.055) + 0.5, abs=1e-4)
    nan = ref.quantize_exact(np.array([[np.nan, 0.5, 0.5, 1.0], [0.5, 0.5, 0.5, np.nan]], f32), (0, 0, 0, 1))
    assert nan.byte[0].tolist() == [0, 188, 188, 255] and nan.byte[1].tolist() == [0, 0, 0, 0]


# ---- the float32 twin against float64: quantisation

def test_twin_bytes_within_band(oracle):
    print()
    for name, (px, bg) in cases.quantize_families().items():
        q = ref.quantize_exact(px, bg)
        got = oracle.quantize_rgba8(px, bg).astype(int)
        diff = np.abs(got - q.byte.astype(int))
        share = float(q.in_band.mean())
        print(f"in-band bytes {name:18s} {100 * share:7.4f} %   twin differs on {int((diff != 0).sum()):4d} of {diff.size}")
        assert diff.max() <= 1, name
        if name.startswith("boundary"):
            continue  # on a boundary on purpose: "differs by at most 1" is all that can be asked
        assert not ((diff != 0) & ~q.in_band).any(), (name, np.argwhere((diff != 0) & ~q.in_band)[:5])
        assert share < BAND_CAP, name


def test_boundary_family_is_on_boundaries():
    """the family does what it is for: every pixel has a channel within 1e-4 of a byte boundary"""
    q = ref.quantize_exact(cases.boundary_pixels(), (0, 0, 0, 1))
    assert (np.abs(q.y[:, :3] - np.rint(q.y[:, :3])).min(axis=1) < 1e-4).all()
    assert q.in_band[:, :3].mean() > 0.2


# ---- PSNR / coverage

@pytest.mark.parametrize("weight", [0.0, 1.0, 2.5])
def test_twin_psnr_within_bound(oracle, weight):
    for name, (a, b, bg) in cases.image_families().items():
        want = ref.psnr_coverage(a, b, bg, weight)
        s, p, c = oracle.score_view(a, b, bg, weight)
        assert math.isfinite(want.psnr_tol) and want.psnr_tol < 0.05, (name, want.psnr_tol)  # the bound says something
        assert abs(p - want.psnr) <= want.psnr_tol, (name, p, want.psnr, want.psnr_tol)
        assert abs(s - want.score) <= want.score_tol, name
        assert abs(c - want.coverage) <= want.coverage_tol, name


def test_psnr_bound_follows_the_noise():
    tols = []
    for noise in cases.NOISE:
        a, b = cases.random_pair(7, 1, 21, 13, noise)
        tols.append(ref.psnr_coverage(a[0], b[0], (0, 0, 0, 1)).psnr_tol)
    assert tols[0] > tols[1] > tols[2] > 0  # a quieter pair has a smaller |d| for the same eps: a wider bound in dB


# ---- SSIM

def test_twin_ssim_deviation_sets_the_tolerance(oracle):
    worst = {}
    for name, (a, b, bg) in cases.image_families().items():
        d = abs(oracle.ssim(a, b, bg) - ref.ssim(a, b, bg))
        key = name.split("/")[0]
        worst[key] = max(worst.get(key, 0.0), d)
    print()
    for key, d in worst.items():
        print(f"twin - float64 SSIM, family {key:10s} max |d| = {d:.3e}")
    top = max(worst.values())
    print(f"largest {top:.3e}; SSIM_TOL = {ref.SSIM_TOL:.3e}")
    assert top <= ref.SSIM_TWIN_MAX  # the constant in image_ref.py is the measurement, rounded up ...
    assert ref.SSIM_TWIN_MAX <= 1.25 * top  # ... and not padded
    assert ref.SSIM_TOL == 4 * ref.SSIM_TWIN_MAX


# ---- ensemble scores

@pytest.mark.parametrize("E", [1, 2, 8])
def test_twin_ensemble_scores(oracle, E):
    for mode in cases.ENSEMBLE_MODES:
        for method, fn_ref, fn_orc in ((3, ref.ensemble_rgbdensity, oracle.score_ensemble_rgbdensity),
                                       (2, ref.ensemble_rgb, oracle.score_ensemble_rgb)):
            for npix in cases.ENSEMBLE_NPIX[method]:
                imgs = cases.members(npix * 8 + E, E, npix, mode)
                want, got = fn_ref(imgs), fn_orc(imgs)
                if method == 3:
                    assert got == want, (mode, npix)  # no transcendental: bit for bit
                else:
                    assert abs(got - want) <= ref.ensemble_rgb_bound(imgs), (mode, npix)
                    terms = ref.ensemble_rgb_terms(imgs)
                    if mode == "gated" or E == 1:
                        assert want == 0.0 and not any(terms)
                    if mode == "negative" and E > 1:
                        assert all(t < 0 for t in terms)
