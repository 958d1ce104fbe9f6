"""An independent float64 statement of the image-space block (test infrastructure, numpy only): byte quantisation, the
PSNR / coverage ranking key, SSIM and the two ensemble scores, written from the contract in include/prv.h and the recipe it
cites -- not from the kernels and not from oracle/prv_oracle.c, which this file does not import.  The inputs are the float32
(or uint8) arrays the device gets; everything after them is float64.  The recipe's constants are the float32 numbers the
contract names (12.92f, 1.055f, 0.055f, the knee 0.0031308f, the exponents, the blur taps, the luminance weights): they are
DATA of the recipe and enter here as exact values, so `x <= knee` means the same thing on both sides.

THE RECIPE (prv.h: prv_render_rgba8, prv_quantize_rgba8, prv_score_psnr_images, prv_evaluate_images)
  composite   C_k = (1 - a) bg_k + c_k  for the three colours and  C_3 = (1 - a) bg_3 + a  for alpha
  bytes       V_k = C_k / C_3 if C_3 != 0 else C_k;  s = clip(srgb(V_k), 0, 1);  y = 255 s + 0.5;  byte = floor(y)
              alpha byte: the same from s = clip(C_3, 0, 1)
  srgb(x)     12.92 x for x <= 0.0031308, else 1.055 x^(1/2.4) - 0.055
  clip        fmin(fmax(., 0), 1): a NaN becomes 0 (fmax returns its other operand), -0.0 and -Inf become 0, +Inf becomes 1
  psnr        s = clip(srgb(C_k)) of the image and of the reference image (NO un-premultiply), mse over pixels x 3,
              psnr = -10 log10(mse);  coverage = mean(a);  score = -psnr + weight * mean((1 - a)^2)
  ssim        luminance l = sum_k kw_k s_k^0.4545..., separable 5-tap blur over the valid region of l_a, l_b, l_a^2, l_b^2,
              l_a l_b;  variances = blurred squares - squared means;  c1 = 0.01^2, c2 = 0.03^2;  mean of the map

THE FLOAT32 ERROR BOUND (what `band` and the PSNR bound are made of)
u = 2^-24 is the unit roundoff: one float32 rounding of a normal result z errs by at most u |z| (2^-149 absolute when z is
subnormal; that term is added to every step below and never matters).  A k-ulp function result errs by at most 2 k u |z|.
Both builds compile without contraction, so every operation written in the recipe is one rounding and fmaf is one.
  1. rem = 1 - a                          1 rounding:  e_rem = u |rem|
  2. C_k = fma(rem, bg_k, c_k)            1 rounding:  e_C = e_rem |bg_k| + u |C_k|       (exact when bg_k = 0)
     C_3 likewise                         1 rounding
  3. V = C_k / C_3                        1 rounding:  e_V = (e_Ck / |C_3| + |V| r_3) / (1 - r_3) + u |V|,  r_3 = e_C3 / |C_3|
     from the ACTUAL operands: as alpha -> 0 the quotient multiplies the composite's rounding by 1 / |C_3|, and a
     cancelling composite (negative colours, alpha > 1) has e_C far above u |C_k|
  4. srgb:  linear branch 12.92 x         1 rounding
            power branch                  powf: POW_ULP = 1 ulp.  HIP documents powf at 1 ulp (HIP math API, "single
                                          precision mathematical functions"); glibc documents powf at 1 ulp on x86-64 (libm
                                          manual, "known maximum errors").  Then 1.055 p and - 0.055: 2 roundings.
     The input's error e_V goes through srgb by evaluating it at V - e_V and V + e_V (it is monotone on either side of the knee;
     an interval that contains the knee takes both branches at the knee, which differ by 2e-6: the standard's two pieces
     do not meet exactly).
  5. clip                                 exact, and it forgets whatever error lies outside [0, 1]
  6. y = s * 255 + 0.5                    2 roundings
A colour byte therefore carries 8 roundings and one powf (6 and none on the linear branch), the alpha byte 4 roundings; the sRGB
value the PSNR compares (no division, no scaling) carries 4 roundings and one powf: eps = e(s) of steps 1, 2, 4.  For s near
1 on an opaque pixel that is (2 + 1 + 1) u = 2.4e-7; it grows with (1 - a) bg and with the slope of srgb below 0.05.
`band` is the resulting half-width on y: a float32 evaluation may return the other byte only where |y - rint(y)| <= band.

PSNR.  With eps_i = eps(image) + eps(reference) per channel value, |d32_i^2 - d_i^2| <= 2 eps_i |d_i| + eps_i^2, so
  dmse <= mean(2 eps_i |d_i| + eps_i^2)            (the per-element form of 2 eps mean|d| + eps^2)
  dpsnr <= (10 / ln 10) * dmse / (mse - dmse)      (infinite when dmse >= mse: nothing can be said)
plus the float32 rounding of the record's psnr field.  The sums are fp64 on the device: N 2^-52 relative, added.

MEASURED (tests/test_image_ref_host.py prints these; x86-64 glibc against this file)
  share of colour and alpha bytes inside their band, per family, the largest over the four backgrounds (cap 1 %):
    noise 0.002   0.0191 %      knee       0.0000 %      boundary  75 % (on boundaries on purpose: outside the cap,
    noise 0.05    0.0319 %      alpha      0.0000 %                asserted with "differs by at most 1")
    noise 0.3     0.0255 %      nonfinite  0.0000 %
    No family's seed had to change; the knee family's translucent half uses alpha 0.75, not 0.5, whose alpha byte is
    exactly 128.0: a boundary of its own.
  largest |oracle.ssim - image_ref.ssim|, per family:
    noise 0.002   1.791e-05  (5x5, white background, SSIM 0.99996: ONE window, nothing averages the float32 cancellation
    noise 0.05    8.305e-06   in blur(a^2) - blur(a)^2 of a bright, nearly constant window against c2 = 9e-4)
    noise 0.3     2.588e-06
    knee          8.837e-07     alpha  7.133e-08     boundary  2.004e-06
    From 6x6 on the largest is 5.3e-6, from 21x13 on below 1e-6.
  SSIM_TWIN_MAX = 1.8e-5 is the largest, rounded up; SSIM_TOL = 4 x that = 7.2e-5.  Below the 1e-4 at which the recipe itself
  would be the finding, but not by much: on a single bright window float32 SSIM is good to five digits, no more.
"""
import math

import numpy as np

U = 2.0 ** -24  # float32 unit roundoff
TINY = 2.0 ** -149  # absolute error of a rounding that lands in the subnormals
POW_ULP = 1.0  # documented bound of HIP's powf and of glibc's, in ulp

f32 = np.float32
K_LIN, K_A, K_B = float(f32(12.92)), float(f32(1.055)), float(f32(0.055))
KNEE = float(f32(0.0031308))
K_EXP = float(f32(0.41666666))
K_GAMMA = float(f32(0.4545454545))
K_LUM = [float(f32(0.2126)), float(f32(0.7152)), float(f32(0.0722))]
K_TAP = np.array([float(f32(t)) for t in (0.120078, 0.233881, 0.292082, 0.233881, 0.120078)])
C1, C2 = 0.01 ** 2, 0.03 ** 2

# 4 x the largest twin-against-float64 deviation of the table above (tests/test_image_ref_host.py re-measures it and fails if
# the measurement no longer supports this number)
SSIM_TWIN_MAX = 1.8e-5
SSIM_TOL = 4 * SSIM_TWIN_MAX


def _f64(a):
    a = np.asarray(a)
    assert a.dtype == np.float32, "the reference starts from the float32 inputs the device gets"
    return a.astype(np.float64)


def srgb(x):
    """the two-piece curve; NaN takes the power branch (the comparison is false) and stays NaN"""
    with np.errstate(all="ignore"):
        return np.where(x <= KNEE, K_LIN * x, K_A * np.power(np.where(x <= KNEE, 1.0, x), K_EXP) - K_B)


def clip01(s):
    return np.fmin(np.fmax(s, 0.0), 1.0)  # fmax / fmin return the operand that is not NaN


def _srgb_round(x):
    """float32 evaluation error of srgb at x (step 4): one rounding, or powf's ulp and two roundings"""
    with np.errstate(all="ignore"):
        p = K_A * np.power(np.where(x <= KNEE, 1.0, x), K_EXP)
        return np.where(x <= KNEE, U * np.abs(K_LIN * x), 2 * POW_ULP * U * p + U * p + U * np.abs(p - K_B)) + TINY


def srgb_clip_err(x, ex):
    """S = clip(srgb(x)) and the bound on |S32 - S| when float32 holds x to within ex and evaluates steps 4-5"""
    S = clip01(srgb(x))
    ok = np.isfinite(x) & np.isfinite(ex)  # non-finite values follow IEEE rules alike in both widths: no band
    lost = np.isfinite(x) & ~np.isfinite(ex)  # a finite value float32 knows nothing about
    xs, es = np.where(ok, x, 0.0), np.where(ok, ex, 0.0)
    lo, hi = xs - es, xs + es
    straddle = (lo <= KNEE) & (hi > KNEE)
    knee_lo = np.minimum(K_LIN * KNEE, K_A * KNEE ** K_EXP - K_B)
    knee_hi = np.maximum(K_LIN * KNEE, K_A * KNEE ** K_EXP - K_B)
    s_min = np.minimum(srgb(lo) - _srgb_round(lo), srgb(hi) - _srgb_round(hi))
    s_max = np.maximum(srgb(lo) + _srgb_round(lo), srgb(hi) + _srgb_round(hi))
    s_min = np.where(straddle, np.minimum(s_min, knee_lo * (1 - 4 * U)), s_min)
    s_max = np.where(straddle, np.maximum(s_max, knee_hi * (1 + 4 * U)), s_max)
    Ss = clip01(srgb(xs))
    err = np.maximum(Ss - clip01(s_min), clip01(s_max) - Ss)
    return S, np.where(lost, np.inf, np.where(ok, err, 0.0))


def _composite(rgba, bg):
    """C (..., 4) and its float32 error bound (steps 1-2)"""
    bg = np.asarray(bg, np.float32).astype(np.float64)
    a = rgba[..., 3:4]
    with np.errstate(all="ignore"):
        rem = 1.0 - a
        e_rem = U * np.abs(rem) + TINY
        src = np.concatenate([rgba[..., :3], a], axis=-1)
        C = rem * bg + src
        eC = np.where(bg == 0.0, 0.0, e_rem * np.abs(bg) * (1 + U) + U * np.abs(C) + TINY)
    return C, eC


class Quantized:
    def __init__(self, y, byte, band):
        self.y, self.byte, self.band = y, byte, band

    @property
    def in_band(self):
        return np.abs(self.y - np.rint(self.y)) <= self.band


def quantize_exact(rgba_f32, bg):
    """-> Quantized(y, byte, band), each of rgba's shape: y = clip(srgb(un-premultiplied composite)) * 255 + 0.5 in float64 (the
    alpha channel: clip(composite alpha) * 255 + 0.5), byte = floor(y) as uint8, band = the float32 bound on y derived above"""
    rgba = _f64(rgba_f32)
    C, eC = _composite(rgba, bg)
    C3, eC3 = C[..., 3:4], eC[..., 3:4]
    with np.errstate(all="ignore"):
        div = C3 != 0.0  # NaN != 0: a NaN alpha divides, and the quotient is NaN
        den = np.where(div, C3, 1.0)
        V = np.where(div, C[..., :3] / den, C[..., :3])
        r3 = np.where(div, eC3 / np.abs(den), 0.0)
        eV = np.where(div, (eC[..., :3] / np.abs(den) + np.abs(V) * r3) / np.maximum(1.0 - r3, 0.0), eC[..., :3])
        eV = eV + U * (np.abs(V) + eV) + TINY
        # float32 cannot tell on which side of 0 the composite alpha is: either rule may apply
        unsure = np.broadcast_to(np.where(div, r3 >= 1.0, eC3 > 0.0), V.shape)
        S, eS = srgb_clip_err(V, np.where(unsure, 0.0, eV))
        S3 = clip01(C3)
        eS3 = np.where(np.isfinite(C3), np.minimum(eC3, 1.0), 0.0)
        S = np.concatenate([S, S3], axis=-1)
        eS = np.concatenate([np.where(unsure, np.inf, eS), eS3], axis=-1)
        y = S * 255.0 + 0.5
        band = 255.0 * eS + U * 255.0 * S + U * y
    return Quantized(y, np.floor(y).astype(np.uint8), band)


class PsnrScore:
    def __init__(self, score, psnr, coverage, mse, psnr_tol, score_tol, coverage_tol, eps_max):
        self.score, self.psnr, self.coverage, self.mse = score, psnr, coverage, mse
        self.psnr_tol, self.score_tol, self.coverage_tol, self.eps_max = psnr_tol, score_tol, coverage_tol, eps_max


def srgb_planes(rgba_f32, bg):
    """clip(srgb(composite)) of the three colours, without un-premultiplying, and its float32 error bound eps"""
    C, eC = _composite(_f64(rgba_f32), bg)
    return srgb_clip_err(C[..., :3], eC[..., :3])


def psnr_coverage(rgba, gt, bg, weight=1.0):
    """one view -> PsnrScore: the ranking key, psnr (dB), coverage, and the bounds a float32 evaluation of the channel values
    stays within (psnr_tol covers the double the device keeps; a float32 copy adds |psnr| 2^-24 of its own)"""
    A, eA = srgb_planes(rgba, bg)
    R, eR = srgb_planes(gt, bg)
    a = _f64(rgba)[..., 3]
    n = a.size
    with np.errstate(all="ignore"):
        d = A - R
        eps = eA + eR
        mse = float(np.sum(d * d)) / (3 * n)
        dmse = float(np.sum(2 * eps * np.abs(d) + eps * eps)) / (3 * n) + mse * 3 * n * 2.0 ** -52
        psnr = -10.0 * math.log10(mse) if mse > 0 else math.inf
        if mse == 0:
            psnr_tol = 0.0 if dmse == 0 else math.inf
        elif dmse >= mse or not math.isfinite(dmse):
            psnr_tol = math.inf
        else:
            psnr_tol = 10.0 / math.log(10.0) * dmse / (mse - dmse) + abs(psnr) * 2.0 ** -50
        coverage = float(np.sum(a)) / n
        unc = float(np.sum((1.0 - a) ** 2)) / n
    cov_tol = abs(coverage) * (U + n * 2.0 ** -52) + TINY  # the record's coverage is a float32
    unc_tol = abs(weight) * unc * n * 2.0 ** -52
    return PsnrScore(-psnr + weight * unc, psnr, coverage, mse, psnr_tol, psnr_tol + unc_tol, cov_tol, float(np.max(eps)) if n else 0.0)


def luminance(rgba_f32, bg):
    S, _ = srgb_planes(rgba_f32, bg)
    with np.errstate(all="ignore"):
        return sum(K_LUM[k] * np.power(np.fmax(S[..., k], 0.0), K_GAMMA) for k in range(3))


def _blur_valid(img):
    h, w = img.shape
    rows = sum(K_TAP[j] * img[:, j:w - 4 + j] for j in range(5))
    return sum(K_TAP[i] * rows[i:h - 4 + i, :] for i in range(5))


def ssim_map(la, lb):
    mA, mB = _blur_valid(la), _blur_valid(lb)
    sA = _blur_valid(la * la) - mA * mA
    sB = _blur_valid(lb * lb) - mB * mB
    sAB = _blur_valid(la * lb) - mA * mB
    return ((2 * mA * mB + C1) / (mA * mA + mB * mB + C1)) * ((2 * sAB + C2) / (sA + sB + C2))


def ssim(rgba, gt, bg):
    """one (h, w, 4) image pair, h, w >= 5 -> the mean of the SSIM map over the valid region"""
    assert rgba.ndim == 3 and rgba.shape[0] >= 5 and rgba.shape[1] >= 5
    return float(np.mean(ssim_map(luminance(rgba, bg), luminance(gt, bg))))


def _channel_variances(imgs):
    """imgs: E arrays (npix, 4) uint8 -> (npix, 3) population variances of the reference's r, g, b = bytes 2, 1, 0 (it reads
    BGRA), sums over the members in order"""
    E = len(imgs)
    x = [np.asarray(i).reshape(-1, 4)[:, [2, 1, 0]].astype(np.float64) for i in imgs]
    mean = x[0].copy()
    for e in range(1, E):
        mean = mean + x[e]
    mean = mean / E
    var = np.zeros_like(mean)
    for e in range(E):
        var = var + (x[e] - mean) * (x[e] - mean)
    return var / E


def _sequential(terms):
    s = 0.0
    for t in terms:
        s += t
    return s


def ensemble_rgb_terms(imgs):
    """method 2's addends, rows x columns x (r, g, b): log(var) where var > 1e-10, else nothing (0.0)"""
    return [math.log(v) if v > 1e-10 else 0.0 for v in _channel_variances(imgs).reshape(-1).tolist()]


def ensemble_rgb(imgs):
    return _sequential(ensemble_rgb_terms(imgs))


def ensemble_rgbdensity_terms(imgs):
    """method 3's addends, two statements per pixel: (var_r + var_g + var_b) / 3, then (1 - mean density)^2"""
    E = len(imgs)
    var = _channel_variances(imgs)
    colour = (var[:, 0] + var[:, 1] + var[:, 2]) / 3.0
    dens = [np.asarray(i).reshape(-1, 4)[:, 3].astype(np.float64) / 255.0 for i in imgs]
    md = dens[0].copy()
    for e in range(1, E):
        md = md + dens[e]
    md = md / E
    return np.stack([colour, (1.0 - md) * (1.0 - md)], axis=1).reshape(-1).tolist()


def ensemble_rgbdensity(imgs):
    return _sequential(ensemble_rgbdensity_terms(imgs))


def ensemble_rgb_bound(imgs):
    """|device - this| for method 2: each log may differ in its last bit: n_terms 2^-52 |term|max"""
    t = ensemble_rgb_terms(imgs)
    return len(t) * 2.0 ** -52 * max([abs(v) for v in t] + [0.0])
