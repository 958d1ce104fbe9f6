"""The input families of the image-space tests (test infrastructure): ONE builder, so that tests/test_image_ref_host.py (the
oracle twin against the float64 reference, no GPU) and tests/test_gpu_image_scores.py (the kernels against it) see the same
bytes.  Everything is seeded; nothing here computes an expected value."""
import numpy as np

f32 = np.float32
KNEE = f32(0.0031308)
BACKGROUNDS = [(0.0, 0.0, 0.0, 0.0), (0.0, 0.0, 0.0, 1.0), (1.0, 1.0, 1.0, 1.0), (0.5, 0.0, 1.0, 1.0)]
NOISE = [0.002, 0.05, 0.3]
ALPHAS = [0.0, 2.0 ** -149, 1e-30, 2.0 ** -24, 1.0 - 2.0 ** -24, 1.0, 1.5, -0.25]
SSIM_SHAPES = [(5, 5), (5, 64), (64, 5), (6, 6), (21, 13), (69, 61), (260, 260)]  # (h, w)


def random_pair(seed, n, h, w, noise):
    """n premultiplied (h, w, 4) images and the same plus Gaussian noise, clipped to [0, 1]: a render and its ground truth"""
    rng = np.random.default_rng(seed)
    a = rng.random((n, h, w, 4)).astype(f32)
    a[..., :3] *= a[..., 3:4]
    b = np.clip(a + rng.normal(scale=noise, size=a.shape), 0, 1).astype(f32)
    return a, b


def _ulp_walk(x, k):
    """the 2k + 1 float32 values within k ulp of x, ascending"""
    bits = np.array([x], f32).view(np.int32)[0]
    ordered = lambda b: np.int64(b) if b >= 0 else np.int64(-(b & 0x7FFFFFFF))  # sign-magnitude -> a line through +-0
    o = ordered(int(bits)) + np.arange(-k, k + 1, dtype=np.int64)
    back = np.where(o >= 0, o, (-o) | 0x80000000).astype(np.uint32)
    return back.view(f32)


def knee_pixels():
    """un-premultiplied values within 64 ulp of the sRGB knee, of 0 (denormals of both signs) and of 1, as opaque pixels (the
    quotient is then exact) and at alpha 0.75 (premultiplied in float32: the quotient lands on or next to the value; not 0.5,
    whose alpha byte 128.0 would sit on a byte boundary itself)"""
    v = np.concatenate([_ulp_walk(KNEE, 64), _ulp_walk(f32(0.0), 64), _ulp_walk(f32(1.0), 64)])
    out = []
    for alpha in (f32(1.0), f32(0.75)):
        px = np.empty((len(v), 4), f32)
        px[:, 0], px[:, 1], px[:, 2] = v * alpha, np.roll(v, 1) * alpha, np.roll(v, 2) * alpha
        px[:, 3] = alpha
        out.append(px)
    return np.concatenate(out)


def alpha_pixels():
    """every alpha of ALPHAS with colours premultiplied by it (t * alpha, t in 0, 0.2, 0.5, 1) and with colours that are NOT
    (2^-149, 1e-30, 0.25, -0.25: the un-premultiply explodes into the clamp, or is negative)"""
    out = []
    for a in ALPHAS:
        a = f32(a)
        for t in (0.0, 0.2, 0.5, 1.0):
            out.append([f32(t) * a, f32(1.0 - t) * a, f32(0.5 * t) * a, a])
        for c in (2.0 ** -149, 1e-30, 0.25, -0.25):
            out.append([f32(c), f32(0.5 * c), f32(-c), a])
    return np.array(out, f32)


def nonfinite_pixels():
    """NaN, +Inf, -Inf and -0.0 in each channel in turn of an ordinary pixel"""
    out = []
    for bad in (np.nan, np.inf, -np.inf, -0.0):
        for ch in range(4):
            px = [0.2, 0.4, 0.6, 0.8]
            px[ch] = bad
            out.append(px)
    return np.array(out, f32)


def boundary_pixels():
    """opaque pixels whose channel sits ON a byte boundary as well as float32 can put it: the float32 neighbours of the value
    whose y = 255 srgb(v) + 0.5 is the integer k, k = 1..255.  The inverse is taken by bisection on the float64 curve: data,
    not an expectation"""
    ks = np.arange(1, 256, dtype=np.float64)
    target = (ks - 0.5) / 255.0
    lo, hi = np.zeros_like(target), np.ones_like(target)
    curve = lambda x: np.where(x <= float(KNEE), float(f32(12.92)) * x,
                               float(f32(1.055)) * np.power(np.maximum(x, 1e-300), float(f32(0.41666666))) - float(f32(0.055)))
    for _ in range(80):
        mid = 0.5 * (lo + hi)
        below = curve(mid) < target
        lo, hi = np.where(below, mid, lo), np.where(below, hi, mid)
    v = hi.astype(f32)
    v = np.concatenate([np.nextafter(v, f32(0)), v, np.nextafter(v, f32(2))])
    px = np.ones((len(v), 4), f32)
    px[:, 0], px[:, 1], px[:, 2] = v, v[::-1], np.roll(v, 7)
    return px


def quantize_families():
    """name -> (pixels (n, 4) float32, background); `boundary*` families are on byte boundaries on purpose (asserted with
    "differs by at most 1", outside the 1 % cap), every other family is under the cap"""
    fam = {}
    for i, noise in enumerate(NOISE):
        for j, bg in enumerate(BACKGROUNDS):
            a, b = random_pair(0x1A6E + 16 * i + j, 1, 37, 53, noise)
            fam[f"noise{noise}/bg{j}"] = (np.concatenate([a.reshape(-1, 4), b.reshape(-1, 4)]), bg)
    for j, bg in enumerate(BACKGROUNDS):
        fam[f"knee/bg{j}"] = (knee_pixels(), bg)
        fam[f"alpha/bg{j}"] = (alpha_pixels(), bg)
        fam[f"nonfinite/bg{j}"] = (nonfinite_pixels(), bg)
        fam[f"boundary/bg{j}"] = (boundary_pixels(), bg)
    return fam


def as_image(pixels, h, w):
    """the pixel list repeated into an (h, w, 4) image"""
    idx = np.arange(h * w) % len(pixels)
    return np.ascontiguousarray(pixels[idx].reshape(h, w, 4))


def image_families():
    """name -> (image (h, w, 4), ground truth (h, w, 4), background): the pairs PSNR and SSIM are compared on.  Random pairs at
    every noise scale, background and SSIM shape; the knee,
    alpha and boundary pixel lists as images against a shifted copy of themselves.  Finite values only: a NaN pixel makes
    every score NaN, which test_gpu_image_scores.py checks on its own."""
    fam = {}
    for i, noise in enumerate(NOISE):
        for j, bg in enumerate(BACKGROUNDS):
            for k, (h, w) in enumerate(SSIM_SHAPES):
                if h * w > 10000 and i != j:
                    continue  # the several-block shape once per noise scale
                a, b = random_pair(0x55A0 + 64 * i + 8 * j + k, 1, h, w, noise)
                fam[f"noise{noise}/bg{j}/{h}x{w}"] = (a[0], b[0], bg)
    for j, bg in enumerate(BACKGROUNDS):
        for name, px in (("knee", knee_pixels()), ("alpha", alpha_pixels()), ("boundary", boundary_pixels())):
            img = as_image(px, 21, 13)
            fam[f"{name}/bg{j}"] = (img, np.ascontiguousarray(np.roll(img, 5, axis=1)), bg)
    return fam


# ---- ensemble scores: the sequential sum streams 512 addends per chunk; method 2 has 3 addends per pixel, method 3 has 2.
# n_terms 1, 511, 512, 513, 1023, 1024, 1025 are reached where the divisor allows, else by the nearest pixel counts on both
# sides: method 2 (x3): 3, 510, 513, 1023, 1026; method 3 (x2): 2, 510, 512, 514, 1022, 1024, 1026
ENSEMBLE_NPIX = {2: [1, 170, 171, 341, 342], 3: [1, 255, 256, 257, 511, 512, 513]}
ENSEMBLE_MODES = ("random", "gated", "negative")


def members(seed, E, npix, mode):
    """E member images (npix, 4) uint8.  random: a base image plus small noise, half of it zero (many zero variances);
    gated: every member the same (all variances 0: every addend of method 2 is skipped); negative: the last member is one grey
    level up in every colour (variance (E - 1) / E^2 <= 1/4: every addend of method 2 is a negative logarithm)"""
    rng = np.random.default_rng(seed)
    base = rng.integers(0, 256, (npix, 4), dtype=np.uint8)
    if mode == "gated":
        return [base.copy() for _ in range(E)]
    if mode == "negative":
        base = np.minimum(base, 254)
        out = [base.copy() for _ in range(E)]
        out[-1][:, :3] += 1
        return out
    return [np.clip(base.astype(int) + rng.integers(-3, 4, base.shape) * (rng.random(base.shape) < 0.5), 0, 255).astype(np.uint8)
            for _ in range(E)]
