"""The one CPU restatement of the oracle's march (test infrastructure): what tests/depth_ref.py, entropy_ref.py, surface_ref.py
and termination_ref.py fold their sums over.

Restates oracle/prv_oracle.c's march_ray and render_worker through the oracle's exported primitives only (its orc_* entry
points: sub-sample offset, ray generation, box intersection, occupancy, field evaluation), each called from exactly one place:
  * `rays`: the pixels' sub-sample rays, sub-sample k at the oracle's own offset k;
  * `ray_samples`: one ray's live samples i, t_i = fmaf(i + 0.5, dt, t0), alpha_i = 1 - exp(-sigma_i dt), rgb_i under either
    stepping rule, in depth order, cut after the first sample that leaves T = prod (1 - alpha_i) < min_T;
  * `composite`: sum_i w_i v_i, w_i = alpha_i T_i, the colour composite's sum for any per-sample values;
  * `mean`: per pixel the sub-samples summed in order, then scaled by 1 / spp;
  * `assert_alpha_is_the_oracles`: the self-check of every reference built on these against the oracle's own render.
fmaf is computed in float64 and rounded to float32; everything else is float32 arithmetic.  exp is the C library's expf, the function
the oracle calls.  The oracle library does not export it: `lib.expf` resolves because dlsym on a library's handle also searches the
library's dependencies, and libprv_oracle.so links libm.  numpy's float32 exp is a different one-ulp implementation, and where
sigma dt is about 2^-25 (the empty space of a trained field) one ulp of exp(-sigma dt) is a whole alpha = 1 - exp(-sigma dt).
"""
import ctypes as C

import numpy as np

f32 = np.float32
NGP_STEPS = 1024
NGP_DT = f32(np.sqrt(f32(3.0)) / f32(1024.0))


def fmaf(a, b, c):
    return f32(np.float64(a) * np.float64(b) + np.float64(c))


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def expf(lib, x):
    """the oracle's expf: libm's, a dependency of the oracle library"""
    fn = lib.expf
    if fn.restype is not C.c_float:
        fn.restype, fn.argtypes = C.c_float, [C.c_float]
    return f32(fn(float(x)))


def forward_cos(cam, d):
    """dot(d, f), f = column 2 of c2w normalised (the depth kernel's order of operations)"""
    m = np.frombuffer(cam.c2w, np.float32)
    fx, fy, fz = f32(m[2]), f32(m[6]), f32(m[10])
    inv = f32(1.0) / f32(np.sqrt(fmaf(fx, fx, fmaf(fy, fy, f32(fz * fz)))))
    return f32(fmaf(d[0], fx, fmaf(d[1], fy, f32(d[2] * fz))) * inv)


def rays(lib, cam, w, h, spp, pixel_stride=1, pixels=None):
    """yields (k, y, x, o, d): sub-sample k's ray of every pixel whose row-major index is a multiple of pixel_stride (pixels: of
    these (y, x) only, whatever their index).  o and d are buffers the next ray overwrites"""
    o, d = np.zeros(3, np.float32), np.zeros(3, np.float32)
    ox, oy = C.c_float(), C.c_float()
    chosen = None if pixels is None else {(int(y), int(x)) for y, x in pixels}
    for k in range(spp):
        lib.orc_spp_offset(k, C.byref(ox), C.byref(oy))
        for y in range(h):
            for x in range(w):
                if (y * w + x) % pixel_stride if chosen is None else (y, x) not in chosen:
                    continue
                lib.orc_raygen(C.byref(cam), x, y, C.c_float(ox.value), C.c_float(oy.value), _p(o), _p(d))
                yield k, y, x, o, d


def ray_samples(lib, field, o, d, step_mode, S, min_T):
    """-> (steps, ts, alphas, rgbs, dt): the ray's live samples in depth order, up to and including the one that cuts the ray;
    steps: the index i each t was formed from.  A ray that misses the box has none"""
    t0, t1 = C.c_float(), C.c_float()
    if not lib.orc_ray_aabb(_p(o), _p(d), C.byref(t0), C.byref(t1)):
        return [], [], [], [], f32(0)
    t0, t1 = f32(t0.value), f32(t1.value)
    if step_mode == 1:
        dt, n = NGP_DT, NGP_STEPS
    else:
        dt, n = f32((t1 - t0) / f32(S)), S
    T = f32(1)
    p = np.zeros(3, np.float32)
    rgb = np.zeros(3, np.float32)
    raw = np.zeros(32, np.float32)
    sigma = C.c_float()
    steps, ts, alphas, rgbs = [], [], [], []
    for i in range(n):
        t = fmaf(f32(i) + f32(0.5), dt, t0)
        if step_mode == 1 and not t < t1:
            break
        p[:] = (fmaf(t, d[0], o[0]), fmaf(t, d[1], o[1]), fmaf(t, d[2], o[2]))
        if not lib.orc_occupied(field.ptr, _p(p)):
            continue
        lib.orc_eval(field.ptr, _p(p), _p(d), C.byref(sigma), _p(rgb), _p(raw))
        alpha = f32(1) - expf(lib, -f32(f32(sigma.value) * dt))
        steps.append(i)
        ts.append(t)
        alphas.append(alpha)
        rgbs.append(tuple(rgb))
        T = f32(T * (f32(1) - alpha))
        if T < min_T:
            break
    return steps, ts, alphas, rgbs, dt


def composite(alphas, values, n):
    """-> ([sum_i w_i v_ij for the n columns j of values], T_end) over a ray's samples, each sum as acc = fmaf(w_i, v_ij, acc)"""
    T, acc = f32(1), [f32(0)] * n
    for a, v in zip(alphas, values):
        wgt = f32(a * T)
        acc = [fmaf(wgt, x, s) for x, s in zip(v, acc)]
        T = f32(T * (f32(1) - a))
    return acc, T


def mean(sub):
    """(spp, ...) -> the pixel: its sub-samples summed in order, then scaled by 1 / spp"""
    acc = np.zeros(sub.shape[1:], np.float32)
    for k in range(sub.shape[0]):
        acc = (acc + sub[k]).astype(np.float32)
    return (acc * (f32(1) / f32(sub.shape[0]))).astype(np.float32)


def strided(img, pixel_stride):
    """(h, w, c) -> (n, c): the pixels `rays(..., pixel_stride=)` visits"""
    img = np.asarray(img)
    return img.reshape(img.shape[0] * img.shape[1], -1)[::pixel_stride]


def assert_alpha_is_the_oracles(f, ocam, w, h, S, spp, min_T, mode, alpha, pixel_stride=1):
    """the self-check: the restatement's alpha (h, w), or its r, g, b, alpha (h, w, 4), is the oracle's own render"""
    img, _ = f.render(ocam, w, h, S, spp, min_T, step_mode=mode)
    alpha = np.asarray(alpha)
    want = img if alpha.ndim == 3 else img[..., 3]
    assert np.abs(strided(alpha, pixel_stride) - strided(want, pixel_stride)).max() <= 1e-6
