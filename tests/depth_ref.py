"""CPU reference of the depth render (test infrastructure, in the spirit of tests/mesh_ref.py).

Restates the oracle's march (oracle/prv_oracle.c: march_ray, render_worker) with the depth sum of prv_render_depth
(include/prv.h), through the oracle's exported primitives only (orc_spp_offset, orc_raygen, orc_ray_aabb, orc_occupied,
orc_eval):
  * D = sum_i w_i t_i over exactly the samples, weights and early termination of the colour composite;
  * per sub-sample z = D * dot(d, f), f = column 2 of the camera's c2w, normalised;
  * per pixel the sub-samples summed in order, then scaled by 1 / spp.
fmaf is computed in float64 and rounded to float32; everything else is float32 arithmetic.
"""
import ctypes as C

import numpy as np

f32 = np.float32
NGP_DT = f32(np.sqrt(f32(3.0)) / f32(1024.0))


def fmaf(a, b, c):
    return f32(np.float64(a) * np.float64(b) + np.float64(c))


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def forward_cos(cam, d):
    """dot(d, f), f = column 2 of c2w normalised (the depth kernel's order of operations)"""
    m = np.frombuffer(cam.c2w, np.float32)
    fx, fy, fz = f32(m[2]), f32(m[6]), f32(m[10])
    inv = f32(1.0) / f32(np.sqrt(fmaf(fx, fx, fmaf(fy, fy, f32(fz * fz)))))
    return f32(fmaf(d[0], fx, fmaf(d[1], fy, f32(d[2] * fz))) * inv)


def march_ray(lib, field, o, d, step_mode, S, min_T):
    """-> (r, g, b, a, D) of one ray: the oracle's march_ray plus the depth sum"""
    t0, t1 = C.c_float(), C.c_float()
    if not lib.orc_ray_aabb(_p(o), _p(d), C.byref(t0), C.byref(t1)):
        return np.zeros(5, np.float32)
    t0, t1 = f32(t0.value), f32(t1.value)
    if step_mode == 1:
        dt, n = NGP_DT, 1024
    else:
        dt, n = f32((t1 - t0) / f32(S)), S
    T, r, g, b, D = f32(1), f32(0), f32(0), f32(0), f32(0)
    p = np.zeros(3, np.float32)
    rgb = np.zeros(3, np.float32)
    raw = np.zeros(32, np.float32)
    sigma = C.c_float()
    for i in range(n):
        t = fmaf(f32(i) + f32(0.5), dt, t0)
        if step_mode == 1 and not t < t1:
            break
        p[:] = (fmaf(t, d[0], o[0]), fmaf(t, d[1], o[1]), fmaf(t, d[2], o[2]))
        if not lib.orc_occupied(field.ptr, _p(p)):
            continue
        lib.orc_eval(field.ptr, _p(p), _p(d), C.byref(sigma), _p(rgb), _p(raw))
        alpha = f32(1) - f32(np.exp(-f32(f32(sigma.value) * dt)))
        wgt = f32(alpha * T)
        r, g, b = fmaf(wgt, rgb[0], r), fmaf(wgt, rgb[1], g), fmaf(wgt, rgb[2], b)
        D = fmaf(wgt, t, D)
        T = f32(T * (f32(1) - alpha))
        if T < min_T:
            break
    return np.array([r, g, b, f32(1) - T, D], np.float32)


def render(lib, field, cam, w, h, S=128, spp=1, min_T=1e-4, step_mode=0, pixel_stride=1):
    """-> (h, w, 5) float32: r, g, b, alpha (as OracleField.render) and z (premultiplied z-depth, engine units).
    pixel_stride n > 1: only the pixels whose row-major index is a multiple of n are computed (`strided` picks the same
    ones out of an image); the others stay 0."""
    out = np.zeros((h, w, 5), np.float32)
    min_T = f32(min_T)
    o, d = np.zeros(3, np.float32), np.zeros(3, np.float32)
    ox, oy = C.c_float(), C.c_float()
    inv_spp = f32(1) / f32(spp)
    offs = []
    for k in range(spp):
        lib.orc_spp_offset(k, C.byref(ox), C.byref(oy))
        offs.append((ox.value, oy.value))
    for y in range(h):
        for x in range(w):
            if (y * w + x) % pixel_stride:
                continue
            acc = np.zeros(5, np.float32)
            for k in range(spp):
                lib.orc_raygen(C.byref(cam), x, y, C.c_float(offs[k][0]), C.c_float(offs[k][1]), _p(o), _p(d))
                px = march_ray(lib, field, o, d, step_mode, S, min_T)
                px[4] = f32(px[4] * forward_cos(cam, d))
                acc = (acc + px).astype(np.float32)
            out[y, x] = (acc * inv_spp).astype(np.float32)
    return out


def strided(img, pixel_stride):
    """(h, w, c) -> (n, c): the pixels `render(..., pixel_stride=)` computes"""
    img = np.asarray(img)
    return img.reshape(img.shape[0] * img.shape[1], -1)[::pixel_stride]


# ---- what the GPU depth tests share (tests/test_gpu_depth.py, tests/test_gpu_instances.py)
def both(ctx, slot, cs, opts, ids=None):
    """render_depth and render of the same views -> rgba, depth, stats, plain rgba, plain stats"""
    rgba, depth, st = ctx.render_depth(slot, cs, ids, opts)
    plain, st0 = ctx.render(slot, cs, ids, opts)
    return rgba.cpu().numpy(), depth.cpu().numpy(), st, plain.cpu().numpy(), st0


def check_identity(rgba, st, plain, st0):
    assert np.array_equal(rgba.view(np.uint32), plain.view(np.uint32))  # bit for bit
    for k in ("rays", "samples_nominal", "samples_evaluated", "samples_live"):
        assert getattr(st, k) == getattr(st0, k), k


def reference(oracle, f, ocam, w, h, S, spp, min_T, mode, pixel_stride=1):
    want = render(oracle.lib(), f, ocam, w, h, S, spp, min_T, mode, pixel_stride)
    # self-check: the restatement's colour is the oracle's own render
    img, _ = f.render(ocam, w, h, S, spp, min_T, step_mode=mode)
    assert np.abs(strided(want, pixel_stride)[:, :4] - strided(img, pixel_stride)).max() <= 1e-6
    return want
