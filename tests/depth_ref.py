"""CPU reference of the depth render (test infrastructure, in the spirit of tests/mesh_ref.py).

A fold over tests/march_ref.py's samples, the one restatement of the oracle's march, with the depth sum of prv_render_depth
(include/prv.h):
  * D = sum_i w_i t_i over exactly the samples, weights and early termination of the colour composite;
  * per sub-sample z = D * dot(d, f), f = column 2 of the camera's c2w, normalised;
  * per pixel the sub-samples summed in order, then scaled by 1 / spp.
"""
import numpy as np

from tests.march_ref import assert_alpha_is_the_oracles, composite, f32, forward_cos, mean, ray_samples, rays


def render(lib, field, cam, w, h, S=128, spp=1, min_T=1e-4, step_mode=0, pixel_stride=1):
    """-> (h, w, 5) float32: r, g, b, alpha (as OracleField.render) and z (premultiplied z-depth, engine units).
    pixel_stride n > 1: only the pixels whose row-major index is a multiple of n are computed (`march_ref.strided` picks the
    same ones out of an image); the others stay 0."""
    sub = np.zeros((spp, h, w, 5), np.float32)
    for k, y, x, o, d in rays(lib, cam, w, h, spp, pixel_stride):
        _, ts, alphas, rgbs, _ = ray_samples(lib, field, o, d, step_mode, S, f32(min_T))
        (r, g, b, D), T = composite(alphas, [(*c, t) for c, t in zip(rgbs, ts)], 4)
        sub[k, y, x] = (r, g, b, f32(1) - T, f32(D * forward_cos(cam, d)))
    return mean(sub)


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
    assert_alpha_is_the_oracles(f, ocam, w, h, S, spp, min_T, mode, want[..., :4], pixel_stride)  # its colour too
    return want
