"""CPU reference of the surface render (test infrastructure, in the manner of tests/entropy_ref.py).

A fold over tests/march_ref.py's samples, the one restatement of the oracle's march, with the first-crossing locator of
prv_render_surface (include/prv.h):
  * the ray's live samples (t_i, alpha_i) are march_ref.ray_samples';
  * H and 1 - T_end of those opacities by entropy_ref.entropy_of_alphas;
  * Dm = t_i of the first sample after which T = T * (1 - alpha_i) is <= T_cross, or 0; hit = Dm > 0;
  * per sub-sample z = Dm * dot(d, f) with march_ref.forward_cos;
  * per pixel the sub-samples summed in order, then scaled by 1 / spp (march_ref.mean).
A GPU ray's T differs from this one's by rounding (exp2 / rcp, MFMA order), so a ray whose T lands on T_cross may cross one
sample apart: `bounds` renders at T_cross * {1, 1 + s, 1 - s}, s = util.TERMINATION_SLACK, in one march.
"""
import numpy as np

from tests import entropy_ref, util
from tests.march_ref import assert_alpha_is_the_oracles, f32, fmaf, forward_cos, mean, ray_samples, rays


def surface_of_alphas(alphas, ts, level, min_T=0.0):
    """-> (Dm, hit) of a ray whose live samples have these opacities and ray parameters, in depth order, located at the
    accumulated opacity `level`: the threshold is 1.0f - level in float32, as the host forms it"""
    return _cross(alphas, ts, [f32(1) - f32(level)], min_T)[0]


def _cross(alphas, ts, T_cross, min_T):
    """[(Dm, hit) per threshold of T_cross]"""
    T = f32(1)
    Dm = [f32(0)] * len(T_cross)
    for a, t in zip(alphas, ts):
        T = f32(T * (f32(1) - f32(a)))
        for j, tc in enumerate(T_cross):
            if Dm[j] == 0 and T <= f32(tc):
                Dm[j] = f32(t)
        if T < f32(min_T):
            break
    return [(d, f32(1) if d > 0 else f32(0)) for d in Dm]


def render_variants(lib, field, cam, w, h, T_cross, S=128, spp=1, min_T=1e-4, step_mode=0):
    """-> (spp, h, w, 2 + 2 n) float32 per SUB-SAMPLE: alpha, H, then (z, hit) for each of the n thresholds of T_cross"""
    out = np.zeros((spp, h, w, 2 + 2 * len(T_cross)), np.float32)
    min_T = f32(min_T)
    for k, y, x, o, d in rays(lib, cam, w, h, spp):
        _, ts, alphas, _, _ = ray_samples(lib, field, o, d, step_mode, S, min_T)
        if not ts:
            continue
        H, T = entropy_ref.entropy_of_alphas(alphas, min_T)
        cos = forward_cos(cam, d)
        px = [f32(1) - T, H]
        for Dm, hit in _cross(alphas, ts, T_cross, min_T):
            px += [f32(Dm * cos), hit]
        out[k, y, x] = px
    return out


def render(lib, field, cam, w, h, T_cross, S=128, spp=1, min_T=1e-4, step_mode=0):
    """-> (h, w, 4) float32 per pixel: H, alpha, z, hit for the threshold T_cross"""
    sub = render_variants(lib, field, cam, w, h, [T_cross], S, spp, min_T, step_mode)
    return mean(sub[..., [1, 0, 2, 3]])


class Bounds:
    """the reference at T_cross * {1, 1 + s, 1 - s}: z_lo / z_hi / hit_lo / hit_hi (h, w) = the mean over the sub-samples of the
    per-sub-sample minimum / maximum across the three variants; z_var / hit_var (3, h, w) = each variant's own pixel"""

    def __init__(self, sub):
        z, hit = sub[..., 2::2], sub[..., 3::2]  # (spp, h, w, 3)
        self.z_lo, self.z_hi = mean(z.min(axis=-1)), mean(z.max(axis=-1))
        self.hit_lo, self.hit_hi = mean(hit.min(axis=-1)), mean(hit.max(axis=-1))
        self.z_var = np.stack([mean(z[..., j]) for j in range(3)])
        self.hit_var = np.stack([mean(hit[..., j]) for j in range(3)])
        self.alpha = mean(sub[..., 0])

    @property
    def hit_pixels(self):
        return self.hit_hi > 0

    @property
    def loose(self):
        """pixels where the three variants disagree, for z or for hit"""
        return (self.z_lo != self.z_hi) | (self.hit_lo != self.hit_hi)


def bounds(oracle, f, ocam, w, h, S, spp, min_T, mode, level):
    T_cross = f32(1) - f32(level)
    sub = render_variants(oracle.lib(), f, ocam, w, h, [f32(v) for v in util.termination_variants(T_cross)], S, spp, min_T, mode)
    b = Bounds(sub)
    assert_alpha_is_the_oracles(f, ocam, w, h, S, spp, min_T, mode, b.alpha)
    return b


# ---- the inputs of the comparison against this reference (tests/test_gpu_surface.py), shared with the cap that keeps it honest
# (tests/test_surface_host.py): every entry of tests/instances.py's matrix x {fixed S = 96; engine's rule} at level 0.5, and
# one more configuration at level 0.25 with min_T = 0.01; two views of FW x FH pixels; spp 1 and 3 of each
FW, FH = 44, 30  # tests/test_gpu_select.py's footprint size: the width is no multiple of 64
S_FIXED = 96
VIEWS = [0, 3]
SPP = (1, 3)
EXTRA = ("F4_5", 1, 0.25, 0.01)
# The matrix's fields at their own density (bias 3) are so thin that a sample near the crossing takes 1-10 % off T: as much as
# the slack between the variants, so on 7-9 % of the hit pixels (fixed rule, 1 spp), 17-22 % (3 spp) and 42-51 % (engine's
# rule, dt = sqrt(3) / 1024) the variants cross a sample apart (measured: tests/test_surface_host.py's cap).  The share is
# about 2 s / -ln(1 - alpha) per sub-sample, so the cases use the same fields with a larger density bias, chosen per stepping
# rule so that crossings still take several samples: the layout and the instance do not depend on it.
DENSITY_BIAS = {0: 4.5, 1: 6.5}


def case_entry(name, mode):
    """the matrix entry `name` with the density of the cases under stepping rule `mode`"""
    from tests import instances

    e = instances.MATRIX[name]
    return instances.Entry(dict(e.kw, density_bias=DENSITY_BIAS[mode]), e.n_dense, e.n_hashed, e.instance, e.wide)


def cases():
    """[(entry name, stepping rule, level, min_T)]"""
    from tests import instances

    return [(name, mode, 0.5, 1e-4) for name in instances.MATRIX for mode in (0, 1)] + [EXTRA]


def case_transforms(oracle):
    tms, scale, offset = util.hemisphere_transforms(oracle, util.fibonacci_hemisphere(6))
    return tms[VIEWS], scale, offset


def case_bounds(oracle, f, ocams, mode, level, min_T):
    """-> {spp: [Bounds per view]}.  Sub-sample k's offset does not depend on spp (orc_spp_offset(k)), so the 1-spp image is
    sub-sample 0 of the 3-spp one: one march serves both"""
    T_cross = f32(1) - f32(level)
    tc = [f32(v) for v in util.termination_variants(T_cross)]
    S = S_FIXED if mode == 0 else 0
    out = {1: [], 3: []}
    for oc in ocams:
        sub = render_variants(oracle.lib(), f, oc, FW, FH, tc, S, 3, min_T, mode)
        for spp in SPP:
            b = Bounds(sub[:spp])
            assert_alpha_is_the_oracles(f, oc, FW, FH, S, spp, min_T, mode, b.alpha)
            out[spp].append(b)
    return out


# ---- two separated semi-opaque shells along a view axis (tests/test_gpu_surface.py: what the locator is for)
SHELL_W, SHELL_H, SHELL_S = 32, 24, 96
SHELL_CELLS = ((19,), (9, 10, 11, 12))  # occupancy cells along z of the shell nearer a camera above the object (thin: a ray leaves it with most of its T), and of the farther one


def two_shell_params(oracle, kw, seed):
    """-> (table, mlp, occ) of the synthetic field of (kw, seed) with its occupancy replaced by two slabs of cells across z: what
    lies between them, in front and behind is empty, so every ray from above meets two sheets of the field's own density"""
    f = oracle.OracleField(oracle.desc(**kw), seed=seed)
    table, mlp, _ = f.params()
    f.close()
    R = kw["occ_res"]
    cells = np.zeros((R, R, R), bool)  # [z, y, x]: bit x + R * (y + R * z)
    for shell in SHELL_CELLS:
        cells[list(shell)] = True
    occ = np.packbits(cells.ravel(), bitorder="little").view(np.uint32)
    return table, mlp, occ


def shell_rays(lib, field, cam, w, h, S, min_T, T_cross):
    """per pixel of a 1-spp fixed-S render, from the oracle alone -> dict of (h, w) arrays: w1 = the opacity accumulated over the
    first shell, t_gap0 / t_gap1 = the ray parameters of the first shell's last sample and of the second shell's first one (0
    where the ray does not meet both), dt, cos, and t_cross (3, h, w) = the crossing sample's t under each threshold (0: none)"""
    out = {k: np.zeros((h, w), np.float32) for k in ("w1", "t_gap0", "t_gap1", "dt", "cos")}
    out["t_cross"] = np.zeros((len(T_cross), h, w), np.float32)
    z_mid = (SHELL_CELLS[0][0] + SHELL_CELLS[1][-1] + 1) / 2.0 / field.desc.occ_res
    for _, y, x, o, d in rays(lib, cam, w, h, 1):
        _, ts, alphas, _, dt = ray_samples(lib, field, o, d, 0, S, f32(min_T))
        first = [i for i, t in enumerate(ts) if fmaf(t, d[2], o[2]) > z_mid]
        if not first or len(first) == len(ts) or first != list(range(len(first))):
            continue  # the ray does not go through the near shell and then the far one
        T = f32(1)
        for a in alphas[: len(first)]:
            T = f32(T * (f32(1) - a))
        out["w1"][y, x] = f32(1) - T
        out["t_gap0"][y, x], out["t_gap1"][y, x] = ts[len(first) - 1], ts[len(first)]
        out["dt"][y, x], out["cos"][y, x] = dt, forward_cos(cam, d)
        out["t_cross"][:, y, x] = [Dm for Dm, _ in _cross(alphas, ts, T_cross, min_T)]
    return out
