"""Surface coverage without a GPU: the CPU reference of the stage (tests/coverage_ref.py) gives the answers one can work out by
hand, the header states the arithmetic the reference restates, and the C ABI's new symbols are declared, exported and bound."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from nerf_prv_amd import _lib, api
from tests import coverage_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32

# view A sits at the origin and looks along +z; view B sits at (0, 0, 3) and looks back along -z (a half turn about y)
CAM_A = ref.Cam([[1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 1, 0]], 4, 4, 2, 2)
CAM_B = ref.Cam([[-1, 0, 0, 0], [0, 1, 0, 0], [0, 0, -1, 3]], 4, 4, 2, 2)


# ---- the reference, by hand
def test_three_points_and_two_views_worked_out_on_paper():
    """4 x 4 pixels, focal length 4, principal point (2, 2).  P0 = (0, 0, 1) and P1 = (0, 0, 2) lie on both optical axes, P2 =
    (0.25, 0, 1) beside them.  From A: P0 -> pixel (2, 2) at z 1, P1 -> the same pixel at z 2 (hidden: 2 > 1 * 1.02), P2 -> u =
    4 * 0.25 + 2 = 3, pixel (3, 2) at z 1.  From B the depths are 3 - z and x flips: P1 -> (2, 2) at z 1, P0 behind it at z 2,
    P2 -> u = 4 * (-0.25 / 2) + 2 = 1.5, pixel (1, 2) at z 2"""
    pts = np.array([[0, 0, 1], [0, 0, 2], [0.25, 0, 1]], np.float32)
    vis, depth = ref.matrix([CAM_A, CAM_B], pts, 4, 4, 1, 0.02)
    assert vis.tolist() == [[True, False, True], [False, True, True]]
    want_a, want_b = np.zeros((4, 4), np.float32), np.zeros((4, 4), np.float32)
    want_a[2, 2] = want_a[2, 3] = 1
    want_b[2, 2], want_b[2, 1] = 1, 2
    assert np.array_equal(depth[0], want_a) and np.array_equal(depth[1], want_b)
    assert [int(ref.pack(v)[0]) for v in vis] == [0b101, 0b110]
    covered, first = ref.curve(vis, [0, 1])
    assert covered == [2, 3] and first.tolist() == [0, 1, 0]
    assert ref.curve(vis, [1, 0])[0] == [2, 3] and ref.curve(vis, [1])[1].tolist() == [ref.NEVER, 0, 0]
    assert ref.greedy(vis, 2) == ([0, 1], [2, 3])  # both see two points: the first view wins the tie
    # a tolerance of 1 lets A see through P0 (2 <= 1 * 2); a 3 x 3 block of P2 reaches pixel (2, 2) at equal depth: nothing changes
    assert ref.matrix([CAM_A], pts, 4, 4, 1, 1.0)[0].tolist() == [[True, True, True]]
    assert ref.matrix([CAM_A], pts, 4, 4, 3, 0.02)[0].tolist() == [[True, False, True]]
    # the projection's edges: behind the camera, at z = 1e-6 exactly, outside the image, not finite
    odd = np.array([[0, 0, -1], [0, 0, 1e-6], [1, 0, 1], [-0.5, 0, 1], [-0.50001, 0, 1], [np.nan, 0, 1], [0, np.inf, 1], [0, 0, np.inf]], np.float32)
    assert ref.matrix([CAM_A], odd, 4, 4, 1, 0.02)[0].tolist() == [[False, False, False, True, False, False, False, False]]


def sphere_cloud(n, seed=0, centre=(0.5, 0.5, 0.5), radius=0.3):
    d = np.random.default_rng(seed).normal(size=(n, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    return (np.asarray(centre) + radius * d).astype(np.float32)


def test_two_opposite_cameras_each_see_a_proper_part_of_a_sphere():
    pts = sphere_cloud(20000)
    front = ref.Cam([[1, 0, 0, 0.5], [0, 1, 0, 0.5], [0, 0, 1, -1.5]], 120, 120, 32, 32)
    back = ref.Cam([[-1, 0, 0, 0.5], [0, 1, 0, 0.5], [0, 0, -1, 2.5]], 120, 120, 32, 32)
    vis, depth = ref.matrix([front, back], pts, 64, 64, 2, 0.02)
    a, b, both = int(vis[0].sum()), int(vis[1].sum()), int((vis[0] | vis[1]).sum())
    assert 0 < a < len(pts) and 0 < b < len(pts) and both > max(a, b) and both <= len(pts)
    assert vis[0][pts[:, 2] < 0.25].mean() > 0.9 and not vis[0][pts[:, 2] > 0.7].any()  # the near cap, never the far one
    assert (depth[0] > 0).sum() > 500 and depth[0][0, 0] == 0
    # depth_tol = 0: exactly the nearest points of each pixel, so the visible points of a pixel share one depth
    vis0, _ = ref.matrix([front], pts, 64, 64, 2, 0.0)
    ok, u, v, z = ref.project(front, pts)
    pix = (np.floor(v).astype(np.int64) * 64 + np.floor(u).astype(np.int64))[vis0[0]]
    zs = z[vis0[0]]
    assert 0 < vis0[0].sum() <= a
    for p in np.unique(pix):
        assert len(np.unique(zs[pix == p])) == 1


def test_an_occluding_plane_hides_what_lies_behind_it():
    ys, xs = np.mgrid[0:4, 0:4]
    plane = np.stack([(xs.ravel() + 0.5 - 2) / 4, (ys.ravel() + 0.5 - 2) / 4, np.ones(16)], axis=1).astype(np.float32)  # one point per pixel, z = 1
    rng = np.random.default_rng(1)
    behind = np.concatenate([rng.uniform(-0.4, 0.4, (200, 2)), rng.uniform(1.5, 3.0, (200, 1))], axis=1).astype(np.float32)
    vis, depth = ref.matrix([CAM_A, CAM_B], np.concatenate([plane, behind]), 4, 4, 1, 0.02)
    assert vis[0][:16].all() and not vis[0][16:].any() and np.all(depth[0] == 1)
    assert vis[1][16:].any()  # from the other side the plane hides nothing of them


def test_greedy_tie_rule_and_zero_gain_rounds():
    vis = np.array([[1, 1, 0, 0, 0], [0, 0, 1, 1, 0], [1, 1, 0, 0, 0], [0, 0, 0, 0, 0], [1, 1, 1, 0, 0]], bool)
    assert ref.greedy(vis, 1) == ([4], [3])
    # after view 4: views 1 gains 1, the others 0; then three zero-gain rounds in position order
    assert ref.greedy(vis, 5) == ([4, 1, 0, 2, 3], [3, 4, 4, 4, 4])
    vis[4] = False
    assert ref.greedy(vis, 3) == ([0, 1, 2], [2, 4, 4])  # views 0, 1 and 2 tie at 2: the smallest position first


def test_an_order_with_repeats_gains_nothing_on_the_repeat():
    vis = np.array([[1, 1, 0, 0], [0, 1, 1, 0]], bool)
    covered, first = ref.curve(vis, [1, 1, 0, 1, 0])
    assert covered == [2, 2, 3, 3, 3] and first.tolist() == [2, 0, 0, ref.NEVER]
    assert ref.curve(vis, [])[0] == [] and (ref.curve(vis, [])[1] == ref.NEVER).all()


def test_bit_packing_is_little_endian_in_the_word():
    vis = np.zeros(130, bool)
    vis[[0, 63, 64, 129]] = True
    assert ref.pack(vis).tolist() == [1 | (1 << 63), 1, 2]
    assert ref.pack(np.zeros(0, bool)).tolist() == []


# ---- the header
def header_text():
    return open(os.path.join(ROOT, "include", "prv.h")).read()


def test_header_states_the_arithmetic_the_reference_restates():
    text = re.sub(r"\s*\n\s*\*\s*", " ", header_text())  # comment lines joined
    text = re.sub(r"\s+", " ", text)
    for phrase in ("d_a = e_a - o_a",
                   "c_a = fmaf(M[0][a], d_0, fmaf(M[1][a], d_1, M[2][a] * d_2))",
                   "c_2 > 1e-6f",
                   "x = c_0 / c_2, y = c_1 / c_2",
                   "u = fmaf(fx, x, cx), v = fmaf(fy, y, cy), z = c_2",
                   "fx0 = floorf(u - 0.5f * ps + 0.5f), fy0 = floorf(v - 0.5f * ps + 0.5f)",
                   "fx0 > -ps, fx0 < (float)width, fy0 > -ps and fy0 < (float)height",
                   "z <= zmin * tol1",
                   "tol1 = 1.0f + depth_tol",
                   "gain_j = popcount(bits[order[j]] & ~C)",
                   "on a tie the smallest position"):
        assert phrase in text, phrase
    # the limits, and that the default tolerance is a choice
    for pattern in (r"POINT z-buffer", r"holes between the points of a sparse cloud", r"grazing angles", r"no incidence-angle",
                    r"SINGLE-RANK", r"default 0\.02 is an option value, NOT a measured one", r"256 MiB"):
        assert re.search(pattern, text), pattern
    assert re.search(r"#define\s+PRV_ABI_VERSION\s+5\b.*prv_coverage_\*.*additive", header_text())


# ---- the ABI
NEW = (("prv_coverage_default_opts", 1), ("prv_coverage_create", 11), ("prv_coverage_info", 4), ("prv_coverage_visible", 2),
       ("prv_coverage_bits", 3), ("prv_coverage_curve", 5), ("prv_coverage_greedy", 4), ("prv_coverage_destroy", 1))


def test_new_symbols_declared_exported_and_bound():
    text = re.sub(r"/\*.*?\*/", "", header_text(), flags=re.S)
    out = subprocess.check_output(["nm", "-D", "--defined-only", os.path.join(ROOT, "nerf_prv_amd", "libprv_hip.so")], text=True)
    exported = {l.split()[-1] for l in out.splitlines() if " T " in l}
    for name, n_args in NEW:
        m = re.search(r"\b(?:int|void)\s+" + name + r"\s*\(([^;]*)\)\s*;", text)
        assert m, f"{name} is not declared in prv.h"
        assert len([a for a in m.group(1).split(",") if a.strip()]) == n_args
        assert name in exported
        assert len(_lib.SIGNATURES[name][1]) == n_args
    assert re.search(r"typedef\s+struct\s+prv_coverage\s+prv_coverage\s*;", text)
    lib = _lib.load()
    assert lib.prv_abi_version() == 5
    o = _lib.CoverageOpts()
    assert lib.prv_coverage_default_opts(C.byref(o)) == 0 and (o.point_size, o.depth_tol) == (1, float(f32(0.02)))
    assert C.sizeof(_lib.CoverageOpts) == 8
    assert lib.prv_coverage_default_opts(None) == _lib.PRV_E_INVALID
    for attr in ("info", "visible", "bits", "curve", "greedy", "close", "__enter__", "__exit__"):
        assert hasattr(api.Coverage, attr)
    assert hasattr(api.Context, "coverage") and hasattr(api.Testbed, "compute_coverage")


@pytest.mark.parametrize("kw,text", [(dict(point_size=0), "point_size"), (dict(point_size=65), "point_size"), (dict(depth_tol=-0.5), "depth_tol"),
                                     (dict(depth_tol=float("nan")), "depth_tol"), (dict(depth_tol=float("inf")), "depth_tol")])
def test_bad_options_give_e_invalid_with_a_message(kw, text):
    """the options are checked before anything else, so this needs no GPU: the message is the no-context one's"""
    lib = _lib.load()
    o = _lib.CoverageOpts(1, 0.02)
    for k, v in kw.items():
        setattr(o, k, v)
    h = C.c_void_p()
    rc = lib.prv_coverage_create(None, None, 0, None, None, 1, 8, 8, C.byref(o), None, C.byref(h))
    assert rc == _lib.PRV_E_INVALID and text in lib.prv_last_error(None).decode() and not h.value


def test_a_null_handle_is_e_invalid_everywhere():
    lib = _lib.load()
    n = C.c_uint64()
    assert lib.prv_coverage_info(None, C.byref(n), None, None) == _lib.PRV_E_INVALID
    assert lib.prv_coverage_visible(None, None) == _lib.PRV_E_INVALID
    assert lib.prv_coverage_bits(None, 0, None) == _lib.PRV_E_INVALID
    assert lib.prv_coverage_curve(None, None, 0, None, None) == _lib.PRV_E_INVALID
    assert lib.prv_coverage_greedy(None, 1, None, None) == _lib.PRV_E_INVALID
    assert "NULL" in lib.prv_last_error(None).decode()
    lib.prv_coverage_destroy(None)


def test_coverage_config_is_the_default_plus_the_keys():
    strip = lambda t: [l for l in t.splitlines() if l.strip() and not l.lstrip().startswith("#")]
    a = strip(open(os.path.join(ROOT, "configs", "DefaultConfiguration.yaml")).read())
    b = strip(open(os.path.join(ROOT, "configs", "CoverageEval.yaml")).read())
    assert b[: len(a)] == a and b[len(a)] == "evaluate_coverage: 1"
    assert {l.split(":")[0] for l in b[len(a):]} <= {"evaluate_coverage", "coverage_point_size", "coverage_depth_tol", "coverage_width",
                                                    "coverage_height", "geometry_mc_res", "geometry_samples", "geometry_reference"}
