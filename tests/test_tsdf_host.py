"""Depth-map fusion without a GPU: the reference of tests/tsdf_ref.py stands on its own (a plane seen by one view, order and
batching, every kind of skipped sample, the colour's own weight, the mask rules of the extraction, a sphere fused from eight
views), and the header section, the ctypes mirrors and the exported symbols agree."""
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np
import pytest

from tests import mesh_ref, raster_ref, tsdf_ref
from tests.coverage_ref import Cam, project
from tests.march_ref import f32

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LO, HI = (0.1, 0.2, 0.3), (0.9, 0.7, 0.8)


def axis_cam(w=16, h=16, focal=8.0, eye=(0.5, 0.5, -1.0)):
    """a camera whose axes are the engine's: the depth of a point is its z minus the eye's, exactly"""
    c2w = np.concatenate([np.eye(3), np.asarray(eye, np.float64).reshape(3, 1)], 1)
    return Cam(c2w, focal, focal, 0.5 * w, 0.5 * h)


def state_bytes(v):
    return b"".join(np.ascontiguousarray(a).tobytes() for a in (v.D, v.W, v.WC, v.C))


# ---- 1. one view against a plane
def test_one_view_against_a_plane_is_exact():
    cam, z0 = axis_cam(), f32(1.5)
    vol = tsdf_ref.Volume((9, 7, 5), LO, HI, 0.125, colors=False)
    vol.integrate([cam], 16, 16, np.full((1, 16, 16), z0, np.float32))
    z = vol.points[:, 2] - f32(-1.0)  # one float32 subtraction: fmaf(0, d0, fmaf(0, d1, 1 * d2)) is d2
    ok, u, v, zp = project(cam, vol.points)
    assert ok.all() and (zp == z).all() and (np.floor(u) >= 0).all() and (np.floor(u) < 16).all() and (np.floor(v) >= 0).all() and (np.floor(v) < 16).all()
    sdf = z0 - z
    seen = ~(sdf < -vol.trunc)
    want = np.minimum(sdf * vol.inv, f32(1)).astype(np.float32)
    assert seen.any() and (~seen).any() and (want[seen] < 1).any() and (want[seen] == 1).any() and (want[seen] < 0).any()
    assert (vol.W[seen] == 1).all() and (vol.D[seen].view(np.uint32) == want[seen].view(np.uint32)).all()
    assert (vol.W[~seen] == 0).all() and (vol.D[~seen] == 0).all()  # z - z0 > trunc: behind the plane, unobserved
    assert ((z - z0 > vol.trunc) == ~seen).all()
    info = vol.info()
    assert info["observed"] == int(seen.sum()) and info["inside"] == int((seen & (want < 0)).sum())


# ---- 2. order and batching
def two_view_input():
    rng = np.random.default_rng(5)
    cams = [axis_cam(), tsdf_ref.look_at((1.6, 0.2, 0.4), (0.5, 0.45, 0.55), 16, 16, math.radians(60))]
    depth, weight, rgba8, _, _ = tsdf_ref.adversarial_images(rng, 2, 16, 16, 1.3)
    return cams, depth, weight, rgba8


def test_one_call_equals_the_views_one_by_one():
    cams, depth, weight, rgba8 = two_view_input()
    both = tsdf_ref.Volume((9, 7, 5), LO, HI, 0.2)
    both.integrate(cams, 16, 16, depth, weight, rgba8)
    split = tsdf_ref.Volume((9, 7, 5), LO, HI, 0.2)
    alone = []
    for j in range(2):
        split.integrate(cams[j:j + 1], 16, 16, depth[j:j + 1], weight[j:j + 1], rgba8[j:j + 1])
        alone.append(tsdf_ref.Volume((9, 7, 5), LO, HI, 0.2))
        alone[j].integrate(cams[j:j + 1], 16, 16, depth[j:j + 1], weight[j:j + 1], rgba8[j:j + 1])
    assert ((alone[0].W > 0) & (alone[1].W > 0)).any() and ((alone[0].WC > 0) & (alone[1].WC > 0)).any()  # points both views update
    assert state_bytes(both) == state_bytes(split)
    again = tsdf_ref.Volume((9, 7, 5), LO, HI, 0.2)
    again.integrate(cams, 16, 16, depth, weight, rgba8)
    assert state_bytes(both) == state_bytes(again)


# ---- 3. skipped samples
def test_every_bad_sample_is_skipped():
    rng = np.random.default_rng(7)
    w, h = 12, 10
    # a camera inside the box looking along +z, narrow: points behind it, points beside the image, points in it
    cam = axis_cam(w, h, focal=9.0, eye=(0.5, 0.45, 0.45))
    vol = tsdf_ref.Volume((17, 13, 9), LO, HI, 10.0)  # (a truncation that cuts nothing: only the named reasons skip)
    ok, u, v, z = project(cam, vol.points)
    with np.errstate(all="ignore"):
        hit = ok & (np.floor(u) >= 0) & (np.floor(u) < w) & (np.floor(v) >= 0) & (np.floor(v) < h)
    met = np.floor(v[hit]).astype(int) * w + np.floor(u[hit]).astype(int)
    assert len(np.unique(met)) >= 24  # the pixels that points fall into take every kind of value
    depth, weight, rgba8, bad_d, bad_w = tsdf_ref.adversarial_images(rng, 1, w, h, 1.4, first=met)
    vol.integrate([cam], w, h, depth, weight, rgba8)
    behind = ~ok
    with np.errstate(all="ignore"):
        fu, fv = np.floor(u), np.floor(v)
    outside = ok & ~((fu >= 0) & (fu < w) & (fv >= 0) & (fv < h))
    inside = ok & ~outside
    xi, yi = np.where(inside, fu, 0).astype(int), np.where(inside, fv, 0).astype(int)
    bad = inside & (bad_d[0][yi, xi] | bad_w[0][yi, xi])
    good = inside & ~bad
    for name, sel in (("behind", behind), ("outside", outside), ("bad", bad), ("good", good)):
        assert sel.any(), name
    for sel in (behind, outside, bad):
        assert (vol.W[sel] == 0).all() and (vol.D[sel] == 0).all() and (vol.WC[sel] == 0).all() and (vol.C[:, sel] == 0).all()
    assert (vol.W[good] == weight[0][yi, xi][good]).all() and np.isfinite(vol.D).all() and np.isfinite(vol.C).all()
    # each sown kind met a point
    for val in (0.0, -1.5, np.inf, -np.inf):
        assert (depth[0][yi, xi][inside] == val).any(), val
    assert np.isnan(depth[0][yi, xi][inside]).any() and np.isnan(weight[0][yi, xi][inside]).any()
    assert (weight[0][yi, xi][inside] == 0).any() and (weight[0][yi, xi][inside] < 0).any()


# ---- 4. the colour's own weight
def test_free_space_in_front_of_another_surface_does_not_tint():
    cam = axis_cam()
    vol = tsdf_ref.Volume((9, 7, 5), (0.1, 0.2, 0.3), (0.9, 0.7, 0.5), 0.25)  # points at depth 1.3 .. 1.5
    red = np.zeros((1, 16, 16, 4), np.uint8)
    red[..., 0], red[..., 3] = 255, 255
    blue = np.zeros((1, 16, 16, 4), np.uint8)
    blue[..., 2], blue[..., 3] = 255, 255
    vol.integrate([cam], 16, 16, np.full((1, 16, 16), 1.4, np.float32), None, red)  # the first surface, through the points
    first = vol.WC.copy()
    assert (first == 1).all() and (vol.C[0] == 255).all() and (vol.C[1:] == 0).all()
    vol.integrate([cam], 16, 16, np.full((1, 16, 16), 3.0, np.float32), None, blue)  # a second surface far behind: free space here
    assert (vol.W == 2).all() and (vol.WC == 1).all() and (vol.C[0] == 255).all() and (vol.C[1:] == 0).all()
    assert (vol.D > 0).all()  # ... which still moved the distance towards free
    vol.integrate([cam], 16, 16, np.full((1, 16, 16), 1.45, np.float32), None, blue)  # a surface at the points does tint
    assert (vol.WC == 2).all() and (vol.C[0] == 127.5).all() and (vol.C[2] == 127.5).all()


# ---- 5. the mask rules, on a hand-made 4 x 3 x 3 grid
def hand_made():
    grid = np.full((3, 3, 4), -1.0, np.float32)  # (rz, ry, rx)
    grid[1, 1, 1], grid[1, 1, 2] = 1.0, 2.0      # two inside points in the middle: every one of the 12 cells holds surface
    return grid


def cells_of(v, lo, hi, shape):
    """per vertex the set of cells (x, y, z) whose closed box holds it"""
    rz, ry, rx = shape
    axes = mesh_ref.grid_axes((rx, ry, rz), lo, hi)
    out = []
    for p in v:
        cells = set()
        for cz in range(rz - 1):
            for cy in range(ry - 1):
                for cx in range(rx - 1):
                    c = (cx, cy, cz)
                    if all(axes[a][c[a]] <= p[a] <= axes[a][c[a] + 1] for a in range(3)):
                        cells.add(c)
        out.append(cells)
    return out


def test_mask_rules_on_a_hand_made_grid():
    grid = hand_made()
    full = mesh_ref.marching_cubes(grid, (0, 0, 0), (1, 1, 1), 0.0)
    none = tsdf_ref.masked_marching_cubes(grid, None, threshold=0.0)
    ones = tsdf_ref.masked_marching_cubes(grid, np.ones(grid.shape, bool), threshold=0.0)
    for got in (none, ones):  # no mask, and a mask that hides nothing: the unmasked extraction itself
        assert all(a.tobytes() == b.tobytes() for a, b in zip(got, full))
    assert len(full[2]) > 0
    valid = np.ones(grid.shape, bool)
    valid[1, 0, 1] = False  # the point (1, 0, 1): the four cells around it go, and with them the vertex on its edge to (1, 1, 1)
    valid[2, 2, 3] = False  # a corner point: only cell (2, 1, 1) goes, and every vertex of it is another cell's too
    kept = tsdf_ref.kept_cells(valid)
    assert kept.sum() == 7 and not kept[0, 0, 0] and not kept[1, 0, 1] and not kept[1, 1, 2]
    v, nrm, tri = tsdf_ref.masked_marching_cubes(grid, valid, threshold=0.0)
    assert 0 < len(tri) < len(full[2]) and 0 < len(v) < len(full[0])
    assert (np.unique(tri) == np.arange(len(v))).all()  # no unused vertex
    cells = cells_of(v, (0, 0, 0), (1, 1, 1), grid.shape)
    for t in tri:  # every triangle lies in one kept cell
        shared = cells[t[0]] & cells[t[1]] & cells[t[2]]
        assert any(kept[c[2], c[1], c[0]] for c in shared)
    # the vertices are the unmasked ones that a kept cell touches, in their order; triangles are the kept cells', in theirs
    fcells = cells_of(full[0], (0, 0, 0), (1, 1, 1), grid.shape)
    stay = np.array([any(kept[c[2], c[1], c[0]] for c in cs) for cs in fcells])
    assert (full[0][stay] == v).all() and (full[1][stay] == nrm).all()
    invalid = tsdf_ref.masked_marching_cubes(grid, np.zeros(grid.shape, bool), threshold=0.0)
    assert len(invalid[0]) == 0 and len(invalid[2]) == 0
    # an unobserved point is NaN in a volume's grid: the crossing edge into it exists for the unmasked extraction, not here
    nan_grid = grid.copy()
    nan_grid[0, 0, 0] = np.nan
    v2, _, tri2 = tsdf_ref.masked_marching_cubes(nan_grid, valid, threshold=0.0)
    assert v2.tobytes() == v.tobytes() and tri2.tobytes() == tri.tobytes() and np.isfinite(v2).all()


# ---- 6. a sphere fused from eight views of the hemisphere, on the reference alone
RADIUS, CENTRE = 0.3, np.array([0.5, 0.5, 0.5])
SPHERE_DEVIATION = 0.022414  # the largest | |v - centre| - radius | the reference's mesh has on this input (measured; see the test)


def icosphere(subdivisions=2):
    t = (1.0 + math.sqrt(5.0)) / 2.0
    v = [(-1, t, 0), (1, t, 0), (-1, -t, 0), (1, -t, 0), (0, -1, t), (0, 1, t), (0, -1, -t), (0, 1, -t), (t, 0, -1), (t, 0, 1), (-t, 0, -1), (-t, 0, 1)]
    f = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8),
         (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)]
    v = [np.asarray(p, np.float64) / np.linalg.norm(p) for p in v]
    for _ in range(subdivisions):
        mid, nf = {}, []

        def middle(a, b):
            key = (min(a, b), max(a, b))
            if key not in mid:
                m = v[a] + v[b]
                v.append(m / np.linalg.norm(m))
                mid[key] = len(v) - 1
            return mid[key]

        for a, b, c in f:
            ab, bc, ca = middle(a, b), middle(b, c), middle(c, a)
            nf += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        f = nf
    return (CENTRE + RADIUS * np.asarray(v)).astype(np.float32), np.asarray(f, np.uint32)


def hemisphere_eyes(n=8, distance=1.1):
    """n eyes on the upper (+z) hemisphere around CENTRE, a golden-angle spiral"""
    out = []
    for i in range(n):
        zz = (i + 0.5) / n
        r, phi = math.sqrt(1.0 - zz * zz), i * math.pi * (3.0 - math.sqrt(5.0))
        out.append(CENTRE + distance * np.array([r * math.cos(phi), r * math.sin(phi), zz]))
    return out


_sphere = {}


def fused_sphere():
    """the reference's volume and mesh of the sphere, computed once"""
    if not _sphere:
        w, h = 80, 45
        v, t = icosphere()
        cams = [tsdf_ref.look_at(eye, CENTRE, w, h, math.radians(50), up=(0.0, 1.0, 0.1)) for eye in hemisphere_eyes()]
        depth = np.stack([raster_ref.depth(c, v, t, w, h) for c in cams])
        vol = tsdf_ref.Volume((33, 33, 33), (0, 0, 0), (1, 1, 1), 3.0 / 32.0, colors=False)
        vol.integrate(cams, w, h, depth)
        _sphere.update(vol=vol, mesh=vol.mesh(), depth=depth)
    return _sphere


def test_fused_sphere_lies_on_the_sphere():
    """Measured on this input (an icosphere of 320 triangles, 8 views at 80 x 45, 33^3 points, trunc = 3 steps): the largest
    deviation of a mesh vertex from the sphere's radius is SPHERE_DEVIATION; the test asserts twice that, the factor absorbing
    nothing but a later change of the icosphere's tessellation."""
    s = fused_sphere()
    v, nrm, rgb, tri = s["mesh"]
    assert (s["depth"] > 0).any() and len(v) > 0 and len(tri) > 0
    dev = np.abs(np.linalg.norm(v.astype(np.float64) - CENTRE, axis=1) - RADIUS)
    print(f"fused sphere: {len(v)} vertices, {len(tri)} triangles, largest deviation {dev.max():.6f}, mean {dev.mean():.6f}")
    assert SPHERE_DEVIATION > 0 and dev.max() <= 2 * SPHERE_DEVIATION
    assert (np.unique(tri) == np.arange(len(v))).all() and np.isfinite(v).all()
    # seen from outside (the free side) the triangles are counter-clockwise: their normals point away from the centre
    a, b, c = (v[tri[:, k]].astype(np.float64) for k in range(3))
    out = np.einsum("ij,ij->i", np.cross(b - a, c - a), (a + b + c) / 3 - CENTRE)
    assert (out > 0).mean() > 0.99


def test_fused_sphere_counts():
    vol = fused_sphere()["vol"]
    info = vol.info()
    observed = int(np.count_nonzero(vol.W))  # (weights are sums of ones here: non-zero is positive)
    inside = sum(1 for d, w in zip(vol.D.tolist(), vol.W.tolist()) if w > 0 and d < 0)
    band = sum(1 for d, w in zip(vol.D.tolist(), vol.W.tolist()) if w > 0 and abs(d) < 1)
    print(info)
    assert info == dict(points=33 ** 3, observed=observed, inside=inside, band=band)
    assert 0 < info["inside"] < info["band"] < info["observed"] < info["points"]
    # the views stand above: the underside of the sphere is unobserved, so the mesh is open there
    grid, valid = vol.grid()
    assert not valid[:8].all() and np.isnan(grid[~valid]).all() and np.isfinite(grid[valid]).all()


# ---- 7. header and bindings
def header_text():
    return open(os.path.join(ROOT, "include", "prv.h")).read()


NEW_SYMBOLS = ("prv_tsdf_default_opts", "prv_tsdf_create", "prv_tsdf_integrate", "prv_tsdf_info", "prv_tsdf_grid", "prv_tsdf_mesh",
               "prv_tsdf_destroy", "prv_debug_tsdf_state", "prv_marching_cubes_grid_valid")


def test_header_section_and_abi():
    text = header_text()
    assert re.search(r"#define\s+PRV_ABI_VERSION\s+5\b.*prv_tsdf_\*.*prv_marching_cubes_grid_valid: additive", text)
    assert "depth-map fusion" in text and "ARITHMETIC CONTRACT of prv_tsdf_integrate" in text
    for frag in ("IN LIST ORDER", "sdf < -trunc", "D = fmaf(D, W, s * ws) / Wn", "fmaf(C[k], WC, (float)byte_k * ws) / WCn", "NOT a measured one",
                 "NEAREST-PIXEL", "SINGLE-RANK", "A cell is KEPT iff all eight"):
        assert frag in text, frag
    for name in NEW_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, text), name


def test_symbols_are_exported_and_bound():
    from nerf_prv_amd import _lib

    out = subprocess.check_output(["nm", "-D", "--defined-only", os.path.join(ROOT, "nerf_prv_amd", "libprv_hip.so")], text=True)
    exported = {l.split()[-1] for l in out.splitlines() if " T " in l}
    for name in NEW_SYMBOLS:
        assert name in exported and name in _lib.SIGNATURES, name
    lib = _lib.load()
    assert lib.prv_abi_version() == 5
    o = _lib.TsdfOpts()
    assert lib.prv_tsdf_default_opts(C.byref(o)) == 0 and lib.prv_tsdf_default_opts(None) == _lib.PRV_E_INVALID
    assert list(o.res) == [256] * 3 and list(o.aabb_lo) == [0.0] * 3 and list(o.aabb_hi) == [1.0] * 3 and o.colors == 1
    assert f32(o.trunc) == f32(3) * (f32(1) / f32(255))  # three steps of the default grid, in float32
    # a NULL handle is refused without a GPU, by every entry point that takes one
    assert lib.prv_tsdf_info(None, (C.c_uint64 * 4)()) == _lib.PRV_E_INVALID
    assert lib.prv_tsdf_mesh(None, 0.0, C.byref(C.c_void_p())) == _lib.PRV_E_INVALID
    lib.prv_tsdf_destroy(None)


def test_ctypes_mirror_is_the_c_compilers(tmp_path):
    from nerf_prv_amd import _lib, api

    src = tmp_path / "tsdf_caller.c"
    src.write_text(
        '#include "prv.h"\n#include <stdio.h>\n#include <stddef.h>\n'
        "int main(void) {\n"
        "  prv_tsdf_opts o;\n"
        "  if (prv_abi_version() != PRV_ABI_VERSION || PRV_ABI_VERSION != 5) return 1;\n"
        "  if (prv_tsdf_default_opts(&o) != PRV_OK) return 2;\n"
        '  printf("sizes %zu %zu %zu %zu\\n", sizeof(prv_tsdf_opts), offsetof(prv_tsdf_opts, aabb_lo), offsetof(prv_tsdf_opts, trunc),\n'
        "         offsetof(prv_tsdf_opts, colors));\n"
        '  printf("defaults %d %d %d %.9g %d\\n", o.res[0], o.res[1], o.res[2], (double)o.trunc, o.colors);\n'
        "  return 0;\n}\n")
    inc, libdir = os.path.join(ROOT, "include"), os.path.join(ROOT, "nerf_prv_amd")
    exe = tmp_path / "tsdf_caller"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", inc, str(src), "-o", str(exe), "-L", libdir, "-lprv_hip",
                           f"-Wl,-rpath,{libdir}", "-Wl,-rpath,/opt/rocm/lib", "-L/opt/rocm/lib"])
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    sizes = [int(x) for x in [l for l in out.stdout.splitlines() if l.startswith("sizes ")][0].split()[1:]]
    T = _lib.TsdfOpts
    assert sizes == [C.sizeof(T), T.aabb_lo.offset, T.trunc.offset, T.colors.offset], sizes
    assert "defaults 256 256 256" in out.stdout
    # the Python default of trunc is the library's rule on the caller's grid
    o = api.tsdf_opts((33, 17, 9), ((0.0, 0.0, 0.0), (1.0, 0.5, 0.5)))
    assert f32(o.trunc) == f32(3) * max(f32(1) / f32(32), f32(0.5) / f32(16), f32(0.5) / f32(8)) and o.colors == 1
    lib = _lib.load()
    d = _lib.TsdfOpts()
    lib.prv_tsdf_default_opts(C.byref(d))
    assert f32(api.tsdf_opts().trunc) == f32(d.trunc)
