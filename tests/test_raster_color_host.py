"""The colour images of a mesh without a GPU: the CPU reference (tests/raster_color_ref.py) gives the answers one can work out by
hand -- one colour everywhere, affine interpolation on a fronto-parallel triangle, the perspective-correct value on a slanted
quad where screen-space interpolation is far off, the depth reference's bits in the high words, the lower id on coincident
triangles; the C ABI's new symbols are declared, exported, bound and documented; the planner's .ply reader round-trips the
writer's file and refuses what it does not read."""
import os
import re
import subprocess

import numpy as np
import pytest

from nerf_prv_amd import _lib, api
from tests import coverage_ref, raster_color_ref as ref, raster_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W = H = 16
F = 16.0
# at the origin, looking along +z, focal length 16, principal point (0, 0): a point (x, y, z) lands on u = 16 x / z, v = 16 y / z
CAM = coverage_ref.Cam([[1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 1, 0]], F, F, 0, 0)


def at_pixels(uv, d):
    """engine points that project onto the pixel coordinates uv at depths d (exact where uv * d / 16 is)"""
    uv = np.asarray(uv, np.float64)
    d = np.broadcast_to(np.asarray(d, np.float64), (len(uv),))
    return np.concatenate([uv * d[:, None] / F, d[:, None]], axis=1).astype(np.float32)


TRI_UV = np.array([[1.5, 1.5], [13.5, 2.5], [3.5, 13.5]])


def test_one_colour_on_all_vertices_gives_that_colour_on_every_covered_pixel():
    for depths in (2.0, [1.0, 3.0, 7.0]):
        v = at_pixels(TRI_UV, depths)
        rgba, depth, tri = ref.render(CAM, v, [[0, 1, 2]], [[17, 130, 251]] * 3, W, H)
        covered = depth > 0
        assert covered.sum() > 40 and np.array_equal(covered, tri == 0) and (tri[~covered] == ref.NO_TRIANGLE).all()
        assert (rgba[covered] == (17, 130, 251, 255)).all() and (rgba[~covered] == ref.BACKGROUND).all()


def test_a_fronto_parallel_triangle_equals_affine_interpolation_to_within_one_code():
    """all three vertices at one depth: the inverse depths are equal, so the perspective-correct weights are the barycentric
    coordinates of the pixel centre in the image.  Those are worked out here from the vertices' exact pixel coordinates in
    float64; the snap is exact for them, so what is left is rounding to a byte: one code"""
    colors = np.array([[250, 0, 30], [10, 200, 90], [60, 20, 255]], np.uint8)
    rgba, depth, _ = ref.render(CAM, at_pixels(TRI_UV, 2.5), [[0, 1, 2]], colors, W, H)
    ys, xs = np.nonzero(depth)
    assert len(ys) > 40
    M = np.concatenate([TRI_UV.T, np.ones((1, 3))])  # barycentric coordinates: M l = (px, py, 1)
    lam = np.linalg.solve(M, np.stack([xs + 0.5, ys + 0.5, np.ones(len(xs))]))
    want = lam.T @ colors.astype(np.float64)
    err = np.abs(rgba[ys, xs, :3].astype(np.float64) - want)
    print("worst difference to affine interpolation, codes:", err.max())
    assert err.max() <= 1.0 and (rgba[ys, xs, 3] == 255).all()


def slanted_quad():
    """a planar quad whose left edge (u = 1.5) is at depth 1 and whose right edge (u = 13.5) at depth 4, black on the left and
    (240, 120, 60) on the right: the colour is one affine function on the quad's plane, so both triangles interpolate it"""
    v = at_pixels([[1.5, 1.5], [13.5, 1.5], [13.5, 13.5], [1.5, 13.5]], [1.0, 4.0, 4.0, 1.0])
    colors = np.array([[0, 0, 0], [240, 120, 60], [240, 120, 60], [0, 0, 0]], np.uint8)
    return v, np.array([[0, 1, 2], [0, 2, 3]], np.uint32), colors


def test_perspective_correct_and_screen_space_interpolation_differ_on_a_slanted_quad():
    """pixel (7, 7), centre u = 7.5: halfway across the quad in the image, t_s = (7.5 - 1.5) / 12 = 0.5.  1 / z is affine in the
    image: 1 / z = 0.5 * 1 + 0.5 * (1 / 4) = 0.625, and the position across the quad on its plane is t = t_s * (1 / 4) / 0.625 = 0.2.
    So the surface there has the colour 0.2 * (240, 120, 60) = (48, 24, 12) and the depth 1.6; screen-space interpolation says
    0.5 * (240, 120, 60) = (120, 60, 30)."""
    v, t, colors = slanted_quad()
    rgba, depth, _ = ref.render(CAM, v, t, colors, W, H)
    screen, _, _ = ref.render(CAM, v, t, colors, W, H, interpolate="screen")
    assert rgba[7, 7].tolist() == [48, 24, 12, 255] and depth[7, 7] == np.float32(1.6)
    assert screen[7, 7].tolist() == [120, 60, 30, 255]
    assert np.abs(rgba[7, 7, :3].astype(int) - screen[7, 7, :3].astype(int)).min() > 1
    # the other diagonal cuts the same plane: the same bytes
    other, _, _ = ref.render(CAM, v, [[0, 1, 3], [1, 2, 3]], colors, W, H)
    assert other[7, 7].tolist() == [48, 24, 12, 255]


def soup(rng, n):
    uv = rng.uniform(-3, W + 3, (n, 3, 2))
    uv[:, 1:] = uv[:, :1] + rng.uniform(-6, 6, (n, 2, 2))
    d = rng.uniform(0.5, 5.0, (n, 3))
    v = np.concatenate([uv.reshape(-1, 2) * d.reshape(-1, 1) / F, d.reshape(-1, 1)], axis=1).astype(np.float32)
    return v, np.arange(3 * n, dtype=np.uint32).reshape(-1, 3), rng.integers(0, 256, (3 * n, 3)).astype(np.uint8)


def test_the_high_words_of_the_keys_are_the_depth_reference_s_keys():
    v, t, colors = soup(np.random.default_rng(3), 200)
    keys = ref.visibility_keys(CAM, v, t, W, H)
    want = raster_ref.depth_keys(CAM, v, t, W, H)
    assert np.array_equal((keys >> np.uint64(32)).astype(np.uint32), want) and (want != raster_ref.NEVER).sum() > 100
    assert ((keys == ref.EMPTY) == (want == raster_ref.NEVER)).all()
    rgba, depth, tri = ref.render(CAM, v, t, colors, W, H)
    assert depth.tobytes() == raster_ref.depth(CAM, v, t, W, H).tobytes()
    assert len(np.unique(tri[depth > 0])) > 5  # intersecting triangles of many ids
    turned, d2, t2 = ref.render(CAM, v, t, colors, W, H, flip=True)
    assert np.array_equal(turned, rgba[::-1, ::-1]) and np.array_equal(d2, depth) and np.array_equal(t2, tri)  # only the image turns


def test_coincident_triangles_take_the_lower_id_s_colours_in_either_order():
    tri = at_pixels(TRI_UV, [1.0, 3.0, 7.0])
    v = np.concatenate([tri, tri])  # the same three positions twice
    red, blue = [[200, 10, 10]] * 3, [[10, 10, 200]] * 3
    for first, second in ((red, blue), (blue, red)):
        rgba, depth, ids = ref.render(CAM, v, [[0, 1, 2], [3, 4, 5]], np.array(first + second, np.uint8), W, H)
        covered = depth > 0
        assert covered.sum() > 40 and (ids[covered] == 0).all()
        assert (rgba[covered] == tuple(first[0]) + (255,)).all()
    # and the mirror-wound twin: the colours go with the vertices, whichever way the triangle is wound
    colors = np.array([[250, 0, 30], [10, 200, 90], [60, 20, 255]], np.uint8)
    a = ref.render(CAM, tri, [[0, 1, 2]], colors, W, H)[0]
    for twin in ([0, 2, 1], [2, 1, 0], [1, 0, 2]):
        assert ref.render(CAM, tri, [twin], colors, W, H)[0].tobytes() == a.tobytes()


def test_an_exactly_white_pixel_is_transparent_and_an_empty_mesh_is_all_background():
    rgba, depth, tri = ref.render(CAM, at_pixels(TRI_UV, 2.0), [[0, 1, 2]], [[255, 255, 255]] * 3, W, H)
    assert (depth > 0).sum() > 40 and (rgba == ref.BACKGROUND).all() and (tri[depth > 0] == 0).all()
    rgba, depth, tri = ref.render(CAM, np.zeros((0, 3), np.float32), np.zeros((0, 3), np.uint32), np.zeros((0, 3), np.uint8), W, H)
    assert (rgba == ref.BACKGROUND).all() and not depth.any() and (tri == ref.NO_TRIANGLE).all()


# ---- the ABI and the documents
NEW = (("prv_mesh_set_colors", 3), ("prv_mesh_render", 11))


def header_text():
    return open(os.path.join(ROOT, "include", "prv.h")).read()


def test_new_symbols_declared_exported_and_bound():
    text = re.sub(r"/\*.*?\*/", "", header_text(), flags=re.S)
    out = subprocess.check_output(["nm", "-D", "--defined-only", os.path.join(ROOT, "nerf_prv_amd", "libprv_hip.so")], text=True)
    exported = {l.split()[-1] for l in out.splitlines() if " T " in l}
    for name, n_args in NEW:
        m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*)\)\s*;", text)
        assert m, f"{name} is not declared in prv.h"
        assert len([a for a in m.group(1).split(",") if a.strip()]) == n_args
        assert name in exported
        assert len(_lib.SIGNATURES[name][1]) == n_args
    assert _lib.load().prv_abi_version() == 5
    assert re.search(r"#define\s+PRV_ABI_VERSION\s+5\b.*prv_mesh_set_colors and prv_mesh_render: additive", header_text())
    import inspect
    assert "colors" in inspect.signature(api.Context.mesh_from_arrays).parameters
    assert {"flip180", "want_depth", "want_triangles"} <= set(inspect.signature(api.Context.mesh_render).parameters)
    assert hasattr(api.Mesh, "set_colors")


def test_null_arguments_are_refused_without_a_context():
    lib = _lib.load()
    assert lib.prv_mesh_render(None, None, None, None, 1, 8, 8, 0, None, None, None) == _lib.PRV_E_INVALID
    assert "context is NULL" in lib.prv_last_error(None).decode()
    assert lib.prv_mesh_set_colors(None, None, 0) != 0


def test_header_states_the_colour_contract_and_the_limits():
    text = re.sub(r"\s*\n\s*\*\s*", " ", header_text())
    text = re.sub(r"\s+", " ", text)
    for phrase in ("mesh colour images", "key = ((uint64)bits of z << 32) | triangle id", "A pixel is empty iff the high word of its key is 0xFFFFFFFF",
                   "TIE RULE", "the lowest triangle id", "p_a = (double)w_a * i_a", "iz = (p_a + p_b) + p_c",
                   "c_k = ((p_a * (double)C_a[k] + p_b * (double)C_b[k]) + p_c * (double)C_c[k]) / iz", "byte_k = (uint8)min(255.0, floor(c_k + 0.5))",
                   "EQUALITY WITH prv_mesh_depth", "255, 255, 255, 0", "(width - 1 - x, height - 1 - y)", "PINHOLE ONLY", "NO NEAR-PLANE CLIPPING",
                   "GOURAUD VERTEX COLOURS ONLY", "NO LIGHTING", "SINGLE-RANK", "call prv_mesh_set_colors", "PRV_COVERAGE_ZBUF_BYTES"):
        assert phrase in text, phrase


# ---- the planner's .ply reader (host/extras/ply_io.hpp), through a stand-alone program as the host tests probe the yaml keys
PROBE = r"""
#include <cstdio>
#include <iostream>
#include "extras/ply_io.hpp"
int main(int argc, char** argv) {
  std::vector<float> xyz(3, 7.0f);
  std::vector<uint8_t> rgb;
  std::vector<uint32_t> tri;
  const std::string why = prvhost::ply_read(argv[1], xyz, rgb, tri);
  if (!why.empty()) {
    std::cout << "refused: " << why << "\nleft " << xyz.size() << " " << rgb.size() << " " << tri.size() << "\n";
    return 1;
  }
  FILE* f = fopen(argv[2], "wb");
  const unsigned long long n[2] = {xyz.size() / 3, tri.size() / 3};
  fwrite(n, 8, 2, f);
  fwrite(xyz.data(), 4, xyz.size(), f);
  fwrite(rgb.data(), 1, rgb.size(), f);
  fwrite(tri.data(), 4, tri.size(), f);
  fclose(f);
  return 0;
}
"""


@pytest.fixture(scope="module")
def ply_probe(tmp_path_factory):
    d = tmp_path_factory.mktemp("ply_probe")
    (d / "probe.cpp").write_text(PROBE)
    exe = d / "probe"
    subprocess.check_call(["g++", "-std=c++17", "-O0", "-Wall", "-I", os.path.join(ROOT, "nerf_prv_amd", "host"), "-o", str(exe), str(d / "probe.cpp")])

    def run(path):
        return subprocess.run([str(exe), str(path), str(d / "out.bin")], text=True, capture_output=True), d / "out.bin"

    return run


def test_the_ply_reader_round_trips_the_writer_s_file_and_refuses_the_rest(ply_probe, tmp_path):
    rng = np.random.default_rng(5)
    v = rng.uniform(-2, 2, (37, 3)).astype(np.float32)
    t = rng.integers(0, 37, (61, 3)).astype(np.uint32)
    c = rng.integers(0, 256, (37, 3)).astype(np.uint8)
    good = tmp_path / "m.ply"
    api.write_mesh(good, v, t, normals=rng.normal(size=(37, 3)), colors=c, scale=1.0, offset=(0.0, 0.0, 0.0))
    out, result = ply_probe(good)
    assert out.returncode == 0, out.stdout + out.stderr
    raw = result.read_bytes()
    nv, nt = np.frombuffer(raw[:16], "<u8")
    assert (nv, nt) == (37, 61)
    xyz = np.frombuffer(raw[16:16 + 37 * 12], "<f4").reshape(-1, 3)
    assert xyz.tobytes() == v[:, [2, 0, 1]].tobytes()  # the file's frame: (e2, e0, e1), scale 1 and offset 0 change no bit
    assert raw[16 + 37 * 12:16 + 37 * 15] == c.tobytes() and raw[16 + 37 * 15:] == t.tobytes()
    data = good.read_bytes()

    def refused(name, content, text):
        p = tmp_path / name
        p.write_bytes(content)
        out, _ = ply_probe(p)
        assert out.returncode == 1 and text in out.stdout, out.stdout
        assert out.stdout.splitlines()[-1] == "left 3 0 0"  # the caller's arrays are as they were

    refused("cut.ply", data[:-5], "truncated")
    refused("cut_vertices.ply", data[: data.index(b"end_header\n") + 11 + 100], "truncated")
    ascii_ply = "ply\nformat ascii 1.0\nelement vertex 1\nproperty float x\nproperty float y\nproperty float z\nend_header\n0 0 0\n"
    refused("ascii.ply", ascii_ply.encode(), "binary_little_endian")
    refused("no_normals.ply", data.replace(b"property float nx\nproperty float ny\nproperty float nz\n", b""), "expected `property float nx`")
    refused("quads.ply", data[:-61 * 13] + bytes([4]) + data[-61 * 13 + 1:], "triangles only")
    far = bytearray(data)
    far[-4:] = (37).to_bytes(4, "little")
    refused("far.ply", bytes(far), "names vertex 37 of 37")
    refused("not.ply", b"solid\n", "not a ply file")
    out, _ = ply_probe(tmp_path / "missing.ply")
    assert out.returncode == 1 and "cannot open" in out.stdout
    empty = tmp_path / "empty.ply"
    api.write_mesh(empty, np.zeros((0, 3), np.float32), np.zeros((0, 3), np.uint32))
    out, result = ply_probe(empty)
    assert out.returncode == 0 and np.frombuffer(result.read_bytes()[:16], "<u8").tolist() == [0, 0]
