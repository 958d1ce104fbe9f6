"""What an install of a model decides on the host (nerf_prv_amd/csrc/prv_field_plan.hpp), without a GPU: the C++ itself against
the Python restatement of tests/instances.py, numpy brute force and the documented definitions.  Host code only: a stand-alone
program built from the header alone with the address and undefined-behaviour sanitizers reads the cases this file writes and
prints what the header answers; every plan's invariants are checked in the program.

Rejections: "invalid field descriptor", "field too large for 32-bit gather offsets" and "level %d has %u vertices per axis (limit
4096)" each have a descriptor here.  The other two rules stay in the code but no descriptor that compute_levels accepts reaches them
today: a hashed level has at most 2^28 entries of at most 8 bytes (2^31 bytes, "hashed level of 4 GiB or more" asks for 2^32), and a
dense level with a z stride of 2^24 bytes or more has 1024 or more vertices per axis, 2^30 entries, which log2_hashmap <= 28 makes a
hashed level ("dense level too large")."""
import json
import os
import subprocess

import numpy as np
import pytest

from nerf_prv_amd import _lib, api
from tests import instances, republish_cases, train_cases as tc, util

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PROGRAM = r"""
#include "prv_field_plan.hpp"
#include <cstdio>
#include <fstream>
#include <iostream>
#include <sstream>
using namespace prv;

#define CHECK(c) do { if (!(c)) { printf("line %d: %s\n", __LINE__, #c); exit(1); } } while (0)

static std::vector<uint32_t> read_words(const char* path) {
  std::ifstream in(path, std::ios::binary);
  std::vector<char> raw((std::istreambuf_iterator<char>(in)), std::istreambuf_iterator<char>());
  std::vector<uint32_t> w(raw.size() / 4);
  memcpy(w.data(), raw.data(), w.size() * 4);
  return w;
}
static uint32_t bits(float f) { uint32_t u; memcpy(&u, &f, 4); return u; }
template <class T> static void print_list(const char* key, const T* v, size_t n) {
  printf("\"%s\":[", key);
  for (size_t i = 0; i < n; i++) printf("%s%llu", i ? "," : "", (unsigned long long)v[i]);
  printf("]");
}

// the properties every accepted plan has, whatever the descriptor
static void check_invariants(const FieldPlan& P) {
  const uint32_t eb = P.ebytes();
  uint64_t end = 0, sum = 0;
  for (int l = 0; l < P.n_levels; l++) {
    const LevelPlan& L = P.levels[l];
    CHECK(P.psize[l] > 0 && (P.lv[l].hashed || (P.psize[l] & (P.psize[l] - 1)) == 0));
    CHECK(P.poff[l] % P.psize[l] == 0 && L.off_b == P.poff[l] * eb); // a multiple of its own physical size
    for (int k = 0; k < l; k++) CHECK(P.poff[k] + (uint64_t)P.psize[k] <= P.poff[l] || P.poff[l] + (uint64_t)P.psize[l] <= P.poff[k]);
    end = std::max(end, P.poff[l] + (uint64_t)P.psize[l]);
    sum += P.psize[l];
    CHECK(L.res_m1 + 1 == P.lv[l].res && bits(L.scale) == bits(P.lv[l].scale));
    if (!P.lv[l].hashed) {
      CHECK(L.my_b == eb << P.sx[l] && L.mz_b == eb << (2 * P.sx[l]) && L.myz_b == L.my_b + L.mz_b && L.m_b == 0xffffffffu);
      CHECK((1u << P.sx[l]) >= P.lv[l].res + 1 && (uint64_t)(P.lv[l].res + 1) << (2 * P.sx[l]) <= P.psize[l]);
      if (P.hash_shared) CHECK((L.pack & ~31u) == L.off_b && (L.pack & 31u) == P.sx[l]);
    } else {
      CHECK(L.m_b == (P.lv[l].size - 1) * eb && L.myz_b == L.my_b + L.mz_b);
      if (P.hash_shared) CHECK((L.pack & ~4095u) == L.off_b && (L.pack & 4095u) == L.res_m1 && L.my_b == P.hash_my_b && L.mz_b == P.hash_mz_b && L.m_b == P.hash_m_b);
      if (!P.wide_offsets) CHECK(L.my_b < (1u << 24) && L.mz_b < (1u << 24) && L.m_b < (1u << 24));
    }
  }
  CHECK(end == P.ptotal && sum == P.ptotal && P.phys_bytes() < (1ull << 32)); // pairwise disjoint and ending at the total: no gap either
  CHECK(P.n_dense_levels + P.n_hashed_levels <= P.n_levels);
  for (int l = 0; l < P.n_dense_levels; l++) CHECK(!P.lv[l].hashed);
}

static bool read_desc(std::istream& in, std::string& name, prv_field_desc& d) {
  d = prv_field_desc{};
  return (bool)(in >> name >> d.n_levels >> d.n_features >> d.log2_hashmap >> d.base_res >> d.finest_res >> d.occ_res >> d.per_level_scale);
}

// layout <cases>: a line per case = name, the descriptor, no_pair
static void layout(const char* path) {
  std::ifstream in(path);
  std::string name, err;
  prv_field_desc d;
  int no_pair;
  while (read_desc(in, name, d) && (in >> no_pair)) {
    FieldPlan P;
    const int rc = plan_field(d, no_pair != 0, P, err);
    printf("{\"name\":\"%s\",\"no_pair\":%d,\"rc\":%d", name.c_str(), no_pair, rc);
    if (rc != PRV_OK) {
      printf(",\"err\":\"%s\"}\n", err.c_str());
      continue;
    }
    check_invariants(P);
    printf(",\"n_dense_levels\":%d,\"n_hashed_levels\":%d,\"hash_shared\":%d,\"wide_offsets\":%d,\"table_bytes_physical\":%llu,\"kernel_dense_levels\":%d,\"table_halfs\":%llu,\"levels\":[",
           P.n_dense_levels, P.n_hashed_levels, P.hash_shared, P.wide_offsets, (unsigned long long)P.phys_bytes(), P.instance(), (unsigned long long)P.table_halfs());
    for (int l = 0; l < P.n_levels; l++) printf("%s[%u,%u,%u,%u]", l ? "," : "", bits(P.lv[l].scale), P.lv[l].res, P.lv[l].hashed, P.lv[l].size);
    printf("]}\n");
  }
}

// occupancy <file>: cases of {R, the grid's words}, back to back
static void occupancy(const char* path) {
  const std::vector<uint32_t> w = read_words(path);
  for (size_t at = 0; at < w.size();) {
    const int R = (int)w[at++];
    const size_t n = ((size_t)R * R * R + 31) / 32;
    CHECK(at + n <= w.size());
    const std::vector<uint32_t> grid(w.begin() + at, w.begin() + at + n); // a block of its own: a read past its end is the sanitizer's finding
    at += n;
    const OccupancySummary S = summarize_occupancy(grid.data(), R);
    uint32_t box[6];
    for (int a = 0; a < 3; a++) box[a] = bits(S.lo[a]), box[3 + a] = bits(S.hi[a]);
    printf("{\"R\":%d,", R);
    print_list("box", box, 6);
    printf(",");
    print_list("coarse", S.coarse.data(), S.coarse.size());
    printf("}\n");
  }
}

// fragments <F> <v64>: the 24 fragments of mlp[i] = i + 1
static void fragments(int F, int v64) {
  std::vector<uint16_t> mlp(PRV_MLP_HALFS);
  for (size_t i = 0; i < mlp.size(); i++) mlp[i] = (uint16_t)(i + 1);
  const std::vector<uint16_t> f = prepack_fragments(mlp.data(), F, v64 != 0);
  printf("{");
  print_list("frags", f.data(), f.size());
  printf("}\n");
}

// replicas <cases>: a line per case = name, the descriptor, no_pair, the cap, the budget in bytes
static void replicas(const char* path) {
  std::ifstream in(path);
  std::string name, err;
  prv_field_desc d;
  int no_pair, cap;
  unsigned long long budget;
  while (read_desc(in, name, d) && (in >> no_pair >> cap >> budget)) {
    FieldPlan P;
    CHECK(plan_field(d, no_pair != 0, P, err) == PRV_OK);
    const ReplicaPlan R = plan_replicas(P, cap, budget);
    CHECK(R.n >= 0 && R.n <= kPlanMaxReplicas && R.n <= std::max(cap, 0) && R.total_bytes <= budget);
    printf("{\"name\":\"%s\",\"n\":%d,\"total_bytes\":%llu,", name.c_str(), R.n, (unsigned long long)R.total_bytes);
    print_list("pack", R.pack, kPlanMaxReplicas);
    printf("}\n");
  }
}

// synthetic <floats>: the occupancy of a fresh field and of the spheres, and f2h of the file's floats
static void synthetic(const char* path) {
  printf("{");
  for (int R : {7, 12, 16}) {
    const std::vector<uint32_t> occ = synthetic_occupancy(R, true);
    char key[16];
    snprintf(key, sizeof(key), "all%d", R);
    print_list(key, occ.data(), occ.size());
    printf(",");
  }
  const std::vector<uint32_t> sph = synthetic_occupancy(16, false);
  print_list("spheres16", sph.data(), sph.size());
  const std::vector<uint32_t> fl = read_words(path);
  std::vector<uint16_t> h(fl.size());
  for (size_t i = 0; i < fl.size(); i++) {
    float f;
    memcpy(&f, &fl[i], 4);
    h[i] = synth::f2h(f);
  }
  printf(",");
  print_list("halfs", h.data(), h.size());
  const std::vector<uint16_t> a = synthetic_mlp(1), b = synthetic_mlp(1), c = synthetic_mlp(2);
  CHECK(a.size() == PRV_MLP_HALFS && a == b && a != c);
  printf("}\n");
}

int main(int argc, char** argv) {
  CHECK(argc >= 3);
  const std::string mode = argv[1];
  if (mode == "layout") layout(argv[2]);
  else if (mode == "occupancy") occupancy(argv[2]);
  else if (mode == "fragments") { CHECK(argc == 4); fragments(atoi(argv[2]), atoi(argv[3])); }
  else if (mode == "replicas") replicas(argv[2]);
  else if (mode == "synthetic") synthetic(argv[2]);
  else CHECK(!"mode");
  CHECK(instance_dense_levels(4, 5, 1) == 5 && instance_dense_levels(4, 3, 1) == 3 && instance_dense_levels(4, 4, 1) == 0 && instance_dense_levels(4, 5, 0) == 0);
  CHECK(instance_dense_levels(2, 10, 1) == 10 && instance_dense_levels(2, 6, 1) == 6 && instance_dense_levels(2, 5, 1) == 0 && instance_dense_levels(2, 10, 0) == 0);
  return 0;
}
"""


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    """the stand-alone program, built once; run(*args) -> one parsed JSON object per printed line"""
    d = tmp_path_factory.mktemp("field_plan")
    src, exe = d / "field_plan.cpp", d / "field_plan"
    src.write_text(PROGRAM)
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan",
                           "-I", os.path.join(ROOT, "nerf_prv_amd", "csrc"), str(src), "-o", str(exe)])

    def run(*args):
        out = subprocess.run([str(exe)] + [str(a) for a in args], text=True, capture_output=True, timeout=60)
        assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
        return [json.loads(line) for line in out.stdout.splitlines()]

    return run


def test_header_is_host_only():
    text = open(os.path.join(ROOT, "nerf_prv_amd", "csrc", "prv_field_plan.hpp")).read()
    includes = [line.split()[1] for line in text.splitlines() if line.startswith("#include")]
    assert '"prv_levels.hpp"' in includes and '"../../include/prv.h"' in includes
    assert not [i for i in includes if "hip" in i or "prv_device" in i or "prv_kernels" in i], includes


# ---------------------------------------------------------------- layout
DESCRIPTORS = {**{k: e.kw for k, e in instances.MATRIX.items()}, **{k: e.kw for k, e in instances.PRODUCT.items()},
               "SMALL": util.SMALL, "SMALL_F2": util.SMALL_F2}
DESC_KEYS = ("n_levels", "n_features", "log2_hashmap", "base_res", "finest_res", "occ_res")


def desc_line(name, kw):
    return " ".join([name] + [str(kw[k]) for k in DESC_KEYS] + [repr(float(kw.get("per_level_scale", 0.0)))])


def test_layout_is_the_restated_one(program, tmp_path):
    cases = tmp_path / "layout.txt"
    cases.write_text("".join(f"{desc_line(name, kw)} {no_pair}\n" for name, kw in DESCRIPTORS.items() for no_pair in (0, 1)))
    got = program("layout", cases)
    assert [(g["name"], g["no_pair"]) for g in got] == [(name, no_pair) for name in DESCRIPTORS for no_pair in (0, 1)]
    for g in got:
        kw = DESCRIPTORS[g["name"]]
        want = instances.restated_layout(kw)
        assert g["rc"] == 0, g
        assert g["n_hashed_levels"] == want["n_hashed_levels"] and g["wide_offsets"] == int(want["wide_offsets"]), g
        assert g["table_bytes_physical"] == want["table_bytes_physical"], g
        if g["no_pair"]:  # every level through the generic gather: no dense level, nothing shared, the generic instance
            assert (g["n_dense_levels"], g["hash_shared"], g["kernel_dense_levels"]) == (0, 0, 0), g
        else:
            assert g["n_dense_levels"] == want["n_dense_levels"] and g["hash_shared"] == int(want["hash_shared"]), g
            assert g["kernel_dense_levels"] == want["kernel_dense_levels"], g
        levels = instances.restated_levels(kw)
        assert g["levels"] == [[int(np.float32(s).view(np.uint32)), res, int(hashed), size] for s, res, hashed, size in levels], g
        assert g["table_halfs"] == sum(size for _, _, _, size in levels) * kw["n_features"]
    assert api.model_sizes(api.field_desc(**util.SMALL))[0] == next(g["table_halfs"] for g in got if g["name"] == "SMALL")


# descriptors that reach a rejection (the module's docstring has the two rules nothing reaches)
NO_FIELD = dict(util.SMALL, n_levels=7)
TOO_LARGE = dict(n_levels=16, n_features=2, log2_hashmap=28, base_res=2, finest_res=513, occ_res=8)  # 0.8 GB canonical; its 513^3 level is 2^30 entries of 4 bytes when padded
PAST_LIMIT = dict(n_levels=8, n_features=4, log2_hashmap=4, base_res=4096, finest_res=4096, occ_res=8, per_level_scale=1.00001)


def test_rejections(program, tmp_path):
    assert instances.restated_layout(TOO_LARGE)["table_bytes_physical"] >= 1 << 32
    assert sum(x[3] for x in instances.restated_levels(TOO_LARGE)) * 4 < 1 << 32  # compute_levels lets it pass
    assert [x[1] for x in instances.restated_levels(PAST_LIMIT)][:2] == [4096, 4097]
    want = {"NO_FIELD": (NO_FIELD, "invalid field descriptor"), "TOO_LARGE": (TOO_LARGE, "field too large for 32-bit gather offsets"),
            "PAST_LIMIT": (PAST_LIMIT, "level 1 has 4097 vertices per axis (limit 4096)")}
    cases = tmp_path / "rejected.txt"
    cases.write_text("".join(f"{desc_line(name, kw)} {no_pair}\n" for name, (kw, _) in want.items() for no_pair in (0, 1)))
    got = program("layout", cases)
    assert len(got) == 6
    for g in got:
        assert g["rc"] == _lib.PRV_E_INVALID and g["err"] == want[g["name"]][1], g


# ---------------------------------------------------------------- occupancy
def pack_bits(cells):
    """bool cells, x fastest -> the grid's uint32 words"""
    flat = np.asarray(cells, bool).ravel()
    padded = np.zeros((flat.size + 31) // 32 * 32, np.uint8)
    padded[:flat.size] = flat
    return np.packbits(padded, bitorder="little").view(np.uint32)


def occupancy_patterns(R, rng):
    empty = np.zeros((R, R, R), bool)  # [z, y, x]
    yield "empty", empty
    yield "full", ~empty
    last = empty.copy()
    last[-1, -1, -1] = True
    yield "last cell", last
    corners = empty.copy()
    corners[np.ix_([0, -1], [0, -1], [0, -1])] = True
    yield "corners", corners
    seam = empty.copy()
    if R > 32:  # either side of the word seam inside one row ...
        seam[2, 1, 31] = seam[2, 1, 32] = True
    elif R ** 3 > 32:  # ... or of the first seam of the bitfield, where a row is shorter than a word
        seam.reshape(-1)[31:33] = True
    yield "seam", seam
    yield "one per cent", rng.random((R, R, R)) < 0.01


def brute_coarse(cells):
    """any cell in the 4^3 block, then the 3 x 3 x 3 dilation -> words"""
    Rc = cells.shape[0] // 4
    blk = cells.reshape(Rc, 4, Rc, 4, Rc, 4).any(axis=(1, 3, 5))
    pad = np.pad(blk, 1)
    out = np.zeros_like(blk)
    for dz in range(3):
        for dy in range(3):
            for dx in range(3):
                out |= pad[dz:dz + Rc, dy:dy + Rc, dx:dx + Rc]
    return pack_bits(out)


def test_occupancy_box_and_coarse_grid(program, tmp_path):
    rng = np.random.default_rng(7)
    grids = [(R, what, cells) for R in (1, 4, 7, 8, 12, 20, 32, 36, 64) for what, cells in occupancy_patterns(R, rng)]
    grids.append((128, "full", np.ones((128, 128, 128), bool)))
    path = tmp_path / "grids.bin"
    with open(path, "wb") as fh:
        for R, _, cells in grids:
            fh.write(np.uint32(R).tobytes() + pack_bits(cells).tobytes())
    got = program("occupancy", path)
    assert len(got) == len(grids)
    f32 = np.float32
    for g, (R, what, cells) in zip(got, grids):
        assert g["R"] == R
        box = republish_cases.occupied_box(pack_bits(cells), R)
        if box is None:
            want = [f32(2.0)] * 3 + [f32(-1.0)] * 3
        else:
            want = [f32(v - 1) / f32(R) for v in box[0]] + [f32(v + 2) / f32(R) for v in box[1]]
        assert g["box"] == [int(f32(v).view(np.uint32)) for v in want], (R, what)
        if R % 4 != 0 or R < 8:
            assert g["coarse"] == [], (R, what)
        else:
            assert g["coarse"] == brute_coarse(cells).tolist(), (R, what)


# ---------------------------------------------------------------- fragments
K_IN, K_OUT, K_OFF = (32, 64, 32, 64, 64), (64, 16, 64, 64, 16), (0, 2048, 3072, 5120, 9216)


def hidden_k(s, h, j):
    return 32 * (s >> 1) + 16 * (s & 1) + 8 * (j >> 2) + 4 * h + (j & 3)


@pytest.mark.parametrize("F", [4, 2])
def test_fragments(program, F):
    n = 24 * 512
    plain = np.array(program("fragments", F, 0)[0]["frags"])
    assert plain.shape == (n,) and sorted(plain[plain != 0].tolist()) == list(range(1, 10241))  # every weight once, zeros elsewhere
    # the render kernel's set, from its definition: fragment (layer, mt, s), lane (r, h), element j = W[k][32 mt + r] with k in
    # canonical order for the first layer; row 20 of layer 2 repeats unit 0, rows 20..22 of layer 5 repeat units 0..2
    W = lambda layer, k, out: K_OFF[layer] + k * K_OUT[layer] + out + 1
    want = []
    order = [(0, mt, s) for mt in range(2) for s in range(2)] + [(1, 0, s) for s in range(4)] + [(2, mt, s) for mt in range(2) for s in range(2)]
    order += [(3, mt, s) for mt in range(2) for s in range(4)] + [(4, 0, s) for s in range(4)]
    for layer, mt, s in order:
        for lane in range(64):
            r, h = lane & 31, lane >> 5
            out = 32 * mt + r
            if layer == 1 and out == 20:
                out = 0
            if layer == 4 and 20 <= out <= 22:
                out -= 20
            for j in range(8):
                if layer == 0:
                    k = 16 * s + 8 * h + j
                elif layer == 2:  # [16 density outputs | 16 SH coefficients]
                    k = hidden_k(0, h, j) if s == 0 else 16 + 8 * h + j
                else:
                    k = hidden_k(s, h, j)
                assert k < K_IN[layer]
                want.append(W(layer, k, out) if out < K_OUT[layer] else 0)
    assert program("fragments", F, 1)[0]["frags"] == want


# ---------------------------------------------------------------- replicas
def test_replicas(program, tmp_path):
    """api.FIELD_256's three hashed levels (116, 173 and 256 vertices per axis) take 13.5 + 43.1 + 143.3 MB, inside the default
    budget of 256 MiB"""
    res = [r for _, r, hashed, _ in instances.restated_levels(api.FIELD_256) if hashed]
    sizes = [api.replica_level(r)[2] for r in res]
    rows = [api.replica_level(r)[0] for r in res]
    assert [round(b / 1e6, 1) for b in sizes] == [13.5, 43.1, 143.3]
    cum = np.cumsum(sizes).tolist()
    default = 256 << 20
    f256 = desc_line("f", api.FIELD_256)
    cases = {"default": (f256, 0, 3, default, 3), "generous": (f256, 0, 99, 1 << 40, 3)}
    for cap in (0, 1, 2):
        cases[f"cap{cap}"] = (f256, 0, cap, default, cap)
    for k in range(3):  # one byte short of k + 1 levels: k levels; exactly enough: k + 1
        cases[f"short{k}"] = (f256, 0, 3, cum[k] - 1, k)
        cases[f"exact{k}"] = (f256, 0, 3, cum[k], k + 1)
    cases["F2"] = (desc_line("f", api.FIELD_512), 0, 3, default, 0)
    cases["no_pair"] = (f256, 1, 3, default, 0)
    cases["generic"] = (desc_line("f", util.SMALL), 0, 3, default, 0)  # four dense levels: <4, 0>
    cases["F4_3"] = (desc_line("f", instances.MATRIX["F4_3"].kw), 0, 3, default, 0)
    cases["F4_5"] = (desc_line("f", instances.MATRIX["F4_5"].kw), 0, 3, default, 3)
    path = tmp_path / "replicas.txt"
    path.write_text("".join(f"{name} {line.split(' ', 1)[1]} {no_pair} {cap} {budget}\n" for name, (line, no_pair, cap, budget, _) in cases.items()))
    got = {g["name"]: g for g in program("replicas", path)}
    assert list(got) == list(cases)
    for name, (_, _, _, _, n) in cases.items():
        g = got[name]
        assert g["n"] == n, g
        if name in ("F4_5", "generic", "F4_3", "F2"):
            continue
        assert g["total_bytes"] == sum(sizes[:n]), g
        assert g["pack"] == [([0] + cum)[k] | rows[k] // 8 if k < n else 0 for k in range(3)], g
    small = [api.replica_level(r)[2] for _, r, hashed, _ in instances.restated_levels(instances.MATRIX["F4_5"].kw) if hashed]
    assert got["F4_5"]["total_bytes"] == sum(small)


# ---------------------------------------------------------------- the synthetic field
def test_synthetic_occupancy_and_half_conversion(program, tmp_path):
    rng = np.random.default_rng(3)
    halves = np.arange(0, 0x7c01, dtype=np.uint16).view(np.float16).astype(np.float32)  # every finite half, infinity,
    ties = (halves[:-2].astype(np.float64) + halves[1:-1].astype(np.float64)) / 2        # the middle of every two neighbours,
    near = np.concatenate([np.nextafter(ties.astype(np.float32), np.float32(0)), np.nextafter(ties.astype(np.float32), np.float32(1e9))])
    big = np.array([65504.0, 65519.99, 65520.0, 65536.0, 1e9, np.inf, 2.0 ** -25, np.nextafter(np.float32(2.0 ** -25), np.float32(1)), 2.0 ** -26, 1e-30], np.float32)
    floats = np.concatenate([halves, ties.astype(np.float32), near, big, rng.uniform(-1, 1, 4096).astype(np.float32), rng.normal(0, 1e-5, 1024).astype(np.float32)])
    floats = np.concatenate([floats, -floats]).astype(np.float32)
    path = tmp_path / "floats.bin"
    path.write_bytes(floats.tobytes())
    got = program("synthetic", path)[0]
    with np.errstate(over="ignore"):
        assert got["halfs"] == floats.astype(np.float16).view(np.uint16).tolist()
    for R in (7, 12, 16):
        words = np.array(got[f"all{R}"], np.uint32)
        assert len(words) == (R ** 3 + 31) // 32 and tc.bits_of(words, len(words) * 32).sum() == R ** 3  # exactly R^3 bits: none in the last word's tail
        assert tc.bits_of(words, R ** 3).all()
    # the four spheres at R = 16: cell centres, d2 = fma(dx, dx, fma(dy, dy, dz * dz)) <= r * r in float32 (a fused multiply-add
    # of float32 values is the float32 rounding of the exact result, which float64 holds for these magnitudes)
    spheres = np.array([[0.50, 0.50, 0.50, 0.35], [0.80, 0.50, 0.62, 0.13], [0.36, 0.80, 0.45, 0.11], [0.40, 0.24, 0.78, 0.10]], np.float32)
    R, f32, f64 = 16, np.float32, np.float64
    c = (np.arange(R, dtype=f32) + f32(0.5)) * (f32(1.0) / f32(R))
    cz, cy, cx = np.meshgrid(c, c, c, indexing="ij")
    inside = np.zeros((R, R, R), bool)
    for x, y, z, r in spheres:
        dx, dy, dz = cx - x, cy - y, cz - z
        inner = (dy.astype(f64) * dy.astype(f64) + (dz * dz).astype(f64)).astype(f32)
        d2 = (dx.astype(f64) * dx.astype(f64) + inner.astype(f64)).astype(f32)
        inside |= d2 <= r * r
    assert 0 < inside.sum() < R ** 3 and got["spheres16"] == pack_bits(inside).tolist()
