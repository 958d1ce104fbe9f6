"""The order the render launch drains a queue region in (nerf_prv_amd/csrc/prv_queue_order.hpp), without a GPU: a stand-alone
program built from the header alone, with the address and undefined-behaviour sanitizers, plays the march of the populations of
tests/queue_cases.py -- every wave with a live ray, in launch order, reserves its block the way region_reserve does (RegionCounter:
the returning add that also hands out the descriptor's index, the tail cut of the one reservation that straddles a region's end,
moving on to the next region) and keys it with region_cell_key -- and sorts every octant region with order_descriptors.

Checked in the program, for every octant region: the sorted list is a permutation of the descriptors (each appears once), keys come
out non-decreasing, descriptors of one key keep their order of arrival (sub-regions interleaved by index), and the blocks of a
sub-region tile exactly [0, records) with records = min(count, seg_cap) - cut: what the render launch drains.  Synthetic lists
cover an empty region, one descriptor, every descriptor in one cell and random keys against std::stable_sort."""
import json
import os
import subprocess

import numpy as np
import pytest

from tests import queue_cases as qc, region_cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32

PROGRAM = r"""
#include "prv_queue_order.hpp"
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <random>
using namespace prv;

#define CHECK(c) do { if (!(c)) { printf("line %d: %s\n", __LINE__, #c); exit(1); } } while (0)

static float from_bits(uint32_t u) { float f; memcpy(&f, &u, 4); return f; }

// the properties of one octant region's sorted list; `first` of a synthetic descriptor is its arrival position
static void check_sorted(const std::vector<std::vector<QueueDesc>>& sub, const std::vector<QueueDesc>& out, int n_keys) {
  std::vector<const QueueDesc*> p;
  std::vector<uint32_t> n;
  size_t total = 0, n_max = 0;
  for (auto& s : sub) { p.push_back(s.data()); n.push_back((uint32_t)s.size()); total += s.size(); n_max = std::max(n_max, s.size()); }
  CHECK(out.size() == total);
  // the reference: arrival order (index-major, sub-regions interleaved), then std::stable_sort by key
  std::vector<QueueDesc> want;
  for (size_t i = 0; i < n_max; i++)
    for (auto& s : sub)
      if (i < s.size()) want.push_back(s[i]);
  std::stable_sort(want.begin(), want.end(), [](const QueueDesc& a, const QueueDesc& b) { return desc_key(a) < desc_key(b); });
  for (size_t i = 0; i < total; i++) {
    CHECK(out[i].first == want[i].first && out[i].info == want[i].info);
    CHECK(desc_key(out[i]) < (uint32_t)n_keys && (i == 0 || desc_key(out[i - 1]) <= desc_key(out[i])));
  }
}

static std::vector<QueueDesc> sort_region(const std::vector<std::vector<QueueDesc>>& sub, int n_keys) {
  std::vector<const QueueDesc*> p;
  std::vector<uint32_t> n;
  for (auto& s : sub) { p.push_back(s.data()); n.push_back((uint32_t)s.size()); }
  return order_descriptors(p.data(), n.data(), (int)sub.size(), n_keys);
}

static void synthetic() {
  std::mt19937 rng(7);
  for (int cells : {1, 2, 4, 8}) {
    const int n_keys = cells * cells * cells;
    for (int n_sub : {1, 8}) {
      for (int kind = 0; kind < 5; kind++) { // empty | one descriptor | all in one cell | random, uneven sub-regions | random, 5000
        std::vector<std::vector<QueueDesc>> sub(n_sub);
        const size_t total = kind == 0 ? 0 : kind == 1 ? 1 : kind == 4 ? 5000 : 300;
        for (size_t i = 0; i < total; i++) {
          const uint32_t key = kind == 2 ? (uint32_t)(n_keys - 1) : rng() % n_keys;
          const int s = kind == 3 ? (int)(rng() % 3) % n_sub : (int)(rng() % n_sub);
          sub[s].push_back(make_desc((uint32_t)i * 64u, 1u + rng() % 64u, key));
        }
        check_sorted(sub, sort_region(sub, n_keys), n_keys);
      }
    }
  }
  // keys: every corner of every cell count lands inside cells^3, whatever the point and the box
  const float lo[3] = {0.1f, 0.2f, 0.3f}, hi[3] = {0.9f, 0.7f, 0.8f}, none_lo[3] = {2, 2, 2}, none_hi[3] = {-1, -1, -1};
  std::uniform_real_distribution<float> u(-0.5f, 1.5f);
  for (int cells : {1, 2, 4, 8})
    for (int i = 0; i < 20000; i++) {
      float p[3] = {u(rng), u(rng), u(rng)};
      if (i % 97 == 0) p[i % 3] = from_bits(0x7fc00000u);
      if (i % 89 == 0) p[i % 3] = from_bits(0x7f800000u);
      CHECK(region_cell_key(p, lo, hi, cells) < (uint32_t)(cells * cells * cells));
      CHECK(region_cell_key(p, none_lo, none_hi, cells) < (uint32_t)(cells * cells * cells));
    }
  { // Morton order: the lowest corner's cell is 0, the highest's the last; a step along x inside the octant changes bit 0 first
    const float a[3] = {0.11f, 0.21f, 0.31f}, b[3] = {0.49f, 0.44f, 0.54f}, c[3] = {0.89f, 0.69f, 0.79f}, d[3] = {0.16f, 0.21f, 0.31f};
    CHECK(region_cell_key(a, lo, hi, 8) == 0 && region_cell_key(b, lo, hi, 8) == 511 && region_cell_key(c, lo, hi, 8) == 511);
    CHECK(region_cell_key(d, lo, hi, 8) == 1 && region_cell_key(d, lo, hi, 1) == 0);
  }
  printf("{\"ok\":1}\n");
}

// waves <file>: seg_cap n_seg n_sub cells lo[3] hi[3] (bits), then per wave: preferred region, live rays, mid-span point (bits)
static void waves(const char* path) {
  std::ifstream in(path);
  uint32_t seg_cap, n_seg, n_sub, box[6];
  int cells;
  in >> seg_cap >> n_seg >> n_sub >> cells;
  for (auto& b : box) in >> b;
  float lo[3], hi[3];
  for (int a = 0; a < 3; a++) lo[a] = from_bits(box[a]), hi[a] = from_bits(box[3 + a]);
  const int n_keys = cells * cells * cells;
  std::vector<RegionCounter> ctr(n_seg);
  std::vector<std::vector<QueueDesc>> desc(n_seg);
  uint32_t pref, n, pb[3];
  unsigned long long rays = 0, moved = 0;
  while (in >> pref >> n >> pb[0] >> pb[1] >> pb[2]) {
    const float p[3] = {from_bits(pb[0]), from_bits(pb[1]), from_bits(pb[2])};
    bool placed = false;
    for (uint32_t k = 0; k < n_seg && !placed; k++) { // region_reserve
      const uint32_t shard = (pref + k) % n_seg;
      if (k != 0 && ctr[shard].w[0] >= seg_cap) continue;
      uint32_t slot, idx;
      if (ctr[shard].reserve(seg_cap, n, &slot, &idx)) {
        CHECK(idx == desc[shard].size() && idx < seg_cap); // dense: the descriptors of a region are 0 .. n - 1, within its array
        desc[shard].push_back(make_desc(shard * seg_cap + slot, n, region_cell_key(p, lo, hi, cells)));
        placed = true;
        moved += k != 0;
      }
    }
    CHECK(placed);
    rays += n;
  }
  unsigned long long drained = 0, straddles = 0, n_desc = 0, empty = 0, single = 0, max_keys = 0, one_cell = 0, one_cell_most = 0;
  for (uint32_t o = 0; o < n_seg / n_sub; o++) {
    std::vector<std::vector<QueueDesc>> sub(desc.begin() + o * n_sub, desc.begin() + (o + 1) * n_sub);
    for (uint32_t s = 0; s < n_sub; s++) {
      const RegionCounter& c = ctr[o * n_sub + s];
      CHECK(c.descriptors() == sub[s].size());
      straddles += c.w[2] != 0;
      uint32_t at = (o * n_sub + s) * seg_cap; // the blocks tile the records the render drains, in index order
      for (auto& d : sub[s]) { CHECK(d.first == at); at += desc_count(d); }
      CHECK(at - (o * n_sub + s) * seg_cap == c.records(seg_cap));
    }
    const std::vector<QueueDesc> out = sort_region(sub, n_keys);
    check_sorted(sub, out, n_keys);
    std::vector<char> seen((size_t)n_keys, 0);
    unsigned long long keys = 0;
    for (auto& d : out) { drained += desc_count(d); keys += !seen[desc_key(d)]; seen[desc_key(d)] = 1; }
    n_desc += out.size();
    empty += out.empty();
    single += out.size() == 1;
    one_cell += out.size() > 1 && keys == 1;
    if (keys == 1) one_cell_most = std::max<unsigned long long>(one_cell_most, out.size());
    max_keys = std::max(max_keys, keys);
  }
  CHECK(drained == rays);
  printf("{\"rays\":%llu,\"descriptors\":%llu,\"moved\":%llu,\"straddles\":%llu,\"empty\":%llu,\"single\":%llu,\"one_cell\":%llu,\"one_cell_most\":%llu,\"max_keys\":%llu}\n", rays, n_desc, moved,
         straddles, empty, single, one_cell, one_cell_most, max_keys);
}

int main(int argc, char** argv) {
  if (argc == 2 && !strcmp(argv[1], "synthetic")) synthetic();
  else if (argc == 3 && !strcmp(argv[1], "waves")) waves(argv[2]);
  else return 2;
  return 0;
}
"""


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    d = tmp_path_factory.mktemp("queue_order")
    src, exe = d / "queue_order.cpp", d / "queue_order"
    src.write_text(PROGRAM)
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan",
                           "-I", os.path.join(ROOT, "nerf_prv_amd", "csrc"), str(src), "-o", str(exe)])

    def run(*args):
        out = subprocess.run([str(exe)] + [str(a) for a in args], text=True, capture_output=True, timeout=60)
        assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
        return [json.loads(line) for line in out.stdout.splitlines()]

    return run


def test_header_needs_no_hip():
    text = open(os.path.join(ROOT, "nerf_prv_amd", "csrc", "prv_queue_order.hpp")).read()
    includes = [line.split()[1] for line in text.splitlines() if line.startswith("#include")]
    assert includes == ["<cstddef>", "<cstdint>", "<vector>"], includes


def test_synthetic_lists_and_keys(program):
    assert program("synthetic") == [{"ok": 1}]


def _bits(a):
    return np.asarray(a, f32).view(np.uint32)


def _wave_file(path, p, layout, cells):
    """the launch's waves that hold a live ray, in launch order: march_emit's preferred region, live rays, mid-span point of the first live lane"""
    c = p.case
    lo, hi = c.occ_box()
    oct_ = p.octants()
    i0 = ((p.first + p.last) >> 1).astype(f32) + f32(0.5)
    t = qc._fma(i0, p.dt, p.t0)
    pm = np.stack([qc._fma(t, p.d[..., a], p.o[..., a]) for a in range(3)], axis=-1)
    lines = [f"{layout.seg_cap(c.n_views)} {layout.n_seg} {layout.n_sub} {cells} " + " ".join(str(int(b)) for b in list(_bits(lo)) + list(_bits(hi)))]
    for lin, lanes in p.waves(layout):
        if not lanes:
            continue
        idx = tuple(np.array(lanes).T)
        lv = p.live[idx]
        if not lv.any():
            continue
        first = int(np.argmax(lv))
        at = tuple(int(a[first]) for a in idx)
        pref = (int(oct_[at]) * layout.n_sub + lin % layout.n_sub) % layout.n_seg
        lines.append(f"{pref} {int(lv.sum())} " + " ".join(str(int(b)) for b in _bits(pm[at])))
    path.write_text("\n".join(lines) + "\n")


RUNS = [("octant_high", qc.FIXED), ("octant_low", qc.NGP), ("one_subregion", qc.FIXED), ("skew", qc.NGP), ("opaque", qc.FIXED),
        ("counts0", qc.FIXED), ("counts1", qc.NGP), ("counts65", qc.FIXED)]


@pytest.mark.parametrize("cells", [2, 8])
@pytest.mark.parametrize("name,mode", RUNS, ids=lambda v: v if isinstance(v, str) else "ngp" if v else "S128")
def test_populations_sort_into_stable_permutations(program, oracle, tmp_path, name, mode, cells):
    c = qc.get(name)
    p = qc.population(oracle, c, mode)
    L = qc.Layout(c.w, c.h, c.spp)
    f = tmp_path / "waves.txt"
    _wave_file(f, p, L, cells)
    (got,) = program("waves", f)
    print(f"QUEUE_ORDER {name} mode {mode} cells {cells}: {got}")
    assert got["rays"] == p.n_rays
    if name.startswith("octant") or name == "one_subregion":
        assert got["straddles"] >= 1 and got["moved"] >= 1  # the tail cut and the waves that moved on are in the sorted lists
    if name == "counts0":
        assert got["descriptors"] == 0 and got["empty"] == 8
    if name == "counts1":
        assert got["descriptors"] == 1 and got["single"] == 1 and got["empty"] == 7
    assert got["max_keys"] <= cells ** 3


@pytest.mark.parametrize("cells", [2, 4, 8])
@pytest.mark.parametrize("mode", [qc.FIXED, qc.NGP], ids=["S128", "ngp"])
def test_one_cell_population_puts_an_octants_descriptors_under_one_key(program, oracle, tmp_path, mode, cells):
    """region_cases.one_cell is what tests/test_gpu_region_cells.py takes it for: an octant region with several 64-descriptor
    steps' worth of descriptors, every one of them under the same key"""
    c = region_cases.one_cell()
    p = qc.population(oracle, c, mode)
    f = tmp_path / "waves.txt"
    _wave_file(f, p, qc.Layout(c.w, c.h, c.spp), cells)
    (got,) = program("waves", f)
    print(f"QUEUE_ORDER one_cell mode {mode} cells {cells}: {got}")
    assert got["rays"] == p.n_rays and got["one_cell"] >= 1
    assert got["one_cell_most"] >= 3 * 64  # order_descriptors_kernel places 64 descriptors per wave step: at least three steps' worth under one key
