// prv_field_plan.hpp -- everything an install of a model decides on the host, before anything is allocated or copied: the
// physical table layout and the kernel instance, the occupancy summary, the MFMA fragments, the replicas, the synthetic field's
// arrays.  Host only, no HIP (tests/test_field_plan_host.py builds it alone); prv_api.cpp allocates, copies and launches by it.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/prv.h"
#include "prv_levels.hpp"

namespace prv {

// ---- the compiled instances of the field-evaluating kernels (render, planes, mesh, field hook): NDENSE = the field's count of
// leading dense levels when an instance for exactly that count exists (5 / 3 for F = 4, 10 / 6 for F = 2: api.FIELD_256 /
// FIELD_512 run <4,5> / <2,10>) and its hashed levels share their hash constants; any other field -- util.SMALL (4 dense),
// SMALL_F2 (9), instant-ngp's base.json (F = 2, 5 dense), levels > 16 MiB -- runs <F, 0> (tests/instances.py)
inline int instance_dense_levels(int n_features, int n_dense, int hash_shared) {
  if (!hash_shared) return 0;
  if (n_features == 4) return n_dense == 5 ? 5 : n_dense == 3 ? 3 : 0;
  return n_dense == 10 ? 10 : n_dense == 6 ? 6 : 0;
}

// ---- the field

struct LevelPlan { // LevelDev's members, in its order (prv_device.hpp says what the kernels do with them; prv_api.cpp: fill_field_dev)
  float scale;
  uint32_t res_m1, my_b, mz_b, m_b, off_b, myz_b, pack;
};

struct FieldPlan {
  prv_field_desc desc;
  int n_levels; // desc.n_levels once compute_levels has accepted the descriptor, 0 before
  HostLevel lv[kMaxFieldLevels];
  uint64_t total; // canonical entries of all levels
  // the physical layout, in entries: dense levels have power-of-two strides (1 << sx vertices per row, as many rows per plane)
  // and every level starts at a multiple of its own power-of-two size
  uint32_t sx[kMaxFieldLevels], psize[kMaxFieldLevels], poff[kMaxFieldLevels];
  uint64_t ptotal;
  LevelPlan levels[kMaxFieldLevels];
  int n_dense_levels, n_hashed_levels;
  uint32_t hash_my_b, hash_mz_b, hash_m_b;
  int hash_shared, wide_offsets;

  uint32_t ebytes() const { return (uint32_t)desc.n_features * 2u; }
  uint64_t table_halfs() const { return total * (uint64_t)desc.n_features; }
  uint64_t phys_bytes() const { return ptotal * ebytes(); }
  uint64_t occ_words() const { return ((uint64_t)desc.occ_res * desc.occ_res * desc.occ_res + 31) / 32; }
  bool has_coarse_occupancy() const { return desc.occ_res % 4 == 0 && desc.occ_res >= 8; }
  int instance() const { return instance_dense_levels(desc.n_features, n_dense_levels, hash_shared); }
};

// PRV_OK, or the code of the rejection with its text in `err`.  no_pair (PRV_NO_PAIR, the tests' switch): every level goes
// through the generic (clamped, 8-load) gather -- no dense level is counted and the hash constants are not shared.
inline int plan_field(const prv_field_desc& d, bool no_pair, FieldPlan& P, std::string& err) {
  auto reject = [&](const char* fmt, unsigned a = 0, unsigned b = 0) {
    char buf[128];
    snprintf(buf, sizeof(buf), fmt, a, b);
    err = buf;
    return (int)PRV_E_INVALID;
  };
  P = FieldPlan{};
  P.desc = d;
  if (compute_levels(d, P.lv, &P.total) != 0) return reject("invalid field descriptor");
  P.n_levels = d.n_levels;
  const HostLevel* lv = P.lv;
  const uint32_t ebytes = P.ebytes();
  // ---- physical layout: power-of-two strides for dense levels, size-aligned level offsets
  int order[kMaxFieldLevels];
  auto ceil_log2 = [](uint32_t v) { uint32_t s = 0; while ((1u << s) < v) s++; return s; };
  for (int l = 0; l < d.n_levels; l++) {
    order[l] = l;
    if (lv[l].hashed) {
      P.sx[l] = 0;
      P.psize[l] = lv[l].size;
      P.n_hashed_levels++;
    } else {
      P.sx[l] = ceil_log2(lv[l].res + 1); // +1: room for the duplicated border vertex / row / plane
      P.psize[l] = 1u << ceil_log2((lv[l].res + 1u) << (2 * P.sx[l])); // res + 1 planes: the last one is duplicated
    }
  }
  std::stable_sort(order, order + d.n_levels, [&](int a, int b) { return P.psize[a] > P.psize[b]; });
  for (int k = 0; k < d.n_levels; k++) {
    P.poff[order[k]] = (uint32_t)P.ptotal; // multiple of every later (smaller or equal) power of two
    P.ptotal += P.psize[order[k]];
  }
  if (P.ptotal * ebytes >= (1ull << 32)) return reject("field too large for 32-bit gather offsets");
  while (!no_pair && P.n_dense_levels < d.n_levels && !lv[P.n_dense_levels].hashed) P.n_dense_levels++;
  // the hashed levels' shared constants (every hashed level has T entries of ebytes): valid for the kernel's shared path
  // when no hashed level is finer than its table, so that (x << esh) needs no mask
  P.hash_my_b = (2654435761u * ebytes) & 0xffffffu;
  P.hash_mz_b = (805459861u * ebytes) & 0xffffffu;
  P.hash_m_b = (uint32_t)(((1ull << d.log2_hashmap) - 1ull) * ebytes);
  P.hash_shared = no_pair ? 0 : 1;
  for (int l = 0; l < d.n_levels; l++) {
    LevelPlan& L = P.levels[l];
    L.scale = lv[l].scale;
    L.res_m1 = lv[l].res - 1;
    if (lv[l].res > 4096) return reject("level %d has %u vertices per axis (limit 4096)", (unsigned)l, lv[l].res);
    if (lv[l].hashed) {
      if (lv[l].res > lv[l].size) P.hash_shared = 0;
      // the kernels multiply with v_mul_u32_u24 (the low 24 bits of the constants are all a level of <= 16 MiB needs).  A hashed
      // level LARGER than 16 MiB (round 6: tables that really leave the 256 MiB Infinity Cache, e.g. log2_hashmap 24 at F = 2)
      // keeps the full 32-bit constants and runs the generic instance, whose gather then multiplies in 32 bits (wide_offsets)
      if ((uint64_t)(lv[l].size - 1u) * ebytes >= (1ull << 32)) return reject("hashed level of 4 GiB or more");
      L.m_b = (lv[l].size - 1u) * ebytes;
      const bool wide = L.m_b >= (1u << 24);
      L.my_b = wide ? 2654435761u * ebytes : (2654435761u * ebytes) & 0xffffffu;
      L.mz_b = wide ? 805459861u * ebytes : (805459861u * ebytes) & 0xffffffu;
      if (wide) {
        P.wide_offsets = 1;
        P.hash_shared = 0;
      }
    } else {
      L.my_b = ebytes << P.sx[l];
      L.mz_b = ebytes << (2 * P.sx[l]);
      L.m_b = 0xffffffffu;
      if (L.mz_b >= (1u << 24)) return reject("dense level too large");
    }
    L.off_b = P.poff[l] * ebytes;
    L.myz_b = L.my_b + L.mz_b;
    // the render kernel's packed word (prv_device.hpp: LevelDev::pack); the alignment the packing relies on is checked
    // (a field whose offsets leave no room for it -- hashed tables below 4 KiB -- runs the generic instance, which reads the
    // unpacked constants)
    if (lv[l].hashed) {
      if ((L.off_b & 4095u) != 0u || L.res_m1 > 4095u) P.hash_shared = 0;
      L.pack = (L.off_b & ~4095u) | (L.res_m1 & 4095u);
    } else {
      if ((L.off_b & 31u) != 0u || P.sx[l] > 31u) P.hash_shared = 0;
      L.pack = (L.off_b & ~31u) | (P.sx[l] & 31u);
    }
  }
  return PRV_OK;
}

// ---- the occupancy grid (R^3 bits, x fastest)

struct OccupancySummary {
  float lo[3], hi[3];           // the occupied cells' bounding box grown by one cell, for the march pass; an empty grid: an empty box
  std::vector<uint32_t> coarse; // (R/4)^3 bits: any occupied fine cell in the 4^3 block or in its 26 neighbour blocks; empty
                                // when R is no multiple of 4 or below 8 (the march pass then goes without)
};

inline OccupancySummary summarize_occupancy(const uint32_t* occ, int R) {
  OccupancySummary S;
  const bool has_coarse = R % 4 == 0 && R >= 8;
  const int Rc = R / 4;
  std::vector<uint8_t> blk(has_coarse ? (size_t)Rc * Rc * Rc : 0, 0);
  int lo[3] = {R, R, R}, hi[3] = {-1, -1, -1};
  // a row goes by 32 cells at a time.  R % 32 == 0: each is one whole word, and a zero word costs one test -- 65 K words
  // instead of 2 M bits for a 128^3 grid (the planner loop installs five fields per round).  Any other R: the 32 (or the
  // row's last few) bits are put together from the two words they lie in
  for (int z = 0; z < R; z++)
    for (int y = 0; y < R; y++)
      for (int x0 = 0; x0 < R; x0 += 32) {
        const size_t b = (size_t)x0 + (size_t)R * ((size_t)y + (size_t)R * (size_t)z);
        const int n = std::min(32, R - x0), sh = (int)(b & 31);
        uint32_t v = occ[b >> 5] >> sh;
        if (sh + n > 32) v |= occ[(b >> 5) + 1] << (32 - sh);
        if (n < 32) v &= (1u << n) - 1u;
        if (!v) continue;
        lo[0] = std::min(lo[0], x0 + __builtin_ctz(v));
        hi[0] = std::max(hi[0], x0 + 31 - __builtin_clz(v));
        lo[1] = std::min(lo[1], y);
        hi[1] = std::max(hi[1], y);
        lo[2] = std::min(lo[2], z);
        hi[2] = std::max(hi[2], z);
        if (!has_coarse) continue;
        uint8_t* row = &blk[(size_t)(x0 / 4) + (size_t)Rc * ((size_t)(y / 4) + (size_t)Rc * (size_t)(z / 4))];
        for (int k = 0; 4 * k < n; k++) // (R is a multiple of 4: a block's four cells never straddle two rows)
          if ((v >> (4 * k)) & 0xfu) row[k] = 1;
      }
  for (int a = 0; a < 3; a++) {
    S.lo[a] = hi[a] < 0 ? 2.0f : (float)(lo[a] - 1) / (float)R;
    S.hi[a] = hi[a] < 0 ? -1.0f : (float)(hi[a] + 2) / (float)R;
  }
  if (!has_coarse) return S;
  S.coarse.assign(((size_t)Rc * Rc * Rc + 31) / 32, 0u);
  for (int z = 0; z < Rc; z++)
    for (int y = 0; y < Rc; y++)
      for (int x = 0; x < Rc; x++) {
        bool any = false;
        for (int dz = -1; dz <= 1 && !any; dz++)
          for (int dy = -1; dy <= 1 && !any; dy++)
            for (int dx = -1; dx <= 1 && !any; dx++) {
              const int xx = x + dx, yy = y + dy, zz = z + dz;
              if (xx < 0 || yy < 0 || zz < 0 || xx >= Rc || yy >= Rc || zz >= Rc) continue;
              any = blk[(size_t)xx + (size_t)Rc * ((size_t)yy + (size_t)Rc * (size_t)zz)] != 0;
            }
        if (any) {
          const size_t b = (size_t)x + (size_t)Rc * ((size_t)y + (size_t)Rc * (size_t)z);
          S.coarse[b >> 5] |= 1u << (b & 31);
        }
      }
  return S;
}

// ---- MFMA A-fragment prepack.  Canonical weights W[layer][in][out] (fp16 bits).
// Fragment (layer, mt, s): lane (r,h), element j = W[kmap(s,h,j)][32*mt + r], zero past n_out.
constexpr int kPlanNumFrags = 24;      // prv_device.hpp: kNumFrags, kFragHalfs (prv_api.cpp asserts that they agree)
constexpr int kPlanFragHalfs = 64 * 8;
const int kIn[5] = {32, 64, 32, 64, 64};
const int kOut[5] = {64, 16, 64, 64, 16};
const int kOff[5] = {0, 2048, 3072, 5120, 9216};

// hidden unit held by element j of lane half h in k-step s of a 64-wide activation
inline int hidden_k(int s, int h, int j) { return 32 * (s >> 1) + 16 * (s & 1) + 8 * (j >> 2) + 4 * h + (j & 3); }

// v64 = the fragment set of render_queue64: first-layer k rows in canonical feature order (the lane gathers every
// level of its own sample), and the units the compositing needs repeated in padding rows that land in lane half 1:
// density layer 2's unit 0 at row 20 (register 8), colour layer 3's units 0..2 at rows 20..22 (registers 8..10).
inline std::vector<uint16_t> prepack_fragments(const uint16_t* mlp, int n_features, bool v64) {
  std::vector<uint16_t> frags((size_t)kPlanNumFrags * kPlanFragHalfs, 0);
  int f = 0;
  auto emit = [&](int layer, int mt, int s, int (*kmap)(int, int, int)) {
    uint16_t* dst = frags.data() + (size_t)f * kPlanFragHalfs;
    for (int lane = 0; lane < 64; lane++) {
      const int r = lane & 31, h = lane >> 5;
      int out = 32 * mt + r;
      if (v64 && (layer == 1 || layer == 4) && out >= 20 && out < 20 + (layer == 1 ? 1 : 3)) out -= 20;
      for (int j = 0; j < 8; j++) {
        const int k = kmap(s, h, j);
        dst[lane * 8 + j] = out < kOut[layer] ? mlp[kOff[layer] + k * kOut[layer] + out] : (uint16_t)0;
      }
    }
    f++;
  };
  // grid features: fragment s, element j of lane half h = feature (j % F) of level 2*(s*LH/2 + j/F) + h
  auto k_feat4 = [](int s, int h, int j) { return 4 * (2 * (s * 2 + j / 4) + h) + j % 4; };
  auto k_feat2 = [](int s, int h, int j) { return 2 * (2 * (s * 4 + j / 2) + h) + j % 2; };
  auto k_rgb_in = [](int s, int h, int j) { return s == 0 ? hidden_k(0, h, j) : 16 + 8 * h + j; }; // [dens | SH]
  auto k_canon = [](int s, int h, int j) { return 16 * s + 8 * h + j; };
  for (int mt = 0; mt < 2; mt++)
    for (int s = 0; s < 2; s++)
      emit(0, mt, s, v64 ? (int (*)(int, int, int))k_canon : n_features == 4 ? (int (*)(int, int, int))k_feat4 : (int (*)(int, int, int))k_feat2);
  for (int s = 0; s < 4; s++) emit(1, 0, s, hidden_k);
  for (int mt = 0; mt < 2; mt++)
    for (int s = 0; s < 2; s++) emit(2, mt, s, k_rgb_in);
  for (int mt = 0; mt < 2; mt++)
    for (int s = 0; s < 4; s++) emit(3, mt, s, hidden_k);
  for (int s = 0; s < 4; s++) emit(4, 0, s, hidden_k);
  return frags;
}

// ---- dense replicas of the leading hashed levels (prv_device.hpp: ReplicaDev)

// one replica of a level of `res` vertices per axis: rows of res + 1 entries rounded up to 8, as many rows per plane, res + 1
// planes; levels start at multiples of 4 KiB.  0 bytes: the level cannot be replicated (its z stride must stay below 2^24 for
// the gather's 24-bit multiplies, its row count / 8 inside the 12 low bits of the pack word)
struct ReplicaLevelLayout {
  uint32_t row;   // entries per row = rows per plane
  uint64_t bytes; // row * row * (res + 1) * ebytes, rounded up to 4 KiB
};
inline ReplicaLevelLayout replica_level_layout(uint32_t res, uint32_t ebytes) {
  const uint32_t row = (res + 1u + 7u) & ~7u;
  const uint64_t mz = (uint64_t)row * row * ebytes;
  if (mz >= (1ull << 24) || row / 8u > 4095u) return {row, 0};
  return {row, (mz * (res + 1u) + 4095ull) & ~4095ull};
}

constexpr int kPlanMaxReplicas = 3; // prv_device.hpp: kMaxReplicas
struct ReplicaPlan {
  int n;                           // levels n_dense_levels .. n_dense_levels + n - 1 are replicated
  uint32_t pack[kPlanMaxReplicas]; // ReplicaDev::pack: byte offset | row entries / 8
  uint64_t total_bytes;
};
// Only a field whose render runs the <4, 5> instance gets replicas (F = 2, the generic instances, wide offsets, levels finer
// than their table: none): as many levels, from the coarsest hashed one, as fit budget_bytes, and at most max_levels.
inline ReplicaPlan plan_replicas(const FieldPlan& P, int max_levels, uint64_t budget_bytes) {
  ReplicaPlan R{};
  if (P.desc.n_features != 4 || P.instance() != 5) return R;
  for (int l = P.n_dense_levels; l < P.n_levels && R.n < std::min(max_levels, kPlanMaxReplicas); l++, R.n++) {
    const uint32_t res = P.levels[l].res_m1 + 1u;
    const ReplicaLevelLayout lay = replica_level_layout(res, 8u);
    if (res > 1024u || lay.bytes == 0 || R.total_bytes + lay.bytes > budget_bytes || R.total_bytes + lay.bytes >= (1ull << 32)) break;
    R.pack[R.n] = (uint32_t)R.total_bytes | (lay.row / 8u); // total_bytes is a multiple of 4 KiB, row / 8 < 4096
    R.total_bytes += lay.bytes;
  }
  return R;
}

constexpr uint64_t kReplicaBudgetDefault = (uint64_t)256 << 20; // api.FIELD_256: 13.5 + 43.1 + 143.3 MB for its three hashed levels

// ---- the host-made arrays of a synthetic field: fp16 conversion and a counter RNG for the (tiny) MLP, four spheres of occupancy
namespace synth { // (prv_kernels.hip has a device mix64 of its own, for the table)
inline uint16_t f2h(float f) { // IEEE binary32 -> binary16 bits, round to nearest even (written out: not every host compiler has _Float16)
  uint32_t x;
  memcpy(&x, &f, 4);
  const uint32_t sign = (x >> 16) & 0x8000u;
  x &= 0x7fffffffu;
  if (x > 0x7f800000u) return (uint16_t)(sign | 0x7e00u | ((x >> 13) & 0x3ffu)); // NaN stays NaN
  if (x >= 0x47800000u) return (uint16_t)(sign | 0x7c00u);                        // 2^16 and above, infinity
  if (x < 0x33000000u) return (uint16_t)sign;                                      // below 2^-25: zero
  uint32_t m = x, shift = 13, bias = 0x38000000u >> 13; // a normal half: drop 13 mantissa bits, rebias the exponent
  if (x < 0x38800000u) {                                // below 2^-14, a subnormal half: units of 2^-24
    m = (x & 0x7fffffu) | 0x800000u;
    shift = 126u - (x >> 23);
    bias = 0;
  }
  uint32_t r = (m >> shift) - bias;
  const uint32_t rem = m & ((1u << shift) - 1u), half = 1u << (shift - 1u);
  if (rem > half || (rem == half && (r & 1u))) r++; // (a carry into the exponent, up to infinity, is the right answer)
  return (uint16_t)(sign | r);
}
inline uint64_t mix64(uint64_t z) {
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}
inline float rng_sym(uint64_t seed, uint64_t stream, uint64_t i, float amp) {
  const uint64_t hsh = mix64(seed + (stream + 1) * 0xD1B54A32D192ED03ull + i * 0x9E3779B97F4A7C15ull);
  const uint32_t u = (uint32_t)(hsh >> 40);
  const float v = (float)u * (1.0f / 8388608.0f) - 1.0f;
  return v * amp;
}
const float kSpheres[4][4] = {
    {0.50f, 0.50f, 0.50f, 0.35f}, {0.80f, 0.50f, 0.62f, 0.13f}, {0.36f, 0.80f, 0.45f, 0.11f}, {0.40f, 0.24f, 0.78f, 0.10f}};
} // namespace synth

inline std::vector<uint16_t> synthetic_mlp(uint64_t seed) { // Xavier-uniform weights, layer l from stream l + 1
  std::vector<uint16_t> mlp(PRV_MLP_HALFS);
  size_t o = 0;
  for (int l = 0; l < 5; l++) {
    const float amp = sqrtf(6.0f / (float)(kIn[l] + kOut[l]));
    const size_t cnt = (size_t)kIn[l] * kOut[l];
    for (size_t i = 0; i < cnt; i++) mlp[o + i] = synth::f2h(synth::rng_sym(seed, (uint64_t)(l + 1), i, amp));
    o += cnt;
  }
  return mlp;
}

inline std::vector<uint32_t> synthetic_occupancy(int R, bool all_occupied) {
  const size_t n_cells = (size_t)R * R * R;
  std::vector<uint32_t> occ((n_cells + 31) / 32, 0u);
  if (all_occupied) { // a fresh field (the planner loop makes five per round): every cell, without the walk over 2 M of them
    std::fill(occ.begin(), occ.end(), 0xffffffffu);
    if (n_cells & 31) occ.back() = (1u << (n_cells & 31)) - 1u;
    return occ;
  }
  const float invR = 1.0f / (float)R;
  for (int z = 0; z < R; z++)
    for (int y = 0; y < R; y++)
      for (int x = 0; x < R; x++) {
        const float cx = ((float)x + 0.5f) * invR, cy = ((float)y + 0.5f) * invR, cz = ((float)z + 0.5f) * invR;
        bool in = false;
        for (int b = 0; b < 4 && !in; b++) {
          const float dx = cx - synth::kSpheres[b][0], dy = cy - synth::kSpheres[b][1], dz = cz - synth::kSpheres[b][2];
          const float d2 = fmaf(dx, dx, fmaf(dy, dy, dz * dz));
          in = d2 <= synth::kSpheres[b][3] * synth::kSpheres[b][3];
        }
        if (in) {
          const size_t bit = (size_t)x + (size_t)R * ((size_t)y + (size_t)R * (size_t)z);
          occ[bit >> 5] |= 1u << (bit & 31);
        }
      }
  return occ;
}

} // namespace prv
