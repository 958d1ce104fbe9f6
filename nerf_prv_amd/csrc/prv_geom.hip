// prv_geom.hip -- geometric evaluation: how close is a reconstructed surface to the real one.
//   sample    area-weighted points on a mesh: integer weights, integer scan, stratified choice by binary search
//   nn        nearest reference point per query: counting-sort uniform grid + a wave-per-64-queries shell walk; brute-force twin
//   reduce    accuracy / completeness sums of the distances
// Arithmetic contracts are stated in include/prv.h; -ffp-contract=off keeps every product and sum its own rounding.
#include "prv_geom.hpp"

#include <algorithm>

namespace prv {

namespace {

__device__ __forceinline__ uint64_t g_mix64(uint64_t z) {
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}
// the project's counter-based RNG (prv_train.hip: rng_u24): 24 bits keyed by (seed, stream, i)
__device__ __forceinline__ uint32_t g_rng_u24(uint64_t seed, uint64_t stream, uint64_t i) {
  return (uint32_t)(g_mix64(seed + (stream + 1) * 0xD1B54A32D192ED03ull + i * 0x9E3779B97F4A7C15ull) >> 40);
}

// ------------------------------------------------------------------ sampling
__global__ __launch_bounds__(256) void geom_tri_weight_kernel(const float* __restrict__ xyz, const uint32_t* __restrict__ tri, uint64_t nt,
                                                              uint64_t* __restrict__ weight) {
  const uint64_t t = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (t >= nt) return;
  double v[3][3];
  for (int k = 0; k < 3; k++) {
    const float* p = xyz + 3 * (size_t)tri[3 * t + k];
    for (int a = 0; a < 3; a++) v[k][a] = (double)p[a];
  }
  const double e1[3] = {v[1][0] - v[0][0], v[1][1] - v[0][1], v[1][2] - v[0][2]};
  const double e2[3] = {v[2][0] - v[0][0], v[2][1] - v[0][1], v[2][2] - v[0][2]};
  const double cx = e1[1] * e2[2] - e1[2] * e2[1], cy = e1[2] * e2[0] - e1[0] * e2[2], cz = e1[0] * e2[1] - e1[1] * e2[0];
  const double area = 0.5 * sqrt((cx * cx + cy * cy) + cz * cz);
  const double w = area * kGeomAreaScale;
  weight[t] = w >= 1.0 && w < 4611686018427387904.0 ? (uint64_t)w : 0ull; // NaN, Inf, >= 2^62: no weight
}

__global__ __launch_bounds__(256) void geom_sample_kernel(const float* __restrict__ xyz, const uint32_t* __restrict__ tri,
                                                          const uint64_t* __restrict__ scan, uint64_t nt, uint64_t q, uint64_t r, uint64_t n,
                                                          uint64_t seed, float* __restrict__ out_xyz, uint32_t* __restrict__ out_tri) {
  const uint64_t k = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (k >= n) return;
  // stratum k = [lo, hi) of the total weight W = q n + r: lo = floor(k W / n) = k q + floor(k r / n)   (k r < n^2 <= 2^62)
  const uint64_t lo = k * q + k * r / n, hi = (k + 1) * q + (k + 1) * r / n, len = hi - lo;
  const uint64_t u48 = ((uint64_t)g_rng_u24(seed, kGeomStreamStratum, k) << 24) | (uint64_t)g_rng_u24(seed, kGeomStreamStratum + 1, k);
  const uint64_t off = (__umul64hi(len, u48) << 16) | ((len * u48) >> 48); // floor(len * u48 / 2^48), len < 2^62
  const uint64_t target = lo + off;
  // the last triangle whose exclusive prefix is <= target: its weight is positive
  uint64_t a = 0, b = nt; // scan[a] <= target (scan[0] = 0), answer in [a, b)
  while (b - a > 1) {
    const uint64_t mid = a + (b - a) / 2;
    if (scan[mid] <= target) a = mid;
    else b = mid;
  }
  float u = (float)g_rng_u24(seed, kGeomStreamBary, k) * (1.0f / 16777216.0f);
  float v = (float)g_rng_u24(seed, kGeomStreamBary + 1, k) * (1.0f / 16777216.0f);
  if (u + v > 1.0f) {
    u = 1.0f - u;
    v = 1.0f - v;
  }
  const float* pa = xyz + 3 * (size_t)tri[3 * a];
  const float* pb = xyz + 3 * (size_t)tri[3 * a + 1];
  const float* pc = xyz + 3 * (size_t)tri[3 * a + 2];
  for (int ax = 0; ax < 3; ax++) {
    const float e1 = pb[ax] - pa[ax], e2 = pc[ax] - pa[ax];
    out_xyz[3 * k + ax] = (pa[ax] + u * e1) + v * e2;
  }
  if (out_tri) out_tri[k] = (uint32_t)a;
}

// ------------------------------------------------------------------ nearest neighbours: validation + grid build
__global__ __launch_bounds__(256) void nn_bbox_kernel(const float* __restrict__ xyz, uint64_t n, float* __restrict__ partial,
                                                      uint32_t* __restrict__ flag) {
  __shared__ float red[6][256];
  const float inf = __builtin_inff();
  float mn[3] = {inf, inf, inf}, mx[3] = {-inf, -inf, -inf};
  bool bad = false;
  for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (uint64_t)gridDim.x * 256) {
    for (int a = 0; a < 3; a++) {
      const float p = xyz[3 * i + a];
      bad |= !(fabsf(p) < inf);
      mn[a] = fminf(mn[a], p);
      mx[a] = fmaxf(mx[a], p);
    }
  }
  if (bad) atomicOr(flag, 1u);
  for (int a = 0; a < 3; a++) {
    red[a][threadIdx.x] = mn[a];
    red[3 + a][threadIdx.x] = mx[a];
  }
  __syncthreads();
  for (int d = 128; d > 0; d >>= 1) {
    if ((int)threadIdx.x < d)
      for (int a = 0; a < 3; a++) {
        red[a][threadIdx.x] = fminf(red[a][threadIdx.x], red[a][threadIdx.x + d]);
        red[3 + a][threadIdx.x] = fmaxf(red[3 + a][threadIdx.x], red[3 + a][threadIdx.x + d]);
      }
    __syncthreads();
  }
  if (threadIdx.x < 6) partial[6 * blockIdx.x + threadIdx.x] = red[threadIdx.x][0];
}

__device__ __forceinline__ int nn_cell(const NNGrid& g, float p, int a) {
  float t = (p - g.lo[a]) * g.inv[a];
  t = fminf(fmaxf(t, 0.0f), (float)(g.dims[a] - 1)); // outside the box: the border cell; NaN (Inf * 0): cell 0
  return (int)t;
}
__device__ __forceinline__ uint32_t nn_key(const NNGrid& g, int cx, int cy, int cz) {
  const uint32_t brick = ((uint32_t)(cz >> 2) * (uint32_t)g.nb[1] + (uint32_t)(cy >> 2)) * (uint32_t)g.nb[0] + (uint32_t)(cx >> 2);
  return brick * 64u + (uint32_t)(((cz & 3) << 4) | ((cy & 3) << 2) | (cx & 3));
}

__global__ __launch_bounds__(256) void nn_keys_kernel(NNGrid g, const float* __restrict__ xyz, uint64_t n, uint32_t* __restrict__ keys,
                                                      unsigned long long* __restrict__ count) {
  const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const uint32_t key = nn_key(g, nn_cell(g, xyz[3 * i], 0), nn_cell(g, xyz[3 * i + 1], 1), nn_cell(g, xyz[3 * i + 2], 2));
  keys[i] = key;
  atomicAdd(&count[key], 1ull);
}

__global__ __launch_bounds__(256) void nn_scatter_kernel(const float* __restrict__ xyz, uint64_t n, const uint32_t* __restrict__ keys,
                                                         unsigned long long* __restrict__ cursor, float4* __restrict__ records) {
  const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const unsigned long long at = atomicAdd(&cursor[keys[i]], 1ull);
  records[at] = make_float4(xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2], __uint_as_float((uint32_t)i));
}

__global__ __launch_bounds__(256) void nn_pack_kernel(const float* __restrict__ xyz, uint64_t n, float4* __restrict__ records) {
  const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < n) records[i] = make_float4(xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2], __uint_as_float((uint32_t)i));
}

// ------------------------------------------------------------------ nearest neighbours: queries
// The contract's arithmetic, and the order-independent choice: smaller d2 first, then the smaller id
__device__ __forceinline__ void nn_test(const float4& q, float px, float py, float pz, uint32_t id, float& best, uint32_t& bid) {
  const float dx = q.x - px, dy = q.y - py, dz = q.z - pz;
  const float d2 = (dx * dx + dy * dy) + dz * dz;
  const bool better = d2 < best || (d2 == best && id < bid);
  best = better ? d2 : best;
  bid = better ? id : bid;
}

__device__ __forceinline__ int wave_min(int v) {
  for (int d = 32; d > 0; d >>= 1) v = min(v, __shfl_xor(v, d));
  return __builtin_amdgcn_readfirstlane(v);
}
__device__ __forceinline__ int wave_max(int v) {
  for (int d = 32; d > 0; d >>= 1) v = max(v, __shfl_xor(v, d));
  return __builtin_amdgcn_readfirstlane(v);
}

// One wave = 64 consecutive binned queries: they sit in a small box of cells [c0, c1].  Round r visits the cells of that box
// grown by r that round r - 1 did not; a cell's records are fetched once per wave (lane j loads record j: 16 bytes, one
// coalesced request) and handed to all 64 queries through v_readlane.  After a round every unvisited reference point lies
// beyond a face of the visited box, so a query stops once its best d2 is below the squared distance to the nearest such face,
// less what fp32 rounding can cost (g.slack on the distance: cell assignment and the faces are each good to a few ulp of the
// box's largest coordinate; 2^-20 relative on the square: d2's own rounding) -- strictly below, so an unvisited point can
// neither beat nor tie it.  The wave walks until all its queries have stopped or the box is the whole grid.
__global__ __launch_bounds__(256) void nn_query_grid_kernel(NNGrid g, const float4* __restrict__ ref, const uint64_t* __restrict__ ref_end,
                                                            const float4* __restrict__ queries, uint64_t m, float* __restrict__ out_d2,
                                                            uint32_t* __restrict__ out_id, unsigned long long* __restrict__ tests) {
  const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  const uint64_t wave_first = i & ~63ull;
  if (wave_first >= m) return; // a whole wave: uniform
  const uint32_t lane = threadIdx.x & 63;
  const bool valid = i < m;
  const float4 q = queries[valid ? i : m - 1]; // a tail lane shadows the last query and writes nothing
  const float qv[3] = {q.x, q.y, q.z};
  int c0[3], c1[3];
  for (int a = 0; a < 3; a++) {
    const int c = nn_cell(g, qv[a], a);
    c0[a] = wave_min(c);
    c1[a] = wave_max(c);
  }
  float best = __builtin_inff();
  uint32_t bid = 0xFFFFFFFFu;
  unsigned long long formed = 0;
  int p0[3] = {0, 0, 0}, p1[3] = {-1, -1, -1}; // the box already visited (empty)
  for (int r = 0;; r++) {
    int b0[3], b1[3];
    for (int a = 0; a < 3; a++) {
      b0[a] = max(c0[a] - r, 0);
      b1[a] = min(c1[a] + r, g.dims[a] - 1);
    }
    for (int z = b0[2]; z <= b1[2]; z++)
      for (int y = b0[1]; y <= b1[1]; y++) {
        const bool inner = z >= p0[2] && z <= p1[2] && y >= p0[1] && y <= p1[1];
        for (int x = b0[0]; x <= b1[0]; x++) {
          if (inner && x >= p0[0] && x <= p1[0]) {
            x = p1[0]; // the run of cells of the last round's box
            continue;
          }
          const uint32_t key = nn_key(g, x, y, z);
          const uint32_t s = __builtin_amdgcn_readfirstlane(key ? (uint32_t)ref_end[key - 1] : 0u);
          const uint32_t e = __builtin_amdgcn_readfirstlane((uint32_t)ref_end[key]);
          for (uint32_t base = s; base < e; base += 64) {
            const uint32_t cnt = min(64u, e - base);
            const float4 p = ref[base + min(lane, cnt - 1)];
            for (uint32_t j = 0; j < cnt; j++)
              nn_test(q, __uint_as_float(__builtin_amdgcn_readlane(__float_as_uint(p.x), j)),
                      __uint_as_float(__builtin_amdgcn_readlane(__float_as_uint(p.y), j)),
                      __uint_as_float(__builtin_amdgcn_readlane(__float_as_uint(p.z), j)),
                      __builtin_amdgcn_readlane(__float_as_uint(p.w), j), best, bid);
            formed += cnt;
          }
        }
      }
    bool whole = true;
    float d = __builtin_inff();
    for (int a = 0; a < 3; a++) {
      if (b0[a] > 0) {
        whole = false;
        d = fminf(d, qv[a] - (g.lo[a] + (float)b0[a] * g.cs[a]));
      }
      if (b1[a] < g.dims[a] - 1) {
        whole = false;
        d = fminf(d, (g.lo[a] + (float)(b1[a] + 1) * g.cs[a]) - qv[a]);
      }
    }
    if (whole) break;
    d -= g.slack;
    const bool done = d > 0.0f && best < (d * d) * (1.0f - 0x1p-20f);
    if (__all(done)) break;
    for (int a = 0; a < 3; a++) {
      p0[a] = b0[a];
      p1[a] = b1[a];
    }
  }
  if (valid) {
    const uint32_t at = __float_as_uint(q.w);
    out_d2[at] = best;
    out_id[at] = bid;
  }
  if (lane == 0) atomicAdd(tests, formed * (unsigned long long)min((uint64_t)64, m - wave_first));
}

// the twin: one query per thread, the reference set streamed through LDS 256 records at a time (every lane reads the same
// record: a broadcast, no bank conflict)
__global__ __launch_bounds__(256) void nn_query_brute_kernel(const float4* __restrict__ ref, uint64_t n, const float* __restrict__ queries,
                                                             uint64_t m, float* __restrict__ out_d2, uint32_t* __restrict__ out_id) {
  __shared__ float4 tile[256];
  const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  const bool valid = i < m;
  const uint64_t qi = valid ? i : m - 1;
  const float4 q = make_float4(queries[3 * qi], queries[3 * qi + 1], queries[3 * qi + 2], 0.0f);
  float best = __builtin_inff();
  uint32_t bid = 0xFFFFFFFFu;
  for (uint64_t base = 0; base < n; base += 256) {
    const uint32_t cnt = (uint32_t)min((uint64_t)256, n - base);
    if (threadIdx.x < cnt) tile[threadIdx.x] = ref[base + threadIdx.x];
    __syncthreads();
    for (uint32_t j = 0; j < cnt; j++) {
      const float4 p = tile[j];
      nn_test(q, p.x, p.y, p.z, __float_as_uint(p.w), best, bid);
    }
    __syncthreads();
  }
  if (valid) {
    out_d2[i] = best;
    out_id[i] = bid;
  }
}

// ------------------------------------------------------------------ metrics
__global__ __launch_bounds__(256) void geom_reduce_kernel(const float* __restrict__ d2, uint64_t n, float tau, GeomPartial* __restrict__ partial) {
  __shared__ double s_d[256], s_d2[256];
  __shared__ uint64_t s_in[256];
  __shared__ float s_mx[256];
  double sd = 0.0, sd2 = 0.0;
  uint64_t in = 0;
  float mx = 0.0f;
  for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (uint64_t)gridDim.x * 256) {
    const float v = d2[i], d = (float)sqrt((double)v); // correctly rounded: the fp64 root of an fp32 value rounds once more without harm
    sd += (double)d;
    sd2 += (double)v;
    in += d <= tau ? 1u : 0u;
    mx = fmaxf(mx, d);
  }
  s_d[threadIdx.x] = sd;
  s_d2[threadIdx.x] = sd2;
  s_in[threadIdx.x] = in;
  s_mx[threadIdx.x] = mx;
  __syncthreads();
  for (int k = 128; k > 0; k >>= 1) { // a fixed tree: the same sum every run
    if ((int)threadIdx.x < k) {
      s_d[threadIdx.x] += s_d[threadIdx.x + k];
      s_d2[threadIdx.x] += s_d2[threadIdx.x + k];
      s_in[threadIdx.x] += s_in[threadIdx.x + k];
      s_mx[threadIdx.x] = fmaxf(s_mx[threadIdx.x], s_mx[threadIdx.x + k]);
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) partial[blockIdx.x] = GeomPartial{s_d[0], s_d2[0], s_in[0], s_mx[0], 0u};
}

__global__ void geom_reduce_final_kernel(const GeomPartial* __restrict__ partial, int blocks, GeomPartial* __restrict__ out) {
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  GeomPartial t{0.0, 0.0, 0ull, 0.0f, 0u};
  for (int b = 0; b < blocks; b++) { // block order
    t.sum_d += partial[b].sum_d;
    t.sum_d2 += partial[b].sum_d2;
    t.within += partial[b].within;
    t.max_d = fmaxf(t.max_d, partial[b].max_d);
  }
  *out = t;
}

inline unsigned blocks_of(uint64_t n) { return (unsigned)((n + 255) / 256); }

} // namespace

hipError_t launch_geom_tri_weights(const float* xyz, const uint32_t* tri, uint64_t nt, uint64_t* weight, hipStream_t s) {
  hipLaunchKernelGGL(geom_tri_weight_kernel, dim3(blocks_of(nt)), dim3(256), 0, s, xyz, tri, nt, weight);
  return hipGetLastError();
}

hipError_t launch_geom_sample(const float* xyz, const uint32_t* tri, const uint64_t* scan, uint64_t nt, uint64_t total, uint64_t n,
                              uint64_t seed, float* out_xyz, uint32_t* out_tri, hipStream_t s) {
  hipLaunchKernelGGL(geom_sample_kernel, dim3(blocks_of(n)), dim3(256), 0, s, xyz, tri, scan, nt, total / n, total % n, n, seed, out_xyz,
                     out_tri);
  return hipGetLastError();
}

hipError_t launch_nn_bbox(const float* xyz, uint64_t n, float* partial, uint32_t* flag, hipStream_t s) {
  hipLaunchKernelGGL(nn_bbox_kernel, dim3(kNNBoxBlocks), dim3(256), 0, s, xyz, n, partial, flag);
  return hipGetLastError();
}

hipError_t launch_nn_keys(const NNGrid& g, const float* xyz, uint64_t n, uint32_t* keys, uint64_t* count, hipStream_t s) {
  hipLaunchKernelGGL(nn_keys_kernel, dim3(blocks_of(n)), dim3(256), 0, s, g, xyz, n, keys, (unsigned long long*)count);
  return hipGetLastError();
}

hipError_t launch_nn_scatter(const float* xyz, uint64_t n, const uint32_t* keys, uint64_t* cursor, float4* records, hipStream_t s) {
  hipLaunchKernelGGL(nn_scatter_kernel, dim3(blocks_of(n)), dim3(256), 0, s, xyz, n, keys, (unsigned long long*)cursor, records);
  return hipGetLastError();
}

hipError_t launch_nn_pack(const float* xyz, uint64_t n, float4* records, hipStream_t s) {
  hipLaunchKernelGGL(nn_pack_kernel, dim3(blocks_of(n)), dim3(256), 0, s, xyz, n, records);
  return hipGetLastError();
}

hipError_t launch_nn_query_grid(const NNGrid& g, const float4* ref, const uint64_t* ref_end, const float4* queries, uint64_t m,
                                float* out_d2, uint32_t* out_id, unsigned long long* tests, hipStream_t s) {
  hipLaunchKernelGGL(nn_query_grid_kernel, dim3(blocks_of(m)), dim3(256), 0, s, g, ref, ref_end, queries, m, out_d2, out_id, tests);
  return hipGetLastError();
}

hipError_t launch_nn_query_brute(const float4* ref, uint64_t n, const float* queries, uint64_t m, float* out_d2, uint32_t* out_id,
                                 hipStream_t s) {
  hipLaunchKernelGGL(nn_query_brute_kernel, dim3(blocks_of(m)), dim3(256), 0, s, ref, n, queries, m, out_d2, out_id);
  return hipGetLastError();
}

hipError_t launch_geom_reduce(const float* d2, uint64_t n, float tau, GeomPartial* partial, GeomPartial* out, hipStream_t s) {
  hipLaunchKernelGGL(geom_reduce_kernel, dim3(kGeomReduceBlocks), dim3(256), 0, s, d2, n, tau, partial);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(geom_reduce_final_kernel, dim3(1), dim3(64), 0, s, (const GeomPartial*)partial, kGeomReduceBlocks, out);
  return hipGetLastError();
}

} // namespace prv
