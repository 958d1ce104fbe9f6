// prv_mesh.hip -- mesh extraction: the density grid of a field, marching cubes on a sigma grid, vertex colours.
//
// Marching cubes runs in deterministic passes: nothing whose order reaches the output depends on atomics or scheduling.
//   classify   per point: crossing flags of its +x/+y/+z edge (one byte), the case of its cell (one byte); per wave of 64
//              points: its vertex and triangle counts
//   scan       exclusive scans of the per-wave counts (hand-written, integer: exact and order-free)
//   emit       vertices in edge-id order (edge id = 3 * point + axis), triangles in cell order, each cell's in table order;
//              a lane ranks itself inside its wave with __ballot / __popcll, and the vertex id of any edge is found from
//              its wave's offset and the crossing flags of the points before it in that wave (64 bytes, 8 words)
// Extra memory: 2 bytes per grid point plus 16 bytes per wave (and the scan's scratch, 1/4096 of that).
// Arithmetic is fp32 with -ffp-contract=off, in the order tests/mesh_ref.py states it.
#include "prv_kernels.hpp"
#include "prv_mc_tables.hpp"
#include "prv_mesh.hpp"

namespace prv {

namespace {

constexpr int kScanPer = 16;                 // elements per thread of the scan
constexpr int kScanChunk = 256 * kScanPer;   // elements per block

__device__ __forceinline__ float grid_coord(const MeshGrid& g, int a, int i) { return g.lo[a] + (float)i * g.step[a]; }

__device__ __forceinline__ uint64_t lanes_below() { return (1ull << (threadIdx.x & 63)) - 1ull; }

// ------------------------------------------------------------------ density grid
template <int F, int NDENSE>
__global__ __launch_bounds__(256) void mesh_density_kernel(FieldDev fd, MeshGrid g, int use_occ, int brick, uint32_t n_waves,
                                                           float* __restrict__ sigma) {
  __shared__ half8 wl[8 * 64]; // the density layers' fragments of the frags64 set
  for (int i = threadIdx.x; i < 8 * 64; i += 256) wl[i] = fd.frags64[i];
  __syncthreads();
  const uint32_t wave = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (wave >= n_waves) return; // wave-uniform
  const int lane = threadIdx.x & 63, grp = lane >> 5;
  int ix, iy, iz;
  if (brick) { // one wave = a 4x4x4 brick: its 64 points share most hash-grid corners
    const uint32_t nbx = (uint32_t)(g.res[0] + 3) >> 2, nby = (uint32_t)(g.res[1] + 3) >> 2;
    const uint32_t bx = wave % nbx, byz = wave / nbx, by = byz % nby, bz = byz / nby;
    ix = (int)(4 * bx) + (lane & 3);
    iy = (int)(4 * by) + ((lane >> 2) & 3);
    iz = (int)(4 * bz) + (lane >> 4);
  } else {
    const uint32_t idx = wave * 64 + lane, rxy = (uint32_t)g.res[0] * (uint32_t)g.res[1];
    ix = (int)(idx % (uint32_t)g.res[0]);
    iy = (int)((idx % rxy) / (uint32_t)g.res[0]);
    iz = (int)(idx / rxy);
  }
  const bool ok = ix < g.res[0] && iy < g.res[1] && iz < g.res[2];
  float p[3] = {0.5f, 0.5f, 0.5f};
  if (ok) {
    p[0] = grid_coord(g, 0, ix);
    p[1] = grid_coord(g, 1, iy);
    p[2] = grid_coord(g, 2, iz);
  }
  const size_t out = ok ? (size_t)ix + (size_t)g.res[0] * ((size_t)iy + (size_t)g.res[1] * (size_t)iz) : 0;
  const bool occ = ok && (!use_occ || occupied(fd, p[0], p[1], p[2]));
  if (use_occ && __ballot(occ) == 0ull) { // no occupied point in the wave: no MLP work
    if (ok) sigma[out] = 0.0f;
    return;
  }
  half8 f[4];
  const HashConsts hc = {fd.hash_my_b, fd.hash_mz_b, fd.hash_m_b, (uint32_t)fd.wide_offsets};
  encode_sample<F, NDENSE>(fd.table, fd.levels, hc, p[0], p[1], p[2], f);
  swap_halves(f[0], f[1]);
  swap_halves(f[2], f[3]);
  const half8 fA[2] = {f[0], f[2]}, fB[2] = {f[1], f[3]};
  f32x16 densA, densB;
  mlp_density2(wl, lane, fA, fB, densA, densB);
  if (ok) sigma[out] = occ ? fast_exp((grp ? densB[8] : densA[0]) + fd.density_bias) : 0.0f;
}

// ------------------------------------------------------------------ kept cells (masked extraction only)
// kept[point] = 1 iff the point is the low corner of a cell whose eight corners are all valid; the tail of the last block is 0
__global__ __launch_bounds__(256) void mesh_kept_kernel(const uint8_t* __restrict__ valid, MeshGrid g, uint32_t n_points, uint8_t* __restrict__ kept) {
  const uint32_t idx = blockIdx.x * 256 + threadIdx.x;
  const uint32_t rx = (uint32_t)g.res[0], ry = (uint32_t)g.res[1], rz = (uint32_t)g.res[2], rxy = rx * ry;
  uint32_t k = 0;
  if (idx < n_points) {
    const uint32_t x = idx % rx, y = (idx % rxy) / rx, z = idx / rxy;
    if (x + 1 < rx && y + 1 < ry && z + 1 < rz) {
      k = 1;
#pragma unroll
      for (int c = 0; c < 8; c++) k &= (uint32_t)(valid[idx + (c & 1) + ((c >> 1) & 1) * rx + (c >> 2) * rxy] != 0);
    }
  }
  kept[idx] = (uint8_t)k;
}

// ------------------------------------------------------------------ classify
// kept == nullptr: every cell counts.  Otherwise only kept cells have a case, and a crossing edge has a vertex only if one of
// the (up to four) cells around it is kept
__global__ __launch_bounds__(256) void mesh_classify_kernel(const float* __restrict__ sigma, MeshGrid g, float thr, uint32_t n_points,
                                                            const uint8_t* __restrict__ kept, uint8_t* __restrict__ flags,
                                                            uint8_t* __restrict__ cases, uint64_t* __restrict__ wave_v,
                                                            uint64_t* __restrict__ wave_t) {
  const uint32_t idx = blockIdx.x * 256 + threadIdx.x;
  const uint32_t rx = (uint32_t)g.res[0], ry = (uint32_t)g.res[1], rz = (uint32_t)g.res[2], rxy = rx * ry;
  uint32_t fl = 0, cs = 0;
  if (idx < n_points) {
    const uint32_t x = idx % rx, y = (idx % rxy) / rx, z = idx / rxy;
    const bool in0 = sigma[idx] > thr; // strict: NaN is outside
    if (x + 1 < rx && in0 != (sigma[idx + 1] > thr)) fl |= 1u;
    if (y + 1 < ry && in0 != (sigma[idx + rx] > thr)) fl |= 2u;
    if (z + 1 < rz && in0 != (sigma[idx + rxy] > thr)) fl |= 4u;
    if (x + 1 < rx && y + 1 < ry && z + 1 < rz) {
#pragma unroll
      for (int c = 0; c < 8; c++) {
        const uint32_t q = idx + (c & 1) + ((c >> 1) & 1) * rx + (c >> 2) * rxy;
        cs |= (uint32_t)(sigma[q] > thr) << c;
      }
    }
    if (kept) { // uniform
      if (!kept[idx]) cs = 0;
      // the cells around the +a edge of this point: the point's own and those one step back along the other two axes (a point
      // without a cell has kept = 0, so only the steps below 0 need a test)
      const uint32_t pos[3] = {x, y, z}, stride[3] = {1u, rx, rxy};
#pragma unroll
      for (int a = 0; a < 3; a++) {
        if (!((fl >> a) & 1u)) continue;
        const int b = (a + 1) % 3, c = (a + 2) % 3;
        bool any = false;
#pragma unroll
        for (int k = 0; k < 4; k++) {
          const uint32_t db = k & 1, dc = k >> 1;
          if (pos[b] >= db && pos[c] >= dc) any = any || kept[idx - db * stride[b] - dc * stride[c]] != 0;
        }
        if (!any) fl &= ~(1u << a);
      }
    }
  }
  const uint32_t nt = kMcTriCount[cs];
  const uint64_t b0 = __ballot(fl & 1u), b1 = __ballot(fl & 2u), b2 = __ballot(fl & 4u);
  const uint64_t t0 = __ballot(nt & 1u), t1 = __ballot(nt & 2u), t2 = __ballot(nt & 4u);
  flags[idx] = (uint8_t)fl; // the buffers cover whole waves: the tail beyond n_points is written as 0
  cases[idx] = (uint8_t)cs;
  if ((threadIdx.x & 63) == 0) {
    const uint32_t w = idx >> 6;
    wave_v[w] = (uint64_t)(__popcll(b0) + __popcll(b1) + __popcll(b2));
    wave_t[w] = (uint64_t)__popcll(t0) + 2ull * (uint64_t)__popcll(t1) + 4ull * (uint64_t)__popcll(t2);
  }
}

// ------------------------------------------------------------------ scan (exclusive, in place, uint64)
// one block = kScanChunk consecutive elements; block_sums (optional) receives the chunk's total
__global__ __launch_bounds__(256) void mesh_scan_chunk_kernel(uint64_t* __restrict__ a, uint64_t n, uint64_t* __restrict__ block_sums) {
  __shared__ uint64_t part[256];
  const uint64_t base = (uint64_t)blockIdx.x * kScanChunk + (uint64_t)threadIdx.x * kScanPer;
  uint64_t v[kScanPer], sum = 0;
#pragma unroll
  for (int k = 0; k < kScanPer; k++) {
    v[k] = base + k < n ? a[base + k] : 0ull;
    sum += v[k];
  }
  part[threadIdx.x] = sum;
  __syncthreads();
  for (int d = 1; d < 256; d <<= 1) { // Hillis-Steele over the 256 thread totals
    const uint64_t add = threadIdx.x >= (unsigned)d ? part[threadIdx.x - d] : 0ull;
    __syncthreads();
    part[threadIdx.x] += add;
    __syncthreads();
  }
  uint64_t run = part[threadIdx.x] - sum; // exclusive prefix of this thread's run
#pragma unroll
  for (int k = 0; k < kScanPer; k++) {
    if (base + k < n) a[base + k] = run;
    run += v[k];
  }
  if (block_sums && threadIdx.x == 255) block_sums[blockIdx.x] = part[255];
}

__global__ __launch_bounds__(256) void mesh_scan_add_kernel(uint64_t* __restrict__ a, uint64_t n, const uint64_t* __restrict__ offs) {
  const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < n) a[i] += offs[i / kScanChunk];
}

// ------------------------------------------------------------------ emit
// sigma gradient at a grid point: central differences, one-sided at the border
__device__ __forceinline__ void grid_gradient(const float* __restrict__ sigma, const MeshGrid& g, const int i[3], float gr[3]) {
  const size_t stride[3] = {1, (size_t)g.res[0], (size_t)g.res[0] * (size_t)g.res[1]};
  const size_t at = (size_t)i[0] + stride[1] * (size_t)i[1] + stride[2] * (size_t)i[2];
#pragma unroll
  for (int a = 0; a < 3; a++) {
    const int ip = min(i[a] + 1, g.res[a] - 1), im = max(i[a] - 1, 0);
    const float diff = sigma[at + (size_t)(ip - i[a]) * stride[a]] - sigma[at - (size_t)(i[a] - im) * stride[a]];
    gr[a] = diff / ((float)(ip - im) * g.step[a]);
  }
}

__global__ __launch_bounds__(256) void mesh_vertices_kernel(const float* __restrict__ sigma, MeshGrid g, float thr, uint32_t n_points,
                                                            const uint8_t* __restrict__ flags, const uint64_t* __restrict__ wave_v,
                                                            float* __restrict__ xyz, float* __restrict__ nrm) {
  const uint32_t idx = blockIdx.x * 256 + threadIdx.x;
  const uint32_t fl = idx < n_points ? flags[idx] : 0u;
  const uint64_t lt = lanes_below();
  const uint64_t b0 = __ballot(fl & 1u), b1 = __ballot(fl & 2u), b2 = __ballot(fl & 4u);
  if (!fl) return;
  uint64_t v = wave_v[idx >> 6] + (uint64_t)(__popcll(b0 & lt) + __popcll(b1 & lt) + __popcll(b2 & lt));
  const uint32_t rx = (uint32_t)g.res[0], rxy = rx * (uint32_t)g.res[1];
  const int ia[3] = {(int)(idx % rx), (int)((idx % rxy) / rx), (int)(idx / rxy)};
  const size_t stride[3] = {1, rx, rxy};
  const float sa = sigma[idx];
  float ga[3];
  grid_gradient(sigma, g, ia, ga);
  for (int a = 0; a < 3; a++) {
    if (!((fl >> a) & 1u)) continue;
    int ib[3] = {ia[0], ia[1], ia[2]};
    ib[a] += 1;
    const float sb = sigma[idx + stride[a]];
    float t = (thr - sa) / (sb - sa);
    if (t != t) t = 0.5f; // an infinite or NaN end, or an overflowed difference; nothing else leaves [0, 1] on a crossing edge
    float gb[3], n[3];
    grid_gradient(sigma, g, ib, gb);
#pragma unroll
    for (int c = 0; c < 3; c++) {
      const float pa = grid_coord(g, c, ia[c]), pb = grid_coord(g, c, ib[c]);
      xyz[3 * v + c] = pa + t * (pb - pa);
      n[c] = -(ga[c] + t * (gb[c] - ga[c]));
    }
    const float n2 = (n[0] * n[0] + n[1] * n[1]) + n[2] * n[2];
    const float inv = n2 > 0.0f ? 1.0f / sqrtf(n2) : 0.0f;
    const bool finite = fabsf(n2) < __builtin_inff(); // inf or NaN (inf - inf gradients): no direction, (0, 0, 0)
#pragma unroll
    for (int c = 0; c < 3; c++) nrm[3 * v + c] = finite ? n[c] * inv : 0.0f;
    v++;
  }
}

// vertex id of the edge (point q, axis a): the wave's offset + crossing flags of the points before q in its wave + q's own
// flags below a (flags only use bits 0..2, so the popcount of a masked 8-byte word counts 8 points at once)
__device__ __forceinline__ uint32_t edge_vertex(const uint8_t* __restrict__ flags, const uint64_t* __restrict__ wave_v, uint32_t q, int a) {
  const uint64_t* w = reinterpret_cast<const uint64_t*>(flags + ((size_t)q & ~(size_t)63));
  const uint32_t within = q & 63u;
  uint32_t cnt = 0;
#pragma unroll
  for (uint32_t j = 0; j < 8; j++) {
    if (8 * j >= within) break;
    const uint64_t word = w[j];
    const uint32_t nb = within - 8 * j; // bytes of this word before q
    cnt += (uint32_t)__popcll(nb >= 8 ? word : word & ((1ull << (8 * nb)) - 1ull));
  }
  cnt += (uint32_t)__popc((uint32_t)flags[q] & ((1u << a) - 1u));
  return (uint32_t)(wave_v[q >> 6] + cnt);
}

__global__ __launch_bounds__(256) void mesh_triangles_kernel(MeshGrid g, uint32_t n_points, const uint8_t* __restrict__ flags,
                                                             const uint8_t* __restrict__ cases, const uint64_t* __restrict__ wave_v,
                                                             const uint64_t* __restrict__ wave_t, uint32_t* __restrict__ tri) {
  const uint32_t idx = blockIdx.x * 256 + threadIdx.x;
  const uint32_t cs = idx < n_points ? cases[idx] : 0u;
  const uint32_t nt = kMcTriCount[cs];
  const uint64_t lt = lanes_below();
  const uint64_t t0 = __ballot(nt & 1u), t1 = __ballot(nt & 2u), t2 = __ballot(nt & 4u);
  if (!nt) return;
  const uint64_t first = wave_t[idx >> 6] + (uint64_t)__popcll(t0 & lt) + 2ull * (uint64_t)__popcll(t1 & lt) +
                         4ull * (uint64_t)__popcll(t2 & lt);
  const uint32_t rx = (uint32_t)g.res[0], rxy = rx * (uint32_t)g.res[1];
  for (uint32_t k = 0; k < nt; k++) {
#pragma unroll
    for (int j = 0; j < 3; j++) {
      const int e = kMcTris[cs][3 * k + j];
      const int axis = e >> 2, lo = e & 1, hi = (e >> 1) & 1;
      const uint32_t ox = axis == 0 ? 0 : lo, oy = axis == 0 ? lo : axis == 1 ? 0 : hi, oz = axis == 2 ? 0 : hi;
      tri[3 * (first + k) + j] = edge_vertex(flags, wave_v, idx + ox + oy * rx + oz * rxy, axis);
    }
  }
}

// ------------------------------------------------------------------ vertex colours
// debug_field64_kernel's path: one lane = one vertex, encode_sample + mlp_forward2 on the frags64 set
template <int F, int NDENSE>
__global__ __launch_bounds__(256) void mesh_color_kernel(FieldDev fd, const float* __restrict__ xyz, const float* __restrict__ nrm,
                                                         uint64_t nv, uint8_t* __restrict__ rgb) {
  __shared__ half8 wl[kNumFrags * 64];
  for (int i = threadIdx.x; i < kNumFrags * 64; i += 256) wl[i] = fd.frags64[i];
  __syncthreads();
  const int lane = threadIdx.x & 63, r = lane & 31, grp = lane >> 5;
  const uint64_t wave = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  const uint64_t idx = wave * 64 + lane, idxA = wave * 64 + r, idxB = idxA + 32;
  if (wave * 64 >= nv) return; // wave-uniform
  const bool ok = idx < nv;
  float p[3] = {0.5f, 0.5f, 0.5f};
  if (ok)
    for (int a = 0; a < 3; a++) p[a] = xyz[idx * 3 + a];
  auto dir_of = [&](uint64_t i, float dd[3]) { // seen from outside: the view direction is -normal
    dd[0] = 0.f; dd[1] = 0.f; dd[2] = 1.f;
    if (i < nv)
      for (int a = 0; a < 3; a++) dd[a] = -nrm[i * 3 + a];
  };
  float dA[3], dB[3];
  dir_of(idxA, dA);
  dir_of(idxB, dB);
  half8 f[4];
  const HashConsts hc = {fd.hash_my_b, fd.hash_mz_b, fd.hash_m_b, (uint32_t)fd.wide_offsets};
  encode_sample<F, NDENSE>(fd.table, fd.levels, hc, p[0], p[1], p[2], f);
  swap_halves(f[0], f[1]);
  swap_halves(f[2], f[3]);
  const half8 fA[2] = {f[0], f[2]}, fB[2] = {f[1], f[3]};
  const MlpOut2 mo = mlp_forward2(wl, lane, fA, fB, sh_fragment(grp, dA[0], dA[1], dA[2]), sh_fragment(grp, dB[0], dB[1], dB[2]));
  if (!ok) return;
  const float bg[4] = {0.0f, 0.0f, 0.0f, 0.0f};
  const uint32_t q = quantize_rgba8(fast_sigmoid(grp ? mo.rgbB[8] : mo.rgbA[0]), fast_sigmoid(grp ? mo.rgbB[9] : mo.rgbA[1]),
                                    fast_sigmoid(grp ? mo.rgbB[10] : mo.rgbA[2]), 1.0f, bg); // an opaque pixel of that colour
  rgb[idx * 3 + 0] = (uint8_t)(q & 255u);
  rgb[idx * 3 + 1] = (uint8_t)((q >> 8) & 255u);
  rgb[idx * 3 + 2] = (uint8_t)((q >> 16) & 255u);
}

} // namespace

size_t mesh_scan_scratch(size_t n) {
  size_t total = 0;
  while (n > (size_t)kScanChunk) {
    n = (n + kScanChunk - 1) / kScanChunk;
    total += n;
  }
  return total + 1;
}

hipError_t launch_mesh_density(const FieldDev& fd, const MeshGrid& g, int use_occ, int brick, float* sigma, hipStream_t s) {
  const uint32_t waves = brick ? (uint32_t)(((g.res[0] + 3) / 4) * ((g.res[1] + 3) / 4) * ((g.res[2] + 3) / 4)) : (uint32_t)mesh_waves(g);
  const unsigned blocks = (waves + 3) / 4;
  with_field_instance(fd, [&](auto f, auto nd) {
    hipLaunchKernelGGL((mesh_density_kernel<decltype(f)::value, decltype(nd)::value>), dim3(blocks), dim3(256), 0, s, fd, g, use_occ, brick, waves, sigma);
  });
  return hipGetLastError();
}

hipError_t launch_mesh_kept(const uint8_t* valid, const MeshGrid& g, uint8_t* kept, hipStream_t s) {
  const size_t waves = mesh_waves(g); // a multiple of 4: every thread of the launch has its byte of kept
  hipLaunchKernelGGL(mesh_kept_kernel, dim3((unsigned)(waves / 4)), dim3(256), 0, s, valid, g, (uint32_t)mesh_points(g), kept);
  return hipGetLastError();
}

hipError_t launch_mesh_classify(const float* sigma, const MeshGrid& g, float thr, const uint8_t* kept, uint8_t* flags, uint8_t* cases,
                                uint64_t* wave_v, uint64_t* wave_t, hipStream_t s) {
  const size_t waves = mesh_waves(g); // a multiple of 4: every thread of the launch has its byte of flags / cases
  hipLaunchKernelGGL(mesh_classify_kernel, dim3((unsigned)(waves / 4)), dim3(256), 0, s, sigma, g, thr, (uint32_t)mesh_points(g),
                     kept, flags, cases, wave_v, wave_t);
  return hipGetLastError();
}

hipError_t launch_mesh_scan(uint64_t* a, size_t n, uint64_t* scratch, uint64_t* total, hipStream_t s) {
  if (n <= (size_t)kScanChunk) {
    hipLaunchKernelGGL(mesh_scan_chunk_kernel, dim3(1), dim3(256), 0, s, a, (uint64_t)n, total);
    return hipGetLastError();
  }
  const size_t nb = (n + kScanChunk - 1) / kScanChunk;
  hipLaunchKernelGGL(mesh_scan_chunk_kernel, dim3((unsigned)nb), dim3(256), 0, s, a, (uint64_t)n, scratch);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  if ((e = launch_mesh_scan(scratch, nb, scratch + nb, total, s)) != hipSuccess) return e;
  hipLaunchKernelGGL(mesh_scan_add_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, a, (uint64_t)n, (const uint64_t*)scratch);
  return hipGetLastError();
}

hipError_t launch_mesh_vertices(const float* sigma, const MeshGrid& g, float thr, const uint8_t* flags, const uint64_t* wave_v,
                                float* xyz, float* nrm, hipStream_t s) {
  const size_t waves = mesh_waves(g);
  hipLaunchKernelGGL(mesh_vertices_kernel, dim3((unsigned)((waves + 3) / 4)), dim3(256), 0, s, sigma, g, thr, (uint32_t)mesh_points(g),
                     flags, wave_v, xyz, nrm);
  return hipGetLastError();
}

hipError_t launch_mesh_triangles(const MeshGrid& g, const uint8_t* flags, const uint8_t* cases, const uint64_t* wave_v,
                                 const uint64_t* wave_t, uint32_t* tri, hipStream_t s) {
  const size_t waves = mesh_waves(g);
  hipLaunchKernelGGL(mesh_triangles_kernel, dim3((unsigned)((waves + 3) / 4)), dim3(256), 0, s, g, (uint32_t)mesh_points(g), flags,
                     cases, wave_v, wave_t, tri);
  return hipGetLastError();
}

hipError_t launch_mesh_colors(const FieldDev& fd, const float* xyz, const float* nrm, uint64_t nv, uint8_t* rgb, hipStream_t s) {
  if (nv == 0) return hipSuccess;
  const unsigned blocks = (unsigned)((nv + 255) / 256);
  with_field_instance(fd, [&](auto f, auto nd) {
    hipLaunchKernelGGL((mesh_color_kernel<decltype(f)::value, decltype(nd)::value>), dim3(blocks), dim3(256), 0, s, fd, xyz, nrm, nv, rgb);
  });
  return hipGetLastError();
}

} // namespace prv
