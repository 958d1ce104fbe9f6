// prv_raster.hip -- a triangle rasteriser for depth: the nearest surface depth of a mesh per pixel and view (prv_mesh_depth) and
// the depth buffer that occludes the points of prv_coverage_create_occluded.  The arithmetic contract is written out in
// include/prv.h; everything after the projection is integer until the depth itself, which is float64.
//
//  raster_small_kernel : one lane = one triangle of one view (grid: ceil(chunk / 256) x views, as the coverage kernels have it).
//       The lane projects the three vertices, snaps them to 1/256 pixel, orients the triangle and clips the pixel box of the
//       snapped vertices to the image.  A box of at most small_max pixels it walks itself: atomicMin of the bits of the depth at
//       every inside pixel centre.  A larger box goes to a list: the wave's __ballot, a popcount prefix and ONE returning atomic add
//       per wave, as the march appends its records.  No lane leaves before the ballot.
//  raster_large_kernel : one workgroup per list entry (block-stride beyond kRasterLargeBlocks), its 256 lanes one 16 x 16 tile of
//       the clipped box at a time; a tile is skipped when an edge function is negative at the tile corner most favourable to it
//       (exact, in integers; block-uniform).  The same raster_pixel as the small path.
//  Both are templates over the buffer's key: uint32_t is the depth buffer above; unsigned long long is the visibility buffer of
//       prv_mesh_render, key = bits of the depth << 32 | triangle id: the nearest depth wins, among equal depth bits the lowest id.
//  raster_visible_kernel : coverage_visible_kernel's twin for a mesh's buffer: an empty pixel passes (nothing stands in front).
//  raster_shade_kernel : one lane per pixel of one view reads the key, runs raster_setup again for the triangle it names and
//       interpolates the vertex colours perspective-correctly in float64 ("mesh colour images" in include/prv.h); RGBA8, and
//       optionally the depth and the triangle id, unflipped.  No atomics.
//
// The buffer takes a minimum, so the chunking, the view batches, small_max and which path a triangle took change no byte.
// No LDS, no MFMA, no workgroup waits for another, nothing spins.  All device writes are vector stores or atomics in plain C++.
#include "prv_raster.hpp"

#include <algorithm>

namespace prv {

struct RasterTri {
  long long xa, ya, xb, yb, xc, yc; // snapped vertices, 1/256 pixel; oriented: E_ab(c) = a2 > 0
  long long a2;
  double ia, ib, ic;  // 1 / depth of a, b, c
  int x0, y0, x1, y1; // the clipped pixel box, inclusive (empty: x1 < x0 or y1 < y0)
  bool exchanged;     // b and c were exchanged (the shading exchanges their colours with them)
};

// E_pq(P) = (Xq - Xp)(Py - Yp) - (Yq - Yp)(Px - Xp): every factor is below 2^25, the result below 2^49
__device__ __forceinline__ long long raster_edge(long long xp, long long yp, long long xq, long long yq, long long px, long long py) {
  return (xq - xp) * (py - yp) - (yq - yp) * (px - xp);
}

__device__ __forceinline__ bool raster_vertex(const CamDev& cam, const float* __restrict__ xyz, uint32_t id, long long& X, long long& Y, double& inv) {
  const float e[3] = {xyz[3 * (size_t)id], xyz[3 * (size_t)id + 1], xyz[3 * (size_t)id + 2]};
  float u, v, z;
  if (!project_engine_point(cam, e, u, v, z)) return false;
  if (!(z < __builtin_inff()) || !(fabsf(u) < 32768.0f) || !(fabsf(v) < 32768.0f)) return false; // (a NaN fails)
  X = (long long)rintf(u * 256.0f);
  Y = (long long)rintf(v * 256.0f);
  inv = 1.0 / (double)z;
  return true;
}

// false: the triangle writes nothing in this view (a vertex fails, no area, or its box misses the image)
__device__ __forceinline__ bool raster_setup(const CamDev& cam, const float* __restrict__ xyz, const uint32_t* __restrict__ tri, size_t t, int W, int H,
                                             RasterTri& s) {
  if (!raster_vertex(cam, xyz, tri[3 * t], s.xa, s.ya, s.ia) || !raster_vertex(cam, xyz, tri[3 * t + 1], s.xb, s.yb, s.ib) ||
      !raster_vertex(cam, xyz, tri[3 * t + 2], s.xc, s.yc, s.ic))
    return false;
  s.a2 = raster_edge(s.xa, s.ya, s.xb, s.yb, s.xc, s.yc);
  if (s.a2 == 0) return false;
  s.exchanged = s.a2 < 0;
  if (s.a2 < 0) { // b <-> c: both windings are rasterised
    const long long x = s.xb, y = s.yb;
    const double i = s.ib;
    s.xb = s.xc, s.yb = s.yc, s.ib = s.ic;
    s.xc = x, s.yc = y, s.ic = i;
    s.a2 = -s.a2;
  }
  // pixel x has its centre at 256 x + 128: the centres within [min X, max X] are x = ceil((min - 128) / 256) .. floor((max - 128) / 256)
  const long long lox = min(s.xa, min(s.xb, s.xc)), hix = max(s.xa, max(s.xb, s.xc));
  const long long loy = min(s.ya, min(s.yb, s.yc)), hiy = max(s.ya, max(s.yb, s.yc));
  s.x0 = (int)max((lox + 127) >> 8, 0ll);
  s.x1 = (int)min((hix - 128) >> 8, (long long)W - 1);
  s.y0 = (int)max((loy + 127) >> 8, 0ll);
  s.y1 = (int)min((hiy - 128) >> 8, (long long)H - 1);
  return s.x1 >= s.x0 && s.y1 >= s.y0;
}

// what a pixel's minimum is taken over: the bits of the depth (uint32), or those bits above the triangle's id (uint64)
__device__ __forceinline__ void raster_key(uint32_t& key, uint32_t zbits, uint32_t) { key = zbits; }
__device__ __forceinline__ void raster_key(unsigned long long& key, uint32_t zbits, uint32_t id) { key = ((unsigned long long)zbits << 32) | id; }

// the one per-pixel function of both paths: x in [0, W), y in [0, H) (the callers walk the clipped box only)
template <typename Key>
__device__ __forceinline__ void raster_pixel(const RasterTri& s, int x, int y, Key* __restrict__ zb, int W, uint32_t id) {
  const long long px = 256ll * x + 128, py = 256ll * y + 128;
  const long long wa = raster_edge(s.xb, s.yb, s.xc, s.yc, px, py);
  const long long wb = raster_edge(s.xc, s.yc, s.xa, s.ya, px, py);
  const long long wc = raster_edge(s.xa, s.ya, s.xb, s.yb, px, py);
  if ((wa | wb | wc) < 0) return; // inclusive: on an edge is inside
  const double iz = ((double)wa * s.ia + (double)wb * s.ib) + (double)wc * s.ic; // > 0: wa + wb + wc = a2 > 0
  const float z = (float)((double)s.a2 / iz);
  Key key;
  raster_key(key, __float_as_uint(z), id);
  atomicMin(zb + (size_t)y * W + x, key);
}

// Key = uint32_t: the depth buffer (the kernels of prv_mesh_depth and the occluder, as they were); unsigned long long: the
// visibility buffer
template <typename Key>
__global__ __launch_bounds__(256) void raster_small_kernel(const float* __restrict__ xyz, const uint32_t* __restrict__ tri, size_t t0, size_t n,
                                                           const CamDev* __restrict__ cams, int W, int H, int small_max,
                                                           RasterPair* __restrict__ list, uint32_t capacity, uint32_t* __restrict__ count,
                                                           Key* __restrict__ zbuf) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  bool defer = false; // (no lane leaves before the ballot)
  if (i < n) {
    const CamDev cam = cams[blockIdx.y];
    RasterTri s;
    if (raster_setup(cam, xyz, tri, t0 + i, W, H, s)) {
      const long long pixels = (long long)(s.x1 - s.x0 + 1) * (long long)(s.y1 - s.y0 + 1);
      if (pixels <= (long long)small_max) {
        Key* zb = zbuf + (size_t)blockIdx.y * W * H;
        for (int y = s.y0; y <= s.y1; y++)
          for (int x = s.x0; x <= s.x1; x++) raster_pixel(s, x, y, zb, W, (uint32_t)(t0 + i));
      } else {
        defer = true;
      }
    }
  }
  const unsigned long long b = __ballot(defer);
  if (b == 0ull) return; // wave-uniform
  const int lane = threadIdx.x & 63;
  const int leader = (int)__builtin_ctzll(b);
  uint32_t base = 0;
  if (lane == leader) base = atomicAdd(count, (uint32_t)__popcll(b));
  base = __shfl(base, leader);
  if (defer) {
    const uint32_t slot = base + (uint32_t)__popcll(b & ((1ull << lane) - 1ull));
    if (slot < capacity) { // (always: at most one entry per lane of the launch, and the launch holds at most `capacity` lanes' worth)
      RasterPair p;
      p.view = blockIdx.y;
      p.tri = (uint32_t)(t0 + i);
      list[slot] = p;
    }
  }
}

template <typename Key>
__global__ __launch_bounds__(256) void raster_large_kernel(const float* __restrict__ xyz, const uint32_t* __restrict__ tri,
                                                           const CamDev* __restrict__ cams, int W, int H, const RasterPair* __restrict__ list,
                                                           uint32_t capacity, const uint32_t* __restrict__ count,
                                                           unsigned long long* __restrict__ large_total, Key* __restrict__ zbuf) {
  const uint32_t entries = min(*count, capacity);
  if (blockIdx.x == 0 && threadIdx.x == 0 && entries != 0u) atomicAdd(large_total, (unsigned long long)entries);
  const int lx = threadIdx.x & 15, ly = threadIdx.x >> 4;
  for (uint32_t e = blockIdx.x; e < entries; e += gridDim.x) { // block-uniform
    const RasterPair p = list[e];
    const CamDev cam = cams[p.view];
    RasterTri s;
    if (!raster_setup(cam, xyz, tri, (size_t)p.tri, W, H, s)) continue; // (never: the small kernel's own setup put it here)
    Key* zb = zbuf + (size_t)p.view * W * H;
    for (int ty = s.y0; ty <= s.y1; ty += 16)
      for (int tx = s.x0; tx <= s.x1; tx += 16) {
        const int ux = min(tx + 15, s.x1), uy = min(ty + 15, s.y1);
        // the pixel centres of the tile span [plx, phx] x [ply, phy]; an edge function is linear: its largest value over the tile
        // sits at the corner picked by the signs of its two coefficients
        const long long plx = 256ll * tx + 128, phx = 256ll * ux + 128, ply = 256ll * ty + 128, phy = 256ll * uy + 128;
        const long long ma = raster_edge(s.xb, s.yb, s.xc, s.yc, s.yc - s.yb >= 0 ? plx : phx, s.xc - s.xb >= 0 ? phy : ply);
        const long long mb = raster_edge(s.xc, s.yc, s.xa, s.ya, s.ya - s.yc >= 0 ? plx : phx, s.xa - s.xc >= 0 ? phy : ply);
        const long long mc = raster_edge(s.xa, s.ya, s.xb, s.yb, s.yb - s.ya >= 0 ? plx : phx, s.xb - s.xa >= 0 ? phy : ply);
        if ((ma | mb | mc) < 0) continue;
        const int x = tx + lx, y = ty + ly;
        if (x <= s.x1 && y <= s.y1) raster_pixel(s, x, y, zb, W, p.tri);
      }
  }
}

// stage B of prv_mesh_render: one lane = one pixel of one view (grid: ceil(W H / 256) x views)
__global__ __launch_bounds__(256) void raster_shade_kernel(const float* __restrict__ xyz, const uint32_t* __restrict__ tri,
                                                           const uint8_t* __restrict__ rgb, const CamDev* __restrict__ cams, int W, int H,
                                                           const unsigned long long* __restrict__ keys, int flip180, uint32_t* __restrict__ rgba,
                                                           float* __restrict__ depth, uint32_t* __restrict__ tri_out) {
  const size_t npix = (size_t)W * H;
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= npix) return;
  const unsigned long long key = keys[(size_t)blockIdx.y * npix + i];
  const uint32_t zbits = (uint32_t)(key >> 32);
  const int x = (int)(i % W), y = (int)(i / W);
  uint32_t px = 0x00ffffffu, id = 0xffffffffu; // white, alpha 0
  float d = 0.0f;
  if (zbits != 0xffffffffu) {
    id = (uint32_t)key;
    d = __uint_as_float(zbits);
    const CamDev cam = cams[blockIdx.y];
    RasterTri s;
    if (raster_setup(cam, xyz, tri, (size_t)id, W, H, s)) { // (always: stage A's own setup wrote the key)
      const long long cx = 256ll * x + 128, cy = 256ll * y + 128;
      const long long wa = raster_edge(s.xb, s.yb, s.xc, s.yc, cx, cy);
      const long long wb = raster_edge(s.xc, s.yc, s.xa, s.ya, cx, cy);
      const long long wc = raster_edge(s.xa, s.ya, s.xb, s.yb, cx, cy);
      const double pa = (double)wa * s.ia, pb = (double)wb * s.ib, pc = (double)wc * s.ic;
      const double iz = (pa + pb) + pc; // the depth's own iz
      const uint8_t* ca = rgb + 3 * (size_t)tri[3 * (size_t)id];
      const uint8_t* cb = rgb + 3 * (size_t)tri[3 * (size_t)id + (s.exchanged ? 2 : 1)];
      const uint8_t* cc = rgb + 3 * (size_t)tri[3 * (size_t)id + (s.exchanged ? 1 : 2)];
      px = 0u;
      for (int k = 0; k < 3; k++) {
        const double c = ((pa * (double)ca[k] + pb * (double)cb[k]) + pc * (double)cc[k]) / iz;
        px |= (uint32_t)fmin(255.0, floor(c + 0.5)) << (8 * k);
      }
      if (px != 0x00ffffffu) px |= 0xff000000u; // convertToAlpha: an exactly-white pixel is transparent
    }
  }
  const size_t o = flip180 ? ((size_t)(H - 1 - y) * W + (size_t)(W - 1 - x)) : i;
  rgba[(size_t)blockIdx.y * npix + o] = px;
  if (depth) depth[(size_t)blockIdx.y * npix + i] = d;
  if (tri_out) tri_out[(size_t)blockIdx.y * npix + i] = id;
}

__global__ __launch_bounds__(256) void raster_visible_kernel(const float* __restrict__ xyz, size_t n, const CamDev* __restrict__ cams, int W, int H,
                                                             const uint32_t* __restrict__ zbuf, float tol1, unsigned long long* __restrict__ bits,
                                                             size_t words) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  bool visible = false; // (no lane leaves before the ballot)
  if (i < n) {
    const CamDev cam = cams[blockIdx.y];
    const float e[3] = {xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2]};
    float u, v, z;
    if (project_engine_point(cam, e, u, v, z) && z < __builtin_inff()) { // (z is a number from here on)
      const float fu = floorf(u), fv = floorf(v);
      if (fu >= 0.0f && fu < (float)W && fv >= 0.0f && fv < (float)H) { // (a NaN fails)
        const uint32_t key = zbuf[(size_t)blockIdx.y * W * H + (size_t)(int)fv * W + (size_t)(int)fu];
        visible = key == kCoverageEmpty || z <= __uint_as_float(key) * tol1; // an empty pixel passes, a NaN z would fail
      }
    }
  }
  const unsigned long long word = __ballot(visible);
  const size_t w = (size_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if ((threadIdx.x & 63) == 0 && w < words) bits[(size_t)blockIdx.y * words + w] = word;
}

template <typename Key>
hipError_t launch_raster(const float* xyz, const uint32_t* tri, size_t t0, size_t n, const CamDev* cams, int n_views, int W, int H,
                         int small_max, RasterPair* list, size_t capacity, uint32_t* count, unsigned long long* large_total, Key* zbuf,
                         hipStream_t s) {
  if (n == 0 || n_views <= 0) return hipSuccess;
  if (n_views > kCoverageMaxBatch || capacity > kRasterListEntriesMost || n > capacity / (size_t)n_views) return hipErrorInvalidValue;
  hipError_t e = hipMemsetAsync(count, 0, 4, s);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(raster_small_kernel<Key>, dim3((unsigned)((n + 255) / 256), (unsigned)n_views), dim3(256), 0, s, xyz, tri, t0, n, cams, W, H,
                     small_max, list, (uint32_t)capacity, count, zbuf);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  const unsigned blocks = (unsigned)std::min<size_t>(kRasterLargeBlocks, n * (size_t)n_views);
  hipLaunchKernelGGL(raster_large_kernel<Key>, dim3(blocks), dim3(256), 0, s, xyz, tri, cams, W, H, list, (uint32_t)capacity, count, large_total,
                     zbuf);
  return hipGetLastError();
}
template hipError_t launch_raster<uint32_t>(const float*, const uint32_t*, size_t, size_t, const CamDev*, int, int, int, int, RasterPair*, size_t,
                                            uint32_t*, unsigned long long*, uint32_t*, hipStream_t);
template hipError_t launch_raster<unsigned long long>(const float*, const uint32_t*, size_t, size_t, const CamDev*, int, int, int, int, RasterPair*,
                                                      size_t, uint32_t*, unsigned long long*, unsigned long long*, hipStream_t);

hipError_t launch_raster_shade(const float* xyz, const uint32_t* tri, const uint8_t* rgb, const CamDev* cams, int n_views, int W, int H,
                               const unsigned long long* keys, int flip180, uint32_t* rgba, float* depth, uint32_t* tri_out, hipStream_t s) {
  if (n_views <= 0) return hipSuccess;
  hipLaunchKernelGGL(raster_shade_kernel, dim3((unsigned)(((size_t)W * H + 255) / 256), (unsigned)n_views), dim3(256), 0, s, xyz, tri, rgb, cams,
                     W, H, keys, flip180, rgba, depth, tri_out);
  return hipGetLastError();
}

hipError_t launch_raster_visible(const float* xyz, size_t n, const CamDev* cams, int n_batch, int W, int H, const uint32_t* zbuf, float tol1,
                                 unsigned long long* bits, size_t words, hipStream_t s) {
  if (n_batch <= 0 || n == 0) return hipSuccess;
  hipLaunchKernelGGL(raster_visible_kernel, dim3((unsigned)((n + 255) / 256), (unsigned)n_batch), dim3(256), 0, s, xyz, n, cams, W, H, zbuf, tol1,
                     bits, words);
  return hipGetLastError();
}

} // namespace prv
