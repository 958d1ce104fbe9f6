// prv_tsdf.hip -- depth-map fusion into a truncated signed distance volume (prv_tsdf_*; the arithmetic contract is written out in
// include/prv.h).  The grid is prv_marching_cubes_grid's, x fastest; a point's state is D, W, WC, C[3] in planes of n floats.
//
//  tsdf_integrate_kernel : one lane = one grid point, so the 64 points of a wave lie along x and project to neighbouring pixels.
//       The loop over the launch's views runs inside the kernel with the state in registers: each state word is read once and
//       written once per launch, not once per view.  The views' cameras are kernel arguments (TsdfLaunch, wave-uniform: the
//       compiler keeps them in scalar registers), so a view costs the lane its projection, one 4-byte gather of the depth pixel
//       and, where asked for, one of the weight and one of the colour pixel.  Views past kTsdfChunk go to further launches.
//  tsdf_info_kernel      : per wave the ballots of three predicates, three 64-bit integer atomic adds by lane 0.
//  tsdf_grid_kernel      : the volume as a sigma-like grid (-D, NaN where unobserved) and its validity mask.
//  tsdf_colors_kernel    : one lane per mesh vertex, the colour of its nearest grid point.
//
// No LDS, no float atomics, no workgroup waits for another: every point is owned by one lane.  All device writes are ordinary
// vector stores (and the three integer atomics of the info kernel) in plain C++.
#include "prv_tsdf.hpp"

#include <algorithm>

namespace prv {

namespace {

__global__ __launch_bounds__(256) void tsdf_integrate_kernel(const TsdfLaunch a, const MeshGrid g, const int colors, const uint32_t n_points,
                                                             float* __restrict__ state, const float* __restrict__ depth,
                                                             const float* __restrict__ weight, const uint32_t* __restrict__ rgba) {
  const uint32_t idx = blockIdx.x * 256 + threadIdx.x;
  if (idx >= n_points) return;
  const size_t n = n_points;
  const uint32_t rx = (uint32_t)g.res[0], rxy = rx * (uint32_t)g.res[1];
  const float e[3] = {g.lo[0] + (float)(idx % rx) * g.step[0], g.lo[1] + (float)((idx % rxy) / rx) * g.step[1],
                      g.lo[2] + (float)(idx / rxy) * g.step[2]};
  float D = state[idx], W = state[n + idx];
  float WC = 0.0f, C[3] = {0.0f, 0.0f, 0.0f};
  const bool paint = colors && rgba; // uniform
  if (paint) {
    WC = state[2 * n + idx];
#pragma unroll
    for (int k = 0; k < 3; k++) C[k] = state[(size_t)(3 + k) * n + idx];
  }
  const float fw = (float)a.width, fh = (float)a.height;
  for (int j = 0; j < a.n_views; j++) {
    const TsdfView& tv = a.view[j];
    CamDev cam; // (the cull rectangle is not read)
#pragma unroll
    for (int k = 0; k < 12; k++) cam.c2w[k] = tv.c2w[k];
    cam.fx = tv.fx, cam.fy = tv.fy, cam.cx = tv.cx, cam.cy = tv.cy;
#pragma unroll
    for (int k = 0; k < 4; k++) cam.lens[k] = tv.lens[k];
    float u, v, z;
    if (!project_engine_point(cam, e, u, v, z) || !(z < __builtin_inff())) continue;
    const float fu = floorf(u), fv = floorf(v);
    if (!(fu >= 0.0f && fu < fw && fv >= 0.0f && fv < fh)) continue; // (a NaN fails; the conversions below see [0, size) only)
    const size_t pix = (size_t)tv.base + (size_t)(int)fv * (size_t)a.width + (size_t)(int)fu;
    const float d = depth[pix];
    const float ws = weight ? weight[pix] : 1.0f;
    if (!(d > 0.0f && d < __builtin_inff() && ws > 0.0f && ws < __builtin_inff())) continue;
    const float sdf = d - z;
    if (sdf < -a.trunc) continue; // behind what this view sees
    const float s = fminf(sdf * a.inv, 1.0f);
    const float Wn = W + ws;
    D = fmaf(D, W, s * ws) / Wn;
    W = Wn;
    if (paint && sdf <= a.trunc) {
      const uint32_t px = rgba[pix]; // r, g, b, a from the low byte up; alpha is not used
      const float WCn = WC + ws;
#pragma unroll
      for (int k = 0; k < 3; k++) C[k] = fmaf(C[k], WC, (float)((px >> (8 * k)) & 255u) * ws) / WCn;
      WC = WCn;
    }
  }
  state[idx] = D;
  state[n + idx] = W;
  if (paint) {
    state[2 * n + idx] = WC;
#pragma unroll
    for (int k = 0; k < 3; k++) state[(size_t)(3 + k) * n + idx] = C[k];
  }
}

__global__ __launch_bounds__(256) void tsdf_info_kernel(const float* __restrict__ state, size_t n, unsigned long long* __restrict__ counts) {
  unsigned long long acc[3] = {0ull, 0ull, 0ull};
  const size_t rounds = (n + (size_t)gridDim.x * 256 - 1) / ((size_t)gridDim.x * 256); // every lane of a wave takes every round: ballots
  for (size_t r = 0; r < rounds; r++) {
    const size_t i = (r * gridDim.x + blockIdx.x) * 256 + threadIdx.x;
    bool obs = false, in = false, band = false;
    if (i < n) {
      const float D = state[i], W = state[n + i];
      obs = W > 0.0f;
      in = obs && D < 0.0f;
      band = obs && fabsf(D) < 1.0f;
    }
    acc[0] += (unsigned long long)__popcll(__ballot(obs));
    acc[1] += (unsigned long long)__popcll(__ballot(in));
    acc[2] += (unsigned long long)__popcll(__ballot(band));
  }
  if ((threadIdx.x & 63) == 0)
    for (int k = 0; k < 3; k++)
      if (acc[k]) atomicAdd(counts + k, acc[k]);
}

__global__ __launch_bounds__(256) void tsdf_grid_kernel(const float* __restrict__ state, size_t n, float min_weight, float* __restrict__ grid,
                                                        uint8_t* __restrict__ valid) {
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) {
    const float W = state[n + i];
    const bool ok = W > 0.0f && W >= min_weight;
    if (grid) grid[i] = ok ? -state[i] : __builtin_nanf("");
    if (valid) valid[i] = ok ? 1 : 0;
  }
}

__global__ __launch_bounds__(256) void tsdf_colors_kernel(const float* __restrict__ state, MeshGrid g, const float* __restrict__ xyz, uint64_t nv,
                                                          uint8_t* __restrict__ rgb) {
  const uint64_t v = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (v >= nv) return;
  size_t at = 0, stride = 1;
#pragma unroll
  for (int a = 0; a < 3; a++) {
    const float q = rintf((xyz[3 * v + a] - g.lo[a]) / g.step[a]); // (a vertex lies on its grid edge: q is in [0, res - 1])
    const int i = min(max((int)q, 0), g.res[a] - 1);
    at += (size_t)i * stride;
    stride *= (size_t)g.res[a];
  }
  const size_t n = stride;
  const bool has = state[2 * n + at] > 0.0f;
#pragma unroll
  for (int k = 0; k < 3; k++) rgb[3 * v + k] = has ? (uint8_t)fminf(255.0f, floorf(state[(size_t)(3 + k) * n + at] + 0.5f)) : (uint8_t)0;
}

unsigned stride_blocks(size_t items, size_t most) { return (unsigned)std::max<size_t>(1, std::min<size_t>(most, (items + 255) / 256)); }

} // namespace

hipError_t launch_tsdf_integrate(const TsdfLaunch& a, const MeshGrid& g, bool colors, float* state, const float* depth, const float* weight,
                                 const uint32_t* rgba, hipStream_t s) {
  if (a.n_views <= 0) return hipSuccess;
  const size_t n = mesh_points(g);
  hipLaunchKernelGGL(tsdf_integrate_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, a, g, colors ? 1 : 0, (uint32_t)n, state, depth,
                     weight, rgba);
  return hipGetLastError();
}

hipError_t launch_tsdf_info(const float* state, size_t n, unsigned long long* counts, hipStream_t s) {
  hipLaunchKernelGGL(tsdf_info_kernel, dim3(stride_blocks(n, 2048)), dim3(256), 0, s, state, n, counts);
  return hipGetLastError();
}

hipError_t launch_tsdf_grid(const float* state, size_t n, float min_weight, float* grid, uint8_t* valid, hipStream_t s) {
  hipLaunchKernelGGL(tsdf_grid_kernel, dim3(stride_blocks(n, 4096)), dim3(256), 0, s, state, n, min_weight, grid, valid);
  return hipGetLastError();
}

hipError_t launch_tsdf_colors(const float* state, const MeshGrid& g, const float* xyz, uint64_t nv, uint8_t* rgb, hipStream_t s) {
  if (nv == 0) return hipSuccess;
  hipLaunchKernelGGL(tsdf_colors_kernel, dim3((unsigned)((nv + 255) / 256)), dim3(256), 0, s, state, g, xyz, nv, rgb);
  return hipGetLastError();
}

} // namespace prv
