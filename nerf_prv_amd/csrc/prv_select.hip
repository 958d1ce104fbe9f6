// prv_select.hip -- several next views per round: the greedy, redundancy-aware choice among the candidates of a scoring round
// (prv_select_from_images / prv_select_views; the arithmetic contract is written out in include/prv.h).
//
//  select_footprint_kernel : one lane per pixel: the gain word q = floor(H * 2^16) and the voxel of the point the ray's expected
//       depth names (0xFFFFFFFF: no point).  Every float operation is its own IEEE rounding (-ffp-contract=off; the multiply and
//       the add of o + t d are written as such), so a float32 restatement on the CPU gives the same words.
//  select_gain_kernel      : all remaining views in one launch (blockIdx.y = view): per lane an exact uint64 sum of q over the
//       pixels whose voxel is not yet covered, reduced within the wave by shuffles, ONE 64-bit integer atomic add per wave into
//       the view's sum.  Integer adds commute: the sums do not depend on the order.  The covered set C (G^3 bits, <= 2 MiB) is
//       read through the cache.
//  select_mark_kernel      : atomicOr of the chosen view's voxels into C.
//
// All device writes are ordinary vector stores or atomics in plain C++.
#include "prv_select.hpp"

#include <algorithm>

namespace prv {

__global__ __launch_bounds__(256) void select_footprint_kernel(SelectFootprintParams P) {
  const size_t npix = (size_t)P.W * (size_t)P.H;
  const size_t p = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (p >= npix) return;
  const int v = blockIdx.y;
  const size_t i = (size_t)v * npix + p;
  const float H = P.entropy[i], a = P.alpha[i], z = P.depth[i];
  // gain: NaN and negative H give 0; the largest float below 2^32 caps the conversion
  uint32_t q = 0u;
  if (H > 0.0f) q = (uint32_t)fminf(floorf(H * 65536.0f), 4294967040.0f);
  uint32_t voxel = kSelectUnlocated;
  if (a >= P.alpha_min && z > 0.0f) {
    const CamDev& cam = P.cams[v];
    const int py = (int)(p / (size_t)P.W), px = (int)(p - (size_t)py * (size_t)P.W);
    float ox, oy, o[3], d[3];
    spp_offset(0, ox, oy);
    raygen(cam, px, py, ox, oy, o, d);
    // the forward cosine, as render_queue64_body (kRenderDepth) forms it
    const float fx = cam.c2w[2], fy = cam.c2w[6], fz = cam.c2w[10];
    const float inv = 1.0f / sqrtf(fmaf(fx, fx, fmaf(fy, fy, fz * fz)));
    const float c = fmaf(d[0], fx, fmaf(d[1], fy, d[2] * fz)) * inv;
    const float t = (z / a) / c;
    const float fG = (float)P.G;
    float g[3];
    bool inside = true;
#pragma unroll
    for (int k = 0; k < 3; k++) {
      const float pa = __fadd_rn(o[k], __fmul_rn(t, d[k])); // a multiply and an add, no FMA
      g[k] = floorf(pa * fG);
      inside = inside && g[k] >= 0.0f && g[k] < fG; // (a NaN fails both)
    }
    if (inside) voxel = (uint32_t)(int)g[0] + (uint32_t)P.G * ((uint32_t)(int)g[1] + (uint32_t)P.G * (uint32_t)(int)g[2]);
  }
  P.voxel[i] = voxel;
  P.q[i] = q;
}

__global__ __launch_bounds__(256) void select_gain_kernel(const uint32_t* __restrict__ voxel, const uint32_t* __restrict__ q, size_t npix,
                                                          const uint32_t* __restrict__ bits, const uint32_t* __restrict__ done,
                                                          unsigned long long* __restrict__ sums) {
  const int v = blockIdx.y;
  if (done[v]) return; // block-uniform
  const uint32_t* vv = voxel + (size_t)v * npix;
  const uint32_t* qv = q + (size_t)v * npix;
  unsigned long long acc = 0ull;
  for (size_t p = (size_t)blockIdx.x * 256 + threadIdx.x; p < npix; p += (size_t)gridDim.x * 256) {
    const uint32_t vox = vv[p];
    bool fresh = true;
    if (vox != kSelectUnlocated) fresh = !((bits[vox >> 5] >> (vox & 31u)) & 1u);
    if (fresh) acc += (unsigned long long)qv[p];
  }
  uint32_t lo = (uint32_t)acc, hi = (uint32_t)(acc >> 32);
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const uint32_t lo2 = (uint32_t)__shfl_down((int)lo, off), hi2 = (uint32_t)__shfl_down((int)hi, off);
    const unsigned long long s = (((unsigned long long)hi << 32) | lo) + (((unsigned long long)hi2 << 32) | lo2);
    lo = (uint32_t)s;
    hi = (uint32_t)(s >> 32);
  }
  const unsigned long long tot = ((unsigned long long)hi << 32) | lo;
  if ((threadIdx.x & 63) == 0 && tot != 0ull) atomicAdd(sums + v, tot);
}

__global__ __launch_bounds__(256) void select_mark_kernel(const uint32_t* __restrict__ voxel, size_t npix, uint32_t* __restrict__ bits,
                                                          uint32_t* __restrict__ done_flag) {
  for (size_t p = (size_t)blockIdx.x * 256 + threadIdx.x; p < npix; p += (size_t)gridDim.x * 256) {
    const uint32_t vox = voxel[p];
    if (vox != kSelectUnlocated) atomicOr(bits + (vox >> 5), 1u << (vox & 31u));
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) *done_flag = 1u;
}

hipError_t launch_select_footprint(const SelectFootprintParams& P, hipStream_t s) {
  const size_t npix = (size_t)P.W * (size_t)P.H;
  if (npix == 0 || P.n_views == 0) return hipSuccess;
  hipLaunchKernelGGL(select_footprint_kernel, dim3((unsigned)((npix + 255) / 256), (unsigned)P.n_views), dim3(256), 0, s, P);
  return hipGetLastError();
}

hipError_t launch_select_gain(const uint32_t* voxel, const uint32_t* q, size_t npix, int n_views, const uint32_t* bits,
                              const uint32_t* done, unsigned long long* sums, hipStream_t s) {
  if (npix == 0 || n_views == 0) return hipSuccess;
  const unsigned bx = (unsigned)std::min<size_t>(kSelectGainBlocks, (npix + 255) / 256);
  hipLaunchKernelGGL(select_gain_kernel, dim3(bx, (unsigned)n_views), dim3(256), 0, s, voxel, q, npix, bits, done, sums);
  return hipGetLastError();
}

hipError_t launch_select_mark(const uint32_t* voxel, size_t npix, int view, uint32_t* bits, uint32_t* done, hipStream_t s) {
  if (npix == 0) return hipSuccess;
  const unsigned bx = (unsigned)std::min<size_t>(1024, (npix + 255) / 256);
  hipLaunchKernelGGL(select_mark_kernel, dim3(bx), dim3(256), 0, s, voxel + (size_t)view * npix, npix, bits, done + view);
  return hipGetLastError();
}

} // namespace prv
