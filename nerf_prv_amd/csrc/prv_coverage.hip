// prv_coverage.hip -- surface coverage of a reference cloud by a set of views (prv_coverage_*; the arithmetic contract is written
// out in include/prv.h).  Which points of an engine-frame cloud does each view see, how many does a list of views see together,
// and how many could the best greedy choice of as many views have seen.
//
//  coverage_depth_kernel   : one lane = one point of one view (grid: ceil(N/256) x views of the batch, as the point splat has it):
//       the point's ps x ps pixel block, clipped, gets atomicMin of the bits of its depth (z > 1e-6: the bits order as the floats
//       do) on a uint32 z-buffer that starts at 0xFFFFFFFF.  A minimum does not depend on the order.
//  coverage_visible_kernel : same grid; the lane's predicate "my point is in the image and not behind the nearest depth of its
//       pixel by more than the tolerance" goes through the wave's __ballot, and lane 0 stores the 64-bit word bits[view][i / 64].
//       No atomics: every word is written exactly once, zero words included; lanes past N contribute 0.
//  coverage_gain_kernel    : blockIdx.y = view, grid-stride over the view's words, popcount(bits & ~covered), reduced within the
//       wave by shuffles, ONE 64-bit integer atomic add per wave into the view's gain.  Integer adds commute.
//  coverage_mark_kernel    : covered |= the chosen view's words (one lane per word: no two lanes touch a word), and the round
//       index into first_seen of the points that are new.
//  coverage_union_kernel   : the OR of all views, one lane per word.
//
// No LDS, no MFMA, no workgroup waits for another.  All device writes are ordinary vector stores or atomics in plain C++.
#include "prv_coverage.hpp"

#include <algorithm>

namespace prv {

// the projection of both passes: the splat's, and the depth must be finite (an Inf or NaN coordinate never is: never visible)
__device__ __forceinline__ bool coverage_project(const CamDev& cam, const float* __restrict__ xyz, size_t i, float& u, float& v, float& z) {
  const float e[3] = {xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2]};
  if (!project_engine_point(cam, e, u, v, z)) return false;
  return z < __builtin_inff();
}

__global__ __launch_bounds__(256) void coverage_depth_kernel(const float* __restrict__ xyz, size_t n, const CamDev* __restrict__ cams, int W, int H,
                                                             int point_size, uint32_t* __restrict__ zbuf) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const CamDev cam = cams[blockIdx.y];
  float u, v, z;
  if (!coverage_project(cam, xyz, i, u, v, z)) return;
  // the splat's block: x0 = (int)floorf(u - 0.5f * ps + 0.5f); the clip is taken on the floats (a NaN or a far-away block fails
  // it), so the conversion to int only ever sees values in (-ps, W)
  const float ps = (float)point_size;
  const float fx0 = floorf(u - 0.5f * ps + 0.5f), fy0 = floorf(v - 0.5f * ps + 0.5f);
  if (!(fx0 > -ps && fx0 < (float)W && fy0 > -ps && fy0 < (float)H)) return;
  const int x0 = (int)fx0, y0 = (int)fy0;
  const int xa = max(x0, 0), xb = min(x0 + point_size, W), ya = max(y0, 0), yb = min(y0 + point_size, H);
  uint32_t* zb = zbuf + (size_t)blockIdx.y * W * H;
  const uint32_t key = __float_as_uint(z);
  for (int y = ya; y < yb; y++)
    for (int x = xa; x < xb; x++) atomicMin(zb + (size_t)y * W + x, key);
}

__global__ __launch_bounds__(256) void coverage_visible_kernel(const float* __restrict__ xyz, size_t n, const CamDev* __restrict__ cams, int W, int H,
                                                               const uint32_t* __restrict__ zbuf, float tol1,
                                                               unsigned long long* __restrict__ bits, size_t words) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  bool visible = false; // (no lane leaves before the ballot)
  if (i < n) {
    const CamDev cam = cams[blockIdx.y];
    float u, v, z;
    if (coverage_project(cam, xyz, i, u, v, z)) {
      const float fu = floorf(u), fv = floorf(v);
      if (fu >= 0.0f && fu < (float)W && fv >= 0.0f && fv < (float)H) { // (a NaN fails)
        const float zmin = __uint_as_float(zbuf[(size_t)blockIdx.y * W * H + (size_t)(int)fv * W + (size_t)(int)fu]);
        visible = z <= zmin * tol1; // (an empty pixel reads as a NaN: false)
      }
    }
  }
  const unsigned long long word = __ballot(visible);
  const size_t w = (size_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if ((threadIdx.x & 63) == 0 && w < words) bits[(size_t)blockIdx.y * words + w] = word;
}

__global__ __launch_bounds__(256) void coverage_resolve_kernel(const uint32_t* __restrict__ zbuf, size_t n_pixels, float* __restrict__ depth) {
  for (size_t p = (size_t)blockIdx.x * 256 + threadIdx.x; p < n_pixels; p += (size_t)gridDim.x * 256) {
    const uint32_t k = zbuf[p];
    depth[p] = k == kCoverageEmpty ? 0.0f : __uint_as_float(k);
  }
}

__global__ __launch_bounds__(256) void coverage_gain_kernel(const unsigned long long* __restrict__ bits, size_t words,
                                                            const unsigned long long* __restrict__ covered, const uint32_t* __restrict__ done,
                                                            unsigned long long* __restrict__ gain) {
  const int v = blockIdx.y;
  if (done && done[v]) return; // block-uniform
  const unsigned long long* bv = bits + (size_t)v * words;
  unsigned long long acc = 0ull;
  for (size_t w = (size_t)blockIdx.x * 256 + threadIdx.x; w < words; w += (size_t)gridDim.x * 256) {
    const unsigned long long c = covered ? covered[w] : 0ull;
    acc += (unsigned long long)__popcll(bv[w] & ~c);
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) acc += __shfl_down(acc, off);
  if ((threadIdx.x & 63) == 0 && acc != 0ull) atomicAdd(gain + v, acc);
}

__global__ __launch_bounds__(256) void coverage_mark_kernel(const unsigned long long* __restrict__ view_bits, size_t words,
                                                            unsigned long long* __restrict__ covered, uint32_t* __restrict__ first_seen,
                                                            uint32_t round, uint32_t* __restrict__ done_flag) {
  for (size_t w = (size_t)blockIdx.x * 256 + threadIdx.x; w < words; w += (size_t)gridDim.x * 256) {
    const unsigned long long b = view_bits[w], c = covered[w];
    unsigned long long fresh = b & ~c;
    if (fresh == 0ull) continue;
    covered[w] = c | b;
    if (first_seen)
      while (fresh) { // (bits of lanes past N are never set: every index is below N)
        const int j = __ffsll((long long)fresh) - 1;
        first_seen[w * 64 + (size_t)j] = round;
        fresh &= fresh - 1ull;
      }
  }
  if (done_flag && blockIdx.x == 0 && threadIdx.x == 0) *done_flag = 1u;
}

__global__ __launch_bounds__(256) void coverage_union_kernel(const unsigned long long* __restrict__ bits, size_t words, int n_views,
                                                             unsigned long long* __restrict__ out) {
  for (size_t w = (size_t)blockIdx.x * 256 + threadIdx.x; w < words; w += (size_t)gridDim.x * 256) {
    unsigned long long acc = 0ull;
    for (int v = 0; v < n_views; v++) acc |= bits[(size_t)v * words + w];
    out[w] = acc;
  }
}

static unsigned stride_blocks(size_t items, size_t most) { return (unsigned)std::max<size_t>(1, std::min<size_t>(most, (items + 255) / 256)); }

hipError_t launch_coverage_depth(const float* xyz, size_t n, const CamDev* cams, int n_batch, int W, int H, int point_size, uint32_t* zbuf,
                                 hipStream_t s) {
  if (n_batch <= 0) return hipSuccess;
  hipError_t e = hipMemsetAsync(zbuf, 0xff, (size_t)n_batch * W * H * 4, s);
  if (e != hipSuccess || n == 0) return e;
  hipLaunchKernelGGL(coverage_depth_kernel, dim3((unsigned)((n + 255) / 256), (unsigned)n_batch), dim3(256), 0, s, xyz, n, cams, W, H, point_size, zbuf);
  return hipGetLastError();
}

hipError_t launch_coverage_visible(const float* xyz, size_t n, const CamDev* cams, int n_batch, int W, int H, const uint32_t* zbuf, float tol1,
                                   unsigned long long* bits, size_t words, hipStream_t s) {
  if (n_batch <= 0 || n == 0) return hipSuccess;
  hipLaunchKernelGGL(coverage_visible_kernel, dim3((unsigned)((n + 255) / 256), (unsigned)n_batch), dim3(256), 0, s, xyz, n, cams, W, H, zbuf, tol1,
                     bits, words);
  return hipGetLastError();
}

hipError_t launch_coverage_resolve(const uint32_t* zbuf, size_t n_pixels, float* depth, hipStream_t s) {
  if (n_pixels == 0) return hipSuccess;
  hipLaunchKernelGGL(coverage_resolve_kernel, dim3(stride_blocks(n_pixels, 4096)), dim3(256), 0, s, zbuf, n_pixels, depth);
  return hipGetLastError();
}

hipError_t launch_coverage_gain(const unsigned long long* bits, size_t words, int n_views, const unsigned long long* covered,
                                const uint32_t* done, unsigned long long* gain, hipStream_t s) {
  if (words == 0 || n_views <= 0) return hipSuccess;
  for (int v0 = 0; v0 < n_views; v0 += kCoverageMaxBatch) { // (gridDim.y)
    const int nv = std::min(kCoverageMaxBatch, n_views - v0);
    hipLaunchKernelGGL(coverage_gain_kernel, dim3(stride_blocks(words, kCoverageGainBlocks), (unsigned)nv), dim3(256), 0, s,
                       bits + (size_t)v0 * words, words, covered, done ? done + v0 : nullptr, gain + v0);
  }
  return hipGetLastError();
}

hipError_t launch_coverage_mark(const unsigned long long* view_bits, size_t words, unsigned long long* covered, uint32_t* first_seen,
                                uint32_t round, uint32_t* done_flag, hipStream_t s) {
  if (words == 0) return hipSuccess;
  hipLaunchKernelGGL(coverage_mark_kernel, dim3(stride_blocks(words, 1024)), dim3(256), 0, s, view_bits, words, covered, first_seen, round, done_flag);
  return hipGetLastError();
}

hipError_t launch_coverage_union(const unsigned long long* bits, size_t words, int n_views, unsigned long long* out, hipStream_t s) {
  if (words == 0) return hipSuccess;
  hipLaunchKernelGGL(coverage_union_kernel, dim3(stride_blocks(words, 1024)), dim3(256), 0, s, bits, words, n_views, out);
  return hipGetLastError();
}

} // namespace prv
