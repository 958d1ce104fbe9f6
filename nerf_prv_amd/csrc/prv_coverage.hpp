// prv_coverage.hpp -- constants and launchers of the surface coverage stage (prv_coverage.hip; the contract is in include/prv.h)
#pragma once
#include "../../include/prv.h"
#include "prv_device.hpp"

namespace prv {

// THE SCRATCH BUDGET of the z-buffers: the views of a handle are processed in batches of floor(budget / (4 W H)) views, at
// least one (a single 16384 x 16384 view takes 1 GiB: one view is always allowed, so no view count fails for z-buffer memory
// alone).  540 views of 80 x 45 take 7.8 MB and 144 views of 800 x 800 take 369 MB: one and two batches.
constexpr size_t kCoverageZBufBudget = (size_t)256 << 20;
constexpr int kCoverageMaxBatch = 65535;       // gridDim.y
constexpr uint32_t kCoverageEmpty = 0xFFFFFFFFu; // a z-buffer pixel no point covers; a first_seen entry of a point never covered
constexpr int kCoverageGainBlocks = 64;        // most blocks per view of the gain launch (grid-stride beyond)

// zbuf[v][y][x] = min over the points whose splat covers the pixel of the bits of their depth (n_batch views of W x H, set to
// kCoverageEmpty first)
hipError_t launch_coverage_depth(const float* xyz, size_t n, const CamDev* cams, int n_batch, int W, int H, int point_size, uint32_t* zbuf,
                                 hipStream_t s);
// bits[v][w] = the wave's ballot of "point 64 w + lane is visible in view v"; words = ceil(n / 64) per view, every one written
hipError_t launch_coverage_visible(const float* xyz, size_t n, const CamDev* cams, int n_batch, int W, int H, const uint32_t* zbuf, float tol1,
                                   unsigned long long* bits, size_t words, hipStream_t s);
// depth[v][y][x] = the z-buffer as float, 0 where empty
hipError_t launch_coverage_resolve(const uint32_t* zbuf, size_t n_pixels, float* depth, hipStream_t s);
// gain[v] += popcount(bits[v] & ~covered) for every view with done[v] == 0 (covered / done may be NULL: nothing covered / all views)
hipError_t launch_coverage_gain(const unsigned long long* bits, size_t words, int n_views, const unsigned long long* covered,
                                const uint32_t* done, unsigned long long* gain, hipStream_t s);
// covered |= view_bits; first_seen (may be NULL) of every newly covered point = round; *done_flag (may be NULL) = 1
hipError_t launch_coverage_mark(const unsigned long long* view_bits, size_t words, unsigned long long* covered, uint32_t* first_seen,
                                uint32_t round, uint32_t* done_flag, hipStream_t s);
// out[w] = OR over the views of bits[v][w]
hipError_t launch_coverage_union(const unsigned long long* bits, size_t words, int n_views, unsigned long long* out, hipStream_t s);

} // namespace prv
