// prv_tsdf.hpp -- depth-map fusion (prv_tsdf.hip): a truncated signed distance volume on the grid of prv_marching_cubes_grid,
// the kernel that fuses depth (and colour) images of a list of views into it, and what turns it into a grid and a mesh.
#pragma once
#include "prv_device.hpp"
#include "prv_mesh.hpp"

namespace prv {

// views one integrate launch takes; a call with more runs several launches over consecutive views (a point's views are then
// still taken in list order, and the state it carries from launch to launch is the float32 state itself: no byte changes)
constexpr int kTsdfChunk = 32;

// what the kernel needs of one view: wave-uniform, read from the kernel arguments into scalar registers
struct TsdfView {
  float c2w[12];           // engine frame, row-major 3x4
  float fx, fy, cx, cy;    // at the call's image size
  float lens[4];           // k1, k2, p1, p2; all zero = pinhole
  unsigned long long base; // pixel offset of the view's image in the call's planes (position in the list x width x height)
};
struct TsdfLaunch {
  TsdfView view[kTsdfChunk];
  int n_views;
  int width, height;
  float trunc, inv; // inv = 1.0f / trunc, formed once on the host in float32
};
static_assert(sizeof(TsdfLaunch) <= 3072, "the launch block travels as kernel arguments (4 KiB with the pointers and the grid)");

// state: planes of n floats each -- D, W and, with colours, WC, C[0], C[1], C[2] (tsdf_planes(colors) * n floats)
inline int tsdf_planes(bool colors) { return colors ? 6 : 2; }

// one lane per grid point: the views of `a` in order, the point's state in registers (read once, written once).
// weight / rgba may be null (1.0f / no colour step); rgba is read as one aligned 32-bit word per pixel
hipError_t launch_tsdf_integrate(const TsdfLaunch& a, const MeshGrid& g, bool colors, float* state, const float* depth, const float* weight,
                                 const uint32_t* rgba, hipStream_t s);
// counts[0..2] += observed (W > 0), inside (observed, D < 0), band (observed, |D| < 1); the caller zeroes them.  Integer adds.
hipError_t launch_tsdf_info(const float* state, size_t n, unsigned long long* counts, hipStream_t s);
// valid = W > 0 && W >= min_weight; grid = valid ? -D : NaN (either output may be null)
hipError_t launch_tsdf_grid(const float* state, size_t n, float min_weight, float* grid, uint8_t* valid, hipStream_t s);
// one lane per vertex: the colour of the nearest grid point, bytes = min(255, floor(C + 0.5)), 0 where WC == 0
hipError_t launch_tsdf_colors(const float* state, const MeshGrid& g, const float* xyz, uint64_t nv, uint8_t* rgb, hipStream_t s);

} // namespace prv
