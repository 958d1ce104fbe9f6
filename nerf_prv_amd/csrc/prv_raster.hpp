// prv_raster.hpp -- constants and launchers of the triangle rasteriser (prv_raster.hip; the contract is in include/prv.h,
// "mesh depth and the mesh occluder")
#pragma once
#include "../../include/prv.h"
#include "prv_coverage.hpp"

namespace prv {

// THE DEFERRED LIST: (view, triangle) pairs whose clipped pixel box holds more than small_max pixels.  Triangles go through
// in chunks with chunk x views <= capacity, every pair adds at most one entry, so the list cannot overflow.
struct RasterPair {
  uint32_t view, tri; // view: position in the launch's camera array; tri: id in the mesh
};
static_assert(sizeof(RasterPair) == 8, "one list entry is 8 bytes");
constexpr size_t kRasterListEntries = (size_t)1 << 22; // default capacity (32 MiB); PRV_RASTER_LIST_ENTRIES overrides it per call
constexpr size_t kRasterListEntriesMost = (size_t)1 << 28;
// most pixels of a clipped box that the lane of the small path walks itself; PRV_RASTER_SMALL_PIXELS overrides it per call.
// Measured (profiles/NOTES.md, scripts/rasterbench.py): 16 to 1024 time the same on both planner-like workloads, 1 and 4 are far
// slower at 800 x 800; 64 stays.
constexpr int kRasterSmallPixels = 64;
constexpr unsigned kRasterLargeBlocks = 4096; // most workgroups of the large launch (entries beyond: block-stride)

// zbuf[v][y][x] = min(zbuf, bits of the depth of triangles [t0, t0 + n) of the mesh at the pixel's centre) for the n_views
// cameras of `cams`: raster_small_kernel, then raster_large_kernel on what it deferred.  n * n_views <= capacity (checked).
// *count is zeroed here; *large_total (device) gains the number of deferred pairs.  zbuf is NOT cleared here.
// Key = uint32_t: the depth buffer as described; Key = unsigned long long: the visibility buffer, bits of the depth << 32 |
// triangle id (instantiated for these two in prv_raster.hip).
template <typename Key>
hipError_t launch_raster(const float* xyz, const uint32_t* tri, size_t t0, size_t n, const CamDev* cams, int n_views, int W, int H,
                         int small_max, RasterPair* list, size_t capacity, uint32_t* count, unsigned long long* large_total, Key* zbuf,
                         hipStream_t s);
// stage B of prv_mesh_render: keys[v][y][x] of n_views views -> rgba[v] (RGBA8 as uint32, turned by 180 degrees if flip180), and,
// where not NULL, depth[v] (0 = empty) and tri_out[v] (0xFFFFFFFF = empty), both unflipped.  rgb: 3 bytes per vertex.
hipError_t launch_raster_shade(const float* xyz, const uint32_t* tri, const uint8_t* rgb, const CamDev* cams, int n_views, int W, int H,
                               const unsigned long long* keys, int flip180, uint32_t* rgba, float* depth, uint32_t* tri_out, hipStream_t s);
// launch_coverage_visible with a mesh's depth buffer: a point whose pixel holds no triangle is visible
hipError_t launch_raster_visible(const float* xyz, size_t n, const CamDev* cams, int n_batch, int W, int H, const uint32_t* zbuf, float tol1,
                                 unsigned long long* bits, size_t words, hipStream_t s);

} // namespace prv
