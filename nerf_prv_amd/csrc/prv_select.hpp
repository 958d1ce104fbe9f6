// prv_select.hpp -- parameter blocks and launchers of the view selection stage (prv_select.hip; the contract is in include/prv.h)
#pragma once
#include "../../include/prv.h"
#include "prv_device.hpp"

namespace prv {

constexpr uint32_t kSelectUnlocated = 0xFFFFFFFFu; // the voxel word of a pixel without a point
constexpr int kSelectGainBlocks = 128;             // most blocks per view of the gain launch (grid-stride beyond)

struct SelectFootprintParams {
  const CamDev* cams; // n_views cameras at W x H, in view_ids order
  int W, H, n_views;
  const float* entropy; // n_views * H * W each
  const float* alpha;
  const float* depth;
  float alpha_min;
  int G;           // grid cells per axis
  uint32_t* voxel; // out, n_views * H * W
  uint32_t* q;     // out, n_views * H * W
};

// voxel / q of every pixel (one lane per pixel)
hipError_t launch_select_footprint(const SelectFootprintParams& P, hipStream_t s);
// sums[v] += sum over view v's pixels of q * [unlocated or bit(voxel) not in bits], for every view with done[v] == 0
hipError_t launch_select_gain(const uint32_t* voxel, const uint32_t* q, size_t npix, int n_views, const uint32_t* bits,
                              const uint32_t* done, unsigned long long* sums, hipStream_t s);
// bits |= the voxels of view `view`'s located pixels; done[view] = 1
hipError_t launch_select_mark(const uint32_t* voxel, size_t npix, int view, uint32_t* bits, uint32_t* done, hipStream_t s);

} // namespace prv
