// prv_geom.hpp -- geometric evaluation (prv_geom.hip): area-weighted mesh sampling, nearest neighbours, distance metrics.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

namespace prv {

// ---- surface sampling (the rule is stated in include/prv.h, prv_mesh_sample)
constexpr double kGeomAreaScale = 1099511627776.0; // 2^40 weight units per unit area
constexpr uint64_t kGeomStreamStratum = 0x5A0, kGeomStreamBary = 0x5A2; // RNG streams: stratum offset (two draws), barycentrics (two)

// weight[t] = floor(area_fp64(t) * 2^40), 0 for a triangle without (finite, positive) area
hipError_t launch_geom_tri_weights(const float* xyz, const uint32_t* tri, uint64_t nt, uint64_t* weight, hipStream_t s);
// scan = the exclusive scan of the weights, total = their sum; q = total / n, r = total % n (the strata's bounds)
hipError_t launch_geom_sample(const float* xyz, const uint32_t* tri, const uint64_t* scan, uint64_t nt, uint64_t total, uint64_t n,
                              uint64_t seed, float* out_xyz, uint32_t* out_tri, hipStream_t s);

// ---- nearest neighbours
// The uniform grid over the reference points' bounding box.  Cell of p on axis a: clamp((int)((p - lo) * inv), 0, dims - 1);
// cells are numbered in 4x4x4 bricks (brick-major, x fastest inside and between bricks), so consecutive keys are neighbours
// in space and the 64 sorted queries of a wave sit in a compact box of cells.
struct NNGrid {
  float lo[3], hi[3], inv[3], cs[3]; // box, cells per unit length, cell size (0 / 0 on an axis without extent: dims 1)
  int dims[3], nb[3];                // cells and bricks per axis
  float slack;                       // what the stopping bound gives away for rounding: 2^-20 * the largest |coordinate| of the box
};
inline size_t nn_keys(const NNGrid& g) { return (size_t)g.nb[0] * g.nb[1] * g.nb[2] * 64; }
constexpr int kNNBoxBlocks = 1024; // blocks (= partial boxes) of the validation pass

// partial[6 * block] = min xyz, max xyz of the block's points (+-inf for none); *flag |= 1 on a non-finite coordinate
hipError_t launch_nn_bbox(const float* xyz, uint64_t n, float* partial, uint32_t* flag, hipStream_t s);
// keys[i] = the cell key of point i; count[key] += 1 (vector integer atomics)
hipError_t launch_nn_keys(const NNGrid& g, const float* xyz, uint64_t n, uint32_t* keys, uint64_t* count, hipStream_t s);
// cursor = the exclusive scan of count; record (x, y, z, id bits) of point i goes to cursor[key]++ : afterwards cursor[key] is
// the END of the cell's run and cursor[key - 1] (0 for key 0) its start.  The order inside a run varies from run to run.
hipError_t launch_nn_scatter(const float* xyz, uint64_t n, const uint32_t* keys, uint64_t* cursor, float4* records, hipStream_t s);
// records without binning, in id order (the brute-force twin's reference set)
hipError_t launch_nn_pack(const float* xyz, uint64_t n, float4* records, hipStream_t s);
// queries = binned records (launch_nn_scatter with the reference's grid); results land at the record's id.  tests += the
// (query, reference) pairs whose distance was formed.
hipError_t launch_nn_query_grid(const NNGrid& g, const float4* ref, const uint64_t* ref_end, const float4* queries, uint64_t m,
                                float* out_d2, uint32_t* out_id, unsigned long long* tests, hipStream_t s);
// every query against every reference record, tiled through LDS
hipError_t launch_nn_query_brute(const float4* ref, uint64_t n, const float* queries, uint64_t m, float* out_d2, uint32_t* out_id,
                                 hipStream_t s);

// ---- metrics
struct GeomPartial { // one direction's reduction
  double sum_d, sum_d2;
  uint64_t within;
  float max_d;
  uint32_t pad;
};
constexpr int kGeomReduceBlocks = 1024;
// dist = the correctly rounded fp32 sqrt of d2 (through fp64); per block: sum of dist and of d2 in fp64, count of dist <= tau, max dist; the blocks' partials are then
// summed in block order by one thread into *out.  partial: kGeomReduceBlocks elements.
hipError_t launch_geom_reduce(const float* d2, uint64_t n, float tau, GeomPartial* partial, GeomPartial* out, hipStream_t s);

} // namespace prv
