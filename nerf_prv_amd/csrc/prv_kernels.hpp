// prv_kernels.hpp -- kernel parameter blocks and host-callable launchers.
#pragma once
#include "../../include/prv.h"
#include "prv_device.hpp"
#include "prv_field_plan.hpp"
#include "prv_queue_order.hpp"
#include <type_traits>

namespace prv {

// one queue record = 96 bytes = 6 x uint4:
//   {o.x o.y o.z t0} {d.x d.y d.z dt} {mask0..3} {pixel, chunk info, 0, 0} {SH coeffs 0..7 fp16} {SH 8..15 fp16}
// The mask is one 128-step CHUNK of the ray's live-sample mask.  PRV_STEP_FIXED_S: the only one (chunk info = 1 << 16).
// PRV_STEP_NGP (up to 1024 steps): the chunk that starts at the ray's first non-empty 32-step word; chunk info = first
// step of that chunk | number of chunks << 16, and chunks 1..n-1 sit in the record's slot of the extension buffer
// (kExtChunks x uint4 per queue slot, chunk-major: chunk j of slot s at [(j - 1) * n_slots + s], so that the lanes of a
// march wave -- consecutive slots -- store a chunk as one contiguous block), read by the render kernel only when a ray gets that far.
constexpr size_t kRecordBytes = 96;
constexpr int kRecordWords = 6;   // uint4 per record
constexpr uint32_t kClaim = 64;   // records a wave claims per atomic on the queue head
constexpr int kMaxSamples = 128;  // PRV_STEP_FIXED_S: the live-sample mask is one 128-bit chunk
constexpr int kNgpMaxSteps = PRV_NGP_MAX_STEPS; // PRV_STEP_NGP: dt = sqrt(3)/1024, the cube's diagonal
constexpr int kExtChunks = kNgpMaxSteps / 128 - 1;
constexpr size_t kExtBytes = (size_t)kExtChunks * 16;

struct MarchParams {
  FieldDev field;
  const CamDev* cams;
  const int* view_ids; // n_views indices into cams
  int W, H, S;
  uint32_t tiles_x, tiles_y;
  int tile_w_log2, tile_h_log2; // pixel tile of one 256-thread block
  int spp_inner_log2;           // > 0: sub-samples on adjacent lanes (spp = 2^n), 0: on grid.z
  int live_grid;                // 1: grid.x = the largest cull rectangle of the batch in tiles (CamDev::cull); pixels outside a
                                //    view's rectangle are NOT written (the caller consumes the image through the rectangles)
  uint32_t live_tiles_max;
  int step_mode; // PRV_STEP_FIXED_S | PRV_STEP_NGP
  void* queue;
  uint4* queue_ext;      // PRV_STEP_NGP: kExtChunks mask chunks per queue slot, chunk-major (n_slots = n_seg * seg_cap)
  unsigned long long* stat; // statistics block: [8 (1 + s)] += live samples (the march count), 8 shards a cache line apart
  uint32_t* queue_count; // n_seg counters, 64 bytes apart: records appended to region s of the queue
  int n_seg;             // the queue is n_seg regions of seg_cap records; a wave appends to the region of its first live ray's octant
  uint32_t seg_cap;      // (spatial_regions; 0: linear block id % n_seg, rounds 1-5), or to the next region that has room
  int spatial_regions;
  int n_sub;             // spatial_regions: the n_seg regions are n_seg / n_sub octant regions of n_sub sub-regions each (a counter per sub-region)
  int n_cells;           // PRV_REGION_CELLS: > 1 = every wave also writes its block's descriptor, keyed by which of n_cells^3 cells of the octant
  QueueDesc* desc;       //   its mid-span point falls in (prv_queue_order.hpp); seg_cap descriptors per region
  float* out_f32; // n_views*H*W*4
  uint32_t* out_u8; // optional, n_views*H*W
  int last_pass;
  float bg[4];
};

// the ensemble's march in one launch (march_multi_kernel): the common fields carry MarchParams' names
// (the host fills them in one place, prv_api.cpp: march_common)
struct MarchMember {
  void* queue;
  uint4* queue_ext;
  uint32_t* queue_count; // this member's n_seg counters, 64 bytes apart
  QueueDesc* desc;       // this member's descriptors (MarchParams::desc)
  float* out_f32;        // where this member's dead rays are written (its own staging / image)
  uint32_t* out_u8;
};
struct MarchMultiParams {
  const uint8_t* occ_bytes;        // occ_res^3 bytes, x fastest: bit e = member e's occupancy bit of the cell
  const uint8_t* occ_coarse_bytes; // (occ_res/4)^3 bytes of the members' dilated coarse grids, or null
  int occ_res;
  float occ_lo[3], occ_hi[3]; // the union of the members' occupied boxes
  const CamDev* cams;         // cull rectangles against the union box
  const int* view_ids;
  int W, H;
  uint32_t tiles_x, tiles_y;
  int tile_w_log2, tile_h_log2, spp_inner_log2;
  unsigned long long* stat;
  int n_seg;
  uint32_t seg_cap;
  int spatial_regions, n_sub; // MarchParams::spatial_regions, n_sub
  int n_cells;                // MarchParams::n_cells
  int last_pass;
  float bg[4];
  int n_members;
  MarchMember mem[PRV_MAX_MODELS];
};
struct OccInterleaveParams {
  const uint32_t* bits[PRV_MAX_MODELS];
  int n_members;
  uint32_t n_cells;
  uint8_t* out;
};
bool march_multi_supported(int n_members); // a compiled instance exists (2 and 5: the paper's ensembles)
hipError_t launch_march_multi(const MarchMultiParams& P, int n_views, int n_spp, hipStream_t s);
// the launch between march and render when n_cells > 1 (order_descriptors_kernel): every octant region's descriptors by cell key
struct OrderParams {
  const QueueDesc* desc;       // what the march wrote: seg_cap per region
  QueueDesc* sorted;           // n_sub * seg_cap per octant region
  const uint32_t* queue_count; // per region: [0] records, [1] descriptor indices handed out, [2] tail cut, [3] closed_at
  uint32_t* queue_head;        // [1] of an octant region's first sub-region <- the length of its sorted list
  int n_seg, n_sub;
  uint32_t seg_cap;
  int n_keys; // n_cells^3
};
hipError_t launch_order_descriptors(const OrderParams& P, hipStream_t s);
hipError_t launch_occ_interleave(const OccInterleaveParams& P, hipStream_t s);

struct RenderParams {
  FieldDev field;
  const void* queue;
  const uint4* queue_ext; // PRV_STEP_NGP: the mask chunks behind the record's own (see kRecordBytes)
  int step_mode;
  const uint32_t* queue_count; // n_segments counters, 64 bytes apart: records in region s
  uint32_t* queue_head; // n_segments heads, 64 bytes apart (region-relative record counts)
  int n_segments;
  int n_sub; // an XCD starts at sub-region 0 of ITS octant region: segment (XCC id % (n_segments / n_sub)) * n_sub
  uint32_t seg_cap;     // records per region: region s = [s * seg_cap, s * seg_cap + queue_count[16 s])
  int n_cells;          // > 1: a region is an OCTANT region, drained descriptor by descriptor from desc_sorted (one cursor: the head of its
  const QueueDesc* desc_sorted; // first sub-region; the list's length behind it), n_sub * seg_cap descriptors apart
  unsigned long long* stat_evaluated;
  float* out_f32;
  uint32_t* out_u8;
  float min_T;
  int last_pass;
  int merge_max; // render_queue64: a group down to <= this many rays hands them to the other group's idle slots (0 = never)
  int pool_on;   // render_queue64: ... or, failing that, to the block's LDS tail pool (any wave's idle slots adopt them)
  int cell_cache; // render_queue64: the instance whose lanes keep their last cell's corner entries per hashed level (incoherent gathers)
  float bg[4];
};

// what a launch renders: the colour image, or scalar planes (render_planes_kernel's MODE)
enum : int { kRenderColour = 0, kRenderDepth = 1, kRenderEntropy = 2, kRenderFootprint = 3, kRenderSurface = 4, kRenderTermination = 5 };

// what a mode computes per sample, and the words of a ray's state that tail merge and pool move between lanes through LDS:
// {record, next sample, T, r, g, b (, D)}, or density-only {record, next sample, T, H (, D | Dm | bin)} (render_queue64_body)
template <int MODE>
struct RenderMode {
  static constexpr bool FOOT = MODE == kRenderFootprint, SURF = MODE == kRenderSurface, TERM = MODE == kRenderTermination;
  static constexpr bool DEPTH = MODE == kRenderDepth || FOOT;                             // the sum D = sum_i w_i t_i
  static constexpr bool ENTROPY = MODE == kRenderEntropy || FOOT || SURF || TERM;          // density layers only; the sum H (TERM: the open bin's sum in its place)
  static constexpr bool DSTATE = DEPTH || SURF;                                           // the ray carries D (SURF: Dm) and keeps its sample's t across the MLP
  static constexpr int kDWord = ENTROPY ? 4 : 6;                                          // where D sits in the moved words (TERM: the bin)
  static constexpr int kMoveWords = kDWord + (DSTATE || TERM ? 1 : 0);
  static constexpr int kFrags = ENTROPY ? 8 : kNumFrags;                                  // fragment sets staged in LDS: the density layers', or both MLPs'
};
static_assert(RenderMode<kRenderColour>::kMoveWords == 6 && RenderMode<kRenderDepth>::kMoveWords == 7 && RenderMode<kRenderEntropy>::kMoveWords == 4, "moved words");
static_assert(RenderMode<kRenderFootprint>::kMoveWords == 5 && RenderMode<kRenderSurface>::kMoveWords == 5 && RenderMode<kRenderTermination>::kMoveWords == 5, "moved words");

// the plane-writing renders (render_planes_kernel): the colour launch's parameters, untouched, plus one float per pixel of
// the launch's images (r.out_f32 / 4) per plane.  A plane starts zeroed, which is what a dead ray contributes.
//   kRenderDepth (prv_render_depth):         the colour image and out_depth
//   kRenderEntropy (prv_render_entropy):     out_entropy and out_alpha; r.out_f32 / out_u8 are not touched
//   kRenderFootprint (prv_render_footprint): all three planes from one density-only launch; r.out_f32 / out_u8 are not touched
//   kRenderSurface (prv_render_surface):     out_entropy and out_alpha as kRenderEntropy; out_depth = the premultiplied z-depth of the first
//                                            sample after which T <= T_cross, out_hit = 1 where there is one; r.out_f32 / out_u8 are not touched
//   kRenderTermination (prv_render_termination): out_bins (n_bins planes, plane_stride floats apart: the ray's compositing weights by
//                                            depth bin) and out_alpha as kRenderEntropy; r.out_f32 / out_u8 are not touched
struct RenderPlanesParams {
  RenderParams r;
  float* out_depth; // premultiplied z-depth, engine units           (null where the mode does not write the plane)
  // depth / footprint, how a ray finds its view's camera: image i of the launch (i = pix / npix; sub-sample i / nb of view
  // i % nb) is seen by cams[view_ids[i % nb]]
  const CamDev* cams;
  const int* view_ids;
  uint32_t npix; // W * H
  uint32_t nb;   // views in the launch
  // the entropy planes come last: in front of the depth fields they cost the all-hashed footprint instance 7 more SGPR spills
  float* out_entropy; // H, bits
  float* out_alpha;   // 1 - T_end
  // the surface mode's own come behind everything the older instances read, so their argument offsets stay what they were
  float T_cross;  // the ray is located at its first sample after which T <= T_cross (the host: 1.0f - level)
  float* out_hit; // 1.0 where the ray got there, else 0.0
  // the termination mode's own, behind those again
  float* out_bins;     // plane k = the weights of the samples in depth bin k, at out_bins + k * plane_stride
  size_t plane_stride; // floats between two bin planes: the pixels of the buffer the launch writes (its images x W x H, or the caller's planes)
  uint32_t bin_mul;    // sample i falls in bin (i * bin_mul) >> 16: floor(n_bins * 65536 / n_max), n_max = the rule's step limit
  uint32_t n_bins;     // a power of two in [4, 64]
};

struct EnsembleParams {
  const uint32_t* imgs[PRV_MAX_MODELS];
  int E;
  int view0; // first view of this batch (the addend buffer holds one batch)
  size_t pixels_per_view;
  double* partial; // addends: [view - view0][pixel][k]
};

struct PsnrParams {
  const float* rgba;
  const float* gt;
  const CamDev* cams; // optional: view v's cull rectangle bounds what was rendered (see score_psnr_kernel)
  int W;
  size_t pixels_per_view;
  float bg[4];
  double* partial;
};

struct RepackLevel { // canonical -> physical copy of one level (entries, not bytes)
  uint32_t canon_off, phys_off, n, res, sx, hashed;
};
hipError_t launch_repack_level(const uint16_t* canon, uint16_t* phys, const RepackLevel& L, int F, hipStream_t s);

hipError_t launch_march(const MarchParams& P, int n_views, int n_spp, hipStream_t s);
hipError_t launch_spp_reduce(const float* stage, size_t n_pixels, int spp, const float bg[4], float* out, uint32_t* out_u8,
                             hipStream_t s);
hipError_t launch_render(const RenderParams& P, const ReplicaDev& R, int n_blocks, hipStream_t s); // R: the model's replicas (n_levels 0: none)
hipError_t launch_render_planes(const RenderPlanesParams& P, int mode, int n_blocks, hipStream_t s); // mode: kRenderDepth / Entropy / Footprint / Surface / Termination
hipError_t launch_spp_reduce_depth(const float* stage, size_t n_pixels, int spp, float* out, hipStream_t s);
hipError_t launch_score_entropy(const float* entropy, const float* alpha, size_t npix, int n_views, int n_blocks, double* partial,
                                hipStream_t s);
// PRV_SCORE_TERMINATION_JSD / prv_termination_divergence: the Jensen-Shannon divergence of E members' termination histograms, per pixel
struct TerminationJsdParams {
  const float* bins[PRV_MAX_MODELS];  // member e: n_bins planes, plane_stride floats apart, of n_views * npix floats
  const float* alpha[PRV_MAX_MODELS]; // member e: n_views * npix floats
  int E, n_bins;
  size_t npix, plane_stride;
  float* out_jsd;  // n_views * npix floats, or null
  double* partial; // [view][block][2]: the block's sums of J and of the members' mean opacity
};
hipError_t launch_score_termination_jsd(const TerminationJsdParams& P, int n_views, int n_blocks, hipStream_t s);
// the compiled instance of the field-evaluating kernels (render, planes, mesh, field hook) a field runs on: prv_field_plan.hpp has the rule
inline int render_instance_dense_levels(const FieldDev& fd) { return instance_dense_levels(fd.n_features, fd.n_dense_levels, fd.hash_shared); }
// calls fn(std::integral_constant<int, F>{}, std::integral_constant<int, NDENSE>{}) for the one compiled instance fd runs on:
// the only list of the six (F, NDENSE) pairs a kernel template is instantiated for
template <class Fn>
void with_field_instance(const FieldDev& fd, Fn&& fn) {
  using std::integral_constant;
  const int nd = render_instance_dense_levels(fd);
  if (fd.n_features == 4) {
    if (nd == 5) fn(integral_constant<int, 4>{}, integral_constant<int, 5>{});
    else if (nd == 3) fn(integral_constant<int, 4>{}, integral_constant<int, 3>{});
    else fn(integral_constant<int, 4>{}, integral_constant<int, 0>{});
  } else {
    if (nd == 10) fn(integral_constant<int, 2>{}, integral_constant<int, 10>{});
    else if (nd == 6) fn(integral_constant<int, 2>{}, integral_constant<int, 6>{});
    else fn(integral_constant<int, 2>{}, integral_constant<int, 0>{});
  }
}
// Dense replicas of hashed levels (prv_device.hpp: ReplicaDev).  Only the <4, 5> instance has replica variants: a model holds
// replicas only if it runs that instance, and the launch goes by what the model holds (0: the plain instance).
// The engine's stepping rule (dt = 0.43 finest cells: it walks the occupied volume densely) gathers from the replicas of at most
// two levels, whatever the model holds.  64 views 800x800 of api.FIELD_256 under that rule, render launch: 40.35 ms without
// replicas, 38.97 / 38.31 / 40.81 ms with 1 / 2 / 3 -- the finest level's 143 MB replica costs more in L2 misses than its hash
// did in instructions.  Under the fixed-S rule all three win (8.07 -> 7.77 / 7.59 / 7.51 ms).  profiles/NOTES.md
constexpr int kReplicaLevelsNgp = 2;
inline int replica_instance_levels(const FieldDev& fd, const ReplicaDev& R) {
  return R.table && fd.n_features == 4 && render_instance_dense_levels(fd) == 5 ? R.n_levels : 0;
}
// (replica_level_layout, one replica's strides and size: prv_field_plan.hpp)
hipError_t launch_fill_replica(const FieldDev& fd, const ReplicaDev& R, int k, hipStream_t s); // replica k from fd.table (the physical table)
struct PreceptPose {
  double w2c[16], c2w[16];
};
hipError_t launch_precept(const FieldDev& fd, const float* voxels, int n, const PreceptPose& pose, const Rs2Intr& in,
                          float max_range, int32_t* out, hipStream_t s);
hipError_t launch_first_hit(const FieldDev& fd, const CamDev* cams, int n_views, int W, int H, float max_range,
                            int32_t* out, hipStream_t s);
hipError_t launch_splat_points(const float* xyz, const uint8_t* rgb, size_t n, float scale, const float off[3],
                               const CamDev* cams, int n_views, int W, int H, int point_size, int flip180,
                               unsigned long long* zbuf, uint32_t* out, hipStream_t s);
hipError_t launch_quantize(const float* in, size_t n, const float bg[4], uint8_t* out, hipStream_t s);
hipError_t launch_score_ensemble(const EnsembleParams& P, int method, int n_views, int n_blocks, prv_score_record* rec,
                                 hipStream_t s);
hipError_t launch_score_psnr(const PsnrParams& P, int n_views, int n_blocks, hipStream_t s);
hipError_t launch_ssim(const float* img, const float* gt, int n_views, int W, int H, const float bg[4], float* la,
                       float* lb, double* partial, int n_blocks, double* out, hipStream_t s);
hipError_t launch_score_finalize(const double* partial, int n_views, int n_blocks, int method,
                                 size_t pixels_per_view, double coverage_weight, prv_score_record* rec, hipStream_t s);
hipError_t launch_synth_table(uint16_t* table, size_t n, uint64_t seed, float amp, hipStream_t s);
hipError_t launch_debug_raygen(const CamDev& cam, int W, int H, int spp_k, float* o, float* d, float* t,
                               hipStream_t s);
hipError_t launch_debug_field(const FieldDev& fd, const ReplicaDev& R, const float* pos, const float* dir, int n, uint16_t* feat,
                              float* out36, int32_t* occ, hipStream_t s);

} // namespace prv
