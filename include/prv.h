/*
 * prv.h -- C ABI of the MI355X-native NeRF render + candidate-view scoring path.
 *
 * This is the drop-in boundary for the hot path of psc0628/NeRF-PRV.  In the
 * reference that boundary is a process + filesystem handshake:
 *   PRV_simulation/main.cpp:1658-1715  NBV_Net_Labeler::train_by_instantNGP writes
 *       interact/run_with_c++.py + ready_c++.txt and polls ready_py.txt;
 *   Instantngp_scripts/train_server.py:7-14 runs the script;
 *   Instantngp_scripts/run.py:284-309 renders every frame of --screenshot_transforms
 *       through pyngp.Testbed.render and writes PNGs;
 *   PRV_simulation/main.cpp:2045-2096 / 2105-2160 reads the PNGs back and scores.
 * Each entry point below names the reference interface it replaces.  Everything is
 * plain C: opaque handles, pointers and sizes, int error codes; nothing throws.
 *
 * Memory spaces: "host" pointers are ordinary memory; "dev" pointers are HIP device
 * memory on the context's GPU (from prv_malloc, or any other HIP allocation such as
 * a torch tensor's data_ptr).  All work is enqueued on the context's stream
 * (prv_set_stream) and functions that return results to host memory synchronise it.
 *
 * The library REQUIRES a gfx950 device: there is no CPU fallback.  prv_create fails
 * with PRV_E_NODEVICE when no GPU is visible.
 */
#ifndef PRV_H
#define PRV_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PRV_ABI_VERSION 5 /* 2: prv_field_desc.per_level_scale; 3: prv_render_opts.step_mode, prv_stats.samples_live; 4: prv_train_opts.patch_w / patch_h; 5: prv_train_opts.step_mode / deterministic (still 5: prv_train_create accepting lr = 0, which it refused, changes no layout and no call that worked; nor do the prv_coverage_* entry points: additive; nor prv_mesh_from_arrays, prv_mesh_depth and prv_coverage_create_occluded: additive too; nor prv_debug_live_bytes; nor prv_mesh_set_colors and prv_mesh_render: additive; nor the prv_tsdf_* entry points and prv_marching_cubes_grid_valid: additive) */

/* error codes (0 = ok, < 0 = error; message via prv_last_error) */
#define PRV_OK 0
#define PRV_E_INVALID (-1)  /* bad argument */
#define PRV_E_HIP (-2)      /* HIP runtime error */
#define PRV_E_IO (-3)       /* file / parse error */
#define PRV_E_NODEVICE (-4) /* no usable GPU */
#define PRV_E_STATE (-5)    /* e.g. model slot empty */
#define PRV_E_INTERNAL (-6) /* host allocation failure / unexpected internal error: no exception crosses the ABI */

/* scoring methods; 2 and 3 are the reference's method_of_IG values (Share_Data.hpp:198-202) */
#define PRV_SCORE_ENSEMBLE_RGB 2         /* main.cpp:2039-2097 */
#define PRV_SCORE_ENSEMBLE_RGB_DENSITY 3 /* main.cpp:2099-2161 */
#define PRV_SCORE_PSNR_COVERAGE 5        /* -PSNR (run.py:257-263, vs supplied images) + w * mean((1 - alpha)^2), the
                                            density term of main.cpp:2148; w = prv_set_coverage_weight */
#define PRV_SCORE_RAY_ENTROPY 7          /* mean over the view's pixels of prv_render_entropy's H: one model, no reference
                                            images.  This build's own (not in the reference), like 5; the ids mirror the
                                            planner's method_of_IG values, where 6 stays unassigned */
#define PRV_SCORE_TERMINATION_JSD 9      /* mean over the view's pixels of the Jensen-Shannon divergence between the ensemble
                                            members' ray-termination histograms (prv_render_termination, prv_termination_divergence):
                                            2..8 models, no reference images.  This build's own; 8 stays unassigned */
#define PRV_TERMINATION_BINS_DEFAULT 16  /* depth bins of PRV_SCORE_TERMINATION_JSD's histograms */
#define PRV_COVERAGE_WEIGHT_DEFAULT 1.0  /* the reference adds its density term with unit weight too (main.cpp:2147-2148) */

#define PRV_MAX_MODELS 8  /* members of one ensemble (one scoring call) */
#define PRV_MAX_SLOTS 64  /* model slots of a context: several objects' ensembles side by side (prv_planner shard: members) */
#define PRV_MLP_HALFS 10240 /* 32*64 + 64*16 + 32*64 + 64*64 + 64*16, canonical [in][out] */

typedef struct prv_ctx prv_ctx;
typedef struct prv_camset prv_camset;

/* The NeRF field: multiresolution hash grid (L levels x F fp16 features, L*F = 32),
 * density MLP 32->64->16, SH-4 direction encoding, colour MLP 32->64->64->16, and an
 * occupancy bitfield.  Stands in for the instant-ngp network the reference trains
 * through run.py:185-208. */
typedef struct prv_field_desc {
  int32_t n_levels;
  int32_t n_features;
  int32_t log2_hashmap;
  int32_t base_res;
  int32_t finest_res;
  int32_t occ_res;
  float density_bias; /* sigma = exp(out0 + density_bias); a sigma below 2^-126 (a logit under about -87.3) may be returned as 0,
                         a logit above 88.72 gives +Inf (tests/test_gpu_field_regimes.py::test_field_outputs, `saturated`) */
  float table_amp;    /* synthetic generator only: table ~ U(-amp, amp) */
  float per_level_scale; /* 0: the levels grow geometrically from base_res to finest_res (double precision, nominal
                            integer resolutions hit exactly).  > 0: tiny-cuda-nn's recipe in float32 -- scale_l =
                            exp2f(l * log2f(per_level_scale)) * base_res - 1, res_l = ceilf(scale_l) + 1 -- the level
                            geometry an imported instant-ngp snapshot was trained with; finest_res is then only a label */
} prv_field_desc;

/* How a ray is sampled.
 * PRV_STEP_FIXED_S: samples_per_ray (<= 128) uniform samples between the AABB entry and exit -- the fixed sample
 *   count BASELINE configs[1] and [3] prescribe.
 * PRV_STEP_NGP: the rule pyngp.Testbed.render applies behind run.py:245-247, 304 for aabb_scale = 1 (the reference's
 *   ray_casting_aabb_scale, DefaultConfiguration.yaml:36): a fixed step dt = sqrt(3)/1024 from the AABB entry, sample i
 *   at t0 + (i + 1/2) dt while inside the box (at most PRV_NGP_MAX_STEPS, the cube's diagonal), every step tested against
 *   the occupancy grid, alpha = 1 - exp(-sigma dt) with that dt; samples_per_ray is ignored.  The engine is not in
 *   the reference tree: the rule is restated from the published algorithm, without its per-ray start
 *   jitter (a renderer-side dither the reference's scores do not depend on); parity unpinned. */
#define PRV_STEP_FIXED_S 0
#define PRV_STEP_NGP 1
#define PRV_NGP_MAX_STEPS 1024

/* render options == the knobs run.py sets on the Testbed before render():
 * w,h (run.py:304), screenshot_spp (run.py:48,304), render_min_transmittance
 * (run.py:235; the engine's default is 0.01), background_color (run.py:94,226).  samples_per_ray is the fixed
 * per-ray sample count of the BASELINE configs (step_mode PRV_STEP_FIXED_S). */
typedef struct prv_render_opts {
  int32_t width;
  int32_t height;
  int32_t samples_per_ray;
  int32_t spp;
  float min_transmittance;
  float background[4];
  int32_t step_mode; /* PRV_STEP_FIXED_S (0) | PRV_STEP_NGP */
} prv_render_opts;

typedef struct prv_score_record { /* 16 bytes: the unit of the multi-GPU all-gather */
  double score;                   /* ranking key: larger = chosen first; NaN ranks last */
  float psnr;                     /* dB (method 5), else 0 */
  float coverage;                 /* mean opacity of the render (methods 5 and 7), else 0 */
} prv_score_record;

typedef struct prv_stats {
  uint64_t rays;              /* primary rays generated (pixels x spp) */
  uint64_t samples_nominal;   /* rays x samples_per_ray (PRV_STEP_NGP: rays x PRV_NGP_MAX_STEPS) */
  uint64_t samples_evaluated; /* field evaluations actually composited */
  uint64_t wave_rounds;       /* render_queue wave iterations (32 sample slots each): slot utilisation */
  uint64_t samples_live;      /* samples in occupied cells, before early termination: the march pass's own count */
} prv_stats;

/* ---- context ------------------------------------------------------------- */
/* replaces: starting train_server.py and importing pyngp (train_server.py:1-7, run.py:90) */
int prv_create(prv_ctx** out, int device_id);
void prv_destroy(prv_ctx* ctx);
/* replaces: nothing -- the reference returns 0 unconditionally (main.cpp:1714) and hangs
 * on failure (main.cpp:1695-1698).  ctx may be NULL for the last error of a failed create. */
const char* prv_last_error(const prv_ctx* ctx);
int prv_abi_version(void);
/* enqueue all work on this hipStream_t from now on; NULL is HIP's legacy default stream.
 * Until this is called the context uses a private non-blocking stream. */
int prv_set_stream(prv_ctx* ctx, void* hip_stream);
/* For a host process that OWNS the GPU runtime (prv_planner) and is about to return from main: ends its use of the GPU
 * in a defined order.  Every context must have been destroyed (PRV_E_STATE otherwise); synchronises and resets every
 * device a context was created on (hipDeviceReset), so the HIP runtime's own state -- its streams, signal pools and
 * worker threads -- is torn down HERE, while the process is still intact, and the static destructors that run after
 * main find nothing left to race with.  (A process in which a communicator loaded librccl is only synchronised, not
 * reset: that library stays loaded and releases device state of its own after main.)  (The reference's boundary had no such step: its GPU work lived in child Python
 * processes, train_server.py:12.)  A process that shares the runtime with another library (Python + torch) must NOT
 * call this. */
int prv_runtime_shutdown(void);
int prv_synchronize(prv_ctx* ctx);
int prv_device_count(void);
/* method 5's ranking key is  -PSNR_dB + weight * mean_pixels((1 - alpha)^2) : the worst-reconstructed and
 * least-covered view first.  The second term is the reference's own density term ((1 - mean_density)^2 per
 * pixel, main.cpp:2148, added with weight 1 to the colour term of method 3), here the mean over the view's
 * pixels so that it does not depend on the image size.  weight 0 ranks by PSNR alone. */
int prv_set_coverage_weight(prv_ctx* ctx, double weight);

/* Per-kernel timing with HIP events on the context's stream (for roofline accounting):
 * between begin and end every march_compact and render_queue launch is bracketed by an
 * event pair.  end synchronises and returns summed durations and launch counts. */
int prv_profile_begin(prv_ctx* ctx);
int prv_profile_end(prv_ctx* ctx, double* render_ms, int* render_launches, double* march_ms,
                    int* march_launches);
/* the render launches of the window prv_profile_end closed last, one duration (ms) each in launch order -- the scoring
 * round of an E-member ensemble launches E per round, member 0 first (main.cpp:2041-2043: one run.py per member).
 * Returns their number (>= 0; ms may be NULL or hold fewer than that) or an error code. */
int prv_profile_render_launches(prv_ctx* ctx, float* ms, int capacity);

/* thin device-memory helpers so a C/C++ host needs no HIP headers */
int prv_malloc(prv_ctx* ctx, void** dev_ptr, size_t bytes);
int prv_free(prv_ctx* ctx, void* dev_ptr);
int prv_memcpy_h2d(prv_ctx* ctx, void* dev_dst, const void* host_src, size_t bytes);
int prv_memcpy_d2h(prv_ctx* ctx, void* host_dst, const void* dev_src, size_t bytes);

/* ---- model --------------------------------------------------------------- */
/* element counts of the three parameter arrays for a descriptor */
int prv_model_sizes(const prv_field_desc* desc, uint64_t* table_halfs, uint64_t* mlp_halfs,
                    uint64_t* occ_words);
/* replaces: testbed.load_snapshot / the trained network state (run.py:123-129, 185-208).
 * host pointers; table = fp16 bit patterns, level-major; mlp = canonical [in][out] fp16,
 * layers density-1, density-2, rgb-1, rgb-2, rgb-3; occ = occ_res^3 bits, x fastest. */
int prv_model_load(prv_ctx* ctx, int slot, const prv_field_desc* desc, const uint16_t* table,
                   const uint16_t* mlp, const uint32_t* occ);
/* deterministic synthetic field (counter-based RNG), generated on the device */
int prv_model_synthetic(prv_ctx* ctx, int slot, const prv_field_desc* desc, uint64_t seed);
/* a field to start training from (replaces the network reset of a new Testbed, run.py:90): the same
 * counter-RNG parameters as prv_model_synthetic -- table ~ U(-table_amp, table_amp), use 1e-4 as upstream
 * does; Xavier-uniform MLP -- with EVERY occupancy cell set */
int prv_model_fresh(prv_ctx* ctx, int slot, const prv_field_desc* desc, uint64_t seed);
int prv_model_export(prv_ctx* ctx, int slot, uint16_t* table, uint16_t* mlp, uint32_t* occ);
/* replaces: testbed.save_snapshot / load_snapshot (run.py:123-127, 210-211).  File = "PRVF" magic,
 * ABI version, prv_field_desc, then table / mlp / occupancy arrays in the canonical layout. */
int prv_model_save_file(prv_ctx* ctx, int slot, const char* path);
int prv_model_load_file(prv_ctx* ctx, int slot, const char* path);
/* replaces: testbed.load_snapshot(<file>.ingp | .msgpack) / save_snapshot (run.py:123-127, 210-211) for snapshots
 * written by instant-ngp itself -- the weights BASELINE configs[2] names.  Reads the msgpack (gzip-compressed for
 * .ingp) network config + "snapshot" {params_binary fp16, density_grid_binary, nerf.aabb_scale}, maps tiny-cuda-nn's
 * parameter order (density MLP | rgb MLP | hash grid; FullyFusedMLP matrices [out][in], outputs padded to 16) to the
 * canonical layout above and the density grid (Morton order, optical thickness) to the occupancy bits; the level
 * geometry follows the file's per_level_scale (prv_field_desc.per_level_scale).  Anything this build cannot
 * represent is refused with PRV_E_INVALID and a message (aabb_scale != 1, L*F != 32, other MLP shapes, ...).
 * LAYOUT ASSUMED FROM UPSTREAM, UNPINNED: neither instant-ngp nor a snapshot exists in the reference tree or the
 * build container; save_ingp is the exact inverse and the pair is tested against an independent Python writer. */
int prv_model_load_ingp(prv_ctx* ctx, int slot, const char* path);
int prv_model_save_ingp(prv_ctx* ctx, int slot, const char* path);
/* the descriptor of the field in a slot (e.g. of a snapshot just loaded) */
int prv_model_desc(prv_ctx* ctx, int slot, prv_field_desc* out);

/* ---- cameras ------------------------------------------------------------- */
/* replaces: json.load(--screenshot_transforms) + set_nerf_camera_matrix + fov from
 * camera_angle_x (run.py:132-135, 285-286, 294-296).  Reads camera_angle_x, w, h, scale,
 * offset and frames[].transform_matrix of a transforms.json written by the planner
 * (main.cpp:1793-1811, 1885-1924). */
int prv_cameras_from_json(prv_ctx* ctx, const char* path, prv_camset** out);
/* same, from memory: tm = n row-major 4x4 transform_matrix */
int prv_cameras_from_matrices(prv_ctx* ctx, const double* tm, int n, double camera_angle_x,
                              int width, int height, double scale, const double offset[3],
                              prv_camset** out);
/* The cameras of a DATASET json, as the engine sees its training / test views: replaces
 * testbed.load_training_data(--test_transforms) + set_camera_to_training_view(i) with
 * render_with_lens_distortion (run.py:145, 238, 242) -- the per-file intrinsics the planner writes at
 * main.cpp:1585-1602 (fl_x, fl_y, cx, cy, w, h; k1, k2, p1, p2 read BY KEY = the yaml's color_k1, color_k2,
 * color_p1, color_p2; k3 is written too but is not a term of the engine's OpenCV lens and is ignored).  Missing fl_* fall
 * back to camera_angle_*, missing cx, cy to the image centre, missing lens terms to 0.  Rendering at
 * another size than (w,h) scales fl and the principal point per axis. */
typedef struct prv_intrinsics {
  double fl_x, fl_y, cx, cy; /* pixels, at (w,h) */
  double k1, k2, p1, p2;     /* OpenCV radial / tangential terms on normalised coordinates */
  int32_t w, h;
} prv_intrinsics;
int prv_cameras_from_dataset_json(prv_ctx* ctx, const char* path, prv_camset** out);
int prv_cameras_from_matrices_intr(prv_ctx* ctx, const double* tm, int n, const prv_intrinsics* intr,
                                   double scale, const double offset[3], prv_camset** out);
/* lens terms {k1,k2,p1,p2} of camera i (all 0 for the screenshot-style sets above) */
int prv_camset_lens(const prv_camset* cs, int i, float lens[4]);
int prv_camset_count(const prv_camset* cs);
int prv_camset_size(const prv_camset* cs, int* width, int* height);
/* engine-frame camera i: c2w[12] row-major 3x4, intr = {fx, fy, cx, cy} at the json w,h */
int prv_camset_get(const prv_camset* cs, int i, float c2w[12], float intr[4]);
void prv_camset_destroy(prv_camset* cs);

/* ---- render -------------------------------------------------------------- */
/* replaces: testbed.render(w, h, spp, linear=True) per frame (run.py:245-247, 304).
 * out_rgba_dev: n_views * h * w * 4 float32, linear premultiplied RGBA, NO background. */
int prv_render(prv_ctx* ctx, int model_slot, const prv_camset* cs, const int* view_ids, int n_views,
               const prv_render_opts* opts, float* out_rgba_dev, prv_stats* stats);
/* replaces: write_image(outname, image) PNG bytes (run.py:309) -- composited over
 * opts->background, un-premultiplied, sRGB, 8 bit.  out: n_views*h*w*4 uint8 (dev). */
int prv_render_rgba8(prv_ctx* ctx, int model_slot, const prv_camset* cs, const int* view_ids,
                     int n_views, const prv_render_opts* opts, uint8_t* out_rgba8_dev,
                     prv_stats* stats);
/* replaces: testbed.render_mode = ngp.Depth; testbed.render(w, h, spp, True) (run.py:287-288, 304).
 * out_depth_dev: n_views*h*w float32, premultiplied z-depth in engine units:
 *   per ray (every spp sub-sample), over exactly the samples, weights and early termination prv_render composites,
 *   D = sum_i w_i t_i (w_i = alpha_i T_i, the sample's colour weight; t_i = fmaf(i + 0.5, dt, t0), its ray parameter:
 *   directions are unit length from the camera centre, so t_i is a distance), and z = D * dot(d, f), f = the view's
 *   forward axis (column 2 of its engine-frame c2w, normalised; lens cameras too): depth along the optical axis,
 *   premultiplied by opacity like the colour channels.  The pixel is the mean of its sub-samples (summed in order, then
 *   scaled by 1/spp); rays that miss the box or have no live sample give exactly 0.  Engine units (the unit cube):
 *   dataset units = engine / scale.  ASSUMED (the engine is not in the reference tree): upstream's Depth mode outputs
 *   camera-axis depth composited like colour.
 * out_rgba_dev: as prv_render (bit-identical to it), or NULL (rendered into a context scratch buffer). */
int prv_render_depth(prv_ctx* ctx, int model_slot, const prv_camset* cs, const int* view_ids, int n_views,
                     const prv_render_opts* opts, float* out_rgba_dev, float* out_depth_dev, prv_stats* stats);
/* The ray entropy of a view (this build's own: the engine has no such mode), from one model and no reference image.
 * out_entropy_dev: n_views*h*w float32, bits.  Per ray (every spp sub-sample), over exactly the samples, weights and early
 *   termination prv_render composites, under either stepping rule:
 *     w_i = alpha_i T_i, the sample's colour weight (the colour kernel's bits);
 *     T_end = the transmittance when the ray stops: after its last sample, or at the min_transmittance cut;
 *     H = sum_i h(w_i) + h(T_end),  h(p) = p >= 2^-126 ? -p log2(p) : 0  (denormal p count as 0),
 *   accumulated in depth order as H = fmaf(p, -log2 p, H), the escape term last.  The w_i and T_end sum to 1: H is the
 *   entropy of "where does this ray end" over its samples plus "it escapes"; 0 for a ray that surely escapes or surely
 *   stops at one sample, large where the field spreads the stop over many samples.  A ray that misses the box or has no
 *   live sample gives exactly 0 (T_end = 1).  The pixel is the sum of its sub-samples in order, times 1/spp, as for depth.
 *   H depends on the stepping rule's dt like any discretised entropy (halving dt splits every weight in two: up to one bit
 *   more): values compare between the views of one call, not between stepping rules or sample counts.
 * out_alpha_dev: n_views*h*w float32, the pixel's opacity 1 - T_end, bit-identical to prv_render's alpha channel; may be
 *   NULL.  stats: as prv_render's for the same views.  No colour is evaluated: the density layers alone run. */
int prv_render_entropy(prv_ctx* ctx, int model_slot, const prv_camset* cs, const int* view_ids, int n_views,
                       const prv_render_opts* opts, float* out_entropy_dev, float* out_alpha_dev, prv_stats* stats);
/* prv_render_rgba8's byte rule alone, on n_pixels linear premultiplied RGBA float32 pixels (dev): composite over bg,
 * un-premultiply (by the composite alpha, unless that is 0), sRGB, clamp, * 255 + 0.5, truncate; the alpha byte from the
 * clamped composite alpha.  The clamp is fminf(fmaxf(v, 0), 1), and fmaxf returns its other operand when one is a NaN:
 * a NaN (a NaN input, 0 * Inf, Inf - Inf, Inf / Inf along the way) gives byte 0, -0.0 and -Inf give 0, +Inf gives 255.
 * The images of prv_score_psnr_images and prv_evaluate_images pass through the same clamp: a non-finite COLOUR counts as
 * 0 (or 1), only a non-finite alpha reaches the coverage sums. */
int prv_quantize_rgba8(prv_ctx* ctx, const float* rgba_dev, size_t n_pixels, const float bg[4],
                       uint8_t* out_rgba8_dev);
/* Entropy, opacity and depth of the same views from ONE density-only launch (this build's own; what the selection stage below
 * consumes): the entropy kernel's density layers plus the depth kernel's one FMA per sample, D = fmaf(w_i, t_i, D), and
 * z = D * dot(d, f) at ray end.  No colour is evaluated.  All three planes are n_views*h*w float32 and all three are required.
 * CONTRACT: out_entropy_dev and out_alpha_dev are bit-identical to prv_render_entropy's, out_depth_dev is bit-identical to
 * prv_render_depth's depth plane, stats are identical to both, for the same views and options (either stepping rule, any spp:
 * each plane is reduced over its sub-samples in order, then scaled by 1/spp). */
int prv_render_footprint(prv_ctx* ctx, int model_slot, const prv_camset* cs, const int* view_ids, int n_views,
                         const prv_render_opts* opts, float* out_entropy_dev, float* out_alpha_dev, float* out_depth_dev,
                         prv_stats* stats);
/* Entropy, opacity and a FIRST-CROSSING depth of the same views from one density-only launch (this build's own; the opt-in
 * locator of the selection stage below, the "median depth" of the NeRF toolkits at level 0.5).  Per ray (every spp sub-sample),
 * over exactly the samples and early termination prv_render_entropy walks, with T_i' = T after sample i (T * (1 - alpha_i)):
 *   Dm = t_i of the first sample with T_i' <= 1.0f - level (one float32 subtraction on the host, one compare per sample),
 *        or 0 when the ray ends above that; t_i > 0 for every sample, so Dm > 0 says the level was reached;
 *   z = Dm * dot(d, f), the forward cosine exactly as prv_render_depth forms it;  hit = Dm > 0 ? 1 : 0.
 * Unlike the expected depth, z always lies on a sample at which the ray really stops.  All four planes are n_views*h*w
 * float32 and all four are required.  The pixel of each plane is the sum of its sub-samples in order, times 1/spp: out_depth_dev
 * is the mean over ALL sub-samples of z (0 where the sub-sample did not hit), out_hit_dev the share of sub-samples that hit, so
 * depth / hit is the mean z over those that did.  Rays that miss the box or have no live sample give exactly 0 in all four.
 * CONTRACT: out_entropy_dev and out_alpha_dev are bit-identical to prv_render_entropy's and stats are identical to its stats,
 * for the same views and options; out_depth_dev and out_hit_dev are as defined above for either stepping rule and any spp.
 * Errors (PRV_E_INVALID with a message): level not in (0, 1) or NaN; 1.0f - level < opts->min_transmittance (the ray could be
 * cut before it can cross); a NULL or host plane. */
int prv_render_surface(prv_ctx* ctx, int model_slot, const prv_camset* cs, const int* view_ids, int n_views,
                       const prv_render_opts* opts, float level, float* out_entropy_dev, float* out_alpha_dev,
                       float* out_depth_dev, float* out_hit_dev, prv_stats* stats);
/* The ray-termination histogram of a view (this build's own): WHERE along the ray its samples' weights lie, over positions that
 * do not depend on the field, so the histograms of different models line up bin for bin.  One density-only launch, like
 * prv_render_entropy; no colour is evaluated.  Per ray (every spp sub-sample), over exactly the samples, weights w_i = alpha_i T_i
 * and early termination prv_render_entropy walks:
 *     bin(i) = (uint32)(i * M) >> 16,  M = floor(n_bins * 65536 / n_max),  i = the sample's step index (t_i = fmaf(i + 0.5, dt, t0)),
 *     n_max = opts->samples_per_ray under PRV_STEP_FIXED_S, 1024 under PRV_STEP_NGP (there a plain shift): n_bins equal
 *     stretches of the ray's unit-cube span, bin(i) < n_bins for every i < n_max (the kernel also takes min(bin, n_bins - 1): a
 *     guard that changes no bin of such a step and keeps any other inside the planes);
 *     out_bins[k] = the sum of the w_i with bin(i) = k, float32 adds in depth order, starting from 0.
 * out_bins_dev: n_bins planes of n_views*h*w float32, plane k at out_bins_dev + k * n_views*h*w; required.  n_bins: a power of
 *   two in [4, 64].  The bins and the escape 1 - alpha sum to 1 within n_bins + 1 roundings.  The pixel of every plane is the
 *   sum of its sub-samples in order, times 1/spp.  Rays that miss the box or have no live sample, and bins no live sample of
 *   the ray falls in, give exactly 0.
 *   The values depend on n_bins and on the stepping rule (which samples exist and which bin they fall in): they compare between
 *   models and views of one set of options, not across them.
 * out_alpha_dev: n_views*h*w float32, the pixel's opacity; may be NULL.
 * CONTRACT: out_alpha_dev and stats are bit-identical to prv_render_entropy's for the same call.
 * Errors (PRV_E_INVALID with a message): n_bins not a power of two in [4, 64]; a NULL out_bins_dev; a host pointer. */
int prv_render_termination(prv_ctx* ctx, int model_slot, const prv_camset* cs, const int* view_ids, int n_views,
                           const prv_render_opts* opts, int n_bins, float* out_bins_dev, float* out_alpha_dev, prv_stats* stats);
/* The Jensen-Shannon divergence between n_models termination histograms, per pixel, and its mean per view: the reduce of
 * PRV_SCORE_TERMINATION_JSD alone, on planes the caller holds (prv_render_termination's, one call per model with the same views
 * and options).  bins_dev[e]: n_bins planes of n_views*width*height float32; alpha_dev[e]: n_views*width*height float32.
 * Per pixel, with p_e[k] (k < n_bins) member e's bins and p_e[n_bins] = 1.0f - alpha_e its escape, all float32 in this order:
 *     m_k = (p_0[k] + p_1[k] + ... + p_{E-1}[k]) * (1.0f / E)                 (members in argument order)
 *     h(p) = p >= 2^-126 ? -p log2(p) : 0                                     (prv_render_entropy's h and hardware log)
 *     A = sum_k h(m_k),  B_e = sum_k h(p_e[k])                                (k ascending, each term one fmaf as there)
 *     J = max(A - (B_0 + ... + B_{E-1}) * (1.0f / E), 0)                      bits
 * J = H(mean of the members) - mean of the members' H: 0 where the members agree however spread the ray is (exactly 0.0 for two
 * identical members), at most log2(E) where they stop in different places.
 * out_jsd_dev: n_views*width*height float32 J, or NULL.  view_jsd_host / view_opacity_host: n_views doubles each, the view's
 * mean J and the mean over members and pixels of alpha (per pixel (a_0 + ... + a_{E-1}) * (1.0f / E) in float32; the sums over
 * pixels in fp64, block partials summed in block order: deterministic); either may be NULL.
 * Errors (PRV_E_INVALID with a message): n_models outside 2..PRV_MAX_MODELS; n_bins as above; a NULL or host plane. */
int prv_termination_divergence(prv_ctx* ctx, const float* const* bins_dev, const float* const* alpha_dev, int n_models,
                               int n_views, int width, int height, int n_bins, float* out_jsd_dev, double* view_jsd_host,
                               double* view_opacity_host);

/* replaces: Perception_3D::precept / precept_thread_process, the reference's CPU render path
 * (main.cpp:98-284: project -> ray -> OctoMap castRay, max range main.cpp:258).  Per pixel the
 * first occupied voxel of the model's occupancy grid along the ray: out_cell_dev[n_views*h*w] =
 * x + R*(y + R*z), or -1 for no hit within max_range (in unit-cube units). */
int prv_first_hit(prv_ctx* ctx, int model_slot, const prv_camset* cs, const int* view_ids, int n_views,
                  int width, int height, float max_range, int32_t* out_cell_dev);

/* The reference's camera intrinsics (rs2_intrinsics, Share_Data.hpp:79-89); coeffs in the YAML order
 * k1,k2,k3,p1,p2 (Share_Data.hpp:395-399); model 2 = inverse Brown-Conrady (yaml color_model). */
typedef struct prv_rs2_intrinsics {
  int32_t width, height;
  float ppx, ppy, fx, fy;
  int32_t model;
  float coeffs[5];
} prv_rs2_intrinsics;
/* replaces: Perception_3D::precept + precept_thread_process (main.cpp:98-284) in full: for every
 * ground-truth voxel centre, rs2_project_point_to_pixel -> cull -> integer pixel ->
 * project_pixel_to_ray_end (rs2_deproject_pixel_to_point at depth 1, Share_Data.hpp:719-726) ->
 * castRay from the camera within max_range.  voxels_dev = n x 3 float (unit-cube coordinates),
 * c2w = camera-to-world 4x4 row-major double (+Z forward, the reference's view_pose_world).
 * out_cell_dev[n] = first occupied cell x + R*(y + R*z), or -1 (culled / no hit). */
int prv_precept(prv_ctx* ctx, int model_slot, const float* voxels_dev, int n, const double c2w[16],
                const prv_rs2_intrinsics* intr, float max_range, int32_t* out_cell_dev);

/* ---- scores -------------------------------------------------------------- */
/* replaces: the per-view loops main.cpp:2045-2094 (method 2) / 2105-2158 (method 3).
 * imgs_dev[e] = n_views*pixels_per_view*4 uint8 of ensemble member e. */
int prv_score_ensemble_images(prv_ctx* ctx, int method, const uint8_t* const* imgs_dev,
                              int n_members, int n_views, size_t pixels_per_view,
                              prv_score_record* records_host);
/* replaces: run.py:257-263 per image.  score = -psnr + coverage weight * mean((1 - alpha)^2), see
 * prv_set_coverage_weight (worst-reconstructed, least-covered view first). */
int prv_score_psnr_images(prv_ctx* ctx, const float* rgba_dev, const float* gt_rgba_dev,
                          int n_views, size_t pixels_per_view, const float bg[4],
                          prv_score_record* records_host);
/* replaces: the per-image metrics of the evaluation block, run.py:257-267:
 *   A,R = clip(srgb(img)), mse -> psnr = -10 log10(mse), ssim = SSIM(A,R)   (SSIM recipe assumed from
 *   instant-ngp's scripts/common.py, which the reference does not vendor).
 * Images: n_views * h * w * 4 float (dev).  psnr_host / ssim_host: n_views doubles each. */
int prv_evaluate_images(prv_ctx* ctx, const float* rgba_dev, const float* gt_rgba_dev, int n_views,
                        int width, int height, const float bg[4], double* psnr_host, double* ssim_host);
/* replaces: the evaluation loop run.py:240-277 for one model: render every listed view at opts,
 * compare with the reference images, return the MEAN of the per-image PSNRs and SSIMs (run.py:271-272;
 * what --save_metrics writes as "PSNR\t..\nSSIM\t..", consumed at main.cpp:1957-1961). */
int prv_evaluate(prv_ctx* ctx, int model_slot, const prv_camset* cs, const int* view_ids, int n_views,
                 const prv_render_opts* opts, const float* gt_rgba_dev, double* mean_psnr, double* mean_ssim);

/* The whole scoring round of nbv_loop for one shard of views, on the device end to end:
 * render every view with every model slot listed, reduce to one record per view.
 *   methods 2,3: model_slots = the ensemble (main.cpp:2041-2043 + 2045-2094);
 *   method 5   : model_slots[0] vs gt_rgba_dev (n_views*h*w*4 float, same view order);
 *   method 7   : model_slots[0] alone (n_models == 1, gt_rgba_dev NULL): score = the mean over the view's pixels of
 *                prv_render_entropy's H in fp64 (block partials summed in block order: deterministic), coverage = the mean
 *                opacity, psnr = 0.  The march and the entropy kernel are the round's only render launches; no colour image.
 *   method 9   : model_slots = the ensemble (2..8 models, gt_rgba_dev NULL): score = the view's mean J of
 *                prv_termination_divergence over the members' prv_render_termination planes at PRV_TERMINATION_BINS_DEFAULT
 *                bins (fp64, deterministic), coverage = the mean over members and pixels of the opacity, psnr = 0.  The members
 *                are rendered one after another per batch of views (E density-only launches, no colour image), then reduced;
 *                only one batch's planes are resident.  Scores compare between the views of one call: the bin count and the
 *                stepping rule change them.
 * records_host and/or records_dev (n_views records) receive the result; records_dev is
 * what a caller hands to its all-gather. */
int prv_score_views(prv_ctx* ctx, int method, const int* model_slots, int n_models,
                    const prv_camset* cs, const int* view_ids, int n_views,
                    const prv_render_opts* opts, const float* gt_rgba_dev,
                    prv_score_record* records_host, prv_score_record* records_dev,
                    prv_stats* stats);
/* replaces: the arg-max bookkeeping main.cpp:1971-1972, 2088-2091, 2096.
 * order = view ids sorted by (score descending, id ascending), NaN scores after every number (the reference's
 * strict '>' never selects a NaN either); host only. */
int prv_rank(const prv_score_record* records, const int* view_ids, int n, int* order);
int prv_argmax(const prv_score_record* records, const int* view_ids, int n);

/* ---- several next views per round: greedy, redundancy-aware selection ---------- */
/* replaces: nothing in the reference -- it adds ONE view per training round (main.cpp:1971-1972).  This build's own: choose k
 * views of a round's candidates so that a later choice is not paid for what an earlier one already sees.  The k best by
 * score do not do that: neighbouring candidates with high ray entropy look at the same unfinished part of the object.
 * Inputs are the three planes of prv_render_footprint for the candidates (width x height each).  Every float operation below
 * is one IEEE float32 operation in the order written, so a float32 restatement is bit-exact.  For pixel (x, y) of view v,
 * with H, alpha, z its entropy, opacity and depth:
 *   gain      q = H > 0 ? (uint32) min(floorf(H * 65536.0f), 4294967040.0f) : 0        (NaN or negative H: 0)
 *   located   iff alpha >= alpha_min and z > 0 (a NaN fails either)
 *   point of a located pixel:
 *     (o, d) = the ray generator's ray of that pixel at sub-sample 0 of a 1-spp render (prv_debug_raygen, spp_index 0);
 *     c = fmaf(d0, fx, fmaf(d1, fy, d2 * fz)) * (1.0f / sqrtf(fmaf(fx, fx, fmaf(fy, fy, fz * fz)))), (fx, fy, fz) = column 2 of
 *         the view's engine-frame c2w: the forward cosine exactly as the depth kernel forms it;
 *     t = (z / alpha) / c                      two IEEE divisions
 *     p_a = o_a + (t * d_a)                    a float32 multiply, then a float32 add: NO FMA
 *     f_a = floorf(p_a * G), G = (float)grid_res; if any f_a is not in [0, G) (NaN included) the pixel is unlocated after
 *     all; otherwise g_a = (int)f_a and voxel = g_x + G * (g_y + G * g_z).  Unlocated pixels carry 0xFFFFFFFF.
 *   greedy rounds: C = a set of voxels (G^3 bits), empty at the start.  k times:
 *     for every view not yet chosen  gain_i = sum over its pixels of q * [unlocated or voxel not in C], an exact uint64 sum;
 *     the view with the largest gain is chosen, on a tie the one that comes first in view_ids;
 *     the voxels of that view's located pixels are added to C.
 *   Unlocated pixels are never discounted, so round 1 ranks the candidates as PRV_SCORE_RAY_ENTROPY does, up to the 2^-16 bit
 *   quantisation of q.
 * chosen_out[j] (host, k ints) = the view id chosen in round j (view_ids[i], or i when view_ids is NULL); gains_out[j] (host, k
 * uint64, may be NULL) = its gain in that round.  voxel_dev / q_dev (device, n_views*h*w uint32 each, optional) receive the
 * per-pixel words.  The sums are integer atomics (order-independent) and the arg-max is taken on the host from a read-back of
 * the n_views sums per round: two calls return identical bytes.  Synchronises.
 * Errors: k < 1, k > n_views, grid_res not a power of two in [16, 256], a NULL or host plane: PRV_E_INVALID with a message.
 * WITH THE SURFACE LOCATOR (prv_select_views_surface, or prv_render_surface's hit plane handed in as alpha_dev and its depth as
 * depth_dev) nothing above changes but what the words mean: "located" is then: the hit fraction is at least alpha_min and
 * z > 0, and the point is at t = (z / hit) / c, the mean first-crossing depth of the sub-samples that reached the level.  At
 * 1 spp with level 0.5 and the default alpha_min the located pixels are the ones the expected-depth locator locates
 * (1 - T_end >= 0.5), up to rays whose final T rounds onto 1/2; only WHERE they are located changes.
 * LIMITS: the expected depth z / alpha is a poor locator on rays whose weights are spread widely (exactly the high-entropy rays:
 * the point then lies between the surfaces the ray may stop at) -- the surface locator is the opt-in answer to that, the
 * default stays the expected depth; coverage is binary (a voxel seen once counts as seen, from
 * whatever angle); the stage is SINGLE-RANK: it needs every candidate's planes on one device, a sharded variant (all-gather of
 * voxel / q words, or of bitsets) is out of scope here. */
typedef struct prv_select_opts {
  int32_t k;        /* views to choose, 1..n_views */
  int32_t grid_res; /* G: power of two, 16..256, default 64 */
  float alpha_min;  /* default 0.5 */
} prv_select_opts;
int prv_select_default_opts(prv_select_opts* opts); /* k 1, grid_res 64, alpha_min 0.5 */
int prv_select_from_images(prv_ctx* ctx, const prv_camset* cs, const int* view_ids, int n_views, int width, int height,
                           const float* entropy_dev, const float* alpha_dev, const float* depth_dev,
                           const prv_select_opts* opts, int* chosen_out, uint64_t* gains_out, uint32_t* voxel_dev,
                           uint32_t* q_dev);
/* prv_render_footprint of the views into context scratch, then prv_select_from_images on those planes at the render's size;
 * stats: the render's */
int prv_select_views(prv_ctx* ctx, int model_slot, const prv_camset* cs, const int* view_ids, int n_views,
                     const prv_render_opts* render_opts, const prv_select_opts* opts, int* chosen_out, uint64_t* gains_out,
                     prv_stats* stats);
/* prv_render_surface of the views at `level` into context scratch, then prv_select_from_images with its hit plane as alpha_dev
 * and its depth plane as depth_dev; stats: the render's.  Errors: prv_select_views' and prv_render_surface's. */
int prv_select_views_surface(prv_ctx* ctx, int model_slot, const prv_camset* cs, const int* view_ids, int n_views,
                             const prv_render_opts* render_opts, float level, const prv_select_opts* opts, int* chosen_out,
                             uint64_t* gains_out, prv_stats* stats);

/* replaces: Perception_3D::render (the PCL screenshot of the coloured ground-truth cloud with
 * points_size_cloud-pixel points on white, main.cpp:68-96) + convertToAlpha (Share_Data.hpp:771-784) +
 * cv::flip(-1) (main.cpp:1616) = the rgbaClip_<i>.png training images of get_coverage (main.cpp:1604-1618),
 * as a z-buffered square-splat rasteriser.  xyz_dev n*3 floats in world units, rgb_dev n*3 bytes; scale /
 * offset = the json's (the cloud goes where the cameras go); cameras = the dataset's.  out: n_views*h*w*4
 * RGBA bytes (device): nearest point's colour, alpha 255; background and exactly-white points 255,255,255,0. */
int prv_splat_points(prv_ctx* ctx, const float* xyz_dev, const uint8_t* rgb_dev, size_t n_points, double scale,
                     const double offset[3], const prv_camset* cs, const int* view_ids, int n_views, int width,
                     int height, int point_size, int flip180, uint8_t* out_rgba8_dev);

/* ---- mesh extraction ------------------------------------------------------- */
/* replaces: testbed.compute_and_save_marching_cubes_mesh(path, [res, res, res]) (run.py:59-60, 279-282).
 * A grid of res[0] x res[1] x res[2] points over [aabb_lo, aabb_hi] (engine frame), x fastest: point i on axis a at
 * lo[a] + (float)i * step[a], step[a] = (hi[a] - lo[a]) / (float)(res[a] - 1).  sigma = the field's density at each point;
 * a corner is inside iff sigma > threshold (strict; NaN is outside).  sigma may hold infinities and NaNs: a vertex sits at
 * pa + t * (pb - pa), t = (threshold - sa) / (sb - sa), and a NaN t (an infinite or NaN end, or a difference that overflows;
 * on a crossing edge nothing else leaves [0, 1]) is replaced by 0.5; a normal whose squared length is 0, infinite or NaN is
 * (0, 0, 0).  Every vertex and normal is therefore finite, and every vertex lies on its grid edge.
 * Vertices come in edge-id order (3 * point + axis), triangles in cell order, counter-clockwise seen from outside (lower
 * sigma); normals = -grad sigma, normalised; colours = the full field at the vertex seen from outside (direction -normal),
 * quantised as an opaque pixel (prv_quantize_rgba8).  Everything is deterministic: two runs give identical bytes.  A grid without a surface is not an error (0 vertices). */
typedef struct prv_mesh prv_mesh; /* owns its device buffers; inert (PRV_E_STATE, not a crash) if it outlives its context */
typedef struct prv_mesh_opts {
  int32_t res[3];               /* grid points per axis, 2..1024 each, product <= 2^30 */
  float aabb_lo[3], aabb_hi[3]; /* engine frame, 0 <= lo < hi <= 1; default the unit cube (upstream's render_aabb) */
  float threshold;              /* sigma iso-level, default 2.5 (instant-ngp's default) */
  int32_t use_occupancy;        /* default 0 = every point evaluated; 1: sigma = 0 where the occupancy bit is clear */
  int32_t colors;               /* default 1 */
} prv_mesh_opts;
int prv_mesh_default_opts(prv_mesh_opts* o); /* res 256^3, unit cube, threshold 2.5, no occupancy, colours */
/* sigma_dev: res[0]*res[1]*res[2] float32 (device), x fastest */
int prv_density_grid(prv_ctx* ctx, int model_slot, const prv_mesh_opts* o, float* sigma_dev);
int prv_marching_cubes(prv_ctx* ctx, int model_slot, const prv_mesh_opts* o, prv_mesh** out);
/* marching cubes on a caller's sigma grid (device, layout of prv_density_grid); no colours (rgb reads as 0) */
int prv_marching_cubes_grid(prv_ctx* ctx, const float* sigma_dev, const prv_mesh_opts* o, prv_mesh** out);
/* the same on a grid of which only some points are known.  valid_dev: one byte per grid point (device, the grid's layout), 0 =
 * not valid; NULL: every point is valid, the call IS prv_marching_cubes_grid, byte for byte.  A cell is KEPT iff all eight of
 * its corners are valid.  Triangles come from kept cells only, in cell order; a grid edge gives a vertex iff it crosses and at
 * least one of the (up to four) cells around it is kept, so no vertex is unused and vertices stay in edge-id order.  Positions
 * and normals are computed as above (a normal whose gradient meets a NaN neighbour is (0, 0, 0) by the rule above).  The result
 * is what prv_marching_cubes_grid gives with the triangles of the other cells dropped and the then-unused vertices removed. */
int prv_marching_cubes_grid_valid(prv_ctx* ctx, const float* grid_dev, const uint8_t* valid_dev, const prv_mesh_opts* o, prv_mesh** out);
int prv_mesh_counts(const prv_mesh* m, uint64_t* n_vertices, uint64_t* n_triangles);
/* host arrays: xyz / normals n_vertices*3 floats, rgb n_vertices*3 bytes, tri n_triangles*3 vertex ids; any may be NULL */
int prv_mesh_get(const prv_mesh* m, float* xyz, float* normals, uint8_t* rgb, uint32_t* tri);
/* Files are written in the dataset (transforms.json) frame: engine position e -> q = (e2, e0, e1) -> (q - offset) / scale,
 * the inverse of nerf_to_ngp (cameras) and prv_splat_points; normals get the same axis cycle (an even permutation: the
 * winding is kept).  By extension: .ply = binary_little_endian 1.0, float x y z nx ny nz, uchar red green blue, faces
 * `list uchar int vertex_indices`; .obj = ASCII `v x y z r g b` (colours in [0,1]), `vn`, `f a//a b//b c//c` (1-based).
 * Any other extension: PRV_E_INVALID.  offset NULL = (0, 0, 0). */
int prv_mesh_save(const prv_mesh* m, const char* path, double scale, const double offset[3]);
/* the writer alone, on host arrays (no GPU; rgb / normals may be NULL: written as 0); errors via prv_last_error(NULL) */
int prv_mesh_write_file(const char* path, uint64_t n_vertices, const float* xyz, const float* normals, const uint8_t* rgb,
                        uint64_t n_triangles, const uint32_t* tri, double scale, const double offset[3]);
void prv_mesh_destroy(prv_mesh* m);

/* Connected components and floater removal.  Two vertices are connected if a triangle uses both; a component is a connected
 * set of vertices, and a vertex that no triangle uses is a component of its own with 0 triangles.  Components are numbered
 * by their smallest vertex id: component c is the one whose smallest vertex is the c-th smallest among them.  A triangle
 * belongs to the component of its first vertex.  The table's counts are integer sums and its box the per-axis minimum /
 * maximum of the component's vertices under the float order with -0 below +0 (every vertex of a mesh is finite), so labels
 * and table are bit-reproducible.  No area: a float sum over atomics would not be.
 * On the device: a union-find over 32-bit parents that are only ever lowered, hooked by one lane per triangle and compressed
 * by one lane per vertex, repeated until a hook pass changes nothing -- at most 64 rounds (PRV_E_INTERNAL beyond, never a
 * longer loop; a mesh takes 2).  No workgroup waits for another.
 * prv_mesh_filter keeps whole components and preserves the order of vertices and of triangles (ids remapped): the result
 * is what boolean-mask compaction of the arrays gives.  The rule, in this order:
 *   1. min_triangles > 0: only components with n_triangles >= min_triangles stay;
 *   2. keep_largest > 0: of those, only the keep_largest with the most triangles stay, equal counts to the lower id;
 *   3. min_diagonal > 0: of those, a component stays if its box's diagonal >= min_diagonal, the diagonal being
 *      sqrt((dx*dx + dy*dy) + dz*dz) in double, d = (double)hi - (double)lo, engine units.
 * Errors: NULL arguments, a negative or non-finite min_diagonal, a capacity below the count: PRV_E_INVALID; a mesh whose
 * context is gone: PRV_E_STATE.  An empty mesh has 0 components and filters to an empty mesh. */
typedef struct prv_mesh_component { /* 48 bytes */
  uint32_t first_vertex, reserved;  /* the component's smallest vertex id; 0 */
  uint64_t n_vertices, n_triangles;
  float lo[3], hi[3];               /* bounding box, engine frame */
} prv_mesh_component;
typedef struct prv_mesh_filter_opts {
  uint64_t min_triangles; /* keep components with at least this many; 0: no limit */
  uint32_t keep_largest;  /* then keep the k with the most triangles, ties to the lower component id; 0: all */
  float min_diagonal;     /* and drop boxes whose diagonal (engine units, computed in double from lo/hi) is below this */
} prv_mesh_filter_opts;
int prv_mesh_filter_default_opts(prv_mesh_filter_opts* o); /* all zero: the identity */
/* labels the mesh once; labels and table are cached on the handle and released with it */
int prv_mesh_components(prv_mesh* m, uint64_t* n_components);
/* the table in component order; capacity = entries out_host can take, at least the component count */
int prv_mesh_component_info(prv_mesh* m, uint64_t capacity, prv_mesh_component* out_host);
/* host arrays: one component id per vertex, one per triangle; either may be NULL */
int prv_mesh_labels(prv_mesh* m, uint32_t* vertex_component_host, uint32_t* triangle_component_host);
/* a new mesh of the same context (colours kept if the mesh has them); the input is unchanged */
int prv_mesh_filter(prv_mesh* m, const prv_mesh_filter_opts* o, prv_mesh** out);

/* ---- geometric evaluation: surface samples, nearest neighbours, Chamfer ----- */
/* replaces: nothing in the reference -- it judges a reconstruction through images only (run.py:257-272).  This build's
 * own: how close the reconstructed surface is to the real one, and how much of it is covered.
 *
 * prv_mesh_sample: n points on the mesh's surface, area-weighted, in the engine frame.  A pure function of (mesh, n, seed):
 *   two calls return identical bytes.  out_xyz_dev n*3 float32, out_tri_dev n triangle ids (may be NULL); n <= 2^31.
 *   Weights: a triangle's area in fp64 from its fp32 vertices -- e1 = b - a, e2 = c - a, c = e1 x e2 (each component
 *     y*z' - z*y' etc.), area = 0.5 * sqrt((cx*cx + cy*cy) + cz*cz) -- quantised to the integer w = floor(area * 2^40)
 *     (0 if that is below 1, not finite or >= 2^62): a res-256 cell's triangle (area ~ 2^-17) keeps 23 bits, a total of
 *     2^22 unit areas stays below 2^62.
 *   Scan: the weights are exclusive-scanned in integers (the mesh extraction's scan): no floating-point prefix sum, no
 *     order dependence.  W = their sum.
 *   Choice: sample k is stratified: its target lies in stratum k = [floor(k W / n), floor((k+1) W / n)) of length len, at
 *     offset floor(len * u48 / 2^48), u48 = (r0 << 24) | r1 from two 24-bit draws of the counter RNG, streams 0x5A0 and
 *     0x5A1, counter k (the RNG of prv_model_synthetic / the training sampler: mix64(seed + (stream + 1) * 0xD1B54A32D192ED03
 *     + k * 0x9E3779B97F4A7C15) >> 40).  The triangle is the last one whose exclusive prefix is <= target (binary search),
 *     so a zero-weight triangle is never chosen.
 *   Position: u = (float)r2 * 2^-24, v = (float)r3 * 2^-24 (streams 0x5A2, 0x5A3); if u + v > 1 (fp32): u = 1 - u,
 *     v = 1 - v; per axis p = (a + u * (b - a)) + v * (c - a), every operation its own fp32 rounding (no contraction).
 *   Errors: n == 0 or NULL / host pointers PRV_E_INVALID; a mesh without triangles or without area PRV_E_STATE. */
int prv_mesh_sample(const prv_mesh* m, uint64_t n, uint64_t seed, float* out_xyz_dev, uint32_t* out_tri_dev);

/* Nearest neighbours.  An index holds n reference points (device n*3 float32, any frame, any bounding box; copied: the
 * caller's array may go away).  A query of m points returns per query the squared distance to, and the id of, its nearest
 * reference point.  ARITHMETIC CONTRACT: dx = q.x - p.x, dy, dz in fp32; d2 = (dx*dx + dy*dy) + dz*dz (no contraction);
 * the minimum is over ALL reference points and on equal d2 the smallest id wins -- an order-independent result, bit-identical
 * to a brute-force float32 restatement whatever the search structure does.
 * PRV_NN_GRID (default): a uniform grid over the reference points' bounding box, about four points per cell (at most 2^23
 *   cells, 1024 per axis: prv_nn_index_info says whether a cap was hit; an axis thinner than a cell gets one layer, so planes,
 *   lines and a single repeated point work), built by counting sort (integer atomics, the mesh scan, a scatter).  A query
 *   is binned with the same grid, clamped to the border cell if outside; a wave takes 64 neighbouring queries, walks
 *   shells of cells outwards around them and stops when no unvisited cell can hold a nearer or equal point, by a bound that
 *   is conservative in fp32 (rounding may cost a visited shell, never a neighbour).
 * PRV_NN_BRUTE: every pair, tiled through LDS: the on-device check of the grid at sizes a CPU cannot reach.  Both
 *   return identical bytes.
 * Limits: 1 <= n, m <= 2^31; NaN / Inf coordinates on either side are refused with PRV_E_INVALID (a validation pass). */
#define PRV_NN_GRID 0
#define PRV_NN_BRUTE 1
typedef struct prv_nn_index prv_nn_index; /* owns its device buffers; inert (PRV_E_STATE) if it outlives its context */
typedef struct prv_nn_opts {
  int32_t algorithm; /* PRV_NN_GRID | PRV_NN_BRUTE */
  int32_t reserved;  /* 0 */
} prv_nn_opts;
int prv_nn_default_opts(prv_nn_opts* o);
int prv_nn_index_create(prv_ctx* ctx, const float* xyz_dev, uint64_t n, const prv_nn_opts* opts /* NULL: defaults */,
                        prv_nn_index** out);
/* out_d2_dev m float32, out_id_dev m uint32, in the caller's query order; synchronises */
int prv_nn_query(prv_nn_index* index, const float* query_xyz_dev, uint64_t m, float* out_d2_dev, uint32_t* out_id_dev);
/* points held, grid cells per axis (0 for PRV_NN_BRUTE), whether a cell cap was hit; any pointer may be NULL */
int prv_nn_index_info(const prv_nn_index* index, uint64_t* n, int32_t dims[3], int32_t* capped);
/* (query, reference) pairs whose distance the last prv_nn_query formed (PRV_NN_BRUTE: m * n) */
int prv_debug_nn_tests(const prv_nn_index* index, uint64_t* tests);
void prv_nn_index_destroy(prv_nn_index* index);

/* The accuracy / completeness / Chamfer / F-score family between a reconstruction's points and a reference's (device n*3
 * float32 each, the same frame).  Builds a grid index per side and queries both ways; per direction, on the device:
 * dist = the correctly rounded fp32 sqrt of the query's d2, widened to fp64; sums over a fixed grid of blocks, the
 * blocks' partials added in block order (deterministic run to run); dist <= tau counted in integers.
 * Distances are in the frame of the inputs, and so is tau: for engine-frame inputs divide the distances by the
 * transforms' `scale` (the squared ones by scale^2) to get dataset units, and pass tau * scale. */
typedef struct prv_geom_metrics {
  uint64_t n_rec, n_ref;
  double accuracy, completeness;       /* mean distance rec->ref, ref->rec */
  double accuracy_sq, completeness_sq; /* mean squared distances */
  double chamfer;                      /* (accuracy + completeness) / 2 */
  double precision, recall, fscore;    /* share of rec / ref points within tau; harmonic mean (0 if both are 0) */
  double hausdorff_rec, hausdorff_ref; /* largest distance each way */
} prv_geom_metrics;
int prv_geometry_metrics(prv_ctx* ctx, const float* rec_xyz_dev, uint64_t n_rec, const float* ref_xyz_dev, uint64_t n_ref,
                         float tau, prv_geom_metrics* out);
/* the same with the caller's index of the reference points (prv_nn_index_create on ref_xyz_dev, either algorithm): the
 * reference side is not indexed again -- a loop that compares every iteration against one reference builds it once.
 * ref_xyz_dev / n_ref must be the points the index was made of (n_ref is checked); identical results. */
int prv_geometry_metrics_indexed(prv_ctx* ctx, const float* rec_xyz_dev, uint64_t n_rec, prv_nn_index* ref_index,
                                 const float* ref_xyz_dev, uint64_t n_ref, float tau, prv_geom_metrics* out);

/* ---- surface coverage of a reference cloud by a set of views ------------------ */
/* replaces: nothing in the reference.  This build's own: the training-free ground truth of the next-best-view literature --
 * the share of a reference surface that a list of views sees, against the number of views, and what the greedy choice of as
 * many views out of the same set would have seen.  It prices a view choice without training a field on it.
 * Inputs: n_points points in the ENGINE frame (device n*3 float32: what prv_mesh_sample writes and prv_nn_index_create takes;
 * a dataset-frame cloud goes through q = fmaf(p, scale, offset), e = (q1, q2, q0) first, as prv_splat_points places it); n_views
 * views of a camset (view_ids NULL: cameras 0..n_views-1) at width x height, with the meaning prv_splat_points gives the size.
 * ARITHMETIC CONTRACT.  Every float operation below is one IEEE float32 operation in the order written (fmaf = one fused
 * multiply-add), so a float32 restatement is bit-exact.  M = the view's engine-frame c2w (3 x 4, row-major), o its column 3,
 * (fx, fy, cx, cy) its intrinsics at width x height, e the point.
 *   projection (prv_splat_points' own):
 *     d_a = e_a - o_a
 *     c_a = fmaf(M[0][a], d_0, fmaf(M[1][a], d_1, M[2][a] * d_2))                  a = 0, 1, 2
 *     it fails unless c_2 > 1e-6f (a NaN fails) and, for this stage, c_2 < +Inf
 *     x = c_0 / c_2, y = c_1 / c_2; a lens camera distorts them: (x, y) = lens_eval(x, y), the OpenCV model in the ray generator's order
 *     u = fmaf(fx, x, cx), v = fmaf(fy, y, cy), z = c_2
 *   stage A, depth buffers: one uint32 per pixel and view, 0xFFFFFFFF at the start.  With ps = (float)point_size:
 *     fx0 = floorf(u - 0.5f * ps + 0.5f), fy0 = floorf(v - 0.5f * ps + 0.5f)      (u - 0.5f * ps, then + 0.5f)
 *     the block is dropped unless fx0 > -ps, fx0 < (float)width, fy0 > -ps and fy0 < (float)height (a NaN fails);
 *     x0 = (int)fx0, y0 = (int)fy0; every pixel (x0 + i, y0 + j), 0 <= i, j < point_size, inside the image takes
 *     min(pixel, bits of z) -- z > 1e-6, so the bits order as the floats do.  These are the pixels prv_splat_points writes.
 *     A minimum does not depend on the order.  depth_out_dev: the buffers as float, 0 where no point fell.
 *   stage B, visibility: point i is visible in view v iff the projection succeeds, fu = floorf(u) and fv = floorf(v) satisfy
 *     0 <= fu < (float)width and 0 <= fv < (float)height (a NaN fails), and
 *         z <= zmin * tol1        one float32 multiply, one comparison
 *     with zmin the depth buffer at ((int)fu, (int)fv) (an empty pixel fails) and tol1 = 1.0f + depth_tol, formed once in
 *     float32.  The point's own block covers its pixel, so zmin <= z: with depth_tol = 0 exactly the nearest points of a pixel
 *     are visible (equal depths all are).  bits[v][w], w < ceil(n_points / 64): bit j of the word = point 64 w + j; the bits
 *     past n_points are 0.
 *   stage C, in integers: C = a set of points, empty at the start.
 *     curve: for j = 0..k-1: gain_j = popcount(bits[order[j]] & ~C); C |= bits[order[j]]; covered[j] = gain_0 + .. + gain_j;
 *       first_seen[i] = the first j whose view sees point i, 0xFFFFFFFF if none does.  A repeated view gains 0.
 *     greedy: k rounds; each takes the largest popcount(bits[i] & ~C) among the views not yet chosen, on a tie the smallest
 *       position i, and goes on when that gain is 0; covered[j] is cumulative as above.
 *   order and chosen_out hold POSITIONS 0..n_views-1 in the handle's view list, not camset ids.
 * The gains are integer atomics and popcounts, the arg-max is taken on the host from a read-back of the gains per round:
 * two calls return identical bytes.  The views' depth buffers are built in batches that fit a fixed scratch budget (256 MiB,
 * at least one view per batch: no view count fails for depth-buffer memory alone); the batching changes no byte.  The handle
 * keeps the bit matrix (n_views * ceil(n_points / 64) * 8 bytes) and copies nothing else: the points may go away.
 * n_points = 0 is not an error: every count is 0.  Synchronises.
 * Errors, PRV_E_INVALID with a message: a NULL or host pointer where a device pointer is required, point_size outside 1..64,
 * depth_tol negative or not finite, k < 1 or k > n_views (greedy), an order entry out of range, more than 2^31 points.
 * LIMITS: visibility comes from a POINT z-buffer, not from a rasterised surface -- holes between the points of a sparse cloud
 * let the far side through.  The answer to that is the mesh occluder, prv_coverage_create_occluded below: where the surface is
 * held as a mesh, its rasterised depth occludes and no hole is left; without a mesh, raise point_size, or sample more points,
 * until a pixel's footprint holds several (fattened silhouettes, or memory).  depth_tol
 * trades the undercount at grazing angles (one pixel spans a range of depths there) against seeing through thin parts; its
 * default 0.02 is an option value, NOT a measured one.  There is no incidence-angle or distance weighting: a point seen
 * once, from whatever angle, counts as seen (the selection stage's "coverage is binary", priced here rather than lifted).
 * The stage is SINGLE-RANK: the bit matrix of every view lives on one device. */
typedef struct prv_coverage prv_coverage; /* owns the bit matrix; inert (PRV_E_STATE) if it outlives its context */
typedef struct prv_coverage_opts {
  int32_t point_size; /* 1..64, default 1 */
  float depth_tol;    /* >= 0, default 0.02 */
} prv_coverage_opts;
int prv_coverage_default_opts(prv_coverage_opts* opts); /* point_size 1, depth_tol 0.02 */
/* opts NULL: the defaults.  depth_out_dev (device, optional): n_views*h*w float32, nearest z per pixel, 0 = empty, unflipped */
int prv_coverage_create(prv_ctx* ctx, const float* xyz_dev, uint64_t n_points, const prv_camset* cs, const int* view_ids,
                        int n_views, int width, int height, const prv_coverage_opts* opts, float* depth_out_dev,
                        prv_coverage** out);
/* n_coverable: points at least one view sees; any pointer may be NULL */
int prv_coverage_info(const prv_coverage* cov, uint64_t* n_points, int* n_views, uint64_t* n_coverable);
/* per_view_host: n_views counts, the points each view sees on its own */
int prv_coverage_visible(const prv_coverage* cov, uint64_t* per_view_host);
/* words_host: the ceil(n_points / 64) words of one view (a test hook) */
int prv_coverage_bits(const prv_coverage* cov, int view, uint64_t* words_host);
/* covered_host: k cumulative counts; first_seen_dev (device, optional): n_points uint32 */
int prv_coverage_curve(prv_coverage* cov, const int* order, int k, uint64_t* covered_host, uint32_t* first_seen_dev);
/* chosen_out: k positions (host); covered_host: k cumulative counts (host, may be NULL) */
int prv_coverage_greedy(prv_coverage* cov, int k, int* chosen_out, uint64_t* covered_host);
void prv_coverage_destroy(prv_coverage* cov);

/* ---- mesh depth and the mesh occluder: a rasterised surface ------------------- */
/* replaces: nothing in the reference.  This build's own: the nearest depth of a triangle mesh per pixel and view -- the
 * ground-truth depth image of a surface, and the occluder that closes the see-through LIMIT of the point z-buffer above.
 * prv_mesh_from_arrays: a mesh from host arrays in the ENGINE frame (n_vertices * 3 float32, n_triangles * 3 uint32), the way
 * in for a ground-truth or hand-made surface.  Normals read as 0 and there are no colours.  The result is an ordinary
 * prv_mesh (prv_mesh_get, _components, _filter, _sample and _save work on it; inert, PRV_E_STATE, if it outlives its context).
 * An empty mesh is allowed.  Errors, PRV_E_INVALID with a message: a coordinate that is not finite, a vertex id >= n_vertices,
 * a NULL array with a non-zero count, more than 2^31 vertices or triangles.
 * ARITHMETIC CONTRACT of prv_mesh_depth and of stage A of prv_coverage_create_occluded.  Every float32 or float64 operation
 * below is one IEEE operation in the order written; the integers are exact.
 *   vertices: each vertex goes through the projection of the coverage section (pinhole only: a camset with any non-zero lens
 *     term among the views asked for is refused, PRV_E_INVALID -- a straight edge does not stay straight under a lens).  A
 *     triangle is dropped for a view if any of its vertices fails the projection (c_2 > 1e-6f, c_2 < +Inf) or has
 *     |u| >= 32768.0f or |v| >= 32768.0f (a NaN fails).
 *   snap: X = (int64)rintf(u * 256.0f), Y = (int64)rintf(v * 256.0f) (round half to even), so |X|, |Y| <= 2^23.
 *   edge functions: pixel (x, y) has its centre at Px = 256 x + 128, Py = 256 y + 128.
 *     E_ab(P) = (Xb - Xa)(Py - Ya) - (Yb - Ya)(Px - Xa)       in int64 (below 2^49)
 *     A2 = E_ab(c); A2 == 0: the triangle is dropped; A2 < 0: b and c are exchanged (and A2 = -A2).  Both windings are
 *     rasterised: an occluder occludes from either side.
 *   inside: w_a = E_bc(P) >= 0, w_b = E_ca(P) >= 0 and w_c = E_ab(P) >= 0.  Inclusive, no top-left rule: the buffer takes a
 *     minimum, so a pixel on a shared edge hit twice is harmless and there are no cracks.
 *   depth: i_k = 1.0 / (double)z_k;  iz = ((double)w_a * i_a + (double)w_b * i_b) + (double)w_c * i_c;
 *     z = (float)((double)A2 / iz); the pixel takes min(pixel, bits of z) on the uint32 buffer of stage A, 0xFFFFFFFF at the start.
 *     depth_out_dev: the buffers as float, 0 where no triangle fell (as prv_coverage_create resolves its own).
 *   visibility (stage B with a mesh): the projection and the in-image test of stage B above, then
 *         visible = empty pixel, or z <= zmin * tol1
 *     with zmin the MESH buffer at the point's pixel: a point whose pixel holds no triangle is visible (nothing stands in
 *     front of it), and a NaN z would fail.  opts->point_size is ignored.  Stage C is the coverage section's, untouched.
 * HOW IT RUNS (no byte depends on it: the result is a minimum).  One lane per (triangle, view) walks the clipped pixel box of
 * the snapped vertices (x from max(0, ceil((min X - 128) / 256)) to min(width - 1, floor((max X - 128) / 256)), y likewise) if it
 * holds at most small_max pixels (64; PRV_RASTER_SMALL_PIXELS, read per call); larger boxes go to a list that a second kernel
 * takes one workgroup per entry, in 16 x 16 tiles.  Triangles pass in chunks with chunk x views <= the list's capacity (2^22
 * entries of 8 bytes; PRV_RASTER_LIST_ENTRIES, read per call), so the list cannot overflow.  The views are batched on the
 * 256 MiB z-buffer budget of prv_coverage_create.  Two calls return identical bytes.  Synchronises.
 * Errors, PRV_E_INVALID with a message: a NULL mesh, a mesh of another context, a lens camera, a NULL or host pointer where a
 * device pointer is required, and what prv_coverage_create refuses.
 * LIMITS: NO NEAR-PLANE CLIPPING -- a triangle with a vertex behind (or at) the camera is dropped whole for that view; the
 * cameras of a view space stand outside the object, so no triangle of its surface straddles their near plane.  depth_tol still
 * absorbs the depth range that one pixel spans on a slanted face (the point's own depth against the depth at the pixel's
 * centre).  No lenses.  SINGLE-RANK, as the coverage stage is. */
int prv_mesh_from_arrays(prv_ctx* ctx, const float* xyz_host, uint64_t n_vertices, const uint32_t* tri_host, uint64_t n_triangles,
                         prv_mesh** out);
/* depth_out_dev (device): n_views*h*w float32, nearest surface depth per pixel and view, 0 = no triangle, unflipped */
int prv_mesh_depth(prv_ctx* ctx, const prv_mesh* m, const prv_camset* cs, const int* view_ids, int n_views, int width, int height,
                   float* depth_out_dev);
/* prv_coverage_create with the mesh, not the points, as what occludes; returns an ordinary prv_coverage */
int prv_coverage_create_occluded(prv_ctx* ctx, const float* xyz_dev, uint64_t n_points, const prv_mesh* occluder, const prv_camset* cs,
                                 const int* view_ids, int n_views, int width, int height, const prv_coverage_opts* opts,
                                 float* depth_out_dev, prv_coverage** out);

/* ---- mesh colour images: a vertex-coloured surface seen from a camera ----------- */
/* replaces: Perception_3D::render (main.cpp:68-96) for an object held as a SURFACE -- prv_splat_points is the same screenshot
 * for a cloud: square splats have holes at close range and need a point size; a mesh has neither.  With convertToAlpha and the
 * flip, these are the rgbaClip_<i>.png images of a mesh (`gt_surface: mesh` in the planner's mode 3).
 * prv_mesh_set_colors: one RGB byte triple per vertex from the host; the mesh then HAS colours (prv_mesh_get, _save and _filter
 * see them).  A marching-cubes mesh extracted with colours has them already.  Errors, PRV_E_INVALID: a count that is not the
 * mesh's, a NULL array with a non-zero count.
 * ARITHMETIC CONTRACT of prv_mesh_render.  A visibility buffer in two stages; every float64 operation below is one IEEE
 * operation in the order written, the integers are exact.
 *   stage A: the vertices, the snap, the edge functions, the inside test and z are those of the depth contract above, bit for
 *     bit.  The pixel takes min(pixel, key) on a uint64 buffer, key = ((uint64)bits of z << 32) | triangle id, all ones at the
 *     start.  A pixel is empty iff the high word of its key is 0xFFFFFFFF.
 *     TIE RULE: the nearest depth wins; among triangles with equal depth bits at a pixel, the lowest triangle id.
 *   stage B, per pixel of a view: empty -> the background.  Otherwise the triangle named by the low word is set up again for the
 *     view (a, b, c: its ORIENTED vertices -- where the depth contract exchanges b and c, their colours go with them), w_a, w_b,
 *     w_c are formed at the pixel's centre, and
 *         p_a = (double)w_a * i_a;  p_b = (double)w_b * i_b;  p_c = (double)w_c * i_c
 *         iz  = (p_a + p_b) + p_c                              -- the depth contract's iz, bit for bit
 *         c_k = ((p_a * (double)C_a[k] + p_b * (double)C_b[k]) + p_c * (double)C_c[k]) / iz      for channel k of r, g, b
 *         byte_k = (uint8)min(255.0, floor(c_k + 0.5))
 *     with C_v the colour bytes of vertex v: perspective-correct (hyperbolic) Gouraud interpolation.
 *   output: RGBA8.  A covered pixel is (r, g, b, 255); the background is 255, 255, 255, 0; a covered pixel whose three bytes
 *     come out exactly 255, 255, 255 gets alpha 0 as well (convertToAlpha's rule, as prv_splat_points applies it).  flip180 puts
 *     pixel (x, y) at (width - 1 - x, height - 1 - y), as prv_splat_points does.
 *   planes (optional, written by the same lane, NEVER flipped, like prv_mesh_depth's output): depth_out_dev = the high word of
 *     the key as float32, 0 = empty; tri_out_dev = the low word, 0xFFFFFFFF = empty.
 *   EQUALITY WITH prv_mesh_depth: the depth plane equals prv_mesh_depth of the same mesh, views and size bit for bit (the high
 *     word of a minimum over keys is the minimum over high words).
 * HOW IT RUNS (no byte depends on it): stage A is the two raster kernels of prv_mesh_depth on the 64-bit key, with the same
 * small_max, list and chunks (PRV_RASTER_SMALL_PIXELS, PRV_RASTER_LIST_ENTRIES); stage B is one lane per pixel, no atomics.  The
 * views are batched on the z-buffer budget of prv_coverage_create at 8 bytes per pixel (PRV_COVERAGE_ZBUF_BYTES).  Two calls
 * return identical bytes.  Synchronises.  An empty mesh (with colours set) gives all background.  prv_debug_raster_stats reports
 * the call as it does prv_mesh_depth.
 * Errors: what prv_mesh_depth refuses, with its messages (a NULL mesh, a mesh of another context, a lens camera, a bad size or
 * view list, a NULL or host pointer where a device pointer is required; a mesh that outlives its context: PRV_E_STATE), and a
 * mesh without colours: PRV_E_INVALID, "call prv_mesh_set_colors".
 * LIMITS: PINHOLE ONLY; NO NEAR-PLANE CLIPPING (a triangle with a vertex behind or at the camera is dropped whole for that view);
 * GOURAUD VERTEX COLOURS ONLY -- no textures, NO LIGHTING, no anti-aliasing: a pixel shows the surface at its centre;
 * SINGLE-RANK. */
/* rgb_host: n_vertices*3 bytes; n_vertices must equal the mesh's; the mesh then has colours (prv_mesh_get, _save, _filter see them) */
int prv_mesh_set_colors(prv_mesh* m, const uint8_t* rgb_host, uint64_t n_vertices);
/* out_rgba8_dev: n_views*h*w*4 bytes; depth_out_dev / tri_out_dev optional (NULL), n_views*h*w each */
int prv_mesh_render(prv_ctx* ctx, const prv_mesh* m, const prv_camset* cs, const int* view_ids, int n_views, int width, int height,
                    int flip180, uint8_t* out_rgba8_dev, float* depth_out_dev, uint32_t* tri_out_dev);

/* ---- depth-map fusion: a truncated signed distance volume from depth images ------- */
/* replaces: nothing in the reference.  This build's own: the surface that a set of views SAW -- depth (and colour) images of
 * the views, from a field (prv_render_surface, prv_render_depth, prv_render_rgba8) or from a ground-truth surface (prv_mesh_depth,
 * prv_mesh_render), fused into a volume whose zero level is extracted as a mesh.  Unlike prv_marching_cubes it needs no density
 * iso-level, keeps no floater that no view's depth confirms, and leaves open what no view observed.
 * The volume's grid points are prv_marching_cubes_grid's, bit for bit (p_a = lo[a] + (float)i * step[a], step[a] = (hi[a] - lo[a])
 * / (float)(res[a] - 1), x fastest), so its mesh aligns with a density mesh of the same options.  State per point: D (the
 * truncated distance in units of trunc), W (its weight), WC (the colour's weight) and C[3] (red, green, blue in byte units), all
 * float32 and all 0 in a new volume.
 * ARITHMETIC CONTRACT of prv_tsdf_integrate.  Every float operation below is one IEEE float32 operation in the order written
 * (fmaf = one fused multiply-add); inv = 1.0f / trunc is formed once.  For each grid point e the views are taken IN LIST ORDER:
 *   1. projection: the coverage section's, unchanged, lens cameras included (c_2 > 1e-6f, c_2 < +Inf; u, v, z = c_2).  fu =
 *      floorf(u), fv = floorf(v); the view is skipped unless 0 <= fu < (float)width and 0 <= fv < (float)height (a NaN fails).
 *   2. the pixel: d = depth[view][(int)fv][(int)fu], ws = weight ? weight[the same pixel] : 1.0f; the view is skipped unless
 *      d > 0, d < +Inf, ws > 0 and ws < +Inf (a NaN fails).  Images are unflipped, as prv_mesh_depth writes them; depth is z along
 *      the optical axis (the z of the projection), engine units.
 *   3. sdf = d - z; the view is skipped if sdf < -trunc: the point lies behind what this view sees.
 *   4. s = fminf(sdf * inv, 1.0f);  Wn = W + ws;  D = fmaf(D, W, s * ws) / Wn;  W = Wn.
 *   5. only if the volume keeps colours, rgba8_dev is given and sdf <= trunc:  WCn = WC + ws;  for k = 0, 1, 2:
 *      C[k] = fmaf(C[k], WC, (float)byte_k * ws) / WCn  (all three with the old WC);  then WC = WCn.  The alpha byte is not used.
 *      The colour has a weight of its own because free space far in front of some other surface must not tint a voxel.
 *   CONSEQUENCES: integrating the views [a, b] in one call equals integrating [a] and then [b], byte for byte (the state between
 *   two views is the float32 state itself); two runs give identical bytes.  There are no atomics: one lane owns a point.
 * prv_tsdf_grid: valid = W > 0 && W >= min_weight; grid = valid ? -D : NaN.  With threshold 0 "inside" is then D < 0, the
 *   orientation of prv_marching_cubes: counter-clockwise seen from the lower value, i.e. from the observed free side.
 * prv_tsdf_mesh: prv_tsdf_grid, then prv_marching_cubes_grid_valid at threshold 0 (cells that touch an unobserved point give
 *   nothing: the back of the truncation band is no second surface), then, if the volume keeps colours, one colour per vertex:
 *   the vertex takes the nearest grid point, i_a = clamp((int)rintf((p_a - lo[a]) / step[a]), 0, res[a] - 1) -- an end of its own
 *   edge, and both ends are valid in a kept cell -- and byte_k = (uint8)fminf(255.0f, floorf(C[k] + 0.5f)) if that point has
 *   WC > 0, else 0.  The result is an ordinary prv_mesh (prv_mesh_get, _save, _components, _filter, _sample, prv_mesh_render and
 *   the occluder of prv_coverage_create_occluded take it).  A volume nothing was fused into gives 0 vertices, not an error.
 * prv_tsdf_info: counts[0] = grid points, [1] = observed (W > 0), [2] = inside (observed and D < 0), [3] = band (observed and
 *   |D| < 1); integer counts.
 * HOW IT RUNS (no byte depends on it): one lane per grid point, x fastest, so a wave's 64 points project to neighbouring pixels;
 * the loop over the views runs inside the kernel with the point's state in registers -- each state word is read once and written
 * once per launch -- and the views' cameras travel as kernel arguments (scalar registers), 32 per launch (PRV_TSDF_CHUNK lowers
 * it, read per call; a longer list takes several launches over consecutive views).  Synchronises.
 * Errors, PRV_E_INVALID with a message: a NULL or host pointer where a device pointer is required, rgba8_dev not 4-byte aligned,
 * a bad image size or view id, trunc not positive and finite, res or aabb that prv_mesh_opts would refuse (with its messages), a
 * min_weight that is NaN or negative; a volume that outlives its context: PRV_E_STATE.  n_views = 0 is a no-op.
 * LIMITS: NEAREST-PIXEL depth lookup, no sub-pixel interpolation of the depth image; colour by the NEAREST GRID POINT; the default
 * trunc (three steps of the default grid) is an option value, NOT a measured one; 24 bytes per point with colours (8 without):
 * about 400 MiB at 256^3; views that leave a side unobserved leave the mesh OPEN there, by design; SINGLE-RANK. */
typedef struct prv_tsdf prv_tsdf; /* owns its device buffers; inert (PRV_E_STATE) if it outlives its context */
typedef struct prv_tsdf_opts {
  int32_t res[3];               /* grid points per axis, exactly prv_mesh_opts' meaning and limits */
  float aabb_lo[3], aabb_hi[3]; /* engine frame, as prv_mesh_opts */
  float trunc;                  /* truncation distance, engine units, > 0 and finite */
  int32_t colors;               /* 1: keep a colour volume */
} prv_tsdf_opts;
int prv_tsdf_default_opts(prv_tsdf_opts* opts); /* 256^3, unit cube, trunc = 3 * the largest grid step, colours */
int prv_tsdf_create(prv_ctx* ctx, const prv_tsdf_opts* opts, prv_tsdf** out);
/* depth_dev: n_views*h*w float32; weight_dev (NULL: 1) the same shape; rgba8_dev (NULL: no colour) n_views*h*w*4 bytes; view_ids
 * NULL: cameras 0..n_views-1 */
int prv_tsdf_integrate(prv_tsdf* tsdf, const prv_camset* cs, const int* view_ids, int n_views, int width, int height,
                       const float* depth_dev, const float* weight_dev, const uint8_t* rgba8_dev);
int prv_tsdf_info(prv_tsdf* tsdf, uint64_t counts[4]);
/* grid_dev: res[0]*res[1]*res[2] float32, the layout of prv_density_grid; valid_dev: as many bytes; either may be NULL */
int prv_tsdf_grid(prv_tsdf* tsdf, float min_weight, float* grid_dev, uint8_t* valid_dev);
int prv_tsdf_mesh(prv_tsdf* tsdf, float min_weight, prv_mesh** out);
/* the state as host planes of one float per grid point: D, W, WC, and C as three planes (red, green, blue); any may be NULL; a
 * volume without colours reads WC and C as 0 (a test hook) */
int prv_debug_tsdf_state(prv_tsdf* tsdf, float* d_host, float* w_host, float* wc_host, float* c_host);
void prv_tsdf_destroy(prv_tsdf* tsdf);

/* ---- several GPUs: view sharding + one all-gather ----------------------------- */
/* replaces: nothing in the reference -- its loops over the candidates are serial (main.cpp:2045-2094, 2105-2158;
 * run.py:293) and it has no multi-GPU path.  One process per GPU (RANK / WORLD_SIZE / LOCAL_RANK as torchrun exports
 * them): the candidate views of a round are dealt to the ranks, every rank scores its shard with the whole ensemble,
 * ONE all-gather of the 16-byte records gives every rank the whole round, the same prv_rank / prv_argmax on every
 * rank gives the same integer ranking.
 * transport "rccl" (default): ncclAllGather / ncclBroadcast on device buffers over xGMI, on the context's stream;
 *   librccl is loaded at run time, rank 0's ncclUniqueId reaches the others over a TCP star at `rendezvous`
 *   ("host:port"; NULL = $MASTER_ADDR : $PRV_COMM_PORT, else $MASTER_PORT + 23).
 * transport "socket": the same calls staged through host memory and that star -- for ranks that SHARE a GPU (RCCL
 *   refuses that), i.e. tests.  NULL transport = $PRV_COMM, else "rccl". */
typedef struct prv_comm prv_comm;
int prv_comm_create(prv_ctx* ctx, int rank, int world, const char* transport, const char* rendezvous, prv_comm** out);
void prv_comm_destroy(prv_comm* comm);
int prv_comm_rank(const prv_comm* comm);
int prv_comm_world(const prv_comm* comm);
const char* prv_comm_transport(const prv_comm* comm); /* "rccl" | "socket" */
/* which librccl the communicator's calls land in (transport "rccl"; empty strings / 0 for "socket"): the file's path as
 * the dynamic loader resolved it, ncclGetVersion's code, and how it was found -- "PRV_RCCL_LIB", "already mapped by the
 * process" (the host program's own copy, e.g. torch.distributed's: ONE RCCL per process) or "soname search" */
int prv_comm_library(const prv_comm* comm, char* path_out, int path_cap, int* version_out, char* how_out, int how_cap);
/* recv_dev = world blocks of bytes_per_rank in rank order, identical on every rank; enqueued on the context's stream */
int prv_comm_all_gather(prv_comm* comm, const void* send_dev, size_t bytes_per_rank, void* recv_dev);
int prv_comm_barrier(prv_comm* comm);
/* the views of `rank`: a contiguous block [rank*per, ...) or, interleaved, rank, rank+world, ... (a hemisphere set runs
 * pole -> equator and top views cost more).  ids_out (may be NULL) holds up to per entries; returns per = ceil(n/world). */
int prv_shard_views(int n_views, int rank, int world, int interleaved, int* ids_out, int* n_mine);
/* the sharded scoring round: prv_score_views on this rank's shard of views [0, n_views_total) of `cs`, one all-gather,
 * records_host = all n_views_total records in view order on every rank.  gt_shard_dev (method 5): the reference images
 * of THIS rank's views, in shard order (method 7: NULL).  comm NULL = one rank.  stats: this rank's share. */
int prv_score_views_sharded(prv_ctx* ctx, prv_comm* comm, int method, const int* model_slots, int n_models,
                            const prv_camset* cs, int n_views_total, int interleaved, const prv_render_opts* opts,
                            const float* gt_shard_dev, prv_score_record* records_host, prv_stats* stats);
/* the exchange step of a multi-GPU NBV iteration (the reference trains its members one after another in one process,
 * main.cpp:2041-2043): member e was trained in slot e of rank e % world; afterwards slot e of EVERY rank holds it bit
 * for bit.  Device to device: one group of broadcasts on the slots' canonical buffers (table | MLP | occupancy). */
int prv_model_exchange(prv_ctx* ctx, prv_comm* comm, int n_members, const prv_field_desc* desc);
/* the general form: member e lives in model slot slots[e] and was trained by rank owners[e] (prv_planner's `shard: members`
 * deals the (object, member) trainings of a round to the ranks round-robin, so an ensemble's members come from different
 * ranks and different objects' ensembles sit in different slots); prv_model_exchange = slots e, owners e % world */
int prv_model_exchange_slots(prv_ctx* ctx, prv_comm* comm, int n_members, const int* slots, const int* owners,
                             const prv_field_desc* desc);

/* ---- training ------------------------------------------------------------- */
/* replaces: the `while testbed.frame()` loop run.py:185-208 drives for `--train --n_steps 2500`
 * (main.cpp:1668) on the dataset of testbed.load_training_data (run.py:109): random rays over the dataset
 * images, L2 loss on linear colours over a random background, backward through both MLPs and the hash
 * grid, Adam with sparse table updates, periodic density-grid refresh -- the published instant-ngp
 * optimiser restated (the optimiser itself is inside pyngp, not in the reference tree).
 * The model slot is trained IN PLACE: after every prv_train_steps call the slot renders / scores with the
 * trained weights and occupancy. */
typedef struct prv_train_opts {
  int32_t n_rays;    /* rays per step (with target_samples: the cap of the adaptive count; default 2^16) */
  int32_t n_samples; /* PRV_STEP_FIXED_S: samples per ray between the AABB hits, <= 128.  PRV_STEP_NGP: the most steps a ray takes,
                        <= PRV_NGP_MAX_STEPS (1024 = the cube's diagonal, what prv_train_default_opts sets for that rule) */
  float lr, beta1, beta2, eps, l2_reg; /* Adam; l2_reg on the MLP weights only.  lr >= 0: at 0 the steps run (loss, sample
                                          budget, density refreshes) and no weight moves */
  float min_T;       /* early termination of a training ray */
  uint64_t seed;
  int32_t random_bg; /* 1: random background colour per ray */
  int32_t occ_every; /* refresh the density grid every N steps (0 = never) */
  float occ_decay, occ_sigma_thresh; /* ema = max(ema*decay, sigma); occupied iff ema > thresh (default 5.9 =
                                        upstream's optical thickness 0.01 over a sqrt(3)/1024 step).  A new trainer's
                                        EMA starts at 0 in every cell, whatever the slot's occupancy says: the first
                                        refresh sets ema = sigma */
  int32_t target_samples; /* > 0: the ray count of a step adapts so that about this many samples are composited
                             (upstream keeps 2^18 samples per batch): after every step active = clamp(target *
                             active / used, active/2, 2*active) within [1, n_rays]; first step min(n_rays,
                             target / n_samples).  0: always n_rays */
  int32_t patch_w, patch_h; /* > 1: a step's rays are drawn as patches of patch_w x patch_h adjacent pixels of one image
                               (patch_w * patch_h <= 16; ray j = pixel j % P of patch j / P, rows walked in snake order)
                               that share one jitter, and the step's sample list is ordered depth step by depth step
                               inside a patch, so that the samples of a backward tile share table entries (fewer
                               memory-side atomic requests per step); 0 or 1: every ray its own pixel (the published
                               i.i.d. sampler).  prv_train_default_opts says which this build defaults to.  PRV_STEP_FIXED_S only */
  int32_t step_mode; /* how a training ray is sampled (the values of prv_render_opts.step_mode).  PRV_STEP_FIXED_S: n_samples
                        uniform samples between the AABB hits under one random offset per ray (rounds 1-5).  PRV_STEP_NGP: the
                        engine's own marcher, what upstream trains with behind run.py:188 `testbed.frame()` --
                        fixed step dt = sqrt(3)/1024 from the AABB entry, per-ray random start: sample i at t0 + (i + jitter) dt
                        while that is inside the box and i < n_samples, every step tested against the occupancy grid,
                        alpha = 1 - exp(-sigma dt) with that dt; the sample budget (target_samples) is unchanged, its first step
                        casts target_samples / n_samples rays.  A step lists at most 2^24 samples under this rule (64 x the
                        default budget); a batch beyond that makes prv_train_steps fail with PRV_E_STATE */
  int32_t deterministic; /* 1 (tests): bit-reproducible training -- the ray batches are listed in ray order (per-block counts, a scan,
                            then the append: three launches per batch, no block waits for another) and the table gradient
                            is summed in 64-bit fixed point (order-independent) instead of f32 atomics; slower.  0: the product path */
} prv_train_opts;
typedef struct prv_trainer prv_trainer;
int prv_train_default_opts(prv_train_opts* opts);
/* dataset = cameras of prv_cameras_from_dataset_json (own intrinsics + lens) and their images,
 * n * height * width * 4 straight-alpha sRGB bytes in device memory (caller keeps them alive); when
 * (width, height) differs from the dataset's size the intrinsics are scaled per axis */
int prv_train_create(prv_ctx* ctx, int model_slot, const prv_camset* dataset, const uint8_t* images_rgba8_dev,
                     int width, int height, const prv_train_opts* opts, prv_trainer** out);
/* n optimiser steps; losses_host (n floats, may be NULL) = the batch loss of each step before its update */
int prv_train_steps(prv_trainer* t, int n_steps, float* losses_host);
/* the members of an ensemble side by side: step i of every trainer (each on its own HIP stream) before step
 * i+1 of any; one slot per trainer, one context; losses_host = n_trainers rows of n_steps, may be NULL */
int prv_train_steps_multi(prv_trainer** trainers, int n_trainers, int n_steps, float* losses_host);
int prv_train_info(const prv_trainer* t, uint32_t* steps_done, uint64_t* samples_last_batch,
                   uint64_t* table_scalars);
/* rays the next step will cast (= n_rays unless target_samples is set) */
int prv_train_active_rays(const prv_trainer* t);
/* STREAMS: a trainer runs on a stream of its own that owns a hardware queue (hipExtStreamCreateWithCUMask naming every CU; the
 * pooled streams of hipStreamCreate share four queues, and five members stepping side by side sat on three of them).  That API
 * takes no flags, so the stream is a BLOCKING one: work an embedder puts on the LEGACY default stream (stream 0; PyTorch's
 * default stream is that one) serialises with every trainer's stream, which undoes the side-by-side overlap of
 * prv_train_steps_multi while such work is in flight.  Hosts that use the legacy default stream should move that work to a
 * stream created with hipStreamNonBlocking (or build with per-thread default streams); PRV_TRAIN_OWN_QUEUE=0 in the
 * environment gives the trainers pooled non-blocking streams instead (slower side by side: round of five 0.524 -> 0.503 ms
 * with own queues, profiles/NOTES.md round 5).
 * The trainer's stream (it owns a hardware queue) and device buffers stay with the CONTEXT for its next trainer of the same
 * sizes (at most 16 GiB / 512 buffers, oldest released first); prv_destroy releases them. */
void prv_train_destroy(prv_trainer* t);
/* parity hooks: gradients of the NEXT batch without an update (host arrays: table_scalars and
 * PRV_MLP_HALFS floats), the fp32 master weights, one density-grid refresh */
int prv_train_gradients(prv_trainer* t, float* table_grad_host, float* mlp_grad_host, float* loss);
int prv_train_master(prv_trainer* t, float* table_host, float* mlp_host);
int prv_train_refresh_occupancy(prv_trainer* t);
/* dev only: 64 phase time stamps of the tile kernels' block 0 (zeros unless built with PRV_TRAIN_ABLATE=16) */
int prv_train_debug_stamps(prv_trainer* t, unsigned long long* out64);

/* ---- stage hooks for parity tests (host in / host out, small n) ---------- */
/* how a loaded field is laid out for the kernels, and which render_queue64_kernel<F, NDENSE> instance prv_render
 * launches for it (tests assert that e.g. the 512^3 / F=2 field really runs the <2,10> instance) */
typedef struct prv_model_layout {
  uint64_t table_bytes_canonical; /* ABI layout: what prv_model_load / export carry */
  uint64_t table_bytes_physical;  /* kernel layout: power-of-two strides on the dense levels, size-aligned levels */
  int32_t kernel_features;        /* F of the instance */
  int32_t kernel_dense_levels;    /* NDENSE of the instance */
  int32_t n_hashed_levels;
  int32_t kernel_slots;           /* ray slots per wave of the render kernel (64) */
  int32_t n_dense_levels;         /* leading physically dense levels */
} prv_model_layout;
int prv_debug_model_layout(prv_ctx* ctx, int model_slot, prv_model_layout* out);
/* Dense replicas of a loaded field's leading hashed levels (a buffer beside the physical table, built when the model is
 * installed): how many levels the model holds them for -- which is the render_queue64 replica variant
 * prv_render launches for it under PRV_STEP_FIXED_S (under PRV_STEP_NGP the launch reads at most two of them); 0: none, the
 * plain instance -- and the bytes of that buffer.  Only F = 4 fields that run the
 * <4, 5> instance get any; PRV_REPLICA_LEVELS (0..3) caps the count, PRV_REPLICA_MB sets the byte budget, both read when a
 * model is installed.  prv_model_layout does not change with them. */
int prv_debug_replica_layout(prv_ctx* ctx, int model_slot, int32_t* n_levels, uint64_t* bytes);
/* The layout arithmetic of one replica, no context needed: a level of `res` vertices per axis with entries of n_features halfs
 * -> entries per row (= rows per plane: res + 1 rounded up to 8), the z stride in bytes (must stay below 2^24) and the bytes
 * of the replica (res + 1 planes, rounded up to 4 KiB; 0: such a level is not replicated). */
int prv_debug_replica_level(uint32_t res, uint32_t n_features, uint32_t* row_entries, uint64_t* z_stride_bytes, uint64_t* bytes);
/* Shader clock the render launches actually ran at (roofline accounting: the VALU issue peak is per clock and the
 * clock under this load is well below the 2.4 GHz maximum).  One wave of every render_queue launch stamps the shader
 * cycle counter and the constant-rate reference counter at its start and end; this returns the two sums since the
 * statistics were last cleared (a prv_render / prv_score_views call with stats clears them) and the reference rate.
 * Average clock = shader_cycles / (ref_ticks / ref_hz).  Synchronises the stream. */
int prv_debug_render_clock(prv_ctx* ctx, uint64_t* shader_cycles, uint64_t* ref_ticks, double* ref_hz);
/* rays of view i at (w,h): o,d = n*3, t = n*2 (AABB entry/exit; exit<=entry => miss) */
int prv_debug_raygen(prv_ctx* ctx, const prv_camset* cs, int view, int width, int height,
                     int spp_index, float* o, float* d, float* t);
/* milliseconds of the last mesh extraction's stages: density grid, classify + scans, emit, colours (HIP events) */
int prv_debug_mesh_stages(prv_ctx* ctx, float ms[4]);
/* hook + compress rounds the mesh's labelling took (0: no triangles); PRV_E_STATE before prv_mesh_components has run */
int prv_debug_mesh_component_rounds(const prv_mesh* m, int* rounds);
/* the last prv_mesh_depth / prv_mesh_render / prv_coverage_create_occluded call: out[0] = (view, triangle) pairs rasterised, out[1] = those whose
 * clipped pixel box held more than small_max pixels (the large path took them) */
int prv_debug_raster_stats(prv_ctx* ctx, uint64_t out[2]);
/* bytes of device memory the library holds in this process: every context's workspaces and models, every handle's arrays,
 * what destroyed trainers left parked.  Not prv_malloc's memory (the caller's).  Back where it was once everything a piece of
 * work created has been destroyed. */
uint64_t prv_debug_live_bytes(void);
/* 32 fp16 features per position (bit patterns) */
int prv_debug_encode(prv_ctx* ctx, int model_slot, const float* pos, int n, uint16_t* feat);
/* per point: out[0]=sigma, out[1..3]=rgb, out[4..19]=density MLP outputs, out[20..35]=rgb MLP
 * outputs; occupied[n] = occupancy bit */
int prv_debug_field(prv_ctx* ctx, int model_slot, const float* pos, const float* dir, int n,
                    float* out36, int32_t* occupied);

#ifdef __cplusplus
}
#endif
#endif /* PRV_H */
