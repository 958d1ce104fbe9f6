/*
 * prv_oracle.h -- CPU ORACLE for the NeRF-PRV render + view-scoring hot path.
 *
 * THIS IS TEST INFRASTRUCTURE, NOT PRODUCT CODE.  Only tests/, the smoke check in
 * __graft_entry__.py and the cpu_baseline leg of bench.py may load it.  The
 * shipped path (nerf_prv_amd/csrc, include/prv.h) never links or calls it.
 *
 * PARITY STATUS: "parity unpinned" against the reference *binary*.
 *   - The reference (psc0628/NeRF-PRV) cannot be compiled here (Win32 headers,
 *     Eigen, OpenCV, PCL, OctoMap, Gurobi, JsonCpp, Boost all absent; see
 *     DESIGN.md) and ships no tests or golden vectors.
 *   - The field arithmetic (hash grid, MLPs, marching, compositing) lives in
 *     NVlabs/instant-ngp + tiny-cuda-nn, which the reference imports as `pyngp`
 *     (Instantngp_scripts/run.py:25) without vendoring or pinning a version.
 *     It is restated here from the published algorithm (Mueller et al. 2022).
 *   - What IS restated literally from in-tree reference code, with file:line
 *     cited at each function: camera pose search (View_Space.hpp:67-140), view
 *     set (View_Space.hpp:517-558), transforms.json matrices
 *     (main.cpp:1623-1641), candidate header (main.cpp:1793-1811), ensemble
 *     scores + arg-max (main.cpp:2053-2096, 2113-2160), PSNR recipe
 *     (run.py:257-271), pinhole/Brown-Conrady camera (Share_Data.hpp:92-196).
 *   - Pins used instead: the reference's Hemisphere/N.txt data files, hand-derived
 *     known answers, and an independent numpy restatement
 *     (tests/golden/gen_golden.py) whose outputs are committed as fixtures.
 */
#ifndef PRV_ORACLE_H
#define PRV_ORACLE_H
#include <stdint.h>
#include <stddef.h>
#ifdef __cplusplus
extern "C" {
#endif

#define ORC_MAX_LEVELS 16
#define ORC_MLP_HALFS 10240 /* 32*64 + 64*16 + 32*64 + 64*64 + 64*16 */

typedef struct {
  int32_t n_levels;     /* L */
  int32_t n_features;   /* F ; L*F must be 32 */
  int32_t log2_hashmap; /* log2 T */
  int32_t base_res;     /* N_min */
  int32_t finest_res;   /* N_max */
  int32_t occ_res;      /* occupancy grid resolution (cells per axis) */
  float density_bias;   /* sigma = exp(out0 + density_bias) */
  float table_amp;      /* synthetic table ~ U(-amp, amp) */
  float per_level_scale; /* 0: geometric growth base_res -> finest_res in double; > 0: tiny-cuda-nn's float32 recipe
                            (grid.h grid_scale / grid_resolution), the geometry of an imported instant-ngp snapshot */
} orc_field_desc;

typedef struct {
  float scale;     /* pos = fmaf(scale, x, 0.5) */
  uint32_t res;    /* vertices per axis */
  uint32_t offset; /* first entry of the level in the table (entries of F halfs) */
  uint32_t size;   /* entries in the level */
  uint32_t hashed; /* 1: spatial hash, 0: dense */
} orc_level;

typedef struct {
  orc_field_desc desc;
  orc_level levels[ORC_MAX_LEVELS];
  uint32_t total_entries;
  uint16_t* table;             /* total_entries * F fp16 bit patterns */
  uint16_t mlp[ORC_MLP_HALFS]; /* canonical [in][out] row-major, layers d1,d2,r1,r2,r3 */
  uint32_t* occ;               /* occ_res^3 bits, bit = x + R*(y + R*z) */
  float mlp_f[ORC_MLP_HALFS];  /* mlp[] widened to float once (exact), for speed only */
} orc_field;

/* ---- fp16 helpers (IEEE binary16, round-to-nearest-even) ---- */
uint16_t orc_f2h(float f);
uint16_t orc_d2h(double v); /* one rounding, for modelling fp16 mul/fma */
uint16_t orc_d2h_soft(double v); /* the same in integer arithmetic only: the definition orc_d2h's fast path is tested against */
float orc_h2f(uint16_t h);

/* ---- field ---- */
int orc_field_levels(const orc_field_desc* d, orc_level* out, uint32_t* total);
orc_field* orc_field_synthetic(const orc_field_desc* d, uint64_t seed);
orc_field* orc_field_from_params(const orc_field_desc* d, const uint16_t* table,
                                 const uint16_t* mlp, const uint32_t* occ);
void orc_field_free(orc_field* f);
void orc_encode(const orc_field* f, const float p[3], uint16_t feat[32]);
void orc_sh4(const float d[3], float out[16]);
/* full field evaluation; mlp_out (optional) receives [density 16 | rgb 16] raw outputs */
void orc_eval(const orc_field* f, const float p[3], const float d[3], float* sigma, float rgb[3],
              float* mlp_out);
int orc_occupied(const orc_field* f, const float p[3]);

/* ---- cameras (reference in-tree math) ---- */
/* View::get_next_camera_pos type 0 with now_camera_pose_world = I (View_Space.hpp:67-140) */
void orc_view_pose(const double init_pos[3], const double center[3], double pose[16]);
/* transform_matrix = P * pose^-1 * diag(1,-1,-1,1)  (main.cpp:1626-1641) */
void orc_transform_matrix(const double pose[16], double out[16]);
/* View_Space::get_view_space positions (View_Space.hpp:550-556); returns #views kept */
int orc_view_space(const double* pt_sphere, int n, double radius, const double center[3],
                   double* out_pos);
/* centroid + 17/16 * max radius (View_Space.hpp:534-548) */
void orc_bbx(const double* pts, int n, double center[3], double* predicted_size);
/* assumed instant-ngp nerf_matrix_to_ngp: out = 3x4 row-major float */
void orc_nerf_to_ngp(const double tm[16], double scale, const double offset[3], float out[12]);
/* Share_Data.hpp:92-137 / 140-196, float32 */
void orc_rs2_project(float pixel[2], const float intr[9], int model, const float point[3]);
void orc_rs2_deproject(float point[3], const float intr[9], int model, const float pixel[2],
                       float depth);

typedef struct {
  float c2w[12]; /* ngp frame, row-major 3x4 */
  float fx, fy, cx, cy;
  float lens[4]; /* k1, k2, p1, p2 of the OpenCV model (the keys of the dataset json); all 0 = pinhole */
} orc_camera;

/* OpenCV radial + tangential model on normalised coordinates, and its inverse by ORC_LENS_ITERS
 * Newton steps with the analytic Jacobian (what a lens-aware marcher does for the test views of
 * run.py:238-247, render_with_lens_distortion run.py:145; upstream's solver is not in tree: own
 * restatement, parity unpinned) */
#define ORC_LENS_ITERS 8
void orc_lens_distort(const float lens[4], float x, float y, float* xd, float* yd);
void orc_lens_undistort(const float lens[4], float* x, float* y);

/* sub-pixel offset of sample k of spp (k=0 -> pixel centre) */
void orc_spp_offset(int k, float* ox, float* oy);
void orc_raygen(const orc_camera* cam, int px, int py, float ox, float oy, float o[3], float d[3]);
int orc_ray_aabb(const float o[3], const float d[3], float* t0, float* t1);

/* ---- render: linear premultiplied RGBA float32, no background ---- */
void orc_render(const orc_field* f, const orc_camera* cam, int w, int h, int n_samples, int spp,
                float min_T, float* rgba, uint64_t* n_evaluated, int n_threads);
/* rows [y0,y1) only -- for bounded CPU-baseline timing */
void orc_render_rows(const orc_field* f, const orc_camera* cam, int w, int h, int y0, int y1,
                     int n_samples, int spp, float min_T, float* rgba, uint64_t* n_evaluated,
                     int n_threads);

/* the two sampling rules of the marcher (prv_oracle.c: march_ray):
 *   ORC_STEP_FIXED_S  n_samples uniform samples between AABB entry and exit (BASELINE configs[1], [3]);
 *   ORC_STEP_NGP      instant-ngp's rule for aabb_scale = 1, what run.py:245-247, 304 renders with: fixed step
 *                     dt = sqrt(3)/1024 from the AABB entry, samples at t0 + (i + 1/2) dt inside the box, every step
 *                     tested against the occupancy grid, no per-ray sample cap below the 1024 steps of the diagonal
 *                     (the engine is not in the reference tree: parity unpinned). */
#define ORC_STEP_FIXED_S 0
#define ORC_STEP_NGP 1
#define ORC_NGP_MAX_STEPS 1024
void orc_render_rows_mode(const orc_field* f, const orc_camera* cam, int w, int h, int y0, int y1, int step_mode,
                          int n_samples, int spp, float min_T, float* rgba, uint64_t* n_evaluated, int n_threads);
/* the march alone: samples of rows [y0,y1) that lie in occupied cells, before any early termination */
uint64_t orc_march_count_rows(const orc_field* f, const orc_camera* cam, int w, int h, int y0, int y1, int step_mode,
                              int n_samples, int spp, int n_threads);

/* ---- image post + scores ---- */
float orc_linear_to_srgb(float x);
/* shade over background bg[4], un-premultiply, sRGB, quantise (assumed upstream common.py) */
void orc_quantize_rgba8(const float* rgba, size_t npix, const float bg[4], uint8_t* out);
/* main.cpp:2053-2086 */
double orc_score_ensemble_rgb(const uint8_t* const* imgs, int E, size_t npix);
/* main.cpp:2113-2150 */
double orc_score_ensemble_rgbdensity(const uint8_t* const* imgs, int E, size_t npix);
/* run.py:257-263 (PSNR of sRGB-clipped images) + mean opacity */
void orc_score_psnr_coverage(const float* rgba, const float* gt_rgba, size_t npix,
                             const float bg[4], double* psnr, double* coverage);
/* PRV_SCORE_PSNR_COVERAGE's key: -psnr + coverage_weight * mean((1 - alpha)^2) (density term of main.cpp:2148) */
void orc_score_view(const float* rgba, const float* gt_rgba, size_t npix, const float bg[4], double coverage_weight,
                    double* score, double* psnr, double* coverage);
/* mean SSIM of two images (run.py:260; recipe assumed from upstream common.py) */
double orc_ssim(const float* rgba, const float* gt_rgba, int w, int h, const float bg[4]);
/* full ranking: stable sort by (-score, id)  (arg-max rule main.cpp:2088-2091) */
void orc_rank(const double* scores, const int* ids, int n, int* order);
int orc_argmax(const double* scores, const int* ids, int n);

/* first-hit voxel DDA over the occupancy grid (CPU-path analogue of main.cpp:238-284) */
int orc_first_hit(const orc_field* f, const float o[3], const float d[3], float max_range,
                  int cell[3]);

void orc_first_hit_rows(const orc_field* f, const orc_camera* cam, int w, int y0, int y1, float max_range, int32_t* out);
/* the whole precept_thread_process per voxel (main.cpp:238-284) on the occupancy grid */
void orc_precept(const orc_field* f, const float* voxels, int n, const double w2c[16], const double c2w[16],
                 const float intr[9], int width, int height, int model, float max_range, int32_t* out);

/* ---- ground-truth image synthesis: the PCL screenshot of the coloured ground-truth cloud
 * (Perception_3D::render main.cpp:68-96, points of points_size_cloud pixels on a white background),
 * convertToAlpha (Share_Data.hpp:771-784: exactly-white pixels -> alpha 0, everything else 255) and the 180
 * degree flip of main.cpp:1616, restated as a z-buffered square-splat rasteriser.  OpenGL's own point
 * rasterisation rules are not reproducible from the tree: parity unpinned.
 * xyz in world units (n*3), rgb n*3 bytes; points go to the engine frame as the json's scale/offset do with
 * camera positions (p*scale + offset, axes cycled y,z,x).  Nearest point wins; equal depths -> smaller packed
 * colour.  out: h*w*4 RGBA bytes. */
void orc_splat_points(const float* xyz, const uint8_t* rgb, size_t n, float scale, const float offset[3],
                      const orc_camera* cam, int w, int h, int point_size, int flip180, uint8_t* out);

/* ---- training step (prv_train.c; published instant-ngp optimiser restated, parity unpinned) ---- */
typedef struct {
  int32_t n_rays;    /* rays per step */
  int32_t n_samples; /* S samples per ray between the AABB hits, <= 128 */
  float lr, beta1, beta2, eps, l2_reg; /* Adam; l2_reg on the MLP weights only */
  float min_T;       /* early termination of a training ray */
  uint64_t seed;
  int32_t random_bg; /* 1: a random background colour per ray blends target and prediction */
  int32_t occ_every; /* refresh the density grid every N steps (0: never) */
  float occ_decay, occ_sigma_thresh; /* ema = max(ema*decay, sigma); occupied iff ema > thresh */
  int32_t target_samples; /* > 0: adaptive ray count, see include/prv.h */
  int32_t patch_w, patch_h; /* > 1: the step's rays are drawn as patches of patch_w x patch_h adjacent pixels of one
                               image that share one jitter (ray j = pixel j % P of patch j / P, rows in snake order);
                               0 or 1: every ray its own pixel */
  int32_t step_mode; /* ORC_STEP_FIXED_S: n_samples jittered uniform samples between the AABB hits.  ORC_STEP_NGP: the
                        engine's own marcher, as upstream trains (run.py:188 `testbed.frame()`): fixed step
                        dt = sqrt(3)/1024 from the AABB entry, per-ray random start -- sample i at t0 + (i + jitter) dt
                        while that is inside the box, i < n_samples <= ORC_NGP_MAX_STEPS --, every step tested against
                        the occupancy grid, alpha = 1 - exp(-sigma dt) with that dt */
  int32_t deterministic; /* (the HIP trainer's test switch: order-independent sums; the oracle is sequential anyway) */
} orc_train_opts;
typedef struct orc_trainer orc_trainer;
uint32_t orc_rng_u24(uint64_t seed, uint64_t stream, uint64_t i);
/* cams[n_img] are dataset cameras at (w,h); rgba8 = n_img*h*w*4 straight-alpha sRGB bytes.  exact = 1:
 * no fp16 rounding (differentiable forward, for the finite-difference check of the backward pass) */
orc_trainer* orc_train_create(const orc_field* init, const orc_train_opts* o, const orc_camera* cams, int n_img,
                              int w, int h, const uint8_t* rgba8, int exact);
void orc_train_free(orc_trainer* t);
double orc_train_step(orc_trainer* t);       /* returns the batch loss before the update */
double orc_train_loss_only(orc_trainer* t);  /* loss of the next batch, nothing changes */
double orc_train_gradients(orc_trainer* t, double* table_grad, double* mlp_grad); /* next batch, no update */
void orc_train_refresh_occupancy(orc_trainer* t);
const orc_field* orc_train_field(const orc_trainer* t);
uint32_t orc_train_steps_done(const orc_trainer* t);
uint64_t orc_train_samples_last(const orc_trainer* t);
uint32_t orc_train_active_rays(const orc_trainer* t); /* ray count of the next step */
float* orc_train_master_table(orc_trainer* t);
float* orc_train_master_mlp(orc_trainer* t);
size_t orc_train_table_size(const orc_trainer* t);
void orc_train_ema(const orc_trainer* t, float* out); /* copy of the density EMA, occ_res^3 floats (all 0 before the first refresh) */

#ifdef __cplusplus
}
#endif
#endif
