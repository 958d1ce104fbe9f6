// prv_select_api.inc -- C ABI of the view selection stage (prv_select.hip); compiled as part of prv_api.cpp

namespace {

int select_check_opts(prv_ctx* c, const prv_select_opts* so, int n_views) {
  if (!so) return fail(c, PRV_E_INVALID, "select options are NULL");
  const int G = so->grid_res;
  if (G < 16 || G > 256 || (G & (G - 1)) != 0) return fail(c, PRV_E_INVALID, "grid_res must be a power of two in [16, 256], got %d", G);
  if (so->k < 1) return fail(c, PRV_E_INVALID, "k must be at least 1, got %d", so->k);
  if (so->k > n_views) return fail(c, PRV_E_INVALID, "k = %d views asked of %d candidates", so->k, n_views);
  return PRV_OK;
}

// the greedy rounds on planes already on the device; the arg-max is a read-back of the n_views sums per round
int select_rounds(prv_ctx* c, const prv_camset* cs, const int* view_ids, int n_views, int W, int H, const float* entropy,
                  const float* alpha, const float* depth, const prv_select_opts* so, int* chosen_out, uint64_t* gains_out,
                  uint32_t* voxel_dev, uint32_t* q_dev) {
  int rc;
  const size_t npix = (size_t)W * (size_t)H, n = npix * (size_t)n_views;
  if (n > ((size_t)1 << 31)) return fail(c, PRV_E_INVALID, "%d views of %dx%d pixels: more than 2^31 pixels", n_views, W, H);
  Upload up;
  if ((rc = upload_views(c, cs, view_ids, n_views, W, H, nullptr, up)) != PRV_OK) return rc;
  if (!voxel_dev) {
    if ((rc = ensure(c, c->sel_voxel, n * 4)) != PRV_OK) return rc;
    voxel_dev = (uint32_t*)c->sel_voxel.p;
  }
  if (!q_dev) {
    if ((rc = ensure(c, c->sel_q, n * 4)) != PRV_OK) return rc;
    q_dev = (uint32_t*)c->sel_q.p;
  }
  const int G = so->grid_res;
  const size_t bit_bytes = (size_t)G * G * G / 8;
  if ((rc = ensure(c, c->sel_bits, bit_bytes)) != PRV_OK) return rc;
  if ((rc = ensure(c, c->sel_sums, (size_t)n_views * 12)) != PRV_OK) return rc; // n_views uint64 sums, then n_views uint32 done flags
  unsigned long long* sums = (unsigned long long*)c->sel_sums.p;
  uint32_t* done = (uint32_t*)(sums + n_views);
  HIPCHK(c, hipMemsetAsync(c->sel_bits.p, 0, bit_bytes, c->stream));
  HIPCHK(c, hipMemsetAsync(done, 0, (size_t)n_views * 4, c->stream));
  SelectFootprintParams fp;
  memset(&fp, 0, sizeof(fp));
  fp.cams = up.cams_dev;
  fp.W = W;
  fp.H = H;
  fp.n_views = n_views;
  fp.entropy = entropy;
  fp.alpha = alpha;
  fp.depth = depth;
  fp.alpha_min = so->alpha_min;
  fp.G = G;
  fp.voxel = voxel_dev;
  fp.q = q_dev;
  HIPCHK(c, launch_select_footprint(fp, c->stream));
  std::vector<unsigned long long> host((size_t)n_views);
  std::vector<char> taken((size_t)n_views, 0);
  for (int round = 0; round < so->k; round++) {
    HIPCHK(c, hipMemsetAsync(sums, 0, (size_t)n_views * 8, c->stream));
    HIPCHK(c, launch_select_gain(voxel_dev, q_dev, npix, n_views, (const uint32_t*)c->sel_bits.p, done, sums, c->stream));
    HIPCHK(c, hipMemcpyAsync(host.data(), sums, (size_t)n_views * 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    int best = -1;
    for (int i = 0; i < n_views; i++) // the largest gain; on a tie the view that comes first
      if (!taken[i] && (best < 0 || host[i] > host[best])) best = i;
    taken[best] = 1;
    chosen_out[round] = view_ids ? view_ids[best] : best;
    if (gains_out) gains_out[round] = (uint64_t)host[best];
    HIPCHK(c, launch_select_mark(voxel_dev, npix, best, (uint32_t*)c->sel_bits.p, done, c->stream));
  }
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return PRV_OK;
}

} // namespace

extern "C" {

int prv_select_default_opts(prv_select_opts* o) {
  if (!o) return PRV_E_INVALID;
  o->k = 1;
  o->grid_res = 64;
  o->alpha_min = 0.5f;
  return PRV_OK;
}

int prv_select_from_images(prv_ctx* c, const prv_camset* cs, const int* view_ids, int n_views, int width, int height,
                           const float* entropy_dev, const float* alpha_dev, const float* depth_dev, const prv_select_opts* so,
                           int* chosen_out, uint64_t* gains_out, uint32_t* voxel_dev, uint32_t* q_dev) try {
  int rc; // (the options are looked at first, context or not: prv_last_error(NULL) names a bad one)
  if ((rc = select_check_opts(c, so, n_views)) != PRV_OK) return rc;
  if (!c) return fail(nullptr, PRV_E_INVALID, "the context is NULL");
  if (!cs || n_views < 0) return fail(c, PRV_E_INVALID, "bad camset / view count");
  if ((rc = check_image_size(c, width, height)) != PRV_OK) return rc;
  if (!entropy_dev || !alpha_dev || !depth_dev || !chosen_out) return fail(c, PRV_E_INVALID, "the entropy, alpha and depth planes and chosen_out are required");
  HIPCHK(c, hipSetDevice(c->device));
  if ((rc = check_device_ptr(c, entropy_dev, "entropy_dev")) != PRV_OK || (rc = check_device_ptr(c, alpha_dev, "alpha_dev")) != PRV_OK ||
      (rc = check_device_ptr(c, depth_dev, "depth_dev")) != PRV_OK || (rc = check_device_ptr(c, voxel_dev, "voxel_dev")) != PRV_OK ||
      (rc = check_device_ptr(c, q_dev, "q_dev")) != PRV_OK)
    return rc;
  return select_rounds(c, cs, view_ids, n_views, width, height, entropy_dev, alpha_dev, depth_dev, so, chosen_out, gains_out, voxel_dev, q_dev);
} catch (...) { return caught(c); }

} // extern "C"

namespace {

// prv_select_views / prv_select_views_surface: the planes of the views into context scratch, then the rounds on them.  surface:
// the first-crossing render at `level`; its hit plane is the rounds' alpha and its depth their depth
int select_views(prv_ctx* c, int slot, const prv_camset* cs, const int* view_ids, int n_views, const prv_render_opts* o, bool surface,
                 float level, const prv_select_opts* so, int* chosen_out, uint64_t* gains_out, prv_stats* st) {
  int rc;
  if ((rc = select_check_opts(c, so, n_views)) != PRV_OK) return rc;
  if (!c) return fail(nullptr, PRV_E_INVALID, "the context is NULL");
  if ((rc = check_model(c, slot)) != PRV_OK || (rc = check_opts(c, o)) != PRV_OK) return rc;
  if (surface && (rc = check_surface_level(c, o, level)) != PRV_OK) return rc;
  if (!cs || n_views < 0) return fail(c, PRV_E_INVALID, "bad camset / view count");
  if (!chosen_out) return fail(c, PRV_E_INVALID, "chosen_out is required");
  HIPCHK(c, hipSetDevice(c->device));
  const size_t n = (size_t)n_views * o->width * o->height;
  if ((rc = ensure(c, c->sel_planes, n * (surface ? 16 : 12))) != PRV_OK) return rc;
  float* ent = (float*)c->sel_planes.p;
  float* alp = ent + n;
  float* dep = alp + n;
  RenderTargets t;
  t.mode = surface ? kRenderSurface : kRenderFootprint;
  t.entropy = ent;
  t.alpha = alp;
  t.depth = dep;
  if (surface) {
    t.hit = dep + n;
    t.level = level;
  }
  if ((rc = render_views(c, slot, cs, view_ids, n_views, o, t)) != PRV_OK) return rc;
  if ((rc = fetch_stats(c, o, n_views, 1, st)) != PRV_OK) return rc;
  return select_rounds(c, cs, view_ids, n_views, o->width, o->height, ent, surface ? t.hit : alp, dep, so, chosen_out, gains_out, nullptr, nullptr);
}

} // namespace

extern "C" {

int prv_select_views(prv_ctx* c, int slot, const prv_camset* cs, const int* view_ids, int n_views, const prv_render_opts* o,
                     const prv_select_opts* so, int* chosen_out, uint64_t* gains_out, prv_stats* st) try {
  return select_views(c, slot, cs, view_ids, n_views, o, false, 0.f, so, chosen_out, gains_out, st);
} catch (...) { return caught(c); }

int prv_select_views_surface(prv_ctx* c, int slot, const prv_camset* cs, const int* view_ids, int n_views, const prv_render_opts* o, float level,
                             const prv_select_opts* so, int* chosen_out, uint64_t* gains_out, prv_stats* st) try {
  return select_views(c, slot, cs, view_ids, n_views, o, true, level, so, chosen_out, gains_out, st);
} catch (...) { return caught(c); }

} // extern "C"
