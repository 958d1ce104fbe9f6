// prv_coverage_api.inc -- C ABI of the surface coverage stage (prv_coverage.hip); compiled as part of prv_api.cpp

struct prv_coverage : prv_handle {
  using prv_handle::prv_handle;
  void detach() override {
    for (Buffer* b : {&bits, &covered, &gain, &done}) b->reset();
  }
  uint64_t n = 0;         // points
  int n_views = 0;
  size_t words = 0;       // ceil(n / 64): words per view
  Buffer bits;            // n_views x words, view-major
  Buffer covered;         // words: the covered set of the call in progress
  Buffer gain;            // uint64 per view (greedy) or per round (curve)
  Buffer done;            // uint32 per view
  std::vector<uint64_t> visible; // points each view sees on its own
  uint64_t n_coverable = 0;      // points at least one view sees
};

static int coverage_alive(const prv_coverage* x) { return handle_alive(x, "the coverage handle", "the coverage handle"); }

namespace {

constexpr uint64_t kCoverageMaxPoints = 1ull << 31;

int coverage_check_opts(prv_ctx* c, const prv_coverage_opts* o) {
  if (o->point_size < 1 || o->point_size > 64) return fail(c, PRV_E_INVALID, "point_size must be in [1, 64], got %d", o->point_size);
  if (!(o->depth_tol >= 0.0f) || !std::isfinite(o->depth_tol))
    return fail(c, PRV_E_INVALID, "depth_tol must be finite and >= 0, got %g", (double)o->depth_tol);
  return PRV_OK;
}

// stages A and B, batch by batch, then the per-view counts and the union's.  occluder != nullptr: stage A rasterises that mesh
// (prv_raster_api.inc) and stage B lets an empty pixel pass; nullptr: the points occlude each other.  up: staged by the caller
int coverage_build(prv_ctx* c, prv_coverage* x, const float* xyz, const prv_mesh* occluder, Upload& up, int W, int H,
                   const prv_coverage_opts& o, float* depth_out) {
  int rc;
  const int V = x->n_views;
  const size_t npix = (size_t)W * (size_t)H;
  const int per_batch = zbuf_views_per_batch(V, npix); // (PRV_COVERAGE_ZBUF_BYTES: several batches at a small size, for tests)
  Buffer z;
  RasterWork raster;
  if ((rc = ensure(c, z, (size_t)per_batch * npix * 4)) != PRV_OK) return rc;
  if (occluder && (rc = raster_begin(c, raster, occluder, per_batch)) != PRV_OK) return rc;
  if ((rc = send_views(c, up)) != PRV_OK) return rc;
  if (x->words > 0) {
    if ((rc = ensure(c, x->bits, (size_t)V * x->words * 8)) != PRV_OK || (rc = ensure(c, x->covered, x->words * 8)) != PRV_OK) return rc;
  }
  if ((rc = ensure(c, x->gain, (size_t)V * 8)) != PRV_OK || (rc = ensure(c, x->done, (size_t)V * 4)) != PRV_OK) return rc;
  const float tol1 = 1.0f + o.depth_tol; // formed once, in float32
  uint32_t* zbuf = (uint32_t*)z.p;
  unsigned long long* bits = (unsigned long long*)x->bits.p;
  for (int v0 = 0; v0 < V; v0 += per_batch) {
    const int nb = std::min(per_batch, V - v0);
    const CamDev* bc = up.cams_dev + v0;
    if (occluder) {
      if ((rc = raster_fill(c, raster, occluder, bc, nb, W, H, zbuf)) != PRV_OK) return rc;
      HIPCHK(c, launch_raster_visible(xyz, (size_t)x->n, bc, nb, W, H, zbuf, tol1, bits + (size_t)v0 * x->words, x->words, c->stream));
    } else {
      HIPCHK(c, launch_coverage_depth(xyz, (size_t)x->n, bc, nb, W, H, o.point_size, zbuf, c->stream));
      HIPCHK(c, launch_coverage_visible(xyz, (size_t)x->n, bc, nb, W, H, zbuf, tol1, bits + (size_t)v0 * x->words, x->words, c->stream));
    }
    if (depth_out) HIPCHK(c, launch_coverage_resolve(zbuf, (size_t)nb * npix, depth_out + (size_t)v0 * npix, c->stream));
  }
  // what each view sees on its own, and what any view sees
  unsigned long long* gain = (unsigned long long*)x->gain.p;
  x->visible.assign((size_t)V, 0);
  HIPCHK(c, hipMemsetAsync(gain, 0, (size_t)V * 8, c->stream));
  HIPCHK(c, launch_coverage_gain(bits, x->words, V, nullptr, nullptr, gain, c->stream));
  HIPCHK(c, hipMemcpyAsync(x->visible.data(), gain, (size_t)V * 8, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  HIPCHK(c, hipMemsetAsync(gain, 0, 8, c->stream));
  HIPCHK(c, launch_coverage_union(bits, x->words, V, (unsigned long long*)x->covered.p, c->stream));
  HIPCHK(c, launch_coverage_gain((const unsigned long long*)x->covered.p, x->words, 1, nullptr, nullptr, gain, c->stream));
  unsigned long long any = 0;
  HIPCHK(c, hipMemcpyAsync(&any, gain, 8, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  x->n_coverable = (uint64_t)any;
  return occluder ? raster_end(c, raster) : PRV_OK;
}

// prv_coverage_create and prv_coverage_create_occluded: one body, the occluder checked by the caller
int coverage_create(prv_ctx* c, const float* xyz, uint64_t n, const prv_mesh* occluder, const prv_camset* cs, const int* view_ids, int n_views,
                    int width, int height, const prv_coverage_opts& o, float* depth_out, prv_coverage** out) {
  int rc;
  if (!cs || n_views < 1) return fail(c, PRV_E_INVALID, "bad camset / view count");
  if ((rc = check_image_size(c, width, height)) != PRV_OK) return rc;
  if (n > kCoverageMaxPoints) return fail(c, PRV_E_INVALID, "%llu points exceed 2^31", (unsigned long long)n);
  if (n > 0 && !xyz) return fail(c, PRV_E_INVALID, "xyz_dev is NULL");
  HIPCHK(c, hipSetDevice(c->device));
  if ((n > 0 && (rc = check_device_ptr(c, xyz, "xyz_dev")) != PRV_OK) || (rc = check_device_ptr(c, depth_out, "depth_out_dev")) != PRV_OK) return rc;
  Upload up; // staged here, sent by coverage_build: a bad view id or a lens is reported before any allocation can fail
  if ((rc = stage_views(c, cs, view_ids, n_views, width, height, nullptr, up)) != PRV_OK) return rc;
  if (occluder && (rc = raster_refuse_lenses(c, up.cams, n_views)) != PRV_OK) return rc;
  std::unique_ptr<prv_coverage> x(new prv_coverage(c));
  x->n = n;
  x->n_views = n_views;
  x->words = (size_t)((n + 63) / 64);
  if ((rc = coverage_build(c, x.get(), xyz, occluder, up, width, height, o, depth_out)) != PRV_OK) {
    (void)hipStreamSynchronize(c->stream); // (before the handle's buffers go)
    return rc;
  }
  *out = x.release();
  return PRV_OK;
}

} // namespace

extern "C" {

int prv_coverage_default_opts(prv_coverage_opts* o) {
  if (!o) return PRV_E_INVALID;
  o->point_size = 1;
  o->depth_tol = 0.02f;
  return PRV_OK;
}

int prv_coverage_create(prv_ctx* c, const float* xyz, uint64_t n, const prv_camset* cs, const int* view_ids, int n_views, int width, int height,
                        const prv_coverage_opts* opts, float* depth_out, prv_coverage** out) try {
  if (out) *out = nullptr;
  prv_coverage_opts o;
  prv_coverage_default_opts(&o);
  if (opts) o = *opts;
  int rc; // (the options are looked at first, context or not: prv_last_error(NULL) names a bad one)
  if ((rc = coverage_check_opts(c, &o)) != PRV_OK) return rc;
  if (!c) return fail(nullptr, PRV_E_INVALID, "the context is NULL");
  if (!out) return fail(c, PRV_E_INVALID, "out is NULL");
  return coverage_create(c, xyz, n, nullptr, cs, view_ids, n_views, width, height, o, depth_out, out);
} catch (...) { return caught(c); }

int prv_coverage_create_occluded(prv_ctx* c, const float* xyz, uint64_t n, const prv_mesh* occluder, const prv_camset* cs, const int* view_ids,
                                 int n_views, int width, int height, const prv_coverage_opts* opts, float* depth_out, prv_coverage** out) try {
  if (out) *out = nullptr;
  prv_coverage_opts o;
  prv_coverage_default_opts(&o);
  if (opts) o.depth_tol = opts->depth_tol; // (point_size is ignored: no point is splatted)
  int rc;
  if ((rc = coverage_check_opts(c, &o)) != PRV_OK) return rc;
  if (!c) return fail(nullptr, PRV_E_INVALID, "the context is NULL");
  if (!out) return fail(c, PRV_E_INVALID, "out is NULL");
  if ((rc = raster_check_mesh(c, occluder, "occluder")) != PRV_OK) return rc;
  return coverage_create(c, xyz, n, occluder, cs, view_ids, n_views, width, height, o, depth_out, out);
} catch (...) { return caught(c); }

int prv_coverage_info(const prv_coverage* x, uint64_t* n_points, int* n_views, uint64_t* n_coverable) {
  const int rc = coverage_alive(x);
  if (rc != PRV_OK) return rc;
  if (n_points) *n_points = x->n;
  if (n_views) *n_views = x->n_views;
  if (n_coverable) *n_coverable = x->n_coverable;
  return PRV_OK;
}

int prv_coverage_visible(const prv_coverage* x, uint64_t* per_view_host) {
  const int rc = coverage_alive(x);
  if (rc != PRV_OK) return rc;
  if (!per_view_host) return fail(x->ctx, PRV_E_INVALID, "per_view_host is NULL");
  memcpy(per_view_host, x->visible.data(), (size_t)x->n_views * 8);
  return PRV_OK;
}

int prv_coverage_bits(const prv_coverage* x, int view, uint64_t* words_host) try {
  const int rc = coverage_alive(x);
  if (rc != PRV_OK) return rc;
  prv_ctx* c = x->ctx;
  if (view < 0 || view >= x->n_views) return fail(c, PRV_E_INVALID, "view %d out of range (the handle holds %d views)", view, x->n_views);
  if (x->words == 0) return PRV_OK;
  if (!words_host) return fail(c, PRV_E_INVALID, "words_host is NULL");
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, hipMemcpyAsync(words_host, (const unsigned long long*)x->bits.p + (size_t)view * x->words, x->words * 8, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return PRV_OK;
} catch (...) { return caught(x && x->ctx ? x->ctx : nullptr); }

int prv_coverage_curve(prv_coverage* x, const int* order, int k, uint64_t* covered_host, uint32_t* first_seen_dev) try {
  int rc = coverage_alive(x);
  if (rc != PRV_OK) return rc;
  prv_ctx* c = x->ctx;
  if (k < 0) return fail(c, PRV_E_INVALID, "k must not be negative, got %d", k);
  if (k > 0 && (!order || !covered_host)) return fail(c, PRV_E_INVALID, "order / covered_host is NULL");
  for (int j = 0; j < k; j++)
    if (order[j] < 0 || order[j] >= x->n_views)
      return fail(c, PRV_E_INVALID, "order[%d] = %d is out of range (the handle holds %d views)", j, order[j], x->n_views);
  HIPCHK(c, hipSetDevice(c->device));
  if ((rc = check_device_ptr(c, first_seen_dev, "first_seen_dev")) != PRV_OK) return rc;
  if (first_seen_dev && x->n > 0) HIPCHK(c, hipMemsetAsync(first_seen_dev, 0xff, (size_t)x->n * 4, c->stream));
  if (k == 0) {
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return PRV_OK;
  }
  if ((rc = ensure(c, x->gain, (size_t)std::max(k, x->n_views) * 8)) != PRV_OK) return rc;
  unsigned long long* gain = (unsigned long long*)x->gain.p;
  unsigned long long* covered = (unsigned long long*)x->covered.p;
  const unsigned long long* bits = (const unsigned long long*)x->bits.p;
  HIPCHK(c, hipMemsetAsync(gain, 0, (size_t)k * 8, c->stream));
  if (x->words > 0) HIPCHK(c, hipMemsetAsync(covered, 0, x->words * 8, c->stream));
  for (int j = 0; j < k; j++) { // round j: what view order[j] adds, then the view into the covered set (a repeat adds 0)
    const unsigned long long* vb = bits + (size_t)order[j] * x->words;
    HIPCHK(c, launch_coverage_gain(vb, x->words, 1, covered, nullptr, gain + j, c->stream));
    HIPCHK(c, launch_coverage_mark(vb, x->words, covered, first_seen_dev, (uint32_t)j, nullptr, c->stream));
  }
  std::vector<unsigned long long> host((size_t)k);
  HIPCHK(c, hipMemcpyAsync(host.data(), gain, (size_t)k * 8, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  uint64_t total = 0;
  for (int j = 0; j < k; j++) covered_host[j] = (total += (uint64_t)host[(size_t)j]);
  return PRV_OK;
} catch (...) { return caught(x && x->ctx ? x->ctx : nullptr); }

int prv_coverage_greedy(prv_coverage* x, int k, int* chosen_out, uint64_t* covered_host) try {
  int rc = coverage_alive(x);
  if (rc != PRV_OK) return rc;
  prv_ctx* c = x->ctx;
  if (k < 1) return fail(c, PRV_E_INVALID, "k must be at least 1, got %d", k);
  if (k > x->n_views) return fail(c, PRV_E_INVALID, "k = %d views asked of %d", k, x->n_views);
  if (!chosen_out) return fail(c, PRV_E_INVALID, "chosen_out is NULL");
  HIPCHK(c, hipSetDevice(c->device));
  const int V = x->n_views;
  if ((rc = ensure(c, x->gain, (size_t)V * 8)) != PRV_OK) return rc;
  unsigned long long* gain = (unsigned long long*)x->gain.p;
  unsigned long long* covered = (unsigned long long*)x->covered.p;
  uint32_t* done = (uint32_t*)x->done.p;
  const unsigned long long* bits = (const unsigned long long*)x->bits.p;
  HIPCHK(c, hipMemsetAsync(done, 0, (size_t)V * 4, c->stream));
  if (x->words > 0) HIPCHK(c, hipMemsetAsync(covered, 0, x->words * 8, c->stream));
  std::vector<unsigned long long> host((size_t)V);
  std::vector<char> taken((size_t)V, 0);
  uint64_t total = 0;
  for (int round = 0; round < k; round++) {
    HIPCHK(c, hipMemsetAsync(gain, 0, (size_t)V * 8, c->stream));
    HIPCHK(c, launch_coverage_gain(bits, x->words, V, covered, done, gain, c->stream));
    HIPCHK(c, hipMemcpyAsync(host.data(), gain, (size_t)V * 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    int best = -1;
    for (int i = 0; i < V; i++) // the largest gain; on a tie the smallest position; a gain of 0 is a gain like any other
      if (!taken[(size_t)i] && (best < 0 || host[(size_t)i] > host[(size_t)best])) best = i;
    taken[(size_t)best] = 1;
    chosen_out[round] = best;
    total += (uint64_t)host[(size_t)best];
    if (covered_host) covered_host[round] = total;
    if (x->words > 0) HIPCHK(c, launch_coverage_mark(bits + (size_t)best * x->words, x->words, covered, nullptr, (uint32_t)round, done + best, c->stream));
  }
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return PRV_OK;
} catch (...) { return caught(x && x->ctx ? x->ctx : nullptr); }

void prv_coverage_destroy(prv_coverage* x) { destroy_handle(x); }

} // extern "C"
