// prv_tsdf_api.inc -- C ABI of depth-map fusion (prv_tsdf.hip); compiled as part of prv_api.cpp, after prv_mesh_api.inc and
// prv_raster_api.inc (the mesh handle, mesh_extract and raster_check_mesh's manner of refusing are theirs)

struct prv_tsdf : prv_handle {
  using prv_handle::prv_handle;
  void detach() override {
    for (Buffer* b : {&state, &counts}) b->reset();
  }
  MeshGrid g{};
  size_t n = 0; // grid points
  float trunc = 0.0f, inv = 0.0f;
  bool colors = false;
  Buffer state;  // tsdf_planes(colors) planes of n floats: D, W, WC, C[0], C[1], C[2]
  Buffer counts; // three uint64 of prv_tsdf_info
};

namespace {

int tsdf_alive(const prv_tsdf* t) { return handle_alive(t, "the volume", "the volume"); }

// views per integrate launch: kTsdfChunk, or PRV_TSDF_CHUNK (1..kTsdfChunk, read per call: tests force several launches)
int tsdf_chunk() {
  int chunk = kTsdfChunk;
  if (const char* e = getenv("PRV_TSDF_CHUNK")) chunk = (int)std::max(1ll, std::min(strtoll(e, nullptr, 10), (long long)kTsdfChunk));
  return chunk;
}

// the volume as a grid and a mask in the caller's or the call's own buffers
int tsdf_grid(prv_tsdf* t, float min_weight, float* grid, uint8_t* valid) {
  prv_ctx* c = t->ctx;
  if (!(min_weight >= 0.0f)) return fail(c, PRV_E_INVALID, "min_weight must not be negative or NaN, got %g", (double)min_weight);
  HIPCHK(c, launch_tsdf_grid((const float*)t->state.p, t->n, min_weight, grid, valid, c->stream));
  return PRV_OK;
}

} // namespace

extern "C" {

int prv_tsdf_default_opts(prv_tsdf_opts* o) {
  if (!o) return PRV_E_INVALID;
  for (int a = 0; a < 3; a++) {
    o->res[a] = 256;
    o->aabb_lo[a] = 0.0f;
    o->aabb_hi[a] = 1.0f;
  }
  o->trunc = 3.0f * (1.0f / 255.0f); // three grid steps of the default grid
  o->colors = 1;
  return PRV_OK;
}

int prv_tsdf_create(prv_ctx* c, const prv_tsdf_opts* o, prv_tsdf** out) try {
  if (out) *out = nullptr;
  if (!c) return fail(nullptr, PRV_E_INVALID, "the context is NULL");
  if (!out) return fail(c, PRV_E_INVALID, "out is NULL");
  if (!o) return fail(c, PRV_E_INVALID, "tsdf options are NULL");
  prv_mesh_opts mo; // res and aabb mean what they mean there, and are refused as they are there
  prv_mesh_default_opts(&mo);
  for (int a = 0; a < 3; a++) {
    mo.res[a] = o->res[a];
    mo.aabb_lo[a] = o->aabb_lo[a];
    mo.aabb_hi[a] = o->aabb_hi[a];
  }
  mo.threshold = 0.0f;
  int rc;
  MeshGrid g;
  if ((rc = mesh_grid(c, &mo, g)) != PRV_OK) return rc;
  if (!(o->trunc > 0.0f) || !std::isfinite(o->trunc)) return fail(c, PRV_E_INVALID, "trunc must be positive and finite, got %g", (double)o->trunc);
  HIPCHK(c, hipSetDevice(c->device));
  std::unique_ptr<prv_tsdf> t(new prv_tsdf(c));
  t->g = g;
  t->n = mesh_points(g);
  t->trunc = o->trunc;
  t->inv = 1.0f / o->trunc;
  t->colors = o->colors != 0;
  const size_t bytes = (size_t)tsdf_planes(t->colors) * t->n * 4;
  if ((rc = ensure(c, t->state, bytes)) != PRV_OK || (rc = ensure(c, t->counts, 32)) != PRV_OK) return rc;
  HIPCHK(c, hipMemsetAsync(t->state.p, 0, bytes, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  *out = t.release();
  return PRV_OK;
} catch (...) { return caught(c); }

int prv_tsdf_integrate(prv_tsdf* t, const prv_camset* cs, const int* view_ids, int n_views, int width, int height, const float* depth,
                       const float* weight, const uint8_t* rgba8) try {
  int rc = tsdf_alive(t);
  if (rc != PRV_OK) return rc;
  prv_ctx* c = t->ctx;
  if (!cs || n_views < 0) return fail(c, PRV_E_INVALID, "bad camset / view count");
  if ((rc = check_image_size(c, width, height)) != PRV_OK) return rc;
  if (n_views == 0) return PRV_OK;
  if (!depth) return fail(c, PRV_E_INVALID, "depth_dev is NULL");
  HIPCHK(c, hipSetDevice(c->device));
  if ((rc = check_device_ptr(c, depth, "depth_dev")) != PRV_OK || (rc = check_device_ptr(c, weight, "weight_dev")) != PRV_OK ||
      (rc = check_device_ptr(c, rgba8, "rgba8_dev")) != PRV_OK)
    return rc;
  if (((uintptr_t)rgba8 & 3u) != 0) return fail(c, PRV_E_INVALID, "rgba8_dev must be 4-byte aligned (a pixel is read as one word)");
  std::vector<CamDev> cams((size_t)n_views);
  if ((rc = gather_cams(c, cs, view_ids, n_views, width, height, cams.data())) != PRV_OK) return rc;
  const size_t npix = (size_t)width * (size_t)height;
  const int chunk = tsdf_chunk();
  for (int v0 = 0; v0 < n_views; v0 += chunk) {
    TsdfLaunch a;
    memset(&a, 0, sizeof(a));
    a.n_views = std::min(chunk, n_views - v0);
    a.width = width;
    a.height = height;
    a.trunc = t->trunc;
    a.inv = t->inv;
    for (int j = 0; j < a.n_views; j++) {
      const CamDev& cam = cams[(size_t)(v0 + j)];
      TsdfView& v = a.view[j];
      memcpy(v.c2w, cam.c2w, sizeof(v.c2w));
      v.fx = cam.fx, v.fy = cam.fy, v.cx = cam.cx, v.cy = cam.cy;
      memcpy(v.lens, cam.lens, sizeof(v.lens));
      v.base = (unsigned long long)(v0 + j) * npix;
    }
    HIPCHK(c, launch_tsdf_integrate(a, t->g, t->colors, (float*)t->state.p, depth, weight, (const uint32_t*)rgba8, c->stream));
  }
  HIPCHK(c, hipStreamSynchronize(c->stream)); // (the caller's images may go away)
  return PRV_OK;
} catch (...) { return caught(t && t->ctx ? t->ctx : nullptr); }

int prv_tsdf_info(prv_tsdf* t, uint64_t counts[4]) try {
  int rc = tsdf_alive(t);
  if (rc != PRV_OK) return rc;
  prv_ctx* c = t->ctx;
  if (!counts) return fail(c, PRV_E_INVALID, "counts is NULL");
  HIPCHK(c, hipSetDevice(c->device));
  unsigned long long host[3] = {0, 0, 0};
  HIPCHK(c, hipMemsetAsync(t->counts.p, 0, 24, c->stream));
  HIPCHK(c, launch_tsdf_info((const float*)t->state.p, t->n, (unsigned long long*)t->counts.p, c->stream));
  HIPCHK(c, hipMemcpyAsync(host, t->counts.p, 24, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  counts[0] = (uint64_t)t->n;
  for (int k = 0; k < 3; k++) counts[1 + k] = (uint64_t)host[k];
  return PRV_OK;
} catch (...) { return caught(t && t->ctx ? t->ctx : nullptr); }

int prv_tsdf_grid(prv_tsdf* t, float min_weight, float* grid_dev, uint8_t* valid_dev) try {
  int rc = tsdf_alive(t);
  if (rc != PRV_OK) return rc;
  prv_ctx* c = t->ctx;
  if (!grid_dev && !valid_dev) return fail(c, PRV_E_INVALID, "grid_dev and valid_dev are both NULL");
  HIPCHK(c, hipSetDevice(c->device));
  if ((rc = check_device_ptr(c, grid_dev, "grid_dev")) != PRV_OK || (rc = check_device_ptr(c, valid_dev, "valid_dev")) != PRV_OK) return rc;
  if ((rc = tsdf_grid(t, min_weight, grid_dev, valid_dev)) != PRV_OK) return rc;
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return PRV_OK;
} catch (...) { return caught(t && t->ctx ? t->ctx : nullptr); }

int prv_tsdf_mesh(prv_tsdf* t, float min_weight, prv_mesh** out) try {
  if (out) *out = nullptr;
  int rc = tsdf_alive(t);
  if (rc != PRV_OK) return rc;
  prv_ctx* c = t->ctx;
  if (!out) return fail(c, PRV_E_INVALID, "out is NULL");
  HIPCHK(c, hipSetDevice(c->device));
  MeshWork w;
  Buffer valid;
  if ((rc = mesh_events(c, w)) != PRV_OK || (rc = ensure(c, w.sigma, t->n * 4)) != PRV_OK || (rc = ensure(c, valid, t->n)) != PRV_OK) return rc;
  HIPCHK(c, hipEventRecord(w.ev[0], c->stream));
  if ((rc = tsdf_grid(t, min_weight, (float*)w.sigma.p, (uint8_t*)valid.p)) != PRV_OK) return rc;
  HIPCHK(c, hipEventRecord(w.ev[1], c->stream));
  prv_mesh* m = nullptr;
  if ((rc = mesh_extract(c, (const float*)w.sigma.p, (const uint8_t*)valid.p, t->g, 0.0f, nullptr, w, &m)) != PRV_OK) {
    (void)hipStreamSynchronize(c->stream); // (before the scratch goes)
    return rc;
  }
  std::unique_ptr<prv_mesh> owned(m);
  if (t->colors) {
    if (m->nv > 0) {
      if ((rc = ensure(c, m->rgb, m->nv * 3)) != PRV_OK) return rc;
      HIPCHK(c, launch_tsdf_colors((const float*)t->state.p, t->g, (const float*)m->xyz.p, m->nv, (uint8_t*)m->rgb.p, c->stream));
      HIPCHK(c, hipStreamSynchronize(c->stream));
    }
    m->colors = true;
  }
  *out = owned.release();
  return PRV_OK;
} catch (...) { return caught(t && t->ctx ? t->ctx : nullptr); }

int prv_debug_tsdf_state(prv_tsdf* t, float* d_host, float* w_host, float* wc_host, float* c_host) try {
  int rc = tsdf_alive(t);
  if (rc != PRV_OK) return rc;
  prv_ctx* c = t->ctx;
  HIPCHK(c, hipSetDevice(c->device));
  const float* s = (const float*)t->state.p;
  const size_t n = t->n;
  if (d_host) HIPCHK(c, hipMemcpyAsync(d_host, s, n * 4, hipMemcpyDeviceToHost, c->stream));
  if (w_host) HIPCHK(c, hipMemcpyAsync(w_host, s + n, n * 4, hipMemcpyDeviceToHost, c->stream));
  if (t->colors) {
    if (wc_host) HIPCHK(c, hipMemcpyAsync(wc_host, s + 2 * n, n * 4, hipMemcpyDeviceToHost, c->stream));
    if (c_host) HIPCHK(c, hipMemcpyAsync(c_host, s + 3 * n, 3 * n * 4, hipMemcpyDeviceToHost, c->stream));
  } else {
    if (wc_host) memset(wc_host, 0, n * 4);
    if (c_host) memset(c_host, 0, 3 * n * 4);
  }
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return PRV_OK;
} catch (...) { return caught(t && t->ctx ? t->ctx : nullptr); }

void prv_tsdf_destroy(prv_tsdf* t) { destroy_handle(t); }

} // extern "C"
