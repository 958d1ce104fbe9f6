// prv_raster_api.inc -- C ABI of the triangle rasteriser (prv_raster.hip): prv_mesh_from_arrays, prv_mesh_depth, and the depth
// buffers that prv_coverage_create_occluded (prv_coverage_api.inc) builds its visibility on; compiled as part of prv_api.cpp

namespace {

constexpr uint64_t kMeshFromArraysMost = 1ull << 31;

// the views of a call in batches that fit the coverage stage's z-buffer budget (PRV_COVERAGE_ZBUF_BYTES: tests)
int zbuf_views_per_batch(int n_views, size_t npix, size_t key_bytes = 4) {
  size_t budget = kCoverageZBufBudget;
  if (const char* e = getenv("PRV_COVERAGE_ZBUF_BYTES")) budget = (size_t)strtoull(e, nullptr, 10);
  return (int)std::max<size_t>(1, std::min<size_t>(std::min<size_t>((size_t)n_views, (size_t)kCoverageMaxBatch), budget / (npix * key_bytes)));
}

int raster_refuse_lenses(prv_ctx* c, const CamDev* cams, int n) {
  for (int i = 0; i < n; i++)
    if (cams[i].lens[0] != 0.0f || cams[i].lens[1] != 0.0f || cams[i].lens[2] != 0.0f || cams[i].lens[3] != 0.0f)
      return fail(c, PRV_E_INVALID, "view %d of the list has a lens: a mesh is rasterised for pinhole cameras only (a straight edge does not stay straight)", i);
  return PRV_OK;
}

int raster_check_mesh(prv_ctx* c, const prv_mesh* m, const char* what) {
  if (!m) return fail(c, PRV_E_INVALID, "%s is NULL", what);
  if (!m->ctx) return fail(nullptr, PRV_E_STATE, "the mesh's context has been destroyed");
  if (m->ctx != c) return fail(c, PRV_E_INVALID, "%s belongs to another context", what);
  return PRV_OK;
}

// the deferred list and its counters, for the length of one call
struct RasterWork {
  Buffer list, counters; // counters: uint32 count of the launch in flight at byte 0, uint64 deferred pairs of the call at byte 8
  size_t capacity = 0;
  int small_max = kRasterSmallPixels;
  uint64_t pairs = 0; // (view, triangle) pairs rasterised so far
};

int raster_begin(prv_ctx* c, RasterWork& w, const prv_mesh* m, int views_per_batch) {
  size_t cap = kRasterListEntries;
  if (const char* e = getenv("PRV_RASTER_LIST_ENTRIES")) cap = (size_t)strtoull(e, nullptr, 10); // tests: many chunks of a small mesh
  if (const char* e = getenv("PRV_RASTER_SMALL_PIXELS")) w.small_max = (int)std::max(0ll, std::min(strtoll(e, nullptr, 10), 0x7fffffffll));
  cap = std::max<size_t>(1, std::min<size_t>(cap, kRasterListEntriesMost));
  w.capacity = std::max<size_t>(1, std::min<size_t>(cap, (size_t)m->nt * (size_t)std::max(1, views_per_batch))); // never more than the pairs of a batch
  int rc;
  if ((rc = ensure(c, w.list, w.capacity * sizeof(RasterPair))) != PRV_OK || (rc = ensure(c, w.counters, 16)) != PRV_OK) return rc;
  HIPCHK(c, hipMemsetAsync(w.counters.p, 0, 16, c->stream));
  return PRV_OK;
}

// zbuf = the depth buffers (Key = uint32_t) or the visibility buffers (Key = unsigned long long) of the nb views of cams_dev:
// cleared to all ones, then every triangle of the mesh, chunk by chunk
template <typename Key>
int raster_fill(prv_ctx* c, RasterWork& w, const prv_mesh* m, const CamDev* cams_dev, int nb, int W, int H, Key* zbuf) {
  const size_t npix = (size_t)W * (size_t)H;
  HIPCHK(c, hipMemsetAsync(zbuf, 0xff, (size_t)nb * npix * sizeof(Key), c->stream));
  if (m->nt == 0) return PRV_OK;
  const int vsub = (int)std::min<size_t>((size_t)nb, w.capacity); // a capacity below the batch: fewer views per launch
  for (int v0 = 0; v0 < nb; v0 += vsub) {
    const int nv = std::min(vsub, nb - v0);
    const size_t chunk = std::min<size_t>(w.capacity / (size_t)nv, (size_t)m->nt); // chunk x views <= capacity
    for (size_t t0 = 0; t0 < (size_t)m->nt; t0 += chunk) {
      const size_t n = std::min(chunk, (size_t)m->nt - t0);
      HIPCHK(c, launch_raster((const float*)m->xyz.p, (const uint32_t*)m->tri.p, t0, n, cams_dev + v0, nv, W, H, w.small_max,
                              (RasterPair*)w.list.p, w.capacity, (uint32_t*)w.counters.p, (unsigned long long*)((char*)w.counters.p + 8),
                              zbuf + (size_t)v0 * npix, c->stream));
    }
  }
  w.pairs += (uint64_t)m->nt * (uint64_t)nb;
  return PRV_OK;
}

// the call's counts -> the context (prv_debug_raster_stats); synchronises
int raster_end(prv_ctx* c, RasterWork& w) {
  unsigned long long large = 0;
  HIPCHK(c, hipMemcpyAsync(&large, (char*)w.counters.p + 8, 8, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  c->raster_stats[0] = w.pairs;
  c->raster_stats[1] = (uint64_t)large;
  return PRV_OK;
}

} // namespace

extern "C" {

int prv_mesh_from_arrays(prv_ctx* c, const float* xyz, uint64_t nv, const uint32_t* tri, uint64_t nt, prv_mesh** out) try {
  if (out) *out = nullptr;
  if (!c) return fail(nullptr, PRV_E_INVALID, "the context is NULL");
  if (!out) return fail(c, PRV_E_INVALID, "out is NULL");
  if (nv > kMeshFromArraysMost || nt > kMeshFromArraysMost)
    return fail(c, PRV_E_INVALID, "%llu vertices / %llu triangles exceed 2^31", (unsigned long long)nv, (unsigned long long)nt);
  if (nv > 0 && !xyz) return fail(c, PRV_E_INVALID, "xyz_host is NULL with %llu vertices", (unsigned long long)nv);
  if (nt > 0 && !tri) return fail(c, PRV_E_INVALID, "tri_host is NULL with %llu triangles", (unsigned long long)nt);
  for (uint64_t i = 0; i < 3 * nv; i++)
    if (!std::isfinite(xyz[i]))
      return fail(c, PRV_E_INVALID, "vertex %llu has a coordinate that is not finite", (unsigned long long)(i / 3));
  for (uint64_t i = 0; i < 3 * nt; i++)
    if (tri[i] >= nv)
      return fail(c, PRV_E_INVALID, "triangle %llu: vertex id %u out of range (%llu vertices)", (unsigned long long)(i / 3), tri[i], (unsigned long long)nv);
  HIPCHK(c, hipSetDevice(c->device));
  std::unique_ptr<prv_mesh> m(new prv_mesh(c)); // an early return below frees what it holds by then
  m->nv = nv;
  m->nt = nt;
  m->colors = false;
  if (nv > 0) { // (as the extraction allocates: nothing for a mesh without vertices, one triangle's room for one without triangles)
    int rc;
    if ((rc = ensure(c, m->xyz, nv * 12)) != PRV_OK || (rc = ensure(c, m->nrm, nv * 12)) != PRV_OK ||
        (rc = ensure(c, m->tri, std::max<uint64_t>(1, nt) * 12)) != PRV_OK)
      return rc;
    hipError_t e = hipMemcpyAsync(m->xyz.p, xyz, nv * 12, hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess) e = hipMemsetAsync(m->nrm.p, 0, nv * 12, c->stream);
    if (e == hipSuccess) e = hipMemsetAsync(m->tri.p, 0, std::max<uint64_t>(1, nt) * 12, c->stream);
    if (e == hipSuccess && nt > 0) e = hipMemcpyAsync(m->tri.p, tri, nt * 12, hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream); // (the host arrays may go away)
    if (e != hipSuccess) return fail(c, PRV_E_HIP, "mesh upload failed: %s", hipGetErrorString(e));
  }
  *out = m.release();
  return PRV_OK;
} catch (...) { return caught(c); }

int prv_mesh_depth(prv_ctx* c, const prv_mesh* m, const prv_camset* cs, const int* view_ids, int n_views, int width, int height,
                   float* depth_out) try {
  if (!c) return fail(nullptr, PRV_E_INVALID, "the context is NULL");
  int rc;
  if ((rc = raster_check_mesh(c, m, "mesh")) != PRV_OK) return rc;
  if (!cs || n_views < 1) return fail(c, PRV_E_INVALID, "bad camset / view count");
  if ((rc = check_image_size(c, width, height)) != PRV_OK) return rc;
  if (!depth_out) return fail(c, PRV_E_INVALID, "depth_out_dev is NULL");
  HIPCHK(c, hipSetDevice(c->device));
  if ((rc = check_device_ptr(c, depth_out, "depth_out_dev")) != PRV_OK) return rc;
  Upload up; // staged here, sent below: a bad view id or a lens is reported before any allocation can fail
  if ((rc = stage_views(c, cs, view_ids, n_views, width, height, nullptr, up)) != PRV_OK || (rc = raster_refuse_lenses(c, up.cams, n_views)) != PRV_OK) return rc;
  const size_t npix = (size_t)width * (size_t)height;
  const int per_batch = zbuf_views_per_batch(n_views, npix);
  Buffer z;
  RasterWork w;
  if ((rc = ensure(c, z, (size_t)per_batch * npix * 4)) != PRV_OK || (rc = raster_begin(c, w, m, per_batch)) != PRV_OK) return rc;
  if ((rc = send_views(c, up)) != PRV_OK) return rc;
  uint32_t* zbuf = (uint32_t*)z.p;
  for (int v0 = 0; v0 < n_views; v0 += per_batch) {
    const int nb = std::min(per_batch, n_views - v0);
    if ((rc = raster_fill(c, w, m, up.cams_dev + v0, nb, width, height, zbuf)) != PRV_OK) break;
    hipError_t e = launch_coverage_resolve(zbuf, (size_t)nb * npix, depth_out + (size_t)v0 * npix, c->stream);
    if (e != hipSuccess) {
      rc = fail(c, PRV_E_HIP, "mesh depth failed: %s", hipGetErrorString(e));
      break;
    }
  }
  if (rc != PRV_OK) {
    (void)hipStreamSynchronize(c->stream); // (the scratch goes away)
    return rc;
  }
  return raster_end(c, w);
} catch (...) { return caught(c); }

int prv_debug_raster_stats(prv_ctx* c, uint64_t out[2]) {
  if (!c || !out) return PRV_E_INVALID;
  out[0] = c->raster_stats[0];
  out[1] = c->raster_stats[1];
  return PRV_OK;
}

} // extern "C"
