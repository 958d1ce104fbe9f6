// prv_raster_color_api.inc -- C ABI of the colour images of a mesh (prv_raster.hip, "mesh colour images" in include/prv.h):
// prv_mesh_set_colors and prv_mesh_render, on the helpers of prv_raster_api.inc; compiled as part of prv_api.cpp

extern "C" {

int prv_mesh_set_colors(prv_mesh* m, const uint8_t* rgb, uint64_t nv) try {
  int rc = mesh_alive(m);
  if (rc != PRV_OK) return rc;
  prv_ctx* c = m->ctx;
  if (nv != m->nv)
    return fail(c, PRV_E_INVALID, "%llu colours for a mesh of %llu vertices", (unsigned long long)nv, (unsigned long long)m->nv);
  if (nv > 0 && !rgb) return fail(c, PRV_E_INVALID, "rgb_host is NULL with %llu vertices", (unsigned long long)nv);
  HIPCHK(c, hipSetDevice(c->device));
  if (nv > 0) {
    if ((rc = ensure(c, m->rgb, nv * 3)) != PRV_OK) return rc;
    HIPCHK(c, hipMemcpyAsync(m->rgb.p, rgb, nv * 3, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream)); // (the host array may go away)
  }
  m->colors = true;
  return PRV_OK;
} catch (...) { return caught(m && m->ctx ? m->ctx : nullptr); }

int prv_mesh_render(prv_ctx* c, const prv_mesh* m, const prv_camset* cs, const int* view_ids, int n_views, int width, int height,
                    int flip180, uint8_t* out, float* depth_out, uint32_t* tri_out) try {
  if (!c) return fail(nullptr, PRV_E_INVALID, "the context is NULL");
  int rc;
  if ((rc = raster_check_mesh(c, m, "mesh")) != PRV_OK) return rc;
  if (!cs || n_views < 1) return fail(c, PRV_E_INVALID, "bad camset / view count");
  if ((rc = check_image_size(c, width, height)) != PRV_OK) return rc;
  if (!out) return fail(c, PRV_E_INVALID, "out_rgba8_dev is NULL");
  if (!m->colors) return fail(c, PRV_E_INVALID, "the mesh has no colours: call prv_mesh_set_colors first (or extract it with colours)");
  HIPCHK(c, hipSetDevice(c->device));
  if ((rc = check_device_ptr(c, out, "out_rgba8_dev")) != PRV_OK || (depth_out && (rc = check_device_ptr(c, depth_out, "depth_out_dev")) != PRV_OK) ||
      (tri_out && (rc = check_device_ptr(c, tri_out, "tri_out_dev")) != PRV_OK))
    return rc;
  Upload up; // staged here, sent below: a bad view id or a lens is reported before any allocation can fail
  if ((rc = stage_views(c, cs, view_ids, n_views, width, height, nullptr, up)) != PRV_OK || (rc = raster_refuse_lenses(c, up.cams, n_views)) != PRV_OK) return rc;
  const size_t npix = (size_t)width * (size_t)height;
  const int per_batch = zbuf_views_per_batch(n_views, npix, 8);
  Buffer z;
  RasterWork w;
  if ((rc = ensure(c, z, (size_t)per_batch * npix * 8)) != PRV_OK || (rc = raster_begin(c, w, m, per_batch)) != PRV_OK) return rc;
  if ((rc = send_views(c, up)) != PRV_OK) return rc;
  unsigned long long* keys = (unsigned long long*)z.p;
  for (int v0 = 0; v0 < n_views; v0 += per_batch) {
    const int nb = std::min(per_batch, n_views - v0);
    const CamDev* bc = up.cams_dev + v0;
    if ((rc = raster_fill(c, w, m, bc, nb, width, height, keys)) != PRV_OK) break;
    hipError_t e = launch_raster_shade((const float*)m->xyz.p, (const uint32_t*)m->tri.p, (const uint8_t*)m->rgb.p, bc, nb, width, height, keys,
                                       flip180, (uint32_t*)out + (size_t)v0 * npix, depth_out ? depth_out + (size_t)v0 * npix : nullptr,
                                       tri_out ? tri_out + (size_t)v0 * npix : nullptr, c->stream);
    if (e != hipSuccess) {
      rc = fail(c, PRV_E_HIP, "mesh render failed: %s", hipGetErrorString(e));
      break;
    }
  }
  if (rc != PRV_OK) {
    (void)hipStreamSynchronize(c->stream); // (the scratch goes away)
    return rc;
  }
  return raster_end(c, w);
} catch (...) { return caught(c); }

} // extern "C"
