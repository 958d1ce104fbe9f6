// prv_geom_api.inc -- C ABI of the geometric evaluation (prv_geom.hip); compiled as part of prv_api.cpp after prv_mesh_api.inc
// (prv_mesh_sample reads the mesh's device buffers)

namespace {

constexpr uint64_t kGeomMaxPoints = 1ull << 31; // ids are 32 bit; the strata's k * r stays below 2^62
constexpr uint64_t kNNMaxCells = 1ull << 23;
constexpr int kNNMaxDim = 1024;

struct NNSet { // a binned (grid) or packed (brute force) reference set
  int algorithm = PRV_NN_GRID;
  uint64_t n = 0;
  NNGrid grid{};
  bool capped = false;
  Buffer rec, cell_end;
};

struct NNWork { // per-call scratch, kept by its owner between calls (grow-only)
  Buffer box, keys, count, rec, scan, misc;
};

// finite coordinates (PRV_E_INVALID otherwise) and, with box, the points' bounding box; synchronises
int nn_validate(prv_ctx* c, NNWork& w, const float* xyz, uint64_t n, const char* what, float box[6]) {
  int rc;
  if ((rc = ensure(c, w.box, (size_t)kNNBoxBlocks * 24 + 4)) != PRV_OK) return rc;
  float* partial = (float*)w.box.p;
  uint32_t* flag = (uint32_t*)(partial + (size_t)kNNBoxBlocks * 6);
  HIPCHK(c, hipMemsetAsync(flag, 0, 4, c->stream));
  HIPCHK(c, launch_nn_bbox(xyz, n, partial, flag, c->stream));
  std::vector<float> host((size_t)kNNBoxBlocks * 6 + 1);
  HIPCHK(c, hipMemcpyAsync(host.data(), partial, host.size() * 4, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  uint32_t bad;
  memcpy(&bad, &host[(size_t)kNNBoxBlocks * 6], 4);
  if (bad) return fail(c, PRV_E_INVALID, "%s hold a non-finite coordinate (NaN or Inf)", what);
  if (box) {
    for (int a = 0; a < 3; a++) {
      box[a] = INFINITY;
      box[3 + a] = -INFINITY;
    }
    for (int b = 0; b < kNNBoxBlocks; b++)
      for (int a = 0; a < 3; a++) {
        box[a] = std::min(box[a], host[(size_t)6 * b + a]);
        box[3 + a] = std::max(box[3 + a], host[(size_t)6 * b + 3 + a]);
      }
  }
  return PRV_OK;
}

// about four points per cell; an axis thinner than a cell gets one layer of cells (a plane, a line, a point all work)
void nn_make_grid(const float box[6], uint64_t n, NNGrid& g, bool& capped) {
  double target = std::max<double>(1.0, (double)n / 4.0);
  capped = target > (double)kNNMaxCells;
  if (capped) target = (double)kNNMaxCells;
  double ext[3];
  bool active[3];
  for (int a = 0; a < 3; a++) {
    ext[a] = (double)(box[3 + a] - box[a]); // the fp32 difference the kernels see
    active[a] = ext[a] > 0.0 && std::isfinite(ext[a]);
  }
  double h = 0.0;
  for (int pass = 0; pass < 3; pass++) {
    int k = 0;
    double vol = 1.0;
    for (int a = 0; a < 3; a++)
      if (active[a]) {
        k++;
        vol *= ext[a];
      }
    if (k == 0) break;
    h = std::pow(vol / target, 1.0 / k);
    bool changed = false;
    for (int a = 0; a < 3; a++)
      if (active[a] && ext[a] < h) {
        active[a] = false;
        changed = true;
      }
    if (!changed) break;
  }
  float amax = 0.0f;
  for (int a = 0; a < 3; a++) {
    int d = 1;
    if (active[a] && h > 0.0) {
      const double want = std::max(1.0, std::ceil(ext[a] / h));
      capped = capped || want > (double)kNNMaxDim;
      d = (int)std::min<double>(kNNMaxDim, want);
    }
    g.dims[a] = d;
    g.nb[a] = (d + 3) / 4;
    g.lo[a] = box[a];
    g.hi[a] = box[3 + a];
    const float e = box[3 + a] - box[a];
    float inv = d > 1 ? (float)d / e : 0.0f, cs = d > 1 ? e / (float)d : 0.0f;
    if (!std::isfinite(inv) || !(cs > 0.0f)) { // an extent so small that cells per unit length overflow (or the cell size underflows): one layer
      d = 1;
      inv = cs = 0.0f;
      g.dims[a] = 1;
      g.nb[a] = 1;
    }
    g.cs[a] = cs;
    g.inv[a] = inv;
    amax = std::max(amax, std::max(std::fabs(box[a]), std::fabs(box[3 + a])));
  }
  g.slack = amax * 0x1p-20f;
}

int nn_build(prv_ctx* c, NNWork& w, const float* xyz, uint64_t n, int algorithm, NNSet& s) {
  int rc;
  float box[6];
  if ((rc = nn_validate(c, w, xyz, n, "the reference points", box)) != PRV_OK) return rc;
  s.algorithm = algorithm;
  s.n = n;
  nn_make_grid(box, n, s.grid, s.capped);
  if ((rc = ensure(c, s.rec, n * 16)) != PRV_OK) return rc;
  if (algorithm == PRV_NN_BRUTE) {
    HIPCHK(c, launch_nn_pack(xyz, n, (float4*)s.rec.p, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return PRV_OK;
  }
  const size_t keys = nn_keys(s.grid);
  if ((rc = ensure(c, s.cell_end, keys * 8)) != PRV_OK || (rc = ensure(c, w.keys, n * 4)) != PRV_OK ||
      (rc = ensure(c, w.scan, mesh_scan_scratch(keys) * 8)) != PRV_OK || (rc = ensure(c, w.misc, 16)) != PRV_OK)
    return rc;
  uint64_t* cell = (uint64_t*)s.cell_end.p;
  HIPCHK(c, hipMemsetAsync(cell, 0, keys * 8, c->stream));
  HIPCHK(c, launch_nn_keys(s.grid, xyz, n, (uint32_t*)w.keys.p, cell, c->stream));
  HIPCHK(c, launch_mesh_scan(cell, keys, (uint64_t*)w.scan.p, (uint64_t*)w.misc.p, c->stream));
  HIPCHK(c, launch_nn_scatter(xyz, n, (const uint32_t*)w.keys.p, cell, (float4*)s.rec.p, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return PRV_OK;
}

int nn_query(prv_ctx* c, NNWork& w, const NNSet& s, const float* q, uint64_t m, float* d2, uint32_t* ids, uint64_t* tests) {
  int rc;
  if ((rc = nn_validate(c, w, q, m, "the query points", nullptr)) != PRV_OK) return rc;
  if (s.algorithm == PRV_NN_BRUTE) {
    HIPCHK(c, launch_nn_query_brute((const float4*)s.rec.p, s.n, q, m, d2, ids, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (tests) *tests = s.n * m;
    return PRV_OK;
  }
  const size_t keys = nn_keys(s.grid);
  if ((rc = ensure(c, w.keys, m * 4)) != PRV_OK || (rc = ensure(c, w.count, keys * 8)) != PRV_OK || (rc = ensure(c, w.rec, m * 16)) != PRV_OK ||
      (rc = ensure(c, w.scan, mesh_scan_scratch(keys) * 8)) != PRV_OK || (rc = ensure(c, w.misc, 16)) != PRV_OK)
    return rc;
  uint64_t* count = (uint64_t*)w.count.p;
  uint64_t* misc = (uint64_t*)w.misc.p;
  HIPCHK(c, hipMemsetAsync(count, 0, keys * 8, c->stream));
  HIPCHK(c, hipMemsetAsync(misc, 0, 16, c->stream));
  HIPCHK(c, launch_nn_keys(s.grid, q, m, (uint32_t*)w.keys.p, count, c->stream));
  HIPCHK(c, launch_mesh_scan(count, keys, (uint64_t*)w.scan.p, misc, c->stream));
  HIPCHK(c, launch_nn_scatter(q, m, (const uint32_t*)w.keys.p, count, (float4*)w.rec.p, c->stream));
  HIPCHK(c, launch_nn_query_grid(s.grid, (const float4*)s.rec.p, (const uint64_t*)s.cell_end.p, (const float4*)w.rec.p, m, d2, ids,
                                 (unsigned long long*)(misc + 1), c->stream));
  uint64_t formed = 0;
  HIPCHK(c, hipMemcpyAsync(&formed, misc + 1, 8, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  if (tests) *tests = formed;
  return PRV_OK;
}

int geom_points_arg(prv_ctx* c, const float* p, uint64_t n, const char* what) {
  if (!p) return fail(c, PRV_E_INVALID, "%s is NULL", what);
  if (n == 0) return fail(c, PRV_E_INVALID, "%s: 0 points", what);
  if (n > kGeomMaxPoints) return fail(c, PRV_E_INVALID, "%s: %llu points exceed 2^31", what, (unsigned long long)n);
  return check_device_ptr(c, p, what);
}

} // namespace

struct prv_nn_index : prv_handle {
  using prv_handle::prv_handle;
  void detach() override {
    set = NNSet{};
    work = NNWork{};
  }
  NNSet set;
  NNWork work;
  uint64_t last_tests = 0;
};

static int nn_alive(const prv_nn_index* x) { return handle_alive(x, "index", "the index"); }

static int geometry_metrics(prv_ctx* c, const float* rec, uint64_t n_rec, const float* ref, uint64_t n_ref, float tau, prv_nn_index* ref_index,
                            prv_geom_metrics* out) {
  if (!c) return PRV_E_INVALID;
  if (!out) return fail(c, PRV_E_INVALID, "out is NULL");
  if (!(tau >= 0.0f) || !std::isfinite(tau)) return fail(c, PRV_E_INVALID, "tau must be finite and >= 0, got %g", (double)tau);
  int rc;
  if ((rc = geom_points_arg(c, rec, n_rec, "rec_xyz_dev")) != PRV_OK || (rc = geom_points_arg(c, ref, n_ref, "ref_xyz_dev")) != PRV_OK) return rc;
  HIPCHK(c, hipSetDevice(c->device));
  struct {
    NNSet set;
    NNWork work;
    Buffer d2, ids, partial;
  } s;
  const uint64_t n_max = std::max(n_rec, n_ref);
  if ((rc = ensure(c, s.d2, n_max * 4)) != PRV_OK || (rc = ensure(c, s.ids, n_max * 4)) != PRV_OK ||
      (rc = ensure(c, s.partial, (size_t)(kGeomReduceBlocks + 2) * sizeof(GeomPartial))) != PRV_OK)
    return rc;
  GeomPartial* partial = (GeomPartial*)s.partial.p;
  GeomPartial host[2];
  for (int dir = 0; dir < 2; dir++) { // 0: rec -> ref (accuracy), 1: ref -> rec (completeness)
    const float* from = dir ? ref : rec;
    const float* to = dir ? rec : ref;
    const uint64_t n_from = dir ? n_ref : n_rec, n_to = dir ? n_rec : n_ref;
    if (dir == 0 && ref_index) { // the caller's index of the reference side: no rebuild
      if ((rc = nn_query(c, ref_index->work, ref_index->set, from, n_from, (float*)s.d2.p, (uint32_t*)s.ids.p, &ref_index->last_tests)) != PRV_OK)
        return rc;
    } else if ((rc = nn_build(c, s.work, to, n_to, PRV_NN_GRID, s.set)) != PRV_OK ||
               (rc = nn_query(c, s.work, s.set, from, n_from, (float*)s.d2.p, (uint32_t*)s.ids.p, nullptr)) != PRV_OK)
      return rc;
    HIPCHK(c, launch_geom_reduce((const float*)s.d2.p, n_from, tau, partial, partial + kGeomReduceBlocks + dir, c->stream));
  }
  HIPCHK(c, hipMemcpyAsync(host, partial + kGeomReduceBlocks, sizeof(host), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  out->n_rec = n_rec;
  out->n_ref = n_ref;
  out->accuracy = host[0].sum_d / (double)n_rec;
  out->completeness = host[1].sum_d / (double)n_ref;
  out->accuracy_sq = host[0].sum_d2 / (double)n_rec;
  out->completeness_sq = host[1].sum_d2 / (double)n_ref;
  out->chamfer = (out->accuracy + out->completeness) / 2.0;
  out->precision = (double)host[0].within / (double)n_rec;
  out->recall = (double)host[1].within / (double)n_ref;
  const double pr = out->precision + out->recall;
  out->fscore = pr > 0.0 ? 2.0 * out->precision * out->recall / pr : 0.0;
  out->hausdorff_rec = (double)host[0].max_d;
  out->hausdorff_ref = (double)host[1].max_d;
  return PRV_OK;
}


extern "C" {

int prv_mesh_sample(const prv_mesh* m, uint64_t n, uint64_t seed, float* out_xyz, uint32_t* out_tri) try {
  int rc = mesh_alive(m);
  if (rc != PRV_OK) return rc;
  prv_ctx* c = m->ctx;
  if (n == 0) return fail(c, PRV_E_INVALID, "n is 0: nothing to sample");
  if (n > kGeomMaxPoints) return fail(c, PRV_E_INVALID, "n = %llu exceeds 2^31 samples", (unsigned long long)n);
  if (!out_xyz) return fail(c, PRV_E_INVALID, "out_xyz_dev is NULL");
  if ((rc = check_device_ptr(c, out_xyz, "out_xyz_dev")) != PRV_OK || (rc = check_device_ptr(c, out_tri, "out_tri_dev")) != PRV_OK) return rc;
  if (m->nt == 0) return fail(c, PRV_E_STATE, "the mesh has no triangles: nothing to sample");
  HIPCHK(c, hipSetDevice(c->device));
  Buffer scan, scratch, total;
  if ((rc = ensure(c, scan, m->nt * 8)) != PRV_OK || (rc = ensure(c, scratch, mesh_scan_scratch(m->nt) * 8)) != PRV_OK ||
      (rc = ensure(c, total, 8)) != PRV_OK)
    return rc;
  HIPCHK(c, launch_geom_tri_weights((const float*)m->xyz.p, (const uint32_t*)m->tri.p, m->nt, (uint64_t*)scan.p, c->stream));
  HIPCHK(c, launch_mesh_scan((uint64_t*)scan.p, m->nt, (uint64_t*)scratch.p, (uint64_t*)total.p, c->stream));
  uint64_t W = 0;
  HIPCHK(c, hipMemcpyAsync(&W, total.p, 8, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  if (W == 0) return fail(c, PRV_E_STATE, "the mesh has no area: every triangle is degenerate");
  if (W >= (1ull << 62)) return fail(c, PRV_E_INVALID, "the mesh's area exceeds the weight range (2^22 unit areas)");
  HIPCHK(c, launch_geom_sample((const float*)m->xyz.p, (const uint32_t*)m->tri.p, (const uint64_t*)scan.p, m->nt, W, n, seed, out_xyz, out_tri,
                               c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return PRV_OK;
} catch (...) { return caught(m && m->ctx ? m->ctx : nullptr); }

int prv_nn_default_opts(prv_nn_opts* o) {
  if (!o) return PRV_E_INVALID;
  o->algorithm = PRV_NN_GRID;
  o->reserved = 0;
  return PRV_OK;
}

int prv_nn_index_create(prv_ctx* c, const float* xyz, uint64_t n, const prv_nn_opts* o, prv_nn_index** out) try {
  if (!c) return PRV_E_INVALID;
  if (!out) return fail(c, PRV_E_INVALID, "out is NULL");
  *out = nullptr;
  const int algorithm = o ? o->algorithm : PRV_NN_GRID;
  if (algorithm != PRV_NN_GRID && algorithm != PRV_NN_BRUTE) return fail(c, PRV_E_INVALID, "unknown algorithm %d", algorithm);
  int rc;
  if ((rc = geom_points_arg(c, xyz, n, "xyz_dev")) != PRV_OK) return rc;
  HIPCHK(c, hipSetDevice(c->device));
  std::unique_ptr<prv_nn_index> x(new prv_nn_index(c));
  if ((rc = nn_build(c, x->work, xyz, n, algorithm, x->set)) != PRV_OK) return rc;
  x->work.keys.reset(); // the build's point keys; a query sizes its own
  *out = x.release();
  return PRV_OK;
} catch (...) { return caught(c); }

int prv_nn_query(prv_nn_index* x, const float* q, uint64_t m, float* out_d2, uint32_t* out_id) try {
  int rc = nn_alive(x);
  if (rc != PRV_OK) return rc;
  prv_ctx* c = x->ctx;
  if ((rc = geom_points_arg(c, q, m, "query_xyz_dev")) != PRV_OK) return rc;
  if (!out_d2 || !out_id) return fail(c, PRV_E_INVALID, "out_d2_dev / out_id_dev is NULL");
  if ((rc = check_device_ptr(c, out_d2, "out_d2_dev")) != PRV_OK || (rc = check_device_ptr(c, out_id, "out_id_dev")) != PRV_OK) return rc;
  HIPCHK(c, hipSetDevice(c->device));
  return nn_query(c, x->work, x->set, q, m, out_d2, out_id, &x->last_tests);
} catch (...) { return caught(x && x->ctx ? x->ctx : nullptr); }

int prv_nn_index_info(const prv_nn_index* x, uint64_t* n, int32_t dims[3], int32_t* capped) {
  const int rc = nn_alive(x);
  if (rc != PRV_OK) return rc;
  if (n) *n = x->set.n;
  for (int a = 0; dims && a < 3; a++) dims[a] = x->set.algorithm == PRV_NN_GRID ? x->set.grid.dims[a] : 0;
  if (capped) *capped = x->set.algorithm == PRV_NN_GRID && x->set.capped;
  return PRV_OK;
}

int prv_debug_nn_tests(const prv_nn_index* x, uint64_t* tests) {
  const int rc = nn_alive(x);
  if (rc != PRV_OK) return rc;
  if (!tests) return PRV_E_INVALID;
  *tests = x->last_tests;
  return PRV_OK;
}

void prv_nn_index_destroy(prv_nn_index* x) { destroy_handle(x); }

int prv_geometry_metrics(prv_ctx* c, const float* rec, uint64_t n_rec, const float* ref, uint64_t n_ref, float tau,
                         prv_geom_metrics* out) try {
  return geometry_metrics(c, rec, n_rec, ref, n_ref, tau, nullptr, out);
} catch (...) { return caught(c); }

int prv_geometry_metrics_indexed(prv_ctx* c, const float* rec, uint64_t n_rec, prv_nn_index* ref_index, const float* ref, uint64_t n_ref,
                                 float tau, prv_geom_metrics* out) try {
  if (!c) return PRV_E_INVALID;
  const int rc = nn_alive(ref_index);
  if (rc != PRV_OK) return fail(c, rc, "%s", prv_last_error(nullptr));
  if (ref_index->ctx != c) return fail(c, PRV_E_INVALID, "the index belongs to another context");
  if (ref_index->set.n != n_ref) return fail(c, PRV_E_INVALID, "the index holds %llu points, n_ref is %llu", (unsigned long long)ref_index->set.n, (unsigned long long)n_ref);
  return geometry_metrics(c, rec, n_rec, ref, n_ref, tau, ref_index, out);
} catch (...) { return caught(c); }

} // extern "C"
