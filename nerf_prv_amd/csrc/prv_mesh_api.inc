// prv_mesh_api.inc -- C ABI of mesh extraction (prv_mesh.hip); compiled as part of prv_api.cpp (shares its context types)
#include <cctype>

struct prv_mesh : prv_handle {
  using prv_handle::prv_handle;
  void detach() override {
    for (Buffer* b : {&xyz, &nrm, &rgb, &tri, &vcomp, &tcomp}) b->reset();
  }
  uint64_t nv = 0, nt = 0;
  bool colors = false;
  Buffer xyz, nrm, rgb, tri;
  // connected components (prv_mesh_components): labelled once, then cached here
  bool labelled = false;
  int label_rounds = 0;
  Buffer vcomp, tcomp; // component id per vertex / per triangle
  std::vector<prv_mesh_component> comps;
};

namespace {

constexpr int kMeshMaxRes = 1024;
constexpr uint64_t kMeshMaxPoints = 1ull << 30;

int mesh_grid(prv_ctx* c, const prv_mesh_opts* o, MeshGrid& g) {
  if (!o) return fail(c, PRV_E_INVALID, "mesh options are NULL");
  uint64_t n = 1;
  for (int a = 0; a < 3; a++) {
    if (o->res[a] < 2 || o->res[a] > kMeshMaxRes)
      return fail(c, PRV_E_INVALID, "res[%d] must be in [2,%d], got %d", a, kMeshMaxRes, o->res[a]);
    n *= (uint64_t)o->res[a];
    const float lo = o->aabb_lo[a], hi = o->aabb_hi[a];
    if (!(lo >= 0.0f && lo < hi && hi <= 1.0f))
      return fail(c, PRV_E_INVALID, "aabb axis %d must satisfy 0 <= lo < hi <= 1, got [%g, %g]", a, (double)lo, (double)hi);
    g.res[a] = o->res[a];
    g.lo[a] = lo;
    g.step[a] = (hi - lo) / (float)(o->res[a] - 1);
  }
  if (n > kMeshMaxPoints) return fail(c, PRV_E_INVALID, "res product %llu exceeds 2^30 grid points", (unsigned long long)n);
  if (!std::isfinite(o->threshold)) return fail(c, PRV_E_INVALID, "threshold must be finite, got %g", (double)o->threshold);
  return PRV_OK;
}

struct MeshWork { // the extraction's scratch and its events
  Buffer sigma, flags, cases, kept, wave_v, wave_t, scratch, totals;
  // stage brackets: [0, 1] density grid, [1, 2] classify + scans, [3, 4] emit, [4, 5] colours (the readback sits in [2, 3])
  hipEvent_t ev[6] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
  ~MeshWork() {
    for (hipEvent_t e : ev)
      if (e) (void)hipEventDestroy(e);
  }
};

// sigma grid -> mesh; fd != nullptr: vertex colours from that field; valid != nullptr: only cells whose eight corners are valid
// give triangles (prv_marching_cubes_grid_valid).  The caller has recorded w.ev[0] and w.ev[1].
int mesh_extract(prv_ctx* c, const float* sigma, const uint8_t* valid, const MeshGrid& g, float thr, const FieldDev* fd, MeshWork& w,
                 prv_mesh** out) {
  const size_t waves = mesh_waves(g);
  int rc;
  if (valid) {
    if ((rc = ensure(c, w.kept, waves * 64)) != PRV_OK) return rc;
    HIPCHK(c, launch_mesh_kept(valid, g, (uint8_t*)w.kept.p, c->stream));
  }
  if ((rc = ensure(c, w.flags, waves * 64)) != PRV_OK || (rc = ensure(c, w.cases, waves * 64)) != PRV_OK ||
      (rc = ensure(c, w.wave_v, waves * 8)) != PRV_OK || (rc = ensure(c, w.wave_t, waves * 8)) != PRV_OK ||
      (rc = ensure(c, w.scratch, mesh_scan_scratch(waves) * 8)) != PRV_OK || (rc = ensure(c, w.totals, 16)) != PRV_OK)
    return rc;
  uint64_t* tot = (uint64_t*)w.totals.p;
  HIPCHK(c, launch_mesh_classify(sigma, g, thr, valid ? (const uint8_t*)w.kept.p : nullptr, (uint8_t*)w.flags.p, (uint8_t*)w.cases.p,
                                 (uint64_t*)w.wave_v.p, (uint64_t*)w.wave_t.p, c->stream));
  HIPCHK(c, launch_mesh_scan((uint64_t*)w.wave_v.p, waves, (uint64_t*)w.scratch.p, tot, c->stream));
  HIPCHK(c, launch_mesh_scan((uint64_t*)w.wave_t.p, waves, (uint64_t*)w.scratch.p, tot + 1, c->stream));
  HIPCHK(c, hipEventRecord(w.ev[2], c->stream));
  uint64_t totals[2] = {0, 0};
  HIPCHK(c, hipMemcpyAsync(totals, tot, 16, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  if (totals[0] >= (1ull << 32)) return fail(c, PRV_E_INTERNAL, "%llu vertices do not fit 32-bit ids", (unsigned long long)totals[0]);
  std::unique_ptr<prv_mesh> m(new prv_mesh(c)); // an early return below frees what it holds by then
  m->nv = totals[0];
  m->nt = totals[1];
  m->colors = fd != nullptr;
  if (m->nv > 0) {
    if ((rc = ensure(c, m->xyz, m->nv * 12)) != PRV_OK || (rc = ensure(c, m->nrm, m->nv * 12)) != PRV_OK ||
        (fd && (rc = ensure(c, m->rgb, m->nv * 3)) != PRV_OK) || (rc = ensure(c, m->tri, std::max<uint64_t>(1, m->nt) * 12)) != PRV_OK)
      return rc;
    HIPCHK(c, hipEventRecord(w.ev[3], c->stream));
    hipError_t e = launch_mesh_vertices(sigma, g, thr, (const uint8_t*)w.flags.p, (const uint64_t*)w.wave_v.p, (float*)m->xyz.p,
                                        (float*)m->nrm.p, c->stream);
    if (e == hipSuccess && m->nt > 0)
      e = launch_mesh_triangles(g, (const uint8_t*)w.flags.p, (const uint8_t*)w.cases.p, (const uint64_t*)w.wave_v.p,
                                (const uint64_t*)w.wave_t.p, (uint32_t*)m->tri.p, c->stream);
    if (e == hipSuccess) e = hipEventRecord(w.ev[4], c->stream);
    if (e == hipSuccess && fd) e = launch_mesh_colors(*fd, (const float*)m->xyz.p, (const float*)m->nrm.p, m->nv, (uint8_t*)m->rgb.p, c->stream);
    if (e == hipSuccess) e = hipEventRecord(w.ev[5], c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (e != hipSuccess) return fail(c, PRV_E_HIP, "mesh emit failed: %s", hipGetErrorString(e));
  } else {
    for (int k = 3; k < 6; k++) HIPCHK(c, hipEventRecord(w.ev[k], c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
  }
  float ms[4] = {0, 0, 0, 0};
  const int from[4] = {0, 1, 3, 4};
  for (int k = 0; k < 4; k++)
    if (hipEventElapsedTime(&ms[k], w.ev[from[k]], w.ev[from[k] + 1]) != hipSuccess) (void)hipGetLastError();
  memcpy(c->mesh_ms, ms, sizeof(ms));
  *out = m.release();
  return PRV_OK;
}

int mesh_events(prv_ctx* c, MeshWork& w) {
  for (hipEvent_t& e : w.ev) HIPCHK(c, hipEventCreate(&e));
  return PRV_OK;
}

int mesh_alive(const prv_mesh* m) { return handle_alive(m, "mesh", "the mesh"); }

// ---- connected components
struct CompWork { // labelling / filter scratch
  Buffer parent, wave_v, wave_t, scratch, misc, table, keep, vmap;
};

float comp_key_float(uint32_t k) { // undoes the kernels' order-preserving image
  const uint32_t b = k ^ ((k >> 31) ? 0x80000000u : 0xFFFFFFFFu);
  float f;
  memcpy(&f, &b, 4);
  return f;
}

// labels the mesh (once): m->vcomp, m->tcomp, m->comps
int mesh_label(prv_mesh* m) {
  if (m->labelled) return PRV_OK;
  prv_ctx* c = m->ctx;
  HIPCHK(c, hipSetDevice(c->device));
  m->comps.clear();
  m->label_rounds = 0;
  if (m->nv == 0) {
    m->labelled = true;
    return PRV_OK;
  }
  CompWork w;
  const size_t waves = mesh_comp_waves(m->nv);
  int rc;
  if ((rc = ensure(c, w.parent, m->nv * 4)) != PRV_OK || (rc = ensure(c, w.wave_v, waves * 8)) != PRV_OK ||
      (rc = ensure(c, w.scratch, mesh_scan_scratch(waves) * 8)) != PRV_OK || (rc = ensure(c, w.misc, 16)) != PRV_OK ||
      (rc = ensure(c, m->vcomp, m->nv * 4)) != PRV_OK || (rc = ensure(c, m->tcomp, std::max<uint64_t>(1, m->nt) * 4)) != PRV_OK)
    return rc;
  uint32_t* parent = (uint32_t*)w.parent.p;
  uint64_t* total = (uint64_t*)w.misc.p;
  uint32_t* changed = (uint32_t*)(total + 1);
  HIPCHK(c, launch_mesh_comp_init(parent, m->nv, c->stream));
  int rounds = 0;
  while (m->nt > 0) { // hook, read the flag back, compress: until a hook pass finds every triangle under one root
    rounds++;
    uint32_t flag = 0;
    HIPCHK(c, hipMemsetAsync(changed, 0, 4, c->stream));
    HIPCHK(c, launch_mesh_comp_hook((const uint32_t*)m->tri.p, m->nt, parent, changed, c->stream));
    HIPCHK(c, hipMemcpyAsync(&flag, changed, 4, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (!flag) break; // nothing hooked since the last compress: parent[] is flat
    if (rounds >= kMeshComponentMaxRounds)
      return fail(c, PRV_E_INTERNAL, "component labelling did not settle in %d rounds (%llu vertices, %llu triangles)", kMeshComponentMaxRounds,
                  (unsigned long long)m->nv, (unsigned long long)m->nt);
    HIPCHK(c, launch_mesh_comp_compress(parent, m->nv, c->stream));
  }
  HIPCHK(c, launch_mesh_comp_roots(parent, m->nv, (uint64_t*)w.wave_v.p, c->stream));
  HIPCHK(c, launch_mesh_scan((uint64_t*)w.wave_v.p, waves, (uint64_t*)w.scratch.p, total, c->stream));
  uint64_t nc = 0;
  HIPCHK(c, hipMemcpyAsync(&nc, total, 8, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  if (nc == 0 || nc > m->nv) return fail(c, PRV_E_INTERNAL, "%llu components of %llu vertices", (unsigned long long)nc, (unsigned long long)m->nv);
  if ((rc = ensure(c, w.table, nc * sizeof(MeshComponentDev))) != PRV_OK) return rc;
  HIPCHK(c, launch_mesh_comp_table(parent, (const uint64_t*)w.wave_v.p, (const float*)m->xyz.p, m->nv, (const uint32_t*)m->tri.p, m->nt,
                                   (uint32_t*)m->vcomp.p, (uint32_t*)m->tcomp.p, (MeshComponentDev*)w.table.p, c->stream));
  std::vector<MeshComponentDev> dev(nc);
  HIPCHK(c, hipMemcpyAsync(dev.data(), w.table.p, nc * sizeof(MeshComponentDev), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  m->comps.resize(nc);
  for (uint64_t i = 0; i < nc; i++) {
    prv_mesh_component& o = m->comps[i];
    o.first_vertex = dev[i].first_vertex;
    o.reserved = 0;
    o.n_vertices = dev[i].n_vertices;
    o.n_triangles = dev[i].n_triangles;
    for (int a = 0; a < 3; a++) {
      o.lo[a] = comp_key_float(dev[i].lo[a]);
      o.hi[a] = comp_key_float(dev[i].hi[a]);
    }
  }
  m->label_rounds = rounds;
  m->labelled = true;
  return PRV_OK;
}

// the filter's rule (include/prv.h): one keep byte per component
std::vector<uint8_t> comp_keep(const std::vector<prv_mesh_component>& comps, const prv_mesh_filter_opts& o) {
  const size_t nc = comps.size();
  std::vector<uint8_t> keep(nc, 1);
  if (o.min_triangles > 0)
    for (size_t i = 0; i < nc; i++) keep[i] = comps[i].n_triangles >= o.min_triangles;
  if (o.keep_largest > 0) {
    std::vector<size_t> order;
    for (size_t i = 0; i < nc; i++)
      if (keep[i]) order.push_back(i);
    std::stable_sort(order.begin(), order.end(), [&](size_t a, size_t b) { return comps[a].n_triangles > comps[b].n_triangles; });
    for (size_t k = o.keep_largest; k < order.size(); k++) keep[order[k]] = 0;
  }
  if (o.min_diagonal > 0.0f)
    for (size_t i = 0; i < nc; i++) {
      const double dx = (double)comps[i].hi[0] - (double)comps[i].lo[0], dy = (double)comps[i].hi[1] - (double)comps[i].lo[1],
                   dz = (double)comps[i].hi[2] - (double)comps[i].lo[2];
      if (std::sqrt((dx * dx + dy * dy) + dz * dz) < (double)o.min_diagonal) keep[i] = 0;
    }
  return keep;
}

// ---- file writer (host only)
bool ends_with_ci(const char* s, const char* suffix) {
  const size_t n = strlen(s), k = strlen(suffix);
  if (n < k) return false;
  for (size_t i = 0; i < k; i++)
    if (tolower((unsigned char)s[n - k + i]) != suffix[i]) return false;
  return true;
}

int write_mesh_file(const char* path, uint64_t nv, const float* xyz, const float* nrm, const uint8_t* rgb, uint64_t nt,
                    const uint32_t* tri, double scale, const double offset[3]) {
  if (!path) return fail(nullptr, PRV_E_INVALID, "path is NULL");
  const bool ply = ends_with_ci(path, ".ply"), obj = ends_with_ci(path, ".obj");
  if (!ply && !obj) return fail(nullptr, PRV_E_INVALID, "%s: mesh files are .ply or .obj", path);
  if (!(scale > 0.0) || !std::isfinite(scale)) return fail(nullptr, PRV_E_INVALID, "scale must be positive and finite, got %g", scale);
  if ((nv > 0 && !xyz) || (nt > 0 && !tri)) return fail(nullptr, PRV_E_INVALID, "NULL vertex or triangle array");
  for (uint64_t i = 0; i < 3 * nt; i++)
    if (tri[i] >= nv) return fail(nullptr, PRV_E_INVALID, "triangle vertex id %u out of range (%llu vertices)", tri[i], (unsigned long long)nv);
  const double off[3] = {offset ? offset[0] : 0.0, offset ? offset[1] : 0.0, offset ? offset[2] : 0.0};
  // engine e -> dataset: q = (e2, e0, e1), (q - offset) / scale; normals: the same cycle
  auto pos = [&](uint64_t i, float p[3]) {
    const float* e = xyz + 3 * i;
    const double q[3] = {e[2], e[0], e[1]};
    for (int a = 0; a < 3; a++) p[a] = (float)((q[a] - off[a]) / scale);
  };
  auto nor = [&](uint64_t i, float n[3]) {
    if (!nrm) {
      n[0] = n[1] = n[2] = 0.0f;
      return;
    }
    const float* e = nrm + 3 * i;
    n[0] = e[2];
    n[1] = e[0];
    n[2] = e[1];
  };
  FILE* f = fopen(path, ply ? "wb" : "w");
  if (!f) return fail(nullptr, PRV_E_IO, "cannot open %s for writing", path);
  bool ok = true;
  if (ply) {
    ok = fprintf(f,
                 "ply\nformat binary_little_endian 1.0\ncomment nerf_prv_amd marching cubes, dataset frame\n"
                 "element vertex %llu\nproperty float x\nproperty float y\nproperty float z\nproperty float nx\nproperty float ny\n"
                 "property float nz\nproperty uchar red\nproperty uchar green\nproperty uchar blue\nelement face %llu\n"
                 "property list uchar int vertex_indices\nend_header\n",
                 (unsigned long long)nv, (unsigned long long)nt) > 0;
    std::vector<unsigned char> buf;
    const size_t kBatch = 1 << 16;
    for (uint64_t i0 = 0; ok && i0 < nv; i0 += kBatch) {
      const uint64_t i1 = std::min<uint64_t>(nv, i0 + kBatch);
      buf.resize((size_t)(i1 - i0) * 27);
      unsigned char* b = buf.data();
      for (uint64_t i = i0; i < i1; i++, b += 27) {
        float rec[6];
        pos(i, rec);
        nor(i, rec + 3);
        memcpy(b, rec, 24); // little-endian host (x86-64 / aarch64)
        for (int k = 0; k < 3; k++) b[24 + k] = rgb ? rgb[3 * i + k] : 0;
      }
      ok = fwrite(buf.data(), 1, buf.size(), f) == buf.size();
    }
    for (uint64_t i0 = 0; ok && i0 < nt; i0 += kBatch) {
      const uint64_t i1 = std::min<uint64_t>(nt, i0 + kBatch);
      buf.resize((size_t)(i1 - i0) * 13);
      unsigned char* b = buf.data();
      for (uint64_t i = i0; i < i1; i++, b += 13) {
        b[0] = 3;
        const int32_t ids[3] = {(int32_t)tri[3 * i], (int32_t)tri[3 * i + 1], (int32_t)tri[3 * i + 2]};
        memcpy(b + 1, ids, 12);
      }
      ok = fwrite(buf.data(), 1, buf.size(), f) == buf.size();
    }
  } else {
    ok = fprintf(f, "# nerf_prv_amd marching cubes, dataset frame\n") > 0;
    for (uint64_t i = 0; ok && i < nv; i++) {
      float p[3];
      pos(i, p);
      const double r = rgb ? rgb[3 * i] / 255.0 : 0.0, g = rgb ? rgb[3 * i + 1] / 255.0 : 0.0, b = rgb ? rgb[3 * i + 2] / 255.0 : 0.0;
      ok = fprintf(f, "v %.9g %.9g %.9g %.9g %.9g %.9g\n", (double)p[0], (double)p[1], (double)p[2], r, g, b) > 0;
    }
    for (uint64_t i = 0; ok && i < nv; i++) {
      float n[3];
      nor(i, n);
      ok = fprintf(f, "vn %.9g %.9g %.9g\n", (double)n[0], (double)n[1], (double)n[2]) > 0;
    }
    for (uint64_t i = 0; ok && i < nt; i++) {
      const unsigned long long a = tri[3 * i] + 1ull, b = tri[3 * i + 1] + 1ull, d = tri[3 * i + 2] + 1ull;
      ok = fprintf(f, "f %llu//%llu %llu//%llu %llu//%llu\n", a, a, b, b, d, d) > 0;
    }
  }
  if (fclose(f) != 0) ok = false;
  if (!ok) return fail(nullptr, PRV_E_IO, "writing %s failed", path);
  return PRV_OK;
}

} // namespace

extern "C" {

int prv_mesh_default_opts(prv_mesh_opts* o) {
  if (!o) return PRV_E_INVALID;
  for (int a = 0; a < 3; a++) {
    o->res[a] = 256;
    o->aabb_lo[a] = 0.0f;
    o->aabb_hi[a] = 1.0f;
  }
  o->threshold = 2.5f;
  o->use_occupancy = 0;
  o->colors = 1;
  return PRV_OK;
}

static int density_grid(prv_ctx* c, int slot, const prv_mesh_opts* o, const MeshGrid& g, float* sigma) {
  // one wave per 64 consecutive points of a row; PRV_MESH_BRICK=1 (dev, scripts/meshbench.py): one wave per 4x4x4 brick --
  // measured slower on the 512^3 field (1.12 vs 0.70 ms at 256^3, 5.9 vs 5.1 ms at 512^3) and even on the 256^3 one
  const char* env = getenv("PRV_MESH_BRICK");
  const int brick = env ? atoi(env) != 0 : 0;
  HIPCHK(c, launch_mesh_density(c->models[slot].dev, g, o->use_occupancy != 0, brick, sigma, c->stream));
  return PRV_OK;
}

int prv_density_grid(prv_ctx* c, int slot, const prv_mesh_opts* o, float* sigma_dev) try {
  if (!c) return PRV_E_INVALID;
  int rc;
  MeshGrid g;
  if ((rc = check_model(c, slot)) != PRV_OK || (rc = mesh_grid(c, o, g)) != PRV_OK) return rc;
  if (!sigma_dev) return fail(c, PRV_E_INVALID, "sigma_dev is NULL");
  if ((rc = check_device_ptr(c, sigma_dev, "sigma_dev")) != PRV_OK) return rc;
  HIPCHK(c, hipSetDevice(c->device));
  if ((rc = density_grid(c, slot, o, g, sigma_dev)) != PRV_OK) return rc;
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return PRV_OK;
} catch (...) { return caught(c); }

int prv_marching_cubes(prv_ctx* c, int slot, const prv_mesh_opts* o, prv_mesh** out) try {
  if (!c) return PRV_E_INVALID;
  if (!out) return fail(c, PRV_E_INVALID, "out is NULL");
  *out = nullptr;
  int rc;
  MeshGrid g;
  if ((rc = check_model(c, slot)) != PRV_OK || (rc = mesh_grid(c, o, g)) != PRV_OK) return rc;
  HIPCHK(c, hipSetDevice(c->device));
  MeshWork w;
  if ((rc = mesh_events(c, w)) != PRV_OK || (rc = ensure(c, w.sigma, mesh_points(g) * 4)) != PRV_OK) return rc;
  HIPCHK(c, hipEventRecord(w.ev[0], c->stream));
  if ((rc = density_grid(c, slot, o, g, (float*)w.sigma.p)) != PRV_OK) return rc;
  HIPCHK(c, hipEventRecord(w.ev[1], c->stream));
  return mesh_extract(c, (const float*)w.sigma.p, nullptr, g, o->threshold, o->colors ? &c->models[slot].dev : nullptr, w, out);
} catch (...) { return caught(c); }

static int marching_cubes_grid(prv_ctx* c, const float* sigma_dev, const uint8_t* valid_dev, const prv_mesh_opts* o, prv_mesh** out) {
  if (!c) return PRV_E_INVALID;
  if (!out) return fail(c, PRV_E_INVALID, "out is NULL");
  *out = nullptr;
  int rc;
  MeshGrid g;
  if ((rc = mesh_grid(c, o, g)) != PRV_OK) return rc;
  if (!sigma_dev) return fail(c, PRV_E_INVALID, "sigma_dev is NULL");
  if ((rc = check_device_ptr(c, sigma_dev, "sigma_dev")) != PRV_OK || (rc = check_device_ptr(c, valid_dev, "valid_dev")) != PRV_OK) return rc;
  HIPCHK(c, hipSetDevice(c->device));
  MeshWork w;
  if ((rc = mesh_events(c, w)) != PRV_OK) return rc;
  HIPCHK(c, hipEventRecord(w.ev[0], c->stream));
  HIPCHK(c, hipEventRecord(w.ev[1], c->stream));
  return mesh_extract(c, sigma_dev, valid_dev, g, o->threshold, nullptr, w, out);
}

int prv_marching_cubes_grid(prv_ctx* c, const float* sigma_dev, const prv_mesh_opts* o, prv_mesh** out) try {
  return marching_cubes_grid(c, sigma_dev, nullptr, o, out);
} catch (...) { return caught(c); }

int prv_marching_cubes_grid_valid(prv_ctx* c, const float* grid_dev, const uint8_t* valid_dev, const prv_mesh_opts* o, prv_mesh** out) try {
  return marching_cubes_grid(c, grid_dev, valid_dev, o, out);
} catch (...) { return caught(c); }

int prv_debug_mesh_stages(prv_ctx* c, float ms[4]) {
  if (!c || !ms) return PRV_E_INVALID;
  memcpy(ms, c->mesh_ms, sizeof(c->mesh_ms));
  return PRV_OK;
}

int prv_mesh_counts(const prv_mesh* m, uint64_t* nv, uint64_t* nt) {
  const int rc = mesh_alive(m);
  if (rc != PRV_OK) return rc;
  if (nv) *nv = m->nv;
  if (nt) *nt = m->nt;
  return PRV_OK;
}

int prv_mesh_get(const prv_mesh* m, float* xyz, float* normals, uint8_t* rgb, uint32_t* tri) try {
  int rc = mesh_alive(m);
  if (rc != PRV_OK) return rc;
  prv_ctx* c = m->ctx;
  HIPCHK(c, hipSetDevice(c->device));
  if (xyz && m->nv) HIPCHK(c, hipMemcpyAsync(xyz, m->xyz.p, m->nv * 12, hipMemcpyDeviceToHost, c->stream));
  if (normals && m->nv) HIPCHK(c, hipMemcpyAsync(normals, m->nrm.p, m->nv * 12, hipMemcpyDeviceToHost, c->stream));
  if (rgb && m->nv) {
    if (m->colors) HIPCHK(c, hipMemcpyAsync(rgb, m->rgb.p, m->nv * 3, hipMemcpyDeviceToHost, c->stream));
    else memset(rgb, 0, m->nv * 3);
  }
  if (tri && m->nt) HIPCHK(c, hipMemcpyAsync(tri, m->tri.p, m->nt * 12, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return PRV_OK;
} catch (...) { return caught(m && m->ctx ? m->ctx : nullptr); }

int prv_mesh_save(const prv_mesh* m, const char* path, double scale, const double offset[3]) try {
  int rc = mesh_alive(m);
  if (rc != PRV_OK) return rc;
  std::vector<float> xyz(m->nv * 3), nrm(m->nv * 3);
  std::vector<uint8_t> rgb(m->nv * 3);
  std::vector<uint32_t> tri(m->nt * 3);
  if ((rc = prv_mesh_get(m, xyz.data(), nrm.data(), rgb.data(), tri.data())) != PRV_OK) return rc;
  rc = write_mesh_file(path, m->nv, xyz.data(), nrm.data(), rgb.data(), m->nt, tri.data(), scale, offset);
  if (rc != PRV_OK) m->ctx->err = g_create_error; // the writer reports through prv_last_error(NULL); the context's too
  return rc;
} catch (...) { return caught(m && m->ctx ? m->ctx : nullptr); }

int prv_mesh_write_file(const char* path, uint64_t nv, const float* xyz, const float* normals, const uint8_t* rgb, uint64_t nt,
                        const uint32_t* tri, double scale, const double offset[3]) try {
  return write_mesh_file(path, nv, xyz, normals, rgb, nt, tri, scale, offset);
} catch (...) { return caught(nullptr); }

int prv_mesh_filter_default_opts(prv_mesh_filter_opts* o) {
  if (!o) return fail(nullptr, PRV_E_INVALID, "filter options are NULL");
  o->min_triangles = 0;
  o->keep_largest = 0;
  o->min_diagonal = 0.0f;
  return PRV_OK;
}

int prv_mesh_components(prv_mesh* m, uint64_t* n_components) try {
  int rc = mesh_alive(m);
  if (rc != PRV_OK) return rc;
  if (!n_components) return fail(m->ctx, PRV_E_INVALID, "n_components is NULL");
  if ((rc = mesh_label(m)) != PRV_OK) return rc;
  *n_components = m->comps.size();
  return PRV_OK;
} catch (...) { return caught(m && m->ctx ? m->ctx : nullptr); }

int prv_mesh_component_info(prv_mesh* m, uint64_t capacity, prv_mesh_component* out_host) try {
  int rc = mesh_alive(m);
  if (rc != PRV_OK) return rc;
  if (!out_host) return fail(m->ctx, PRV_E_INVALID, "out_host is NULL");
  if ((rc = mesh_label(m)) != PRV_OK) return rc;
  if (capacity < m->comps.size())
    return fail(m->ctx, PRV_E_INVALID, "capacity %llu is below the mesh's %llu components", (unsigned long long)capacity,
                (unsigned long long)m->comps.size());
  if (!m->comps.empty()) memcpy(out_host, m->comps.data(), m->comps.size() * sizeof(prv_mesh_component));
  return PRV_OK;
} catch (...) { return caught(m && m->ctx ? m->ctx : nullptr); }

int prv_mesh_labels(prv_mesh* m, uint32_t* vertex_component, uint32_t* triangle_component) try {
  int rc = mesh_alive(m);
  if (rc != PRV_OK) return rc;
  if ((rc = mesh_label(m)) != PRV_OK) return rc;
  prv_ctx* c = m->ctx;
  HIPCHK(c, hipSetDevice(c->device));
  if (vertex_component && m->nv) HIPCHK(c, hipMemcpyAsync(vertex_component, m->vcomp.p, m->nv * 4, hipMemcpyDeviceToHost, c->stream));
  if (triangle_component && m->nt) HIPCHK(c, hipMemcpyAsync(triangle_component, m->tcomp.p, m->nt * 4, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return PRV_OK;
} catch (...) { return caught(m && m->ctx ? m->ctx : nullptr); }

int prv_mesh_filter(prv_mesh* m, const prv_mesh_filter_opts* o, prv_mesh** out) try {
  int rc = mesh_alive(m);
  if (rc != PRV_OK) return rc;
  prv_ctx* c = m->ctx;
  if (!out) return fail(c, PRV_E_INVALID, "out is NULL");
  *out = nullptr;
  if (!o) return fail(c, PRV_E_INVALID, "filter options are NULL");
  if (!(o->min_diagonal >= 0.0f) || !std::isfinite(o->min_diagonal))
    return fail(c, PRV_E_INVALID, "min_diagonal must be finite and >= 0, got %g", (double)o->min_diagonal);
  if ((rc = mesh_label(m)) != PRV_OK) return rc;
  HIPCHK(c, hipSetDevice(c->device));
  const std::vector<uint8_t> keep = comp_keep(m->comps, *o);
  uint64_t nv = 0, nt = 0;
  for (size_t i = 0; i < keep.size(); i++)
    if (keep[i]) {
      nv += m->comps[i].n_vertices;
      nt += m->comps[i].n_triangles;
    }
  std::unique_ptr<prv_mesh> f(new prv_mesh(c)); // an early return below frees what it holds by then
  f->nv = nv;
  f->nt = nt;
  f->colors = m->colors;
  if (nv > 0) {
    CompWork w;
    const size_t waves_v = mesh_comp_waves(m->nv), waves_t = mesh_comp_waves(m->nt);
    if ((rc = ensure(c, w.keep, keep.size())) != PRV_OK || (rc = ensure(c, w.wave_v, waves_v * 8)) != PRV_OK ||
        (rc = ensure(c, w.wave_t, std::max<size_t>(1, waves_t) * 8)) != PRV_OK ||
        (rc = ensure(c, w.scratch, mesh_scan_scratch(std::max(waves_v, waves_t)) * 8)) != PRV_OK || (rc = ensure(c, w.misc, 16)) != PRV_OK ||
        (rc = ensure(c, w.vmap, m->nv * 4)) != PRV_OK)
      return rc;
    const uint8_t* keep_dev = (const uint8_t*)w.keep.p;
    uint64_t* tot = (uint64_t*)w.misc.p;
    HIPCHK(c, hipMemcpyAsync(w.keep.p, keep.data(), keep.size(), hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemsetAsync(tot, 0, 16, c->stream));
    HIPCHK(c, launch_mesh_comp_keep_count((const uint32_t*)m->vcomp.p, m->nv, keep_dev, (uint64_t*)w.wave_v.p, c->stream));
    HIPCHK(c, launch_mesh_scan((uint64_t*)w.wave_v.p, waves_v, (uint64_t*)w.scratch.p, tot, c->stream));
    if (m->nt > 0) {
      HIPCHK(c, launch_mesh_comp_keep_count((const uint32_t*)m->tcomp.p, m->nt, keep_dev, (uint64_t*)w.wave_t.p, c->stream));
      HIPCHK(c, launch_mesh_scan((uint64_t*)w.wave_t.p, waves_t, (uint64_t*)w.scratch.p, tot + 1, c->stream));
    }
    uint64_t totals[2] = {0, 0};
    HIPCHK(c, hipMemcpyAsync(totals, tot, 16, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (totals[0] != nv || totals[1] != nt) // the gather's extents come from the table: they must be the scans' too
      return fail(c, PRV_E_INTERNAL, "filter counts disagree: table %llu / %llu, scan %llu / %llu", (unsigned long long)nv, (unsigned long long)nt,
                  (unsigned long long)totals[0], (unsigned long long)totals[1]);
    if ((rc = ensure(c, f->xyz, nv * 12)) != PRV_OK || (rc = ensure(c, f->nrm, nv * 12)) != PRV_OK ||
        (f->colors && (rc = ensure(c, f->rgb, nv * 3)) != PRV_OK) || (rc = ensure(c, f->tri, std::max<uint64_t>(1, nt) * 12)) != PRV_OK)
      return rc;
    hipError_t e = launch_mesh_comp_gather_vertices((const uint32_t*)m->vcomp.p, m->nv, keep_dev, (const uint64_t*)w.wave_v.p, (const float*)m->xyz.p,
                                                    (const float*)m->nrm.p, f->colors ? (const uint8_t*)m->rgb.p : nullptr, (float*)f->xyz.p,
                                                    (float*)f->nrm.p, (uint8_t*)f->rgb.p, (uint32_t*)w.vmap.p, c->stream);
    if (e == hipSuccess && nt > 0)
      e = launch_mesh_comp_gather_triangles((const uint32_t*)m->tcomp.p, m->nt, keep_dev, (const uint64_t*)w.wave_t.p, (const uint32_t*)m->tri.p,
                                            (const uint32_t*)w.vmap.p, (uint32_t*)f->tri.p, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (e != hipSuccess) return fail(c, PRV_E_HIP, "mesh filter failed: %s", hipGetErrorString(e));
  }
  *out = f.release();
  return PRV_OK;
} catch (...) { return caught(m && m->ctx ? m->ctx : nullptr); }

int prv_debug_mesh_component_rounds(const prv_mesh* m, int* rounds) {
  const int rc = mesh_alive(m);
  if (rc != PRV_OK) return rc;
  if (!rounds) return fail(m->ctx, PRV_E_INVALID, "rounds is NULL");
  if (!m->labelled) return fail(m->ctx, PRV_E_STATE, "the mesh has not been labelled yet (prv_mesh_components)");
  *rounds = m->label_rounds;
  return PRV_OK;
}

void prv_mesh_destroy(prv_mesh* m) { destroy_handle(m); }

} // extern "C"
