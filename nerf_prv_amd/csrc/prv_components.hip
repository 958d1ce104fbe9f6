// prv_components.hip -- connected components of a mesh and floater removal: labelling, the per-component table, the filter.
//
// Two vertices are connected if a triangle uses both; a vertex's label is the smallest vertex id of its connected set.
//   label      a union-find over parent[] (nv 32-bit ids) with the invariant parent[v] <= v: a parent is only ever lowered
//              (a compare-and-swap of a root towards the smaller root, atomicMin everywhere else), so every root walk is a
//              strictly decreasing chain and ends on its own.  hook: one lane per triangle joins the roots of its vertices;
//              compress: one lane per vertex points itself at its root.  The host repeats the two until a hook pass finds
//              every triangle's vertices under one root already (a device flag, one 4-byte read-back per round).
//              NO WAITING: no lane waits for another's write.  A failed compare-and-swap means someone else hooked that root
//              (some lane always makes progress); what other workgroups write during a launch is read with agent-scope
//              atomic loads, and a stale value is still an ancestor of the vertex: it can cost a step or a round, never the
//              answer, because a pass only reports "no change" for triangles whose walks met in one vertex.
//   rank       roots (parent[v] == v) in vertex-id order: per-wave counts by __ballot / __popcll, the mesh scan, the rank
//   table      first vertex, vertex and triangle counts (integer atomic adds), bounding box (atomicMin / atomicMax on the
//              order-preserving unsigned image of the float): every sum and extremum is order-independent, the table is
//              bit-reproducible.  A wave whose vertices (triangles) share one component reduces in registers first.
//   filter     one keep byte per component; per-wave counts of kept vertices / triangles, the scan, a gather that keeps
//              vertex and triangle order and remaps the ids: boolean-mask compaction.
// Extra memory: labelling 4 bytes per vertex of scratch (parent) + 4 per vertex and 4 per triangle kept on the handle (the
// labels) + 48 per component; the filter 4 bytes per vertex (the id map) + 8 per wave of vertices and of triangles.
#include "prv_mesh.hpp"

namespace prv {

namespace {

__device__ __forceinline__ uint64_t lanes_below() { return (1ull << (threadIdx.x & 63)) - 1ull; }

__device__ __forceinline__ uint32_t load_agent(const uint32_t* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// order-preserving unsigned image of a float: a < b (as floats, -0 below +0) <=> key(a) < key(b)
__device__ __forceinline__ uint32_t float_key(float x) {
  const uint32_t b = __float_as_uint(x);
  return b ^ ((b >> 31) ? 0xFFFFFFFFu : 0x80000000u);
}

// ------------------------------------------------------------------ labelling
// the root of v's tree; on the way every visited vertex is pointed at its grandparent (an ancestor: the sets stay, the
// invariant stays, the chains halve)
__device__ __forceinline__ uint32_t comp_find(uint32_t* parent, uint32_t v) {
  uint32_t p = load_agent(parent + v);
  while (p != v) { // p < v
    const uint32_t g = load_agent(parent + p);
    if (g != p) atomicMin(parent + v, g);
    v = p;
    p = g;
  }
  return v;
}

// joins the sets of a and b; true if their walks did not end in one vertex (the pass changed something, or may have)
__device__ __forceinline__ bool comp_union(uint32_t* parent, uint32_t a, uint32_t b) {
  uint32_t ra = comp_find(parent, a), rb = comp_find(parent, b);
  const bool differ = ra != rb;
  while (ra != rb) {
    if (ra < rb) {
      const uint32_t t = ra;
      ra = rb;
      rb = t;
    }
    const uint32_t old = atomicCAS(parent + ra, ra, rb); // only a root is hooked, and only below itself
    if (old == ra) break;
    ra = comp_find(parent, old); // somebody hooked ra first (their progress): go on from where it points now
  }
  return differ;
}

__global__ __launch_bounds__(256) void comp_init_kernel(uint32_t* __restrict__ parent, uint64_t nv) {
  const uint64_t v = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (v < nv) parent[v] = (uint32_t)v;
}

__global__ __launch_bounds__(256) void comp_hook_kernel(const uint32_t* __restrict__ tri, uint64_t nt, uint32_t* parent, uint32_t* changed) {
  const uint64_t t = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  bool ch = false;
  if (t < nt) {
    const uint32_t a = tri[3 * t], b = tri[3 * t + 1], c = tri[3 * t + 2];
    ch = comp_union(parent, a, b);
    ch = comp_union(parent, b, c) || ch;
  }
  if (__ballot(ch) != 0ull && (threadIdx.x & 63) == 0) atomicOr(changed, 1u);
}

__global__ __launch_bounds__(256) void comp_compress_kernel(uint32_t* parent, uint64_t nv) {
  const uint64_t v = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (v >= nv) return;
  const uint32_t r = comp_find(parent, (uint32_t)v); // roots do not move in this launch: r is the root
  atomicMin(parent + v, r);
}

// ------------------------------------------------------------------ component ids
__global__ __launch_bounds__(256) void comp_roots_kernel(const uint32_t* __restrict__ parent, uint64_t nv, uint64_t* __restrict__ wave_n) {
  const uint64_t v = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  const uint64_t roots = __ballot(v < nv && parent[v] == (uint32_t)v);
  if ((threadIdx.x & 63) == 0 && v < nv) wave_n[v >> 6] = (uint64_t)__popcll(roots);
}

// a root's component id = its rank among the roots; its table entry starts empty
__global__ __launch_bounds__(256) void comp_rank_kernel(const uint32_t* __restrict__ parent, uint64_t nv, const uint64_t* __restrict__ wave_n,
                                                        uint32_t* __restrict__ vcomp, MeshComponentDev* __restrict__ table) {
  const uint64_t v = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  const bool root = v < nv && parent[v] == (uint32_t)v;
  const uint64_t roots = __ballot(root);
  if (!root) return;
  const uint32_t c = (uint32_t)(wave_n[v >> 6] + (uint64_t)__popcll(roots & lanes_below()));
  vcomp[v] = c;
  MeshComponentDev e;
  e.first_vertex = (uint32_t)v;
  e.reserved = 0;
  e.n_vertices = 0;
  e.n_triangles = 0;
  for (int a = 0; a < 3; a++) {
    e.lo[a] = 0xFFFFFFFFu;
    e.hi[a] = 0u;
  }
  table[c] = e;
}

// every vertex takes its root's id and enters the table.  vcomp is read at roots (written by the launch before) and written
// at the others: no lane reads what this launch writes.
__global__ __launch_bounds__(256) void comp_label_kernel(const uint32_t* __restrict__ parent, const float* __restrict__ xyz, uint64_t nv,
                                                         uint32_t* vcomp, MeshComponentDev* table) {
  const uint64_t v = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  const bool ok = v < nv;
  uint32_t c = 0, lo[3] = {0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu}, hi[3] = {0u, 0u, 0u};
  if (ok) {
    const uint32_t p = parent[v];
    c = vcomp[p];
    if (p != (uint32_t)v) vcomp[v] = c;
#pragma unroll
    for (int a = 0; a < 3; a++) lo[a] = hi[a] = float_key(xyz[3 * v + a]);
  }
  const uint64_t live = __ballot(ok);
  if (__all(!ok || c == __shfl(c, 0))) { // one component in the wave (lane 0 is live if any lane is): one lane enters it
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1)
#pragma unroll
      for (int a = 0; a < 3; a++) {
        lo[a] = min(lo[a], (uint32_t)__shfl_xor((int)lo[a], d));
        hi[a] = max(hi[a], (uint32_t)__shfl_xor((int)hi[a], d));
      }
    if ((threadIdx.x & 63) != 0 || !ok) return;
    atomicAdd(&table[c].n_vertices, (unsigned long long)__popcll(live));
  } else {
    if (!ok) return;
    atomicAdd(&table[c].n_vertices, 1ull);
  }
#pragma unroll
  for (int a = 0; a < 3; a++) {
    atomicMin(&table[c].lo[a], lo[a]);
    atomicMax(&table[c].hi[a], hi[a]);
  }
}

// a triangle belongs to the component of its first vertex
__global__ __launch_bounds__(256) void comp_triangles_kernel(const uint32_t* __restrict__ tri, uint64_t nt, const uint32_t* __restrict__ vcomp,
                                                             uint32_t* __restrict__ tcomp, MeshComponentDev* table) {
  const uint64_t t = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  const bool ok = t < nt;
  uint32_t c = 0;
  if (ok) {
    c = vcomp[tri[3 * t]];
    tcomp[t] = c;
  }
  const uint64_t live = __ballot(ok);
  if (__all(!ok || c == __shfl(c, 0))) {
    if ((threadIdx.x & 63) == 0 && ok) atomicAdd(&table[c].n_triangles, (unsigned long long)__popcll(live));
  } else if (ok) {
    atomicAdd(&table[c].n_triangles, 1ull);
  }
}

// ------------------------------------------------------------------ filter
// per wave of 64 elements (vertices or triangles): how many are of a kept component
__global__ __launch_bounds__(256) void comp_keep_count_kernel(const uint32_t* __restrict__ comp, uint64_t n, const uint8_t* __restrict__ keep,
                                                              uint64_t* __restrict__ wave_n) {
  const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  const uint64_t kept = __ballot(i < n && keep[comp[i]] != 0);
  if ((threadIdx.x & 63) == 0 && i < n) wave_n[i >> 6] = (uint64_t)__popcll(kept);
}

__global__ __launch_bounds__(256) void comp_gather_vertices_kernel(const uint32_t* __restrict__ vcomp, uint64_t nv, const uint8_t* __restrict__ keep,
                                                                   const uint64_t* __restrict__ wave_n, const float* __restrict__ xyz,
                                                                   const float* __restrict__ nrm, const uint8_t* __restrict__ rgb,
                                                                   float* __restrict__ out_xyz, float* __restrict__ out_nrm,
                                                                   uint8_t* __restrict__ out_rgb, uint32_t* __restrict__ vmap) {
  const uint64_t v = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  const bool k = v < nv && keep[vcomp[v]] != 0;
  const uint64_t kept = __ballot(k);
  if (!k) return;
  const uint64_t o = wave_n[v >> 6] + (uint64_t)__popcll(kept & lanes_below());
  vmap[v] = (uint32_t)o;
#pragma unroll
  for (int a = 0; a < 3; a++) {
    out_xyz[3 * o + a] = xyz[3 * v + a];
    out_nrm[3 * o + a] = nrm[3 * v + a];
  }
  if (rgb) {
#pragma unroll
    for (int a = 0; a < 3; a++) out_rgb[3 * o + a] = rgb[3 * v + a];
  }
}

__global__ __launch_bounds__(256) void comp_gather_triangles_kernel(const uint32_t* __restrict__ tcomp, uint64_t nt, const uint8_t* __restrict__ keep,
                                                                    const uint64_t* __restrict__ wave_n, const uint32_t* __restrict__ tri,
                                                                    const uint32_t* __restrict__ vmap, uint32_t* __restrict__ out_tri) {
  const uint64_t t = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  const bool k = t < nt && keep[tcomp[t]] != 0;
  const uint64_t kept = __ballot(k);
  if (!k) return;
  const uint64_t o = wave_n[t >> 6] + (uint64_t)__popcll(kept & lanes_below());
#pragma unroll
  for (int j = 0; j < 3; j++) out_tri[3 * o + j] = vmap[tri[3 * t + j]]; // its vertices are of its component: kept, mapped
}

inline unsigned blocks_of(uint64_t n) { return (unsigned)((n + 255) / 256); }

} // namespace

hipError_t launch_mesh_comp_init(uint32_t* parent, uint64_t nv, hipStream_t s) {
  if (nv == 0) return hipSuccess;
  hipLaunchKernelGGL(comp_init_kernel, dim3(blocks_of(nv)), dim3(256), 0, s, parent, nv);
  return hipGetLastError();
}

hipError_t launch_mesh_comp_hook(const uint32_t* tri, uint64_t nt, uint32_t* parent, uint32_t* changed, hipStream_t s) {
  if (nt == 0) return hipSuccess;
  hipLaunchKernelGGL(comp_hook_kernel, dim3(blocks_of(nt)), dim3(256), 0, s, tri, nt, parent, changed);
  return hipGetLastError();
}

hipError_t launch_mesh_comp_compress(uint32_t* parent, uint64_t nv, hipStream_t s) {
  if (nv == 0) return hipSuccess;
  hipLaunchKernelGGL(comp_compress_kernel, dim3(blocks_of(nv)), dim3(256), 0, s, parent, nv);
  return hipGetLastError();
}

hipError_t launch_mesh_comp_roots(const uint32_t* parent, uint64_t nv, uint64_t* wave_n, hipStream_t s) {
  if (nv == 0) return hipSuccess;
  hipLaunchKernelGGL(comp_roots_kernel, dim3(blocks_of(nv)), dim3(256), 0, s, parent, nv, wave_n);
  return hipGetLastError();
}

hipError_t launch_mesh_comp_table(const uint32_t* parent, const uint64_t* wave_n, const float* xyz, uint64_t nv, const uint32_t* tri, uint64_t nt,
                                  uint32_t* vcomp, uint32_t* tcomp, MeshComponentDev* table, hipStream_t s) {
  if (nv == 0) return hipSuccess;
  hipLaunchKernelGGL(comp_rank_kernel, dim3(blocks_of(nv)), dim3(256), 0, s, parent, nv, wave_n, vcomp, table);
  hipLaunchKernelGGL(comp_label_kernel, dim3(blocks_of(nv)), dim3(256), 0, s, parent, xyz, nv, vcomp, table);
  if (nt > 0) hipLaunchKernelGGL(comp_triangles_kernel, dim3(blocks_of(nt)), dim3(256), 0, s, tri, nt, (const uint32_t*)vcomp, tcomp, table);
  return hipGetLastError();
}

hipError_t launch_mesh_comp_keep_count(const uint32_t* comp, uint64_t n, const uint8_t* keep, uint64_t* wave_n, hipStream_t s) {
  if (n == 0) return hipSuccess;
  hipLaunchKernelGGL(comp_keep_count_kernel, dim3(blocks_of(n)), dim3(256), 0, s, comp, n, keep, wave_n);
  return hipGetLastError();
}

hipError_t launch_mesh_comp_gather_vertices(const uint32_t* vcomp, uint64_t nv, const uint8_t* keep, const uint64_t* wave_n, const float* xyz,
                                            const float* nrm, const uint8_t* rgb, float* out_xyz, float* out_nrm, uint8_t* out_rgb,
                                            uint32_t* vmap, hipStream_t s) {
  if (nv == 0) return hipSuccess;
  hipLaunchKernelGGL(comp_gather_vertices_kernel, dim3(blocks_of(nv)), dim3(256), 0, s, vcomp, nv, keep, wave_n, xyz, nrm, rgb, out_xyz,
                     out_nrm, out_rgb, vmap);
  return hipGetLastError();
}

hipError_t launch_mesh_comp_gather_triangles(const uint32_t* tcomp, uint64_t nt, const uint8_t* keep, const uint64_t* wave_n, const uint32_t* tri,
                                             const uint32_t* vmap, uint32_t* out_tri, hipStream_t s) {
  if (nt == 0) return hipSuccess;
  hipLaunchKernelGGL(comp_gather_triangles_kernel, dim3(blocks_of(nt)), dim3(256), 0, s, tcomp, nt, keep, wave_n, tri, vmap, out_tri);
  return hipGetLastError();
}

} // namespace prv
