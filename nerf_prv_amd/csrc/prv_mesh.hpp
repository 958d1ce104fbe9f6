// prv_mesh.hpp -- mesh extraction (prv_mesh.hip): the density grid of a field and marching cubes on a sigma grid.
#pragma once
#include "prv_device.hpp"

namespace prv {

// A grid of res[0] x res[1] x res[2] points, x fastest; point i on axis a sits at lo[a] + (float)i * step[a]
// (one multiply, one add: -ffp-contract=off), step[a] = (hi[a] - lo[a]) / (float)(res[a] - 1), computed by the host.
struct MeshGrid {
  int res[3];
  float lo[3], step[3];
};

inline size_t mesh_points(const MeshGrid& g) { return (size_t)g.res[0] * g.res[1] * g.res[2]; }
// waves of 64 points the per-point passes run: whole blocks of 4 (the per-point buffers hold mesh_waves * 64 bytes)
inline size_t mesh_waves(const MeshGrid& g) { return (mesh_points(g) + 255) / 256 * 4; }
// uint64 elements of scratch the scan of n elements needs (launch_mesh_scan)
size_t mesh_scan_scratch(size_t n);

// sigma[point] = fast_exp(density MLP output 0 + bias) of the field at every grid point; use_occ: 0 where the point's
// occupancy bit is clear.  brick: one wave = a 4x4x4 brick of points, else 64 consecutive points of a row (the default:
// measured faster, scripts/meshbench.py).
hipError_t launch_mesh_density(const FieldDev& fd, const MeshGrid& g, int use_occ, int brick, float* sigma, hipStream_t s);
// per point: crossing flags of its +x/+y/+z edge (bits 0..2) and the case of the cell it is the low corner of; per wave of
// 64 points: vertices (crossing edges) and triangles.  flags / cases: mesh_waves * 64 bytes (the tail is written as 0).
// kept (launch_mesh_kept's bytes, or nullptr: no mask): a cell that is not kept has case 0, and a crossing edge is flagged only
// if a cell around it is kept -- the emit passes then need no mask of their own.
hipError_t launch_mesh_classify(const float* sigma, const MeshGrid& g, float thr, const uint8_t* kept, uint8_t* flags, uint8_t* cases,
                                uint64_t* wave_v, uint64_t* wave_t, hipStream_t s);
// kept[point] = 1 iff the point is the low corner of a cell whose eight corners all have valid != 0; mesh_waves * 64 bytes
hipError_t launch_mesh_kept(const uint8_t* valid, const MeshGrid& g, uint8_t* kept, hipStream_t s);
// exclusive scan of n uint64 in place; the grand total to *total (device); scratch: mesh_scan_scratch(n) elements
hipError_t launch_mesh_scan(uint64_t* a, size_t n, uint64_t* scratch, uint64_t* total, hipStream_t s);
// vertices in edge-id order (3 * point + axis): position and normal (-grad sigma)
hipError_t launch_mesh_vertices(const float* sigma, const MeshGrid& g, float thr, const uint8_t* flags, const uint64_t* wave_v,
                                float* xyz, float* nrm, hipStream_t s);
// triangles in cell order, each cell's in table order, as vertex ids
hipError_t launch_mesh_triangles(const MeshGrid& g, const uint8_t* flags, const uint8_t* cases, const uint64_t* wave_v,
                                 const uint64_t* wave_t, uint32_t* tri, hipStream_t s);
// the full field at each vertex seen from outside (dir = -normal), quantised as an opaque pixel
hipError_t launch_mesh_colors(const FieldDev& fd, const float* xyz, const float* nrm, uint64_t nv, uint8_t* rgb, hipStream_t s);

// ---- connected components and the filter (prv_components.hip)
// hook + compress rounds the labelling may take; beyond it the call fails, it never loops on
constexpr int kMeshComponentMaxRounds = 64;
// prv_mesh_component's layout on the device, the box as order-preserving unsigned images of its floats
// (key = bits ^ (sign ? 0xFFFFFFFF : 0x80000000): the host undoes it)
struct MeshComponentDev {
  uint32_t first_vertex, reserved;
  unsigned long long n_vertices, n_triangles;
  uint32_t lo[3], hi[3];
};
static_assert(sizeof(MeshComponentDev) == 48, "one table entry is 48 bytes on both sides");
inline size_t mesh_comp_waves(uint64_t n) { return (size_t)((n + 63) / 64); }

// parent[v] = v
hipError_t launch_mesh_comp_init(uint32_t* parent, uint64_t nv, hipStream_t s);
// one lane per triangle joins the roots of its vertices (the larger root under the smaller); *changed |= 1 if any triangle's
// vertices were not under one root yet.  The caller zeroes *changed before the launch.
hipError_t launch_mesh_comp_hook(const uint32_t* tri, uint64_t nt, uint32_t* parent, uint32_t* changed, hipStream_t s);
// one lane per vertex: parent[v] = its root
hipError_t launch_mesh_comp_compress(uint32_t* parent, uint64_t nv, hipStream_t s);
// roots (parent[v] == v) per wave of 64 vertices: wave_n holds mesh_comp_waves(nv) counts, to be scanned (launch_mesh_scan)
hipError_t launch_mesh_comp_roots(const uint32_t* parent, uint64_t nv, uint64_t* wave_n, hipStream_t s);
// parent fully compressed, wave_n scanned: component ids in root order to vcomp (nv) and tcomp (nt), and the table (one
// entry per root)
hipError_t launch_mesh_comp_table(const uint32_t* parent, const uint64_t* wave_n, const float* xyz, uint64_t nv, const uint32_t* tri, uint64_t nt,
                                  uint32_t* vcomp, uint32_t* tcomp, MeshComponentDev* table, hipStream_t s);
// elements (vertices or triangles, by their component id) of kept components per wave of 64: mesh_comp_waves(n) counts
hipError_t launch_mesh_comp_keep_count(const uint32_t* comp, uint64_t n, const uint8_t* keep, uint64_t* wave_n, hipStream_t s);
// wave_n scanned: the kept vertices in their order (rgb may be NULL), and vmap[v] = the new id of every kept vertex
hipError_t launch_mesh_comp_gather_vertices(const uint32_t* vcomp, uint64_t nv, const uint8_t* keep, const uint64_t* wave_n, const float* xyz,
                                            const float* nrm, const uint8_t* rgb, float* out_xyz, float* out_nrm, uint8_t* out_rgb,
                                            uint32_t* vmap, hipStream_t s);
// wave_n scanned: the kept triangles in their order, with the new vertex ids
hipError_t launch_mesh_comp_gather_triangles(const uint32_t* tcomp, uint64_t nt, const uint8_t* keep, const uint64_t* wave_n, const uint32_t* tri,
                                             const uint32_t* vmap, uint32_t* out_tri, hipStream_t s);

} // namespace prv
