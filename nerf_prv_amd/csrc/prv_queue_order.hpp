// prv_queue_order.hpp -- the order in which the render launch drains a queue region: cell keys, descriptors and their sort.
// Host and device (no HIP header needed): tests/test_queue_order_host.py builds a stand-alone program from this file alone.
//
// A march wave appends its <= 64 live records to one region of the queue as ONE contiguous block (region_reserve) and, with
// PRV_REGION_CELLS = C > 1, says so in an 8-byte DESCRIPTOR {first queue slot, count | cell key << 8}.  The cell key is which of
// C x C x C cells of its octant the wave's mid-span point falls in, cells numbered in Morton order (consecutive keys are
// neighbours).  Between march and render one small launch (order_descriptors_kernel) sorts every octant's descriptors by
// (cell key, arrival), stable, and the render launch takes its records descriptor by descriptor from that list: all waves of an
// XCD walk through the cells of their octant together, and what their L2 holds is one cell's tube, not the octant's.
//
// Arrival: an octant's region is n_sub sub-regions with a counter each; descriptor i of sub-region s comes i-th in that
// sub-region's own order (the counter's), and the sub-regions are interleaved: (0, 0), (1, 0), ... (n_sub - 1, 0), (0, 1), ...
// -- a march launch walks the views in order and deals its blocks to the sub-regions round robin, so this is close to the
// order of the launch and the views stay in order inside a cell.
#pragma once
#include <cstddef>
#include <cstdint>
#if defined(__HIPCC__)
#define PRV_QO_HD __host__ __device__
#else
#define PRV_QO_HD
#include <vector>
#endif

namespace prv {

constexpr int kMaxRegionCells = 8;                                                        // cells per axis and octant: 1, 2, 4 or 8
constexpr int kMaxCellKeys = kMaxRegionCells * kMaxRegionCells * kMaxRegionCells;          // 512
constexpr uint32_t kDescKeyShift = 8;                                                     // descriptor word 1 = count (<= 64) | key << 8

struct QueueDesc {
  uint32_t first; // queue slot of the block's first record
  uint32_t info;  // count | cell key << kDescKeyShift (count 0: nothing)
};
PRV_QO_HD inline uint32_t desc_count(const QueueDesc& d) { return d.info & ((1u << kDescKeyShift) - 1u); }
PRV_QO_HD inline uint32_t desc_key(const QueueDesc& d) { return d.info >> kDescKeyShift; }
PRV_QO_HD inline QueueDesc make_desc(uint32_t first, uint32_t count, uint32_t key) { return QueueDesc{first, count | key << kDescKeyShift}; }

// PRV_REGION_CELLS as given -> 1, 2, 4 or 8 (anything else: the next smaller of them)
inline int region_cells_clamp(int c) { return c >= 8 ? 8 : c >= 4 ? 4 : c >= 2 ? 2 : 1; }

// bits 0..2 of x, y, z interleaved: x0 y0 z0 x1 y1 z1 x2 y2 z2 (x0 lowest)
PRV_QO_HD inline uint32_t morton3(uint32_t x, uint32_t y, uint32_t z) {
  uint32_t k = 0u;
  for (int b = 0; b < 3; b++) k |= (((x >> b) & 1u) << (3 * b)) | (((y >> b) & 1u) << (3 * b + 1)) | (((z >> b) & 1u) << (3 * b + 2));
  return k;
}

// the cell of point p inside ITS octant of the box [lo, hi] (the octant by ray_octant's comparison, p > the box's middle), cells
// per axis; always < cells^3, whatever p is (outside the box: the nearest cell; NaN: cell 0)
PRV_QO_HD inline uint32_t region_cell_key(const float p[3], const float lo[3], const float hi[3], int cells) {
  uint32_t c[3];
  for (int a = 0; a < 3; a++) {
    const float mid = 0.5f * (lo[a] + hi[a]);
    const float from = p[a] > mid ? mid : lo[a];
    float u = (p[a] - from) * ((float)cells / (mid - lo[a]));
    u = u > 0.f ? u : 0.f; // (false for NaN)
    const float top = (float)(cells - 1);
    c[a] = (uint32_t)(u < top ? u : top);
  }
  return morton3(c[0], c[1], c[2]);
}

// the descriptors of one sub-region that count: n_added were reserved an index (the counter's high word); when the region closed,
// the first reservation that failed left its own index + 1 in `closed_at`: every index from there on belongs to a failed reservation
PRV_QO_HD inline uint32_t desc_valid_count(uint32_t n_added, uint32_t closed_at) { return closed_at ? closed_at - 1u : n_added; }

#if !defined(__HIPCC__)
// ---- host models (the device code in prv_kernels.hip does the same in parallel; the tests hold the two to the same properties)

// region_reserve with descriptors, one region's counter words: [0] records added, [1] descriptor indices handed out, [2] tail cut,
// [3] closed_at.  A reservation of n records gets (slot, descriptor index) or fails (the region is closed / closes now).
struct RegionCounter {
  uint32_t w[4] = {0, 0, 0, 0};
  bool reserve(uint32_t seg_cap, uint32_t n, uint32_t* slot, uint32_t* idx) {
    const uint32_t old = w[0], i = w[1];
    w[0] += n;
    w[1] += 1u;
    if (old + n <= seg_cap) {
      *slot = old;
      *idx = i;
      return true;
    }
    if (old <= seg_cap) { // the first reservation that fails: it straddles the end, or the region is exactly full
      if (old < seg_cap) w[2] = seg_cap - old;
      w[3] = i + 1u;
    }
    return false;
  }
  uint32_t records(uint32_t seg_cap) const { return (w[0] < seg_cap ? w[0] : seg_cap) - w[2]; } // what the render launch drains
  uint32_t descriptors() const { return desc_valid_count(w[1], w[3]); }
};

// the sort of one octant region: sub[s] = the n[s] descriptors of sub-region s in index order -> all of them by (key, arrival)
inline std::vector<QueueDesc> order_descriptors(const QueueDesc* const* sub, const uint32_t* n, int n_sub, int n_keys) {
  std::vector<uint32_t> at((std::size_t)n_keys + 1, 0u);
  uint32_t n_max = 0u;
  for (int s = 0; s < n_sub; s++) {
    n_max = n[s] > n_max ? n[s] : n_max;
    for (uint32_t i = 0; i < n[s]; i++) at[desc_key(sub[s][i]) + 1u]++;
  }
  for (int k = 0; k < n_keys; k++) at[k + 1] += at[k];
  std::vector<QueueDesc> out(at[n_keys]);
  for (uint32_t i = 0; i < n_max; i++)
    for (int s = 0; s < n_sub; s++)
      if (i < n[s]) out[at[desc_key(sub[s][i])]++] = sub[s][i];
  return out;
}
#endif

} // namespace prv
