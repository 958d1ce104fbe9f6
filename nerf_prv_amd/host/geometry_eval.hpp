// geometry_eval.hpp -- the planner's geometric evaluation (`evaluate_geometry: 1`): its yaml keys, the frame change of a
// reference cloud and the `metrics/<it>_geometry.txt` writer.  Host only (no GPU call here); prv_planner-private: nothing
// of this is exported from libprv_host.so.
#pragma once
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <string>
#include <vector>

#include "../../include/prv.h"
#include "Share_Data.hpp"

namespace prvhost {

struct GeometryEvalConfig {
  bool on = false;              // evaluate_geometry: 1 (absent = off: every existing config and output tree is what it was)
  int mc_res = 256;             // geometry_mc_res: marching-cubes grid points per axis, reconstruction and reference alike
  uint64_t samples = 1u << 20;  // geometry_samples: surface samples per side
  double tau = -1.0;            // geometry_tau, dataset units; < 0 = 1 % of the object size
  std::string reference;        // geometry_reference: a .pcd cloud (dataset frame); empty = the ground-truth field's mesh (slot 6)
  double tau_for(double object_size) const { return tau >= 0.0 ? tau : 0.01 * object_size; }
};

inline GeometryEvalConfig geometry_eval_config(const FileStorage& fs) {
  GeometryEvalConfig g;
  g.on = fs.has("evaluate_geometry") && fs.num("evaluate_geometry") > 0;
  if (fs.has("geometry_mc_res")) g.mc_res = (int)fs.num("geometry_mc_res");
  if (fs.has("geometry_samples")) g.samples = (uint64_t)fs.num("geometry_samples");
  if (fs.has("geometry_tau")) g.tau = fs.num("geometry_tau");
  if (fs.has("geometry_reference")) g.reference = fs.str("geometry_reference");
  return g;
}

// "" if the configuration can run, else what is wrong with it (checked before any training)
inline std::string geometry_eval_problem(const GeometryEvalConfig& g) {
  if (!g.on) return "";
  if (g.mc_res < 2 || g.mc_res > 1024) return "geometry_mc_res must be in [2, 1024]";
  if (g.samples < 1 || g.samples > (1ull << 31)) return "geometry_samples must be in [1, 2^31]";
  if (g.tau >= 0.0 && !std::isfinite(g.tau)) return "geometry_tau must be finite";
  if (!g.reference.empty()) {
    const size_t n = g.reference.size();
    if (n < 4 || g.reference.substr(n - 4) != ".pcd") return "geometry_reference must name a .pcd file";
  }
  return "";
}

// dataset-frame points -> the engine frame, exactly as prv_splat_points places a cloud: q = fmaf(p, scale, offset) in
// fp32, e = (q1, q2, q0)
inline void geometry_to_engine(std::vector<float>& xyz, double scale, const double offset[3]) {
  const float s = (float)scale, o[3] = {(float)offset[0], (float)offset[1], (float)offset[2]};
  for (size_t i = 0; i + 2 < xyz.size(); i += 3) {
    const float q[3] = {std::fmaf(xyz[i], s, o[0]), std::fmaf(xyz[i + 1], s, o[1]), std::fmaf(xyz[i + 2], s, o[2])};
    xyz[i] = q[1];
    xyz[i + 1] = q[2];
    xyz[i + 2] = q[0];
  }
}

// one `name<TAB>value` line per field of prv_geom_metrics in struct order, in the style of the PSNR / SSIM file; the
// engine-frame distances divided by `scale` (squared ones by scale^2): dataset units
inline std::string geometry_metrics_text(const prv_geom_metrics& m, double scale) {
  char buf[1024];
  const double s = scale, s2 = scale * scale;
  snprintf(buf, sizeof(buf),
           "n_rec\t%llu\nn_ref\t%llu\naccuracy\t%.17g\ncompleteness\t%.17g\naccuracy_sq\t%.17g\ncompleteness_sq\t%.17g\nchamfer\t%.17g\n"
           "precision\t%.17g\nrecall\t%.17g\nfscore\t%.17g\nhausdorff_rec\t%.17g\nhausdorff_ref\t%.17g\n",
           (unsigned long long)m.n_rec, (unsigned long long)m.n_ref, m.accuracy / s, m.completeness / s, m.accuracy_sq / s2,
           m.completeness_sq / s2, m.chamfer / s, m.precision, m.recall, m.fscore, m.hausdorff_rec / s, m.hausdorff_ref / s);
  return buf;
}

} // namespace prvhost
