// coverage_eval.hpp -- the planner's surface coverage evaluation (`evaluate_coverage: 1`): its yaml keys and the
// `metrics/<it>_coverage.txt` writer.  Host only (no GPU call here); prv_planner-private: nothing of this is exported from
// libprv_host.so.  The reference surface is the geometric evaluation's (geometry_eval.hpp: geometry_reference, or the
// ground-truth field's mesh at geometry_mc_res / geometry_samples).
#pragma once
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <string>

#include "Share_Data.hpp"

namespace prvhost {

struct CoverageEvalConfig {
  bool on = false;         // evaluate_coverage: 1 (absent = off: every existing config and output tree is what it was)
  int point_size = 1;      // coverage_point_size: prv_coverage_opts.point_size
  double depth_tol = 0.02; // coverage_depth_tol: prv_coverage_opts.depth_tol (an option value, not a measured one)
  int width = 0, height = 0; // coverage_width / coverage_height; 0 = the candidates' size
  // coverage_occluder: points | mesh (absent = points: every file is byte for byte what it was).  mesh: the ground-truth field's
  // marching-cubes mesh, rasterised, occludes the reference points (prv_coverage_create_occluded); coverage_point_size is ignored
  std::string occluder = "points";
  bool mesh_occluder() const { return on && occluder == "mesh"; }
};

inline CoverageEvalConfig coverage_eval_config(const FileStorage& fs) {
  CoverageEvalConfig c;
  c.on = fs.has("evaluate_coverage") && fs.num("evaluate_coverage") > 0;
  if (fs.has("coverage_point_size")) c.point_size = (int)fs.num("coverage_point_size");
  if (fs.has("coverage_depth_tol")) c.depth_tol = fs.num("coverage_depth_tol");
  if (fs.has("coverage_width")) c.width = (int)fs.num("coverage_width");
  if (fs.has("coverage_height")) c.height = (int)fs.num("coverage_height");
  if (fs.has("coverage_occluder")) c.occluder = fs.str("coverage_occluder");
  return c;
}

// "" if the configuration can run, else what is wrong with it (checked before any training).  reference_cloud: a
// geometry_reference cloud is named -- then there is no mesh to take (reading mesh files is out of scope)
inline std::string coverage_eval_problem(const CoverageEvalConfig& c, bool reference_cloud = false) {
  if (!c.on) return "";
  if (c.occluder != "points" && c.occluder != "mesh") return "coverage_occluder must be points or mesh, got \"" + c.occluder + "\"";
  if (c.occluder == "mesh" && reference_cloud)
    return "coverage_occluder: mesh needs the ground-truth field's mesh, and geometry_reference names a cloud: there is no mesh to take";
  if (c.point_size < 1 || c.point_size > 64) return "coverage_point_size must be in [1, 64]";
  if (!(c.depth_tol >= 0.0) || !std::isfinite(c.depth_tol)) return "coverage_depth_tol must be finite and >= 0";
  if ((c.width == 0) != (c.height == 0)) return "coverage_width and coverage_height go together";
  if (c.width < 0 || c.width > 16384 || c.height < 0 || c.height > 16384) return "coverage_width / coverage_height must be in [1, 16384]";
  return "";
}

// one `name<TAB>value` line each, in the style of the PSNR / SSIM file: the counts, then coverage = covered / n_coverable and
// efficiency = covered / greedy_covered (nan where the denominator is 0), 17 significant digits; with the mesh occluder one more
// line, `occluder<TAB>mesh`
inline std::string coverage_text(uint64_t n_points, uint64_t n_coverable, int n_views, uint64_t covered, uint64_t greedy_covered,
                                 bool mesh_occluder = false) {
  char buf[512];
  const double coverage = n_coverable ? (double)covered / (double)n_coverable : NAN;
  const double efficiency = greedy_covered ? (double)covered / (double)greedy_covered : NAN;
  snprintf(buf, sizeof(buf), "n_points\t%llu\nn_coverable\t%llu\nn_views\t%d\ncovered\t%llu\ncoverage\t%.17g\ngreedy_covered\t%llu\nefficiency\t%.17g\n",
           (unsigned long long)n_points, (unsigned long long)n_coverable, n_views, (unsigned long long)covered, coverage,
           (unsigned long long)greedy_covered, efficiency);
  return mesh_occluder ? std::string(buf) + "occluder\tmesh\n" : std::string(buf);
}

} // namespace prvhost
