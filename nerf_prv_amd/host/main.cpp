// main.cpp -- prv_planner: the planner executable.  Mirrors the console protocol of the
// reference's main() (PRV_simulation/main.cpp:2294-2309): read a mode number, then object
// names until "-1", from stdin.  Mode 21 (ViewPlanning, main.cpp:3834-4004) is the one on
// the hot path; every render/score goes through the C ABI of include/prv.h in-process.
//
//   prv_planner [config.yaml]      (default "../DefaultConfiguration.yaml", main.cpp:2312)
// Mode 4 (InstantNGP, main.cpp:2463-2487) is here too: the PSNR-vs-#views curve files of an object.
//
// Ensemble members / the field under test come from model files
//   <model_path>/<object>/member_<e>.prvf  (prv_model_save_file format)
// or, when the config carries `synthetic_seed`, from the deterministic synthetic generator
// (member e = seed + e; reference images for method 5 from seed + 4096),
// or -- `train_steps: N` -- they are TRAINED in process every iteration, as the reference does through
// train_by_instantNGP (main.cpp:1658-1715, 2041-2043): a fresh field per member, N optimiser steps on the
// views chosen so far; the training images are rendered from the ground-truth field
// (`ground_truth_seed`, slot 6) with the dataset cameras of the iteration's json -- or, with `coverage_images: 1`
// and `train_images: files`, written once as <gt_path>/<N>/rgbaClip_<i>.png (what mode 3 leaves on disk) and read
// back through each iteration's json exactly as run.py's load_training_data does.
#include <cstdio>
#include <cstring>
#include <iostream>
#include <string>
#include <vector>

extern "C" {
#include "../../include/prv.h"
#include "../../include/prv_host.h"
}
#include "planner.hpp"
#include "fit_curve.hpp"
#include "geometry_eval.hpp"
#include "extras/pcd_io.hpp" // mode 3 only: the coloured cloud the splat rasteriser turns into rgbaClip images (not exported)
#include "extras/ply_io.hpp" // mode 3 with `gt_surface: mesh`: the vertex-coloured mesh prv_mesh_render turns into them (not exported)
#include "png_io.hpp"
#include "engine.hpp" // PlannerEngine, EngineConfig and, through it, the handles of prv_handles.hpp

using namespace prvhost;

namespace {

enum { GetCoverage = 3, InstantNGP = 4, GetPathPlan = 20, ViewPlanning = 21 }; // main.cpp:2284-2292

// get_coverage's images (main.cpp:1604-1618) from the ground-truth field: <gt_path>/<N>/rgbaClip_<i>.png for every
// view of the set, at the dataset size -- what mode 3 (GetCoverage) leaves on disk with PCL
int write_coverage_images(prv_ctx* ctx, const std::shared_ptr<Share_Data>& sd) {
  const std::string n = std::to_string(sd->num_of_views);
  CamsetPtr ds;
  if (prv_cameras_from_dataset_json(ctx, (sd->gt_path + "/" + n + ".json").c_str(), out_arg(ds)) != PRV_OK) return -60;
  int w = 0, h = 0;
  prv_camset_size(ds.get(), &w, &h);
  prv_render_opts o{};
  o.width = w;
  o.height = h;
  o.samples_per_ray = sd->samples_per_ray; // the rule of every other render of the run (0 = the engine's own stepping)
  o.step_mode = sd->samples_per_ray > 0 ? PRV_STEP_FIXED_S : PRV_STEP_NGP;
  o.spp = 1;
  o.min_transmittance = 1e-4f;
  const int count = prv_camset_count(ds.get());
  sd->access_directory(sd->gt_path + "/" + n);
  DeviceArray<uint8_t> dev;
  int rc = dev.alloc(ctx, (size_t)w * h * 4);
  std::vector<uint8_t> px((size_t)w * h * 4);
  for (int i = 0; rc == PRV_OK && i < count; i++) {
    rc = prv_render_rgba8(ctx, 6, ds.get(), &i, 1, &o, dev.get(), nullptr);
    if (rc == PRV_OK) rc = prv_memcpy_d2h(ctx, px.data(), dev.get(), px.size());
    if (rc == PRV_OK && png_write_rgba8(sd->gt_path + "/" + n + "/rgbaClip_" + std::to_string(i) + ".png", w, h, px.data()) != 0) rc = PRV_E_IO;
  }
  if (rc != PRV_OK) std::cerr << "coverage images: " << prv_last_error(ctx) << std::endl;
  return rc;
}

// One object's planning run: everything view_planning does around NBV_Net_Labeler::nbv_loop, kept in one place so that the
// shell can hold SEVERAL objects' loops at once (`shard: members`: run_members_lockstep below).  slot_base / pair_base: where
// the object's members live and who trains them (PlannerEngine).  The job owns the engine; the labeler's callbacks point at it.
struct PlanningJob {
  std::shared_ptr<Share_Data> sd;
  std::unique_ptr<PlannerEngine> engine; // (declared before the labeler: it outlives the callbacks that point at it)
  std::unique_ptr<NBV_Net_Labeler> lab;
  int first_view_id = -1;
  int setup(prv_ctx* ctx, const std::string& cfg, const std::string& name, int method, prv_comm* comm, int slot_base = 0, int pair_base = 0);
  int finish(int rc);

private:
  // setup()'s steps, in its order; each returns 0 or the run's exit code
  int read_config(const std::string& cfg, const std::string& name, int method, prv_comm* comm, bool lockstep, EngineConfig* config);
  int load_fixed_models(const std::string& name);
  int build_labeler(const Vec3& center, double size);
  int install_callbacks(const Vec3& center, double size);
};

// the object's Share_Data (this->sd; on ranks > 0 with its output tree moved to rank<r>/) and the engine's settings out of
// the yaml, with every refusal that needs no model, no training and no file of the run: -10, -1, -14, -25
int PlanningJob::read_config(const std::string& cfg, const std::string& name, int method, prv_comm* comm, bool lockstep, EngineConfig* config) {
  if (!NBV_Net_Labeler::method_in_scope(method)) { // before any directory, model or training: methods 1 / 4 are the PRVNet pipeline's
    std::cerr << "method_of_IG " << method << " is not built: this planner runs methods 0 (RandomIterative), 2 (EnsembleRGB), 3 "
                 "(EnsembleRGBDensity), 5 (PSNRCoverage) and 7 (RayEntropy), plus 9 (EnsembleTermination); 1 (RandomOneshot) and 4 (PVBCoverage) need the reference's PRVNet server" << std::endl;
    return -10;
  }
  sd = std::make_shared<Share_Data>(cfg, name, -1, -1, method); // main.cpp:3876
  if (!sd->ok) {
    std::cerr << sd->error << std::endl;
    return -1;
  }
  const int rank = comm ? prv_comm_rank(comm) : 0, world = comm ? prv_comm_world(comm) : 1;
  if (sd->views_per_iteration > 1 && (!NBV_Net_Labeler::batch_in_scope(method, sd->score_from_pngs) || world > 1)) { // before anything is written
    std::cerr << "views_per_iteration " << sd->views_per_iteration << " needs method_of_IG 7 (RayEntropy), score_path: fused and one rank "
                 "(the selection stage is single-rank); nothing was written" << std::endl;
    return -14;
  }
  if (!NBV_Net_Labeler::score_path_in_scope(method, sd->score_from_pngs)) { // before anything is written
    std::cerr << "method_of_IG 9 (EnsembleTermination) needs score_path: fused, not score_path: png; nothing was written" << std::endl;
    return -16;
  }
  if (rank > 0) sd->relocate_outputs(sd->pre_path + "rank" + std::to_string(rank) + "/"); // same loop, own scratch tree
  FileStorage fs;
  fs.open(cfg);
  *config = engine_config(fs, *sd, method);
  if (config->train_steps == 0 && method != RandomIterative)
    std::cerr << "WARNING: the members are NOT retrained on the chosen views (train_steps: 0 / pretrained_members: 1): "
                 "the view ranking of this run does not depend on the views it acquires (the reference retrains "
                 "n_steps per member per iteration, main.cpp:1668)" << std::endl;
  if (config->train_steps == 0 && lockstep) {
    std::cerr << "shard: members deals TRAININGS to the ranks: it needs train_steps > 0" << std::endl;
    return -25;
  }
  return 0;
}

// the fields that stay what they are for the whole run: the members of a run that does not train (synthetic seeds, or
// <model_path>/<object>/member_<e>.prvf / the instant-ngp snapshot of the same name), the ground truth of one that does
int PlanningJob::load_fixed_models(const std::string& name) {
  prv_ctx* ctx = engine->ctx;
  const EngineConfig& c = engine->cfg;
  int rc = PRV_OK;
  for (int e = 0; e < c.n_members && c.train_steps == 0 && rc == PRV_OK; e++) {
    if (c.synthetic) rc = prv_model_synthetic(ctx, e, &c.field, c.synthetic_seed + (uint64_t)e);
    else {
      const std::string stem = sd->model_path + name + "/member_" + std::to_string(e);
      rc = PRV_E_IO;
      for (const char* ext : {".prvf", ".ingp", ".msgpack"}) {
        if (!std::ifstream(stem + ext).is_open()) continue;
        rc = std::string(ext) == ".prvf" ? prv_model_load_file(ctx, e, (stem + ext).c_str()) : prv_model_load_ingp(ctx, e, (stem + ext).c_str());
        break;
      }
      if (rc == PRV_E_IO && !std::ifstream(stem + ".prvf").is_open() && !std::ifstream(stem + ".ingp").is_open() && !std::ifstream(stem + ".msgpack").is_open())
        rc = prv_model_load_file(ctx, e, (stem + ".prvf").c_str()); // for its error message
    }
  }
  if (rc == PRV_OK && c.train_steps > 0) rc = engine->load_ground_truth(); // members are trained from scratch every iteration
  if (rc != PRV_OK) std::cerr << "prv: " << prv_last_error(ctx) << std::endl;
  return rc;
}

// the labeler on the object's view space, its scorer and score dump, and what it leaves on disk before the loop starts
int PlanningJob::build_labeler(const Vec3& center, double size) {
  PlannerEngine* e = engine.get();
  lab.reset(new NBV_Net_Labeler(sd, center, size, [e](int method, int iteration, const std::string& scene, const std::string& render,
                                                       const std::vector<int>& ids, std::vector<double>& scores) {
    return e->score(method, iteration, scene, render, ids, scores);
  }));
  if (e->cfg.dump_records) { // diagnostics of the shell, not of the loop: every iteration's scores (raw doubles) beside the gathered records
    auto sd = this->sd;
    lab->on_scores = [sd](int iteration, const std::vector<int>&, const std::vector<double>& scores) {
      sd->access_directory(sd->save_path + "/scores");
      write_text(sd->save_path + "/scores/" + std::to_string(iteration) + ".bin", std::string((const char*)scores.data(), scores.size() * sizeof(double)));
    };
  }
  lab->get_coverage(); // <gt_path>/<N>.json (main.cpp:3882-3978, json part)
  if (e->cfg.coverage_images && e->cfg.train_steps > 0) return write_coverage_images(e->ctx, sd);
  return 0;
}

// evaluator, geometry evaluator, selector and engine: the other callbacks of the labeler, every one a pointer to the job's engine
int PlanningJob::install_callbacks(const Vec3& center, double size) {
  PlannerEngine* e = engine.get();
  if (sd->evaluate) {
    if (e->cfg.train_steps == 0) { // evaluation needs a ground truth to compare with
      const int rc = e->load_ground_truth();
      if (rc != PRV_OK) return rc;
    }
    lab->evaluator = [e, center, size](const std::string& scene, double* p, double* q) { return e->evaluate(scene, center, size, p, q); };
  }
  if (e->cfg.cover.on) { // a bad key of the coverage evaluation is reported before anything is set up or trained
    const std::string problem = coverage_eval_problem(e->cfg.cover, !e->cfg.geom.reference.empty());
    if (!problem.empty()) {
      std::cerr << "evaluate_coverage: " << problem << "; nothing was trained" << std::endl;
      return -85;
    }
  }
  if (e->cfg.geom.on || e->cfg.cover.on) { // the reference surface once per object; a run without a usable one stops here, before any training
    const int rc = e->geometry_setup(center, size);
    if (rc != PRV_OK) return rc;
    if (e->cfg.geom.on) lab->geometry_evaluator = [e](const std::string& path) { return e->geometry_evaluate(e->slot_of(0), path); };
  }
  if (e->cfg.cover.on) { // which reference point each view of the space sees, once per object
    const int rc = e->coverage_setup(lab->view_space->views, center, size);
    if (rc != PRV_OK) return rc;
    lab->coverage_evaluator = [e](const std::vector<int>& chosen, const std::string& path) { return e->coverage_evaluate(chosen, path); };
  }
  if (sd->views_per_iteration > 1)
    lab->selector = [e](int iteration, const std::string& scene, const std::string& render, const std::vector<int>& ids, int k,
                        std::vector<int>& chosen) { return e->select(iteration, scene, render, ids, k, chosen); };
  // train_by_instantNGP's reference signature -> the in-process engine (one run.py invocation per call); the same engine
  // object as the scorer's, so `score_path: png` and the fused path train and render the same members
  lab->engine = [e](const RunPyArgs& a) { return e->run_py(a); };
  if (sd->score_from_pngs && e->comm) {
    std::cerr << "score_path: png is the reference's single-process data flow; shard: views needs score_path: fused" << std::endl;
    return -24;
  }
  return 0;
}

int PlanningJob::setup(prv_ctx* ctx, const std::string& cfg, const std::string& name, int method, prv_comm* comm, int slot_base, int pair_base) {
  EngineConfig config;
  int rc = read_config(cfg, name, method, comm, slot_base != 0 || pair_base != 0, &config);
  if (rc != 0) return rc;
  engine.reset(new PlannerEngine(ctx, comm, sd, config, slot_base, pair_base));
  const double size = config.object_size;
  const Vec3 center(1e-10, 1e-10, 1e-10);
  if ((rc = load_fixed_models(name)) != 0) return rc;
  if ((rc = build_labeler(center, size)) != 0) return rc;
  if (method == PSNRCoverage && (rc = engine->render_references(name, lab->view_space->views, center, size)) != 0) return rc;
  // first view = the (0,0,r) top view of the set (main.cpp:3985-3995)
  first_view_id = -1;
  for (size_t i = 0; i < lab->view_space->views.size(); i++) {
    const Vec3& p = lab->view_space->views[i].init_pos;
    if (std::fabs(p.x) < 1e-6 && std::fabs(p.y) < 1e-6 && std::fabs(p.z - sd->view_space_radius) < 1e-6) first_view_id = (int)i;
  }
  if (first_view_id == -1) std::cout << "can not find now view id" << std::endl; // main.cpp:3993-3995
  return install_callbacks(center, size);
}

int PlanningJob::finish(int rc) {
  if (lab->final_psnr >= 0) std::cout << "final PSNR " << lab->final_psnr << " SSIM " << lab->final_ssim << std::endl;
  std::cout << "chosen_nbvs:";
  for (int v : lab->chosen_nbvs) std::cout << ' ' << v;
  std::cout << std::endl;
  return rc;
}

int view_planning(prv_ctx* ctx, const std::string& cfg, const std::string& name, int method, prv_comm* comm) {
  PlanningJob job;
  int rc = job.setup(ctx, cfg, name, method, comm);
  if (rc != 0) return rc;
  return job.finish(job.lab->nbv_loop(job.first_view_id, 0));
}

// `shard: members` (BASELINE configs[4] on several GPUs; SURVEY section 8(e), main.cpp:2041-2043): the objects' loops in
// LOCKSTEP.  Round k of every object is prepared (its json pair written), then the E member-trainings of every object --
// objects x E (object, member) pairs, dealt to the ranks round-robin: pair p = o * E + e goes to rank p % world -- run side
// by side on their owners (prv_train_steps_multi over everything this rank owns), then object by object the members are
// brought together (prv_model_exchange_slots: one group of broadcasts), the candidates scored views-sharded (one all-gather)
// and the next view chosen.  With `shard: objects` 5 objects keep 5 of 8 GPUs busy; here 25 pairs keep all 8 busy with 3 or 4
// trainings each (22 % idle against 37.5 %).  Every rank walks every object's loop, so every collective is entered by all
// ranks in the same order; objects beyond the slots of one context (7 ensembles of up to 8 members) go in further batches.
int run_members_lockstep(prv_ctx* ctx, const std::string& cfg, const std::vector<std::string>& names, int method, prv_comm* comm) {
  constexpr int kBatch = (PRV_MAX_SLOTS - 8) / PRV_MAX_MODELS; // slots 0..7 stay the shared ones (ground truth 6, reference 7)
  int worst = 0;
  for (size_t b0 = 0; b0 < names.size(); b0 += (size_t)kBatch) {
    const size_t nb = std::min(names.size() - b0, (size_t)kBatch);
    std::vector<std::unique_ptr<PlanningJob>> jobs;
    std::vector<int> live; // 0: in the loop, 1: ended, < 0: failed
    for (size_t k = 0; k < nb; k++) {
      std::cout << "object " << names[b0 + k] << " method " << method << " (lockstep batch of " << nb << ")" << std::endl;
      jobs.emplace_back(new PlanningJob());
      PlanningJob& j = *jobs.back();
      int members = 1;
      {
        Share_Data probe(cfg, names[b0 + k], -1, -1, method);
        if (probe.ok && (method == EnsembleRGB || method == EnsembleRGBDensity || method == EnsembleTermination)) members = probe.ensemble_num;
      }
      int rc = j.setup(ctx, cfg, names[b0 + k], method, comm, 8 + (int)k * PRV_MAX_MODELS, (int)(b0 + k) * members);
      if (rc == 0) rc = j.lab->nbv_begin(j.first_view_id, 0);
      live.push_back(rc);
    }
    for (;;) {
      bool any = false;
      for (size_t k = 0; k < nb; k++) // a round's json pairs (and, where a loop ends here, its final evaluation)
        if (live[k] == 0) {
          live[k] = jobs[k]->lab->nbv_prepare();
          any = any || live[k] == 0;
        }
      if (!any) break;
      // every (object, member) pair of the round this rank owns, side by side
      std::vector<TrainerPtr> trs;
      std::vector<char> trained(nb, 0); // the objects whose members this round trains here: their scoring step only brings them together
      int rc = PRV_OK, steps = 0;
      const double t0 = now_seconds();
      for (size_t k = 0; k < nb && rc == PRV_OK; k++) {
        if (live[k] != 0 || jobs[k]->engine->cfg.train_steps <= 0 || method == RandomIterative) continue;
        PlannerEngine& e = *jobs[k]->engine;
        std::vector<int> all(e.n_members);
        for (int m = 0; m < e.n_members; m++) all[m] = m;
        rc = e.create_trainers(jobs[k]->lab->run.scene_json, all, trs);
        steps = e.cfg.train_steps;
        trained[k] = rc == PRV_OK;
      }
      const size_t n_mine = trs.size();
      if (rc == PRV_OK && !trs.empty()) {
        std::vector<prv_trainer*> raw = raw_trainers(trs);
        rc = prv_train_steps_multi(raw.data(), (int)raw.size(), steps, nullptr);
      }
      trs.clear(); // order is behaviour: the trainers are destroyed before the timing line is printed, and before the exchange
      if (getenv("PRV_PLANNER_TIMING"))
        std::cerr << "train_pairs: " << n_mine << " (object, member) trainings of this round on rank " << (comm ? prv_comm_rank(comm) : 0) << ", " << steps
                  << " steps side by side, " << now_seconds() - t0 << " s" << std::endl;
      if (rc != PRV_OK) {
        std::cerr << "prv: " << prv_last_error(ctx) << std::endl;
        for (size_t k = 0; k < nb; k++)
          if (live[k] == 0) live[k] = rc; // (every rank fails the same way or the next collective reports it)
        break; // (first finding: a rank that fails alone leaves here while the others wait in the next collective)
      }
      for (size_t k = 0; k < nb; k++)
        if (live[k] == 0) {
          // the scoring step only brings these members together: score / select -> prepare_members -> train_members takes the flag.
          // (third finding: methods 2 and 3 under `score_path: png` score through run_py, which never takes it -- the
          // flag then stays set into the final `evaluate`, which skips its training)
          if (trained[k]) jobs[k]->engine->members_pretrained = true;
          live[k] = jobs[k]->lab->nbv_decide();
        }
    }
    for (size_t k = 0; k < nb; k++) {
      const int rc = jobs[k]->lab ? jobs[k]->finish(live[k] < 0 ? live[k] : 0) : live[k];
      if (rc != 0) worst = rc;
    }
  }
  return worst;
}

// mode 4 (main.cpp:2463-2487): the PSNR-vs-#views curve of an object.  For n = 3, 3 + add, ... <= max: a field is
// trained on the n-view coverage set (<gt_path>/<n>.json, written here; view set <viewspace_path>/<n>.txt or, when
// that file does not exist, a generated n-point hemisphere) and evaluated on the test set; <gt_path>/<n>.txt gets
// run.py's two metrics lines -- the files NeRF_fit_curve.cpp:103-115 reads.  Existing files are kept (:2473).
int instant_ngp_curves(prv_ctx* ctx, const std::string& cfg, const std::string& name) {
  FileStorage fs;
  fs.open(cfg);
  const Vec3 center(1e-10, 1e-10, 1e-10);
  auto sd0 = std::make_shared<Share_Data>(cfg, name, -1, -1, 0);
  if (!sd0->ok) {
    std::cerr << sd0->error << std::endl;
    return -1;
  }
  PlannerEngine engine(ctx, nullptr, sd0, engine_config(fs, *sd0, 0));
  const double size = engine.cfg.object_size;
  if (engine.cfg.train_steps <= 0) {
    std::cerr << "mode 4 trains: n_steps / train_steps must be positive" << std::endl;
    return -50;
  }
  int rc = engine.load_ground_truth();
  if (rc != PRV_OK) {
    std::cerr << "prv: " << prv_last_error(ctx) << std::endl;
    return rc;
  }
  const int n_max = sd0->coverage_view_num_max > 0 ? sd0->coverage_view_num_max : 90;
  const int n_add = sd0->coverage_view_num_add > 0 ? sd0->coverage_view_num_add : 1;
  sd0->access_directory(sd0->gt_path);
  std::vector<int> counts;
  for (int n = 3; n <= n_max; n += n_add) counts.push_back(n);
  const int n_full = fs.has("coverage_view_num_full") ? (int)fs.num("coverage_view_num_full") : 100; // main.cpp:2480-2484
  counts.push_back(n_full); // the upper bound of the curve ("100.txt")
  std::vector<double> xs, ys;
  double max_psnr = 0.0;
  // pass 1: which curve points are missing (existing metrics files are kept, :2473), and their scene jsons
  std::vector<double> psnrs(counts.size(), 0.0);
  std::vector<size_t> missing;
  std::vector<std::string> scenes;
  for (size_t ci = 0; ci < counts.size(); ci++) {
    const int n = counts[ci];
    const std::string metrics = sd0->gt_path + "/" + std::to_string(n) + ".txt";
    double ssim = 0;
    if (prvh_read_metrics(metrics.c_str(), &psnrs[ci], &ssim) == 0) continue;
    // the n-view coverage set
    std::vector<std::vector<double>> pts((size_t)n, std::vector<double>(3, 0.0));
    std::ifstream fin(sd0->viewspace_path + std::to_string(n) + ".txt");
    if (fin.is_open()) {
      for (int i = 0; i < n; i++)
        for (int j = 0; j < 3; j++) fin >> pts[i][j];
    } else {
      std::vector<double> flat((size_t)n * 3);
      prvh_hemisphere_generate(n, flat.data());
      for (int i = 0; i < n; i++)
        for (int j = 0; j < 3; j++) pts[i][j] = flat[(size_t)i * 3 + j];
    }
    sd0->num_of_views = n;
    sd0->pt_sphere = pts;
    sd0->pt_norm = std::sqrt(pts[0][0] * pts[0][0] + pts[0][1] * pts[0][1] + pts[0][2] * pts[0][2]);
    View_Space vs(sd0);
    vs.set_view_space(center, size);
    Value root = transforms_header(sd0->color_intrinsics, sd0->ray_casting_aabb_scale, size, center, 0);
    for (size_t i = 0; i < vs.views.size(); i++) {
      Value v;
      v["file_path"] = Value(std::to_string(n) + "/rgbaClip_" + std::to_string(i) + ".png");
      v["transform_matrix"] = matrix_json(view_transform_matrix(vs.views[i], Mat4::Identity(), center));
      root["frames"].append(v);
    }
    // the test set's own json is <gt_path>/<evaluate_views>.json: keep the two apart when the sizes coincide
    const std::string scene = sd0->gt_path + "/" + std::to_string(n) + (n == engine.cfg.eval_views ? "_train.json" : ".json");
    write_text(scene, prvjson::to_styled_string(root));
    missing.push_back(ci);
    scenes.push_back(scene);
  }
  // pass 2: the missing points, four fields at a time side by side (train_scenes_side_by_side), each evaluated on the test set
  // (a member-step costs 95 us in a round of four, 101 in a round of five, 98 of three: profiles/r05_member_queues.txt)
  std::string test_json;
  if (!missing.empty() && (rc = engine.write_test_json(center, size, &test_json)) != PRV_OK) return rc;
  constexpr size_t kSideBySide = 4;
  for (size_t g0 = 0; g0 < missing.size(); g0 += kSideBySide) {
    const size_t g1 = std::min(missing.size(), g0 + kSideBySide);
    const bool timing = getenv("PRV_PLANNER_TIMING") != nullptr; // dev: where the curve's seconds go
    double t0 = now_seconds();
    if ((rc = engine.train_scenes_side_by_side(std::vector<std::string>(scenes.begin() + (long)g0, scenes.begin() + (long)g1))) != PRV_OK) return rc;
    if (timing) std::cerr << "curve_group: " << g1 - g0 << " fields trained in " << now_seconds() - t0 << " s" << std::endl;
    for (size_t k = g0; k < g1; k++) {
      const int n = counts[missing[k]];
      double psnr = 0, ssim = 0;
      t0 = now_seconds();
      rc = engine.evaluate_on(test_json, (int)(k - g0), &psnr, &ssim);
      if (timing) std::cerr << "curve_eval: " << n << " views, evaluated in " << now_seconds() - t0 << " s" << std::endl;
      if (rc != PRV_OK) return rc;
      prvh_write_metrics((sd0->gt_path + "/" + std::to_string(n) + ".txt").c_str(), psnr, ssim);
      std::cout << "views " << n << " PSNR " << psnr << " SSIM " << ssim << std::endl;
      psnrs[missing[k]] = psnr;
    }
  }
  for (size_t ci = 0; ci < counts.size(); ci++) {
    if (ci + 1 < counts.size()) {
      xs.push_back((double)counts[ci]);
      ys.push_back(psnrs[ci]);
    } else {
      max_psnr = psnrs[ci];
    }
  }
  // the label file Origin's fit script leaves next to the curve (NeRF_fit_curve.cpp:119-206)
  if (xs.size() >= 4) {
    const FitResult fit = fit_lognormal_cdf(xs, ys, max_psnr);
    write_label_file(sd0->gt_path + "/label.txt", fit, max_psnr);
    const Labels L = make_labels(fit.f, max_psnr);
    std::cout << "label: converged " << (fit.converged ? 1 : 0) << " gap 2% at " << L.gap[2] << " views, gradient 0.02 at "
              << L.gradient[1] << " views" << std::endl; // main.cpp:2641-2642 uses gradient index 1
  }
  return 0;
}

// mode 3 (GetCoverage, main.cpp:2343-2462 -> NBV_Net_Labeler's constructor :636-1035 + get_coverage :1581-1656) for
// an object given as a coloured cloud <model_path>/<name>.pcd: centre the cloud on its centroid, bounding radius x
// 17/16 (:827-833), bring it to the object size (the reference draws a random size in [0.075, 0.115] m and keeps it
// in <gt_path>/size.txt, :851-867; here: that file if it exists, else `object_size`), place the N views, write
// <gt_path>/<N>.json and the <N>/rgbaClip_<i>.png images (PCL screenshot + convertToAlpha + flip = prv_splat_points).
// `gt_surface: mesh` (default `points`): the object is the vertex-coloured mesh <model_path>/<name>.ply instead (the layout
// prv_mesh_write_file writes); its vertices are centred and scaled as the cloud's points are, and the images are
// prv_mesh_render's -- a surface without holes and without a point size.  A bad key or file is refused before anything is written.
int get_coverage_from_cloud(prv_ctx* ctx, const std::string& cfg, const std::string& name) {
  FileStorage fs;
  fs.open(cfg);
  const std::string surface = fs.has("gt_surface") ? fs.str("gt_surface") : "points";
  if (surface != "points" && surface != "mesh") {
    std::cerr << "gt_surface must be points or mesh, got \"" << surface << "\": nothing was written" << std::endl;
    return -73;
  }
  const bool mesh = surface == "mesh";
  auto sd = std::make_shared<Share_Data>(cfg, name, -1, -1, 0);
  if (!sd->ok) {
    std::cerr << sd->error << std::endl;
    return -1;
  }
  std::vector<float> xyz;
  std::vector<uint8_t> rgb;
  std::vector<uint32_t> tri; // (gt_surface: mesh)
  if (mesh) {
    std::string why = ply_read(sd->model_path + name + ".ply", xyz, rgb, tri);
    if (why.empty() && xyz.empty()) why = sd->model_path + name + ".ply: a mesh without vertices";
    if (!why.empty()) {
      std::cerr << "gt_surface: mesh: " << why << ": nothing was written" << std::endl;
      return -74;
    }
  } else {
    const std::string cloud = sd->model_path + name + ".pcd";
    const int prc = pcd_read(cloud, xyz, rgb);
    if (prc != 0) {
      std::cerr << "cannot read " << cloud << " (" << prc << ")" << std::endl;
      return -70;
    }
  }
  const size_t n = xyz.size() / 3;
  double c[3] = {0, 0, 0};
  for (size_t i = 0; i < n; i++)
    for (int a = 0; a < 3; a++) c[a] += xyz[3 * i + a];
  for (int a = 0; a < 3; a++) c[a] /= (double)n;
  double radius = 0.0;
  for (size_t i = 0; i < n; i++) {
    double d2 = 0;
    for (int a = 0; a < 3; a++) {
      xyz[3 * i + a] = (float)(xyz[3 * i + a] - c[a]); // "move to centre" (:793-797)
      d2 += (double)xyz[3 * i + a] * xyz[3 * i + a];
    }
    radius = std::max(radius, std::sqrt(d2));
  }
  const double predicted_raw = radius * 17.0 / 16.0;
  sd->access_directory(sd->gt_path);
  PlannerEngine engine(ctx, nullptr, sd, engine_config(fs, *sd, 0)); // (its labeler only places the views: nothing is scored here)
  double size = engine.cfg.object_size;
  {
    std::ifstream size_reader(sd->gt_path + "/size.txt");
    double v = -1;
    if (size_reader.is_open() && (size_reader >> v)) {
      if (v < 0) {
        std::cout << "no size. Skip." << std::endl; // :858-862
        return 0;
      }
      size = v;
    } else {
      write_text(sd->gt_path + "/size.txt", std::to_string(size) + "\n");
    }
  }
  std::vector<Vec3> pts(n);
  for (size_t i = 0; i < n; i++) {
    for (int a = 0; a < 3; a++) xyz[3 * i + a] = (float)(xyz[3 * i + a] * size / predicted_raw);
    pts[i] = Vec3(xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2]);
  }
  NBV_Net_Labeler labeler(sd, Vec3(0, 0, 0), size, [&engine](int method, int iteration, const std::string& scene, const std::string& render,
                                                             const std::vector<int>& ids, std::vector<double>& scores) {
    return engine.score(method, iteration, scene, render, ids, scores);
  });
  labeler.view_space->get_view_space(pts); // centroid + 17/16 x radius of the scaled cloud (View_Space.hpp:517-558)
  if (labeler.get_coverage() != 0) return -71;
  const std::string N = std::to_string(sd->num_of_views);
  CamsetPtr ds;
  if (prv_cameras_from_dataset_json(ctx, (sd->gt_path + "/" + N + ".json").c_str(), out_arg(ds)) != PRV_OK) return -72;
  int w = 0, h = 0;
  prv_camset_size(ds.get(), &w, &h);
  const int count = prv_camset_count(ds.get());
  const int point_size = fs.has("points_size_cloud") ? (int)fs.num("points_size_cloud") : 5; // yaml:18
  DeviceArray<float> xyz_dev;
  DeviceArray<uint8_t> rgb_dev, img_dev;
  MeshPtr surface_mesh;
  const Vec3 oc = labeler.view_space->object_center_world;
  const double scale = 0.5 / labeler.view_space->predicted_size; // the json's (main.cpp:1599-1602)
  const double offset[3] = {0.5 + oc.z, 0.5 + oc.x, 0.5 + oc.y};
  int rc = img_dev.alloc(ctx, (size_t)w * h * 4);
  if (mesh) { // the vertices go where prv_splat_points puts the cloud's points (geometry_eval.hpp)
    geometry_to_engine(xyz, scale, offset);
    if (rc == PRV_OK) rc = prv_mesh_from_arrays(ctx, xyz.data(), n, tri.data(), tri.size() / 3, out_arg(surface_mesh));
    if (rc == PRV_OK) rc = prv_mesh_set_colors(surface_mesh.get(), rgb.data(), n);
  } else {
    if (rc == PRV_OK) rc = xyz_dev.alloc(ctx, xyz.size() * 4);
    if (rc == PRV_OK) rc = rgb_dev.alloc(ctx, rgb.size());
    if (rc == PRV_OK) rc = prv_memcpy_h2d(ctx, xyz_dev.get(), xyz.data(), xyz.size() * 4);
    if (rc == PRV_OK) rc = prv_memcpy_h2d(ctx, rgb_dev.get(), rgb.data(), rgb.size());
  }
  sd->access_directory(sd->gt_path + "/" + N);
  std::vector<uint8_t> px((size_t)w * h * 4);
  for (int i = 0; rc == PRV_OK && i < count; i++) {
    rc = mesh ? prv_mesh_render(ctx, surface_mesh.get(), ds.get(), &i, 1, w, h, 1, img_dev.get(), nullptr, nullptr)
              : prv_splat_points(ctx, xyz_dev.get(), rgb_dev.get(), n, scale, offset, ds.get(), &i, 1, w, h, point_size, 1, img_dev.get());
    if (rc == PRV_OK) rc = prv_memcpy_d2h(ctx, px.data(), img_dev.get(), px.size());
    if (rc == PRV_OK && png_write_rgba8(sd->gt_path + "/" + N + "/rgbaClip_" + std::to_string(i) + ".png", w, h, px.data()) != 0) rc = PRV_E_IO;
  }
  if (rc != PRV_OK) std::cerr << "prv: " << prv_last_error(ctx) << std::endl;
  std::cout << "object " << name << ": " << n << (mesh ? " vertices, " + std::to_string(tri.size() / 3) + " triangles" : std::string(" points")) << ", size " << size
            << " m, " << count << " views" << std::endl;
  return rc;
}

// mode 20 (main.cpp:3622-3832): for every view set <viewspace_path>/<N>.txt, N = 3..100, the shortest open tour
// over the unit view sphere from the (0,0,1) view, written to <N>_path.txt, one id per line (:3826-3830).
// No GPU involved.  Sets without a (0,0,1) view are reported and skipped ("can not find now view id", :3648).
int get_path_plan(const std::string& cfg) {
  FileStorage fs;
  if (!fs.open(cfg)) {
    std::cerr << "cannot open " << cfg << std::endl;
    return 5;
  }
  const std::string vs = fs.str("viewspace_path");
  const std::string out_dir = fs.has("path_plan_out") ? fs.str("path_plan_out") : vs; // the reference writes next to the inputs
  int written = 0;
  for (int n = 3; n <= 100; n++) {
    std::ifstream fin(vs + std::to_string(n) + ".txt");
    if (!fin.is_open()) continue;
    std::vector<View> views;
    std::vector<int> labels;
    int now_view_id = -1;
    for (int i = 0; i < n; i++) {
      double x = 0, y = 0, z = 0;
      fin >> x >> y >> z;
      views.emplace_back(Vec3(x, y, z));
      if (std::fabs(x) < 1e-6 && std::fabs(y) < 1e-6 && std::fabs(z - 1) < 1e-6) now_view_id = i;
      labels.push_back(i);
    }
    if (now_view_id == -1) {
      std::cout << "can not find now view id (" << n << ".txt)" << std::endl;
      continue;
    }
    Global_Path_Planner gpp(views, labels, now_view_id, Vec3(1e-10, 1e-10, 1e-10), 0.0);
    const double total_dis = gpp.solve();
    std::string text;
    for (int id : gpp.get_path_id_set()) text += std::to_string(id) + "\n";
    if (!write_text(out_dir + std::to_string(n) + "_path.txt", text)) return -3;
    std::cout << "view space " << n << " total dis is: " << total_dis << (gpp.exact ? "" : " (heuristic)") << std::endl;
    written++;
  }
  return written > 0 ? 0 : -1;
}

int env_int(const char* key, int fallback) {
  const char* v = getenv(key);
  return v && *v ? atoi(v) : fallback;
}

} // namespace

// PRV_SEGV_TRACE=1 (diagnostics): a crash prints where it happened before the process dies -- the phase of the process
// (running / shutting the runtime down / returning from main / exit handlers), the faulting thread, the fault address, the
// program counter and the mapping it lies in (a PC in no mapping = code that has been unloaded under a running thread)
#include <csignal>
#include <execinfo.h>
#include <sys/syscall.h>
#include <ucontext.h>
#include <unistd.h>
static volatile int g_phase = 0; // 0 run(), 1 inside prv_runtime_shutdown, 2 main is returning, 3 exit handlers have started
static void segv_trace(int sig, siginfo_t* info, void* uc_) {
  char buf[512];
  const ucontext_t* uc = (const ucontext_t*)uc_;
  const unsigned long long pc = uc ? (unsigned long long)uc->uc_mcontext.gregs[REG_RIP] : 0ull;
  const long tid = syscall(SYS_gettid);
  int n = snprintf(buf, sizeof(buf), "prv_planner: fatal signal %d in phase %d, thread %ld (%s), fault address %p, pc 0x%llx\n", sig,
                   g_phase, tid, tid == (long)getpid() ? "main" : "not main", info ? info->si_addr : nullptr, pc);
  (void)!write(2, buf, (size_t)n);
  if (FILE* maps = fopen("/proc/self/maps", "r")) { // not async-signal-safe; the process is dying anyway
    bool found = false;
    while (fgets(buf, sizeof(buf), maps)) {
      unsigned long long lo = 0, hi = 0;
      if (sscanf(buf, "%llx-%llx", &lo, &hi) == 2 && pc >= lo && pc < hi) {
        (void)!write(2, "  pc lies in: ", 14);
        (void)!write(2, buf, strlen(buf));
        found = true;
      }
    }
    fclose(maps);
    if (!found) (void)!write(2, "  pc lies in NO mapping (unloaded code)\n", 40);
  }
  void* frames[64];
  const int nf = backtrace(frames, 64);
  backtrace_symbols_fd(frames, nf, 2);
  signal(sig, SIG_DFL);
  raise(sig);
}
static void install_trace() {
  struct sigaction sa;
  memset(&sa, 0, sizeof(sa));
  sa.sa_sigaction = segv_trace;
  sa.sa_flags = SA_SIGINFO | SA_NODEFER;
  sigaction(SIGSEGV, &sa, nullptr);
  sigaction(SIGBUS, &sa, nullptr);
  sigaction(SIGABRT, &sa, nullptr);
  atexit([] { g_phase = 3; });
}

static int run(int argc, char** argv);

// Every context has been destroyed and every file closed when run() returns.  What an ordinary exit then adds is the
// static teardown of the HIP / HSA runtime, which this process does not control: 4 of 19,300 exits that shut the runtime
// down in order (prv_runtime_shutdown: synchronise + hipDeviceReset) and then returned from main still died AFTER main
// had returned, on a worker thread of the runtime itself (profiles/NOTES.md, round 3).  A planner run that finished
// correctly must not report SIGSEGV, so the DEFAULT exit is: ordered prv_runtime_shutdown, flush every stream, _exit(rc)
// -- the runtime's exit handlers never run.  PRV_PLANNER_EXIT=normal: the same shutdown, then an ordinary return (static
// destructors and atexit handlers run; chosen automatically under a profiler, which writes its files from an exit
// handler); =noreset: a plain return without the shutdown (round 2's behaviour, for the stress script only).
int main(int argc, char** argv) {
  if (getenv("PRV_SEGV_TRACE")) install_trace();
  const int rc = run(argc, argv);
  const char* how_c = getenv("PRV_PLANNER_EXIT");
  std::string how = how_c && *how_c ? how_c : "quick";
  if (how == "quick") {
    if (const char* pre = getenv("LD_PRELOAD"))
      if (std::string(pre).find("rocprof") != std::string::npos) how = "normal";
    for (char** e = environ; e && *e; e++)
      if (strncmp(*e, "ROCPROF", 7) == 0 || strncmp(*e, "ROCP_", 5) == 0 || strncmp(*e, "ROCTRACER", 9) == 0) how = "normal";
  }
  g_phase = 1;
  if (how != "noreset") (void)prv_runtime_shutdown();
  g_phase = 2;
  std::cout.flush();
  std::cerr.flush();
  fflush(nullptr);
  if (how == "quick") _exit(rc);
  return rc;
}

static int run(int argc, char** argv) {
  const std::string cfg = argc > 1 ? argv[1] : "../DefaultConfiguration.yaml";
  int mode = -1;
  std::cout << "input mode:" << std::endl;
  if (!(std::cin >> mode)) return 2;
  std::vector<std::string> names;
  std::cout << "input object names (-1 to stop):" << std::endl; // main.cpp:2299-2309
  std::string name;
  while (std::cin >> name && name != "-1") names.push_back(name);
  // Several GPUs, one process per GPU, launched by torchrun or by hand with RANK / WORLD_SIZE / LOCAL_RANK:
  //  shard objects (default; BASELINE config 5): the objects are independent, rank r takes the names i % world == r,
  //    no collective;
  //  shard views (`shard: views` in the yaml or PRV_SHARD=views; BASELINE config 4): every rank runs the loop of every
  //    object, the candidates of an iteration are dealt to the ranks, ONE all-gather of the score records per round
  //    (RCCL over xGMI; PRV_COMM=socket for ranks that share a GPU), trained members exchanged device to device;
  //  shard members (`shard: members` / PRV_SHARD=members; BASELINE config 5 with more GPUs than objects): the objects'
  //    loops in lockstep, the (object, member) trainings of a round dealt to the ranks round-robin (run_members_lockstep).
  const int world = env_int("WORLD_SIZE", 1), rank = env_int("RANK", 0);
  if (world < 1 || rank < 0 || rank >= world) {
    std::cerr << "RANK " << rank << " / WORLD_SIZE " << world << " make no sense" << std::endl;
    return 2;
  }
  bool shard_views = false, shard_members = false;
  {
    FileStorage fs0;
    const char* e = getenv("PRV_SHARD");
    std::string how = e && *e ? e : (fs0.open(cfg) && fs0.has("shard") ? fs0.str("shard") : "objects");
    if (how != "objects" && how != "views" && how != "members") {
      std::cerr << "shard must be 'objects', 'views' or 'members', not '" << how << "'" << std::endl;
      return 2;
    }
    shard_views = how == "views" && world > 1 && mode == ViewPlanning;
    shard_members = how == "members" && mode == ViewPlanning; // (with one rank: the lockstep walk alone, every training on this GPU)
  }
  if (world > 1 && !shard_views && !shard_members) {
    std::vector<std::string> mine;
    for (size_t i = 0; i < names.size(); i++)
      if ((int)(i % (size_t)world) == rank) mine.push_back(names[i]);
    names.swap(mine);
  }
  if (mode == GetPathPlan) return rank != 0 || get_path_plan(cfg) == 0 ? 0 : 1; // host only: before any GPU context exists
  if (mode != ViewPlanning && mode != InstantNGP && mode != GetCoverage) {
    std::cerr << "mode " << mode << " is outside the render/score path this build covers (21 = ViewPlanning, 4 = InstantNGP, "
                 "3 = GetCoverage, 20 = GetPathPlan)" << std::endl;
    return 3;
  }
  prv_ctx* ctx = nullptr;
  const int n_dev = prv_device_count();
  const int device = n_dev > 0 ? env_int("LOCAL_RANK", rank) % n_dev : 0; // fewer GPUs than ranks: they share
  if (prv_create(&ctx, device) != PRV_OK) {
    std::cerr << "prv: " << prv_last_error(nullptr) << std::endl;
    return 4;
  }
  FileStorage fs;
  if (!fs.open(cfg)) {
    std::cerr << "cannot open " << cfg << std::endl;
    return 5;
  }
  prv_comm* comm = nullptr;
  if (shard_views || (shard_members && world > 1)) {
    if (prv_comm_create(ctx, rank, world, nullptr, nullptr, &comm) != PRV_OK) {
      std::cerr << "prv: " << prv_last_error(ctx) << std::endl;
      prv_destroy(ctx);
      return 6;
    }
    std::cout << "rank " << rank << " of " << world << ": " << (shard_members ? "member trainings dealt round-robin, views sharded" : "views sharded") << ", transport "
              << prv_comm_transport(comm) << std::endl;
  }
  if (mode == InstantNGP || mode == GetCoverage) {
    int worst = 0;
    for (const auto& n : names) {
      const int rc = mode == InstantNGP ? instant_ngp_curves(ctx, cfg, n) : get_coverage_from_cloud(ctx, cfg, n);
      if (rc != 0) worst = rc;
    }
    prv_destroy(ctx);
    return worst == 0 ? 0 : 1;
  }
  // main.cpp:3838-3840 runs methods {4,0,1,2,3}; here: the configured one, or all that are in scope
  std::vector<int> methods;
  if (fs.has("method_of_IG") && fs.num("method_of_IG") >= 0) methods.push_back((int)fs.num("method_of_IG"));
  else methods = {RandomIterative, EnsembleRGB, EnsembleRGBDensity, PSNRCoverage};
  int worst = 0;
  if (shard_members) {
    for (int m : methods) {
      const int rc = run_members_lockstep(ctx, cfg, names, m, comm);
      if (rc != 0) worst = rc;
    }
  } else {
    for (const auto& n : names)
      for (int m : methods) {
        std::cout << "object " << n << " method " << m << std::endl;
        const int rc = view_planning(ctx, cfg, n, m, comm);
        if (rc != 0) worst = rc;
      }
  }
  if (comm) prv_comm_destroy(comm);
  prv_destroy(ctx);
  return worst == 0 ? 0 : 1;
}
