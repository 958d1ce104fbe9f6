// engine.hpp -- PlannerEngine: what stands behind the callbacks of one object's NBV_Net_Labeler in prv_planner -- the
// scorer, the in-process run.py engine, the member trainer and exchange, the final and the geometric evaluator and the
// batch selector, all through the C ABI of include/prv.h.  One engine per object, owned by the shell (PlanningJob) and
// never copied: the callbacks are lambdas that hold a pointer to it, and its destructor is the only clean-up.
// Everything it is told comes from ONE reading of the yaml, engine_config().
// prv_planner-private: included by main.cpp only (libprv_host.so holds no libprv_hip symbol).
#pragma once
#include <cstdio>
#include <iostream>
#include <string>
#include <vector>

#include "planner.hpp"
#include "geometry_eval.hpp"
#include "coverage_eval.hpp"
#include "extras/pcd_io.hpp"
#include "png_io.hpp"
#include "prv_handles.hpp"

namespace prvhost {

// Optimiser steps per member per iteration.  The reference retrains every ensemble member on the views chosen so
// far in EVERY iteration with `--n_steps <n_steps>` (main.cpp:1668, 2041-2043), so the yaml's `n_steps` is the
// default; `train_steps: N` overrides the count.  Scoring members that are NOT retrained (files / synthetic seeds:
// a ranking that does not depend on the acquired views) is an explicit opt-in: `train_steps: 0` or
// `pretrained_members: 1`.
inline int configured_train_steps(const FileStorage& fs, const Share_Data& sd) {
  if (fs.has("pretrained_members") && fs.num("pretrained_members") > 0) return 0;
  if (fs.has("train_steps")) return std::max(0, (int)fs.num("train_steps"));
  return std::max(0, sd.n_steps);
}

// every yaml key the shell and its engine read beyond Share_Data's own, read once
struct EngineConfig {
  int n_members = 1;        // methods 2, 3 and 9: Share_Data's ensemble_num; every other method scores one field
  prv_field_desc field{};   // field_* / synthetic_table_amp: the members that are loaded or synthesised, the ground truth, the reference
  double object_size = 0.1; // synthetic objects sit at the origin (+1e-10, main.cpp:447) with the configured size
  bool synthetic = false;   // synthetic_seed: member e = seed + e, method 5's reference field = seed + 4096
  uint64_t synthetic_seed = 0;
  uint64_t ground_truth_seed = 0x5EED0002ull; // the ground-truth field of slot 6
  // training in the loop (read only when train_steps > 0: a run that does not train evaluates at the dataset size)
  int train_steps = 0;
  int train_rays = 0;                         // 0: the library default
  int train_patch_w = 0, train_patch_h = 0;   // prv_train_opts.patch_w / patch_h (0: the library default, single pixels); a speed / quality trade, DESIGN.md
  int train_step_mode = -1;                   // prv_train_opts.step_mode (-1: the library default = the engine's marcher; 0: 128 uniform samples per ray, rounds 1-5)
  int train_w = 0, train_h = 0;               // train_width / train_height (0: the dataset size)
  prv_field_desc train_desc{};                // a fresh member: `field` with train_density_bias and a table amplitude of 1e-4
  uint64_t train_seed = 0x1234;
  bool train_deterministic = false;           // prv_train_opts.deterministic (bit-reproducible members: tests)
  bool images_from_files = false;             // train_images: files -> the json's file_path PNGs (the reference's data flow)
  bool coverage_images = false;               // coverage_images: 1 -> <gt_path>/<N>/rgbaClip_<i>.png from the ground truth (with training only)
  bool save_renders = false;                  // save_renders: 1 -> the PNG tree the reference's run.py leaves (main.cpp:1676-1684)
  bool save_members = false;                  // save_members: 1 -> <save_path>/members/<iteration>/member_<e>.prvf, the fields an iteration scored with
  bool dump_records = false;                  // dump_scores: 1, or PRV_PLANNER_DUMP_RECORDS in the environment: scores, records and gains of every iteration on disk
  int eval_views = 100;                       // evaluate_views: the test view set <viewspace_path>/<n>.txt (100 as in main.cpp:1956)
  // views_per_iteration > 1 (read only then)
  int select_grid_res = 0;        // select_grid_res / select_alpha_min (0 / negative: prv_select_default_opts')
  float select_alpha_min = -1.f;
  bool select_surface = false;    // select_locator: surface -- prv_select_views_surface at select_level (read and policed by Share_Data)
  float select_level = 0.5f;
  GeometryEvalConfig geom;        // evaluate_geometry and its keys (geometry_eval.hpp)
  CoverageEvalConfig cover;       // evaluate_coverage and its keys (coverage_eval.hpp)

  void apply_train_opts(prv_train_opts& to) const {
    if (train_deterministic) to.deterministic = 1;
    if (train_step_mode == PRV_STEP_FIXED_S) {
      to.step_mode = PRV_STEP_FIXED_S;
      to.n_samples = 128;
    } else if (train_step_mode == PRV_STEP_NGP) {
      to.step_mode = PRV_STEP_NGP;
      to.n_samples = PRV_NGP_MAX_STEPS;
    }
    if (train_rays > 0) to.n_rays = train_rays;
    if (train_patch_w > 0) to.patch_w = train_patch_w;
    if (train_patch_h > 0) to.patch_h = train_patch_h;
    if (std::max(to.patch_w, 1) * std::max(to.patch_h, 1) > 1 && train_step_mode < 0) { // pixel patches are an option of the fixed rule
      to.step_mode = PRV_STEP_FIXED_S;
      to.n_samples = 128;
    }
  }
};

inline EngineConfig engine_config(const FileStorage& fs, const Share_Data& sd, int method) {
  EngineConfig c;
  auto num = [&](const char* k, double dflt) { return fs.has(k) ? fs.num(k) : dflt; };
  auto on = [&](const char* k) { return fs.has(k) && fs.num(k) > 0; };
  c.n_members = (method == EnsembleRGB || method == EnsembleRGBDensity || method == EnsembleTermination) ? sd.ensemble_num : 1;
  c.field.n_levels = (int)num("field_levels", 8);
  c.field.n_features = (int)num("field_features", 4);
  c.field.log2_hashmap = (int)num("field_log2_hashmap", 19);
  c.field.base_res = (int)num("field_base_res", 16);
  c.field.finest_res = (int)num("field_finest_res", 256);
  c.field.occ_res = (int)num("field_occ_res", 128);
  c.field.density_bias = (float)num("field_density_bias", 3.0);
  c.field.table_amp = (float)num("synthetic_table_amp", 4.0);
  c.field.per_level_scale = (float)num("field_per_level_scale", 0.0); // > 0: tiny-cuda-nn's level recipe (include/prv.h)
  c.object_size = num("object_size", 0.1);
  c.synthetic = fs.has("synthetic_seed");
  if (c.synthetic) c.synthetic_seed = (uint64_t)fs.num("synthetic_seed");
  if (fs.has("ground_truth_seed")) c.ground_truth_seed = (uint64_t)fs.num("ground_truth_seed");
  c.train_steps = configured_train_steps(fs, sd);
  if (c.train_steps > 0) {
    c.train_rays = (int)num("train_rays", 0);
    c.train_patch_w = (int)num("train_patch_w", 0);
    c.train_patch_h = (int)num("train_patch_h", 0);
    c.train_step_mode = (int)num("train_step_mode", -1); // how a training ray is sampled (include/prv.h: prv_train_opts.step_mode)
    c.train_w = (int)num("train_width", 0);
    c.train_h = (int)num("train_height", 0);
    c.train_desc = c.field;
    c.train_desc.density_bias = (float)num("train_density_bias", 0.0);
    c.train_desc.table_amp = 1e-4f;
    if (fs.has("train_seed")) c.train_seed = (uint64_t)fs.num("train_seed");
    c.train_deterministic = on("train_deterministic");
    c.images_from_files = fs.has("train_images") && fs.str("train_images") == "files";
  }
  c.coverage_images = on("coverage_images");
  c.save_renders = on("save_renders");
  c.save_members = on("save_members");
  c.dump_records = on("dump_scores") || getenv("PRV_PLANNER_DUMP_RECORDS") != nullptr;
  c.eval_views = (int)num("evaluate_views", 100);
  if (sd.views_per_iteration > 1) {
    c.select_grid_res = (int)num("select_grid_res", 0);
    c.select_alpha_min = (float)num("select_alpha_min", -1.0);
    c.select_surface = sd.select_surface;
    c.select_level = (float)sd.select_level;
  }
  c.geom = geometry_eval_config(fs);
  c.cover = coverage_eval_config(fs);
  return c;
}

struct PlannerEngine {
  // ================================================================================ where and who
  // views-sharded job (`shard: views` / PRV_SHARD=views under RANK / WORLD_SIZE): every rank runs the same loop on the
  // same object; the members are trained by their owners and exchanged, the candidates of an iteration are dealt to the
  // ranks and ONE all-gather of the 16-byte records gives every rank every score.
  // Where the members live and who trains them.  Default (one object at a time): member e in model slot e, trained by rank
  // e % world.  `shard: members` walks several objects' loops in lockstep: object o's members sit in slots slot_base + e and
  // the (object, member) trainings of a round are dealt round-robin, member e to rank (pair_base + e) % world with
  // pair_base = o * n_members.
  prv_ctx* const ctx;
  prv_comm* const comm;
  const int rank, world;
  const int slot_base, pair_base;
  const std::shared_ptr<Share_Data> sd;
  const EngineConfig cfg;
  const int n_members;
  int slot_of(int e) const { return slot_base + e; }
  int owner_of(int e) const { return member_pair_owner(0, pair_base + e, 1 << 30, world); } // (pair_base = object * n_members: planner.hpp's rule)

  PlannerEngine(prv_ctx* ctx_, prv_comm* comm_, const std::shared_ptr<Share_Data>& sd_, const EngineConfig& cfg_, int slot_base_ = 0, int pair_base_ = 0)
      : ctx(ctx_), comm(comm_), rank(comm_ ? prv_comm_rank(comm_) : 0), world(comm_ ? prv_comm_world(comm_) : 1), slot_base(slot_base_),
        pair_base(pair_base_), sd(sd_), cfg(cfg_), n_members(cfg_.n_members) {}
  PlannerEngine(const PlannerEngine&) = delete;
  PlannerEngine& operator=(const PlannerEngine&) = delete;
  ~PlannerEngine() { // the caches of an object's life, in the order the shell has always released them
    data.drop();
    test.drop();
    cover.drop();
    geom_ref.drop();
    references.reset();
  }

  // the ground-truth field (slot 6): what the training images, the test images and the geometric reference are rendered from
  int load_ground_truth() { return prv_model_synthetic(ctx, 6, &cfg.field, cfg.ground_truth_seed); }

  // ================================================================================ training
  // load_training_data (run.py:109) of one scene json: dataset cameras + the RGBA8 training images on the device.  Kept
  // until another scene is asked for: the reference's per-member run.py calls of one iteration (main.cpp:2041-2043) all
  // name the same json, and every one of them would reload the same files.  Dropped at the end of train_members.
  struct TrainingData {
    std::string scene;
    CamsetPtr cams;
    DeviceArray<uint8_t> imgs;
    int w = 0, h = 0;
    void drop() {
      cams.reset();
      imgs.reset();
      scene.clear();
    }
  } data;

  int training_data(const std::string& scene_json) {
    if (data.cams && data.scene == scene_json) return PRV_OK;
    data.drop();
    DeviceArray<uint8_t> imgs;
    CamsetPtr ds;
    if (prv_cameras_from_dataset_json(ctx, scene_json.c_str(), out_arg(ds)) != PRV_OK) return -30;
    int w = 0, h = 0;
    prv_camset_size(ds.get(), &w, &h);
    prv_render_opts o{};
    o.width = cfg.train_w > 0 ? cfg.train_w : w; // training images at the dataset size unless the config shrinks them
    o.height = cfg.train_h > 0 ? cfg.train_h : h;
    // the ground truth is rendered with the rule every other render of this run uses (yaml samples_per_ray; 0 = the
    // engine's own stepping): the PSNR evaluation compares like with like
    o.samples_per_ray = sd->samples_per_ray;
    o.step_mode = sd->samples_per_ray > 0 ? PRV_STEP_FIXED_S : PRV_STEP_NGP;
    o.spp = 1;
    o.min_transmittance = 1e-4f;
    const int n = prv_camset_count(ds.get());
    int rc = imgs.alloc(ctx, (size_t)n * o.width * o.height * 4);
    if (rc == PRV_OK && cfg.images_from_files) {
      // every frame's file_path, relative to the json, as RGBA8
      std::string text, err;
      prvjson::Value root;
      if (!prvjson::read_file(scene_json, text) || !prvjson::Parser(text).parse(root, err)) rc = -31;
      const std::string base = scene_json.substr(0, scene_json.find_last_of('/') + 1);
      std::vector<uint8_t> px;
      for (int i = 0; rc == PRV_OK && i < n; i++) {
        std::string fp = root.at("frames").arr[(size_t)i].at("file_path").s;
        if (fp.size() < 4 || fp.substr(fp.size() - 4) != ".png") fp += ".png";
        int iw = 0, ih = 0;
        const int prc = png_read_rgba8(base + fp, &iw, &ih, px);
        if (prc != 0 || iw != o.width || ih != o.height) {
          std::cerr << "training image " << base + fp << ": " << (prc ? "cannot read (" + std::to_string(prc) + ")" : "size differs from the json") << std::endl;
          rc = -32;
          break;
        }
        rc = prv_memcpy_h2d(ctx, imgs.get() + (size_t)i * o.width * o.height * 4, px.data(), px.size());
      }
    } else if (rc == PRV_OK) {
      rc = prv_render_rgba8(ctx, 6, ds.get(), nullptr, n, &o, imgs.get(), nullptr); // straight alpha over nothing
    }
    if (rc != PRV_OK) {
      std::cerr << "prv: " << prv_last_error(ctx) << std::endl;
      return rc;
    }
    data.scene = scene_json;
    data.cams = std::move(ds);
    data.imgs = std::move(imgs);
    data.w = o.width;
    data.h = o.height;
    return PRV_OK;
  }

  // trainers of the listed members on one scene json, for the members this rank owns: a fresh field per member
  // (seed = train_seed + e) in the member's slot; appended to `trs` (the caller steps them and decides when they go)
  int create_trainers(const std::string& scene_json, const std::vector<int>& members, std::vector<TrainerPtr>& trs, double* t_fresh = nullptr,
                      double* t_create = nullptr) {
    int rc = training_data(scene_json);
    for (size_t k = 0; rc == PRV_OK && k < members.size(); k++) {
      const int e = members[k];
      if (owner_of(e) != rank) continue;
      double t0 = now_seconds();
      rc = prv_model_fresh(ctx, slot_of(e), &cfg.train_desc, cfg.train_seed + (uint64_t)e);
      if (t_fresh) *t_fresh += now_seconds() - t0;
      prv_train_opts to;
      prv_train_default_opts(&to);
      cfg.apply_train_opts(to);
      to.seed += (uint64_t)e;
      TrainerPtr tr;
      t0 = now_seconds();
      if (rc == PRV_OK) rc = prv_train_create(ctx, slot_of(e), data.cams.get(), data.imgs.get(), data.w, data.h, &to, out_arg(tr));
      if (t_create) *t_create += now_seconds() - t0;
      if (tr) trs.push_back(std::move(tr));
    }
    if (rc != PRV_OK) std::cerr << "prv: " << prv_last_error(ctx) << std::endl;
    return rc;
  }

  // `--train --n_steps N` for the listed members on one scene json, the members stepping side by side (prv_train_steps_multi);
  // with several ranks a member is trained by its owner (owner_of)
  int train_member_list(const std::string& scene_json, const std::vector<int>& members, int steps) {
    const bool timing = getenv("PRV_PLANNER_TIMING") != nullptr; // dev: where an iteration's seconds go
    const double t_start = now_seconds();
    double t_fresh = 0, t_create = 0;
    int rc = training_data(scene_json);
    if (rc != PRV_OK) return rc;
    if (timing) prv_synchronize(ctx);
    const double t_gt = now_seconds() - t_start;
    std::vector<TrainerPtr> trs;
    rc = create_trainers(scene_json, members, trs, &t_fresh, &t_create);
    std::vector<prv_trainer*> raw = raw_trainers(trs);
    const double t0 = now_seconds();
    if (rc == PRV_OK && !raw.empty()) rc = prv_train_steps_multi(raw.data(), (int)raw.size(), steps, nullptr);
    const double t_steps = now_seconds() - t0;
    uint64_t samples_last = 0;
    int active_rays = 0;
    if (timing && !raw.empty()) {
      (void)prv_train_info(raw[0], nullptr, &samples_last, nullptr);
      active_rays = prv_train_active_rays(raw[0]);
    }
    trs.clear(); // order is behaviour: the trainers are destroyed before the timing line is printed, and before the exchange
    if (timing) // (third finding: members[0] need not be the member raw[0] belongs to on ranks > 0)
      std::cerr << "train_members: views " << prv_camset_count(data.cams.get()) << " gt " << t_gt << " s, fresh " << t_fresh << " s, create "
                << t_create << " s, steps " << t_steps << " s, total " << now_seconds() - t_start << " s; last batch of member " << (raw.empty() ? -1 : members[0])
                << ": " << samples_last << " samples, " << active_rays << " rays" << std::endl;
    if (rc != PRV_OK) std::cerr << "prv: " << prv_last_error(ctx) << std::endl;
    return rc;
  }

  // the first n members of the ensemble reach every rank (each trained by its owner): one group of broadcasts
  int exchange_members(int n) {
    if (!comm) return PRV_OK;
    std::vector<int> slots(n), owners(n);
    for (int e = 0; e < n; e++) {
      slots[e] = slot_of(e);
      owners[e] = owner_of(e);
    }
    const int rc = prv_model_exchange_slots(ctx, comm, n, slots.data(), owners.data(), &cfg.train_desc);
    if (rc != PRV_OK) std::cerr << "prv: " << prv_last_error(ctx) << std::endl;
    return rc;
  }

  // `shard: members`: the shell's lockstep round has trained this object's members already.  Set by run_members_lockstep
  // before the round's scoring step and by nobody else; the next train_members call takes it (reads and clears it).
  bool members_pretrained = false;

  // members 0 .. n-1 of an iteration in one go (the fused path): train, then exchange between ranks
  int train_members(const std::string& scene_json, int n) {
    std::vector<int> all(n);
    for (int e = 0; e < n; e++) all[e] = e;
    int rc = members_pretrained ? PRV_OK : train_member_list(scene_json, all, cfg.train_steps); // (pretrained: this call only brings them together)
    members_pretrained = false;
    if (rc == PRV_OK) rc = exchange_members(n);
    data.drop(); // the next iteration's json differs
    return rc;
  }

  // the members an iteration scores (or selects) with: trained on the scene json's views, saved when the yaml asks
  int prepare_members(int iteration, const std::string& scene_json) {
    if (cfg.train_steps > 0) {
      const int trc = train_members(scene_json, n_members);
      if (trc != PRV_OK) return trc;
    }
    if (cfg.save_members) {
      const std::string dir = sd->save_path + "/members/" + std::to_string(iteration);
      sd->access_directory(dir);
      for (int e = 0; e < n_members; e++)
        if (prv_model_save_file(ctx, slot_of(e), (dir + "/member_" + std::to_string(e) + ".prvf").c_str()) != PRV_OK) {
          std::cerr << "prv: " << prv_last_error(ctx) << std::endl;
          return -26;
        }
    }
    return PRV_OK;
  }

  // Mode 4's curve points trained SIDE BY SIDE: one fresh field per scene json on model slots 0, 1, ... (at most 5: slots
  // 6 and 7 hold the ground truth and the reference field), each on its own dataset, all stepped together by
  // prv_train_steps_multi -- the reference trains them one run.py after another (main.cpp:2469-2479); the fields are the
  // same fields either way (own slot, own seed, own data), the GPU is just not left idle between a single trainer's kernels.
  int train_scenes_side_by_side(const std::vector<std::string>& scenes) {
    struct Job { // (a job goes as it always has: trainer, cameras, images)
      DeviceArray<uint8_t> imgs;
      CamsetPtr cams;
      TrainerPtr tr;
    };
    std::vector<Job> jobs(scenes.size());
    int rc = PRV_OK;
    for (size_t k = 0; rc == PRV_OK && k < scenes.size(); k++) {
      data.drop();
      if ((rc = training_data(scenes[k])) != PRV_OK) break;
      jobs[k].cams = std::move(data.cams); // the job owns them from here
      jobs[k].imgs = std::move(data.imgs);
      data.scene.clear();
      rc = prv_model_fresh(ctx, (int)k, &cfg.train_desc, cfg.train_seed); // every curve point starts from the same initial field, as `evaluate` does
      prv_train_opts to;
      prv_train_default_opts(&to);
      cfg.apply_train_opts(to);
      if (rc == PRV_OK) rc = prv_train_create(ctx, (int)k, jobs[k].cams.get(), jobs[k].imgs.get(), data.w, data.h, &to, out_arg(jobs[k].tr));
    }
    std::vector<prv_trainer*> trs;
    for (auto& j : jobs)
      if (j.tr) trs.push_back(j.tr.get());
    if (rc == PRV_OK && !trs.empty()) rc = prv_train_steps_multi(trs.data(), (int)trs.size(), cfg.train_steps, nullptr);
    if (rc != PRV_OK) std::cerr << "prv: " << prv_last_error(ctx) << std::endl;
    return rc;
  }

  // ================================================================================ evaluation
  // the reference images of the test set are rendered once per test json and size and kept for the object's life: mode 4
  // evaluates a dozen fields on them
  struct TestImages {
    DeviceArray<float> gt;
    std::string key;
    void drop() {
      gt.reset();
      key.clear();
    }
  } test;

  // `evaluate: 1`: train ONE field on the final view set and score it on the test view set
  // (<viewspace_path>/<evaluate_views>.txt, default 100 as in main.cpp:1956) against renders of the ground truth
  int evaluate(const std::string& scene_json, const Vec3& center, double size, double* psnr, double* ssim) {
    int rc = cfg.train_steps > 0 ? train_members(scene_json, 1) : PRV_OK; // without training: member 0 as loaded
    if (rc != PRV_OK) return rc;
    std::string test_json;
    if ((rc = write_test_json(center, size, &test_json)) != PRV_OK) return rc;
    return evaluate_on(test_json, slot_of(0), psnr, ssim);
  }

  // the test cameras' json, <gt_path>/<evaluate_views>.json: the test view set placed like the candidates, full-size
  // dataset header (what get_coverage leaves for the reference's "100" test set, main.cpp:1581-1651)
  int write_test_json(const Vec3& center, double size, std::string* path) {
    auto sd_test = std::make_shared<Share_Data>(sd->yaml_file_path, sd->name_of_pcd, cfg.eval_views, -1, sd->method_of_IG);
    if (!sd_test->ok) {
      std::cerr << sd_test->error << std::endl;
      return -40;
    }
    View_Space vs(sd_test);
    vs.set_view_space(center, size);
    Value root = transforms_header(sd->color_intrinsics, sd->ray_casting_aabb_scale, size, center, 0);
    for (size_t i = 0; i < vs.views.size(); i++) {
      Value v;
      v["file_path"] = Value(std::to_string(cfg.eval_views) + "/rgbaClip_" + std::to_string(i) + ".png");
      v["transform_matrix"] = matrix_json(view_transform_matrix(vs.views[i], Mat4::Identity(), center));
      root["frames"].append(v);
    }
    *path = sd->gt_path + "/" + std::to_string(cfg.eval_views) + ".json";
    sd->access_directory(sd->gt_path);
    return write_text(*path, prvjson::to_styled_string(root)) ? PRV_OK : PRV_E_IO;
  }

  // run.py:226-277 for one model slot: every frame of the test json (full-size dataset cameras, lens included) at
  // spp 1 / min_T 1e-4 over opaque black, against renders of the ground-truth field (slot 6) -> mean PSNR, mean SSIM
  int evaluate_on(const std::string& test_json, int slot, double* psnr, double* ssim) {
    CamsetPtr cams;
    if (prv_cameras_from_dataset_json(ctx, test_json.c_str(), out_arg(cams)) != PRV_OK) {
      std::cerr << "prv: " << prv_last_error(ctx) << std::endl;
      return -41;
    }
    int w = 0, h = 0;
    prv_camset_size(cams.get(), &w, &h);
    prv_render_opts o{};
    o.width = cfg.train_w > 0 ? cfg.train_w : w;
    o.height = cfg.train_h > 0 ? cfg.train_h : h;
    o.samples_per_ray = sd->samples_per_ray;
    o.step_mode = sd->samples_per_ray > 0 ? PRV_STEP_FIXED_S : PRV_STEP_NGP;
    o.spp = 1; // snap_to_pixel_centers (run.py:231)
    o.min_transmittance = 1e-4f; // run.py:235
    o.background[3] = 1.f;       // black, opaque (run.py:226)
    const int n = prv_camset_count(cams.get());
    int rc = PRV_OK;
    const std::string key = test_json + "@" + std::to_string(o.width) + "x" + std::to_string(o.height);
    if (!test.gt || test.key != key) {
      test.drop();
      rc = test.gt.alloc(ctx, (size_t)n * o.width * o.height * 16);
      prv_render_opts og = o;
      og.background[3] = 0.f;
      if (rc == PRV_OK) rc = prv_render(ctx, 6, cams.get(), nullptr, n, &og, test.gt.get(), nullptr);
      if (rc == PRV_OK) test.key = key;
      else test.drop();
    }
    if (rc == PRV_OK) rc = prv_evaluate(ctx, slot, cams.get(), nullptr, n, &o, test.gt.get(), psnr, ssim);
    if (rc != PRV_OK) std::cerr << "prv: " << prv_last_error(ctx) << std::endl;
    return rc;
  }

  // ================================================================================ geometry
  // `evaluate_geometry: 1` (geometry_eval.hpp): beside every metrics/<it>.txt the loop writes, member 0's marching-cubes mesh is
  // sampled and compared with a reference surface -- a .pcd cloud (`geometry_reference`, read here and nowhere else) or samples of
  // the ground-truth field's mesh (slot 6), made once per object and kept for its life -- and metrics/<it>_geometry.txt gets
  // prv_geom_metrics in dataset units.  The reference's index is built once: every iteration compares against the same points.
  struct GeometryReference {
    DeviceArray<float> points;
    uint64_t n = 0;
    NnIndexPtr index;
    MeshPtr mesh; // the ground-truth mesh, kept from geometry_setup to coverage_setup when `coverage_occluder: mesh` asks for it
    double scale = 1.0, size = 0.1; // engine units per dataset unit (the json's scale); the object size
    void drop() {
      mesh.reset();
      index.reset();
      points.reset();
      n = 0;
    }
  } geom_ref;

  prv_mesh_opts geometry_mesh_opts() const {
    prv_mesh_opts mo;
    prv_mesh_default_opts(&mo);
    for (int a = 0; a < 3; a++) mo.res[a] = cfg.geom.mc_res;
    mo.colors = 0;
    return mo;
  }

  // the reference surface in the engine frame + its index; every failure is a message and an error BEFORE any training
  int geometry_setup(const Vec3& center, double size) {
    GeometryEvalConfig checked = cfg.geom; // (evaluate_coverage alone uses the same reference: the same keys are policed)
    checked.on = true;
    const std::string problem = geometry_eval_problem(checked);
    if (!problem.empty()) {
      std::cerr << "evaluate_geometry: " << problem << std::endl;
      return -80;
    }
    geom_ref.drop();
    geom_ref.size = size;
    geom_ref.scale = 0.5 / size; // the json's scale and offset (transforms_header; prv_splat_points takes the same pair)
    const double offset[3] = {0.5 + center.z, 0.5 + center.x, 0.5 + center.y};
    int rc = PRV_OK;
    if (!cfg.geom.reference.empty()) {
      std::vector<float> xyz;
      std::vector<uint8_t> rgb;
      const int prc = pcd_read(cfg.geom.reference, xyz, rgb);
      if (prc != 0 || xyz.size() < 3) {
        std::cerr << "evaluate_geometry: cannot read a cloud from geometry_reference " << cfg.geom.reference << " (" << prc << "); nothing was trained" << std::endl;
        return -81;
      }
      geometry_to_engine(xyz, geom_ref.scale, offset);
      geom_ref.n = xyz.size() / 3;
      rc = geom_ref.points.alloc(ctx, xyz.size() * 4);
      if (rc == PRV_OK) rc = prv_memcpy_h2d(ctx, geom_ref.points.get(), xyz.data(), xyz.size() * 4);
    } else {
      prv_field_desc d;
      if (prv_model_desc(ctx, 6, &d) != PRV_OK) {
        std::cerr << "evaluate_geometry: no usable reference -- no geometry_reference cloud is named and there is no ground-truth field in "
                     "slot 6 (train_steps or evaluate puts one there); nothing was trained" << std::endl;
        return -82;
      }
      const prv_mesh_opts mo = geometry_mesh_opts();
      MeshPtr m;
      rc = prv_marching_cubes(ctx, 6, &mo, out_arg(m));
      uint64_t nt = 0;
      if (rc == PRV_OK) prv_mesh_counts(m.get(), nullptr, &nt);
      if (rc == PRV_OK && nt == 0) {
        std::cerr << "evaluate_geometry: no usable reference -- the ground-truth field has no surface at the iso-level; nothing was trained" << std::endl;
        return -83;
      }
      geom_ref.n = cfg.geom.samples;
      if (rc == PRV_OK) rc = geom_ref.points.alloc(ctx, geom_ref.n * 12);
      if (rc == PRV_OK) rc = prv_mesh_sample(m.get(), geom_ref.n, 1, geom_ref.points.get(), nullptr);
      if (rc == PRV_OK && cfg.cover.mesh_occluder()) geom_ref.mesh = std::move(m); // coverage_setup rasterises it, then lets it go
      m.reset(); // (before the index is built and any echo, as ever)
    }
    if (rc == PRV_OK && cfg.geom.on) rc = prv_nn_index_create(ctx, geom_ref.points.get(), geom_ref.n, nullptr, out_arg(geom_ref.index));
    if (rc != PRV_OK) {
      std::cerr << "evaluate_geometry: " << prv_last_error(ctx) << std::endl;
      geom_ref.drop();
    }
    return rc;
  }

  // the field in `slot` against the reference -> `path`.  A field without a surface yet is not an error: the file says n_rec 0.
  int geometry_evaluate(int slot, const std::string& path) {
    if (!cfg.geom.on || !geom_ref.index) return PRV_OK;
    const prv_mesh_opts mo = geometry_mesh_opts();
    MeshPtr m;
    int rc = prv_marching_cubes(ctx, slot, &mo, out_arg(m));
    uint64_t nt = 0;
    if (rc == PRV_OK) prv_mesh_counts(m.get(), nullptr, &nt);
    prv_geom_metrics gm{};
    gm.n_ref = geom_ref.n;
    DeviceArray<float> rec;
    if (rc == PRV_OK && nt > 0) {
      rc = rec.alloc(ctx, cfg.geom.samples * 12);
      if (rc == PRV_OK) rc = prv_mesh_sample(m.get(), cfg.geom.samples, 0, rec.get(), nullptr);
      if (rc == PRV_OK)
        rc = prv_geometry_metrics_indexed(ctx, rec.get(), cfg.geom.samples, geom_ref.index.get(), geom_ref.points.get(), geom_ref.n,
                                          (float)(cfg.geom.tau_for(geom_ref.size) * geom_ref.scale), &gm);
    } else if (rc == PRV_OK) {
      std::cerr << "evaluate_geometry: the field has no surface at the iso-level yet (" << path << ": n_rec 0)" << std::endl;
      gm.accuracy = gm.completeness = gm.accuracy_sq = gm.completeness_sq = gm.chamfer = gm.hausdorff_rec = gm.hausdorff_ref = NAN;
    }
    rec.reset();
    m.reset();
    if (rc != PRV_OK) {
      std::cerr << "evaluate_geometry: " << prv_last_error(ctx) << std::endl;
      return rc;
    }
    return write_text(path, geometry_metrics_text(gm, geom_ref.scale)) ? PRV_OK : PRV_E_IO;
  }

  // ================================================================================ coverage
  // `evaluate_coverage: 1` (coverage_eval.hpp): how much of the reference surface (geom_ref.points: geometry_setup runs first) the
  // views chosen so far see, and what the greedy choice of as many views of the whole view space would have seen.  The handle --
  // which point is visible from which view of the space -- is built once per object; an iteration costs one curve and one greedy
  // call on it.  Nothing here trains or renders a field.
  struct CoverageState {
    CoveragePtr handle;
    uint64_t n_points = 0, n_coverable = 0;
    int n_views = 0;
    void drop() { handle.reset(); }
  } cover;

  int coverage_setup(std::vector<View>& views, const Vec3& center, double size) {
    cover.drop();
    if (!geom_ref.points.get()) return PRV_E_STATE;
    const std::string all_json = sd->gt_path + "/" + std::to_string(sd->num_of_views) + "_coverage.json"; // every view of the space, candidate header
    Value root = transforms_header(sd->color_intrinsics, sd->ray_casting_aabb_scale, size, center, sd->candidate_divisor);
    for (size_t i = 0; i < views.size(); i++) {
      Value v;
      v["file_path"] = Value("rgbaClip_" + std::to_string(i) + ".png");
      v["transform_matrix"] = matrix_json(view_transform_matrix(views[i], Mat4::Identity(), center));
      root["frames"].append(v);
    }
    write_text(all_json, prvjson::to_styled_string(root));
    CamsetPtr cams;
    if (prv_cameras_from_json(ctx, all_json.c_str(), out_arg(cams)) != PRV_OK) {
      std::cerr << "evaluate_coverage: " << prv_last_error(ctx) << std::endl;
      return -84;
    }
    const prv_render_opts o = candidate_opts(cams.get()); // the candidates' size unless the config names one
    prv_coverage_opts co;
    prv_coverage_default_opts(&co);
    co.point_size = cfg.cover.point_size;
    co.depth_tol = (float)cfg.cover.depth_tol;
    const int n = prv_camset_count(cams.get());
    const int cw = cfg.cover.width > 0 ? cfg.cover.width : o.width, ch = cfg.cover.height > 0 ? cfg.cover.height : o.height;
    int rc;
    if (cfg.cover.mesh_occluder()) {
      if (!geom_ref.mesh) {
        std::cerr << "evaluate_coverage: coverage_occluder: mesh, and no ground-truth mesh was kept" << std::endl;
        return PRV_E_STATE;
      }
      rc = prv_coverage_create_occluded(ctx, geom_ref.points.get(), geom_ref.n, geom_ref.mesh.get(), cams.get(), nullptr, n, cw, ch, &co, nullptr,
                                        out_arg(cover.handle));
      geom_ref.mesh.reset(); // the handle keeps the bit matrix and nothing else
    } else {
      rc = prv_coverage_create(ctx, geom_ref.points.get(), geom_ref.n, cams.get(), nullptr, n, cw, ch, &co, nullptr, out_arg(cover.handle));
    }
    if (rc == PRV_OK) rc = prv_coverage_info(cover.handle.get(), &cover.n_points, &cover.n_views, &cover.n_coverable);
    if (rc != PRV_OK) {
      std::cerr << "evaluate_coverage: " << prv_last_error(ctx) << std::endl;
      cover.drop();
    }
    return rc;
  }

  // the views chosen so far (ids of the view space = positions in the handle) -> `path`; n_views in the file = how many they are
  int coverage_evaluate(const std::vector<int>& chosen, const std::string& path) {
    if (!cfg.cover.on || !cover.handle || chosen.empty()) return PRV_OK;
    const int k = (int)chosen.size();
    std::vector<uint64_t> covered((size_t)k), greedy((size_t)k);
    std::vector<int> picks((size_t)k);
    int rc = prv_coverage_curve(cover.handle.get(), chosen.data(), k, covered.data(), nullptr);
    if (rc == PRV_OK) rc = prv_coverage_greedy(cover.handle.get(), std::min(k, cover.n_views), picks.data(), greedy.data());
    if (rc != PRV_OK) {
      std::cerr << "evaluate_coverage: " << prv_last_error(ctx) << std::endl;
      return rc;
    }
    return write_text(path, coverage_text(cover.n_points, cover.n_coverable, k, covered.back(), greedy[(size_t)std::min(k, cover.n_views) - 1],
                                          cfg.cover.mesh_occluder())) ? PRV_OK : PRV_E_IO;
  }

  // ================================================================================ selection and scoring
  DeviceArray<float> references; // method 5: reference images of ALL views at the candidate size, kept for the object's life

  // the candidate renders' options: the render json's own w x h (run.py:304), screenshot_spp sub-samples, the engine's
  // stepping rule unless the yaml fixes a sample count, opaque black background (run.py:94)
  prv_render_opts candidate_opts(const prv_camset* cams) const {
    int w = 0, h = 0;
    prv_camset_size(cams, &w, &h);
    prv_render_opts o{};
    o.width = sd->render_width > 0 ? sd->render_width : w;
    o.height = sd->render_height > 0 ? sd->render_height : h;
    o.samples_per_ray = sd->samples_per_ray;
    o.step_mode = sd->samples_per_ray > 0 ? PRV_STEP_FIXED_S : PRV_STEP_NGP;
    o.spp = sd->screenshot_spp;
    o.min_transmittance = (float)sd->min_transmittance;
    o.background[0] = o.background[1] = o.background[2] = 0.f;
    o.background[3] = 1.f;
    return o;
  }

  // method 5 (PSNRCoverage): the reference field into slot 7 (synthetic_seed + 4096, or <model_path>/<object>/reference.prvf)
  // and its images of every view of the set, rendered once with the candidate header (divisor 16) so they match the render json
  int render_references(const std::string& object, std::vector<View>& views, const Vec3& center, double size) {
    int rc = cfg.synthetic ? prv_model_synthetic(ctx, 7, &cfg.field, cfg.synthetic_seed + 4096)
                           : prv_model_load_file(ctx, 7, (sd->model_path + object + "/reference.prvf").c_str());
    if (rc != PRV_OK) {
      std::cerr << "prv: " << prv_last_error(ctx) << std::endl;
      return rc;
    }
    const std::string all_json = sd->gt_path + "/" + std::to_string(sd->num_of_views) + "_render.json";
    Value root = transforms_header(sd->color_intrinsics, sd->ray_casting_aabb_scale, size, center, sd->candidate_divisor);
    for (size_t i = 0; i < views.size(); i++) {
      Value v;
      v["file_path"] = Value("rgbaClip_" + std::to_string(i) + ".png");
      v["transform_matrix"] = matrix_json(view_transform_matrix(views[i], Mat4::Identity(), center));
      root["frames"].append(v);
    }
    write_text(all_json, prvjson::to_styled_string(root));
    CamsetPtr cams;
    if (prv_cameras_from_json(ctx, all_json.c_str(), out_arg(cams)) != PRV_OK) return -22;
    prv_render_opts o = candidate_opts(cams.get());
    o.background[3] = 0.f; // straight alpha over nothing, as the scoring round renders the candidates it compares with them
    const int n = prv_camset_count(cams.get());
    if (references.alloc(ctx, (size_t)n * o.width * o.height * 16) != PRV_OK) return -23;
    rc = prv_render(ctx, 7, cams.get(), nullptr, n, &o, references.get(), nullptr);
    if (rc != PRV_OK) std::cerr << "prv: " << prv_last_error(ctx) << std::endl;
    return rc;
  }

  // views_per_iteration > 1 (planner.hpp: Selector): train the member, then prv_select_views on the candidates of the render
  // json -- the footprint render and the greedy rounds; chosen = k candidate ids in selection order
  int select(int iteration, const std::string& scene_json, const std::string& render_json, const std::vector<int>& ids, int k,
             std::vector<int>& chosen) {
    int rc = prepare_members(iteration, scene_json);
    if (rc != PRV_OK) return rc;
    CamsetPtr cams;
    if (prv_cameras_from_json(ctx, render_json.c_str(), out_arg(cams)) != PRV_OK) {
      std::cerr << "prv: " << prv_last_error(ctx) << std::endl;
      return -20;
    }
    const int n = prv_camset_count(cams.get());
    const prv_render_opts o = candidate_opts(cams.get());
    prv_select_opts so;
    prv_select_default_opts(&so);
    so.k = k;
    if (cfg.select_grid_res > 0) so.grid_res = cfg.select_grid_res;
    if (cfg.select_alpha_min >= 0.f) so.alpha_min = cfg.select_alpha_min;
    std::vector<int> frames((size_t)std::max(k, 1));
    std::vector<uint64_t> gains((size_t)std::max(k, 1));
    if (n != (int)ids.size()) rc = PRV_E_INVALID;
    else if (cfg.select_surface) rc = prv_select_views_surface(ctx, slot_of(0), cams.get(), nullptr, n, &o, cfg.select_level, &so, frames.data(), gains.data(), nullptr);
    else rc = prv_select_views(ctx, slot_of(0), cams.get(), nullptr, n, &o, &so, frames.data(), gains.data(), nullptr);
    cams.reset();
    if (rc != PRV_OK) {
      std::cerr << "prv: " << (n == (int)ids.size() ? prv_last_error(ctx) : "the render json does not hold the candidates") << std::endl;
      return rc;
    }
    chosen.clear();
    for (int j = 0; j < k; j++) chosen.push_back(ids[(size_t)frames[(size_t)j]]); // frame i of the render json is candidate ids[i]
    if (cfg.dump_records) { // the gains of the round, raw uint64, beside the other diagnostics
      sd->access_directory(sd->save_path + "/gains");
      write_text(sd->save_path + "/gains/" + std::to_string(iteration) + ".bin", std::string((const char*)gains.data(), (size_t)k * sizeof(uint64_t)));
    }
    return 0;
  }

  // the scoring callback of the loop (planner.hpp: Scorer): the members of the iteration, then every candidate of the render json
  int score(int method, int iteration, const std::string& scene_json, const std::string& render_json, const std::vector<int>& ids,
            std::vector<double>& scores) {
    {
      const int prc = prepare_members(iteration, scene_json);
      if (prc != PRV_OK) return prc;
    }
    const bool timing = getenv("PRV_PLANNER_TIMING") != nullptr; // dev: where an iteration's seconds go
    const double t_round = now_seconds();
    CamsetPtr cams;
    if (prv_cameras_from_json(ctx, render_json.c_str(), out_arg(cams)) != PRV_OK) {
      std::cerr << "prv: " << prv_last_error(ctx) << std::endl;
      return -20;
    }
    const double t_json = now_seconds() - t_round;
    const int n = prv_camset_count(cams.get());
    prv_render_opts o = candidate_opts(cams.get());
    std::vector<int> slots(n_members);
    for (int e = 0; e < n_members; e++) slots[e] = slot_of(e);
    std::vector<prv_score_record> rec(n);
    // this rank's shard of the frames of the render json (all of them with one rank): interleaved, as bench.py deals them
    std::vector<int> mine((size_t)std::max(1, (n + world - 1) / world));
    int n_mine = 0;
    prv_shard_views(n, rank, world, 1, mine.data(), &n_mine);
    int rc;
    if (method == PSNRCoverage) {
      // frame k of the render json is candidate ids[k]: pick its reference image out of the full set
      const size_t px = (size_t)o.width * o.height * 4;
      DeviceArray<float> gt_sel;
      if (gt_sel.alloc(ctx, (size_t)std::max(1, n_mine) * px * sizeof(float)) != PRV_OK) return -21;
      std::vector<float> tmp(px);
      for (int k = 0; k < n_mine; k++) { // device-to-device through the host keeps this file free of HIP headers
        prv_memcpy_d2h(ctx, tmp.data(), references.get() + (size_t)ids[mine[k]] * px, px * sizeof(float));
        prv_memcpy_h2d(ctx, gt_sel.get() + (size_t)k * px, tmp.data(), px * sizeof(float));
      }
      o.background[3] = 0.f;
      rc = prv_score_views_sharded(ctx, comm, PRV_SCORE_PSNR_COVERAGE, slots.data(), 1, cams.get(), n, 1, &o, gt_sel.get(), rec.data(), nullptr);
    } else { // the ensembles (EnsembleTermination = PRV_SCORE_TERMINATION_JSD among them), and RayEntropy (= PRV_SCORE_RAY_ENTROPY): one member, no reference images
      rc = prv_score_views_sharded(ctx, comm, method, slots.data(), n_members, cams.get(), n, 1, &o, nullptr, rec.data(), nullptr);
      if (rc == PRV_OK && cfg.save_renders) { // <save_path>/render/<it>/ensemble_<e>/rgbaClip_<view id>.png, the files :2047 reads
        DeviceArray<uint8_t> dev;
        std::vector<uint8_t> px((size_t)o.width * o.height * 4);
        rc = dev.alloc(ctx, (size_t)n * px.size());
        for (int e = 0; rc == PRV_OK && e < n_members; e++) {
          const std::string dir = sd->save_path + "/render/" + std::to_string(iteration) + "/ensemble_" + std::to_string(e);
          sd->access_directory(dir);
          rc = prv_render_rgba8(ctx, slot_of(e), cams.get(), nullptr, n, &o, dev.get(), nullptr);
          for (int k = 0; rc == PRV_OK && k < n; k++) {
            rc = prv_memcpy_d2h(ctx, px.data(), dev.get() + (size_t)k * px.size(), px.size());
            if (rc == PRV_OK && png_write_rgba8(dir + "/rgbaClip_" + std::to_string(ids[k]) + ".png", o.width, o.height, px.data()) != 0) rc = PRV_E_IO;
          }
        }
      }
    }
    cams.reset();
    if (rc != PRV_OK) {
      std::cerr << "prv: " << prv_last_error(ctx) << std::endl;
      return rc;
    }
    if (timing) std::cerr << "score_round: views " << n << " cameras " << t_json << " s, total " << now_seconds() - t_round << " s" << std::endl;
    for (int k = 0; k < n; k++) scores[k] = rec[k].score;
    if (cfg.dump_records) { // the gathered records of every iteration, byte for byte
      sd->access_directory(sd->save_path + "/records");
      write_text(sd->save_path + "/records/" + std::to_string(iteration) + ".bin",
                 std::string((const char*)rec.data(), rec.size() * sizeof(prv_score_record)));
    }
    return 0;
  }

  // The engine behind NBV_Net_Labeler::train_by_instantNGP's reference signature: ONE run.py invocation
  // (run.py:185-208 train, :226-277 evaluate, :284-309 screenshots) through include/prv.h, in process.
  //   --scene S --n_steps N                        train model slot max(ensemble_id, 0) on S (skipped when the run is
  //                                                configured with pretrained members: train_steps == 0)
  //   --screenshot_transforms J --screenshot_dir D  render every frame of J at its w x h, spp = screenshot_spp, opaque
  //                                                black background (run.py:94), write D/<basename(file_path)>
  //   --test_transforms T --save_metrics M          render every frame of T (spp 1, min_T 1e-4, run.py:231-235), PSNR /
  //                                                SSIM against renders of the ground-truth field, "PSNR\t..\nSSIM\t.." -> M
  int run_py(const RunPyArgs& a) {
    const int member = a.ensemble_id >= 0 ? a.ensemble_id : 0, slot = slot_of(member);
    if (cfg.train_steps > 0) { // (third finding: this path neither reads nor clears members_pretrained -- under `shard: members` it trains the member again)
      const int rc = train_member_list(a.scene, {member}, a.n_steps > 0 ? std::min(a.n_steps, cfg.train_steps) : cfg.train_steps);
      if (rc != PRV_OK) return rc;
    }
    if (!a.screenshot_transforms.empty()) {
      CamsetPtr cams;
      if (prv_cameras_from_json(ctx, a.screenshot_transforms.c_str(), out_arg(cams)) != PRV_OK) {
        std::cerr << "prv: " << prv_last_error(ctx) << std::endl;
        return -20;
      }
      std::string text, err;
      prvjson::Value root;
      if (!prvjson::read_file(a.screenshot_transforms, text) || !prvjson::Parser(text).parse(root, err)) {
        std::cerr << "prv: cannot read " << a.screenshot_transforms << (err.empty() ? "" : ": " + err) << std::endl;
        return -31;
      }
      const prv_render_opts o = candidate_opts(cams.get());
      const int n = prv_camset_count(cams.get());
      if (!root.has("frames") || (int)root.at("frames").arr.size() != n) { // the names below index the same array the cameras came from
        std::cerr << "prv: " << a.screenshot_transforms << ": " << n << " cameras but " << (root.has("frames") ? root.at("frames").arr.size() : 0) << " frames" << std::endl;
        return -32;
      }
      const size_t bytes = (size_t)o.width * o.height * 4;
      DeviceArray<uint8_t> dev;
      std::vector<uint8_t> px(bytes);
      int rc = dev.alloc(ctx, (size_t)std::max(1, n) * bytes);
      if (rc == PRV_OK) rc = prv_render_rgba8(ctx, slot, cams.get(), nullptr, n, &o, dev.get(), nullptr);
      if (rc != PRV_OK) std::cerr << "prv: " << prv_last_error(ctx) << std::endl;
      sd->access_directory(a.screenshot_dir);
      for (int k = 0; rc == PRV_OK && k < n; k++) {
        std::string name = root.at("frames").arr[(size_t)k].at("file_path").s; // os.path.basename(f["file_path"]) (run.py:297)
        name = name.substr(name.find_last_of('/') + 1);
        if (name.find('.') == std::string::npos) name += ".png";
        rc = prv_memcpy_d2h(ctx, px.data(), dev.get() + (size_t)k * bytes, bytes);
        if (rc != PRV_OK) std::cerr << "prv: " << prv_last_error(ctx) << std::endl;
        else if (png_write_rgba8(a.screenshot_dir + name, o.width, o.height, px.data()) != 0) {
          std::cerr << "prv: cannot write " << a.screenshot_dir + name << std::endl; // (not prv_last_error: the failure is the file's)
          rc = PRV_E_IO;
        }
      }
      return rc;
    }
    if (!a.test_transforms.empty()) {
      double psnr = 0, ssim = 0;
      const int rc = evaluate_on(a.test_transforms, slot, &psnr, &ssim);
      if (rc != PRV_OK) return rc;
      char buf[128];
      snprintf(buf, sizeof(buf), "PSNR\t%.17g\nSSIM\t%.17g", psnr, ssim); // run.py:275-277
      if (!write_text(a.save_metrics, buf)) return PRV_E_IO;
      std::string g = a.save_metrics; // <...>/<it>.txt -> <...>/<it>_geometry.txt
      if (g.size() >= 4 && g.substr(g.size() - 4) == ".txt") g.resize(g.size() - 4);
      return geometry_evaluate(slot, g + "_geometry.txt");
    }
    return 0;
  }
};

} // namespace prvhost
