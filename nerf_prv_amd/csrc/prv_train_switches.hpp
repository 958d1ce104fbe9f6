// prv_train_switches.hpp -- the trainer's PRV_TRAIN_* environment switches: experiments, A/B runs and the tests' fallback paths;
// none is needed for normal operation.  Read once, when a trainer is created (prv_train_create), and kept in it.  No HIP dependency.
#pragma once
#include <cstdlib>
#include <cstring>

namespace prv {

struct TrainSwitches {
  // on unless set to something atoi() reads as 0 ("0", "", "abc")
  bool use_graph = true;    // PRV_TRAIN_GRAPH: a step is one replay of a captured graph (0: plain launches)
  bool fast_forward = true; // PRV_TRAIN_FAST_FWD: forward logits through the f16-MFMA path of the render kernel (0: f32 tiles)
  bool reg_chain = true;    // PRV_TRAIN_REG_CHAIN: backward dX chain register-resident on bf16-split MFMAs (0: the LDS / f32-MFMA chain)
  bool keep_act = true;     // PRV_TRAIN_KEEP_ACT: the fast forward pass keeps its activations for the backward pass (0: recomputed)
  bool own_queue = true;    // PRV_TRAIN_OWN_QUEUE: the trainer's stream owns a hardware queue (0: a stream of the runtime's pool)
  bool tile_skip = true;    // PRV_TRAIN_TILE_SKIP: the backward pass skips the tiles behind the rays' terminations (0: walks all)
  bool list_ahead = true;   // PRV_TRAIN_LIST_AHEAD: the next step's ray batch rides on the table's Adam launch (0: every step lists its own)
  bool patch_ray_jitter = false; // PRV_TRAIN_PATCH_JITTER: on for the exact string "ray": every ray of a patch its own jitter (no oracle counterpart)
  int act_cap = 0;          // PRV_TRAIN_ACT_CAP: samples the kept-activation buffer covers, at least 32 (0 = unset: sized from the sample budget)
  int bwd_blocks = 0;       // PRV_TRAIN_BWD_BLOCKS: blocks of the backward launch, when positive (else 0: the trainer's own rule)
  int fwd_blocks = 0;       // PRV_TRAIN_FWD_BLOCKS: blocks of the fast forward launch, when positive (else 0: two per CU)
  bool timing = false;      // PRV_TRAIN_TIMING: set to anything: per-call timing lines on stderr
};

inline TrainSwitches train_switches_from_env() {
  const auto on = [](const char* name) { const char* e = getenv(name); return !e || atoi(e) != 0; };
  const auto positive = [](const char* name) { const char* e = getenv(name); return e && atoi(e) > 0 ? atoi(e) : 0; };
  TrainSwitches s;
  s.use_graph = on("PRV_TRAIN_GRAPH");
  s.fast_forward = on("PRV_TRAIN_FAST_FWD");
  s.reg_chain = on("PRV_TRAIN_REG_CHAIN");
  s.keep_act = on("PRV_TRAIN_KEEP_ACT");
  s.own_queue = on("PRV_TRAIN_OWN_QUEUE");
  s.tile_skip = on("PRV_TRAIN_TILE_SKIP");
  s.list_ahead = on("PRV_TRAIN_LIST_AHEAD");
  if (const char* e = getenv("PRV_TRAIN_PATCH_JITTER")) s.patch_ray_jitter = !strcmp(e, "ray");
  if (const char* e = getenv("PRV_TRAIN_ACT_CAP")) s.act_cap = atoi(e) > 32 ? atoi(e) : 32;
  s.bwd_blocks = positive("PRV_TRAIN_BWD_BLOCKS");
  s.fwd_blocks = positive("PRV_TRAIN_FWD_BLOCKS");
  s.timing = getenv("PRV_TRAIN_TIMING") != nullptr;
  return s;
}

} // namespace prv
