// prv_train_api.inc -- C ABI of the training step; compiled as part of prv_api.cpp (shares its context types)

struct prv_trainer : prv_handle {
  using prv_handle::prv_handle;
  ~prv_trainer() override { close(); }
  void close();             // the step graphs and the stream go
  void detach() override;   // the context goes first
  void retire() override;   // destroyed under a live context: the stream and the buffers are parked there
  int slot = 0;
  prv_field_desc desc{};
  uint64_t generation = 0; // the slot's parameter generation this trainer's masters were widened from
  prv_train_opts o{};
  int n_img = 0, W = 0, H = 0;
  const uint8_t* images = nullptr; // caller-owned device memory
  uint32_t step = 0;
  uint32_t n_active = 0; // host mirror of TrainState::n_active at the last synchronisation
  uint64_t samples_last = 0, n_table = 0;
  hipStream_t stream = nullptr; // own stream: several trainers (ensemble members) step concurrently
  bool own_queue = false;       // ... created with a CU mask: it owns a hardware queue, and is parked in the context when the trainer goes (prv_ctx::idle_queues)
  hipGraphExec_t step_graph[2] = {nullptr, nullptr}; // one optimiser step behind its ray batch, captured once per variant ([1]: it also lists the next step's batch), replayed every step
  bool rays_listed = false;             // the batch of the next step to run is there already (the previous step's Adam launch listed it)
  prv::TrainSwitches sw;     // the PRV_TRAIN_* environment, as it was when the trainer was created
  bool graph_failed = false; // a step graph could not be captured: plain launches for good
  prv::LevelCanon levels[kMaxLevels];
  uint32_t list_cap = 0; // samples the step's list holds (n_rays x n_samples; PRV_STEP_NGP: at most 2^24)
  uint32_t act_cap = 0;  // samples the kept-activation buffer covers (0: the backward pass recomputes the forward pass)
  bool side_by_side = false; // this call steps several trainers (prv_train_steps_multi): one backward block per CU (bwd_blocks)
  int graph_bwd_blocks[2] = {0, 0}; // the backward block count each captured step graph was recorded with
  // the device buffers: each is named here and once in buffer_table(), which is all that allocates, zeroes, parks and frees them
  Buffer cams, tab_wmv, tab_g, mlp_w, mlp_m, mlp_v, mlp_g, mlp_f, ema, rays, samples, logits, seeds,
      ray_loss, ray_used, scal, losses, dw_part, loss_part, frags, slot_of, frag_pos, tab_gq, block_tot, tile_live, act;
  struct BufferRow {
    Buffer prv_trainer::*buf;
    size_t bytes; // what this trainer needs when it is created (0: nothing)
    bool zeroed;  // starts at zero, all of it, whoever held the memory before
  };
  std::vector<BufferRow> buffer_table() const;
};

namespace {

// backward blocks per CU: what 74-80 KB of LDS per block allows
constexpr int kBwdBlocksPerCu = 2;
// Blocks of the backward launch.  A trainer stepping alone fills the chip (two 80 KB blocks per CU).  Several trainers side
// by side (the members of an ensemble, prv_train_steps_multi) launch ONE block per CU each: with two per CU a member's
// persistent blocks hold every CU's LDS until they exit and the next member's launch waits behind them -- the launches run one
// after another and the memory side's atomic unit idles through every head, chain and tail; with one per CU two members'
// launches share the CUs and one's table adds meet the other's tile work (measured, the planner loop's batch: round of five
// 0.570 -> 0.531 ms, of two 0.246 -> 0.233; one trainer alone 0.166 -> 0.181, hence the rule).  PRV_TRAIN_BWD_BLOCKS (dev) overrides.
static int bwd_blocks(const prv_trainer* t) {
  const int full = t->ctx->n_cu * kBwdBlocksPerCu;
  if (t->sw.bwd_blocks > 0) return std::min(t->sw.bwd_blocks, full);
  return t->side_by_side ? t->ctx->n_cu : full;
}

int train_check(prv_trainer* t) {
  if (!t || !t->ctx) return PRV_E_INVALID; // also: a trainer whose context has been destroyed
  prv_ctx* c = t->ctx;
  int rc = model_present(c, t->slot); // not check_model: a trainer works on the canonical arrays, never needs a republish
  if (rc != PRV_OK) return rc;
  if (memcmp(&c->models[t->slot].desc, &t->desc, sizeof(prv_field_desc)) != 0)
    return fail(c, PRV_E_STATE, "model slot %d was replaced by a different field since the trainer was created", t->slot);
  // same shape, new parameters (prv_model_fresh / load / load_file on the slot): the trainer's fp32 masters, moments,
  // density EMA and captured graph belong to the OLD model and would silently overwrite the new one
  if (c->models[t->slot].generation != t->generation)
    return fail(c, PRV_E_STATE, "model slot %d was re-installed since the trainer was created: destroy the trainer and create a new one", t->slot);
  return PRV_OK;
}

// the trainer's scalars on the device: a device pointer, only ever used to take a field's address
static prv::TrainScal* train_scal(const prv_trainer* t) { return (prv::TrainScal*)t->scal.p; }

// the ray batch of the step in flight (next = false) or of the one after it (true: launched beside the table's Adam pass)
prv::TrainRaysParams train_rays_params(prv_trainer* t, bool next) {
  Model& m = t->ctx->models[t->slot];
  prv::TrainRaysParams rp{};
  rp.cams = (const CamDev*)t->cams.p;
  rp.images = t->images;
  rp.occ = (const uint32_t*)m.occ.p;
  rp.n_img = t->n_img;
  rp.W = t->W;
  rp.H = t->H;
  rp.S = t->o.n_samples;
  rp.n_rays = t->o.n_rays;
  rp.occ_res = t->desc.occ_res;
  rp.random_bg = t->o.random_bg;
  rp.state = &train_scal(t)->state;
  rp.seed = t->o.seed;
  rp.rays = (prv::TrainRay*)t->rays.p;
  rp.samples = (uint2*)t->samples.p;
  rp.sample_count = train_scal(t)->sample_count;
  rp.next = next ? 1 : 0;
  rp.target_samples = t->o.target_samples;
  rp.loss_part = (const double*)t->loss_part.p;
  const bool patches = t->o.patch_w * t->o.patch_h > 1;
  rp.patch_w = patches ? t->o.patch_w : 1;
  rp.patch_h = patches ? t->o.patch_h : 1;
  rp.slot_of = patches ? (uint32_t*)t->slot_of.p : nullptr;
  rp.patch_ray_jitter = t->sw.patch_ray_jitter ? 1 : 0;
  rp.step_mode = t->o.step_mode;
  rp.sample_cap = t->list_cap;
  rp.block_tot = t->o.deterministic ? (uint32_t*)t->block_tot.p : nullptr;
  return rp;
}

// Opens the step in flight: its ray batch.  The step's scalars are set by the previous step's last kernel (or by
// train_begin_call); the plain path has a kernel of its own for that, which also clears the step's counter: it runs before the rays.
int train_open_step(prv_trainer* t) {
  prv::TrainScal* const sc = train_scal(t);
  if (!t->sw.fast_forward) HIPCHK(t->ctx, prv::launch_train_begin(&sc->state, sc->sample_count, t->o.lr, t->o.beta1, t->o.beta2, t->stream));
  HIPCHK(t->ctx, prv::launch_train_rays(train_rays_params(t, false), t->stream));
  return PRV_OK;
}

// forward -> compositing (+ loss) -> backward of the step in flight, whose ray batch is there (train_open_step, or the previous
// step's Adam launch listed it)
int train_forward_backward(prv_trainer* t, prv::DwReduce reduce, int* dw_slots_out) {
  prv_ctx* c = t->ctx;
  Model& m = c->models[t->slot];
  prv::TrainScal* const sc = train_scal(t);
  const prv::TrainRaysParams rp = train_rays_params(t, false);
  prv::TrainTileParams tp{};
  tp.table = (const uint16_t*)m.table.p;
  tp.mlp = (const float*)t->mlp_f.p;
  memcpy(tp.levels, t->levels, sizeof(tp.levels));
  tp.n_levels = t->desc.n_levels;
  tp.n_features = t->desc.n_features;
  tp.rays = rp.rays;
  tp.samples = rp.samples;
  tp.sample_count = sc->sample_count;
  tp.state = &sc->state;
  tp.logits = (float4*)t->logits.p;
  tp.seeds = (const float4*)t->seeds.p;
  tp.table_grad = (float*)t->tab_g.p;
  tp.mlp_grad = (float*)t->mlp_g.p;
  tp.mlp_grad_partial = (float*)t->dw_part.p;
  tp.stamps = sc->stamps; // dev only
  tp.act = t->sw.fast_forward && t->act_cap ? (uint4*)t->act.p : nullptr;
  tp.bwd_frags = tp.act && t->sw.reg_chain ? (const uint4*)((const uint16_t*)t->frags.p + (size_t)kNumFrags * kFragHalfs) : nullptr;
  tp.act_cap = t->act_cap;
  tp.sample_cap = t->list_cap;
  tp.table_grad_q = t->o.deterministic ? (long long*)t->tab_gq.p : nullptr;
  tp.tile_live = t->sw.tile_skip ? (uint8_t*)t->tile_live.p : nullptr;
  tp.scatter_ways = t->o.patch_w * t->o.patch_h > 1 ? 4 : 1;
  // two blocks per CU (eight waves: a batch of 33 K samples is 1,040 wave-rounds): four per CU staged the 24 KB of fragments twice as often
  // for nothing -- round of five 0.4990 -> 0.4968 / 0.4970 -> 0.4914 ms on two boxes, of four 0.3746 -> 0.3658, one trainer and the 2^16-ray batch unchanged
  if (t->sw.fast_forward) HIPCHK(c, prv::launch_train_forward_fast(tp, (const half8*)t->frags.p, t->sw.fwd_blocks > 0 ? t->sw.fwd_blocks : c->n_cu * 2, t->stream));
  else HIPCHK(c, prv::launch_train_forward(tp, c->n_cu * 4, t->stream));
  prv::TrainCompositeParams cp{};
  cp.rays = rp.rays;
  cp.state = &sc->state;
  cp.n_rays = t->o.n_rays;
  cp.logits = tp.logits;
  cp.seeds = (float4*)t->seeds.p;
  cp.density_bias = t->desc.density_bias;
  cp.min_T = t->o.min_T;
  cp.ray_loss = (float*)t->ray_loss.p;
  cp.ray_used = (uint32_t*)t->ray_used.p;
  cp.slot_of = rp.slot_of;
  cp.S = t->o.n_samples;
  cp.tile_live = tp.tile_live;
  HIPCHK(c, prv::launch_train_composite(cp, t->stream));
  // the loss of the batch and its used-sample count: summed by one block of the backward launch (train_tile_kernel)
  tp.ray_loss = cp.ray_loss;
  tp.ray_used = cp.ray_used;
  tp.n_rays = t->o.n_rays;
  tp.loss_part = (double*)t->loss_part.p; // its slices are added up by the step's last kernel (end_step) or launch_train_loss_finish
  HIPCHK(c, prv::launch_train_backward(tp, bwd_blocks(t), reduce, dw_slots_out, t->stream));
  return PRV_OK;
}

int train_density_refresh(prv_trainer* t) {
  prv_ctx* c = t->ctx;
  Model& m = c->models[t->slot];
  prv::DensityParams dp{};
  dp.table = (const uint16_t*)m.table.p;
  dp.mlp = (const float*)t->mlp_f.p;
  memcpy(dp.levels, t->levels, sizeof(dp.levels));
  dp.occ_res = t->desc.occ_res;
  dp.density_bias = t->desc.density_bias;
  dp.decay = t->o.occ_decay;
  dp.thresh = t->o.occ_sigma_thresh;
  dp.ema = (float*)t->ema.p;
  dp.occ = (uint32_t*)m.occ.p;
  // (eight persistent blocks per CU; 2, 4, 16 and 64 per CU measured the same in the round of five)
  if (t->sw.fast_forward) HIPCHK(c, prv::launch_density_refresh_fast(dp, t->desc.n_features, (const half8*)t->frags.p, c->n_cu * 8, t->stream));
  else HIPCHK(c, prv::launch_density_refresh(dp, t->desc.n_features, t->stream));
  return PRV_OK;
}

// the slot's derived render state is stale now; check_model rebuilds it when somebody renders from the slot
int train_publish(prv_trainer* t) {
  t->ctx->models[t->slot].dirty = true;
  return PRV_OK;
}

// May the next step's ray batch be listed beside this step's Adam pass?  Single-pixel batches on the fast path only (the
// patch kernel has another block size; the plain path opens a step with a kernel of its own), and never a deterministic
// trainer's: its batch is three launches of its own (prv::launch_train_rays), so the shared launch orders nothing.
static bool can_list_ahead(const prv_trainer* t) {
  return t->sw.list_ahead && t->sw.fast_forward && t->o.patch_w * t->o.patch_h <= 1 && !t->o.deterministic;
}

static bool use_graph(const prv_trainer* t) { return t->sw.use_graph && !t->graph_failed; }

// The launches of one optimiser step behind its ray batch (everything that varies per step is read from TrainState on the
// device): forward, compositing, backward (+ loss slices), the table's Adam pass (+ the dW reduction's first stage,
// + list_next: the NEXT step's ray batch), the MLP's Adam pass, fragments + end of step.
int train_step_launches(prv_trainer* t, bool list_next) {
  prv_ctx* c = t->ctx;
  Model& m = c->models[t->slot];
  int rc;
  int dw_slots = 0; // the backward launch's written dW slots: their first reduction stage rides on the table's Adam launch
  if ((rc = train_forward_backward(t, prv::DwReduce::AdamPasses, &dw_slots)) != PRV_OK) return rc;
  prv::TrainScal* const sc = train_scal(t);
  prv::AdamParams ap;
  ap.state = &sc->state;
  ap.beta1 = t->o.beta1;
  ap.beta2 = t->o.beta2;
  ap.eps = t->o.eps;
  ap.used = &sc->used;
  ap.loss_part = (const double*)t->loss_part.p;
  ap.target_samples = t->o.target_samples;
  ap.n_rays = t->o.n_rays;
  const prv::TrainRaysParams next = train_rays_params(t, true);
  float* const dw_stage = prv::train_dw_stage((float*)t->dw_part.p, bwd_blocks(t));
  prv::AdamTableArgs at{};
  at.n = t->n_table;
  at.grad = (float*)t->tab_g.p;
  at.wmv = (float*)t->tab_wmv.p;
  at.w16 = (uint16_t*)m.table.p;
  at.dw_partial = (const float*)t->dw_part.p;
  at.dw_slots = dw_slots;
  at.dw_stage = dw_stage;
  at.next_rays = list_next ? &next : nullptr;
  at.grad_q = t->o.deterministic ? (long long*)t->tab_gq.p : nullptr;
  HIPCHK(c, prv::launch_adam_table(ap, at, t->stream));
  // the step's last kernel: the MLP's Adam pass; on the fast path every thread also writes its weight into the MFMA fragments of
  // the next forward / backward pass and thread 0 closes the step
  prv::AdamMlpArgs am{};
  am.l2_reg = t->o.l2_reg;
  am.grad = (float*)t->mlp_g.p;
  am.w = (float*)t->mlp_w.p;
  am.m = (float*)t->mlp_m.p;
  am.v = (float*)t->mlp_v.p;
  am.w16 = (uint16_t*)m.mlp.p;
  am.w16_as_f32 = (float*)t->mlp_f.p;
  am.stage = dw_stage;
  am.end_of_step = t->sw.fast_forward ? 0 : 1;
  am.frags = t->sw.fast_forward ? (uint16_t*)t->frags.p : nullptr;
  am.frag_pos = (const int*)t->frag_pos.p;
  am.sample_count = sc->sample_count;
  am.lr = t->o.lr;
  HIPCHK(c, prv::launch_adam_mlp(ap, am, t->stream));
  return PRV_OK;
}

// One optimiser step, enqueued on the trainer's own stream (no host synchronisation).  Its ray batch first, unless the
// previous step's Adam launch listed it already; then a replay of the captured step graph (5 kernel nodes, one launch; one
// graph per variant: with / without the next step's batch), or the plain launches when graphs are switched off.  The next
// step's batch is listed ahead unless this is the call's last step or a density-grid refresh follows it (the batch must see
// the refreshed grid, as the oracle's does).
int train_enqueue_step(prv_trainer* t, bool last_of_call) {
  prv_ctx* c = t->ctx;
  int rc;
  const bool refresh_follows = t->o.occ_every > 0 && (t->step + 1u) % (uint32_t)t->o.occ_every == 0;
  const bool list_next = can_list_ahead(t) && !last_of_call && !refresh_follows;
  if (!t->rays_listed && (rc = train_open_step(t)) != PRV_OK) return rc;
  hipGraphExec_t& graph = t->step_graph[list_next ? 1 : 0];
  if (use_graph(t) && graph && t->graph_bwd_blocks[list_next ? 1 : 0] != bwd_blocks(t)) { // alone before, side by side now (or back): the count is baked into the graph
    (void)hipGraphExecDestroy(graph);
    graph = nullptr;
  }
  if (use_graph(t) && !graph) {
    t->graph_bwd_blocks[list_next ? 1 : 0] = bwd_blocks(t);
    hipGraph_t g = nullptr;
    // Captured on a stream of the context's that exists for nothing else, replayed on the trainer's own: a stream created with a
    // CU mask is a BLOCKING stream (the API has no flags), and by the stream-capture rules a legacy-default-stream call of
    // another thread (PyTorch's default stream is that one) while a blocking stream captures is an implicit dependency on the
    // capture, i.e. an error.  This runtime did not raise it when tried (tests/test_gpu_train.py runs such a thread beside four
    // captures, with and without this); a non-blocking capture stream costs nothing and does not depend on that.
    hipStream_t const run_stream = t->stream;
    if (!c->capture_stream && hipStreamCreateWithFlags(&c->capture_stream, hipStreamNonBlocking) != hipSuccess) {
      (void)hipGetLastError();
      c->capture_stream = nullptr;
    }
    if (!c->capture_stream || hipStreamBeginCapture(c->capture_stream, hipStreamCaptureModeThreadLocal) != hipSuccess) {
      t->graph_failed = true;
    } else {
      t->stream = c->capture_stream; // (the launchers below enqueue on t->stream)
      rc = train_step_launches(t, list_next);
      t->stream = run_stream;
      const hipError_t e = hipStreamEndCapture(c->capture_stream, &g);
      if (rc != PRV_OK || e != hipSuccess || !g || hipGraphInstantiate(&graph, g, nullptr, nullptr, 0) != hipSuccess) {
        graph = nullptr;
        t->graph_failed = true; // fall back to plain launches for good
      }
      if (g) (void)hipGraphDestroy(g);
    }
  }
  if (use_graph(t) && graph) HIPCHK(c, hipGraphLaunch(graph, t->stream));
  else if ((rc = train_step_launches(t, list_next)) != PRV_OK) return rc;
  t->rays_listed = list_next;
  t->step += 1; // mirrors TrainState::step, which the step's last kernel advances on the device
  if (t->o.occ_every > 0 && t->step % (uint32_t)t->o.occ_every == 0 && (rc = train_density_refresh(t)) != PRV_OK) return rc;
  return PRV_OK;
}

// point the device state at this call's loss array
int train_begin_call(prv_trainer* t, float* losses_dev) {
  prv::TrainState st{};
  st.step = t->step;
  st.step0 = t->step;
  st.n_active = t->n_active;
  st.losses = losses_dev;
  { // the first step of the call is opened here (later ones by the previous step's last kernel)
    const double n = (double)t->step + 1.0;
    st.lr_t = (float)((double)t->o.lr * std::sqrt(1.0 - std::pow((double)t->o.beta2, n)) / (1.0 - std::pow((double)t->o.beta1, n)));
  }
  HIPCHK(t->ctx, hipMemsetAsync(train_scal(t)->sample_count, 0, sizeof(prv::TrainScal::sample_count), t->stream));
  t->rays_listed = false;
  HIPCHK(t->ctx, hipMemcpyAsync(&train_scal(t)->state, &st, sizeof(st), hipMemcpyHostToDevice, t->stream));
  HIPCHK(t->ctx, hipStreamSynchronize(t->stream)); // `st` is a stack object
  return PRV_OK;
}

// after the last step: losses and the used-sample count to the host, then the slot's render state
int train_finish(prv_trainer* t, int n_steps, float* losses_host) {
  prv_ctx* c = t->ctx;
  unsigned long long used = 0;
  if (losses_host) HIPCHK(c, hipMemcpyAsync(losses_host, t->losses.p, (size_t)n_steps * 4, hipMemcpyDeviceToHost, t->stream));
  prv::TrainState st{};
  prv::TrainScal* const sc = train_scal(t);
  HIPCHK(c, hipMemcpyAsync(&used, &sc->used, sizeof(used), hipMemcpyDeviceToHost, t->stream));
  HIPCHK(c, hipMemcpyAsync(&st, &sc->state, sizeof(st), hipMemcpyDeviceToHost, t->stream));
  uint32_t listed = 0;
  const bool timing = t->sw.timing;
  if (timing) HIPCHK(c, hipMemcpyAsync(&listed, &sc->listed, sizeof(listed), hipMemcpyDeviceToHost, t->stream));
  HIPCHK(c, hipStreamSynchronize(t->stream));
  if (timing) // dev: how many of the samples the forward pass evaluated lie beyond their ray's termination (zero gradient seeds)
    fprintf(stderr, "prv_train_steps: last batch of slot %d: %u samples listed (forward pass), %llu composited before termination\n", t->slot, listed, used);
  t->samples_last = used;
  t->n_active = st.n_active;
  if (st.overflow) {
    (void)train_publish(t);
    return fail(c, PRV_E_STATE, "a step's ray batch listed more than %u samples (the sample list's capacity; PRV_STEP_NGP: 2^24): that step and every "
                                "later one of the call were void -- lower n_rays or target_samples", t->list_cap);
  }
  return train_publish(t);
}

// a trainer's device buffer: one a destroyed trainer of this context left behind (same size), else a new allocation.  The
// planner loop builds and drops five trainers per round: their 24 buffers each (250 MB per trainer) cost 8 ms to free and 3 ms
// to allocate per trainer, 5 s of a 175 s loop.  Nothing may rely on a fresh allocation's contents (prv_train_create zeroes what
// has to start at zero).
static int train_buffer(prv_ctx* c, Buffer& b, size_t bytes) {
  if (b.p && b.bytes >= bytes) return PRV_OK;
  if (!b.p && c->parked.take(b, bytes)) return PRV_OK;
  return ensure(c, b, bytes);
}

} // namespace

void prv_trainer::close() {
  for (hipGraphExec_t& g : step_graph) {
    if (g) (void)hipGraphExecDestroy(g);
    g = nullptr;
  }
  if (stream) (void)hipStreamDestroy(stream);
  stream = nullptr;
}

// Rows in allocation order: the parked pool hands its buffers out by size, oldest first, so the order decides which one a request gets.
std::vector<prv_trainer::BufferRow> prv_trainer::buffer_table() const {
  using T = prv_trainer;
  const size_t ns = list_cap, n_rays = (size_t)o.n_rays, R = (size_t)desc.occ_res, pp = (size_t)std::max(o.patch_w * o.patch_h, 1);
  return {
      {&T::cams, sizeof(CamDev) * (size_t)n_img, false},
      {&T::tab_wmv, (n_table + 3) / 4 * 48, true}, // {w[4], m[4], v[4]} per group of four scalars
      {&T::tab_g, n_table * 4, true},
      {&T::mlp_w, PRV_MLP_HALFS * 4, false},
      {&T::mlp_m, PRV_MLP_HALFS * 4, true},
      {&T::mlp_v, PRV_MLP_HALFS * 4, true},
      {&T::mlp_g, PRV_MLP_HALFS * 4, true},
      {&T::mlp_f, PRV_MLP_HALFS * 4, false},
      {&T::ema, R * R * R * 4, true},
      {&T::rays, sizeof(prv::TrainRay) * n_rays, false},
      {&T::samples, ns * 8, false},
      {&T::logits, ns * 16, false},
      {&T::seeds, ns * 16, false},
      {&T::ray_loss, n_rays * 4, false},
      {&T::ray_used, n_rays * 4, false},
      {&T::scal, sizeof(prv::TrainScal), true},
      {&T::losses, 0, false}, // a call's per-step losses: grown by prv_train_steps_multi
      {&T::dw_part, ((size_t)prv::train_dw_slots(ctx->n_cu * kBwdBlocksPerCu) + 16) * PRV_MLP_HALFS * 4, false}, // slots + the reduction's 16 group sums
      {&T::loss_part, (n_rays + 1023) / 1024 * 16, false},
      {&T::frags, (size_t)(kNumFrags + prv::kBwdFrags) * kFragHalfs * 2, false}, // forward fragments, then the backward ones
      {&T::slot_of, pp > 1 ? ns * 4 : 0, false}, // patches: list position of (ray, k-th live sample)
      {&T::frag_pos, (size_t)2 * PRV_MLP_HALFS * sizeof(int), false}, // every weight's place in the forward / backward fragments
      {&T::tab_gq, o.deterministic ? n_table * 8 : 0, true}, // the table gradient in 64-bit fixed point (prv_train.hip: table_grad_add)
      // a word per block of the ray launch, whichever kernel lists the batch (four rays, or a patch, per block: TrainRaysParams::block_tot)
      {&T::block_tot, o.deterministic ? std::max((n_rays + 3) / 4, (n_rays + pp - 1) / pp) * 4 : 0, true},
      {&T::tile_live, (ns + 31) / 32 + 64, true}, // one byte per 32-sample tile of the list (TrainTileParams::tile_live)
      {&T::act, (size_t)act_cap / 32 * prv::kActTileBytes, false}, // the forward pass's kept activations
  };
}

void prv_trainer::detach() {
  if (stream) (void)hipStreamSynchronize(stream);
  close();
  for (const BufferRow& r : buffer_table()) (this->*r.buf).reset();
}

// the trainer's stream (idle by now) stays with the context for the next trainer -- creating a stream with a queue of its own
// takes 11 ms, and the planner loop creates five trainers per round -- and so do its buffers (train_buffer)
void prv_trainer::retire() {
  if (stream) (void)hipStreamSynchronize(stream);
  hipStream_t keep = stream && own_queue && ctx->idle_queues.size() < 16 ? stream : nullptr;
  if (keep) stream = nullptr;
  close();
  if (keep) ctx->idle_queues.push_back(keep);
  for (const BufferRow& r : buffer_table()) ctx->parked.park(std::move(this->*r.buf));
}

extern "C" {

int prv_train_default_opts(prv_train_opts* o) {
  if (!o) return PRV_E_INVALID;
  memset(o, 0, sizeof(*o));
  o->n_rays = 1 << 16; // cap of the adaptive batch: large enough that target_samples (below) is what binds, as upstream
  o->n_samples = 128;
  o->lr = 1e-2f;
  o->beta1 = 0.9f;
  o->beta2 = 0.99f;
  o->eps = 1e-15f;
  o->l2_reg = 1e-6f;
  o->min_T = 1e-4f;
  o->seed = 0x7EA10001ull;
  o->random_bg = 1;
  o->occ_every = 16;
  o->occ_decay = 0.95f;
  // upstream's rule: optical thickness 0.01 over ITS march step, sqrt(3)/1024 (not this build's coarser 128-sample
  // step): cells below sigma = 5.9 are culled.  Measured on the synthetic scene: the 128-sample equivalent
  // (0.74) keeps a faint speckled haze alive in empty space (held-out SSIM 0.73 after 2500 steps); 5.9 gives
  // SSIM 0.99 and +1 dB PSNR.
  o->occ_sigma_thresh = 0.01f * 1024.0f / 1.7320508f;
  o->target_samples = 1 << 18; // upstream's batch: 2^18 samples per step (n_rays = 4096 would cap a carved scene at ~16 K)
  // The engine's own marcher, as upstream trains (run.py:188).  Measured at this batch (profiles/r06_train_rules.txt, one MI355X):
  // 597 M trained samples/s against 335 M under the fixed rule (a ray's consecutive samples share their table entries: 9.8
  // memory-side atomic requests per sample against 26.4), the planner loop's round of five member-steps 1.84 ms against 2.58;
  // held-out PSNR after the same 2,500 steps is LOWER, 25.45 against 25.84 dB on the loop's 5-view case and 37.0 against 39.3 dB
  // on trainbench's 64 views -- the 2^18-sample budget buys ~16 K rays of ~16 samples under this rule and ~65 K rays of ~3 under
  // the fixed one.  Fidelity to the reference's training workload decides; PRV_STEP_FIXED_S with n_samples = 128 is rounds 1-5.
  o->step_mode = PRV_STEP_NGP;
  o->n_samples = PRV_NGP_MAX_STEPS;
  o->deterministic = 0;
  return PRV_OK;
}

int prv_train_create(prv_ctx* c, int slot, const prv_camset* cs, const uint8_t* images_rgba8_dev, int width, int height,
                     const prv_train_opts* o, prv_trainer** out) try {
  if (!c) return PRV_E_INVALID;
  if (!out) return fail(c, PRV_E_INVALID, "out is NULL");
  *out = nullptr;
  int rc = check_model(c, slot);
  if (rc != PRV_OK) return rc;
  if (!cs || cs->cams.empty() || !images_rgba8_dev || !o) return fail(c, PRV_E_INVALID, "NULL / empty training data");
  if ((rc = check_image_size(c, width, height)) != PRV_OK) return rc;
  if (o->n_rays < 1 || o->n_rays > (1 << 22)) return fail(c, PRV_E_INVALID, "n_rays must be in [1, 2^22], got %d", o->n_rays);
  if (o->step_mode != PRV_STEP_FIXED_S && o->step_mode != PRV_STEP_NGP) return fail(c, PRV_E_INVALID, "step_mode must be PRV_STEP_FIXED_S or PRV_STEP_NGP, got %d", o->step_mode);
  const int max_s = o->step_mode == PRV_STEP_NGP ? prv::kMaxTrainSteps : prv::kMaxTrainSamples;
  if (o->n_samples < 1 || o->n_samples > max_s)
    return fail(c, PRV_E_INVALID, "n_samples must be in [1,%d] under step_mode %d, got %d", max_s, o->step_mode, o->n_samples);
  if (o->step_mode == PRV_STEP_NGP && std::max(o->patch_w, 1) * std::max(o->patch_h, 1) > 1)
    return fail(c, PRV_E_INVALID, "pixel patches are defined for PRV_STEP_FIXED_S only");
  if (o->target_samples < 0) return fail(c, PRV_E_INVALID, "target_samples < 0");
  {
    const int pw = std::max(o->patch_w, 1), ph = std::max(o->patch_h, 1);
    if (o->patch_w < 0 || o->patch_h < 0 || pw > 16 || ph > 16 || pw * ph > 16 || pw > width || ph > height)
      return fail(c, PRV_E_INVALID, "patch_w x patch_h must be at most 16 pixels and fit the image, got %dx%d", o->patch_w, o->patch_h);
  }
  if (!(o->lr >= 0.0f) || !(o->beta1 >= 0.0f && o->beta1 < 1.0f) || !(o->beta2 >= 0.0f && o->beta2 < 1.0f) || !(o->eps > 0.0f))
    return fail(c, PRV_E_INVALID, "bad optimiser settings");
  HIPCHK(c, hipSetDevice(c->device));
  if ((rc = check_device_ptr(c, images_rgba8_dev, "images_rgba8_dev")) != PRV_OK) return rc;
  HIPCHK(c, prv::train_prepare_kernels());
  Model& m = c->models[slot];
  std::unique_ptr<prv_trainer> owner(new prv_trainer(c)); // until the very end: an early return (and an exception) frees what it holds
  prv_trainer* t = owner.get();
  t->slot = slot;
  t->desc = m.desc;
  t->generation = m.generation;
  t->o = *o;
  t->o.patch_w = std::max(o->patch_w, 1);
  t->o.patch_h = std::max(o->patch_h, 1);
  t->n_img = (int)cs->cams.size();
  t->W = width;
  t->H = height;
  t->images = images_rgba8_dev;
  t->n_table = m.table_halfs;
  t->n_active = (uint32_t)o->n_rays;
  if (o->target_samples > 0) t->n_active = std::min<uint32_t>(t->n_active, std::max<uint32_t>(1u, (uint32_t)o->target_samples / (uint32_t)o->n_samples));
  t->sw = prv::train_switches_from_env();
  // The trainer's stream gets a hardware queue of its own.  Streams from hipStreamCreate share the runtime's pool of four
  // queues: five members stepping side by side sat on three of them, two pairs taking turns inside their queue.  A stream
  // created with a CU mask owns its queue -- the mask names every CU (restricting a member to a share of the CUs was measured
  // too, and is slower in every split: profiles/NOTES.md, round 5): round of five 0.548 -> 0.527 ms on one box.
  // PRV_TRAIN_OWN_QUEUE=0 (dev) keeps the pooled stream for an A/B on one box.
  hipError_t se = hipErrorUnknown;
  if (t->sw.own_queue && !c->idle_queues.empty()) { // a destroyed trainer's (prv_trainer::retire)
    t->stream = c->idle_queues.back();
    c->idle_queues.pop_back();
    t->own_queue = true;
    se = hipSuccess;
  } else if (t->sw.own_queue) {
    const std::vector<uint32_t> every_cu((size_t)(c->n_cu + 31) / 32, 0xffffffffu); // bits beyond the CU count are ignored
    se = hipExtStreamCreateWithCUMask(&t->stream, (uint32_t)every_cu.size(), every_cu.data());
    t->own_queue = se == hipSuccess;
    if (se != hipSuccess) (void)hipGetLastError();
  }
  if (se != hipSuccess) se = hipStreamCreateWithFlags(&t->stream, hipStreamNonBlocking);
  if (se != hipSuccess) {
    t->stream = nullptr;
    return fail(c, PRV_E_HIP, "stream create failed");
  }
  HostLevel lv[kMaxLevels];
  uint64_t total = 0;
  compute_levels(m.desc, lv, &total);
  for (int l = 0; l < m.desc.n_levels; l++) t->levels[l] = prv::LevelCanon{lv[l].scale, lv[l].res, lv[l].offset, lv[l].size, lv[l].hashed};
  // the step's sample list: every ray's every sample under the fixed rule; under the engine's rule a ray may list 1024 steps but
  // the budget keeps a step near target_samples -- 2^24 (64 x the default budget), and a batch beyond it fails loudly (TrainState::overflow)
  size_t ns = (size_t)o->n_rays * (size_t)o->n_samples;
  if (o->step_mode == PRV_STEP_NGP) ns = std::min<size_t>(ns, prv::kNgpListCap);
  if (ns > 0xffffffffull) return fail(c, PRV_E_INVALID, "n_rays x n_samples must stay below 2^32");
  t->list_cap = (uint32_t)ns;
  // The forward pass keeps its activations for the backward pass (528 B per sample: 512 of activations + the position; PRV_TRAIN_KEEP_ACT=0: recompute).
  // Sized for the step the sample budget aims at, with room for the adaptive ray count to overshoot (it may double from
  // one step to the next); tiles beyond the buffer -- the all-occupied first steps of a large n_rays -- are recomputed.
  if (t->sw.fast_forward && t->sw.keep_act) {
    size_t cap = o->target_samples > 0 ? std::max<size_t>((size_t)4 * (size_t)o->target_samples, (size_t)1 << 20) : (size_t)1 << 22;
    if (t->sw.act_cap) cap = (size_t)t->sw.act_cap; // tests: force the two-launch backward pass
    t->act_cap = (uint32_t)(std::min(std::min(cap, (size_t)1 << 22), (ns + 31) / 32 * 32) / 32 * 32);
  }
  // a buffer a destroyed trainer of this context left behind (same size), else a new allocation (train_buffer); what has to
  // start at zero is zeroed whole, not only the bytes asked for
  const std::vector<prv_trainer::BufferRow> table = t->buffer_table();
  for (const auto& r : table)
    if (r.bytes && (rc = train_buffer(c, t->*r.buf, r.bytes)) != PRV_OK) return rc;
  std::vector<CamDev> cams(cs->cams.size());
  for (size_t i = 0; i < cams.size(); i++) cams[i] = cam_at(cs, (int)i, width, height);
  hipError_t e = hipMemcpyAsync(t->cams.p, cams.data(), sizeof(CamDev) * cams.size(), hipMemcpyHostToDevice, c->stream);
  for (const auto& r : table)
    if (e == hipSuccess && r.bytes && r.zeroed) e = hipMemsetAsync((t->*r.buf).p, 0, (t->*r.buf).bytes, c->stream);
  if (e == hipSuccess) e = prv::launch_widen_table((const uint16_t*)m.table.p, t->n_table, (float*)t->tab_wmv.p, c->stream);
  if (e == hipSuccess) e = prv::launch_widen((const uint16_t*)m.mlp.p, PRV_MLP_HALFS, (float*)t->mlp_w.p, c->stream);
  if (e == hipSuccess) e = prv::launch_widen((const uint16_t*)m.mlp.p, PRV_MLP_HALFS, (float*)t->mlp_f.p, c->stream);
  if (e == hipSuccess) e = prv::launch_prepack_frags((const uint16_t*)m.mlp.p, m.desc.n_features, (uint16_t*)t->frags.p, c->stream);
  if (e == hipSuccess) e = prv::launch_frag_positions(m.desc.n_features, (int*)t->frag_pos.p, c->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
  if (e != hipSuccess) return fail(c, PRV_E_HIP, "trainer setup: %s", hipGetErrorString(e));
  *out = owner.release();
  return PRV_OK;
} catch (...) { return caught(c); }

int prv_train_steps(prv_trainer* t, int n_steps, float* losses_host) { return prv_train_steps_multi(&t, 1, n_steps, losses_host); }

/* several trainers of one context (the members of an ensemble, main.cpp:2041-2043) step side by side: step i
 * of every trainer is enqueued on that trainer's own stream before step i+1 of any, so the small launches
 * of one member fill the gaps of the others.  losses_host: n_trainers rows of n_steps (may be NULL). */
int prv_train_steps_multi(prv_trainer** ts, int n_trainers, int n_steps, float* losses_host) try {
  if (!ts || n_trainers < 1 || !ts[0]) return PRV_E_INVALID;
  prv_ctx* c = ts[0]->ctx;
  int rc;
  for (int k = 0; k < n_trainers; k++) {
    if (!ts[k] || ts[k]->ctx != c) return fail(c, PRV_E_INVALID, "trainers must belong to one context");
    if ((rc = train_check(ts[k])) != PRV_OK) return rc;
    for (int j = 0; j < k; j++)
      if (ts[j]->slot == ts[k]->slot) return fail(c, PRV_E_INVALID, "two trainers on model slot %d", ts[k]->slot);
  }
  if (n_steps < 0) return fail(c, PRV_E_INVALID, "n_steps < 0");
  if (n_steps == 0) return PRV_OK;
  HIPCHK(c, hipSetDevice(c->device));
  for (int k = 0; k < n_trainers; k++)
    if ((rc = ensure(c, ts[k]->losses, (size_t)n_steps * 4)) != PRV_OK) return rc;
  HIPCHK(c, hipStreamSynchronize(c->stream)); // renders of these slots that are still in flight
  for (int k = 0; k < n_trainers; k++) ts[k]->side_by_side = n_trainers > 1;
  for (int k = 0; k < n_trainers; k++)
    if ((rc = train_begin_call(ts[k], (float*)ts[k]->losses.p)) != PRV_OK) return rc;
  const bool timing = ts[0]->sw.timing; // dev: is the host or the GPU the slower side?
  const auto t0 = std::chrono::steady_clock::now();
  for (int i = 0; i < n_steps; i++)
    for (int k = 0; k < n_trainers; k++)
      if ((rc = train_enqueue_step(ts[k], i == n_steps - 1)) != PRV_OK) return rc;
  const auto t1 = std::chrono::steady_clock::now();
  if (timing) {
    for (int k = 0; k < n_trainers; k++) (void)hipStreamSynchronize(ts[k]->stream);
    const auto t2 = std::chrono::steady_clock::now();
    fprintf(stderr, "prv_train_steps: %d x %d steps: host enqueue %.3f ms, then waited %.3f ms for the GPU\n", n_trainers, n_steps,
            std::chrono::duration<double, std::milli>(t1 - t0).count(), std::chrono::duration<double, std::milli>(t2 - t1).count());
  }
  for (int k = 0; k < n_trainers; k++)
    if ((rc = train_finish(ts[k], n_steps, losses_host ? losses_host + (size_t)k * n_steps : nullptr)) != PRV_OK) return rc;
  return PRV_OK;
} catch (...) { return caught((ts && n_trainers > 0 && ts[0]) ? ts[0]->ctx : nullptr); }

int prv_train_gradients(prv_trainer* t, float* table_grad_host, float* mlp_grad_host, float* loss) try {
  int rc = train_check(t);
  if (rc != PRV_OK) return rc;
  prv_ctx* c = t->ctx;
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  prv::TrainScal* const sc = train_scal(t);
  if ((rc = train_begin_call(t, &sc->loss)) != PRV_OK) return rc;
  if ((rc = train_open_step(t)) != PRV_OK) return rc;
  if ((rc = train_forward_backward(t, prv::DwReduce::Here, nullptr)) != PRV_OK) return rc;
  HIPCHK(c, prv::launch_train_loss_finish((const double*)t->loss_part.p, t->o.n_rays, &sc->state, &sc->used, t->stream));
  unsigned long long used = 0;
  if (t->o.deterministic) HIPCHK(c, prv::launch_grad_q_to_f32((long long*)t->tab_gq.p, t->n_table, (float*)t->tab_g.p, t->stream));
  if (table_grad_host) HIPCHK(c, hipMemcpyAsync(table_grad_host, t->tab_g.p, t->n_table * 4, hipMemcpyDeviceToHost, t->stream));
  if (mlp_grad_host) HIPCHK(c, hipMemcpyAsync(mlp_grad_host, t->mlp_g.p, PRV_MLP_HALFS * 4, hipMemcpyDeviceToHost, t->stream));
  if (loss) HIPCHK(c, hipMemcpyAsync(loss, &sc->loss, sizeof(float), hipMemcpyDeviceToHost, t->stream));
  HIPCHK(c, hipMemcpyAsync(&used, &sc->used, sizeof(used), hipMemcpyDeviceToHost, t->stream));
  HIPCHK(c, hipMemsetAsync(t->tab_g.p, 0, t->n_table * 4, t->stream));
  HIPCHK(c, hipMemsetAsync(t->mlp_g.p, 0, PRV_MLP_HALFS * 4, t->stream));
  prv::TrainState st{};
  HIPCHK(c, hipMemcpyAsync(&st, &sc->state, sizeof(st), hipMemcpyDeviceToHost, t->stream));
  HIPCHK(c, hipStreamSynchronize(t->stream));
  t->samples_last = used;
  if (st.overflow) return fail(c, PRV_E_STATE, "the ray batch listed more than %u samples (the sample list's capacity)", t->list_cap);
  return PRV_OK;
} catch (...) { return caught(t ? t->ctx : nullptr); }

int prv_train_refresh_occupancy(prv_trainer* t) try {
  int rc = train_check(t);
  if (rc != PRV_OK) return rc;
  HIPCHK(t->ctx, hipSetDevice(t->ctx->device));
  HIPCHK(t->ctx, hipStreamSynchronize(t->ctx->stream));
  if ((rc = train_density_refresh(t)) != PRV_OK) return rc;
  HIPCHK(t->ctx, hipStreamSynchronize(t->stream));
  return train_publish(t);
} catch (...) { return caught(t ? t->ctx : nullptr); }

int prv_train_debug_stamps(prv_trainer* t, unsigned long long* out64) try {
  if (!t || !t->ctx || !out64) return PRV_E_INVALID;
  prv_ctx* c = t->ctx;
  HIPCHK(c, hipMemcpy(out64, train_scal(t)->stamps, sizeof(prv::TrainScal::stamps), hipMemcpyDeviceToHost));
  return PRV_OK;
} catch (...) { return caught(t ? t->ctx : nullptr); }

int prv_train_active_rays(const prv_trainer* t) { return t ? (int)t->n_active : PRV_E_INVALID; }

int prv_train_info(const prv_trainer* t, uint32_t* steps_done, uint64_t* samples_last, uint64_t* table_scalars) try {
  if (!t) return PRV_E_INVALID;
  if (steps_done) *steps_done = t->step;
  if (samples_last) *samples_last = t->samples_last;
  if (table_scalars) *table_scalars = t->n_table;
  return PRV_OK;
} catch (...) { return caught(t ? t->ctx : nullptr); }

int prv_train_master(prv_trainer* t, float* table_host, float* mlp_host) try {
  int rc = train_check(t);
  if (rc != PRV_OK) return rc;
  prv_ctx* c = t->ctx;
  HIPCHK(c, hipSetDevice(c->device));
  Buffer flat; // the w part of every {w, m, v} record (16 of 48 bytes), made contiguous on the device: ONE linear copy
  // (a 2-D copy of millions of 16-byte rows at a 48-byte pitch into pageable memory is the copy engine's worst shape)
  if (table_host) {
    if ((rc = ensure(c, flat, t->n_table * 4)) != PRV_OK) return rc;
    hipError_t e = prv::launch_narrow_table((const float*)t->tab_wmv.p, t->n_table, (float*)flat.p, t->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(table_host, flat.p, t->n_table * 4, hipMemcpyDeviceToHost, t->stream);
    if (e != hipSuccess) {
      (void)hipStreamSynchronize(t->stream);
      return fail(c, PRV_E_HIP, "master weights: %s", hipGetErrorString(e));
    }
  }
  hipError_t e = mlp_host ? hipMemcpyAsync(mlp_host, t->mlp_w.p, PRV_MLP_HALFS * 4, hipMemcpyDeviceToHost, t->stream) : hipSuccess;
  const hipError_t e2 = hipStreamSynchronize(t->stream); // (before `flat` goes)
  if (e != hipSuccess || e2 != hipSuccess) return fail(c, PRV_E_HIP, "master weights: %s", hipGetErrorString(e != hipSuccess ? e : e2));
  return PRV_OK;
} catch (...) { return caught(t ? t->ctx : nullptr); }

void prv_train_destroy(prv_trainer* t) { destroy_handle(t); }

} // extern "C"
