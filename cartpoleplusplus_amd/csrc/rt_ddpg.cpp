// DDPG train ops, the fused inner step and its hipGraph, the data-parallel half steps (cpp_ddpg_*)
#include "rt_internal.h"

// ---------------------------------------------------------------------------------------------
// DDPG
// ---------------------------------------------------------------------------------------------

struct cpp_ddpg {
  cpp_ctx* ctx; cpp_net *actor, *critic, *tactor, *tcritic; cpp_ddpg_hyper hp;
  int maxB; long nA, nC;
  float* gradbuf; float *dq_da, *td, *dq, *loss_norms /* [0] loss [1] actor norm [2] critic norm */, *ones;
  double* norm_part;
  double* heads_part;                              // fused heads kernel: per-workgroup partial sums of td^2 (a distributional trainer: dist_td_kernel's)
  // how the accessors find what the last gradient pass left: the loss (cpp_ddpg_last_stats: heads_part's partials to add, or
  // loss_norms[0]) and the rows behind sac_part (cpp_ddpg_last_sac; cpp_ddpg_apply_gradients).  Written by whoever ran the pass; a
  // replayed graph puts back its own (step_ran)
  LossAt last;
  // graph replay of the full inner step (the sampler's range is read from the replay's device size word: one graph survives growth)
  StepGraph graph;
  cpp_batch* step_batch;
  // graph replay of ONE minibatch on host-drawn rows, no target update (cpp_ddpg_train_rows: the reference's literal loop)
  StepGraph rgraph;
  uint64_t graph_gen = 0;    // part of every graph's key: invalidate_graphs() moves it
  uint64_t epoch;            // cpp_ctx::kernel_epoch the cached graphs were captured under (route_check)
  DpGraph dgraph;            // the data-parallel step (default mode)
  // graph replay of the data-parallel half step (sample + both gradient sets)
  // three variants: 0 samples its own minibatch; 1 / 2 find it presampled (by the previous call's rider, conv1_dw_gather.hip)
  // in the second / first set of slot arrays.  One key for all three and for both families (half_key).
  // hg[0]: the whole half step as one graph per variant; hg[1]: split at the conv backward (two graphs per variant) so that the
  // all-reduce of the fully-connected layers' gradients can run beside the conv backward (cpp_ddpg_dp_train_step, overlap)
  struct HalfGraphs { StepGraph g[3][2]; int next[3] = {0, 0, 0}; } hg[2];   // next: variant of the following call
  GraphKey half_key; uint64_t h_write_gen;
  uint64_t dp_local;       // minibatches applied locally since the last parameter averaging (periodic mode)
  int pre_variant;         // variant of the next cpp_ddpg_sample_and_compute call if its key still matches (0: sample)
  int32_t* slot_set[2][2]; // the two sets of slot arrays of step_batch
  // the update rule of the two 'optimiser' scopes (ddpg_cartpole.py:118-119, :218; cpp_ddpg_set_optimiser).  GradientDescent has no state.
  // Momentum / Adam: slots over gradbuf's layout [actor | critic], and one step count per list on the device (captured graphs replay
  // them): [0] counts the actor's applies, [1] the critic's.
  int opt_kind; float opt_momentum, opt_beta1, opt_beta2, opt_epsilon;
  float *opt_m, *opt_v; uint64_t* opt_step;
  // target policy smoothing (cpp_ddpg_set_target_smoothing; common.h: TpsArgs).  tps_n[0]: the count of target-forming gradient passes (a
  // device word: captured graphs replay it), tps_n[1]: the count the last pass drew at; tps_eps: its clipped noise, maxB x A
  bool tps_on; float tps_sigma, tps_clip; uint64_t tps_seed; uint64_t* tps_n; float* tps_eps;
  // A pass that reads tps_n[0] owes it one increment (PassLeft::noise_owed): the apply() behind it carries it, or tps_settle()
  // delayed policy updates (cpp_ddpg_set_policy_delay; common.h: DdpgHeadsArgs::pd, OptSegs::hold).  pd_d: the delay (1: off, and pd is
  // never passed to a launch); pd: three device words (captured graphs replay them) -- the critic updates applied since the configuring
  // call, whether the last minibatch held the actor, the count modulo pd_d
  int pd_d; uint64_t* pd;
  Arena arena;
  // twin Q heads (cpp_net_create_twin_q: both critics are twin critics, or neither): head 2's temporal difference, maxB.  The trainer
  // has no switch of its own -- what the critics are decides every path
  bool twin = false; float* td2 = nullptr;
  // the actor on the minimum head (cpp_ddpg_set_actor_min_q; twin critics only): dq_da -- and with it the actor's list -- is the gradient of
  // the smaller online head at a = mu(s1), chosen per row.  amin_sel: the last pass's choices (1 or 2), maxB; Q1 and Q2 at mu(s1) are left in
  // the critic's second workspace (out, out2) by whoever ran the pass -- the GEMM levels' q layers or the heads kernel's TWIN_MIN instances
  bool amin = false; int* amin_sel = nullptr;
  // the behaviour-cloning actor term (cpp_ddpg_set_behaviour_cloning; TD3+BC): bc_alpha > 0 switches it on -- such a trainer always takes
  // the GEMM levels of compute_gradients, where bc.hip stands behind the action-columns dX GEMM.  bc_stat: {lambda, m} of the last pass that
  // ran the actor's half, bc_g: its grad_ys at the actor's output (maxB x A), bc_rows: its per-row (1/A) sum (mu - a)^2 (maxB).  Alpha and
  // the floor are captured by value
  float bc_alpha = 0.f, bc_floor = 0.f; float *bc_stat = nullptr, *bc_g = nullptr, *bc_rows = nullptr;
  // distributional critic (cpp_net_create_distributional: both critics with one (N, v_min, v_max), or neither): what the last gradient
  // pass left for cpp_ddpg_last_distribution -- p of the fed evaluation, p' of the target evaluation, the projected target m, each
  // maxB x N.  Such a trainer always takes the GEMM levels of compute_gradients; dist.hip stands where td_kernel and `ones` stand
  int dist_n = 0; float *dist_p = nullptr, *dist_tp = nullptr, *dist_m = nullptr;
  // quantile critic (cpp_net_create_quantile: both critics with one N, or neither): dist_n is N, the three buffers hold theta, the sorted
  // target atoms and y for cpp_ddpg_last_quantiles, quant.hip stands where dist.hip stands.  kappa and the dropped top atoms
  // (cpp_ddpg_set_quantile_target) are captured by value
  bool quant = false; float quant_kappa = 1.f; int quant_drop = 0;
  // soft actor-critic (cpp_net_create_gaussian: both actors Gaussian with one (lo, hi), or neither; cpp_ddpg_set_sac).  sac_w: the
  // temperature words (common.h: SAC_W_*), sac_step: Adam's count, sac_part: the partials of g_alpha the last actor pass left for a batch
  // of last.sac_rows rows (0: none yet); [0] / [1]: the draw at state_1 / state_2 -- eps (maxB x A), logp (maxB); sac_rsoft: the soft reward the
  // TD kernels read where they read the batch's reward.  The noise count is tps_n (smoothing is refused with SAC), owed as smoothing's is.
  // Target entropy, rate and seed are captured by value.
  bool sac = false; float sac_hbar = 0.f, sac_lr = 0.f; uint64_t sac_seed = 0;
  float* sac_w = nullptr; uint64_t* sac_step = nullptr; double* sac_part = nullptr;
  float *sac_eps[2] = {nullptr, nullptr}, *sac_logp[2] = {nullptr, nullptr}, *sac_rsoft = nullptr;
};

// jobs 1 / 2 of sac.hip on the head the (target) actor's forward left in its first workspace: a sample (draw) or the mean
static SacSampleArgs sac_sample_args(const cpp_ddpg* d, bool target, bool draw, const cpp_batch* b = nullptr) {
  const cpp_net* n = target ? d->tactor : d->actor;
  SacSampleArgs s; memset(&s, 0, sizeof(s));
  s.logits = n->ws[0].logits; s.A = n->spec.action_dim; s.lo = n->ls_lo; s.hi = n->ls_hi;
  s.n = draw ? (const unsigned long long*)d->tps_n : nullptr;
  s.stream = target ? 0x300u : 0x200u; s.seed_lo = (unsigned)d->sac_seed; s.seed_hi = (unsigned)(d->sac_seed >> 32);
  s.eps = d->sac_eps[target ? 1 : 0]; s.a_out = n->ws[0].out; s.logp = d->sac_logp[target ? 1 : 0];
  if (target) {
    s.n_out = draw ? (unsigned long long*)(d->tps_n + 1) : nullptr;
    s.log_alpha = d->sac_w + SAC_W_TARGET; s.r = b->r; s.mask = b->m; s.discount = d->hp.discount; s.r_soft = d->sac_rsoft;
  }
  return s;
}
static SacGradArgs sac_grad_args(const cpp_ddpg* d, int B) {
  const cpp_net* a = d->actor;
  SacGradArgs g; memset(&g, 0, sizeof(g));
  g.logits = a->ws[0].logits; g.a = a->ws[0].out; g.eps = d->sac_eps[0]; g.dq_da = d->dq_da; g.logp = d->sac_logp[0];
  g.log_alpha = d->sac_w + SAC_W_LOG_ALPHA; g.B = B; g.A = a->spec.action_dim; g.lo = a->ls_lo; g.hi = a->ls_hi; g.target_entropy = d->sac_hbar;
  g.dz = a->ws[0].dz[a->fc.size() - 1]; g.part = d->sac_part; g.alpha_out = d->sac_w + SAC_W_ALPHA;
  return g;
}
// SAC has no target actor: its parameters are a bit copy of the actor's (and the target-forming pass's temperature word of log_alpha)
static int sac_sync_target(cpp_ddpg* d) {
  hipStream_t st = d->ctx->stream;
  if (d->tactor != d->actor)      // (actor-only training binds the live networks as stand-ins)
    HIP_CHECK(hipMemcpyAsync(d->tactor->params, d->actor->params, (size_t)d->nA * sizeof(float), hipMemcpyDeviceToDevice, st));
  HIP_CHECK(hipMemcpyAsync(d->sac_w + SAC_W_TARGET, d->sac_w + SAC_W_LOG_ALPHA, sizeof(float), hipMemcpyDeviceToDevice, st));
  d->tactor->wimg_key = nullptr;      // (the image the rider built is of the parameters before the copy)
  return CPP_OK;
}
static void reconfigured(cpp_ddpg* d);
static int sac_configure(cpp_ddpg* d, float init_temperature, float target_entropy, float lr, uint64_t seed) {
  cpp_ctx* ctx = d->ctx;
  HIP_CHECK(ctx_sync_stream(ctx));
  float w[SAC_WORDS]; memset(w, 0, sizeof(w));
  w[SAC_W_LOG_ALPHA] = w[SAC_W_TARGET] = logf(init_temperature); w[SAC_W_ALPHA] = init_temperature;
  HIP_CHECK(hipMemcpyAsync(d->sac_w, w, sizeof(w), hipMemcpyHostToDevice, ctx->stream));
  HIP_CHECK(hipMemsetAsync(d->sac_step, 0, sizeof(uint64_t), ctx->stream));
  HIP_CHECK(hipMemsetAsync(d->tps_n, 0, 2 * sizeof(uint64_t), ctx->stream));
  RC(sac_sync_target(d));
  HIP_CHECK(ctx_sync_stream(ctx));
  d->sac_hbar = target_entropy; d->sac_lr = lr; d->sac_seed = seed; d->last.sac_rows = 0;
  reconfigured(d);
  return CPP_OK;
}

// the minibatch's loss from the per-workgroup partials of the heads kernel or of dist.hip's job (b), added in a fixed order
static float loss_of_parts(const double* parts, int n, int B) {
  double s = 0.0;
  for (int i = 0; i < n; ++i) s += parts[i];
  return (float)(s / (double)B);
}

// job (b) of dist.hip on the fed and the target evaluation the forward passes left in the first workspaces
static int dist_td(cpp_ddpg* d, const cpp_batch* b, int B, bool backward, const float* w) {
  cpp_net *c = d->critic, *tc = d->tcritic;
  if (d->quant)
    return launch_quant_td(d->ctx, c->ws[0].logits, tc->ws[0].logits, b->r, b->m, d->hp.discount, B, d->dist_n, d->quant_kappa, d->quant_drop,
                           c->ws[0].out, tc->ws[0].out, d->dist_p, d->dist_tp, d->dist_m, d->td, backward ? c->ws[0].dz[c->fc.size() - 1] : nullptr,
                           d->heads_part, w);
  return launch_dist_td(d->ctx, c->ws[0].logits, tc->ws[0].logits, b->r, b->m, d->hp.discount, B, d->dist_n, c->dist_vmin, c->dist_vmax,
                        c->ws[0].out, tc->ws[0].out, d->dist_p, d->dist_tp, d->dist_m, d->td, backward ? c->ws[0].dz[c->fc.size() - 1] : nullptr,
                        d->heads_part, w);
}

extern "C" int cpp_ddpg_create(cpp_ctx* ctx, cpp_net* actor, cpp_net* critic, cpp_net* tactor, cpp_net* tcritic,
                               const cpp_ddpg_hyper* hp, cpp_ddpg** out) {
  ARG_CHECK(ctx && actor && critic && tactor && tcritic && hp && out, "cpp_ddpg_create: NULL argument");
  ARG_CHECK(actor->spec.kind == CPP_ACTOR && tactor->spec.kind == CPP_ACTOR, "cpp_ddpg_create: actor kinds");
  ARG_CHECK(critic->spec.kind == CPP_CRITIC && tcritic->spec.kind == CPP_CRITIC, "cpp_ddpg_create: critic kinds");
  ARG_CHECK(!actor->twin && !tactor->twin, "cpp_ddpg_create: a twin actor");
  ARG_CHECK(critic->twin == tcritic->twin, "cpp_ddpg_create: a twin critic needs a twin target critic (and a plain one a plain one)");
  ARG_CHECK(!actor->dist_n && !tactor->dist_n, "cpp_ddpg_create: a distributional actor");
  ARG_CHECK(critic->dist_n == tcritic->dist_n && critic->dist_vmin == tcritic->dist_vmin && critic->dist_vmax == tcritic->dist_vmax,
            "cpp_ddpg_create: critic and target critic must carry one value distribution (N, v_min, v_max), or none");
  ARG_CHECK(!(critic->dist_n && critic->twin), "cpp_ddpg_create: a distributional critic with twin Q heads");
  ARG_CHECK(critic->quant == tcritic->quant, "cpp_ddpg_create: a quantile critic needs a quantile target critic with the same N (never a categorical or a plain one)");
  ARG_CHECK(actor->gauss == tactor->gauss && actor->ls_lo == tactor->ls_lo && actor->ls_hi == tactor->ls_hi,
            "cpp_ddpg_create: a Gaussian actor needs a Gaussian target actor with the same log std bounds (and a plain one a plain one)");
  ARG_CHECK(!(actor->gauss && critic->dist_n), "cpp_ddpg_create: a Gaussian actor with a distributional or quantile critic");
  for (cpp_net* n : {actor, critic, tactor, tcritic})
    ARG_CHECK(!(actor->gauss && (n->spec.use_batch_norm || n->spec.use_dropout)), "cpp_ddpg_create: a Gaussian actor with batch norm or dropout");
  ARG_CHECK(actor->ln == critic->ln && actor->ln == tactor->ln && actor->ln == tcritic->ln,
            "cpp_ddpg_create: a feature layer norm on some of the four networks (cpp_net_create_feature_norm: all four, or none)");
  for (cpp_net* n : {critic, tactor, tcritic})
    ARG_CHECK(!actor->ln || (n->ln_act == actor->ln_act && n->ln_eps == actor->ln_eps),
              "cpp_ddpg_create: the four networks' feature layer norms differ in activation or epsilon");
  ARG_CHECK(actor->nparams == tactor->nparams && critic->nparams == tcritic->nparams, "cpp_ddpg_create: target shapes differ");
  ARG_CHECK(actor->state_elems == critic->state_elems && actor->spec.action_dim == critic->spec.action_dim,
            "cpp_ddpg_create: actor/critic input shapes differ");
  HIP_CHECK(hipSetDevice(ctx->device));
  cpp_ddpg* d = new cpp_ddpg();
  d->arena.stream = ctx->stream;
  d->ctx = ctx; d->actor = actor; d->critic = critic; d->tactor = tactor; d->tcritic = tcritic; d->hp = *hp;
  d->maxB = actor->maxB < critic->maxB ? actor->maxB : critic->maxB;
  d->nA = actor->nparams; d->nC = critic->nparams;
  d->step_batch = nullptr;
  d->epoch = ctx->kernel_epoch;
  d->dp_local = 0;
  d->h_write_gen = 0; d->pre_variant = 0;
  memset(d->slot_set, 0, sizeof(d->slot_set));
  d->opt_kind = OPT_SGD; d->opt_momentum = 0.f; d->opt_beta1 = 0.9f; d->opt_beta2 = 0.999f; d->opt_epsilon = 1e-8f;
  d->opt_m = d->opt_v = nullptr; d->opt_step = nullptr;
  d->pd_d = 1; d->pd = nullptr;
  d->tps_on = false; d->tps_sigma = d->tps_clip = 0.f; d->tps_seed = 0; d->tps_n = nullptr; d->tps_eps = nullptr;
  const int A = actor->spec.action_dim;
  int rc = dalloc(d->arena, &d->gradbuf, (size_t)(d->nA + d->nC));
  if (!rc) rc = dalloc(d->arena, &d->dq_da, (size_t)d->maxB * A);
  if (!rc) rc = dalloc(d->arena, &d->td, (size_t)d->maxB);
  if (!rc) rc = dalloc(d->arena, &d->dq, (size_t)d->maxB);
  if (!rc) rc = dalloc(d->arena, &d->ones, (size_t)d->maxB);
  if (!rc) rc = dalloc(d->arena, &d->loss_norms, (size_t)4);
  if (!rc) rc = dalloc(d->arena, &d->norm_part, (size_t)OPT_MAX_SEGS * NORM_PARTS);
  if (!rc) rc = dalloc(d->arena, &d->heads_part, (size_t)DDPG_HEADS_MAX_WGS);
  d->twin = critic->twin;
  if (!rc && d->twin) rc = dalloc(d->arena, &d->td2, (size_t)d->maxB);
  d->dist_n = critic->dist_n; d->quant = critic->quant;
  if (d->dist_n && dist_td_grid(d->maxB) > DDPG_HEADS_MAX_WGS) {
    cpp_set_error("cpp_ddpg_create: a distributional trainer takes batches up to %d (got %d)", 4 * DDPG_HEADS_MAX_WGS, d->maxB);
    rc = CPP_ERR_ARG;
  }
  for (float** p : {&d->dist_p, &d->dist_tp, &d->dist_m})
    if (!rc && d->dist_n) rc = dalloc(d->arena, p, (size_t)d->maxB * d->dist_n);
  d->sac = actor->gauss;
  if (d->sac && sac_grid(d->maxB) > DDPG_HEADS_MAX_WGS) {
    cpp_set_error("cpp_ddpg_create: a soft actor-critic trainer takes batches up to %d (got %d)", 4 * DDPG_HEADS_MAX_WGS, d->maxB);
    rc = CPP_ERR_ARG;
  }
  if (d->sac) {
    if (!rc) rc = dalloc(d->arena, &d->sac_w, (size_t)SAC_WORDS);
    if (!rc) rc = dalloc(d->arena, &d->sac_step, (size_t)1);
    if (!rc) rc = dalloc(d->arena, &d->tps_n, (size_t)2);
    if (!rc) rc = dalloc(d->arena, &d->sac_part, (size_t)DDPG_HEADS_MAX_WGS);
    if (!rc) rc = dalloc(d->arena, &d->sac_rsoft, (size_t)d->maxB);
    for (int k = 0; k < 2; ++k) {
      if (!rc) rc = dalloc(d->arena, &d->sac_eps[k], (size_t)d->maxB * A);
      if (!rc) rc = dalloc(d->arena, &d->sac_logp[k], (size_t)d->maxB);
    }
    // (until cpp_ddpg_set_sac: temperature 0.1, target entropy -A, rate 1e-4, seed 0)
    if (!rc) rc = sac_configure(d, 0.1f, -(float)A, 1e-4f, 0);
  }
  if (!rc) rc = launch_fill(ctx, d->ones, 1, 0, 1, d->maxB, 1.0f);
  if (rc) { d->arena.release(); delete d; return rc; }
  actor->grads = d->gradbuf; critic->grads = d->gradbuf + d->nA;
  HIP_CHECK(ctx_sync_stream(ctx));
  ctx->n_trainers += 1;
  *out = d;
  return CPP_OK;
}

// Everything the captured launches hold by value has changed (the conv1 route, the optimiser's rule, target smoothing): every cached graph
// of this trainer, the half steps' variants included, misses at its next use.  A new cache needs no line here: gen is part of its key.
static void invalidate_graphs(cpp_ddpg* d) { ++d->graph_gen; }
// ... which is how every setter ends; a minibatch presampled for the half steps goes with the graphs that would have consumed it
static void reconfigured(cpp_ddpg* d) { invalidate_graphs(d); d->pre_variant = 0; }

// What a cached step_body leaves on the host: its record for the accessors is kept with the graph it was captured into and put back by
// a replay of that graph, which -- as the eager body -- also leaves no presampled minibatch for the half steps (it lived in the
// step_batch the step has just used).
static int step_ran(cpp_ddpg* d, StepGraph& G, int rc, StepRan how) {
  if (rc) return rc;
  if (how == STEP_CAPTURED) G.left = d->last;
  if (how == STEP_REPLAYED) { d->last = G.left; d->pre_variant = 0; }
  return CPP_OK;
}

// Every training entry point starts here: the context may have moved conv1 to the other kernel family since the last call (nearly
// constant channels: common.h, cpp_ctx::conv1_f32) -- the cached graphs then hold the wrong launches and a presampled minibatch may be
// in the wrong form (sampled slots against a gathered copy): everything is rebuilt by the calls' own "key changed" paths.
static void route_check(cpp_ddpg* d) {
  if (route_check(d->ctx, &d->epoch, &d->graph_gen, {d->actor, d->critic, d->tactor, d->tcritic})) d->pre_variant = 0;
}

extern "C" int cpp_ddpg_destroy(cpp_ddpg* d) {
  if (!d) return CPP_OK;
  (void)hipSetDevice(d->ctx->device);
  (void)ctx_sync_stream(d->ctx);
  if (d->step_batch) cpp_batch_destroy(d->step_batch);
  d->actor->grads = nullptr; d->critic->grads = nullptr;
  d->ctx->n_trainers -= 1;
  d->arena.release(); delete d; return CPP_OK;      // (the cached graphs go with their StepGraph members)
}

static int check_batch(cpp_ddpg* d, cpp_batch* b, const char* who) {
  ARG_CHECK(d && b, "%s: NULL argument", who);
  ARG_CHECK(b->B >= 1 && b->B <= d->maxB, "%s: batch size %d outside [1,%d]", who, b->B, d->maxB);
  ARG_CHECK(b->elems == d->actor->state_elems && b->A == d->actor->spec.action_dim, "%s: batch shape does not match the networks", who);
  return CPP_OK;
}

static TpsArgs tps_args(const cpp_ddpg* d) {
  TpsArgs t; memset(&t, 0, sizeof(t));
  if (!d->tps_on) return t;
  t.n = (const unsigned long long*)d->tps_n; t.n_out = (unsigned long long*)(d->tps_n + 1); t.eps = d->tps_eps;
  t.sigma = d->tps_sigma; t.clip = d->tps_clip; t.seed_lo = (unsigned)d->tps_seed; t.seed_hi = (unsigned)(d->tps_seed >> 32);
  return t;
}
// the increment of a target-forming pass that no apply() follows (cpp_ddpg_compute_gradients, the half steps): a launch of its own
// behind the pass -- only with smoothing on
static int tps_settle(cpp_ddpg* d, const PassLeft& left) {
  return left.noise_owed ? launch_counter_add(d->ctx, d->tps_n, 1) : CPP_OK;
}

const float* white_of(cpp_batch* b, int which, int C) { return b->white + (long)which * 2 * C; }

// The critic's loss on the fed and the target evaluation the forward passes left in the first workspaces (ddpg_cartpole.py:210-214):
// the TD values, the loss (d->heads_part's partials of a distributional trainer, else d->loss_norms[0]) and -- backward -- dz of the q layer
static int critic_td(cpp_ddpg* d, const cpp_batch* b, int B, bool backward, const float* w) {
  cpp_net *c = d->critic, *tc = d->tcritic;
  if (d->dist_n) return dist_td(d, b, B, backward, w);
  const int last = (int)c->fc.size() - 1;
  const float* rw = d->sac ? d->sac_rsoft : b->r;      // (r_soft: written by sac.hip's job 2 on the target actor's head)
  if (d->twin)
    return launch_td_twin(d->ctx, c->ws[0].out, c->ws[0].out2, tc->ws[0].out, tc->ws[0].out2, rw, b->m, d->hp.discount, B, d->td, d->td2,
                          backward ? c->ws[0].dz[last] : nullptr, backward ? c->ws[0].dz2[last] : nullptr, d->loss_norms, w);
  return launch_td(d->ctx, c->ws[0].out, tc->ws[0].out, rw, b->m, d->hp.discount, B, d->td, backward ? c->ws[0].dz[last] : nullptr, d->loss_norms, w);
}
// ... and where that leaves the loss
static LossAt critic_loss_at(const cpp_ddpg* d, int B, bool fused_heads) {
  LossAt at;
  at.parts = fused_heads ? (B + 3) / 4 : (d->dist_n ? dist_td_grid(B) : 0); at.B = B;
  return at;
}

// The optimiser's launch of the lists the plan names (rt_internal.h: OptPlan).  folded: only for gradients that are applied as computed
// (both lists, no scaling, nothing in between); next: that minibatch's whitening tables are computed by this launch's rider instead of
// a stats_finalize launch behind it.  *targets_left: both target updates left with this launch (the plan closes an outer step).
static int apply(cpp_ddpg* d, const OptPlan& plan, bool* targets_left = nullptr) {
  const bool do_actor = plan.actor, do_critic = plan.critic;
  const float grad_scale = plan.grad_scale;
  const NextBatch& nx = plan.next;
  OptSegs s; memset(&s, 0, sizeof(s));
  s.bump = plan.bump;
  if (plan.pass.noise_owed) s.bump2 = d->tps_n;      // (the pass in front read the count; nobody in this launch does)
  const bool ride = opt_closing_riders(d->ctx, s, plan, {d->tactor, d->tcritic}, d->hp.target_update_rate);
  if (targets_left) *targets_left = ride;
  opt_next_stats(d->ctx, s, nx);
  d->actor->wimg_key = nullptr; d->critic->wimg_key = nullptr;      // (the parameters change)
  s.nseg = 2; s.kind = d->opt_kind;
  const bool bumped = plan.pass.counted;
  // delayed policy updates: the launch in front has counted this minibatch and left the actor's hold word -- the heads kernel of the
  // gradient pass (step_body), or one tick launch here, which then moves the step counts as well.  The critic's half alone counts the
  // minibatch; the actor's half alone looks one ahead (it belongs to the minibatch whose critic half follows) and counts nothing.
  const bool pd_on = d->pd_d > 1;
  if (pd_on && do_actor) s.hold[0] = d->pd + PD_HOLD;
  if (pd_on && !bumped)
    RC(launch_pd_tick(d->ctx, d->pd, (unsigned)d->pd_d, s.kind != OPT_SGD ? d->opt_step : nullptr, do_actor, do_critic, do_actor && !do_critic));
  if (s.kind != OPT_SGD) {
    s.momentum = d->opt_momentum; s.beta1 = d->opt_beta1; s.beta2 = d->opt_beta2; s.epsilon = d->opt_epsilon;
    s.m[0] = d->opt_m; s.m[1] = d->opt_m + d->nA; s.v[0] = d->opt_v; s.v[1] = d->opt_v ? d->opt_v + d->nA : nullptr;
    s.step_seg[0] = d->opt_step; s.step_seg[1] = d->opt_step + 1;
    // a list's count moves with its own applies only (actor.train / critic.train: two optimisers).  Not in the optimiser's launch, whose
    // other workgroups read the counts: in the heads kernel of the gradient pass (step_body) or, on the other paths, a launch in front
    if (!bumped && !pd_on) {
      if (do_actor) RC(launch_counter_add(d->ctx, d->opt_step, 1));
      if (do_critic) RC(launch_counter_add(d->ctx, d->opt_step + 1, 1));
    }
  }
  s.p[0] = d->actor->params; s.g[0] = d->gradbuf; s.n[0] = do_actor ? d->nA : 0; s.lr[0] = d->hp.actor_learning_rate; s.group[0] = 0;
  s.p[1] = d->critic->params; s.g[1] = d->gradbuf + d->nA; s.n[1] = do_critic ? d->nC : 0; s.lr[1] = d->hp.critic_learning_rate; s.group[1] = 1;
  RC(opt_norms(d->ctx, s, plan, 2, d->norm_part));
  // conv1's operand images of the next minibatch ride along too (conv_rs16.h; opt_apply_kernel's second rider): both updates are in
  // this launch, the next minibatch's statistics are, conv1 of all four networks will run on that kernel
  cpp_net* inets[4] = {d->actor, d->critic, d->tactor, d->tcritic};
  const ConvL* L0 = d->actor->spec.pixel ? &d->actor->conv[0] : nullptr;
  // (CPP_RIDE_IMAGE_UPDATE=0, ablation build: no image workgroups at all -- conv1's parameters and slots are advanced by the update's
  // plain workgroups and the forward builds its image by a launch of its own: what the rider's restated update is compared with)
  static const bool no_img = cpp_switch_off("CPP_RIDE_IMAGE_UPDATE");
  const bool img = nx.b && nx.C > 0 && do_actor && do_critic && L0 && !d->actor->spec.use_batch_norm && !d->critic->spec.use_batch_norm &&
                   conv_rs16_ok(d->ctx, L0->Cin, L0->H, L0->W, kConvOut) && nx.B >= 2 && !no_img &&
                   conv1_opens_params(d->actor) && conv1_opens_params(d->critic);
  if (img) {
    s.img_n = 4; s.img_cin = L0->Cin;
    for (int j = 0; j < 4; ++j) {      // (the trained networks read state_1's tables, the targets state_2's)
      opt_img_net(s, j, inets[j], j < 2 ? j : -1, j < 2 ? 0 : 1, nx);
      const ConvL& L = inets[j]->conv[0];
      if (j < 2 && s.kind != OPT_SGD) { s.img[j].mw = s.m[j] + L.w_off; s.img[j].mb = s.m[j] + L.b_off; }
      if (j < 2 && s.kind == OPT_ADAM) { s.img[j].vw = s.v[j] + L.w_off; s.img[j].vb = s.v[j] + L.b_off; }
    }
  }
  // soft actor-critic: the temperature's update leaves with the actor's list, a launch of its own (rate 0: a fixed temperature, none)
  const int sac_rows = plan.pass.loss.sac_rows;
  if (d->sac && do_actor && d->sac_lr > 0.f && sac_rows > 0) RC(launch_sac_temperature(d->ctx, d->sac_part, sac_rows, d->sac_lr, d->sac_w, d->sac_step));
  // norms_out[group] is only written for lists that were applied (n > 0)
  RC(launch_opt_apply(d->ctx, s, grad_scale, d->hp.gradient_clip, d->norm_part, NORM_PARTS, d->loss_norms + 1));
  opt_img_built(s, inets, nx);
  // ... and the critic's list closes a minibatch: the target actor becomes the actor as this launch left it (behind the soft update)
  if (d->sac && do_critic) RC(sac_sync_target(d));
  return CPP_OK;
}

static int prep_batch(cpp_ddpg* d, cpp_batch* b) {
  if (d->actor->spec.pixel) RC(batch_ensure_stats(b, d->actor->spec.C));
  return CPP_OK;
}

// What a caller wants of the gradient pass: the halves to run -- the actor's (ddpg_cartpole.py:111-113, :220-222: dQ/da at actor(s1),
// pushed through the actor) and the critic's (:199-214: the TD loss against the target networks) -- and whether it trains.  train ==
// false is an evaluation (cpp_ddpg_check_loss, cpp_ddpg_q_gradients_wrt_actions): no critic backward, no noise drawn and nothing owed;
// soft actor-critic runs at eps = 0 and leaves the partials and the recorded temperature to the last training pass.
struct PassParts { bool actor = true, critic = true, train = true; };

// Both gradient sets of one minibatch (ddpg_cartpole.py:331-334) as one dependency graph: 4 conv trunk
// forwards, the MLP GEMMs batched level by level, 2 conv trunk backwards.  The critic trunk + the layers in
// front of the action splice run once for both uses of critic(s1, .).
// phase 0: everything.  The data-parallel step can split the pass at the conv backward: phase 1 = everything before it (all
// gradients of the fully connected layers are then final), phase 2 = the conv backward + the dW reductions.
// count_in_heads: the apply() behind this pass takes both lists (step_body) -- the heads kernel, where there is one, advances both step
// counts and the policy-delay words itself.  per: rt_internal.h, PerPass.  *left: what the pass left, written only when it succeeds.
// want: the parts of the pass (PassParts).  One half alone builds only its own nodes on the GEMM levels: per-network conv launches, no
// fused heads, no folded norms, nothing counted, no phase split.
static int compute_gradients(cpp_ddpg* d, cpp_batch* b, PassLeft* left, int phase = 0, bool count_in_heads = false, const PerPass& per = PerPass(),
                             const PassParts& want = PassParts()) {
  const bool doA = want.actor, doC = want.critic, both = doA && doC, train = want.train;
  if (!both && (phase != 0 || count_in_heads)) { cpp_set_error("compute_gradients: one half of the pass has no phases and counts nothing"); return CPP_ERR_STATE; }
  cpp_ctx* ctx = d->ctx;
  cpp_net *a = d->actor, *c = d->critic, *ta = d->tactor, *tc = d->tcritic;
  const int B = b->B, A = a->spec.action_dim, C = a->spec.pixel ? a->spec.C : 0;
  const float *w1 = white_of(b, 0, C), *w2 = white_of(b, 1, C);
  const void *s1 = b->direct_store ? b->direct_store : b->s[0], *s2 = b->direct_store ? b->direct_store : b->s[1];
  SlotScope slot_scope(b, {a, c}, {ta, tc});      // (conv1 of the four networks addresses its images through the sampled slots while this graph runs)
  const int dt = b->dtype;
  const int na = (int)a->fc.size(), nc = (int)c->fc.size(), cat = c->cat_layer;
  const FcL& Lcat = c->fc[cat];
  const long ldcat = Lcat.n_in + 1;
  OpGraph G;
  // The kernels that write the gradients also leave their share of the two lists' squared norms (cpp_ctx::sq_part): list 0 = actor,
  // list 1 = critic.  Not with batch norm (dbeta comes out of the BN backward kernels) and not for a split pass.
  SqScope sq_scope(ctx, 2, {0, 1}, both && phase == 0 && !a->spec.use_batch_norm && !c->spec.use_batch_norm);

  // ---- forward: the four conv trunks.  conv1 saturates the chip per network; the narrow conv2 / conv3 layers
  // of all four networks share one launch each.  (One half: its own networks, one by one -- batch norm follows each network's is_training.)
  int tA = -1, tC, tTA = -1, tTC = -1;
  if (both && a->spec.pixel && !a->spec.use_batch_norm) {
    cpp_net* nets[4] = {a, c, ta, tc};
    const void* sts[4] = {s1, s1, s2, s2};
    const float* whs[4] = {w1, w1, w2, w2};
    // conv1 / conv2 (+ conv3 as conv2's tail) of the four networks in one launch per layer; the two target networks have no
    // backward pass (nets_forward_trunk_fused, rt_net.cpp)
    const int t1 = G.fn([=] { return nets_forward_trunk_fused(ctx, nets, 4, sts, whs, 2, dt, B); }, {});
    tA = tC = tTA = tTC = t1;
  } else if (both && a->spec.pixel) {       // batch norm (training mode for the whole graph, ddpg_cartpole.py:145,237)
    cpp_net* nets[4] = {a, c, ta, tc};
    const void* sts[4] = {s1, s1, s2, s2};
    const float* whs[4] = {w1, w1, w2, w2};
    const int t1 = G.fn([=] { return nets_forward_trunk_bn(ctx, nets, 4, sts, whs, dt, B); }, {});
    tA = tC = tTA = tTC = t1;
  } else {      // the low-dimensional state's conversion; one half of a pixel pass: its own networks, each by its own is_training
    if (doA) tA = G.fn([=] { return net_forward_trunk(a, a->ws[0], s1, dt, w1, B); }, {});
    tC = G.fn([=] { return net_forward_trunk(c, c->ws[0], s1, dt, w1, B); }, {});
    if (doC) tTA = G.fn([=] { return net_forward_trunk(ta, ta->ws[0], s2, dt, w2, B); }, {});
    if (doC) tTC = G.fn([=] { return net_forward_trunk(tc, tc->ws[0], s2, dt, w2, B); }, {});
  }
  // ---- fused heads (heads.hip): when the critic is "[prefix, action] -> relu layer -> linear q" and the actor ends in a tanh
  // layer (the reference's networks, ddpg_cartpole.py:95-100, :166-171), everything from the actors' / critics' last hidden
  // activations to the first backward layer is one row-local kernel instead of five dependent GEMM levels + TD + copies.
  // CPP_FUSED_HEADS=0 keeps the GEMM levels.
  static const bool no_heads = cpp_switch_off("CPP_FUSED_HEADS");
  DdpgHeadsArgs hd; memset(&hd, 0, sizeof(hd));
  const bool twin = d->twin;
  const bool sac = d->sac;         // (its actor's head is 2A wide and linear: never the fused heads)
  const int dist = d->dist_n;      // (its q layer has N outputs: never the fused heads)
  const bool bc = d->bc_alpha > 0.f;      // (lambda needs every row of the minibatch: never the fused heads, whose rows are spread over workgroups)
  bool fused = both && !dist && !bc && !no_heads && na >= 2 && cat >= 1 && nc - cat == 2 && a->fc[na - 1].act == GE_TANH && Lcat.act == GE_RELU &&
               c->fc[nc - 1].n_out == 1 && c->fc[nc - 1].act == GE_NONE && a->fc[na - 1].n_out == A;
  // feature layer norm: the heads kernel writes dz[na - 2] through that layer's ReLU mask -- never the normalised layer 0, whose
  // activation derivative is ln.hip's.  (The critic's is dz[cat - 1] = dz[1].)
  if (a->ln && na < 3) fused = false;
  if (fused) {
    const FcL& Lo = a->fc[na - 1];
    hd.B = B; hd.A = A; hd.discount = d->hp.discount;
    hd.h2a = a->ws[0].fcin[na - 1]; hd.h2ta = ta->ws[0].fcin[na - 1]; hd.ld_h2a = Lo.n_in + 1; hd.n2a = Lo.n_in;
    hd.Wo = a->params + Lo.w_off; hd.Wo_t = ta->params + Lo.w_off;
    hd.h2c = c->ws[0].fcin[cat]; hd.h2tc = tc->ws[0].fcin[cat]; hd.ld_h2c = (int)ldcat; hd.n2c = Lcat.n_in - A;
    hd.W3 = c->params + Lcat.w_off; hd.W3_t = tc->params + Lcat.w_off; hd.n3 = Lcat.n_out;
    hd.wq = c->params + c->fc[nc - 1].w_off; hd.wq_t = tc->params + c->fc[nc - 1].w_off;
    hd.act = b->a; hd.r = b->r; hd.mask = b->m;
    hd.a_out = a->ws[0].out; hd.dq_da = d->dq_da; hd.adz = a->ws[0].dz[na - 1]; hd.dz_h2a = a->ws[0].dz[na - 2];
    hd.relu_x2 = relu_grad_epi(a, na - 2) == GE_MUL_RELU_GRAD_X2;
    hd.cat_splice = c->ws[0].fcin[cat] + (Lcat.n_in - A);
    hd.h3_out = c->ws[0].fcin[nc - 1]; hd.ld_h3 = Lcat.n_out + 1;
    hd.q_out = c->ws[0].out; hd.tq_out = tc->ws[0].out; hd.td = d->td; hd.dzq = c->ws[0].dz[nc - 1];
    hd.dz3 = c->ws[0].dz[cat]; hd.dz2c = c->ws[0].dz[cat - 1];
    hd.loss_part = d->heads_part;
    hd.w = per.w;
    hd.step_bump = (count_in_heads && d->opt_kind != OPT_SGD && phase == 0) ? (unsigned long long*)d->opt_step : nullptr;
    hd.tps = tps_args(d);
    if (count_in_heads && d->pd_d > 1 && phase == 0) { hd.pd = (unsigned long long*)d->pd; hd.pd_d = (unsigned)d->pd_d; }
    if (twin) {      // twin Q heads: head 2's two layers of both critics (nc - cat == 2), its buffers of the first workspace
      const FcL &L3b = c->fc2[cat], &Lqb = c->fc2[nc - 1];
      hd.W3b = c->params + L3b.w_off; hd.W3b_t = tc->params + L3b.w_off; hd.wqb = c->params + Lqb.w_off; hd.wqb_t = tc->params + Lqb.w_off;
      hd.h3b_out = c->ws[0].fcin2[nc - 1]; hd.q2_out = c->ws[0].out2; hd.tq2_out = tc->ws[0].out2; hd.td2 = d->td2;
      hd.dzq2 = c->ws[0].dz2[nc - 1]; hd.dz3b = c->ws[0].dz2[cat];
      // the actor on the minimum head: Q1 and Q2 at mu(s1) land where the GEMM levels leave them
      if (d->amin) { hd.min_q1 = c->ws[1].out; hd.min_q2 = c->ws[1].out2; hd.min_sel = d->amin_sel; }
    }
    fused = ddpg_heads_supported(hd);
    // the actors are one layer deeper than the critics' prefix (100-100-50 against 200-50): their last hidden layer joins the
    // heads kernel so that both stacks reach it, and leave it, in the same number of GEMM levels.  CPP_HEADS_PRE=0: GEMMs.
    static const bool no_pre = cpp_switch_off("CPP_HEADS_PRE");
    // (an actor with two hidden layers and a feature layer norm: fc[na - 3] is the normalised layer, GE_NONE -- no `pre`)
    if (fused && !no_pre && na >= 3 && !a->drop_counter && a->fc[na - 2].act == GE_RELU && a->fc[na - 3].act == GE_RELU) {
      DdpgHeadsArgs hp = hd;
      const FcL& L2 = a->fc[na - 2];
      hp.h1a = a->ws[0].fcin[na - 2]; hp.h1ta = ta->ws[0].fcin[na - 2]; hp.ld_h1a = L2.n_in + 1; hp.n1a = L2.n_in;
      hp.W2 = a->params + L2.w_off; hp.W2_t = ta->params + L2.w_off;
      hp.h2a_out = a->ws[0].fcin[na - 1]; hp.dz_h1a = a->ws[0].dz[na - 3];
      if (ddpg_heads_supported(hp)) hd = hp;
    }
  }
  const int pre = (fused && hd.n1a > 0) ? 1 : 0;
  int adz = -1, cdz = -1;
  // ---- feature layer norm: layer 0 of every network this pass runs is one GEMM level, and ONE ln launch stands behind it; its output
  // (the critic's: shared by both evaluations) is what layer 1 reads
  int aF = tA, taF = tTA, cP = tC, tcP = tTC, l0 = 0;
  if (a->ln) {
    cpp_net* ln_nets[4]; int ln_deps[4]; int nn = 0;
    auto layer0 = [&](cpp_net* n, int dep) { ln_nets[nn] = n; ln_deps[nn++] = G.gemm(fc_fwd_args(n, n->ws[0], 0, B), {dep}); };
    if (doA) layer0(a, tA);
    layer0(c, tC);
    if (doC) { layer0(ta, tTA); layer0(tc, tTC); }
    aF = taF = cP = tcP = add_ln_forward(G, ctx, ln_nets, nn, ln_deps, B);
    l0 = 1;
  }
  if (fused) {
    for (int l = l0; l < na - 1 - pre; ++l) {
      aF = G.gemm(fc_fwd_args(a, a->ws[0], l, B), {aF});
      taF = G.gemm(fc_fwd_args(ta, ta->ws[0], l, B), {taF});
    }
    if (a->drop_counter) {     // --use-dropout: this forward is counted once its layers have read the counter
      G.fn([=] { return bump_dropout(a); }, {aF});
      G.fn([=] { return bump_dropout(ta); }, {taF});
    }
    for (int l = l0; l < cat; ++l) {
      cP = G.gemm(fc_fwd_args(c, c->ws[0], l, B), {cP});
      tcP = G.gemm(fc_fwd_args(tc, tc->ws[0], l, B), {tcP});
    }
    const int hk = G.fn([=] { return launch_ddpg_heads(ctx, hd); }, {aF, taF, cP, tcP});
    if (per.hook) G.fn(per.hook, {hk});      // (prioritized replay: as soon as the TD values are known)
    // ---- actor backward below its head (the head's dX is part of the fused kernel)
    G.gemm(sq_gemm(ctx, 0, fc_dw_args(a, a->ws[0], na - 1, B, a->ws[0].dz[na - 1])), {hk});
    adz = add_fc_backward(G, a, a->ws[0], B, na - 2, hk, 0, pre ? na - 2 : -1);      // (pre: dz[na - 3] came out of the heads kernel)
    // ---- critic backward below its concat layer
    G.gemm(sq_gemm(ctx, 1, fc_dw_args(c, c->ws[0], nc - 1, B, c->ws[0].dz[nc - 1])), {hk});
    G.gemm(sq_gemm(ctx, 1, fc_dw_args(c, c->ws[0], cat, B, c->ws[0].dz[cat])), {hk});
    if (twin) {      // head 2's two dW GEMMs depend on the heads launch alone: they ride in this level
      G.gemm(sq_gemm(ctx, 1, twin_dw_args(c, c->ws[0], nc - 1, B)), {hk});
      G.gemm(sq_gemm(ctx, 1, twin_dw_args(c, c->ws[0], cat, B)), {hk});
    }
    // (the helper's relu_grad_epi(c, l) is GE_MUL_RELU_GRAD for every critic: a CPP_CRITIC's hidden layers are built with GE_RELU,
    // dropout or not -- rt_net.cpp's constructor gives GE_RELU_DROPOUT to actors and NAF heads only)
    cdz = add_fc_backward(G, c, c->ws[0], B, cat - 1, hk, 1);
    if (a->ln) {      // both chains stopped at g = dL/dy of layer 0
      cpp_net* ln_nets[2] = {a, c}; int ln_deps[2] = {adz, cdz}; const int ln_lists[2] = {0, 1};
      add_ln_backward(G, ctx, ln_nets, 2, ln_deps, ln_lists, B);
      adz = ln_deps[0]; cdz = ln_deps[1];
    }
  } else {      // the GEMM levels, each half's nodes only where one half is asked for
  const int cb = doC ? G.fn([=] { return launch_copy_cols(ctx, c->ws[0].fcin[cat], ldcat, Lcat.n_in - A, b->a, A, 0, A, B); }, {}) : -1;
  for (int l = l0; l < na; ++l) {
    GemmArgs g = fc_fwd_args(a, a->ws[0], l, B), t = fc_fwd_args(ta, ta->ws[0], l, B);
    if (l == na - 1 && !sac) {      // actions land directly in the critics' splice columns as well
      g.C2 = c->ws[1].fcin[cat] + (Lcat.n_in - A); g.ldc2 = ldcat;
      t.C2 = tc->ws[0].fcin[cat] + (Lcat.n_in - A); t.ldc2 = ldcat;
    }
    if (doA) aF = G.gemm(g, {aF});
    if (doC) taF = G.gemm(t, {taF});
  }
  if (a->drop_counter) {     // --use-dropout: this forward is counted once its layers have read the counter
    if (doA) G.fn([=] { return bump_dropout(a); }, {aF});
    if (doC) G.fn([=] { return bump_dropout(ta); }, {taF});
  }
  if (sac) {      // sac.hip's jobs 1 and 2 stand where the tanh epilogue stood: sample, log-density, splice columns, the soft reward
    SacSampleArgs sa = sac_sample_args(d, false, train), st = sac_sample_args(d, true, train, b);      // (an evaluation: eps = 0, the count unread)
    sa.B = st.B = B; sa.ld_splice = st.ld_splice = ldcat;
    sa.splice = c->ws[1].fcin[cat] + (Lcat.n_in - A); st.splice = tc->ws[0].fcin[cat] + (Lcat.n_in - A);
    if (doA) aF = G.fn([=] { return launch_sac_sample(ctx, sa); }, {aF});
    if (doC) taF = G.fn([=] { return launch_sac_sample(ctx, st); }, {taF});
  }
  for (int l = l0; l < cat; ++l) {
    GemmArgs g = fc_fwd_args(c, c->ws[0], l, B);
    if (l == cat - 1 && doA) { g.C2 = c->ws[1].fcin[cat]; g.ldc2 = ldcat; }   // same prefix for the second evaluation
    cP = G.gemm(g, {cP});
    if (doC) tcP = G.gemm(fc_fwd_args(tc, tc->ws[0], l, B), {tcP});
  }
  if (cat == 0 && doA)     // low-dim critic: the "prefix" is the converted state itself
    cP = G.fn([=] { return launch_copy_cols(ctx, c->ws[1].fcin[0], ldcat, 0, c->ws[0].fcin[0], ldcat, 0, Lcat.n_in - A, B); }, {tC});
  // target policy smoothing: the target actor's action in the target critic's splice columns, between the GEMM that wrote it and the
  // concat GEMM that reads it (ta->ws[0].out keeps the unsmoothed action).  An evaluation draws nothing
  int taS = taF;
  if (d->tps_on && doC && train) {
    const TpsArgs ts = tps_args(d);
    float* col = tc->ws[0].fcin[cat] + (Lcat.n_in - A);
    taS = G.fn([=] { return launch_tps_smooth(ctx, ts, col, (int)ldcat, col, (int)ldcat, B, A); }, {taF});
  }
  const bool amin = d->amin;      // (twin critics: cpp_ddpg_set_actor_min_q)
  int c1 = -1, c0 = -1, tcH = -1, c0b = -1, tcHb = -1, c1b = -1;
  for (int l = cat; l < nc; ++l) {
    if (doA) c1 = G.gemm(fc_fwd_args(c, c->ws[1], l, B), {l == cat ? cP : c1, l == cat ? aF : -1});
    // the actor on the minimum head: head 2 at a = mu(s1) as well, in head 1's levels (with the actor's half alone too)
    if (doA && amin) c1b = G.gemm(twin_fwd_args(c, c->ws[1], l, B), {l == cat ? cP : c1b, l == cat ? aF : -1});
    if (!doC) continue;
    c0 = G.gemm(fc_fwd_args(c, c->ws[0], l, B), {l == cat ? cP : c0, l == cat ? cb : -1, l == cat ? tC : -1});
    tcH = G.gemm(fc_fwd_args(tc, tc->ws[0], l, B), {l == cat ? tcP : tcH, l == cat ? taS : -1});
    if (twin) {      // head 2 of both critics on the same concat inputs (one smoothed action for both target heads), in head 1's levels
      c0b = G.gemm(twin_fwd_args(c, c->ws[0], l, B), {l == cat ? cP : c0b, l == cat ? cb : -1, l == cat ? tC : -1});
      tcHb = G.gemm(twin_fwd_args(tc, tc->ws[0], l, B), {l == cat ? tcP : tcHb, l == cat ? taS : -1});
    }
  }

  if (doA) {
  // ---- dQ/da at a = actor(s1): back through q_value .. splice on the second evaluation (dz of q is 1)
  int g = c1;
  // (a distributional critic: the gradient of the expectation, p (z - Q), stands where the scalar critic's q layer is fed ones)
  if (dist) g = G.fn([=] { return dist_expect(c, c->ws[1], B, c->ws[1].dz[nc - 1]); }, {c1});
  // (the minimum head: per row 1 for the chosen head and 0 for the other, in the q layers' dz of the second workspace -- actor_min.hip)
  if (amin) g = G.fn([=] { return launch_actor_min(ctx, c->ws[1].out, c->ws[1].out2, B, c->ws[1].dz[nc - 1], c->ws[1].dz2[nc - 1], d->amin_sel); }, {c1, c1b});
  const float* top = (dist || amin) ? c->ws[1].dz[nc - 1] : d->ones;
  int g2 = g;      // head 2's chain down to the concat layer, beside head 1's
  for (int l = nc - 1; l > cat; --l) {
    const FcL& L = c->fc[l];
    const float* dz = (l == nc - 1) ? top : c->ws[1].dz[l];
    g = G.gemm(fc_dx_args(c, l, B, dz, L.n_out, 0, L.n_in, c->ws[1].dz[l - 1], L.n_in, GE_MUL_RELU_GRAD,
                          c->ws[1].fcin[l], L.n_in + 1), {g});
    if (amin) g2 = G.gemm(twin_dx_args(c, c->ws[1], l, B), {g2});
  }
  {   // dQ/da (kept for cpp_ddpg_q_gradients_wrt_actions) and, in the same epilogue, the actor's head gradient
    const float* dz = (cat == nc - 1) ? top : c->ws[1].dz[cat];
    const bool plain_da = sac || bc;      // (the head gradient is a launch of its own behind this GEMM: sac.hip's job 3, bc.hip)
    const int epi = plain_da ? GE_NONE : GE_ACTOR_HEAD;
    const float* ay = plain_da ? nullptr : a->ws[0].out; const long lday = plain_da ? 0 : A;
    // the minimum head: (head 1's action columns) + (head 2's), then the epilogue -- a row's unselected head adds exact zeros
    const int h1 = amin ? G.gemm(fc_dx_args(c, cat, B, dz, Lcat.n_out, Lcat.n_in - A, A, d->dq_da, A, GE_NONE, nullptr, 0), {g}) : -1;
    GemmArgs ga = amin ? twin_da_args(c, c->ws[1], B, d->dq_da, epi, ay, lday)
                       : fc_dx_args(c, cat, B, dz, Lcat.n_out, Lcat.n_in - A, A, d->dq_da, A, epi, ay, lday);
    if (!plain_da) { ga.C2 = a->ws[0].dz[na - 1]; ga.ldc2 = A; }
    adz = amin ? G.gemm(ga, {h1, g2, aF}) : G.gemm(ga, {g, aF});
    if (bc) {      // behaviour cloning: lambda from Q(s1, mu(s1)) of the followed head (this chain started behind its q layer), then the head gradient
      BcArgs ba; memset(&ba, 0, sizeof(ba));
      ba.q1 = c->ws[1].out; ba.q2 = amin ? c->ws[1].out2 : nullptr; ba.sel = amin ? d->amin_sel : nullptr;
      ba.dq_da = d->dq_da; ba.mu = a->ws[0].out; ba.act = b->a; ba.B = B; ba.A = A; ba.alpha = d->bc_alpha; ba.q_floor = d->bc_floor;
      ba.adz = a->ws[0].dz[na - 1]; ba.stat = d->bc_stat; ba.g = d->bc_g; ba.rows = d->bc_rows;
      adz = G.fn([=] { return launch_bc(ctx, ba); }, {adz});
    }
    if (sac) {      // job 3: the (B, 2A) head gradient and the temperature gradient's partials
      SacGradArgs sg = sac_grad_args(d, B);
      if (!train) { sg.part = nullptr; sg.alpha_out = nullptr; }      // (an evaluation leaves both to the last training pass)
      adz = G.fn([=] { return launch_sac_actor_grad(ctx, sg); }, {adz});
    }
  }

  // ---- actor backward
  adz = add_fc_backward(G, a, a->ws[0], B, na - 1, adz, 0);
  }

  // ---- TD target + critic backward on the first evaluation (fed actions)
  const float* per_w = per.w;
  if (doC) cdz = G.fn([=] { return critic_td(d, b, B, train, per_w); }, {c0, tcH, c0b, tcHb});      // (twin: both heads of both critics; r_soft: job 2's, which tcH follows)
  if (doC && per.hook) G.fn(per.hook, {cdz});
  int cdz2 = cdz;      // head 2's chain down to the concat layer, level by level beside head 1's
  for (int l = nc - 1; l >= (c->ln ? 1 : 0) && doC && train; --l) {      // (a feature layer norm: layer 0 is add_ln_backward's)
    const FcL& L = c->fc[l];
    G.gemm(sq_gemm(ctx, 1, fc_dw_args(c, c->ws[0], l, B, c->ws[0].dz[l])), {cdz});
    const int ncols = L.cat ? L.n_in - A : L.n_in;
    if (twin && l >= cat) {
      G.gemm(sq_gemm(ctx, 1, twin_dw_args(c, c->ws[0], l, B)), {cdz2});
      if (l > cat) cdz2 = G.gemm(twin_dx_args(c, c->ws[0], l, B), {cdz2});
    }
    if (twin && l == cat && l > 0) {      // the shared layer's dz: (head 1) + (head 2), then the mask
      const int h1 = G.gemm(fc_dx_args(c, l, B, c->ws[0].dz[l], L.n_out, 0, ncols, c->ws[0].dz[l - 1], ncols, GE_NONE, nullptr, 0), {cdz});
      cdz = G.gemm(twin_dx_args(c, c->ws[0], l, B), {h1, cdz2});
    } else if (l == 1 && c->ln)      // g = dL/dy of the normalised layer: ln.hip owns its activation's derivative
      cdz = G.gemm(fc_dx_args(c, l, B, c->ws[0].dz[l], L.n_out, 0, ncols, c->ws[0].dz[0], ncols, GE_NONE, nullptr, 0), {cdz});
    else if (l > 0)
      cdz = G.gemm(fc_dx_args(c, l, B, c->ws[0].dz[l], L.n_out, 0, ncols, c->ws[0].dz[l - 1], ncols, GE_MUL_RELU_GRAD,
                              c->ws[0].fcin[l], L.n_in + 1), {cdz});
    else if (c->spec.pixel)
      cdz = G.gemm(fc_dx_args(c, 0, B, c->ws[0].dz[0], L.n_out, 0, c->flat, c->ws[0].dpool[2], c->flat, GE_NONE, nullptr, 0), {cdz});
  }
  if (a->ln) {      // the chains of the halves that ran a backward stopped at g = dL/dy of layer 0
    cpp_net* ln_nets[2]; int ln_deps[2], ln_lists[2], nn = 0;
    if (doA) { ln_nets[nn] = a; ln_deps[nn] = adz; ln_lists[nn++] = 0; }
    if (doC && train) { ln_nets[nn] = c; ln_deps[nn] = cdz; ln_lists[nn++] = 1; }
    if (nn) add_ln_backward(G, ctx, ln_nets, nn, ln_deps, ln_lists, B);
    nn = 0;
    if (doA) adz = ln_deps[nn++];
    if (doC && train) cdz = ln_deps[nn++];
  }
  }
  int conv_bwd = -1;
  if (c->spec.pixel && both) {     // both conv backward passes, layer by layer, two networks per launch
    cpp_net* bn[2] = {a, c};
    conv_bwd = G.fn([=] { return nets_backward_conv(ctx, bn, 2, B, s1, dt, w1); }, {adz, cdz});
  } else if (c->spec.pixel && (doA || train)) {      // one half: its trained network's
    cpp_net* n = doA ? a : c;
    conv_bwd = G.fn([=] { return net_backward_conv(n, n->ws[0], B, s1, dt, w1); }, {doA ? adz : cdz});
  }
  DwPendingGuard pending(ctx);      // (a failure below drops what was queued)
  if (phase == 2) {
    if (conv_bwd >= 0) RC(G.ops[conv_bwd].fn());
  } else {
    RC(G.run(ctx, phase == 1 ? conv_bwd : -1));
  }
  if (phase == 1) pending.keep();
  else RC(flush_dw_reduce(ctx));      // all six dW reductions (3 layers x 2 networks) in one launch
  left->counted = fused && (hd.step_bump != nullptr || hd.pd != nullptr);
  left->noise_owed = (d->tps_on || sac) && phase != 2 && doC && train;      // (this pass read the count: exactly one increment follows it)
  sq_scope.left(left->sq_cnt);
  if (doC) left->loss = critic_loss_at(d, B, fused);
  if (sac && doA && train) left->loss.sac_rows = B;
  return CPP_OK;
}

// The single ops are the pass with one half asked for.  The actor's half (ddpg_cartpole.py:111-113 + :220-222) ...
static int actor_half(cpp_ddpg* d, cpp_batch* b, bool train, PassLeft* left) {
  return compute_gradients(d, b, left, 0, false, PerPass(), PassParts{true, false, train});
}
// ... and the critic's (:199-214).  train == false is check_loss (:239-248), which feeds IS_TRAINING False; the train op (:237) feeds
// True for the whole graph, target networks included.  Set around the pass: its nodes read the flag while the graph is built
static int critic_gradients(cpp_ddpg* d, cpp_batch* b, bool train, PassLeft* left) {
  cpp_net* nets[3] = {d->critic, d->tactor, d->tcritic};
  for (cpp_net* n : nets) n->is_training = train;
  const int rc = compute_gradients(d, b, left, 0, false, PerPass(), PassParts{false, true, train});
  for (cpp_net* n : nets) n->is_training = true;
  return rc;
}

extern "C" int cpp_ddpg_train_actor(cpp_ddpg* d, cpp_batch* b) {
  RC(check_batch(d, b, "cpp_ddpg_train_actor"));
  HIP_CHECK(hipSetDevice(d->ctx->device));
  RC(prep_batch(d, b));
  OptPlan plan; plan.critic = false;
  RC(actor_half(d, b, true, &plan.pass));
  d->last.sac_rows = plan.pass.loss.sac_rows;
  return apply(d, plan);
}

extern "C" int cpp_ddpg_train_critic(cpp_ddpg* d, cpp_batch* b) {
  RC(check_batch(d, b, "cpp_ddpg_train_critic"));
  HIP_CHECK(hipSetDevice(d->ctx->device));
  RC(prep_batch(d, b));
  OptPlan plan; plan.actor = false;
  RC(critic_gradients(d, b, true, &plan.pass));
  d->last.parts = plan.pass.loss.parts; d->last.B = plan.pass.loss.B;
  return apply(d, plan);
}

extern "C" int cpp_ddpg_check_loss(cpp_ddpg* d, cpp_batch* b, float* loss, float* td, float* q) {
  RC(check_batch(d, b, "cpp_ddpg_check_loss"));
  HIP_CHECK(hipSetDevice(d->ctx->device));
  RC(prep_batch(d, b));
  PassLeft left;
  RC(critic_gradients(d, b, false, &left));
  d->last.parts = left.loss.parts; d->last.B = left.loss.B;      // (the evaluation's loss stands where a train op's would)
  double parts[DDPG_HEADS_MAX_WGS];      // (a distributional trainer: the cross-entropy from its per-workgroup partials, as cpp_ddpg_last_stats)
  const int nparts = left.loss.parts;
  const size_t nB = (size_t)b->B * sizeof(float);
  RC(read_back(d->ctx, {{loss && nparts ? parts : nullptr, d->heads_part, (size_t)nparts * sizeof(double)}, {nparts ? nullptr : loss, d->loss_norms, sizeof(float)},
                        {td, d->td, nB}, {q, d->critic->ws[0].out, nB}}));
  if (loss && nparts) *loss = loss_of_parts(parts, nparts, left.loss.B);
  return CPP_OK;
}

extern "C" int cpp_ddpg_q_gradients_wrt_actions(cpp_ddpg* d, cpp_batch* b, float* dq_da, float* actions, float* q) {
  RC(check_batch(d, b, "cpp_ddpg_q_gradients_wrt_actions"));
  HIP_CHECK(hipSetDevice(d->ctx->device));
  RC(prep_batch(d, b));
  PassLeft left;      // (an evaluation: nothing drawn, nothing left; the actor's backward runs all the same -- cpp_ddpg_grad_buffer shows it)
  RC(actor_half(d, b, false, &left));
  const size_t nB = (size_t)b->B * sizeof(float), nA = nB * d->actor->spec.action_dim;
  return read_back(d->ctx, {{dq_da, d->dq_da, nA}, {actions, d->actor->ws[0].out, nA}, {q, d->critic->ws[1].out, nB}});
}

extern "C" int cpp_ddpg_compute_gradients(cpp_ddpg* d, cpp_batch* b) {
  RC(check_batch(d, b, "cpp_ddpg_compute_gradients"));
  HIP_CHECK(hipSetDevice(d->ctx->device));
  RC(prep_batch(d, b));
  PassLeft left;
  RC(compute_gradients(d, b, &left));
  d->last = left.loss;
  return tps_settle(d, left);
}

extern "C" int cpp_ddpg_grad_buffer(cpp_ddpg* d, void** p, int64_t* n) {
  ARG_CHECK(d && p && n, "cpp_ddpg_grad_buffer: NULL argument");
  *p = d->gradbuf; *n = d->nA + d->nC;
  return CPP_OK;
}

extern "C" int cpp_ddpg_apply_gradients(cpp_ddpg* d, float grad_scale) {
  ARG_CHECK(d, "cpp_ddpg_apply_gradients: NULL argument");
  HIP_CHECK(hipSetDevice(d->ctx->device));
  OptPlan plan; plan.grad_scale = grad_scale;
  plan.pass.loss.sac_rows = d->last.sac_rows;      // (the temperature's gradient of the pass cpp_ddpg_compute_gradients ran)
  return apply(d, plan);
}

// ddpg_cartpole.py:118-119 and :218 build the two train ops with tf.train.GradientDescentOptimizer; util.py:73-76 is the reference's
// rule for every other optimiser (tf.train.<name>Optimizer): Momentum and Adam with TensorFlow's semantics, one optimiser per list.
// Allocates and zeroes the slots (m; v for Adam) over gradbuf's layout, zeroes both step counts, drops the cached graphs.
extern "C" int cpp_ddpg_set_optimiser(cpp_ddpg* d, int kind, float momentum, float beta1, float beta2, float epsilon) {
  ARG_CHECK(d, "cpp_ddpg_set_optimiser: NULL argument");
  ARG_CHECK(kind >= CPP_OPT_SGD && kind <= CPP_OPT_ADAM, "cpp_ddpg_set_optimiser: optimiser %d", kind);
  ARG_CHECK(kind != CPP_OPT_MOMENTUM || (momentum >= 0.f && momentum < 1e30f), "cpp_ddpg_set_optimiser: momentum %g", (double)momentum);
  ARG_CHECK(kind != CPP_OPT_ADAM || (beta1 >= 0.f && beta1 < 1.f && beta2 >= 0.f && beta2 < 1.f && epsilon > 0.f && epsilon < 1e30f),
            "cpp_ddpg_set_optimiser: beta1 %g, beta2 %g (both in [0, 1)), epsilon %g (> 0)", (double)beta1, (double)beta2, (double)epsilon);
  cpp_ctx* ctx = d->ctx;
  HIP_CHECK(hipSetDevice(ctx->device));
  HIP_CHECK(ctx_sync_stream(ctx));
  const size_t n = (size_t)(d->nA + d->nC);
  if (kind != CPP_OPT_SGD && !d->opt_m) RC(dalloc(d->arena, &d->opt_m, n));
  if (kind == CPP_OPT_ADAM && !d->opt_v) RC(dalloc(d->arena, &d->opt_v, n));
  if (kind != CPP_OPT_SGD && !d->opt_step) RC(dalloc(d->arena, &d->opt_step, (size_t)2));
  if (d->opt_m) HIP_CHECK(hipMemsetAsync(d->opt_m, 0, n * sizeof(float), ctx->stream));
  if (d->opt_v) HIP_CHECK(hipMemsetAsync(d->opt_v, 0, n * sizeof(float), ctx->stream));
  if (d->opt_step) HIP_CHECK(hipMemsetAsync(d->opt_step, 0, 2 * sizeof(uint64_t), ctx->stream));
  HIP_CHECK(ctx_sync_stream(ctx));
  d->opt_kind = kind; d->opt_momentum = momentum; d->opt_beta1 = beta1; d->opt_beta2 = beta2; d->opt_epsilon = epsilon;
  reconfigured(d);      // (the captured launches carry the old rule)
  return CPP_OK;
}

// Target policy smoothing of the critic's target (an extension of ddpg_cartpole.py:199-209; include/cartpolepp_abi.h).  sigma, clip and
// the seed are captured by value: the call drops the cached graphs, and it zeroes the count.
extern "C" int cpp_ddpg_set_target_smoothing(cpp_ddpg* d, float sigma, float clip, uint64_t seed) {
  ARG_CHECK(d, "cpp_ddpg_set_target_smoothing: NULL argument");
  ARG_CHECK(sigma >= 0.f && sigma < 1e30f && clip >= 0.f && clip < 1e30f, "cpp_ddpg_set_target_smoothing: sigma %g, clip %g (both finite, >= 0)",
            (double)sigma, (double)clip);
  ARG_CHECK(!(sigma > 0.f && clip == 0.f), "cpp_ddpg_set_target_smoothing: sigma %g with clip 0 (the noise would be clipped away)", (double)sigma);
  ARG_CHECK(!(sigma == 0.f && clip > 0.f), "cpp_ddpg_set_target_smoothing: clip %g without a noise (sigma 0, clip 0 switches smoothing off)", (double)clip);
  ARG_CHECK(!(d->sac && sigma > 0.f), "cpp_ddpg_set_target_smoothing: a soft actor-critic trainer (its target action is a sample already)");
  if (d->sac) return CPP_OK;      // ("off" on a soft actor-critic trainer: the count word is its noise stream's and stays as it is)
  cpp_ctx* ctx = d->ctx;
  HIP_CHECK(hipSetDevice(ctx->device));
  HIP_CHECK(ctx_sync_stream(ctx));
  const size_t n = (size_t)d->maxB * d->actor->spec.action_dim;
  if (sigma > 0.f && !d->tps_n) RC(dalloc(d->arena, &d->tps_n, (size_t)2));
  if (sigma > 0.f && !d->tps_eps) RC(dalloc(d->arena, &d->tps_eps, n));
  if (d->tps_n) HIP_CHECK(hipMemsetAsync(d->tps_n, 0, 2 * sizeof(uint64_t), ctx->stream));
  if (d->tps_eps) HIP_CHECK(hipMemsetAsync(d->tps_eps, 0, n * sizeof(float), ctx->stream));
  HIP_CHECK(ctx_sync_stream(ctx));
  d->tps_on = sigma > 0.f; d->tps_sigma = sigma; d->tps_clip = clip; d->tps_seed = seed;
  reconfigured(d);      // (the captured launches carry the old values, or none)
  return CPP_OK;
}

// Delayed policy updates (TD3: Fujimoto et al. 2018, Algorithm 1; an extension of ddpg_cartpole.py:332-337; include/cartpolepp_abi.h).  The
// delay is captured by value: the call drops the cached graphs, and it zeroes the count.  delay 1 is off: no launch carries the words.
extern "C" int cpp_ddpg_set_policy_delay(cpp_ddpg* d, int delay) {
  ARG_CHECK(d, "cpp_ddpg_set_policy_delay: NULL argument");
  ARG_CHECK(delay >= 1 && delay <= 65536, "cpp_ddpg_set_policy_delay: delay %d outside [1, 65536]", delay);
  ARG_CHECK(!(d->sac && delay > 1), "cpp_ddpg_set_policy_delay: a soft actor-critic trainer updates its policy in every minibatch");
  cpp_ctx* ctx = d->ctx;
  HIP_CHECK(hipSetDevice(ctx->device));
  HIP_CHECK(ctx_sync_stream(ctx));
  if (delay > 1 && !d->pd) RC(dalloc(d->arena, &d->pd, (size_t)PD_WORDS));
  if (d->pd) HIP_CHECK(hipMemsetAsync(d->pd, 0, PD_WORDS * sizeof(uint64_t), ctx->stream));
  HIP_CHECK(ctx_sync_stream(ctx));
  d->pd_d = delay;
  reconfigured(d);      // (the captured launches carry the old delay, or none)
  return CPP_OK;
}

// The actor on the minimum head (TD3 / DrQ-v2 / SAC's actor objective on twin critics: min(Q1, Q2) at the policy's action; an extension of
// ddpg_cartpole.py:111-113, :220-222; include/cartpolepp_abi.h).  The switch is captured by the launches: the call drops the cached graphs.
extern "C" int cpp_ddpg_set_actor_min_q(cpp_ddpg* d, int on) {
  ARG_CHECK(d, "cpp_ddpg_set_actor_min_q: NULL argument");
  ARG_CHECK(d->twin, "cpp_ddpg_set_actor_min_q: both critics must carry twin Q heads (cpp_net_create_twin_q)");
  cpp_ctx* ctx = d->ctx;
  HIP_CHECK(hipSetDevice(ctx->device));
  HIP_CHECK(ctx_sync_stream(ctx));
  if (on && !d->amin_sel) RC(dalloc(d->arena, &d->amin_sel, (size_t)d->maxB));
  d->amin = on != 0;
  reconfigured(d);      // (the captured launches carry the other family of heads instances, or the other GEMM levels)
  return CPP_OK;
}

extern "C" int cpp_ddpg_last_actor_min(cpp_ddpg* d, int B, float* q1, float* q2, int32_t* sel) {
  ARG_CHECK(d, "cpp_ddpg_last_actor_min: NULL argument");
  ARG_CHECK(B >= 1 && B <= d->maxB, "cpp_ddpg_last_actor_min: batch %d outside [1,%d]", B, d->maxB);
  if (!d->amin) { cpp_set_error("cpp_ddpg_last_actor_min: the actor follows Q1 (cpp_ddpg_set_actor_min_q is off)"); return CPP_ERR_STATE; }
  HIP_CHECK(hipSetDevice(d->ctx->device));
  const size_t n = (size_t)B * sizeof(float);
  return read_back(d->ctx, {{q1, d->critic->ws[1].out, n}, {q2, d->critic->ws[1].out2, n}, {sel, d->amin_sel, (size_t)B * sizeof(int32_t)}}, true);
}

// The behaviour-cloning actor term (TD3+BC, Fujimoto & Gu 2021: the actor ascends lambda Q and regresses onto the minibatch's stored action;
// an extension of ddpg_cartpole.py:111-113; include/cartpolepp_abi.h).  Alpha and the floor are captured by value: the call drops the cached
// graphs.  alpha 0 is off: the trainer cpp_ddpg_create left.
extern "C" int cpp_ddpg_set_behaviour_cloning(cpp_ddpg* d, float alpha, float q_floor) {
  ARG_CHECK(d, "cpp_ddpg_set_behaviour_cloning: NULL argument");
  ARG_CHECK(alpha >= 0.f && alpha < 1e30f && q_floor > 0.f && q_floor < 1e30f,
            "cpp_ddpg_set_behaviour_cloning: alpha %g (finite, >= 0; 0 is off), q_floor %g (finite, > 0)", (double)alpha, (double)q_floor);
  ARG_CHECK(!d->dist_n, "cpp_ddpg_set_behaviour_cloning: a distributional or quantile critic");
  ARG_CHECK(!d->sac, "cpp_ddpg_set_behaviour_cloning: a soft actor-critic trainer (its actor's head is a Gaussian's)");
  cpp_ctx* ctx = d->ctx;
  HIP_CHECK(hipSetDevice(ctx->device));
  HIP_CHECK(ctx_sync_stream(ctx));
  if (alpha > 0.f && !d->bc_stat) {
    const size_t n = (size_t)d->maxB * d->actor->spec.action_dim;
    RC(dalloc(d->arena, &d->bc_stat, (size_t)2));
    RC(dalloc(d->arena, &d->bc_g, n));
    RC(dalloc(d->arena, &d->bc_rows, (size_t)d->maxB));
    HIP_CHECK(ctx_sync_stream(ctx));      // (the arena zeroes what it hands out)
  }
  d->bc_alpha = alpha; d->bc_floor = q_floor;
  reconfigured(d);      // (the captured launches carry the fused heads, or the other alpha)
  return CPP_OK;
}

extern "C" int cpp_ddpg_last_behaviour_cloning(cpp_ddpg* d, int B, float* lambda, float* m, float* g, float* bc_rows) {
  ARG_CHECK(d, "cpp_ddpg_last_behaviour_cloning: NULL argument");
  ARG_CHECK(B >= 1 && B <= d->maxB, "cpp_ddpg_last_behaviour_cloning: batch %d outside [1,%d]", B, d->maxB);
  if (!(d->bc_alpha > 0.f)) { cpp_set_error("cpp_ddpg_last_behaviour_cloning: behaviour cloning is off (cpp_ddpg_set_behaviour_cloning)"); return CPP_ERR_STATE; }
  HIP_CHECK(hipSetDevice(d->ctx->device));
  const size_t nB = (size_t)B * sizeof(float);
  return read_back(d->ctx, {{lambda, d->bc_stat, sizeof(float)}, {m, d->bc_stat + 1, sizeof(float)},
                            {g, d->bc_g, nB * d->actor->spec.action_dim}, {bc_rows, d->bc_rows, nB}}, true);
}

extern "C" int cpp_ddpg_policy_delay_status(cpp_ddpg* d, int* delay, uint64_t* n, int* held) {
  ARG_CHECK(d, "cpp_ddpg_policy_delay_status: NULL argument");
  uint64_t w[PD_WORDS] = {0, 0, 0};
  if (d->pd) {
    HIP_CHECK(hipSetDevice(d->ctx->device));
    HIP_CHECK(hipMemcpyAsync(w, d->pd, sizeof(w), hipMemcpyDeviceToHost, d->ctx->stream));
    HIP_CHECK(ctx_sync_stream(d->ctx));
  }
  if (delay) *delay = d->pd_d;
  if (n) *n = w[PD_N];
  if (held) *held = (d->pd_d > 1 && w[PD_HOLD]) ? 1 : 0;
  return CPP_OK;
}

extern "C" int cpp_ddpg_last_target_noise(cpp_ddpg* d, int B, float* eps, uint64_t* n) {
  ARG_CHECK(d, "cpp_ddpg_last_target_noise: NULL argument");
  ARG_CHECK(B >= 1 && B <= d->maxB, "cpp_ddpg_last_target_noise: batch %d outside [1,%d]", B, d->maxB);
  if (!d->tps_on) { cpp_set_error("cpp_ddpg_last_target_noise: target policy smoothing is off"); return CPP_ERR_STATE; }
  HIP_CHECK(hipSetDevice(d->ctx->device));
  return read_back(d->ctx, {{eps, d->tps_eps, (size_t)B * d->actor->spec.action_dim * sizeof(float)}, {n, d->tps_n + 1, sizeof(uint64_t)}}, true);
}

// the slots and the two step counts for checkpoints (util.py:88-90: tf.train.Saver saves the slot variables of both 'optimiser' scopes,
// ddpg_cartpole.py:118, :218).  n = actor + critic parameters; m / v: the actor's list, then the critic's; v is left alone unless Adam.
extern "C" int64_t cpp_ddpg_opt_state_size(const cpp_ddpg* d) { return d ? (int64_t)(d->nA + d->nC) : -1; }
extern "C" int cpp_ddpg_get_opt_state(cpp_ddpg* d, float* m, float* v, int64_t n, uint64_t steps[2]) {
  ARG_CHECK(d && steps, "cpp_ddpg_get_opt_state: NULL argument");
  ARG_CHECK(d->opt_kind != OPT_SGD, "cpp_ddpg_get_opt_state: GradientDescent has no slots");
  ARG_CHECK(n == d->nA + d->nC, "cpp_ddpg_get_opt_state: asked %ld values, the optimisers have %ld", (long)n, d->nA + d->nC);
  HIP_CHECK(hipSetDevice(d->ctx->device));
  return read_back(d->ctx, {{m, d->opt_m, (size_t)n * sizeof(float)}, {d->opt_kind == OPT_ADAM ? v : nullptr, d->opt_v, (size_t)n * sizeof(float)},
                            {steps, d->opt_step, 2 * sizeof(uint64_t)}}, true);
}
extern "C" int cpp_ddpg_set_opt_state(cpp_ddpg* d, const float* m, const float* v, int64_t n, const uint64_t steps[2]) {
  ARG_CHECK(d && m && steps, "cpp_ddpg_set_opt_state: NULL argument");
  ARG_CHECK(d->opt_kind != OPT_SGD, "cpp_ddpg_set_opt_state: GradientDescent has no slots");
  ARG_CHECK(d->opt_kind != OPT_ADAM || v, "cpp_ddpg_set_opt_state: Adam needs v");
  ARG_CHECK(n == d->nA + d->nC, "cpp_ddpg_set_opt_state: got %ld values, the optimisers have %ld", (long)n, d->nA + d->nC);
  HIP_CHECK(hipSetDevice(d->ctx->device));
  hipStream_t st = d->ctx->stream;
  HIP_CHECK(hipMemcpyAsync(d->opt_m, m, (size_t)n * sizeof(float), hipMemcpyHostToDevice, st));
  if (d->opt_kind == OPT_ADAM) HIP_CHECK(hipMemcpyAsync(d->opt_v, v, (size_t)n * sizeof(float), hipMemcpyHostToDevice, st));
  HIP_CHECK(hipMemcpyAsync(d->opt_step, steps, 2 * sizeof(uint64_t), hipMemcpyHostToDevice, st));
  HIP_CHECK(ctx_sync_stream(d->ctx));
  return CPP_OK;
}

// publish_route: the launch closes a training call -- it also publishes the call's largest whitening scale and resets the scale word
static int soft_update_targets(cpp_ddpg* d, bool publish_route) {
  HIP_CHECK(hipSetDevice(d->ctx->device));
  d->tactor->wimg_key = nullptr; d->tcritic->wimg_key = nullptr;
  return launch_soft_update(d->ctx, d->tactor->params, d->actor->params, d->nA, d->tcritic->params, d->critic->params,
                            d->nC, d->hp.target_update_rate, publish_route);
}
extern "C" int cpp_ddpg_update_targets(cpp_ddpg* d) {
  ARG_CHECK(d, "cpp_ddpg_update_targets: NULL argument");
  return soft_update_targets(d, false);
}

// The fused step does not need a gathered copy of the minibatch when conv1 runs on the f16-pipe kernels: they take the
// replay store plus the sampled slots (the gather kernel then only reads -- statistics -- and writes 2 B ints).
// CPP_DIRECT_REPLAY=0 keeps the copy.  So does a memory with random shift on (cpp_replay_set_random_shift): the shifted images exist
// only in the gathered copy.
bool direct_replay_ok(cpp_net* a, cpp_replay* r, int B) {
  static const bool off = cpp_switch_off("CPP_DIRECT_REPLAY");
  if (off || !a->spec.pixel || r->store_dtype != CPP_F16 || r->shift_pad > 0) return false;
  const int C = a->spec.C;
  int g = 8, c = C; while (c) { int t = g % c; g = c; c = t; }
  if (r->elems % 8 != 0 || C / g > 16 || r->elems % C != 0) return false;       // statistics come from the gather kernel
  return conv1_f16_pipes_ok(a->ctx, C, a->conv[0].H, a->conv[0].W, B, a->spec.use_batch_norm != 0);
}

// The inner step ddpg_cartpole.py:331-337: the shared minibatch loop (rt_step.cpp: run_minibatches -- the sample rider, the prioritized
// draws), then the target updates.  On a prioritized memory the optimiser's launch moves the sampler's counter, as on a uniform one.
// dp: this rank's part of the data-parallel step (cpp_ddpg_dp_train_step): between a minibatch's gradients and its update the flat
// gradient buffer is summed over the ranks (comm; NULL: a single learner on the same path) and the update takes the mean -- the
// all-reduce is issued on the context's stream, i.e. it is PART OF THE CAPTURED GRAPH (RCCL's kernels capture like any other).
static int step_body(cpp_ddpg* d, cpp_replay* r, int B, int n_batches, const int32_t* rows_dev, uint64_t seed, bool targets = true,
                     bool dp = false, cpp_comm* comm = nullptr) {
  d->pre_variant = 0;        // (the half steps' presampled minibatch lives in the same step_batch)
  cpp_ctx* ctx = d->ctx;
  MinibatchLoop L;
  L.ctx = ctx; L.r = r; L.step_batch = d->step_batch; L.trunk = d->actor;
  L.td = d->td; L.stats_switch = true;
  L.gradients = [=](const PerPass& per, PassLeft* left) {
    RC(compute_gradients(d, d->step_batch, left, 0, true, per));      // (the apply() behind it takes both lists)
    d->last = left->loss;
    return (int)CPP_OK;
  };
  bool targets_left = false;
  L.apply = [=, &targets_left](bool more, const NextBatch& next, const PassLeft& left) {
    // (dp: the norm is the reduced gradient's -- the partials the gradient kernels folded in are this rank's only: sumsq runs)
    if (dp) RC(step_allreduce(ctx, comm, d->gradbuf, (size_t)(d->nA + d->nC)));
    static const bool no_tgt_ride = cpp_switch_off("CPP_RIDE_TARGETS");
    OptPlan plan;
    plan.grad_scale = (dp && comm) ? 1.0f / (float)comm->world : 1.0f; plan.bump = rows_dev ? nullptr : r->counter; plan.folded = !dp;
    plan.next = next; plan.pass = left;
    plan.closes_step = !more && targets && !dp && !no_tgt_ride;      // (the last minibatch of an outer step: the target updates ride in its optimiser launch)
    plan.closes_call = !more && (!targets || plan.closes_step);      // (... which then closes the call)
    return apply(d, plan, &targets_left);
  };
  RC(run_minibatches(L, B, n_batches, rows_dev, seed));
  if (!targets || targets_left) return CPP_OK;      // (both target updates and the route's publish left with the optimiser's launch)
  return soft_update_targets(d, true);      // (the largest whitening scale of this step rides to the host in that launch)
}

// ddpg_cartpole.py:332-334 for ONE minibatch whose rows the HOST drew (replay_memory.random_indexes: numpy's RNG, :123-129):
// sample + gather of exactly those rows, actor update, critic update -- the fused minibatch of cpp_ddpg_train_step, without the
// target updates (the caller's loop runs them after `batches_per_step` minibatches, :336-337: cpp_net_soft_update).  This is what
// `actor.train(batch.state_1); critic.train(batch)` of the reference's loop becomes (cartpoleplusplus_amd/ddpg_cartpole.py defers the
// actor's call until the critic's arrives).  One hipGraph per (B, replay); the rows travel through pinned memory, so the call
// returns while the previous minibatch is still running.
extern "C" int cpp_ddpg_train_rows(cpp_ddpg* d, cpp_replay* r, int B, const int32_t* idxs) {
  ARG_CHECK(d && r && idxs, "cpp_ddpg_train_rows: NULL argument");
  RC(train_entry_checks("cpp_ddpg_train_rows", r, B, d->maxB, d->actor->state_elems, d->actor->spec.action_dim, d->hp.discount));
  route_check(d);
  cpp_ctx* ctx = d->ctx;
  HIP_CHECK(hipSetDevice(ctx->device));
  if (!d->step_batch) RC(cpp_batch_create(ctx, d->maxB, r->elems, r->A, &d->step_batch));
  RC(replay_stage_rows(r, idxs, B, "cpp_ddpg_train_rows"));
  static const bool no_graph = cpp_switch_set("CPP_NO_GRAPH");
  StepRan how;
  const int rc = run_step_graph(ctx, d->rgraph, GraphKey{B, 1, 0, r->uid, 0, d->graph_gen}, [&] { return step_body(d, r, B, 1, r->rows_in, 0, false); }, &how, no_graph);
  return step_ran(d, d->rgraph, rc, how);
}

extern "C" int cpp_ddpg_train_step(cpp_ddpg* d, cpp_replay* r, int B, int n_batches, const int32_t* idxs, uint64_t seed) {
  ARG_CHECK(d && r, "cpp_ddpg_train_step: NULL argument");
  RC(train_entry_checks("cpp_ddpg_train_step", r, B, d->maxB, d->actor->state_elems, d->actor->spec.action_dim, d->hp.discount, &n_batches));
  route_check(d);
  cpp_ctx* ctx = d->ctx;
  HIP_CHECK(hipSetDevice(ctx->device));
  if (!d->step_batch) RC(cpp_batch_create(ctx, d->maxB, r->elems, r->A, &d->step_batch));
  if (idxs) {
    RC(replay_upload_rows(r, idxs, n_batches * B, "cpp_ddpg_train_step"));
    return step_body(d, r, B, n_batches, r->rows_in, seed);
  }
  static const bool no_graph = cpp_switch_set("CPP_NO_GRAPH");   // plain in-order stream launches (A/B measurements)
  StepRan how;
  const int rc = run_step_graph(ctx, d->graph, GraphKey{B, n_batches, seed, r->uid, 0, d->graph_gen}, [&] { return step_body(d, r, B, n_batches, nullptr, seed); }, &how, no_graph);
  return step_ran(d, d->graph, rc, how);
}

// variant 0: sample + gather + statistics of this call's minibatch; 1 / 2: it was presampled by the previous call's rider into
// slot set 1 / 0 (only its whitening tables are still to do).  Every variant tries to send the NEXT minibatch's sample pass
// along with conv1's dW (the sampler's counter has been advanced by then, so the rider draws with the counter as it stands);
// *next: the variant the following call must use.  CPP_RIDE_DP=0 (ablation build): always variant 0, no rider.
// phase 0: the whole half step; 1: up to the conv backward; 2: the conv backward (with the rider) + dW reductions.
static int half_step_body(cpp_ddpg* d, cpp_replay* r, int B, uint64_t seed, int variant, int* next, int phase) {
  const int C = d->actor->spec.pixel ? d->actor->spec.C : 0;
  cpp_ctx* ctx = d->ctx;
  cpp_batch* b = d->step_batch;
  const bool direct = direct_replay_ok(d->actor, r, B);
  static const bool no_ride = cpp_switch_off("CPP_RIDE_DP");
  const int cur = variant == 1 ? 1 : 0;
  for (int k = 0; k < 2; ++k) { b->slot[k] = d->slot_set[cur][k]; b->slot_alt[k] = d->slot_set[1 - cur][k]; }
  int Cg = 0;
  GatherArgs ga = replay_gather_args(r, B, nullptr, seed, r->counter, C, b, direct, &Cg);
  if (phase != 2) {
    if (variant == 0) RC(launch_gather_stats(ctx, ga, r->store_dtype));
    bool bumped = false;
    RC(replay_sample_finish(r, B, Cg, C, b, r->counter, &bumped));
    if (!bumped) RC(launch_counter_add(ctx, r->counter, 1));
  }
  PassLeft left;
  if (phase == 1) { RC(compute_gradients(d, b, &left, 1)); d->last = left.loss; return tps_settle(d, left); }
  const bool ride_ok = !no_ride && direct && Cg > 0 && r->store_dtype == CPP_F16;
  int rc;
  {
    RideScope ride(ctx);
    if (ride_ok) ride.arm(&ga, b, r->store_dtype, true, true);
    rc = compute_gradients(d, b, &left, phase);
    *next = ride.rode() ? (cur == 0 ? 1 : 2) : 0;
  }
  if (rc) return rc;
  d->last = left.loss;
  RC(tps_settle(d, left));      // (phase 2 reads no count and owes nothing)
  return ctx_route_publish(ctx);
}

// One half step: sample (or find presampled) a minibatch and leave both gradient sets in the flat buffer.  hipGraph replay after
// the first call per (variant, B, seed, replay).  split: two graphs per variant, `between` is called on the host between their
// launches (the data-parallel step starts the all-reduce of the fully connected layers' gradients there).
static int half_step(cpp_ddpg* d, cpp_replay* r, int B, uint64_t seed, bool split, const std::function<int()>& between) {
  cpp_ctx* ctx = d->ctx;
  if (!d->step_batch) RC(cpp_batch_create(ctx, d->maxB, r->elems, r->A, &d->step_batch));
  if (d->slot_set[0][0] == nullptr)
    for (int k = 0; k < 2; ++k) { d->slot_set[0][k] = d->step_batch->slot[k]; d->slot_set[1][k] = d->step_batch->slot_alt[k]; }
  const GraphKey key{B, 0, seed, r->uid, 0, d->graph_gen};
  if (!(d->half_key == key)) {                       // another batch size / seed / memory, or invalidated: start over
    for (auto& F : d->hg) for (auto& variant : F.g) for (StepGraph& g : variant) g.drop();
    d->pre_variant = 0;
    d->half_key = key;
  }
  // a minibatch the previous call's rider presampled is only good while the memory is as it was: an episode added since may have
  // overwritten its rows or recycled their state slots (the slots are read at step time).  Draw again (same counter, new contents).
  if (d->h_write_gen != r->write_gen) { d->pre_variant = 0; d->h_write_gen = r->write_gen; }
  cpp_ddpg::HalfGraphs& H = d->hg[split ? 1 : 0];
  const int v = d->pre_variant;
  d->pre_variant = 0;                                // (stays 0 if anything below fails)
  auto eager = [&](int variant, int* nx) -> int {
    if (!split) return half_step_body(d, r, B, seed, variant, nx, 0);
    RC(half_step_body(d, r, B, seed, variant, nx, 1));
    if (between) RC(between());
    return half_step_body(d, r, B, seed, variant, nx, 2);
  };
  const int parts = split ? 2 : 1;
  auto capture = [&](int variant, int* nx) -> int {
    for (int k = 0; k < parts; ++k)
      RC(H.g[variant][k].capture(ctx, key, [&] { return half_step_body(d, r, B, seed, variant, nx, split ? k + 1 : 0); }));
    H.g[variant][parts - 1].left = d->last;      // (the record of the body just captured: its replays put it back)
    return CPP_OK;
  };
  int next = 0;
  if (ctx->prof) { RC(eager(v, &next)); d->pre_variant = next; return CPP_OK; }
  if (!H.g[v][parts - 1].hit(key)) {                 // (the last part is captured last: a variant is there whole or not at all)
    // Variants 1 / 2 consume a presampled minibatch: their work must be done by the captured graph's first launch (an eager
    // pass would consume it and leave another one behind).  Kernel attributes (LDS sizes: not allowed during capture) are set
    // by variant 0's eager pass, which is also that call's work.
    int nx = 0;
    if (v == 0) {
      RC(eager(0, &next));
      HIP_CHECK(ctx_sync_stream(ctx));
      RC(capture(0, &nx));
      H.next[0] = nx;
      d->pre_variant = next;
      return CPP_OK;
    }
    HIP_CHECK(ctx_sync_stream(ctx));
    RC(capture(v, &nx));
    H.next[v] = nx;
  }
  RC(H.g[v][0].launch(ctx));
  if (split) {
    if (between) RC(between());
    RC(H.g[v][1].launch(ctx));
  }
  d->last = H.g[v][parts - 1].left;
  d->pre_variant = H.next[v];
  return CPP_OK;
}

// the data-parallel entry points: g_alpha is not in the flat gradient buffer the ranks reduce
static int sac_refuse(const cpp_ddpg* d, const char* who) {
  ARG_CHECK(!(d && d->sac), "%s: a soft actor-critic trainer has no data-parallel step (the temperature's gradient is not in the reduced buffer)", who);
  return CPP_OK;
}
static int half_step_checks(cpp_ddpg* d, cpp_replay* r, int B, const char* who) {
  ARG_CHECK(d && r, "%s: NULL argument", who);
  return train_entry_checks(who, r, B, d->maxB, d->actor->state_elems, d->actor->spec.action_dim, d->hp.discount, nullptr, false);
}

extern "C" int cpp_ddpg_sample_and_compute(cpp_ddpg* d, cpp_replay* r, int B, uint64_t seed) {
  RC(sac_refuse(d, "cpp_ddpg_sample_and_compute"));
  RC(per_refuse(r, "cpp_ddpg_sample_and_compute"));
  if (d) route_check(d);
  RC(half_step_checks(d, r, B, "cpp_ddpg_sample_and_compute"));
  RC(nstep_refuse(r, d->hp.discount, "cpp_ddpg_sample_and_compute"));
  HIP_CHECK(hipSetDevice(d->ctx->device));
  return half_step(d, r, B, seed, false, nullptr);
}

// ---- collectives of the data-parallel learners (communicator: rt_comm.cpp) --------------------------------------
// the flat gradient buffer is [actor conv | actor fc | critic conv | critic fc]: offsets of the two fc parts
static long fc_start(const cpp_net* n) { return n->fc[0].w_off; }

extern "C" int cpp_ddpg_allreduce_grads(cpp_ddpg* d, cpp_comm* c) {
  ARG_CHECK(d && c, "cpp_ddpg_allreduce_grads: NULL argument");
  RC(sac_refuse(d, "cpp_ddpg_allreduce_grads"));
  ARG_CHECK(c->ctx == d->ctx, "cpp_ddpg_allreduce_grads: communicator and networks live on different contexts");
  HIP_CHECK(hipSetDevice(d->ctx->device));
  NCCL_CHECK(ncclAllReduce(d->gradbuf, d->gradbuf, (size_t)(d->nA + d->nC), ncclFloat, ncclSum, c->comm, d->ctx->stream));
  return CPP_OK;
}

// periodic mode: replicas that took k local steps meet again at the mean of their parameters (targets included: they are
// functions of the parameter history and would otherwise drift apart)
extern "C" int cpp_ddpg_average_params(cpp_ddpg* d, cpp_comm* c) {
  ARG_CHECK(d && c, "cpp_ddpg_average_params: NULL argument");
  RC(sac_refuse(d, "cpp_ddpg_average_params"));
  ARG_CHECK(c->ctx == d->ctx, "cpp_ddpg_average_params: communicator and networks live on different contexts");
  HIP_CHECK(hipSetDevice(d->ctx->device));
  cpp_net* nets[4] = {d->actor, d->critic, d->tactor, d->tcritic};
  NCCL_CHECK(ncclGroupStart());
  for (cpp_net* n : nets)
    NCCL_CHECK(ncclAllReduce(n->params, n->params, (size_t)n->nparams, ncclFloat, ncclAvg, c->comm, d->ctx->stream));
  // (the optimiser slots meet at their mean too, as rt_naf.cpp's: the step counts are equal on every rank)
  if (d->opt_kind != OPT_SGD) NCCL_CHECK(ncclAllReduce(d->opt_m, d->opt_m, (size_t)(d->nA + d->nC), ncclFloat, ncclAvg, c->comm, d->ctx->stream));
  if (d->opt_kind == OPT_ADAM) NCCL_CHECK(ncclAllReduce(d->opt_v, d->opt_v, (size_t)(d->nA + d->nC), ncclFloat, ncclAvg, c->comm, d->ctx->stream));
  NCCL_CHECK(ncclGroupEnd());
  d->dp_local = 0;
  return CPP_OK;
}

// The inner step ddpg_cartpole.py:331-337 for N synchronous learners (this rank's part).  Per minibatch: sample from the own
// replay shard + both gradient sets (hipGraph) -> sum over the ranks of the flat gradient buffer -> clip + SGD on the mean on
// every rank (identical inputs: the replicas stay bit-identical without a broadcast).  sync_every = k > 1 ("periodic"): k local
// minibatch updates, then the parameters are averaged.  overlap: the gradients of the fully connected layers (93 % of the
// buffer) are reduced on a second stream while the conv backward of the same minibatch runs; the conv layers' follow.
// comm == NULL: a single learner taking the same path (tests).  Whitening statistics and target updates are local.
extern "C" int cpp_ddpg_dp_train_step(cpp_ddpg* d, cpp_replay* r, cpp_comm* c, int B, int n_batches, uint64_t seed,
                                      int sync_every, int overlap) {
  RC(sac_refuse(d, "cpp_ddpg_dp_train_step"));
  RC(per_refuse(r, "cpp_ddpg_dp_train_step"));
  RC(half_step_checks(d, r, B, "cpp_ddpg_dp_train_step"));
  RC(nstep_refuse(r, d->hp.discount, "cpp_ddpg_dp_train_step"));
  ARG_CHECK(n_batches >= 1 && sync_every >= 1, "cpp_ddpg_dp_train_step: n_batches %d, sync_every %d", n_batches, sync_every);
  ARG_CHECK(!c || c->ctx == d->ctx, "cpp_ddpg_dp_train_step: communicator and networks live on different contexts");
  route_check(d);
  cpp_ctx* ctx = d->ctx;
  HIP_CHECK(hipSetDevice(ctx->device));
  const float inv = c ? 1.0f / (float)c->world : 1.0f;
  const long fa = fc_start(d->actor), fcr = fc_start(d->critic);
  static const bool no_dp_graph = cpp_switch_off("CPP_DP_GRAPH");
  if (sync_every == 1 && !overlap && !no_dp_graph) {
    // The default mode as ONE hipGraph per outer step (round 4): sample -> gradients -> ncclAllReduce -> norm -> clip + SGD for each of
    // the n_batches minibatches, then the target updates -- the single learner's fused step (step_body) with the collective and the
    // norm of the REDUCED gradient inside.  No host launch, copy or fill per minibatch; the sample pass of minibatch i + 1 rides in
    // i's conv1 dW as in the fused step.  (Rounds 2-3: one graph per half step, the all-reduce, sumsq and the optimiser as host
    // launches per minibatch: 0.946 of the fused step at world size 1.)
    if (!d->step_batch) RC(cpp_batch_create(ctx, d->maxB, r->elems, r->A, &d->step_batch));
    // (No N > 1 box has run this yet: a refused capture leaves the same sequence as stream launches -- rt_internal.h, DpGraph)
    StepRan how;
    const int rc = run_dp_graph(ctx, d->dgraph, GraphKey{B, n_batches, seed, r->uid, c ? c->uid : 0, d->graph_gen}, "DDPG",
                                [&] { return step_body(d, r, B, n_batches, nullptr, seed, true, true, c); }, &how);
    return step_ran(d, d->dgraph.graph, rc, how);
  }
  for (int i = 0; i < n_batches; ++i) {
    if (sync_every > 1) {                           // local update; every k-th one is followed by the parameter averaging
      RC(half_step(d, r, B, seed, false, nullptr));
      RC(apply(d, OptPlan()));
      if (++d->dp_local >= (uint64_t)sync_every && c) RC(cpp_ddpg_average_params(d, c));
      continue;
    }
    if (c && overlap) {
      RC(half_step(d, r, B, seed, true, [&]() -> int {        // between the two graphs: the fc gradients are final
        HIP_CHECK(hipEventRecord(c->ev_fc, ctx->stream));
        HIP_CHECK(hipStreamWaitEvent(c->side, c->ev_fc, 0));
        NCCL_CHECK(ncclGroupStart());
        NCCL_CHECK(ncclAllReduce(d->gradbuf + fa, d->gradbuf + fa, (size_t)(d->nA - fa), ncclFloat, ncclSum, c->comm, c->side));
        NCCL_CHECK(ncclAllReduce(d->gradbuf + d->nA + fcr, d->gradbuf + d->nA + fcr, (size_t)(d->nC - fcr), ncclFloat, ncclSum, c->comm, c->side));
        NCCL_CHECK(ncclGroupEnd());
        return CPP_OK; }));
      HIP_CHECK(hipEventRecord(c->ev_bwd, ctx->stream));      // conv backward + dW reductions done: the conv parts follow
      HIP_CHECK(hipStreamWaitEvent(c->side, c->ev_bwd, 0));
      if (fa > 0 || fcr > 0) {
        NCCL_CHECK(ncclGroupStart());
        if (fa > 0) NCCL_CHECK(ncclAllReduce(d->gradbuf, d->gradbuf, (size_t)fa, ncclFloat, ncclSum, c->comm, c->side));
        if (fcr > 0) NCCL_CHECK(ncclAllReduce(d->gradbuf + d->nA, d->gradbuf + d->nA, (size_t)fcr, ncclFloat, ncclSum, c->comm, c->side));
        NCCL_CHECK(ncclGroupEnd());
      }
      HIP_CHECK(hipEventRecord(c->ev_done, c->side));
      HIP_CHECK(hipStreamWaitEvent(ctx->stream, c->ev_done, 0));
    } else {
      RC(half_step(d, r, B, seed, false, nullptr));
      if (c) RC(cpp_ddpg_allreduce_grads(d, c));
    }
    OptPlan plan; plan.grad_scale = inv;
    RC(apply(d, plan));
  }
  return cpp_ddpg_update_targets(d);
}

// which form the default data-parallel step of this trainer takes: 0 = none run yet, 1 = one hipGraph replay per outer step (the
// collective inside), 2 = the same sequence as stream launches (the capture was refused; `reason` says by what)
extern "C" int cpp_ddpg_dp_status(const cpp_ddpg* d, int* mode, char* reason, int cap) {
  ARG_CHECK(d && mode, "cpp_ddpg_dp_status: NULL argument");
  *mode = d->dgraph.mode(d->graph_gen);
  if (reason && cap > 0) snprintf(reason, (size_t)cap, "%s", d->dgraph.reason);
  return CPP_OK;
}

extern "C" int cpp_ddpg_last_stats(cpp_ddpg* d, float out[3]) {
  ARG_CHECK(d && out, "cpp_ddpg_last_stats: NULL argument");
  double parts[DDPG_HEADS_MAX_WGS];
  const LossAt& at = d->last;
  RC(read_back(d->ctx, {{out, d->loss_norms, 3 * sizeof(float)}, {at.parts > 0 ? parts : nullptr, d->heads_part, (size_t)at.parts * sizeof(double)}}, true));
  if (at.parts > 0) out[0] = loss_of_parts(parts, at.parts, at.B);      // fused heads kernel: mean(td^2); dist.hip: mean(w L)
  return CPP_OK;
}

extern "C" int cpp_ddpg_last_values(cpp_ddpg* d, int B, float* actions, float* dq_da, float* q, float* td) {
  ARG_CHECK(d, "cpp_ddpg_last_values: NULL argument");
  ARG_CHECK(B >= 1 && B <= d->maxB, "cpp_ddpg_last_values: batch %d outside [1,%d]", B, d->maxB);
  HIP_CHECK(hipSetDevice(d->ctx->device));
  const size_t nB = (size_t)B * sizeof(float), nA = nB * d->actor->spec.action_dim;
  return read_back(d->ctx, {{actions, d->actor->ws[0].out, nA}, {dq_da, d->dq_da, nA}, {q, d->critic->ws[0].out, nB}, {td, d->td, nB}});
}


// Twin Q heads: what head 2 and the two target heads left in the last minibatch's gradient pass (cpp_ddpg_last_values keeps reporting
// head 1's q and td): Q2(state_1, fed action), Q1'(state_2, a'), Q2'(state_2, a') and td_2 = Q2 - y, each (B).  NULL pointers are skipped.
extern "C" int cpp_ddpg_last_twin_values(cpp_ddpg* d, int B, float* q2, float* target_q1, float* target_q2, float* td2) {
  ARG_CHECK(d, "cpp_ddpg_last_twin_values: NULL argument");
  ARG_CHECK(B >= 1 && B <= d->maxB, "cpp_ddpg_last_twin_values: batch %d outside [1,%d]", B, d->maxB);
  if (!d->twin) { cpp_set_error("cpp_ddpg_last_twin_values: the trainer's critics are not twin critics"); return CPP_ERR_STATE; }
  HIP_CHECK(hipSetDevice(d->ctx->device));
  const size_t n = (size_t)B * sizeof(float);
  return read_back(d->ctx, {{q2, d->critic->ws[0].out2, n}, {target_q1, d->tcritic->ws[0].out, n}, {target_q2, d->tcritic->ws[0].out2, n}, {td2, d->td2, n}});
}

// Quantile trainers (Dabney et al. 2018; Kuznetsov et al. 2020; an extension of the target ddpg_cartpole.py:199-214): the Huber threshold
// and the number of top target atoms dropped.  Both are captured by value: the call drops the cached graphs.
extern "C" int cpp_ddpg_set_quantile_target(cpp_ddpg* d, float kappa, int drop_top) {
  ARG_CHECK(d, "cpp_ddpg_set_quantile_target: NULL argument");
  if (!d->quant) { cpp_set_error("cpp_ddpg_set_quantile_target: the trainer's critics are not quantile critics"); return CPP_ERR_STATE; }
  ARG_CHECK(std::isfinite(kappa) && kappa > 0.f, "cpp_ddpg_set_quantile_target: kappa %g (finite, positive)", (double)kappa);
  ARG_CHECK(drop_top >= 0 && drop_top <= d->dist_n - 1, "cpp_ddpg_set_quantile_target: %d dropped atoms outside [0, %d]", drop_top, d->dist_n - 1);
  HIP_CHECK(hipSetDevice(d->ctx->device));
  HIP_CHECK(ctx_sync_stream(d->ctx));
  d->quant_kappa = kappa; d->quant_drop = drop_top;
  reconfigured(d);      // (the captured launches carry the old values)
  return CPP_OK;
}

// Quantile trainers: what the last minibatch's gradient pass left (the critic of ddpg_cartpole.py:166-177 at the fed action, the target
// :199-214) -- theta of the fed evaluation, the target critic's atoms at the (smoothed) target action sorted ascending, and
// y_j = r + g s_j (columns j >= M zero), each (B, N).  NULL pointers are skipped.
extern "C" int cpp_ddpg_last_quantiles(cpp_ddpg* d, int B, float* theta, float* sorted_target_theta, float* y) {
  ARG_CHECK(d, "cpp_ddpg_last_quantiles: NULL argument");
  ARG_CHECK(B >= 1 && B <= d->maxB, "cpp_ddpg_last_quantiles: batch %d outside [1,%d]", B, d->maxB);
  if (!d->quant) { cpp_set_error("cpp_ddpg_last_quantiles: the trainer's critics are not quantile critics"); return CPP_ERR_STATE; }
  HIP_CHECK(hipSetDevice(d->ctx->device));
  const size_t n = (size_t)B * d->dist_n * sizeof(float);
  return read_back(d->ctx, {{theta, d->dist_p, n}, {sorted_target_theta, d->dist_tp, n}, {y, d->dist_m, n}});
}

// Distributional trainers: what the last minibatch's gradient pass left -- p of the fed evaluation, p' of the target evaluation at the
// (smoothed) target action and the projected target m, each (B, N).  NULL pointers are skipped.
extern "C" int cpp_ddpg_last_distribution(cpp_ddpg* d, int B, float* p, float* target_p, float* m) {
  ARG_CHECK(d, "cpp_ddpg_last_distribution: NULL argument");
  ARG_CHECK(B >= 1 && B <= d->maxB, "cpp_ddpg_last_distribution: batch %d outside [1,%d]", B, d->maxB);
  if (!d->dist_n || d->quant) { cpp_set_error("cpp_ddpg_last_distribution: the trainer's critics are not distributional"); return CPP_ERR_STATE; }
  HIP_CHECK(hipSetDevice(d->ctx->device));
  const size_t n = (size_t)B * d->dist_n * sizeof(float);
  return read_back(d->ctx, {{p, d->dist_p, n}, {target_p, d->dist_tp, n}, {m, d->dist_m, n}});
}

// Soft actor-critic (Haarnoja et al. 2018; an extension of the actor's train op ddpg_cartpole.py:102-119 and of the critic's target
// :199-214; include/cartpolepp_abi.h).  Temperature, target entropy, rate and seed are captured by value: the call zeroes the noise count,
// Adam's slots and count, copies the actor into the target actor and drops the cached graphs.
extern "C" int cpp_ddpg_set_sac(cpp_ddpg* d, float init_temperature, float target_entropy, float temperature_lr, uint64_t seed) {
  ARG_CHECK(d, "cpp_ddpg_set_sac: NULL argument");
  if (!d->sac) { cpp_set_error("cpp_ddpg_set_sac: the trainer's actors are not Gaussian actors (cpp_net_create_gaussian)"); return CPP_ERR_STATE; }
  ARG_CHECK(std::isfinite(init_temperature) && init_temperature > 0.f, "cpp_ddpg_set_sac: temperature %g (finite, positive)", (double)init_temperature);
  ARG_CHECK(std::isfinite(target_entropy), "cpp_ddpg_set_sac: target entropy %g (finite)", (double)target_entropy);
  ARG_CHECK(std::isfinite(temperature_lr) && temperature_lr >= 0.f, "cpp_ddpg_set_sac: temperature learning rate %g (finite, >= 0; 0: fixed)", (double)temperature_lr);
  ARG_CHECK(d->tps_on == false && d->pd_d == 1, "cpp_ddpg_set_sac: target policy smoothing or a policy delay is on");
  HIP_CHECK(hipSetDevice(d->ctx->device));
  return sac_configure(d, init_temperature, target_entropy, temperature_lr, seed);
}

// What the last gradient pass of a soft actor-critic trainer left (the sample that stands where ddpg_cartpole.py:95-100's tanh stood, the
// target :199-214): eps, a (B, A) and logp (B) of the draw at state_1 and of the draw at state_2, r_soft (B), the temperature the actor
// pass read, g_alpha of its rows and the count the target draw was made at; dz: the head gradient (d m | d x), (B, 2A).  NULL pointers are skipped.
extern "C" int cpp_ddpg_last_sac(cpp_ddpg* d, int B, float* eps, float* a, float* logp, float* eps2, float* a2, float* logp2, float* r_soft,
                                 float* alpha, float* g_alpha, uint64_t* n, float* dz) {
  ARG_CHECK(d, "cpp_ddpg_last_sac: NULL argument");
  ARG_CHECK(B >= 1 && B <= d->maxB, "cpp_ddpg_last_sac: batch %d outside [1,%d]", B, d->maxB);
  if (!d->sac) { cpp_set_error("cpp_ddpg_last_sac: the trainer's actors are not Gaussian actors"); return CPP_ERR_STATE; }
  HIP_CHECK(hipSetDevice(d->ctx->device));
  const size_t nA = (size_t)B * d->actor->spec.action_dim * sizeof(float), nB = (size_t)B * sizeof(float);
  double parts[DDPG_HEADS_MAX_WGS];
  const int rows = d->last.sac_rows, np = rows > 0 ? sac_grid(rows) : 0;
  RC(read_back(d->ctx, {{eps, d->sac_eps[0], nA}, {a, d->actor->ws[0].out, nA}, {logp, d->sac_logp[0], nB},
                        {eps2, d->sac_eps[1], nA}, {a2, d->tactor->ws[0].out, nA}, {logp2, d->sac_logp[1], nB}, {r_soft, d->sac_rsoft, nB},
                        {dz, d->actor->ws[0].dz[d->actor->fc.size() - 1], 2 * nA}, {alpha, d->sac_w + SAC_W_ALPHA, sizeof(float)},
                        {n, d->tps_n + 1, sizeof(uint64_t)}, {g_alpha && np ? parts : nullptr, d->sac_part, (size_t)np * sizeof(double)}}));
  if (g_alpha) {      // (the fixed-order finalisation of sac.hip's job 4)
    double s = 0.0;
    for (int i = 0; i < np; ++i) s += parts[i];
    *g_alpha = np ? (float)(-(s / (double)rows)) : 0.f;
  }
  return CPP_OK;
}

// What the last gradient pass left of the feature layer norm of the actor (which = 0) or the critic (1): include/cartpolepp_abi.h
extern "C" int cpp_ddpg_last_feature_norm(cpp_ddpg* d, int B, int which, float* xhat, float* rstd, float* y, float* dz, float* dgamma, float* dbeta) {
  ARG_CHECK(d, "cpp_ddpg_last_feature_norm: NULL argument");
  ARG_CHECK(B >= 1 && B <= d->maxB, "cpp_ddpg_last_feature_norm: batch %d outside [1,%d]", B, d->maxB);
  ARG_CHECK(which == 0 || which == 1, "cpp_ddpg_last_feature_norm: which %d (0: the actor, 1: the critic)", which);
  if (!d->actor->ln) { cpp_set_error("cpp_ddpg_last_feature_norm: the trainer's networks have no feature layer norm"); return CPP_ERR_STATE; }
  HIP_CHECK(hipSetDevice(d->ctx->device));
  cpp_net* n = which ? d->critic : d->actor;
  const Workspace& w = n->ws[0];
  const int width = n->fc[0].n_out;
  const size_t row = (size_t)width * sizeof(float), all = (size_t)B * row;
  if (y) HIP_CHECK(hipMemcpy2DAsync(y, row, w.fcin[1], (size_t)(n->fc[1].n_in + 1) * sizeof(float), row, B, hipMemcpyDeviceToHost, d->ctx->stream));
  return read_back(d->ctx, {{xhat, w.ln_xhat, all}, {rstd, w.ln_rstd, (size_t)B * sizeof(float)}, {dz, w.dz[0], all},
                            {dgamma, n->grads + n->ln_g_off, row}, {dbeta, n->grads + n->ln_b_off, row}});
}

// log_alpha, Adam's slots and its count for checkpoints (util.py:88-90: tf.train.Saver saves every variable of the graph).  set == 0: read
// into the pointers; otherwise written from them (all four needed).  The noise count is not part of it: a resumed run restarts the stream.
extern "C" int cpp_ddpg_sac_temperature(cpp_ddpg* d, int set, float* log_alpha, float* m, float* v, uint64_t* step) {
  ARG_CHECK(d, "cpp_ddpg_sac_temperature: NULL argument");
  if (!d->sac) { cpp_set_error("cpp_ddpg_sac_temperature: the trainer's actors are not Gaussian actors"); return CPP_ERR_STATE; }
  HIP_CHECK(hipSetDevice(d->ctx->device));
  hipStream_t st = d->ctx->stream;
  float w[SAC_WORDS];
  HIP_CHECK(hipMemcpyAsync(w, d->sac_w, sizeof(w), hipMemcpyDeviceToHost, st));
  HIP_CHECK(hipStreamSynchronize(st));
  if (!set) {
    if (log_alpha) *log_alpha = w[SAC_W_LOG_ALPHA];
    if (m) *m = w[SAC_W_M];
    if (v) *v = w[SAC_W_V];
    if (step) { HIP_CHECK(hipMemcpyAsync(step, d->sac_step, sizeof(uint64_t), hipMemcpyDeviceToHost, st)); HIP_CHECK(hipStreamSynchronize(st)); }
    return CPP_OK;
  }
  ARG_CHECK(log_alpha && m && v && step, "cpp_ddpg_sac_temperature: NULL argument");
  ARG_CHECK(std::isfinite(*log_alpha) && std::isfinite(*m) && std::isfinite(*v) && *v >= 0.f, "cpp_ddpg_sac_temperature: log_alpha %g, m %g, v %g",
            (double)*log_alpha, (double)*m, (double)*v);
  w[SAC_W_LOG_ALPHA] = w[SAC_W_TARGET] = *log_alpha; w[SAC_W_M] = *m; w[SAC_W_V] = *v;
  HIP_CHECK(hipMemcpyAsync(d->sac_w, w, sizeof(w), hipMemcpyHostToDevice, st));
  HIP_CHECK(hipMemcpyAsync(d->sac_step, step, sizeof(uint64_t), hipMemcpyHostToDevice, st));
  HIP_CHECK(hipStreamSynchronize(st));
  return CPP_OK;
}
