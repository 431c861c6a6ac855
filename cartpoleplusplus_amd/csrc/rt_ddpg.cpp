// DDPG train ops, the fused inner step and its hipGraph, the data-parallel half steps (cpp_ddpg_*).  The gradient pass they all run is
// rt_ddpg_pass.cpp, the setters and accessors rt_ddpg_config.cpp; the trainer itself: rt_ddpg.h
#include "rt_ddpg.h"

float loss_of_parts(const double* parts, int n, int B) {
  double s = 0.0;
  for (int i = 0; i < n; ++i) s += parts[i];
  return (float)(s / (double)B);
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
  ARG_CHECK(critic->pooled() == tcritic->pooled(), "cpp_ddpg_create: pooled quantile critics come as a pair with one N (cpp_net_create_pooled_quantile: both critics, or neither)");
  ARG_CHECK(!(critic->dist_n && critic->twin) || critic->pooled(), "cpp_ddpg_create: a distributional critic with twin Q heads");
  ARG_CHECK(critic->quant == tcritic->quant, "cpp_ddpg_create: a quantile critic needs a quantile target critic with the same N (never a categorical or a plain one)");
  ARG_CHECK(actor->gauss == tactor->gauss && actor->ls_lo == tactor->ls_lo && actor->ls_hi == tactor->ls_hi,
            "cpp_ddpg_create: a Gaussian actor needs a Gaussian target actor with the same log std bounds (and a plain one a plain one)");
  ARG_CHECK(!(actor->gauss && critic->dist_n) || critic->pooled(), "cpp_ddpg_create: a Gaussian actor with a distributional or quantile critic");
  for (cpp_net* n : {actor, critic, tactor, tcritic})
    ARG_CHECK(!(actor->gauss && (n->spec.use_batch_norm || n->spec.use_dropout)), "cpp_ddpg_create: a Gaussian actor with batch norm or dropout");
  ARG_CHECK(actor->ln == critic->ln && actor->ln == tactor->ln && actor->ln == tcritic->ln,
            "cpp_ddpg_create: a feature layer norm on some of the four networks (cpp_net_create_feature_norm: all four, or none)");
  for (cpp_net* n : {critic, tactor, tcritic})
    ARG_CHECK(!actor->ln || (n->ln_act == actor->ln_act && n->ln_eps == actor->ln_eps),
              "cpp_ddpg_create: the four networks' feature layer norms differ in activation or epsilon");
  ARG_CHECK(actor->enc_less == tactor->enc_less, "cpp_ddpg_create: one encoder-less actor (cpp_net_create_encoderless: the actor and the target actor, or neither)");
  ARG_CHECK(!actor->enc_less || (actor->encoder == critic && tactor->encoder == tcritic),      // (actor-only training binds the live pair twice)
            "cpp_ddpg_create: encoder-less actors come as a pair, each bound (cpp_net_set_encoder) to the critic it is created with");
  ARG_CHECK(actor->nparams == tactor->nparams && critic->nparams == tcritic->nparams, "cpp_ddpg_create: target shapes differ");
  ARG_CHECK(actor->state_elems == critic->state_elems && actor->spec.action_dim == critic->spec.action_dim,
            "cpp_ddpg_create: actor/critic input shapes differ");
  HIP_CHECK(hipSetDevice(ctx->device));
  cpp_ddpg* d = new cpp_ddpg();
  d->arena.stream = ctx->stream;
  d->ctx = ctx; d->actor = actor; d->critic = critic; d->tactor = tactor; d->tcritic = tcritic; d->hp = *hp;
  d->maxB = actor->maxB < critic->maxB ? actor->maxB : critic->maxB;
  d->nA = actor->nparams; d->nC = critic->nparams;
  d->shared = actor->enc_less; d->trunk = d->shared ? critic : actor;
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
  d->pool = critic->pooled();      // (the pool's two buffers are 2N wide, and theta^2 has one of its own)
  if (!rc && d->dist_n) rc = dalloc(d->arena, &d->dist_p, (size_t)d->maxB * d->dist_n);
  for (float** p : {&d->dist_tp, &d->dist_m})
    if (!rc && d->dist_n) rc = dalloc(d->arena, p, (size_t)d->maxB * d->dist_n * (d->pool ? 2 : 1));
  if (!rc && d->pool) rc = dalloc(d->arena, &d->pool_p2, (size_t)d->maxB * d->dist_n);
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
void reconfigured(cpp_ddpg* d) { invalidate_graphs(d); d->pre_variant = 0; }

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

// the increment of a target-forming pass that no apply() follows (cpp_ddpg_compute_gradients, the half steps): a launch of its own
// behind the pass -- only with smoothing on
static int tps_settle(cpp_ddpg* d, const PassLeft& left) {
  return left.noise_owed ? launch_counter_add(d->ctx, d->tps_n, 1) : CPP_OK;
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
  // (a shared encoder: the two critics are the networks with a conv1 -- one trained and one target, as NAF's pair)
  cpp_net* inets[4] = {d->actor, d->critic, d->tactor, d->tcritic};
  if (d->shared) { inets[0] = d->critic; inets[1] = d->tcritic; }
  const int n_img = d->shared ? 2 : 4;
  const ConvL* L0 = has_conv(d->trunk) ? &d->trunk->conv[0] : nullptr;
  // (CPP_RIDE_IMAGE_UPDATE=0, ablation build: no image workgroups at all -- conv1's parameters and slots are advanced by the update's
  // plain workgroups and the forward builds its image by a launch of its own: what the rider's restated update is compared with)
  static const bool no_img = cpp_switch_off("CPP_RIDE_IMAGE_UPDATE");
  const bool img = nx.b && nx.C > 0 && do_actor && do_critic && L0 && !d->actor->spec.use_batch_norm && !d->critic->spec.use_batch_norm &&
                   conv_rs16_ok(d->ctx, L0->Cin, L0->H, L0->W, kConvOut) && nx.B >= 2 && !no_img &&
                   (d->shared || conv1_opens_params(d->actor)) && conv1_opens_params(d->critic);
  if (img) {
    s.img_n = n_img; s.img_cin = L0->Cin;
    for (int j = 0; j < n_img; ++j) {      // (the trained networks read state_1's tables, the targets state_2's)
      const bool trained = j < n_img / 2;
      const int seg = d->shared ? 1 : j;      // (the segment of a trained network: the shared encoder is in the critic's)
      opt_img_net(s, j, inets[j], trained ? seg : -1, trained ? 0 : 1, nx);
      const ConvL& L = inets[j]->conv[0];
      if (trained && s.kind != OPT_SGD) { s.img[j].mw = s.m[seg] + L.w_off; s.img[j].mb = s.m[seg] + L.b_off; }
      if (trained && s.kind == OPT_ADAM) { s.img[j].vw = s.v[seg] + L.w_off; s.img[j].vb = s.v[seg] + L.b_off; }
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
  // --use-dropout: nothing drawn means no mask and no count either.  The actor's layers look for its counter while the pass is built:
  // without one they are the inference layers (no unit dropped, no factor 2) and the forward is not counted, so the masks of the
  // training calls around this one are the ones they would have drawn without it
  uint64_t* const drop_counter = d->actor->drop_counter;
  d->actor->drop_counter = nullptr;
  const int rc = actor_half(d, b, false, &left);
  d->actor->drop_counter = drop_counter;
  RC(rc);
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
  L.ctx = ctx; L.r = r; L.step_batch = d->step_batch; L.trunk = d->trunk;
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
  const bool direct = direct_replay_ok(d->trunk, r, B);
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
