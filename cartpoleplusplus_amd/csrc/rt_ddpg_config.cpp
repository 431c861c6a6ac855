// The DDPG trainer's configuration and inspection surface: the setters, the cpp_ddpg_last_* accessors, the checkpointed state
#include "rt_ddpg.h"

// How every setter runs once its arguments are checked: the stream drains, `body` allocates and zeroes what the setting needs, the stream
// drains again and the cached graphs are dropped (the captured launches carry the old values).  An error leaves the graphs alone; the
// caller stores the new values behind a CPP_OK.
static int reconfigure(cpp_ddpg* d, const std::function<int()>& body = nullptr) {
  HIP_CHECK(hipSetDevice(d->ctx->device));
  HIP_CHECK(ctx_sync_stream(d->ctx));
  if (body) RC(body());
  HIP_CHECK(ctx_sync_stream(d->ctx));
  reconfigured(d);
  return CPP_OK;
}

// How every accessor of what the last pass left for a batch of B rows starts.  off: the feature it reports is not this trainer's
// (CPP_ERR_STATE with off_msg)
static int last_entry(cpp_ddpg* d, int B, const char* who, bool off = false, const char* off_msg = "") {
  ARG_CHECK(d, "%s: NULL argument", who);
  ARG_CHECK(B >= 1 && B <= d->maxB, "%s: batch %d outside [1,%d]", who, B, d->maxB);
  if (off) { cpp_set_error("%s: %s", who, off_msg); return CPP_ERR_STATE; }
  HIP_CHECK(hipSetDevice(d->ctx->device));
  return CPP_OK;
}

// SAC has no target actor: its parameters are a bit copy of the actor's (and the target-forming pass's temperature word of log_alpha)
int sac_sync_target(cpp_ddpg* d) {
  hipStream_t st = d->ctx->stream;
  if (d->tactor != d->actor)      // (actor-only training binds the live networks as stand-ins)
    HIP_CHECK(hipMemcpyAsync(d->tactor->params, d->actor->params, (size_t)d->nA * sizeof(float), hipMemcpyDeviceToDevice, st));
  HIP_CHECK(hipMemcpyAsync(d->sac_w + SAC_W_TARGET, d->sac_w + SAC_W_LOG_ALPHA, sizeof(float), hipMemcpyDeviceToDevice, st));
  d->tactor->wimg_key = nullptr;      // (the image the rider built is of the parameters before the copy)
  return CPP_OK;
}
int sac_configure(cpp_ddpg* d, float init_temperature, float target_entropy, float lr, uint64_t seed) {
  float w[SAC_WORDS]; memset(w, 0, sizeof(w));      // (read by the copy below until the frame's second drain)
  w[SAC_W_LOG_ALPHA] = w[SAC_W_TARGET] = logf(init_temperature); w[SAC_W_ALPHA] = init_temperature;
  RC(reconfigure(d, [&]() -> int {
    hipStream_t st = d->ctx->stream;
    HIP_CHECK(hipMemcpyAsync(d->sac_w, w, sizeof(w), hipMemcpyHostToDevice, st));
    HIP_CHECK(hipMemsetAsync(d->sac_step, 0, sizeof(uint64_t), st));
    HIP_CHECK(hipMemsetAsync(d->tps_n, 0, 2 * sizeof(uint64_t), st));
    return sac_sync_target(d);
  }));
  d->sac_hbar = target_entropy; d->sac_lr = lr; d->sac_seed = seed; d->last.sac_rows = 0;
  return CPP_OK;
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
  RC(reconfigure(d, [&]() -> int {
    hipStream_t st = d->ctx->stream;
    const size_t n = (size_t)(d->nA + d->nC);
    if (kind != CPP_OPT_SGD && !d->opt_m) RC(dalloc(d->arena, &d->opt_m, n));
    if (kind == CPP_OPT_ADAM && !d->opt_v) RC(dalloc(d->arena, &d->opt_v, n));
    if (kind != CPP_OPT_SGD && !d->opt_step) RC(dalloc(d->arena, &d->opt_step, (size_t)2));
    if (d->opt_m) HIP_CHECK(hipMemsetAsync(d->opt_m, 0, n * sizeof(float), st));
    if (d->opt_v) HIP_CHECK(hipMemsetAsync(d->opt_v, 0, n * sizeof(float), st));
    if (d->opt_step) HIP_CHECK(hipMemsetAsync(d->opt_step, 0, 2 * sizeof(uint64_t), st));
    return CPP_OK;
  }));
  d->opt_kind = kind; d->opt_momentum = momentum; d->opt_beta1 = beta1; d->opt_beta2 = beta2; d->opt_epsilon = epsilon;
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
  RC(reconfigure(d, [&]() -> int {
    hipStream_t st = d->ctx->stream;
    const size_t n = (size_t)d->maxB * d->actor->spec.action_dim;
    if (sigma > 0.f && !d->tps_n) RC(dalloc(d->arena, &d->tps_n, (size_t)2));
    if (sigma > 0.f && !d->tps_eps) RC(dalloc(d->arena, &d->tps_eps, n));
    if (d->tps_n) HIP_CHECK(hipMemsetAsync(d->tps_n, 0, 2 * sizeof(uint64_t), st));
    if (d->tps_eps) HIP_CHECK(hipMemsetAsync(d->tps_eps, 0, n * sizeof(float), st));
    return CPP_OK;
  }));
  d->tps_on = sigma > 0.f; d->tps_sigma = sigma; d->tps_clip = clip; d->tps_seed = seed;
  return CPP_OK;
}

extern "C" int cpp_ddpg_last_target_noise(cpp_ddpg* d, int B, float* eps, uint64_t* n) {
  RC(last_entry(d, B, "cpp_ddpg_last_target_noise", !(d && d->tps_on), "target policy smoothing is off"));
  return read_back(d->ctx, {{eps, d->tps_eps, (size_t)B * d->actor->spec.action_dim * sizeof(float)}, {n, d->tps_n + 1, sizeof(uint64_t)}}, true);
}

// Delayed policy updates (TD3: Fujimoto et al. 2018, Algorithm 1; an extension of ddpg_cartpole.py:332-337; include/cartpolepp_abi.h).  The
// delay is captured by value: the call drops the cached graphs, and it zeroes the count.  delay 1 is off: no launch carries the words.
extern "C" int cpp_ddpg_set_policy_delay(cpp_ddpg* d, int delay) {
  ARG_CHECK(d, "cpp_ddpg_set_policy_delay: NULL argument");
  ARG_CHECK(delay >= 1 && delay <= 65536, "cpp_ddpg_set_policy_delay: delay %d outside [1, 65536]", delay);
  ARG_CHECK(!(d->sac && delay > 1), "cpp_ddpg_set_policy_delay: a soft actor-critic trainer updates its policy in every minibatch");
  RC(reconfigure(d, [&]() -> int {
    if (delay > 1 && !d->pd) RC(dalloc(d->arena, &d->pd, (size_t)PD_WORDS));
    if (d->pd) HIP_CHECK(hipMemsetAsync(d->pd, 0, PD_WORDS * sizeof(uint64_t), d->ctx->stream));
    return CPP_OK;
  }));
  d->pd_d = delay;
  return CPP_OK;
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

// The actor on the minimum head (TD3 / DrQ-v2 / SAC's actor objective on twin critics: min(Q1, Q2) at the policy's action; an extension of
// ddpg_cartpole.py:111-113, :220-222; include/cartpolepp_abi.h).  The switch is captured by the launches: the call drops the cached graphs.
extern "C" int cpp_ddpg_set_actor_min_q(cpp_ddpg* d, int on) {
  ARG_CHECK(d, "cpp_ddpg_set_actor_min_q: NULL argument");
  ARG_CHECK(d->twin, "cpp_ddpg_set_actor_min_q: both critics must carry twin Q heads (cpp_net_create_twin_q)");
  ARG_CHECK(!d->pool, "cpp_ddpg_set_actor_min_q: pooled quantile critics (their actor ascends the mean over all atoms of both heads)");
  RC(reconfigure(d, [&]() -> int { return (on && !d->amin_sel) ? dalloc(d->arena, &d->amin_sel, (size_t)d->maxB) : (int)CPP_OK; }));
  d->amin = on != 0;      // (the other family of heads instances, or the other GEMM levels)
  return CPP_OK;
}

extern "C" int cpp_ddpg_last_actor_min(cpp_ddpg* d, int B, float* q1, float* q2, int32_t* sel) {
  RC(last_entry(d, B, "cpp_ddpg_last_actor_min", !(d && d->amin), "the actor follows Q1 (cpp_ddpg_set_actor_min_q is off)"));
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
  RC(reconfigure(d, [&]() -> int {      // (the arena zeroes what it hands out)
    if (!(alpha > 0.f) || d->bc_stat) return CPP_OK;
    RC(dalloc(d->arena, &d->bc_stat, (size_t)2));
    RC(dalloc(d->arena, &d->bc_g, (size_t)d->maxB * d->actor->spec.action_dim));
    return dalloc(d->arena, &d->bc_rows, (size_t)d->maxB);
  }));
  d->bc_alpha = alpha; d->bc_floor = q_floor;      // (the fused heads, or the other alpha)
  return CPP_OK;
}

extern "C" int cpp_ddpg_last_behaviour_cloning(cpp_ddpg* d, int B, float* lambda, float* m, float* g, float* bc_rows) {
  RC(last_entry(d, B, "cpp_ddpg_last_behaviour_cloning", !(d && d->bc_alpha > 0.f), "behaviour cloning is off (cpp_ddpg_set_behaviour_cloning)"));
  const size_t nB = (size_t)B * sizeof(float);
  return read_back(d->ctx, {{lambda, d->bc_stat, sizeof(float)}, {m, d->bc_stat + 1, sizeof(float)},
                            {g, d->bc_g, nB * d->actor->spec.action_dim}, {bc_rows, d->bc_rows, nB}}, true);
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

extern "C" int cpp_ddpg_last_stats(cpp_ddpg* d, float out[3]) {
  ARG_CHECK(d && out, "cpp_ddpg_last_stats: NULL argument");
  double parts[DDPG_HEADS_MAX_WGS];
  const LossAt& at = d->last;
  RC(read_back(d->ctx, {{out, d->loss_norms, 3 * sizeof(float)}, {at.parts > 0 ? parts : nullptr, d->heads_part, (size_t)at.parts * sizeof(double)}}, true));
  if (at.parts > 0) out[0] = loss_of_parts(parts, at.parts, at.B);      // fused heads kernel: mean(td^2); dist.hip: mean(w L)
  return CPP_OK;
}

extern "C" int cpp_ddpg_last_values(cpp_ddpg* d, int B, float* actions, float* dq_da, float* q, float* td) {
  RC(last_entry(d, B, "cpp_ddpg_last_values"));
  const size_t nB = (size_t)B * sizeof(float), nA = nB * d->actor->spec.action_dim;
  return read_back(d->ctx, {{actions, d->actor->ws[0].out, nA}, {dq_da, d->dq_da, nA}, {q, d->critic->ws[0].out, nB}, {td, d->td, nB}});
}

// Twin Q heads: what head 2 and the two target heads left in the last minibatch's gradient pass (cpp_ddpg_last_values keeps reporting
// head 1's q and td): Q2(state_1, fed action), Q1'(state_2, a'), Q2'(state_2, a') and td_2 = Q2 - y, each (B).  NULL pointers are skipped.
extern "C" int cpp_ddpg_last_twin_values(cpp_ddpg* d, int B, float* q2, float* target_q1, float* target_q2, float* td2) {
  RC(last_entry(d, B, "cpp_ddpg_last_twin_values", !(d && d->twin), "the trainer's critics are not twin critics"));
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
  RC(reconfigure(d));
  d->quant_kappa = kappa; d->quant_drop = drop_top;
  return CPP_OK;
}

// Quantile trainers: what the last minibatch's gradient pass left (the critic of ddpg_cartpole.py:166-177 at the fed action, the target
// :199-214) -- theta of the fed evaluation, the target critic's atoms at the (smoothed) target action sorted ascending, and
// y_j = r + g s_j (columns j >= M zero), each (B, N).  NULL pointers are skipped.
extern "C" int cpp_ddpg_last_quantiles(cpp_ddpg* d, int B, float* theta, float* sorted_target_theta, float* y) {
  RC(last_entry(d, B, "cpp_ddpg_last_quantiles", !(d && d->quant && !d->pool), "the trainer's critics are not quantile critics"));
  const size_t n = (size_t)B * d->dist_n * sizeof(float);
  return read_back(d->ctx, {{theta, d->dist_p, n}, {sorted_target_theta, d->dist_tp, n}, {y, d->dist_m, n}});
}

// Pooled quantile trainers (cpp_net_create_pooled_quantile; an extension of the target ddpg_cartpole.py:199-214): what the last minibatch's
// gradient pass left -- theta^1 and theta^2 of the fed evaluation ((B, N) each), both target heads' atoms at the ONE target action pooled and
// sorted ascending, and y_j = r* + g s_j (columns j >= M = 2N - 2d zero), (B, 2N) each.  NULL pointers are skipped.
extern "C" int cpp_ddpg_last_pooled_quantiles(cpp_ddpg* d, int B, float* theta1, float* theta2, float* sorted_pool, float* y) {
  RC(last_entry(d, B, "cpp_ddpg_last_pooled_quantiles", !(d && d->pool), "the trainer's critics are not pooled quantile critics"));
  const size_t n = (size_t)B * d->dist_n * sizeof(float);
  return read_back(d->ctx, {{theta1, d->dist_p, n}, {theta2, d->pool_p2, n}, {sorted_pool, d->dist_tp, 2 * n}, {y, d->dist_m, 2 * n}});
}

// Distributional trainers: what the last minibatch's gradient pass left -- p of the fed evaluation, p' of the target evaluation at the
// (smoothed) target action and the projected target m, each (B, N).  NULL pointers are skipped.
extern "C" int cpp_ddpg_last_distribution(cpp_ddpg* d, int B, float* p, float* target_p, float* m) {
  RC(last_entry(d, B, "cpp_ddpg_last_distribution", !(d && d->dist_n && !d->quant), "the trainer's critics are not distributional"));
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
  return sac_configure(d, init_temperature, target_entropy, temperature_lr, seed);
}

// What the last gradient pass of a soft actor-critic trainer left (the sample that stands where ddpg_cartpole.py:95-100's tanh stood, the
// target :199-214): eps, a (B, A) and logp (B) of the draw at state_1 and of the draw at state_2, r_soft (B), the temperature the actor
// pass read, g_alpha of its rows and the count the target draw was made at; dz: the head gradient (d m | d x), (B, 2A).  NULL pointers are skipped.
extern "C" int cpp_ddpg_last_sac(cpp_ddpg* d, int B, float* eps, float* a, float* logp, float* eps2, float* a2, float* logp2, float* r_soft,
                                 float* alpha, float* g_alpha, uint64_t* n, float* dz) {
  RC(last_entry(d, B, "cpp_ddpg_last_sac", !(d && d->sac), "the trainer's actors are not Gaussian actors"));
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
  RC(last_entry(d, B, "cpp_ddpg_last_feature_norm"));
  ARG_CHECK(which == 0 || which == 1, "cpp_ddpg_last_feature_norm: which %d (0: the actor, 1: the critic)", which);
  if (!d->actor->ln) { cpp_set_error("cpp_ddpg_last_feature_norm: the trainer's networks have no feature layer norm"); return CPP_ERR_STATE; }
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
