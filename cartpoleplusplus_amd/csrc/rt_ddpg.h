// The DDPG trainer and what its three translation units share: rt_ddpg.cpp (create / destroy, the optimiser's launch, the train ops and
// steps), rt_ddpg_pass.cpp (the gradient pass), rt_ddpg_config.cpp (the setters and the last_* accessors).  Internal, as rt_internal.h
#pragma once
#include "rt_internal.h"

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
  // pooled twin quantile critics (cpp_net_create_pooled_quantile: both critics with one N, or neither): twin, quant and dist_n = N at once.
  // quant_pool.hip stands where quant.hip stands and, for the actor, where actor_min.hip stands; quant_drop is d PER HEAD.  dist_p holds
  // theta^1 and pool_p2 theta^2 (maxB x N each), dist_tp the sorted pool and dist_m y (maxB x 2N each) for cpp_ddpg_last_pooled_quantiles
  bool pool = false; float* pool_p2 = nullptr;
  // soft actor-critic (cpp_net_create_gaussian: both actors Gaussian with one (lo, hi), or neither; cpp_ddpg_set_sac).  sac_w: the
  // temperature words (common.h: SAC_W_*), sac_step: Adam's count, sac_part: the partials of g_alpha the last actor pass left for a batch
  // of last.sac_rows rows (0: none yet); [0] / [1]: the draw at state_1 / state_2 -- eps (maxB x A), logp (maxB); sac_rsoft: the soft reward the
  // TD kernels read where they read the batch's reward.  The noise count is tps_n (smoothing is refused with SAC), owed as smoothing's is.
  // Target entropy, rate and seed are captured by value.
  bool sac = false; float sac_hbar = 0.f, sac_lr = 0.f; uint64_t sac_seed = 0;
  float* sac_w = nullptr; uint64_t* sac_step = nullptr; double* sac_part = nullptr;
  float *sac_eps[2] = {nullptr, nullptr}, *sac_logp[2] = {nullptr, nullptr}, *sac_rsoft = nullptr;
  // shared conv encoder (cpp_net_create_encoderless: both actors without conv layers, each bound to the critic beside it, or neither): the
  // actors read the critics' conv3 outputs, and only the critic's loss reaches the conv gradients.  trunk: the network whose conv1 decides
  // the form of a minibatch (direct_replay_ok) -- the critic then, the actor otherwise
  bool shared = false; cpp_net* trunk = nullptr;
  // parameter-space exploration noise (cpp_ddpg_set_param_noise; rt_ddpg_noise.cpp; common.h: PnWords).  pn_net: the perturbed copy of the
  // actor, the caller's network (nullptr: off); pn_words: sigma, the draw count, the last distance and whether the last resample adapted, on the
  // device; pn_a / pn_at: the two action batches of the last measured resample (maxB x A), pn_B its rows (0: none yet).  Target distance,
  // factor and seed travel by value in launches that are never captured: no graph knows of any of this
  cpp_net* pn_net = nullptr; PnWords* pn_words = nullptr; float pn_delta = 0.f, pn_alpha = 1.f; uint64_t pn_seed = 0;
  float *pn_a = nullptr, *pn_at = nullptr; int pn_B = 0;
};

// What a caller wants of the gradient pass: the halves to run -- the actor's (ddpg_cartpole.py:111-113, :220-222: dQ/da at actor(s1),
// pushed through the actor) and the critic's (:199-214: the TD loss against the target networks) -- and whether it trains.  train ==
// false is an evaluation (cpp_ddpg_check_loss, cpp_ddpg_q_gradients_wrt_actions): no critic backward, no noise drawn and nothing owed;
// soft actor-critic runs at eps = 0 and leaves the partials and the recorded temperature to the last training pass.
struct PassParts { bool actor = true, critic = true, train = true; };

// the gradient pass (rt_ddpg_pass.cpp)
int compute_gradients(cpp_ddpg* d, cpp_batch* b, PassLeft* left, int phase = 0, bool count_in_heads = false, const PerPass& per = PerPass(),
                      const PassParts& want = PassParts());

// (rt_ddpg.cpp) how every setter ends: the cached graphs miss at their next use, a minibatch presampled for the half steps goes with them
void reconfigured(cpp_ddpg* d);
// the minibatch's loss from the per-workgroup partials of the heads kernel or of dist.hip's job (b), added in a fixed order
float loss_of_parts(const double* parts, int n, int B);
// (rt_ddpg_config.cpp) soft actor-critic as cpp_ddpg_set_sac leaves it (cpp_ddpg_create: its defaults); the target actor as a bit copy of the actor
int sac_configure(cpp_ddpg* d, float init_temperature, float target_entropy, float lr, uint64_t seed);
int sac_sync_target(cpp_ddpg* d);
