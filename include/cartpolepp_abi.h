/*
 * cartpolepp_abi.h -- C ABI of libcartpolepp_hip.so (MI355X / gfx950).
 *
 * The reference (matpalm/cartpoleplusplus, /root/reference) has no FFI boundary of its own: its
 * DDPG-from-pixels hot path sits behind plain Python classes that call TensorFlow.  This header is
 * the boundary inserted directly beneath those classes; every entry point cites the reference
 * interface it replaces (paths relative to /root/reference).  Plain pointers and sizes only: no
 * torch types, no Python objects, no C++ exceptions cross.  INTEGRATION.md shows the ctypes stubs a
 * maintainer of the reference would add.
 *
 * Conventions
 *   - every function returns CPP_OK (0) or a CPP_ERR_* code; cpp_last_error() gives the message
 *     (thread-local).  Python wrappers raise RuntimeError(cpp_last_error()).
 *   - the library owns all device memory behind opaque handles; every *_create has a *_destroy.
 *   - host pointers are read/written only for the duration of the call.
 *   - a cpp_ctx is one GPU + one HIP stream; calls on one ctx are serialised by the caller
 *     (the reference is single-threaded: one implicit tf.Session).
 *   - results are f32-grade: IEEE f32 accumulation of products of the reference's f32 / f16 operands, far inside the 1e-5 the
 *     parity tests allow and measured as close to a float64 evaluation as f32-input matrix instructions get.  Where an operand
 *     already is an f16 number (conv1's input: the replay store's pixels, replay_memory.py:32) the other, f32, operand is split by
 *     round-to-nearest into f16 pieces and the f16 x f16 products -- each exact -- are accumulated in f32 (v_mfma_f32_16x16x32_f16):
 *     two pieces under CPP_PRECISION_FAST (the default: the operand to within 2^-22 relative, about one f32 ulp), three under
 *     CPP_PRECISION_EXACT (the operand itself).  conv2's forward and dW split BOTH f32 operands into three bf16 pieces (exactly) and
 *     issue the six largest of the nine piece products (FAST: the dropped three are at most half an f32 ulp of the product) or all
 *     nine (EXACT) (v_mfma_f32_16x16x32_bf16); everything else multiplies f32 operands directly (v_mfma_f32_16x16x4_f32).  Both
 *     modes are in the one release library: cpp_ctx_set_precision below.  DESIGN.md section 4.
 *     f32 states, odd layouts and B = 1 run on the f32-input MFMA kernels throughout.  The release library has no run-time kernel
 *     switches; the ablation build (libcartpolepp_hip_ablation.so, CARTPOLEPP_ABLATION=1) can force the f32-input kernels
 *     everywhere (CPP_CONV_K16=0 CPP_CONV_B16=0) -- bench.py's `control` run; bench.py's `control_exact_products` run is the
 *     release library under CPP_PRECISION_EXACT.
 *   - replay states are stored as f16 exactly like replay_memory.py:32 (or as their 8-bit pixel codes); indices are int32.
 *   - state batches handed to the conv kernels always live in the library's own guard-banded device allocations (host
 *     pointers are copied in first); the f16-pipe kernels refuse anything else.
 *   - flat parameter order = TF variable creation order "<scope>/weights", "<scope>/biases":
 *     conv1, conv2, conv3, then the fully connected layers.
 */
#ifndef CARTPOLEPP_ABI_H
#define CARTPOLEPP_ABI_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CPP_ABI_VERSION 1

enum { CPP_OK = 0, CPP_ERR_ARG = 1, CPP_ERR_HIP = 2, CPP_ERR_STATE = 3, CPP_ERR_NUMERIC = 4 };
enum { CPP_F32 = 0, CPP_F16 = 1,           /* host/device element type of state payloads        */
       CPP_U8 = 2 };                        /* replay store only: 8-bit pixel codes k, read back as f16(k/255) */
enum { CPP_ACTOR = 0, CPP_CRITIC = 1,       /* ddpg_cartpole.py:78 ActorNetwork / :148 CriticNetwork */
       CPP_HEAD = 2 };                      /* naf_cartpole.py: state network + one 'fc' head (value / mu / l_values) */
enum { CPP_OPT_SGD = 0, CPP_OPT_MOMENTUM = 1, CPP_OPT_ADAM = 2 };   /* util.py:73-76 tf.train.<name>Optimizer */

typedef struct cpp_ctx cpp_ctx;
typedef struct cpp_net cpp_net;
typedef struct cpp_batch cpp_batch;
typedef struct cpp_replay cpp_replay;
typedef struct cpp_ddpg cpp_ddpg;
typedef struct cpp_naf cpp_naf;
typedef struct cpp_comm cpp_comm;

/* ---- library / context ------------------------------------------------------------------- */
int cpp_abi_version(void);
const char* cpp_last_error(void);

/* One GPU + one stream.  `hip_stream` may be NULL (library creates its own non-blocking stream) or
 * an existing hipStream_t (e.g. torch.cuda.Stream().cuda_stream) so that host-side RCCL collectives
 * issued through torch.distributed are ordered with the kernels.  Replaces the implicit default
 * tf.Session of ddpg_cartpole.py:416. */
int cpp_ctx_create(int device_id, void* hip_stream, cpp_ctx** out);
int cpp_ctx_destroy(cpp_ctx* ctx);
int cpp_sync(cpp_ctx* ctx);

/* The arithmetic contract of the conv kernels that run on the f16 / bf16 matrix pipes (conv1 forward and dW, conv2 forward and
 * dW; everything else is f32-input MFMA or f32 VALU whatever the mode).  Accumulation is f32 and every issued product is exact
 * in both modes; the modes differ in how much of an f32 OPERAND reaches the multiplier:
 *   CPP_PRECISION_FAST  (default)  conv1's f32 operand (W s, dY) as two f16 pieces: the operand to within 2^-22 relative (~ one
 *                                  f32 ulp); conv2's operands as three bf16 pieces each with the six largest of the nine piece
 *                                  products (the dropped three: <= 2^-23 of a product).  Against the float64 oracle it is as
 *                                  close as the f32-input MFMA kernels (tests/test_gpu_fullsize.py, tests/test_gpu_render_inputs.py).
 *   CPP_PRECISION_EXACT            three f16 pieces / all nine products: no operand bit is dropped, the result is the
 *                                  f32-accumulated sum of the exact products of the f32 operands (rounds 1-2; ~0.87 x the speed).
 * The reference's TF CPU kernels multiply and accumulate in f32 (base_network.py:103-123 -> Eigen): both modes sit inside what
 * one f32 FMA chain rounds.  Must be called before a trainer (cpp_ddpg / cpp_naf) is created on the ctx -- captured step graphs
 * hold the kernels of the mode they were captured in -- and fails with CPP_ERR_ARG afterwards. */
#define CPP_PRECISION_FAST 0
#define CPP_PRECISION_EXACT 1
int cpp_ctx_set_precision(cpp_ctx* ctx, int mode);
int cpp_ctx_get_precision(cpp_ctx* ctx, int* mode);
/* Nearly constant channels.  The f16-pipe conv1 kernels multiply the replay store's RAW pixels by whitened weights; on a channel whose
 * whitening scale is ~10^3 and whose values do not cancel exactly (a blind camera with a rare off-colour pixel) that sits a few times
 * further from a float64 evaluation than whitening each element first, as base_network.py:95-99 does.  Every training call leaves the
 * largest scale of its whitening tables in pinned host memory, tagged with the call's number; above `threshold` (default 100; 0 =
 * never) later calls run conv1 forward / dW and conv2 forward on the f32-input kernels (which whiten per element) until the scale has
 * fallen under half of it.  WHICH call's scale a call decides from depends on the order of the caller's calls only, never on host /
 * GPU timing: call k reads call k - 2's (behind an event that guarantees it has landed; no wait in a loop that runs ahead of the
 * GPU), or call k - 1's if the stream has been synchronised since (cpp_sync, a parameter read, the eager pass in front of a graph
 * capture).  The first one or two affected calls therefore still run on the f16 pipes -- the same ones in every run.
 * cpp_ctx_get_route reports the current choice and the scale of the newest call known to have finished.  Only training calls feed the
 * scale: the gathers of cpp_replay_sample and cpp_replay_gather_shifted are inspections, and what they whiten never reaches a later
 * call's choice. */
int cpp_ctx_set_route_threshold(cpp_ctx* ctx, float threshold);
int cpp_ctx_get_route(cpp_ctx* ctx, int* conv1_f32, float* last_max_scale);

/* HIP-event stopwatch on the ctx stream (bench.py; the reference only has util.StopWatch, util.py:22). */
int cpp_timer_begin(cpp_ctx* ctx);
int cpp_timer_end(cpp_ctx* ctx, float* elapsed_ms);

/* Per-kernel HIP-event profile of the launches issued on this ctx (disables graph replay while on).
 * kernel ids: see cpp_prof_kernel_name(). */
int cpp_prof_enable(cpp_ctx* ctx, int on);
int cpp_prof_reset(cpp_ctx* ctx);
int cpp_prof_num_kernels(void);
const char* cpp_prof_kernel_name(int kernel_id);
int cpp_prof_read(cpp_ctx* ctx, int kernel_id, double* total_ms, int64_t* launches);

/* ---- networks (base_network.py:13-134, ddpg_cartpole.py:78-100, :148-184) ------------------- */
typedef struct cpp_net_spec {
  int32_t kind;          /* CPP_ACTOR / CPP_CRITIC                                              */
  int32_t pixel;         /* opts.use_raw_pixels: conv trunk (base_network.py:73-127) in front    */
  int32_t H, W, C;       /* pixel: image dims, C = 3*num_cameras*action_repeats (:85-90)         */
  int32_t state_elems;   /* low-dim: flattened state length (repeats*2*7, bullet_cartpole.py:125) */
  int32_t action_dim;
  int32_t n_hidden;      /* actor: opts.actor_hidden_layers; low-dim critic: critic_hidden_layers */
  int32_t hidden[8];     /* (pixel critic is the fixed 200/50/+action/50 head of :168-171)       */
  int32_t head_out;      /* CPP_HEAD: outputs of the 'fc' head (1, action_dim, action_dim*(action_dim+1)/2) */
  int32_t head_act;      /* CPP_HEAD: 0 linear, 2 tanh (naf_cartpole.py:109,161,184)              */
  int32_t use_batch_norm; /* opts.use_batch_norm (base_network.py:74-79): slim.batch_norm after every conv; the conv then has no
                           * bias and the '<conv>/biases' slot of the flat layout is '<conv>/BatchNorm/beta'.  Training-mode
                           * entry points (the train ops) use batch statistics, inference-mode ones (cpp_net_forward*,
                           * check_loss, NAF action / debug) the never-updated moving averages (mean 0, variance 1).  */
  int32_t use_dropout;   /* opts.use_dropout (base_network.py:69-70): slim.dropout (keep 0.5) after the ReLU of every layer made by
                          * hidden_layers_starting_at *with opts* -- the actor's and the NAF networks' hidden stacks; the critics
                          * have none (ddpg_cartpole.py:168-177).  Training-mode entry points draw the keep bits from
                          * Philox4x32-10(key = dropout_seed; counter = (row * units + unit, layer, forward count)).
                          * The forward count is per network: the number of training-mode forwards of its hidden stack so far.  Every
                          * minibatch of every training entry point (the fused steps, *_train_rows*, *_sample_and_compute, the
                          * data-parallel steps, eager or replayed from a captured graph) advances it by one, behind the layers that
                          * read it; the stand-alone actor op counts the actor, the critic op the target actor.  Inference-mode entry
                          * points neither drop a unit nor count.  Delayed policy updates (cpp_ddpg_set_policy_delay, d > 1) hold the
                          * actor's optimiser step alone: a minibatch whose actor update is held still runs the actor's and the target
                          * actor's forward in training mode, so it draws masks and is counted -- minibatch k of a trainer (from 0)
                          * draws count k in both networks whatever d is. */
  uint32_t dropout_seed;
} cpp_net_spec;

int cpp_net_create(cpp_ctx* ctx, const cpp_net_spec* spec, int max_batch, cpp_net** out);
/* Twin Q heads (TD3's clipped double-Q, Fujimoto et al. 2018, Algorithm 1, on a shared representation as in DrQ-v2), an extension of
 * the critic ddpg_cartpole.py:166-171 (pixel) / :172-177 (low-dimensional): a critic whose layers from the concat layer upward exist
 * twice.  The first cpp_net_num_params(plain critic) floats of the flat buffer are laid out exactly as cpp_net_create's critic --
 * names, shapes, offsets --; the twin variables follow in creation order: 'hidden3b/weights', 'hidden3b/biases', 'q_valueb/weights',
 * 'q_valueb/biases' (pixel); 'h<i>b/...' for every hidden layer, then 'q_valueb/...' (low-dimensional: the whole stack is twinned,
 * which is TD3 exactly).  spec->kind must be CPP_CRITIC (CPP_ERR_ARG otherwise).  Head 1 is the plain critic's: cpp_net_forward*
 * evaluate it and never read head 2.  A trainer built on twin critics (cpp_ddpg_create: both critics, or neither) is a twin trainer:
 *     y = r + mask discount min(Q1'(s2, a'), Q2'(s2, a')),  td_k = Q_k(s1, a) - y,  loss = mean_b(w_b (td_1^2 + td_2^2))
 * with ONE a' for both target heads (target policy smoothing: one noise draw).  The gradient into the shared layer below the concat
 * layer is head 1's term plus head 2's, added in that order, then the ReLU mask.  The actor follows dQ1/da only (unless cpp_ddpg_set_actor_min_q); priorities,
 * cpp_ddpg_last_values, cpp_ddpg_check_loss's td and q and q_gradients_wrt_actions stay head 1's; the loss they report is the twin
 * loss.  The clip's norm, the optimiser slots, the soft update and the collectives cover the longer buffer.  cpp_naf_create refuses
 * twin networks. */
int cpp_net_create_twin_q(cpp_ctx* ctx, const cpp_net_spec* spec, int max_batch, cpp_net** out);
/* 1 for a network made by cpp_net_create_twin_q, 0 for any other (NULL included) */
int cpp_net_is_twin_q(const cpp_net* net);
/* Distributional (categorical) critic: Bellemare et al. 2017 ("C51") as the critic of D4PG (Barth-Maron et al. 2018), an extension of the
 * critic ddpg_cartpole.py:166-171 (pixel) / :172-177 (low-dimensional) and of its target :199-214.  The layout is cpp_net_create's critic
 * except that 'q_value/weights' is (n_in, N) and 'q_value/biases' is (N): the last layer emits N logits.  spec->kind must be CPP_CRITIC,
 * 2 <= N <= 64, v_min < v_max, both finite (CPP_ERR_ARG otherwise).  All arithmetic below is float32.
 *   support   z_i = v_min + i * delta,  delta = (v_max - v_min) / (N - 1),  i = 0 .. N-1
 *   p = softmax(logits), the row maximum subtracted first;  Q = sum_i p_i z_i
 * cpp_net_forward* return Q (width 1).  A trainer built on such critics (cpp_ddpg_create: both critics with equal (N, v_min, v_max), or
 * neither; never together with twin Q heads) trains, per row b of the minibatch,
 *   g    = mask_b * discount              (an n-step memory has folded its powers into mask, as for the scalar target)
 *   a'   = mu'(s2), smoothed if target policy smoothing is on;   p' = softmax(target critic's logits at (s2, a'))
 *   Tz_j = clamp(r_b + g * z_j, v_min, v_max),   b_j = (Tz_j - v_min) / delta
 *   m_i  = sum_j p'_j * max(0, 1 - |b_j - i|),   summed in the order j = 0 .. N-1
 *   L_b  = -sum_i m_i log p_i(s1, a_fed),   loss = mean_b(w_b L_b)   (w: importance weights, 1 without prioritized replay)
 * The triangular kernel is the usual floor / ceil scatter of the projection, puts the whole mass on atom b_j when b_j is an integer, needs
 * no atomics and has one summation order.  The gradient into the fed evaluation's logits is (w_b / B) (p_i - m_i).  The actor follows
 * dQ/da at a = mu(s1): the gradient entering the critic's last layer on that evaluation is p_i (z_i - Q) where the scalar critic feeds ones.
 *   y_b  = sum_i m_i z_i  (= r + g Q' whenever no clamp binds),   td_b = Q(s1, a_fed) - y_b
 * is what priorities, cpp_ddpg_last_values and cpp_ddpg_check_loss's td read; their q is Q; the loss they report is the cross-entropy.
 * Such a trainer always takes the GEMM levels of the gradient pass; batches up to 1024.  cpp_naf_create refuses such networks.  The support
 * is not part of a checkpoint: a mismatch in N fails the layout check, (v_min, v_max) are the creator's to keep. */
int cpp_net_create_distributional(cpp_ctx* ctx, const cpp_net_spec* spec, int max_batch, int n_atoms, float v_min, float v_max, cpp_net** out);
/* (N, v_min, v_max) of a network made by cpp_net_create_distributional; n_atoms 0 for any other.  NULL pointers are skipped. */
int cpp_net_distribution_info(const cpp_net* net, int* n_atoms, float* v_min, float* v_max);
/* Quantile critic: quantile regression (Dabney et al. 2018, QR-DQN) with truncated targets (Kuznetsov et al. 2020, TQC, within one network),
 * an extension of the critic ddpg_cartpole.py:166-171 (pixel) / :172-177 (low-dimensional) and of its target :199-214.  The layout is
 * cpp_net_create_distributional's: 'q_value/weights' is (n_in, N), 'q_value/biases' is (N).  Output i, theta_i(s, a), estimates the
 * quantile at tau_i = (2 i + 1) / (2 N); there is no support to configure.  spec->kind must be CPP_CRITIC, 2 <= N <= 64 (CPP_ERR_ARG
 * otherwise).  All arithmetic below is float32 except the loss, whose terms are formed and added in float64.
 *   Q(s, a) = (sum_i theta_i) / N
 * cpp_net_forward* return Q (width 1).  A trainer built on such critics (cpp_ddpg_create: both critics with one N, or neither; never with
 * twin Q heads, never mixed with categorical ones) trains, per row b of the minibatch, with kappa and d of cpp_ddpg_set_quantile_target,
 *   g      = mask_b * discount              (an n-step memory has folded its powers into mask, as for the scalar target)
 *   a'     = mu'(s2), smoothed if target policy smoothing is on;   theta' = the target critic's N outputs at (s2, a')
 *   s_0 <= s_1 <= .. <= s_{N-1}             theta' sorted ascending (always, also with d = 0: one summation order)
 *   M      = N - d;   y_j = r_b + g * s_j,  j = 0 .. M-1          the d largest target atoms are dropped
 *   u_ij   = y_j - theta_i(s1, a_fed)
 *   H(u)   = u^2 / 2 if |u| <= kappa, else kappa (|u| - kappa / 2)
 *   rho_ij = |tau_i - [u_ij < 0]| * H(u_ij) / kappa
 *   L_b    = (1 / (N M)) sum_i sum_j rho_ij   (j ascending inside i),   loss = mean_b(w_b L_b)   (w: importance weights, 1 without them)
 *   d theta_i = -(w_b / B) (1 / (N M)) sum_j |tau_i - [u_ij < 0]| * clip(u_ij, -kappa, kappa) / kappa
 *   td_b   = Q(s1, a_fed) - (sum_{j<M} y_j) / M
 * td is what priorities, cpp_ddpg_last_values and cpp_ddpg_check_loss's td read; their q is Q; the loss they report is the quantile Huber
 * loss.  Truncation works on values: ties among the theta' cannot change any result.  The actor follows dQ/da at a = mu(s1): the gradient
 * entering the critic's last layer on that evaluation is the constant 1 / N where the scalar critic feeds ones.  Such a trainer always
 * takes the GEMM levels of the gradient pass; batches up to 1024.  cpp_naf_create refuses such networks.  A checkpoint carries the N-wide
 * q_value by name: a mismatch in N fails the layout check.  cpp_net_distribution_info answers n_atoms = 0 for such a network. */
int cpp_net_create_quantile(cpp_ctx* ctx, const cpp_net_spec* spec, int max_batch, int n_quantiles, cpp_net** out);
/* N of a network made by cpp_net_create_quantile (the critic of ddpg_cartpole.py:166-177 widened); 0 for any other.  NULL is skipped. */
int cpp_net_quantile_info(const cpp_net* net, int* n_quantiles);
/* Pooled twin quantile critics: Truncated Quantile Critics (Kuznetsov et al. 2020, TQC) with two heads on one representation, an extension
 * of the critic ddpg_cartpole.py:166-171 (pixel) / :172-177 (low-dimensional) and of its target :199-214.  The layout is
 * cpp_net_create_twin_q's with both q layers N wide: the plain critic's variables first ('q_value/weights' (n_in, N), 'q_value/biases' (N)),
 * then head 2's copy of the layers from the concat layer upward ('hidden3b/*', 'q_valueb/*'; low-dimensional: 'h<i>b/*', 'q_valueb/*').
 * spec->kind must be CPP_CRITIC, 2 <= N <= 32: the pool of both heads' atoms fills the 64 lanes of one wave (CPP_ERR_ARG otherwise).  All
 * arithmetic below is float32 except the loss, whose terms are formed and added in float64.  Per row b, with kappa and d (PER HEAD) of
 * cpp_ddpg_set_quantile_target:
 *   theta^k_i  = atom i of online head k at (s1, a_fed), k = 1, 2, i < N;   tau_i = (2 i + 1) / (2 N)
 *   z          = (theta'^1_0 .. theta'^1_{N-1}, theta'^2_0 .. theta'^2_{N-1}): both target heads at (s2, a'), ONE a' (smoothed, or soft
 *                actor-critic's sample)
 *   s          = z sorted ascending (2N values, always sorted, also at d = 0);   M = 2N - 2d;   g = mask_b * discount
 *   y_j        = r* + g s_j, j < M;   r* = r_b, or r_soft under soft actor-critic (cpp_ddpg_set_sac)
 *   u^k_ij     = y_j - theta^k_i;   H and rho as in cpp_net_create_quantile's text
 *   L^k_b      = (1 / (N M)) sum_i sum_j rho^k_ij   (j ascending inside i);   L_b = L^1_b + L^2_b;   loss = mean_b(w_b L_b)
 *   d theta^k_i = -(w_b / B) (1 / (N M)) sum_j |tau_i - [u^k_ij < 0]| clip(u^k_ij, -kappa, kappa) / kappa
 *   Q_k = (sum_i theta^k_i) / N;   Qbar = (Q_1 + Q_2) / 2
 *   td_b = Q_1 - (sum_{j<M} y_j) / M;   td2_b = Q_2 - the same mean
 * td (head 1's, as for every twin critic) is what priorities, cpp_ddpg_last_values and cpp_ddpg_check_loss read; cpp_ddpg_last_twin_values
 * reads Q_2, Q_1', Q_2' (the target heads' own means, before pooling) and td2.  The actor ascends Qbar(s1, mu(s1)): the gradient entering
 * BOTH q layers on that evaluation is the constant 1 / (2N), and dq_da = dQbar/da; a soft actor-critic trainer's actor minimises
 * alpha logp - Qbar.  cpp_net_forward* return Q_1 (width 1) and cpp_ddpg_q_gradients_wrt_actions returns Q_1 beside dQbar/da, as
 * cpp_ddpg_set_actor_min_q returns Q_1 beside the minimum's gradient.  Truncation works on values: ties cannot change any result.
 * cpp_ddpg_create accepts such critics only as a pair with one N, under plain or Gaussian actors; cpp_ddpg_set_actor_min_q and
 * cpp_ddpg_set_behaviour_cloning refuse such a trainer, which always takes the GEMM levels of the gradient pass; batches up to 1024.
 * cpp_naf_create refuses such networks.  A checkpoint carries every variable by name: it fails the layout check against a twin, a quantile
 * or a plain critic, and against another N.  cpp_net_quantile_info and cpp_net_distribution_info answer 0 for such a network,
 * cpp_net_is_twin_q answers 1. */
int cpp_net_create_pooled_quantile(cpp_ctx* ctx, const cpp_net_spec* spec, int max_batch, int n_quantiles, cpp_net** out);
/* The same critic behind cpp_net_create_feature_norm's layer norm on fully connected layer 0 (an extension of ddpg_cartpole.py:168 'hidden1';
 * that entry's variant record names one variant at a time).  Its rules for a critic hold: pixel, no batch norm, no dropout, activation
 * CPP_NORM_TANH or CPP_NORM_RELU, a finite positive epsilon; gamma and beta sit behind head 2's variables. */
int cpp_net_create_pooled_quantile_norm(cpp_ctx* ctx, const cpp_net_spec* spec, int max_batch, int n_quantiles, int activation, float epsilon,
                                        cpp_net** out);
/* N per head of a network made by cpp_net_create_pooled_quantile(_norm) (the critic of ddpg_cartpole.py:166-177 widened); 0 for any other.
 * NULL is skipped. */
int cpp_net_pooled_quantile_info(const cpp_net* net, int* n_quantiles);
/* Gaussian actor: the stochastic tanh-Gaussian policy of soft actor-critic (Haarnoja et al. 2018), an extension of the actor
 * ddpg_cartpole.py:95-100.  The layout is cpp_net_create's actor except that 'output_action/weights' is (n_in, 2A) and
 * 'output_action/biases' is (2A): the last layer is linear and emits (m_k, x_k), k < A -- m in columns [0, A), x in [A, 2A).  spec->kind
 * must be CPP_ACTOR, lo < hi both finite, 1 <= A <= 64 (CPP_ERR_ARG otherwise; a trainer needs a critic, whose A is at most 16).  All
 * arithmetic below is float32, every operation rounded on its own, sums over k ascending from 0.
 *   ls_k = lo + (0.5 (hi - lo)) (tanh(x_k) + 1)                 smooth bounds, no kinks
 *   u_k  = m_k + exp(ls_k) eps_k ;   a_k = tanh(u_k)
 *   logp = sum_k [ ((-0.5 eps_k^2 - ls_k) - 0.5 log(2 pi)) - 2 ((log 2 - u_k) - softplus(-2 u_k)) ]
 *   softplus(y) = max(y, 0) + log1p(exp(-|y|))                  the stable form, never log(1 - a^2 + 1e-6)
 * cpp_net_forward* return tanh(m) (eps = 0, width A); cpp_net_forward_gaussian returns m and ls for host-side sampling.
 * A trainer built on such actors (cpp_ddpg_create: both actors Gaussian with one (lo, hi), or neither; never with distributional or
 * quantile critics, batch norm or dropout; batches up to 1024) is a soft actor-critic trainer.  With alpha = exp(log_alpha), log_alpha
 * one f32 in device memory, per row b of minibatch t:
 *   eps    the unclipped Box-Muller z = sqrt(-2 log u1) cospi(2 u2) on two 24-bit uniforms of
 *          philox4x32_10({row, S + k, n_lo, n_hi}, seed), S = 0x200 for the draw at state_1, 0x300 for the draw at state_2; n counts the
 *          target-forming gradient passes since cpp_ddpg_set_sac (a device word: a replayed graph draws fresh noise; the pass that reads
 *          it never writes it, the optimiser's launch behind it or a launch of its own does)
 *   a', logp'  a sample of the policy as it stood before t's actor update, at state_2 (SAC has no target actor: the target actor's
 *          parameters are a bit copy of the actor's, made behind every launch that applies the critic's list and when SAC is configured;
 *          the soft update no longer decides them)
 *   r_soft = r - ((mask discount) alpha) logp' ;   td = Q(s1, a_fed) - (r_soft + mask discount Q'(s2, a'))
 *          (twin heads: min(Q1', Q2'); an n-step memory has folded its powers into mask) -- priorities, cpp_ddpg_last_values and
 *          cpp_ddpg_check_loss read this td; check_loss keeps the entropy term at eps = 0 and draws nothing
 *   actor  minimises sum_b (alpha logp - Q(s1, a)) at a sample a at state_1 (twin heads: head 1; cpp_ddpg_set_actor_min_q: min(Q1, Q2)(s1, a), row by row).  With dq = dQ/da_k:
 *          g_u = 2 alpha a_k - dq (1 - a_k^2);   d m_k = g_u;   d x_k = ((g_u exp(ls_k)) eps_k - alpha) * ((0.5 (hi - lo)) (1 - tanh(x_k)^2))
 *   temperature  g_alpha = -(1/B) sum_b (logp_b + Hbar), the gradient of -log_alpha (logp + Hbar), from per-workgroup f64 partials (four
 *          rows each, in order) added in order; applied by Adam (TensorFlow's semantics, betas 0.9 / 0.999, epsilon 1e-8) at the
 *          temperature's rate, in a launch of its own when the actor's list is applied; rate 0: a fixed temperature, no launch.
 *          Both passes of minibatch t read the temperature as it stood before t's update.
 * cpp_ddpg_q_gradients_wrt_actions evaluates at eps = 0.  Such a trainer always takes the GEMM levels of the gradient pass, refuses
 * target policy smoothing, a policy delay above 1 and the data-parallel entry points.  cpp_naf_create refuses such networks.  A
 * checkpoint carries the 2A-wide head by name: a plain checkpoint fails the layout check, in both directions. */
int cpp_net_create_gaussian(cpp_ctx* ctx, const cpp_net_spec* spec, int max_batch, float log_std_min, float log_std_max, cpp_net** out);
/* gaussian = 1 and (lo, hi) of a network made by cpp_net_create_gaussian (the actor of ddpg_cartpole.py:95-100 widened); 0 for any other. */
int cpp_net_gaussian_info(const cpp_net* net, int* gaussian, float* log_std_min, float* log_std_max);
/* The head of a Gaussian actor on a fed state batch (ddpg_cartpole.py:123-125 widened; the exploration noise of :127-134 stays on the
 * host): m and ls, each (B, A); each != 0: every row whitened with its own statistics, as cpp_net_forward_each. */
int cpp_net_forward_gaussian(cpp_net* net, const void* state, int state_dtype, int B, int each, float* m, float* ls);
/* Feature layer norm: Linear -> LayerNorm -> tanh on the first fully connected layer, between the conv features and the MLP (the trunk of
 * DrQ-v2, Yarats et al. 2021; layer normalisation: Ba et al. 2016), an extension of the actor's 'h0' (ddpg_cartpole.py:95, through
 * base_network.py:64-71) and of the pixel critic's 'hidden1' (ddpg_cartpole.py:168).  Pixel networks only.  Per row b of layer 0, of width
 * n <= 1024, with z = [x, 1][W; b] from the layer's GEMM, which has no activation of its own.  All arithmetic is float32, every operation
 * rounded on its own:
 *   mu = mean_j z_j          var = mean_j (z_j - mu)^2          (biased, two passes)
 *   rstd = 1 / sqrt(var + epsilon)          xhat_j = (z_j - mu) rstd
 *   u_j = gamma_j xhat_j + beta_j           y_j = act(u_j),  act = tanh (CPP_NORM_TANH) or relu (CPP_NORM_RELU)
 * Backward, with g = dL/dy from the layer above (no activation derivative applied yet):
 *   du = g act'(y)           (1 - y^2, or y > 0)
 *   dgamma_j = sum_b du_bj xhat_bj          dbeta_j = sum_b du_bj          (one fixed order, a function of B alone: sixteen contiguous
 *                                                                           parts of the batch, b ascending in each, added in order)
 *   dxh = du gamma           dz = rstd ((dxh - mean_j dxh) - xhat mean_j(dxh xhat))
 * and dz feeds layer 0's [dW; db] and the gradient of the conv features unchanged.  There is no training / inference distinction: target
 * networks, cpp_net_forward*, cpp_ddpg_check_loss and every train op normalise the same way.
 * Layout: two variables, '<layer0>/LayerNorm/gamma' and '<layer0>/LayerNorm/beta', each (n), behind EVERY other variable of the network
 * (twin ones included): the first cpp_net_num_params(the same network without the norm) floats keep their names, shapes and offsets.  The
 * clip's norm, the optimiser slots, the soft update, soft actor-critic's target-actor copy and the collectives cover the longer buffer.
 * The constructor leaves gamma = 1, beta = 0.  A checkpoint carries both by name: a plain checkpoint fails the layout check, in both directions.
 * variant (NULL: the plain network): what the network is besides -- at most one of twin_q (cpp_net_create_twin_q), n_atoms with
 * (v_min, v_max) (cpp_net_create_distributional), n_quantiles (cpp_net_create_quantile), gaussian with the log std bounds
 * (cpp_net_create_gaussian), each under that constructor's rules.
 * CPP_ERR_ARG, by name and before anything is allocated: a low-dimensional network, use_batch_norm, use_dropout, a CPP_HEAD network, an
 * activation other than the two, epsilon not finite and positive.  cpp_naf_create refuses such networks; cpp_ddpg_create takes four of
 * them with one activation and one epsilon, or none.  The fused heads launch of the gradient pass never owns the normalised layer's
 * activation derivative: an actor with three or more hidden layers keeps the default route, one with two hidden layers keeps the heads
 * launch without its leading actor layer, one with a single hidden layer takes the GEMM levels. */
#define CPP_NORM_TANH 0
#define CPP_NORM_RELU 1
typedef struct cpp_net_variant {
  int32_t twin_q;                        /* != 0: twin Q heads                                  */
  int32_t n_atoms; float v_min, v_max;   /* n_atoms != 0: a categorical value distribution      */
  int32_t n_quantiles;                   /* != 0: a quantile critic                             */
  int32_t gaussian; float log_std_min, log_std_max;   /* gaussian != 0: a Gaussian actor        */
} cpp_net_variant;
int cpp_net_create_feature_norm(cpp_ctx* ctx, const cpp_net_spec* spec, int max_batch, const cpp_net_variant* variant, int activation,
                                float epsilon, cpp_net** out);
/* on = 1, the activation and epsilon of a network made by cpp_net_create_feature_norm; on = 0 for any other.  NULL pointers are skipped. */
int cpp_net_feature_norm_info(const cpp_net* net, int* on, int* activation, float* epsilon);
/* Shared conv encoder: the actor reads the critic's features (SAC-AE, Yarats et al. 2019; DrQ, Kostrikov et al. 2020; DrQ-v2, Yarats et
 * al. 2021), an extension of ddpg_cartpole.py:78-100 and :148-171, where each of the four networks runs base_network.py:73-127 on its own.
 * Pixel DDPG learners only.  Definition:
 *   - The actor and the target actor have NO conv variables: cpp_net_create_encoderless makes a pixel actor whose variable list is its
 *     fully connected layers alone ('h<i>', 'output_action', then the feature layer norm's pair if any), from offset 0.  Flat buffers,
 *     gradient lists, optimiser slots, the clip's norm, soft updates, soft actor-critic's target-actor copy, checkpoints and the
 *     collectives cover that shorter buffer.  'h0/weights' is (flat, n) with flat the width of the critic's flattened conv3 output.
 *   - cpp_net_set_encoder(actor, critic) binds such an actor to a pixel critic of the same image geometry, action_dim, context and
 *     max_batch (no batch norm): the actor's layer 0 reads the critic's flattened conv3 output of the same state -- the very buffer,
 *     whose bias column of ones serves both; no copy and no second conv forward.  An actor is bound once (a second call answers CPP_ERR_ARG); cpp_net_destroy of
 *     the critic leaves its actors unbound again, and their forwards then answer CPP_ERR_STATE.
 *   - cpp_ddpg_create takes encoder-less actors only as a pair: the actor bound to the critic, the target actor bound to the target
 *     critic (CPP_ERR_ARG otherwise).  The target actor therefore reads the target critic's conv3 output at state_2: a' = mu'(s2) is
 *     computed on the soft-updated encoder.  Four networks and the target update as before.
 *   - Stop gradient: the actor's backward pass ends at its layer-0 [dW; db].  No dX of that layer is formed, nothing of the actor's
 *     objective reaches a conv gradient: the encoder's gradient is exactly the critic's loss gradient, and the encoder is stepped by
 *     the critic's optimiser, rate and clip alone.
 *   - Conv launches of a minibatch: forward {critic @ s1, target critic @ s2} (one trained network, one target), backward {critic};
 *     the dW-reduction launch carries three layers x one network.  A single half (cpp_ddpg_train_actor alone) runs the critic's trunk
 *     on s1 and no conv backward.
 *   - Soft actor-critic: the target actor stays a bit copy of the actor's (fully connected) parameters; (a', logp') are sampled on the
 *     target critic's features.  No conv1 operand image is rebuilt for it: it has no conv1.
 *   - Inference: cpp_net_forward, cpp_net_forward_each and cpp_net_forward_gaussian of such an actor run the bound critic's trunk in
 *     inference mode on the given states (its staging buffers, statistics and first workspace), then the actor's fully connected
 *     stack; an actor that is not bound yet answers CPP_ERR_STATE.
 * norm: CPP_NORM_NONE, or the feature layer norm's activation with its epsilon (cpp_net_create_feature_norm's rules).  variant (NULL:
 * plain): only `gaussian` with its bounds (cpp_net_create_gaussian's rules).
 * CPP_ERR_ARG, by name and before anything is allocated: a network that is not a CPP_ACTOR, a low-dimensional network, use_batch_norm,
 * use_dropout, a critic's variant.  cpp_naf_create has no actor and takes none. */
#define CPP_NORM_NONE (-1)
int cpp_net_create_encoderless(cpp_ctx* ctx, const cpp_net_spec* spec, int max_batch, const cpp_net_variant* variant, int norm, float epsilon,
                               cpp_net** out);
int cpp_net_set_encoder(cpp_net* actor, cpp_net* critic);
/* encoderless = 1 for a network made by cpp_net_create_encoderless, bound = 1 once cpp_net_set_encoder has bound it.  NULL pointers are skipped. */
int cpp_net_encoder_info(const cpp_net* net, int* encoderless, int* bound);
int cpp_net_destroy(cpp_net* net);
/* Network.trainable_model_vars (base_network.py:51-56): variables in creation order. */
int64_t cpp_net_num_params(const cpp_net* net);
int cpp_net_num_vars(const cpp_net* net);
int cpp_net_var_info(const cpp_net* net, int i, char* name, int name_cap, int* rank,
                     int shape[4], int64_t* offset);
/* variable init / checkpoint restore / SIGUSR2 weight dump (ddpg_cartpole.py:421-427, :402-409) */
int cpp_net_set_params(cpp_net* net, const float* host, int64_t n);
int cpp_net_get_params(cpp_net* net, float* host, int64_t n);
int cpp_net_get_grads(cpp_net* net, float* host, int64_t n);   /* pre-clip gradients of last train */
/* Network._create_variables_copy_op (base_network.py:20-33): target -= coeff * (target - source). */
int cpp_net_soft_update(cpp_net* target, const cpp_net* source, float coeff);
/* session.run(output_action | q_value) on a fed state batch (ddpg_cartpole.py:123-125).  `state` is
 * a host array (B, state_elems) of `state_dtype`; `action` (B, action_dim) host f32, critics only.
 * Whitening always uses the statistics of THIS batch (base_network.py:95-99), also at B = 1. */
int cpp_net_forward(cpp_net* net, const void* state, int state_dtype, int B, const float* action,
                    float* out);
/* B independent `action_given` calls (ddpg_cartpole.py:121-126 once per row) in one pass: every image is whitened with
 * its OWN statistics (base_network.py:95-99 at batch size 1), so row i of `out` equals cpp_net_forward on row i alone.
 * Rollout-side inference for many env workers. */
int cpp_net_forward_each(cpp_net* net, const void* state, int state_dtype, int B, const float* action,
                         float* out);
/* Network.pool1/2/3 (base_network.py:108,116,124) of the last forward: which = 1..3, (B,h,w,10).
 * Debug: which = 11..13 returns the arg-max codes (0..3, as floats) of the same layers' 2x2 windows. */
int cpp_net_get_pool(cpp_net* net, int which, int B, float* out);

/* ---- minibatch resident in HBM (replay_memory.py:9 Batch) ----------------------------------- */
int cpp_batch_create(cpp_ctx* ctx, int max_batch, int64_t state_elems, int action_dim, cpp_batch** out);
int cpp_batch_destroy(cpp_batch* batch);
/* feed_dict of ddpg_cartpole.py:231-237: host Batch -> device. */
int cpp_batch_upload(cpp_batch* batch, int B, const void* state_1, const void* state_2,
                     int state_dtype, const float* action, const float* reward,
                     const float* terminal_mask);
/* np.copy(...) columns of replay_memory.py:134-138: device -> caller-owned host arrays.  States come
 * back in the batch's stored dtype (f16 after cpp_replay_sample). */
int cpp_batch_download(cpp_batch* batch, void* state_1, void* state_2, float* action,
                       float* reward, float* terminal_mask);
int cpp_batch_size(const cpp_batch* batch);
int cpp_batch_state_dtype(const cpp_batch* batch);

/* ---- replay memory payload in HBM (replay_memory.py:11-138) --------------------------------- */
/* Slot allocation / eviction (replay_memory.py:66,84,90,104) stays on the host so the FIFO order is
 * exact; the device holds the f16 state store and mirrors of the five event columns. */
int cpp_replay_create(cpp_ctx* ctx, int buffer_size, int state_slots, int64_t state_elems,
                      int action_dim, cpp_replay** out);
/* The same with a chosen store type: CPP_F16, or CPP_U8 -- 8-bit pixel codes k that read back as f16(k/255), i.e. exactly what
 * the f16 store holds for the reference's renders (bullet_cartpole.py:239-243) in half the HBM.  A CPP_U8 memory refuses states
 * that are not such images (cpp_replay_write_states returns an error). */
int cpp_replay_create_ex(cpp_ctx* ctx, int buffer_size, int state_slots, int64_t state_elems,
                         int action_dim, int store_dtype, cpp_replay** out);
int cpp_replay_destroy(cpp_replay* replay);
/* self.state[idx] = s (replay_memory.py:67,106): n states, f32 is rounded to f16 (RNE) like numpy. */
int cpp_replay_write_states(cpp_replay* replay, const int32_t* slots, int n, const void* states,
                            int state_dtype);
/* rows of the five event columns (replay_memory.py:94-101,105). */
int cpp_replay_write_rows(cpp_replay* replay, const int32_t* rows, int n, const int32_t* state_1_idx,
                          const int32_t* state_2_idx, const float* action, const float* reward,
                          const float* terminal_mask);
/* the same columns read back from the device for n rows (any of the outputs may be NULL) -- replay_memory.py's public attributes
 * state_1_idx / action / reward / terminal_mask / state_2_idx (:22-29) as the sampler sees them */
int cpp_replay_read_rows(cpp_replay* replay, const int32_t* rows, int n, int32_t* s1_idx, int32_t* s2_idx, float* action,
                         float* reward, float* terminal_mask);
/* Keep per-state whitening sums (sum x, sum x^2 per channel, f64) in the store for `channels` interleaved channels: the statistics of
 * base_network.py:95-96 for a sampled minibatch then cost 2 B rows of 2 C doubles instead of a pass over 2 B images.  Results are
 * bit-identical (the same per-image sums, added in the same order).  0 turns them off. */
int cpp_replay_set_stats_channels(cpp_replay* replay, int channels);
int cpp_replay_set_size(cpp_replay* replay, int size);          /* ReplayMemory.size(), :120 */
int cpp_replay_read_states(cpp_replay* replay, const int32_t* slots, int n, void* out_f16);
/* random_indexes + batch (replay_memory.py:123-138) fused: idxs == NULL draws B uniform rows on the
 * device with Philox4x32-10 keyed (seed, counter); otherwise uses the caller's rows (parity tests,
 * numpy-RNG-driven callers).  Also produces the per-channel whitening statistics of both state
 * batches for pixel states of `channels` interleaved channels (channels = 0: none). */
int cpp_replay_sample(cpp_replay* replay, int B, const int32_t* idxs, uint64_t seed, uint64_t counter,
                      int channels, cpp_batch* out);
int cpp_replay_last_indexes(cpp_replay* replay, int B, int32_t* out);   /* rows drawn by last sample */
/* bench/test helper: fill n_rows transitions on the device (SURVEY 8d synthetic inputs):
 * states f16(k/255), k~U{0..255}; a~U(-1,1); reward 1; terminal w.p. 1/50; s2 = s1 slot + 1. */
int cpp_replay_fill_synthetic(cpp_replay* replay, int n_rows, uint64_t seed);

/* ---- prioritized experience replay (Schaul et al. 2016, proportional variant) on the device ----------------------------------
 * Extension, no reference counterpart (the reference samples uniformly, replay_memory.py:123-129).  Opt-in per memory; a memory
 * without cpp_replay_enable_priorities behaves exactly as before.  Semantics:
 *  - Tree: complete binary sum tree in f64, heap layout: node 1 is the root, leaf i at node 2^L + i (2^L >= buffer_size) holds
 *    (double)p_i, p_i row i's f32 priority; every inner node is left + right of its final children (order-independent contents).
 *  - Priority from TD: p = powf(|td| + eps, alpha) in f32 (alpha == 1: |td| + eps exactly; alpha == 0: 1.0f exactly).
 *  - Duplicates: a row listed twice in one update takes the priority of its LAST occurrence.
 *  - New rows (cpp_replay_write_rows, cpp_replay_fill_synthetic, FIFO overwrites included) take the running maximum priority: a
 *    device scalar that starts at 1.0 and is the max of every priority written since (all entries of an update, duplicates included).
 *    Enabling gives every row already in the memory that maximum; rows >= size hold 0 and are never drawn.
 *  - Draw (stratified) of minibatch row b: r = philox4x32_10({b, 1, lo(counter), hi(counter)}, seed) (word 1 = 1: disjoint from the
 *    uniform sampler's stream), U = (double)(((uint64)r.x << 32 | r.y) >> 11) * 2^-53, u = ((double)b + U) * (total / (double)B);
 *    from the root go left if u < left, else u -= left and go right.  Top-end guard: a leaf at or past `size` (rounding) is
 *    replaced by the last row, size - 1.  The counter advances by one per minibatch, as the uniform sampler's.
 *  - Importance weights: w_b = pow(size * leaf_b / total, -beta) in f64, divided by the batch maximum, stored as f32.  beta is a
 *    device scalar; setting it is a stream-ordered write, captured graph replays read the new value.
 *  - DDPG: critic loss mean(w td^2), dz_q = (td w) 2 / B (w == 1: today's bits); cpp_ddpg_last_stats()[0] is the weighted loss; the
 *    actor's update is unweighted.  The priorities of minibatch k are in the tree before minibatch k+1 is drawn, in the fused step
 *    (cpp_ddpg_train_step) and in the literal loop (cpp_replay_draw_prioritized + cpp_ddpg_train_rows) alike: the same rows.
 *  - NAF: loss mean(w td^2), dQ = (td w) 2 / B (w == 1: today's bits); everything below dQ inherits the weight; cpp_naf_last_stats()[0]
 *    is the weighted loss.  cpp_naf_train_step (fused) and cpp_naf_train_rows / cpp_naf_train_rows_async (the literal loop, after
 *    cpp_replay_draw_prioritized) write minibatch k's priorities before k+1 is drawn, as DDPG's.  A non-finite minibatch (the
 *    check_numerics flag: l_values, L or the loss not finite) writes no priority and, in cpp_naf_train_step and
 *    cpp_naf_train_rows_async, no parameter: for as long as the flag stays set (it is sticky on those two paths).  The draws and the
 *    counter go on.  cpp_naf_train_step's target soft update still runs (the value network it follows has not moved).
 *  - cpp_replay_sample(idxs == NULL) draws by priority (key (seed, counter) as given).  cpp_ddpg_dp_train_step,
 *    cpp_ddpg_sample_and_compute, cpp_naf_dp_train_step and cpp_naf_sample_and_compute (per-shard trees: not built) return
 *    CPP_ERR_ARG on a prioritized memory, writing nothing.
 * Batches of a prioritized memory hold at most 1024 rows. */
/* alpha >= 0; eps > 0 unless alpha == 0.  Called again: new alpha / eps, the maximum back to 1.0 and every row at it. */
int cpp_replay_enable_priorities(cpp_replay* replay, float alpha, float eps);
int cpp_replay_set_priority_beta(cpp_replay* replay, float beta);           /* beta >= 0 (0 until set) */
/* the priorities of n rows from |td| values (abs_td >= 0), the duplicate rule above */
int cpp_replay_update_priorities(cpp_replay* replay, const int32_t* rows, int n, const float* abs_td);
int cpp_replay_read_priorities(cpp_replay* replay, const int32_t* rows, int n, float* p);
/* the whole tree, 2^(L+1) doubles (node 0 unused, 0): tests */
int cpp_replay_read_priority_tree(cpp_replay* replay, double* out, int64_t cap);
/* importance weights of the last prioritized draw or minibatch (B <= 1024) */
int cpp_replay_last_weights(cpp_replay* replay, int B, float* w);
/* the literal loop's draw: B rows by priority keyed (seed, the training sampler's counter), which then advances by one -- the rows
 * cpp_ddpg_train_step would draw for its next minibatch; rows and weights come back to the host (either may be NULL) */
int cpp_replay_draw_prioritized(cpp_replay* replay, int B, uint64_t seed, int32_t* idxs, float* w);

/* ---- n-step returns (D4PG, Rainbow) in the gather ---------------------------------------------------------------------------
 * Extension, no reference counterpart (the reference trains on r + mask * discount * Q'(s2), ddpg_cartpole.py:397).  Opt-in per
 * memory with cpp_replay_set_n_step(replay, n, discount); n = 1 is the default and means exactly the one-step behaviour, bit for bit,
 * on every path.  For a drawn row i, in a memory of R = buffer_size rows and current `size`:
 *  - Walk: j_0 = i.  For k = 0 .. n-2 the walk goes on to j_{k+1} only if mask[j_k] != 0; the next row exists (j_k + 1 < size, or
 *    the memory is full (size == R), in which case j_{k+1} = (j_k + 1) mod R); j_{k+1} != i; and s2_idx[j_k] == s1_idx[j_{k+1}].
 *    Otherwise it stops.  m is the number of rows walked, 1 <= m <= n.
 *  - The contiguity test is sound at the FIFO write head: a live row's state slots are in use, and a newly written row's s2 comes
 *    from the free list, so the newest row (whose s2 is a slot no live row's s1 can hold) never appears to continue into the oldest
 *    one.  For memories filled by add_episode (whole episodes, the last row of each with mask 0) the walk gives the exact n-step return.
 *  - Arithmetic, all f32, every operation rounded on its own (no contraction): g_0 = 1, g_k = g_{k-1} * discount; R_0 = r[j_0],
 *    R_k = R_{k-1} + r[j_k] * g_k.  The gathered reward is R_{m-1}, the gathered terminal_mask is mask[j_{m-1}] * g_{m-1}, the
 *    gathered state_2 (and its whitening statistics) is the state in slot s2_idx[j_{m-1}]; state_1 and action come from j_0.  The
 *    head kernels' target reward + (mask * discount) * Q'(s2) is then the n-step target.  At n = 1 these are the stored values.
 *  - Trainers: cpp_ddpg_train_step, cpp_ddpg_train_rows, cpp_ddpg_sample_and_compute, cpp_ddpg_dp_train_step, cpp_naf_train_step,
 *    cpp_naf_train_rows, cpp_naf_train_rows_async, cpp_naf_sample_and_compute and cpp_naf_dp_train_step return CPP_ERR_ARG, writing
 *    nothing, on a memory with n > 1 whose discount is not bit-equal to their own hyper.discount.  A cpp_batch gathered by
 *    cpp_replay_sample carries the folded columns: training it under another discount is the caller's affair.
 *  - Prioritized replay combines unchanged: a drawn row's priority comes from its n-step TD; the draws and weights are as before.
 *  - 1 <= n <= 64 (one wavefront); discount finite and >= 0.  n and the discount are device words written in stream order: a change
 *    takes effect at the next minibatch, also inside already captured step graphs. */
int cpp_replay_set_n_step(cpp_replay* replay, int n, float discount);
int cpp_replay_get_n_step(cpp_replay* replay, int* n, float* discount);       /* (1, 0) until set; either output may be NULL */

/* ---- Random shift (DrQ, DrQ-v2) in the gather ---------------------------------------------------------------------------------
 * Extension, no reference counterpart (the reference trains on the stored renders).  Opt-in per memory with
 * cpp_replay_set_random_shift(replay, H, W, pad, seed); a memory on which it was never enabled, or with pad = 0, behaves bit for bit
 * as before on every path.  Pixel memories only: state shape (H, W, 3, cameras, repeats) with the C = 3 * cameras * repeats channels
 * innermost, i.e. a memory for which cpp_replay_set_stats_channels was called with C > 0, and H * W * C == state_elems.
 *  - The shifted image.  For gathered state (b, which) -- which = 0: state_1, 1: state_2 -- with shift (dy, dx), each in [-pad, pad]:
 *      out[y, x, c] = in[clamp(y + dy, 0, H-1), clamp(x + dx, 0, W-1), c]
 *    i.e. replicate padding by `pad` followed by a crop at offset (pad + dy, pad + dx): DrQ-v2's RandomShiftsAug at integer shifts.
 *    The same rule for the f16 and the 8-bit store (which gathers to f16 through its table, as without the shift).  The whitening
 *    statistics of the minibatch are those of the shifted images: what the networks see.
 *  - The draw.  r = philox4x32_10(ctr = {b, 2 + which, n_lo, n_hi}, key = {seed_lo, seed_hi}); `seed` is the augmentation's own, n
 *    the memory's augmentation counter.  (ctr.y is 0 for the uniform row draw and 1 for the prioritized draw: 2 and 3 keep the shift
 *    streams disjoint from both, even under equal seeds.)  dy = (int)(((uint64)r.x * (2 pad + 1)) >> 32) - pad, dx likewise from r.y.
 *  - The counter.  A 64-bit device word per memory, 0 when the augmentation is enabled (every call of cpp_replay_set_random_shift
 *    with pad > 0 resets it).  It advances by exactly one per minibatch gathered with augmentation, in stream order, inside the
 *    gather's own launch, on every path that trains: cpp_ddpg_train_step / cpp_naf_train_step (eager or replayed from a captured
 *    graph), cpp_ddpg_train_rows / cpp_naf_train_rows / cpp_naf_train_rows_async (the literal loop: rows from the host),
 *    cpp_ddpg_sample_and_compute / cpp_naf_sample_and_compute and the data-parallel steps.  It does not depend on the sampler's
 *    counter (which stands still when the host draws the rows).
 *  - Where it applies: to the trainers' own gathers, listed above, and to cpp_replay_gather_shifted.  cpp_replay_sample keeps
 *    returning the stored pixels and does not move the counter, so a cpp_batch it filled is trained as it is.
 *  - A memory with pad > 0 always materialises its minibatch (the gathered-copy route of the 8-bit store); conv1 never reads the store
 *    directly.  n-step: the shift is applied to the state in the slot the walk ends on.  Prioritized replay, batch norm and dropout
 *    are unaffected.  Data-parallel learners: each rank's memory has its own seed and counter; distinct seeds per rank are the
 *    caller's business.
 *  - cpp_replay_set_random_shift returns CPP_ERR_ARG and writes nothing if the memory is not a pixel memory or its state_elems is no
 *    multiple of 8 (the shifted gather moves whole vectors of 8 elements; the message names the element count), if H * W * C !=
 *    state_elems (C: the memory's statistics channels), if pad is outside [0, 16] or >= min(H, W), or if a row holds fewer than 8
 *    elements (W * C < 8).  pad = 0 switches the feature off (the direct path again).  Every effective change re-issues the memory's
 *    graph key: the trainers capture their step graphs again at the next call, none replays the old form. */
int cpp_replay_set_random_shift(cpp_replay* replay, int H, int W, int pad, uint64_t seed);
/* synchronises the stream for the counter; (0, 0, 0) when off; any output may be NULL */
int cpp_replay_get_random_shift(cpp_replay* replay, int* pad, uint64_t* seed, uint64_t* counter);
/* the (2, B, 2) shifts [which][b][dy, dx] of the last augmented gather of B rows (written by the gather next to its rows) */
int cpp_replay_last_shifts(cpp_replay* replay, int B, int32_t* out);
/* cpp_replay_sample(idxs != NULL)'s contract with the augmentation applied: the B host-given rows gathered, shifted, into `out`,
 * the counter advancing by one (inspection / tests).  CPP_ERR_STATE on a memory without the augmentation. */
int cpp_replay_gather_shifted(cpp_replay* replay, int B, const int32_t* idxs, int channels, cpp_batch* out);

/* ---- DDPG train ops (ddpg_cartpole.py:102-119, :186-248, :329-337) --------------------------- */
typedef struct cpp_ddpg_hyper {
  float actor_learning_rate;     /* --actor-learning-rate  (ddpg_cartpole.py:41)  */
  float critic_learning_rate;    /* --critic-learning-rate (:42)                  */
  float discount;                /* --discount             (:43)                  */
  float gradient_clip;           /* --gradient-clip, util.py:11; <= 0 disables    */
  float target_update_rate;      /* --target-update-rate   (:35)                  */
} cpp_ddpg_hyper;

int cpp_ddpg_create(cpp_ctx* ctx, cpp_net* actor, cpp_net* critic, cpp_net* target_actor,
                    cpp_net* target_critic, const cpp_ddpg_hyper* hyper, cpp_ddpg** out);
int cpp_ddpg_destroy(cpp_ddpg* ddpg);
/* ActorNetwork.train(state) (ddpg_cartpole.py:140-145): uses batch.state_1 only. */
int cpp_ddpg_train_actor(cpp_ddpg* ddpg, cpp_batch* batch);
/* CriticNetwork.train(batch) (:230-237). */
int cpp_ddpg_train_critic(cpp_ddpg* ddpg, cpp_batch* batch);
/* CriticNetwork.check_loss(batch) (:239-248): loss scalar, td (B), q (B). */
int cpp_ddpg_check_loss(cpp_ddpg* ddpg, cpp_batch* batch, float* loss, float* td, float* q);
/* CriticNetwork.q_gradients_wrt_actions() evaluated at a = actor(state_1) (:220-222): (B, A);
 * also returns the actions and q-values of that evaluation when the pointers are non-NULL.  An evaluation: under use_dropout it drops no
 * unit and is not counted, as cpp_ddpg_check_loss. */
int cpp_ddpg_q_gradients_wrt_actions(cpp_ddpg* ddpg, cpp_batch* batch, float* dq_da, float* actions,
                                     float* q);
/* Fused form of one loop body of :331-334.  Both gradient sets are taken from the same parameter
 * snapshot (the critic step never reads the live actor, the actor step never writes the critic) and
 * land in ONE flat f32 buffer [actor grads | critic grads] that a data-parallel host all-reduces
 * (RCCL) between the two calls. */
int cpp_ddpg_compute_gradients(cpp_ddpg* ddpg, cpp_batch* batch);
int cpp_ddpg_grad_buffer(cpp_ddpg* ddpg, void** device_ptr, int64_t* n_floats);
/* clip_by_global_norm per list (util.py:47-50) + SGD (ddpg_cartpole.py:118-119,213,218).  The
 * gradients are first multiplied by grad_scale (1/world_size after a sum all-reduce). */
int cpp_ddpg_apply_gradients(cpp_ddpg* ddpg, float grad_scale);
/* target_actor.update_weights(); target_critic.update_weights() (:336-337). */
int cpp_ddpg_update_targets(cpp_ddpg* ddpg);
/* The update rule of the two train ops.  ddpg_cartpole.py:118-119 and :218 build them with tf.train.GradientDescentOptimizer (the
 * default here, and the only rule until this call); util.py:73-76 is the reference's rule for any other optimiser,
 * tf.train.<name>Optimizer -- CPP_OPT_MOMENTUM: accum = momentum accum + g, p -= lr accum; CPP_OPT_ADAM: lr_t = lr sqrt(1 - beta2^t) /
 * (1 - beta1^t), m = beta1 m + (1 - beta1) g, v = beta2 v + (1 - beta2) g^2, p -= lr_t m / (sqrt(v) + epsilon).  g is the list's
 * gradient after its own global-norm clip (util.py:45-50); the learning rates stay cpp_ddpg_hyper's.  The actor's and the critic's
 * optimisers are separate (the reference's two 'optimiser' scopes): each list has its own slots and its own step count t, and a call
 * that applies one list (cpp_ddpg_train_actor, cpp_ddpg_train_critic) advances that list's t only.  The call allocates and zeroes the
 * slots (actor + critic parameters, the gradient buffer's layout), zeroes both step counts and drops the captured graphs.  Bad kinds
 * and ranges (momentum < 0, a beta outside [0, 1), epsilon <= 0) are refused. */
int cpp_ddpg_set_optimiser(cpp_ddpg* ddpg, int kind, float momentum, float beta1, float beta2, float epsilon);
/* Target policy smoothing (TD3: Fujimoto et al. 2018, section 5.3), an extension of the critic's target ddpg_cartpole.py:199-209: with
 * sigma > 0 every pass that forms a training target evaluates the target critic at
 *     a' = clamp(mu'(s2) + clamp(sigma z, -clip, clip), -1, 1),   z ~ N(0, 1) per row b and action component i, fresh in every minibatch:
 *     (x, y, _, _) = philox4x32_10({b, 0x100 + i, n_lo, n_hi}, key = (seed_lo, seed_hi))
 *     u1 = ((x >> 8) + 1) 2^-24,  u2 = (y >> 8) 2^-24,  z = sqrtf(-2 logf(u1)) cos(2 pi u2)          (f32, the accurate logf / cosine)
 * n is the trainer's count of such passes since this call: a 64-bit device word that the call zeroes and that every pass advances
 * by exactly one -- cpp_ddpg_train_critic, cpp_ddpg_compute_gradients, cpp_ddpg_train_rows, cpp_ddpg_sample_and_compute and each
 * minibatch of cpp_ddpg_train_step / cpp_ddpg_dp_train_step, graph replays included.  cpp_ddpg_check_loss is an evaluation: no
 * noise, no count.  The actor's update, dQ/da and the fed-action Q are untouched.  sigma == 0 with clip == 0 switches the feature
 * off (the state after cpp_ddpg_create: every path then launches exactly what it did before the feature existed).  Refused
 * (CPP_ERR_ARG): a negative, NaN or infinite sigma or clip, sigma > 0 with clip == 0, clip > 0 with sigma == 0.  sigma, clip and
 * seed are captured by value: the call drops the captured graphs.  n is not part of any checkpoint: a resumed run restarts the
 * stream.  Data-parallel learners: distinct seeds per rank are the caller's business (distributed.py adds the rank). */
int cpp_ddpg_set_target_smoothing(cpp_ddpg* ddpg, float sigma, float clip, uint64_t seed);
/* the (B, action_dim) clipped noise clamp(sigma z, -clip, clip) of the last target-forming pass and the count n it was drawn at (written
 * by the launch that applied it); either output may be NULL.  CPP_ERR_STATE when smoothing is off. */
int cpp_ddpg_last_target_noise(cpp_ddpg* ddpg, int B, float* eps, uint64_t* n);
/* Delayed policy updates (TD3: Fujimoto et al. 2018, Algorithm 1: `total_it += 1; if total_it % policy_freq == 0`), an extension of the
 * loop body ddpg_cartpole.py:332-337.  delay is d, 1 <= d <= 65536; d = 1 is off, the trainer's state after cpp_ddpg_create (every path
 * then launches exactly what it did before the feature existed).  n is a 64-bit word in device memory: the critic updates this trainer
 * has applied since this call.  A minibatch that applies the critic's list advances n by one, to n'; the actor's list is applied iff
 * n' % d == 0 and is otherwise HELD: its parameters, its Momentum / Adam slots and its own step count do not move, and no bit of them
 * is rewritten to a different value.  On a held minibatch the actor's gradient is still computed and its pre-clip norm still reported
 * (cpp_ddpg_last_stats); the critic's list, the sampler's counter, the smoothing count, the priorities and the whitening tables are
 * what they would have been.  The decision is taken on the device, so one captured graph serves every phase of the schedule.
 * Target updates keep :336-337's cadence: both targets take their soft update at the end of every outer step, whether or not the
 * actor was held in its last minibatch (the target actor then takes it from the held, unchanged actor); with n_batches == d the
 * actor moves in the outer step's last minibatch and the targets follow: TD3's schedule exactly.
 * Who counts: cpp_ddpg_train_step, cpp_ddpg_train_rows and cpp_ddpg_dp_train_step per minibatch; cpp_ddpg_train_critic;
 * cpp_ddpg_apply_gradients (both lists, under the predicate).  cpp_ddpg_train_actor does not advance n and applies iff
 * (n + 1) % d == 0: it is the actor half of the minibatch whose critic half follows (:333-334).  cpp_ddpg_compute_gradients and
 * cpp_ddpg_sample_and_compute alone, cpp_ddpg_check_loss and cpp_ddpg_q_gradients_wrt_actions count nothing; neither does a gradient
 * pass that fails.  The call zeroes n and drops the captured graphs (d is captured by value).  Refused (CPP_ERR_ARG, the call's name in
 * cpp_last_error): d outside [1, 65536], a NULL handle.  n is not part of any checkpoint: a resumed run restarts the phase.
 * Data-parallel learners each count their own minibatches: the schedule is the same on every rank. */
int cpp_ddpg_set_policy_delay(cpp_ddpg* ddpg, int delay);
/* d, n and whether the last counted minibatch (or the last cpp_ddpg_train_actor) held the actor; any output may be NULL. */
int cpp_ddpg_policy_delay_status(cpp_ddpg* ddpg, int* delay, uint64_t* n, int* held);
/* The slot variables tf.train.Saver checkpoints besides the weights (util.py:88-90; the slots of ddpg_cartpole.py:118 and :218's
 * optimisers): m and v hold the actor's list, then the critic's (n = cpp_ddpg_opt_state_size values each; v only under Adam);
 * steps[0] is the actor's step count, steps[1] the critic's.  Refused under GradientDescent, which has no slots. */
int64_t cpp_ddpg_opt_state_size(const cpp_ddpg* ddpg);
int cpp_ddpg_get_opt_state(cpp_ddpg* ddpg, float* m, float* v, int64_t n, uint64_t steps[2]);
int cpp_ddpg_set_opt_state(cpp_ddpg* ddpg, const float* m, const float* v, int64_t n, const uint64_t steps[2]);
/* The whole inner step :331-337 on device-resident replay: n_batches x {sample B, both updates},
 * then the target updates.  idxs: NULL (device Philox, counter advances by one per minibatch) or
 * n_batches*B caller-chosen rows.  Captured into a hipGraph after the first call per (B, n_batches)
 * when idxs == NULL and profiling is off. */
int cpp_ddpg_train_step(cpp_ddpg* ddpg, cpp_replay* replay, int B, int n_batches,
                        const int32_t* idxs, uint64_t seed);
/* ddpg_cartpole.py:332-334 for ONE minibatch on B rows the HOST drew (replay_memory.py:123-129, numpy's RNG):
 *     batch = self.replay_memory.batch(batch_size); self.actor.train(batch.state_1); self.critic.train(batch)
 * as the same fused device sequence as one minibatch of cpp_ddpg_train_step -- no gathered copy of the states, no PCIe traffic
 * but the B row indexes -- WITHOUT the target updates (:336-337 stay the caller's: cpp_net_soft_update).  hipGraph-replayed after
 * the first call per (B, replay); returns while the minibatch is still running. */
int cpp_ddpg_train_rows(cpp_ddpg* ddpg, cpp_replay* replay, int B, const int32_t* idxs);
/* Data-parallel learners: the first half of one minibatch of the inner step -- sample B rows on the
 * device (Philox; the counter advances by one) and leave both gradient sets in the flat gradient
 * buffer.  cpp_ddpg_allreduce_grads + cpp_ddpg_apply_gradients(1/N) finish the minibatch
 * (cpp_ddpg_dp_train_step does all three).  hipGraph-captured after the first call per (B, seed, replay). */
int cpp_ddpg_sample_and_compute(cpp_ddpg* ddpg, cpp_replay* replay, int B, uint64_t seed);
/* scalars of the last minibatch: [0] td loss, [1] actor grad norm, [2] critic grad norm (pre-clip). */
int cpp_ddpg_last_stats(cpp_ddpg* ddpg, float out[3]);
/* The per-row values the last minibatch's gradient pass left on the device (whichever entry point ran it: the train ops,
 * cpp_ddpg_compute_gradients, the fused / graph-replayed cpp_ddpg_train_step, cpp_ddpg_sample_and_compute): the actor's
 * actions on state_1 (B, A), dQ/da at those actions (B, A), Q(state_1, fed action) (B) and the temporal difference (B) --
 * what the reference prints under VERBOSE_DEBUG (ddpg_cartpole.py:339-349).  NULL pointers are skipped.  Parity tests read
 * the fused step's values through this call. */
int cpp_ddpg_last_values(cpp_ddpg* ddpg, int B, float* actions, float* dq_da, float* q, float* td);
/* Twin trainers (cpp_net_create_twin_q; an extension of the target ddpg_cartpole.py:199-214): what head 2 and the two target heads left
 * in the last minibatch's gradient pass -- Q2(state_1, fed action), Q1'(state_2, a'), Q2'(state_2, a') and td_2 = Q2 - y, each (B).
 * NULL pointers are skipped.  CPP_ERR_STATE on a trainer of plain critics. */
int cpp_ddpg_last_twin_values(cpp_ddpg* ddpg, int B, float* q2, float* target_q1, float* target_q2, float* td2);
/* The actor on the minimum head (the actor's objective of DrQ-v2, SAC and DrQ on twin critics; an extension of the actor's train op
 * ddpg_cartpole.py:111-113, :220-222).  Twin trainers only: CPP_ERR_ARG unless both critics are twin critics (so never with a
 * distributional or quantile critic).  With on != 0 every gradient pass chooses, per row b, at a = mu(state_1) (soft actor-critic: at its
 * sample),
 *     q1 = Q1(s1_b, a),  q2 = Q2(s1_b, a),  sel_b = 1 if q1 <= q2 else 2      (a tie is head 1's)
 *     dq_da_b = d Q_{sel_b}(s1_b, a) / da
 * with the shared prefix of the critic evaluated once.  The deterministic actor's head gradient is -dq_da (1 - a^2) as before; a soft
 * actor-critic trainer's actor minimises alpha logp - min(Q1, Q2)(s1, a) through the same dq_da.  A row's unselected head contributes
 * exact zeros.  Everything else stays head 1's or the twin step's: the critic's target, both temporal differences and the twin loss,
 * priorities, cpp_ddpg_last_values' q and td, cpp_ddpg_check_loss, cpp_net_forward*, and what a held actor means under a policy delay.
 * cpp_ddpg_q_gradients_wrt_actions returns the minimum's dq_da, and Q1 as q.  Where the fused heads kernel runs, its instances for
 * this switch run in its place: no launch is added.  On the GEMM levels head 2's forward and dX GEMMs ride beside head 1's, one kernel
 * makes the choice and one more GEMM level adds head 2's action columns.  There is no new state: checkpoints are unchanged.  The switch
 * is captured by the launches: the call drops the captured graphs, as cpp_ddpg_set_policy_delay does.  on == 0 restores the trainer the
 * call found after cpp_ddpg_create, bit for bit. */
int cpp_ddpg_set_actor_min_q(cpp_ddpg* ddpg, int on);
/* Such trainers: Q1 and Q2 at mu(state_1) (B each) and the head each row followed (B, int32: 1 or 2) in the last gradient pass that ran
 * the actor's half.  NULL pointers are skipped.  CPP_ERR_STATE while the switch is off. */
int cpp_ddpg_last_actor_min(cpp_ddpg* ddpg, int B, float* q1, float* q2, int32_t* sel);
/* The behaviour-cloning actor term (TD3+BC, Fujimoto & Gu 2021: the cure for extrapolation error when the memory is a fixed data set; an
 * extension of the actor's train op ddpg_cartpole.py:111-113, whose grad_ys -dQ/da these lines replace).  With alpha > 0 every gradient pass
 * that runs the actor's half computes, with a_b the minibatch's stored action, mu_b = actor(state_1_b) and B the rows of THIS minibatch,
 *     q_b    = Q(s1_b, mu_b) of the head the actor follows (Q1; cpp_ddpg_set_actor_min_q: the row's selected head)
 *     m      = (1 / B) sum_b |q_b|             (every workgroup adds all B values itself in one fixed order, in f64: one lambda to the bit)
 *     lambda = alpha / max(m, q_floor)         (a constant of the minibatch: no gradient flows through it)
 *     g_bi   = -lambda dq_da_bi + (2 / A) (mu_bi - a_bi)         (grad_ys at the actor's output)
 *     adz_bi = g_bi (1 - mu_bi^2)                                (what the actor's backward starts from)
 * which is B times the paper's loss -lambda mean(Q) + mse(mu, a), as the actor's list without the term is B times the usual mean: the
 * actor's learning rate keeps its meaning.  q_floor is the one departure from the paper: a critic whose Q is exactly 0 gives a finite step.
 * dq_da as cpp_ddpg_last_values and cpp_ddpg_q_gradients_wrt_actions report it stays the unscaled dQ/da; the critic's side, priorities,
 * cpp_ddpg_check_loss and what a held actor means under a policy delay are unchanged; the actor's term takes no importance weights, as
 * before.  Such a trainer always takes the GEMM levels of the gradient pass (as soft actor-critic does), plus one launch per minibatch.  In
 * the data-parallel step each rank takes lambda from its own minibatch: the summed list is the sum of the ranks' lists, each under its own
 * lambda, not the list of the concatenated minibatch.  There is no new state: checkpoints are unchanged.
 * alpha == 0 switches the term off, the state after cpp_ddpg_create, bit for bit.  CPP_ERR_ARG, with nothing written: alpha < 0, q_floor <= 0,
 * a value that is not finite, a trainer whose critic is distributional or quantile or whose actor is soft actor-critic's.  Alpha and the floor
 * are captured by the launches: the call drops the captured graphs, as cpp_ddpg_set_actor_min_q does. */
int cpp_ddpg_set_behaviour_cloning(cpp_ddpg* ddpg, float alpha, float q_floor);
/* Such trainers: lambda and m (one float each), g (B, A) and the per-row (1 / A) sum_i (mu_bi - a_bi)^2 (B) of the last gradient pass that ran
 * the actor's half.  NULL pointers are skipped.  CPP_ERR_STATE while the term is off. */
int cpp_ddpg_last_behaviour_cloning(cpp_ddpg* ddpg, int B, float* lambda, float* m, float* g, float* bc_rows);
/* Distributional trainers (cpp_net_create_distributional): p of the fed evaluation, p' of the target evaluation and the projected target m
 * of the last minibatch's gradient pass, each (B, N).  NULL pointers are skipped.  CPP_ERR_STATE on any other trainer. */
int cpp_ddpg_last_distribution(cpp_ddpg* ddpg, int B, float* p, float* target_p, float* m);
/* Quantile trainers (cpp_net_create_quantile; an extension of the target ddpg_cartpole.py:199-214): the Huber threshold kappa and the
 * number d of largest target atoms dropped before the regression.  After cpp_ddpg_create: kappa 1, d 0 (plain quantile regression).
 * CPP_ERR_ARG for a kappa that is not finite and positive or a d outside [0, N - 1]; CPP_ERR_STATE on any other trainer.  Both values are
 * captured by value: the call drops the captured graphs, as cpp_ddpg_set_policy_delay does.  A pooled quantile trainer
 * (cpp_net_create_pooled_quantile) takes d PER HEAD: the 2d largest atoms of the pool of 2N are dropped. */
int cpp_ddpg_set_quantile_target(cpp_ddpg* ddpg, float kappa, int drop_top);
/* Quantile trainers (an extension of ddpg_cartpole.py:166-177, :199-214): theta of the fed evaluation, the target evaluation's atoms
 * sorted ascending and y_j = r + g s_j of the last minibatch's gradient pass, each (B, N); columns j >= M of y are zero.  NULL pointers are
 * skipped.  CPP_ERR_STATE on any other trainer. */
int cpp_ddpg_last_quantiles(cpp_ddpg* ddpg, int B, float* theta, float* sorted_target_theta, float* y);
/* Pooled quantile trainers (cpp_net_create_pooled_quantile; an extension of ddpg_cartpole.py:166-177, :199-214): theta^1 and theta^2 of the
 * fed evaluation ((B, N) each), the pool of both target heads' atoms sorted ascending and y_j = r* + g s_j of the last minibatch's gradient
 * pass ((B, 2N) each); columns j >= M = 2N - 2d of y are zero.  NULL pointers are skipped.  CPP_ERR_STATE on any other trainer, as
 * cpp_ddpg_last_quantiles answers on this one. */
int cpp_ddpg_last_pooled_quantiles(cpp_ddpg* ddpg, int B, float* theta1, float* theta2, float* sorted_pool, float* y);
/* Soft actor-critic trainers (cpp_net_create_gaussian; an extension of the actor's train op ddpg_cartpole.py:102-119 and of the target
 * :199-214): the initial temperature alpha (> 0), the target entropy Hbar, the temperature's Adam rate (0: fixed) and the noise seed, all
 * captured by value.  Zeroes the noise count, Adam's slots and count, copies the actor into the target actor, drops the cached graphs.  A
 * trainer that was never told has alpha 0.1, Hbar = -A, rate 1e-4, seed 0.  CPP_ERR_STATE on a trainer whose actors are not Gaussian. */
int cpp_ddpg_set_sac(cpp_ddpg* ddpg, float init_temperature, float target_entropy, float temperature_lr, uint64_t seed);
/* What the last gradient pass of such a trainer left (the sample standing where ddpg_cartpole.py:95-100's tanh stood): eps, a (B, A) and
 * logp (B) of the draw at state_1, the same three of the draw at state_2, r_soft (B), the alpha the actor pass read, g_alpha of its rows
 * and the count n the target draw was made at; dz: the actor's head gradient (d m | d x), (B, 2A), as the actor's backward read it.
 * NULL pointers are skipped. */
int cpp_ddpg_last_sac(cpp_ddpg* ddpg, int B, float* eps, float* a, float* logp, float* eps2, float* a2, float* logp2, float* r_soft,
                      float* alpha, float* g_alpha, uint64_t* n, float* dz);
/* log_alpha, its Adam slots m, v and its count for checkpoints (util.py:88-90).  set == 0: read into the pointers (NULL: skipped); else
 * written from them (all needed).  The noise count is not checkpointed. */
int cpp_ddpg_sac_temperature(cpp_ddpg* ddpg, int set, float* log_alpha, float* m, float* v, uint64_t* step);
/* Trainers on networks with a feature layer norm (cpp_net_create_feature_norm; an extension of ddpg_cartpole.py:95 and :168): what the last
 * minibatch's gradient pass left for the actor (which = 0) or the critic (which = 1), n the width of its layer 0 -- xhat (B, n), rstd (B),
 * y (B, n), dz = dL/dz (B, n), and dgamma, dbeta (n) as computed, before the clip.  NULL pointers are skipped; CPP_ERR_STATE on any other trainer. */
int cpp_ddpg_last_feature_norm(cpp_ddpg* ddpg, int B, int which, float* xhat, float* rstd, float* y, float* dz, float* dgamma, float* dbeta);
/* Parameter-space exploration noise (Plappert et al. 2018; an extension of ddpg_cartpole.py:127-134, where the reference adds one
 * Ornstein-Uhlenbeck sample to the action on the host).  perturbed_actor is a network of the caller's with the actor's layout (an
 * encoder-less one bound to the trainer's critic); the trainer keeps sigma (f32), the draw count n (u64), the last distance d (f32) and
 * whether the last resample adapted on the device.  A RESAMPLE (cpp_ddpg_param_noise_resample) does, in this order, on the context's
 * stream and with no host wait:
 *   1. perturb: for every element i of the actor's flat parameter buffer p, pt[i] = fmaf(sigma, z(seed, n, i), p[i]), where z is the
 *      Box-Muller normal of target policy smoothing -- u1 = ((x >> 8) + 1) 2^-24, u2 = (y >> 8) 2^-24, z = sqrt(-2 log u1) cos(2 pi u2),
 *      the accurate logf / cospif, no clip -- on (x, y, _, _) = philox4x32_10({i, 0x200, n_lo, n_hi}, key = seed).  The elements of
 *      '<layer 0>/LayerNorm/gamma' and '.../beta' (cpp_net_create_feature_norm), which close the flat buffer, are copied unperturbed.
 *   2. measure (batch != NULL): the actor and the perturbed actor on the batch's state_1 in inference mode with the batch's whitening
 *      statistics, a and at, (B, A); d = sqrt(sum_{b,k} (a[b][k] - at[b][k])^2 / (B A)), the differences and squares in f64, added by one
 *      workgroup in one fixed order, rounded to f32 once.
 *   3. adapt (batch != NULL): sigma <- d < delta ? sigma * alpha : sigma / alpha, one f32 operation, read by the NEXT resample.
 *   4. count: n <- n + 1.
 * The copy that was measured is the copy the caller acts with until the next resample.  No launch of a training call reads or writes any
 * of this and no captured graph is dropped: the actor, the critic, the targets, the optimisers' slots and every count stay what a trainer
 * without the noise holds, bit for bit.
 * cpp_ddpg_set_param_noise: sigma0 the initial sigma (>= 0), delta the target distance (> 0), alpha the factor (>= 1; 1 keeps sigma
 * fixed), all finite; zeroes n and d and ends with a resample without a batch (n = 1 behind it).  perturbed_actor == NULL with sigma0 == 0
 * switches the noise off, the trainer cpp_ddpg_create left.  CPP_ERR_ARG, with nothing changed: a value out of range, a network whose
 * layout is not the actor's or that a trainer owns, an encoder-less copy not bound to the trainer's critic, a soft actor-critic trainer
 * (its policy explores by itself).  The network must outlive the setting. */
int cpp_ddpg_set_param_noise(cpp_ddpg* ddpg, cpp_net* perturbed_actor, float sigma0, float delta, float alpha, uint64_t seed);
/* One resample (ddpg_cartpole.py:127-134 extended: the episode boundary, where the reference's noise process would be reset).  batch: a
 * device minibatch with a gathered copy of its states (cpp_replay_sample, cpp_batch_upload), or NULL for steps 1 and 4 alone.
 * CPP_ERR_STATE while the noise is off. */
int cpp_ddpg_param_noise_resample(cpp_ddpg* ddpg, cpp_batch* batch_or_null);
/* The device's words (the state of the exploration ddpg_cartpole.py:127-134 kept on the host): sigma as the next resample will read it,
 * d of the last measured resample, n, and whether the last resample adapted.  NULL pointers are skipped.  Waits for the stream. */
int cpp_ddpg_param_noise_status(cpp_ddpg* ddpg, float* sigma, float* distance, uint64_t* n, int* adapted);
/* sigma and n for checkpoints (util.py:88-90) and tests.  set == 0: read into the pointers (NULL: skipped); else written from them (both
 * needed); the perturbed copy stays what it is until the next resample, which then draws at (seed, n). */
int cpp_ddpg_param_noise_state(cpp_ddpg* ddpg, int set, float* sigma, uint64_t* n);
/* a and at of the last measured resample (step 2 above; the policy of ddpg_cartpole.py:95-100 beside its perturbed copy), each (B, A) with
 * B at most that resample's rows.  NULL pointers are skipped.  CPP_ERR_STATE before the first measured resample. */
int cpp_ddpg_last_param_noise(cpp_ddpg* ddpg, int B, float* a, float* at);

/* ---- data-parallel actor-learners (the reference's TODO "switch back to async training with multiple replicas",
 * ddpg_cartpole.py:259, naf_cartpole.py:294; its exps only launch independent processes, exps/run_87.sh:12-36) ------------
 * One learner per GPU = one process with one cpp_ctx; replicated weights, an own replay shard and an own minibatch per
 * learner; RCCL collectives over xGMI issued by the library on the context's stream.  Rank 0 makes the id, the host
 * distributes its CPP_COMM_ID_BYTES bytes to the other ranks by any means (bench.py: a torch.distributed / gloo broadcast),
 * every rank then calls cpp_comm_create. */
#define CPP_COMM_ID_BYTES 128
int cpp_comm_unique_id(void* out, int cap);                       /* ncclGetUniqueId */
int cpp_comm_create(cpp_ctx* ctx, const void* unique_id, int rank, int world, cpp_comm** out);   /* ncclCommInitRank */
int cpp_comm_destroy(cpp_comm* comm);
int cpp_comm_info(const cpp_comm* comm, int* rank, int* world);
/* in-place sum (average != 0: mean) over the ranks of n floats at a DEVICE address, on the context's stream */
int cpp_comm_allreduce(cpp_comm* comm, void* device_f32, int64_t n, int average);
/* max over the ranks of one host double / a barrier (bench.py's timed region: max-over-ranks time between two barriers) */
int cpp_comm_max_double(cpp_comm* comm, double* value);
/* element-wise max over the ranks of n (1..8) host doubles.  The agents' --data-parallel loops decide "train this iteration" and
 * "leave the loop" with it once per outer iteration (the per-process tests of ddpg_cartpole.py:329 and :379-383 / naf_cartpole.py:
 * 365,386-389 in front of a collective step would leave the slower ranks blocked in ncclAllReduce). */
int cpp_comm_max_doubles(cpp_comm* comm, double* values, int n);
int cpp_comm_barrier(cpp_comm* comm);
/* sum over the ranks of the flat gradient buffer [actor grads | critic grads] left by cpp_ddpg_sample_and_compute /
 * cpp_ddpg_compute_gradients; cpp_ddpg_apply_gradients(1 / world) then gives every rank the same update. */
int cpp_ddpg_allreduce_grads(cpp_ddpg* ddpg, cpp_comm* comm);
/* periodic mode: the mean over the ranks of all four networks' parameters */
int cpp_ddpg_average_params(cpp_ddpg* ddpg, cpp_comm* comm);
/* This rank's part of the inner step ddpg_cartpole.py:331-337 for N synchronous learners: n_batches x {sample from the own
 * shard + both gradient sets (hipGraph) -> all-reduce -> clip + SGD on the mean}, then the (local) target updates.
 * sync_every = k > 1: k local minibatch updates between parameter averagings instead of a gradient all-reduce per minibatch.
 * overlap != 0: the gradients of the fully connected layers are reduced on a second stream while the conv backward of the
 * same minibatch runs.  comm == NULL: one learner on the same code path. */
int cpp_ddpg_dp_train_step(cpp_ddpg* ddpg, cpp_replay* replay, cpp_comm* comm, int B, int n_batches, uint64_t seed,
                           int sync_every, int overlap);
/* the same for NAF (naf_cartpole.py:367-373): flat buffer [value | mu | l_values]; the averaging includes the optimiser slots */
int cpp_naf_sample_and_compute(cpp_naf* naf, cpp_replay* replay, int B, uint64_t seed);
int cpp_naf_allreduce_grads(cpp_naf* naf, cpp_comm* comm);
int cpp_naf_average_params(cpp_naf* naf, cpp_comm* comm);
int cpp_naf_dp_train_step(cpp_naf* naf, cpp_replay* replay, cpp_comm* comm, int B, int n_batches, uint64_t seed,
                          int sync_every);
/* Which form the default data-parallel step (sync_every 1, no overlap) of this trainer takes -- the reference has no counterpart
 * (ddpg_cartpole.py:259 / naf_cartpole.py:294 are its "TODO: distributed" notes); *mode: 0 = none run yet, 1 = one hipGraph replay
 * per outer step with the all-reduce inside, 2 = the same launches issued on the stream because the runtime or RCCL refused the
 * capture (`reason`, if given, receives what it said). */
int cpp_ddpg_dp_status(const cpp_ddpg* ddpg, int* mode, char* reason, int cap);
int cpp_naf_dp_status(const cpp_naf* naf, int* mode, char* reason, int cap);

/* ---- NAF train ops (naf_cartpole.py:93-284, :365-373) ----------------------------------------- */
typedef struct cpp_naf_hyper {
  float discount;                /* --discount (naf_cartpole.py:46)                               */
  float gradient_clip;           /* --gradient-clip (util.py:11); <= 0 disables                    */
  float target_update_rate;      /* --target-update-rate (:36)                                     */
  int32_t optimiser;             /* --optimiser: CPP_OPT_* (util.py:15, :73-76)                    */
  float learning_rate;           /* --optimiser-args                                               */
  float momentum;                /*   Momentum                                                     */
  float beta1, beta2, epsilon;   /*   Adam (TF defaults .9 / .999 / 1e-8)                          */
} cpp_naf_hyper;

/* NafNetwork.__init__ (:117-245).  value / target_value: CPP_HEAD nets with head_out 1 (ValueNetwork,
 * :93-114).  mu: tanh head with action_dim outputs, l_values: linear head with A(A+1)/2 outputs.  With
 * share != 0 (--share-input-state-representation, :151-152,176-177) mu and l_values must be head-only
 * nets (pixel = 0, n_hidden = 0, state_elems = width of value's last hidden layer) and read value's
 * input_state_representation; otherwise they are full nets with their own trunks on state_1. */
int cpp_naf_create(cpp_ctx* ctx, cpp_net* value, cpp_net* target_value, cpp_net* mu, cpp_net* l_values,
                   int share, const cpp_naf_hyper* hyper, cpp_naf** out);
int cpp_naf_destroy(cpp_naf* naf);
/* NafNetwork.action_given without the noise (:247-253): output_action for a host state batch. */
int cpp_naf_action(cpp_naf* naf, const void* state, int state_dtype, int B, float* out);
/* NafNetwork.train(batch) (:264-272): check_numerics + train_op + loss.  Returns CPP_ERR_NUMERIC when
 * l_values, L or the loss is not finite (tf.check_numerics, :242-245); parameters are then untouched. */
int cpp_naf_train(cpp_naf* naf, cpp_batch* batch, float* loss);
/* NafNetwork.debug_values(batch) (:274-284): l_values (B, A(A+1)/2), loss, value (B), advantage (B),
 * target value (B). */
int cpp_naf_debug_values(cpp_naf* naf, cpp_batch* batch, float* l_values, float* loss, float* value,
                         float* advantage, float* target_value);
/* Gradient halves for data-parallel learners, as for DDPG: flat buffer [value | mu | l_values]. */
int cpp_naf_compute_gradients(cpp_naf* naf, cpp_batch* batch);
int cpp_naf_grad_buffer(cpp_naf* naf, void** device_ptr, int64_t* n_floats);
int cpp_naf_apply_gradients(cpp_naf* naf, float grad_scale);
/* target_value_net.update_weights() (:373). */
int cpp_naf_update_targets(cpp_naf* naf);
/* The whole inner step :367-373 on device-resident replay; hipGraph-captured like cpp_ddpg_train_step.
 * A non-finite minibatch sets a sticky flag that cpp_naf_last_stats reports (out[2] != 0). */
int cpp_naf_train_step(cpp_naf* naf, cpp_replay* replay, int B, int n_batches, const int32_t* idxs,
                       uint64_t seed);
/* naf_cartpole.py:367-371 for ONE minibatch on B rows the HOST drew: `batch = replay_memory.batch(B); loss = naf.train(batch)` with the
 * sample pass reading the replay store through those rows (no gathered copy).  *loss = the minibatch's loss; CPP_ERR_NUMERIC (the
 * optimiser does not run) when l_values, L or the loss is not finite, like cpp_naf_train.  No target update (:373 stays the caller's). */
int cpp_naf_train_rows(cpp_naf* naf, cpp_replay* replay, int B, const int32_t* idxs, float* loss);
/* The same minibatch without waiting for it: gradients and optimiser are enqueued (the optimiser kernel stands down by itself when
 * the check_numerics flag is set), *ticket names the call.  cpp_naf_loss_wait(ticket, &loss) waits for THAT minibatch and returns
 * its loss, or CPP_ERR_NUMERIC; a ticket stays readable until CPP_NAF_TICKETS later calls have been made.  The reference's
 * `losses.append(naf.train(batch))` (naf_cartpole.py:369-371) only ever averages the losses for its STATS line. */
#define CPP_NAF_TICKETS 8
int cpp_naf_train_rows_async(cpp_naf* naf, cpp_replay* replay, int B, const int32_t* idxs, uint64_t* ticket);
int cpp_naf_loss_wait(cpp_naf* naf, uint64_t ticket, float* loss);
/* [0] loss of the last minibatch, [1] pre-clip global gradient norm, [2] non-finite flag (sticky). */
int cpp_naf_last_stats(cpp_naf* naf, float out[3]);
/* The optimiser's slot variables, which tf.train.Saver checkpoints with everything else (util.py:88-90): Momentum accumulators
 * / Adam first moments `m` and Adam second moments `v`, each n = params(value) + params(mu) + params(l_values) floats in the
 * flat order [value | mu | l_values], and the number of applied updates `step` (Adam's beta powers are beta^step).  NULL
 * pointers are skipped. */
int64_t cpp_naf_opt_state_size(const cpp_naf* naf);
int cpp_naf_get_opt_state(cpp_naf* naf, float* m, float* v, int64_t n, uint64_t* step);
int cpp_naf_set_opt_state(cpp_naf* naf, const float* m, const float* v, int64_t n, uint64_t step);
/* cpp_naf_train_rows_async keeps the check_numerics flag of a non-finite minibatch set: every later update stands down, as the
 * reference's run ends there (naf_cartpole.py:242-245,265).  cpp_naf_set_opt_state (a restored checkpoint) clears it; so does this
 * call, for a caller that has put good parameters back with cpp_net_set_params. */
int cpp_naf_clear_numeric_error(cpp_naf* naf);

#ifdef __cplusplus
}
#endif
#endif /* CARTPOLEPP_ABI_H */
