// Internal declarations shared by the rt_*.cpp translation units (the C-ABI implementation of include/cartpolepp_abi.h):
// handle structs, the device-memory arena, the launch-sequence helpers of the networks and the level-synchronous
// launch scheduler.  Host-side logic only; all arithmetic is in the HIP kernels.
#pragma once
#include "../../include/cartpolepp_abi.h"
#include "common.h"

#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <string>
#include <vector>
#include <algorithm>

#include <rccl/rccl.h>

#define ARG_CHECK(cond, ...)                \
  do {                                      \
    if (!(cond)) {                          \
      cpp_set_error(__VA_ARGS__);           \
      return CPP_ERR_ARG;                   \
    }                                       \
  } while (0)
#define RC(expr)                  \
  do {                            \
    int _rc = (expr);             \
    if (_rc) return _rc;          \
  } while (0)

// ---------------------------------------------------------------------------------------------
// device memory helper
// ---------------------------------------------------------------------------------------------
struct Arena {
  std::vector<void*> ptrs;
  hipStream_t stream = nullptr;     // zero-fills are ordered on the owning ctx's stream (never the null stream)
  // every allocation sits between two 256-byte guard bands: the conv1 operand loads (conv_k16.h) read up to 128 bytes
  // before and 256 after an image batch (masked out, but the addresses must be mapped)
  static constexpr size_t GUARD = 256;
  int alloc(void** p, size_t bytes, bool zero = true) {
    if (bytes == 0) bytes = 16;
    void* raw = nullptr;
    HIP_CHECK(hipMalloc(&raw, bytes + 2 * GUARD));
    ptrs.push_back(raw);
    cpp_arena_register(raw, bytes + 2 * GUARD);
    *p = (char*)raw + GUARD;
    if (zero) HIP_CHECK(hipMemsetAsync(raw, 0, bytes + 2 * GUARD, stream));
    return 0;
  }
  void release() { for (void* p : ptrs) { cpp_arena_unregister(p); (void)hipFree(p); } ptrs.clear(); }
};
template <typename T> static int dalloc(Arena& a, T** p, size_t count, bool zero = true) {
  return a.alloc((void**)p, count * sizeof(T), zero);
}

// ---------------------------------------------------------------------------------------------
// networks
// ---------------------------------------------------------------------------------------------
static const int kConvKs[3] = {5, 5, 3};          // base_network.py:103,111,119
static const int kConvOut = 10;
static const char* kConvNames[3] = {"conv1", "conv2", "conv3"};

struct ConvL { int H, W, Cin, ks, Hp, Wp; long w_off, b_off; };
struct FcL { int n_in, n_out, act, cat; long w_off; std::string name; };   // bias row at w_off + n_in*n_out
struct VarInfo { std::string name; int rank; int shape[4]; long offset; };

struct Workspace {
  float* pool[3] = {nullptr, nullptr, nullptr};
  unsigned short* pool_b16 = nullptr;      // pool[0] once more as three bf16 planes (conv2 forward on the bf16 pipes)
  uint8_t* amax[3] = {nullptr, nullptr, nullptr};
  float* dpool[3] = {nullptr, nullptr, nullptr};
  float* dpool_imax = nullptr;             // [maxB][DX_IMAX_SLOTS]: bounds of |dpool[0]| per image, left by conv2's dX (conv_dx_rs.h) for conv1's dW
  // batch norm (training mode): plain conv output (overwritten by its gradient in the backward pass), (inv, -mean*inv)
  float* z[3] = {nullptr, nullptr, nullptr};
  float* bn_stat[3] = {nullptr, nullptr, nullptr};
  std::vector<float*> fcin, dz;
  float* out = nullptr;
  // twin Q heads (cpp_net_create_twin_q): the second copy of the layers [cat, nfc) on the fed action (ws[0]) and, for an actor on the
  // minimum head (cpp_ddpg_set_actor_min_q), at a = mu(s1) (a critic's ws[1]).  fcin2[cat] is the workspace's
  // fcin[cat] itself -- both heads read one concat input, and with it one smoothed target action --, the others are its own
  std::vector<float*> fcin2, dz2;
  float* out2 = nullptr;
  // distributional critic (cpp_net_create_distributional): the last layer's N logits land here, (maxB, N), and `out` holds Q = sum_i p_i z_i,
  // (maxB), which dist.hip writes -- every reader of `out` keeps its width of one.  nullptr for every other network.
  float* logits = nullptr;
  // pooled twin quantile critics (cpp_net_create_pooled_quantile): head 2's N atoms land here, (maxB, N), and `out2` holds Q_2, (maxB), which
  // quant_pool.hip writes.  nullptr for every other network.
  float* logits2 = nullptr;
  // feature layer norm (cpp_net_create_feature_norm): xhat, (maxB, fc[0].n_out), and rstd, (maxB), of the last forward of layer 0 -- the
  // first workspace's; a critic's second evaluation shares them with the prefix.  nullptr for every other network.
  float *ln_xhat = nullptr, *ln_rstd = nullptr;
};

struct cpp_net {
  cpp_ctx* ctx; cpp_net_spec spec; int maxB;
  std::vector<ConvL> conv; std::vector<FcL> fc; std::vector<VarInfo> vars;
  long nparams; int flat; int cat_layer; long state_elems;
  float* params; float* grads; float* own_grads;
  Workspace ws[2];
  bool use_b16;             // this forward: conv1 (f16 pipes) leaves bf16 planes of pool1, conv2 forward reads them
  void* wimg;               // conv1's operand image on the f16 pipes (conv_rs16.h)
  const float* wimg_key;    // the whitening table (scale pointer) the optimiser's launch built wimg for, with the weights it left; nullptr: stale --
                            // the next conv1 forward builds it itself.  Cleared by everything that changes the parameters.
  const int32_t* img_slot;  // conv1 reads image b from row img_slot[b] of the state pointer (the replay store); nullptr: b
  float* white;            // [2][C] statistics for cpp_net_forward
  float* white_rows;       // [maxB][2][C]: per-image statistics for cpp_net_forward_each
  double* stats_part;      // [maxB][2C]
  float* dw_partial[3];     // one per conv layer: their reductions are deferred and batched
  bool is_training;         // base_network.IS_TRAINING for the next forward (batch norm and dropout look at it)
  uint64_t* drop_counter;   // dropout: number of training-mode forwards so far (device; part of the Philox counter)
  double* bn_part; float* bn_means; float* bn_scratch;   // batch norm: reduction partials, (mean dy, mean dy*zhat), dW bias-slot dump
  void* stage_state; float* stage_action; float* stage_out;
  Arena arena;
  // twin Q heads (TD3's clipped double-Q with a shared representation): fc2[l], l in [cat_layer, nfc), is the second copy of fc[l];
  // its variables follow the plain critic's nparams in the flat buffer.  Empty for every other network.
  bool twin = false; std::vector<FcL> fc2;
  // distributional critic: N atoms on the support [v_min, v_max] (dist_n == 0: every other network); q_value is (n_in, N)
  int dist_n = 0; float dist_vmin = 0.f, dist_vmax = 0.f;
  // quantile critic (cpp_net_create_quantile): the same N-wide q_value and `logits` workspace, dist_n = N, read as N quantile atoms
  // theta_i at tau_i = (2 i + 1) / (2 N) -- there is no support, and cpp_net_distribution_info keeps answering 0 atoms
  bool quant = false;
  // pooled twin quantile critics (cpp_net_create_pooled_quantile): twin, quant and dist_n = N <= 32 at once -- head 2's q_valueb is N wide too
  bool pooled() const { return twin && quant; }
  // Gaussian actor (cpp_net_create_gaussian): output_action is 2A wide, (m | x), and lands in `logits`; `out` stays (maxB, A) and holds
  // the action sac.hip forms from it.  ls = lo + 0.5 (hi - lo) (tanh(x) + 1).  gauss_stage: (2, maxB, A) for cpp_net_forward_gaussian
  bool gauss = false; float ls_lo = 0.f, ls_hi = 0.f; float* gauss_stage = nullptr;
  // feature layer norm (cpp_net_create_feature_norm): fc[0] is a plain GEMM (GE_NONE) and ln.hip stands behind it -- y = act(gamma xhat
  // + beta) with ln_act GE_TANH or GE_RELU.  '<layer0>/LayerNorm/gamma' and '.../beta' sit behind every other variable of the flat buffer
  bool ln = false; int ln_act = GE_TANH; float ln_eps = 0.f; long ln_g_off = 0, ln_b_off = 0;
  // shared conv encoder (cpp_net_create_encoderless): a pixel actor without conv layers -- `conv` is empty, `flat` is the width the
  // critic's conv3 leaves, and ws[0].fcin[0] is nullptr until cpp_net_set_encoder makes it the encoder's very buffer (bias column included)
  bool enc_less = false; cpp_net* encoder = nullptr;
  std::vector<cpp_net*> enc_users;      // a critic: the actors bound to it (cpp_net_destroy unbinds them)
};
// a network with conv layers of its own (a low-dimensional network and an encoder-less actor have none)
inline bool has_conv(const cpp_net* n) { return !n->conv.empty(); }
// What net_create (rt_net.cpp) needs beyond the spec: which variant of the network the entry point asked for.  The defaults mean "plain";
// net_create copies the record into the cpp_net fields of the same names (their comments above say what each one is).
struct NetVariant {
  bool twin = false;                                       // twin Q heads
  int dist_n = 0; float v_min = 0.f, v_max = 0.f;          // atoms on the support [v_min, v_max] -- or, quant, that many quantiles and no support
  bool quant = false;
  bool gauss = false; float ls_lo = 0.f, ls_hi = 0.f;      // Gaussian actor and its log-std bounds
  int ln_act = 0; float ln_eps = 0.f;                      // feature layer norm: GE_TANH / GE_RELU and epsilon (0: none)
  bool enc_less = false;                                   // a pixel actor without conv layers
};
// floats from one image's row to the next in layer i's pooled output and in its gradient: conv3's pooled output is fc[0]'s input, whose
// rows end in the bias column of ones
struct PoolRows { long pool, dpool; };
inline PoolRows pool_rows(const cpp_net* n, int i) {
  const long dense = (long)n->conv[i].Hp * n->conv[i].Wp * kConvOut;
  return i == 2 ? PoolRows{(long)n->flat + 1, (long)n->flat} : PoolRows{dense, dense};
}

struct cpp_batch {
  cpp_ctx* ctx; int maxB, B; long elems; int A; int dtype;
  void* s[2]; float *a, *r, *m;
  float* white;        // [2 states][2][CPP_MAX_CHANNELS]-compatible: laid out [2][2*C] for the current C
  double* part;        // [2][maxB][2*CPP_MAX_CHANNELS]
  int stats_C;         // channels the statistics were computed for (0: none yet)
  // device-sampled minibatch that was NOT gathered: state k of row b is row slot[k][b] of direct_store (the replay store);
  // only the f16-pipe conv1 kernels can consume it (direct_store == nullptr: s[] holds the gathered copy)
  int32_t* slot[2]; const void* direct_store;
  int32_t* slot_alt[2];   // the set the NEXT minibatch's sample pass writes while conv1's dW still reads slot[] (run_minibatches)
  Arena arena;
};

#define CPP_ROWS_RING 8
#define CPP_ROWS_RING_SLOT 4096      // ints per slot (larger draws take the synchronous copy)
struct cpp_replay {
  cpp_ctx* ctx; int rows, slots, A, size; long elems;
  int store_dtype;         // CPP_F16 (replay_memory.py:32) or CPP_U8 (pixel codes k, read back as f16(k/255): half the HBM)
  void* store; int32_t *s1, *s2, *rows_in, *rows_out; float *action, *reward, *mask;
  uint64_t* counter;       // device-side Philox counter of the train steps (graph replay)
  uint64_t* counter_adhoc; // the same for cpp_replay_sample(idxs == NULL): inspection draws never move the training sampler
  int32_t* size_dev;       // rows currently in the memory, on the device: the sampler's range of captured launches
  uint64_t uid;            // unique per cpp_replay_create (graph keys: an address can be reused, this cannot)
  bool sampled;            // a sample pass has been built on this memory since the uid was issued: captured step graphs may hold its slot_stats pointer
  uint64_t write_gen;      // bumped by every call that changes rows, states or the size: a minibatch presampled before it is stale
  __half* lut; int* bad; uint16_t lut_host[256];      // CPP_U8: f16(k/255) table, "not a pixel image" flag
  // per-state whitening sums (cpp_replay_set_stats_channels): [slots][2 * stats_C] doubles, kept current by every call that writes states
  double* slot_stats; int stats_C, stats_cap; int32_t* slot_list; size_t slot_list_cap;
  void* stage; size_t stage_cap;                      // device staging of incoming states (conversion source)
  void* pinned; size_t pinned_cap; hipEvent_t pinned_free; bool pinned_busy;   // host staging: writes return before the copy ends
  // host-drawn minibatch rows on their way to rows_in (cpp_ddpg_train_rows / cpp_naf_train_rows): a ring of pinned slots, so that the
  // call returns while the previous minibatch is still running (a pageable hipMemcpyAsync would wait for the stream)
  int32_t* rows_pin; hipEvent_t rows_pin_ev[CPP_ROWS_RING]; bool rows_pin_used[CPP_ROWS_RING]; int rows_pin_k;
  // prioritized replay (cpp_replay_enable_priorities; per.hip): nullptr tree = uniform memory
  double* per_tree; int per_L; float per_alpha, per_eps;
  float* per_maxp; float* per_beta;                        // device scalars (written by value, in stream order)
  int32_t* per_rows; float* per_w;                         // the rows of the last draw and the importance weights of the last minibatch
  int32_t* per_list; float* per_vals;                      // staging of host rows / values (cpp_replay_update_priorities, write_rows)
  // n-step returns (cpp_replay_set_n_step; gather_body.h: nstep_walk): nullptr = never set, the uniform gathers.  Host copies of the
  // device words for the trainers' discount check
  NStepWords* nstep_dev; int nstep_n; float nstep_discount;
  // random shift (cpp_replay_set_random_shift; gather_body.h): pad 0 = off.  shift_dev: the augmentation counter and the gathers'
  // tickets; shift_out: the (2, B, 2) shifts of the last augmented gather.  Both allocated at the first enable.
  ShiftWords* shift_dev; int32_t* shift_out; int shift_pad, shift_H, shift_W; uint64_t shift_seed;
  Arena arena;
};
static size_t replay_esz(const cpp_replay* r) { return r->store_dtype == CPP_U8 ? 1 : sizeof(__half); }

constexpr int NORM_PARTS = 64;

// ---------------------------------------------------------------------------------------------
// Level-synchronous launch scheduler for the fused step.  The MLP heads are ~36 tiny, latency-bound
// GEMMs per minibatch; most of them are mutually independent (four networks' forwards, dW vs dX of one
// layer, the actor's and the critic's backward chains).  Ops declare their dependencies; each round
// launches every ready op, with all ready GEMMs sharing ONE launch (gemm_batch_kernel).  Everything stays
// on the ctx stream, so the order is also what a hipGraph capture records.
// ---------------------------------------------------------------------------------------------
struct OpGraph {
  struct Op { bool is_gemm; GemmArgs g; std::function<int()> fn; std::vector<int> deps; bool done; };
  std::vector<Op> ops;
  int gemm(const GemmArgs& g, std::initializer_list<int> deps) {
    Op o; o.is_gemm = true; o.g = g; o.done = false;
    for (int d : deps) if (d >= 0) o.deps.push_back(d);
    ops.push_back(o); return (int)ops.size() - 1;
  }
  int fn(std::function<int()> f, std::initializer_list<int> deps) {
    Op o; o.is_gemm = false; o.fn = f; o.done = false; memset(&o.g, 0, sizeof(o.g));
    for (int d : deps) if (d >= 0) o.deps.push_back(d);
    ops.push_back(o); return (int)ops.size() - 1;
  }
  // skip >= 0: that op is left out (the caller runs it on its own later -- the data-parallel step's split at the conv backward)
  int run(cpp_ctx* ctx, int skip = -1) {
    size_t remaining = ops.size();
    if (skip >= 0 && skip < (int)ops.size() && !ops[skip].done) { ops[skip].done = true; --remaining; }
    std::vector<int> ready; std::vector<GemmArgs> batch;
    while (remaining) {
      ready.clear(); batch.clear();
      for (size_t i = 0; i < ops.size(); ++i) {
        if (ops[i].done) continue;
        bool ok = true;
        for (int d : ops[i].deps) if (!ops[d].done) { ok = false; break; }
        if (ok) ready.push_back((int)i);
      }
      if (ready.empty()) { cpp_set_error("OpGraph: dependency cycle"); return CPP_ERR_STATE; }
      static const bool dbg = cpp_switch_set("CPP_OPGRAPH_DEBUG");
      if (dbg) {
        fprintf(stderr, "[opgraph] level:");
        for (int i : ready) {
          if (ops[i].is_gemm) fprintf(stderr, " gemm#%d(M%d N%d K%d e%d)", i, ops[i].g.M, ops[i].g.N, ops[i].g.K, ops[i].g.epi);
          else fprintf(stderr, " fn#%d", i);
        }
        fprintf(stderr, "\n");
      }
      for (int i : ready) if (!ops[i].is_gemm) RC(ops[i].fn());
      for (int i : ready) ops[i].done = true;
      remaining -= ready.size();
      for (int i : ready) if (ops[i].is_gemm) batch.push_back(ops[i].g);
      if (!batch.empty()) RC(launch_gemm_batch(ctx, batch.data(), (int)batch.size()));
    }
    return CPP_OK;
  }
};

// ---------------------------------------------------------------------------------------------
// Cached step graphs (definitions: rt_core.cpp).  A training entry point replays its launch sequence as ONE hipGraph while everything
// the captured launches hold by value stays what it was: that is the key.  gen is the owning trainer's generation number: its
// invalidate_graphs() bumps it, and every graph of that trainer is captured again at its next use.
// ---------------------------------------------------------------------------------------------
struct GraphKey {
  int B = 0, nb = 0; uint64_t seed = 0, replay_uid = 0, comm_uid = 0, gen = 0;
  bool operator==(const GraphKey& o) const {
    return B == o.B && nb == o.nb && seed == o.seed && replay_uid == o.replay_uid && comm_uid == o.comm_uid && gen == o.gen;
  }
};
enum StepRan { STEP_EAGER, STEP_CAPTURED, STEP_REPLAYED, STEP_CAPTURE_FAILED };
// Where a gradient pass left the minibatch's loss for the accessors that read it later: `parts` per-workgroup partials to add and divide
// by B (0: the loss word itself); sac_rows: the rows behind the partials of the temperature's gradient (0: none)
struct LossAt { int parts = 0, B = 0, sac_rows = 0; };
struct StepGraph {
  hipGraph_t g = nullptr; hipGraphExec_t e = nullptr; bool ok = false; GraphKey key;
  LossAt left;      // what the captured body left for the owner's accessors: kept at the capture, put back behind every launch of THIS graph
  StepGraph() = default;
  StepGraph(const StepGraph&) = delete;
  StepGraph& operator=(const StepGraph&) = delete;
  ~StepGraph() { drop(); }
  bool hit(const GraphKey& k) const { return ok && key == k; }
  void drop();
  // body's launches, captured (thread-local mode) and instantiated under key k; any failure leaves the StepGraph empty
  int capture(cpp_ctx* ctx, const GraphKey& k, const std::function<int()>& body);
  int launch(cpp_ctx* ctx);
  // a miss: the eager pass is this call's work and sets the kernels' LDS attributes (not allowed during capture); the stream drains;
  // then the capture, for the next call
  int rebuild(cpp_ctx* ctx, const GraphKey& k, const std::function<int()>& body, StepRan* ran);
};
// One call of a cached entry point: on a miss the eager pass, sync and capture; on a hit one hipGraphLaunch.  The profiler (cpp_ctx::prof)
// and `eager` keep the call on plain stream launches.  (A template, so that a hit builds no std::function.)
template <class Body>
int run_step_graph(cpp_ctx* ctx, StepGraph& G, const GraphKey& key, Body&& body, StepRan* ran = nullptr, bool eager = false) {
  StepRan how_;
  StepRan& how = ran ? *ran : how_;
  how = STEP_EAGER;
  if (ctx->prof || eager) return body();
  if (!G.hit(key)) return G.rebuild(ctx, key, body, &how);
  how = STEP_REPLAYED;
  return G.launch(ctx);
}
// The data-parallel step's graph has the collective inside.  If the runtime or RCCL refuses to capture or instantiate it, the trainer
// keeps the SAME sequence as plain stream launches (identical arithmetic on every rank) instead of failing: the very same calls have
// just run eagerly and returned CPP_OK, so whatever fails in the capture fails BECAUSE of the capture.  A failure of the eager pass is
// returned.
struct DpGraph {
  StepGraph graph; bool refused = false; char reason[256] = "";
  // cpp_*_dp_status: 0 = no graph (none run yet, or invalidated since), 1 = one hipGraph replay per outer step, 2 = stream launches (refused)
  int mode(uint64_t gen) const { return refused ? 2 : (graph.ok && graph.key.gen == gen ? 1 : 0); }
};
int dp_graph_refused(DpGraph& D, const char* learner);
template <class Body>
int run_dp_graph(cpp_ctx* ctx, DpGraph& D, const GraphKey& key, const char* learner, Body&& body, StepRan* ran = nullptr) {
  StepRan how_;
  StepRan& how = ran ? *ran : how_;
  const int rc = run_step_graph(ctx, D.graph, key, body, &how, D.refused);
  return (rc && how == STEP_CAPTURE_FAILED) ? dp_graph_refused(D, learner) : rc;
}

// kernel ids of conv layer i's forward / dW / dX launches (profile rows)
static const int kFwdKid[3] = {K_CONV1_FWD, K_CONV2_FWD, K_CONV3_FWD};
static const int kDwKid[3] = {K_CONV1_DW, K_CONV2_DW, K_CONV3_DW};
static const int kDxKid[3] = {-1, K_CONV2_DX, K_CONV3_DX};

// ---- rt_net_conv.cpp: launch descriptors of conv layer i, the trunk's forward and the conv backward sequences, whitening statistics
ConvArgs conv_fwd_args(cpp_net* n, Workspace& w, int i, const void* state, int dtype, const float* white, int B, int* mode, long white_bstride = 0);
void conv_dy_desc(cpp_net* n, Workspace& w, int i, ConvArgs& a, int B);
ConvArgs conv_dw_args(cpp_net* n, Workspace& w, int i, const void* state, int dtype, const float* white, int B, int* mode);
ConvArgs conv_dx_args(cpp_net* n, Workspace& w, int i, int B);
BnNet bn_net_desc(cpp_net* n, Workspace& w, int i);
// layer i of nn batch-norm networks for one bn.hip launch: their first workspaces, or (one network) the workspace given
BnBatch bn_batch(cpp_net* const* nets, int nn, int i, int B, Workspace* w = nullptr);
bool trunk_b16(const cpp_net* n, int dtype, int B, long white_bstride);
int net_forward_trunk(cpp_net* n, Workspace& w, const void* state, int dtype, const float* white, int B, long white_bstride = 0);
int nets_forward_trunk_fused(cpp_ctx* ctx, cpp_net* const* nets, int nn, const void* const* sts, const float* const* whs, int first_target, int dt, int B);
int nets_forward_trunk_bn(cpp_ctx* ctx, cpp_net* const* nets, int nn, const void* const* states, const float* const* whites, int dtype, int B);
int net_backward_conv(cpp_net* n, Workspace& w, int B, const void* state, int dtype, const float* white);
int nets_backward_conv(cpp_ctx* ctx, cpp_net* const* nets, int nn, int B, const void* state, int dtype, const float* white);
int batch_stats(cpp_ctx* ctx, const void* s0, const void* s1, int dtype, long elems, int B, int C, double* part, float* white);
int batch_stats_each(cpp_ctx* ctx, const void* s, int dtype, long elems, int B, int C, double* part, float* white_rows);
// ---- rt_net_fc.cpp: GEMM descriptors of the fully connected stacks, dropout, the eager forward, the heads behind the last layer
// (add_fc_backward, add_ln_backward: the end of this file)
GemmArgs mk_gemm(const float* A, long sAm, long sAk, const float* Bm, long sBk, long sBn, float* C, long ldc, int M, int N, int K, int epi, const float* Y = nullptr, long ldy = 0);
void set_dropout(GemmArgs& g, cpp_net* n, int l);
int relu_grad_epi(const cpp_net* n, int producer_layer);
int bump_dropout(cpp_net* n);
int net_forward_fc(cpp_net* n, Workspace& w, int from, int B, const float* action);
GemmArgs fc_fwd_args(cpp_net* n, Workspace& w, int l, int B);
GemmArgs fc_dw_args(cpp_net* n, Workspace& w, int l, int B, const float* dz);
GemmArgs fc_dx_args(cpp_net* n, int l, int B, const float* dz, long dz_ld, int col0, int ncols, float* C, long ldc, int epi, const float* Y, long ldy);
// the same three for head 2 of a twin critic (layers [cat, nfc) of ws[0]); twin_dx_args at the concat layer adds into C (head 1's
// term is there already) before the epilogue: "(head 1) + (head 2), then the mask"
GemmArgs twin_fwd_args(cpp_net* n, Workspace& w, int l, int B);
GemmArgs twin_dw_args(cpp_net* n, Workspace& w, int l, int B);
GemmArgs twin_dx_args(cpp_net* n, Workspace& w, int l, int B);
GemmArgs twin_da_args(cpp_net* n, Workspace& w, int B, float* C, int epi, const float* Y, long ldy);      // (the concat layer's action columns)
// feature layer norm behind the layer-0 GEMMs of `nn` networks (their first workspaces), one launch: the inference path's call
int ln_forward(cpp_ctx* ctx, cpp_net* const* nets, int nn, int B);
// ... and the same launch as a node of a gradient pass, behind the GEMM level that holds those GEMMs (deps; -1: none).  Returns the node.
int add_ln_forward(struct OpGraph& G, cpp_ctx* ctx, cpp_net* const* nets, int nn, const int* deps, int B);
// where the last layer's GEMM writes: the logits of a distributional critic, `out` otherwise
inline float* fc_last_out(const Workspace& w) { return w.logits ? w.logits : w.out; }
inline float* twin_last_out(const Workspace& w) { return w.logits2 ? w.logits2 : w.out2; }      // (head 2's)
// Q (and, dz != nullptr, p (z - Q); a quantile critic: 1 / N) from the logits the forward left in w: a no-op for every other network
int dist_expect(cpp_net* n, Workspace& w, int B, float* dz);
// a = tanh(m) (eps = 0) of a Gaussian actor from the head the forward left in w, into w.out: a no-op for every other network
int gauss_mean(cpp_net* n, Workspace& w, int B, float* m_out = nullptr, float* ls_out = nullptr);
// ---- rt_net_infer.cpp: a host batch through e's trunk and the stacks of nets[0 .. nn) in inference mode (the definition says what the callers vary)
int infer_host_batch(cpp_net* e, cpp_net* const* nets, int nn, bool each, const void* state, int dtype, int B, const float* action, int A,
                     float* m_out = nullptr, float* ls_out = nullptr);
// ---- rt_replay.cpp, rt_ddpg.cpp, rt_ddpg_pass.cpp (what the two learners share of a step: the end of this file)
int batch_ensure_stats(cpp_batch* b, int C);
uint64_t replay_next_uid();      // graph keys: a fresh uid per cpp_replay_create and per change of a sampled memory's statistics setting
int nstep_refuse(const cpp_replay* r, float discount, const char* who);      // CPP_ERR_ARG: an n-step memory folded with another discount
int train_entry_checks(const char* who, const cpp_replay* r, int B, int maxB, long state_elems, int A, float discount, const int* n_batches = nullptr,
                       bool nstep = true);      // batch range, replay shape, n-step discount, empty memory, prioritized batch limit
GatherArgs replay_gather_args(cpp_replay* r, int B, const int32_t* rows_dev, uint64_t seed, const uint64_t* counter_dev, int channels, cpp_batch* out, bool direct, int* C_out,
                              bool augment = true);      // augment: a memory with random shift on gathers shifted (false: cpp_replay_sample, the stored pixels)
// feeds_route: the minibatch is a training call's -- its largest whitening scale goes into the context's white_max_dev, which that call
// publishes to the conv1 route.  false: an inspection gather (cpp_replay_sample, cpp_replay_gather_shifted), which a later training
// call must not publish in its own name
int replay_sample_finish(cpp_replay* r, int B, int C, int channels, cpp_batch* out, uint64_t* bump = nullptr, bool* bumped = nullptr, bool feeds_route = true);
int replay_sample_device(cpp_replay* r, int B, const int32_t* rows_dev, uint64_t seed, const uint64_t* counter_dev, int channels, cpp_batch* out, bool direct = false,
                         uint64_t* bump = nullptr, bool* bumped = nullptr, bool augment = true, bool feeds_route = true);
int replay_stage_rows(cpp_replay* r, const int32_t* idxs, int n, const char* who);
PerArgs per_args(const cpp_replay* r);            // the memory's tree, size word, maximum and beta; nothing to write, nothing to draw
int per_refuse(const cpp_replay* r, const char* who);   // CPP_ERR_ARG (with the message) on a prioritized memory
int replay_upload_rows(cpp_replay* r, const int32_t* idxs, int n, const char* who);      // the same check, a plain copy (the eager step on the caller's rows)
const float* white_of(cpp_batch* b, int which, int C);
bool direct_replay_ok(cpp_net* a, cpp_replay* r, int B);

// ---- communicator of the data-parallel learners (rt_comm.cpp): one rank per cpp_ctx, RCCL over xGMI
struct cpp_comm {
  cpp_ctx* ctx; ncclComm_t comm; int rank, world;
  uint64_t uid;                // unique per cpp_comm_create (graph keys: an address can be reused by the allocator, this cannot)
  hipStream_t side;            // second stream: collectives that overlap the conv backward of the same minibatch
  hipEvent_t ev_fc, ev_bwd, ev_done;
  double* scratch;             // CPP_COMM_SCRATCH_WORDS device doubles of cpp_comm_max_doubles (allocated on first use)
};
#define CPP_COMM_SCRATCH_WORDS 8
#define NCCL_CHECK(expr)                                                                   \
  do {                                                                                     \
    ncclResult_t _r = (expr);                                                              \
    if (_r != ncclSuccess) {                                                               \
      cpp_set_error("%s:%d: %s -> %s", __FILE__, __LINE__, #expr, ncclGetErrorString(_r)); \
      return CPP_ERR_HIP;                                                                  \
    }                                                                                      \
  } while (0)

// ---------------------------------------------------------------------------------------------
// What the DDPG and the NAF learner share of a training call (definitions: rt_step.cpp; add_fc_backward, add_ln_backward: rt_net_fc.cpp)
// ---------------------------------------------------------------------------------------------
// The squared norms of `lists` gradient lists (1 or 2), folded into the kernels that write the gradients (cpp_ctx::sq_part) while the
// scope lives; groups: the list of each network of the conv backward.  left(cnt), once the pass has run: the partials it left for list
// l -- for every list, or for none (a list whose region overflowed: the sumsq kernel runs).  on == false: nothing is folded, none are left.
struct SqScope {
  cpp_ctx* c; int lists;
  SqScope(cpp_ctx* c_, int lists_, std::initializer_list<int> groups, bool on) : c(c_), lists(lists_) {
    if (!on) return;
    for (int l = 0; l < 2; ++l) c->sq_n[l] = l < lists ? 0 : -1;
    int k = 0;
    for (int g : groups) c->sq_conv_group[k++] = g;
  }
  void left(int* cnt) const {
    bool all = true;
    for (int l = 0; l < lists; ++l) all = all && c->sq_n[l] > 0;
    for (int l = 0; l < lists; ++l) cnt[l] = all ? c->sq_n[l] : 0;
  }
  ~SqScope() {
    c->sq_n[0] = c->sq_n[1] = -1;
    for (int& g : c->sq_conv_group) g = -1;
  }
};
// a dW GEMM of `list` takes the next slots of its region -- in call order, which is the order the optimiser adds them in
GemmArgs sq_gemm(cpp_ctx* ctx, int list, GemmArgs g);
// ... and so does any other kernel that writes gradients of the list: the next `count` slots, or nullptr (folding off, or the region is full)
double* sq_take(cpp_ctx* ctx, int list, int count);
// conv1 addresses its images through the sampled slots while the scope lives: `s1` read state_1's, `s2` state_2's (at most four networks)
struct SlotScope {
  cpp_net* n[4]; int nn = 0;
  SlotScope(const cpp_batch* b, std::initializer_list<cpp_net*> s1, std::initializer_list<cpp_net*> s2) {
    for (cpp_net* x : s1) { if (x->enc_less) continue; n[nn++] = x; if (b->direct_store) x->img_slot = b->slot[0]; }      // (an encoder-less actor has no conv1)
    for (cpp_net* x : s2) { if (x->enc_less) continue; n[nn++] = x; if (b->direct_store) x->img_slot = b->slot[1]; }
  }
  ~SlotScope() { for (int k = 0; k < nn; ++k) n[k]->img_slot = nullptr; }
};
// The minibatch whose sample pass has already run when the optimiser's launch of the one before it leaves: b->part holds its per-row
// statistics (B rows, C channels, `elems` values per state); tables_done: the dW reductions' launch has finished its whitening tables.
// b == nullptr: none.
struct NextBatch { const cpp_batch* b = nullptr; int B = 0, C = 0; long elems = 0; bool tables_done = false; };
// What prioritized replay hands a gradient pass: the importance weights its loss reads, and the launch the pass places behind the TD
// values of its minibatch (priorities into the tree, the next minibatch's rows and weights).  Default: a uniform memory, neither.
struct PerPass { const float* w = nullptr; std::function<int()> hook; };
// What a gradient pass that succeeded left on the host for the optimiser's launch behind it.  Default: nothing (no pass in this call,
// or one inside a replayed graph: the launches that settle it are in that graph too).
struct PassLeft {
  bool counted = false;         // its heads kernel advanced the optimiser's step counts / the policy-delay words (the launch behind must not)
  bool noise_owed = false;      // it read the noise count: exactly one increment follows it
  int sq_cnt[2] = {0, 0};       // squared-norm partials folded per list into cpp_ctx::sq_part (0: none, the sumsq kernel runs)
  LossAt loss;
};
// One optimiser launch, as its caller wants it
struct OptPlan {
  bool actor = true, critic = true;      // DDPG: the lists to apply
  bool unless_nonfinite = false;         // NAF: the update stands down while the check_numerics flag is set
  float grad_scale = 1.0f;
  uint64_t* bump = nullptr;              // the replay sampler's counter, advanced by this launch
  bool folded = false;                   // take the norms from pass.sq_cnt's partials -- gradients applied as computed only (opt_norms)
  NextBatch next;                        // the minibatch whose sample pass has already run
  bool closes_step = false;              // the last launch of an outer step: the target updates ride in it
  bool closes_call = false;              // ... of the training call: the route's publish rides in it
  PassLeft pass;                         // what the gradient pass in front left
};
// The next minibatch's sample pass as a rider of this gradient pass (cpp_ctx::ride: conv1's dW when at_dw, else the dW reductions), and
// its whitening tables as a rider of the dW reductions (cpp_ctx::st_ride).  Both point into the caller's frame: disarmed on every way out.
struct RideScope {
  cpp_ctx* c;
  explicit RideScope(cpp_ctx* c_) : c(c_) {}
  ~RideScope() { c->ride = nullptr; c->st_ride = nullptr; }
  void arm(GatherArgs* ga, const cpp_batch* b, int store_dtype, bool direct, bool at_dw) {      // direct: into the second set of slot arrays
    if (direct) { ga->out_slot[0] = b->slot_alt[0]; ga->out_slot[1] = b->slot_alt[1]; }
    c->ride = ga; c->ride_done = false; c->ride_dtype = store_dtype; c->ride_at_dw = at_dw;
  }
  void arm_stats(const StatsRide* sr) { c->st_ride = sr; c->st_ride_done = false; }
  bool rode() const { return c->ride != nullptr && c->ride_done; }
  bool tables_done() const { return c->st_ride != nullptr && c->st_ride_done && rode(); }
};

StatsRide next_stats_ride(cpp_ctx* ctx, const NextBatch& nx);              // its tables as the dW reductions' rider
void opt_next_stats(cpp_ctx* ctx, OptSegs& s, const NextBatch& nx);        // ... or as the optimiser launch's (unless they are done)
// What closes an outer step or a call rides in the optimiser's last launch of it (no next minibatch, every list applied): the soft
// update of `targets` (OptSegs::tgt, one per segment in order) and the route's publish (OptSegs::pub_*).  true: the target updates ride.
bool opt_closing_riders(cpp_ctx* ctx, OptSegs& s, const OptPlan& p, std::initializer_list<cpp_net*> targets, float coeff);
// the squared norms of the `lists` gradient lists: the partials the pass folded (list l's region of cpp_ctx::sq_part), or the sumsq kernel
int opt_norms(cpp_ctx* ctx, OptSegs& s, const OptPlan& p, int lists, double* norm_part);
// conv1's operand image of the next minibatch as a rider of the optimiser's launch: record j is network n's on state column col.
// seg >= 0: n is the network of segment seg, whose leading conv1 parameters the image workgroup updates itself (gradient pointers; the
// learner adds its optimiser's slots); seg < 0: a target network.  conv1_opens_params: the layout the rider's update assumes.
bool conv1_opens_params(const cpp_net* n);
void opt_img_net(OptSegs& s, int j, cpp_net* n, int seg, int col, const NextBatch& nx);
void opt_img_built(const OptSegs& s, cpp_net* const* nets, const NextBatch& nx);      // behind the launch: the images are current for those tables

// What a learner supplies to run_minibatches.  Plain fields for what differs between the learners, two callables for their own launches.
struct MinibatchLoop {
  cpp_ctx* ctx; cpp_replay* r; cpp_batch* step_batch;
  cpp_net* trunk;                         // the network whose conv1 decides the form of the minibatch (direct_replay_ok) and its channels
  const float* td;                        // the TD values the priorities are written from
  const int* skip_if_set = nullptr;       // prioritized memory: the priority writes stand down while this flag is set
  bool draws_bump = false;                // prioritized memory: the draws advance the sampler's counter themselves (else: the optimiser's launch)
  bool ride_ok = true;                    // the learner's own condition on the sample rider
  bool stats_switch = false;              // CPP_RIDE_STATS=0 also keeps the tables out of the optimiser's launch
  std::function<int(const PerPass& per, PassLeft* left)> gradients;      // the gradient pass on step_batch
  std::function<int(bool more, const NextBatch& next, const PassLeft& left)> apply;      // the all-reduce if any, then the optimiser's launch
};
int run_minibatches(const MinibatchLoop& L, int B, int n_batches, const int32_t* rows_dev, uint64_t seed);
int step_allreduce(cpp_ctx* ctx, cpp_comm* comm, float* grads, size_t n);      // in place, on the context's stream (inside a captured step)
// Every training entry point starts here: the context may have moved conv1 to the other kernel family (cpp_ctx::conv1_f32).  true: it has --
// *gen has moved (every cached graph of the trainer misses at its next use) and the networks' conv1 images are stale.
bool route_check(cpp_ctx* ctx, uint64_t* epoch, uint64_t* gen, std::initializer_list<cpp_net*> nets);
// dst <- src for every item with a destination, then ONE synchronisation of the context's stream (through_ctx: ctx_sync_stream)
struct Readback { void* dst; const void* src; size_t bytes; };
int read_back(cpp_ctx* ctx, std::initializer_list<Readback> items, bool through_ctx = false);
// backward of the fully connected stack of a network without an action splice, from layer `start` down: per layer [dW; db] (into the
// list's norm partials: sq_gemm) then dX, two independent GEMMs.  skip_dx: the layer whose dX a kernel in front has already produced.
// Returns the op that completes d(flat) (pixel) / dz[0].
// A network with a feature layer norm: the chain stops behind layer 1's dX, taken with GE_NONE into dz[0] (g = dL/dy; ln.hip owns the
// activation's derivative), and add_ln_backward finishes it.
int add_fc_backward(OpGraph& G, cpp_net* n, Workspace& w, int B, int start, int dep, int list, int skip_dx = -1);
// The backward of the feature layer norm of `nn` trained networks (1 or 2) in two launches for all of them -- the column sums dgamma /
// dbeta (into lists[k]'s norm partials), then g -> dz in place on dz[0] -- and layer 0's [dW; db] and dX behind them.  deps[k]: the op
// that completed network k's dz[0]; on return the op that completed its d(flat).
void add_ln_backward(OpGraph& G, cpp_ctx* ctx, cpp_net* const* nets, int nn, int* deps, const int* lists, int B);
