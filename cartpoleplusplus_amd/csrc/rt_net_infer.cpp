// networks, inference on a host batch: the one staging / statistics / forward sequence of cpp_net_forward, cpp_net_forward_each,
// cpp_net_forward_gaussian and cpp_naf_action (rt_naf.cpp); cpp_net_get_pool
#include "rt_internal.h"

// A host batch of B states through the trunk of `e` and then the fully connected stacks of nets[0 .. nn), in inference mode, on the
// context's stream; nothing is read back and nothing waits -- the caller copies what it wants from the workspaces and synchronises.
// What the callers vary: the statistics (each: every image whitened with ITS OWN, exactly as B separate batches of one would be
// (base_network.py:95-99 at B = 1) -- everything behind the whitening is row-local anyway; else the batch's), the stacks, and what
// they read back.  action: the host's (B, A) batch for a critic's concat layer, or nullptr; A is also the width of the staged action
// buffer (the network's action_dim; NAF gives its own A, its head networks' action_dim being their output width).  m_out / ls_out:
// device buffers a Gaussian actor's mean kernel also fills (cpp_net_forward_gaussian).  dist_expect / gauss_mean run on the last
// network, the one whose output is read: no-ops for every network a NAF learner accepts.
int infer_host_batch(cpp_net* e, cpp_net* const* nets, int nn, bool each, const void* state, int dtype, int B, const float* action, int A,
                     float* m_out, float* ls_out) {
  cpp_ctx* ctx = e->ctx;
  cpp_net* n = nets[nn - 1];
  HIP_CHECK(hipSetDevice(ctx->device));
  if (!e->stage_state) {
    RC(e->arena.alloc(&e->stage_state, (size_t)e->maxB * e->state_elems * sizeof(float), false));
    RC(dalloc(e->arena, &e->stage_action, (size_t)e->maxB * A));
  }
  const size_t esz = dtype == CPP_F16 ? 2 : 4;
  HIP_CHECK(hipMemcpyAsync(e->stage_state, state, (size_t)B * e->state_elems * esz, hipMemcpyHostToDevice, ctx->stream));
  if (action) HIP_CHECK(hipMemcpyAsync(e->stage_action, action, (size_t)B * A * sizeof(float), hipMemcpyHostToDevice, ctx->stream));
  const int C = e->spec.C;
  if (e->spec.pixel)
    RC(each ? batch_stats_each(ctx, e->stage_state, dtype, e->state_elems, B, C, e->stats_part, e->white_rows)
            : batch_stats(ctx, e->stage_state, nullptr, dtype, e->state_elems, B, C, e->stats_part, e->white));
  const long wbs = (each && e->spec.pixel) ? 2 * C : 0;
  e->is_training = false;                                               // IS_TRAINING: False (ddpg_cartpole.py:125, naf_cartpole.py:253)
  for (int k = 0; k < nn; ++k) nets[k]->is_training = false;
  int frc = net_forward_trunk(e, e->ws[0], e->stage_state, dtype, each ? e->white_rows : e->white, B, wbs);
  for (int k = 0; k < nn && !frc; ++k) frc = net_forward_fc(nets[k], nets[k]->ws[0], 0, B, action ? e->stage_action : nullptr);
  if (!frc) frc = dist_expect(n, n->ws[0], B, nullptr);
  if (!frc) frc = gauss_mean(n, n->ws[0], B, m_out, ls_out);
  e->is_training = true;
  for (int k = 0; k < nn; ++k) nets[k]->is_training = true;
  return frc;
}

// The network whose conv trunk (or state conversion) feeds n's fully connected stack: n itself, or the critic an encoder-less actor is
// bound to -- whose staging buffers, statistics and first workspace the inference entry points then use (ws[0].fcin[0] is shared)
static int trunk_owner(cpp_net* n, const char* who, cpp_net** e) {
  *e = n;
  if (!n->enc_less) return CPP_OK;
  if (!n->encoder) { cpp_set_error("%s: an encoder-less actor that is not bound to a critic yet (cpp_net_set_encoder)", who); return CPP_ERR_STATE; }
  *e = n->encoder;
  return CPP_OK;
}
// cpp_net_forward (each == false) / cpp_net_forward_each: B independent action_given calls in one pass (rollout-side
// inference for many env workers).  out == nullptr: nothing is copied back (cpp_net_forward_gaussian reads m_out / ls_out itself)
static int forward_host(cpp_net* n, bool each, const void* state, int state_dtype, int B, const float* action, float* out, float* m_out, float* ls_out) {
  const char* who = each ? "cpp_net_forward_each" : "cpp_net_forward";
  ARG_CHECK(n && state, "%s: NULL argument", each ? who : "cpp_net_forward / cpp_net_forward_gaussian");
  ARG_CHECK(B >= 1 && B <= n->maxB, "%s: batch %d outside [1,%d]", who, B, n->maxB);
  ARG_CHECK(state_dtype == CPP_F32 || state_dtype == CPP_F16, "%s: dtype %d", who, state_dtype);
  ARG_CHECK(n->spec.kind != CPP_CRITIC || action, "%s: critic needs an action batch", who);
  cpp_net* e = nullptr;
  RC(trunk_owner(n, who, &e));
  const int A = n->spec.action_dim, no = n->dist_n ? 1 : n->gauss ? A : n->fc.back().n_out;      // (a distributional critic returns Q, a Gaussian actor tanh(m))
  RC(infer_host_batch(e, &n, 1, each, state, state_dtype, B, action, A, m_out, ls_out));
  if (!out) return CPP_OK;
  HIP_CHECK(hipMemcpyAsync(out, n->ws[0].out, (size_t)B * no * sizeof(float), hipMemcpyDeviceToHost, n->ctx->stream));
  HIP_CHECK(ctx_sync_stream(n->ctx));
  return CPP_OK;
}

extern "C" int cpp_net_forward(cpp_net* n, const void* state, int state_dtype, int B, const float* action, float* out) {
  ARG_CHECK(out, "cpp_net_forward: NULL argument");
  return forward_host(n, false, state, state_dtype, B, action, out, nullptr, nullptr);
}
extern "C" int cpp_net_forward_each(cpp_net* n, const void* state, int state_dtype, int B, const float* action, float* out) {
  ARG_CHECK(out, "cpp_net_forward_each: NULL argument");
  return forward_host(n, true, state, state_dtype, B, action, out, nullptr, nullptr);
}

// The head of a Gaussian actor for host-side sampling (the exploration of ddpg_cartpole.py:127-134, whose noise stays outside the device
// graph): m and ls, each (B, A), of cpp_net_forward (each == 0) or cpp_net_forward_each (each != 0) on the same states
extern "C" int cpp_net_forward_gaussian(cpp_net* n, const void* state, int state_dtype, int B, int each, float* m, float* ls) {
  ARG_CHECK(n && state && m && ls, "cpp_net_forward_gaussian: NULL argument");
  if (!n->gauss) { cpp_set_error("cpp_net_forward_gaussian: not a Gaussian actor"); return CPP_ERR_STATE; }
  ARG_CHECK(B >= 1 && B <= n->maxB, "cpp_net_forward_gaussian: batch %d outside [1,%d]", B, n->maxB);
  const int A = n->spec.action_dim;
  HIP_CHECK(hipSetDevice(n->ctx->device));
  if (!n->gauss_stage) RC(dalloc(n->arena, &n->gauss_stage, (size_t)2 * n->maxB * A));
  float *dm = n->gauss_stage, *dls = n->gauss_stage + (size_t)n->maxB * A;
  RC(forward_host(n, each != 0, state, state_dtype, B, nullptr, nullptr, dm, dls));
  HIP_CHECK(hipMemcpyAsync(m, dm, (size_t)B * A * sizeof(float), hipMemcpyDeviceToHost, n->ctx->stream));
  HIP_CHECK(hipMemcpyAsync(ls, dls, (size_t)B * A * sizeof(float), hipMemcpyDeviceToHost, n->ctx->stream));
  HIP_CHECK(ctx_sync_stream(n->ctx));
  return CPP_OK;
}

extern "C" int cpp_net_get_pool(cpp_net* n, int which, int B, float* out) {
  ARG_CHECK(n && out, "cpp_net_get_pool: NULL argument");
  ARG_CHECK(B >= 1 && B <= n->maxB, "cpp_net_get_pool: batch %d", B);
  ARG_CHECK(!n->enc_less, "cpp_net_get_pool: an encoder-less actor has no conv layers (ask the critic it is bound to)");
  if (n->spec.pixel && which >= 11 && which <= 13) {   // debug: arg-max codes (0..3) of the 2x2 windows, as floats
    const ConvL& L = n->conv[which - 11];
    const size_t cnt = (size_t)B * L.Hp * L.Wp * kConvOut;
    std::vector<uint8_t> tmp(cnt);
    HIP_CHECK(hipMemcpyAsync(tmp.data(), n->ws[0].amax[which - 11], cnt, hipMemcpyDeviceToHost, n->ctx->stream));
    HIP_CHECK(ctx_sync_stream(n->ctx));
    for (size_t i = 0; i < cnt; ++i) out[i] = (float)(tmp[i] & 3);      // (bit 2 of the byte: "the pooled output is > 0", conv_kyo.h POOL_ACTIVE)
    return CPP_OK;
  }
  if (n->spec.pixel && which >= 21 && which <= 22) {   // debug: the pooled-gradient buffers of the last backward pass (dX of conv2 / conv3)
    const ConvL& L = n->conv[which - 21];
    ARG_CHECK(n->ws[0].dpool[which - 21], "cpp_net_get_pool: no gradient workspace");
    const size_t cnt = (size_t)B * L.Hp * L.Wp * kConvOut;
    HIP_CHECK(hipMemcpyAsync(out, n->ws[0].dpool[which - 21], cnt * sizeof(float), hipMemcpyDeviceToHost, n->ctx->stream));
    HIP_CHECK(ctx_sync_stream(n->ctx));
    return CPP_OK;
  }
  ARG_CHECK(n->spec.pixel && which >= 1 && which <= 3, "cpp_net_get_pool: which=%d (pixel nets, 1..3)", which);
  const ConvL& L = n->conv[which - 1];
  const size_t row = (size_t)L.Hp * L.Wp * kConvOut * sizeof(float);
  const size_t spitch = (size_t)pool_rows(n, which - 1).pool * sizeof(float);
  HIP_CHECK(hipMemcpy2DAsync(out, row, n->ws[0].pool[which - 1], spitch, row, B, hipMemcpyDeviceToHost, n->ctx->stream));
  HIP_CHECK(ctx_sync_stream(n->ctx));
  return CPP_OK;
}
