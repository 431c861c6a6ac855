// The DDPG trainer's parameter-space exploration noise (cpp_ddpg_set_param_noise, cpp_ddpg_param_noise_*; param_noise.hip; the trainer
// itself: rt_ddpg.h).  It stands beside the gradient pass: nothing here is captured into a graph, drops one, or writes what a training
// call reads -- the networks' first workspaces excepted, which every inference forward overwrites as well
#include "rt_ddpg.h"

// perturb, (measure, adapt,) count -- on the context's stream, with no host wait.  b == nullptr: no measurement
static int pn_resample(cpp_ddpg* d, cpp_batch* b) {
  cpp_ctx* ctx = d->ctx;
  cpp_net *a = d->actor, *p = d->pn_net;
  const int A = a->spec.action_dim;
  RC(launch_pn_perturb(ctx, d->pn_words, d->pn_seed, a->params, p->params, a->nparams, a->ln ? a->ln_g_off : a->nparams));
  p->wimg_key = nullptr;      // (conv1's operand image is of the copy before: the next forward builds its own)
  if (!b) return launch_pn_measure(ctx, d->pn_words, nullptr, nullptr, 0, A, d->pn_delta, d->pn_alpha, nullptr, nullptr);
  // both actors on state_1 in inference mode with the batch's statistics; a shared encoder: the critic's trunk once, both stacks behind it
  const int B = b->B, C = a->spec.pixel ? a->spec.C : 0;
  if (C > 0) RC(batch_ensure_stats(b, C));
  const float* w1 = white_of(b, 0, C);
  cpp_net* owners[2] = {d->shared ? d->critic : a, d->shared ? nullptr : p};
  cpp_net* nets[3] = {a, p, d->shared ? d->critic : nullptr};
  for (cpp_net* n : nets) if (n) n->is_training = false;      // IS_TRAINING: False (ddpg_cartpole.py:125)
  int rc = CPP_OK;
  for (cpp_net* e : owners) if (e && !rc) rc = net_forward_trunk(e, e->ws[0], b->s[0], b->dtype, w1, B);
  for (int k = 0; k < 2 && !rc; ++k) rc = net_forward_fc(nets[k], nets[k]->ws[0], 0, B, nullptr);
  for (cpp_net* n : nets) if (n) n->is_training = true;
  RC(rc);
  RC(launch_pn_measure(ctx, d->pn_words, a->ws[0].out, p->ws[0].out, B, A, d->pn_delta, d->pn_alpha, d->pn_a, d->pn_at));
  d->pn_B = B;
  return CPP_OK;
}

// what makes `p` a copy of the trainer's actor: one layout of the flat buffer, one forward
static bool pn_same_layout(const cpp_net* a, const cpp_net* p) {
  const cpp_net_spec &x = a->spec, &y = p->spec;
  bool same = x.kind == y.kind && x.pixel == y.pixel && x.H == y.H && x.W == y.W && x.C == y.C && x.state_elems == y.state_elems &&
              x.action_dim == y.action_dim && x.n_hidden == y.n_hidden && x.use_batch_norm == y.use_batch_norm && x.use_dropout == y.use_dropout;
  for (int i = 0; same && i < x.n_hidden; ++i) same = x.hidden[i] == y.hidden[i];
  return same && a->nparams == p->nparams && a->ln == p->ln && a->ln_act == p->ln_act && a->ln_eps == p->ln_eps && a->enc_less == p->enc_less &&
         a->gauss == p->gauss && a->maxB == p->maxB;
}

// Parameter-space exploration noise (Plappert et al. 2018; an extension of ddpg_cartpole.py:127-134, where the reference adds its
// Ornstein-Uhlenbeck sample to the action; include/cartpolepp_abi.h).  Ends with a resample without a batch: the copy is usable at once.
extern "C" int cpp_ddpg_set_param_noise(cpp_ddpg* d, cpp_net* perturbed_actor, float sigma0, float delta, float alpha, uint64_t seed) {
  ARG_CHECK(d, "cpp_ddpg_set_param_noise: NULL argument");
  cpp_net* p = perturbed_actor;
  if (!p) {      // off: the trainer cpp_ddpg_create left (the words stay allocated and are never read)
    ARG_CHECK(sigma0 == 0.f, "cpp_ddpg_set_param_noise: sigma %g without a perturbed network (NULL with sigma 0 switches the noise off)", (double)sigma0);
    HIP_CHECK(hipSetDevice(d->ctx->device));
    HIP_CHECK(ctx_sync_stream(d->ctx));
    d->pn_net = nullptr; d->pn_B = 0;
    return CPP_OK;
  }
  ARG_CHECK(sigma0 >= 0.f && sigma0 < 1e30f && delta > 0.f && delta < 1e30f && alpha >= 1.f && alpha < 1e30f,
            "cpp_ddpg_set_param_noise: sigma %g (finite, >= 0), target distance %g (finite, > 0), factor %g (finite, >= 1)", (double)sigma0, (double)delta,
            (double)alpha);
  ARG_CHECK(!d->sac, "cpp_ddpg_set_param_noise: a soft actor-critic trainer (its policy explores by itself)");
  ARG_CHECK(p != d->actor && p != d->tactor && p != d->critic && p != d->tcritic && !p->grads, "cpp_ddpg_set_param_noise: the perturbed network is one a trainer owns");
  ARG_CHECK(p->ctx == d->ctx, "cpp_ddpg_set_param_noise: the perturbed network lives on another context");
  ARG_CHECK(pn_same_layout(d->actor, p), "cpp_ddpg_set_param_noise: the perturbed network's layout is not the actor's (%ld parameters against %ld)",
            p->nparams, d->actor->nparams);
  ARG_CHECK(!p->enc_less || p->encoder == d->critic, "cpp_ddpg_set_param_noise: an encoder-less copy must be bound (cpp_net_set_encoder) to the trainer's critic");
  HIP_CHECK(hipSetDevice(d->ctx->device));
  HIP_CHECK(ctx_sync_stream(d->ctx));
  if (!d->pn_words) {
    const size_t n = (size_t)d->maxB * d->actor->spec.action_dim;
    RC(dalloc(d->arena, &d->pn_words, (size_t)1));
    RC(dalloc(d->arena, &d->pn_a, n));
    RC(dalloc(d->arena, &d->pn_at, n));
  }
  PnWords w; memset(&w, 0, sizeof(w));      // (read by the copy below until the stream drains)
  w.sigma = sigma0;
  HIP_CHECK(hipMemcpyAsync(d->pn_words, &w, sizeof(w), hipMemcpyHostToDevice, d->ctx->stream));
  HIP_CHECK(ctx_sync_stream(d->ctx));
  d->pn_net = p; d->pn_delta = delta; d->pn_alpha = alpha; d->pn_seed = seed; d->pn_B = 0;
  return pn_resample(d, nullptr);
}

static int pn_on(const cpp_ddpg* d, const char* who) {
  ARG_CHECK(d, "%s: NULL argument", who);
  if (!d->pn_net) { cpp_set_error("%s: parameter-space noise is off (cpp_ddpg_set_param_noise)", who); return CPP_ERR_STATE; }
  HIP_CHECK(hipSetDevice(d->ctx->device));
  return CPP_OK;
}

// One resample (an extension of ddpg_cartpole.py:127-134: what stands where the reference resets its noise process between episodes):
// batch != NULL also measures the action distance on its state_1 and adapts sigma for the next resample
extern "C" int cpp_ddpg_param_noise_resample(cpp_ddpg* d, cpp_batch* batch) {
  RC(pn_on(d, "cpp_ddpg_param_noise_resample"));
  if (batch) {
    ARG_CHECK(batch->B >= 1 && batch->B <= d->maxB, "cpp_ddpg_param_noise_resample: batch size %d outside [1,%d]", batch->B, d->maxB);
    ARG_CHECK(batch->elems == d->actor->state_elems && batch->ctx == d->ctx, "cpp_ddpg_param_noise_resample: batch shape does not match the networks");
    ARG_CHECK(!batch->direct_store, "cpp_ddpg_param_noise_resample: a minibatch without a gathered copy of its states");
  }
  return pn_resample(d, batch);
}

// the device's words (ddpg_cartpole.py:127-134 extended: the noise's scale is state of the learner now).  Waits for the stream.
extern "C" int cpp_ddpg_param_noise_status(cpp_ddpg* d, float* sigma, float* distance, uint64_t* n, int* adapted) {
  RC(pn_on(d, "cpp_ddpg_param_noise_status"));
  PnWords w;
  RC(read_back(d->ctx, {{&w, d->pn_words, sizeof(w)}}, true));
  if (sigma) *sigma = w.sigma;
  if (distance) *distance = w.d;
  if (n) *n = w.n;
  if (adapted) *adapted = w.adapted ? 1 : 0;
  return CPP_OK;
}

// sigma and the draw count for checkpoints and tests (util.py:88-90: tf.train.Saver saves every variable of the graph; the noise of
// ddpg_cartpole.py:127-134 had none).  set == 0: read into the pointers; otherwise written from them (both needed); the perturbed copy
// stays what it is until the next resample.
extern "C" int cpp_ddpg_param_noise_state(cpp_ddpg* d, int set, float* sigma, uint64_t* n) {
  RC(pn_on(d, "cpp_ddpg_param_noise_state"));
  PnWords w;
  RC(read_back(d->ctx, {{&w, d->pn_words, sizeof(w)}}, true));
  if (!set) {
    if (sigma) *sigma = w.sigma;
    if (n) *n = w.n;
    return CPP_OK;
  }
  ARG_CHECK(sigma && n, "cpp_ddpg_param_noise_state: NULL argument");
  ARG_CHECK(*sigma >= 0.f && *sigma < 1e30f, "cpp_ddpg_param_noise_state: sigma %g (finite, >= 0)", (double)*sigma);
  w.sigma = *sigma; w.n = *n;
  HIP_CHECK(hipMemcpyAsync(d->pn_words, &w, sizeof(w), hipMemcpyHostToDevice, d->ctx->stream));
  HIP_CHECK(ctx_sync_stream(d->ctx));
  return CPP_OK;
}

// the actor's and the perturbed actor's actions, each (B, A), of the last measured resample (the exploration of ddpg_cartpole.py:127-134
// compared with the policy it perturbs).  NULL pointers are skipped.
extern "C" int cpp_ddpg_last_param_noise(cpp_ddpg* d, int B, float* a, float* at) {
  RC(pn_on(d, "cpp_ddpg_last_param_noise"));
  if (d->pn_B < 1) { cpp_set_error("cpp_ddpg_last_param_noise: no resample has measured a batch yet"); return CPP_ERR_STATE; }
  ARG_CHECK(B >= 1 && B <= d->pn_B, "cpp_ddpg_last_param_noise: batch %d outside [1,%d] (the rows of the last measured resample)", B, d->pn_B);
  const size_t n = (size_t)B * d->actor->spec.action_dim * sizeof(float);
  return read_back(d->ctx, {{a, d->pn_a, n}, {at, d->pn_at, n}}, true);
}
