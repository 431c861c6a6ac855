// NAF train ops and inner step (cpp_naf_*)
#include <utility>
#include "rt_internal.h"

// ---------------------------------------------------------------------------------------------
// NAF (naf_cartpole.py)
// ---------------------------------------------------------------------------------------------
struct cpp_naf {
  cpp_ctx* ctx; cpp_net *value, *tvalue, *mu, *lv; int share; cpp_naf_hyper hp;
  int maxB, A, NL; long nV, nM, nL;
  float* gradbuf; float *m, *v;           // optimiser state over the same flat layout (Momentum / Adam)
  float *adv, *q, *td, *stats;            // stats: [0] loss [1] norm
  int* nonfinite; uint64_t* opt_step; double* norm_part;
  double* heads_part; unsigned* heads_ticket;      // fused heads kernel (naf_heads_kernel): per-workgroup td^2 sums + bad flags, arrival counter
  StepGraph graph;           // the full inner step (cpp_naf_train_step)
  StepGraph hgraph;          // the data-parallel half step (sample + gradients) as a graph of its own
  StepGraph rgraph;          // ONE minibatch on host-drawn rows up to (not including) the optimiser (cpp_naf_train_rows)
  DpGraph dgraph;            // the data-parallel step
  StepGraph agraph;          // ... and including it, the loss coming back later (cpp_naf_train_rows_async / cpp_naf_loss_wait): pinned (loss, flag) slots
  uint64_t graph_gen = 0;    // part of every graph's key: moved by naf_route_check, every graph is then captured again
  uint64_t epoch;            // cpp_ctx::kernel_epoch the cached graphs were captured under (naf_route_check)
  float* res_pin; hipEvent_t res_ev[CPP_NAF_TICKETS]; uint64_t next_ticket;
  uint64_t dp_local;       // minibatches applied locally since the last parameter averaging (periodic mode)
  cpp_batch* step_batch;
  Arena arena;
};

extern "C" int cpp_naf_create(cpp_ctx* ctx, cpp_net* value, cpp_net* tvalue, cpp_net* mu, cpp_net* lv, int share,
                              const cpp_naf_hyper* hp, cpp_naf** out) {
  ARG_CHECK(ctx && value && tvalue && mu && lv && hp && out, "cpp_naf_create: NULL argument");
  for (cpp_net* n : {value, tvalue, mu, lv}) ARG_CHECK(!n->twin, "cpp_naf_create: a twin Q network (cpp_net_create_twin_q) belongs to the DDPG learner");
  for (cpp_net* n : {value, tvalue, mu, lv}) ARG_CHECK(!n->ln, "cpp_naf_create: a network with a feature layer norm (cpp_net_create_feature_norm) belongs to the DDPG learner");
  for (cpp_net* n : {value, tvalue, mu, lv}) ARG_CHECK(!n->enc_less, "cpp_naf_create: an encoder-less actor (cpp_net_create_encoderless) belongs to the DDPG learner");
  for (cpp_net* n : {value, tvalue, mu, lv}) ARG_CHECK(!n->gauss, "cpp_naf_create: a Gaussian actor (cpp_net_create_gaussian) belongs to the DDPG learner");
  for (cpp_net* n : {value, tvalue, mu, lv}) ARG_CHECK(!n->quant, "cpp_naf_create: a quantile critic (cpp_net_create_quantile) belongs to the DDPG learner");
  for (cpp_net* n : {value, tvalue, mu, lv}) ARG_CHECK(!n->dist_n, "cpp_naf_create: a distributional critic (cpp_net_create_distributional) belongs to the DDPG learner");
  for (cpp_net* n : {value, tvalue, mu, lv}) ARG_CHECK(n->spec.kind == CPP_HEAD, "cpp_naf_create: networks must be CPP_HEAD");
  ARG_CHECK(value->spec.head_out == 1 && tvalue->spec.head_out == 1 && value->nparams == tvalue->nparams,
            "cpp_naf_create: value / target_value shapes");
  const int A = mu->spec.head_out;
  ARG_CHECK(A >= 1 && A <= 8, "cpp_naf_create: action_dim %d outside [1, 8] (the NAF head's L matrix is at most 8 x 8)", A);
  ARG_CHECK(lv->spec.head_out == A * (A + 1) / 2, "cpp_naf_create: mu has %d outputs, l_values %d (want A and A(A+1)/2)",
            A, lv->spec.head_out);
  ARG_CHECK(mu->spec.head_act == 2 && lv->spec.head_act == 0 && value->spec.head_act == 0, "cpp_naf_create: head activations");
  ARG_CHECK(hp->optimiser >= CPP_OPT_SGD && hp->optimiser <= CPP_OPT_ADAM, "cpp_naf_create: optimiser %d", hp->optimiser);
  const int rep = value->fc.back().n_in;
  if (share) {
    for (cpp_net* n : {mu, lv})
      ARG_CHECK(!n->spec.pixel && n->fc.size() == 1 && n->fc[0].n_in == rep,
                "cpp_naf_create: shared heads must be head-only nets over the %d-wide representation", rep);
  } else {
    for (cpp_net* n : {mu, lv}) ARG_CHECK(n->state_elems == value->state_elems, "cpp_naf_create: state shapes differ");
  }
  HIP_CHECK(hipSetDevice(ctx->device));
  cpp_naf* f = new cpp_naf();
  f->arena.stream = ctx->stream;
  f->ctx = ctx; f->value = value; f->tvalue = tvalue; f->mu = mu; f->lv = lv; f->share = share; f->hp = *hp;
  f->maxB = value->maxB; f->A = A; f->NL = A * (A + 1) / 2;
  for (cpp_net* n : {tvalue, mu, lv}) if (n->maxB < f->maxB) f->maxB = n->maxB;
  f->nV = value->nparams; f->nM = mu->nparams; f->nL = lv->nparams;
  f->step_batch = nullptr;
  f->epoch = ctx->kernel_epoch;
  f->res_pin = nullptr; f->next_ticket = 0; memset(f->res_ev, 0, sizeof(f->res_ev));
  f->dp_local = 0;
  const size_t nall = (size_t)(f->nV + f->nM + f->nL);
  int rc = dalloc(f->arena, &f->gradbuf, nall);
  if (!rc) rc = dalloc(f->arena, &f->m, nall);
  if (!rc) rc = dalloc(f->arena, &f->v, nall);
  if (!rc) rc = dalloc(f->arena, &f->adv, (size_t)f->maxB);
  if (!rc) rc = dalloc(f->arena, &f->q, (size_t)f->maxB);
  if (!rc) rc = dalloc(f->arena, &f->td, (size_t)f->maxB);
  if (!rc) rc = dalloc(f->arena, &f->stats, (size_t)4);
  if (!rc) rc = dalloc(f->arena, &f->nonfinite, (size_t)1);
  if (!rc) rc = dalloc(f->arena, &f->opt_step, (size_t)1);
  if (!rc) rc = dalloc(f->arena, &f->norm_part, (size_t)OPT_MAX_SEGS * NORM_PARTS);
  if (!rc) rc = dalloc(f->arena, &f->heads_part, (size_t)2 * NAF_HEADS_MAX_WGS);
  if (!rc) rc = dalloc(f->arena, &f->heads_ticket, (size_t)1);
  if (rc) { f->arena.release(); delete f; return rc; }
  value->grads = f->gradbuf; mu->grads = f->gradbuf + f->nV; lv->grads = f->gradbuf + f->nV + f->nM;
  if (share) {      // the heads read value's input_state_representation in place (naf_cartpole.py:151-152,176-177)
    mu->ws[0].fcin[0] = value->ws[0].fcin.back();
    lv->ws[0].fcin[0] = value->ws[0].fcin.back();
  }
  HIP_CHECK(ctx_sync_stream(ctx));
  ctx->n_trainers += 1;
  *out = f;
  return CPP_OK;
}

extern "C" int cpp_naf_destroy(cpp_naf* f) {
  if (!f) return CPP_OK;
  (void)hipSetDevice(f->ctx->device);
  (void)ctx_sync_stream(f->ctx);
  if (f->res_pin) (void)hipHostFree(f->res_pin);
  for (hipEvent_t e : f->res_ev) if (e) (void)hipEventDestroy(e);
  if (f->step_batch) cpp_batch_destroy(f->step_batch);
  f->value->grads = nullptr; f->mu->grads = nullptr; f->lv->grads = nullptr;
  f->ctx->n_trainers -= 1;
  f->arena.release(); delete f; return CPP_OK;      // (the cached graphs go with their StepGraph members)
}

static int naf_check_batch(cpp_naf* f, cpp_batch* b, const char* who) {
  ARG_CHECK(f && b, "%s: NULL argument", who);
  ARG_CHECK(b->B >= 1 && b->B <= f->maxB, "%s: batch size %d outside [1,%d]", who, b->B, f->maxB);
  ARG_CHECK(b->elems == f->value->state_elems && b->A == f->A, "%s: batch shape does not match the networks", who);
  if (f->value->spec.pixel) RC(batch_ensure_stats(b, f->value->spec.C));
  return CPP_OK;
}

// value / mu / l_values on state_1 (device pointer), optionally V'(state_2)
static int naf_forward(cpp_naf* f, const void* s1, const void* s2, int dtype, const float* w1, const float* w2, int B) {
  cpp_net *v = f->value, *tv = f->tvalue;
  RC(net_forward_trunk(v, v->ws[0], s1, dtype, w1, B));
  RC(net_forward_fc(v, v->ws[0], 0, B, nullptr));
  for (cpp_net* n : {f->mu, f->lv}) {
    if (!f->share) RC(net_forward_trunk(n, n->ws[0], s1, dtype, w1, B));
    RC(net_forward_fc(n, n->ws[0], 0, B, nullptr));
  }
  if (s2) {
    RC(net_forward_trunk(tv, tv->ws[0], s2, dtype, w2, B));
    RC(net_forward_fc(tv, tv->ws[0], 0, B, nullptr));
  }
  return CPP_OK;
}

static int naf_head(cpp_naf* f, cpp_batch* b, bool backward, const float* per_w = nullptr) {
  NafHeadArgs a; memset(&a, 0, sizeof(a));
  a.value = f->value->ws[0].out; a.mu = f->mu->ws[0].out; a.lv = f->lv->ws[0].out;
  a.action = b->a; a.reward = b->r; a.mask = b->m; a.target_value = f->tvalue->ws[0].out;
  a.discount = f->hp.discount; a.B = b->B; a.A = f->A;
  a.adv = f->adv; a.q = f->q; a.td = f->td; a.loss = f->stats; a.nonfinite = f->nonfinite;
  if (backward) {
    a.d_value = f->value->ws[0].dz.back(); a.d_mu_z = f->mu->ws[0].dz.back(); a.d_l = f->lv->ws[0].dz.back();
  }
  return launch_naf_head(f->ctx, a, per_w);
}

// One NAF minibatch (naf_cartpole.py:264-272 without the apply) as a dependency graph, batched like the DDPG
// step: conv layers of the networks that run them share launches, independent GEMMs share launches.
// fold (the fused single-learner step only: the gradients are applied as computed): the kernels that write the gradients leave
// their share of the list's squared norm in cpp_ctx::sq_part (as the DDPG step, rt_ddpg.cpp) and the heads kernel advances the
// optimiser's step counter -- naf_apply then runs neither the sumsq nor the counter kernel
// bump_step: the heads kernel also advances the optimiser's step counter (only where no check_numerics flag can stand the update down)
// per: rt_internal.h, PerPass.  *left: what the pass left for the naf_apply behind it, written only when it succeeds.
static int naf_compute_gradients(cpp_naf* f, cpp_batch* b, PassLeft* left, bool fold = false, bool bump_step = true, const PerPass& per = PerPass()) {
  cpp_ctx* ctx = f->ctx;
  SqScope sq_scope(ctx, 1, {0, 0, 0, 0}, fold && !f->value->spec.use_batch_norm);      // ONE list, every conv network's in it
  cpp_net *v = f->value, *tv = f->tvalue, *mu = f->mu, *lv = f->lv;
  const int B = b->B, C = v->spec.pixel ? v->spec.C : 0, dt = b->dtype;
  const float *w1 = white_of(b, 0, C), *w2 = white_of(b, 1, C);
  const void *s1 = b->direct_store ? b->direct_store : b->s[0], *s2 = b->direct_store ? b->direct_store : b->s[1];
  SlotScope slot_scope(b, {v, mu, lv}, {tv});      // (conv1 addresses its images through the sampled slots while this graph runs)
  const bool share = f->share != 0;
  OpGraph G;

  // ---- forward trunks
  cpp_net* tn[4]; const void* ts[4]; const float* tw[4]; int nt = 0;
  tn[nt] = v; ts[nt] = s1; tw[nt] = w1; ++nt;
  if (!share) { tn[nt] = mu; ts[nt] = s1; tw[nt] = w1; ++nt; tn[nt] = lv; ts[nt] = s1; tw[nt] = w1; ++nt; }
  tn[nt] = tv; ts[nt] = s2; tw[nt] = w2; ++nt;
  int t1;
  if (v->spec.pixel && !v->spec.use_batch_norm) {
    std::vector<cpp_net*> nets(tn, tn + nt); std::vector<const void*> sts(ts, ts + nt); std::vector<const float*> whs(tw, tw + nt);
    // one launch per conv layer for all trunks, conv3 as conv2's tail, the target network forward-only (rt_net_conv.cpp)
    t1 = G.fn([=] { return nets_forward_trunk_fused(ctx, nets.data(), nt, sts.data(), whs.data(), nt - 1, dt, B); }, {});
  } else {
    std::vector<cpp_net*> nets(tn, tn + nt); std::vector<const void*> sts(ts, ts + nt); std::vector<const float*> whs(tw, tw + nt);
    t1 = G.fn([=] {        // low-dim states, or batch-norm trunks (training mode: naf_cartpole.py:271)
      if (nets[0]->spec.pixel) return nets_forward_trunk_bn(ctx, nets.data(), nt, sts.data(), whs.data(), dt, B);
      for (int k = 0; k < nt; ++k) RC(net_forward_trunk(nets[k], nets[k]->ws[0], sts[k], dt, whs[k], B));
      return (int)CPP_OK; }, {});
  }
  // ---- forward MLPs
  auto chain = [&](cpp_net* n, int from, int dep) {
    for (int l = from; l < (int)n->fc.size(); ++l) dep = G.gemm(fc_fwd_args(n, n->ws[0], l, B), {dep});
    return dep;
  };
  const int Lh = (int)v->fc.size() - 1;                 // value's 'fc' head
  // Shared representation with a hidden stack (the reference's pixel NAF, naf_cartpole.py:151-152): the four head layers, the
  // head arithmetic and d(representation) are ONE row-local launch (naf_heads_kernel, gemm.hip) instead of a forward GEMM level,
  // the head kernel and three dependent GEMM levels.  CPP_NAF_HEADS=0 (ablation build): the GEMM levels.
  static const bool no_fused_heads = cpp_switch_off("CPP_NAF_HEADS");
  NafHeadsArgs nh; memset(&nh, 0, sizeof(nh));
  bool fused = share && Lh > 0 && !no_fused_heads;
  if (fused) {
    const FcL& hv = v->fc[Lh];
    nh.B = B; nh.A = f->A; nh.rep = hv.n_in; nh.discount = f->hp.discount;
    nh.x = v->ws[0].fcin[Lh]; nh.xt = tv->ws[0].fcin[Lh]; nh.ldx = hv.n_in + 1;
    nh.Wv = v->params + hv.w_off; nh.Wmu = mu->params + mu->fc[0].w_off; nh.Wl = lv->params + lv->fc[0].w_off; nh.Wvt = tv->params + tv->fc[Lh].w_off;
    nh.action = b->a; nh.reward = b->r; nh.mask = b->m;
    nh.value = v->ws[0].out; nh.mu = mu->ws[0].out; nh.lv = lv->ws[0].out; nh.target_value = tv->ws[0].out;
    nh.adv = f->adv; nh.q = f->q; nh.td = f->td; nh.loss = f->stats; nh.nonfinite = f->nonfinite;
    nh.d_value = v->ws[0].dz[Lh]; nh.d_mu_z = mu->ws[0].dz[0]; nh.d_l = lv->ws[0].dz[0];
    nh.drep = v->ws[0].dz[Lh - 1]; nh.ldd = hv.n_in; nh.epi = relu_grad_epi(v, Lh - 1); nh.Y = v->ws[0].fcin[Lh]; nh.ldy = hv.n_in + 1;
    nh.part = f->heads_part; nh.ticket = f->heads_ticket;
    nh.step_bump = (fold && bump_step) ? (unsigned long long*)f->opt_step : nullptr;
    fused = naf_heads_supported(nh) && (nh.epi == GE_MUL_RELU_GRAD || nh.epi == GE_MUL_RELU_GRAD_X2);
  }
  // ... and with exactly two hidden layers (the reference's 100, 50) the second one joins that launch, forward and backward, on the
  // matrix pipes (naf_mlp_kernel): one forward and one backward GEMM level are left.  CPP_NAF_MLP=0 (ablation build): naf_heads_kernel.
  static const bool no_mlp = cpp_switch_off("CPP_NAF_MLP");
  NafMlpArgs nm; memset(&nm, 0, sizeof(nm));
  bool mlp = fused && !no_mlp && Lh == 2 && v->fc[0].act == GE_RELU && v->fc[1].act == GE_RELU && tv->fc[1].act == GE_RELU &&
             relu_grad_epi(v, 0) == GE_MUL_RELU_GRAD && relu_grad_epi(v, 1) == GE_MUL_RELU_GRAD && !v->drop_counter;
  if (mlp) {
    nm.h = nh;
    nm.x0 = v->ws[0].fcin[1]; nm.x0t = tv->ws[0].fcin[1]; nm.ld0 = v->fc[1].n_in + 1; nm.n0 = v->fc[1].n_in;
    nm.W1 = v->params + v->fc[1].w_off; nm.W1t = tv->params + tv->fc[1].w_off;
    nm.h1_out = v->ws[0].fcin[2]; nm.ld1 = v->fc[2].n_in + 1; nm.dz0 = v->ws[0].dz[0];
    mlp = naf_mlp_supported(nm);
  }
  int vrep = t1;
  for (int l = 0; l < Lh - (mlp ? 1 : 0); ++l) vrep = G.gemm(fc_fwd_args(v, v->ws[0], l, B), {vrep});
  int vout, tvout, muout, lvout;
  if (fused) {
    int tvrep = t1;
    for (int l = 0; l < Lh - (mlp ? 1 : 0); ++l) tvrep = G.gemm(fc_fwd_args(tv, tv->ws[0], l, B), {tvrep});
    vout = vrep; tvout = tvrep; muout = lvout = vrep;
  } else {
    vout = G.gemm(fc_fwd_args(v, v->ws[0], Lh, B), {vrep});
    tvout = chain(tv, 0, t1);
    muout = share ? chain(mu, 0, vrep) : chain(mu, 0, t1);
    lvout = share ? chain(lv, 0, vrep) : chain(lv, 0, t1);
  }
  if (v->drop_counter) {     // --use-dropout: count this training-mode forward of every network with a hidden stack
    G.fn([=] { return bump_dropout(v); }, {vout});
    G.fn([=] { return bump_dropout(tv); }, {tvout});
    if (!share) { G.fn([=] { return bump_dropout(mu); }, {muout}); G.fn([=] { return bump_dropout(lv); }, {lvout}); }
  }
  // ---- NAF head: L, advantage, TD loss and the gradients of the three head outputs (prioritized replay: weighted by per.w)
  const float* per_w = per.w;
  const int head = mlp ? G.fn([=] { return launch_naf_mlp(ctx, nm, per_w); }, {vout, tvout})
                 : fused ? G.fn([=] { return launch_naf_heads(ctx, nh, per_w); }, {vout, tvout})
                         : G.fn([=] { return naf_head(f, b, true, per_w); }, {vout, tvout, muout, lvout});
  // (prioritized replay: as soon as the TD values are known -- the next op level, ahead of the conv backward that carries the next
  // minibatch's gather)
  if (per.hook) G.fn(per.hook, {head});

  // ---- backward
  if (!share) {
    const int dv = add_fc_backward(G, v, v->ws[0], B, (int)v->fc.size() - 1, head, 0);
    const int dm = add_fc_backward(G, mu, mu->ws[0], B, (int)mu->fc.size() - 1, head, 0);
    const int dl = add_fc_backward(G, lv, lv->ws[0], B, (int)lv->fc.size() - 1, head, 0);
    if (v->spec.pixel) {
      cpp_net* bn[3] = {v, mu, lv};
      G.fn([=] { return nets_backward_conv(ctx, bn, 3, B, s1, dt, w1); }, {dv, dm, dl});
    }
  } else {
    // shared representation: head gradients, then d(rep) = sum of the three heads' contributions
    const FcL& hv = v->fc[Lh];
    const int rep = hv.n_in;
    struct Head { cpp_net* n; const FcL* L; const float* dz; };
    Head heads[3] = {{v, &hv, v->ws[0].dz[Lh]}, {mu, &mu->fc[0], mu->ws[0].dz[0]}, {lv, &lv->fc[0], lv->ws[0].dz[0]}};
    float* drep = nullptr; long ldd = rep; int final_epi = GE_NONE; const float* Y = nullptr; long ldy = 0;
    if (Lh > 0) { drep = v->ws[0].dz[Lh - 1]; final_epi = relu_grad_epi(v, Lh - 1); Y = v->ws[0].fcin[Lh]; ldy = rep + 1; }
    else if (v->spec.pixel) { drep = v->ws[0].dpool[2]; }
    int dep = head;
    for (int k = 0; k < 3; ++k) {
      const Head& h = heads[k];
      const float* x = v->ws[0].fcin[Lh];        // [rep, 1] rows, shared by the three heads
      G.gemm(sq_gemm(ctx, 0, mk_gemm(x, 1, rep + 1, h.dz, h.L->n_out, 1, h.n->grads + h.L->w_off, h.L->n_out, rep + 1, h.L->n_out, B, GE_NONE)), {head});
      if (drep && !fused) {
        GemmArgs g = mk_gemm(h.dz, h.L->n_out, 1, h.n->params + h.L->w_off, 1, h.L->n_out, drep, ldd, B, rep, h.L->n_out,
                             k == 2 ? final_epi : GE_NONE, k == 2 ? Y : nullptr, ldy);
        g.accumulate = k > 0;
        dep = G.gemm(g, {dep});                  // accumulation order value -> mu -> l_values is fixed
      }
    }
    if (mlp) G.gemm(sq_gemm(ctx, 0, fc_dw_args(v, v->ws[0], 1, B, v->ws[0].dz[1])), {head});      // (dz[1] and dz[0] came out of naf_mlp_kernel)
    const int dv = add_fc_backward(G, v, v->ws[0], B, mlp ? 0 : Lh - 1, dep, 0);
    if (v->spec.pixel) {     // conv3's and conv2's dW + dX as one launch each, like the DDPG step (nets_backward_conv)
      cpp_net* bn[1] = {v};
      G.fn([=] { return nets_backward_conv(ctx, bn, 1, B, s1, dt, w1); }, {dv});
    }
  }
  DwPendingGuard pending(ctx);      // (a failure below drops what was queued)
  RC(G.run(ctx));
  RC(flush_dw_reduce(ctx));
  left->counted = fused && nh.step_bump != nullptr;
  sq_scope.left(left->sq_cnt);
  return CPP_OK;
}

// The optimiser's launch (rt_internal.h: OptPlan).  next: that minibatch's whitening tables are finished by this launch's extra grid
// row unless they are done.  *targets_left: the target update and the route's publish left with this launch (the plan closes an outer step).
static int naf_apply(cpp_naf* f, const OptPlan& plan, bool* targets_left = nullptr) {
  const bool unless_nonfinite = plan.unless_nonfinite;
  const float grad_scale = plan.grad_scale;
  const NextBatch& nx = plan.next;
  OptSegs s; memset(&s, 0, sizeof(s));
  if (unless_nonfinite) s.skip_if = f->nonfinite;
  s.bump = plan.bump;
  f->value->wimg_key = nullptr; f->mu->wimg_key = nullptr;      // (the parameters change)
  opt_next_stats(f->ctx, s, nx);
  s.nseg = 3; s.kind = f->hp.optimiser; s.momentum = f->hp.momentum; s.beta1 = f->hp.beta1; s.beta2 = f->hp.beta2;
  s.epsilon = f->hp.epsilon; s.step = f->opt_step;
  cpp_net* nets[3] = {f->value, f->mu, f->lv};
  long off = 0;
  for (int k = 0; k < 3; ++k) {
    s.p[k] = nets[k]->params; s.g[k] = f->gradbuf + off; s.m[k] = f->m + off; s.v[k] = f->v + off;
    s.n[k] = nets[k]->nparams; s.lr[k] = f->hp.learning_rate; s.group[k] = 0;      // ONE list, one global norm
    off += nets[k]->nparams;
  }
  // the target value network's soft update (naf_cartpole.py:373) and the route's publish leave with an outer step's last launch
  const bool ride = opt_closing_riders(f->ctx, s, plan, {f->tvalue}, f->hp.target_update_rate);
  if (targets_left) *targets_left = ride;
  const bool bumped = plan.pass.counted;
  // (unless_nonfinite: a skipped update must not count as an optimiser step -- Adam's bias correction reads the count; the heads
  // kernel's bump was undone below by never happening: naf_compute_gradients leaves it to this launch when the flag can stand the update down)
  if (!bumped) RC(launch_counter_add(f->ctx, f->opt_step, 1, unless_nonfinite ? f->nonfinite : nullptr));
  RC(opt_norms(f->ctx, s, plan, 1, f->norm_part));
  // conv1's operand images of the next minibatch ride along (shared trunk: the value network's conv1 on state_1, the target value
  // network's on state_2; SGD or Momentum -- Adam's update is not restated in this learner's rider)
  cpp_net* inets[2] = {f->value, f->tvalue};
  const ConvL* L0 = (f->share && f->value->spec.pixel) ? &f->value->conv[0] : nullptr;
  const bool img = nx.b && nx.C > 0 && L0 && !unless_nonfinite && !f->value->spec.use_batch_norm && nx.B >= 2 &&
                   (s.kind == OPT_SGD || s.kind == OPT_MOMENTUM) && conv_rs16_ok(f->ctx, L0->Cin, L0->H, L0->W, kConvOut) &&
                   conv1_opens_params(f->value);
  if (img) {
    s.img_n = 2; s.img_cin = L0->Cin;
    opt_img_net(s, 0, f->value, 0, 0, nx);
    s.img[0].mw = s.m[0] + L0->w_off; s.img[0].mb = s.m[0] + L0->b_off;
    opt_img_net(s, 1, f->tvalue, -1, 1, nx);
  }
  RC(launch_opt_apply(f->ctx, s, grad_scale, f->hp.gradient_clip, f->norm_part, NORM_PARTS, f->stats + 1));
  opt_img_built(s, inets, nx);
  return CPP_OK;
}

extern "C" int cpp_naf_action(cpp_naf* f, const void* state, int dtype, int B, float* out) {
  ARG_CHECK(f && state && out, "cpp_naf_action: NULL argument");
  ARG_CHECK(B >= 1 && B <= f->maxB, "cpp_naf_action: batch %d outside [1,%d]", B, f->maxB);
  ARG_CHECK(dtype == CPP_F32 || dtype == CPP_F16, "cpp_naf_action: dtype %d", dtype);
  cpp_ctx* ctx = f->ctx;
  // the network whose trunk sees the state; shared: the value network's stack (the representation), then mu's on top of it
  cpp_net* stacks[2] = {f->share ? f->value : f->mu, f->mu};
  RC(infer_host_batch(stacks[0], stacks, f->share ? 2 : 1, false, state, dtype, B, nullptr, f->A));
  HIP_CHECK(hipMemcpyAsync(out, f->mu->ws[0].out, (size_t)B * f->A * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
  HIP_CHECK(ctx_sync_stream(ctx));
  return CPP_OK;
}

extern "C" int cpp_naf_compute_gradients(cpp_naf* f, cpp_batch* b) {
  RC(naf_check_batch(f, b, "cpp_naf_compute_gradients"));
  HIP_CHECK(hipSetDevice(f->ctx->device));
  PassLeft left;      // (nothing folded, nothing counted: cpp_naf_apply_gradients needs none of it)
  return naf_compute_gradients(f, b, &left);
}
extern "C" int cpp_naf_grad_buffer(cpp_naf* f, void** p, int64_t* n) {
  ARG_CHECK(f && p && n, "cpp_naf_grad_buffer: NULL argument");
  *p = f->gradbuf; *n = f->nV + f->nM + f->nL;
  return CPP_OK;
}
extern "C" int cpp_naf_apply_gradients(cpp_naf* f, float grad_scale) {
  ARG_CHECK(f, "cpp_naf_apply_gradients: NULL argument");
  HIP_CHECK(hipSetDevice(f->ctx->device));
  OptPlan plan; plan.grad_scale = grad_scale;
  return naf_apply(f, plan);
}
// publish_route: the launch closes a training call -- it also publishes the call's largest whitening scale and resets the scale word
static int naf_soft_update_target(cpp_naf* f, bool publish_route) {
  HIP_CHECK(hipSetDevice(f->ctx->device));
  f->tvalue->wimg_key = nullptr;
  return launch_soft_update(f->ctx, f->tvalue->params, f->value->params, f->nV, nullptr, nullptr, 0, f->hp.target_update_rate, publish_route);
}
extern "C" int cpp_naf_update_targets(cpp_naf* f) {
  ARG_CHECK(f, "cpp_naf_update_targets: NULL argument");
  return naf_soft_update_target(f, false);
}

extern "C" int cpp_naf_train(cpp_naf* f, cpp_batch* b, float* loss) {
  RC(naf_check_batch(f, b, "cpp_naf_train"));
  cpp_ctx* ctx = f->ctx;
  HIP_CHECK(hipSetDevice(ctx->device));
  HIP_CHECK(hipMemsetAsync(f->nonfinite, 0, sizeof(int), ctx->stream));
  OptPlan plan;
  RC(naf_compute_gradients(f, b, &plan.pass));
  int bad = 0; float l = 0.f;
  RC(read_back(ctx, {{&bad, f->nonfinite, sizeof(int)}, {&l, f->stats, sizeof(float)}}, true));
  if (loss) *loss = l;
  if (bad) { cpp_set_error("check_numerics: l_values / L / loss is not finite (naf_cartpole.py:242-245)"); return CPP_ERR_NUMERIC; }
  return naf_apply(f, plan);
}

extern "C" int cpp_naf_debug_values(cpp_naf* f, cpp_batch* b, float* l_values, float* loss, float* value, float* advantage,
                                    float* target_value) {
  RC(naf_check_batch(f, b, "cpp_naf_debug_values"));
  cpp_ctx* ctx = f->ctx;
  HIP_CHECK(hipSetDevice(ctx->device));
  const int B = b->B, C = f->value->spec.pixel ? f->value->spec.C : 0;
  for (cpp_net* n : {f->value, f->tvalue, f->mu, f->lv}) n->is_training = false;      // IS_TRAINING: False (naf_cartpole.py:282)
  const int frc = naf_forward(f, b->s[0], b->s[1], b->dtype, white_of(b, 0, C), white_of(b, 1, C), B);
  for (cpp_net* n : {f->value, f->tvalue, f->mu, f->lv}) n->is_training = true;
  if (frc) return frc;
  RC(naf_head(f, b, false));
  const size_t nB = (size_t)B * sizeof(float);
  return read_back(ctx, {{l_values, f->lv->ws[0].out, nB * f->NL}, {loss, f->stats, sizeof(float)}, {value, f->value->ws[0].out, nB},
                         {advantage, f->adv, nB}, {target_value, f->tvalue->ws[0].out, nB}});
}

static void naf_route_check(cpp_naf* f) { route_check(f->ctx, &f->epoch, &f->graph_gen, {f->value, f->tvalue, f->mu}); }

// The inner step naf_cartpole.py:367-373: the shared minibatch loop (rt_step.cpp: run_minibatches), then the target update.
// dp / comm: the gradient all-reduce sits between a minibatch's gradients and its update, inside the graph.
// Prioritized memory (per.hip; the data-parallel step refuses one): the draws advance the sampler's counter themselves, not the
// optimiser's launch: that launch stands down while the check_numerics flag is set (unless_nonfinite, as on the asynchronous rows path)
// and the priority writes with it (skip_if_set), the draws and the counter going on as before.
static int naf_step_body(cpp_naf* f, cpp_replay* r, int B, int n_batches, const int32_t* rows_dev, uint64_t seed, bool dp = false, cpp_comm* comm = nullptr) {
  cpp_ctx* ctx = f->ctx;
  const bool per = r->per_tree != nullptr;
  MinibatchLoop L;
  L.ctx = ctx; L.r = r; L.step_batch = f->step_batch; L.trunk = f->value;
  L.td = f->td; L.skip_if_set = f->nonfinite; L.draws_bump = true;
  L.ride_ok = !f->value->spec.use_batch_norm;
  L.gradients = [=](const PerPass& pp, PassLeft* left) { return naf_compute_gradients(f, f->step_batch, left, true, !per, pp); };
  bool targets_left = false;
  L.apply = [=, &targets_left](bool more, const NextBatch& next, const PassLeft& left) {
    if (dp) RC(step_allreduce(ctx, comm, f->gradbuf, (size_t)(f->nV + f->nM + f->nL)));
    static const bool no_tgt_ride = cpp_switch_off("CPP_RIDE_TARGETS");
    OptPlan plan;
    plan.grad_scale = (dp && comm) ? 1.0f / (float)comm->world : 1.0f; plan.unless_nonfinite = per;
    plan.bump = (rows_dev || per) ? nullptr : r->counter; plan.folded = !dp; plan.next = next; plan.pass = left;
    // (the last minibatch of an outer step: the target update and the publish ride in its optimiser launch -- unless that launch can stand down)
    plan.closes_step = plan.closes_call = !more && !dp && !no_tgt_ride && !per;
    return naf_apply(f, plan, &targets_left);
  };
  RC(run_minibatches(L, B, n_batches, rows_dev, seed));
  if (targets_left) return CPP_OK;      // (the target update and the route's publish left with the optimiser's launch)
  return naf_soft_update_target(f, true);      // (the largest whitening scale of this step rides to the host in that launch, for the next call's choice of conv1 kernels)
}

extern "C" int cpp_naf_train_step(cpp_naf* f, cpp_replay* r, int B, int n_batches, const int32_t* idxs, uint64_t seed) {
  if (f) naf_route_check(f);
  ARG_CHECK(f && r, "cpp_naf_train_step: NULL %s", r && r->per_tree ? "NAF learner for a prioritized memory" : "argument");
  RC(train_entry_checks("cpp_naf_train_step", r, B, f->maxB, f->value->state_elems, f->A, f->hp.discount, &n_batches));
  cpp_ctx* ctx = f->ctx;
  HIP_CHECK(hipSetDevice(ctx->device));
  if (!f->step_batch) RC(cpp_batch_create(ctx, f->maxB, r->elems, r->A, &f->step_batch));
  if (idxs) {
    RC(replay_upload_rows(r, idxs, n_batches * B, "cpp_naf_train_step"));
    return naf_step_body(f, r, B, n_batches, r->rows_in, seed);
  }
  return run_step_graph(ctx, f->graph, GraphKey{B, n_batches, seed, r->uid, 0, f->graph_gen}, [&] { return naf_step_body(f, r, B, n_batches, nullptr, seed); });
}

// naf_cartpole.py:367-371 for ONE minibatch whose rows the HOST drew: `batch = replay_memory.batch(B); loss = naf.train(batch)` without a
// gathered copy of the minibatch crossing PCIe or HBM twice -- the sample pass reads the replay store through those rows.  Like
// cpp_naf_train: gradients, then the loss and the check_numerics flag come back (one stream sync: the reference's train() returns the
// loss), then the optimiser -- which does not run when the flag is set.  The gradient half is one hipGraph per (B, replay).
// sticky: the check_numerics flag is NOT cleared (cpp_naf_train_rows_async: the host learns of a non-finite minibatch up to two calls
// later; until it has, every later optimiser launch must stand down as the first one did -- the reference's check_numerics stops
// training before any further train op, naf_cartpole.py:242-245,265)
// Prioritized memory: the importance weights of the caller's rows against the tree as it stands (the rows of cpp_replay_draw_prioritized
// get the weights that draw computed), and the priorities of the minibatch written behind its head kernel -- unless the check_numerics
// flag is set (sticky: as long as it stays set)
static int naf_rows_body(cpp_naf* f, cpp_replay* r, int B, PassLeft* left, bool fold = false, bool sticky = false) {
  const int C = f->value->spec.pixel ? f->value->spec.C : 0;
  if (!sticky) HIP_CHECK(hipMemsetAsync(f->nonfinite, 0, sizeof(int), f->ctx->stream));
  PerPass per;
  if (r->per_tree) {
    per.w = r->per_w;
    PerArgs p = per_args(r);
    p.B = B; p.w_rows = r->rows_in; p.out_w = r->per_w;
    RC(launch_per_update_sample(f->ctx, p));
    PerArgs u = per_args(r);
    u.up_rows = r->rows_in; u.n_up = B; u.up_td = f->td; u.skip_if_set = f->nonfinite;
    cpp_ctx* ctx = f->ctx;
    per.hook = [ctx, u] { return launch_per_update_sample(ctx, u); };
  }
  RC(replay_sample_device(r, B, r->rows_in, 0, nullptr, C, f->step_batch, direct_replay_ok(f->value, r, B)));
  RC(naf_compute_gradients(f, f->step_batch, left, fold, !sticky, per));
  return ctx_route_publish(f->ctx);
}
extern "C" int cpp_naf_train_rows(cpp_naf* f, cpp_replay* r, int B, const int32_t* idxs, float* loss) {
  if (f) naf_route_check(f);
  ARG_CHECK(f && r && idxs, "cpp_naf_train_rows: NULL %s", r && r->per_tree ? "argument (NAF learner or rows) for a prioritized memory" : "argument");
  RC(train_entry_checks("cpp_naf_train_rows", r, B, f->maxB, f->value->state_elems, f->A, f->hp.discount));
  cpp_ctx* ctx = f->ctx;
  HIP_CHECK(hipSetDevice(ctx->device));
  if (!f->step_batch) RC(cpp_batch_create(ctx, f->maxB, r->elems, r->A, &f->step_batch));
  RC(replay_stage_rows(r, idxs, B, "cpp_naf_train_rows"));
  RC(run_step_graph(ctx, f->rgraph, GraphKey{B, 1, 0, r->uid, 0, f->graph_gen}, [&] { PassLeft left; return naf_rows_body(f, r, B, &left); }));      // (nothing folded, nothing counted)
  int bad = 0; float l = 0.f;
  RC(read_back(ctx, {{&bad, f->nonfinite, sizeof(int)}, {&l, f->stats, sizeof(float)}}, true));
  if (loss) *loss = l;
  if (bad) { cpp_set_error("check_numerics: l_values / L / loss is not finite (naf_cartpole.py:242-245)"); return CPP_ERR_NUMERIC; }
  return naf_apply(f, OptPlan());
}

// The same minibatch without the host in the loop: gradients AND the optimiser in one hipGraph -- the optimiser kernel itself stands
// down when the check_numerics flag is set -- and the (loss, flag) pair copied into a pinned slot behind it.  The call returns a
// ticket at once; cpp_naf_loss_wait(ticket) is the sync the reference's `loss = naf.train(batch)` implies, taken when somebody
// reads the loss (the agents only log its mean) -- so a loop of train calls keeps the GPU fed like cpp_naf_train_step does.
// At most CPP_NAF_TICKETS results are outstanding: a slot is reused CPP_NAF_TICKETS calls later.
static int naf_rows_apply_body(cpp_naf* f, cpp_replay* r, int B) {
  OptPlan plan; plan.unless_nonfinite = true; plan.folded = true;
  RC(naf_rows_body(f, r, B, &plan.pass, true, true));  // (gradients and optimiser in ONE captured body: the fold's partials go from one to the other)
  return naf_apply(f, plan);
}
extern "C" int cpp_naf_train_rows_async(cpp_naf* f, cpp_replay* r, int B, const int32_t* idxs, uint64_t* ticket) {
  if (f) naf_route_check(f);
  ARG_CHECK(f && r && idxs && ticket, "cpp_naf_train_rows_async: NULL %s", r && r->per_tree ? "argument for a prioritized memory" : "argument");
  RC(train_entry_checks("cpp_naf_train_rows_async", r, B, f->maxB, f->value->state_elems, f->A, f->hp.discount));
  cpp_ctx* ctx = f->ctx;
  HIP_CHECK(hipSetDevice(ctx->device));
  if (!f->step_batch) RC(cpp_batch_create(ctx, f->maxB, r->elems, r->A, &f->step_batch));
  if (!f->res_pin) {
    HIP_CHECK(hipHostMalloc((void**)&f->res_pin, CPP_NAF_TICKETS * 2 * sizeof(float), hipHostMallocDefault));
    for (hipEvent_t& e : f->res_ev) HIP_CHECK(hipEventCreateWithFlags(&e, hipEventDisableTiming));
  }
  RC(replay_stage_rows(r, idxs, B, "cpp_naf_train_rows_async"));
  RC(run_step_graph(ctx, f->agraph, GraphKey{B, 1, 0, r->uid, 0, f->graph_gen}, [&] { return naf_rows_apply_body(f, r, B); }));
  const uint64_t t = f->next_ticket++;
  float* slot = f->res_pin + (t % CPP_NAF_TICKETS) * 2;
  HIP_CHECK(hipMemcpyAsync(slot, f->stats, sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
  HIP_CHECK(hipMemcpyAsync(slot + 1, f->nonfinite, sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
  HIP_CHECK(hipEventRecord(f->res_ev[t % CPP_NAF_TICKETS], ctx->stream));
  *ticket = t;
  return CPP_OK;
}
extern "C" int cpp_naf_loss_wait(cpp_naf* f, uint64_t ticket, float* loss) {
  ARG_CHECK(f && f->res_pin, "cpp_naf_loss_wait: no asynchronous train call has been made");
  ARG_CHECK(ticket < f->next_ticket && ticket + CPP_NAF_TICKETS >= f->next_ticket, "cpp_naf_loss_wait: ticket %llu is not one of the last %d",
            (unsigned long long)ticket, CPP_NAF_TICKETS);
  HIP_CHECK(hipEventSynchronize(f->res_ev[ticket % CPP_NAF_TICKETS]));
  const float* slot = f->res_pin + (ticket % CPP_NAF_TICKETS) * 2;
  if (loss) *loss = slot[0];
  int bad; memcpy(&bad, slot + 1, sizeof(int));
  if (bad) { cpp_set_error("check_numerics: l_values / L / loss is not finite (naf_cartpole.py:242-245)"); return CPP_ERR_NUMERIC; }
  return CPP_OK;
}

// ---- data-parallel learners: the halves of one minibatch of naf_cartpole.py:367-371 -------------------------
static int naf_half_body(cpp_naf* f, cpp_replay* r, int B, uint64_t seed) {
  const int C = f->value->spec.pixel ? f->value->spec.C : 0;
  bool bumped = false;       // (the statistics kernel advances the sampler's counter when there is one: replay_sample_finish)
  RC(replay_sample_device(r, B, nullptr, seed, r->counter, C, f->step_batch, direct_replay_ok(f->value, r, B), r->counter, &bumped));
  if (!bumped) RC(launch_counter_add(f->ctx, r->counter, 1));
  PassLeft left;      // (nothing folded, nothing counted)
  RC(naf_compute_gradients(f, f->step_batch, &left));
  return ctx_route_publish(f->ctx);
}

static int naf_half_checks(cpp_naf* f, cpp_replay* r, int B, const char* who) {
  ARG_CHECK(f && r, "%s: NULL argument", who);
  return train_entry_checks(who, r, B, f->maxB, f->value->state_elems, f->A, f->hp.discount, nullptr, false);
}

// sample B rows on the device (Philox; the counter advances by one) and leave the gradients of the three networks in the flat
// buffer [value | mu | l_values]; hipGraph-captured after the first call per (B, seed, replay)
extern "C" int cpp_naf_sample_and_compute(cpp_naf* f, cpp_replay* r, int B, uint64_t seed) {
  RC(per_refuse(r, "cpp_naf_sample_and_compute"));      // (the half step of the data-parallel learners: one tree per shard is not built)
  if (f) naf_route_check(f);
  RC(naf_half_checks(f, r, B, "cpp_naf_sample_and_compute"));
  RC(nstep_refuse(r, f->hp.discount, "cpp_naf_sample_and_compute"));
  cpp_ctx* ctx = f->ctx;
  HIP_CHECK(hipSetDevice(ctx->device));
  if (!f->step_batch) RC(cpp_batch_create(ctx, f->maxB, r->elems, r->A, &f->step_batch));
  return run_step_graph(ctx, f->hgraph, GraphKey{B, 1, seed, r->uid, 0, f->graph_gen}, [&] { return naf_half_body(f, r, B, seed); });
}

extern "C" int cpp_naf_allreduce_grads(cpp_naf* f, cpp_comm* c) {
  ARG_CHECK(f && c, "cpp_naf_allreduce_grads: NULL argument");
  ARG_CHECK(c->ctx == f->ctx, "cpp_naf_allreduce_grads: communicator and networks live on different contexts");
  HIP_CHECK(hipSetDevice(f->ctx->device));
  NCCL_CHECK(ncclAllReduce(f->gradbuf, f->gradbuf, (size_t)(f->nV + f->nM + f->nL), ncclFloat, ncclSum, c->comm, f->ctx->stream));
  return CPP_OK;
}

// periodic mode: parameters, the target and the optimiser slots (Momentum accumulators / Adam moments) of the replicas meet at
// their mean
extern "C" int cpp_naf_average_params(cpp_naf* f, cpp_comm* c) {
  ARG_CHECK(f && c, "cpp_naf_average_params: NULL argument");
  ARG_CHECK(c->ctx == f->ctx, "cpp_naf_average_params: communicator and networks live on different contexts");
  HIP_CHECK(hipSetDevice(f->ctx->device));
  const size_t nall = (size_t)(f->nV + f->nM + f->nL);
  cpp_net* nets[4] = {f->value, f->mu, f->lv, f->tvalue};
  NCCL_CHECK(ncclGroupStart());
  for (cpp_net* n : nets)
    NCCL_CHECK(ncclAllReduce(n->params, n->params, (size_t)n->nparams, ncclFloat, ncclAvg, c->comm, f->ctx->stream));
  if (f->hp.optimiser != CPP_OPT_SGD) NCCL_CHECK(ncclAllReduce(f->m, f->m, nall, ncclFloat, ncclAvg, c->comm, f->ctx->stream));
  if (f->hp.optimiser == CPP_OPT_ADAM) NCCL_CHECK(ncclAllReduce(f->v, f->v, nall, ncclFloat, ncclAvg, c->comm, f->ctx->stream));
  NCCL_CHECK(ncclGroupEnd());
  f->dp_local = 0;
  return CPP_OK;
}

// the inner step naf_cartpole.py:367-373 for N synchronous learners (this rank's part); see cpp_ddpg_dp_train_step
extern "C" int cpp_naf_dp_status(const cpp_naf* f, int* mode, char* reason, int cap) {      // (see cpp_ddpg_dp_status)
  ARG_CHECK(f && mode, "cpp_naf_dp_status: NULL argument");
  *mode = f->dgraph.mode(f->graph_gen);
  if (reason && cap > 0) snprintf(reason, (size_t)cap, "%s", f->dgraph.reason);
  return CPP_OK;
}

extern "C" int cpp_naf_dp_train_step(cpp_naf* f, cpp_replay* r, cpp_comm* c, int B, int n_batches, uint64_t seed, int sync_every) {
  RC(per_refuse(r, "cpp_naf_dp_train_step"));      // (one tree per shard: not built)
  if (f) naf_route_check(f);
  RC(naf_half_checks(f, r, B, "cpp_naf_dp_train_step"));
  RC(nstep_refuse(r, f->hp.discount, "cpp_naf_dp_train_step"));
  ARG_CHECK(n_batches >= 1 && sync_every >= 1, "cpp_naf_dp_train_step: n_batches %d, sync_every %d", n_batches, sync_every);
  ARG_CHECK(!c || c->ctx == f->ctx, "cpp_naf_dp_train_step: communicator and networks live on different contexts");
  const float inv = c ? 1.0f / (float)c->world : 1.0f;
  static const bool no_dp_graph = cpp_switch_off("CPP_DP_GRAPH");
  if (sync_every == 1 && !no_dp_graph) {             // ONE hipGraph per outer step, the all-reduce inside (see cpp_ddpg_dp_train_step)
    cpp_ctx* ctx = f->ctx;
    HIP_CHECK(hipSetDevice(ctx->device));
    if (!f->step_batch) RC(cpp_batch_create(ctx, f->maxB, r->elems, r->A, &f->step_batch));
    return run_dp_graph(ctx, f->dgraph, GraphKey{B, n_batches, seed, r->uid, c ? c->uid : 0, f->graph_gen}, "NAF",
                        [&] { return naf_step_body(f, r, B, n_batches, nullptr, seed, true, c); });
  }
  for (int i = 0; i < n_batches; ++i) {
    RC(cpp_naf_sample_and_compute(f, r, B, seed));
    if (sync_every > 1) {
      RC(naf_apply(f, OptPlan()));
      if (++f->dp_local >= (uint64_t)sync_every && c) RC(cpp_naf_average_params(f, c));
    } else {
      if (c) RC(cpp_naf_allreduce_grads(f, c));
      OptPlan plan; plan.grad_scale = inv;
      RC(naf_apply(f, plan));
    }
  }
  return cpp_naf_update_targets(f);
}

extern "C" int cpp_naf_last_stats(cpp_naf* f, float out[3]) {
  ARG_CHECK(f && out, "cpp_naf_last_stats: NULL argument");
  int bad = 0;
  RC(read_back(f->ctx, {{out, f->stats, 2 * sizeof(float)}, {&bad, f->nonfinite, sizeof(int)}}, true));
  out[2] = (float)bad;
  return CPP_OK;
}


// optimiser slots for checkpoints (util.py:88-90: tf.train.Saver saves the Momentum / Adam slot variables too)
extern "C" int64_t cpp_naf_opt_state_size(const cpp_naf* f) { return f ? (int64_t)(f->nV + f->nM + f->nL) : -1; }
extern "C" int cpp_naf_get_opt_state(cpp_naf* f, float* m, float* v, int64_t n, uint64_t* step) {
  ARG_CHECK(f, "cpp_naf_get_opt_state: NULL argument");
  ARG_CHECK(n == f->nV + f->nM + f->nL, "cpp_naf_get_opt_state: asked %ld values, the optimiser has %ld", (long)n, f->nV + f->nM + f->nL);
  HIP_CHECK(hipSetDevice(f->ctx->device));
  return read_back(f->ctx, {{m, f->m, (size_t)n * sizeof(float)}, {v, f->v, (size_t)n * sizeof(float)}, {step, f->opt_step, sizeof(uint64_t)}});
}
extern "C" int cpp_naf_set_opt_state(cpp_naf* f, const float* m, const float* v, int64_t n, uint64_t step) {
  ARG_CHECK(f, "cpp_naf_set_opt_state: NULL argument");
  ARG_CHECK(n == f->nV + f->nM + f->nL, "cpp_naf_set_opt_state: got %ld values, the optimiser has %ld", (long)n, f->nV + f->nM + f->nL);
  hipStream_t st = f->ctx->stream;
  HIP_CHECK(hipSetDevice(f->ctx->device));
  if (m) HIP_CHECK(hipMemcpyAsync(f->m, m, (size_t)n * sizeof(float), hipMemcpyHostToDevice, st));
  if (v) HIP_CHECK(hipMemcpyAsync(f->v, v, (size_t)n * sizeof(float), hipMemcpyHostToDevice, st));
  HIP_CHECK(hipMemcpyAsync(f->opt_step, &step, sizeof(uint64_t), hipMemcpyHostToDevice, st));
  // a restored checkpoint is a fresh start: the sticky check_numerics flag of cpp_naf_train_rows_async goes with the state it condemned
  HIP_CHECK(hipMemsetAsync(f->nonfinite, 0, sizeof(int), st));
  HIP_CHECK(hipStreamSynchronize(st));
  return CPP_OK;
}
// After CPP_ERR_NUMERIC on the asynchronous path every later update of this trainer stands down (the reference's check_numerics ends the
// run, naf_cartpole.py:242-245,265).  A caller that has repaired the parameters (cpp_net_set_params of a checkpoint) says so here.
extern "C" int cpp_naf_clear_numeric_error(cpp_naf* f) {
  ARG_CHECK(f, "cpp_naf_clear_numeric_error: NULL argument");
  HIP_CHECK(hipSetDevice(f->ctx->device));
  HIP_CHECK(hipMemsetAsync(f->nonfinite, 0, sizeof(int), f->ctx->stream));
  return CPP_OK;
}
