// DDPG's gradient pass (compute_gradients): one op graph per minibatch, built by named stages in a fixed order
#include "rt_ddpg.h"

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

// job (b) of dist.hip on the fed and the target evaluation the forward passes left in the first workspaces
static int dist_td(cpp_ddpg* d, const cpp_batch* b, int B, bool backward, const float* w) {
  cpp_net *c = d->critic, *tc = d->tcritic;
  if (d->pool) {      // both heads of both critics, one launch; the soft reward where critic_td reads it
    const int last = (int)c->fc.size() - 1;
    QpoolTdIo io;
    io.theta1 = c->ws[0].logits; io.theta2 = c->ws[0].logits2; io.ttheta1 = tc->ws[0].logits; io.ttheta2 = tc->ws[0].logits2;
    io.q1_out = c->ws[0].out; io.q2_out = c->ws[0].out2; io.tq1_out = tc->ws[0].out; io.tq2_out = tc->ws[0].out2;
    io.theta1_out = d->dist_p; io.theta2_out = d->pool_p2; io.sorted_out = d->dist_tp; io.y_out = d->dist_m; io.td = d->td; io.td2 = d->td2;
    io.dz1 = backward ? c->ws[0].dz[last] : nullptr; io.dz2 = backward ? c->ws[0].dz2[last] : nullptr;
    return launch_qpool_td(d->ctx, io, d->sac ? d->sac_rsoft : b->r, b->m, d->hp.discount, B, d->dist_n, d->quant_kappa, d->quant_drop, d->heads_part, w);
  }
  if (d->quant)
    return launch_quant_td(d->ctx, c->ws[0].logits, tc->ws[0].logits, b->r, b->m, d->hp.discount, B, d->dist_n, d->quant_kappa, d->quant_drop,
                           c->ws[0].out, tc->ws[0].out, d->dist_p, d->dist_tp, d->dist_m, d->td, backward ? c->ws[0].dz[c->fc.size() - 1] : nullptr,
                           d->heads_part, w);
  return launch_dist_td(d->ctx, c->ws[0].logits, tc->ws[0].logits, b->r, b->m, d->hp.discount, B, d->dist_n, c->dist_vmin, c->dist_vmax,
                        c->ws[0].out, tc->ws[0].out, d->dist_p, d->dist_tp, d->dist_m, d->td, backward ? c->ws[0].dz[c->fc.size() - 1] : nullptr,
                        d->heads_part, w);
}

static TpsArgs tps_args(const cpp_ddpg* d) {
  TpsArgs t; memset(&t, 0, sizeof(t));
  if (!d->tps_on) return t;
  t.n = (const unsigned long long*)d->tps_n; t.n_out = (unsigned long long*)(d->tps_n + 1); t.eps = d->tps_eps;
  t.sigma = d->tps_sigma; t.clip = d->tps_clip; t.seed_lo = (unsigned)d->tps_seed; t.seed_hi = (unsigned)(d->tps_seed >> 32);
  return t;
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

// One gradient pass: what compute_gradients is asked for and derives from it once, the op graph under construction, and the dependency
// ids the stages hand each other (-1: no such node in this pass).  The stages are the member functions below, in the order they run; the
// nodes' functions read the members through `this`, so a Pass outlives the run of its graph.
struct Pass {
  cpp_ddpg* d; cpp_batch* b; int phase; bool count_in_heads; const PerPass& per; PassParts want;
  const bool doA = want.actor, doC = want.critic, both = doA && doC, train = want.train;
  cpp_ctx* ctx = d->ctx;
  cpp_net *a = d->actor, *c = d->critic, *ta = d->tactor, *tc = d->tcritic;
  const int B = b->B, A = a->spec.action_dim, C = a->spec.pixel ? a->spec.C : 0, dt = b->dtype;
  const float *w1 = white_of(b, 0, C), *w2 = white_of(b, 1, C);
  const void *s1 = b->direct_store ? b->direct_store : b->s[0], *s2 = b->direct_store ? b->direct_store : b->s[1];
  const int na = (int)a->fc.size(), nc = (int)c->fc.size(), cat = c->cat_layer;
  const FcL& Lcat = c->fc[cat]; const long ldcat = Lcat.n_in + 1;
  const bool twin = d->twin, amin = d->amin;      // (amin: twin critics only, cpp_ddpg_set_actor_min_q)
  const bool pool = d->pool;                      // (pooled quantile critics: twin and dist at once; the actor ascends the mean of both heads)
  const bool two = amin || pool;                  // (both heads at mu(s1), two dX chains, head 2's action columns added to head 1's)
  const bool sac = d->sac;                        // (its actor's head is 2A wide and linear: never the fused heads)
  const int dist = d->dist_n;                     // (its q layer has N outputs: never the fused heads)
  const bool bc = d->bc_alpha > 0.f;              // (lambda needs every row of the minibatch: never the fused heads, whose rows are spread over workgroups)
  const bool shared = d->shared;                  // (the actors read the critics' conv features; only the critic's loss reaches a conv gradient)
  OpGraph G;
  int tA = -1, tC = -1, tTA = -1, tTC = -1;       // the four conv trunks (or the low-dimensional state's conversions)
  int aF = -1, taF = -1, cP = -1, tcP = -1;       // how far the actors' stacks and the critics' prefixes have come
  int l0 = 0;                                     // the first FC layer the GEMM levels run: 1 behind a feature layer norm
  bool fused = false; int pre = 0; DdpgHeadsArgs hd;      // the heads plan
  int c1 = -1, c1b = -1, c0 = -1, c0b = -1, tcH = -1, tcHb = -1;      // the q layers: critic(s1, mu(s1)), critic(s1, a), the target's; b: head 2
  int adz = -1, cdz = -1;                         // what completed d(flat) (a feature layer norm: dz[0]) of the actor, the critic

  void trunks(); void plan_heads(); void layer0_norm();                  // every pass
  void fused_branch();                                                   // the heads kernel and both backward chains, or ...
  void levels_forward(); void actor_objective(); void critic_objective();      // ... the GEMM levels, each half's where it is asked for
  int head_level(const GemmArgs& g, int l, int chain, int prefix, int splice, int extra = -1);
  int close(const SqScope& sq_scope, PassLeft* left);
};

// ---- forward: the four conv trunks.  conv1 saturates the chip per network; the narrow conv2 / conv3 layers
// of all four networks share one launch each.  (One half: its own networks, one by one -- batch norm follows each network's is_training.)
void Pass::trunks() {
  if (shared) {      // a shared encoder: the critics' trunks are the actors' -- one trained network and one target, as NAF's pair
    if (both) {
      cpp_net* nets[2] = {c, tc};
      const void* sts[2] = {s1, s2};
      const float* whs[2] = {w1, w2};
      tC = tTC = G.fn([=] { return nets_forward_trunk_fused(ctx, nets, 2, sts, whs, 1, dt, B); }, {});
    } else {      // one half: the critic's trunk on s1 either way, the target critic's on s2 for the critic's half
      tC = G.fn([=] { return net_forward_trunk(c, c->ws[0], s1, dt, w1, B); }, {});
      if (doC) tTC = G.fn([=] { return net_forward_trunk(tc, tc->ws[0], s2, dt, w2, B); }, {});
    }
    tA = tC; tTA = tTC;
  } else if (both && a->spec.pixel) {
    cpp_net* nets[4] = {a, c, ta, tc};
    const void* sts[4] = {s1, s1, s2, s2};
    const float* whs[4] = {w1, w1, w2, w2};
    // conv1 / conv2 (+ conv3 as conv2's tail) of the four networks in one launch per layer; the two target networks have no
    // backward pass (nets_forward_trunk_fused, rt_net_conv.cpp).  Batch norm: training mode for the whole graph (ddpg_cartpole.py:145,237)
    const bool bn = a->spec.use_batch_norm;
    tA = tC = tTA = tTC = G.fn([=] { return bn ? nets_forward_trunk_bn(ctx, nets, 4, sts, whs, dt, B)
                                               : nets_forward_trunk_fused(ctx, nets, 4, sts, whs, 2, dt, B); }, {});
  } else {      // the low-dimensional state's conversion; one half of a pixel pass: its own networks, each by its own is_training
    if (doA) tA = G.fn([=] { return net_forward_trunk(a, a->ws[0], s1, dt, w1, B); }, {});
    tC = G.fn([=] { return net_forward_trunk(c, c->ws[0], s1, dt, w1, B); }, {});
    if (doC) tTA = G.fn([=] { return net_forward_trunk(ta, ta->ws[0], s2, dt, w2, B); }, {});
    if (doC) tTC = G.fn([=] { return net_forward_trunk(tc, tc->ws[0], s2, dt, w2, B); }, {});
  }
  aF = tA; taF = tTA; cP = tC; tcP = tTC;
}

// ---- fused heads (heads.hip): when the critic is "[prefix, action] -> relu layer -> linear q" and the actor ends in a tanh
// layer (the reference's networks, ddpg_cartpole.py:95-100, :166-171), everything from the actors' / critics' last hidden
// activations to the first backward layer is one row-local kernel instead of five dependent GEMM levels + TD + copies.
// CPP_FUSED_HEADS=0 keeps the GEMM levels.  The plan creates no node: it decides `fused` and `pre` and fills the kernel's arguments --
// every reason a trainer never takes the heads kernel is read here.
void Pass::plan_heads() {
  static const bool no_heads = cpp_switch_off("CPP_FUSED_HEADS");
  memset(&hd, 0, sizeof(hd));
  fused = both && !dist && !bc && !sac && !no_heads && na >= 2 && cat >= 1 && nc - cat == 2 && a->fc[na - 1].act == GE_TANH && Lcat.act == GE_RELU &&
          c->fc[nc - 1].n_out == 1 && c->fc[nc - 1].act == GE_NONE && a->fc[na - 1].n_out == A;
  // feature layer norm: the heads kernel writes dz[na - 2] through that layer's ReLU mask -- never the normalised layer 0, whose
  // activation derivative is ln.hip's.  (The critic's is dz[cat - 1] = dz[1].)
  if (a->ln && na < 3) fused = false;
  if (!fused) return;
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
    if (amin) { hd.min_q1 = c->ws[1].out; hd.min_q2 = c->ws[1].out2; hd.min_sel = d->amin_sel; }
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
  pre = (fused && hd.n1a > 0) ? 1 : 0;
}

// ---- feature layer norm: layer 0 of every network this pass runs is one GEMM level, and ONE ln launch stands behind it; its output
// (the critic's: shared by both evaluations) is what layer 1 reads
void Pass::layer0_norm() {
  if (!a->ln) return;
  cpp_net* ln_nets[4]; int ln_deps[4]; int nn = 0;
  auto layer0 = [&](cpp_net* n, int dep) { ln_nets[nn] = n; ln_deps[nn++] = G.gemm(fc_fwd_args(n, n->ws[0], 0, B), {dep}); };
  if (doA) layer0(a, tA);
  layer0(c, tC);
  if (doC) { layer0(ta, tTA); layer0(tc, tTC); }
  aF = taF = cP = tcP = add_ln_forward(G, ctx, ln_nets, nn, ln_deps, B);
  l0 = 1;
}

// ---- the fused branch (both halves, training): the levels in front of the heads kernel, its launch, both backward chains behind it
void Pass::fused_branch() {
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
}

// One GEMM of the critics' head levels [cat, nc): it follows the level below in its own chain, or -- the concat layer -- the prefix, what
// wrote its splice columns and (the fed evaluation: the prefix node may be the second workspace's copy) the critic's trunk
int Pass::head_level(const GemmArgs& g, int l, int chain, int prefix, int splice, int extra) {
  return l == cat ? G.gemm(g, {prefix, splice, extra}) : G.gemm(g, {chain});
}

// ---- the GEMM levels' forward, each half's nodes only where one half is asked for: the actors, the critics' prefixes, the q layers
void Pass::levels_forward() {
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
  for (int l = cat; l < nc; ++l) {
    if (doA) c1 = head_level(fc_fwd_args(c, c->ws[1], l, B), l, c1, cP, aF);
    // the actor on the minimum head: head 2 at a = mu(s1) as well, in head 1's levels (with the actor's half alone too)
    if (doA && two) c1b = head_level(twin_fwd_args(c, c->ws[1], l, B), l, c1b, cP, aF);
    if (!doC) continue;
    c0 = head_level(fc_fwd_args(c, c->ws[0], l, B), l, c0, cP, cb, tC);
    tcH = head_level(fc_fwd_args(tc, tc->ws[0], l, B), l, tcH, tcP, taS);
    if (twin) {      // head 2 of both critics on the same concat inputs (one smoothed action for both target heads), in head 1's levels
      c0b = head_level(twin_fwd_args(c, c->ws[0], l, B), l, c0b, cP, cb, tC);
      tcHb = head_level(twin_fwd_args(tc, tc->ws[0], l, B), l, tcHb, tcP, taS);
    }
  }
}

// ---- the actor's objective on the GEMM levels: dQ/da at a = actor(s1), back through q_value .. splice on the second evaluation (dz of
// q is 1), the actor's head gradient, the actor's FC backward
void Pass::actor_objective() {
  int g = c1;
  // (a distributional critic: the gradient of the expectation, p (z - Q), stands where the scalar critic's q layer is fed ones)
  if (dist && !pool) g = G.fn([=] { return dist_expect(c, c->ws[1], B, c->ws[1].dz[nc - 1]); }, {c1});
  // (pooled quantile critics: Q_1, Q_2 and the tops of Qbar, 1 / (2N) in both q layers' dz of the second workspace -- quant_pool.hip)
  if (pool) g = G.fn([=] { return launch_qpool_expect(ctx, c->ws[1].logits, c->ws[1].logits2, B, dist, c->ws[1].out, c->ws[1].out2, c->ws[1].dz[nc - 1], c->ws[1].dz2[nc - 1]); }, {c1, c1b});
  // (the minimum head: per row 1 for the chosen head and 0 for the other, in the q layers' dz of the second workspace -- actor_min.hip)
  if (amin) g = G.fn([=] { return launch_actor_min(ctx, c->ws[1].out, c->ws[1].out2, B, c->ws[1].dz[nc - 1], c->ws[1].dz2[nc - 1], d->amin_sel); }, {c1, c1b});
  const float* top = (dist || amin) ? c->ws[1].dz[nc - 1] : d->ones;
  int g2 = g;      // head 2's chain down to the concat layer, beside head 1's
  for (int l = nc - 1; l > cat; --l) {
    const FcL& L = c->fc[l];
    const float* dz = (l == nc - 1) ? top : c->ws[1].dz[l];
    g = G.gemm(fc_dx_args(c, l, B, dz, L.n_out, 0, L.n_in, c->ws[1].dz[l - 1], L.n_in, GE_MUL_RELU_GRAD,
                          c->ws[1].fcin[l], L.n_in + 1), {g});
    if (two) g2 = G.gemm(twin_dx_args(c, c->ws[1], l, B), {g2});
  }
  // dQ/da (kept for cpp_ddpg_q_gradients_wrt_actions) and, in the same epilogue, the actor's head gradient
  const float* dz = (cat == nc - 1) ? top : c->ws[1].dz[cat];
  const bool plain_da = sac || bc;      // (the head gradient is a launch of its own behind this GEMM: sac.hip's job 3, bc.hip)
  const int epi = plain_da ? GE_NONE : GE_ACTOR_HEAD;
  const float* ay = plain_da ? nullptr : a->ws[0].out; const long lday = plain_da ? 0 : A;
  // the minimum head: (head 1's action columns) + (head 2's), then the epilogue -- a row's unselected head adds exact zeros
  const int h1 = two ? G.gemm(fc_dx_args(c, cat, B, dz, Lcat.n_out, Lcat.n_in - A, A, d->dq_da, A, GE_NONE, nullptr, 0), {g}) : -1;
  GemmArgs ga = two ? twin_da_args(c, c->ws[1], B, d->dq_da, epi, ay, lday)
                     : fc_dx_args(c, cat, B, dz, Lcat.n_out, Lcat.n_in - A, A, d->dq_da, A, epi, ay, lday);
  if (!plain_da) { ga.C2 = a->ws[0].dz[na - 1]; ga.ldc2 = A; }
  adz = two ? G.gemm(ga, {h1, g2, aF}) : G.gemm(ga, {g, aF});
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
  // ---- actor backward
  adz = add_fc_backward(G, a, a->ws[0], B, na - 1, adz, 0);
}

// ---- the critic's objective on the GEMM levels: TD target + critic backward on the first evaluation (fed actions)
void Pass::critic_objective() {
  cdz = G.fn([=] { return critic_td(d, b, B, train, per.w); }, {c0, tcH, c0b, tcHb});      // (twin: both heads of both critics; r_soft: job 2's, which tcH follows)
  if (per.hook) G.fn(per.hook, {cdz});
  int cdz2 = cdz;      // head 2's chain down to the concat layer, level by level beside head 1's
  for (int l = nc - 1; l >= (c->ln ? 1 : 0) && train; --l) {      // (a feature layer norm: layer 0 is add_ln_backward's)
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
}

// ---- closing: the feature layer norm's backward behind the GEMM levels, the conv backward, the run (by phase), what the pass left
int Pass::close(const SqScope& sq_scope, PassLeft* left) {
  if (a->ln && !fused) {      // the chains of the halves that ran a backward stopped at g = dL/dy of layer 0
    cpp_net* ln_nets[2]; int ln_deps[2], ln_lists[2], nn = 0;
    if (doA) { ln_nets[nn] = a; ln_deps[nn] = adz; ln_lists[nn++] = 0; }
    if (doC && train) { ln_nets[nn] = c; ln_deps[nn] = cdz; ln_lists[nn++] = 1; }
    if (nn) add_ln_backward(G, ctx, ln_nets, nn, ln_deps, ln_lists, B);
    nn = 0;
    if (doA) adz = ln_deps[nn++];
    if (doC && train) cdz = ln_deps[nn++];
  }
  int conv_bwd = -1;
  if (shared) {      // the encoder's backward is the critic's alone (the actor's chain ended at its layer-0 dW): three layers x one network
    if (doC && train) {
      cpp_net* bn[1] = {c};
      conv_bwd = G.fn([=] { return nets_backward_conv(ctx, bn, 1, B, s1, dt, w1); }, {adz, cdz});
    }
  } else if (c->spec.pixel && both) {     // both conv backward passes, layer by layer, two networks per launch
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
  else RC(flush_dw_reduce(ctx));      // all six dW reductions (3 layers x 2 networks; a shared encoder: 3 x 1) in one launch
  left->counted = fused && (hd.step_bump != nullptr || hd.pd != nullptr);
  left->noise_owed = (d->tps_on || sac) && phase != 2 && doC && train;      // (this pass read the count: exactly one increment follows it)
  sq_scope.left(left->sq_cnt);
  if (doC) left->loss = critic_loss_at(d, B, fused);
  if (sac && doA && train) left->loss.sac_rows = B;
  return CPP_OK;
}

// Both gradient sets of one minibatch (ddpg_cartpole.py:331-334) as one dependency graph: 4 conv trunk
// forwards, the MLP GEMMs batched level by level, 2 conv trunk backwards.  The critic trunk + the layers in
// front of the action splice run once for both uses of critic(s1, .).
// phase 0: everything.  The data-parallel step can split the pass at the conv backward: phase 1 = everything before it (all
// gradients of the fully connected layers are then final), phase 2 = the conv backward + the dW reductions.
// count_in_heads: the apply() behind this pass takes both lists (step_body) -- the heads kernel, where there is one, advances both step
// counts and the policy-delay words itself.  per: rt_internal.h, PerPass.  *left: what the pass left, written only when it succeeds.
// want: the parts of the pass (PassParts).  One half alone builds only its own nodes on the GEMM levels: per-network conv launches, no
// fused heads, no folded norms, nothing counted, no phase split.
int compute_gradients(cpp_ddpg* d, cpp_batch* b, PassLeft* left, int phase, bool count_in_heads, const PerPass& per, const PassParts& want) {
  if (!(want.actor && want.critic) && (phase != 0 || count_in_heads)) { cpp_set_error("compute_gradients: one half of the pass has no phases and counts nothing"); return CPP_ERR_STATE; }
  SlotScope slot_scope(b, {d->actor, d->critic}, {d->tactor, d->tcritic});      // (conv1 of the four networks addresses its images through the sampled slots while this graph runs)
  Pass p{d, b, phase, count_in_heads, per, want};
  // The kernels that write the gradients also leave their share of the two lists' squared norms (cpp_ctx::sq_part): list 0 = actor,
  // list 1 = critic.  Not with batch norm (dbeta comes out of the BN backward kernels) and not for a split pass.
  // (a shared encoder: the conv backward's only network is the critic's, list 1)
  SqScope sq_scope(p.ctx, 2, {d->shared ? 1 : 0, d->shared ? -1 : 1}, p.both && phase == 0 && !p.a->spec.use_batch_norm && !p.c->spec.use_batch_norm);
  p.trunks();
  p.plan_heads();
  p.layer0_norm();
  if (p.fused) p.fused_branch();
  else {
    p.levels_forward();
    if (p.doA) p.actor_objective();
    if (p.doC) p.critic_objective();
  }
  return p.close(sq_scope, left);
}
