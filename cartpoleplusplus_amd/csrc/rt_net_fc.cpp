// networks, the fully connected stacks: GEMM descriptors (forward, dW, dX; head 2 of a twin critic), dropout, the eager forward of a
// stack, its backward chain as nodes of a gradient pass, the feature layer norm's job and nodes, the distributional / Gaussian heads
#include "rt_internal.h"

GemmArgs mk_gemm(const float* A, long sAm, long sAk, const float* Bm, long sBk, long sBn, float* C, long ldc,
                        int M, int N, int K, int epi, const float* Y, long ldy) {
  GemmArgs g; memset(&g, 0, sizeof(g));
  g.A = A; g.sAm = sAm; g.sAk = sAk; g.B = Bm; g.sBk = sBk; g.sBn = sBn; g.C = C; g.ldc = ldc;
  g.Y = Y; g.ldy = ldy; g.M = M; g.N = N; g.K = K; g.epi = epi;
  return g;
}
// --use-dropout: a training-mode forward draws its keep bits from (seed, layer, the network's forward count); inference
// mode is the plain ReLU.  The backward pass of such a layer doubles what it lets through (Y > 0 <=> kept and active).
void set_dropout(GemmArgs& g, cpp_net* n, int l) {
  if (g.epi != GE_RELU_DROPOUT) return;
  if (n->is_training && n->drop_counter) { g.drop_counter = n->drop_counter; g.drop_seed = n->spec.dropout_seed; g.drop_layer = (uint32_t)l; }
  else g.epi = GE_RELU;
}
int relu_grad_epi(const cpp_net* n, int producer_layer) {
  return (producer_layer >= 0 && n->fc[producer_layer].act == GE_RELU_DROPOUT) ? GE_MUL_RELU_GRAD_X2 : GE_MUL_RELU_GRAD;
}
int bump_dropout(cpp_net* n) {      // after every training-mode forward of the network's FC stack
  if (!n->drop_counter || !n->is_training) return CPP_OK;
  return launch_counter_add(n->ctx, n->drop_counter, 1);
}
// y = act([x, 1] [W; b]) of layer l into the next layer's input buffer (or w.out for the last layer)
GemmArgs fc_fwd_args(cpp_net* n, Workspace& w, int l, int B) {
  const FcL& L = n->fc[l];
  const int nfc = (int)n->fc.size();
  float* C = (l + 1 < nfc) ? w.fcin[l + 1] : fc_last_out(w);
  const long ldc = (l + 1 < nfc) ? n->fc[l + 1].n_in + 1 : L.n_out;
  GemmArgs g = mk_gemm(w.fcin[l], L.n_in + 1, 1, n->params + L.w_off, L.n_out, 1, C, ldc, B, L.n_out, L.n_in + 1, L.act);
  set_dropout(g, n, l);
  return g;
}
// [dW; db] = [x, 1]^T dz
GemmArgs fc_dw_args(cpp_net* n, Workspace& w, int l, int B, const float* dz) {
  const FcL& L = n->fc[l];
  return mk_gemm(w.fcin[l], 1, L.n_in + 1, dz, L.n_out, 1, n->grads + L.w_off, L.n_out, L.n_in + 1, L.n_out, B, GE_NONE);
}
// columns [col0, col0+ncols) of dz W^T, optionally times relu'(Y)
GemmArgs fc_dx_args(cpp_net* n, int l, int B, const float* dz, long dz_ld, int col0, int ncols, float* C, long ldc,
                           int epi, const float* Y, long ldy) {
  const FcL& L = n->fc[l];
  return mk_gemm(dz, dz_ld, 1, n->params + L.w_off + (long)col0 * L.n_out, 1, L.n_out, C, ldc, B, ncols, L.n_out, epi, Y, ldy);
}

// fully connected layers [from, end); `action` (device, (B, A)) is spliced in front of the cat layer
int net_forward_fc(cpp_net* n, Workspace& w, int from, int B, const float* action) {
  cpp_ctx* ctx = n->ctx;
  const int nfc = (int)n->fc.size(), A = n->spec.action_dim;
  for (int l = from; l < nfc; ++l) {
    const FcL& L = n->fc[l];
    if (L.cat) {
      if (!action) { cpp_set_error("critic forward needs an action batch"); return CPP_ERR_ARG; }
      RC(launch_copy_cols(ctx, w.fcin[l], L.n_in + 1, L.n_in - A, action, A, 0, A, B));
    }
    RC(launch_gemm(ctx, fc_fwd_args(n, w, l, B)));
    if (l == 0 && n->ln) RC(ln_forward(ctx, &n, 1, B));
  }
  return from == 0 ? bump_dropout(n) : CPP_OK;
}

// (rt_internal.h.  dW before dX per layer, top down: sq_gemm hands out the norm partials' slots in this order)
int add_fc_backward(OpGraph& G, cpp_net* n, Workspace& w, int B, int start, int dep, int list, int skip_dx) {
  for (int l = start; l >= (n->ln ? 1 : 0); --l) {      // (a feature layer norm: layer 0 is add_ln_backward's)
    const FcL& L = n->fc[l];
    G.gemm(sq_gemm(n->ctx, list, fc_dw_args(n, w, l, B, w.dz[l])), {dep});
    if (l == skip_dx) continue;
    if (l == 1 && n->ln)      // g = dL/dy of the normalised layer: ln.hip owns its activation's derivative
      dep = G.gemm(fc_dx_args(n, l, B, w.dz[l], L.n_out, 0, L.n_in, w.dz[0], L.n_in, GE_NONE, nullptr, 0), {dep});
    else if (l > 0)
      dep = G.gemm(fc_dx_args(n, l, B, w.dz[l], L.n_out, 0, L.n_in, w.dz[l - 1], L.n_in, relu_grad_epi(n, l - 1), w.fcin[l], L.n_in + 1), {dep});
    else if (has_conv(n))      // (an encoder-less actor: the stop gradient -- no dX of layer 0 is formed)
      dep = G.gemm(fc_dx_args(n, 0, B, w.dz[0], L.n_out, 0, n->flat, w.dpool[2], n->flat, GE_NONE, nullptr, 0), {dep});
  }
  return dep;
}

// ---- head 2 of a twin critic: layers [cat, nfc) of the first workspace
GemmArgs twin_fwd_args(cpp_net* n, Workspace& w, int l, int B) {
  const FcL& L = n->fc2[l];
  const int nfc = (int)n->fc2.size();
  float* C = (l + 1 < nfc) ? w.fcin2[l + 1] : twin_last_out(w);
  const long ldc = (l + 1 < nfc) ? n->fc2[l + 1].n_in + 1 : L.n_out;
  return mk_gemm(w.fcin2[l], L.n_in + 1, 1, n->params + L.w_off, L.n_out, 1, C, ldc, B, L.n_out, L.n_in + 1, L.act);
}
GemmArgs twin_dw_args(cpp_net* n, Workspace& w, int l, int B) {
  const FcL& L = n->fc2[l];
  return mk_gemm(w.fcin2[l], 1, L.n_in + 1, w.dz2[l], L.n_out, 1, n->grads + L.w_off, L.n_out, L.n_in + 1, L.n_out, B, GE_NONE);
}
// l > cat: dz2[l - 1] = (dz2[l] W2^T) relu'(fcin2[l]); l == cat (> 0): the shared layer's dz += dz2[cat] W2^T (state columns), then its mask
GemmArgs twin_dx_args(cpp_net* n, Workspace& w, int l, int B) {
  const FcL& L = n->fc2[l];
  if (l > n->cat_layer)
    return mk_gemm(w.dz2[l], L.n_out, 1, n->params + L.w_off, 1, L.n_out, w.dz2[l - 1], L.n_in, B, L.n_in, L.n_out, GE_MUL_RELU_GRAD, w.fcin2[l], L.n_in + 1);
  const int ncols = L.n_in - n->spec.action_dim;
  GemmArgs g = mk_gemm(w.dz2[l], L.n_out, 1, n->params + L.w_off, 1, L.n_out, w.dz[l - 1], ncols, B, ncols, L.n_out, relu_grad_epi(n, l - 1), w.fcin[l], L.n_in + 1);
  g.accumulate = 1;
  return g;
}
// the action columns of head 2's concat layer, added to head 1's in C (B x A), then the epilogue: dQ/da of an actor on the minimum head
GemmArgs twin_da_args(cpp_net* n, Workspace& w, int B, float* C, int epi, const float* Y, long ldy) {
  const int cat = n->cat_layer, A = n->spec.action_dim;
  const FcL& L = n->fc2[cat];
  GemmArgs g = mk_gemm(w.dz2[cat], L.n_out, 1, n->params + L.w_off + (long)(L.n_in - A) * L.n_out, 1, L.n_out, C, A, B, A, L.n_out, epi, Y, ldy);
  g.accumulate = 1;
  return g;
}

// ---- feature layer norm: the ln.hip job of a network's first workspace (backward pointers once a trainer has bound the gradient buffer)
static LnJob ln_job(cpp_net* n) {
  Workspace& w = n->ws[0];
  LnJob j; memset(&j, 0, sizeof(j));
  j.io = w.fcin[1]; j.ld = n->fc[1].n_in + 1; j.n = n->fc[0].n_out;
  j.gamma = n->params + n->ln_g_off; j.beta = n->params + n->ln_b_off; j.xhat = w.ln_xhat; j.rstd = w.ln_rstd;
  if (n->grads) { j.dz = w.dz[0]; j.dgamma = n->grads + n->ln_g_off; j.dbeta = n->grads + n->ln_b_off; }
  return j;
}
static LnArgs ln_args(cpp_net* const* nets, int nn, int B) {
  LnArgs a; memset(&a, 0, sizeof(a));
  a.count = nn; a.B = B; a.act = nets[0]->ln_act; a.eps = nets[0]->ln_eps;
  for (int k = 0; k < nn && k < LN_JOBS_MAX; ++k) a.j[k] = ln_job(nets[k]);
  return a;
}
int ln_forward(cpp_ctx* ctx, cpp_net* const* nets, int nn, int B) { return launch_ln_forward(ctx, ln_args(nets, nn, B)); }
int add_ln_forward(OpGraph& G, cpp_ctx* ctx, cpp_net* const* nets, int nn, const int* deps, int B) {
  const LnArgs a = ln_args(nets, nn, B);
  return G.fn([=] { return launch_ln_forward(ctx, a); }, {deps[0], nn > 1 ? deps[1] : -1, nn > 2 ? deps[2] : -1, nn > 3 ? deps[3] : -1});
}
void add_ln_backward(OpGraph& G, cpp_ctx* ctx, cpp_net* const* nets, int nn, int* deps, const int* lists, int B) {
  LnArgs a = ln_args(nets, nn, B);
  for (int k = 0; k < nn; ++k) a.j[k].sq_part = sq_take(ctx, lists[k], ln_col_blocks(a.j[k].n));
  const int cols = G.fn([=] { return launch_ln_backward_cols(ctx, a); }, {deps[0], nn > 1 ? deps[1] : -1});
  const int rows = G.fn([=] { return launch_ln_backward_rows(ctx, a); }, {cols});
  for (int k = 0; k < nn; ++k) {
    cpp_net* n = nets[k];
    Workspace& w = n->ws[0];
    const int dw = G.gemm(sq_gemm(ctx, lists[k], fc_dw_args(n, w, 0, B, w.dz[0])), {rows});
    if (!has_conv(n)) { deps[k] = dw; continue; }      // (an encoder-less actor: the stop gradient -- its backward ends at layer 0's dW)
    deps[k] = G.gemm(fc_dx_args(n, 0, B, w.dz[0], n->fc[0].n_out, 0, n->flat, w.dpool[2], n->flat, GE_NONE, nullptr, 0), {rows});
  }
}

// ---- the heads behind the last layer
int gauss_mean(cpp_net* n, Workspace& w, int B, float* m_out, float* ls_out) {
  if (!n->gauss) return CPP_OK;
  SacSampleArgs s; memset(&s, 0, sizeof(s));
  s.logits = w.logits; s.B = B; s.A = n->spec.action_dim; s.lo = n->ls_lo; s.hi = n->ls_hi;
  s.a_out = w.out; s.m_out = m_out; s.ls_out = ls_out;
  return launch_sac_sample(n->ctx, s);
}
int dist_expect(cpp_net* n, Workspace& w, int B, float* dz) {
  if (!n->dist_n) return CPP_OK;
  if (n->quant) return launch_quant_expect(n->ctx, w.logits, B, n->dist_n, w.out, dz);
  return launch_dist_expect(n->ctx, w.logits, B, n->dist_n, n->dist_vmin, n->dist_vmax, w.out, dz);
}
