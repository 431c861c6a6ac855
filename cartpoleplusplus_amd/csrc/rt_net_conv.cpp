// networks, the conv trunk: launch descriptors of the conv and batch-norm layers, the trunk's forward sequences (single, fused, batch norm),
// the conv backward sequences (single, multi, batch norm), the whitening statistics of a batch
#include "rt_internal.h"

// launch descriptors of conv layer i of a network (forward, dW, dX)
ConvArgs conv_fwd_args(cpp_net* n, Workspace& w, int i, const void* state, int dtype, const float* white, int B, int* mode,
                              long white_bstride) {
  const ConvL& L = n->conv[i];
  ConvArgs a; memset(&a, 0, sizeof(a));
  if (i == 0) { a.in = state; a.in_bstride = n->state_elems; a.scale = white; a.shift = white + n->spec.C; a.white_bstride = white_bstride;
                a.img_slot = n->img_slot; a.wimg = n->wimg; a.wimg_key = n->wimg_key;
                *mode = dtype == CPP_F16 ? IN_F16_WHITEN : IN_F32_WHITEN; }
  else { a.in = w.pool[i - 1]; a.in_bstride = (long)L.H * L.W * L.Cin; *mode = IN_F32_PLAIN; }
  a.w = n->params + L.w_off; a.bias = n->params + L.b_off;
  a.out = w.pool[i]; a.out_bstride = pool_rows(n, i).pool;
  a.out_amax = w.amax[i];
  a.B = B; a.H = L.H; a.W = L.W; a.nout = kConvOut;
  if (n->use_b16 && w.pool_b16) {
    const long plane = (long)n->maxB * n->conv[0].Hp * n->conv[0].Wp * kConvOut;      // halves per plane
    if (i == 0) { a.out_b16 = w.pool_b16; a.out_b16_plane = plane; }
    if (i == 1) { a.in_b16 = w.pool_b16; a.plane_stride = plane * 2; }
  }
  return a;
}
void conv_dy_desc(cpp_net* n, Workspace& w, int i, ConvArgs& a, int B) {
  const ConvL& L = n->conv[i];
  const PoolRows r = pool_rows(n, i);
  a.dy.dpool = w.dpool[i]; a.dy.pool = w.pool[i]; a.dy.amax = w.amax[i];
  a.dy.dpool_bstride = r.dpool;
  a.dy.pool_bstride = r.pool;
  a.dy.Hp = L.Hp; a.dy.Wp = L.Wp;
  a.B = B; a.H = L.H; a.W = L.W;
}
ConvArgs conv_dw_args(cpp_net* n, Workspace& w, int i, const void* state, int dtype, const float* white, int B, int* mode) {
  const ConvL& L = n->conv[i];
  ConvArgs d; memset(&d, 0, sizeof(d));
  conv_dy_desc(n, w, i, d, B);
  if (i == 0) { d.in = state; d.in_bstride = n->state_elems; d.scale = white; d.shift = white + n->spec.C; d.img_slot = n->img_slot;
                *mode = dtype == CPP_F16 ? IN_F16_WHITEN : IN_F32_WHITEN; }
  else { d.in = w.pool[i - 1]; d.in_bstride = (long)L.H * L.W * L.Cin; *mode = IN_F32_PLAIN; }
  d.nout = kConvOut; d.partial = n->dw_partial[i];
  // conv1's dW: the bound of |dpool[0]| per image that conv2's dX left (the same predicate as that launcher's: conv_dx_rs_dispatch)
  if (i == 0 && !n->spec.use_batch_norm && w.dpool_imax && (n->conv[1].W == 32 || n->conv[1].W == 64) &&
      conv_dx_rs_ok(n->ctx, kConvOut, n->conv[1].ks, n->conv[1].H, n->conv[1].W, kConvOut)) d.dy.imax = w.dpool_imax;
  return d;
}
ConvArgs conv_dx_args(cpp_net* n, Workspace& w, int i, int B) {
  const ConvL& L = n->conv[i];
  ConvArgs x; memset(&x, 0, sizeof(x));
  conv_dy_desc(n, w, i, x, B);
  x.w = n->params + L.w_off; x.nout = L.Cin;
  x.out = w.dpool[i - 1]; x.out_bstride = (long)L.H * L.W * L.Cin;
  if (i == 1 && !n->spec.use_batch_norm) x.dx_imax = w.dpool_imax;      // (conv2's dX on conv_dx_rs.h leaves the bound conv1's dW scales by)
  return x;
}

// slim.batch_norm's epsilon; the moving variance stays at its initial 1 (never updated by the reference's train ops)
static const double kBnEps = 1e-3;
// floats per image of layer i's plain conv output (w.z[i]: batch norm in training mode)
static long z_rows(const ConvL& L) { return (long)L.H * L.W * kConvOut; }

// descriptor of layer i of a batch-norm network for the bn.hip launches
BnNet bn_net_desc(cpp_net* n, Workspace& w, int i) {
  const ConvL& L = n->conv[i];
  const PoolRows r = pool_rows(n, i);
  BnNet d; memset(&d, 0, sizeof(d));
  d.z = w.z[i]; d.stat = w.bn_stat[i]; d.beta = n->params + L.b_off;
  d.pool = w.pool[i]; d.pool_bstride = r.pool; d.amax = w.amax[i];
  d.dpool = w.dpool[i]; d.dpool_bstride = r.dpool;
  d.part = n->bn_part; d.means = n->bn_means; d.dbeta = n->grads ? n->grads + L.b_off : nullptr;
  return d;
}
BnBatch bn_batch(cpp_net* const* nets, int nn, int i, int B, Workspace* w) {
  BnBatch bb; memset(&bb, 0, sizeof(bb));
  const ConvL& L = nets[0]->conv[i];
  bb.count = nn; bb.B = B; bb.H = L.H; bb.W = L.W; bb.C = kConvOut;
  for (int k = 0; k < nn; ++k) bb.n[k] = bn_net_desc(nets[k], w ? *w : nets[k]->ws[0], i);
  return bb;
}
// the batch-norm (training mode) form of a forward descriptor: the plain conv output, no bias, into z -- statistics, BN, ReLU and pool follow
static ConvArgs conv_plain_z(const ConvArgs& full, const ConvL& L, Workspace& w, int i) {
  ConvArgs p = full;
  p.out = w.z[i]; p.out_bstride = z_rows(L); p.out_amax = nullptr; p.bias = nullptr;
  return p;
}
// ... and of the backward's dX: the gradient w.r.t. the plain conv output is dense (bn.hip wrote it over z), a flipped plain conv
static ConvArgs conv_dx_dense_args(cpp_net* n, Workspace& w, int i, int B) {
  const ConvL& L = n->conv[i];
  ConvArgs x; memset(&x, 0, sizeof(x));
  x.in = w.z[i]; x.in_bstride = z_rows(L); x.w = n->params + L.w_off; x.nout = L.Cin;
  x.out = w.dpool[i - 1]; x.out_bstride = (long)L.H * L.W * L.Cin;
  x.B = B; x.H = L.H; x.W = L.W;
  return x;
}
// ... and of its dW: the same dense rows beside the pooled descriptor
static ConvArgs conv_dw_dense_args(cpp_net* n, Workspace& w, int i, const void* state, int dtype, const float* white, int B, int* mode) {
  ConvArgs d = conv_dw_args(n, w, i, state, dtype, white, B, mode);
  d.dy_dense = w.z[i]; d.dy_dense_bstride = z_rows(n->conv[i]);
  return d;
}

// conv trunk (pixel) or state conversion (low-dim) into ws.fcin[0]
// conv1 on the f16 pipes can leave bf16 planes of pool1 for a conv2 forward on the bf16 pipes (same launch sequence only)
bool trunk_b16(const cpp_net* n, int dtype, int B, long white_bstride) {
  return has_conv(n) && !n->spec.use_batch_norm && dtype == CPP_F16 && white_bstride == 0 &&
         conv12_b16_ok(n->ctx, n->conv[0].Cin, n->conv[0].H, n->conv[0].W, B);
}

int net_forward_trunk(cpp_net* n, Workspace& w, const void* state, int dtype, const float* white, int B,
                             long white_bstride) {
  cpp_ctx* ctx = n->ctx;
  n->use_b16 = trunk_b16(n, dtype, B, white_bstride);
  if (!n->spec.pixel)
    return launch_state_to_f32(ctx, w.fcin[0], n->fc[0].n_in + 1, state, dtype, n->state_elems, B);
  for (int i = 0; i < 3; ++i) {
    const ConvL& L = n->conv[i];
    int mode;
    ConvArgs a = conv_fwd_args(n, w, i, state, dtype, white, B, &mode, white_bstride);
    if (i == 0) n->wimg_key = nullptr;
    if (!n->spec.use_batch_norm) {
      RC(launch_conv_fwd(ctx, kFwdKid[i], L.Cin, L.ks, mode, EPI_RELU_POOL, a));
    } else if (!n->is_training) {
      // inference: (z - 0) / sqrt(1 + eps) + beta  ==  the fused kernel with scaled weights and beta as the bias
      a.wscale = (float)(1.0 / sqrt(1.0 + kBnEps));
      RC(launch_conv_fwd(ctx, kFwdKid[i], L.Cin, L.ks, mode, EPI_RELU_POOL, a));
    } else {                                            // plain conv output (no bias) -> statistics -> BN + ReLU + pool
      RC(launch_conv_fwd(ctx, kFwdKid[i], L.Cin, L.ks, mode, EPI_PLAIN, conv_plain_z(a, L, w, i)));
      RC(launch_bn_forward(ctx, bn_batch(&n, 1, i, B, &w), kBnEps));
    }
  }
  return CPP_OK;
}

// the same for several batch-norm networks in training mode, layer by layer: ONE plain-conv launch for all of them
// (the (ky,o) kernel needs the four networks of a minibatch to fill the chip), then statistics + BN/ReLU/pool per network
int nets_forward_trunk_bn(cpp_ctx* ctx, cpp_net* const* nets, int nn, const void* const* states, const float* const* whites,
                                 int dtype, int B) {
  for (int i = 0; i < 3; ++i) {
    const ConvL& L = nets[0]->conv[i];
    ConvArgs plain[CONV_BATCH_MAX]; int mode = 0;
    for (int k = 0; k < nn; ++k)
      plain[k] = conv_plain_z(conv_fwd_args(nets[k], nets[k]->ws[0], i, states[k], dtype, whites[k], B, &mode), L, nets[k]->ws[0], i);
    RC(launch_conv_fwd_multi(ctx, kFwdKid[i], L.Cin, L.ks, mode, EPI_PLAIN, plain, nn));
    RC(launch_bn_forward(ctx, bn_batch(nets, nn, i, B), kBnEps));
  }
  return CPP_OK;
}

// The conv trunks (no batch norm) of nn same-shaped networks, one launch per layer: networks [0, first_target) will run a backward
// pass, networks [first_target, nn) are forward-only (target networks: base_network.py:35-49).
//  * conv1 of all of them is ONE launch: 16 tiles per persistent workgroup amortise the weight preload and the tail (measured
//    0.560 -> 0.526 ms per step for DDPG's four networks);
//  * a forward-only network whose conv2 reads the bf16 planes of pool1 never reads pool1's f32 copy or its arg-max codes (26 MB of
//    writes per minibatch at 64x64x18): null outputs, which the kernel skips;
//  * conv2 (bf16 pipes, 32x32 inputs) carries conv3 + pool3 as its tail when the geometry allows (conv23_fuse_ok): one launch
//    less, and the forward-only networks' pool2 never leaves LDS.
int nets_forward_trunk_fused(cpp_ctx* ctx, cpp_net* const* nets, int nn, const void* const* sts, const float* const* whs, int first_target,
                             int dt, int B) {
  if (nn < 1 || nn > CONV_BATCH_MAX) { cpp_set_error("conv trunks: batch of %d networks", nn); return CPP_ERR_ARG; }
  cpp_net* a = nets[0];
  for (int k = 0; k < nn; ++k) nets[k]->use_b16 = trunk_b16(nets[k], dt, B, 0);
  {
    ConvArgs cl[CONV_BATCH_MAX]; int mode = 0;
    for (int k = 0; k < nn; ++k) cl[k] = conv_fwd_args(nets[k], nets[k]->ws[0], 0, sts[k], dt, whs[k], B, &mode);
    for (int k = first_target; k < nn; ++k)
      if (nets[k]->use_b16 && cl[k].out_b16) { cl[k].out = nullptr; cl[k].out_amax = nullptr; }
    for (int k = 0; k < nn; ++k) nets[k]->wimg_key = nullptr;      // (consumed -- or not used: either way the next forward builds its own)
    RC(launch_conv_fwd_multi(ctx, kFwdKid[0], a->conv[0].Cin, a->conv[0].ks, mode, EPI_RELU_POOL, cl, nn));
  }
  bool fuse23 = conv23_fuse_ok(a->conv[1].H, a->conv[1].W, B, kConvOut);
  for (int k = 0; k < nn; ++k) fuse23 = fuse23 && nets[k]->use_b16;
  for (int i = 1; i < 3; ++i) {
    if (i == 2 && fuse23) break;
    ConvArgs cl[CONV_BATCH_MAX]; int mode = 0;
    for (int k = 0; k < nn; ++k) {
      cl[k] = conv_fwd_args(nets[k], nets[k]->ws[0], i, sts[k], dt, whs[k], B, &mode);
      if (i == 1 && fuse23) {
        int m3 = 0;
        const ConvArgs c3 = conv_fwd_args(nets[k], nets[k]->ws[0], 2, sts[k], dt, whs[k], B, &m3);
        cl[k].n3_w = c3.w; cl[k].n3_bias = c3.bias; cl[k].n3_out = c3.out; cl[k].n3_out_bstride = c3.out_bstride; cl[k].n3_amax = c3.out_amax;
        if (k >= first_target) { cl[k].out = nullptr; cl[k].out_amax = nullptr; }      // pool2 only feeds conv3, which reads it from LDS
      }
    }
    RC(launch_conv_fwd_multi(ctx, kFwdKid[i], a->conv[i].Cin, a->conv[i].ks, mode, EPI_RELU_POOL, cl, nn));
  }
  return CPP_OK;
}

// conv trunk backward from w.dpool[2] (= d flat): dW/db of the three convs, dX for conv3/conv2
// batch norm (training mode): the gradient w.r.t. the plain conv output is dense -- reductions over the pooled tensors,
// dz written over z, then dW and dX from dense rows.  dbeta goes straight into the '<conv>/BatchNorm/beta' slot.
static int net_backward_conv_bn(cpp_net* n, Workspace& w, int B, const void* state, int dtype, const float* white) {
  cpp_ctx* ctx = n->ctx;
  for (int i = 2; i >= 0; --i) {
    const ConvL& L = n->conv[i];
    RC(launch_bn_backward(ctx, bn_batch(&n, 1, i, B, &w)));
    int mode;
    const ConvArgs d = conv_dw_dense_args(n, w, i, state, dtype, white, B, &mode);
    RC(launch_conv_dw(ctx, kDwKid[i], L.Cin, L.ks, mode, d, n->grads + L.w_off, n->bn_scratch));
    if (i > 0) RC(launch_conv_fwd(ctx, kDxKid[i], kConvOut, L.ks, IN_F32_FLIP, EPI_PLAIN, conv_dx_dense_args(n, w, i, B)));
  }
  return CPP_OK;
}

int net_backward_conv(cpp_net* n, Workspace& w, int B, const void* state, int dtype, const float* white) {
  cpp_ctx* ctx = n->ctx;
  if (n->spec.use_batch_norm) return net_backward_conv_bn(n, w, B, state, dtype, white);
  for (int i = 2; i >= 0; --i) {
    const ConvL& L = n->conv[i];
    int mode;
    ConvArgs d = conv_dw_args(n, w, i, state, dtype, white, B, &mode);
    RC(launch_conv_dw(ctx, kDwKid[i], L.Cin, L.ks, mode, d, n->grads + L.w_off, n->grads + L.b_off));
    if (i > 0)      // dX -> gradient w.r.t. the previous pooled output (conv1's input is data: no dX)
      RC(launch_conv_fwd(ctx, kDxKid[i], kConvOut, L.ks, IN_DY, EPI_PLAIN, conv_dx_args(n, w, i, B)));
  }
  return CPP_OK;
}

// the same for several networks with identical geometry, every layer's kernels batched into one launch
int nets_backward_conv(cpp_ctx* ctx, cpp_net* const* nets, int nn, int B, const void* state, int dtype, const float* white) {
  if (nets[0]->spec.use_batch_norm) {                 // dense dz per layer, then dW / dX of all networks in one launch each
    for (int i = 2; i >= 0; --i) {
      const ConvL& L = nets[0]->conv[i];
      RC(launch_bn_backward(ctx, bn_batch(nets, nn, i, B)));
      ConvArgs dl[CONV_BATCH_MAX], xl[CONV_BATCH_MAX]; float *gw[CONV_BATCH_MAX], *gb[CONV_BATCH_MAX];
      int mode = 0;
      for (int k = 0; k < nn; ++k) {
        cpp_net* n = nets[k];
        dl[k] = conv_dw_dense_args(n, n->ws[0], i, state, dtype, white, B, &mode);
        gw[k] = n->grads + L.w_off; gb[k] = n->bn_scratch;
        if (i > 0) xl[k] = conv_dx_dense_args(n, n->ws[0], i, B);
      }
      RC(launch_conv_dw_multi(ctx, kDwKid[i], L.Cin, L.ks, mode, dl, nn, gw, gb));
      if (i > 0) RC(launch_conv_fwd_multi(ctx, kDxKid[i], kConvOut, L.ks, IN_F32_FLIP, EPI_PLAIN, xl, nn));
    }
    return CPP_OK;
  }
  for (int i = 2; i >= 0; --i) {
    const ConvL& L = nets[0]->conv[i];
    ConvArgs dl[CONV_BATCH_MAX], xl[CONV_BATCH_MAX]; float *gw[CONV_BATCH_MAX], *gb[CONV_BATCH_MAX];
    int mode = 0;
    for (int k = 0; k < nn; ++k) {
      dl[k] = conv_dw_args(nets[k], nets[k]->ws[0], i, state, dtype, white, B, &mode);
      gw[k] = nets[k]->grads + L.w_off; gb[k] = nets[k]->grads + L.b_off;
      if (i > 0) xl[k] = conv_dx_args(nets[k], nets[k]->ws[0], i, B);
    }
    // a layer's dW and dX leave in one launch (conv3_bwd_pair.hip, conv2_bwd_pair.hip; CPP_CONV3_PAIR=0 / CPP_CONV2_PAIR=0: two)
    static const bool no_pair3 = cpp_switch_off("CPP_CONV3_PAIR");
    static const bool no_pair2 = cpp_switch_off("CPP_CONV2_PAIR");
    const bool no_pair = i == 2 ? no_pair3 : (i == 1 ? no_pair2 : true);
    ConvPairSlot slot; slot.have_dw = slot.have_dx = false; slot.dx_rs = slot.dw_rs = false; slot.layer = i;
    if (!no_pair) ctx->pair = &slot;
    int rc = launch_conv_dw_multi(ctx, kDwKid[i], L.Cin, L.ks, mode, dl, nn, gw, gb);
    if (!rc && i > 0) rc = launch_conv_fwd_multi(ctx, kDxKid[i], kConvOut, L.ks, IN_DY, EPI_PLAIN, xl, nn);
    ctx->pair = nullptr;
    RC(rc);
    if (!no_pair) RC(i == 2 ? launch_conv3_bwd_pair(ctx, slot) : launch_conv2_bwd_pair(ctx, slot));
  }
  return CPP_OK;
}

// the vector kernel's condition on a batch's shape (launch_gather_stats; else the generic kernel, one launch per table)
static bool stats_vec_ok(long elems, int C) {
  int g = 8, c = C; while (c) { int t = g % c; g = c; c = t; }     // gcd(8, C)
  return (elems % 8 == 0) && (C / g <= 16);
}
// whitening statistics of a device-resident (B, H*W*C) batch -> white[2][C]
int batch_stats(cpp_ctx* ctx, const void* s0, const void* s1, int dtype, long elems, int B, int C,
                       double* part, float* white) {
  const int nw = s1 ? 2 : 1;
  if (stats_vec_ok(elems, C)) {
    GatherArgs a; memset(&a, 0, sizeof(a));
    a.store[0] = s0; a.store[1] = s1 ? s1 : s0; a.part = part; a.elems = elems; a.B = B; a.C = C;
    RC(launch_gather_stats(ctx, a, dtype));     // grid (B,2): second column recomputes s0 when s1 == NULL (cheap, rare)
    RC(launch_stats_finalize(ctx, part, B, nw, C, (double)B * (double)(elems / C), white));
  } else {
    RC(launch_stats_generic(ctx, s0, dtype, (long)B * (elems / C), C, white));
    if (s1) RC(launch_stats_generic(ctx, s1, dtype, (long)B * (elems / C), C, white + 2 * C));
  }
  return CPP_OK;
}
// ... and of every image of it on its own -> white_rows[B][2][C], what B batches of one would compute (cpp_net_forward_each)
int batch_stats_each(cpp_ctx* ctx, const void* s, int dtype, long elems, int B, int C, double* part, float* white_rows) {
  const long npix = elems / C;
  if (stats_vec_ok(elems, C)) {       // per-row partial sums, finalised row by row
    GatherArgs ga; memset(&ga, 0, sizeof(ga));
    ga.store[0] = s; ga.store[1] = s; ga.part = part; ga.elems = elems; ga.B = B; ga.C = C;
    RC(launch_gather_stats(ctx, ga, dtype));
    RC(launch_stats_finalize(ctx, part, 1, B, C, (double)npix, white_rows));
  } else {
    const size_t esz = dtype == CPP_F16 ? 2 : 4;
    for (int b = 0; b < B; ++b)
      RC(launch_stats_generic(ctx, (const char*)s + (size_t)b * elems * esz, dtype, npix, C, white_rows + (long)b * 2 * C));
  }
  return CPP_OK;
}
