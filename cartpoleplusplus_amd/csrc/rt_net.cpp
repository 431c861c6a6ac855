// networks: layout (TF variable order), workspaces, the variants' argument rules and the one constructor, the cpp_net_create_* /
// cpp_net_*_info entry points, the shared encoder's binding, parameters / gradients / soft update.  The launch sequences: rt_net_conv.cpp
// (conv trunk), rt_net_fc.cpp (fully connected stacks), rt_net_infer.cpp (inference on a host batch)
#include "rt_internal.h"

static int net_build(cpp_net* n) {
  const cpp_net_spec& s = n->spec;
  long off = 0;
  int h = s.H, w = s.W, cin = s.C;
  if (s.pixel && n->enc_less) {      // the features are the bound critic's: no conv variable, the same flat width
    for (int i = 0; i < 3; ++i) { h /= 2; w /= 2; }
    if (h < 1 || w < 1) { cpp_set_error("image %dx%d too small for three 2x2 pools", s.H, s.W); return CPP_ERR_ARG; }
    n->flat = h * w * kConvOut;
    n->state_elems = (long)s.H * s.W * s.C;
  } else if (s.pixel) {
    for (int i = 0; i < 3; ++i) {
      ConvL L; L.H = h; L.W = w; L.Cin = cin; L.ks = kConvKs[i]; L.Hp = h / 2; L.Wp = w / 2;
      L.w_off = off; off += (long)L.ks * L.ks * cin * kConvOut; L.b_off = off; off += kConvOut;
      n->conv.push_back(L);
      VarInfo vw; vw.name = std::string(kConvNames[i]) + "/weights"; vw.rank = 4;
      vw.shape[0] = L.ks; vw.shape[1] = L.ks; vw.shape[2] = cin; vw.shape[3] = kConvOut; vw.offset = L.w_off;
      VarInfo vb; vb.name = std::string(kConvNames[i]) + (s.use_batch_norm ? "/BatchNorm/beta" : "/biases"); vb.rank = 1;
      vb.shape[0] = kConvOut; vb.shape[1] = vb.shape[2] = vb.shape[3] = 0; vb.offset = L.b_off;
      n->vars.push_back(vw); n->vars.push_back(vb);
      cin = kConvOut; h /= 2; w /= 2;
    }
    if (h < 1 || w < 1) { cpp_set_error("image %dx%d too small for three 2x2 pools", s.H, s.W); return CPP_ERR_ARG; }
    n->flat = h * w * kConvOut;
    n->state_elems = (long)s.H * s.W * s.C;
  } else {
    n->flat = s.state_elems;
    n->state_elems = s.state_elems;
  }
  const int A = s.action_dim;
  auto add_fc = [&](const std::string& name, int n_in, int n_out, int act, int cat) {
    FcL L; L.n_in = n_in; L.n_out = n_out; L.act = act; L.cat = cat; L.w_off = off; L.name = name;
    off += (long)n_in * n_out + n_out;
    n->fc.push_back(L);
    VarInfo vw; vw.name = name + "/weights"; vw.rank = 2; vw.shape[0] = n_in; vw.shape[1] = n_out;
    vw.shape[2] = vw.shape[3] = 0; vw.offset = L.w_off;
    VarInfo vb; vb.name = name + "/biases"; vb.rank = 1; vb.shape[0] = n_out;
    vb.shape[1] = vb.shape[2] = vb.shape[3] = 0; vb.offset = L.w_off + (long)n_in * n_out;
    n->vars.push_back(vw); n->vars.push_back(vb);
  };
  n->cat_layer = -1;
  int n_in = n->flat;
  const int hid_act = s.use_dropout ? GE_RELU_DROPOUT : GE_RELU;       // hidden_layers_starting_at with opts (base_network.py:69-70)
  if (s.kind == CPP_ACTOR) {
    for (int i = 0; i < s.n_hidden; ++i) { add_fc("h" + std::to_string(i), n_in, s.hidden[i], hid_act, 0); n_in = s.hidden[i]; }
    add_fc("output_action", n_in, n->gauss ? 2 * A : A, n->gauss ? GE_NONE : GE_TANH, 0);      // ddpg_cartpole.py:95-100 (a Gaussian actor: (m | x))
  } else if (s.kind == CPP_HEAD) {                                      // naf_cartpole.py:104-109,156-161,180-184
    for (int i = 0; i < s.n_hidden; ++i) { add_fc("h" + std::to_string(i), n_in, s.hidden[i], hid_act, 0); n_in = s.hidden[i]; }
    add_fc("fc", n_in, s.head_out, s.head_act == 2 ? GE_TANH : GE_NONE, 0);
  } else if (s.pixel) {                                                 // ddpg_cartpole.py:168-171 (intent)
    add_fc("hidden1", n_in, 200, GE_RELU, 0);
    add_fc("hidden2", 200, 50, GE_RELU, 0);
    add_fc("hidden3", 50 + A, 50, GE_RELU, 1); n->cat_layer = 2;
    add_fc("q_value", 50, n->dist_n ? n->dist_n : 1, GE_NONE, 0);      // (a distributional critic: N logits)
  } else {                                                              // ddpg_cartpole.py:174-177
    n_in += A;
    for (int i = 0; i < s.n_hidden; ++i) { add_fc("h" + std::to_string(i), n_in, s.hidden[i], GE_RELU, i == 0); n_in = s.hidden[i]; }
    n->cat_layer = 0;
    add_fc("q_value", n_in, n->dist_n ? n->dist_n : 1, GE_NONE, 0);
  }
  // twin Q heads: a second copy of the layers from the concat layer upward, behind the plain critic's variables (whose names, shapes
  // and offsets stay what they are): 'hidden3b', 'q_valueb' (pixel), 'h<i>b', 'q_valueb' (low-dimensional: the whole stack)
  if (n->twin) {
    const std::vector<FcL> head1 = n->fc;
    n->fc2 = head1;
    for (int l = n->cat_layer; l < (int)head1.size(); ++l) {
      const FcL L = head1[l];
      add_fc(L.name + "b", L.n_in, L.n_out, L.act, L.cat);
      n->fc2[l] = n->fc.back();
      n->fc.pop_back();
    }
  }
  // feature layer norm: layer 0 is a plain GEMM, its activation is ln.hip's; gamma and beta behind every other variable, twin ones
  // included -- the plain prefix of the flat buffer keeps its names, shapes and offsets
  if (n->ln) {
    n->fc[0].act = GE_NONE;
    const int width = n->fc[0].n_out;
    for (int k = 0; k < 2; ++k) {
      VarInfo v; v.name = n->fc[0].name + (k == 0 ? "/LayerNorm/gamma" : "/LayerNorm/beta"); v.rank = 1;
      v.shape[0] = width; v.shape[1] = v.shape[2] = v.shape[3] = 0; v.offset = off;
      (k == 0 ? n->ln_g_off : n->ln_b_off) = off;
      off += width;
      n->vars.push_back(v);
    }
  }
  n->nparams = off;
  return CPP_OK;
}

static int ws_alloc(cpp_net* n, Workspace& w, int from_layer, bool trunk) {
  const int mb = n->maxB;
  const int nfc = (int)n->fc.size();
  w.fcin.assign(nfc, nullptr);
  w.dz.assign(nfc, nullptr);
  for (int l = from_layer; l < nfc; ++l) {
    const FcL& L = n->fc[l];
    if (!(l == 0 && n->enc_less)) {      // (an encoder-less actor: cpp_net_set_encoder aliases the critic's buffer, ones column included)
      RC(dalloc(n->arena, &w.fcin[l], (size_t)mb * (L.n_in + 1)));
      RC(launch_fill(n->ctx, w.fcin[l], L.n_in + 1, L.n_in, 1, mb, 1.0f));   // the bias "ones" column
    }
    RC(dalloc(n->arena, &w.dz[l], (size_t)mb * L.n_out));
  }
  if (n->dist_n) {      // distributional critic: the logits beside a Q of width one
    RC(dalloc(n->arena, &w.logits, (size_t)mb * n->dist_n));
    RC(dalloc(n->arena, &w.out, (size_t)mb));
  } else if (n->gauss) {      // Gaussian actor: the 2A-wide head beside an action of width A
    RC(dalloc(n->arena, &w.logits, (size_t)mb * n->fc.back().n_out));
    RC(dalloc(n->arena, &w.out, (size_t)mb * n->spec.action_dim));
  } else
  RC(dalloc(n->arena, &w.out, (size_t)mb * n->fc.back().n_out));
  if (n->twin) {      // (head 2 on the fed action: the first workspace; at a = mu(s1), for an actor on the minimum head: the second)
    w.fcin2.assign(nfc, nullptr);
    w.dz2.assign(nfc, nullptr);
    for (int l = n->cat_layer; l < nfc; ++l) {
      const FcL& L = n->fc2[l];
      if (l == n->cat_layer) w.fcin2[l] = w.fcin[l];
      else {
        RC(dalloc(n->arena, &w.fcin2[l], (size_t)mb * (L.n_in + 1)));
        RC(launch_fill(n->ctx, w.fcin2[l], L.n_in + 1, L.n_in, 1, mb, 1.0f));
      }
      RC(dalloc(n->arena, &w.dz2[l], (size_t)mb * L.n_out));
    }
    if (n->dist_n) {      // pooled twin quantile critics: head 2's atoms beside a Q_2 of width one
      RC(dalloc(n->arena, &w.logits2, (size_t)mb * n->dist_n));
      RC(dalloc(n->arena, &w.out2, (size_t)mb));
    } else
    RC(dalloc(n->arena, &w.out2, (size_t)mb * n->fc2.back().n_out));
  }
  if (trunk && n->ln) {
    RC(dalloc(n->arena, &w.ln_xhat, (size_t)mb * n->fc[0].n_out));
    RC(dalloc(n->arena, &w.ln_rstd, (size_t)mb));
  }
  if (trunk && has_conv(n)) {
    for (int i = 0; i < 3; ++i) {
      const ConvL& L = n->conv[i];
      const size_t pe = (size_t)mb * L.Hp * L.Wp * kConvOut;
      if (i < 2) RC(dalloc(n->arena, &w.pool[i], pe)); else w.pool[i] = w.fcin[0];
      if (i == 0 && !n->spec.use_batch_norm) RC(dalloc(n->arena, &w.pool_b16, 3 * pe));
      RC(dalloc(n->arena, &w.amax[i], pe));
      RC(dalloc(n->arena, &w.dpool[i], pe));
      if (i == 0) RC(dalloc(n->arena, &w.dpool_imax, (size_t)mb * DX_IMAX_SLOTS));
      if (n->spec.use_batch_norm) {
        RC(dalloc(n->arena, &w.z[i], (size_t)mb * L.H * L.W * kConvOut));
        RC(dalloc(n->arena, &w.bn_stat[i], (size_t)2 * kConvOut));
      }
    }
  }
  return CPP_OK;
}

// the variants' own argument rules, shared by their constructors and cpp_net_create_feature_norm (who: the entry point's name)
static int check_twin(const char* who, const cpp_net_spec* spec) {
  ARG_CHECK(spec->kind == CPP_CRITIC, "%s: kind %d (twin Q heads belong to a critic)", who, spec->kind);
  return CPP_OK;
}
static int check_distributional(const char* who, const cpp_net_spec* spec, int n_atoms, float v_min, float v_max) {
  ARG_CHECK(spec->kind == CPP_CRITIC, "%s: kind %d (a value distribution belongs to a critic)", who, spec->kind);
  ARG_CHECK(n_atoms >= 2 && n_atoms <= 64, "%s: %d atoms outside [2, 64]", who, n_atoms);
  ARG_CHECK(std::isfinite(v_min) && std::isfinite(v_max) && v_min < v_max, "%s: support [%g, %g] (finite, v_min < v_max)", who, (double)v_min, (double)v_max);
  return CPP_OK;
}
static int check_quantile(const char* who, const cpp_net_spec* spec, int n_quantiles) {
  ARG_CHECK(spec->kind == CPP_CRITIC, "%s: kind %d (quantiles belong to a critic)", who, spec->kind);
  ARG_CHECK(n_quantiles >= 2 && n_quantiles <= 64, "%s: %d quantiles outside [2, 64]", who, n_quantiles);
  return CPP_OK;
}
static int check_pooled_quantile(const char* who, const cpp_net_spec* spec, int n_quantiles) {
  ARG_CHECK(spec->kind == CPP_CRITIC, "%s: kind %d (quantiles belong to a critic)", who, spec->kind);
  ARG_CHECK(n_quantiles >= 2 && n_quantiles <= 32, "%s: %d quantiles per head outside [2, 32] (the pool of both heads fills one wave's 64 lanes)", who, n_quantiles);
  return CPP_OK;
}
static int check_gaussian(const char* who, const cpp_net_spec* spec, float log_std_min, float log_std_max) {
  ARG_CHECK(spec->kind == CPP_ACTOR, "%s: kind %d (a Gaussian policy belongs to an actor)", who, spec->kind);
  ARG_CHECK(std::isfinite(log_std_min) && std::isfinite(log_std_max) && log_std_min < log_std_max, "%s: log std bounds [%g, %g] (finite, min < max)", who,
            (double)log_std_min, (double)log_std_max);
  ARG_CHECK(spec->action_dim >= 1 && spec->action_dim <= 64, "%s: action_dim %d outside [1, 64]", who, spec->action_dim);
  return CPP_OK;
}
// the one constructor: the spec's layout as the variant record `v` (rt_internal.h) widens it; the entry points below check their own
// arguments, fill a record by field name and end here
static int net_create(cpp_ctx* ctx, const cpp_net_spec* spec, int max_batch, const NetVariant& v, cpp_net** out) {
  ARG_CHECK(ctx && spec && out, "cpp_net_create: NULL argument");
  ARG_CHECK(max_batch >= 1, "cpp_net_create: max_batch %d", max_batch);
  ARG_CHECK(spec->kind == CPP_ACTOR || spec->kind == CPP_CRITIC || spec->kind == CPP_HEAD, "cpp_net_create: kind %d", spec->kind);
  if (spec->kind == CPP_HEAD) ARG_CHECK(spec->head_out >= 1 && spec->head_out <= 64 && (spec->head_act == 0 || spec->head_act == 2),
                                        "cpp_net_create: head_out %d head_act %d", spec->head_out, spec->head_act);
  // (a head network's action_dim is its output width -- NAF's l_values head has A (A + 1) / 2 outputs, up to 36 -- and shapes nothing)
  if (spec->kind != CPP_HEAD && !v.gauss)      // (cpp_net_create_gaussian has checked its own range)
    ARG_CHECK(spec->action_dim >= 1 && spec->action_dim <= 16, "cpp_net_create: action_dim %d outside [1, 16]", spec->action_dim);
  else if (spec->kind == CPP_HEAD) ARG_CHECK(spec->action_dim >= 1, "cpp_net_create: action_dim %d", spec->action_dim);
  ARG_CHECK(spec->n_hidden >= 0 && spec->n_hidden <= 8, "cpp_net_create: n_hidden %d outside [0, 8]", spec->n_hidden);
  for (int i = 0; i < spec->n_hidden; ++i)
    ARG_CHECK(spec->hidden[i] >= 1, "cpp_net_create: hidden layer %d has width %d (at least 1)", i, spec->hidden[i]);
  if (spec->pixel) ARG_CHECK(spec->H >= 8 && spec->W >= 8 && spec->C >= 1 && spec->C <= CPP_MAX_CHANNELS,
                             "cpp_net_create: pixel dims %dx%dx%d", spec->H, spec->W, spec->C);
  else ARG_CHECK(spec->state_elems >= 1, "cpp_net_create: state_elems %d", spec->state_elems);
  if (spec->kind == CPP_ACTOR || (spec->kind == CPP_CRITIC && !spec->pixel)) ARG_CHECK(spec->n_hidden >= 1, "cpp_net_create: need hidden layers");
  HIP_CHECK(hipSetDevice(ctx->device));
  cpp_net* n = new cpp_net();
  n->ctx = ctx; n->spec = *spec; n->maxB = max_batch; n->arena.stream = ctx->stream;
  n->grads = nullptr; n->own_grads = nullptr; n->stage_state = nullptr; n->stage_action = nullptr;
  n->stage_out = nullptr; n->dw_partial[0] = n->dw_partial[1] = n->dw_partial[2] = nullptr; n->white = nullptr; n->white_rows = nullptr; n->stats_part = nullptr;
  n->img_slot = nullptr; n->use_b16 = false; n->wimg = nullptr; n->wimg_key = nullptr;
  n->is_training = true; n->drop_counter = nullptr; n->bn_part = nullptr; n->bn_means = nullptr; n->bn_scratch = nullptr;
  n->twin = v.twin;
  n->dist_n = v.dist_n; n->dist_vmin = v.v_min; n->dist_vmax = v.v_max; n->quant = v.quant;
  n->gauss = v.gauss; n->ls_lo = v.ls_lo; n->ls_hi = v.ls_hi;
  n->ln = v.ln_act != 0; n->ln_act = v.ln_act ? v.ln_act : GE_TANH; n->ln_eps = v.ln_eps;
  n->enc_less = v.enc_less;
  int rc = net_build(n);
  if (rc) { delete n; return rc; }
  auto fail = [&](int r) { n->arena.release(); delete n; return r; };
  if ((rc = dalloc(n->arena, &n->params, (size_t)n->nparams))) return fail(rc);
  if (spec->use_dropout && (rc = n->arena.alloc((void**)&n->drop_counter, sizeof(uint64_t), true))) return fail(rc);
  if ((rc = ws_alloc(n, n->ws[0], 0, true))) return fail(rc);
  if (n->ln && (rc = launch_fill(ctx, n->params + n->ln_g_off, 1, 0, 1, n->fc[0].n_out, 1.0f))) return fail(rc);      // (gamma = 1, beta = 0)
  if (spec->kind == CPP_CRITIC) {
    n->ws[1] = n->ws[0];
    if ((rc = ws_alloc(n, n->ws[1], n->cat_layer, false))) return fail(rc);
    for (int l = 0; l < n->cat_layer; ++l) { n->ws[1].fcin[l] = n->ws[0].fcin[l]; n->ws[1].dz[l] = n->ws[0].dz[l]; }
    for (int i = 0; i < 3; ++i) { n->ws[1].pool[i] = n->ws[0].pool[i]; n->ws[1].amax[i] = n->ws[0].amax[i]; n->ws[1].dpool[i] = n->ws[0].dpool[i]; n->ws[1].dpool_imax = n->ws[0].dpool_imax;
                                  n->ws[1].z[i] = n->ws[0].z[i]; n->ws[1].bn_stat[i] = n->ws[0].bn_stat[i]; }
  }
  if (has_conv(n)) {
    for (int i = 0; i < 3; ++i)
      if ((rc = dalloc(n->arena, &n->dw_partial[i], conv_dw_partial_floats(ctx, n->conv[i].Cin, n->conv[i].ks, kConvOut)))) return fail(rc);
    if ((rc = n->arena.alloc(&n->wimg, conv_rs16_image_bytes(), true))) return fail(rc);
    if ((rc = dalloc(n->arena, &n->white, (size_t)2 * spec->C))) return fail(rc);
    if ((rc = dalloc(n->arena, &n->white_rows, (size_t)max_batch * 2 * spec->C))) return fail(rc);
    if ((rc = dalloc(n->arena, &n->stats_part, (size_t)2 * max_batch * 2 * spec->C))) return fail(rc);
    if (spec->use_batch_norm) {
      size_t pd = (size_t)2 * max_batch * 2 * kConvOut;
      if (pd < bn_part_doubles(kConvOut)) pd = bn_part_doubles(kConvOut);
      if ((rc = n->arena.alloc((void**)&n->bn_part, pd * sizeof(double), false))) return fail(rc);
      if ((rc = dalloc(n->arena, &n->bn_means, (size_t)2 * kConvOut))) return fail(rc);
      if ((rc = dalloc(n->arena, &n->bn_scratch, (size_t)kConvOut))) return fail(rc);
    }
  }
  HIP_CHECK(ctx_sync_stream(ctx));
  *out = n;
  return CPP_OK;
}
extern "C" int cpp_net_create(cpp_ctx* ctx, const cpp_net_spec* spec, int max_batch, cpp_net** out) {
  return net_create(ctx, spec, max_batch, NetVariant(), out);
}
// A critic whose layers from the concat layer upward exist twice (TD3's clipped double-Q on a shared representation; an extension of
// ddpg_cartpole.py:166-171): see include/cartpolepp_abi.h
extern "C" int cpp_net_create_twin_q(cpp_ctx* ctx, const cpp_net_spec* spec, int max_batch, cpp_net** out) {
  ARG_CHECK(ctx && spec && out, "cpp_net_create_twin_q: NULL argument");
  RC(check_twin("cpp_net_create_twin_q", spec));
  NetVariant nv; nv.twin = true;
  return net_create(ctx, spec, max_batch, nv, out);
}
extern "C" int cpp_net_is_twin_q(const cpp_net* n) { return (n && n->twin) ? 1 : 0; }

// A critic whose last layer emits N logits over a fixed support (Bellemare et al. 2017; D4PG, Barth-Maron et al. 2018; an extension of
// ddpg_cartpole.py:166-177): see include/cartpolepp_abi.h
extern "C" int cpp_net_create_distributional(cpp_ctx* ctx, const cpp_net_spec* spec, int max_batch, int n_atoms, float v_min, float v_max, cpp_net** out) {
  ARG_CHECK(ctx && spec && out, "cpp_net_create_distributional: NULL argument");
  RC(check_distributional("cpp_net_create_distributional", spec, n_atoms, v_min, v_max));
  NetVariant nv; nv.dist_n = n_atoms; nv.v_min = v_min; nv.v_max = v_max;
  return net_create(ctx, spec, max_batch, nv, out);
}
extern "C" int cpp_net_distribution_info(const cpp_net* n, int* n_atoms, float* v_min, float* v_max) {
  ARG_CHECK(n, "cpp_net_distribution_info: NULL argument");
  if (n_atoms) *n_atoms = n->quant ? 0 : n->dist_n;      // (a quantile critic has no support)
  if (v_min) *v_min = n->dist_vmin;
  if (v_max) *v_max = n->dist_vmax;
  return CPP_OK;
}
// A critic whose last layer emits N quantile atoms (Dabney et al. 2018, QR-DQN; truncated targets: Kuznetsov et al. 2020, TQC; an
// extension of ddpg_cartpole.py:166-177 and :199-214): see include/cartpolepp_abi.h.  The layout, the N-wide q_value and the `logits`
// workspace are the distributional critic's; what reads them differs (quant.hip)
extern "C" int cpp_net_create_quantile(cpp_ctx* ctx, const cpp_net_spec* spec, int max_batch, int n_quantiles, cpp_net** out) {
  ARG_CHECK(ctx && spec && out, "cpp_net_create_quantile: NULL argument");
  RC(check_quantile("cpp_net_create_quantile", spec, n_quantiles));
  NetVariant nv; nv.dist_n = n_quantiles; nv.quant = true;
  return net_create(ctx, spec, max_batch, nv, out);
}
// the critic of ddpg_cartpole.py:166-177 widened: N of a network made by cpp_net_create_quantile, 0 for any other
extern "C" int cpp_net_quantile_info(const cpp_net* n, int* n_quantiles) {
  ARG_CHECK(n, "cpp_net_quantile_info: NULL argument");
  if (n_quantiles) *n_quantiles = (n->quant && !n->twin) ? n->dist_n : 0;      // (a pooled critic: cpp_net_pooled_quantile_info)
  return CPP_OK;
}
// A critic with two heads of N quantile atoms each on one representation, for the pooled truncated target of TQC (Kuznetsov et al. 2020;
// an extension of ddpg_cartpole.py:166-177 and :199-214): see include/cartpolepp_abi.h.  The layout is the twin critic's with q_value and
// q_valueb N wide; head 2's atoms land in a second `logits` workspace (quant_pool.hip reads both)
extern "C" int cpp_net_create_pooled_quantile(cpp_ctx* ctx, const cpp_net_spec* spec, int max_batch, int n_quantiles, cpp_net** out) {
  ARG_CHECK(ctx && spec && out, "cpp_net_create_pooled_quantile: NULL argument");
  RC(check_pooled_quantile("cpp_net_create_pooled_quantile", spec, n_quantiles));
  NetVariant nv; nv.twin = true; nv.quant = true; nv.dist_n = n_quantiles;
  return net_create(ctx, spec, max_batch, nv, out);
}
// ... and the same critic behind a feature layer norm (an extension of ddpg_cartpole.py:168 'hidden1'; cpp_net_create_feature_norm's rules for
// a critic; its variant record names one variant at a time, and this kind is two of its fields at once)
extern "C" int cpp_net_create_pooled_quantile_norm(cpp_ctx* ctx, const cpp_net_spec* spec, int max_batch, int n_quantiles, int activation, float epsilon,
                                                   cpp_net** out) {
  const char* who = "cpp_net_create_pooled_quantile_norm";
  ARG_CHECK(ctx && spec && out, "%s: NULL argument", who);
  RC(check_pooled_quantile(who, spec, n_quantiles));
  ARG_CHECK(spec->pixel, "%s: a low-dimensional network (there are no conv features to normalise)", who);
  ARG_CHECK(!spec->use_batch_norm && !spec->use_dropout, "%s: use_batch_norm or use_dropout (cpp_net_create_feature_norm's rules)", who);
  ARG_CHECK(activation == CPP_NORM_TANH || activation == CPP_NORM_RELU, "%s: activation %d (CPP_NORM_TANH or CPP_NORM_RELU)", who, activation);
  ARG_CHECK(std::isfinite(epsilon) && epsilon > 0.f, "%s: epsilon %g (finite, positive)", who, (double)epsilon);
  NetVariant nv; nv.twin = true; nv.quant = true; nv.dist_n = n_quantiles;
  nv.ln_act = activation == CPP_NORM_TANH ? GE_TANH : GE_RELU; nv.ln_eps = epsilon;
  return net_create(ctx, spec, max_batch, nv, out);
}
// the critic of ddpg_cartpole.py:166-177 widened: N per head of a network made by cpp_net_create_pooled_quantile(_norm), 0 for any other
extern "C" int cpp_net_pooled_quantile_info(const cpp_net* n, int* n_quantiles) {
  ARG_CHECK(n, "cpp_net_pooled_quantile_info: NULL argument");
  if (n_quantiles) *n_quantiles = n->pooled() ? n->dist_n : 0;
  return CPP_OK;
}
// An actor whose last layer emits the mean and the bounded log standard deviation of a Gaussian under a tanh (Haarnoja et al. 2018; an
// extension of ddpg_cartpole.py:95-100): see include/cartpolepp_abi.h
extern "C" int cpp_net_create_gaussian(cpp_ctx* ctx, const cpp_net_spec* spec, int max_batch, float log_std_min, float log_std_max, cpp_net** out) {
  ARG_CHECK(ctx && spec && out, "cpp_net_create_gaussian: NULL argument");
  RC(check_gaussian("cpp_net_create_gaussian", spec, log_std_min, log_std_max));
  NetVariant nv; nv.gauss = true; nv.ls_lo = log_std_min; nv.ls_hi = log_std_max;
  return net_create(ctx, spec, max_batch, nv, out);
}
// the actor of ddpg_cartpole.py:95-100 widened: 1 and the bounds for a network made by cpp_net_create_gaussian, 0 for any other
extern "C" int cpp_net_gaussian_info(const cpp_net* n, int* gaussian, float* log_std_min, float* log_std_max) {
  ARG_CHECK(n, "cpp_net_gaussian_info: NULL argument");
  if (gaussian) *gaussian = n->gauss ? 1 : 0;
  if (log_std_min) *log_std_min = n->ls_lo;
  if (log_std_max) *log_std_max = n->ls_hi;
  return CPP_OK;
}
// A pixel network whose fully connected layer 0 is Linear -> LayerNorm -> tanh / relu (the trunk of DrQ-v2, Yarats et al. 2021; an
// extension of ddpg_cartpole.py:95 'h0' and :168 'hidden1'): see include/cartpolepp_abi.h.  v: the variant it composes with.
extern "C" int cpp_net_create_feature_norm(cpp_ctx* ctx, const cpp_net_spec* spec, int max_batch, const cpp_net_variant* v, int activation, float epsilon,
                                           cpp_net** out) {
  ARG_CHECK(ctx && spec && out, "cpp_net_create_feature_norm: NULL argument");
  ARG_CHECK(spec->kind == CPP_ACTOR || spec->kind == CPP_CRITIC, "cpp_net_create_feature_norm: kind %d (an actor or a critic of the DDPG learner)", spec->kind);
  ARG_CHECK(spec->pixel, "cpp_net_create_feature_norm: a low-dimensional network (there are no conv features to normalise)");
  ARG_CHECK(!spec->use_batch_norm, "cpp_net_create_feature_norm: use_batch_norm (one normalisation: the feature layer norm or the convs' batch norm)");
  ARG_CHECK(!spec->use_dropout, "cpp_net_create_feature_norm: use_dropout (the normalised layer would be dropped behind its activation)");
  ARG_CHECK(activation == CPP_NORM_TANH || activation == CPP_NORM_RELU, "cpp_net_create_feature_norm: activation %d (CPP_NORM_TANH or CPP_NORM_RELU)", activation);
  ARG_CHECK(std::isfinite(epsilon) && epsilon > 0.f, "cpp_net_create_feature_norm: epsilon %g (finite, positive)", (double)epsilon);
  const int width = spec->kind == CPP_ACTOR ? (spec->n_hidden >= 1 ? spec->hidden[0] : 0) : 200;
  ARG_CHECK(width >= 1 && width <= LN_MAX_WIDTH, "cpp_net_create_feature_norm: layer 0 has width %d outside [1, %d]", width, LN_MAX_WIDTH);
  static const cpp_net_variant plain = {0, 0, 0.f, 0.f, 0, 0, 0.f, 0.f};
  if (!v) v = &plain;
  const int picked = (v->twin_q ? 1 : 0) + (v->n_atoms ? 1 : 0) + (v->n_quantiles ? 1 : 0) + (v->gaussian ? 1 : 0);
  ARG_CHECK(picked <= 1, "cpp_net_create_feature_norm: %d variants at once (twin_q, n_atoms, n_quantiles, gaussian: at most one)", picked);
  const char* who = "cpp_net_create_feature_norm";
  NetVariant nv;      // (the picked one's own rule, then its fields)
  nv.ln_act = activation == CPP_NORM_TANH ? GE_TANH : GE_RELU; nv.ln_eps = epsilon;
  if (v->n_atoms) {
    RC(check_distributional(who, spec, v->n_atoms, v->v_min, v->v_max));
    nv.dist_n = v->n_atoms; nv.v_min = v->v_min; nv.v_max = v->v_max;
  } else if (v->n_quantiles) {
    RC(check_quantile(who, spec, v->n_quantiles));
    nv.dist_n = v->n_quantiles; nv.quant = true;
  } else if (v->gaussian) {
    RC(check_gaussian(who, spec, v->log_std_min, v->log_std_max));
    nv.gauss = true; nv.ls_lo = v->log_std_min; nv.ls_hi = v->log_std_max;
  } else if (v->twin_q) {
    RC(check_twin(who, spec));
    nv.twin = true;
  }
  return net_create(ctx, spec, max_batch, nv, out);
}
// on = 1, the activation and epsilon of a network made by cpp_net_create_feature_norm; on = 0 for any other
extern "C" int cpp_net_feature_norm_info(const cpp_net* n, int* on, int* activation, float* epsilon) {
  ARG_CHECK(n, "cpp_net_feature_norm_info: NULL argument");
  if (on) *on = n->ln ? 1 : 0;
  if (activation) *activation = n->ln_act == GE_RELU ? CPP_NORM_RELU : CPP_NORM_TANH;
  if (epsilon) *epsilon = n->ln_eps;
  return CPP_OK;
}
// A pixel actor without conv layers, for a shared conv encoder (SAC-AE, DrQ, DrQ-v2; an extension of ddpg_cartpole.py:78-100, whose
// actor runs base_network.py:73-127 on its own): see include/cartpolepp_abi.h
extern "C" int cpp_net_create_encoderless(cpp_ctx* ctx, const cpp_net_spec* spec, int max_batch, const cpp_net_variant* v, int norm, float epsilon,
                                          cpp_net** out) {
  const char* who = "cpp_net_create_encoderless";
  ARG_CHECK(ctx && spec && out, "%s: NULL argument", who);
  ARG_CHECK(spec->kind == CPP_ACTOR, "%s: kind %d (the encoder is a critic's; only an actor goes without one)", who, spec->kind);
  ARG_CHECK(spec->pixel, "%s: a low-dimensional network (there is no conv encoder to share)", who);
  ARG_CHECK(!spec->use_batch_norm, "%s: use_batch_norm (the critic's batch statistics would be the actor's)", who);
  ARG_CHECK(!spec->use_dropout, "%s: use_dropout", who);
  ARG_CHECK(norm == CPP_NORM_NONE || norm == CPP_NORM_TANH || norm == CPP_NORM_RELU, "%s: norm %d (CPP_NORM_NONE, CPP_NORM_TANH or CPP_NORM_RELU)", who, norm);
  NetVariant nv;
  nv.enc_less = true;
  if (norm != CPP_NORM_NONE) {
    ARG_CHECK(std::isfinite(epsilon) && epsilon > 0.f, "%s: epsilon %g (finite, positive)", who, (double)epsilon);
    const int width = spec->n_hidden >= 1 ? spec->hidden[0] : 0;
    ARG_CHECK(width >= 1 && width <= LN_MAX_WIDTH, "%s: layer 0 has width %d outside [1, %d]", who, width, LN_MAX_WIDTH);
    nv.ln_act = norm == CPP_NORM_TANH ? GE_TANH : GE_RELU; nv.ln_eps = epsilon;
  }
  if (v) ARG_CHECK(!v->twin_q && !v->n_atoms && !v->n_quantiles, "%s: a critic's variant (an actor is plain or gaussian)", who);
  if (v && v->gaussian) {
    RC(check_gaussian(who, spec, v->log_std_min, v->log_std_max));
    nv.gauss = true; nv.ls_lo = v->log_std_min; nv.ls_hi = v->log_std_max;
  }
  return net_create(ctx, spec, max_batch, nv, out);
}
// the actor's layer 0 reads the critic's flattened conv3 output: the very buffer, bias column of ones included
extern "C" int cpp_net_set_encoder(cpp_net* actor, cpp_net* critic) {
  ARG_CHECK(actor && critic, "cpp_net_set_encoder: NULL argument");
  ARG_CHECK(actor->enc_less, "cpp_net_set_encoder: the first network has conv layers of its own (cpp_net_create_encoderless makes one without)");
  ARG_CHECK(critic->spec.kind == CPP_CRITIC && has_conv(critic), "cpp_net_set_encoder: the encoder is a pixel critic's");
  ARG_CHECK(actor->ctx == critic->ctx, "cpp_net_set_encoder: the two networks live on different contexts");
  ARG_CHECK(!critic->spec.use_batch_norm, "cpp_net_set_encoder: a critic with batch norm");
  ARG_CHECK(actor->spec.H == critic->spec.H && actor->spec.W == critic->spec.W && actor->spec.C == critic->spec.C && actor->flat == critic->flat,
            "cpp_net_set_encoder: geometry differs (actor %dx%dx%d, critic %dx%dx%d)", actor->spec.H, actor->spec.W, actor->spec.C, critic->spec.H,
            critic->spec.W, critic->spec.C);
  ARG_CHECK(actor->spec.action_dim == critic->spec.action_dim, "cpp_net_set_encoder: action_dim differs (%d vs %d)", actor->spec.action_dim, critic->spec.action_dim);
  ARG_CHECK(actor->maxB == critic->maxB, "cpp_net_set_encoder: max_batch differs (%d vs %d)", actor->maxB, critic->maxB);
  ARG_CHECK(!actor->grads, "cpp_net_set_encoder: the actor belongs to a trainer already");
  ARG_CHECK(!actor->encoder, "cpp_net_set_encoder: the actor is bound already (an actor keeps the encoder it was given)");
  actor->encoder = critic;
  actor->ws[0].fcin[0] = critic->ws[0].fcin[0];
  critic->enc_users.push_back(actor);
  return CPP_OK;
}
// Either end of a binding going away: a destroyed critic leaves its actors unbound (their next forward answers CPP_ERR_STATE instead of
// reading freed memory), a destroyed actor leaves its critic's list
static void encoder_unbind(cpp_net* n) {
  for (cpp_net* a : n->enc_users) { a->encoder = nullptr; a->ws[0].fcin[0] = nullptr; }
  n->enc_users.clear();
  if (n->encoder) {
    std::vector<cpp_net*>& u = n->encoder->enc_users;
    u.erase(std::remove(u.begin(), u.end(), n), u.end());
    n->encoder = nullptr;
  }
}
extern "C" int cpp_net_encoder_info(const cpp_net* n, int* encoderless, int* bound) {
  ARG_CHECK(n, "cpp_net_encoder_info: NULL argument");
  if (encoderless) *encoderless = n->enc_less ? 1 : 0;
  if (bound) *bound = n->encoder ? 1 : 0;
  return CPP_OK;
}

extern "C" int cpp_net_destroy(cpp_net* n) {
  if (!n) return CPP_OK;
  (void)hipSetDevice(n->ctx->device);
  (void)ctx_sync_stream(n->ctx);
  encoder_unbind(n);
  n->arena.release();
  delete n;
  return CPP_OK;
}

extern "C" int64_t cpp_net_num_params(const cpp_net* n) { return n ? n->nparams : -1; }
extern "C" int cpp_net_num_vars(const cpp_net* n) { return n ? (int)n->vars.size() : -1; }
extern "C" int cpp_net_var_info(const cpp_net* n, int i, char* name, int cap, int* rank, int shape[4], int64_t* offset) {
  ARG_CHECK(n && i >= 0 && i < (int)n->vars.size(), "cpp_net_var_info: index %d", i);
  const VarInfo& v = n->vars[i];
  if (name && cap > 0) { strncpy(name, v.name.c_str(), cap - 1); name[cap - 1] = 0; }
  if (rank) *rank = v.rank;
  if (shape) for (int k = 0; k < 4; ++k) shape[k] = v.shape[k];
  if (offset) *offset = v.offset;
  return CPP_OK;
}

extern "C" int cpp_net_set_params(cpp_net* n, const float* host, int64_t cnt) {
  ARG_CHECK(n && host, "cpp_net_set_params: NULL argument");
  ARG_CHECK(cnt == n->nparams, "cpp_net_set_params: got %ld values, network has %ld", (long)cnt, n->nparams);
  n->wimg_key = nullptr;
  HIP_CHECK(hipMemcpyAsync(n->params, host, cnt * sizeof(float), hipMemcpyHostToDevice, n->ctx->stream));
  HIP_CHECK(ctx_sync_stream(n->ctx));
  return CPP_OK;
}
extern "C" int cpp_net_get_params(cpp_net* n, float* host, int64_t cnt) {
  ARG_CHECK(n && host, "cpp_net_get_params: NULL argument");
  ARG_CHECK(cnt == n->nparams, "cpp_net_get_params: asked %ld values, network has %ld", (long)cnt, n->nparams);
  HIP_CHECK(hipMemcpyAsync(host, n->params, cnt * sizeof(float), hipMemcpyDeviceToHost, n->ctx->stream));
  HIP_CHECK(ctx_sync_stream(n->ctx));
  return CPP_OK;
}
extern "C" int cpp_net_get_grads(cpp_net* n, float* host, int64_t cnt) {
  ARG_CHECK(n && host, "cpp_net_get_grads: NULL argument");
  ARG_CHECK(cnt == n->nparams, "cpp_net_get_grads: asked %ld values, network has %ld", (long)cnt, n->nparams);
  if (!n->grads) { cpp_set_error("cpp_net_get_grads: network has no train op (init_ops_for_training not called)"); return CPP_ERR_STATE; }
  HIP_CHECK(hipMemcpyAsync(host, n->grads, cnt * sizeof(float), hipMemcpyDeviceToHost, n->ctx->stream));
  HIP_CHECK(ctx_sync_stream(n->ctx));
  return CPP_OK;
}

extern "C" int cpp_net_soft_update(cpp_net* target, const cpp_net* source, float coeff) {
  ARG_CHECK(target && source, "cpp_net_soft_update: NULL argument");
  ARG_CHECK(coeff >= 0.f && coeff <= 1.f, "affine_combo_coeff %g outside [0,1]", coeff);    // base_network.py:22
  ARG_CHECK(target->nparams == source->nparams, "cpp_net_soft_update: shapes differ (%ld vs %ld)",
            target->nparams, source->nparams);                                             // base_network.py:30
  target->wimg_key = nullptr;
  return launch_soft_update(target->ctx, target->params, source->params, target->nparams, nullptr, nullptr, 0, coeff, false);
}
