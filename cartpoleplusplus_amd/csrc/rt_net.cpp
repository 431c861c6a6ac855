// networks: layout (TF variable order), workspaces, launch sequences of the conv trunk / MLP stacks, cpp_net_* entry points
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

static int net_create(cpp_ctx* ctx, const cpp_net_spec* spec, int max_batch, bool twin, cpp_net** out, int dist_n = 0, float v_min = 0.f, float v_max = 0.f,
                      bool quant = false, bool gauss = false, float ls_lo = 0.f, float ls_hi = 0.f, int ln_act = 0, float ln_eps = 0.f,
                      bool enc_less = false);
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
static int check_gaussian(const char* who, const cpp_net_spec* spec, float log_std_min, float log_std_max) {
  ARG_CHECK(spec->kind == CPP_ACTOR, "%s: kind %d (a Gaussian policy belongs to an actor)", who, spec->kind);
  ARG_CHECK(std::isfinite(log_std_min) && std::isfinite(log_std_max) && log_std_min < log_std_max, "%s: log std bounds [%g, %g] (finite, min < max)", who,
            (double)log_std_min, (double)log_std_max);
  ARG_CHECK(spec->action_dim >= 1 && spec->action_dim <= 64, "%s: action_dim %d outside [1, 64]", who, spec->action_dim);
  return CPP_OK;
}
extern "C" int cpp_net_create(cpp_ctx* ctx, const cpp_net_spec* spec, int max_batch, cpp_net** out) {
  return net_create(ctx, spec, max_batch, false, out);
}
// A critic whose layers from the concat layer upward exist twice (TD3's clipped double-Q on a shared representation; an extension of
// ddpg_cartpole.py:166-171): see include/cartpolepp_abi.h
extern "C" int cpp_net_create_twin_q(cpp_ctx* ctx, const cpp_net_spec* spec, int max_batch, cpp_net** out) {
  ARG_CHECK(ctx && spec && out, "cpp_net_create_twin_q: NULL argument");
  RC(check_twin("cpp_net_create_twin_q", spec));
  return net_create(ctx, spec, max_batch, true, out);
}
extern "C" int cpp_net_is_twin_q(const cpp_net* n) { return (n && n->twin) ? 1 : 0; }

// A critic whose last layer emits N logits over a fixed support (Bellemare et al. 2017; D4PG, Barth-Maron et al. 2018; an extension of
// ddpg_cartpole.py:166-177): see include/cartpolepp_abi.h
extern "C" int cpp_net_create_distributional(cpp_ctx* ctx, const cpp_net_spec* spec, int max_batch, int n_atoms, float v_min, float v_max, cpp_net** out) {
  ARG_CHECK(ctx && spec && out, "cpp_net_create_distributional: NULL argument");
  RC(check_distributional("cpp_net_create_distributional", spec, n_atoms, v_min, v_max));
  return net_create(ctx, spec, max_batch, false, out, n_atoms, v_min, v_max);
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
  return net_create(ctx, spec, max_batch, false, out, n_quantiles, 0.f, 0.f, true);
}
// the critic of ddpg_cartpole.py:166-177 widened: N of a network made by cpp_net_create_quantile, 0 for any other
extern "C" int cpp_net_quantile_info(const cpp_net* n, int* n_quantiles) {
  ARG_CHECK(n, "cpp_net_quantile_info: NULL argument");
  if (n_quantiles) *n_quantiles = n->quant ? n->dist_n : 0;
  return CPP_OK;
}
// An actor whose last layer emits the mean and the bounded log standard deviation of a Gaussian under a tanh (Haarnoja et al. 2018; an
// extension of ddpg_cartpole.py:95-100): see include/cartpolepp_abi.h
extern "C" int cpp_net_create_gaussian(cpp_ctx* ctx, const cpp_net_spec* spec, int max_batch, float log_std_min, float log_std_max, cpp_net** out) {
  ARG_CHECK(ctx && spec && out, "cpp_net_create_gaussian: NULL argument");
  RC(check_gaussian("cpp_net_create_gaussian", spec, log_std_min, log_std_max));
  return net_create(ctx, spec, max_batch, false, out, 0, 0.f, 0.f, false, true, log_std_min, log_std_max);
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
  const int ln_act = activation == CPP_NORM_TANH ? GE_TANH : GE_RELU;
  static const cpp_net_variant plain = {0, 0, 0.f, 0.f, 0, 0, 0.f, 0.f};
  if (!v) v = &plain;
  const int picked = (v->twin_q ? 1 : 0) + (v->n_atoms ? 1 : 0) + (v->n_quantiles ? 1 : 0) + (v->gaussian ? 1 : 0);
  ARG_CHECK(picked <= 1, "cpp_net_create_feature_norm: %d variants at once (twin_q, n_atoms, n_quantiles, gaussian: at most one)", picked);
  const char* who = "cpp_net_create_feature_norm";
  if (v->n_atoms) {
    RC(check_distributional(who, spec, v->n_atoms, v->v_min, v->v_max));
    return net_create(ctx, spec, max_batch, false, out, v->n_atoms, v->v_min, v->v_max, false, false, 0.f, 0.f, ln_act, epsilon);
  }
  if (v->n_quantiles) {
    RC(check_quantile(who, spec, v->n_quantiles));
    return net_create(ctx, spec, max_batch, false, out, v->n_quantiles, 0.f, 0.f, true, false, 0.f, 0.f, ln_act, epsilon);
  }
  if (v->gaussian) {
    RC(check_gaussian(who, spec, v->log_std_min, v->log_std_max));
    return net_create(ctx, spec, max_batch, false, out, 0, 0.f, 0.f, false, true, v->log_std_min, v->log_std_max, ln_act, epsilon);
  }
  if (v->twin_q) RC(check_twin(who, spec));
  return net_create(ctx, spec, max_batch, v->twin_q != 0, out, 0, 0.f, 0.f, false, false, 0.f, 0.f, ln_act, epsilon);
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
  int ln_act = 0;
  if (norm != CPP_NORM_NONE) {
    ARG_CHECK(std::isfinite(epsilon) && epsilon > 0.f, "%s: epsilon %g (finite, positive)", who, (double)epsilon);
    const int width = spec->n_hidden >= 1 ? spec->hidden[0] : 0;
    ARG_CHECK(width >= 1 && width <= LN_MAX_WIDTH, "%s: layer 0 has width %d outside [1, %d]", who, width, LN_MAX_WIDTH);
    ln_act = norm == CPP_NORM_TANH ? GE_TANH : GE_RELU;
  }
  if (v) ARG_CHECK(!v->twin_q && !v->n_atoms && !v->n_quantiles, "%s: a critic's variant (an actor is plain or gaussian)", who);
  const bool gauss = v && v->gaussian;
  if (gauss) RC(check_gaussian(who, spec, v->log_std_min, v->log_std_max));
  return net_create(ctx, spec, max_batch, false, out, 0, 0.f, 0.f, false, gauss, gauss ? v->log_std_min : 0.f, gauss ? v->log_std_max : 0.f, ln_act,
                    ln_act ? epsilon : 0.f, true);
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
// the ln.hip job of a network's first workspace (backward pointers once a trainer has bound the gradient buffer)
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

static int net_create(cpp_ctx* ctx, const cpp_net_spec* spec, int max_batch, bool twin, cpp_net** out, int dist_n, float v_min, float v_max, bool quant,
                      bool gauss, float ls_lo, float ls_hi, int ln_act, float ln_eps, bool enc_less) {
  ARG_CHECK(ctx && spec && out, "cpp_net_create: NULL argument");
  ARG_CHECK(max_batch >= 1, "cpp_net_create: max_batch %d", max_batch);
  ARG_CHECK(spec->kind == CPP_ACTOR || spec->kind == CPP_CRITIC || spec->kind == CPP_HEAD, "cpp_net_create: kind %d", spec->kind);
  if (spec->kind == CPP_HEAD) ARG_CHECK(spec->head_out >= 1 && spec->head_out <= 64 && (spec->head_act == 0 || spec->head_act == 2),
                                        "cpp_net_create: head_out %d head_act %d", spec->head_out, spec->head_act);
  // (a head network's action_dim is its output width -- NAF's l_values head has A (A + 1) / 2 outputs, up to 36 -- and shapes nothing)
  if (spec->kind != CPP_HEAD && !gauss)      // (cpp_net_create_gaussian has checked its own range)
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
  n->twin = twin;
  n->dist_n = dist_n; n->dist_vmin = v_min; n->dist_vmax = v_max; n->quant = quant;
  n->gauss = gauss; n->ls_lo = ls_lo; n->ls_hi = ls_hi;
  n->ln = ln_act != 0; n->ln_act = ln_act ? ln_act : GE_TANH; n->ln_eps = ln_eps;      // (ln_act: GE_TANH / GE_RELU, 0: no feature layer norm)
  n->enc_less = enc_less;
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

// --- launch sequences -------------------------------------------------------------------------
int gemm(cpp_ctx* ctx, const float* A, long sAm, long sAk, const float* Bm, long sBk, long sBn,
                float* C, long ldc, int M, int N, int K, int epi, const float* Y, long ldy,
                int accumulate) {
  GemmArgs g; memset(&g, 0, sizeof(g)); g.accumulate = accumulate; g.A = A; g.sAm = sAm; g.sAk = sAk; g.B = Bm; g.sBk = sBk; g.sBn = sBn; g.C = C; g.ldc = ldc;
  g.Y = Y; g.ldy = ldy; g.M = M; g.N = N; g.K = K; g.epi = epi;
  return launch_gemm(ctx, g);
}


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
  a.out = w.pool[i]; a.out_bstride = (i == 2) ? (long)n->flat + 1 : (long)L.Hp * L.Wp * kConvOut;
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
  a.dy.dpool = w.dpool[i]; a.dy.pool = w.pool[i]; a.dy.amax = w.amax[i];
  a.dy.dpool_bstride = (i == 2) ? (long)n->flat : (long)L.Hp * L.Wp * kConvOut;
  a.dy.pool_bstride = (i == 2) ? (long)n->flat + 1 : (long)L.Hp * L.Wp * kConvOut;
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

// descriptor of layer i of a batch-norm network for the bn.hip launches
BnNet bn_net_desc(cpp_net* n, Workspace& w, int i) {
  const ConvL& L = n->conv[i];
  BnNet d; memset(&d, 0, sizeof(d));
  d.z = w.z[i]; d.stat = w.bn_stat[i]; d.beta = n->params + L.b_off;
  d.pool = w.pool[i]; d.pool_bstride = (i == 2) ? (long)n->flat + 1 : (long)L.Hp * L.Wp * kConvOut; d.amax = w.amax[i];
  d.dpool = w.dpool[i]; d.dpool_bstride = (i == 2) ? (long)n->flat : (long)L.Hp * L.Wp * kConvOut;
  d.part = n->bn_part; d.means = n->bn_means; d.dbeta = n->grads ? n->grads + L.b_off : nullptr;
  return d;
}
BnBatch bn_batch(cpp_net* const* nets, int nn, int i, int B) {
  BnBatch bb; memset(&bb, 0, sizeof(bb));
  const ConvL& L = nets[0]->conv[i];
  bb.count = nn; bb.B = B; bb.H = L.H; bb.W = L.W; bb.C = kConvOut;
  for (int k = 0; k < nn; ++k) bb.n[k] = bn_net_desc(nets[k], nets[k]->ws[0], i);
  return bb;
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
    int mode;
    ConvArgs a = conv_fwd_args(n, w, i, state, dtype, white, B, &mode, white_bstride);
    if (i == 0) n->wimg_key = nullptr;
    if (!n->spec.use_batch_norm) {
      RC(launch_conv_fwd(ctx, kFwdKid[i], n->conv[i].Cin, n->conv[i].ks, mode, EPI_RELU_POOL, a));
    } else if (!n->is_training) {
      // inference: (z - 0) / sqrt(1 + eps) + beta  ==  the fused kernel with scaled weights and beta as the bias
      a.wscale = (float)(1.0 / sqrt(1.0 + kBnEps));
      RC(launch_conv_fwd(ctx, kFwdKid[i], n->conv[i].Cin, n->conv[i].ks, mode, EPI_RELU_POOL, a));
    } else {
      const ConvL& L = n->conv[i];
      ConvArgs p = a;                                   // plain conv output (no bias) -> statistics -> BN + ReLU + pool
      p.out = w.z[i]; p.out_bstride = (long)L.H * L.W * kConvOut; p.out_amax = nullptr; p.bias = nullptr;
      RC(launch_conv_fwd(ctx, kFwdKid[i], L.Cin, L.ks, mode, EPI_PLAIN, p));
      BnBatch bb; memset(&bb, 0, sizeof(bb));
      bb.count = 1; bb.B = B; bb.H = L.H; bb.W = L.W; bb.C = kConvOut; bb.n[0] = bn_net_desc(n, w, i);
      RC(launch_bn_forward(ctx, bb, kBnEps));
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
    ConvArgs full[CONV_BATCH_MAX], plain[CONV_BATCH_MAX]; int mode = 0;
    for (int k = 0; k < nn; ++k) {
      full[k] = conv_fwd_args(nets[k], nets[k]->ws[0], i, states[k], dtype, whites[k], B, &mode);
      plain[k] = full[k];
      plain[k].out = nets[k]->ws[0].z[i]; plain[k].out_bstride = (long)L.H * L.W * kConvOut; plain[k].out_amax = nullptr; plain[k].bias = nullptr;
    }
    RC(launch_conv_fwd_multi(ctx, kFwdKid[i], L.Cin, L.ks, mode, EPI_PLAIN, plain, nn));
    RC(launch_bn_forward(ctx, bn_batch(nets, nn, i, B), kBnEps));
  }
  return CPP_OK;
}

// fully connected layers [from, end); `action` (device, (B, A)) is spliced in front of the cat layer
GemmArgs mk_gemm(const float* A, long sAm, long sAk, const float* Bm, long sBk, long sBn, float* C, long ldc,
                        int M, int N, int K, int epi) { return mk_gemm(A, sAm, sAk, Bm, sBk, sBn, C, ldc, M, N, K, epi, nullptr, 0); }
int net_forward_fc(cpp_net* n, Workspace& w, int from, int B, const float* action) {
  cpp_ctx* ctx = n->ctx;
  const int nfc = (int)n->fc.size(), A = n->spec.action_dim;
  for (int l = from; l < nfc; ++l) {
    const FcL& L = n->fc[l];
    if (L.cat) {
      if (!action) { cpp_set_error("critic forward needs an action batch"); return CPP_ERR_ARG; }
      RC(launch_copy_cols(ctx, w.fcin[l], L.n_in + 1, L.n_in - A, action, A, 0, A, B));
    }
    float* C = (l + 1 < nfc) ? w.fcin[l + 1] : fc_last_out(w);
    const long ldc = (l + 1 < nfc) ? n->fc[l + 1].n_in + 1 : L.n_out;
    GemmArgs g = mk_gemm(w.fcin[l], L.n_in + 1, 1, n->params + L.w_off, L.n_out, 1, C, ldc, B, L.n_out, L.n_in + 1, L.act, nullptr, 0);
    set_dropout(g, n, l);
    RC(launch_gemm(ctx, g));
    if (l == 0 && n->ln) RC(ln_forward(ctx, &n, 1, B));
  }
  return from == 0 ? bump_dropout(n) : CPP_OK;
}

// conv trunk backward from w.dpool[2] (= d flat): dW/db of the three convs, dX for conv3/conv2
// batch norm (training mode): the gradient w.r.t. the plain conv output is dense -- reductions over the pooled tensors,
// dz written over z, then dW and dX from dense rows.  dbeta goes straight into the '<conv>/BatchNorm/beta' slot.
static int net_backward_conv_bn(cpp_net* n, Workspace& w, int B, const void* state, int dtype, const float* white) {
  cpp_ctx* ctx = n->ctx;
  for (int i = 2; i >= 0; --i) {
    const ConvL& L = n->conv[i];
    const long zbs = (long)L.H * L.W * kConvOut;
    BnBatch bb; memset(&bb, 0, sizeof(bb));
    bb.count = 1; bb.B = B; bb.H = L.H; bb.W = L.W; bb.C = kConvOut; bb.n[0] = bn_net_desc(n, w, i);
    RC(launch_bn_backward(ctx, bb));
    int mode;
    ConvArgs d = conv_dw_args(n, w, i, state, dtype, white, B, &mode);
    d.dy_dense = w.z[i]; d.dy_dense_bstride = zbs;
    RC(launch_conv_dw(ctx, kDwKid[i], L.Cin, L.ks, mode, d, n->grads + L.w_off, n->bn_scratch));
    if (i > 0) {
      ConvArgs x; memset(&x, 0, sizeof(x));
      x.in = w.z[i]; x.in_bstride = zbs; x.w = n->params + L.w_off; x.nout = L.Cin;
      x.out = w.dpool[i - 1]; x.out_bstride = (long)L.H * L.W * L.Cin;
      x.B = B; x.H = L.H; x.W = L.W;
      RC(launch_conv_fwd(ctx, kDxKid[i], kConvOut, L.ks, IN_F32_FLIP, EPI_PLAIN, x));
    }
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

int nets_backward_conv(cpp_ctx* ctx, cpp_net* const* nets, int nn, int B, const void* state, int dtype, const float* white) {
  if (nets[0]->spec.use_batch_norm) {                 // dense dz per layer, then dW / dX of all networks in one launch each
    for (int i = 2; i >= 0; --i) {
      const ConvL& L = nets[0]->conv[i];
      const long zbs = (long)L.H * L.W * kConvOut;
      RC(launch_bn_backward(ctx, bn_batch(nets, nn, i, B)));
      ConvArgs dl[CONV_BATCH_MAX], xl[CONV_BATCH_MAX]; float *gw[CONV_BATCH_MAX], *gb[CONV_BATCH_MAX];
      int mode = 0;
      for (int k = 0; k < nn; ++k) {
        cpp_net* n = nets[k];
        dl[k] = conv_dw_args(n, n->ws[0], i, state, dtype, white, B, &mode);
        dl[k].dy_dense = n->ws[0].z[i]; dl[k].dy_dense_bstride = zbs;
        gw[k] = n->grads + L.w_off; gb[k] = n->bn_scratch;
        if (i > 0) {
          ConvArgs& x = xl[k]; memset(&x, 0, sizeof(x));
          x.in = n->ws[0].z[i]; x.in_bstride = zbs; x.w = n->params + L.w_off; x.nout = L.Cin;
          x.out = n->ws[0].dpool[i - 1]; x.out_bstride = (long)L.H * L.W * L.Cin;
          x.B = B; x.H = L.H; x.W = L.W;
        }
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
  float* C = (l + 1 < nfc) ? w.fcin2[l + 1] : w.out2;
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

// whitening statistics of a device-resident (B, H*W*C) batch -> white[2][C]
int batch_stats(cpp_ctx* ctx, const void* s0, const void* s1, int dtype, long elems, int B, int C,
                       double* part, float* white) {
  int g = 8, c = C; while (c) { int t = g % c; g = c; c = t; }     // gcd(8, C)
  const bool vec = (elems % 8 == 0) && (C / g <= 16);
  const int nw = s1 ? 2 : 1;
  if (vec) {
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

// The network whose conv trunk (or state conversion) feeds n's fully connected stack: n itself, or the critic an encoder-less actor is
// bound to -- whose staging buffers, statistics and first workspace the inference entry points then use (ws[0].fcin[0] is shared)
static int trunk_owner(cpp_net* n, const char* who, cpp_net** e) {
  *e = n;
  if (!n->enc_less) return CPP_OK;
  if (!n->encoder) { cpp_set_error("%s: an encoder-less actor that is not bound to a critic yet (cpp_net_set_encoder)", who); return CPP_ERR_STATE; }
  *e = n->encoder;
  return CPP_OK;
}
// (m_out / ls_out: device buffers a Gaussian actor's mean kernel also fills -- cpp_net_forward_gaussian; out == nullptr: nothing is copied back)
static int forward_batch(cpp_net* n, const void* state, int state_dtype, int B, const float* action, float* out, float* m_out, float* ls_out) {
  ARG_CHECK(n && state, "cpp_net_forward / cpp_net_forward_gaussian: NULL argument");
  ARG_CHECK(B >= 1 && B <= n->maxB, "cpp_net_forward: batch %d outside [1,%d]", B, n->maxB);
  ARG_CHECK(state_dtype == CPP_F32 || state_dtype == CPP_F16, "cpp_net_forward: dtype %d", state_dtype);
  ARG_CHECK(n->spec.kind != CPP_CRITIC || action, "cpp_net_forward: critic needs an action batch");
  cpp_ctx* ctx = n->ctx;
  cpp_net* e = nullptr;
  RC(trunk_owner(n, "cpp_net_forward", &e));
  HIP_CHECK(hipSetDevice(ctx->device));
  const int A = n->spec.action_dim, no = n->dist_n ? 1 : n->gauss ? A : n->fc.back().n_out;      // (a distributional critic returns Q, a Gaussian actor tanh(m))
  if (!e->stage_state) {
    RC(e->arena.alloc(&e->stage_state, (size_t)n->maxB * e->state_elems * sizeof(float), false));
    RC(dalloc(e->arena, &e->stage_action, (size_t)n->maxB * A));
  }
  const size_t esz = state_dtype == CPP_F16 ? 2 : 4;
  HIP_CHECK(hipMemcpyAsync(e->stage_state, state, (size_t)B * e->state_elems * esz, hipMemcpyHostToDevice, ctx->stream));
  if (action) HIP_CHECK(hipMemcpyAsync(e->stage_action, action, (size_t)B * A * sizeof(float), hipMemcpyHostToDevice, ctx->stream));
  if (e->spec.pixel)
    RC(batch_stats(ctx, e->stage_state, nullptr, state_dtype, e->state_elems, B, e->spec.C, e->stats_part, e->white));
  n->is_training = e->is_training = false;                              // IS_TRAINING: False (ddpg_cartpole.py:125)
  int frc = net_forward_trunk(e, e->ws[0], e->stage_state, state_dtype, e->white, B);
  if (!frc) frc = net_forward_fc(n, n->ws[0], 0, B, action ? e->stage_action : nullptr);
  if (!frc) frc = dist_expect(n, n->ws[0], B, nullptr);
  if (!frc) frc = gauss_mean(n, n->ws[0], B, m_out, ls_out);
  n->is_training = e->is_training = true;
  if (frc) return frc;
  if (!out) return CPP_OK;
  HIP_CHECK(hipMemcpyAsync(out, n->ws[0].out, (size_t)B * no * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
  HIP_CHECK(ctx_sync_stream(ctx));
  return CPP_OK;
}

// B independent action_given calls in one pass (rollout-side inference for many env workers): every
// image is whitened with ITS OWN statistics, exactly as B separate batches of one would be (base_network.py:95-99
// at B = 1); everything after the whitening is row-local anyway.
static int forward_each(cpp_net* n, const void* state, int state_dtype, int B, const float* action, float* out, float* m_out, float* ls_out) {
  ARG_CHECK(n && state, "cpp_net_forward_each: NULL argument");
  ARG_CHECK(B >= 1 && B <= n->maxB, "cpp_net_forward_each: batch %d outside [1,%d]", B, n->maxB);
  ARG_CHECK(state_dtype == CPP_F32 || state_dtype == CPP_F16, "cpp_net_forward_each: dtype %d", state_dtype);
  ARG_CHECK(n->spec.kind != CPP_CRITIC || action, "cpp_net_forward_each: critic needs an action batch");
  cpp_ctx* ctx = n->ctx;
  cpp_net* e = nullptr;
  RC(trunk_owner(n, "cpp_net_forward_each", &e));
  HIP_CHECK(hipSetDevice(ctx->device));
  const int A = n->spec.action_dim, no = n->dist_n ? 1 : n->gauss ? A : n->fc.back().n_out, C = e->spec.C;
  if (!e->stage_state) {
    RC(e->arena.alloc(&e->stage_state, (size_t)n->maxB * e->state_elems * sizeof(float), false));
    RC(dalloc(e->arena, &e->stage_action, (size_t)n->maxB * A));
  }
  const size_t esz = state_dtype == CPP_F16 ? 2 : 4;
  HIP_CHECK(hipMemcpyAsync(e->stage_state, state, (size_t)B * e->state_elems * esz, hipMemcpyHostToDevice, ctx->stream));
  if (action) HIP_CHECK(hipMemcpyAsync(e->stage_action, action, (size_t)B * A * sizeof(float), hipMemcpyHostToDevice, ctx->stream));
  long wbs = 0;
  if (e->spec.pixel) {
    int g = 8, c = C; while (c) { int t = g % c; g = c; c = t; }
    const long npix = e->state_elems / C;
    if (e->state_elems % 8 == 0 && C / g <= 16) {       // per-row partial sums, finalised row by row
      GatherArgs ga; memset(&ga, 0, sizeof(ga));
      ga.store[0] = e->stage_state; ga.store[1] = e->stage_state; ga.part = e->stats_part; ga.elems = e->state_elems; ga.B = B; ga.C = C;
      RC(launch_gather_stats(ctx, ga, state_dtype));
      RC(launch_stats_finalize(ctx, e->stats_part, 1, B, C, (double)npix, e->white_rows));
    } else {
      for (int b = 0; b < B; ++b)
        RC(launch_stats_generic(ctx, (const char*)e->stage_state + (size_t)b * e->state_elems * esz, state_dtype, npix, C,
                                e->white_rows + (long)b * 2 * C));
    }
    wbs = 2 * C;
  }
  n->is_training = e->is_training = false;
  int frc = net_forward_trunk(e, e->ws[0], e->stage_state, state_dtype, e->white_rows, B, wbs);
  if (!frc) frc = net_forward_fc(n, n->ws[0], 0, B, action ? e->stage_action : nullptr);
  if (!frc) frc = dist_expect(n, n->ws[0], B, nullptr);
  if (!frc) frc = gauss_mean(n, n->ws[0], B, m_out, ls_out);
  n->is_training = e->is_training = true;
  if (frc) return frc;
  if (!out) return CPP_OK;
  HIP_CHECK(hipMemcpyAsync(out, n->ws[0].out, (size_t)B * no * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
  HIP_CHECK(ctx_sync_stream(ctx));
  return CPP_OK;
}

extern "C" int cpp_net_forward(cpp_net* n, const void* state, int state_dtype, int B, const float* action, float* out) {
  ARG_CHECK(out, "cpp_net_forward: NULL argument");
  return forward_batch(n, state, state_dtype, B, action, out, nullptr, nullptr);
}
extern "C" int cpp_net_forward_each(cpp_net* n, const void* state, int state_dtype, int B, const float* action, float* out) {
  ARG_CHECK(out, "cpp_net_forward_each: NULL argument");
  return forward_each(n, state, state_dtype, B, action, out, nullptr, nullptr);
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
  RC(each ? forward_each(n, state, state_dtype, B, nullptr, nullptr, dm, dls) : forward_batch(n, state, state_dtype, B, nullptr, nullptr, dm, dls));
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
  const size_t spitch = (which == 3) ? ((size_t)n->flat + 1) * sizeof(float) : row;
  HIP_CHECK(hipMemcpy2DAsync(out, row, n->ws[0].pool[which - 1], spitch, row, B, hipMemcpyDeviceToHost, n->ctx->stream));
  HIP_CHECK(ctx_sync_stream(n->ctx));
  return CPP_OK;
}

