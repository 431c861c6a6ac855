"""The shared conv encoder of the DDPG learner (include/cartpolepp_abi.h: cpp_net_create_encoderless, cpp_net_set_encoder) restated on the
float64 oracle.  Nothing of the arithmetic is new: the restatement composes oracle.ddpg_np and the existing tests/*_np.py learners.

  - shared_actor_spec(spec): the same actor spec (plain, Gaussian, with a feature layer norm) whose layout() names no conv variable.
  - with_shared_encoder(Base): Base whose `actor` reads `critic`'s flattened pool3 and whose `target_actor` reads `target_critic`'s --
    every oracle Net the learner is handed for such a spec is adopted (the way tests.layer_norm_np adopts its nets): its forward runs
    the encoder's trunk on the given states and then its own fully connected stack, its backward ends at layer 0's [dW; db].  The
    d(features) it would have sent on is kept in the cache (c['d_features']) and goes nowhere: the stop gradient.
  - SharedDDPG: tests.ddpg_opt_np.DDPGWithOptimiser (GradientDescent, Momentum, Adam; the clip per list) on a shared encoder, with
    importance weights, and the planted faults of tests/test_shared_encoder_host.py.

Also the cases the CPU and the GPU tests share and the bars they are held to.  Test-only: product code never imports it."""
import collections
import copy

import numpy as np

from oracle import ddpg_np as O
from tests import ddpg_opt_np as R
from tests.helpers import DEFAULT_ACTOR_HIDDEN, F32_GRAD_FACTOR, delta_bound

# planted faults (tests/test_shared_encoder_host.py)
FAULTS = ("actor_grad_into_encoder",            # the actor's d(features) added into the encoder's gradient
          "target_actor_on_online_features",    # the target actor reads the ONLINE critic's features at state_2
          "actor_on_target_features",           # the actor reads the TARGET critic's features at state_1
          "conv_in_actor_norm",                 # the conv gradient of the actor's objective counted in the actor's clip norm
          "encoder_actor_rate")                 # the encoder stepped with the actor's rate


# ---- the spec: an actor spec without conv variables -------------------------------------------------------------------------------
def _no_conv(pairs):
    return [(n, s) for n, s in pairs if not n.startswith("conv")]


_spec_classes = {}


def shared_actor_spec(spec):
    """a copy of the pixel actor spec `spec` (any oracle NetSpec subclass) whose layout() holds the fully connected variables only"""
    assert spec.kind == "actor" and spec.pixel and not spec.batch_norm and not spec.dropout
    base = type(spec)
    if base not in _spec_classes:
        body = {"layout": lambda self: _no_conv(base.layout(self)), "shared_encoder": True}
        if hasattr(base, "plain_layout"):
            body["plain_layout"] = lambda self: _no_conv(base.plain_layout(self))
        _spec_classes[base] = type("Shared" + base.__name__, (base,), body)
    s = copy.copy(spec)
    s.fc = list(spec.fc)
    s.__class__ = _spec_classes[base]
    return s


def conv_params(spec):
    """floats of the three conv layers' variables: the head of a pixel network's flat buffer"""
    return int(sum(int(np.prod(s)) for n, s in O.NetSpec.layout(spec) if n.startswith("conv")))


# ---- the adopted actor net ------------------------------------------------------------------------------------------------------------
_TRUNK_KEYS = [n for n, _k, _c in O.CONV_DEFS] + [n + sfx for n, _k, _c in O.CONV_DEFS for sfx in (":zmax", ":margin", ":amax_own")]
_net_classes = {}


def _encoder_of(owner, which):
    """the network whose trunk `which` ('actor' / 'target_actor') reads"""
    fault = getattr(owner, "enc_fault", None)
    if which == "target_actor":
        return owner.critic if fault == "target_actor_on_online_features" else owner.target_critic
    return owner.target_critic if fault == "actor_on_target_features" else owner.critic


def encoder_features(enc, state, white=None, training=True):
    """(flattened pool3, the encoder's cache) of a critic-like oracle net on `state`: its own forward, at a zero action"""
    B = np.asarray(state).shape[0]
    c = enc.forward(state, action=np.zeros((B, enc.spec.action_dim), enc.dt), white=white, training=training)
    return c["fc"][0][0], c


def _net_class(base):
    if base in _net_classes:
        return _net_classes[base]

    class EncActorNet(base):
        def forward(self, state, action=None, white=None, training=True):
            enc = _encoder_of(self._owner, self._which)
            feats, ce = encoder_features(enc, state, white=white, training=training)
            sp = self.spec
            sp.pixel = False      # (the oracle's forward from the flattened features on)
            try:
                c = base.forward(self, feats, action=action, white=None, training=training)
            finally:
                sp.pixel = True
            for k in _TRUNK_KEYS:      # the routes the tests read off an actor's cache are the encoder's
                c[k] = ce[k]
            c["white"], c["pool_shape"], c["encoder_cache"], c["encoder"] = ce["white"], ce["pool_shape"], ce, enc
            return c

        def backward_trunk(self, c, dp):
            c["d_features"] = np.asarray(dp)      # ... and stops here
            return collections.OrderedDict()

    EncActorNet.__name__ = "EncActor" + base.__name__
    _net_classes[base] = EncActorNet
    return EncActorNet


class _AdoptsShared(object):
    """every oracle Net (of whatever class the learner's other mix-ins made it) this learner is handed as `actor` or `target_actor` for a
    shared_actor_spec becomes an EncActorNet that knows the learner"""
    enc_fault = None

    def __setattr__(self, key, value):
        super(_AdoptsShared, self).__setattr__(key, value)      # (tests.layer_norm_np's adoption, if the learner has it, comes first)
        value = self.__dict__.get(key)      # (another mix-in may have changed its class on the way)
        if key in ("actor", "target_actor", "_soft") and getattr(getattr(value, "spec", None), "shared_encoder", False):
            if not hasattr(value, "_owner"):
                value.__class__ = _net_class(type(value))
            value._owner, value._which = self, "actor" if key == "actor" else "target_actor"


_made = {}


def with_shared_encoder(Base):
    if Base not in _made:
        _made[Base] = type("SharedEncoder" + Base.__name__, (_AdoptsShared, Base), {})
    return _made[Base]


def encoder_leak(ca):
    """the conv gradient the actor's objective would send into its encoder, flat over the conv variables in layout order: what the stop
    gradient withholds (the faults add it somewhere)"""
    enc, ce = ca["encoder"], ca["encoder_cache"]
    trunk = getattr(enc, "h1", enc)
    g = trunk.backward_trunk(ce, np.asarray(ca["d_features"]).reshape(ce["pool_shape"]))
    return np.concatenate([np.asarray(g[n], trunk.dt).ravel() for n, _s in O.NetSpec.layout(enc.spec) if n.startswith("conv")])


# ---- the learner ------------------------------------------------------------------------------------------------------------------------
class SharedDDPG(with_shared_encoder(R.DDPGWithOptimiser)):
    def __init__(self, actor_spec, critic_spec, actor_flat, critic_flat, dt=np.float64, hyper=O.DEFAULT_HYPER, optimiser="GradientDescent",
                 optimiser_args=None, fault=None):
        assert fault is None or fault in FAULTS
        self.enc_fault = fault
        super(SharedDDPG, self).__init__(actor_spec, critic_spec, actor_flat, critic_flat, dt, hyper, optimiser, optimiser_args)
        self.leak = None

    def critic_gradients(self, batch, training=True, td_override=None, weights=None):
        """oracle.DDPG.critic_gradients with importance weights on the loss (prioritized replay): loss = mean(w td^2)"""
        if weights is None:
            return super(SharedDDPG, self).critic_gradients(batch, training, td_override)
        s1, a, r, mask, s2 = batch
        dt = self.dt
        w2 = self._white(self.target_actor, s2)
        ta = self.target_actor.forward(s2, white=w2, training=training)
        tq = self.target_critic.forward(s2, action=ta["out"], white=w2, training=training)
        y = np.asarray(r, dt) + np.asarray(mask, dt) * dt(self.hp.discount) * tq["out"]
        cb = self.critic.forward(s1, action=np.asarray(a, dt), training=training)
        td = cb["out"] - y
        w = np.asarray(weights, dt).reshape(td.shape)
        grads, _ = self.critic.backward(cb, (dt(2.0) * w * td / dt(td.shape[0])).astype(dt))
        return {"q": cb["out"], "td": td, "loss": (w * td * td).mean(dtype=dt), "target_q": tq["out"], "target_actions": ta["out"],
                "cache_critic": cb, "grads": O.flatten(self.critic.spec, grads, dt)}

    def _apply(self, which, grads):
        fault, dt, hp = self.enc_fault, self.dt, self.hp
        net = getattr(self, which)
        nconv = conv_params(self.critic.spec)
        grads = np.asarray(grads, dt)
        if fault == "actor_grad_into_encoder" and which == "critic":
            grads = grads.copy()
            grads[:nconv] += self.leak
        if fault == "conv_in_actor_norm" and which == "actor":
            clipped, norm = O.clip_by_global_norm(np.concatenate([grads, self.leak]), hp.gradient_clip, dt)
            new, _n = R.apply_rule(self.opt[which], net.flat(), clipped[:len(grads)], None, self.slots[which], dt)
        elif fault == "encoder_actor_rate" and which == "critic":
            other = copy.deepcopy(self.slots[which])
            wrong, _n = R.apply_rule(self.opt["actor"], net.flat(), grads, hp.gradient_clip, other, dt)
            new, norm = R.apply_rule(self.opt[which], net.flat(), grads, hp.gradient_clip, self.slots[which], dt)
            new[:nconv] = wrong[:nconv]
            self.slots[which].m[:nconv], self.slots[which].v[:nconv] = other.m[:nconv], other.v[:nconv]
        else:
            new, norm = R.apply_rule(self.opt[which], net.flat(), grads, hp.gradient_clip, self.slots[which], dt)
        setattr(self, which, O.Net(net.spec, new, dt))
        return norm

    def train_minibatch(self, batch, weights=None):
        """both gradient sets from the same snapshot, then both applies (tests.ddpg_opt_np.DDPGWithOptimiser.train_minibatch); returns
        every compared quantity"""
        self._call()
        ag = self.actor_gradients(batch[0])
        cg = self.critic_gradients(batch, weights=weights)
        self.leak = encoder_leak(ag["cache_actor"])
        a_norm = self._apply("actor", ag["grads"])
        c_norm = self._apply("critic", cg["grads"])
        return {"actions": ag["actions"], "q_actor": ag["q"], "dq_da": ag["dq_da"], "actor_grads": ag["grads"], "actor_norm": float(a_norm),
                "target_actions": cg["target_actions"], "target_q": cg["target_q"], "q": cg["q"], "td": cg["td"], "loss": float(cg["loss"]),
                "critic_grads": cg["grads"], "critic_norm": float(c_norm), "cache_actor": ag["cache_actor"], "cache_critic": cg["cache_critic"],
                "leak": self.leak}

    # ---- the device's state in, the restatement's out (a common start per minibatch)
    def set_state(self, vec):
        dt = self.dt
        for which in ("actor", "critic", "target_actor", "target_critic"):
            setattr(self, which, O.Net(getattr(self, which).spec, np.asarray(vec[which], dt), dt))
        nA = len(vec["actor"])
        for which, sl in (("actor", slice(0, nA)), ("critic", slice(nA, None))):
            s = self.slots[which]
            s.m, s.v = np.asarray(vec["m"][sl], dt).copy(), np.asarray(vec["v"][sl], dt).copy()
            s.t = int(vec["step"][0 if which == "actor" else 1])

    def vectors(self):
        f = lambda n: np.asarray(n.flat(), np.float64)
        st = self.state()
        return {"actor": f(self.actor), "critic": f(self.critic), "target_actor": f(self.target_actor), "target_critic": f(self.target_critic),
                "m": st["m"], "v": st["v"], "step": [int(x) for x in st["step"]]}


VECTORS = ("actor", "critic", "target_actor", "target_critic", "m", "v")


def specs_for(shape, action_dim=2, actor_hidden=DEFAULT_ACTOR_HIDDEN):
    kw = dict(pixel=True, H=shape[0], W=shape[1], C=int(np.prod(shape[2:])))
    return (shared_actor_spec(O.NetSpec("actor", action_dim, list(actor_hidden), **kw)), O.NetSpec("critic", action_dim, [], **kw))


def restatement(specs, P, dt=np.float64, hyper=O.DEFAULT_HYPER, opt="gradient-descent", fault=None):
    name, args = OPTIMISERS[opt]
    ref = SharedDDPG(specs[0], specs[1], P[0], P[1], dt, hyper, name, args, fault=fault)
    ref.set_targets(P[2], P[3])
    return ref


# ---- the cases --------------------------------------------------------------------------------------------------------------------------
OPTIMISERS = dict(R.OPTIMISERS, **{"gradient-descent": ("GradientDescent", {})})
SHAPES = {"8x8x6": (8, 8, 3, 1, 2), "12x10x9": (12, 10, 3, 1, 3), "64x64x18": (64, 64, 3, 2, 3)}
ROWS = 24
NB = 2          # minibatches per case, each from the device's own state
# id, shape, A, B, optimiser, gradient clip, actor hidden layers.  8x8x6 at B = 1, 5, 7 (the heads kernel's four-row tail) and A = 1, 2;
# hidden (100, 100, 50): the fused heads with their leading actor layer (`pre`), (100, 50): without; 12x10x9: odd geometry, the generic
# conv1 route; 64x64x18: the row-streaming conv1 and the bf16 conv2 / conv3 tail at two forward networks.  The clip: tests.helpers.LOUD's 0.5
# sits below both pre-clip norms of these cases and UNCLIPPED_1E4's 1e4 above both; 4.25 and 40 sit between the actor's norm -- now of its
# fully connected layers alone -- and the critic's (SIDES; tests/test_shared_encoder_host.py holds every case to its side).
CASES = (("8x8x6-A2-B5-sgd", "8x8x6", 2, 5, "gradient-descent", 0.5, (100, 100, 50)),
         ("8x8x6-A1-B1-sgd", "8x8x6", 1, 1, "gradient-descent", 1e4, (100, 100, 50)),
         ("8x8x6-A2-B7-momentum", "8x8x6", 2, 7, "momentum-0.5", 0.5, (100, 50)),
         ("8x8x6-A1-B5-adam", "8x8x6", 1, 5, "adam", 1e4, (100, 50)),
         ("8x8x6-A2-B5-adam-split", "8x8x6", 2, 5, "adam", 4.25, (100, 100, 50)),
         ("12x10x9-A2-B3-momentum", "12x10x9", 2, 3, "momentum-0.5", 1e4, (100, 100, 50)),
         ("64x64x18-A2-B8-sgd", "64x64x18", 2, 8, "gradient-descent", 0.5, (100, 100, 50)),
         ("64x64x18-A2-B8-adam-split", "64x64x18", 2, 8, "adam", 40.0, (100, 100, 50)))
SEEDS = {c[0]: 1 for c in CASES}
SIDES = {c[0]: {0.5: "below", 1e4: "above"}.get(c[5], "between") for c in CASES}


def case_of(cid):
    return [c for c in CASES if c[0] == cid][0]


def hyper_of(case):
    """tests.helpers.LOUD's discount and target rate; the rates of tests.ddpg_opt_np per rule (Adam's differ between the lists, so a rate on
    the wrong list shows; GradientDescent takes LOUD's own, which differ as well)"""
    opt, clip = case[4], case[5]
    la, lc = R.RATES.get(opt, (1e-2, 5e-2))
    return O.Hyper(la, lc, 0.9, clip, 0.25)


def case_inputs(case, nb=NB, seed=None):
    """(specs, P, episodes, idxs, batches) as tests.helpers.host_case makes them, for a shared-encoder learner: the actor's parameters
    are the plain actor's fully connected tail (the same numbers a plain case draws)"""
    from tests.helpers import host_case
    cid, shape_name, A, B, _opt, _clip, hidden = case
    shape = SHAPES[shape_name]
    (aspec, cspec), P, episodes, idxs, batches = host_case(shape, B, nb, SEEDS[cid] if seed is None else seed, rows=ROWS, action_dim=A, actor_hidden=hidden)
    k = conv_params(aspec)
    P = [P[0][k:].copy(), P[1], P[2][k:].copy(), P[3]]
    return (shared_actor_spec(aspec), cspec), P, episodes, idxs, batches


def initial_state(P):
    n = len(P[0]) + len(P[1])
    f = lambda v: np.asarray(v, np.float64)
    return {"actor": f(P[0]), "critic": f(P[1]), "target_actor": f(P[2]), "target_critic": f(P[3]), "m": np.zeros(n), "v": np.zeros(n), "step": [0, 0]}


# ---- the bars (the ones the existing whole-minibatch tests take from tests/helpers.py) ---------------------------------------------
ROW_ATOL = 1e-5          # a, a', Q, td, dq_da per element and the loss, times max(1, |value|): "the ordinary 1e-5"
NORM_RTOL = 1e-4         # both pre-clip norms (tests/test_gpu_ddpg_optimisers.py)
GRAD_REL = 2e-5          # both gradient lists per variable (tests.helpers.assert_flat_close), or F32_GRAD_FACTOR x the float32 twin's
DELTA_R = 5e-5           # the parameter, target and slot deltas: tests.helpers.delta_bound(theta, delta, r, nb = 1)
ROW_KEYS = ("actions", "target_actions", "q", "td", "dq_da")


def f32_rel_of(spec, twin_grads, want_grads):
    from tests.helpers import per_var_report
    return {n: F32_GRAD_FACTOR * r for n, _m, r in per_var_report(spec, np.asarray(twin_grads, np.float64), want_grads)}


def ratios(specs, start, got, got_vec, want, want_vec):
    """error / bar of every compared quantity of one minibatch (start: the common start's vectors).  Gradient lists: the worst variable,
    by tests.helpers.per_var_report's relative l2 against GRAD_REL -- the float32 twin's own distance is applied by the callers that
    have one (assert_flat_close's rel_of)"""
    from tests.helpers import per_var_report
    f = lambda v: np.asarray(v, np.float64)
    r = {}
    for k in ROW_KEYS:
        if k not in got:      # (a' where the caller could not take it: the device's own draw)
            continue
        w = f(want[k]).reshape(-1)
        r[k] = float(np.max(np.abs(f(got[k]).reshape(-1) - w) / (ROW_ATOL * np.maximum(1.0, np.abs(w)))))
    r["loss"] = abs(float(got["loss"]) - want["loss"]) / (ROW_ATOL * max(1.0, abs(want["loss"])))
    for k in ("actor_norm", "critic_norm"):
        r[k] = abs(float(got[k]) - want[k]) / (NORM_RTOL * max(1.0, want[k]))
    for k, spec in (("actor_grads", specs[0]), ("critic_grads", specs[1])):
        scale = float(np.linalg.norm(f(want[k]))) / np.sqrt(len(want[k])) + 1e-30
        r[k] = max(min(rel / GRAD_REL, mx / (GRAD_REL * scale)) for _n, mx, rel in per_var_report(spec, f(got[k]), f(want[k])))
    for k in VECTORS:
        d = f(want_vec[k]) - f(start[k])
        if not d.any() and not f(got_vec[k]).any():
            r[k] = 0.0
            continue
        r[k] = float(np.linalg.norm(f(got_vec[k]) - f(want_vec[k]))) / delta_bound(start[k], d, DELTA_R)
    return r


# ---- the compositions: the existing restatements on a shared encoder ---------------------------------------------------------------------
# Each is one of the tests/*_np.py learners of tests.td3_np.DelayedDDPG's family (its own arithmetic untouched) with the two actors
# adopted; soft actor-critic is tests.sac_np.ComposedSac (sac_* below).  One whole-minibatch case each, the smallest shape at which the
# path can go wrong; the DrQ-v2 stack whole at 64x64x18, B = 8.
COMP_SMOOTHING = (0.2, 0.5, 7)          # sigma, clip, seed: TD3's and DrQ-v2's sigma
COMP_QUANT = (8, 1.0, 0)                # N, kappa, dropped top quantiles
COMP_SHIFT = (4, 3)                     # pad, seed
# name: kind, shape, A, B, optimiser, clip, delay, smoothing, device options beyond the optimiser's and the hyperparameters'
COMPOSITIONS = collections.OrderedDict([
    ("twin-actor-min", ("min", "8x8x6", 2, 5, "gradient-descent", 0.5, 1, None, dict(twin_q=True, actor_min_q=True))),
    ("feature-layer-norm", ("ln", "8x8x6", 2, 5, "gradient-descent", 0.5, 1, None, dict(feature_layer_norm=True))),
    ("smoothing-policy-delay-2", ("plain", "8x8x6", 2, 5, "gradient-descent", 0.5, 2, COMP_SMOOTHING,
                                  dict(target_policy_noise=COMP_SMOOTHING[0], target_policy_noise_clip=COMP_SMOOTHING[1],
                                       target_policy_noise_seed=COMP_SMOOTHING[2], policy_delay=2))),
    ("bc-alpha-2.5", ("bc", "8x8x6", 2, 5, "gradient-descent", 0.5, 1, None, dict(bc_alpha=2.5))),
    ("quantile", ("quant", "8x8x6", 2, 5, "gradient-descent", 0.5, 1, None,
                  dict(quantile_critic=True, num_quantiles=COMP_QUANT[0], quantile_huber_kappa=COMP_QUANT[1], drop_top_quantiles=COMP_QUANT[2]))),
    ("drq-v2-64x64x18", ("ln+min", "64x64x18", 2, 8, "adam", 0.5, 1, COMP_SMOOTHING,
                         dict(twin_q=True, actor_min_q=True, feature_layer_norm=True, n_step=3, target_policy_noise=COMP_SMOOTHING[0],
                              target_policy_noise_clip=COMP_SMOOTHING[1], target_policy_noise_seed=COMP_SMOOTHING[2],
                              random_shift=COMP_SHIFT[0], random_shift_seed=COMP_SHIFT[1], replay_store="u8")))])
COMP_SEED = 1


def comp_hyper(name):
    _kind, _sn, _A, _B, opt, clip, _d, _sm, _kw = COMPOSITIONS[name]
    la, lc = R.RATES.get(opt, (1e-2, 5e-2))
    return O.Hyper(la, lc, 0.9, clip, 0.25)


def _comp_modules():
    from tests import actor_min_np as AM, bc_np as BC, layer_norm_np as L, quant_np as Q, td3_np as T3, twin_np as W, tps_np as T
    from tests import dist_np as DN
    return AM, BC, L, Q, T3, W, T, DN


def comp_inputs(name, nb=NB):
    """{specs, layout (the specs per_var_report walks the two lists with), P in the DEVICE's order, episodes, idxs, batches}: tests.helpers.
    host_case's numbers, the actor's fully connected tail, and what the composition adds (twin tails, gamma / beta, the N-wide q_value)
    from a stream of its own"""
    from tests.helpers import host_case
    AM, BC, L, Q, T3, W, T, DN = _comp_modules()
    kind, shape_name, A, B, _opt, _clip, _d, _sm, _kw = COMPOSITIONS[name]
    shape = SHAPES[shape_name]
    (aspec, cspec), P, episodes, idxs, batches = host_case(shape, B, nb, COMP_SEED, rows=ROWS, action_dim=A)
    rng = np.random.default_rng(4000 + COMP_SEED)
    k = conv_params(aspec)
    P = [P[0][k:].copy(), P[1].copy(), P[2][k:].copy(), P[3].copy()]
    if "ln" in kind:
        kw = dict(pixel=True, H=shape[0], W=shape[1], C=int(np.prod(shape[2:])))
        aspec, cspec = L.LnSpec("actor", A, list(aspec.hidden), "tanh", L.EPS, **kw), L.LnSpec("critic", A, [], "tanh", L.EPS, **kw)
    if kind == "quant":
        n = COMP_QUANT[0]
        cut = cspec.fc[-1][1] * 1 + 1
        tail, ttail = Q.q_value_tail(cspec, n, rng)
        cspec = DN.dist_spec(cspec, n)
        P[1], P[3] = np.concatenate([P[1][:-cut], tail]), np.concatenate([P[3][:-cut], ttail])
    norm = {}
    if "ln" in kind:      # gamma around 1, beta around 0: both carry signal
        for i, spec in ((0, aspec), (1, cspec), (2, aspec), (3, cspec)):
            w = spec.fc[0][2]
            norm[i] = np.concatenate([1.0 + rng.normal(0, 0.1, w), rng.normal(0, 0.1, w)]).astype(np.float32)
    if "min" in kind:     # the twin tails behind the plain critic (the device's order: [plain | twin | gamma beta])
        tail, ttail = W.twin_tail(cspec, rng)
        P[1], P[3] = np.concatenate([P[1], tail]), np.concatenate([P[3], ttail])
    for i in norm:
        P[i] = np.concatenate([P[i], norm[i]])
    aspec = shared_actor_spec(aspec)
    layout = (aspec, W.TwinLayoutSpec(cspec) if "min" in kind else cspec)
    return {"name": name, "specs": (aspec, cspec), "layout": layout, "P": P, "episodes": episodes, "idxs": idxs, "batches": batches}


def comp_critic_to_ref(name, inputs, v):
    """a critic-shaped vector (parameters, a gradient list, a slot) from the device's order into the restatement's, and back"""
    if COMPOSITIONS[name][0] != "ln+min":
        return np.asarray(v)
    from tests import layer_norm_np as L
    return L.twin_from_device(inputs["specs"][1], np.asarray(v))


def comp_critic_to_device(name, inputs, v):
    if COMPOSITIONS[name][0] != "ln+min":
        return np.asarray(v)
    from tests import layer_norm_np as L
    return L.twin_to_device(inputs["specs"][1], np.asarray(v))


def comp_restatement(name, inputs, dt=np.float64, fault=None):
    AM, BC, L, Q, T3, W, T, DN = _comp_modules()
    kind, _sn, _A, _B, opt, _clip, delay, smoothing, _kw = COMPOSITIONS[name]
    base = {"min": AM.MinTwinDDPG, "ln": T3.DelayedDDPG, "plain": T3.DelayedDDPG, "bc": BC.BcDDPG, "quant": Q.QuantDDPG, "ln+min": AM.MinTwinDDPG}[kind]
    if "ln" in kind:
        base = L.with_feature_norm(base)
    cls = with_shared_encoder(base)
    aspec, cspec = inputs["specs"]
    P = inputs["P"]
    pc, ptc = comp_critic_to_ref(name, inputs, P[1]), comp_critic_to_ref(name, inputs, P[3])
    oname, oargs = OPTIMISERS[opt]
    hp = comp_hyper(name)
    if kind == "quant":
        ref = cls(aspec, cspec, P[0], pc, COMP_QUANT, dt, hp, oname, oargs, delay, smoothing)
    elif kind == "bc":
        ref = cls(aspec, cspec, P[0], pc, dt, hp, oname, oargs, delay, smoothing, alpha=2.5, q_floor=BC.Q_FLOOR)
    else:
        ref = cls(aspec, cspec, P[0], pc, dt, hp, oname, oargs, delay, smoothing)
    ref.enc_fault = fault
    ref.set_targets(P[2], ptc)
    return ref


def comp_initial_state(inputs):
    P = inputs["P"]
    n = len(P[0]) + len(P[1])
    f = lambda v: np.asarray(v, np.float64)
    return {"actor": f(P[0]), "critic": f(P[1]), "target_actor": f(P[2]), "target_critic": f(P[3]), "m": np.zeros(n), "v": np.zeros(n), "step": [0, 0]}


def comp_set_state(ref, name, inputs, vec, k):
    """the device's vectors (its order) before minibatch k of a trainer that has run k minibatches"""
    dt = ref.dt
    nA = len(vec["actor"])
    to_ref = lambda v: comp_critic_to_ref(name, inputs, v)
    ref.actor = O.Net(ref.actor.spec, np.asarray(vec["actor"], dt), dt)
    ref.target_actor = O.Net(ref.actor.spec, np.asarray(vec["target_actor"], dt), dt)
    for which in ("critic", "target_critic"):
        old = getattr(ref, which)
        flat = np.asarray(to_ref(vec[which]), dt)
        setattr(ref, which, O.Net(old.spec, flat, dt) if isinstance(old, O.Net) else type(old).__mro__[-2](old.spec, flat, dt))
    for which, sl in (("actor", slice(0, nA)), ("critic", slice(nA, None))):
        sdev = ref.slots[which]
        conv = (lambda v: v) if which == "actor" else to_ref
        sdev.m, sdev.v = np.asarray(conv(vec["m"][sl]), dt).copy(), np.asarray(conv(vec["v"][sl]), dt).copy()
        sdev.t = int(vec["step"][0 if which == "actor" else 1])
    ref.n, ref.tps_n = k, k


def comp_vectors(ref, name, inputs):
    f = lambda n: np.asarray(n.flat(), np.float64)
    to_dev = lambda v: comp_critic_to_device(name, inputs, v)
    m = np.concatenate([np.asarray(ref.slots["actor"].m, np.float64), to_dev(np.asarray(ref.slots["critic"].m, np.float64))])
    v = np.concatenate([np.asarray(ref.slots["actor"].v, np.float64), to_dev(np.asarray(ref.slots["critic"].v, np.float64))])
    return {"actor": f(ref.actor), "critic": to_dev(f(ref.critic)), "target_actor": f(ref.target_actor), "target_critic": to_dev(f(ref.target_critic)),
            "m": m, "v": v, "step": [ref.slots["actor"].t, ref.slots["critic"].t]}


def comp_minibatch(ref, name, inputs, batch, eps=None, routes=None):
    """one minibatch and its target update on the restatement, every compared quantity returned (the critic's list in the restatement's
    own order: comp_critic_to_ref takes the device's there).  eps: the device's clipped target noise, fed where the composition smooths
    (itself held to the restated draw by the caller); routes: (pool codes, ReLU decisions) of the device's critic"""
    AM, BC, L, Q, T3, W, T, DN = _comp_modules()
    rec = {}
    if routes is not None:
        ref.critic.amax_override, ref.critic.relu_override = routes
    orig_a, orig_c = ref.actor_gradients, ref.critic_gradients

    def actor_gradients(*a, **kw):
        rec["ag"] = orig_a(*a, **kw)
        return rec["ag"]

    def critic_gradients(b, *a, **kw):
        if eps is not None and not a and not kw:
            if isinstance(ref, W.TwinDDPG):
                rec["cg"] = orig_c(b, noise=np.asarray(eps, np.float64))
            else:
                rec["cg"] = T.SmoothedDDPG.critic_gradients(ref, b, np.asarray(eps, np.float64))
        else:
            rec["cg"] = orig_c(b, *a, **kw)
        return rec["cg"]
    ref.__dict__["actor_gradients"], ref.__dict__["critic_gradients"] = actor_gradients, critic_gradients
    try:
        out = ref.train_minibatch(batch)
    finally:
        del ref.__dict__["actor_gradients"], ref.__dict__["critic_gradients"]
    ref.update_targets()
    ag, cg = rec["ag"], rec["cg"]
    return {"actions": ag["actions"], "dq_da": ag["dq_da"], "actor_grads": ag["grads"], "actor_norm": float(out["actor_norm"]),
            "target_actions": cg["target_actions"], "q": cg["q"], "td": cg["td"], "loss": float(cg["loss"]), "critic_grads": cg["grads"],
            "critic_norm": float(out["critic_norm"]), "cache_actor": ag["cache_actor"], "cache_critic": cg["cache_critic"],
            "applied": out.get("applied", True), "target_dq_da": cg.get("target_dq_da"), "noise": cg.get("noise")}


def comp_noise(name, k, B, A):
    """the restated clipped target noise of minibatch k, or None"""
    sm = COMPOSITIONS[name][7]
    if sm is None:
        return None
    from tests import tps_np as T
    return T.target_noise(sm[2], k, B, A, sm[0], sm[1], np.float64)


# ---- soft actor-critic with twin heads on a shared encoder: tests.sac_np.ComposedSac, its case, its bars (tests.sac_np.ratios)
SAC_CASE = "twin-sgd-clip0.5-A2-B8"


def sac_inputs():
    """tests.sac_np.composed_inputs of SAC_CASE with the Gaussian actor's spec and parameters cut to its fully connected layers"""
    from tests import sac_np as SAC
    case = SAC.composed_case(SAC_CASE)
    inputs = list(SAC.composed_inputs(case))
    aspec, cspec = inputs[0]
    k = conv_params(aspec)
    P = list(inputs[1])
    P[0], P[2] = P[0][k:].copy(), P[2][k:].copy()
    inputs[0], inputs[1] = (shared_actor_spec(aspec), cspec), P
    return case, tuple(inputs)


def sac_restatement(case, inputs, dt=np.float64, fault=None):
    """tests.sac_np.composed_restatement on the adopted class; fault: one of the two wrong-encoder faults"""
    from tests import sac_np as SAC
    _cid, _sn, A, _B, opt, _clip, _tau, twin, _w, _n, _pad = case
    specs, P = inputs[0], inputs[1]
    name, args = SAC.T3.OPTIMISERS[opt]
    ref = with_shared_encoder(SAC.ComposedSac)(specs[0], specs[1], P[0], P[1], dt, SAC.composed_hyper(case),
                                               SAC.SacState(SAC.C_TEMPERATURE, -float(A), SAC.C_TEMPERATURE_LR, SAC.C_NOISE_SEED), name, args, twin)
    ref.enc_fault = fault
    ref.set_target_critic(P[3])
    return ref
