"""Twin Q heads (TD3's clipped double-Q, Fujimoto et al. 2018, Algorithm 1, on a shared representation; include/cartpolepp_abi.h,
cpp_net_create_twin_q) restated on the float64 oracle: a twin critic built from oracle.ddpg_np.Net -- the plain critic plus a second
copy of the layers from the concat layer upward --, and TwinDDPG, a subclass of tests.td3_np.DelayedDDPG, so that the optimisers, target
policy smoothing and the policy delay compose with it:

    y    = r + mask discount min(Q1'(s2, a'), Q2'(s2, a'))         one a' (one noise draw) for both target heads
    td_k = Q_k(s1, a) - y,  loss = mean_b(w_b (td_1^2 + td_2^2)),  dz_qk = 2 td_k w_b / B
    d(shared layer) = (head 1's term) + (head 2's term), then the ReLU mask;  the actor follows dQ1/da only

Also the cases the CPU and the GPU tests share, and the faults the CPU test plants.  Test-only: product code never imports it."""
import collections

import numpy as np

from oracle import ddpg_np as O
from tests import ddpg_opt_np as R
from tests import td3_np as T3
from tests import tps_np as T

FAULTS = ("max_for_min",                      # the larger of the two target heads
          "target_q1_only",                   # the target from Q1' alone
          "loss_td1_only",                    # the loss (and with it head 2's gradient) from td_1 alone
          "head2_own_target",                 # head 2 regressed onto Q2', not the min
          "head2_missing_from_shared_grad",   # the shared layer's gradient from head 1 alone
          "actor_follows_q2",
          "actor_follows_min",                # the actor ascends min(Q1, Q2)
          "two_noise_draws",                  # one smoothing draw per target head
          "target_head2_not_updated",         # head 2 of the target critic left out of the soft update
          "weight_on_td1_only",               # the importance weight on td_1 only
          "head2_outside_clip_norm")          # the clip's global norm over the plain critic's variables only


def cat_index(spec):
    return [i for i, l in enumerate(spec.fc) if l[4]][0]


def twin_layout(spec):
    """[(name, shape)] of the twin variables, in flat-buffer order behind spec.layout()"""
    out = []
    for name, n_in, n_out, _a, _c in spec.fc[cat_index(spec):]:
        out.append((name + "b/weights", (n_in, n_out)))
        out.append((name + "b/biases", (n_out,)))
    return out


def full_layout(spec):
    return list(spec.layout()) + twin_layout(spec)


def num_params(spec):
    return int(sum(int(np.prod(s)) for _n, s in full_layout(spec)))


class TwinLayoutSpec(object):
    """what tests.helpers.assert_flat_close / per_var_report need of a spec: layout() over the twin critic's whole flat buffer"""

    def __init__(self, spec):
        self.spec = spec

    def layout(self):
        return full_layout(self.spec)


class TwinCritic(object):
    """oracle Net of the plain critic + the second tail; `flat` is [plain critic | twin variables]"""

    def __init__(self, spec, flat, dt):
        assert spec.kind == "critic"
        self.spec, self.dt = spec, dt
        n1 = spec.num_params()
        assert len(flat) == num_params(spec), (len(flat), num_params(spec))
        self.h1 = O.Net(spec, flat[:n1], dt)
        self.p2, off = collections.OrderedDict(), n1
        for name, shape in twin_layout(spec):
            n = int(np.prod(shape))
            self.p2[name] = np.asarray(flat[off:off + n], dtype=dt).reshape(shape)
            off += n
        self.k = cat_index(spec)

    # (the routing overrides of the GPU tests belong to the shared trunk)
    amax_override = property(lambda s: s.h1.amax_override, lambda s, v: setattr(s.h1, "amax_override", v))
    relu_override = property(lambda s: s.h1.relu_override, lambda s, v: setattr(s.h1, "relu_override", v))

    def flat(self):
        return np.concatenate([self.h1.flat()] + [np.asarray(v, self.dt).ravel() for v in self.p2.values()])

    def forward(self, state, action=None, white=None, training=True):
        """the plain critic's cache (c['out'] is head 1) + c['fc2'], c['out2']: head 2 on the same concat input"""
        c = self.h1.forward(state, action=action, white=white, training=training)
        h = c["fc"][self.k][0]
        c["fc2"] = []
        for name, _n_in, _n_out, act, _cat in self.spec.fc[self.k:]:
            y = O._act(h @ self.p2[name + "b/weights"] + self.p2[name + "b/biases"], act)
            c["fc2"].append((h, y))
            h = y
        c["out2"] = h
        return c

    def _tail(self, p, suffix, pairs, dout, g):
        dh = np.asarray(dout, dtype=self.dt)
        for (name, _n_in, _n_out, act, _cat), (h, y) in reversed(list(zip(self.spec.fc[self.k:], pairs))):
            dz = O._act_bwd(dh, y, act)
            if g is not None:
                g[name + suffix + "/biases"] = dz.sum(axis=0)
                g[name + suffix + "/weights"] = h.T @ dz
            dh = dz @ p[name + suffix + "/weights"].T
        return dh                                             # w.r.t. the concat input [h, a]

    def d_action(self, c, head=1):
        """dQ_head/da of the cached forward (dz of the linear q layer is 1)"""
        A, n_in = self.spec.action_dim, self.spec.fc[self.k][1]
        ones = np.ones_like(c["out"])
        dh = self._tail(self.h1.p, "", c["fc"][self.k:], ones, None) if head == 1 else self._tail(self.p2, "b", c["fc2"], ones, None)
        return dh[:, n_in - A:]

    def backward(self, c, dout1, dout2=None, params=True, share_head2=True):
        """(grads in full_layout order, dQ1/da).  params=False: oracle Net.backward's contract, head 1's dQ/da alone."""
        if not params:
            return None, self.d_action(c, 1)
        sp, dt = self.spec, self.dt
        A, n_in = sp.action_dim, sp.fc[self.k][1]
        g = collections.OrderedDict()
        dh1 = self._tail(self.h1.p, "", c["fc"][self.k:], dout1, g)
        dh2 = self._tail(self.p2, "b", c["fc2"], dout2, g)
        d_action = dh1[:, n_in - A:]
        dh = dh1[:, :n_in - A]
        if share_head2:
            dh = (dh + dh2[:, :n_in - A]).astype(dt)          # head 1 + head 2, in that order; the mask follows
        for (name, _ni, _no, act, _cat), (h, y) in reversed(list(zip(sp.fc[:self.k], c["fc"][:self.k]))):
            dz = O._act_bwd(dh, y, act)
            g[name + "/biases"] = dz.sum(axis=0)
            g[name + "/weights"] = h.T @ dz
            dh = dz @ self.h1.p[name + "/weights"].T
        if sp.pixel:
            g.update(self.h1.backward_trunk(c, dh.reshape(c["pool_shape"])))
        return collections.OrderedDict((n, g[n]) for n, _s in full_layout(sp)), d_action


def flatten_grads(spec, grads, dt):
    return np.concatenate([np.asarray(grads[n], dtype=dt).ravel() for n, _s in full_layout(spec)])


class TwinDDPG(T3.DelayedDDPG):
    def __init__(self, actor_spec, critic_spec, actor_flat, critic_flat, dt=np.float64, hyper=O.DEFAULT_HYPER,
                 optimiser="GradientDescent", optimiser_args=None, delay=1, smoothing=None, fault=None):
        assert fault is None or fault in FAULTS, fault
        n1 = critic_spec.num_params()
        super(TwinDDPG, self).__init__(actor_spec, critic_spec, actor_flat, critic_flat[:n1], dt, hyper, optimiser, optimiser_args,
                                       delay, smoothing, None)
        self.twin_fault = fault
        self.critic = TwinCritic(critic_spec, critic_flat, dt)
        self.target_critic = TwinCritic(critic_spec, O.soft_update(np.zeros_like(critic_flat), critic_flat, 1.0, dt), dt)
        self.slots["critic"] = R.Slots(len(critic_flat), dt)
        self.weights = None                  # importance weights (B, 1) of the next minibatch (prioritized replay), or None
        self.min_share = []                  # per target-forming pass: the share of rows whose minimum is head 1's

    def set_targets(self, target_actor_flat, target_critic_flat):
        self.target_actor = O.Net(self.actor.spec, target_actor_flat, self.dt)
        self.target_critic = TwinCritic(self.critic.spec, target_critic_flat, self.dt)

    def update_targets(self):
        tau, dt = self.hp.target_update_rate, self.dt
        if not (self.pd_fault == "target_actor_skips_when_held" and self.held):
            self.target_actor = O.Net(self.actor.spec, O.soft_update(self.target_actor.flat(), self.actor.flat(), tau, dt), dt)
        new = O.soft_update(self.target_critic.flat(), self.critic.flat(), tau, dt)
        if self.twin_fault == "target_head2_not_updated":
            n1 = self.critic.spec.num_params()
            new[n1:] = self.target_critic.flat()[n1:]
        self.target_critic = TwinCritic(self.critic.spec, new, dt)

    def _apply(self, which, grads):
        if which != "critic":
            return super(TwinDDPG, self)._apply(which, grads)
        net, dt, clip = self.critic, self.dt, self.hp.gradient_clip
        if self.twin_fault == "head2_outside_clip_norm" and clip is not None:
            n1 = net.spec.num_params()
            g, norm = O.clip_by_global_norm(grads[:n1], clip, dt)
            scale = dt(clip) * min(dt(1.0) / norm if norm > 0 else dt(np.inf), dt(1.0) / dt(clip))
            new, _n = R.apply_rule(self.opt[which], net.flat(), (np.asarray(grads, dt) * dt(scale)).astype(dt), None, self.slots[which], dt)
        else:
            new, norm = R.apply_rule(self.opt[which], net.flat(), grads, clip, self.slots[which], dt)
        self.critic = TwinCritic(net.spec, new, dt)
        return norm

    # ddpg_cartpole.py:111-113 + :220-222: the actor ascends Q1
    def actor_gradients(self, s1):
        w1 = self._white(self.actor, s1)
        ca = self.actor.forward(s1, white=w1)
        cc = self.critic.forward(s1, action=ca["out"], white=w1)
        dq_da = self.critic.d_action(cc, 1)
        if self.twin_fault == "actor_follows_q2":
            dq_da = self.critic.d_action(cc, 2)
        elif self.twin_fault == "actor_follows_min":
            dq_da = np.where(cc["out"] <= cc["out2"], dq_da, self.critic.d_action(cc, 2))
        grads, _ = self.actor.backward(ca, -dq_da)
        self.last_ag = {"actions": ca["out"], "q": cc["out"], "dq_da": dq_da, "grads": O.flatten(self.actor.spec, grads, self.dt), "cache_actor": ca}
        return self.last_ag

    def critic_gradients(self, batch, noise="draw", training=True, w=None):
        """noise: 'draw' (the smoothing of the restatement, if any: one draw, the count advances), None, or a (B, A) array.
        w: (B, 1) importance weights (default: self.weights, else uniform)"""
        s1, a, r, mask, s2 = batch
        dt, fault = self.dt, self.twin_fault
        act = np.asarray(a)
        B, A = act.shape[0], act.shape[1]
        noise2 = None
        if isinstance(noise, str):
            noise = None
            if self.smoothing is not None and training:
                sigma, clip, seed = self.smoothing
                noise = T.target_noise(seed, self.tps_n, B, A, sigma, clip, np.float64)
                if fault == "two_noise_draws":
                    noise2 = T.target_noise(seed + 1, self.tps_n, B, A, sigma, clip, np.float64)
                self.tps_n += 1
        w = self.weights if w is None else w
        w = np.ones((B, 1), dt) if w is None else np.asarray(w, dt).reshape(B, 1)
        w2 = self._white(self.target_actor, s2)
        ta = self.target_actor.forward(s2, white=w2, training=training)

        def smoothed(n):
            return ta["out"] if n is None else np.clip((ta["out"] + np.asarray(n, dt)).astype(dt), dt(-1.0), dt(1.0))
        sm = smoothed(noise)
        tq = self.target_critic.forward(s2, action=sm, white=w2, training=training)
        tq1, tq2 = tq["out"], tq["out2"]
        if noise2 is not None:
            tq2 = self.target_critic.forward(s2, action=smoothed(noise2), white=w2, training=training)["out2"]
        tdq = [self.target_critic.d_action(tq, 1), self.target_critic.d_action(tq, 2)]
        tmin = np.maximum(tq1, tq2) if fault == "max_for_min" else tq1 if fault == "target_q1_only" else np.minimum(tq1, tq2)
        self.min_share.append(float((tq1 <= tq2).mean()))
        scale = np.asarray(mask, dt) * dt(self.hp.discount)
        y = np.asarray(r, dt) + scale * tmin
        y2 = np.asarray(r, dt) + scale * tq2 if fault == "head2_own_target" else y
        cb = self.critic.forward(s1, action=np.asarray(a, dt), training=training)
        td1, td2 = cb["out"] - y, cb["out2"] - y2
        wt2 = np.ones_like(w) if fault == "weight_on_td1_only" else w
        if fault == "loss_td1_only":
            loss = (w * td1 * td1).mean(dtype=dt)
            dz2 = np.zeros_like(td2)
        else:
            loss = (w * (td1 * td1) + wt2 * (td2 * td2)).mean(dtype=dt)
            dz2 = (dt(2.0) * td2 * wt2 / dt(B)).astype(dt)
        dz1 = (dt(2.0) * td1 * w / dt(B)).astype(dt)
        grads, _ = self.critic.backward(cb, dz1, dz2, share_head2=fault != "head2_missing_from_shared_grad")
        self.last_cg = {"q": cb["out"], "q2": cb["out2"], "td": td1, "td2": td2, "loss": loss, "target_q": tq1, "target_q2": tq2,
                "target_actions": ta["out"], "smoothed_actions": sm, "target_dq_da": tdq[0], "target_dq_da2": tdq[1], "noise": noise,
                "cache_critic": cb, "grads": flatten_grads(self.critic.spec, grads, dt), "w": w}
        return self.last_cg

    def check_loss(self, batch):      # ddpg_cartpole.py:239-248 (IS_TRAINING: False): the same formula, no noise; td and q are head 1's
        out = self.critic_gradients(batch, noise=None, training=False, w=np.ones((np.asarray(batch[1]).shape[0], 1)))
        return out["loss"], out["td"], out["q"]


def td_bar(discount, sigma, cg, atol=1e-5):
    """tests.tps_np.td_bar over both target heads (the target is one of them, row by row)"""
    return max(T.td_bar(discount, sigma, cg["target_dq_da"], atol), T.td_bar(discount, sigma, cg["target_dq_da2"], atol))


def restatement(specs, P, dt, hyper, opt_name="gradient-descent", delay=1, smoothing=None, fault=None):
    name, args = T3.OPTIMISERS[opt_name]
    ref = TwinDDPG(specs[0], specs[1], P[0], P[1], dt, hyper, name, args, delay, smoothing, fault)
    ref.set_targets(P[2], P[3])
    return ref


# ---- the cases.  tests.helpers.host_case's parameters, episodes and rows; the twin variables from a stream of their own.  Independently
# initialised heads do not exercise the min on these inputs (one head is the smaller on nearly every row), so head 2's q_valueb bias, in
# the online and the target critic, is shifted by the median over the rows of Q1' - Q2' on the case's first minibatch: each head is then
# the minimum on half of its rows, and tests/test_twin_q_host.py requires at least a quarter in every compared minibatch.
MIN_SHARE = 0.25
SMOOTHING = (0.2, 0.5, 0x7D3)          # sigma, clip, seed: TD3's own sigma and clip


def twin_tail(spec, rng):
    """the twin variables, xavier + tests.helpers.make_pair's perturbation: (online, target) float32 vectors"""
    parts = []
    for name, shape in twin_layout(spec):
        if name.endswith("/biases"):
            parts.append(np.zeros(shape, np.float32))
        else:
            lim = np.sqrt(6.0 / (shape[0] + shape[1]))
            parts.append(rng.uniform(-lim, lim, shape).astype(np.float32))
    p = np.concatenate([x.ravel() for x in parts])
    p = p + rng.normal(0, 0.05, p.shape).astype(np.float32)
    return p, p + rng.normal(0, 0.01, p.shape).astype(np.float32)


def host_case(shape, B, nb, seed, rows=24, action_dim=2, batch_norm=False, drop_count=0, **plain_kw):
    """tests.helpers.host_case with twin critics: (specs, P, episodes, idxs, batches); P[1] and P[3] carry the twin variables.
    plain_kw: dropout, actor_hidden (--use-dropout: the bias shift below is taken under the masks of forward count drop_count)"""
    from tests.helpers import host_case as plain_case, set_actor_masks
    specs, P, episodes, idxs, batches = plain_case(shape, B, nb, seed, rows=rows, action_dim=action_dim, batch_norm=batch_norm, **plain_kw)
    on, tg = twin_tail(specs[1], np.random.default_rng(5000 + seed))
    P = [P[0], np.concatenate([P[1], on]), P[2], np.concatenate([P[3], tg])]
    ref = TwinDDPG(specs[0], specs[1], P[0], P[1], np.float64)
    ref.set_targets(P[2], P[3])
    set_actor_masks(ref, B, drop_count)
    s2 = batches[0][4]
    w2 = ref._white(ref.target_actor, s2)
    tq = ref.target_critic.forward(s2, action=ref.target_actor.forward(s2, white=w2)["out"], white=w2)
    shift = np.float32(np.median(tq["out"] - tq["out2"]))
    P[1][-1] += shift
    P[3][-1] += shift
    return specs, P, episodes, idxs, batches


SHAPES = {"16x16x3": (16, 16, 3, 1, 1), "32x32x6": (32, 32, 3, 1, 2), "lowdim": (2, 2, 7)}
ROWS = 24
NB, STEPS = 3, 1
# (id, shape, action_dim, B, optimiser, delay, smoothing, clip, tau): the minibatch sizes with a row tail (5, 7), every width of the
# heads kernel's instances (1, 2, 3, 4, 5, 8) and one past it (9), the whole stack twinned (lowdim), TD3 whole
CASES = (("A2-B8-sgd", "16x16x3", 2, 8, "gradient-descent", 1, None, 0.5, 0.25),
         ("A1-B5-sgd", "16x16x3", 1, 5, "gradient-descent", 1, None, 1e4, 1.0),
         ("A3-B7-momentum", "16x16x3", 3, 7, "momentum-0.5", 1, None, 0.5, 0.25),
         ("A4-B8-smoothed", "16x16x3", 4, 8, "gradient-descent", 1, SMOOTHING, 0.5, 0.25),
         ("A5-B5-smoothed", "16x16x3", 5, 5, "gradient-descent", 1, SMOOTHING, 0.5, 1.0),
         ("A8-B7-adam", "16x16x3", 8, 7, "adam", 1, None, 0.5, 0.25),
         ("A9-B8-sgd", "16x16x3", 9, 8, "gradient-descent", 1, None, 0.5, 0.25),
         ("A2-B7-weighted", "16x16x3", 2, 7, "gradient-descent", 1, None, 0.5, 0.25),
         ("A4-B5-weighted-smoothed", "16x16x3", 4, 5, "momentum-0.5", 1, SMOOTHING, 0.5, 0.25),
         ("A2-B8-32x32x6-td3", "32x32x6", 2, 8, "adam", 2, SMOOTHING, 0.5, 0.25),
         ("lowdim-A3-B16-td3", "lowdim", 3, 16, "adam", 2, SMOOTHING, 0.5, 0.25))


# host_case seeds: per case the first of 1, 2, ... on which every compared minibatch meets MIN_SHARE, the float32 evaluation keeps the float64
# routes and stays inside the GPU test's bounds, and no route is closer to a tie than tests.td3_np.TIE_FLOOR (tests/test_twin_q_host.py
# asserts all of it; a case that fails is given another seed, never a wider bound)
SEEDS = dict({c[0]: 1 for c in CASES}, **{"A4-B8-smoothed": 2, "A5-B5-smoothed": 2, "A8-B7-adam": 4, "A9-B8-sgd": 2, "A4-B5-weighted-smoothed": 4})


def case_of(cid):
    return [c for c in CASES if c[0] == cid][0]


def case_inputs(case, nb=NB, seed=None, **kw):
    cid, shape_name, A, B, _opt, _d, _sm, _clip, _tau = case
    shape = SHAPES[shape_name]
    return host_case(shape, B, nb, SEEDS[cid] if seed is None else seed, rows=ROWS, action_dim=A, **kw)


def hyper_of(case):
    _cid, _sn, _A, _B, opt, _d, _sm, clip, tau = case
    return T3.hyper_of(opt, clip, tau)


def vectors(ref):
    return R.vectors(ref)


def bounds(P, want, nb):
    return R.bounds(P, want, nb)


def structure(case):
    """(minibatches per outer step, outer steps): the weighted cases take one minibatch per call -- the device's importance weights can be
    read back for the last minibatch of a call only"""
    return (1, NB) if "weighted" in case[0] else (NB, STEPS)


def run_case(case, inputs, dt=np.float64, fault=None, nb=None, steps=None, weights=None):
    """`steps` outer steps of `nb` minibatches (default: structure(case)), the target update behind each: (the six vectors, step counts,
    per-minibatch outputs, the restatement).  weights: per-minibatch (B, 1) importance weights"""
    _cid, _sn, _A, _B, opt, d, sm, _clip, _tau = case
    if nb is None:
        nb, steps = structure(case)
    specs, P, _ep, _idxs, batches = inputs
    ref = restatement(specs, P, dt, hyper_of(case), opt, d, sm, fault)
    outs = []
    for s in range(steps):
        for k in range(s * nb, (s + 1) * nb):
            ref.weights = None if weights is None else weights[k]
            outs.append(ref.train_minibatch(batches[k]))
        ref.update_targets()
    return vectors(ref), ref.state()["step"], outs, ref


def case_weights(case, nb=NB):
    """importance weights for the weighted cases: lognormal, normalised to a maximum of 1 as per.hip's are"""
    rng = np.random.default_rng(77)
    out = []
    for _k in range(nb):
        w = rng.lognormal(0.0, 1.0, (case[3], 1))
        out.append((w / w.max()).astype(np.float32))
    return out


# ---- graph replay: TD3 whole (Adam, smoothing, --policy-delay 2, twin heads) on the rows the device draws (tests.td3_np.device_rows), the first
# outer step the eager pass and the capture, the others replays of ONE graph.  (id, shape, A, B, optimiser, delay, smoothing, clip, tau),
# minibatches per step, outer steps, sample seed
GRAPH_CASE = (("td3-16x16x3-5x3", "16x16x3", 2, 8, "adam", 2, SMOOTHING, 0.5, 0.25), 3, 5, 0)
GRAPH_SEED = 124          # (the first host_case seed on which all fifteen minibatches meet the conditions above)


def graph_inputs(seed=None, sample_seed=None):
    case, nb, steps, ss = GRAPH_CASE
    _cid, shape_name, A, B, _opt, _d, _sm, _clip, _tau = case
    specs, P, episodes, _idxs, _b = host_case(SHAPES[shape_name], B, 1, GRAPH_SEED if seed is None else seed, rows=ROWS, action_dim=A)
    rows = np.concatenate([T3.device_rows(ss if sample_seed is None else sample_seed, k, B, ROWS) for k in range(steps * nb)])
    return specs, P, episodes, rows, T3.batches_of(SHAPES[shape_name], episodes, ROWS, rows, B, action_dim=A)
