"""The actor on the minimum head (--actor-min-q; include/cartpolepp_abi.h, cpp_ddpg_set_actor_min_q) restated on the float64 oracle:
tests.twin_np.TwinDDPG and tests.sac_np.ComposedSac with actor_gradients alone overridden,

    q1 = Q1(s1, a),  q2 = Q2(s1, a)  at a = mu(s1) (soft actor-critic: at its sample),  sel_b = 1 if q1_b <= q2_b else 2
    dq_da_b = d Q_{sel_b}(s1_b, a) / da

everything else -- the critic's target, both TDs, the twin loss, the optimisers, smoothing, the delay -- is those classes'.  Also the
cases the CPU and the GPU tests share, their seeds, and the faults the CPU test plants.  Test-only: product code never imports it."""
import numpy as np

from oracle import ddpg_np as O
from tests import sac_np as S
from tests import td3_np as T3
from tests import twin_np as W

FAULTS = ("follows_q1",                       # the switch ignored
          "follows_q2",
          "follows_max",                      # the larger head
          "one_choice_per_batch",             # one head for the whole minibatch, by the batch means
          "choice_at_fed_action",             # sel from Q(s1, a_batch), the critic's first evaluation
          "choice_from_target_heads",         # sel from the target critic's heads at (s1, a)
          "mean_of_heads",                    # the mean of the two gradients
          "tie_goes_to_q2",
          "relu_mask_of_other_head",          # the selected head's weights behind the other head's concat-layer mask
          "q_layer_weight_of_other_head")     # the selected head's chain started from the other head's q-layer weights
P_BAR = 1e-5          # the project's bar on a, Q, td and dQ/da
TIE_MARGIN = 1e-4     # ten times the bar on Q: a device within its bar cannot choose differently
MIN_SHARE = W.MIN_SHARE


def d_action_mixed(critic, cc, head, mask_head=None, qw_head=None):
    """dQ_head/da of a tests.twin_np.TwinCritic's cached forward; mask_head: whose concat-layer activation masks, qw_head: whose q-layer
    weights start the chain (None: the head's own -- then tests.twin_np.TwinCritic.d_action)"""
    sp, k = critic.spec, critic.k
    layers = sp.fc[k:]
    side = {1: (critic.h1.p, "", cc["fc"][k:]), 2: (critic.p2, "b", cc["fc2"])}
    dh = np.ones_like(cc["out"])
    n = len(layers)
    for i in reversed(range(n)):
        name, _ni, _no, act, _cat = layers[i]
        hm = mask_head if (i == 0 and mask_head) else head
        hw = qw_head if (i == n - 1 and qw_head) else head
        dz = O._act_bwd(dh, side[hm][2][i][1], act)
        dh = dz @ side[hw][0][name + side[hw][1] + "/weights"].T
    A, n_in = sp.action_dim, sp.fc[k][1]
    return dh[:, n_in - A:]


class _MinChoice(object):
    """what both restatements share: the choice and the chosen head's gradient on a cached forward of the twin critic at (s1, a)"""
    amin_fault = None
    fed = None            # the minibatch's fed actions (the fault "choice_at_fed_action" reads them)

    def _min(self, s1, w1, a, cc):
        f, crit = self.amin_fault, self.critic
        assert f is None or f in FAULTS, f
        q1, q2 = cc["out"], cc["out2"]
        c1, c2 = q1, q2
        if f == "choice_at_fed_action":
            cb = crit.forward(s1, action=np.asarray(self.fed, self.dt), white=w1)
            c1, c2 = cb["out"], cb["out2"]
        elif f == "choice_from_target_heads":
            ct = self.target_critic.forward(s1, action=a, white=w1)
            c1, c2 = ct["out"], ct["out2"]
        first = c1 <= c2
        if f == "follows_q1":
            first = np.ones_like(first)
        elif f == "follows_q2":
            first = np.zeros_like(first)
        elif f == "follows_max":
            first = c1 > c2
        elif f == "tie_goes_to_q2":
            first = c1 < c2
        elif f == "one_choice_per_batch":
            first = np.full_like(first, c1.mean() <= c2.mean())
        other = {}
        if f == "relu_mask_of_other_head":
            other = dict(mask_head=True)
        elif f == "q_layer_weight_of_other_head":
            other = dict(qw_head=True)
        d1 = d_action_mixed(crit, cc, 1, **{k: 2 for k in other})
        d2 = d_action_mixed(crit, cc, 2, **{k: 1 for k in other})
        dq = np.where(first, d1, d2)
        if f == "mean_of_heads":
            dq = (self.dt(0.5) * (d1 + d2)).astype(self.dt)
        return {"dq_da": dq, "sel": np.where(first, 1, 2).astype(np.int32).ravel(), "q1": q1, "q2": q2}


class MinTwinDDPG(_MinChoice, W.TwinDDPG):
    def __init__(self, *a, **kw):
        self.amin_fault = kw.pop("amin_fault", None)
        super(MinTwinDDPG, self).__init__(*a, **kw)

    def actor_gradients(self, s1):
        w1 = self._white(self.actor, s1)
        ca = self.actor.forward(s1, white=w1)
        cc = self.critic.forward(s1, action=ca["out"], white=w1)
        m = self._min(s1, w1, ca["out"], cc)
        grads, _ = self.actor.backward(ca, -m["dq_da"])
        self.last_ag = dict(m, actions=ca["out"], q=cc["out"], grads=O.flatten(self.actor.spec, grads, self.dt), cache_actor=ca)
        return self.last_ag


class MinComposedSac(_MinChoice, S.ComposedSac):
    def __init__(self, *a, **kw):
        self.amin_fault = kw.pop("amin_fault", None)
        super(MinComposedSac, self).__init__(*a, **kw)

    def actor_gradients(self, s1, eps1=None, fault=None, row_scale=None):
        assert self.twin and fault is None and row_scale is None
        dt = self.dt
        alpha = dt(np.exp(np.float64(self.sac.log_alpha)))
        w1 = self._white(self.actor, s1)
        ca, m, x = self._head(self.actor, s1, w1)
        eps = np.zeros_like(m) if eps1 is None else np.asarray(eps1, dt)
        pol = S.policy(m, x, eps, self.lo, self.hi, dt, None)
        cc = self.critic.forward(s1, action=pol["a"], white=w1)
        mn = self._min(s1, w1, pol["a"], cc)
        dq = mn["dq_da"]
        dm, dx = S.head_gradient(x, pol["a"], eps, dq, alpha, self.lo, self.hi, dt, None)
        grads, _ = self.actor.backward(ca, np.concatenate([dm, dx], axis=1))
        g_alpha = S.temperature_gradient(pol["logp"], self.sac.hbar, alpha)
        self.last_ag = dict(mn, actions=pol["a"], logp=pol["logp"], q=cc["out"], dm=dm, dx=dx, alpha=alpha, g_alpha=g_alpha,
                            grads=O.flatten(self.actor.spec, grads, dt), m=m, x=x, eps=eps, cache_actor=ca)
        return self.last_ag


# ---- the deterministic cases.  tests.twin_np.host_case's numbers (its shift balances the TARGET heads); head 2's online q_valueb bias is then
# shifted once more, to the midpoint between the two middle values of Q1 - Q2 at a = mu(s1) over the rows of all the case's minibatches at the
# starting parameters: each online head is the minimum on about half of the rows, and no row starts at a tie.
# (id, shape, A, B, optimiser, delay, smoothing, clip, tau) as tests.twin_np's, then {weighted, actor_hidden}.  8x8x6 is the smallest image
# the conv trunk takes; 5 and 7 rows leave the last workgroup of four teams partly empty; A = 3 and 5 run the padded instances; [200, 50]:
# an actor with two hidden layers whose first is too wide for the heads kernel's `pre` layer; A = 9 and the low-dimensional pair take the
# GEMM levels (the latter: TD3 proper -- the whole stack twinned, smoothing, delay 2)
SHAPES = {"8x8x6": (8, 8, 3, 1, 2), "lowdim": (2, 2, 7), "64x64x18": (64, 64, 3, 2, 3)}
ROWS, NB = 24, 3
SM = W.SMOOTHING
CASES = (("A1-B5-sgd", "8x8x6", 1, 5, "gradient-descent", 1, None, 0.5, 0.25, {}),
         ("A2-B7-weighted", "8x8x6", 2, 7, "gradient-descent", 1, None, 0.5, 0.25, {"weighted": True}),
         ("A3-B5-smoothed", "8x8x6", 3, 5, "momentum-0.5", 1, SM, 0.5, 0.25, {}),
         ("A5-B7-weighted-smoothed", "8x8x6", 5, 7, "adam", 1, SM, 0.5, 0.25, {"weighted": True}),
         ("A8-B5-adam", "8x8x6", 8, 5, "adam", 1, None, 0.5, 0.25, {}),
         ("A2-B1-sgd", "8x8x6", 2, 1, "gradient-descent", 1, None, 0.5, 0.25, {}),
         ("A2-B5-no-pre", "8x8x6", 2, 5, "gradient-descent", 1, None, 0.5, 0.25, {"actor_hidden": (200, 50)}),
         ("A9-B5-sgd", "8x8x6", 9, 5, "gradient-descent", 1, None, 0.5, 0.25, {}),
         ("lowdim-A3-B5-td3", "lowdim", 3, 5, "adam", 2, SM, 0.5, 0.25, {}))
FUSED = ("A1-B5-sgd", "A2-B7-weighted", "A3-B5-smoothed", "A5-B7-weighted-smoothed", "A8-B5-adam", "A2-B1-sgd", "A2-B5-no-pre")
# host_case seeds: per case the first of 1, 2, ... on which every condition of tests/test_actor_min_host.py holds -- in every compared
# minibatch each head is the minimum on at least a quarter of the rows (B = 1: over the case's minibatches together, where a quarter of one row
# has no meaning), no row has |Q1 - Q2| < TIE_MARGIN, the float32 twin chooses as float64 does, keeps its routes and stays inside the bars
SEEDS = {"A1-B5-sgd": 15, "A2-B7-weighted": 1, "A3-B5-smoothed": 2, "A5-B7-weighted-smoothed": 82, "A8-B5-adam": 94, "A2-B1-sgd": 2,
         "A2-B5-no-pre": 11, "A9-B5-sgd": 3, "lowdim-A3-B5-td3": 2}
# (what rejects the earlier seeds is nearly always the share: with 5 or 7 rows only 2 .. 3 or 2 .. 5 of them may follow head 1, in all three
# minibatches, while every update moves the two heads apart -- under Adam by more than the rows' spread within a minibatch or two)
# (A2-B1-sgd: on seed 1 the target heads order its three rows as the online heads do, and "choice_from_target_heads" cannot show)


def case_of(cid):
    return [c for c in CASES if c[0] == cid][0]


def hyper_of(case):
    return W.hyper_of(case[:9])


def restatement(case, specs, P, dt=np.float64, fault=None):
    _cid, _sn, _A, _B, opt, d, sm, _clip, _tau, _x = case
    name, args = T3.OPTIMISERS[opt]
    ref = MinTwinDDPG(specs[0], specs[1], P[0], P[1], dt, hyper_of(case), name, args, d, sm, amin_fault=fault)
    ref.set_targets(P[2], P[3])
    return ref


def midpoint_shift(diffs):
    d = np.sort(np.asarray(diffs, np.float64).ravel())
    return np.float32(0.5 * (d[len(d) // 2 - 1] + d[len(d) // 2]))


def case_inputs(case, seed=None, nb=NB):
    cid, shape_name, A, B, _opt, _d, _sm, _clip, _tau, extra = case
    kw = {"actor_hidden": extra["actor_hidden"]} if extra.get("actor_hidden") else {}
    specs, P, episodes, idxs, batches = W.host_case(SHAPES[shape_name], B, nb, SEEDS[cid] if seed is None else seed, rows=ROWS, action_dim=A, **kw)
    ref = restatement(case, specs, P)
    diffs = []
    for b in batches:
        ag = ref.actor_gradients(b[0])
        diffs.append((ag["q1"] - ag["q2"]).ravel())
    P[1][-1] += midpoint_shift(np.concatenate(diffs))
    return specs, P, episodes, idxs, batches


def case_weights(case, nb=NB):
    return W.case_weights(case[:9], nb) if case[9].get("weighted") else None


def run_case(case, inputs, dt=np.float64, fault=None, weights=None, probe=()):
    """NB calls of one minibatch, the target update behind each (what the GPU test runs): (the six vectors, per-minibatch actor outputs,
    per-minibatch critic outputs, per-minibatch step outputs, the restatement).  probe: faults whose dq_da and sel are taken on every
    minibatch's starting state beside the unfaulted pass -- {fault: [(dq_da, sel)] per minibatch}, returned as the sixth value"""
    specs, P, _ep, _idxs, batches = inputs
    ref = restatement(case, specs, P, dt, fault)
    ags, cgs, outs, probed = [], [], [], {f: [] for f in probe}
    for k, b in enumerate(batches):
        ref.weights = None if weights is None else weights[k]
        ref.fed = b[1]
        for f in probe:
            ref.amin_fault = f
            ag = ref.actor_gradients(b[0])
            probed[f].append((ag["dq_da"], ag["sel"]))
        ref.amin_fault = fault
        outs.append(ref.train_minibatch(b))
        ags.append(ref.last_ag)
        cgs.append(ref.last_cg)
        ref.update_targets()
    return W.vectors(ref), ags, cgs, outs, ref, probed


def shares(ags):
    """per minibatch: the share of rows that follow head 1, and the smallest |Q1 - Q2|"""
    return [float((ag["sel"] == 1).mean()) for ag in ags], [float(np.abs(ag["q1"] - ag["q2"]).min()) for ag in ags]


def tie_inputs(case, inputs):
    """the case with head 2 a copy of head 1 in the online critic: Q1 == Q2 on every row"""
    specs, P, episodes, idxs, batches = inputs
    spec = specs[1]
    n1, k = spec.num_params(), W.cat_index(spec)
    tail = sum(int(np.prod(s)) for name, s in spec.layout() if any(name.startswith(l[0] + "/") for l in spec.fc[k:]))
    # (the twinned layers are the last of the plain layout, in the twin variables' order)
    names = [n for n, _s in spec.layout()][-2 * len(spec.fc[k:]):]
    assert names == [n.replace("b/", "/") for n, _s in W.twin_layout(spec)], names
    P = [p.copy() for p in P]
    P[1][n1:] = P[1][n1 - tail:n1]
    return specs, P, episodes, idxs, batches


# ---- the soft actor-critic cases: tests.sac_np's composed inputs (twin critics), head 2's online bias balanced at the sample of minibatch
# k's own noise.  tests.sac_np's case tuple: (id, shape, A, B, optimiser, clip, tau, twin, weighted, n-step, pad)
SAC_CASES = (("sac-A2-B5", "16x16x6", 2, 5, "adam", 0.5, 0.25, True, False, 1, 0),
             ("sac-A9-B5", "16x16x6", 9, 5, "gradient-descent", 0.5, 0.25, True, False, 1, 0))
SAC_SEEDS = {"sac-A2-B5": 64, "sac-A9-B5": 8}      # (also: each TARGET head the minimum on a quarter of the rows, as tests.sac_np asks)
SAC_NB = 2


def sac_case_of(cid):
    return [c for c in SAC_CASES if c[0] == cid][0]


def sac_restatement(case, inputs, dt=np.float64, fault=None):
    _cid, _sn, A, _B, opt, _clip, _tau, twin, _w, _n, _pad = case
    specs, P = inputs[0], inputs[1]
    name, args = T3.OPTIMISERS[opt]
    ref = MinComposedSac(specs[0], specs[1], P[0], P[1], dt, S.composed_hyper(case),
                         S.SacState(S.C_TEMPERATURE, -float(A), S.C_TEMPERATURE_LR, S.C_NOISE_SEED), name, args, twin, amin_fault=fault)
    ref.set_target_critic(P[3])
    return ref


def sac_eps(case, k):
    _cid, _sn, A, B = case[:4]
    return S.noise(S.C_NOISE_SEED, k, B, A, S.STREAM_S1), S.noise(S.C_NOISE_SEED, k, B, A, S.STREAM_S2)


def sac_inputs(case, seed=None, nb=SAC_NB):
    cid = case[0]
    # (tests.sac_np.composed_inputs looks its seed up by the case's id: the seed is passed)
    specs, P, episodes, idxs, batches = S.composed_inputs(case, SAC_SEEDS[cid] if seed is None else seed, nb)
    ref = sac_restatement(case, (specs, P))
    diffs = []
    for k, b in enumerate(batches):
        ag = ref.actor_gradients(b[0], sac_eps(case, k)[0])
        diffs.append((ag["q1"] - ag["q2"]).ravel())
    P[1][-1] += midpoint_shift(np.concatenate(diffs))
    return specs, P, episodes, idxs, batches


def run_sac(case, inputs, dt=np.float64, fault=None, probe=()):
    ref = sac_restatement(case, inputs, dt, fault)
    ags, outs, probed = [], [], {f: [] for f in probe}
    for k, b in enumerate(inputs[4]):
        e1, e2 = sac_eps(case, k)
        ref.fed = b[1]
        for f in probe:
            ref.amin_fault = f
            ag = ref.actor_gradients(b[0], e1)
            probed[f].append((ag["dq_da"], ag["sel"]))
        ref.amin_fault = fault
        outs.append(ref.train_minibatch(b, e1, e2))
        ags.append(ref.last_ag)
        ref.update_targets()
    return ref.vectors(), ags, outs, ref, probed
