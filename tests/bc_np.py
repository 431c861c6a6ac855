"""The behaviour-cloning actor term (--bc-alpha; include/cartpolepp_abi.h, cpp_ddpg_set_behaviour_cloning; TD3+BC, Fujimoto & Gu 2021) restated
on the float64 oracle: tests.td3_np.DelayedDDPG, tests.twin_np.TwinDDPG and tests.actor_min_np.MinTwinDDPG with actor_gradients alone
overridden.  With a the minibatch's stored action, mu = actor(s1) and B the rows of this minibatch,

    q_b    = Q(s1_b, mu_b) of the head the actor follows (Q1; --actor-min-q: the row's selected head)
    m      = (1 / B) sum_b |q_b|;   lambda = alpha / max(m, q_floor)         (a constant: no gradient flows through it)
    g_bi   = -lambda dq_da_bi + (2 / A) (mu_bi - a_bi);   adz_bi = g_bi (1 - mu_bi^2)

everything else -- the critic's side, the optimisers, smoothing, the delay, the reported dq_da -- is those classes'.  Also the cases the CPU
and the GPU tests share, their seeds, the bars with their derivations, and the faults the CPU test plants.  Test-only: product code never
imports it."""
import numpy as np

from oracle import ddpg_np as O
from tests import actor_min_np as AM
from tests import td3_np as T3
from tests import twin_np as W

FAULTS = ("mean_then_abs",                    # |mean q| for mean |q|
          "lambda_per_row",                   # alpha / max(|q_b|, floor), row by row
          "lambda_from_fed_action_q",         # m from Q(s1, a_batch), the critic's first evaluation
          "lambda_from_target_critic",        # m from the target critic at (s1, mu)
          "mean_over_capacity",               # the sum divided by the batch buffer's size, not B
          "lambda_of_previous_minibatch",
          "no_floor",
          "floor_added",                      # alpha / (m + floor)
          "bc_sign",
          "bc_not_over_A",                    # 2 (mu - a)
          "bc_factor_one",                    # (1 / A) (mu - a)
          "bc_against_target_actor",          # mu'(s1) - a
          "bc_behind_tanh_missing",           # the cloning term added behind the tanh derivative, not in front of it
          "lambda_on_bc_term",                # lambda (-dq_da + (2 / A)(mu - a))
          "reported_dq_da_scaled",            # last_values' dq_da is lambda dq_da
          "follows_q1_under_min")             # --actor-min-q: m from Q1 on every row
CAPACITY_EXTRA = 3        # "mean_over_capacity" divides by B + 3

# ---- the bars
P_BAR = 1e-5              # the project's bar on a, Q, td and dQ/da
M_MIN = 0.05              # every case off the floor branch has m >= M_MIN: Q's bar is then at most 2e-4 of lambda
FLOOR_GAP = 0.1           # |m - q_floor| >= FLOOR_GAP q_floor: a device inside Q's bar takes the restatement's branch of the max
ALPHA = 2.5               # the paper's
Q_FLOOR = 1e-3            # the flag's default
HIGH_FLOOR = 2.0          # above every case's m: the floor branch
# The kernel against its own float32 inputs, recomputed in float64 (tests/test_gpu_behaviour_cloning.py).  u = 2^-24, one float32 rounding.
#   m: the sum and the division are float64 (relative error ~B 2^-53, nothing at float32's scale); one rounding to float32: u.  Bar 2u = 2^-23.
#   lambda = alpha / max(m, floor): m's u, the division's u: 2u.  Bar 4u = 2^-22.
#   g = (2 / A) (mu - a) - lambda dq_da: on the lambda term lambda's 2u + the product's u = 3u |lambda dq_da| (a fused multiply-add drops the
#       product's); on the cloning term the quotient 2 / A, the difference, the product: 3u (2 / A)|mu - a|; the final sum u of the result, at most
#       u (|lambda dq_da| + (2 / A)|mu - a|): 4u of that sum in all.  Bar 8u = 2^-21 of it.
#   adz = g (1 - mu^2): g's error times (1 - mu^2); 1 - mu^2 as one fused multiply-add has an absolute error <= u / 2 (the result is <= 1), the
#       product another u |adz| <= u |g|: 1.5 u |g|.  (Unfused: 2.5 u.)  Bar 4u |g| = 2^-22 |g| beside the first term.
M_REL, LAMBDA_REL, G_REL, ADZ_ABS = 2.0 ** -23, 2.0 ** -22, 2.0 ** -21, 2.0 ** -22


def kernel_reference(q, dq_da, mu, a, alpha, q_floor):
    """float64 on the device's own float32 inputs: (m, lambda, g, adz, bc_rows, the bars on g and adz)"""
    q, dq_da, mu, a = (np.asarray(x, np.float64) for x in (q, dq_da, mu, a))
    A = mu.shape[1]
    m = np.abs(q).mean()
    lam = alpha / max(m, q_floor)
    t1, t2 = lam * dq_da, (2.0 / A) * (mu - a)
    g = t2 - t1
    g_bar = G_REL * (np.abs(t1) + np.abs(t2))
    adz = g * (1.0 - mu * mu)
    adz_bar = g_bar * (1.0 - mu * mu) + ADZ_ABS * np.abs(g)
    return m, lam, g, adz, ((mu - a) ** 2).mean(axis=1), g_bar, adz_bar


# Whole minibatches against the restatement from a common start: Q is held to P_BAR, so m is (the mean of B errors of at most P_BAR each), and
# lambda = alpha / m moves by at most lambda P_BAR / m; 2^-22 is the kernel's own arithmetic (above).  On the floor branch lambda is alpha / floor,
# exactly representable arithmetic aside: the same bar covers it.  g: lambda's move times |dq_da|, dq_da's and (mu - a)'s P_BAR times their factors.
def lambda_bar(lam64, m64):
    return lam64 * (P_BAR / m64 + LAMBDA_REL)


def g_bar(lam64, m64, dq_da64, A):
    return lambda_bar(lam64, m64) * np.abs(dq_da64) + (lam64 + 2.0 / A) * P_BAR


class _Cloning(object):
    """what the three restatements share: lambda and the head gradient from Q, dQ/da and mu at mu(s1)"""
    bc_alpha, bc_floor, bc_fault = ALPHA, Q_FLOOR, None
    fed = None                  # the minibatch's stored actions
    prev_lambda = None          # the lambda of the last minibatch train_minibatch ran ("lambda_of_previous_minibatch")

    def _bc_init(self, kw):
        self.bc_alpha, self.bc_floor, self.bc_fault = kw.pop("alpha", ALPHA), kw.pop("q_floor", Q_FLOOR), kw.pop("bc_fault", None)
        assert self.bc_fault is None or self.bc_fault in FAULTS, self.bc_fault

    def _cloned(self, s1, w1, ca, q, dq_da, q1=None):
        """grad_ys at the actor's output; q: Q of the followed head at mu(s1), (B, 1); q1: head 1's under --actor-min-q"""
        f, dt = self.bc_fault, self.dt
        mu, a = ca["out"], np.asarray(self.fed, dt)
        assert a.shape == mu.shape, (a.shape, mu.shape)      # no row is ever left out
        B, A = mu.shape
        qs = q
        if f == "lambda_from_fed_action_q":
            qs = self.critic.forward(s1, action=a, white=w1)["out"]
        elif f == "lambda_from_target_critic":
            qs = self.target_critic.forward(s1, action=mu, white=w1)["out"]
        elif f == "follows_q1_under_min" and q1 is not None:
            qs = q1
        m = np.abs(qs).mean(dtype=dt)
        if f == "mean_then_abs":
            m = np.abs(qs.mean(dtype=dt))
        elif f == "mean_over_capacity":
            m = dt(np.abs(qs).sum(dtype=dt) / dt(B + CAPACITY_EXTRA))
        alpha, floor = dt(self.bc_alpha), dt(self.bc_floor)
        lam_own = dt(alpha / max(m, floor))
        lam = lam_own
        if f == "no_floor":
            lam = dt(alpha / m)
        elif f == "floor_added":
            lam = dt(alpha / (m + floor))
        elif f == "lambda_of_previous_minibatch" and self.prev_lambda is not None:
            lam = dt(self.prev_lambda)
        self._lambda_now = lam_own
        lam_rows = lam
        if f == "lambda_per_row":
            lam_rows = (alpha / np.maximum(np.abs(qs), floor)).astype(dt)
            lam = dt(lam_rows.mean())
        diff = (mu - a).astype(dt)
        if f == "bc_against_target_actor":
            diff = (self.target_actor.forward(s1, white=w1)["out"] - a).astype(dt)
        k = dt(2.0) / dt(A)
        if f == "bc_not_over_A":
            k = dt(2.0)
        elif f == "bc_factor_one":
            k = dt(1.0) / dt(A)
        elif f == "bc_sign":
            k = -k
        t1, t2 = (lam_rows * dq_da).astype(dt), (k * diff).astype(dt)
        g = (t2 - t1).astype(dt)
        if f == "lambda_on_bc_term":
            g = (lam_rows * (t2 - dq_da)).astype(dt)
        elif f == "bc_behind_tanh_missing":      # adz = -lambda dq_da (1 - mu^2) + t2: as grad_ys in front of the tanh derivative
            g = (t2 / (dt(1.0) - mu * mu) - t1).astype(dt)
        grads, _ = self.actor.backward(ca, g)
        reported = (lam * dq_da).astype(dt) if f == "reported_dq_da_scaled" else dq_da
        return {"actions": mu, "q_mu": q, "dq_da": reported, "m": float(m), "lambda": float(lam), "g": g, "adz": (g * (dt(1.0) - mu * mu)).astype(dt),
                "bc_rows": (diff * diff).mean(axis=1, dtype=dt), "grads": O.flatten(self.actor.spec, grads, dt), "cache_actor": ca}

    def critic_gradients(self, batch, *a, **kw):      # (unchanged; kept for the comparisons, as tests.twin_np.TwinDDPG keeps its own)
        self.last_cg = super(_Cloning, self).critic_gradients(batch, *a, **kw)
        return self.last_cg

    def train_minibatch(self, batch):
        self.fed = batch[1]
        out = super(_Cloning, self).train_minibatch(batch)
        self.prev_lambda = self._lambda_now
        return out


class BcDDPG(_Cloning, T3.DelayedDDPG):
    def __init__(self, *a, **kw):
        self._bc_init(kw)
        super(BcDDPG, self).__init__(*a, **kw)

    def actor_gradients(self, s1):
        w1 = self._white(self.actor, s1)
        ca = self.actor.forward(s1, white=w1)
        cc = self.critic.forward(s1, action=ca["out"], white=w1)
        _, dq_da = self.critic.backward(cc, np.ones_like(cc["out"]), params=False)
        self.last_ag = dict(self._cloned(s1, w1, ca, cc["out"], dq_da), q=cc["out"])
        return self.last_ag


class BcTwinDDPG(_Cloning, W.TwinDDPG):
    def __init__(self, *a, **kw):
        self._bc_init(kw)
        super(BcTwinDDPG, self).__init__(*a, **kw)

    def actor_gradients(self, s1):
        w1 = self._white(self.actor, s1)
        ca = self.actor.forward(s1, white=w1)
        cc = self.critic.forward(s1, action=ca["out"], white=w1)
        self.last_ag = dict(self._cloned(s1, w1, ca, cc["out"], self.critic.d_action(cc, 1)), q=cc["out"], q1=cc["out"], q2=cc["out2"])
        return self.last_ag


class BcMinTwinDDPG(_Cloning, AM.MinTwinDDPG):
    def __init__(self, *a, **kw):
        self._bc_init(kw)
        super(BcMinTwinDDPG, self).__init__(*a, **kw)

    def actor_gradients(self, s1):
        w1 = self._white(self.actor, s1)
        ca = self.actor.forward(s1, white=w1)
        cc = self.critic.forward(s1, action=ca["out"], white=w1)
        mn = self._min(s1, w1, ca["out"], cc)
        q = np.where((mn["sel"] == 1).reshape(-1, 1), mn["q1"], mn["q2"])
        self.last_ag = dict(self._cloned(s1, w1, ca, q, mn["dq_da"], q1=mn["q1"]), q=cc["out"], q1=mn["q1"], q2=mn["q2"], sel=mn["sel"])
        return self.last_ag


# ---- the cases.  (id, shape, A, B, optimiser, delay, smoothing, clip, tau) as tests.twin_np's, then {critic: plain | twin | min, floor,
# weighted (importance weights on the critic's side: the twin restatement carries them; the actor's term takes none)}.  tests.helpers.host_case's numbers (twin: tests.twin_np.host_case's; min: tests.actor_min_np.case_inputs', head 2 balanced).
# 8x8x6 is the smallest image the conv trunk takes; 5 and 7 rows: a partial wave; "lowdim28" is the 28-element state of the kernel test, whose
# B = 65 minibatches carry Q of both signs and cross the wave boundary.  clip 0.5 engages the clip on both lists, 1e4 on neither.
SHAPES = {"8x8x6": (8, 8, 3, 1, 2), "16x16x6": (16, 16, 3, 1, 2), "lowdim28": (28,), "64x64x18": (64, 64, 3, 2, 3)}
ROWS, NB = 24, 3
SM = W.SMOOTHING
CASES = (("A1-B5-sgd", "8x8x6", 1, 5, "gradient-descent", 1, None, 0.5, 0.25, {}),
         ("A2-B7-adam-clipped", "8x8x6", 2, 7, "adam", 1, None, 0.5, 0.25, {}),
         ("A8-B5-adam-unclipped", "8x8x6", 8, 5, "adam", 1, None, 1e4, 0.25, {}),
         ("A2-B5-floor", "8x8x6", 2, 5, "gradient-descent", 1, None, 0.5, 0.25, {"floor": HIGH_FLOOR}),
         ("A2-B7-delay2", "8x8x6", 2, 7, "momentum-0.5", 2, None, 0.5, 0.25, {}),
         ("A2-B5-smoothed", "8x8x6", 2, 5, "gradient-descent", 1, SM, 0.5, 0.25, {}),
         ("A2-B7-weighted", "8x8x6", 2, 7, "gradient-descent", 1, None, 0.5, 0.25, {"critic": "twin", "weighted": True}),
         ("A2-B5-twin", "8x8x6", 2, 5, "gradient-descent", 1, None, 0.5, 0.25, {"critic": "twin"}),
         ("A2-B7-twin-min", "8x8x6", 2, 7, "gradient-descent", 1, None, 0.5, 0.25, {"critic": "min"}),
         ("A2-B8-16x16x6", "16x16x6", 2, 8, "gradient-descent", 1, None, 0.5, 0.25, {}),
         ("lowdim-A3-B5", "lowdim28", 3, 5, "gradient-descent", 1, None, 0.5, 0.25, {}),
         ("lowdim-A2-B65-mixed", "lowdim28", 2, 65, "gradient-descent", 1, None, 0.5, 0.25, {}),
         ("lowdim-A3-B7-td3-min", "lowdim28", 3, 7, "adam", 2, SM, 0.5, 0.25, {"critic": "min"}),
         ("64x64x18-B8-td3", "64x64x18", 2, 8, "adam", 2, SM, 0.5, 0.25, {"critic": "twin"}))
BIG = ("64x64x18-B8-td3",)      # (the offline TD3 stack at the flagship's geometry: one minibatch pair on the device, not part of the fault sweep)
# host_case seeds: per case the first of 1, 2, ... on which every condition of tests/test_bc_host.py holds (A1-B5-sgd: on seed 1 the third
# minibatch's m is 0.017; lowdim-A3-B7-td3-min: on seed 1 head 1 is followed on one row of seven in the third minibatch)
SEEDS = dict({c[0]: 1 for c in CASES}, **{"A1-B5-sgd": 2, "lowdim-A3-B7-td3-min": 2})


def case_of(cid):
    return [c for c in CASES if c[0] == cid][0]


def hyper_of(case):
    return W.hyper_of(case[:9])


def floor_of(case):
    return case[9].get("floor", Q_FLOOR)


def rows_of(case):
    return max(ROWS, 2 * case[3])


def restatement(case, specs, P, dt=np.float64, fault=None):
    _cid, _sn, _A, _B, opt, d, sm, _clip, _tau, extra = case
    name, args = T3.OPTIMISERS[opt]
    cls = {"plain": BcDDPG, "twin": BcTwinDDPG, "min": BcMinTwinDDPG}[extra.get("critic", "plain")]
    ref = cls(specs[0], specs[1], P[0], P[1], dt, hyper_of(case), name, args, d, sm, alpha=ALPHA, q_floor=floor_of(case), bc_fault=fault)
    ref.set_targets(P[2], P[3])
    return ref


def case_inputs(case, seed=None, nb=NB):
    from tests.helpers import host_case
    cid, shape_name, A, B, _opt, _d, _sm, _clip, _tau, extra = case
    seed = SEEDS[cid] if seed is None else seed
    kind = extra.get("critic", "plain")
    if kind == "plain":
        return host_case(SHAPES[shape_name], B, nb, seed, rows=rows_of(case), action_dim=A)
    specs, P, episodes, idxs, batches = W.host_case(SHAPES[shape_name], B, nb, seed, rows=rows_of(case), action_dim=A)
    if kind == "min":      # head 2's online bias balanced as tests.actor_min_np.case_inputs balances it
        ref = restatement(case, specs, P)
        diffs = []
        for b in batches:
            ref.fed = b[1]
            ag = ref.actor_gradients(b[0])
            diffs.append((ag["q1"] - ag["q2"]).ravel())
        P[1][-1] += AM.midpoint_shift(np.concatenate(diffs))
    return specs, P, episodes, idxs, batches


def case_weights(case, nb=NB):
    return W.case_weights(case[:9], nb) if case[9].get("weighted") else None


def run_case(case, inputs, dt=np.float64, fault=None, weights=None, probe=()):
    """NB calls of one minibatch, the target update behind each (what the GPU test runs): (the six vectors, per-minibatch actor outputs,
    per-minibatch critic outputs, per-minibatch step outputs, the restatement, {fault: [actor outputs] per minibatch} for the faults in
    `probe`, each taken on the minibatch's starting state beside the unfaulted pass)"""
    specs, P, _ep, _idxs, batches = inputs
    ref = restatement(case, specs, P, dt, fault)
    ags, cgs, outs, probed = [], [], [], {f: [] for f in probe}
    for k, b in enumerate(batches):
        ref.weights = None if weights is None else weights[k]
        ref.fed = b[1]
        for f in probe:
            ref.bc_fault = f
            probed[f].append(ref.actor_gradients(b[0]))
        ref.bc_fault = fault
        outs.append(ref.train_minibatch(b))
        ags.append(ref.last_ag)
        cgs.append(ref.last_cg)
        ref.update_targets()
    return W.vectors(ref), ags, cgs, outs, ref, probed


def seen(ag, bad, A):
    """by how many bars the GPU test's comparisons of one minibatch's actor pass would see `bad` beside `ag`: the largest of the ratios on
    lambda, g, the reported dq_da and the actor's pre-clip list (rel 2e-5)"""
    lam, m = ag["lambda"], ag["m"]
    r = [abs(bad["lambda"] - lam) / lambda_bar(lam, m),
         float((np.abs(bad["g"] - ag["g"]) / g_bar(lam, m, ag["dq_da"], A)).max()),
         float(np.abs(bad["dq_da"] - ag["dq_da"]).max()) / P_BAR,
         float(np.linalg.norm(bad["grads"] - ag["grads"]) / (2e-5 * np.linalg.norm(ag["grads"])))]
    return max(r)
