"""Pooled twin quantile critics (Truncated Quantile Critics, Kuznetsov et al. 2020, with two heads on one representation;
include/cartpolepp_abi.h, cpp_net_create_pooled_quantile) restated in numpy, in float64 and float32:

    theta^k_i  = atom i of online head k at (s1, a_fed), k = 1, 2, i < N;  tau_i = (2 i + 1) / (2 N)
    z          = (theta'^1_0 .. theta'^1_{N-1}, theta'^2_0 .. theta'^2_{N-1}): both target heads at (s2, a'), ONE a' (smoothed, or SAC's sample)
    s          = z sorted ascending (2N values, always sorted, also at d = 0);  M = 2N - 2d;  g = mask discount
    y_j        = r* + g s_j, j < M;   r* = r, or r_soft under SAC
    u^k_ij     = y_j - theta^k_i;  H(u) = u^2 / 2 if |u| <= kappa else kappa (|u| - kappa / 2);  rho = |tau_i - [u < 0]| H(u) / kappa
    L^k_b      = (1 / (N M)) sum_i sum_j rho^k_ij;   L_b = L^1_b + L^2_b;   loss = mean_b(w_b L_b)
    d theta^k_i = -(w_b / B) (1 / (N M)) sum_j |tau_i - [u^k_ij < 0]| clip(u^k_ij, -kappa, kappa) / kappa
    Q_k = (sum_i theta^k_i) / N;   Qbar = (Q_1 + Q_2) / 2
    td_b = Q_1 - (sum_{j<M} y_j) / M;   td2_b = Q_2 - the same mean
    actor: ascends Qbar(s1, mu(s1)) -- dz of BOTH q layers is 1 / (2N);  dq_da = dQbar/da;  under SAC alpha logp - Qbar

The critic is tests.twin_np.TwinCritic over tests.quant_np.quant_spec (both q layers N wide).  Two learners: PoolDDPG, a subclass of
tests.twin_np.TwinDDPG (the optimisers, target policy smoothing, the policy delay, importance weights and n-step columns compose with
it), and PoolSac, a subclass of tests.sac_np.ComposedSac.  Also a float32 variant of the row functions that follows the device's order
(csrc/quant_pool.hip: lane l < N holds target head 1's atom l, lane N <= l < 2N target head 2's atom l - N, +inf beyond; xor butterflies,
the bitonic network, j ascending, every product and sum rounded on its own), the cases the CPU and the GPU tests share, their
conditions, and the faults the CPU test plants.  Test-only: product code never imports it."""
import numpy as np

from oracle import ddpg_np as O
from tests import ddpg_opt_np as R
from tests import quant_np as Q
from tests import sac_np as S
from tests import td3_np as T3
from tests import tps_np as T
from tests import twin_np as W

FAULTS = ("truncation_per_head",          # d dropped from the top of each target head, then pooled
          "two_d_read_as_d",              # d atoms of the pool dropped, not 2d
          "target_from_min_of_means",     # y = r + g min(Q_1', Q_2'): the twin scalar target
          "target_head1_only",            # the target from head 1's atoms alone (its d largest dropped)
          "pool_not_sorted",              # the first M atoms of the pool as the heads emit them
          "normaliser_2nm",               # 1 / (2 N M) in loss and gradient
          "tau_over_2n",                  # tau_i = (2 i + 1) / (4 N): the pool's midpoints on the online heads
          "actor_head1_only",             # the actor ascends Q_1
          "tops_1_over_n",                # both tops 1 / N: the actor ascends Q_1 + Q_2
          "head2_loss_missing",           # loss and gradient from head 1 alone
          "weight_missing_on_head2",      # the importance weight on head 1's loss and gradient only
          "td_from_qbar",                 # td = Qbar - mean y
          "r_not_r_soft",                 # under SAC: the batch's reward where the soft reward belongs
          "two_sampled_actions")          # one a' per target head
SAC_ONLY_FAULTS = ("r_not_r_soft",)
NOISE_FAULTS = ("two_sampled_actions",)   # (a second draw: SAC's sample, or the smoothing's noise)
WEIGHT_FAULTS = ("weight_missing_on_head2",)


# ---- the row functions, any dt ---------------------------------------------------------------------------------------------------------
def taus(n, dt=np.float64, fault=None):
    dt = np.dtype(dt).type
    i = np.arange(n).astype(dt)
    return ((dt(2.0) * i + dt(1.0)) / dt((4 if fault == "tau_over_2n" else 2) * n)).astype(dt)


def pool_target(tt1, tt2, r, g, drop, dt=np.float64, fault=None):
    """(s, y, from1): the pool sorted ascending (B, 2N), y_j = r + g s_j over the kept atoms (B, M), and per row how many of the 2d dropped
    atoms are target head 1's"""
    tt1, tt2 = np.asarray(tt1, dt), np.asarray(tt2, dt)
    n, d = tt1.shape[1], int(drop)
    assert tt2.shape == tt1.shape and 0 <= d <= n - 1
    z = np.concatenate([tt1, tt2], axis=1)
    order = np.argsort(z, axis=1, kind="stable")
    s = np.take_along_axis(z, order, axis=1)
    m = 2 * n - 2 * d
    from1 = (order[:, m:] < n).sum(axis=1)
    if fault == "truncation_per_head":
        kept = np.sort(np.concatenate([np.sort(tt1, axis=1)[:, :n - d], np.sort(tt2, axis=1)[:, :n - d]], axis=1), axis=1)
    elif fault == "two_d_read_as_d":
        kept = s[:, :2 * n - d]
    elif fault == "target_from_min_of_means":
        kept = np.minimum(tt1.mean(axis=1, keepdims=True), tt2.mean(axis=1, keepdims=True))
    elif fault == "target_head1_only":
        kept = np.sort(tt1, axis=1)[:, :n - d]
    elif fault == "pool_not_sorted":
        kept = z[:, :m]
    else:
        kept = s[:, :m]
    y = (np.asarray(r, dt).reshape(-1, 1) + np.asarray(g, dt).reshape(-1, 1) * kept).astype(dt)
    return s, y, from1


def pair_loss(theta, y, kappa, dt=np.float64, fault=None):
    """(L (B, 1), G (B, N)) of one head: its quantile Huber loss and sum_j |tau_i - [u_ij < 0]| clip(u_ij) / kappa over N M --
    d theta_i = -(w_b / B) G_i"""
    dtt = np.dtype(dt).type
    theta, y = np.asarray(theta, dt), np.asarray(y, dt)
    n, m = theta.shape[1], y.shape[1]
    u = y[:, None, :] - theta[:, :, None]                       # (B, N, M)
    k = np.abs(taus(n, dt, fault)[None, :, None] - (u < 0).astype(dt))
    h, c = Q.huber(u, kappa, dt), np.clip(u, -dtt(kappa), dtt(kappa))
    nm = dtt((2 if fault == "normaliser_2nm" else 1) * n * m)
    L = ((k * h / dtt(kappa)).sum(axis=2).sum(axis=1, keepdims=True) / nm).astype(dt)      # j inside i
    G = ((k * c / dtt(kappa)).sum(axis=2) / nm).astype(dt)
    return L, G, u


def rows(theta1, theta2, tt1, tt2, r, mask, discount, kappa, drop, dt=np.float64, w=None, fault=None):
    """everything the td job of csrc/quant_pool.hip writes per row, in `dt` with numpy's own summation order; y is padded with zeros to
    (B, 2N); dz1 / dz2 carry w_b / B"""
    dtt = np.dtype(dt).type
    theta1, theta2 = np.asarray(theta1, dt), np.asarray(theta2, dt)
    B, n = theta1.shape
    g = (np.asarray(mask, dt).reshape(-1, 1) * dtt(discount)).astype(dt)
    s, y, from1 = pool_target(tt1, tt2, r, g, drop, dt, fault)
    L1, G1, u1 = pair_loss(theta1, y, kappa, dt, fault)
    L2, G2, u2 = pair_loss(theta2, y, kappa, dt, fault)
    w = np.ones((B, 1), dt) if w is None else np.asarray(w, dt).reshape(B, 1)
    w2 = np.ones_like(w) if fault == "weight_missing_on_head2" else w
    if fault == "head2_loss_missing":
        L2, G2 = np.zeros_like(L2), np.zeros_like(G2)
    q1, q2 = (theta1.sum(axis=1, keepdims=True) / dtt(n)).astype(dt), (theta2.sum(axis=1, keepdims=True) / dtt(n)).astype(dt)
    ym = (y.sum(axis=1, keepdims=True) / dtt(y.shape[1])).astype(dt)
    qtd = ((q1 + q2) / dtt(2.0)).astype(dt) if fault == "td_from_qbar" else q1
    ypad = np.zeros((B, 2 * n), dt)
    ypad[:, :min(y.shape[1], 2 * n)] = y[:, :2 * n]
    return {"theta1": theta1, "theta2": theta2, "sorted": s, "y": ypad, "ykept": y, "q": q1, "q2": q2, "td": (qtd - ym).astype(dt),
            "td2": (q2 - ym).astype(dt), "target_q": np.asarray(tt1, dt).mean(axis=1, keepdims=True),
            "target_q2": np.asarray(tt2, dt).mean(axis=1, keepdims=True), "L1": L1, "L2": L2, "loss": (w * L1 + w2 * L2).mean(dtype=dt),
            "dz1": (-G1 * w / dtt(B)).astype(dt), "dz2": (-G2 * w2 / dtt(B)).astype(dt), "u1": u1, "u2": u2, "from1": from1, "w": w, "g": g}


# ---- the float32 variant: the device's order -------------------------------------------------------------------------------------------
_butterfly, _lanes, _butterfly64, bitonic_sort = Q._butterfly, Q._lanes, Q._butterfly64, Q.bitonic_sort


def pool_lanes(tt1, tt2):
    """(B, 64): lane l < N target head 1's atom l, lane N <= l < 2N target head 2's atom l - N, +inf beyond"""
    return _lanes(np.concatenate([np.asarray(tt1, np.float32), np.asarray(tt2, np.float32)], axis=1), np.inf)


def rows_f32(theta1, theta2, tt1, tt2, r, mask, discount, kappa, drop, w=None):
    """rows() in float32, operation by operation as the td job of csrc/quant_pool.hip"""
    f = np.float32
    th1_in, th2_in = np.asarray(theta1, np.float32), np.asarray(theta2, np.float32)
    B, n = th1_in.shape
    assert 2 <= n <= 32
    m = 2 * n - 2 * int(drop)
    lane = np.arange(64)
    on, on2, kept = (lane < n)[None, :], ((lane >= n) & (lane < 2 * n))[None, :], (lane < m)[None, :]
    th = [_lanes(th1_in, 0.0), _lanes(th2_in, 0.0)]
    z = pool_lanes(tt1, tt2)
    tq1 = (_butterfly(np.where(on, z, f(0)), np.add) / f(n)).astype(np.float32)
    tq2 = (_butterfly(np.where(on2, z, f(0)), np.add) / f(n)).astype(np.float32)
    s = bitonic_sort(z)
    q = [(_butterfly(t, np.add) / f(n)).astype(np.float32) for t in th]
    r = np.asarray(r, np.float32).reshape(-1, 1)
    g = (np.asarray(mask, np.float32).reshape(-1, 1) * f(discount)).astype(np.float32)
    with np.errstate(invalid="ignore"):
        y = np.where(kept, (r + (g * s).astype(np.float32)).astype(np.float32), f(0)).astype(np.float32)
    ym = (_butterfly(y, np.add) / f(m)).astype(np.float32)
    tau = ((2 * lane + 1).astype(np.float32) / f(2 * n)).astype(np.float32)[None, :]
    kap, kd = f(kappa), float(f(kappa))
    gs = [np.zeros((B, 64), np.float32), np.zeros((B, 64), np.float32)]
    ls = [np.zeros((B, 64), np.float64), np.zeros((B, 64), np.float64)]
    for j in range(m):
        for h in range(2):
            u = (y[:, j:j + 1] - th[h]).astype(np.float32)
            k = np.abs((tau - np.where(u < 0, f(1), f(0))).astype(np.float32))
            c = np.minimum(np.maximum(u, -kap), kap)
            gs[h] = (gs[h] + (k * c).astype(np.float32)).astype(np.float32)
            ud = u.astype(np.float64)
            au = np.abs(ud)
            ls[h] = ls[h] + k.astype(np.float64) * np.where(au <= kd, 0.5 * ud * ud, kd * (au - 0.5 * kd))
    L = [_butterfly64(np.where(on, x, 0.0)) / (kd * (float(n) * float(m))) for x in ls]
    inv_b, inv_nm = f(1.0) / f(B), f(1.0) / f(n * m)
    dz = []
    for h in range(2):
        d = (-((gs[h] / kap).astype(np.float32) * inv_nm).astype(np.float32)).astype(np.float32)
        if w is not None:
            d = (d * np.asarray(w, np.float32).reshape(-1, 1)).astype(np.float32)
        dz.append((d * inv_b).astype(np.float32)[:, :n])
    wd = np.ones((B, 1)) if w is None else np.asarray(w, np.float32).astype(np.float64).reshape(B, 1)
    wl = wd * L[0] + wd * L[1]                                  # head 1's row loss before head 2's
    parts = [sum(float(x) for x in wl[i:i + 4, 0]) for i in range(0, B, 4)]      # a workgroup's four rows in order, the partials in order
    loss = np.float32(sum(parts) / float(B))
    return {"theta1": th[0][:, :n], "theta2": th[1][:, :n], "sorted": s[:, :2 * n], "y": y[:, :2 * n], "q": q[0], "q2": q[1],
            "td": (q[0] - ym).astype(np.float32), "td2": (q[1] - ym).astype(np.float32), "target_q": tq1, "target_q2": tq2, "L1": L[0], "L2": L[1],
            "loss": loss, "dz1": dz[0], "dz2": dz[1]}


# ---- the critic's two sides, shared by both learners ----------------------------------------------------------------------------------
def dqbar_da(critic, c, dt, fault=None):
    """dQbar/da of a cached forward of a TwinCritic with N-wide q layers: 1 / (2N) into both q layers, the action columns of both
    heads' concat layers added, head 1's first"""
    n = c["out"].shape[1]
    A, n_in = critic.spec.action_dim, critic.spec.fc[critic.k][1]
    top = dt(1.0) / dt(n if fault in ("tops_1_over_n", "actor_head1_only") else 2 * n)
    dh1 = critic._tail(critic.h1.p, "", c["fc"][critic.k:], np.full_like(c["out"], top), None)
    if fault == "actor_head1_only":
        return dh1[:, n_in - A:]
    dh2 = critic._tail(critic.p2, "b", c["fc2"], np.full_like(c["out2"], top), None)
    return (dh1[:, n_in - A:] + dh2[:, n_in - A:]).astype(dt)


def actor_side(ref, cc, fault=None):
    """{q, q2, dq_da} of the critic's evaluation at the actor's action"""
    dt = ref.dt
    n = cc["out"].shape[1]
    return {"q": (cc["out"].sum(axis=1, keepdims=True) / dt(n)).astype(dt), "q2": (cc["out2"].sum(axis=1, keepdims=True) / dt(n)).astype(dt),
            "dq_da": dqbar_da(ref.critic, cc, dt, fault)}


def critic_side(ref, batch, at, at2, r_star, w, w2_white, training, fault=None):
    """the pooled target at the target action `at` (at2: head 2's own action, the fault two_sampled_actions; None: the same), both heads'
    losses and the critic's gradient list"""
    s1, a, _r, mask, s2 = batch
    dt = ref.dt
    _n, kappa, drop = ref.pool
    tq = ref.target_critic.forward(s2, action=at, white=w2_white, training=training)
    tt1, tt2 = tq["out"], tq["out2"]
    if at2 is not None:
        tt2 = ref.target_critic.forward(s2, action=at2, white=w2_white, training=training)["out2"]
    cb = ref.critic.forward(s1, action=np.asarray(a, dt), training=training)
    out = rows(cb["out"], cb["out2"], tt1, tt2, r_star, mask, ref.hp.discount, kappa, drop, dt, w, fault)
    grads, _ = ref.critic.backward(cb, out["dz1"], out["dz2"])
    out.update(cache_critic=cb, grads=W.flatten_grads(ref.critic.spec, grads, dt), target_theta1=tt1, target_theta2=tt2)
    return out


class PoolDDPG(W.TwinDDPG):
    """the deterministic learner (TD3 with a pooled truncated target).  pool: (N, kappa, d per head)"""

    def __init__(self, actor_spec, critic_spec, actor_flat, critic_flat, pool, dt=np.float64, hyper=O.DEFAULT_HYPER,
                 optimiser="GradientDescent", optimiser_args=None, delay=1, smoothing=None, fault=None):
        assert fault is None or fault in FAULTS, fault
        assert critic_spec.fc[-1][2] == pool[0] and 0 <= pool[2] <= pool[0] - 1
        super(PoolDDPG, self).__init__(actor_spec, critic_spec, actor_flat, critic_flat, dt, hyper, optimiser, optimiser_args, delay, smoothing, None)
        self.pool, self.pool_fault = (int(pool[0]), float(np.float32(pool[1])), int(pool[2])), fault

    def actor_gradients(self, s1):
        w1 = self._white(self.actor, s1)
        ca = self.actor.forward(s1, white=w1)
        cc = self.critic.forward(s1, action=ca["out"], white=w1)
        side = actor_side(self, cc, self.pool_fault)
        grads, _ = self.actor.backward(ca, -side["dq_da"])
        self.last_ag = dict(side, actions=ca["out"], grads=O.flatten(self.actor.spec, grads, self.dt), cache_actor=ca)
        return self.last_ag

    def critic_gradients(self, batch, noise="draw", training=True, w=None):
        """noise: 'draw' (the smoothing of the restatement, if any: one draw, the count advances), None, or a (B, A) array.
        w: (B, 1) importance weights (default: self.weights, else uniform)"""
        s1, a, r, mask, s2 = batch
        dt, fault = self.dt, self.pool_fault
        act = np.asarray(a)
        B, A = act.shape[0], act.shape[1]
        noise2 = None
        if isinstance(noise, str):
            noise = None
            if self.smoothing is not None and training:
                sigma, clip, seed = self.smoothing
                noise = T.target_noise(seed, self.tps_n, B, A, sigma, clip, np.float64)
                self.tps_n += 1
        if noise is not None and fault == "two_sampled_actions":
            sigma, clip, seed = self.smoothing
            noise2 = T.target_noise(seed + 1, max(self.tps_n - 1, 0), B, A, sigma, clip, np.float64)
        w = self.weights if w is None else w
        w2 = self._white(self.target_actor, s2)
        ta = self.target_actor.forward(s2, white=w2, training=training)

        def smoothed(n):
            return ta["out"] if n is None else np.clip((ta["out"] + np.asarray(n, dt)).astype(dt), dt(-1.0), dt(1.0))
        out = critic_side(self, batch, smoothed(noise), None if noise2 is None else smoothed(noise2), r, w, w2, training, fault)
        out.update(target_actions=ta["out"], smoothed_actions=smoothed(noise), noise=noise)
        self.last_cg = out
        return out

    def check_loss(self, batch):
        out = self.critic_gradients(batch, noise=None, training=False, w=np.ones((np.asarray(batch[1]).shape[0], 1)))
        return out["loss"], out["td"], out["q"]

    def train_minibatch(self, batch, noise="draw", weights=None, routes=None):
        """both gradient sets from one snapshot, then both applies (the actor's list held by the policy delay's rule)"""
        if routes is not None:
            self.actor.amax_override, self.critic.amax_override, self.actor.relu_override, self.critic.relu_override = routes
        self.weights = None if weights is None else np.asarray(weights, self.dt).reshape(-1, 1)
        ag = self.actor_gradients(batch[0])
        cg = self.critic_gradients(batch, noise=noise)
        self.n += 1
        applied = self._applies(self.n)
        self.held = not applied
        a_norm = self._actor(ag["grads"], applied)
        c_norm = self._apply("critic", cg["grads"])
        out = {"actor_grads": ag["grads"], "critic_grads": cg["grads"], "actor_norm": float(a_norm), "critic_norm": float(c_norm),
               "applied": applied, "cache_actor": ag["cache_actor"], "cache_critic": cg["cache_critic"], "actions": ag["actions"],
               "dq_da": ag["dq_da"], "q_mu": ag["q"], "q2_mu": ag["q2"], "target_actions": cg["smoothed_actions"]}
        out.update({k: cg[k] for k in ROW_KEYS + ("loss", "from1", "u1", "u2", "ykept", "target_theta1", "target_theta2")})
        out["loss"] = float(out["loss"])
        return out

    def set_state(self, vec):
        dt = self.dt
        self.actor, self.target_actor = O.Net(self.actor.spec, np.asarray(vec["actor"], dt), dt), O.Net(self.actor.spec, np.asarray(vec["target_actor"], dt), dt)
        self.critic = W.TwinCritic(self.critic.spec, np.asarray(vec["critic"], dt), dt)
        self.target_critic = W.TwinCritic(self.critic.spec, np.asarray(vec["target_critic"], dt), dt)
        na = len(self.slots["actor"].m)
        for which, sl in (("actor", slice(0, na)), ("critic", slice(na, None))):
            self.slots[which].m, self.slots[which].v = np.asarray(vec["m"][sl], dt).copy(), np.asarray(vec["v"][sl], dt).copy()
        self.slots["actor"].t, self.slots["critic"].t = (int(t) for t in vec["step"])
        self.n, self.tps_n = int(vec["n"]), int(vec["n"])

    def vectors(self):
        f = lambda v: np.asarray(v, np.float64)
        return {"actor": f(self.actor.flat()), "critic": f(self.critic.flat()), "target_actor": f(self.target_actor.flat()),
                "target_critic": f(self.target_critic.flat()),
                "m": np.concatenate([f(self.slots[w].m) for w in R.LISTS]), "v": np.concatenate([f(self.slots[w].v) for w in R.LISTS]),
                "step": [0 if self.opt[w].kind == "sgd" else int(self.slots[w].t) for w in R.LISTS], "n": int(self.n)}


class PoolSac(S.ComposedSac):
    """soft actor-critic on pooled quantile critics: TQC.  pool: (N, kappa, d per head)"""

    def __init__(self, actor_spec, critic_spec, actor_flat, critic_flat, pool, dt=np.float64, hyper=O.DEFAULT_HYPER, state=None,
                 optimiser="GradientDescent", optimiser_args=None, fault=None):
        assert fault is None or fault in FAULTS, fault
        S.ComposedSac.__init__(self, actor_spec, critic_spec, actor_flat, critic_flat, dt, hyper, state, optimiser, optimiser_args, True, None)
        self.pool, self.pool_fault = (int(pool[0]), float(np.float32(pool[1])), int(pool[2])), fault

    def _dq_da(self, cc):
        return dqbar_da(self.critic, cc, self.dt, self.pool_fault)

    def actor_gradients(self, s1, eps1=None, fault=None, row_scale=None):
        out = S.ComposedSac.actor_gradients(self, s1, eps1, fault, row_scale)
        n = self.pool[0]
        out["q_atoms"], out["q"] = out["q"], (out["q"].sum(axis=1, keepdims=True) / self.dt(n)).astype(self.dt)
        out["q2"] = (out["q2"].sum(axis=1, keepdims=True) / self.dt(n)).astype(self.dt)
        return out

    def critic_gradients(self, batch, eps2=None, training=True, fault=None, weights=None):
        s1, a, r, mask, s2 = batch
        dt, pf = self.dt, self.pool_fault
        alpha = dt(np.exp(np.float64(self.target_log_alpha)))
        w2 = self._white(self.target_actor, s2)
        _c, m, x = self._head(self.target_actor, s2, w2, training)
        eps = np.zeros_like(m) if eps2 is None else np.asarray(eps2, dt)
        pol = S.policy(m, x, eps, self.lo, self.hi, dt, fault)
        at2 = None
        if pf == "two_sampled_actions":      # (head 2's a' from the draw of state_1's stream)
            B, A = m.shape
            at2 = S.policy(m, x, S.noise(self.sac.seed, self.sac.n, B, A, S.STREAM_S1), self.lo, self.hi, dt, fault)["a"]
        rs = S.soft_reward(r, mask, self.hp.discount, alpha, pol["logp"], dt, fault).reshape(-1, 1)
        r_star = np.asarray(r, dt).reshape(-1, 1) if pf == "r_not_r_soft" else rs
        out = critic_side(self, batch, pol["a"], at2, r_star, weights, w2, training, pf)
        out.update(target_actions=pol["a"], logp2=pol["logp"], r_soft=rs[:, 0], m2=m, x2=x)
        return out

    def train_critic(self, batch, eps2, weights=None):
        cg = S.ComposedSac.train_critic(self, batch, eps2, weights)
        self.last_cg = cg
        return cg

    def train_actor(self, s1, eps1, weights=None):
        ag = S.ComposedSac.train_actor(self, s1, eps1, weights)
        self.last_ag = ag
        return ag


ROW_KEYS = ("theta1", "theta2", "sorted", "y", "q", "q2", "td", "td2", "target_q", "target_q2")


def sac_outputs(ref, out):
    """ComposedSac.train_minibatch's outputs with the pooled rows beside them"""
    out = dict(out)
    out.update({k: ref.last_cg[k] for k in ROW_KEYS + ("from1", "u1", "u2", "ykept", "target_theta1", "target_theta2")})
    out.update(q_mu=ref.last_ag["q"], q2_mu=ref.last_ag["q2"], applied=True)
    return out


# ---- the cases.  Low-dimensional networks with hidden widths 8 unless a geometry is named; tests.helpers.host_case's episodes and rows
# (rewards 0, 1, 2, every episode ends in a terminal row); parameters from a stream of their own: xavier + 0.05, both q layers as
# tests.quant_np.q_value_tail draws them (weights scaled up, biases spread over the scale of the returns: the atoms are far from sorted, the two
# heads interleave, and the u fall on both sides of kappa), targets 0.01 away.
SHAPES = {"lowdim": (2, 2, 7), "8x8x6": (8, 8, 3, 1, 2), "64x64x18": (64, 64, 3, 2, 3)}
HIDDEN = (8, 8)
ROWS, NB = 24, 3
# the one stack at 64x64x18: SAC on a shared encoder behind a feature layer norm (tanh), the u8 store, random shift 4 -- tests.layer_norm_np's
# and tests.shared_encoder_np's mix-ins around PoolSac, the default actor stack (100, 100, 50), two minibatches
STACK, STACK_HIDDEN, STACK_NB, STACK_SHIFT = "64x64x18", (100, 100, 50), 2, (4, 3)          # shape, hidden, minibatches, (pad, seed)
SMOOTHING = (0.2, 0.5, 0x7C)          # sigma, clip, seed
TEMPERATURE, TEMPERATURE_LR, NOISE_SEED, DISCOUNT = 0.2, 1e-2, 0x79C, 0.9
PER = S.PER
CLIP_SIDE_FACTOR = 1.2
# (id, form, shape, A, B, N, d, kappa, optimiser, clip, tau, delay, smoothing, weighted, n_step, sides of the clip (actor, critic) or None)
CASES = (("A1-B5-N25-d2-sgd", "td3", "lowdim", 1, 5, 25, 2, 1.0, "gradient-descent", 0.5, 0.25, 1, None, False, 1, None),
         ("A2-B8-N25-d2-sgd", "td3", "lowdim", 2, 8, 25, 2, 1.0, "gradient-descent", 0.5, 0.25, 1, None, False, 1, None),
         ("A9-B7-N32-d1-sgd", "td3", "lowdim", 9, 7, 32, 1, 1.0, "gradient-descent", 0.5, 0.25, 1, None, False, 1, None),
         ("A2-B8-N25-d2-adam-clipped", "td3", "lowdim", 2, 8, 25, 2, 1.0, "adam", 0.05, 0.25, 1, None, False, 1, ("above", "above")),
         ("A2-B8-N25-d2-adam-unclipped", "td3", "lowdim", 2, 8, 25, 2, 1.0, "adam", 1e4, 1.0, 1, None, False, 1, ("below", "below")),
         ("A2-B8-N5-d1-smoothed-delay2", "td3", "lowdim", 2, 8, 5, 1, 1.0, "adam", 0.5, 0.25, 2, SMOOTHING, False, 1, None),
         ("A2-B8-N25-d2-per-nstep3", "td3", "lowdim", 2, 8, 25, 2, 1.0, "momentum-0.5", 0.5, 0.25, 1, None, True, 3, None),
         ("A2-B5-N25-d2-8x8x6", "td3", "8x8x6", 2, 5, 25, 2, 1.0, "gradient-descent", 0.5, 0.25, 1, None, False, 1, None),
         ("sac-A2-B8-N25-d2-adam", "sac", "lowdim", 2, 8, 25, 2, 1.0, "adam", 0.5, 0.25, 1, None, False, 1, None),
         ("sac-A9-B7-N25-d2-adam", "sac", "lowdim", 9, 7, 25, 2, 1.0, "adam", 0.5, 0.25, 1, None, False, 1, None),
         ("sac-drq-64x64x18-A2-B8-N25-d2-adam", "sac", STACK, 2, 8, 25, 2, 1.0, "adam", 0.5, 0.25, 1, None, False, 1, None))
# case_inputs' seeds: per case the first of 1, 2, ... on which every compared minibatch meets conditions() (tests/test_pooled_quantile_host.py
# asserts it; a case that fails is given another seed, never a relaxed condition)
SEEDS = dict({c[0]: 1 for c in CASES}, **{"A2-B8-N5-d1-smoothed-delay2": 2})


def case_of(cid):
    return [c for c in CASES if c[0] == cid][0]


def is_stack(case):
    return case[2] == STACK


def nb_of(case):
    return STACK_NB if is_stack(case) else NB


def pool_of(case):
    return (case[5], case[7], case[6])          # (N, kappa, d per head)


def hyper_of(case):
    return T3.hyper_of(case[8], case[9], case[10])._replace(discount=DISCOUNT)


def specs_of(case):
    _cid, form, shape_name, A = case[:4]
    shape = SHAPES[shape_name]
    pixel = len(shape) == 5
    kw = dict(pixel=True, H=shape[0], W=shape[1], C=int(np.prod(shape[2:]))) if pixel else dict(pixel=False, state_elems=int(np.prod(shape)))
    if is_stack(case):
        from tests import layer_norm_np as L, shared_encoder_np as SE
        aspec, cspec = L.specs_for(shape, STACK_HIDDEN, "tanh", A)
        name, n_in, _n_out, _act, cat = aspec.fc[-1]
        aspec.fc[-1] = (name, n_in, 2 * int(A), "linear", cat)          # (m | x), as tests.sac_np.gaussian_spec's
        return SE.shared_actor_spec(aspec), Q.quant_spec(cspec, case[5])
    aspec = S.gaussian_spec(A, HIDDEN, **kw) if form == "sac" else O.NetSpec("actor", A, HIDDEN, **kw)
    return aspec, Q.quant_spec(O.NetSpec("critic", A, HIDDEN, **kw), case[5])


def _perturb(spec, p, rng, sd, pick):
    """N(0, sd) on the variables of `p` (spec.layout()'s order) whose name `pick` accepts"""
    off = 0
    for name, shape in spec.layout():
        n = int(np.prod(shape))
        if pick(name):
            p[off:off + n] += rng.normal(0, sd, n).astype(np.float32)
        off += n


def _params(specs, N, form, A, seed):
    """the restatement's order: the critic is [plain (| gamma beta) | twin variables] (tests.twin_np.full_layout)"""
    rng = np.random.default_rng(9000 + seed)
    aspec, cspec = specs
    norm = hasattr(cspec, "ln_names")
    if norm:
        from tests import layer_norm_np as L
    pa = (L.init_params if norm else O.init_params)(aspec, rng)
    pa = pa + rng.normal(0, 0.05, pa.shape).astype(np.float32)
    if form == "sac":
        _perturb(aspec, pa, rng, S.HEAD_PERTURBATION, lambda name: name.startswith("output_action/"))
    pc = (L.init_params if norm else O.init_params)(cspec, rng)
    pc = pc + rng.normal(0, 0.05, pc.shape).astype(np.float32)
    if norm:      # gamma around 1, beta around 0: both carry signal
        _perturb(aspec, pa, rng, 0.1, lambda name: "/LayerNorm/" in name)
        _perturb(cspec, pc, rng, 0.1, lambda name: "/LayerNorm/" in name)
    pc = np.concatenate([pc, W.twin_tail(cspec, rng)[0]])
    pt = pc + rng.normal(0, 0.01, pc.shape).astype(np.float32)
    _name, n_in, _n, _a, _c = cspec.fc[-1]
    cut = n_in * N + N
    n1 = cspec.num_plain() if norm else cspec.num_params()
    for lo in (n1 - cut, len(pc) - cut):          # q_value, then q_valueb: each its own draw
        on, tg = Q.q_value_tail(cspec, N, rng)
        pc[lo:lo + cut], pt[lo:lo + cut] = on, tg
    ta = pa.copy() if form == "sac" else pa + rng.normal(0, 0.01, pa.shape).astype(np.float32)
    return [pa, pc, ta, pt]


def critic_to_device(case, specs, v):
    """a critic-shaped vector (parameters, a gradient list, a slot) from the restatement's order into the device's, [plain | twin | gamma beta]"""
    if not is_stack(case):
        return np.asarray(v)
    from tests import layer_norm_np as L
    return L.twin_to_device(specs[1], np.asarray(v))


def critic_from_device(case, specs, v):
    if not is_stack(case):
        return np.asarray(v)
    from tests import layer_norm_np as L
    return L.twin_from_device(specs[1], np.asarray(v))


def shifted(batch, k):
    """minibatch k of the stack's memory: the k-th augmented gather (tests.shift_np)"""
    from tests import shift_np
    s1, a, r, m, s2 = batch
    sh = shift_np.shifts(STACK_SHIFT[1], k, np.asarray(a).shape[0], STACK_SHIFT[0])
    return (shift_np.shift_images(s1, sh[0]), a, r, m, shift_np.shift_images(s2, sh[1]))


def case_inputs(case, seed=None, nb=None):
    """(specs, P, episodes, idxs, batches): P = [actor, critic + twin variables, target actor, target critic + twin variables]"""
    from tests.helpers import host_case as plain_case
    from tests import dist_np as DN
    cid, form, shape_name, A, B, N = case[:6]
    seed = SEEDS[cid] if seed is None else seed
    nb = nb_of(case) if nb is None else nb
    shape = SHAPES[shape_name]
    _specs, _P, episodes, idxs, batches = plain_case(shape, B, nb, seed, rows=ROWS, action_dim=A)
    specs = specs_of(case)
    if case[14] > 1:
        batches = DN.n_step_batches(shape, episodes, ROWS, idxs, B, A, case[14], DISCOUNT)
    if is_stack(case):
        batches = [shifted(b, k) for k, b in enumerate(batches)]
    return specs, _params(specs, N, form, A, seed), episodes, idxs, batches


def batches_of(case, episodes, rows):
    """the minibatches the rows select, on the case's memory (one-step or n-step)"""
    from tests import dist_np as DN
    _cid, _form, shape_name, A, B = case[:5]
    return DN.n_step_batches(SHAPES[shape_name], episodes, ROWS, np.asarray(rows), len(rows), A, case[14], DISCOUNT)


def restatement(case, inputs, dt=np.float64, fault=None):
    specs, P = inputs[0], inputs[1]
    name, args = T3.OPTIMISERS[case[8]]
    if case[1] == "sac":
        cls = PoolSac
        if is_stack(case):
            from tests import layer_norm_np as L, shared_encoder_np as SE
            cls = SE.with_shared_encoder(L.with_feature_norm(PoolSac))
        ref = cls(specs[0], specs[1], P[0], P[1], pool_of(case), dt, hyper_of(case),
                      S.SacState(TEMPERATURE, -float(case[3]), TEMPERATURE_LR, NOISE_SEED), name, args, fault)
        ref.set_target_critic(P[3])
        return ref
    ref = PoolDDPG(specs[0], specs[1], P[0], P[1], pool_of(case), dt, hyper_of(case), name, args, case[11], case[12], fault)
    ref.set_targets(P[2], P[3])
    return ref


def initial_state(case, inputs):
    P = inputs[1]
    n = len(P[0]) + len(P[1])
    f = lambda v: np.asarray(v, np.float64)
    out = {"actor": f(P[0]), "critic": f(P[1]), "target_actor": f(P[2]), "target_critic": f(P[3]), "m": np.zeros(n), "v": np.zeros(n),
           "step": [0, 0], "n": 0}
    if case[1] == "sac":
        out.update(log_alpha=float(np.float32(np.log(np.float32(TEMPERATURE)))), alpha_m=0.0, alpha_v=0.0, alpha_step=0)
    return out


def case_noise(case, k):
    """what a minibatch's restated draws are: (eps1, eps2) under SAC, the smoothing's clipped noise (or None) otherwise"""
    A, B = case[3], case[4]
    if case[1] == "sac":
        return S.noise(NOISE_SEED, k, B, A, S.STREAM_S1), S.noise(NOISE_SEED, k, B, A, S.STREAM_S2)
    if case[12] is None:
        return None
    sigma, clip, seed = case[12]
    return T.target_noise(seed, k, B, A, sigma, clip, np.float64)


def step(ref, case, batch, k, noise=None, weights=None, routes=None, start=None):
    """one minibatch and the target update behind it, from `start` (vectors() of another run) if given: (outputs, vectors())"""
    if start is not None:
        ref.set_state(start)
    if case[1] == "sac":
        ref.sac.n = k
        e1, e2 = noise if noise is not None else case_noise(case, k)
        out = sac_outputs(ref, ref.train_minibatch(batch, e1, e2, weights=weights, routes=routes))
    else:
        ref.n = ref.tps_n = k
        z = noise if noise is not None else case_noise(case, k)
        out = ref.train_minibatch(batch, noise=z, weights=weights, routes=routes)
    ref.update_targets()
    return out, ref.vectors()


def case_weights(case, nb=NB):
    """importance weights for the weighted case on the host: lognormal, normalised to a maximum of 1 as per.hip's are"""
    rng = np.random.default_rng(79)
    return [(lambda w: (w / w.max()).astype(np.float32))(rng.lognormal(0.0, 1.0, (case[4], 1))) for _k in range(nb)]


def run_case(case, inputs, dt=np.float64, fault=None, states=None, weights=None):
    """the case's minibatches, one per outer step; states: per minibatch the vectors() that minibatch k + 1 starts from"""
    ref = restatement(case, inputs, dt, fault)
    outs, vecs = [], []
    if weights is None and case[13]:
        weights = case_weights(case, len(inputs[4]))
    for k, b in enumerate(inputs[4]):
        o, v = step(ref, case, b, k, weights=None if weights is None else weights[k], start=None if states is None or k == 0 else states[k - 1])
        outs.append(o)
        vecs.append(v)
    return outs, vecs, ref


# ---- the conditions every compared minibatch meets on the float64 restatement (tests/test_pooled_quantile_host.py asserts them; the GPU
# test asserts them again on what the device ran)
def conditions(case, out):
    """{name: (value, floor)}: the share of rows whose 2d dropped atoms are NOT d from each head (d > 0), each target head's share of the
    kept atoms, and per online head the share of u on either side of kappa"""
    N, d, kappa = case[5], case[6], float(np.float32(case[7]))
    res = {}
    if d > 0:
        res["rows_not_d_per_head"] = (float((np.asarray(out["from1"]) != d).mean()), 0.25)
    kept1 = N - np.asarray(out["from1"], np.float64)
    M = 2 * N - 2 * d
    res["kept_share_head1"] = (float(kept1.sum() / (M * len(kept1))), 0.25)
    res["kept_share_head2"] = (1.0 - res["kept_share_head1"][0], 0.25)
    for h in ("u1", "u2"):
        au = np.abs(np.asarray(out[h], np.float64))
        res[h + "_quadratic"], res[h + "_linear"] = (float((au <= kappa).mean()), 0.1), (float((au > kappa).mean()), 0.1)
    return res


# ---- the bars of the GPU comparison (tests/test_pooled_quantile_host.py re-measures and asserts these figures): the float32 restatement
# -- the learner evaluated in float32, its atoms through rows_f32 -- against float64, worst over every minibatch of every case from the
# float64 run's states.  Each bar is that figure times 8; where the product is below ATOL / 4 the suite's ordinary ATOL is kept.
ATOL, BAR_FACTOR = 1e-5, 8.0
# Measured (head 1 / head 2): theta 1.74e-6 / 1.78e-6, the sorted pool 2.41e-6, y 2.07e-6 (these three at 64x64x18), Q 3.90e-7 / 3.87e-7, td
# 5.92e-7 / 6.00e-7, the target heads' means 5.16e-7 / 4.82e-7, dQbar/da 3.99e-8, d theta 6.75e-9, a 3.04e-7, a' 3.28e-7.  The two heads are one
# quantity: each pair shares the larger figure.  Bars: theta 1.44e-5, the pool 1.96e-5, y 1.68e-5, Q 3.1e-6, td 4.8e-6, the target means 4.2e-6,
# a and a' 2.7e-6; dQbar/da and d theta 1e-5.
F32_ERR = {"theta1": 1.8e-6, "theta2": 1.8e-6, "sorted": 2.45e-6, "y": 2.1e-6, "q": 3.9e-7, "q2": 3.9e-7, "td": 6.05e-7, "td2": 6.05e-7,
           "target_q": 5.2e-7, "target_q2": 5.2e-7, "dq_da": 4.0e-8, "dz": 6.8e-9, "actions": 3.3e-7, "target_actions": 3.3e-7}
PAIRS = (("theta1", "theta2"), ("q", "q2"), ("td", "td2"), ("target_q", "target_q2"), ("actions", "target_actions"))


def bar(key):
    e = F32_ERR[key]
    return ATOL if BAR_FACTOR * e < ATOL / 4 else BAR_FACTOR * e


def f32_twin_rows(case, out32, batch, weights=None):
    """the float32 learner's atoms through rows_f32: what the device's kernel makes of a float32 forward"""
    _n, kappa, drop = pool_of(case)
    r_star = out32["r_soft"] if case[1] == "sac" else batch[2]
    return rows_f32(out32["theta1"], out32["theta2"], out32["target_theta1"], out32["target_theta2"], r_star, batch[3], DISCOUNT, kappa, drop, weights)


def measure_f32(cases=CASES):
    """{quantity: worst |float32 twin - float64|} over every minibatch of the cases, each minibatch from the float64 run's state"""
    worst = {k: 0.0 for k in F32_ERR}
    for case in cases:
        inputs = case_inputs(case)
        outs, vecs, _ref = run_case(case, inputs)
        twin = restatement(case, inputs, np.float32)
        wts = case_weights(case, len(inputs[4])) if case[13] else None
        for k, b in enumerate(inputs[4]):
            o32, _v = step(twin, case, b, k, weights=None if wts is None else wts[k], start=None if k == 0 else vecs[k - 1])
            r32 = f32_twin_rows(case, o32, b, None if wts is None else wts[k])
            f = lambda v: np.asarray(v, np.float64)
            for key in ROW_KEYS:
                worst[key] = max(worst[key], float(np.max(np.abs(f(r32[key]) - f(outs[k][key])))))
            for key in ("dq_da", "actions", "target_actions"):
                worst[key] = max(worst[key], float(np.max(np.abs(f(o32[key]) - f(outs[k][key])))))
            ref64 = rows(outs[k]["theta1"], outs[k]["theta2"], outs[k]["target_theta1"], outs[k]["target_theta2"],
                         outs[k]["r_soft"] if case[1] == "sac" else b[2], b[3], DISCOUNT, pool_of(case)[1], pool_of(case)[2], np.float64,
                         None if wts is None else wts[k])
            worst["dz"] = max(worst["dz"], float(np.max(np.abs(f(r32["dz1"]) - ref64["dz1"]))), float(np.max(np.abs(f(r32["dz2"]) - ref64["dz2"]))))
    return worst


# ---- the comparison both test modules make: one minibatch from a common start, every compared quantity as error / bar.  The rows at
# bar(...); the lists, norms, deltas, slots, counts and the temperature at tests.sac_np.ratios' bars (tests/test_gpu_sac_composed.py) and
# tests.ddpg_opt_np's, unchanged.
ROW_BARS = ROW_KEYS + ("dq_da", "actions", "target_actions")
SAC_ROW_BARS = ("logp", "logp2", "r_soft", "g_alpha")


def layout_of(specs):
    return W.TwinLayoutSpec(specs[1])


def ratios(case, specs, start, got, got_vec, want, want_vec, twin32, twin32_vec):
    from tests.helpers import F32_GRAD_FACTOR, delta_bound
    f = lambda v: np.asarray(v, np.float64).reshape(-1)
    out = {}
    for k in ROW_BARS:
        if k == "target_actions" and case[1] != "sac":          # (a deterministic trainer does not report the smoothed a': the one key that may be absent)
            continue
        assert got.get(k) is not None, k
        out[k] = float(np.max(np.abs(f(got[k]) - f(want[k])))) / bar(k)
    sac = case[1] == "sac"
    if sac:
        for k in SAC_ROW_BARS:
            out[k] = float(np.max(np.abs(f(got[k]) - f(want[k])))) / S.composed_bar(k)
    out["loss"] = abs(float(got["loss"]) - float(want["loss"])) / (1e-5 * abs(float(want["loss"])))
    for k in ("actor_norm", "critic_norm"):
        out[k] = abs(float(got[k]) - float(want[k])) / (1e-4 * max(1.0, float(want[k])))
    cspec = layout_of(specs)
    out["actor_grads"] = S.flat_ratio(specs[0], got["actor_grads"], want["actor_grads"], 2e-5, S.f32_rel_of(specs[0], twin32["actor_grads"], want["actor_grads"]))
    out["critic_grads"] = S.flat_ratio(cspec, got["critic_grads"], want["critic_grads"], 2e-5, S.f32_rel_of(cspec, twin32["critic_grads"], want["critic_grads"]))
    for k in ("actor", "critic", "target_actor", "target_critic", "m", "v"):
        if k == "target_actor" and sac:
            continue
        d_want = want_vec[k] - start[k]
        size = float(np.linalg.norm(d_want))
        if size == 0:
            # (a held list, a vector without a slot: nothing moves -- the float32 values of the start, bit for bit)
            out[k + "_delta"] = 0.0 if np.array_equal(np.asarray(got_vec[k], np.float32), np.asarray(start[k], np.float32)) else np.inf
            continue
        r = 5e-5
        if k not in ("m", "v"):
            r = max(r, F32_GRAD_FACTOR * float(np.linalg.norm(twin32_vec[k] - want_vec[k])) / size)
        out[k + "_delta"] = float(np.linalg.norm(f(got_vec[k]) - want_vec[k])) / delta_bound(start[k], d_want, r, 1)
    same = list(got_vec["step"]) == list(want_vec["step"])
    if sac:
        same = same and got_vec["alpha_step"] == want_vec["alpha_step"]
        out["log_alpha"] = abs(got_vec["log_alpha"] - want_vec["log_alpha"]) / S.composed_bar("log_alpha")
        e, g = S.composed_bar("g_alpha"), abs(float(want["g_alpha"]))
        out["alpha_m"] = abs(got_vec["alpha_m"] - want_vec["alpha_m"]) / (0.1 * e + 2.0 ** -23 * abs(want_vec["alpha_m"]) + 1e-30)
        out["alpha_v"] = abs(got_vec["alpha_v"] - want_vec["alpha_v"]) / (1e-3 * (2 * g + e) * e + 2.0 ** -23 * abs(want_vec["alpha_v"]) + 1e-30)
    out["counts"] = 0.0 if same else np.inf
    return out
