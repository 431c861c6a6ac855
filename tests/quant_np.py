"""Quantile critic (quantile regression, Dabney et al. 2018, with the truncated targets of Kuznetsov et al. 2020 inside one network;
include/cartpolepp_abi.h, cpp_net_create_quantile) restated on the float64 oracle: the critic is oracle.ddpg_np.Net over the plain
critic's spec with a q_value layer of N outputs, and QuantDDPG is a subclass of tests.td3_np.DelayedDDPG, so that the optimisers, target
policy smoothing, the policy delay, importance weights and n-step columns compose with it:

    tau_i = (2 i + 1) / (2 N),  Q = (sum_i theta_i) / N
    g = mask discount,  s = sort(theta'(s2, a')),  M = N - d,  y_j = r + g s_j  (j < M: the d largest target atoms are dropped)
    u_ij = y_j - theta_i,  H(u) = u^2 / 2 if |u| <= kappa else kappa (|u| - kappa / 2)
    L_b = (1 / (N M)) sum_i sum_j |tau_i - [u_ij < 0]| H(u_ij) / kappa,  loss = mean_b(w_b L_b)
    d theta_i = -(w_b / B) (1 / (N M)) sum_j |tau_i - [u_ij < 0]| clip(u_ij, -kappa, kappa) / kappa
    the actor follows dQ/da: 1 / N enters the critic's last layer where the scalar critic feeds ones
    td = Q - (sum_{j<M} y_j) / M

Also a float32 variant of the row functions that follows the device's order (xor butterflies over 64 lanes, the bitonic network, j
ascending, every product and sum rounded on its own), the cases the CPU and the GPU tests share, and the faults the CPU test plants.
Test-only: product code never imports it."""
import numpy as np

from oracle import ddpg_np as O
from tests import ddpg_opt_np as R
from tests import dist_np as DN
from tests import td3_np as T3
from tests import tps_np as T

FAULTS = ("targets_not_sorted",               # the first M target atoms as the network emits them
          "smallest_dropped",                 # the d smallest target atoms dropped, not the d largest
          "tau_i_over_n",                     # tau_i = i / N
          "indicator_on_theta_minus_y",       # [theta_i - y_j < 0]
          "huber_without_kappa",              # rho and its gradient without the / kappa
          "plain_l2",                         # u^2 / 2 at every |u|: no linear branch, no clip
          "nm_missing",                       # 1 / (N M) missing from loss and gradient
          "mean_missing",                     # 1 / B missing from the gradient
          "weight_missing",                   # the importance weight left out of loss and gradient
          "discount_without_mask",            # g = discount on terminal (and n-step) rows too
          "target_theta_from_online_critic",  # theta' from the online critic at (s2, a')
          "unsmoothed_target_action",         # theta' at mu'(s2) with smoothing on
          "actor_fed_ones",                   # the actor's chain starts from ones (N times the mean), not 1 / N
          "target_q_value_not_updated")       # the target critic's q_value layer left out of the soft update

ROW_FAULTS = FAULTS[:9]


# ---- the row functions, float64 (any dt) ----------------------------------------------------------------------------------------------
def taus(n, dt=np.float64, fault=None):
    dt = np.dtype(dt).type
    i = np.arange(n).astype(dt)
    if fault == "tau_i_over_n":
        return (i / dt(n)).astype(dt)
    return ((dt(2.0) * i + dt(1.0)) / dt(2 * n)).astype(dt)


def sort_truncate(ttheta, r, g, drop, dt=np.float64, fault=None):
    """(s, y): theta' sorted ascending (B, N) and y_j = r + g s_j over the M = N - drop kept atoms (B, M)"""
    tt = np.asarray(ttheta, dt)
    n = tt.shape[1]
    m = n - int(drop)
    assert 1 <= m <= n
    s = np.sort(tt, axis=1)
    kept = tt[:, :m] if fault == "targets_not_sorted" else (s[:, n - m:] if fault == "smallest_dropped" else s[:, :m])
    y = (np.asarray(r, dt).reshape(-1, 1) + np.asarray(g, dt).reshape(-1, 1) * kept).astype(dt)
    return s, y


def huber(u, kappa, dt=np.float64):
    dt = np.dtype(dt).type
    au = np.abs(u)
    return np.where(au <= dt(kappa), u * u / dt(2.0), dt(kappa) * (au - dt(kappa) / dt(2.0))).astype(dt)


def pair_loss(theta, y, kappa, dt=np.float64, fault=None):
    """(L (B, 1), G (B, N)): the row's quantile Huber loss and sum_j |tau_i - [u_ij < 0]| clip(u_ij) / kappa scaled by 1 / (N M) --
    d theta_i = -(w_b / B) G_i"""
    dtt = np.dtype(dt).type
    theta, y = np.asarray(theta, dt), np.asarray(y, dt)
    n, m = theta.shape[1], y.shape[1]
    u = y[:, None, :] - theta[:, :, None]                       # (B, N, M)
    below = (-u < 0) if fault == "indicator_on_theta_minus_y" else (u < 0)
    k = np.abs(taus(n, dt, fault)[None, :, None] - below.astype(dt))
    if fault == "plain_l2":
        h, c = u * u / dtt(2.0), u
    else:
        h, c = huber(u, kappa, dt), np.clip(u, -dtt(kappa), dtt(kappa))
    div = dtt(1.0) if fault == "huber_without_kappa" else dtt(kappa)
    nm = dtt(1.0) if fault == "nm_missing" else dtt(n * m)
    L = ((k * h / div).sum(axis=2).sum(axis=1, keepdims=True) / nm).astype(dt)      # j inside i
    G = ((k * c / div).sum(axis=2) / nm).astype(dt)
    return L, G


def rows(theta, ttheta, r, mask, discount, kappa, drop, dt=np.float64):
    """everything job (b) of csrc/quant.hip writes per row, in `dt` with numpy's own summation order; y is padded with zeros to (B, N)"""
    dtt = np.dtype(dt).type
    theta = np.asarray(theta, dt)
    n = theta.shape[1]
    g = (np.asarray(mask, dt) * dtt(discount)).astype(dt)
    s, y = sort_truncate(ttheta, r, g, drop, dt)
    L, G = pair_loss(theta, y, kappa, dt)
    q, tq = theta.mean(axis=1, keepdims=True), s.mean(axis=1, keepdims=True)
    ypad = np.zeros_like(theta)
    ypad[:, :y.shape[1]] = y
    return {"theta": theta, "sorted": s, "y": ypad, "q": q, "tq": tq, "td": q - y.mean(axis=1, keepdims=True), "L": L, "G": G}


# ---- the float32 variant: the device's order ---------------------------------------------------------------------------------------------
_butterfly, _lanes = DN._butterfly, DN._lanes


def _butterfly64(v):
    v = np.array(v, np.float64)
    lanes = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        v = v + v[:, lanes ^ o]
    return v[:, :1]


def bitonic_sort(v):
    """quant_sort of csrc/quant.hip on (B, 64): 21 compare-exchange stages, each lane keeps the minimum or the maximum by its lane bits"""
    v = np.array(v, np.float32)
    lanes = np.arange(64)
    stages = 0
    k = 2
    while k <= 64:
        j = k >> 1
        while j > 0:
            o = v[:, lanes ^ j]
            keep_min = ((lanes & j) == 0) == ((lanes & k) == 0)
            v = np.where(keep_min[None, :], np.minimum(v, o), np.maximum(v, o)).astype(np.float32)
            stages += 1
            j >>= 1
        k <<= 1
    assert stages == 21
    return v


def rows_f32(theta, ttheta, r, mask, discount, kappa, drop, w=None):
    """rows() in float32, operation by operation as job (b) of csrc/quant.hip; also "dz", the gradient (w_b / B folded in)"""
    f = np.float32
    th_in = np.asarray(theta, np.float32)
    B, n = th_in.shape
    m = n - int(drop)
    lane = np.arange(64)
    on, kept = (lane < n)[None, :], (lane < m)[None, :]
    th = _lanes(th_in, 0.0)
    s = bitonic_sort(_lanes(ttheta, np.inf))
    q = (_butterfly(th, np.add) / f(n)).astype(np.float32)
    tq = (_butterfly(np.where(on, s, f(0)), np.add) / f(n)).astype(np.float32)
    r = np.asarray(r, np.float32).reshape(-1, 1)
    g = (np.asarray(mask, np.float32).reshape(-1, 1) * f(discount)).astype(np.float32)
    with np.errstate(invalid="ignore"):
        y = np.where(kept, (r + (g * s).astype(np.float32)).astype(np.float32), f(0)).astype(np.float32)
    ym = (_butterfly(y, np.add) / f(m)).astype(np.float32)
    tau = ((2 * lane + 1).astype(np.float32) / f(2 * n)).astype(np.float32)[None, :]
    kap = f(kappa)
    gs, ls = np.zeros((B, 64), np.float32), np.zeros((B, 64), np.float64)
    for j in range(m):
        u = (y[:, j:j + 1] - th).astype(np.float32)
        k = np.abs((tau - np.where(u < 0, f(1), f(0))).astype(np.float32))
        c = np.minimum(np.maximum(u, -kap), kap)
        gs = (gs + (k * c).astype(np.float32)).astype(np.float32)
        ud, kd = u.astype(np.float64), float(kap)
        au = np.abs(ud)
        ls = ls + k.astype(np.float64) * np.where(au <= kd, 0.5 * ud * ud, kd * (au - 0.5 * kd))
    L = _butterfly64(np.where(on, ls, 0.0)) / (float(kap) * (float(n) * float(m)))
    inv_b, inv_nm = f(1.0) / f(B), f(1.0) / f(n * m)
    d = (-((gs / kap).astype(np.float32) * inv_nm).astype(np.float32)).astype(np.float32)
    if w is not None:
        d = (d * np.asarray(w, np.float32).reshape(-1, 1)).astype(np.float32)
    dz = (d * inv_b).astype(np.float32)
    return {"theta": th[:, :n], "sorted": s[:, :n], "y": y[:, :n], "q": q, "tq": tq, "td": (q - ym).astype(np.float32), "L": L, "dz": dz[:, :n]}


# ---- the learner ----------------------------------------------------------------------------------------------------------------------
quant_spec = DN.dist_spec          # the plain critic's spec with q_value (n_in, N)


class QuantDDPG(T3.DelayedDDPG):
    def __init__(self, actor_spec, critic_spec, actor_flat, critic_flat, quant, dt=np.float64, hyper=O.DEFAULT_HYPER,
                 optimiser="GradientDescent", optimiser_args=None, delay=1, smoothing=None, fault=None):
        """critic_spec: quant_spec(...); quant: (n_quantiles, kappa, drop_top)"""
        assert fault is None or fault in FAULTS, fault
        assert critic_spec.fc[-1][2] == quant[0] and 0 <= quant[2] <= quant[0] - 1
        super(QuantDDPG, self).__init__(actor_spec, critic_spec, actor_flat, critic_flat, dt, hyper, optimiser, optimiser_args,
                                        delay, smoothing, None)
        self.quant, self.quant_fault = (int(quant[0]), float(np.float32(quant[1])), int(quant[2])), fault
        self.weights = None                  # importance weights (B, 1) of the next minibatch (prioritized replay), or None

    def update_targets(self):
        if self.quant_fault != "target_q_value_not_updated":
            return super(QuantDDPG, self).update_targets()
        keep = self.target_critic.flat()
        super(QuantDDPG, self).update_targets()
        new = self.target_critic.flat()
        _name, n_in, n_out, _a, _c = self.critic.spec.fc[-1]
        k = n_in * n_out + n_out
        new[-k:] = keep[-k:]
        self.target_critic = O.Net(self.critic.spec, new, self.dt)

    # ddpg_cartpole.py:111-113 + :220-222 through the mean of the quantiles
    def actor_gradients(self, s1):
        dt = self.dt
        n = self.quant[0]
        w1 = self._white(self.actor, s1)
        ca = self.actor.forward(s1, white=w1)
        cc = self.critic.forward(s1, action=ca["out"], white=w1)
        theta = np.asarray(cc["out"], dt)
        q = (theta.sum(axis=1, keepdims=True) / dt(n)).astype(dt)
        top = np.ones_like(theta) if self.quant_fault == "actor_fed_ones" else np.full_like(theta, dt(1.0) / dt(n))
        _, dq_da = self.critic.backward(cc, top, params=False)
        grads, _ = self.actor.backward(ca, -dq_da)
        self.last_ag = {"actions": ca["out"], "q": q, "dq_da": dq_da, "grads": O.flatten(self.actor.spec, grads, dt), "cache_actor": ca}
        return self.last_ag

    def critic_gradients(self, batch, noise="draw", training=True, w=None):
        """noise: 'draw' (the smoothing of the restatement, if any; the count advances), None, or a (B, A) array.  w: (B, 1) importance
        weights (default: self.weights, else uniform)"""
        s1, a, r, mask, s2 = batch
        dt, fault = self.dt, self.quant_fault
        n, kappa, drop = self.quant
        act = np.asarray(a)
        B, A = act.shape[0], act.shape[1]
        if isinstance(noise, str):
            noise = None
            if self.smoothing is not None and training:
                sigma, clip, seed = self.smoothing
                noise = T.target_noise(seed, self.tps_n, B, A, sigma, clip, np.float64)
                self.tps_n += 1
        w = self.weights if w is None else w
        w = np.ones((B, 1), dt) if w is None else np.asarray(w, dt).reshape(B, 1)
        w2 = self._white(self.target_actor, s2)
        ta = self.target_actor.forward(s2, white=w2, training=training)
        sm = ta["out"] if noise is None else np.clip((ta["out"] + np.asarray(noise, dt)).astype(dt), dt(-1.0), dt(1.0))
        at = ta["out"] if fault == "unsmoothed_target_action" else sm
        src = self.critic if fault == "target_theta_from_online_critic" else self.target_critic
        tq = src.forward(s2, action=at, white=w2, training=training)
        g = np.full((B, 1), dt(self.hp.discount)) if fault == "discount_without_mask" else (np.asarray(mask, dt) * dt(self.hp.discount)).astype(dt)
        s, y = sort_truncate(tq["out"], r, g, drop, dt, fault)
        cb = self.critic.forward(s1, action=np.asarray(a, dt), training=training)
        theta = np.asarray(cb["out"], dt)
        L, G = pair_loss(theta, y, kappa, dt, fault)
        q = (theta.sum(axis=1, keepdims=True) / dt(n)).astype(dt)
        td = (q - y.sum(axis=1, keepdims=True) / dt(y.shape[1])).astype(dt)
        wl = np.ones_like(w) if fault == "weight_missing" else w
        loss = (wl * L).mean(dtype=dt)
        dz = (-G * wl).astype(dt) if fault == "mean_missing" else (-G * wl / dt(B)).astype(dt)
        grads, _ = self.critic.backward(cb, dz)
        # dQ'/da' at the smoothed action (tests.tps_np.td_bar's propagated noise term)
        _, tdq = src.backward(tq, np.full_like(theta, dt(1.0) / dt(n)), params=False)
        ypad = np.zeros_like(theta)
        ypad[:, :y.shape[1]] = y
        self.last_cg = {"q": q, "td": td, "y": ypad, "loss": loss, "target_q": s.mean(axis=1, keepdims=True), "theta": theta, "sorted": s,
                        "L": L, "target_theta": tq["out"], "target_actions": ta["out"], "smoothed_actions": sm, "target_dq_da": tdq,
                        "noise": noise, "cache_critic": cb, "grads": O.flatten(self.critic.spec, grads, dt), "w": w, "dz": dz, "g": g,
                        "u": y[:, None, :] - theta[:, :, None]}
        return self.last_cg

    def check_loss(self, batch):      # ddpg_cartpole.py:239-248 (IS_TRAINING: False): the same formula, no noise, no weights
        out = self.critic_gradients(batch, noise=None, training=False, w=np.ones((np.asarray(batch[1]).shape[0], 1)))
        return out["loss"], out["td"], out["q"]


def restatement(specs, P, quant, dt, hyper, opt_name="gradient-descent", delay=1, smoothing=None, fault=None):
    name, args = T3.OPTIMISERS[opt_name]
    ref = QuantDDPG(specs[0], specs[1], P[0], P[1], quant, dt, hyper, name, args, delay, smoothing, fault)
    ref.set_targets(P[2], P[3])
    return ref


# ---- the cases.  tests.helpers.host_case's parameters, episodes and rows (its rewards are 0, 1, 2 and every episode ends in a terminal
# row), the q_value layer redrawn at N outputs from a stream of its own: weights scaled up and biases spread over the scale of the returns,
# so that the atoms are far from sorted and the u_ij fall on both sides of kappa.
SMOOTHING = DN.SMOOTHING          # sigma, clip, seed
SHAPES, ROWS, NB, STEPS = DN.SHAPES, DN.ROWS, DN.NB, DN.STEPS
TAIL_SCALE, BIAS_MEAN, BIAS_SPREAD = 3.0, 1.0, 1.0
SMALL_KAPPA = 0.25
# (id, shape, action_dim, B, N, drop_top, kappa, discount, optimiser, delay, smoothing, clip, tau, n_step)
#   B = 1, 5, 8: on both sides of a workgroup's four rows;  N = 2, 25, 33, 64: idle lanes, the default, past the half wave, every lane (the
#   full sort);  d = 0 (plain QR), 2, N - 1 (M = 1);  kappa = 1 and one small kappa that puts most pairs on the linear branch
CASES = (("A2-B8-N25-d0-sgd", "16x16x3", 2, 8, 25, 0, 1.0, 0.9, "gradient-descent", 1, None, 0.5, 0.25, 1),
         ("A2-B5-N33-d2", "16x16x3", 2, 5, 33, 2, 1.0, 0.9, "gradient-descent", 1, None, 1e4, 1.0, 1),
         ("A2-B1-N2-d1", "16x16x3", 2, 1, 2, 1, 1.0, 0.9, "gradient-descent", 1, None, 0.5, 0.25, 1),
         ("A9-B8-N64-d2-momentum", "16x16x3", 9, 8, 64, 2, 1.0, 0.9, "momentum-0.5", 1, None, 0.5, 0.25, 1),
         ("A2-B5-N64-d63-adam", "16x16x3", 2, 5, 64, 63, 1.0, 0.9, "adam", 1, None, 0.5, 0.25, 1),
         ("A2-B8-N25-d2-smallkappa", "16x16x3", 2, 8, 25, 2, SMALL_KAPPA, 0.9, "gradient-descent", 1, None, 0.5, 0.25, 1),
         ("A2-B8-N25-d2-smoothed", "16x16x3", 2, 8, 25, 2, 1.0, 0.9, "gradient-descent", 1, SMOOTHING, 0.5, 0.25, 1),
         ("A2-B5-N33-d2-weighted", "16x16x3", 2, 5, 33, 2, 1.0, 0.9, "gradient-descent", 1, None, 0.5, 0.25, 1),
         ("A2-B8-N25-d2-nstep3", "16x16x3", 2, 8, 25, 2, 1.0, 0.9, "gradient-descent", 1, None, 0.5, 0.25, 3),
         ("lowdim-A3-B8-N25-d2-tqc", "lowdim", 3, 8, 25, 2, 1.0, 0.9, "adam", 2, SMOOTHING, 0.5, 0.25, 1))
SEEDS = {c[0]: 1 for c in CASES}
SEEDS["A2-B1-N2-d1"] = 6          # (its one row and two pairs must do what eight rows do elsewhere: a first row that is not terminal, target atoms that
#                                    arrive unsorted, one pair on each Huber branch and of each sign, no route closer to a tie than float32 can decide)


def case_of(cid):
    return [c for c in CASES if c[0] == cid][0]


def quant_of(case):
    return (case[4], case[6], case[5])          # (N, kappa, drop_top)


def hyper_of(case):
    return T3.hyper_of(case[8], case[11], case[12])._replace(discount=case[7])


def q_value_tail(spec, n, rng):
    """the q_value layer at N outputs: (online, target) float32 vectors, make_pair's perturbations"""
    _name, n_in, _n, _a, _c = spec.fc[-1]
    lim = np.sqrt(6.0 / (n_in + n))
    p = np.concatenate([(TAIL_SCALE * rng.uniform(-lim, lim, (n_in, n))).astype(np.float32).ravel(),
                        rng.normal(BIAS_MEAN, BIAS_SPREAD, n).astype(np.float32)])
    return p, p + rng.normal(0, 0.05, p.shape).astype(np.float32)


def host_case(shape, B, nb, seed, n, rows=ROWS, action_dim=2, n_step=1, discount=0.9, **plain_kw):
    """tests.helpers.host_case with quantile critics: (specs, P, episodes, idxs, batches); specs[1] is quant_spec's, P[1] and P[3] end in
    the wider q_value layer.  n_step > 1: the minibatches carry the n-step columns the device's gather forms."""
    from tests.helpers import host_case as plain_case
    specs, P, episodes, idxs, batches = plain_case(shape, B, nb, seed, rows=rows, action_dim=action_dim, **plain_kw)      # (dropout, actor_hidden)
    cspec = specs[1]
    _name, n_in, _one, _a, _c = cspec.fc[-1]
    cut = n_in + 1
    on, tg = q_value_tail(cspec, n, np.random.default_rng(8000 + seed))
    P = [P[0], np.concatenate([P[1][:-cut], on]), P[2], np.concatenate([P[3][:-cut], tg])]
    if n_step > 1:
        batches = DN.n_step_batches(shape, episodes, rows, idxs, B, action_dim, n_step, discount)
    return (specs[0], quant_spec(cspec, n)), P, episodes, idxs, batches


def case_inputs(case, nb=NB, seed=None, **kw):
    cid, shape_name, A, B, N = case[:5]
    return host_case(SHAPES[shape_name], B, nb, SEEDS[cid] if seed is None else seed, N, rows=ROWS, action_dim=A, n_step=case[13],
                     discount=case[7], **kw)


def structure(case):
    """(minibatches per outer step, outer steps): the weighted case takes one minibatch per call -- the device's importance weights can
    be read back for the last minibatch of a call only"""
    return (1, NB) if "weighted" in case[0] else (NB, STEPS)


OUT_KEYS = ("theta", "sorted", "y", "q")


def run_case(case, inputs, dt=np.float64, fault=None, nb=None, steps=None, weights=None, quant=None):
    """`steps` outer steps of `nb` minibatches (default: structure(case)), the target update behind each: (the six vectors, step counts,
    per-minibatch outputs, the restatement)"""
    if nb is None:
        nb, steps = structure(case)
    specs, P, _ep, _idxs, batches = inputs
    ref = restatement(specs, P, quant or quant_of(case), dt, hyper_of(case), case[8], case[9], case[10], fault)
    outs = []
    for s in range(steps):
        for k in range(s * nb, (s + 1) * nb):
            ref.weights = None if weights is None else weights[k]
            o = ref.train_minibatch(batches[k])
            o.update({key: ref.last_cg[key] for key in OUT_KEYS}, dq_da=ref.last_ag["dq_da"], actions=ref.last_ag["actions"],
                     actor_grads=ref.last_ag["grads"], critic_grads=ref.last_cg["grads"], u=ref.last_cg["u"], dz=ref.last_cg["dz"])
            outs.append(o)
        ref.update_targets()
    return R.vectors(ref), ref.state()["step"], outs, ref


case_weights = DN.case_weights


def bounds(P, want, nb):
    return R.bounds(P, want, nb)


# ---- the bars of the GPU comparison, derived in tests/test_quantile_host.py (which re-measures and asserts these figures): the float32
# restatement -- the learner evaluated in float32, its atoms through rows_f32 -- against float64, worst over the first minibatch of every
# case, for theta, the sorted theta', y, d theta, Q, td and dQ/da.  Each bar is that figure times 8 (the margin covers the device's
# reduction order in the layers below, which differs from numpy's); where the figure is below ATOL / 4 the suite's ordinary ATOL is kept.
ATOL, GRAD_REL, PARAM_REL = 1e-5, 2e-5, R.PARAM_REL
BAR_FACTOR = 8.0
# Measured: theta 1.44e-6, sorted theta' 1.57e-6, y 1.41e-6, d theta 8.77e-7, Q 1.58e-7, td 1.46e-6, dQ/da 4.40e-8 -- every one below
# ATOL / 4, so every bar is ATOL.
F32_ERR = {"theta": 1.5e-6, "sorted": 1.6e-6, "y": 1.45e-6, "dz": 9.0e-7, "q": 1.65e-7, "td": 1.5e-6, "dq_da": 4.5e-8}


def bar(key):
    e = F32_ERR[key]
    return ATOL if e < ATOL / 4 else BAR_FACTOR * e


def f32_rows_of(case, inputs, k=0):
    """(float64 critic outputs, float32 row outputs) of minibatch k at the case's starting parameters; weighted cases take case_weights"""
    b = inputs[4][k]
    w = case_weights(case)[k] if "weighted" in case[0] else None
    out = {}
    for dt in (np.float64, np.float32):
        ref = restatement(inputs[0], inputs[1], quant_of(case), dt, hyper_of(case), case[8], case[9], case[10])
        out[dt] = dict(ref.critic_gradients(b, w=w), dq_da=ref.actor_gradients(b[0])["dq_da"])
    c32 = out[np.float32]
    n, kappa, drop = quant_of(case)
    r32 = rows_f32(c32["theta"], c32["target_theta"], b[2], b[3], case[7], kappa, drop, w)
    r32["dq_da"] = c32["dq_da"]
    return out[np.float64], r32


# ---- graph replay: the learner whole on one device (Adam, smoothing, --policy-delay 2, 3-step returns, the quantile critic with two
# dropped atoms) on the rows the device draws (tests.td3_np.device_rows), the first outer step the eager pass and the capture, the others
# replays of ONE graph.  case, minibatches per step, outer steps, sample seed
GRAPH_CASE = (("tqc-16x16x3-4x3", "16x16x3", 2, 8, 25, 2, 1.0, 0.9, "adam", 2, SMOOTHING, 0.5, 0.25, 3), 3, 4, 0)
GRAPH_SEED = 1


def graph_inputs(seed=None, sample_seed=None):
    case, nb, steps, ss = GRAPH_CASE
    shape, A, B, N = SHAPES[case[1]], case[2], case[3], case[4]
    specs, P, episodes, _idxs, _b = host_case(shape, B, 1, GRAPH_SEED if seed is None else seed, N, rows=ROWS, action_dim=A)
    rows_ = np.concatenate([T3.device_rows(ss if sample_seed is None else sample_seed, k, B, ROWS) for k in range(steps * nb)])
    return specs, P, episodes, rows_, DN.n_step_batches(shape, episodes, ROWS, rows_, B, A, case[13], case[7])
