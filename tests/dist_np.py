"""Distributional (categorical) critic (Bellemare et al. 2017 as D4PG uses it, Barth-Maron et al. 2018; include/cartpolepp_abi.h,
cpp_net_create_distributional) restated on the float64 oracle: the critic is oracle.ddpg_np.Net over the plain critic's spec with a
q_value layer of N outputs, and DistDDPG is a subclass of tests.td3_np.DelayedDDPG, so that the optimisers, target policy smoothing, the
policy delay, importance weights and n-step columns compose with it:

    z_i = v_min + i delta,  p = softmax(logits),  Q = sum_i p_i z_i
    g = mask discount,  Tz_j = clamp(r + g z_j, v_min, v_max),  b_j = (Tz_j - v_min) / delta
    m_i = sum_j p'_j max(0, 1 - |b_j - i|)                       (j = 0 .. N-1 in order)
    L_b = -sum_i m_i log p_i,  loss = mean_b(w_b L_b),  d logits = (w_b / B)(p - m)
    the actor follows dQ/da: p (z - Q) enters the critic's last layer where the scalar critic feeds ones
    y = sum_i m_i z_i,  td = Q - y

Also a float32 variant of the row functions that follows the device's order (xor butterflies over 64 lanes, every product and sum rounded
on its own), the cases the CPU and the GPU tests share, and the faults the CPU test plants.  Test-only: product code never imports it."""
import copy

import numpy as np

from oracle import ddpg_np as O
from tests import ddpg_opt_np as R
from tests import td3_np as T3
from tests import tps_np as T

FAULTS = ("projection_unclamped",             # Tz not clamped: the mass beyond the ends is lost
          "discount_without_mask",            # g = discount on terminal (and n-step) rows too
          "target_p_from_online_critic",      # p' from the online critic at (s2, a')
          "m_from_unsmoothed_action",         # the target distribution at mu'(s2) with smoothing on
          "log_of_wrong_evaluation",          # the cross-entropy against the target evaluation's own log p'
          "weight_missing",                   # the importance weight left out of loss and gradient
          "mean_missing",                     # 1/B missing from the logit gradient
          "actor_fed_ones",                   # the actor's chain starts from ones (the sum of the logits), not p (z - Q)
          "support_off_by_one",               # z_i = v_min + (i + 1) delta
          "integer_b_loses_mass",             # the floor / ceil scatter as often coded: nothing lands when b_j is an integer
          "target_q_value_not_updated")       # the target critic's q_value layer left out of the soft update


# ---- the row functions, float64 (any dt) ----------------------------------------------------------------------------------------------
def support(n_atoms, v_min, v_max, dt=np.float64, fault=None):
    dt = np.dtype(dt).type
    delta = (dt(v_max) - dt(v_min)) / dt(n_atoms - 1)
    i = np.arange(n_atoms).astype(dt) + (dt(1.0) if fault == "support_off_by_one" else dt(0.0))
    return (dt(v_min) + i * delta).astype(dt), delta


def softmax(logits, dt=np.float64):
    """(p, log p) with the row maximum subtracted first"""
    x = np.asarray(logits, dt)
    c = x - x.max(axis=1, keepdims=True)
    e = np.exp(c)
    s = e.sum(axis=1, keepdims=True)
    return (e / s).astype(dt), (c - np.log(s)).astype(dt)


def project(tp, r, g, n_atoms, v_min, v_max, dt=np.float64, fault=None):
    """m (B, N): the Bellman-shifted target distribution projected onto the support by the triangular kernel, j in order"""
    dtt = np.dtype(dt).type
    z, delta = support(n_atoms, v_min, v_max, dt)
    tp, r, g = np.asarray(tp, dt), np.asarray(r, dt).reshape(-1, 1), np.asarray(g, dt).reshape(-1, 1)
    i = np.arange(n_atoms).astype(dt)[None, :]
    m = np.zeros_like(tp)
    for j in range(n_atoms):
        tz = r + g * z[j]
        if fault != "projection_unclamped":
            tz = np.clip(tz, dtt(v_min), dtt(v_max))
        b = (tz - dtt(v_min)) / delta
        if fault == "integer_b_loses_mass":
            lo, hi = np.floor(b), np.ceil(b)
            k = np.where(i == lo, hi - b, dtt(0.0)) + np.where(i == hi, b - lo, dtt(0.0))
        else:
            k = np.maximum(dtt(0.0), dtt(1.0) - np.abs(b - i))
        m = (m + tp[:, j:j + 1] * k).astype(dt)
    return m


def scatter_projection(tp, r, g, n_atoms, v_min, v_max):
    """the usual floor / ceil scatter in float64, with the integer case handled (the whole mass on atom b_j): what the triangular form is
    checked against"""
    z, delta = support(n_atoms, v_min, v_max, np.float64)
    tp, r, g = np.asarray(tp, np.float64), np.asarray(r, np.float64).ravel(), np.asarray(g, np.float64).ravel()
    m = np.zeros_like(tp)
    for row in range(tp.shape[0]):
        for j in range(n_atoms):
            b = (min(max(r[row] + g[row] * z[j], v_min), v_max) - v_min) / delta
            lo, hi = int(np.floor(b)), int(np.ceil(b))
            if lo == hi:
                m[row, lo] += tp[row, j]
            else:
                m[row, lo] += tp[row, j] * (hi - b)
                m[row, hi] += tp[row, j] * (b - lo)
    return m


def rows(logits, tlogits, r, mask, discount, n_atoms, v_min, v_max, dt=np.float64):
    """everything job (b) of csrc/dist.hip writes per row, in `dt` with numpy's own summation order"""
    dtt = np.dtype(dt).type
    z, _delta = support(n_atoms, v_min, v_max, dt)
    p, logp = softmax(logits, dt)
    tp, _ = softmax(tlogits, dt)
    g = (np.asarray(mask, dt) * dtt(discount)).astype(dt)
    m = project(tp, r, g, n_atoms, v_min, v_max, dt)
    q, tq, y = (p * z).sum(axis=1, keepdims=True), (tp * z).sum(axis=1, keepdims=True), (m * z).sum(axis=1, keepdims=True)
    return {"p": p, "tp": tp, "m": m, "q": q, "tq": tq, "y": y, "td": q - y, "ce": -(m * logp).sum(axis=1, keepdims=True)}


# ---- the float32 variant: the device's order ---------------------------------------------------------------------------------------------
def _butterfly(v, op):
    """xor butterfly over 64 lanes, offsets 32 .. 1: lane i takes op(v_i, v_{i ^ o}); every lane ends with the same float32 bits"""
    v = np.array(v, np.float32)
    lanes = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        v = op(v, v[:, lanes ^ o]).astype(np.float32)
    return v[:, :1]


def _lanes(x, fill):
    x = np.asarray(x, np.float32)
    out = np.full((x.shape[0], 64), fill, np.float32)
    out[:, :x.shape[1]] = x
    return out


def softmax_f32(logits, z64):
    """(p, log p, Q) over 64 lanes as dist_softmax computes them (numpy's expf / logf stand in for the device's)"""
    n = np.asarray(logits).shape[1]
    x = _lanes(logits, -np.inf)
    mx = _butterfly(x, np.maximum)
    c = np.where(np.arange(64)[None, :] < n, x - mx, np.float32(0)).astype(np.float32)
    e = np.where(np.arange(64)[None, :] < n, np.exp(c), np.float32(0)).astype(np.float32)
    s = _butterfly(e, np.add)
    p = (e / s).astype(np.float32)
    logp = (c - np.log(s)).astype(np.float32)
    q = _butterfly((p * z64).astype(np.float32), np.add)
    return p, logp, q


def rows_f32(logits, tlogits, r, mask, discount, n_atoms, v_min, v_max):
    """rows() in float32, operation by operation as job (b) of csrc/dist.hip: every product and sum rounded on its own"""
    f = np.float32
    n = int(n_atoms)
    delta = f((f(v_max) - f(v_min)) / f(n - 1))
    lane = np.arange(64).astype(np.float32)
    z = (f(v_min) + (lane * delta).astype(np.float32)).astype(np.float32)[None, :]
    p, logp, q = softmax_f32(logits, z)
    tp, _lp, tq = softmax_f32(tlogits, z)
    r = np.asarray(r, np.float32).reshape(-1, 1)
    g = (np.asarray(mask, np.float32).reshape(-1, 1) * f(discount)).astype(np.float32)
    m = np.zeros_like(p)
    for j in range(n):
        tz = np.minimum(np.maximum((r + (g * z[0, j]).astype(np.float32)).astype(np.float32), f(v_min)), f(v_max))
        b = ((tz - f(v_min)).astype(np.float32) / delta).astype(np.float32)
        k = np.maximum(f(0), (f(1) - np.abs((b - lane[None, :]).astype(np.float32))).astype(np.float32))
        m = (m + (tp[:, j:j + 1] * k).astype(np.float32)).astype(np.float32)
    m[:, n:] = 0
    y = _butterfly((m * z).astype(np.float32), np.add)
    ce = -(m[:, :n].astype(np.float64) * logp[:, :n].astype(np.float64)).sum(axis=1, keepdims=True)
    return {"p": p[:, :n], "tp": tp[:, :n], "m": m[:, :n], "q": q, "tq": tq, "y": y, "td": (q - y).astype(np.float32), "ce": ce}


# ---- the learner ----------------------------------------------------------------------------------------------------------------------
def dist_spec(cspec, n_atoms):
    """the plain critic's spec with q_value (n_in, N)"""
    assert cspec.kind == "critic"
    sp = copy.copy(cspec)
    name, n_in, _one, act, cat = cspec.fc[-1]
    assert name == "q_value" and _one == 1
    sp.fc = list(cspec.fc[:-1]) + [(name, n_in, int(n_atoms), act, cat)]
    return sp


class DistDDPG(T3.DelayedDDPG):
    def __init__(self, actor_spec, critic_spec, actor_flat, critic_flat, dist, dt=np.float64, hyper=O.DEFAULT_HYPER,
                 optimiser="GradientDescent", optimiser_args=None, delay=1, smoothing=None, fault=None):
        """critic_spec: dist_spec(...); dist: (n_atoms, v_min, v_max)"""
        assert fault is None or fault in FAULTS, fault
        assert critic_spec.fc[-1][2] == dist[0]
        super(DistDDPG, self).__init__(actor_spec, critic_spec, actor_flat, critic_flat, dt, hyper, optimiser, optimiser_args,
                                       delay, smoothing, None)
        self.dist, self.dist_fault = (int(dist[0]), float(np.float32(dist[1])), float(np.float32(dist[2]))), fault
        self.weights = None                  # importance weights (B, 1) of the next minibatch (prioritized replay), or None

    def update_targets(self):
        if self.dist_fault != "target_q_value_not_updated":
            return super(DistDDPG, self).update_targets()
        keep = self.target_critic.flat()
        super(DistDDPG, self).update_targets()
        new = self.target_critic.flat()
        name, n_in, n_out, _a, _c = self.critic.spec.fc[-1]
        k = n_in * n_out + n_out
        new[-k:] = keep[-k:]
        self.target_critic = O.Net(self.critic.spec, new, self.dt)

    def _z(self, fault=None):
        return support(self.dist[0], self.dist[1], self.dist[2], self.dt, fault)[0][None, :]

    # ddpg_cartpole.py:111-113 + :220-222 through the expectation
    def actor_gradients(self, s1):
        dt = self.dt
        z = self._z("support_off_by_one" if self.dist_fault == "support_off_by_one" else None)
        w1 = self._white(self.actor, s1)
        ca = self.actor.forward(s1, white=w1)
        cc = self.critic.forward(s1, action=ca["out"], white=w1)
        p, _lp = softmax(cc["out"], dt)
        q = (p * z).sum(axis=1, keepdims=True)
        top = np.ones_like(p) if self.dist_fault == "actor_fed_ones" else (p * (z - q)).astype(dt)
        _, dq_da = self.critic.backward(cc, top, params=False)
        grads, _ = self.actor.backward(ca, -dq_da)
        self.last_ag = {"actions": ca["out"], "q": q, "dq_da": dq_da, "grads": O.flatten(self.actor.spec, grads, dt), "cache_actor": ca,
                        "p": p}
        return self.last_ag

    def critic_gradients(self, batch, noise="draw", training=True, w=None):
        """noise: 'draw' (the smoothing of the restatement, if any; the count advances), None, or a (B, A) array.  w: (B, 1) importance
        weights (default: self.weights, else uniform)"""
        s1, a, r, mask, s2 = batch
        dt, fault = self.dt, self.dist_fault
        n_atoms, v_min, v_max = self.dist
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
        at = ta["out"] if fault == "m_from_unsmoothed_action" else sm
        src = self.critic if fault == "target_p_from_online_critic" else self.target_critic
        tq = src.forward(s2, action=at, white=w2, training=training)
        z = self._z("support_off_by_one" if fault == "support_off_by_one" else None)
        tp, tlogp = softmax(tq["out"], dt)
        g = np.full((B, 1), dt(self.hp.discount)) if fault == "discount_without_mask" else (np.asarray(mask, dt) * dt(self.hp.discount)).astype(dt)
        m = project(tp, r, g, n_atoms, v_min, v_max, dt, fault if fault in ("projection_unclamped", "integer_b_loses_mass") else None)
        if fault == "support_off_by_one":      # (the shifted support moves Tz as well: the projection on it)
            zz, delta = support(n_atoms, v_min, v_max, dt, fault)
            m = np.zeros_like(tp)
            i = np.arange(n_atoms).astype(dt)[None, :]
            for j in range(n_atoms):
                b = (np.clip(np.asarray(r, dt).reshape(B, 1) + g * zz[j], dt(v_min), dt(v_max)) - dt(v_min)) / delta
                m = m + tp[:, j:j + 1] * np.maximum(dt(0.0), dt(1.0) - np.abs(b - i))
        cb = self.critic.forward(s1, action=np.asarray(a, dt), training=training)
        p, logp = softmax(cb["out"], dt)
        q, y = (p * z).sum(axis=1, keepdims=True), (m * z).sum(axis=1, keepdims=True)
        td = q - y
        pg, lg = (tp, tlogp) if fault == "log_of_wrong_evaluation" else (p, logp)
        ce = -(m * lg).sum(axis=1, keepdims=True)
        wl = np.ones_like(w) if fault == "weight_missing" else w
        loss = (wl * ce).mean(dtype=dt)
        dz = ((pg - m) * wl).astype(dt) if fault == "mean_missing" else ((pg - m) * wl / dt(B)).astype(dt)
        grads, _ = self.critic.backward(cb, dz)
        # dQ'/da' at the smoothed action (tests.tps_np.td_bar's propagated noise term)
        _, tdq = src.backward(tq, (tp * (z - (tp * z).sum(axis=1, keepdims=True))).astype(dt), params=False)
        self.last_cg = {"q": q, "td": td, "y": y, "loss": loss, "target_q": (tp * z).sum(axis=1, keepdims=True), "p": p, "tp": tp, "m": m,
                        "ce": ce, "logits": cb["out"], "target_logits": tq["out"], "target_actions": ta["out"], "smoothed_actions": sm,
                        "target_dq_da": tdq, "noise": noise, "cache_critic": cb, "grads": O.flatten(self.critic.spec, grads, dt), "w": w,
                        "dz": dz, "g": g}
        return self.last_cg

    def check_loss(self, batch):      # ddpg_cartpole.py:239-248 (IS_TRAINING: False): the same formula, no noise, no weights
        out = self.critic_gradients(batch, noise=None, training=False, w=np.ones((np.asarray(batch[1]).shape[0], 1)))
        return out["loss"], out["td"], out["q"]


def restatement(specs, P, dist, dt, hyper, opt_name="gradient-descent", delay=1, smoothing=None, fault=None):
    name, args = T3.OPTIMISERS[opt_name]
    ref = DistDDPG(specs[0], specs[1], P[0], P[1], dist, dt, hyper, name, args, delay, smoothing, fault)
    ref.set_targets(P[2], P[3])
    return ref


# ---- the cases.  tests.helpers.host_case's parameters, episodes and rows (its rewards are 0, 1, 2 and every episode ends in a terminal
# row), the q_value layer redrawn at N outputs from a stream of its own, scaled up so that the distributions are far from uniform.
SMOOTHING = (0.2, 0.5, 0xD4)          # sigma, clip, seed
SHAPES = {"16x16x3": (16, 16, 3, 1, 1), "lowdim": (2, 2, 7)}
ROWS = 24
NB, STEPS = 3, 1
LOGIT_SCALE = 6.0
# (id, shape, action_dim, B, n_atoms, v_min, v_max, discount, optimiser, delay, smoothing, clip, tau, n_step)
#   B = 1, 5, 8: on both sides of a workgroup's four rows;  N = 2, 33, 51, 64: idle lanes, an odd count, the default, every lane
#   integer: a support from 0 whose delta is a power of two ([0, 8] at N = 33: 1/4; [0, 7.875] at N = 64: 1/8), integer rewards and
#   discount 1 -- b_j is an integer on every row, as on [0, N - 1], with the support inside [-10, 10]
#   ends: [0.5, 1.5], the rewards 0 (terminal rows) and 2 lie beyond each end
#   wide: [-100, 100], the one case beyond [-10, 10] (its own scaled bars)
CASES = (("A2-B8-N51-sgd", "16x16x3", 2, 8, 51, -10.0, 10.0, 0.9, "gradient-descent", 1, None, 0.5, 0.25, 1),
         ("A1-B5-N33-integer", "16x16x3", 1, 5, 33, 0.0, 8.0, 1.0, "gradient-descent", 1, None, 1e4, 1.0, 1),
         ("A2-B1-N2-ends", "16x16x3", 2, 1, 2, 0.5, 1.5, 0.9, "gradient-descent", 1, None, 0.5, 0.25, 1),
         ("A9-B8-N64-ends-momentum", "16x16x3", 9, 8, 64, 0.5, 1.5, 0.9, "momentum-0.5", 1, None, 0.5, 0.25, 1),
         ("A2-B5-N64-integer-adam", "16x16x3", 2, 5, 64, 0.0, 7.875, 1.0, "adam", 1, None, 0.5, 0.25, 1),
         ("A2-B8-N51-smoothed", "16x16x3", 2, 8, 51, -10.0, 10.0, 0.9, "gradient-descent", 1, SMOOTHING, 0.5, 0.25, 1),
         ("A2-B5-N33-weighted", "16x16x3", 2, 5, 33, -2.0, 8.0, 0.9, "gradient-descent", 1, None, 0.5, 0.25, 1),
         ("A2-B8-N51-nstep3", "16x16x3", 2, 8, 51, -10.0, 10.0, 0.9, "gradient-descent", 1, None, 0.5, 0.25, 3),
         ("A2-B8-N51-wide", "16x16x3", 2, 8, 51, -100.0, 100.0, 0.9, "gradient-descent", 1, None, 0.5, 0.25, 1),
         ("lowdim-A3-B8-N51-d4pg", "lowdim", 3, 8, 51, -10.0, 10.0, 0.9, "adam", 2, SMOOTHING, 0.5, 0.25, 1))
SEEDS = {c[0]: 1 for c in CASES}


def case_of(cid):
    return [c for c in CASES if c[0] == cid][0]


def dist_of(case):
    return (case[4], case[5], case[6])


def zmax_of(case):
    """max(1, max |z|): what the project's atol is scaled by for Q, td and y"""
    return max(1.0, abs(case[5]), abs(case[6]))


def hyper_of(case):
    return T3.hyper_of(case[8], case[11], case[12])._replace(discount=case[7])


def q_value_tail(spec, n_atoms, rng):
    """the q_value layer at N outputs: (online, target) float32 vectors, make_pair's perturbations"""
    _name, n_in, _n, _a, _c = spec.fc[-1]
    lim = np.sqrt(6.0 / (n_in + n_atoms))
    p = np.concatenate([(LOGIT_SCALE * rng.uniform(-lim, lim, (n_in, n_atoms))).astype(np.float32).ravel(),
                        rng.normal(0, 0.5, n_atoms).astype(np.float32)])
    return p, p + rng.normal(0, 0.05, p.shape).astype(np.float32)


def host_case(shape, B, nb, seed, n_atoms, rows=ROWS, action_dim=2, n_step=1, discount=0.9, **plain_kw):
    """tests.helpers.host_case with distributional critics: (specs, P, episodes, idxs, batches); specs[1] is dist_spec's, P[1] and P[3]
    end in the wider q_value layer.  n_step > 1: the minibatches carry the n-step columns the device's gather forms
    (cartpoleplusplus_amd.replay_memory.n_step_columns over the same store), state_2 with them."""
    from tests.helpers import host_case as plain_case
    specs, P, episodes, idxs, batches = plain_case(shape, B, nb, seed, rows=rows, action_dim=action_dim, **plain_kw)      # (dropout, actor_hidden)
    cspec = specs[1]
    _name, n_in, _one, _a, _c = cspec.fc[-1]
    cut = n_in + 1
    on, tg = q_value_tail(cspec, n_atoms, np.random.default_rng(7000 + seed))
    P = [P[0], np.concatenate([P[1][:-cut], on]), P[2], np.concatenate([P[3][:-cut], tg])]
    if n_step > 1:
        batches = n_step_batches(shape, episodes, rows, idxs, B, action_dim, n_step, discount)
    return (specs[0], dist_spec(cspec, n_atoms)), P, episodes, idxs, batches


def n_step_batches(shape, episodes, rows, idxs, B, action_dim, n, discount):
    """the minibatches of an n-step memory over host_case's episodes: reward = sum_k discount^k r_k, mask = discount^(k-1) if the walk
    ends inside an episode's live rows (0 at a terminal), state_2 of the last row walked -- tests.nstep_np's walk over the oracle memory"""
    from oracle.replay_np import OracleReplayMemory
    from tests import nstep_np as NS
    orm = OracleReplayMemory(rows, shape, action_dim)
    for ep in episodes:
        orm.add_episode(*ep)
    out = []
    for k in range(len(idxs) // B):
        ix = np.asarray(idxs[k * B:(k + 1) * B], np.int64)
        r, m, s2 = NS.columns(ix, orm.state_1_idx, orm.state_2_idx, orm.reward, orm.terminal_mask, orm.size(), orm.buffer_size, n, discount)
        out.append((np.copy(orm.state[orm.state_1_idx[ix]]), np.copy(orm.action[ix]), r, m, np.copy(orm.state[s2])))
    return out


def case_inputs(case, nb=NB, seed=None, **kw):
    cid, shape_name, A, B, N = case[:5]
    return host_case(SHAPES[shape_name], B, nb, SEEDS[cid] if seed is None else seed, N, rows=ROWS, action_dim=A, n_step=case[13],
                     discount=case[7], **kw)


def structure(case):
    """(minibatches per outer step, outer steps): the weighted case takes one minibatch per call -- the device's importance weights can
    be read back for the last minibatch of a call only"""
    return (1, NB) if "weighted" in case[0] else (NB, STEPS)


def run_case(case, inputs, dt=np.float64, fault=None, nb=None, steps=None, weights=None):
    """`steps` outer steps of `nb` minibatches (default: structure(case)), the target update behind each: (the six vectors, step counts,
    per-minibatch outputs, the restatement)"""
    if nb is None:
        nb, steps = structure(case)
    specs, P, _ep, _idxs, batches = inputs
    ref = restatement(specs, P, dist_of(case), dt, hyper_of(case), case[8], case[9], case[10], fault)
    outs = []
    for s in range(steps):
        for k in range(s * nb, (s + 1) * nb):
            ref.weights = None if weights is None else weights[k]
            o = ref.train_minibatch(batches[k])
            o.update({key: ref.last_cg[key] for key in ("p", "tp", "m", "q", "y")}, dq_da=ref.last_ag["dq_da"], actions=ref.last_ag["actions"],
                     actor_grads=ref.last_ag["grads"], critic_grads=ref.last_cg["grads"])
            outs.append(o)
        ref.update_targets()
    return R.vectors(ref), ref.state()["step"], outs, ref


def case_weights(case, nb=NB):
    """importance weights for the weighted case: lognormal, normalised to a maximum of 1 as per.hip's are"""
    rng = np.random.default_rng(78)
    out = []
    for _k in range(nb):
        w = rng.lognormal(0.0, 1.0, (case[3], 1))
        out.append((w / w.max()).astype(np.float32))
    return out


def bounds(P, want, nb):
    return R.bounds(P, want, nb)


# ---- the two bars of the GPU comparison, derived in tests/test_distributional_host.py (which re-measures and asserts these figures): the
# float32 restatement -- the learner evaluated in float32, its logits through rows_f32 -- against float64, worst over the first minibatch
# of every case whose support lies within [-10, 10]; measured 3.19e-7 for p and p', 3.93e-6 for m (N = 64 on [0.5, 1.5]: b_j carries
# the error of Tz divided by a delta of 1/63).  Each bar is the figure times 8: the margin covers the device's expf / logf and its
# reduction order in the layers below, which differ from numpy's.
F32_ERR_P, F32_ERR_M = 3.2e-7, 4.0e-6
BAR_FACTOR = 8.0
P_BAR, M_BAR = BAR_FACTOR * F32_ERR_P, BAR_FACTOR * F32_ERR_M
ATOL, GRAD_REL, PARAM_REL = 1e-5, 2e-5, R.PARAM_REL      # the suite's ordinary bars; Q, td and y take ATOL * zmax_of(case)
# dQ/da takes ATOL itself on every case within [-10, 10].  The wide case states its own: on [-100, 100] the derivative is ten times the
# [-10, 10] cases' (7.9 against 0.79 at its largest), the float32 restatement's dQ/da sits 1.303e-5 from float64 there -- beyond ATOL
# before any device runs --, and the bar is that figure times 8, as for p and m (tests/test_distributional_host.py re-measures it).
F32_ERR_DQDA_WIDE = 1.31e-5


def dqda_bar(case):
    return ATOL if zmax_of(case) <= 10.0 else BAR_FACTOR * F32_ERR_DQDA_WIDE


def f32_rows_of(case, inputs, k=0):
    """(float64 critic outputs, float32 row outputs) of minibatch k at the case's starting parameters"""
    b = inputs[4][k]
    out = {}
    for dt in (np.float64, np.float32):
        ref = restatement(inputs[0], inputs[1], dist_of(case), dt, hyper_of(case), case[8], case[9], case[10])
        out[dt] = dict(ref.critic_gradients(b), dq_da=ref.actor_gradients(b[0])["dq_da"])
    c32 = out[np.float32]
    out[np.float64]["dq_da_f32_err"] = float(np.abs(out[np.float32]["dq_da"] - out[np.float64]["dq_da"]).max())
    return out[np.float64], rows_f32(c32["logits"], c32["target_logits"], b[2], b[3], case[7], *dist_of(case))


# ---- graph replay: D4PG's learner whole on one device (Adam, smoothing, --policy-delay 2, 3-step returns, the distributional critic) on
# the rows the device draws (tests.td3_np.device_rows), the first outer step the eager pass and the capture, the others replays of ONE
# graph.  case, minibatches per step, outer steps, sample seed
GRAPH_CASE = (("d4pg-16x16x3-4x3", "16x16x3", 2, 8, 51, -10.0, 10.0, 0.9, "adam", 2, SMOOTHING, 0.5, 0.25, 3), 3, 4, 0)
GRAPH_SEED = 1


def graph_inputs(seed=None, sample_seed=None):
    case, nb, steps, ss = GRAPH_CASE
    shape, A, B, N = SHAPES[case[1]], case[2], case[3], case[4]
    specs, P, episodes, _idxs, _b = host_case(shape, B, 1, GRAPH_SEED if seed is None else seed, N, rows=ROWS, action_dim=A)
    rows = np.concatenate([T3.device_rows(ss if sample_seed is None else sample_seed, k, B, ROWS) for k in range(steps * nb)])
    return specs, P, episodes, rows, n_step_batches(shape, episodes, ROWS, rows, B, A, case[13], case[7])
