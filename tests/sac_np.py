"""Soft actor-critic (Haarnoja et al. 2018) restated in numpy, in float64 and float32: the tanh-Gaussian policy, its log-density, the
soft reward, the actor's head gradient, the temperature's gradient and Adam element, and the noise the device draws
(include/cartpolepp_abi.h, cpp_net_create_gaussian / cpp_ddpg_set_sac).  No tests here: tests/test_sac_host.py and
tests/test_gpu_sac.py share these.

    ls_k = lo + 0.5 (hi - lo) (tanh(x_k) + 1);   u_k = m_k + exp(ls_k) eps_k;   a_k = tanh(u_k)
    logp = sum_k [ -0.5 eps_k^2 - ls_k - 0.5 log(2 pi) - 2 (log 2 - u_k - softplus(-2 u_k)) ]          k ascending
    r_soft = r - (mask discount) alpha logp';   td = Q - (r_soft + mask discount Q')
    g_u = 2 alpha a_k - dq (1 - a_k^2);   d m_k = g_u;   d x_k = (g_u exp(ls_k) eps_k - alpha) 0.5 (hi - lo) (1 - tanh(x_k)^2)
    g_alpha = -(1/B) sum_b (logp_b + Hbar);   Adam (TensorFlow's semantics) on log_alpha

Every function takes `dt` (np.float64 or np.float32: each operation rounded to dt, sums over k in ascending order) and `fault`, one of
FAULTS: the planted faults of the sensitivity test."""
import numpy as np

from oracle import ddpg_np as O
from tests.helpers import philox4x32_10_np

LO, HI = -10.0, 2.0
STREAM_S1, STREAM_S2 = 0x200, 0x300
FAULTS = ("correction_1e-6", "correction_missing", "entropy_sign", "entropy_unmasked", "one_eps_for_both_draws", "eps_not_refreshed",
          "target_actor_soft_updated", "copy_before_update", "bounds_swapped", "no_2_alpha_a", "no_minus_alpha_in_dx", "no_std_eps_in_dx",
          "gradient_wrt_alpha", "adam_bias_one_step_off", "g_alpha_summed", "temperature_updated_first")


def _sum_k(t, dt):
    """sum over the last axis, ascending, each partial sum rounded to dt"""
    s = np.zeros(t.shape[:-1], dt)
    for k in range(t.shape[-1]):
        s = (s + t[..., k]).astype(dt)
    return s


def log_std(x, lo=LO, hi=HI, dt=np.float64, fault=None):
    if fault == "bounds_swapped":
        lo, hi = hi, lo
    x = np.asarray(x, dt)
    h = dt(dt(0.5) * (dt(hi) - dt(lo)))
    return (dt(lo) + (h * (np.tanh(x) + dt(1.0)).astype(dt)).astype(dt)).astype(dt)


def softplus(y, dt=np.float64):
    y = np.asarray(y, dt)
    return (np.maximum(y, dt(0)) + np.log1p(np.exp(-np.abs(y)).astype(dt)).astype(dt)).astype(dt)


def policy(m, x, eps, lo=LO, hi=HI, dt=np.float64, fault=None):
    """{ls, u, a, logp} of the head (m, x) at the noise eps, each (B, A) but logp (B)"""
    m, eps = np.asarray(m, dt), np.asarray(eps, dt)
    ls = log_std(x, lo, hi, dt, fault)
    u = (m + (np.exp(ls).astype(dt) * eps).astype(dt)).astype(dt)
    a = np.tanh(u).astype(dt)
    if fault == "correction_1e-6":
        corr = np.log(((dt(1.0) - (a * a).astype(dt)).astype(dt) + dt(1e-6)).astype(dt)).astype(dt)
    elif fault == "correction_missing":
        corr = np.zeros_like(u)
    else:
        corr = (dt(2.0) * ((dt(np.log(2.0)) - u).astype(dt) - softplus((dt(-2.0) * u).astype(dt), dt)).astype(dt)).astype(dt)
    t = ((((dt(-0.5) * (eps * eps).astype(dt)).astype(dt) - ls).astype(dt) - dt(0.5 * np.log(2.0 * np.pi))).astype(dt) - corr).astype(dt)
    return {"ls": ls, "u": u, "a": a, "logp": _sum_k(t, dt)}


def noise(seed, n, B, A, stream, dtype=np.float64, fault=None):
    """the (B, A) unclipped Box-Muller draws of pass number n on philox4x32_10({row, stream + k, n_lo, n_hi}, seed)"""
    seed, n = int(seed), int(n)
    if fault == "eps_not_refreshed":
        n = 0
    if fault == "one_eps_for_both_draws":
        stream = STREAM_S1
    b = np.repeat(np.arange(B, dtype=np.uint64), A)
    k = np.tile(np.arange(A, dtype=np.uint64), B)
    x, y, _z, _w = philox4x32_10_np(b, np.uint64(stream) + k, np.full_like(b, n & 0xFFFFFFFF), np.full_like(b, n >> 32),
                                    seed & 0xFFFFFFFF, seed >> 32)
    dt = np.dtype(dtype).type
    u1 = (((x >> np.uint64(8)) + np.uint64(1)).astype(dtype) * dt(2.0 ** -24)).astype(dtype)
    u2 = ((y >> np.uint64(8)).astype(dtype) * dt(2.0 ** -24)).astype(dtype)
    z = (np.sqrt((dt(-2.0) * np.log(u1)).astype(dtype)).astype(dtype) * np.cos(dt(2.0 * np.pi) * u2).astype(dtype)).astype(dtype)
    return z.reshape(B, A)


def soft_reward(r, mask, discount, alpha, logp2, dt=np.float64, fault=None):
    r, mask, logp2 = (np.asarray(v, dt).reshape(-1) for v in (r, mask, logp2))
    g = (mask * dt(discount)).astype(dt) if fault != "entropy_unmasked" else np.ones_like(mask)
    e = ((g * dt(alpha)).astype(dt) * logp2).astype(dt)
    return (r + e).astype(dt) if fault == "entropy_sign" else (r - e).astype(dt)


def head_gradient(x, a, eps, dq, alpha, lo=LO, hi=HI, dt=np.float64, fault=None):
    """(d m, d x), each (B, A), of sum_b (alpha logp_b - Q_b)"""
    x, a, eps, dq, alpha = np.asarray(x, dt), np.asarray(a, dt), np.asarray(eps, dt), np.asarray(dq, dt), dt(alpha)
    th = np.tanh(x).astype(dt)
    h = dt(dt(0.5) * (dt(hi) - dt(lo)))
    sd = np.exp(log_std(x, lo, hi, dt)).astype(dt)
    ent = ((dt(2.0) * alpha) * a).astype(dt) if fault != "no_2_alpha_a" else np.zeros_like(a)
    gu = (ent - (dq * (dt(1.0) - (a * a).astype(dt)).astype(dt)).astype(dt)).astype(dt)
    inner = ((gu * sd).astype(dt) * eps).astype(dt) if fault != "no_std_eps_in_dx" else gu
    if fault != "no_minus_alpha_in_dx":
        inner = (inner - alpha).astype(dt)
    dx = (inner * (h * (dt(1.0) - (th * th).astype(dt)).astype(dt)).astype(dt)).astype(dt)
    return gu, dx


def temperature_gradient(logp, hbar, alpha=None, rows_per_part=4, fault=None):
    """g_alpha = -(1/B) sum_b (logp_b + Hbar): f64 partials of rows_per_part rows, added in order, rounded to f32 once"""
    t = np.asarray(logp, np.float64).reshape(-1) + np.float64(np.float32(hbar))
    B = len(t)
    s = 0.0
    for i in range(0, B, rows_per_part):
        p = 0.0
        for v in t[i:i + rows_per_part]:
            p += v
        s += p
    g = -s if fault == "g_alpha_summed" else -(s / B)
    if fault == "gradient_wrt_alpha":       # d/d alpha of -alpha (logp + Hbar) instead of d/d log_alpha of -log_alpha (logp + Hbar)
        g = g / float(alpha)
    return np.float32(g)


def adam(p, g, m, v, t, lr, beta1=0.9, beta2=0.999, epsilon=1e-8, dt=np.float32, fault=None):
    """TensorFlow's Adam element on one parameter; t: the count INCLUDING this apply.  Returns (p, m, v)"""
    p, g, m, v = dt(p), dt(g), dt(m), dt(v)
    tt = float(t - 1 if fault == "adam_bias_one_step_off" and t > 1 else (t + 1 if fault == "adam_bias_one_step_off" else t))
    lr_t = dt(float(np.float32(lr)) * np.sqrt(1.0 - float(np.float32(beta2)) ** tt) / (1.0 - float(np.float32(beta1)) ** tt))
    b1, b2 = dt(np.float32(beta1)), dt(np.float32(beta2))
    m = dt(b1 * m + dt((dt(1) - b1) * g))
    v = dt(b2 * v + dt(dt((dt(1) - b2) * g) * g))
    p = dt(p - dt(dt(lr_t * m) / dt(np.sqrt(v) + dt(np.float32(epsilon)))))
    return p, m, v


# ---- the learner: oracle.DDPG with a Gaussian actor ------------------------------------------------------------------------------------
def gaussian_spec(action_dim, hidden, **kw):
    """O.NetSpec of an actor whose output_action is linear and 2A wide: (m | x)"""
    s = O.NetSpec("actor", action_dim, hidden, **kw)
    name, n_in, _n_out, _act, cat = s.fc[-1]
    s.fc[-1] = (name, n_in, 2 * int(action_dim), "linear", cat)
    return s


class SacState(object):
    """the temperature and its Adam state, the noise count"""

    def __init__(self, init_temperature=0.1, target_entropy=-2.0, lr=1e-4, seed=0):
        self.log_alpha = np.float32(np.log(np.float32(init_temperature)))
        self.m, self.v, self.step, self.n = np.float32(0), np.float32(0), 0, 0
        self.hbar, self.lr, self.seed = float(target_entropy), float(lr), int(seed)


class SacDDPG(O.DDPG):
    """oracle.DDPG (ddpg_cartpole.py:102-119, :186-218) as a soft actor-critic learner.  The target actor is the actor as it stood before
    the minibatch's actor update.  eps1 / eps2: the (B, A) noise of the two draws, the device's own in the GPU tests."""

    def __init__(self, actor_spec, critic_spec, actor_flat, critic_flat, dt=np.float64, hyper=O.DEFAULT_HYPER, lo=LO, hi=HI, state=None):
        O.DDPG.__init__(self, actor_spec, critic_spec, actor_flat, critic_flat, dt, hyper)
        self.lo, self.hi = lo, hi
        self.sac = state or SacState(target_entropy=-float(actor_spec.action_dim))
        self.target_actor = O.Net(actor_spec, np.asarray(actor_flat), dt)
        self.target_log_alpha = self.sac.log_alpha
        self._soft = O.Net(actor_spec, np.asarray(actor_flat), dt)      # (what a soft-updated target actor would hold: a fault's)

    def _A(self):
        return self.actor.spec.action_dim

    def _head(self, net, s, white, training=True):
        c = net.forward(s, white=white, training=training)
        A = self._A()
        return c, c["out"][:, :A], c["out"][:, A:]

    def action_given(self, state):
        _c, m, _x = self._head(self.actor, np.asarray(state)[None], None, training=False)
        return np.tanh(m)

    def actor_gradients(self, s1, eps1=None, fault=None):
        dt = self.dt
        alpha = dt(np.exp(np.float64(self.sac.log_alpha)))
        w1 = self._white(self.actor, s1)
        ca, m, x = self._head(self.actor, s1, w1)
        eps = np.zeros_like(m) if eps1 is None else np.asarray(eps1, dt)
        pol = policy(m, x, eps, self.lo, self.hi, dt, fault)
        cc = self.critic.forward(s1, action=pol["a"], white=w1)
        _, dq = self.critic.backward(cc, np.ones_like(cc["out"]), params=False)
        dm, dx = head_gradient(x, pol["a"], eps, dq, alpha, self.lo, self.hi, dt, fault)
        grads, _ = self.actor.backward(ca, np.concatenate([dm, dx], axis=1))
        g_alpha = temperature_gradient(pol["logp"], self.sac.hbar, alpha, fault=fault)
        return {"actions": pol["a"], "logp": pol["logp"], "q": cc["out"], "dq_da": dq, "dm": dm, "dx": dx, "alpha": alpha, "g_alpha": g_alpha,
                "grads": O.flatten(self.actor.spec, grads, dt), "m": m, "x": x, "eps": eps}

    def critic_gradients(self, batch, eps2=None, training=True, fault=None, weights=None):
        s1, a, r, mask, s2 = batch
        dt = self.dt
        alpha = dt(np.exp(np.float64(self.target_log_alpha)))
        w2 = self._white(self.target_actor, s2)
        _c, m, x = self._head(self.target_actor, s2, w2, training)
        eps = np.zeros_like(m) if eps2 is None else np.asarray(eps2, dt)
        pol = policy(m, x, eps, self.lo, self.hi, dt, fault)
        tq = self.target_critic.forward(s2, action=pol["a"], white=w2, training=training)
        rs = soft_reward(r, mask, self.hp.discount, alpha, pol["logp"], dt, fault).reshape(-1, 1)
        y = rs + np.asarray(mask, dt).reshape(-1, 1) * dt(self.hp.discount) * tq["out"]
        cb = self.critic.forward(s1, action=np.asarray(a, dt), training=training)
        td = cb["out"] - y
        B = td.shape[0]
        w = np.ones_like(td) if weights is None else np.asarray(weights, dt).reshape(td.shape)
        loss = (w * td * td).mean(dtype=dt)
        grads, _ = self.critic.backward(cb, (dt(2.0) * w * td / dt(B)).astype(dt))
        return {"q": cb["out"], "td": td, "loss": loss, "target_q": tq["out"], "target_actions": pol["a"], "logp2": pol["logp"], "r_soft": rs[:, 0],
                "m2": m, "x2": x, "grads": O.flatten(self.critic.spec, grads, dt)}

    def update_temperature(self, g_alpha, fault=None):
        s = self.sac
        if s.lr <= 0.0:
            return
        s.step += 1
        s.log_alpha, s.m, s.v = adam(s.log_alpha, g_alpha, s.m, s.v, s.step, s.lr, fault=fault)

    def train_minibatch(self, batch, eps1=None, eps2=None, fault=None, weights=None):
        """actor.train(s1) then critic.train(batch) on one snapshot; gradient descent on both lists (the other rules: the device's own
        tests); then the temperature, then the copy that makes the target actor the updated actor"""
        dt, hp = self.dt, self.hp
        if fault == "temperature_updated_first":      # both passes then read the temperature this minibatch's update left
            self.update_temperature(self.actor_gradients(batch[0], eps1)["g_alpha"])
            self.target_log_alpha = self.sac.log_alpha
        if fault == "target_actor_soft_updated":      # a' from a lagging target actor that only soft updates move
            self.target_actor = self._soft
        ag = self.actor_gradients(batch[0], eps1, fault)
        a_clip, a_norm = O.clip_by_global_norm(ag["grads"], hp.gradient_clip, dt)
        new_a = (self.actor.flat() - dt(hp.actor_lr) * a_clip).astype(dt)
        if fault == "copy_before_update":      # the target of THIS minibatch is already the updated actor
            self.target_actor = O.Net(self.actor.spec, new_a, dt)
        cg = self.critic_gradients(batch, eps2, fault=fault, weights=weights)
        c_clip, c_norm = O.clip_by_global_norm(cg["grads"], hp.gradient_clip, dt)
        new_c = (self.critic.flat() - dt(hp.critic_lr) * c_clip).astype(dt)
        self.actor = O.Net(self.actor.spec, new_a, dt)
        self.critic = O.Net(self.critic.spec, new_c, dt)
        if fault != "temperature_updated_first":
            self.update_temperature(ag["g_alpha"], fault)
        self.target_actor = O.Net(self.actor.spec, new_a, dt)
        self.target_log_alpha = self.sac.log_alpha
        self.sac.n += 1
        out = {"actor_grads": ag["grads"], "critic_grads": cg["grads"], "actor_norm": a_norm, "critic_norm": c_norm,
               "log_alpha": self.sac.log_alpha}
        out.update({k: ag[k] for k in ("actions", "logp", "dq_da", "dm", "dx", "alpha", "g_alpha", "m", "x")})
        out.update({k: cg[k] for k in ("q", "td", "loss", "target_q", "target_actions", "logp2", "r_soft", "m2", "x2")})
        return out

    def update_targets(self):      # the critic's alone: the target actor is a copy
        self._soft = O.Net(self.actor.spec, O.soft_update(self._soft.flat(), self.actor.flat(), self.hp.target_update_rate, self.dt), self.dt)
        self.target_critic = O.Net(self.critic.spec, O.soft_update(self.target_critic.flat(), self.critic.flat(), self.hp.target_update_rate,
                                                                   self.dt), self.dt)


# ---- the GPU test's cases, made on the host so that the host test derives its bars from the same numbers ---------------------------------
BATCHES = (1, 3, 5, 64, 65, 257)
ACTION_DIMS = (1, 2, 3, 8, 16)      # (a trainer's critic takes action dimensions up to 16; the forward entry points are held at 64 too)
CASES = [(B, A) for B in BATCHES for A in ((2,) if B not in (5, 65) else ACTION_DIMS)]
P_BAR = 1e-5          # the project's bar on a, Q, td and dQ/da


def head_case(B, A, seed=0):
    """(m, x, eps1, eps2, dq, r, mask) of one case: heads wide enough that a tenth of the actions saturates (|a| > 0.99), a tenth stays
    small (|a| < 0.5) and the pre-activations x reach both tails of the bound"""
    rng = np.random.default_rng(1000 * B + A + seed)
    n = B * A
    m = rng.normal(0.0, 1.0, n)
    m[rng.permutation(n)[:max(1, n // 4)]] *= 0.2
    sat = rng.permutation(n)[:max(1, (n + 3) // 4)]
    m[sat] = np.sign(m[sat] + 1e-3) * rng.uniform(3.0, 6.0, len(sat))
    x = rng.normal(0.0, 1.5, n)
    x[rng.permutation(n)[:max(1, n // 6)]] = rng.uniform(2.5, 4.0, max(1, n // 6))
    x[rng.permutation(n)[:max(1, n // 6)]] = rng.uniform(-4.0, -2.5, max(1, n // 6))
    if n >= 2:
        x[0], x[-1] = 3.0, -3.0
    f = lambda v: np.asarray(v, np.float32).reshape(B, A)
    return {"m": f(m), "x": f(x), "eps1": noise(7, 0, B, A, STREAM_S1, np.float32), "eps2": noise(7, 0, B, A, STREAM_S2, np.float32),
            "dq": f(rng.normal(0, 1.0, n)), "r": rng.normal(0, 1, B).astype(np.float32),
            "mask": (rng.uniform(size=B) > 0.2).astype(np.float32), "alpha": np.float32(0.2), "discount": np.float32(0.9), "hbar": -float(A)}


def rows_of(case, dt, fault=None):
    """every row-local quantity of one head case in precision dt"""
    p1 = policy(case["m"], case["x"], case["eps1"], LO, HI, dt, fault)
    e2 = case["eps1"] if fault == "one_eps_for_both_draws" else case["eps2"]
    p2 = policy(case["m"], case["x"], e2, LO, HI, dt, fault)
    dm, dx = head_gradient(case["x"], p1["a"], case["eps1"], case["dq"], case["alpha"], LO, HI, dt, fault)
    rs = soft_reward(case["r"], case["mask"], case["discount"], case["alpha"], p2["logp"], dt, fault)
    g = temperature_gradient(p1["logp"], case["hbar"], case["alpha"], fault=fault)
    la, m, v = np.float32(np.log(case["alpha"])), np.float32(0), np.float32(0)
    for t in range(1, 4):
        la, m, v = adam(la, g, m, v, t, 1e-2, fault=fault)
    return {"a": p1["a"], "logp": p1["logp"], "a2": p2["a"], "logp2": p2["logp"], "r_soft": rs, "dm": dm, "dx": dx, "g_alpha": g, "log_alpha": la,
            "u": p1["u"]}


ROW_KEYS = ("logp", "r_soft", "dm", "dx", "g_alpha", "log_alpha")


def measured_error(key, cases=None):
    """the float32 restatement's worst absolute error against float64 over the GPU test's cases"""
    worst = 0.0
    for B, A in (cases or CASES):
        c = head_case(B, A)
        f64, f32 = rows_of(c, np.float64), rows_of(c, np.float32)
        k2 = (key, key + "2") if key == "logp" else (key,)
        for k in k2:
            worst = max(worst, float(np.max(np.abs(np.asarray(f64[k], np.float64) - np.asarray(f32[k], np.float64)))))
    return worst


def bar(key, cases=None):
    """the GPU bar of a row-local quantity: 8x the float32 restatement's worst error (the device's library functions and its reduction
    orders), the project's 1e-5 wherever that product is below a quarter of it"""
    if key in ("a", "a2", "q", "td", "dq_da"):
        return P_BAR
    b = 8.0 * measured_error(key, cases)
    return P_BAR if b < P_BAR / 4 else b


def eps_bar():
    """|z_f32 - z_f64| of the Box-Muller draw over the cases' draws, times 8, by the same rule"""
    worst = 0.0
    for B, A in CASES:
        for s in (STREAM_S1, STREAM_S2):
            worst = max(worst, float(np.max(np.abs(noise(7, 0, B, A, s, np.float64) - noise(7, 0, B, A, s, np.float32).astype(np.float64)))))
    b = 8.0 * worst
    return P_BAR if b < P_BAR / 4 else b
