"""Feature layer norm (Linear -> LayerNorm -> tanh / relu on the first fully connected layer of a pixel network: the trunk of DrQ-v2;
include/cartpolepp_abi.h, cpp_net_create_feature_norm) restated on the float64 oracle:

    z = [x, 1][W; b]            mu = mean_j z_j         var = mean_j (z_j - mu)^2       (biased, two passes)
    rstd = 1 / sqrt(var + eps)  xhat = (z - mu) rstd    u = gamma xhat + beta           y = act(u)
    du = g act'(y)              dgamma = sum_b du xhat  dbeta = sum_b du
    dxh = du gamma              dz = rstd ((dxh - mean_j dxh) - xhat mean_j(dxh xhat))

LnSpec is an oracle NetSpec whose layout() ends in '<layer0>/LayerNorm/gamma' and '.../beta' -- behind every other variable, as in the
device's flat buffer -- and LnNet an oracle Net that normalises layer 0.  with_feature_norm(Base) makes any of the DDPG restatements
(oracle.ddpg_np.DDPG, tests.ddpg_opt_np.DDPGWithOptimiser, tests.td3_np.DelayedDDPG with or without smoothing, tests.twin_np.TwinDDPG,
tests.dist_np.DistDDPG, tests.quant_np.QuantDDPG, tests.sac_np.SacDDPG) run on such networks:
every network they create for an LnSpec becomes an LnNet, and since their gradient lists, clips, optimiser slots and target updates run
over spec.layout(), the two variables are covered with no further work.  Also the cases the CPU and the GPU tests share, and the faults
the CPU test plants.  Test-only: product code never imports it."""
import collections

import numpy as np

from oracle import ddpg_np as O

EPS = 1e-5                                     # what the Python surface passes (torch.nn.LayerNorm's default)
FAULTS = ("no_mean_dxh",                       # the `mean dxh` term dropped
          "no_xhat_term",                      # the `xhat mean(dxh xhat)` term dropped
          "unbiased_variance",                 # var over n - 1
          "eps_outside_root",                  # 1 / (sqrt(var) + eps)
          "gamma_missing_from_dxh",
          "dgamma_from_u",                     # dgamma = sum_b du u
          "act_grad_at_wrong_layer",           # the activation's derivative taken at z, the GEMM's output, instead of at u
          "relu_mask_for_tanh",                # (tanh cases) y > 0 where 1 - y^2 belongs
          "norm_vars_outside_clip_norm",       # the clip's global norm over the plain variables only
          "norm_vars_not_in_target_update")    # gamma / beta of the targets left where they were
NET_FAULTS = FAULTS[:8]


class LnSpec(O.NetSpec):
    """an oracle NetSpec whose layer 0 is Linear -> LayerNorm -> `ln_act`"""

    def __init__(self, kind, action_dim, hidden, ln_act="tanh", eps=EPS, **kw):
        assert kw.get("pixel", False) and not kw.get("batch_norm", False) and not kw.get("dropout", False)
        assert ln_act in ("tanh", "relu")
        self.ln_act, self.eps = ln_act, float(eps)
        super(LnSpec, self).__init__(kind, action_dim, hidden, **kw)

    def _fc_layers(self):
        fc = super(LnSpec, self)._fc_layers()
        name, n_in, n_out, _act, cat = fc[0]
        fc[0] = (name, n_in, n_out, "linear", cat)      # (the GEMM has no activation of its own)
        return fc

    def plain_layout(self):
        return super(LnSpec, self).layout()

    def ln_names(self):
        return self.fc[0][0] + "/LayerNorm/gamma", self.fc[0][0] + "/LayerNorm/beta"

    def layout(self):
        n = self.fc[0][2]
        return list(self.plain_layout()) + [(self.ln_names()[0], (n,)), (self.ln_names()[1], (n,))]

    def num_plain(self):
        return int(sum(int(np.prod(s)) for _n, s in self.plain_layout()))


def init_params(spec, rng):
    """oracle.init_params for the plain variables, gamma = 1, beta = 0"""
    parts = []
    for name, shape in spec.layout():
        if name.endswith("/biases") or name.endswith("/LayerNorm/beta"):
            parts.append(np.zeros(shape, np.float32))
        elif name.endswith("/LayerNorm/gamma"):
            parts.append(np.ones(shape, np.float32))
        elif name.startswith("output_action"):
            parts.append(rng.uniform(-1e-3, 1e-3, shape).astype(np.float32))
        else:
            fan_in, fan_out = (shape[0] * shape[1] * shape[2], shape[0] * shape[1] * shape[3]) if len(shape) == 4 else shape
            lim = np.sqrt(6.0 / (fan_in + fan_out))
            parts.append(rng.uniform(-lim, lim, shape).astype(np.float32))
    return np.concatenate([p.ravel() for p in parts])


def ln_forward(z, gamma, beta, act, eps, dt, fault=None):
    n = z.shape[1]
    mu = (z.sum(axis=1, keepdims=True, dtype=dt) / dt(n)).astype(dt)
    d = (z - mu).astype(dt)
    var = ((d * d).sum(axis=1, keepdims=True, dtype=dt) / dt(n - 1 if fault == "unbiased_variance" else n)).astype(dt)
    rstd = (dt(1.0) / (np.sqrt(var) + dt(eps))) if fault == "eps_outside_root" else (dt(1.0) / np.sqrt(var + dt(eps)))
    rstd = rstd.astype(dt)
    xhat = (d * rstd).astype(dt)
    u = (gamma * xhat + beta).astype(dt)
    return {"z": z, "mu": mu, "var": var, "rstd": rstd, "xhat": xhat, "u": u, "y": O._act(u, act).astype(dt)}


def ln_backward(g, ln, gamma, act, dt, fault=None):
    """(dz, dgamma, dbeta) from g = dL/dy"""
    n = g.shape[1]
    y, xhat = ln["y"], ln["xhat"]
    if fault == "act_grad_at_wrong_layer":
        y = O._act(ln["z"], act).astype(dt)
    if fault == "relu_mask_for_tanh" and act == "tanh":
        du = np.where(y > 0, g, 0).astype(dt)
    else:
        du = O._act_bwd(g, y, act).astype(dt)
    dgamma = (du * (ln["u"] if fault == "dgamma_from_u" else xhat)).sum(axis=0, dtype=dt)
    dbeta = du.sum(axis=0, dtype=dt)
    dxh = du if fault == "gamma_missing_from_dxh" else (du * gamma).astype(dt)
    m1 = (dxh.sum(axis=1, keepdims=True, dtype=dt) / dt(n)).astype(dt)
    m2 = ((dxh * xhat).sum(axis=1, keepdims=True, dtype=dt) / dt(n)).astype(dt)
    t = dxh if fault == "no_mean_dxh" else (dxh - m1)
    if fault != "no_xhat_term":
        t = t - xhat * m2
    return (ln["rstd"] * t).astype(dt), dgamma, dbeta


class LnNet(O.Net):
    """oracle Net over an LnSpec: the trunk and the layers above layer 0 are the oracle's, layer 0 is normalised.  c['ln']: what the
    layer held (z, mu, var, rstd, xhat, u, y); after a backward also dz, dgamma, dbeta."""
    fault = None

    def forward(self, state, action=None, white=None, training=True):
        sp, dt = self.spec, self.dt
        # (the oracle's forward: the trunk, and layer 0 as the plain GEMM its spec says -- the layers above are redone below)
        c = O.Net.forward(self, state, action=None if action is None else action, white=white, training=training)
        B = c["B"]
        h0, z = c["fc"][0]
        gname, bname = sp.ln_names()
        ln = ln_forward(z, self.p[gname], self.p[bname], sp.ln_act, sp.eps, dt, self.fault)
        c["ln"] = ln
        c["fc"] = [(h0, ln["y"])]
        h = ln["y"]
        for name, _n_in, _n_out, act, cat in sp.fc[1:]:
            if cat:
                h = np.concatenate([h, np.asarray(action, dtype=dt).reshape(B, -1)], axis=1)
            y = O._act(h @ self.p[name + "/weights"] + self.p[name + "/biases"], act)
            c["fc"].append((h, y))
            h = y
        c["out"] = h
        return c

    def backward(self, c, dout, params=True):
        sp, dt = self.spec, self.dt
        g = collections.OrderedDict()
        d_action = None
        dh = np.asarray(dout, dtype=dt)
        for (name, n_in, _n_out, act, cat), (h, y) in reversed(list(zip(sp.fc[1:], c["fc"][1:]))):
            dz = O._act_bwd(dh, y, act)
            if params:
                g[name + "/biases"] = dz.sum(axis=0)
                g[name + "/weights"] = h.T @ dz
            dh = dz @ self.p[name + "/weights"].T
            if cat:
                d_action = dh[:, n_in - sp.action_dim:]
                dh = dh[:, :n_in - sp.action_dim]
                if not params:
                    return None, d_action
        if not params:
            return None, d_action
        name = sp.fc[0][0]
        gname, bname = sp.ln_names()
        dz, g[gname], g[bname] = ln_backward(dh, c["ln"], self.p[gname], sp.ln_act, dt, self.fault)
        c["ln"].update(g=dh, dz=dz, dgamma=g[gname], dbeta=g[bname])
        g[name + "/biases"] = dz.sum(axis=0)
        g[name + "/weights"] = c["fc"][0][0].T @ dz
        dh = dz @ self.p[name + "/weights"].T
        c["d_flat"] = dh
        g.update(self.backward_trunk(c, dh.reshape(c["pool_shape"])))
        return collections.OrderedDict((n, g[n]) for n, _s in sp.layout()), d_action


def _twin():
    from tests import twin_np as W
    return W


def twin_critic_class():
    """tests.twin_np.TwinCritic over an LnSpec: head 1 is an LnNet, the shared layers' backward goes through the norm.  Its flat vector is
    in tests.twin_np.full_layout's order, [plain | gamma beta | twin]; the device's is [plain | twin | gamma beta]: twin_to_device /
    twin_from_device permute at the boundary."""
    W = _twin()
    if "cls" in _twin_made:
        return _twin_made["cls"]

    class LnTwinCritic(W.TwinCritic):
        def backward(self, c, dout1, dout2=None, params=True, share_head2=True):
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
            for (name, _ni, _no, act, _cat), (h, y) in reversed(list(zip(sp.fc[1:self.k], c["fc"][1:self.k]))):
                dz = O._act_bwd(dh, y, act)
                g[name + "/biases"] = dz.sum(axis=0)
                g[name + "/weights"] = h.T @ dz
                dh = dz @ self.h1.p[name + "/weights"].T
            name = sp.fc[0][0]
            gname, bname = sp.ln_names()
            dz, g[gname], g[bname] = ln_backward(dh, c["ln"], self.h1.p[gname], sp.ln_act, dt, self.h1.fault)
            c["ln"].update(g=dh, dz=dz, dgamma=g[gname], dbeta=g[bname])
            g[name + "/biases"] = dz.sum(axis=0)
            g[name + "/weights"] = c["fc"][0][0].T @ dz
            g.update(self.h1.backward_trunk(c, (dz @ self.h1.p[name + "/weights"].T).reshape(c["pool_shape"])))
            return collections.OrderedDict((n, g[n]) for n, _s in W.full_layout(sp)), d_action

    _twin_made["cls"] = LnTwinCritic
    return LnTwinCritic


_twin_made = {}


def twin_to_device(spec, v):
    """[plain | gamma beta | twin] -> the device's [plain | twin | gamma beta]"""
    k, n = spec.num_plain(), 2 * spec.fc[0][2]
    return np.concatenate([v[:k], v[k + n:], v[k:k + n]])


def twin_from_device(spec, v):
    k, n = spec.num_plain(), 2 * spec.fc[0][2]
    return np.concatenate([v[:k], v[len(v) - n:], v[k:len(v) - n]])


class _Adopts(object):
    """every oracle Net this restatement is handed for an LnSpec becomes an LnNet (the classes build their networks with oracle.Net), and
    every tests.twin_np.TwinCritic over an LnSpec the twin critic above"""
    net_fault = None

    def __setattr__(self, key, value):
        if type(value) is O.Net and isinstance(value.spec, LnSpec):
            value.__class__ = LnNet
            if self.net_fault is not None:
                value.fault = self.net_fault
        elif type(value).__name__ == "TwinCritic" and isinstance(value.spec, LnSpec):
            value.__class__ = twin_critic_class()
            value.h1.__class__ = LnNet
        object.__setattr__(self, key, value)


_made = {}


def with_feature_norm(Base):
    if Base not in _made:
        _made[Base] = type("FeatureNorm" + Base.__name__, (_Adopts, Base), {})
    return _made[Base]


class LnDDPG(with_feature_norm(O.DDPG)):
    """oracle.DDPG on normalised networks, with the two faults that live above the networks"""

    def __init__(self, *a, **kw):
        self.ddpg_fault = kw.pop("fault", None)
        if self.ddpg_fault in NET_FAULTS:
            self.net_fault = self.ddpg_fault
        super(LnDDPG, self).__init__(*a, **kw)

    def train_minibatch(self, batch):
        if self.ddpg_fault != "norm_vars_outside_clip_norm":
            return super(LnDDPG, self).train_minibatch(batch)
        dt, hp = self.dt, self.hp
        ag, cg = self.actor_gradients(batch[0]), self.critic_gradients(batch)
        out = {}
        for which, gr, lr in (("actor", ag["grads"], hp.actor_lr), ("critic", cg["grads"], hp.critic_lr)):
            net = getattr(self, which)
            _c, norm = O.clip_by_global_norm(gr[:net.spec.num_plain()], hp.gradient_clip, dt)
            scale = dt(1.0) if hp.gradient_clip is None else dt(hp.gradient_clip) * min(dt(1.0) / norm, dt(1.0) / dt(hp.gradient_clip))
            setattr(self, which, O.Net(net.spec, (net.flat() - dt(lr) * (np.asarray(gr, dt) * scale)).astype(dt), dt))
            out[which + "_norm"] = norm
        out.update(td=cg["td"], loss=cg["loss"], q=cg["q"], actions=ag["actions"], dq_da=ag["dq_da"], actor_grads=ag["grads"], critic_grads=cg["grads"])
        return out

    def update_targets(self):
        old = [self.target_actor.flat(), self.target_critic.flat()]
        super(LnDDPG, self).update_targets()
        if self.ddpg_fault == "norm_vars_not_in_target_update":
            for which, o in zip(("target_actor", "target_critic"), old):
                net = getattr(self, which)
                f, k = net.flat(), net.spec.num_plain()
                f[k:] = o[k:]
                setattr(self, which, O.Net(net.spec, f, self.dt))


def specs_for(shape, actor_hidden, ln_act="tanh", action_dim=2, eps=EPS):
    kw = dict(pixel=True, H=shape[0], W=shape[1], C=int(np.prod(shape[2:])))
    return (LnSpec("actor", action_dim, list(actor_hidden), ln_act, eps, **kw), LnSpec("critic", action_dim, [], ln_act, eps, **kw))


def restatement(specs, P, dt=np.float64, hyper=O.DEFAULT_HYPER, fault=None):
    ref = LnDDPG(specs[0], specs[1], P[0], P[1], dt, hyper, fault=fault)
    ref.set_targets(P[2], P[3])
    return ref


def host_case(shape, B, nb, seed, actor_hidden, ln_act="tanh", rows=24, action_dim=2, spread=0.5, layer0_scale=1.0, critic_atoms=0, gaussian=False):
    """tests.helpers.host_case for normalised networks: specs, the four parameter vectors (xavier + perturbations; gamma and beta perturbed
    by `spread` so that neither is the identity; critic_atoms: the width of a distributional / quantile critic's q_value; gaussian: a soft actor-critic actor; layer0_scale: layer 0's weights and biases times that), episodes, rows and the minibatches they select"""
    from oracle.replay_np import OracleReplayMemory
    specs = specs_for(shape, actor_hidden, ln_act, action_dim)
    if critic_atoms:      # a distributional or quantile critic: q_value (n_in, N), in its place of the layout
        from tests import dist_np
        specs = (specs[0], dist_np.dist_spec(specs[1], critic_atoms))
    if gaussian:          # a Gaussian actor: output_action is linear and 2A wide, (m | x), as tests.sac_np.gaussian_spec's
        name, n_in, _n_out, _act, cat = specs[0].fc[-1]
        specs[0].fc[-1] = (name, n_in, 2 * int(action_dim), "linear", cat)
    rng = np.random.default_rng(3000 + seed)
    P = []
    for spec in specs:
        p = init_params(spec, rng)
        p = p + rng.normal(0, 0.05, p.shape).astype(np.float32)
        k = spec.num_plain()
        p[k:] += rng.normal(0, spread, len(p) - k).astype(np.float32)
        if layer0_scale != 1.0:      # a quiet layer 0: var of the order of eps, so that where eps sits shows
            off = 0
            for name, shp in spec.layout():
                n = int(np.prod(shp))
                if name in (spec.fc[0][0] + "/weights", spec.fc[0][0] + "/biases"):
                    p[off:off + n] *= np.float32(layer0_scale)
                off += n
        P.append(p.astype(np.float32))
    for p in list(P):
        P.append((p + rng.normal(0, 0.01, p.shape)).astype(np.float32))
    orm = OracleReplayMemory(rows, shape, action_dim)
    mk = lambda: rng.integers(0, 256, shape).astype(np.float16) / np.float16(255)
    episodes, left = [], rows
    while left > 0:
        n = min(left, int(rng.integers(2, 7)))
        episodes.append((mk(), [(rng.uniform(-1, 1, (1, action_dim)).astype(np.float32), float(rng.integers(0, 3)), mk()) for _ in range(n)]))
        orm.add_episode(*episodes[-1])
        left -= n
    idxs = rng.integers(0, rows, nb * B).astype(np.int32)
    batches = []
    for i in range(nb):
        ob = orm.batch(idxs=idxs[i * B:(i + 1) * B])
        batches.append((ob.state_1, ob.action, ob.reward, ob.terminal_mask, ob.state_2))
    return specs, P, episodes, idxs, batches


def dead_layer(P, specs, constant=0.5):
    """layer-0 weights zero and biases one constant in all four networks: var = 0 exactly in both precisions (the constant and n times
    the constant are exact floats), so xhat = 0, y = act(beta) and rstd = 1 / sqrt(eps)"""
    out = []
    for p, spec in zip(P, (specs[0], specs[1], specs[0], specs[1])):
        p, off = p.copy(), 0
        for name, shp in spec.layout():
            n = int(np.prod(shp))
            if name == spec.fc[0][0] + "/weights":
                p[off:off + n] = 0.0
            if name == spec.fc[0][0] + "/biases":
                p[off:off + n] = constant
            off += n
        out.append(p)
    return out


# ---- the compared quantities of one minibatch's gradient pass and the house rule for their bars
LN_QUANTITIES = ("xhat", "rstd", "y", "dz", "dgamma", "dbeta")


def ln_quantities(ref, batch):
    """{'actor' / 'critic': {quantity: array}} and the pass's other outputs, from one actor and one critic gradient pass"""
    ag, cg = ref.actor_gradients(batch[0]), ref.critic_gradients(batch)
    out = {}
    for name, cache in (("actor", ag["cache_actor"]), ("critic", cg["cache_critic"])):
        ln = cache["ln"]
        out[name] = {k: np.asarray(ln[k], np.float64).reshape(-1) if k == "rstd" else np.asarray(ln[k], np.float64) for k in LN_QUANTITIES}
        out[name]["u"] = np.asarray(ln["u"], np.float64)
        out[name]["sd"] = np.sqrt(np.asarray(ln["var"], np.float64)).reshape(-1)
    return out, ag, cg


def rel_err(got, want):
    """largest absolute error over the largest magnitude of the reference (at least 1e-30)"""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    return float(np.abs(got - want).max() / max(float(np.abs(want).max()), 1e-30))


ORDINARY_BAR = 1e-5


def derived_bar(twin_err):
    """the house rule: 8 x the float32 twin's own error against float64, or the ordinary 1e-5 where that product is below a quarter of it"""
    return ORDINARY_BAR if 8.0 * twin_err < 0.25 * ORDINARY_BAR else 8.0 * twin_err


def conditions(q, act):
    """the conditions a case must meet, on the float64 quantities alone; returns the first that fails, or None"""
    for name in ("actor", "critic"):
        sd, u = q[name]["sd"], q[name]["u"]
        if sd.min() < 0.05 * np.median(sd):
            return "%s: a row's sqrt(var) %.3e below 0.05 of the median %.3e" % (name, sd.min(), np.median(sd))
        if act == "tanh":
            if (np.abs(u) > 1).mean() < 0.1 or (np.abs(u) < 0.5).mean() < 0.1:
                return "%s: tanh units %.2f beyond 1, %.2f inside 0.5" % (name, (np.abs(u) > 1).mean(), (np.abs(u) < 0.5).mean())
        elif (u > 0).mean() < 0.1 or (u < 0).mean() < 0.1:
            return "%s: relu units %.2f above 0" % (name, (u > 0).mean())
    return None


# ---- the cases of the kernel-edge test (tests/test_gpu_layer_norm.py) and of the CPU test that derives their bars: 16x16x6 images
EDGE_SHAPE, EDGE_ROWS = (16, 16, 3, 1, 2), 24
# (id, layer-0 width of the actor, B, activation): every width with one B, every B with one width, both activations
EDGE_CASES = [("w5-b3-tanh", 5, 3, "tanh"), ("w64-b5-tanh", 64, 5, "tanh"), ("w65-b33-tanh", 65, 33, "tanh"), ("w333-b1-relu", 333, 1, "relu"),
              ("w1024-b3-relu", 1024, 3, "relu"), ("w65-b1-tanh", 65, 1, "tanh"), ("w65-b5-relu", 65, 5, "relu"),
              ("w64-b5-tanh-quiet", 64, 5, "tanh")]      # quiet: layer 0 times 0.01 -- sqrt(var) of the order of sqrt(eps)
QUIET_SCALE = 0.01
EDGE_TAIL = (20, 10)                           # the actor's hidden layers behind layer 0: three hidden layers, the default route
SEEDS = range(1, 40)


def edge_case(cid, dead=False):
    """host_case of an EDGE_CASES id on the first seed on which conditions() hold (a dead layer: seed 1)"""
    _cid, width, B, act = [c for c in EDGE_CASES if c[0] == cid][0]
    for seed in SEEDS:
        case = host_case(EDGE_SHAPE, B, 1, seed, (width,) + EDGE_TAIL, act, rows=EDGE_ROWS, layer0_scale=QUIET_SCALE if cid.endswith("quiet") else 1.0)
        if dead:
            return (case[0], dead_layer(case[1], case[0])) + case[2:] + (seed,)
        q, _ag, _cg = ln_quantities(restatement(case[0], case[1]), case[4][0])
        if conditions(q, act) is None:
            return case + (seed,)
    raise AssertionError("no seed of %s meets the conditions for %s" % (list(SEEDS), cid))


def pinned_twin(specs, P, batch, hyper=O.DEFAULT_HYPER, fault=None, dt=np.float32):
    """ln_quantities of another evaluation (the float32 twin, or a faulted float64 one) on the float64 evaluation's pool and ReLU routes:
    rounding -- or the fault -- is what is compared, not a flipped tie.  Returns (float64 quantities, ag, cg, the other's quantities, ag, cg)"""
    ref = restatement(specs, P, np.float64, hyper)
    q, ag, cg = ln_quantities(ref, batch)
    other = restatement(specs, P, dt, hyper, fault=fault)
    for net, cache in ((other.actor, ag["cache_actor"]), (other.critic, cg["cache_critic"])):
        net.amax_override = {name: cache[name + ":amax_own"] for name, _k, _c in O.CONV_DEFS}
        net.relu_override = {name: cache[name][1] > 0 for name, _k, _c in O.CONV_DEFS}
    q2, ag2, cg2 = ln_quantities(other, batch)
    return q, ag, cg, q2, ag2, cg2


def edge_bars(case):
    """{(network, quantity): (the float32 twin's error against float64, its bar)} of an edge case, and the float64 quantities"""
    q, _ag, _cg, q32, _a, _c = pinned_twin(case[0], case[1], case[4][0])
    bars = {}
    for net in ("actor", "critic"):
        for k in LN_QUANTITIES:
            e = rel_err(q32[net][k], q[net][k])
            bars[(net, k)] = (e, derived_bar(e))
    return bars, q


# ---- whole minibatches (tests/test_gpu_layer_norm.py) against the restatement composed with tests.ddpg_opt_np: 16x16x6 images, B = 8
def _R():
    from tests import ddpg_opt_np as R
    return R


WHOLE_SHAPE, WHOLE_B, WHOLE_ROWS = (16, 16, 3, 1, 2), 8, 24
# id: (actor's hidden layers, activation, minibatches, optimiser (tests.ddpg_opt_np.OPTIMISERS; None: GradientDescent), clip, the route)
WHOLE_CASES = collections.OrderedDict([
    ("default-sgd", ((65, 20, 10), "tanh", 1, None, 0.5, "heads+pre")),
    ("default-relu-sgd", ((65, 20, 10), "relu", 1, None, 0.5, "heads+pre")),
    ("two-hidden-sgd", ((65, 20), "tanh", 1, None, 0.5, "heads")),            # the heads launch without its leading actor layer
    ("one-hidden-sgd", ((65,), "tanh", 1, None, 0.5, "gemm")),                # the GEMM levels
    ("momentum-clipped", ((65, 20, 10), "tanh", 3, "momentum-0.5", 0.5, "heads+pre")),
    ("momentum-unclipped", ((65, 20, 10), "tanh", 3, "momentum-0.5", 1e4, "heads+pre")),
    ("adam-clipped", ((65, 20, 10), "tanh", 3, "adam", 0.5, "heads+pre")),
    ("adam-unclipped", ((65, 20, 10), "relu", 3, "adam", 1e4, "heads+pre"))])
WHOLE_TAU = 0.25


def whole_hyper(cid):
    _h, _act, _nb, opt, clip, _route = WHOLE_CASES[cid]
    if opt is None:
        return O.Hyper(1e-2, 5e-2, 0.9, clip, WHOLE_TAU)
    return _R().hyper_of(opt, clip, WHOLE_TAU)


def run_whole(specs, P, batches, hyper, opt, dt=np.float64, pin=None):
    """the minibatches and the target update on tests.ddpg_opt_np's restatement over normalised networks.  Returns (the six vectors,
    per-minibatch outputs).  pin: per minibatch (actor routes, critic routes) as {conv: codes} / {conv: active} pairs to evaluate on."""
    R = _R()
    name, args = R.OPTIMISERS[opt] if opt else ("GradientDescent", {})
    ref = with_feature_norm(R.DDPGWithOptimiser)(specs[0], specs[1], P[0], P[1], dt, hyper, name, args)
    ref.set_targets(P[2], P[3])
    outs = []
    for i, b in enumerate(batches):
        if pin is not None:
            (ref.actor.amax_override, ref.actor.relu_override), (ref.critic.amax_override, ref.critic.relu_override) = pin[i]
        outs.append(ref.train_minibatch(b))
    ref.update_targets()
    return R.vectors(ref), outs


def whole_case(cid):
    """host_case of a WHOLE_CASES id on the first seed on which conditions() hold in the first minibatch, every minibatch's two norms are
    1.2 x off the clip on the case's side, and the float32 twin takes the float64 evaluation's pool and ReLU routes in every minibatch"""
    hidden, act, nb, opt, clip, _route = WHOLE_CASES[cid]
    hp = whole_hyper(cid)
    for seed in SEEDS:
        case = host_case(WHOLE_SHAPE, WHOLE_B, nb, seed, hidden, act, rows=WHOLE_ROWS)
        q, _ag, _cg = ln_quantities(restatement(case[0], case[1], np.float64, hp), case[4][0])
        if conditions(q, act) is not None:
            continue
        want, outs = run_whole(case[0], case[1], case[4], hp, opt)
        norms = [n for o in outs for n in (o["actor_norm"], o["critic_norm"])]
        if not (min(norms) > 1.2 * clip if clip < 1 else max(norms) * 1.2 < clip):
            continue
        twin, outs32 = run_whole(case[0], case[1], case[4], hp, opt, np.float32)
        if all(np.array_equal(x, y) for a, b in zip(outs, outs32) for x, y in zip(a["routes"], b["routes"])):
            return case + (seed, want, outs, twin)
    raise AssertionError("no seed of %s meets the conditions for %s" % (list(SEEDS), cid))


# ---- twin Q heads: tests.twin_np.TwinDDPG on normalised networks (the critics' vectors in twin_np's order; twin_to_device for the device's)
TWIN_CASES = collections.OrderedDict([("twin-sgd", ("gradient-descent", 1, 0.5)), ("twin-adam", ("adam", 3, 0.5))])      # optimiser, minibatches, clip


def twin_hyper(cid):
    from tests import td3_np as T3
    opt, _nb, clip = TWIN_CASES[cid]
    return T3.hyper_of(opt, clip, WHOLE_TAU)


def run_twin(specs, P, batches, hyper, opt, dt=np.float64, pin=None):
    W = _twin()
    name, args = W.T3.OPTIMISERS[opt]
    ref = with_feature_norm(W.TwinDDPG)(specs[0], specs[1], P[0], P[1], dt, hyper, name, args)
    ref.set_targets(P[2], P[3])
    outs = []
    for i, b in enumerate(batches):
        if pin is not None:
            (ref.actor.amax_override, ref.actor.relu_override), (ref.critic.amax_override, ref.critic.relu_override) = pin[i]
        o = ref.train_minibatch(b)
        o.update(ag=ref.last_ag, cg=ref.last_cg)
        outs.append(o)
    ref.update_targets()
    return W.vectors(ref), outs, ref


def twin_case(cid):
    """whole_case for twin critics: host_case's numbers, the twin variables from tests.twin_np.twin_tail, head 2's last bias shifted so
    that each target head is the minimum on about half of the rows (as tests.twin_np.host_case does); the first seed on which the
    conditions hold, both norms are 1.2 x above the clip, each head is the minimum on a quarter of the rows of every minibatch and the
    float32 twin keeps the float64 routes"""
    W = _twin()
    opt, nb, clip = TWIN_CASES[cid]
    hp = twin_hyper(cid)
    for seed in SEEDS:
        specs, P, episodes, idxs, batches = host_case(WHOLE_SHAPE, WHOLE_B, nb, seed, (65, 20, 10), "tanh", rows=WHOLE_ROWS)
        on, tg = W.twin_tail(specs[1], np.random.default_rng(5000 + seed))
        P = [P[0], np.concatenate([P[1], on]), P[2], np.concatenate([P[3], tg])]
        ref = with_feature_norm(W.TwinDDPG)(specs[0], specs[1], P[0], P[1], np.float64)
        ref.set_targets(P[2], P[3])
        s2 = batches[0][4]
        w2 = ref._white(ref.target_actor, s2)
        tq = ref.target_critic.forward(s2, action=ref.target_actor.forward(s2, white=w2)["out"], white=w2)
        shift = np.float32(np.median(tq["out"] - tq["out2"]))
        P[1][-1] += shift
        P[3][-1] += shift
        want, outs, ref = run_twin(specs, P, batches, hp, opt)
        norms = [n for o in outs for n in (o["actor_norm"], o["critic_norm"])]
        if min(norms) <= 1.2 * clip or not all(W.MIN_SHARE <= x <= 1 - W.MIN_SHARE for x in ref.min_share):
            continue
        twin, outs32, _r = run_twin(specs, P, batches, hp, opt, np.float32)
        if all(np.array_equal(x, y) for a, b in zip(outs, outs32) for x, y in zip(a["routes"], b["routes"])):
            return specs, P, episodes, idxs, batches, seed, want, outs, twin
    raise AssertionError("no seed of %s meets the conditions for %s" % (list(SEEDS), cid))


# ---- the categorical and the quantile critic: tests.dist_np.DistDDPG / tests.quant_np.QuantDDPG on normalised networks (the GEMM levels)
DIST, QUANT = (11, -2.0, 12.0), (7, 1.0, 2)      # (atoms, v_min, v_max); (quantiles, kappa, dropped top atoms)
VALUE_CASES = collections.OrderedDict([("categorical-adam", ("dist", "adam", 3, 0.5)), ("quantile-momentum", ("quant", "momentum-0.5", 3, 0.5))])


def value_hyper(cid):
    from tests import td3_np as T3
    _kind, opt, _nb, clip = VALUE_CASES[cid]
    return T3.hyper_of(opt, clip, WHOLE_TAU)


def run_value(kind, specs, P, batches, hyper, opt, dt=np.float64):
    from tests import dist_np, quant_np, td3_np as T3
    name, args = T3.OPTIMISERS[opt]
    Base, par = (dist_np.DistDDPG, DIST) if kind == "dist" else (quant_np.QuantDDPG, QUANT)
    ref = with_feature_norm(Base)(specs[0], specs[1], P[0], P[1], par, dt, hyper, name, args)
    ref.set_targets(P[2], P[3])
    outs = []
    for b in batches:
        o = ref.train_minibatch(b)
        o.update(ag=ref.last_ag, cg=ref.last_cg)
        outs.append(o)
    ref.update_targets()
    return _R().vectors(ref), outs


def value_case(cid):
    """whole_case for a VALUE_CASES id: the first seed on which the conditions hold, both norms of every minibatch are 1.2 x above the
    clip and the float32 twin keeps the float64 routes"""
    kind, opt, nb, clip = VALUE_CASES[cid]
    hp = value_hyper(cid)
    for seed in SEEDS:
        case = host_case(WHOLE_SHAPE, WHOLE_B, nb, seed, (65, 20, 10), "tanh", rows=WHOLE_ROWS, critic_atoms=(DIST if kind == "dist" else QUANT)[0])
        want, outs = run_value(kind, case[0], case[1], case[4], hp, opt)
        q = {}
        for name, cache in (("actor", outs[0]["ag"]["cache_actor"]), ("critic", outs[0]["cg"]["cache_critic"])):
            q[name] = {"u": np.asarray(cache["ln"]["u"], np.float64), "sd": np.sqrt(np.asarray(cache["ln"]["var"], np.float64)).reshape(-1)}
        norms = [n for o in outs for n in (o["actor_norm"], o["critic_norm"])]
        if conditions(q, "tanh") is not None or min(norms) <= 1.2 * clip:
            continue
        twin, outs32 = run_value(kind, case[0], case[1], case[4], hp, opt, np.float32)
        if all(np.array_equal(x, y) for a, b in zip(outs, outs32) for x, y in zip(a["routes"], b["routes"])):
            return case + (seed, want, outs, twin)
    raise AssertionError("no seed of %s meets the conditions for %s" % (list(SEEDS), cid))


# ---- soft actor-critic: tests.sac_np.SacDDPG on normalised networks, one minibatch under gradient descent, the device's own noise
SAC_CLIP = 0.5


def sac_hyper():
    return O.Hyper(1e-2, 5e-2, 0.9, SAC_CLIP, WHOLE_TAU)


def sac_case(seed=1):
    """host_case with a Gaussian actor; the target actor is the actor (soft actor-critic has no other)"""
    specs, P, episodes, idxs, batches = host_case(WHOLE_SHAPE, WHOLE_B, 1, seed, (65, 20, 10), "tanh", rows=WHOLE_ROWS, gaussian=True)
    return specs, [P[0], P[1], P[0].copy(), P[3]], episodes, idxs, batches


def run_sac(specs, P, batch, eps1, eps2, dt=np.float64, routes=None):
    """one tests.sac_np.SacDDPG.train_minibatch (the temperature's defaults: 0.1, target entropy -A, rate 1e-4) and the critic's target
    update on normalised networks.  Returns (actor, critic, target critic vectors, the minibatch's outputs, the actor pass, the critic pass)"""
    from tests import sac_np as S
    ref = with_feature_norm(S.SacDDPG)(specs[0], specs[1], P[0], P[1], dt, sac_hyper())
    ref.target_critic = O.Net(specs[1], P[3], dt)
    if routes is not None:
        (ref.actor.amax_override, ref.actor.relu_override), (ref.critic.amax_override, ref.critic.relu_override) = routes
    ag, cg = ref.actor_gradients(batch[0], eps1), ref.critic_gradients(batch, eps2)
    out = ref.train_minibatch(batch, eps1, eps2)
    ref.update_targets()
    return [np.asarray(n.flat(), np.float64) for n in (ref.actor, ref.critic, ref.target_critic)], out, ag, cg
