"""Delayed policy updates (TD3: Fujimoto et al. 2018, Algorithm 1; include/cartpolepp_abi.h, cpp_ddpg_set_policy_delay) restated on the
float64 oracle: a subclass of tests.ddpg_opt_np.DDPGWithOptimiser that keeps the delay d and the count n of applied critic updates and
applies the actor's list iff n' % d == 0.  A held list keeps its parameters, its slots and its own step count; its gradient is still
computed and its norm reported.  The target updates keep the outer step's cadence, whatever the last minibatch did.  With `smoothing`
the critic's gradients are tests.tps_np.SmoothedDDPG's (the two TD3 ingredients this learner has, composed).  Also the cases the CPU
and the GPU tests share, and the faults the CPU test plants.  Test-only: product code never imports it."""
import numpy as np

from oracle import ddpg_np as O
from tests import ddpg_opt_np as R
from tests import tps_np as T

# planted faults (tests/test_policy_delay_host.py)
FAULTS = ("actor_every_minibatch",            # the delay ignored
          "phase_off_by_one",                 # applies when n' % d == 1
          "adam_count_on_hold",               # the actor's step count advancing on held minibatches
          "slots_on_hold",                    # the actor's Momentum slot (Adam: both moments) accumulating on held minibatches
          "critic_held_too",                  # the hold reaching the critic's list
          "target_actor_skips_when_held",     # no target-actor update behind an outer step whose last minibatch was held
          "train_actor_advances_n")           # the stand-alone actor op counting the minibatch (the critic op counts it again)


class DelayedDDPG(R.DDPGWithOptimiser):
    def __init__(self, actor_spec, critic_spec, actor_flat, critic_flat, dt=np.float64, hyper=O.DEFAULT_HYPER,
                 optimiser="GradientDescent", optimiser_args=None, delay=1, smoothing=None, fault=None):
        assert fault is None or fault in FAULTS, fault
        super(DelayedDDPG, self).__init__(actor_spec, critic_spec, actor_flat, critic_flat, dt, hyper, optimiser, optimiser_args, None)
        assert 1 <= int(delay) <= 65536
        self.d, self.n, self.held = int(delay), 0, False
        self.pd_fault = fault
        self.smoothing, self.tps_n = smoothing, 0      # (sigma, clip, seed) or None; the count of target-forming passes
        self.schedule = []                             # per counted minibatch: was the actor's list applied
        # --use-dropout (include/cartpolepp_abi.h, cpp_net_spec.use_dropout): training-mode forwards so far of the actor and of the target
        # actor.  The hold reaches the optimiser alone -- a held minibatch still runs both forwards, draws masks and is counted
        self.drop_n = {"actor": 0, "target_actor": 0}

    # ---- the rule
    def _applies(self, n_new):
        if self.pd_fault == "actor_every_minibatch":
            return True
        if self.pd_fault == "phase_off_by_one":
            return n_new % self.d == 1 % self.d
        return n_new % self.d == 0

    def _actor(self, grads, applied):
        """the actor's list behind its gradient pass: applied, or held (norm only)"""
        if applied:
            return self._apply("actor", grads)
        _g, norm = O.clip_by_global_norm(grads, self.hp.gradient_clip, self.dt)
        sl, opt = self.slots["actor"], self.opt["actor"]
        if self.pd_fault == "adam_count_on_hold":
            sl.t += 1
        if self.pd_fault == "slots_on_hold":
            if opt.kind == "momentum":
                sl.m = (self.dt(opt.momentum) * sl.m + _g).astype(self.dt)
            elif opt.kind != "sgd":
                sl.m = (self.dt(opt.beta1) * sl.m + self.dt(1.0 - opt.beta1) * _g).astype(self.dt)
                sl.v = (self.dt(opt.beta2) * sl.v + self.dt(1.0 - opt.beta2) * _g * _g).astype(self.dt)
        return norm

    def critic_gradients(self, batch, *a, **kw):
        if self.smoothing is None or a or kw:
            return super(DelayedDDPG, self).critic_gradients(batch, *a, **kw)
        sigma, clip, seed = self.smoothing
        act = np.asarray(batch[1])
        noise = T.target_noise(seed, self.tps_n, act.shape[0], act.shape[1], sigma, clip, np.float64)
        self.tps_n += 1
        return T.SmoothedDDPG.critic_gradients(self, batch, noise)

    def _draw_masks(self, B, *which):
        """the masks of the next training-mode forward of the named networks; their counts advance (nothing to do without dropout)"""
        if not self.actor.spec.dropout:
            return
        from tests.helpers import dropout_masks
        for name in which:
            getattr(self, name).drop_masks = dropout_masks(name, self.actor.spec.hidden, B, self.drop_n[name])
            self.drop_n[name] += 1

    # ---- the entry points
    def train_minibatch(self, batch):
        self._draw_masks(np.asarray(batch[1]).shape[0], "actor", "target_actor")
        ag, cg = self.actor_gradients(batch[0]), self.critic_gradients(batch)
        routes, tie = [], np.inf
        for cache in (ag["cache_actor"], cg["cache_critic"]):
            for name, _k, _co in O.CONV_DEFS if self.actor.spec.pixel else ():
                pooled = cache[name][1]
                routes.append(np.where(pooled > 0, cache[name + ":amax_own"], 255).astype(np.uint8))
                live = pooled > 0
                if live.any():      # the closest call among the pooling windows that carry gradient, relative as tests.helpers measures it
                    tie = min(tie, float((cache[name + ":margin"] / np.maximum(1.0, np.abs(pooled)))[live].min()))
                tie = min(tie, float(np.abs(cache[name + ":zmax"]).min()))      # ... and among the ReLU decisions on the pooled outputs
        self.n += 1
        applied = self._applies(self.n)
        self.held = not applied
        self.schedule.append(applied)
        a_norm = self._actor(ag["grads"], applied)
        if self.pd_fault == "critic_held_too" and not applied:
            _g, c_norm = O.clip_by_global_norm(cg["grads"], self.hp.gradient_clip, self.dt)
        else:
            c_norm = self._apply("critic", cg["grads"])
        return {"actor_norm": float(a_norm), "critic_norm": float(c_norm), "routes": routes, "td": cg["td"], "loss": float(cg["loss"]),
                "applied": applied, "target_dq_da": cg.get("target_dq_da"), "tie": tie}

    def train_actor(self, s1):
        """the actor half of the minibatch whose critic half follows: looks one ahead, counts nothing"""
        if self.pd_fault == "train_actor_advances_n":
            self.n += 1
            applied = self._applies(self.n)
        else:
            applied = self._applies(self.n + 1)
        self.held = not applied
        self._draw_masks(np.asarray(s1).shape[0], "actor")
        ag = self.actor_gradients(s1)
        return {"actor_norm": float(self._actor(ag["grads"], applied)), "applied": applied}

    def train_critic(self, batch):
        self.n += 1
        applied = self._applies(self.n)
        self.held = not applied
        self.schedule.append(applied)
        self._draw_masks(np.asarray(batch[1]).shape[0], "target_actor")
        cg = self.critic_gradients(batch)
        if self.pd_fault == "critic_held_too" and not applied:
            return {"critic_norm": float(O.clip_by_global_norm(cg["grads"], self.hp.gradient_clip, self.dt)[1]), "td": cg["td"]}
        return {"critic_norm": float(self._apply("critic", cg["grads"])), "td": cg["td"], "loss": float(cg["loss"])}

    def update_targets(self):
        if self.pd_fault == "target_actor_skips_when_held" and self.held:
            keep = self.target_actor
            super(DelayedDDPG, self).update_targets()
            self.target_actor = keep
            return
        super(DelayedDDPG, self).update_targets()


def expected_schedule(d, n_minibatches):
    """which of the minibatches 1 .. n apply the actor's list"""
    return [k % d == 0 for k in range(1, n_minibatches + 1)]


def restatement(specs, P, dt, hyper, opt_name, delay, smoothing=None, fault=None):
    name, args = OPTIMISERS[opt_name]
    ref = DelayedDDPG(specs[0], specs[1], P[0], P[1], dt, hyper, name, args, delay, smoothing, fault)
    ref.set_targets(P[2], P[3])
    return ref


# ---- the cases.  Shapes, batch sizes, seeds, rates and optimiser arguments are tests/ddpg_opt_np.py's; GradientDescent joins at the
# Momentum rates (tests.helpers.LOUD's).
OPTIMISERS = dict(R.OPTIMISERS, **{"gradient-descent": ("GradientDescent", {})})
SHAPES = R.SHAPES
VECTORS = R.VECTORS


def hyper_of(opt_name, clip, tau):
    """tests.ddpg_opt_np.hyper_of's rates, except: unclipped, GradientDescent and Momentum run at a hundredth of LOUD's rates, not a tenth --
    that module's unclipped cases are three minibatches long; over the six of a case here the critic at 64x64x18 leaves the range at a
    tenth (its pre-clip norms go 160, 5.5e3, 1.8e4, 1.9e6, 2.7e13), at a hundredth they stay between 13 and 160"""
    hp = R.hyper_of("momentum-0.5" if opt_name == "gradient-descent" else opt_name, clip, tau)
    if opt_name != "adam" and clip > 1:
        hp = hp._replace(actor_lr=hp.actor_lr / 10, critic_lr=hp.critic_lr / 10)
    return hp


def opt_kw(opt_name):
    """the agent's options for an optimiser of OPTIMISERS"""
    import json
    name, args = OPTIMISERS[opt_name]
    return {} if name == "GradientDescent" else dict(ddpg_optimiser=name, ddpg_optimiser_args=json.dumps(args))


def grid():
    """(id, optimiser, shape, delay, minibatches per outer step, outer steps, clip, tau) of the cases held to the float64 restatement with
    the caller's rows.  Every (optimiser, shape) pair meets both delays, the clip below and above every norm and both target rates.
    d = 2 over 3 minibatches ends its outer step on a held one, d = 3 over 3 on an applied one (TD3's own schedule); 2 x 3 minibatches
    under d = 2 apply at positions 2 | 1, 3 of the two outer steps, 2 x 2 under d = 3 at position 1 of the second alone.  64x64x18, where
    minibatches 2 .. read conv1 through the operand image the optimiser's launch built -- behind a held minibatch and behind an applied
    one --, takes the two arrangements that cover all of that in four minibatches at the most (the float32 twin leaves the float64 routes
    in the fifth minibatch of the 2 x 3 arrangement there: tests/test_policy_delay_host.py)."""
    combos = {"16x16x6": ((2, 3, 1, 0.5, 0.25), (3, 3, 1, 1e4, 1.0), (2, 3, 2, 1e4, 0.25), (3, 2, 2, 0.5, 1.0)),
              "64x64x18": ((2, 3, 1, 0.5, 0.25), (3, 2, 2, 1e4, 1.0))}
    out = []
    for opt in ("gradient-descent", "momentum-0.5", "adam"):
        for shape in ("16x16x6", "64x64x18"):
            for d, nb, steps, clip, tau in combos[shape]:
                out.append(("%s-%s-d%d-%dx%d-clip%g-tau%g" % (opt, shape, d, steps, nb, clip, tau), opt, shape, d, nb, steps, clip, tau))
    return out


# A case is only good if float32 can decide every route it takes: a pooling window whose two largest pre-activations lie within a few
# float32 ulps of each other (or a pooled output that close to zero) is routed one way by numpy's float32 twin and the other way by a
# kernel that adds the same products in another order -- both are right, and the two updates then differ by a whole gradient element.
# 2^-21 is eight ulps of a value near 1: sums of a few hundred float32 products in two orders differ by less.  The float64 run of every
# case must stay above it in every minibatch (tests/test_policy_delay_host.py); a case that does not is replaced, not loosened.
TIE_FLOOR = 2.0 ** -21

# which of host_case's minibatches an arrangement starts at: 64x64x18's 2 x 2 arrangement starts at the second -- from the first, the
# GradientDescent critic reaches a conv2 pooling window 4.9e-8 from a tie in its third minibatch (below TIE_FLOOR; from the second, the
# closest call of the three optimisers is 8.3e-7)
FIRST_MINIBATCH = {("64x64x18", 3, 2, 2): 1}


def case_batches(case, idxs, batches, B):
    """the row numbers and minibatches of a grid() case"""
    _cid, _opt, shape_name, d, nb, steps, _clip, _tau = case
    k = FIRST_MINIBATCH.get((shape_name, d, nb, steps), 0)
    assert k + steps * nb <= MAX_MINIBATCHES
    return idxs[k * B:(k + steps * nb) * B], batches[k:k + steps * nb]


MAX_MINIBATCHES = 6          # per case with the caller's rows: 2 x 3

# ---- graph replay: the device draws the rows (device_rows: sample seed 0, the sampler's counter = the minibatch's number), the first
# outer step is the eager pass and the capture, the others replay.  (id, optimiser, shape, delay, minibatches per step, outer steps,
# sample seed); clip 0.5, target rate 0.25.  (Sample seed 2 for the Momentum case: on the rows of seed 0 it comes within 1.3e-7 of a
# tie, below TIE_FLOOR; on seed 2's its closest call is 8.3e-7.)  The first is "one graph, a schedule that does not divide it": 5 minibatches under d = 2 apply at
# positions 2, 4 of the odd outer steps and 1, 3, 5 of the even ones.
GRAPH_ROWS, GRAPH_CLIP, GRAPH_TAU = 24, 0.5, 0.25
GRAPH_CASES = (("adam-16x16x6-d2-4x5", "adam", "16x16x6", 2, 5, 4, 0),
               ("gradient-descent-16x16x6-d3-3x2", "gradient-descent", "16x16x6", 3, 2, 3, 0),
               ("momentum-0.5-64x64x18-d2-2x2", "momentum-0.5", "64x64x18", 2, 2, 2, 2),
               ("adam-64x64x18-d3-2x2", "adam", "64x64x18", 3, 2, 2, 0))


def graph_case(cid):
    """host_case's parameters and episodes of the shape, with the rows the device will draw and the minibatches they select"""
    from tests.helpers import host_case
    _cid, opt, shape_name, d, nb, steps, sample_seed = [c for c in GRAPH_CASES if c[0] == cid][0]
    shape, B, seed = SHAPES[shape_name]
    specs, P, episodes, _idxs, _b = host_case(shape, B, 1, seed, rows=GRAPH_ROWS)
    rows = np.concatenate([device_rows(sample_seed, k, B, GRAPH_ROWS) for k in range(steps * nb)])
    return specs, P, episodes, rows, batches_of(shape, episodes, GRAPH_ROWS, rows, B)


def bounds(P, want, nb):
    return R.bounds(P, want, nb)


def run_case(specs, P, batches, hyper, opt_name, delay, nb, steps, dt=np.float64, fault=None, smoothing=None, targets=True):
    """`steps` outer steps of `nb` minibatches each over batches[0 : steps * nb], the target update behind each; returns (the six
    vectors, step counts, per-minibatch outputs, the restatement)"""
    ref = restatement(specs, P, dt, hyper, opt_name, delay, smoothing, fault)
    outs = []
    for s in range(steps):
        for b in batches[s * nb:(s + 1) * nb]:
            outs.append(ref.train_minibatch(b))
        if targets:
            ref.update_targets()
    return R.vectors(ref), ref.state()["step"], outs, ref


def run_literal(specs, P, batches, hyper, opt_name, delay, dt=np.float64, fault=None):
    """the reference's loop unpaired (ddpg_cartpole.py:332-337 with host arrays): actor.train, critic.train, both target updates, one
    minibatch per outer step -- the actor's gradient is taken BEFORE the critic's update here, as in the fused minibatch, and the
    critic's never reads the live actor, so the two orders agree"""
    ref = restatement(specs, P, dt, hyper, opt_name, delay, None, fault)
    for b in batches:
        ref.train_actor(b[0])
        ref.train_critic(b)
        ref.update_targets()
    return R.vectors(ref), ref.state()["step"], ref


def device_rows(seed, counter, B, size):
    """the rows the device's sampler draws for the minibatch keyed by `counter` (include/cartpolepp_abi.h: Philox4x32-10 over
    {i, 0, counter_lo, counter_hi}, row = (word0 * size) >> 32)"""
    from tests.helpers import philox4x32_10_np
    i = np.arange(B, dtype=np.uint64)
    x, _y, _z, _w = philox4x32_10_np(i, np.zeros_like(i), np.full_like(i, counter & 0xFFFFFFFF), np.full_like(i, counter >> 32),
                                     seed & 0xFFFFFFFF, seed >> 32)
    return ((x * np.uint64(size)) >> np.uint64(32)).astype(np.int32)


def batches_of(shape, episodes, rows, idxs, B, action_dim=2):
    """the minibatches the row numbers select from host_case's episodes"""
    from oracle.replay_np import OracleReplayMemory
    orm = OracleReplayMemory(rows, shape, action_dim)
    for ep in episodes:
        orm.add_episode(*ep)
    out = []
    for k in range(len(idxs) // B):
        ob = orm.batch(idxs=np.asarray(idxs[k * B:(k + 1) * B]))
        out.append((ob.state_1, ob.action, ob.reward, ob.terminal_mask, ob.state_2))
    return out
