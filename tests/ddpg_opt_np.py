"""Momentum and Adam for the DDPG learner, restated on the float64 oracle (include/cartpolepp_abi.h: cpp_ddpg_set_optimiser): a subclass
of oracle.ddpg_np.DDPG whose train calls apply oracle.naf_np.make_optimiser's rule -- the one oracle.naf_np.NAF.apply states -- to each
gradient list on its own: the actor's and the critic's optimisers are separate (the reference's two 'optimiser' scopes), each with its
own slots and its own step count t, and a call that trains one list advances that list's t only.  The learning rates stay the two
lists' own (Hyper.actor_lr / critic_lr).  Also the cases the CPU and the GPU tests share, and the faults the CPU test plants.
Test-only: product code never imports it."""
import numpy as np

from oracle import ddpg_np as O
from oracle import naf_np as N

LISTS = ("actor", "critic")
# planted faults (tests/test_ddpg_optimiser_host.py): one t for both lists; no bias correction; epsilon inside the square root; the clip
# applied to the update after the moments instead of to the gradient before them
FAULTS = ("shared_t", "no_bias_correction", "eps_in_sqrt", "clip_after_moments")


class Slots(object):
    def __init__(self, n, dt):
        self.m, self.v, self.t = np.zeros(n, dt), np.zeros(n, dt), 0


def apply_rule(opt, flat, grads, clip, slots, dt, fault=None):
    """oracle.naf_np.NAF.apply for one list: clip by the list's global norm, then the optimiser's rule on its slots.  Returns (new
    flat vector, pre-clip norm)."""
    g, norm = O.clip_by_global_norm(grads, clip, dt)
    if fault == "clip_after_moments":
        scale = dt(1.0) if clip is None or norm == 0 else dt(clip) * min(dt(1.0) / norm, dt(1.0) / dt(clip))
        g = np.asarray(grads, dt)
    slots.t += 1
    if opt.kind == "sgd":
        step = dt(opt.learning_rate) * g
    elif opt.kind == "momentum":
        slots.m = (dt(opt.momentum) * slots.m + g).astype(dt)
        step = dt(opt.learning_rate) * slots.m
    else:
        lr_t = opt.learning_rate * np.sqrt(1.0 - opt.beta2 ** slots.t) / (1.0 - opt.beta1 ** slots.t)
        if fault == "no_bias_correction":
            lr_t = opt.learning_rate
        slots.m = (dt(opt.beta1) * slots.m + dt(1.0 - opt.beta1) * g).astype(dt)
        slots.v = (dt(opt.beta2) * slots.v + dt(1.0 - opt.beta2) * g * g).astype(dt)
        if fault == "eps_in_sqrt":
            step = dt(lr_t) * slots.m / np.sqrt(slots.v + dt(opt.epsilon))
        else:
            step = dt(lr_t) * slots.m / (np.sqrt(slots.v) + dt(opt.epsilon))
    if fault == "clip_after_moments":
        step = step * scale
    return (np.asarray(flat, dt) - step).astype(dt), norm


class DDPGWithOptimiser(O.DDPG):
    def __init__(self, actor_spec, critic_spec, actor_flat, critic_flat, dt=np.float64, hyper=O.DEFAULT_HYPER,
                 optimiser="GradientDescent", optimiser_args=None, fault=None):
        super(DDPGWithOptimiser, self).__init__(actor_spec, critic_spec, actor_flat, critic_flat, dt, hyper=hyper)
        args = dict(optimiser_args or {})
        assert "learning_rate" not in args
        self.opt = {"actor": N.make_optimiser(optimiser, dict(args, learning_rate=hyper.actor_lr)),
                    "critic": N.make_optimiser(optimiser, dict(args, learning_rate=hyper.critic_lr))}
        self.slots = {"actor": Slots(len(actor_flat), dt), "critic": Slots(len(critic_flat), dt)}
        self.fault, self.calls = fault, 0

    def _call(self):
        """planted fault 'shared_t': ONE count, advanced by every train call whichever list it serves, read by both lists"""
        self.calls += 1
        if self.fault == "shared_t":
            for w in LISTS:
                self.slots[w].t = self.calls - 1      # (apply_rule counts the apply it serves)

    def _apply(self, which, grads):
        net = getattr(self, which)
        new, norm = apply_rule(self.opt[which], net.flat(), grads, self.hp.gradient_clip, self.slots[which], self.dt, self.fault)
        setattr(self, which, O.Net(net.spec, new, self.dt))
        return norm

    def train_actor(self, s1):                 # actor.train(batch.state_1), ddpg_cartpole.py:332-333
        self._call()
        ag = self.actor_gradients(s1)
        return {"actor_norm": float(self._apply("actor", ag["grads"]))}

    def train_critic(self, batch):             # critic.train(batch), ddpg_cartpole.py:334
        self._call()
        cg = self.critic_gradients(batch)
        return {"critic_norm": float(self._apply("critic", cg["grads"])), "td": cg["td"], "loss": float(cg["loss"])}

    def train_minibatch(self, batch):
        """DDPG.train_minibatch with the two rules: both gradient sets from the same snapshot, then both applies.  Also returns the
        trunk's routes as tests.helpers.oracle_minibatch does."""
        self._call()
        ag, cg = self.actor_gradients(batch[0]), self.critic_gradients(batch)
        routes = []
        for cache in (ag["cache_actor"], cg["cache_critic"]):
            for name, _k, _co in O.CONV_DEFS if self.actor.spec.pixel else ():
                routes.append(np.where(cache[name][1] > 0, cache[name + ":amax_own"], 255).astype(np.uint8))
        a_norm = self._apply("actor", ag["grads"])
        c_norm = self._apply("critic", cg["grads"])
        return {"actor_norm": float(a_norm), "critic_norm": float(c_norm), "routes": routes, "td": cg["td"], "loss": float(cg["loss"]),
                "actor_grads": ag["grads"], "critic_grads": cg["grads"]}

    def state(self):
        """what the device trainer's get_optimiser_state() holds: m and v over [actor | critic], step = (actor's t, critic's t)"""
        return {"m": np.concatenate([np.asarray(self.slots[w].m, np.float64) for w in LISTS]),
                "v": np.concatenate([np.asarray(self.slots[w].v, np.float64) for w in LISTS]),
                "step": np.array([self.slots[w].t for w in LISTS], np.uint64)}


def restatement(specs, P, dt, hyper, optimiser, optimiser_args, fault=None):
    ref = DDPGWithOptimiser(specs[0], specs[1], P[0], P[1], dt, hyper, optimiser, optimiser_args, fault)
    ref.set_targets(P[2], P[3])
    return ref


def vectors(ref):
    """the six compared vectors: the four parameter vectors, then m and v"""
    st = ref.state()
    return [np.asarray(n.flat(), np.float64) for n in (ref.actor, ref.critic, ref.target_actor, ref.target_critic)] + [st["m"], st["v"]]


VECTORS = ("actor", "critic", "target_actor", "target_critic", "m", "v")

# ---- the cases.  Momentum 0.5; Adam with betas and epsilon away from TensorFlow's defaults, as tests.helpers.NAF_OPTIMISERS'
# "adam-third-step": with epsilon 1e-3 an element whose |g| is at the float32 noise of the gradient moves by lr g / epsilon, a quantity
# float32 decides, instead of by +-lr (tests/test_ddpg_optimiser_host.py checks that per case with the float32 twin).  Three minibatches
# in one call: t = 3 in the bias correction, and at 64x64x18 minibatches 2 and 3 read conv1 through the operand image the rider built.
SMALL, CFG3 = (16, 16, 3, 1, 2), (64, 64, 3, 2, 3)
NB = 3
OPTIMISERS = {"momentum-0.5": ("Momentum", {"momentum": 0.5}),
              "momentum-0.0": ("Momentum", {"momentum": 0.0}),
              "adam": ("Adam", {"beta1": 0.8, "beta2": 0.9, "epsilon": 1e-3})}
# learning rates: Momentum at tests.helpers.LOUD's; Adam's update is ~lr per element whatever the gradient's size, so its rates are
# smaller (and differ between the lists: swapped rates show)
RATES = {"momentum-0.5": (1e-2, 5e-2), "momentum-0.0": (1e-2, 5e-2), "adam": (2e-3, 5e-3)}
SHAPES = {"16x16x6": (SMALL, 16, 3), "64x64x18": (CFG3, 8, 3)}          # shape, B, host_case seed (64x64x18: of seeds 1 .. 6 the one on which the
                                                                          # float32 twin keeps the float64 routes in all four of its cases)


def hyper_of(opt_name, clip, tau):
    la, lc = RATES[opt_name]
    if opt_name.startswith("momentum") and clip > 1:      # (unclipped, norms of 20 .. 160 at LOUD's rates leave the minibatches' range)
        la, lc = la / 10, lc / 10
    return O.Hyper(la, lc, 0.9, clip, tau)


def grid():
    """(id, optimiser name, shape name, clip, target update rate): both shapes take every combination"""
    out = []
    for opt in ("momentum-0.5", "adam"):
        for clip in (0.5, 1e4):          # below every norm of these minibatches / above every one (asserted by the tests)
            for tau in (0.25, 1.0):
                out.append(("%s-16x16x6-clip%g-tau%g" % (opt, clip, tau), opt, "16x16x6", clip, tau))
        for clip in (0.5, 1e4):
            for tau in (0.25, 1.0):
                out.append(("%s-64x64x18-clip%g-tau%g" % (opt, clip, tau), opt, "64x64x18", clip, tau))
    return out


# tolerances of the GPU test, per vector: a float32 update may sit 2^-23 * nb * |theta| + r * |delta| from the float64 one
# (tests.helpers.delta_bound, tests/test_gpu_hyperparameters.py) with r at that module's floor, 5e-5 -- never widened by what a run gives.
# The slots start at zero (theta = 0, delta = the slot) and are held to the same r.  Besides, parameters and targets at rel 2e-5 of the vector (tests/test_gpu_naf.py).
R = {"actor": 5e-5, "critic": 5e-5, "target_actor": 5e-5, "target_critic": 5e-5, "m": 5e-5, "v": 5e-5}
PARAM_REL = 2e-5


def bounds(P, want, nb=NB):
    from tests.helpers import delta_bound
    start = list(P) + [np.zeros_like(want[4]), np.zeros_like(want[5])]
    return [delta_bound(p, w - p, R[name], nb) for name, p, w in zip(VECTORS, start, want)]


def run_case(specs, P, batches, hyper, opt_name, dt=np.float64, fault=None, actor_first=None):
    """NB minibatches and the target update; returns (the six vectors, step counts, per-minibatch outputs).  actor_first: a state
    batch for one actor.train call of its own in front (the step counts then differ between the lists)."""
    name, args = OPTIMISERS[opt_name]
    ref = restatement(specs, P, dt, hyper, name, args, fault)
    if actor_first is not None:
        ref.train_actor(actor_first)
    outs = [ref.train_minibatch(b) for b in batches]
    ref.update_targets()
    return vectors(ref), ref.state()["step"], outs
