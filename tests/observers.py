"""Observers between training calls ("Observers"): helpers of tests/test_gpu_observers.py and
tests/test_observers_host.py -- no tests in here.

A real run acts, evaluates, draws inspection batches, reads state back and saves checkpoints between two training calls.  All of that is
meant to observe.  The property held here is bit identity: the same training calls with and without the observers leave the same bytes.

  CLASSES        every cpp_* symbol of include/cartpolepp_abi.h in exactly one class, taken from the header's comment for the symbol
  CASES          the agents the property is held on, built with the option builders the variant test modules export
  CATALOGUE      observer operations at the Python level the product uses, each with a predicate over a case record and the
                 observer-class symbols it reaches
  snapshot       everything a later training call can read, as arrays
  after_call     what a training call left, read before any observer runs
  first_difference   the first (call, key) at which two traces differ, by bytes
  run            one run of an entry point: "A" (training calls only), "A'" (with the test's own reads), "B" (with observer blocks)

Nothing here imports the device library at import time: the host test reads the tables without a GPU."""
import collections
import ctypes as C
import os
import re

import numpy as np

from tests import td3_np as T3
from tests.test_gpu_twin_q import PER_KW

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "cartpolepp_abi.h")
HostBatch = collections.namedtuple("HostBatch", "state_1 action reward terminal_mask state_2")

TRAINING, OBSERVER, MUTATOR, CONFIGURATION, LIFECYCLE = "training", "observer", "mutator", "configuration", "lifecycle"


def declared_symbols(path=HEADER):
    """the cpp_* functions include/cartpolepp_abi.h declares, in order (comments stripped first: the prose names many of them)"""
    text = re.sub(r"/\*.*?\*/", " ", open(path).read(), flags=re.S)
    text = re.sub(r"//[^\n]*", " ", text)
    return re.findall(r"\b(cpp_[a-z0-9_]+)\s*\(", text)


# ---- the classification.  One line of the header's own words per symbol that is not obvious from its name.
_TABLE = {
    TRAINING: """
        cpp_net_soft_update cpp_ddpg_train_actor cpp_ddpg_train_critic cpp_ddpg_compute_gradients cpp_ddpg_apply_gradients
        cpp_ddpg_update_targets cpp_ddpg_train_step cpp_ddpg_train_rows cpp_ddpg_sample_and_compute cpp_ddpg_allreduce_grads
        cpp_ddpg_average_params cpp_ddpg_dp_train_step cpp_comm_allreduce cpp_naf_sample_and_compute cpp_naf_allreduce_grads
        cpp_naf_average_params cpp_naf_dp_train_step cpp_naf_train cpp_naf_compute_gradients cpp_naf_apply_gradients
        cpp_naf_update_targets cpp_naf_train_step cpp_naf_train_rows cpp_naf_train_rows_async
        cpp_naf_loss_wait
        cpp_replay_draw_prioritized
    """,
    # cpp_naf_loss_wait: "waits for THAT minibatch and returns its loss" -- the second half of cpp_naf_train_rows_async
    # cpp_replay_draw_prioritized: "the literal loop's draw ... the training sampler's counter, which then advances by one"
    OBSERVER: """
        cpp_abi_version cpp_last_error cpp_sync cpp_ctx_get_precision cpp_ctx_get_route cpp_timer_begin cpp_timer_end cpp_prof_reset
        cpp_prof_num_kernels cpp_prof_kernel_name cpp_prof_read
        cpp_net_is_twin_q cpp_net_distribution_info cpp_net_quantile_info cpp_net_pooled_quantile_info cpp_net_gaussian_info
        cpp_net_feature_norm_info cpp_net_encoder_info cpp_net_num_params cpp_net_num_vars cpp_net_var_info
        cpp_net_get_params cpp_net_get_grads cpp_net_forward cpp_net_forward_each cpp_net_forward_gaussian cpp_net_get_pool
        cpp_batch_upload cpp_batch_download cpp_batch_size cpp_batch_state_dtype
        cpp_replay_read_rows cpp_replay_read_states cpp_replay_sample cpp_replay_last_indexes cpp_replay_read_priorities
        cpp_replay_read_priority_tree cpp_replay_last_weights cpp_replay_get_n_step cpp_replay_get_random_shift cpp_replay_last_shifts
        cpp_ddpg_check_loss cpp_ddpg_q_gradients_wrt_actions cpp_ddpg_grad_buffer cpp_ddpg_last_target_noise
        cpp_ddpg_policy_delay_status cpp_ddpg_opt_state_size cpp_ddpg_get_opt_state cpp_ddpg_last_stats cpp_ddpg_last_values
        cpp_ddpg_last_twin_values cpp_ddpg_last_actor_min cpp_ddpg_last_behaviour_cloning cpp_ddpg_last_distribution
        cpp_ddpg_last_quantiles cpp_ddpg_last_pooled_quantiles cpp_ddpg_last_sac cpp_ddpg_sac_temperature cpp_ddpg_last_feature_norm
        cpp_ddpg_param_noise_status cpp_ddpg_param_noise_state cpp_ddpg_last_param_noise
        cpp_comm_info cpp_comm_max_double cpp_comm_max_doubles cpp_comm_barrier cpp_ddpg_dp_status cpp_naf_dp_status
        cpp_naf_action cpp_naf_debug_values cpp_naf_grad_buffer cpp_naf_last_stats cpp_naf_opt_state_size cpp_naf_get_opt_state
    """,
    # cpp_sync: the route's "k - 1 or k - 2" rule reads it; every run here synchronises after every call, so it decides alike
    # cpp_batch_upload / cpp_replay_sample: fill a minibatch of the CALLER's; a training call reads a cpp_batch only when it is handed
    #   that one, and the product's train ops fill theirs first.  cpp_replay_sample "does not move the counter" (random shift) and takes
    #   its key (seed, counter) as given
    # cpp_ddpg_sac_temperature / cpp_ddpg_param_noise_state: "set == 0: read into the pointers"; set != 0 is a checkpoint restore, which
    #   no observer here performs
    # cpp_ddpg_check_loss: "an evaluation: no noise, no count"; cpp_ddpg_q_gradients_wrt_actions: "count nothing"
    MUTATOR: """
        cpp_net_set_params cpp_replay_write_states cpp_replay_write_rows cpp_replay_set_size cpp_replay_fill_synthetic
        cpp_replay_update_priorities cpp_replay_gather_shifted cpp_ddpg_set_opt_state cpp_ddpg_param_noise_resample
        cpp_naf_set_opt_state cpp_naf_clear_numeric_error
    """,
    # cpp_replay_set_size: ReplayMemory.size(), the range the samplers draw from -- the last write of add_episode
    # cpp_replay_gather_shifted: "the counter advancing by one"; cpp_ddpg_param_noise_resample: perturb, measure, adapt, count
    # cpp_replay_write_rows / cpp_replay_fill_synthetic: "New rows ... take the running maximum priority"
    CONFIGURATION: """
        cpp_ctx_create cpp_ctx_set_precision cpp_ctx_set_route_threshold cpp_prof_enable
        cpp_net_create cpp_net_create_twin_q cpp_net_create_distributional cpp_net_create_quantile cpp_net_create_pooled_quantile
        cpp_net_create_pooled_quantile_norm cpp_net_create_gaussian cpp_net_create_feature_norm cpp_net_create_encoderless
        cpp_net_set_encoder cpp_batch_create cpp_replay_create cpp_replay_create_ex cpp_replay_set_stats_channels
        cpp_replay_enable_priorities cpp_replay_set_priority_beta cpp_replay_set_n_step cpp_replay_set_random_shift
        cpp_ddpg_create cpp_ddpg_set_optimiser cpp_ddpg_set_target_smoothing cpp_ddpg_set_policy_delay cpp_ddpg_set_actor_min_q
        cpp_ddpg_set_behaviour_cloning cpp_ddpg_set_quantile_target cpp_ddpg_set_sac cpp_ddpg_set_param_noise
        cpp_comm_unique_id cpp_comm_create cpp_naf_create
    """,
    LIFECYCLE: """
        cpp_ctx_destroy cpp_net_destroy cpp_batch_destroy cpp_replay_destroy cpp_ddpg_destroy cpp_comm_destroy cpp_naf_destroy
    """,
}
CLASS_LISTS = {cls: tuple(text.split()) for cls, text in _TABLE.items()}      # (a symbol named twice stays visible to the host test)
CLASSES = {sym: cls for cls, syms in CLASS_LISTS.items() for sym in syms}


# ---- cases
DEFAULT_SHAPE, LOWDIM, BIG_SHAPE = (16, 16, 3, 1, 2), (2, 2, 7), (64, 64, 3, 2, 3)
# 64x64x18: the smallest batch at which tests.helpers.conv_routes reports conv1's forward on the row-streaming f16 kernel
# ('conv1_fwd_f16') and the profile counts the operand-image rider's launch ('conv1_image'): B = 2 -- B = 1 runs on the f32-input
# kernels throughout (cartpolepp_abi.h) and the optimiser's launch carries no image (test_gpu_observers.py holds both facts)
BIG_B = 2
SMOOTHING = dict(target_policy_noise=0.2, target_policy_noise_clip=0.5, target_policy_noise_seed=3)

Case = collections.namedtuple("Case", "id kind shape B capacity kw entries")
_DDPG_ENTRIES = ("fused", "literal", "ops")


def _ddpg(cid, kw, shape=DEFAULT_SHAPE, B=8, capacity=8, entries=_DDPG_ENTRIES):
    return Case(cid, "ddpg", shape, B, capacity, kw, tuple(entries))


CASES = (
    _ddpg("plain", {}, entries=_DDPG_ENTRIES + ("literal-mid", "dp", "dp-overlap", "dp-sync2")),
    _ddpg("capacity16", {}, capacity=16),      # a capacity-size actions_given leaves data in every workspace row
    _ddpg("lowdim", {}, shape=LOWDIM),
    _ddpg("adam-td3", dict(T3.opt_kw("adam"), twin_q=True, actor_min_q=True, policy_delay=2, **SMOOTHING),
          entries=_DDPG_ENTRIES + ("dp", "dp-overlap", "dp-sync2")),
    _ddpg("momentum", dict(T3.opt_kw("momentum-0.5"))),
    _ddpg("categorical", dict(distributional_critic=True, num_atoms=11, v_min=-2.0, v_max=8.0)),
    _ddpg("quantile", dict(quantile_critic=True, num_quantiles=8, drop_top_quantiles=1)),
    _ddpg("pooled-sac", dict(pooled_quantile_critics=True, pooled_num_quantiles=5, pooled_drop_per_head=1, soft_actor_critic=True, sac_seed=7)),
    _ddpg("twin-sac", dict(twin_q=True, soft_actor_critic=True, sac_seed=7)),
    _ddpg("drqv2", dict(feature_layer_norm=True, shared_encoder=True, random_shift=4, random_shift_seed=5, n_step=3, replay_store="u8")),
    _ddpg("bc", dict(bc_alpha=2.5)),
    _ddpg("per-nstep", dict(PER_KW, n_step=3)),
    _ddpg("param-noise", dict(param_noise_stddev=0.05)),
    _ddpg("dropout", dict(use_dropout=True)),
    _ddpg("batch-norm", dict(use_batch_norm=True)),
    Case("naf-adam", "naf", DEFAULT_SHAPE, 8, 8, dict(optimiser="Adam", optimiser_args={"learning_rate": 0.01}), ("fused", "rows")),
    Case("naf-per", "naf", DEFAULT_SHAPE, 8, 8, dict(PER_KW), ("fused", "rows")),
    _ddpg("big-plain", {}, shape=BIG_SHAPE, B=BIG_B, capacity=4, entries=("fused", "literal")),
    _ddpg("big-shared", dict(shared_encoder=True), shape=BIG_SHAPE, B=BIG_B, capacity=4, entries=("fused", "literal")),
)
CASE = {c.id: c for c in CASES}
ROWS, REPLAY_SIZE = 40, 64


class Record(object):
    """what a predicate may ask of a (case, entry point) pair"""

    def __init__(self, case, entry):
        kw = case.kw
        self.case, self.entry, self.id = case, entry, "%s-%s" % (case.id, entry)
        self.ddpg, self.naf = case.kind == "ddpg", case.kind == "naf"
        self.pixel = len(case.shape) == 5
        self.B, self.capacity = case.B, case.capacity
        self.pooled = bool(kw.get("pooled_quantile_critics"))
        self.twin = bool(kw.get("twin_q")) or self.pooled
        self.gaussian = bool(kw.get("soft_actor_critic"))
        self.prioritized = bool(kw.get("prioritized_replay"))
        self.shift = bool(kw.get("random_shift"))
        self.n_step = int(kw.get("n_step", 1))
        self.param_noise = kw.get("param_noise_stddev") is not None
        self.slots = self.naf or "ddpg_optimiser" in kw
        self.smoothing = "target_policy_noise" in kw
        self.delay = int(kw.get("policy_delay", 1))
        self.categorical = bool(kw.get("distributional_critic"))
        self.quantile = bool(kw.get("quantile_critic"))
        self.feature_norm = bool(kw.get("feature_layer_norm"))
        self.shared = bool(kw.get("shared_encoder"))
        self.bc = "bc_alpha" in kw
        self.actor_min = bool(kw.get("actor_min_q"))
        self.dropout, self.batch_norm = bool(kw.get("use_dropout")), bool(kw.get("use_batch_norm"))
        self.comm = entry.startswith("dp")
        self.samples = entry != "ops"          # the entry point draws from the replay memory
        self.actor_conv = self.pixel and not self.shared


RECORDS = tuple(Record(c, e) for c in CASES for e in c.entries)
RECORD = {r.id: r for r in RECORDS}


# ---- building an agent of a case
def reset_route():
    """as test_the_route_is_a_function_of_the_calls_not_of_host_timing does: on the f16 pipes, nothing seen yet"""
    from cartpoleplusplus_amd import _lib
    ctx = _lib.default_context()
    ctx.sync()
    ctx.set_route_threshold(0.0)
    ctx.set_route_threshold(100.0)
    return ctx


class Env(object):
    """one run's agent and what the observers and the entry points need around it"""

    def __init__(self, rec, tmp_path=None):
        from cartpoleplusplus_amd import _lib
        self.rec, self.tmp_path, self.lib = rec, tmp_path, _lib
        # a context of the run's own: what cpp_ctx_get_route reports behind a call that published no scale is the last scale a decision
        # read -- on the process-wide context that may be one of an agent closed long ago, which a reset of the threshold does not forget
        self._outer_ctx = _lib._default_ctx
        self.ctx = _lib.Context(int(os.environ.get("LOCAL_RANK", "0")))
        _lib.set_default_context(self.ctx)
        self.agent = self.learner = self.comm = None
        try:
            reset_route()
            np.random.seed(1234)
            self.agent = make_agent(rec)
            self._prepare()
        except Exception:
            self.close()
            raise

    def _prepare(self):
        rec, agent = self.rec, self.agent
        rm = agent.replay_memory
        rm.fill_synthetic(ROWS, seed=24)
        if rec.param_noise:
            agent.begin_episode()          # a measured resample: cpp_ddpg_last_param_noise has something to read
        if rec.comm:
            from cartpoleplusplus_amd import ddpg_cartpole as D
            from cartpoleplusplus_amd.distributed import Communicator, NativeLearner
            self.comm = Communicator.single(agent.trainer.ctx)
            self.learner = NativeLearner(agent, rec.B, int(D.opts.sample_seed), self.comm, sync_every=2 if rec.entry == "dp-sync2" else 1,
                                         overlap=rec.entry == "dp-overlap")
        # states the inference observers feed: rows of the memory, and one constant frame (every pixel equal: a whitening scale far
        # above the route threshold)
        n = max(rec.capacity, rec.B)
        self.pool16 = rm.state[rm.state_1_idx[:n]].copy()
        self.const16 = np.full(rm.state_shape, 0.5, np.float16)
        rng = np.random.default_rng(99)
        self.actions = rng.uniform(-1, 1, (n, agent.replay_memory.action_dim)).astype(np.float32)
        self.host_batches = [self._host_batch(range(8 * i, 8 * i + rec.B), rng) for i in range(3)]

    def _host_batch(self, rows, rng):
        rm = self.agent.replay_memory
        rows = np.asarray(list(rows), np.int32)
        return HostBatch(rm.state[rm.state_1_idx[rows]], rm.action[rows].copy(), rng.uniform(0, 2, (len(rows), 1)).astype(np.float32),
                         rm.terminal_mask[rows].copy(), rm.state[rm.state_2_idx[rows]])

    def states(self, n, dtype=np.float16, const=True):
        """n inference states of the memory, the constant frame among them"""
        s = self.pool16[:n].copy()
        if const:
            s[n // 2] = self.const16
        return s.astype(dtype)

    def inspection_batch(self):
        """a host batch for the evaluation observers: the third host batch, the constant frame as one of its states"""
        hb = self.host_batches[2]
        s1 = hb.state_1.copy()
        s1[0] = self.const16
        return hb._replace(state_1=s1)

    @property
    def trainer(self):
        return self.agent.trainer

    def nets(self):
        nets = list(self.agent.networks())
        if getattr(self.agent, "perturbed_actor", None) is not None:
            nets.append(self.agent.perturbed_actor)
        return nets

    def close(self):
        try:
            if self.learner is not None:
                self.learner.close()
        finally:
            try:
                if self.agent is not None:
                    self.agent.close()
            finally:
                self.lib.set_default_context(self._outer_ctx)
                self.ctx.close()


def make_agent(rec):
    """the agent of a record: tests.helpers.make_pair's seeds and perturbations (the actor's head and the biases away from zero, the
    targets away from their sources) without its oracle, whose layout is the plain networks'"""
    case = rec.case
    if rec.naf:
        from tests.test_gpu_naf_prioritized_replay import make_naf
        kw = dict(case.kw)
        opt, args = kw.pop("optimiser", "Momentum"), kw.pop("optimiser_args", None)
        return make_naf(case.shape, case.capacity, True, optimiser=opt, optimiser_args=args, seed=3, replay_size=REPLAY_SIZE, **kw)[0]
    from cartpoleplusplus_amd import ddpg_cartpole as D
    from tests.helpers import FakeEnv, make_opts
    make_opts(D, case.shape, case.capacity, rec.pixel, replay_memory_size=REPLAY_SIZE, **case.kw)
    agent = D.DeepDeterministicPolicyGradientAgent(FakeEnv(case.shape, 2))
    try:
        agent.initialise_variables(seed=3)
        rng = np.random.default_rng(103)
        for nets, sd in (((agent.actor, agent.critic), 0.05), ((agent.target_actor, agent.target_critic), 0.01)):
            for net in nets:
                p = net.get_params()
                net.set_params(p + rng.normal(0, sd, p.shape).astype(np.float32))
            if sd == 0.05:
                agent.post_var_init_setup()
    except Exception:
        agent.close()
        raise
    return agent


# ---- the entry points: each a list of training calls
def training_calls(env):
    rec, agent, B = env.rec, env.agent, env.rec.B
    rm = agent.replay_memory
    lib, check, ptr = env.lib.lib, env.lib.check, env.lib.ptr
    if rec.entry == "fused":          # the eager pass, the capture, two replays
        return [lambda: agent.train_step(B, 2)] * 4
    if rec.entry.startswith("dp"):
        return [lambda: env.learner.train_step(2)] * 4
    if rec.naf and rec.entry == "rows":
        def rows_step():
            idxs = np.ascontiguousarray(rm.batch(B).idxs, dtype=np.int32)
            loss = C.c_float()
            check(lib.cpp_naf_train_rows(agent.naf.handle, rm.handle, B, ptr(idxs), C.byref(loss)))
            agent.target_value_net.update_weights()
        return [rows_step] * 4
    if rec.entry == "literal":          # ddpg_cartpole.py:331-337 at one minibatch per step
        def step():
            batch = rm.batch(B)
            agent.actor.train(batch.state_1)
            agent.critic.train(batch)
            agent.target_actor.update_weights()
            agent.target_critic.update_weights()
        return [step] * 4
    if rec.entry == "literal-mid":      # the same in two halves: an observed actor gets the unfused update first, run A asks for it by name
        held = {}

        def first():
            held["batch"] = rm.batch(B)
            agent.actor.train(held["batch"].state_1)
            agent.trainer.flush()

        def second():
            agent.critic.train(held.pop("batch"))
            agent.target_actor.update_weights()
            agent.target_critic.update_weights()
        return [first, second, first, second]
    assert rec.entry == "ops", rec.entry
    hbs = env.host_batches

    def actor_op(i):
        return lambda: agent.actor.train(hbs[i] if rec.bc else hbs[i].state_1)

    def critic_op(i):
        def op():
            agent.critic.train(hbs[i])
            agent.target_actor.update_weights()
            agent.target_critic.update_weights()
        return op
    return [actor_op(0), critic_op(0), actor_op(1), critic_op(1)]


# ---- what is compared
def _u64(x):
    return np.asarray(int(x), np.uint64)


def snapshot(env):
    """everything a later training call can read: {key: array}, counters first (first_difference names the first key that differs)"""
    rec, agent, lib, check, ptr = env.rec, env.agent, env.lib.lib, env.lib.check, env.lib.ptr
    rm = agent.replay_memory
    out = collections.OrderedDict()
    routed, scale = env.ctx.route()
    out["route"] = np.asarray([float(routed), scale], np.float32)
    n, disc = C.c_int(), C.c_float()
    check(lib.cpp_replay_get_n_step(rm.handle, C.byref(n), C.byref(disc)))
    out["n_step"] = np.asarray([n.value, disc.value], np.float32)
    if rec.shift:
        out["shift_counter"] = _u64(rm.shift_counter())
    if rec.ddpg:
        t = env.trainer
        d, cnt, held = t.policy_delay_status()
        out["policy_delay"] = np.asarray([d, cnt, int(held)], np.uint64)
        if rec.param_noise:
            sigma, dist, cnt, adapted = t.param_noise_status()
            out["param_noise.n"] = _u64(cnt)
            out["param_noise.sigma"] = np.asarray([sigma, dist, float(adapted)], np.float32)
            st = t.get_param_noise_state()
            out["param_noise.state"] = np.asarray([float(st["sigma"]), float(st["n"])], np.float64)
        if rec.gaussian:
            st = t.get_sac_state()
            out["sac.temperature"] = np.asarray([st["log_alpha"], st["m"], st["v"]], np.float32)
            out["sac.step"] = _u64(st["step"])
        if rec.slots:
            st = t.get_optimiser_state()
            out["optimiser.step"], out["optimiser.m"], out["optimiser.v"] = st["step"].copy(), st["m"], st["v"]
    else:
        st = agent.naf.get_optimiser_state()
        out["optimiser.step"], out["optimiser.m"], out["optimiser.v"] = _u64(st["step"]), st["m"], st["v"]
    if rec.prioritized:
        out["priority_tree"] = rm.priority_tree()
    for net in env.nets():
        out["params." + net.namespace] = net.get_params()
    return out


def after_call(env, k):
    """what training call k left on the device, read before any observer runs"""
    rec, agent, B, lib, check, ptr = env.rec, env.agent, env.rec.B, env.lib.lib, env.lib.check, env.lib.ptr
    rm = agent.replay_memory
    out = collections.OrderedDict()
    if rec.entry in ("ops", "literal-mid"):          # one half per call: what that half's pass wrote, nothing of the other's
        t = env.trainer
        st, (actions, dq_da, q, td) = t.last_stats(), t.last_values(B)
        if k % 2 == 0:
            out["last_stats.actor_norm"], out["last_values.actions"], out["last_values.dq_da"] = st[1:2].copy(), actions, dq_da
            out["grads.actor"] = agent.actor.get_grads()
        else:
            out["last_stats.critic"], out["last_values.q"], out["last_values.td"] = st[[0, 2]], q, td
            out["grads.critic"] = agent.critic.get_grads()
        return out
    if rec.samples:
        idxs = np.empty(B, np.int32)
        check(lib.cpp_replay_last_indexes(rm.handle, B, ptr(idxs)))
        out["last_indexes"] = idxs
        if rec.prioritized:
            out["last_weights"] = rm.last_weights(B)
        if rec.shift:
            out["last_shifts"] = rm.last_shifts(B)
    if rec.naf:
        out["last_stats"] = agent.naf.last_stats()
        for net in (agent.value_net, agent.naf.mu_net, agent.naf.l_net):
            out["grads." + net.namespace] = net.get_grads()
        return out
    t = env.trainer
    out["last_stats"] = t.last_stats()
    for name, v in zip(("actions", "dq_da", "q", "td"), t.last_values(B)):
        out["last_values." + name] = v
    if rec.twin:
        for name, v in zip(("q2", "target_q1", "target_q2", "td2"), t.last_twin_values(B)):
            out["last_twin." + name] = v
    if rec.smoothing:
        eps, n = t.last_target_noise(B)
        out["target_noise.n"], out["target_noise.eps"] = _u64(n), eps
    if rec.actor_min:
        for name, v in zip(("q1", "q2", "sel"), t.last_actor_min(B)):
            out["actor_min." + name] = v
    if rec.bc:
        lam, m, g, rows = t.last_behaviour_cloning(B)
        out["bc.lambda"], out["bc.g"], out["bc.rows"] = np.asarray([lam, m], np.float32), g, rows
    if rec.categorical:
        for name, v in zip(("p", "target_p", "m"), t.last_distribution(B)):
            out["distribution." + name] = v
    if rec.quantile:
        for name, v in zip(("theta", "sorted", "y"), t.last_quantiles(B)):
            out["quantiles." + name] = v
    if rec.pooled:
        for name, v in zip(("theta1", "theta2", "pool", "y"), t.last_pooled_quantiles(B)):
            out["pooled." + name] = v
    if rec.gaussian:
        for name, v in sorted(t.last_sac(B).items()):
            out["sac." + name] = np.asarray(v)
    if rec.feature_norm:
        for which, d in sorted(t.last_feature_norm(B).items()):
            for name, v in sorted(d.items()):
                out["feature_norm.%s.%s" % (which, name)] = v
    out["grads.actor"], out["grads.critic"] = agent.actor.get_grads(), agent.critic.get_grads()
    return out


def first_difference(a, b):
    """a, b: traces -- sequences of {key: array}, one per call (a single dict is a trace of one).  Compared by bytes: NaN equals NaN, -0
    differs from +0.  Returns (call, key, number of differing elements, max |difference|) of the first difference, or None.  A key that one
    side lacks, a shape or a type that changed count every element (the difference is then nan)."""
    if isinstance(a, dict):
        a, b = [a], [b]
    for call in range(max(len(a), len(b))):
        if call >= len(a) or call >= len(b):
            return (call, None, 0, float("nan"))
        da, db = a[call], b[call]
        for key in list(da) + [k for k in db if k not in da]:
            if key not in da or key not in db:
                present = np.asarray(da[key] if key in da else db[key])
                return (call, key, int(present.size), float("nan"))
            x, y = np.ascontiguousarray(da[key]), np.ascontiguousarray(db[key])
            if x.shape != y.shape or x.dtype != y.dtype:
                return (call, key, int(max(x.size, y.size)), float("nan"))
            if x.tobytes() == y.tobytes():
                continue
            width = x.dtype.itemsize
            diff = (np.frombuffer(x.tobytes(), np.uint8).reshape(-1, width) != np.frombuffer(y.tobytes(), np.uint8).reshape(-1, width)).any(axis=1)
            with np.errstate(all="ignore"):
                if x.dtype.kind in "fiub":
                    delta = np.abs(x.astype(np.float64).ravel() - y.astype(np.float64).ravel())[diff]
                    worst = float(np.nanmax(delta)) if np.isfinite(delta).any() else float("nan")
                else:
                    worst = float("nan")
            return (call, key, int(diff.sum()), worst)
    return None


# ---- the observer catalogue
Observer = collections.namedtuple("Observer", "name applies symbols run")
CATALOGUE = []


def observer(name, applies, symbols):
    def deco(fn):
        CATALOGUE.append(Observer(name, applies, tuple(symbols.split()), fn))
        return fn
    return deco


def _sizes(rec):
    return sorted({1, min(3, rec.capacity), rec.capacity})


@observer("action_given", lambda r: r.ddpg, "cpp_net_forward")
def _(env):
    actor = env.agent.actor
    actor.action_given(env.pool16[1])
    actor.action_given(env.const16)
    actor.action_given(env.pool16[2].astype(np.float32))


@observer("action_given+noise", lambda r: r.ddpg, "cpp_net_forward cpp_net_forward_gaussian")
def _(env):          # Ornstein-Uhlenbeck on the host; --soft-actor-critic: the policy's sample; --param-noise-stddev: the perturbed copy
    actor = env.agent.actor
    actor.action_given(env.const16, add_noise=True)
    actor.action_given(env.pool16[0], add_noise=True)


@observer("actions_given-f16", lambda r: r.ddpg, "cpp_net_forward_each cpp_net_forward_gaussian")
def _(env):
    for n in _sizes(env.rec):
        env.agent.actor.actions_given(env.states(n))
    env.agent.actor.actions_given(env.states(env.rec.capacity), add_noise=True)


@observer("actions_given-f32", lambda r: r.ddpg, "cpp_net_forward_each")
def _(env):
    for n in _sizes(env.rec):
        env.agent.actor.actions_given(env.states(n, np.float32))


@observer("forward_gaussian", lambda r: r.gaussian, "cpp_net_forward_gaussian")
def _(env):
    s = env.states(min(3, env.rec.capacity))
    env.agent.actor.forward_gaussian(s, each=False)
    env.agent.actor.forward_gaussian(s, each=True)
    env.agent.target_actor.forward_gaussian(s.astype(np.float32), each=True)


@observer("network-forwards", lambda r: r.ddpg, "cpp_net_forward")
def _(env):          # the four networks on whole batches (one whitening table per batch), the constant batch among them
    a, B = env.agent, env.rec.B
    s, act = env.states(B), env.actions[:B]
    flat = np.broadcast_to(env.const16, (B,) + env.const16.shape).copy()
    a.actor.forward(s)
    a.target_actor.forward(s.astype(np.float32))
    a.critic.forward(s, act)
    a.target_critic.forward(s, act)
    a.critic.forward(flat, act)
    a.actor.forward(flat)
    a.critic.forward(env.const16[None], act[:1])


@observer("check_loss-host", lambda r: r.ddpg, "cpp_ddpg_check_loss cpp_batch_upload cpp_batch_size")
def _(env):
    env.agent.critic.check_loss(env.inspection_batch())


@observer("check_loss-replay", lambda r: r.ddpg, "cpp_ddpg_check_loss cpp_replay_sample cpp_batch_size")
def _(env):
    rm, B = env.agent.replay_memory, env.rec.B
    batch = rm.batch(idxs=np.arange(3, 3 + B)) if env.rec.prioritized else rm.batch(B)
    env.agent.critic.check_loss(batch)


@observer("q_gradients_wrt_actions", lambda r: r.ddpg, "cpp_ddpg_q_gradients_wrt_actions cpp_batch_upload cpp_replay_sample")
def _(env):
    rm, B = env.agent.replay_memory, env.rec.B
    env.agent.critic.q_gradients_wrt_actions(env.states(B))
    env.agent.critic.q_gradients_wrt_actions(rm.batch(idxs=np.arange(5, 5 + B)))


@observer("replay.batch-read-on-the-host", lambda r: True, "cpp_replay_read_states")
def _(env):          # numpy's global generator draws the rows, as the reference's: the block puts its state back
    rm, B = env.agent.replay_memory, env.rec.B
    batch = rm.batch(idxs=np.arange(1, 1 + B)) if env.rec.prioritized else rm.batch(B)
    np.asarray(batch.state_1), np.asarray(batch.state_2)
    rm.state[[0, 1]]
    rm.current_stats()


@observer("replay.sample_on_device", lambda r: True, "cpp_replay_sample cpp_replay_last_indexes cpp_batch_download cpp_batch_state_dtype")
def _(env):
    rm, B = env.agent.replay_memory, env.rec.B
    batch = rm.sample_on_device(B, seed=5)
    np.asarray(batch.state_1)
    batch.device.state_dtype
    rm.sample_on_device(min(3, B), seed=0, counter=0)


@observer("replay.columns", lambda r: True, "cpp_replay_read_rows cpp_replay_get_n_step")
def _(env):
    rm, lib, check, ptr = env.agent.replay_memory, env.lib.lib, env.lib.check, env.lib.ptr
    rows = np.arange(4, dtype=np.int32)
    s1, s2, r = np.empty(4, np.int32), np.empty(4, np.int32), np.empty((4, 1), np.float32)
    check(lib.cpp_replay_read_rows(rm.handle, ptr(rows), 4, ptr(s1), ptr(s2), None, ptr(r), None))
    n, d = C.c_int(), C.c_float()
    check(lib.cpp_replay_get_n_step(rm.handle, C.byref(n), C.byref(d)))


@observer("replay.priorities", lambda r: r.prioritized, "cpp_replay_read_priorities cpp_replay_read_priority_tree cpp_replay_last_weights")
def _(env):
    rm = env.agent.replay_memory
    rm.priorities(np.arange(rm.size()))
    rm.priority_tree()
    rm.last_weights(env.rec.B)


@observer("replay.shifts", lambda r: r.shift, "cpp_replay_last_shifts cpp_replay_get_random_shift")
def _(env):
    rm = env.agent.replay_memory
    rm.last_shifts(env.rec.B)
    rm.shift_counter()


@observer("get_params+get_grads", lambda r: True, "cpp_net_get_params cpp_net_get_grads cpp_net_num_vars cpp_net_var_info")
def _(env):
    a = env.agent
    trained = (a.value_net, a.naf.mu_net, a.naf.l_net) if env.rec.naf else (a.actor, a.critic)
    for net in env.nets():
        net.get_params()
        net.trainable_model_vars()[0].eval()
        if net in trained:          # (a network without a train op has no gradient list and says so)
            net.get_grads()


@observer("pools", lambda r: r.pixel, "cpp_net_get_pool")
def _(env):          # Layer.eval and the debug codes; 21 / 22 are refused by a network that has no gradient workspace
    from tests.helpers import device_pool_codes
    lib, ptr, B = env.lib.lib, env.lib.ptr, env.rec.B
    for net in env.nets():
        if getattr(net, "pool1", None) is None:
            continue
        for p in (net.pool1, net.pool2, net.pool3):
            p.eval(B)
        device_pool_codes(net, B)
        for which, p in ((21, net.pool1), (22, net.pool2)):
            lib.cpp_net_get_pool(net.handle, which, B, ptr(np.empty([B] + p.shape[1:], np.float32)))


@observer("trainer.last", lambda r: r.ddpg, "cpp_ddpg_last_stats cpp_ddpg_last_values cpp_ddpg_policy_delay_status cpp_ddpg_grad_buffer")
def _(env):
    t, B = env.trainer, env.rec.B
    t.last_stats(), t.last_values(B), t.last_values(1), t.policy_delay_status(), t.grad_buffer()


@observer("trainer.last_twin_values", lambda r: r.twin, "cpp_ddpg_last_twin_values")
def _(env):
    env.trainer.last_twin_values(env.rec.B)


@observer("trainer.last_target_noise", lambda r: r.smoothing, "cpp_ddpg_last_target_noise")
def _(env):
    env.trainer.last_target_noise(env.rec.B)


@observer("trainer.last_actor_min", lambda r: r.actor_min, "cpp_ddpg_last_actor_min")
def _(env):
    env.trainer.last_actor_min(env.rec.B)


@observer("trainer.last_behaviour_cloning", lambda r: r.bc, "cpp_ddpg_last_behaviour_cloning")
def _(env):
    env.trainer.last_behaviour_cloning(env.rec.B)


@observer("trainer.last_distribution", lambda r: r.categorical, "cpp_ddpg_last_distribution")
def _(env):
    env.trainer.last_distribution(env.rec.B)


@observer("trainer.last_quantiles", lambda r: r.quantile, "cpp_ddpg_last_quantiles")
def _(env):
    env.trainer.last_quantiles(env.rec.B)


@observer("trainer.last_pooled_quantiles", lambda r: r.pooled, "cpp_ddpg_last_pooled_quantiles")
def _(env):
    env.trainer.last_pooled_quantiles(env.rec.B)


@observer("trainer.sac", lambda r: r.gaussian, "cpp_ddpg_last_sac cpp_ddpg_sac_temperature")
def _(env):
    env.trainer.last_sac(env.rec.B)
    env.trainer.get_sac_state()


@observer("trainer.last_feature_norm", lambda r: r.feature_norm, "cpp_ddpg_last_feature_norm")
def _(env):
    env.trainer.last_feature_norm(env.rec.B)


@observer("trainer.optimiser_state", lambda r: r.ddpg and r.slots, "cpp_ddpg_opt_state_size cpp_ddpg_get_opt_state")
def _(env):
    env.trainer.get_optimiser_state()


@observer("trainer.param_noise", lambda r: r.param_noise, "cpp_ddpg_param_noise_status cpp_ddpg_param_noise_state cpp_ddpg_last_param_noise")
def _(env):
    t = env.trainer
    t.param_noise_status(), t.get_param_noise_state(), t.last_param_noise(env.rec.B)


@observer("checkpoint", lambda r: True, "cpp_net_get_params cpp_net_var_info cpp_net_num_vars")
def _(env):          # force_save alone: SaverUtil's constructor restores or initialises, which is no observation
    from cartpoleplusplus_amd import util
    saver = util.SaverUtil.__new__(util.SaverUtil)
    saver.agent, saver.ckpt_dir, saver.save_freq = env.agent, str(env.tmp_path), 60
    saver.force_save()


@observer("context", lambda r: True, "cpp_sync cpp_ctx_get_route cpp_ctx_get_precision cpp_timer_begin cpp_timer_end cpp_prof_reset "
                                     "cpp_prof_num_kernels cpp_prof_kernel_name cpp_prof_read")
def _(env):
    ctx = env.ctx
    ctx.sync(), ctx.route(), ctx.precision
    ctx.timer_begin()
    ctx.timer_end()
    ctx.prof_reset()
    ctx.prof_read()
    env.lib.lib.cpp_prof_kernel_name(0)


@observer("abi-info", lambda r: True, "cpp_abi_version cpp_last_error cpp_net_is_twin_q cpp_net_distribution_info cpp_net_quantile_info "
                                      "cpp_net_pooled_quantile_info cpp_net_gaussian_info cpp_net_feature_norm_info cpp_net_encoder_info "
                                      "cpp_net_num_params")
def _(env):
    lib = env.lib.lib
    lib.cpp_abi_version(), lib.cpp_last_error()
    i, j, f, g = C.c_int(), C.c_int(), C.c_float(), C.c_float()
    for net in env.nets():
        h = net.handle
        lib.cpp_net_is_twin_q(h), lib.cpp_net_num_params(h)
        lib.cpp_net_distribution_info(h, C.byref(i), C.byref(f), C.byref(g))
        lib.cpp_net_quantile_info(h, C.byref(i))
        lib.cpp_net_pooled_quantile_info(h, C.byref(i))
        lib.cpp_net_gaussian_info(h, C.byref(i), C.byref(f), C.byref(g))
        lib.cpp_net_feature_norm_info(h, C.byref(i), C.byref(j), C.byref(f))
        lib.cpp_net_encoder_info(h, C.byref(i), C.byref(j))


@observer("communicator", lambda r: r.comm, "cpp_comm_info cpp_comm_max_double cpp_comm_max_doubles cpp_comm_barrier cpp_ddpg_dp_status")
def _(env):
    lib, check = env.lib.lib, env.lib.check
    rank, world, v = C.c_int(), C.c_int(), C.c_double(2.5)
    check(lib.cpp_comm_info(env.comm.handle, C.byref(rank), C.byref(world)))
    check(lib.cpp_comm_max_double(env.comm.handle, C.byref(v)))
    env.comm.max_over_ranks(1.0, 2.0)
    env.comm.barrier()
    env.learner.dp_status()


@observer("naf.action+debug_values", lambda r: r.naf, "cpp_naf_action cpp_naf_debug_values cpp_net_forward cpp_batch_upload cpp_replay_sample")
def _(env):
    agent, rm, B = env.agent, env.agent.replay_memory, env.rec.B
    agent.naf.action_given(env.const16, False)
    agent.naf.action_given(env.pool16[1], True)
    agent.naf.forward(env.states(B, np.float32))
    agent.value_net.value_given(env.states(B))
    agent.naf.debug_values(env.inspection_batch())
    agent.naf.debug_values(rm.batch(idxs=np.arange(2, 2 + B)))


@observer("naf.state", lambda r: r.naf, "cpp_naf_grad_buffer cpp_naf_last_stats cpp_naf_opt_state_size cpp_naf_get_opt_state cpp_naf_dp_status")
def _(env):
    naf, lib = env.agent.naf, env.lib.lib
    naf.get_grads(), naf.last_stats(), naf.get_optimiser_state()
    mode = C.c_int()
    env.lib.check(lib.cpp_naf_dp_status(naf.handle, C.byref(mode), None, 0))


BY_NAME = {o.name: o for o in CATALOGUE}


def applicable(rec):
    return [o for o in CATALOGUE if o.applies(rec)]


def subset(rec, seed):
    """a seeded random subset of the applicable observers in random order (at least one)"""
    rng = np.random.default_rng(seed)
    obs = applicable(rec)
    keep = [o for o in obs if rng.random() < 0.5] or obs[:1]
    return [keep[i] for i in rng.permutation(len(keep))]


def observer_block(env, observers):
    """the observers in the order given; numpy's global generator is left as it was found (the literal loop draws its rows from it)"""
    state = np.random.get_state()
    try:
        for o in observers:
            o.run(env)
    finally:
        np.random.set_state(state)


# ---- the runs
def _merge(*dicts):
    out = collections.OrderedDict()
    for d in dicts:
        out.update(d)
    return out


def run(rec, mode, tmp_path=None, observers=(), slip=None):
    """one run of rec's entry point from the same seed, parameters and memory.  mode "A": the training calls, a synchronisation after each,
    state read once at the end.  "A'": after_call and snapshot behind every call as well.  "B": that, an observer block between every two
    calls, and a second snapshot behind each block.  slip = (k, fn): fn(env) runs at the end of the block behind call k (the positive
    controls).  Returns (trace, end): trace[k] = what stood behind call k ("B": trace[k] = (behind the call, behind its block)), end =
    after_call + snapshot when all calls are done."""
    env = Env(rec, tmp_path)
    try:
        calls = training_calls(env)
        trace = []
        for k, call in enumerate(calls):
            call()
            env.ctx.sync()
            if mode == "A":
                continue
            behind_call = _merge(snapshot(env), after_call(env, k))
            if mode == "B" and k + 1 < len(calls):
                observer_block(env, observers)
                if slip is not None and slip[0] == k:
                    slip[1](env)
                trace.append((behind_call, snapshot(env)))
            elif mode == "B":
                trace.append((behind_call, None))
            else:
                trace.append(behind_call)
        env.ctx.sync()
        end = _merge(snapshot(env), after_call(env, len(calls) - 1))
        return trace, end
    finally:
        env.close()


def compare_with_observers(trace_b, trace_ref):
    """run B's trace against run A''s: behind every call everything must be equal, behind every observer block the snapshot must still
    be the one A' took behind the call.  Returns (first_difference, where) with where "call" or "observers", or None."""
    for k, (behind_call, behind_block) in enumerate(trace_b):
        d = first_difference(behind_call, trace_ref[k])
        if d is not None:
            return (k,) + d[1:], "call"
        if behind_block is not None:
            ref = collections.OrderedDict((key, trace_ref[k][key]) for key in behind_block)
            d = first_difference(behind_block, ref)
            if d is not None:
                return (k,) + d[1:], "observers"
    return None
