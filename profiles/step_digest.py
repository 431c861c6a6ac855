#!/usr/bin/env python
"""What the training entry points compute and launch, as digests: the check that a change of the host code (rt_*.cpp) left both alone.
For every configuration below a learner is built from fixed seeds at the smallest shapes the routes allow (64x64x6 pixel states or the
low-dimensional state, B = 8, a memory of 64 rows: rendered episodes / random states), then
    digests   three outer steps of four minibatches; after each the sha256 of every network's parameters, the optimiser's slots and counts,
              the priority tree, the temperature words and the policy-delay words where there are any, the augmentation counter, last_stats
    launches  one more outer step under the library's profiling mode (the eager launch sequence): launches per kernel family
(The sampler's counter has no accessor: the rows of the second and third outer step are drawn at it, so their digests carry it --
in the configurations the device samples; on the caller's rows nothing moves or reads it, and nothing here checks it.)
Run it on a build of the parent commit -- twice: a configuration whose digests differ between the two is not deterministic and proves
nothing -- and on the head, then merge:
    step_digest.py > parent_a.json; step_digest.py > parent_b.json; step_digest.py > head.json        (each in its own tree)
    CARTPOLEPP_ABLATION=1 CPP_FUSED_HEADS=0 step_digest.py > ..._abl.json                             (the GEMM levels of the DDPG step)
    step_digest.py --merge parent_a.json parent_b.json head.json [the three _abl files] > step_digest.json
While the ABI stands, one tree does: the parent's two libraries copied into cartpoleplusplus_amd/lib/ under build names, the runs
    CARTPOLEPP_ABLATION=<release name> step_digest.py;  CARTPOLEPP_ABLATION=<ablation name> CPP_FUSED_HEADS=0 step_digest.py
(CPP_FUSED_HEADS=0 selects the ablation list; the library is whichever CARTPOLEPP_ABLATION names).
Equality is the bar.  The single_* configurations drive the four single entry points (train_actor, train_critic, check_loss,
q_gradients_wrt_actions) on host batches, one round of the four per outer step; their digests also cover what check_loss and
q_gradients_wrt_actions return and both networks' gradient buffers after every call.  Their launch counts are recorded and not compared
(LAUNCHES_RECORDED_ONLY): a build that batches the GEMMs of a level launches fewer.  The infer_* configurations drive the host-batch
inference entry points (cpp_net_forward, cpp_net_forward_each, cpp_net_forward_gaussian, cpp_net_get_pool, cpp_naf_action) on fresh states,
one round per outer step, and digest the bytes they return; no training step runs in them.  The merged file is a record of one comparison, not a fixture: the digests move with every intended kernel change.
Usage: step_digest.py [config name ...] | --merge parent_a parent_b head [parent_a_abl parent_b_abl head_abl]"""
import ctypes as C
import hashlib, json, os, sys
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

PIXEL, LOWDIM, B, NB, ROWS, OUTER = (64, 64, 3, 1, 2), (2, 2, 7), 8, 4, 64, 3
ABLATION = os.environ.get("CPP_FUSED_HEADS") == "0"      # (on CARTPOLEPP_ABLATION=1, or =<name> of an ablation build of another commit)
MOMENTUM = dict(optimiser="Momentum", optimiser_args='{"learning_rate": 0.001, "momentum": 0.9}')
ADAM = dict(optimiser="Adam", optimiser_args='{"learning_rate": 0.001}')
# the trainers of the single entry points' configurations (single_<trainer>, single_<trainer>_lowdim)
SINGLE_TRAINERS = {
    "plain": {},
    "twin": dict(twin_q=True),
    "categorical": dict(distributional_critic=True, num_atoms=51, v_min=-5.0, v_max=25.0),
    "quantile": dict(quantile_critic=True, num_quantiles=25, drop_top_quantiles=2),
    "sac": dict(soft_actor_critic=True),
    "smoothing_adam_delay2": dict(target_policy_noise=0.2, ddpg_optimiser="Adam", policy_delay=2),
    "twin_min": dict(twin_q=True, actor_min_q=True),
    "bc": dict(bc_alpha=2.5),
    "feature_norm": dict(feature_layer_norm=True),
    "sac_twin_min": dict(soft_actor_critic=True, twin_q=True, actor_min_q=True),
}
# (--feature-layer-norm is refused without --use-raw-pixels: a low-dimensional network has no conv features to normalise)
PIXEL_ONLY = ("feature_norm",)
LAUNCHES_RECORDED_ONLY = set("single_%s%s" % (t, sfx) for t in SINGLE_TRAINERS for sfx in ("", "_lowdim") if not (sfx and t in PIXEL_ONLY))


def merge(paths):
    runs = [json.load(open(p)) for p in paths]
    for k in range(3, len(runs)):
        runs[k - 3].update(runs[k])
    out = {}
    for name in runs[0]:
        pa, pb, head = (r.get(name) for r in runs[:3])
        ran = all(r and r.get("digests") and r.get("launches") and "error" not in r for r in (pa, pb, head))      # (a refused or broken run verifies nothing)
        out[name] = {"parent": pa, "head": head, "ran": ran, "parent_deterministic": ran and pa == pb,
                     "digests_equal": ran and pa["digests"] == head["digests"], "launches_equal": ran and pa["launches"] == head["launches"],
                     "launches_compared": name not in LAUNCHES_RECORDED_ONLY}
    json.dump(out, sys.stdout, indent=1, sort_keys=True)
    bad = [n for n, v in out.items() if not v["ran"] or (v["parent_deterministic"] and not (
        v["digests_equal"] and (v["launches_equal"] or not v["launches_compared"])))]
    sys.stderr.write("%d configurations, %d not deterministic on the parent, %d differ: %s\n" % (
        len(out), sum(not v["parent_deterministic"] for v in out.values()), len(bad), bad))
    sys.exit(1 if bad else 0)


if len(sys.argv) > 1 and sys.argv[1] == "--merge":
    merge(sys.argv[2:])

from cartpoleplusplus_amd import _lib, ddpg_cartpole as D, naf_cartpole as N
from oracle import ddpg_np as O
from tests.helpers import FakeEnv, fill_with_rendered_episodes
lib, check, ptr = _lib.lib, _lib.check, _lib.ptr


def sha(arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


def fill(agent, shape, opts, u8):
    if len(shape) == 5:
        return fill_with_rendered_episodes(agent, shape, ROWS, seed=3, as_u8=u8, opts=opts)
    rng, left = np.random.default_rng(5), ROWS
    while left > 0:
        n = min(left, int(rng.integers(2, 7)))
        mk = lambda: rng.standard_normal(shape).astype(np.float32)
        agent.replay_memory.add_episode(mk(), [(rng.uniform(-1, 1, (1, 2)).astype(np.float32), float(rng.integers(0, 3)), mk()) for _ in range(n)])
        left -= n


def shape_opts(shape):
    if len(shape) == 5:
        return dict(use_raw_pixels=True, render_height=shape[0], render_width=shape[1], num_cameras=shape[3], action_repeats=shape[4])
    return dict(use_raw_pixels=False, action_repeats=shape[0])


def perturb(nets, rng, sd):      # (away from the near-zero heads and zero biases: every path carries signal)
    for net in nets:
        p = net.get_params()
        net.set_params(p + rng.normal(0, sd, p.shape).astype(np.float32))


def ddpg_agent(shape, shift=0, **kw):
    o = D.default_opts(batch_size=B, replay_memory_size=ROWS, sample_seed=7, **dict(shape_opts(shape), **kw))
    D.set_opts(o)
    a = D.DeepDeterministicPolicyGradientAgent(FakeEnv(shape))
    a.initialise_variables(seed=1)
    rng = np.random.default_rng(101)
    perturb((a.actor, a.critic), rng, 0.05)
    a.post_var_init_setup()
    perturb((a.target_actor, a.target_critic), rng, 0.01)
    fill(a, shape, o, kw.get("replay_store") == "u8")
    if shift:
        a.replay_memory.enable_random_shift(shift, seed=11)
    return a


def naf_agent(shape, **kw):
    o = N.default_opts(batch_size=B, replay_memory_size=ROWS, sample_seed=7, **dict(shape_opts(shape), **kw))
    N.set_opts(o)
    a = N.NormalizedAdvantageFunctionAgent(FakeEnv(shape))
    a.initialise_variables(seed=1)
    rng = np.random.default_rng(102)
    perturb((a.value_net, a.naf.mu_net, a.naf.l_net), rng, 0.05)
    a.post_var_init_setup()
    perturb((a.target_value_net,), rng, 0.01)
    fill(a, shape, o, False)
    return a


def ddpg_state(a):
    t, rm = a.trainer, a.replay_memory
    out = [n.get_params() for n in a.networks()]
    if t.has_optimiser_slots():
        st = t.get_optimiser_state()
        out += [np.asarray(st[k]) for k in sorted(st)]
    if getattr(rm, "prioritized", False):
        out.append(rm.priority_tree())
    if getattr(rm, "random_shift", (0, 0))[0]:
        out.append(np.array([rm.shift_counter()], np.uint64))
    if a.actor.sac:
        st = t.get_sac_state()
        out += [np.asarray(st[k]) for k in sorted(st)]
    out.append(np.array(t.policy_delay_status(), np.int64).reshape(-1))
    out.append(t.last_stats())
    return out


class HostBatch(object):
    def __init__(self, t):
        self.state_1, self.action, self.reward, self.terminal_mask, self.state_2 = t


def single_ops(a, k):      # one round of the four single entry points on host batch k; what they return and leave rides in a.single
    grads = lambda: [a.actor.get_grads(), a.critic.get_grads()]
    shape = a.env.observation_space.shape
    hb = HostBatch(O.synthetic_batch(np.random.default_rng(700 + k), B, shape, 2, len(shape) == 5))
    a.single = []
    a.actor.train(hb if a.trainer.behaviour_cloning[0] > 0.0 else hb.state_1)      # (--bc-alpha clones the batch's actions: the whole batch)
    a.single += grads()
    a.critic.train(hb)
    a.single += grads()
    loss, td, q = a.critic.check_loss(hb)
    a.single += [np.float32(loss), td, q] + grads()
    a.single += [a.critic.q_gradients_wrt_actions(hb)] + grads()


def single_state(a):
    return ddpg_state(a) + a.single


def infer_states(a, k):      # float32 states of round k: pixel values in [0, 1), standard normal low-dimensional ones
    shape, rng = a.env.observation_space.shape, np.random.default_rng(800 + k)
    return (rng.random((B,) + tuple(shape)) if len(shape) == 5 else rng.standard_normal((B,) + tuple(shape))).astype(np.float32)


def pools_of(net, shape):      # pool1..3 of the network's last forward
    out = []
    for i in (1, 2, 3):
        p = np.empty((B, shape[0] >> i, shape[1] >> i, 10), np.float32)
        check(lib.cpp_net_get_pool(net.handle, i, B, ptr(p)))
        out.append(p)
    return out


def infer_ddpg(a, k):      # one round of the inference entry points; what they return rides in a.infer
    s, shape = infer_states(a, k), a.env.observation_space.shape
    owner = a.critic if a.actor.shared_encoder else a.actor      # (the network whose trunk sees the actor's states)
    pools = (lambda n: pools_of(n, shape)) if len(shape) == 5 else (lambda n: [])
    a.infer = [a.actor.forward(s[:1]), a.actor.forward(s)] + pools(owner)
    a.infer += [a.actor.actions_given(s), a.actor.actions_given(s.astype(np.float16))] + pools(owner)
    act = np.random.default_rng(850 + k).uniform(-1, 1, (B, a.actor.action_dim)).astype(np.float32)
    a.infer += [a.critic.forward(s, act)] + pools(a.critic)
    if a.actor.sac:
        for each in (False, True):
            a.infer += list(a.actor.forward_gaussian(s, each=each)) + pools(owner)


def infer_naf(a, k):
    s = infer_states(a, k)
    a.infer = [a.naf.forward(s[:1]), a.naf.forward(s)]


def infer_state(a):
    return a.infer


def naf_state(a):
    st = a.naf.get_optimiser_state()
    out = [n.get_params() for n in a.networks()] + [np.asarray(st[k]) for k in sorted(st)]
    if getattr(a.replay_memory, "prioritized", False):
        out.append(a.replay_memory.priority_tree())
    out.append(a.naf.last_stats())
    return out


def rows_of(step):      # the caller's rows of outer step `step`: NB x B
    return np.random.default_rng(900 + step).integers(0, ROWS, NB * B).astype(np.int32)


# ---- one outer step through each entry point
def ddpg_step(a, k): a.train_step(B, NB)
def ddpg_step_idxs(a, k): a.train_step(B, NB, idxs=rows_of(k))
def ddpg_rows(a, k):
    for r in rows_of(k).reshape(NB, B):
        check(lib.cpp_ddpg_train_rows(a.trainer.handle, a.replay_memory.handle, B, ptr(np.ascontiguousarray(r))))
    check(lib.cpp_ddpg_update_targets(a.trainer.handle))
def ddpg_dp(sync_every, overlap):
    return lambda a, k: check(lib.cpp_ddpg_dp_train_step(a.trainer.handle, a.replay_memory.handle, None, B, NB, 7, sync_every, overlap))
def naf_step(a, k): a.train_step(B, NB)
def naf_step_idxs(a, k): a.train_step(B, NB, idxs=rows_of(k))
def naf_rows(a, k):
    loss = C.c_float()
    for r in rows_of(k).reshape(NB, B):
        check(lib.cpp_naf_train_rows(a.naf.handle, a.replay_memory.handle, B, ptr(np.ascontiguousarray(r)), C.byref(loss)))
    check(lib.cpp_naf_update_targets(a.naf.handle))
def naf_rows_async(a, k):
    ticket, loss = C.c_uint64(), C.c_float()
    for r in rows_of(k).reshape(NB, B):
        check(lib.cpp_naf_train_rows_async(a.naf.handle, a.replay_memory.handle, B, ptr(np.ascontiguousarray(r)), C.byref(ticket)))
        check(lib.cpp_naf_loss_wait(a.naf.handle, ticket.value, C.byref(loss)))
    check(lib.cpp_naf_update_targets(a.naf.handle))
def naf_dp(a, k): check(lib.cpp_naf_dp_train_step(a.naf.handle, a.replay_memory.handle, None, B, NB, 7, 1))


DDPG, NAF, SINGLE = (ddpg_agent, ddpg_state), (naf_agent, naf_state), (ddpg_agent, single_state)
INFER_DDPG, INFER_NAF = (ddpg_agent, infer_state), (naf_agent, infer_state)
DRQV2 = dict(twin_q=True, actor_min_q=True, feature_layer_norm=True, n_step=3, target_policy_noise=0.2, shift=4)
# name: (learner, shape, options, one outer step)
CONFIGS = {
    "ddpg_sgd": (DDPG, PIXEL, {}, ddpg_step),
    "ddpg_sgd_lowdim": (DDPG, LOWDIM, {}, ddpg_step),
    "ddpg_adam_clip": (DDPG, PIXEL, dict(ddpg_optimiser="Adam", gradient_clip=0.05), ddpg_step),
    "ddpg_twin_delay2_smoothing": (DDPG, PIXEL, dict(twin_q=True, policy_delay=2, target_policy_noise=0.2), ddpg_step),
    "ddpg_categorical": (DDPG, PIXEL, dict(distributional_critic=True, num_atoms=21, v_min=-5.0, v_max=25.0), ddpg_step),
    "ddpg_quantile": (DDPG, PIXEL, dict(quantile_critic=True, num_quantiles=9, drop_top_quantiles=2), ddpg_step),
    "ddpg_sac": (DDPG, PIXEL, dict(soft_actor_critic=True), ddpg_step),
    "ddpg_sac_lowdim": (DDPG, LOWDIM, dict(soft_actor_critic=True), ddpg_step),
    "ddpg_batch_norm": (DDPG, PIXEL, dict(use_batch_norm=True), ddpg_step),
    "ddpg_u8_store": (DDPG, PIXEL, dict(replay_store="u8"), ddpg_step),
    "ddpg_prioritized": (DDPG, PIXEL, dict(prioritized_replay=True), ddpg_step),
    "ddpg_prioritized_momentum_lowdim": (DDPG, LOWDIM, dict(prioritized_replay=True, ddpg_optimiser="Momentum", ddpg_optimiser_args='{"momentum": 0.9}'), ddpg_step),
    "ddpg_3_step": (DDPG, PIXEL, dict(n_step=3), ddpg_step),
    "ddpg_random_shift": (DDPG, PIXEL, dict(shift=4), ddpg_step),
    "ddpg_step_idxs": (DDPG, PIXEL, {}, ddpg_step_idxs),
    "ddpg_step_idxs_prioritized": (DDPG, PIXEL, dict(prioritized_replay=True), ddpg_step_idxs),
    "ddpg_rows": (DDPG, PIXEL, {}, ddpg_rows),
    "ddpg_rows_prioritized": (DDPG, PIXEL, dict(prioritized_replay=True), ddpg_rows),
    "ddpg_dp": (DDPG, PIXEL, {}, ddpg_dp(1, 0)),
    "ddpg_dp_sync_every_2": (DDPG, PIXEL, {}, ddpg_dp(2, 0)),
    "ddpg_dp_overlap": (DDPG, PIXEL, {}, ddpg_dp(1, 1)),
    "ddpg_feature_norm": (DDPG, PIXEL, dict(feature_layer_norm=True), ddpg_step),
    "ddpg_categorical_feature_norm": (DDPG, PIXEL, dict(feature_layer_norm=True, distributional_critic=True, num_atoms=21, v_min=-5.0, v_max=25.0), ddpg_step),
    "ddpg_twin_min": (DDPG, PIXEL, dict(twin_q=True, actor_min_q=True), ddpg_step),
    "ddpg_twin_min_adam_delay2_smoothing": (DDPG, PIXEL, dict(twin_q=True, actor_min_q=True, ddpg_optimiser="Adam", policy_delay=2, target_policy_noise=0.2), ddpg_step),
    "ddpg_bc": (DDPG, PIXEL, dict(bc_alpha=2.5), ddpg_step),
    "ddpg_twin_min_bc_lowdim": (DDPG, LOWDIM, dict(twin_q=True, actor_min_q=True, bc_alpha=2.5), ddpg_step),
    "ddpg_sac_twin_min": (DDPG, PIXEL, dict(soft_actor_critic=True, twin_q=True, actor_min_q=True), ddpg_step),
    "ddpg_dropout": (DDPG, PIXEL, dict(use_dropout=True), ddpg_step),
    "ddpg_drqv2": (DDPG, PIXEL, DRQV2, ddpg_step),
    "ddpg_shared_encoder": (DDPG, PIXEL, dict(shared_encoder=True), ddpg_step),
    "ddpg_shared_encoder_sac": (DDPG, PIXEL, dict(shared_encoder=True, soft_actor_critic=True), ddpg_step),
    "ddpg_shared_encoder_drqv2": (DDPG, PIXEL, dict(DRQV2, shared_encoder=True), ddpg_step),
    "naf_shared": (NAF, PIXEL, dict(share_input_state_representation=True), naf_step),
    "naf_unshared": (NAF, PIXEL, {}, naf_step),
    "naf_lowdim": (NAF, LOWDIM, {}, naf_step),
    "naf_shared_momentum": (NAF, PIXEL, dict(share_input_state_representation=True, **MOMENTUM), naf_step),
    "naf_shared_adam": (NAF, PIXEL, dict(share_input_state_representation=True, **ADAM), naf_step),
    "naf_prioritized": (NAF, PIXEL, dict(share_input_state_representation=True, prioritized_replay=True), naf_step),
    "naf_batch_norm": (NAF, PIXEL, dict(share_input_state_representation=True, use_batch_norm=True), naf_step),
    "naf_step_idxs": (NAF, PIXEL, dict(share_input_state_representation=True), naf_step_idxs),
    "naf_step_idxs_prioritized": (NAF, PIXEL, dict(share_input_state_representation=True, prioritized_replay=True), naf_step_idxs),
    "naf_rows": (NAF, PIXEL, dict(share_input_state_representation=True), naf_rows),
    "naf_rows_prioritized": (NAF, PIXEL, dict(share_input_state_representation=True, prioritized_replay=True), naf_rows),
    "naf_rows_async": (NAF, PIXEL, dict(share_input_state_representation=True, **MOMENTUM), naf_rows_async),
    "naf_dp": (NAF, PIXEL, dict(share_input_state_representation=True), naf_dp),
    "infer_ddpg": (INFER_DDPG, PIXEL, {}, infer_ddpg),
    "infer_ddpg_lowdim": (INFER_DDPG, LOWDIM, {}, infer_ddpg),
    "infer_ddpg_batch_norm": (INFER_DDPG, PIXEL, dict(use_batch_norm=True), infer_ddpg),
    "infer_ddpg_categorical": (INFER_DDPG, PIXEL, dict(distributional_critic=True, num_atoms=21, v_min=-5.0, v_max=25.0), infer_ddpg),
    "infer_ddpg_quantile": (INFER_DDPG, PIXEL, dict(quantile_critic=True, num_quantiles=9, drop_top_quantiles=2), infer_ddpg),
    "infer_ddpg_twin": (INFER_DDPG, PIXEL, dict(twin_q=True), infer_ddpg),
    "infer_ddpg_feature_norm": (INFER_DDPG, PIXEL, dict(feature_layer_norm=True), infer_ddpg),
    "infer_ddpg_sac": (INFER_DDPG, PIXEL, dict(soft_actor_critic=True), infer_ddpg),
    "infer_ddpg_shared_encoder": (INFER_DDPG, PIXEL, dict(shared_encoder=True), infer_ddpg),
    "infer_naf_shared": (INFER_NAF, PIXEL, dict(share_input_state_representation=True), infer_naf),
    "infer_naf_unshared": (INFER_NAF, PIXEL, {}, infer_naf),
    "infer_naf_lowdim": (INFER_NAF, LOWDIM, {}, infer_naf),
}
for _t, _kw in SINGLE_TRAINERS.items():
    CONFIGS["single_" + _t] = (SINGLE, PIXEL, _kw, single_ops)
    if _t not in PIXEL_ONLY:
        CONFIGS["single_%s_lowdim" % _t] = (SINGLE, LOWDIM, _kw, single_ops)
assert LAUNCHES_RECORDED_ONLY == set(n for n in CONFIGS if n.startswith("single_"))
# CPP_FUSED_HEADS=0 on an ablation library: the GEMM levels of compute_gradients (rt_ddpg_pass.cpp) under the trainers that otherwise
# take the heads kernel
ABLATION_CONFIGS = {
    "ddpg_sgd_gemm_levels": (DDPG, PIXEL, {}, ddpg_step),
    "ddpg_adam_clip_gemm_levels": (DDPG, PIXEL, dict(ddpg_optimiser="Adam", gradient_clip=0.05), ddpg_step),
    "ddpg_twin_gemm_levels": (DDPG, PIXEL, dict(twin_q=True), ddpg_step),
    "ddpg_twin_min_gemm_levels": (DDPG, PIXEL, dict(twin_q=True, actor_min_q=True), ddpg_step),
    "ddpg_feature_norm_gemm_levels": (DDPG, PIXEL, dict(feature_layer_norm=True), ddpg_step),
    "ddpg_dropout_gemm_levels": (DDPG, PIXEL, dict(use_dropout=True), ddpg_step),
    "ddpg_shared_encoder_gemm_levels": (DDPG, PIXEL, dict(shared_encoder=True), ddpg_step),
}
if ABLATION:
    assert os.environ.get("CARTPOLEPP_ABLATION") not in (None, "", "0"), "the switch is compiled into the ablation builds only: CARTPOLEPP_ABLATION=1 (or a named ablation build) CPP_FUSED_HEADS=0"
    CONFIGS = ABLATION_CONFIGS

def run(name):
    (make, state), shape, kw, step = CONFIGS[name]
    agent = make(shape, **kw)
    ctx = _lib.default_context()
    digests = []
    for k in range(OUTER):
        step(agent, k)
        digests.append(sha(state(agent)))
    ctx.sync()
    ctx.prof_reset()
    ctx.prof_enable(True)
    try:
        step(agent, OUTER)
        ctx.sync()
    finally:
        ctx.prof_enable(False)
    launches = {k: int(n) for k, (_ms, n) in sorted(ctx.prof_read().items()) if n}
    ctx.prof_reset()
    agent.close()
    return {"digests": digests, "launches": launches}


out = {}
for name in (sys.argv[1:] or list(CONFIGS)):
    try:
        out[name] = run(name)
    except (Exception, SystemExit) as e:      # a refused configuration is a result; a failed launch or copy ends the run
        out[name] = {"digests": None, "launches": None, "error": "%s: %s" % (type(e).__name__, e)}
        if " -> " in str(e):
            print(json.dumps(out, sort_keys=True))
            raise
    sys.stderr.write("%s %s\n" % (name, json.dumps(out[name])[:300]))
print(json.dumps(out, sort_keys=True))
