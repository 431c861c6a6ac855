"""The single train ops are the gradient pass with one half asked for (rt_ddpg_pass.cpp: compute_gradients; rt_ddpg.h: PassParts).

Two trainers are built from the same seeds and fed the same host batch.  One runs cpp_ddpg_compute_gradients -- on the GEMM levels of
the release library: a low-dimensional critic has no prefix in front of its action splice, nine actions are more than the fused heads
kernel takes, a categorical critic and a Gaussian actor never take it --, the other q_gradients_wrt_actions, check_loss, train_actor and
train_critic.  Byte for byte (tobytes()):
    the fully connected slices of the actor's and the critic's gradients;
    dq_da of q_gradients_wrt_actions against cpp_ddpg_last_values' dq_da;  td of check_loss against last_values' td.
Soft actor-critic: the two evaluations run at eps = 0, the pass draws -- what they return is another quantity.  Its dq_da and td are
compared where the single TRAIN ops leave them (last_values behind train_actor and train_critic), and cpp_ddpg_set_sac, which zeroes the
noise count, is called before each side.
The conv slices of the pixel case come from other launches on the two sides (one network per launch against two): both sides are held
to the float64 oracle at tests/helpers.py's bar (assert_flat_close, 2e-5 relative L2 per variable), not to each other."""
import numpy as np
import pytest

from oracle import ddpg_np as O
from tests import dist_np, twin_np
from tests.helpers import FakeEnv, _profiled_calls, assert_flat_close, make_opts

pytestmark = pytest.mark.gpu

LOWDIM, PIXEL = ((2, 2, 7), 2, 5), ((16, 16, 3, 1, 2), 9, 8)      # shape, A, B
DIST = (51, -10.0, 10.0)
TRAINERS = {"plain": {}, "twin": dict(twin_q=True),
            "categorical": dict(distributional_critic=True, num_atoms=DIST[0], v_min=DIST[1], v_max=DIST[2]),
            "sac": dict(soft_actor_critic=True)}
CASES = [pytest.param(LOWDIM, t, id="lowdim-A2-B5-" + t) for t in ("plain", "twin", "categorical", "sac")] + \
        [pytest.param(PIXEL, t, id="16x16x6-A9-B8-" + t) for t in ("plain", "twin", "categorical")]


class HostBatch(object):
    def __init__(self, t):
        self.state_1, self.action, self.reward, self.terminal_mask, self.state_2 = t


def _agent(shape, A, B, kw):
    """tests.helpers.make_pair's agent (its seeds and perturbation) for any trainer"""
    from cartpoleplusplus_amd import ddpg_cartpole as D
    make_opts(D, shape, B, len(shape) == 5, replay_memory_size=8, **kw)
    agent = D.DeepDeterministicPolicyGradientAgent(FakeEnv(shape, A))
    agent.initialise_variables(seed=0)
    rng = np.random.default_rng(100)

    def perturb(nets, sd):
        for net in nets:
            p = net.get_params()
            net.set_params(p + rng.normal(0, sd, p.shape).astype(np.float32))
    perturb((agent.actor, agent.critic), 0.05)
    agent.post_var_init_setup()
    perturb((agent.target_actor, agent.target_critic), 0.01)
    return agent


def _reset_noise(agent):
    t = agent.trainer
    if t.sac:
        t.set_sac(t.sac["init_temperature"], t.sac["target_entropy"], t.sac["temperature_learning_rate"], t.sac["seed"])


def _specs(shape, A, trainer):
    from cartpoleplusplus_amd import ddpg_cartpole as D
    kw = dict(pixel=True, H=shape[0], W=shape[1], C=int(np.prod(shape[2:])))
    aspec = O.NetSpec("actor", A, D._hidden(D.opts.actor_hidden_layers), **kw)
    cspec = O.NetSpec("critic", A, D._hidden(D.opts.critic_hidden_layers), **kw)
    return aspec, dist_np.dist_spec(cspec, DIST[0]) if trainer == "categorical" else cspec


def _oracle_grads(specs, trainer, P, t):
    hyper = O.DEFAULT_HYPER
    if trainer == "twin":
        ref = twin_np.restatement(specs, P, np.float64, hyper)
    elif trainer == "categorical":
        ref = dist_np.restatement(specs, P, DIST, np.float64, hyper)
    else:
        ref = O.DDPG(specs[0], specs[1], P[0], P[1], np.float64)
        ref.set_targets(P[2], P[3])
    return ref.actor_gradients(t[0])["grads"], ref.critic_gradients(t)["grads"]


def _conv_slices_against_oracle(layout_spec, got, want, what):
    """only the conv variables of `got` are compared: every other slice is the oracle's own"""
    mixed, off = np.asarray(want, np.float64).copy(), 0
    for name, shp in layout_spec.layout():
        n = int(np.prod(shp))
        if name.startswith("conv"):
            mixed[off:off + n] = got[off:off + n]
        off += n
    assert off == len(got) == len(want), (off, len(got), len(want))
    assert_flat_close(layout_spec, mixed, want, rel=2e-5, what=what)


@pytest.mark.parametrize("case,trainer", CASES)
def test_single_ops_leave_what_the_pass_leaves(case, trainer):
    from cartpoleplusplus_amd._lib import lib, check
    shape, A, B = case
    pixel = len(shape) == 5
    t = O.synthetic_batch(np.random.default_rng(5), B, shape, A, pixel)
    hb = HostBatch(t)
    whole, single = _agent(shape, A, B, TRAINERS[trainer]), _agent(shape, A, B, TRAINERS[trainer])
    try:
        P = [n.get_params() for n in whole.networks()]
        for p, q in zip(P, [n.get_params() for n in single.networks()]):
            assert p.tobytes() == q.tobytes()
        # ---- the pass, both halves
        _reset_noise(whole)
        tr = whole.trainer
        dev = tr.device_batch_for(hb)
        seen = _profiled_calls(whole.actor.ctx, lambda: check(lib.cpp_ddpg_compute_gradients(tr.handle, dev.handle)))
        assert seen.get("heads", 0) == 0 and seen.get("gemm", 0) > 0, seen      # (the GEMM levels)
        _act, dq_da, _q, td = tr.last_values(B)
        ga, gc = whole.actor.get_grads(), whole.critic.get_grads()
        # ---- the single ops
        _reset_noise(single)
        if trainer == "sac":
            single.actor.train(hb.state_1)
            ga1 = single.actor.get_grads()
            single.critic.train(hb)
            _act1, dq_da1, _q1, td1 = single.trainer.last_values(B)
        else:
            dq_da1 = single.critic.q_gradients_wrt_actions(hb)
            _loss, td1, _q1 = single.critic.check_loss(hb)
            single.actor.train(hb.state_1)
            ga1 = single.actor.get_grads()
            single.critic.train(hb)
        gc1 = single.critic.get_grads()
    finally:
        whole.close()
        single.close()
    assert np.abs(dq_da).max() > 0 and np.abs(td).max() > 0 and np.abs(ga).max() > 0 and np.abs(gc).max() > 0
    assert dq_da1.tobytes() == dq_da.tobytes(), np.abs(dq_da1 - dq_da).max()
    assert td1.tobytes() == td.tobytes(), np.abs(td1 - td).max()
    specs = _specs(shape, A, trainer) if pixel else None
    for name, spec, g, g1 in (("actor", specs and specs[0], ga, ga1), ("critic", specs and specs[1], gc, gc1)):
        assert g.shape == g1.shape
        fc0 = sum(int(np.prod(shp)) for n, shp in spec.layout() if n.startswith("conv")) if pixel else 0
        assert fc0 < len(g)
        assert g1[fc0:].tobytes() == g[fc0:].tobytes(), (name, np.abs(g1[fc0:] - g[fc0:]).max())
    if pixel:
        want_a, want_c = _oracle_grads(specs, trainer, P, t)
        cl = twin_np.TwinLayoutSpec(specs[1]) if trainer == "twin" else specs[1]
        for side, a_, c_ in (("the pass", ga, gc), ("the single ops", ga1, gc1)):
            _conv_slices_against_oracle(specs[0], a_, want_a, "actor conv gradients of %s" % side)
            _conv_slices_against_oracle(cl, c_, want_c, "critic conv gradients of %s" % side)
