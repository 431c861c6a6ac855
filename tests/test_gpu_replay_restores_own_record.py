"""A trainer caches several graphs (the fused step's, the literal pair's, the data-parallel step's, the half steps'), and what a body
leaves on the HOST for the accessors -- how many per-workgroup partials cpp_ddpg_last_stats adds and the batch size it divides by, the
rows behind the temperature gradient's partials of cpp_ddpg_last_sac -- is a fact of the graph that was replayed, not of the body
that happened to be built last.  Replaying the B = 8 step graph after the literal pair's graph was captured at B = 4 must report the
B = 8 minibatch's loss: the same calls on the same rows with every train_step run eagerly are the reference, bit for bit.

Only the families that keep their loss in partials can show a stale record: the fused heads kernel, the distributional critic (and
the quantile critic, dist.hip's sibling on the same path) and, for g_alpha, soft actor-critic."""
import numpy as np
import pytest

from tests.helpers import FakeEnv, ddpg_path, make_opts

pytestmark = pytest.mark.gpu

SHAPE, B_STEP, B_PAIR, ROWS = (16, 16, 3, 1, 1), 8, 4, 48


def _twin_agents(**kw):
    """tests/test_gpu_literal_loop.py's _twin_agents without the float64 oracle (whose layouts know neither an N-atom critic nor a
    Gaussian actor): two agents from one seed, perturbed alike, on the same synthetic rows"""
    from cartpoleplusplus_amd import ddpg_cartpole as D
    out = []
    for _ in range(2):
        make_opts(D, SHAPE, B_STEP, True, replay_memory_size=ROWS + 40, **kw)
        agent = D.DeepDeterministicPolicyGradientAgent(FakeEnv(SHAPE, 2))
        agent.initialise_variables(seed=3)
        rng = np.random.default_rng(103)
        for net in (agent.actor, agent.critic):
            p = net.get_params()
            net.set_params(p + rng.normal(0, 0.05, p.shape).astype(np.float32))
        agent.post_var_init_setup()
        agent.replay_memory.fill_synthetic(ROWS, seed=21)
        out.append(agent)
    return out


def _same_params(replayed, eager, what):
    for x, y in zip(replayed.networks(), eager.networks()):
        assert np.array_equal(x.get_params(), y.get_params()), (x.namespace, what)


def _run(replayed, eager):
    """train_step(8, 1) twice (eager + capture, replay), the reference's literal pair at B = 4 twice (its graph's capture, its replay),
    train_step(8, 1) once more: a replay of the FIRST graph behind a body built at another batch size"""
    from tests.test_gpu_batchnorm_training import _last_rows

    def step(k):
        replayed.train_step(B_STEP, 1)
        eager.train_step(B_STEP, 1, idxs=_last_rows(replayed, B_STEP))
        _same_params(replayed, eager, "train_step %d" % k)

    def pair(k):
        for agent in (replayed, eager):
            np.random.seed(1234 + k)                      # both draw the same rows
            batch = agent.replay_memory.batch(B_PAIR)     # ddpg_cartpole.py:332-334, verbatim
            agent.actor.train(batch.state_1)
            agent.critic.train(batch)
        _same_params(replayed, eager, "pair %d" % k)

    step(0); step(1)
    pair(0); pair(1)
    assert replayed.trainer.fused_pairs == 2 and eager.trainer.fused_pairs == 2
    step(2)
    got, want = replayed.trainer.last_stats(), eager.trainer.last_stats()
    print("last_stats replayed %r eager %r" % (got.tolist(), want.tolist()))
    assert np.array_equal(got, want)


def test_fused_heads_loss_after_a_replay_behind_another_batch_size():
    from cartpoleplusplus_amd import ddpg_cartpole as D
    replayed, eager = _twin_agents()
    try:
        hidden = D._hidden(D.opts.actor_hidden_layers), D._hidden(D.opts.critic_hidden_layers)
        for agent in (replayed, eager):      # (one eager minibatch each, drawn by the same sampler: the twins stay twins)
            assert ddpg_path(agent, B_STEP, hidden[0], hidden[1], True).startswith("heads")
        _same_params(replayed, eager, "ddpg_path")
        _run(replayed, eager)
    finally:
        replayed.close(); eager.close()


def test_distributional_loss_after_a_replay_behind_another_batch_size():
    replayed, eager = _twin_agents(distributional_critic=True, num_atoms=51, v_min=-10.0, v_max=10.0)
    try:
        _run(replayed, eager)
        for x, y in zip(replayed.trainer.last_distribution(B_STEP), eager.trainer.last_distribution(B_STEP)):
            assert np.array_equal(x, y)
    finally:
        replayed.close(); eager.close()


def test_sac_temperature_gradient_after_a_replay_behind_another_batch_size():
    replayed, eager = _twin_agents(soft_actor_critic=True)
    try:
        _run(replayed, eager)
        got, want = replayed.trainer.last_sac(B_STEP), eager.trainer.last_sac(B_STEP)
        print("g_alpha replayed %r eager %r, n %d / %d" % (got["g_alpha"], want["g_alpha"], got["n"], want["n"]))
        assert got["g_alpha"] == want["g_alpha"] and got["n"] == want["n"]
    finally:
        replayed.close(); eager.close()
