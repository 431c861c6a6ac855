"""Soft actor-critic on the device against tests/sac_np.py (float64): the sample and its log-density, the soft reward, the temporal
difference, both gradient lists, the temperature, the target actor's copy, the forms of the training step, the refusals.

Every comparison feeds the device's own eps (read through last_sac) into the restatement; eps itself is checked against the restated
draw.  The bars are tests/sac_np.py's (tests/test_sac_host.py derives them): the project's 1e-5 on a, Q, td and dQ/da, eight times the
float32 restatement's error on the rest."""
import collections
import ctypes as C

import numpy as np
import pytest

from oracle import ddpg_np as O
from tests import sac_np as S
from tests.helpers import FakeEnv, _profiled_calls, fill_with_rendered_episodes, make_opts

pytestmark = pytest.mark.gpu

Batch = collections.namedtuple("Batch", "state_1 action reward terminal_mask state_2")
PIXEL = (16, 16, 3, 1, 2)
HYPER = O.Hyper(actor_lr=0.01, critic_lr=0.01, discount=0.9, gradient_clip=None, target_update_rate=0.05)


def _abi():
    from cartpoleplusplus_amd import _lib
    return _lib


def _agent(shape, B, pixel, A=2, seed=1, replay=64, perturb=0.05, hyper=HYPER, **kw):
    from cartpoleplusplus_amd import ddpg_cartpole as D
    kw.setdefault("soft_actor_critic", True)
    opt = dict(actor_learning_rate=hyper.actor_lr, critic_learning_rate=hyper.critic_lr, discount=hyper.discount, target_update_rate=hyper.target_update_rate)
    opt.update(kw)
    make_opts(D, shape, B, pixel, replay_memory_size=replay, **opt)
    agent = D.DeepDeterministicPolicyGradientAgent(FakeEnv(shape, A))
    agent.initialise_variables(seed=seed)
    if perturb:
        rng = np.random.default_rng(seed + 100)
        for net in (agent.actor, agent.critic):
            p = net.get_params()
            net.set_params(p + rng.normal(0, perturb, p.shape).astype(np.float32))
    agent.post_var_init_setup()
    return agent


def _ref(agent, shape, pixel, A, hyper=HYPER, dt=np.float64, temperature=0.1, lr=1e-4, seed=0):
    from cartpoleplusplus_amd import ddpg_cartpole as D
    kw = dict(pixel=True, H=shape[0], W=shape[1], C=int(np.prod(shape[2:]))) if pixel else dict(pixel=False, state_elems=int(np.prod(shape)))
    aspec = S.gaussian_spec(A, D._hidden(D.opts.actor_hidden_layers), **kw)
    cspec = O.NetSpec("critic", A, D._hidden(D.opts.critic_hidden_layers), **kw)
    ref = S.SacDDPG(aspec, cspec, agent.actor.get_params(), agent.critic.get_params(), dt, hyper,
                    state=S.SacState(temperature, -float(A), lr, seed))
    ref.target_critic = O.Net(cspec, agent.target_critic.get_params(), dt)
    return ref


def _identity_actor(agent, A):
    """an actor whose head is its state: h = relu([s, -s]), (m | x) = h[:2A] - h[2A:] -- exact in float32, so that the device's head is
    tests/sac_np.py's case to the bit"""
    n = 2 * A
    eye = np.eye(n, dtype=np.float32)
    flat = np.concatenate([np.concatenate([eye, -eye], axis=1).ravel(), np.zeros(2 * n, np.float32),
                           np.concatenate([eye, -eye], axis=0).ravel(), np.zeros(n, np.float32)])
    assert len(flat) == agent.actor.num_params
    agent.actor.set_params(flat)
    agent.target_actor.set_params(flat)


def _compute(agent, batch):
    lib = _abi()
    t = agent.trainer
    dev = t.device_batch_for(batch)
    lib.check(lib.lib.cpp_ddpg_compute_gradients(t.handle, dev.handle))
    return t.last_sac(len(batch.state_1))


def _apply(agent):
    lib = _abi()
    lib.check(lib.lib.cpp_ddpg_apply_gradients(agent.trainer.handle, 1.0))


def _err(got, want):
    return float(np.max(np.abs(np.asarray(got, np.float64).reshape(-1) - np.asarray(want, np.float64).reshape(-1))))


# ---- 1. the row-local kernels on the shared cases: every B and A off the wave and workgroup multiples
@pytest.mark.parametrize("B,A", S.CASES)
def test_one_minibatch_against_the_float64_restatement(B, A):
    case = S.head_case(B, A)
    state = np.concatenate([case["m"], case["x"]], axis=1)
    agent = _agent((2, A), B, False, A, actor_hidden_layers=str(4 * A), critic_hidden_layers="16,8", sac_init_temperature=float(case["alpha"]),
                   sac_temperature_learning_rate=1e-2, sac_seed=7, discount=float(case["discount"]), gradient_clip=None)
    try:
        _identity_actor(agent, A)
        rng = np.random.default_rng(B + A)
        batch = Batch(state.reshape(B, 2, A), rng.uniform(-1, 1, (B, A)).astype(np.float32), case["r"].reshape(B, 1), case["mask"].reshape(B, 1),
                      state.reshape(B, 2, A))
        hyper = HYPER._replace(discount=float(case["discount"]))
        ref = _ref(agent, (2, A), False, A, hyper, temperature=float(case["alpha"]), lr=1e-2, seed=7)
        got = _compute(agent, batch)
        acts, dq, q, td = agent.trainer.last_values(B)
        # the noise: the restated draw of pass 0 on the two streams
        assert got["n"] == 0
        assert _err(got["eps"], case["eps1"]) <= S.eps_bar() and _err(got["eps2"], case["eps2"]) <= S.eps_bar()
        want = ref.train_minibatch(batch, got["eps"], got["eps2"])
        np.testing.assert_array_equal(want["m"], case["m"])      # (the identity actor: the oracle's head is the case's)
        fig = {"a": _err(got["a"], want["actions"]), "a2": _err(got["a2"], want["target_actions"]), "logp": _err(got["logp"], want["logp"]),
               "logp2": _err(got["logp2"], want["logp2"]), "r_soft": _err(got["r_soft"], want["r_soft"]), "q": _err(q, want["q"]),
               "td": _err(td, want["td"]), "dq_da": _err(dq, want["dq_da"]), "g_alpha": abs(got["g_alpha"] - float(want["g_alpha"]))}
        print("B %d A %d" % (B, A), {k: "%.2e" % v for k, v in fig.items()})
        fig["dm"], fig["dx"] = _err(got["dz"][:, :A], want["dm"]), _err(got["dz"][:, A:], want["dx"])      # the B x 2A head gradient itself
        for k, v in fig.items():
            assert v <= S.bar("logp" if k == "logp2" else k), (k, v)
        assert abs(got["alpha"] - float(case["alpha"])) < 1e-7
        assert abs(agent.trainer.last_stats()[0] - float(want["loss"])) <= 1e-5 * max(1.0, abs(float(want["loss"])))
        np.testing.assert_array_equal(acts, got["a"])
        # the actor's list: the head layer's [dW; db] = [h, 1]^T (d m | d x) -- |error| <= sum_b |h_b| bar(d x); the layer below through
        # |W| as well (W = [I; -I]: one entry per column).  The critic's list at the project's relative bound on its norm.
        ga, gc = agent.actor.get_grads(), agent.critic.get_grads()
        h = np.maximum(np.concatenate([state, -state], axis=1), 0).astype(np.float64)
        dz_bar = max(S.bar("dm"), S.bar("dx"))
        n = 2 * A
        off = n * 2 * n + 2 * n
        bound_w = np.repeat((np.abs(h).sum(axis=0) * dz_bar + 1e-5)[:, None], n, axis=1).ravel()
        assert np.all(np.abs(ga[off:off + 2 * n * n] - want["actor_grads"][off:off + 2 * n * n]) <= bound_w)
        assert _err(ga[off + 2 * n * n:], want["actor_grads"][off + 2 * n * n:]) <= B * dz_bar + 1e-5
        assert _err(ga[:off], want["actor_grads"][:off]) <= (np.abs(state).sum(axis=0).max() + B) * dz_bar + 1e-5
        assert np.linalg.norm(gc - want["critic_grads"]) <= 2e-5 * np.linalg.norm(want["critic_grads"]) + 1e-6
        # apply: the temperature's Adam step, both lists, the target actor's copy
        _apply(agent)
        st = agent.trainer.get_sac_state()
        assert abs(float(st["log_alpha"]) - float(want["log_alpha"])) <= S.bar("log_alpha") and int(st["step"]) == 1
        np.testing.assert_array_equal(agent.target_actor.get_params(), agent.actor.get_params())
        assert _err(agent.actor.get_params(), ref.actor.flat()) <= hyper.actor_lr * ((np.abs(state).sum(axis=0).max() + B) * dz_bar + 1e-5) + 1e-6
    finally:
        agent.close()


@pytest.mark.parametrize("B,A", [(5, 1), (3, 64), (65, 64)])
def test_the_forward_entry_points_return_tanh_of_the_mean_and_draw_nothing(B, A):
    """also at A = 64, which no trainer reaches (a critic takes action dimensions up to 16)"""
    from cartpoleplusplus_amd import base_network, ddpg_cartpole as D
    make_opts(D, (2, A), B, False, actor_hidden_layers=str(4 * A), soft_actor_critic=True)
    actor = D.ActorNetwork("actor", base_network.Placeholder([None, 2, A]), A)
    try:
        n = 2 * A
        eye = np.eye(n, dtype=np.float32)
        actor.set_params(np.concatenate([np.concatenate([eye, -eye], axis=1).ravel(), np.zeros(2 * n, np.float32),
                                         np.concatenate([eye, -eye], axis=0).ravel(), np.zeros(n, np.float32)]))
        rng = np.random.default_rng(A)
        s = rng.normal(0, 2, (B, 2, A)).astype(np.float32)
        flat = s.reshape(B, n)
        a = actor.forward(s)
        assert _err(a, np.tanh(flat[:, :A].astype(np.float64))) <= 1e-5
        np.testing.assert_array_equal(a, actor.forward(s))
        np.testing.assert_array_equal(a, actor.actions_given(s))
        m, ls = actor.forward_gaussian(s)
        np.testing.assert_array_equal(m, flat[:, :A])
        assert _err(ls, S.log_std(flat[:, A:])) <= 1e-5
        noisy = actor.actions_given(s, add_noise=True)
        assert np.all(np.abs(noisy) <= 1) and not np.array_equal(noisy, a)
        info = [C.c_int(), C.c_float(), C.c_float()]
        lib = _abi()
        lib.check(lib.lib.cpp_net_gaussian_info(actor.handle, *[C.byref(v) for v in info]))
        assert (info[0].value, info[1].value, info[2].value) == (1, -10.0, 2.0)
    finally:
        actor.close()


# ---- 2. the steps: outer steps on a replay memory, every form, on the small pixel geometry
def _pixel_agent(B=8, rows=40, **kw):
    agent = _agent(PIXEL, B, True, 2, **kw)
    fill_with_rendered_episodes(agent, PIXEL, rows)
    return agent


def _state(agent):
    st = agent.trainer.get_sac_state()
    return [agent.actor.get_params(), agent.critic.get_params(), agent.target_actor.get_params(), agent.target_critic.get_params(),
            np.array([st["log_alpha"], st["m"], st["v"]], np.float32)]


def _rows(agent, rows):
    """(s1, a, r, mask, s2) of the memory's rows, on the host"""
    b = agent.replay_memory.batch(len(rows), idxs=rows)
    return (np.asarray(b.state_1), np.asarray(b.action), np.asarray(b.reward), np.asarray(b.terminal_mask), np.asarray(b.state_2))


def test_outer_steps_on_pixels_against_the_float64_restatement_and_the_target_actor_is_the_actor():
    B, nb = 5, 2
    kw = dict(sac_init_temperature=0.2, sac_temperature_learning_rate=1e-2, sac_seed=3, gradient_clip=None)
    agent = _pixel_agent(B, **kw)
    try:
        rng = np.random.default_rng(5)
        rm = agent.replay_memory
        ref = _ref(agent, PIXEL, True, 2, temperature=0.2, lr=1e-2, seed=3)
        for step in range(2):
            idxs = rng.integers(0, rm.size(), nb * B).astype(np.int32)
            # minibatch by minibatch (the eager fused body on given rows), so that each one's eps can be read back
            for k in range(nb):
                rows = idxs[k * B:(k + 1) * B]
                agent.train_step(B, 1, idxs=rows)
                got = agent.trainer.last_sac(B)
                assert got["n"] == step * nb + k
                z1, z2 = S.noise(3, got["n"], B, 2, S.STREAM_S1), S.noise(3, got["n"], B, 2, S.STREAM_S2)
                assert _err(got["eps"], z1) <= S.eps_bar() and _err(got["eps2"], z2) <= S.eps_bar()
                assert np.abs(got["eps"] - got["eps2"]).max() > 0.1
                want = ref.train_minibatch(_rows(agent, rows), got["eps"], got["eps2"])
                ref.update_targets()
                acts, dq, q, td = agent.trainer.last_values(B)
                for name, g, w, bar in (("a", got["a"], want["actions"], 1e-5), ("a2", got["a2"], want["target_actions"], 1e-5),
                                        ("q", q, want["q"], 1e-5), ("td", td, want["td"], 1e-5), ("dq_da", dq, want["dq_da"], 1e-5),
                                        ("logp", got["logp"], want["logp"], S.bar("logp")), ("r_soft", got["r_soft"], want["r_soft"], S.bar("r_soft")),
                                        ("g_alpha", got["g_alpha"], want["g_alpha"], S.bar("g_alpha"))):
                    assert _err(g, w) <= bar, (step, k, name, _err(g, w))
                np.testing.assert_array_equal(agent.target_actor.get_params(), agent.actor.get_params())
                assert abs(float(agent.trainer.get_sac_state()["log_alpha"]) - float(want["log_alpha"])) <= S.bar("log_alpha")
        assert _err(agent.critic.get_params(), ref.critic.flat()) <= 2e-5
        assert _err(agent.target_critic.get_params(), ref.target_critic.flat()) <= 2e-5
        assert _err(agent.actor.get_params(), ref.actor.flat()) <= 2e-5
    finally:
        agent.close()


RIDER = (64, 64, 3, 2, 3)      # conv1's operand images and their rider in the optimiser's launch exist at 64 x 64 only


# (optimiser, actor's rate): gradient descent and Momentum at 0.1; Adam's update is ~ its rate per element whatever the gradient's size, so
# it runs at tests.ddpg_opt_np.RATES' 2e-3 -- under Adam the rider restates Adam's element for conv1, another piece of the optimiser's launch
RIDER_OPTIMISERS = {"gradient-descent": 0.1, "momentum-0.5": 0.1, "adam": 2e-3}


@pytest.mark.parametrize("opt", sorted(RIDER_OPTIMISERS))
def test_where_the_image_rider_runs_the_target_forward_reads_the_copied_parameters(opt):
    """three minibatches in one call at 64x64x18: the optimiser's launch of minibatch 2 builds the target actor's conv1 operand image
    from its parameters BEFORE the copy behind it.  a' of minibatch 3 must come from the actor as minibatch 2 left it: compared with a
    forward of a second agent that stopped there, at the device's own eps.  (Two device evaluations, each held to 1e-5 of the float64
    value elsewhere: 2e-5 between them.  The actor's rate is RIDER_OPTIMISERS', so that one minibatch moves a' by far more.)"""
    B, nb = 8, 3
    idxs = np.random.default_rng(12).integers(0, 40, nb * B).astype(np.int32)
    from tests import td3_np as T3
    kw = dict(T3.opt_kw(opt), actor_learning_rate=RIDER_OPTIMISERS[opt], sac_seed=6, sac_init_temperature=0.2)
    before = _agent(RIDER, B, True, 2, **kw)
    try:
        fill_with_rendered_episodes(before, RIDER, 40)
        before.train_step(B, nb - 1, idxs=idxs[:(nb - 1) * B])
        moved = before.trainer.last_sac(B)["a2"]
        agent = _agent(RIDER, B, True, 2, **kw)
        try:
            fill_with_rendered_episodes(agent, RIDER, 40)
            agent.train_step(B, nb, idxs=idxs)
            got = agent.trainer.last_sac(B)
            np.testing.assert_array_equal(agent.target_actor.get_params(), agent.actor.get_params())
            s2 = _rows(agent, idxs[-B:])[4]
        finally:
            agent.close()
        m, ls = before.actor.forward_gaussian(s2)
        want = np.tanh(m.astype(np.float64) + np.exp(ls.astype(np.float64)) * got["eps2"])
        assert got["n"] == nb - 1
        assert _err(got["a2"], want) <= 2e-5, _err(got["a2"], want)
        # (the comparison has power against exactly this fault: the actor after minibatch 2 with ONLY its conv1 weights and biases taken
        # from the actor after minibatch 1 -- what a stale operand image would compute -- answers differently by more than 10x the bar)
        stale = _agent(RIDER, B, True, 2, **kw)
        try:
            fill_with_rendered_episodes(stale, RIDER, 40)
            stale.train_step(B, nb - 2, idxs=idxs[:(nb - 2) * B])
            n1 = 5 * 5 * int(np.prod(RIDER[2:])) * 10 + 10                      # conv1's block opens the flat buffer
            names = [v.name for v in stale.actor.trainable_model_vars()[:3]]
            assert names[0].endswith("conv1/weights:0") and names[1].endswith("conv1/biases:0") and "conv2" in names[2]
            assert stale.actor.trainable_model_vars()[2].offset == n1
            mixed = before.actor.get_params().copy()
            mixed[:n1] = stale.actor.get_params()[:n1]
            stale.actor.set_params(mixed)
            m1, ls1 = stale.actor.forward_gaussian(s2)
        finally:
            stale.close()
        shift = _err(np.tanh(m1.astype(np.float64) + np.exp(ls1.astype(np.float64)) * got["eps2"]), want)
        assert shift > 10 * 2e-5 and moved.shape == want.shape, shift
    finally:
        before.close()


def _run_form(form, B=8, nb=2, steps=3, **kw):
    """the same three outer steps as the eager body, graph replays, or the literal loop's deferred pairs"""
    agent = _pixel_agent(B, sac_seed=5, sac_temperature_learning_rate=1e-2, sample_seed=11, **kw)
    lib = _abi()
    try:
        sac = []
        if form == "literal":
            rng = np.random.default_rng(3)
            for _ in range(steps):
                for _k in range(nb):
                    batch = agent.replay_memory.batch(B, idxs=rng.integers(0, agent.replay_memory.size(), B))
                    agent.actor.train(batch.state_1)
                    agent.critic.train(batch)
                    sac.append(agent.trainer.last_sac(B))
                agent.target_actor.update_weights()
                agent.target_critic.update_weights()
            assert agent.trainer.fused_pairs == steps * nb
        elif form == "rows":
            rng = np.random.default_rng(3)
            for _ in range(steps):
                for _k in range(nb):
                    rows = rng.integers(0, agent.replay_memory.size(), B).astype(np.int32)
                    lib.check(lib.lib.cpp_ddpg_train_rows(agent.trainer.handle, agent.replay_memory.handle, B, lib.ptr(rows)))
                    sac.append(agent.trainer.last_sac(B))
                lib.check(lib.lib.cpp_ddpg_update_targets(agent.trainer.handle))
        else:
            for _ in range(steps):
                if form == "eager":
                    _profiled_calls(agent.actor.ctx, lambda: agent.train_step(B, nb))      # (profiling keeps the call on stream launches)
                else:
                    agent.train_step(B, nb)
                sac.append(agent.trainer.last_sac(B))
        return _state(agent), sac
    finally:
        agent.close()


def test_eager_runs_graph_replays_and_repeated_runs_are_bit_identical_and_every_replay_draws_fresh_noise():
    eager, _ = _run_form("eager")
    graph, sac = _run_form("graph")
    again, _ = _run_form("graph")
    for x, y, z in zip(eager, graph, again):
        np.testing.assert_array_equal(x, y)
        np.testing.assert_array_equal(y, z)
    assert [o["n"] for o in sac] == [1, 3, 5]                       # two passes per outer step; the replays advance the device's count
    assert np.abs(sac[1]["eps"] - sac[2]["eps"]).max() > 0.1 and np.abs(sac[1]["eps2"] - sac[2]["eps2"]).max() > 0.1
    np.testing.assert_array_equal(graph[0], graph[2])                # target actor == actor


def test_the_literal_loops_deferred_pairs_are_the_fused_minibatch_on_rows_bit_for_bit():
    literal, sac_l = _run_form("literal")
    rows, sac_r = _run_form("rows")
    for x, y in zip(literal, rows):
        np.testing.assert_array_equal(x, y)
    assert [o["n"] for o in sac_l] == list(range(6)) == [o["n"] for o in sac_r]
    np.testing.assert_array_equal(literal[0], literal[2])


# ---- 3. the single ops
def test_train_actor_then_train_critic_is_the_definition():
    """the actor's op updates the actor and the temperature; the critic's op behind it still samples a' from the actor as it stood, reads
    the temperature as it stood, and closes the minibatch with the copy"""
    B, A = 5, 2
    agent = _agent((2, 3), B, False, A, actor_hidden_layers="12,8", critic_hidden_layers="12,8", sac_init_temperature=0.2,
                   sac_temperature_learning_rate=1e-2, sac_seed=9, gradient_clip=None, perturb=0.3)
    try:
        ref = _ref(agent, (2, 3), False, A, temperature=0.2, lr=1e-2, seed=9)
        rng = np.random.default_rng(2)
        t = agent.trainer
        for i in range(3):
            batch = Batch(rng.normal(0, 1, (B, 2, 3)).astype(np.float32), rng.uniform(-1, 1, (B, A)).astype(np.float32),
                          rng.normal(0, 1, (B, 1)).astype(np.float32), (rng.uniform(size=(B, 1)) > 0.3).astype(np.float32),
                          rng.normal(0, 1, (B, 2, 3)).astype(np.float32))
            before = agent.actor.get_params()
            agent.actor.train(batch.state_1)
            first = t.last_sac(B)
            np.testing.assert_array_equal(agent.target_actor.get_params(), before)      # not yet: the critic's op closes the minibatch
            agent.critic.train(batch)
            second = t.last_sac(B)
            assert second["n"] == i and _err(second["eps2"], S.noise(9, i, B, A, S.STREAM_S2)) <= S.eps_bar()
            assert _err(first["eps"], S.noise(9, i, B, A, S.STREAM_S1)) <= S.eps_bar()
            want = ref.train_minibatch(batch, first["eps"], second["eps2"])
            assert _err(first["a"], want["actions"]) <= 1e-5 and _err(first["logp"], want["logp"]) <= S.bar("logp")
            assert _err(second["a2"], want["target_actions"]) <= 1e-5 and _err(second["r_soft"], want["r_soft"]) <= S.bar("r_soft")
            assert _err(t.last_values(B)[3], want["td"]) <= 1e-5
            np.testing.assert_array_equal(agent.target_actor.get_params(), agent.actor.get_params())
            assert abs(float(t.get_sac_state()["log_alpha"]) - float(want["log_alpha"])) <= S.bar("log_alpha")
        assert _err(agent.actor.get_params(), ref.actor.flat()) <= 2e-5 and _err(agent.critic.get_params(), ref.critic.flat()) <= 2e-5
    finally:
        agent.close()


def test_check_loss_and_the_evaluations_are_deterministic_and_leave_the_count_alone():
    B, A = 5, 2
    agent = _agent((2, 3), B, False, A, actor_hidden_layers="12,8", critic_hidden_layers="12,8", sac_seed=4, perturb=0.3, gradient_clip=None)
    try:
        ref = _ref(agent, (2, 3), False, A, seed=4)
        rng = np.random.default_rng(8)
        batch = Batch(rng.normal(0, 1, (B, 2, 3)).astype(np.float32), rng.uniform(-1, 1, (B, A)).astype(np.float32),
                      rng.normal(0, 1, (B, 1)).astype(np.float32), np.ones((B, 1), np.float32), rng.normal(0, 1, (B, 2, 3)).astype(np.float32))
        got = _compute(agent, batch)
        assert got["n"] == 0
        l1, l2 = agent.critic.check_loss(batch), agent.critic.check_loss(batch)
        for x, y in zip(l1, l2):
            np.testing.assert_array_equal(x, y)
        want = ref.critic_gradients(batch, None, training=False)      # eps = 0: the entropy term of the mean action stays
        assert _err(l1[1], want["td"]) <= 1e-5 and abs(l1[0] - float(want["loss"])) <= 1e-5 * max(1.0, float(want["loss"]))
        assert np.abs(want["r_soft"] - batch.reward[:, 0]).max() > 0.01
        before = agent.trainer.last_sac(B)
        d1, d2 = agent.critic.q_gradients_wrt_actions(batch), agent.critic.q_gradients_wrt_actions(batch)
        after = agent.trainer.last_sac(B)
        assert after["g_alpha"] == before["g_alpha"] and after["alpha"] == before["alpha"]      # (an evaluation leaves the temperature's gradient alone)
        np.testing.assert_array_equal(d1, d2)
        assert _err(d1, ref.actor_gradients(batch.state_1, None)["dq_da"]) <= 1e-5
        np.testing.assert_array_equal(agent.actor.forward(batch.state_1), agent.actor.forward(batch.state_1))
        assert _compute(agent, batch)["n"] == 1                          # only the gradient pass before moved it
    finally:
        agent.close()


# ---- 4. the temperature
def test_a_fixed_temperature_launches_no_apply_and_a_learned_one_launches_one_per_minibatch():
    B, nb = 8, 2
    counts = {}
    for lr in (0.0, 1e-3):
        agent = _pixel_agent(B, sac_temperature_learning_rate=lr, sac_init_temperature=0.3)
        try:
            counts[lr] = _profiled_calls(agent.actor.ctx, lambda: agent.train_step(B, nb)).get("sac", 0)
            agent.train_step(B, nb)
            st = agent.trainer.get_sac_state()
            if lr == 0.0:
                assert float(st["log_alpha"]) == float(np.log(np.float32(0.3))) and int(st["step"]) == 0
            else:
                assert float(st["log_alpha"]) != float(np.log(np.float32(0.3))) and int(st["step"]) == 2 * nb
        finally:
            agent.close()
    assert counts[0.0] == 3 * nb and counts[1e-3] == 4 * nb, counts      # sample, target, head gradient (+ the temperature's apply)


def test_the_launches_of_a_sac_outer_step_are_the_scalar_steps_on_the_gemm_levels_plus_the_named_additions():
    """family by family against the scalar step on the same GEMM levels (the ablation build's CPP_FUSED_HEADS=0 is a build of its own:
    here the scalar trainer is forced onto the levels by a twin-free, policy-delay-free low-dimensional critic, which never fuses)"""
    B, nb = 5, 2
    rows = {}
    for sac in (False, True):
        agent = _agent((2, 3), B, False, 2, actor_hidden_layers="12,8", critic_hidden_layers="12,8", soft_actor_critic=sac,
                       **(dict(sac_temperature_learning_rate=1e-3) if sac else {}))
        try:
            rng = np.random.default_rng(0)
            s = [rng.normal(0, 1, (2, 3)).astype(np.float32) for _ in range(31)]
            agent.replay_memory.add_episode(s[0], [(rng.uniform(-1, 1, (1, 2)).astype(np.float32), 1.0, s[i + 1]) for i in range(30)])
            rows[sac] = _profiled_calls(agent.actor.ctx, lambda: agent.train_step(B, nb))
        finally:
            agent.close()
    plain, sac = rows[False], rows[True]
    assert plain.get("sac", 0) == 0 and sac["sac"] == 4 * nb
    # the same GEMMs in two more launches per minibatch: jobs 1 / 2 and job 3 each stand between two levels of the longest chain (the
    # actor's head, the second critic evaluation, dQ/da, the actor's backward), and the round in which they run still launches the other
    # chains' ready GEMMs on its own.  Every other family launches what it launched.
    assert sac["gemm"] == plain["gemm"] + 2 * nb, (plain, sac)
    for fam in set(plain) | set(sac):
        if fam not in ("sac", "gemm"):
            assert sac.get(fam, 0) == plain.get(fam, 0), (fam, plain, sac)


# ---- 5. what composes
@pytest.mark.parametrize("opt", ["Adam", "Momentum"])
def test_with_twin_q_and_the_other_optimisers_the_target_takes_the_smaller_head(opt):
    B = 8
    agent = _pixel_agent(B, twin_q=True, ddpg_optimiser=opt, sac_seed=2, sac_init_temperature=0.2, sac_temperature_learning_rate=1e-3, discount=0.9)
    try:
        rng = np.random.default_rng(4)
        for _ in range(3):
            rows = rng.integers(0, agent.replay_memory.size(), B).astype(np.int32)
            agent.train_step(B, 1, idxs=rows)
        got = agent.trainer.last_sac(B)
        _acts, _dq, q, td = agent.trainer.last_values(B)
        q2, tq1, tq2, td2 = agent.trainer.last_twin_values(B)
        _s1, _a, r, mask, _s2 = (np.asarray(v, np.float64) for v in _rows(agent, rows))
        rs = S.soft_reward(r, mask, 0.9, got["alpha"], got["logp2"])
        assert _err(got["r_soft"], rs) <= S.bar("r_soft") and np.abs(rs - r.reshape(-1)).max() > 1e-3
        y = rs + mask.reshape(-1) * np.float64(np.float32(0.9)) * np.minimum(tq1, tq2).reshape(-1).astype(np.float64)
        assert _err(td, q.reshape(-1) - y) <= 1e-5 and _err(td2, q2.reshape(-1) - y) <= 1e-5
        assert got["n"] == 2 and np.isfinite(agent.actor.get_params()).all()
        np.testing.assert_array_equal(agent.target_actor.get_params(), agent.actor.get_params())
    finally:
        agent.close()


def _soft_target_checks(agent, B, rows, discount=0.9, weights=None):
    """r_soft, both temporal differences and the loss of the last minibatch recomputed from the memory's own reward and mask columns of
    its rows (an n-step memory: the folded reward, the mask carrying discount^(n-1)), the device's logp', alpha and target values"""
    got = agent.trainer.last_sac(B)
    _acts, _dq, q, td = agent.trainer.last_values(B)
    q2, tq1, tq2, td2 = agent.trainer.last_twin_values(B)
    _s1, _a, r, mask, _s2 = (np.asarray(v, np.float64) for v in _rows(agent, rows))
    rs = S.soft_reward(r, mask, discount, got["alpha"], got["logp2"])
    assert _err(got["r_soft"], rs) <= S.bar("r_soft") and np.abs(rs - r.reshape(-1)).max() > 1e-3
    y = rs + mask.reshape(-1) * np.float64(np.float32(discount)) * np.minimum(tq1, tq2).reshape(-1).astype(np.float64)
    assert _err(td, q.reshape(-1) - y) <= 1e-5 and _err(td2, q2.reshape(-1) - y) <= 1e-5
    w = np.ones(B) if weights is None else np.asarray(weights, np.float64).reshape(-1)
    loss = float(np.mean(w * ((q.reshape(-1) - y) ** 2 + (q2.reshape(-1) - y) ** 2)))
    assert abs(float(agent.trainer.last_stats()[0]) - loss) <= 1e-5 * max(1.0, loss), (agent.trainer.last_stats()[0], loss)
    return got, td.reshape(-1), mask.reshape(-1)


def test_with_prioritized_replay_and_n_step_the_loss_is_weighted_and_the_priorities_come_from_td():
    B, nb = 8, 2
    agent = _pixel_agent(B, twin_q=True, prioritized_replay=True, n_step=3, sac_seed=2, sac_init_temperature=0.2, discount=0.9, priority_alpha=1.0,
                         priority_eps=1e-3, priority_beta=0.5, priority_beta_final=0.5)
    lib = _abi()
    try:
        for _ in range(3):
            agent.train_step(B, nb)
        rows = np.zeros(B, np.int32)
        lib.check(lib.lib.cpp_replay_last_indexes(agent.replay_memory.handle, B, lib.ptr(rows)))
        w = np.asarray(agent.replay_memory.last_weights(B), np.float64)
        assert w.min() > 0 and w.max() <= 1.0 + 1e-6 and w.max() - w.min() > 1e-3      # (importance weights that weigh)
        got, td, mask = _soft_target_checks(agent, B, rows, weights=w)
        assert got["n"] == 3 * nb - 1 and set(np.round(mask, 6)) - {0.0, 1.0}             # the mask column carries discount^(n-1) here
        np.testing.assert_array_equal(agent.target_actor.get_params(), agent.actor.get_params())
        # (rows drawn twice in one minibatch keep the priority of their last occurrence: compare the rows that occur once)
        once = [i for i in range(B) if list(rows).count(rows[i]) == 1]
        pri = np.asarray(agent.replay_memory.priorities(rows[once]), np.float64)
        np.testing.assert_allclose(pri, np.abs(td[once]).astype(np.float64) + 1e-3, rtol=1e-5)
    finally:
        agent.close()


def test_with_random_shift_and_the_u8_store():
    B = 8
    agent = _agent(PIXEL, B, True, 2, replay_store="u8", sac_seed=2, twin_q=True, sac_init_temperature=0.2)
    lib = _abi()
    try:
        fill_with_rendered_episodes(agent, PIXEL, 40, as_u8=True)
        agent.replay_memory.enable_random_shift(2, seed=3)
        for _ in range(2):
            agent.train_step(B, 2)
        rows = np.zeros(B, np.int32)
        lib.check(lib.lib.cpp_replay_last_indexes(agent.replay_memory.handle, B, lib.ptr(rows)))
        got, _td, _mask = _soft_target_checks(agent, B, rows)
        assert got["n"] == 3 and np.abs(np.asarray(agent.replay_memory.last_shifts(B))).max() > 0      # (the gathers were shifted ones)
        np.testing.assert_array_equal(agent.target_actor.get_params(), agent.actor.get_params())
    finally:
        agent.close()


# ---- 6. checkpoints
def test_checkpoints_carry_the_temperature_and_the_layout_check_refuses_both_ways(tmp_path):
    from cartpoleplusplus_amd import util
    B = 8
    agent = _pixel_agent(B, sac_temperature_learning_rate=1e-2)
    try:
        saver = util.SaverUtil(agent, str(tmp_path / "sac"), 3600)      # (no checkpoint yet: initialises the variables, as main() has it)
        agent.post_var_init_setup()
        agent.train_step(B, 2)
        saver.force_save()
        want, st = _state(agent), agent.trainer.get_sac_state()
        assert int(st["step"]) == 2
        data = np.load(str(tmp_path / "sac" / open(str(tmp_path / "sac" / "checkpoint")).read().split('"')[1]) + ".npz")
        assert {"sac::log_alpha", "sac::m", "sac::v", "sac::step"} <= set(data.files)
    finally:
        agent.close()
    agent = _pixel_agent(B, seed=7, sac_temperature_learning_rate=1e-2)
    try:
        util.SaverUtil(agent, str(tmp_path / "sac"), 3600)
        for x, y in zip(_state(agent), want):
            np.testing.assert_array_equal(x, y)
        assert int(agent.trainer.get_sac_state()["step"]) == 2
        with pytest.raises(AssertionError, match="checkpoint does not match actor"):
            plain = _pixel_agent(B, soft_actor_critic=False)
            try:
                util.SaverUtil(plain, str(tmp_path / "plain"), 3600).force_save()
                util.SaverUtil(plain, str(tmp_path / "sac"), 3600)
            finally:
                plain.close()
        with pytest.raises(AssertionError, match="checkpoint does not match actor"):
            util.SaverUtil(agent, str(tmp_path / "plain"), 3600)
    finally:
        agent.close()


# ---- 7. the refusals
def test_the_runtime_refusals():
    from cartpoleplusplus_amd import ddpg_cartpole as D, base_network
    lib = _abi()
    L = lib.lib
    agent = _agent((2, 3), 4, False, 2, actor_hidden_layers="8", critic_hidden_layers="8")
    plain = None
    try:
        t = agent.trainer
        for call, match in ((lambda: t.set_target_smoothing(0.2, 0.5, 0), "soft actor-critic"), (lambda: t.set_policy_delay(2), "soft actor-critic"),
                            (lambda: t.set_sac(0.0, -2.0, 1e-3, 0), "temperature"), (lambda: t.set_sac(0.1, float("nan"), 1e-3, 0), "entropy"),
                            (lambda: t.set_sac(0.1, -2.0, -1.0, 0), "rate"),
                            (lambda: lib.check(L.cpp_ddpg_sample_and_compute(t.handle, agent.replay_memory.handle, 4, 0)), "data-parallel"),
                            (lambda: lib.check(L.cpp_ddpg_dp_train_step(t.handle, agent.replay_memory.handle, None, 4, 1, 0, 1, 0)), "data-parallel")):
            with pytest.raises(RuntimeError, match=match):
                call()
        t.set_policy_delay(1)
        # mixed pairs, the critics that are refused, NAF
        ctx = agent.actor.ctx.handle
        h = C.c_void_p()
        hp = lib.DdpgHyper(1e-3, 1e-2, 0.9, 5.0, 1e-3)
        make_opts(D, (2, 3), 4, False, actor_hidden_layers="8", critic_hidden_layers="8")
        plain = D.DeepDeterministicPolicyGradientAgent(FakeEnv((2, 3), 2))
        with pytest.raises(RuntimeError, match="Gaussian target actor"):
            lib.check(L.cpp_ddpg_create(ctx, agent.actor.handle, agent.critic.handle, plain.target_actor.handle, agent.target_critic.handle, C.byref(hp), C.byref(h)))
        with pytest.raises(RuntimeError, match="not Gaussian"):
            plain.trainer.set_sac(0.1, -2.0, 1e-3, 0)
        with pytest.raises(RuntimeError, match="not Gaussian"):
            plain.trainer.last_sac(4)
        with pytest.raises(RuntimeError, match="not a Gaussian actor"):
            lib.check(L.cpp_net_forward_gaussian(plain.actor.handle, lib.ptr(np.zeros((1, 6), np.float32)), 0, 1, 0, lib.ptr(np.zeros((1, 2), np.float32)),
                                                 lib.ptr(np.zeros((1, 2), np.float32))))
        info = C.c_int(7)
        lib.check(L.cpp_net_gaussian_info(plain.actor.handle, C.byref(info), None, None))
        assert info.value == 0
        lib.check(L.cpp_net_gaussian_info(agent.critic.handle, C.byref(info), None, None))
        assert info.value == 0
        spec = agent.actor.spec
        for lo, hi, match in ((1.0, 1.0, "bounds"), (float("-inf"), 0.0, "bounds"), (2.0, -10.0, "bounds")):
            with pytest.raises(RuntimeError, match=match):
                lib.check(L.cpp_net_create_gaussian(ctx, C.byref(spec), 4, lo, hi, C.byref(h)))
        with pytest.raises(RuntimeError, match="belongs to an actor"):
            lib.check(L.cpp_net_create_gaussian(ctx, C.byref(agent.critic.spec), 4, -10.0, 2.0, C.byref(h)))
        wide = lib.NetSpec.from_buffer_copy(spec)
        wide.action_dim = 65
        with pytest.raises(RuntimeError, match=r"outside \[1, 64\]"):
            lib.check(L.cpp_net_create_gaussian(ctx, C.byref(wide), 4, -10.0, 2.0, C.byref(h)))
        # a Gaussian pair with different bounds; Gaussian actors whose spec asks for batch norm or dropout; NAF
        made = []
        try:
            def gaussian(lo, hi, **flags):
                sp = lib.NetSpec.from_buffer_copy(spec)
                for k, v in flags.items():
                    setattr(sp, k, v)
                g = C.c_void_p()
                lib.check(L.cpp_net_create_gaussian(ctx, C.byref(sp), 4, lo, hi, C.byref(g)))
                made.append(g)
                return g
            other = gaussian(-5.0, 1.0)
            with pytest.raises(RuntimeError, match="same log std bounds"):
                lib.check(L.cpp_ddpg_create(ctx, agent.actor.handle, agent.critic.handle, other, agent.target_critic.handle, C.byref(hp), C.byref(h)))
            for flags in (dict(use_batch_norm=1), dict(use_dropout=1)):
                a1, a2 = gaussian(-10.0, 2.0, **flags), gaussian(-10.0, 2.0, **flags)
                with pytest.raises(RuntimeError, match="batch norm or dropout"):
                    lib.check(L.cpp_ddpg_create(ctx, a1, agent.critic.handle, a2, agent.target_critic.handle, C.byref(hp), C.byref(h)))
            nh = lib.NafHyper(0.9, 5.0, 1e-3, 0, 1e-3, 0.0, 0.9, 0.999, 1e-8)
            with pytest.raises(RuntimeError, match="Gaussian actor .* belongs to the DDPG learner"):
                lib.check(L.cpp_naf_create(ctx, other, other, other, other, 0, C.byref(nh), C.byref(h)))
        finally:
            for g in made:
                L.cpp_net_destroy(g)
        # (cpp_ddpg_allreduce_grads and cpp_ddpg_average_params refuse such a trainer too, behind their NULL check: they need a
        # communicator, which takes a second process to make -- not triggered here)
        t.set_target_smoothing(0.0, 0.0, 0)      # "off" is accepted and leaves the noise count alone
        # a quantile critic under a Gaussian actor
        make_opts(D, (2, 3), 4, False, actor_hidden_layers="8", critic_hidden_layers="8", quantile_critic=True)
        qc = D.CriticNetwork("critic", plain.actor)
        try:
            with pytest.raises(RuntimeError, match="distributional or quantile"):
                lib.check(L.cpp_ddpg_create(ctx, agent.actor.handle, qc.handle, agent.target_actor.handle, qc.handle, C.byref(hp), C.byref(h)))
        finally:
            qc.close()
        # batches above what the partial buffers hold
        make_opts(D, (2, 3), 1028, False, actor_hidden_layers="8", critic_hidden_layers="8", soft_actor_critic=True)
        big = D.DeepDeterministicPolicyGradientAgent(FakeEnv((2, 3), 2))
        try:
            with pytest.raises(RuntimeError, match="batches up to 1024"):
                big.trainer
        finally:
            big.close()
    finally:
        agent.close()
        if plain is not None:
            plain.close()


# ---- 8. off means off
def test_a_plain_trainer_made_after_a_sac_one_launches_and_computes_what_it_did():
    """a scalar trainer's outer steps in a process that has run soft actor-critic before: the launch census and the bits of a run without"""
    B, nb = 8, 2

    def plain_run():
        agent = _pixel_agent(B, soft_actor_critic=False, sample_seed=5)
        try:
            census = _profiled_calls(agent.actor.ctx, lambda: agent.train_step(B, nb))
            for _ in range(2):
                agent.train_step(B, nb)
            return census, [agent.actor.get_params(), agent.critic.get_params(), agent.target_actor.get_params(), agent.target_critic.get_params()]
        finally:
            agent.close()

    first = plain_run()
    sac = _pixel_agent(B)
    try:
        sac.train_step(B, nb)
    finally:
        sac.close()
    second = plain_run()
    assert first[0] == second[0] and "sac" not in first[0]
    for x, y in zip(first[1], second[1]):
        np.testing.assert_array_equal(x, y)
    assert not np.array_equal(first[1][0], first[1][2])      # (and its target actor is a soft-updated one)
