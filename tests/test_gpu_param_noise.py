"""Parameter-space exploration noise on the device (--param-noise-stddev; cpp_ddpg_set_param_noise, cpp_ddpg_param_noise_resample;
csrc/param_noise.hip) against the restatement tests/param_noise_np.py, whose comparison functions -- error over bar, none above 1 -- are
the ones tests/test_param_noise_host.py shows every planted fault to leave.  The perturbed copy's forward and the two measured action
batches are held to the float64 oracle's inference forward at the ordinary 1e-5; sigma, the count and every copy that must be a copy are
compared by bits.  Only a world of one is exercised: under --data-parallel rank r draws with seed + r, which no test here can run.

Every test of this file fails on a tree without the feature: the options do not parse and the entry points do not exist."""
import numpy as np
import pytest

from oracle import ddpg_np as O
from tests import layer_norm_np as LN
from tests import param_noise_np as PN
from tests import shared_encoder_np as SE
from tests.helpers import FakeEnv, _profiled_calls, make_opts

pytestmark = pytest.mark.gpu
ACTION_BAR = 1e-5
SEED = 0x5EEDF00D12345
HIDDEN = (20, 10)
# name: (state shape, pixel, actor hidden layers, options).  The low-dimensional actor has 62 (A = 1) / 66 (A = 2) parameters, the pixel actors
# 5382 and (layer norm) 5422 -- none a multiple of 4 or of the block -- and, without conv layers, 452; `wide` has 2 116 202, more than the
# perturbation's grid covers in one stride on 256 compute units (2048 blocks x 256 threads x 4 elements)
CONFIGS = {"lowdim": ((7,), False, (5, 3), {}),
           "8x8x6": ((8, 8, 3, 1, 2), True, HIDDEN, {}),
           "8x8x6-ln": ((8, 8, 3, 1, 2), True, HIDDEN, {"feature_layer_norm": True}),
           "8x8x6-shared": ((8, 8, 3, 1, 2), True, HIDDEN, {"shared_encoder": True}),
           "12x10x9": ((12, 10, 3, 1, 3), True, HIDDEN, {}),
           "wide": ((7,), False, (1500, 1400), {})}


def _abi():
    from cartpoleplusplus_amd._lib import lib, check, ptr
    return lib, check, ptr


def _agent(cfg, B=8, A=2, noise=True, seed=1, rows=0, **kw):
    """a device agent of configuration cfg, its parameters moved off the zero biases and the near-zero head; noise: with the feature
    (sigma 0.05, fixed: the tests configure their own through the trainer)"""
    from cartpoleplusplus_amd import ddpg_cartpole as D
    shape, pixel, hidden, extra = CONFIGS[cfg]
    opts = dict(extra, replay_memory_size=max(rows, 8) + 8, actor_hidden_layers=",".join(str(h) for h in hidden))
    if noise:
        opts.update(param_noise_stddev=0.05, param_noise_adapt=1.0, param_noise_seed=SEED)
    opts.update(kw)
    make_opts(D, shape, B, pixel, **opts)
    agent = D.DeepDeterministicPolicyGradientAgent(FakeEnv(shape, A))
    try:
        agent.initialise_variables(seed=seed)
        rng = np.random.default_rng(seed + 100)
        for net in (agent.actor, agent.critic):
            p = net.get_params()
            net.set_params(p + rng.normal(0, 0.05, p.shape).astype(np.float32))
        agent.post_var_init_setup()
        if rows:
            agent.replay_memory.fill_synthetic(rows, seed=21 + seed)
    except Exception:
        agent.close()
        raise
    return agent


def _states(cfg, n, seed=3):
    shape, pixel = CONFIGS[cfg][:2]
    rng = np.random.default_rng(seed)
    if pixel:
        return (rng.integers(0, 256, (n,) + shape).astype(np.float16) / np.float16(255)).astype(np.float16)
    return rng.standard_normal((n,) + shape).astype(np.float32)


def _n_noise(agent):
    """elements in front of the feature layer norm's gamma and beta (which close the flat buffer)"""
    names = [v for v in agent.actor.trainable_model_vars() if "/LayerNorm/" in v.name]
    total = agent.actor.num_params
    if not names:
        return total
    assert [v.name.rsplit("/", 1)[1] for v in names] == ["gamma:0", "beta:0"]
    width = names[0].shape[0]
    assert names[0].offset == total - 2 * width and names[1].offset == total - width
    return total - 2 * width


def _oracle_actions(cfg, A, actor_flat, critic_flat, states, each):
    """the float64 oracle's inference forward of an actor holding actor_flat on `states`: each image whitened with its own statistics
    (each: action_given / actions_given) or all with the batch's (the measured resample)"""
    shape, pixel, hidden, extra = CONFIGS[cfg]
    states = np.asarray(states)
    if not pixel:
        spec = O.NetSpec("actor", A, list(hidden), pixel=False, state_elems=int(np.prod(shape)))
        return O.Net(spec, actor_flat, np.float64).forward(states, training=False)["out"]
    kw = dict(pixel=True, H=shape[0], W=shape[1], C=int(np.prod(shape[2:])))
    ln = bool(extra.get("feature_layer_norm"))
    spec = LN.LnSpec("actor", A, list(hidden), **kw) if ln else O.NetSpec("actor", A, list(hidden), **kw)
    cls = LN.LnNet if ln else O.Net
    groups = [states[i:i + 1] for i in range(len(states))] if each else [states]
    out = []
    for s in groups:
        if extra.get("shared_encoder"):
            cspec = O.NetSpec("critic", A, [], **kw)
            feats, _c = SE.encoder_features(O.Net(cspec, critic_flat, np.float64), s, training=False)
            sp = SE.shared_actor_spec(spec)
            net = cls(sp, actor_flat, np.float64)
            sp.pixel = False      # (the oracle's forward from the flattened features on, as tests.shared_encoder_np's adopted actor)
            try:
                out.append(net.forward(feats, training=False)["out"])
            finally:
                sp.pixel = True
        else:
            out.append(cls(spec, actor_flat, np.float64).forward(s, training=False)["out"])
    return np.concatenate(out)


def _bits(x):
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


def _assert_inside(ratios, what):
    print(what, {k: float("%.3g" % v) for k, v in ratios.items()})
    assert PN.worst(ratios) <= 1.0, (what, ratios)


# ---- 1. the perturbation against the restatement
@pytest.mark.parametrize("cfg,A", [("lowdim", 1), ("lowdim", 2), ("8x8x6", 2), ("8x8x6-ln", 2), ("8x8x6-shared", 2), ("wide", 2)])
def test_the_perturbed_copy_is_the_restatements_element_for_element(cfg, A):
    agent = _agent(cfg, A=A)
    try:
        t, pert = agent.trainer, agent.perturbed_actor
        p = agent.actor.get_params()
        n_noise = _n_noise(agent)
        if cfg == "8x8x6-ln":
            assert n_noise == len(p) - 2 * HIDDEN[0]
        if cfg == "8x8x6-shared":      # fully connected layers only
            assert all(not v.name.split("/")[1].startswith("conv") for v in pert.trainable_model_vars()) and len(p) < 1000
        assert (len(p) % 4 != 0 or cfg == "8x8x6-shared") and pert.num_params == len(p)      # (452 there: the vector body alone)
        for sigma in ((0.05,) if cfg == "wide" else (0.0, 0.05, 1.0)):
            t.set_param_noise(pert, sigma, 0.1, 1.0, SEED)
            got = pert.get_params()
            s, d, n, adapted = t.param_noise_status()
            assert (float(s), float(d), n, adapted) == (float(np.float32(sigma)), 0.0, 1, False)
            r = PN.perturbation_ratio(got, p, sigma, SEED, 0, n_noise)
            print(cfg, A, "sigma", sigma, "worst element at %.3g of its bar" % r)
            assert r <= 1.0, (cfg, sigma, r)
            assert np.array_equal(_bits(agent.actor.get_params()), _bits(p))      # (the actor is read, never written)
            if sigma == 0.0:
                assert np.array_equal(_bits(got), _bits(p))
            else:
                assert (got[:n_noise] != p[:n_noise]).mean() > 0.99 and got[n_noise - 1] != p[n_noise - 1]
                assert np.array_equal(_bits(got[n_noise:]), _bits(p[n_noise:]))
    finally:
        agent.close()


# ---- 2. the draw count
def test_successive_resamples_differ_and_the_same_seed_and_count_give_the_same_bits():
    agent = _agent("8x8x6-ln")
    try:
        t, pert = agent.trainer, agent.perturbed_actor
        p, n_noise = agent.actor.get_params(), _n_noise(agent)
        t.set_param_noise(pert, 0.05, 0.1, 1.0, SEED)
        copies = [pert.get_params()]
        for k in range(1, 4):
            t.param_noise_resample()
            assert t.param_noise_status()[2] == k + 1
            copies.append(pert.get_params())
            assert PN.perturbation_ratio(copies[k], p, 0.05, SEED, k, n_noise) <= 1.0
        for i in range(4):
            for j in range(i):
                assert not np.array_equal(copies[i], copies[j])
        t.set_param_noise_state({"sigma": np.float32(0.05), "n": 2})      # (the copy stays until the next resample)
        assert np.array_equal(_bits(pert.get_params()), _bits(copies[3]))
        t.param_noise_resample()
        assert np.array_equal(_bits(pert.get_params()), _bits(copies[2])) and t.param_noise_status()[2] == 3
        # another seed draws other numbers at the same count
        t.set_param_noise(pert, 0.05, 0.1, 1.0, SEED + 1)
        assert not np.array_equal(pert.get_params(), copies[0])
    finally:
        agent.close()


def test_the_count_is_sixty_four_bits_wide():
    agent = _agent("lowdim", A=2)
    try:
        t, pert = agent.trainer, agent.perturbed_actor
        p = agent.actor.get_params()
        t.set_param_noise(pert, 1.0, 0.1, 1.0, SEED)
        low = pert.get_params()      # n = 0
        got = {}
        t.set_param_noise_state({"sigma": np.float32(1.0), "n": (1 << 32) - 1})
        for n in ((1 << 32) - 1, 1 << 32):
            assert t.get_param_noise_state()["n"] == n
            t.param_noise_resample()
            got[n] = pert.get_params()
            assert PN.perturbation_ratio(got[n], p, 1.0, SEED, n, len(p)) <= 1.0, n
        assert t.param_noise_status()[2] == (1 << 32) + 1
        assert not np.array_equal(got[1 << 32], low) and not np.array_equal(got[1 << 32], got[(1 << 32) - 1])
    finally:
        agent.close()


# ---- 3. the perturbed copy's forward
@pytest.mark.parametrize("cfg,A", [("lowdim", 1), ("lowdim", 2), ("8x8x6", 2), ("8x8x6-ln", 2), ("8x8x6-shared", 2), ("12x10x9", 2)])
def test_acting_with_noise_is_the_oracles_forward_of_the_devices_perturbed_parameters(cfg, A):
    states = _states(cfg, 4)
    agent = _agent(cfg, A=A)
    try:
        t, pert = agent.trainer, agent.perturbed_actor
        t.set_param_noise(pert, 0.05, 0.1, 1.0, SEED)
        first = agent.actor.action_given(states[0], True)
        second = agent.actor.action_given(states[0], True)
        assert first.shape == (1, A) and np.array_equal(_bits(first), _bits(second)), "the operand image of the fresh copy was stale"
        flat, cflat = pert.get_params(), agent.critic.get_params()
        want = _oracle_actions(cfg, A, flat, cflat, states, each=True)
        many = agent.actor.actions_given(states, True)
        err = max(np.abs(first - want[:1]).max(), np.abs(many - want).max())
        print(cfg, A, "perturbed actions vs the oracle: %.3g" % err)
        assert err < ACTION_BAR and np.abs(want).max() <= 1.0
        clean = _oracle_actions(cfg, A, agent.actor.get_params(), cflat, states, each=True)
        assert np.abs(want - clean).max() > 100 * ACTION_BAR      # (the noise is seen in the actions)
        assert np.abs(agent.actor.action_given(states[0], False) - clean[:1]).max() < ACTION_BAR
        # after the next resample the forward is the NEW copy's
        t.param_noise_resample()
        again = agent.actor.action_given(states[0], True)
        want2 = _oracle_actions(cfg, A, pert.get_params(), cflat, states[:1], each=True)
        assert np.abs(again - want2).max() < ACTION_BAR and not np.array_equal(again, first)
        quiet = agent.actor.action_given(states[0], False), agent.actor.actions_given(states, False)
    finally:
        agent.close()
    plain = _agent(cfg, A=A, noise=False)
    try:
        assert plain.perturbed_actor is None and plain.actor.perturbed is None and plain.begin_episode() is None
        assert np.array_equal(_bits(plain.actor.action_given(states[0], False)), _bits(quiet[0]))
        assert np.array_equal(_bits(plain.actor.actions_given(states, False)), _bits(quiet[1]))
    finally:
        plain.close()


# ---- 4. measure and adapt
def _measured(agent, cfg, A, dev, states, sigma0, delta, alpha):
    """configure, one measured resample on the device batch `dev`: every bar of tests.param_noise_np, and a / at against the oracle"""
    t, pert = agent.trainer, agent.perturbed_actor
    B = len(states)
    p, n_noise = agent.actor.get_params(), _n_noise(agent)
    t.set_param_noise(pert, sigma0, delta, alpha, SEED)
    before = t.param_noise_status()
    t.param_noise_resample(dev)
    words = t.param_noise_status()
    a, at = t.last_param_noise(B)
    assert PN.decided(words[1], delta, B * A), "|d - delta| is inside d's bar: the case decides nothing (d %r, delta %r)" % (words[1], delta)
    r = PN.resample_ratios(pert.get_params(), words, p, n_noise, before[:3], SEED, delta, alpha, (a, at))
    cflat = agent.critic.get_params()
    r["a"] = float(np.abs(a - _oracle_actions(cfg, A, p, cflat, states, each=False)).max()) / ACTION_BAR
    r["at"] = float(np.abs(at - _oracle_actions(cfg, A, pert.get_params(), cflat, states, each=False)).max()) / ACTION_BAR
    return r, words


@pytest.mark.parametrize("A", [1, 2, 9])
def test_distance_and_adaptation_over_batch_and_action_sizes(A):
    from cartpoleplusplus_amd import replay_memory as R
    cfg = "lowdim"
    agent = _agent(cfg, B=33, A=A)
    dev = R.DeviceBatch(33, 7, A)
    try:
        t = agent.trainer
        for B in (1, 5, 7, 33):
            states = _states(cfg, B, seed=B)
            dev.upload(states)
            for delta, alpha, grows in ((1e-6, 1.25, False), (10.0, 1.25, True), (10.0, 1.0, None)):
                r, (sigma1, d, n, adapted) = _measured(agent, cfg, A, dev, states, 0.05, delta, alpha)
                _assert_inside(r, "A %d B %d delta %g alpha %g: d %.4g" % (A, B, delta, alpha, d))
                assert adapted and n == 2 and 1e-6 < d < 10.0
                want = np.float32(0.05) if grows is None else (np.float32(0.05) * np.float32(alpha) if grows else np.float32(0.05) / np.float32(alpha))
                assert _bits(sigma1) == _bits(want)
            # a resample without a batch leaves sigma and d alone
            before = t.param_noise_status()
            t.param_noise_resample()
            after = t.param_noise_status()
            assert _bits(after[0]) == _bits(before[0]) and _bits(after[1]) == _bits(before[1]) and after[2] == before[2] + 1 and after[3] is False
            assert before[3] is True
    finally:
        dev.close()
        agent.close()


@pytest.mark.parametrize("cfg,B", [("8x8x6", 5), ("8x8x6-ln", 7), ("8x8x6-shared", 5), ("12x10x9", 33)])
def test_distance_and_adaptation_on_a_minibatch_of_the_replay_memory(cfg, B):
    """the batch is the memory's own device-side draw, as agent.begin_episode() takes it: the rows are read back for the oracle"""
    A = 2
    agent = _agent(cfg, B=B, A=A, rows=40)
    try:
        rm = agent.replay_memory
        batch = rm.sample_on_device(B, seed=7)
        states = np.asarray(rm.state[rm.state_1_idx[batch.idxs]])
        for delta, alpha in ((1e-6, 1.25), (10.0, 1.25)):
            r, (_s, d, _n, _ad) = _measured(agent, cfg, A, batch.device, states, 0.05, delta, alpha)
            _assert_inside(r, "%s B %d delta %g: d %.4g" % (cfg, B, delta, d))
    finally:
        agent.close()


def test_ten_resamples_drive_the_distance_across_the_target_and_back():
    from cartpoleplusplus_amd import replay_memory as R
    cfg, A, B, delta, alpha = "lowdim", 2, 7, 0.05, 1.5
    agent = _agent(cfg, B=B, A=A)
    dev = R.DeviceBatch(B, 7, A)
    try:
        t, pert = agent.trainer, agent.perturbed_actor
        p = agent.actor.get_params()
        states = _states(cfg, B)
        dev.upload(states)
        t.set_param_noise(pert, 0.01, delta, alpha, SEED)
        twin = PN.Restated(0.01, delta, alpha, SEED, np.float32)
        twin.resample(p, len(p))
        below = []
        for k in range(10):
            before = t.param_noise_status()
            assert _bits(before[0]) == _bits(twin.sigma) and before[2] == twin.n == k + 1
            t.param_noise_resample(dev)
            words = t.param_noise_status()
            acts = t.last_param_noise(B)
            assert PN.decided(words[1], delta, B * A), (k, words)
            _assert_inside(PN.resample_ratios(pert.get_params(), words, p, len(p), before[:3], SEED, delta, alpha, acts), "resample %d" % k)
            twin.resample(p, len(p), lambda _pt: acts)      # the restatement, step by step, on the device's own actions
            assert _bits(words[0]) == _bits(twin.sigma)      # (d itself: inside its bar above; its bits hang on the order of the f64 sum)
            below.append(bool(words[1] < np.float32(delta)))
        print("d < delta per resample:", below)
        first_above = below.index(False)
        assert below[0] and True in below[first_above:], below      # below, across, and back
    finally:
        dev.close()
        agent.close()


# ---- 5. beside the learner
def _digest(agent):
    t = agent.trainer
    out = [n.get_params() for n in agent.networks()]
    st = t.get_optimiser_state()
    out += [st["m"], st["v"], np.asarray(st["step"], np.float64), np.asarray(t.policy_delay_status(), np.float64)]
    out.append(np.asarray(t.last_stats(), np.float64))
    return [np.asarray(x) for x in out]


def _learner(noise, B=8, nb=2, **kw):
    return _agent("8x8x6", B=B, noise=noise, rows=60, ddpg_optimiser="Adam", policy_delay=2, sample_seed=5, **kw)


def test_the_learner_does_not_notice_the_resamples():
    """three fused outer steps (the eager pass and the capture, two graph replays) with measured resamples in between against an agent
    without the feature, from a common start: parameters, targets, slots and counts bit for bit, and the same launches per outer step"""
    B, nb = 8, 2
    digests, census = {}, {}
    for noise in (False, True):
        agent = _learner(noise, B, nb)
        try:
            for step in range(3):
                agent.begin_episode()
                if noise:
                    s, d, n, adapted = agent.trainer.param_noise_status()
                    assert adapted and n == step + 2 and d > 0
                    agent.actor.action_given(_states("8x8x6", 1)[0], True)
                agent.train_step(B, nb)
            agent.begin_episode()
            digests[noise] = _digest(agent)
            census[noise] = _profiled_calls(agent.actor.ctx, lambda: agent.train_step(B, nb))
            if noise:      # a resample's own launches: the perturbation and the distance, nothing else of its own name
                one = _profiled_calls(agent.actor.ctx, agent.begin_episode)
                assert one.get("param_noise", 0) == 2, one
        finally:
            agent.close()
    assert all(np.array_equal(x, y) for x, y in zip(digests[False], digests[True]))
    print(census[True])
    assert census[False] == census[True] and "param_noise" not in census[True]


def test_switched_off_again_the_agent_is_one_that_never_had_it():
    B, nb = 8, 2
    state = _states("8x8x6", 1)[0]
    out = {}
    for noise in (False, True):
        agent = _learner(noise, B, nb)
        try:
            t = agent.trainer
            if noise:
                agent.begin_episode()
                agent.train_step(B, nb)
                t.set_param_noise(None)
                assert t.param_noise is None and agent.actor.perturbed is None
                with pytest.raises(RuntimeError, match="parameter-space noise is off"):
                    t.param_noise_status()
                with pytest.raises(RuntimeError, match="parameter-space noise is off"):
                    t.param_noise_resample()
            else:
                agent.train_step(B, nb)
            np.random.seed(4)      # (the Ornstein-Uhlenbeck process is numpy's)
            agent.actor.exploration_noise = type(agent.actor.exploration_noise)(2, 0.01, 0.05)
            acted = agent.actor.action_given(state, True)
            agent.train_step(B, nb)
            agent.train_step(B, nb)
            out[noise] = _digest(agent) + [acted]
        finally:
            agent.close()
    assert all(np.array_equal(x, y) for x, y in zip(out[False], out[True]))


# ---- 6. checkpoints
def test_a_checkpoint_restores_sigma_and_the_count(tmp_path):
    from cartpoleplusplus_amd import ddpg_cartpole as D, util
    agent = _agent("8x8x6-ln", B=5, rows=20, param_noise_adapt=1.5, param_noise_target=0.05)
    try:
        assert [e[0] for e in agent.checkpoint_extras()] == ["param_noise::"]
        assert agent.perturbed_actor not in agent.networks() and len(agent.networks()) == 4
        for _ in range(3):
            agent.begin_episode()
        sigma, _d, n, adapted = agent.trainer.param_noise_status()
        assert n == 4 and adapted and _bits(sigma) != _bits(np.float32(0.05))
        util.SaverUtil(agent, str(tmp_path / "ckpt"), 3600).force_save()
        want_actor = agent.actor.get_params()
    finally:
        agent.close()
    import glob
    files = glob.glob(str(tmp_path / "ckpt" / "*.npz"))
    data = np.load(files[0])
    assert set(k for k in data.files if k.startswith("param_noise::")) == {"param_noise::sigma", "param_noise::n"}
    assert not any(k.startswith("perturbed_actor") for k in data.files)
    agent = _agent("8x8x6-ln", B=5, seed=9, param_noise_adapt=1.5, param_noise_target=0.05)
    try:
        util.SaverUtil(agent, str(tmp_path / "ckpt"), 3600)
        got = agent.trainer.param_noise_status()
        assert _bits(got[0]) == _bits(sigma) and got[2] == n
        assert np.array_equal(_bits(agent.actor.get_params()), _bits(want_actor))
        agent.begin_episode()      # (an empty memory: no batch) draws at the restored (sigma, n)
        assert PN.perturbation_ratio(agent.perturbed_actor.get_params(), want_actor, sigma, SEED, n, _n_noise(agent)) <= 1.0
    finally:
        agent.close()
    assert D.default_opts().param_noise_stddev is None


# ---- 7. the refusals at the ABI
def test_the_refusals_of_the_entry_points():
    from cartpoleplusplus_amd import base_network, ddpg_cartpole as D
    lib, check, _ptr = _abi()
    agent = _agent("8x8x6-shared", B=5)
    try:
        t, pert = agent.trainer, agent.perturbed_actor
        h = t.handle
        for args, word in (((-0.1, 0.1, 1.01), "sigma"), ((float("nan"), 0.1, 1.01), "sigma"), ((0.1, 0.0, 1.01), "target distance"),
                           ((0.1, 0.1, 0.99), "factor"), ((0.1, float("inf"), 1.01), "target distance")):
            with pytest.raises(RuntimeError, match=word):
                t.set_param_noise(pert, *args, seed=0)
        with pytest.raises(RuntimeError, match="without a perturbed network"):
            check(lib.cpp_ddpg_set_param_noise(h, None, 0.1, 0.1, 1.01, 0))
        for own in (agent.actor, agent.target_actor):
            with pytest.raises(RuntimeError, match="one a trainer owns"):
                t.set_param_noise(own, 0.1, 0.1, 1.01, 0)
        # the refusals changed nothing: the configuration of the agent's start still answers
        assert t.param_noise_status()[2] == 1 and agent.actor.perturbed is pert
        s1 = base_network.Placeholder([None, 8, 8, 3, 1, 2])
        unbound = D.ActorNetwork("unbound", s1, 2)      # encoder-less, never given to a critic
        try:
            with pytest.raises(RuntimeError, match="must be bound"):
                t.set_param_noise(unbound, 0.1, 0.1, 1.01, 0)
            check(lib.cpp_net_set_encoder(unbound.handle, agent.target_critic.handle))
            with pytest.raises(RuntimeError, match="must be bound"):      # ... to THIS trainer's critic
                t.set_param_noise(unbound, 0.1, 0.1, 1.01, 0)
        finally:
            unbound.close()
        D.opts.actor_hidden_layers = "20,11"
        other = D.ActorNetwork("other", s1, 2)
        try:
            check(lib.cpp_net_set_encoder(other.handle, agent.critic.handle))
            with pytest.raises(RuntimeError, match="layout is not the actor's"):
                t.set_param_noise(other, 0.1, 0.1, 1.01, 0)
        finally:
            other.close()
        with pytest.raises(RuntimeError, match="no resample has measured"):
            t.last_param_noise(1)
        assert agent.actor.perturbed is pert      # (a refused call leaves the exploring copy where it was)
    finally:
        agent.close()
    sac = _agent("8x8x6", B=5, noise=False, soft_actor_critic=True)
    try:
        s1 = base_network.Placeholder([None, 8, 8, 3, 1, 2])
        copy = D.ActorNetwork("copy", s1, 2)
        try:
            with pytest.raises(RuntimeError, match="soft actor-critic"):
                sac.trainer.set_param_noise(copy, 0.1, 0.1, 1.01, 0)
        finally:
            copy.close()
    finally:
        sac.close()
    with pytest.raises(SystemExit, match="--soft-actor-critic"):
        _agent("8x8x6", B=5, soft_actor_critic=True)
