"""Target policy smoothing on the device (cpp_ddpg_set_target_smoothing; csrc/heads.hip's SMOOTH instances and tps_smooth_kernel)
against its numpy restatement tests/tps_np.py: the noise read back to the bit pattern of the definition, the fused step against
SmoothedDDPG(float64) fed the restated noise, the count of target-forming passes through every entry point, and what must not
change -- check_loss, and a trainer with the feature switched off.

Bars: the noise at Z_BAR * sigma = 4e-6 * sigma (tests/test_tps_host.py: numpy's float32 evaluation sits 1.6e-6 from float64;
2.5x for a 2-ulp logf / cosine), exact where the clip binds beyond that; actions, dQ/da and Q at the suite's 1e-5; TD and the loss
at 1e-5 + discount * 4e-6 * sigma * max_b sum_i |dQ'/da'_{b,i}| (tps_np.td_bar: the noise bar propagated through the oracle's
target critic); gradients and updated parameters at tests/helpers.py's bars."""
import ctypes
import collections

import numpy as np
import pytest

from oracle import ddpg_np as O
from tests import tps_np as T
from tests.helpers import (assert_flat_close, ddpg_path, device_pool_codes, device_relu_active, dropout_masks, host_case, make_pair,
                           pool_flips_are_near_ties, relu_flips_are_at_the_boundary)

pytestmark = pytest.mark.gpu
PIX, LOWDIM, ROWS = T.CASE_SHAPE, (2, 2, 7), T.CASE_ROWS
DEFAULT_ACTOR = [100, 100, 50]
SIGMA, CLIP, SEED = T.SIGMA, T.CLIP, T.NOISE_SEED


def _abi():
    from cartpoleplusplus_amd._lib import lib, check, ptr
    return lib, check, ptr


def _agent(B, A=2, shape=PIX, pixel=True, smooth=True, rows=ROWS, seed=3, **kw):
    agent, _ref, specs = make_pair(shape, B, pixel, seed=seed, replay_size=rows + 50, action_dim=A, **kw)
    agent.replay_memory.fill_synthetic(rows, seed=21)
    if smooth:
        agent.trainer.set_target_smoothing(SIGMA, CLIP, SEED)
    return agent, specs


def assert_noise(eps, n, sigma=SIGMA, clip=CLIP, seed=SEED, what=""):
    """the device's clipped noise against the float64 restatement at count n; returns the largest distance"""
    B, A = eps.shape
    z = T.standard_normals(seed, n, B, A)
    want = np.clip(sigma * z, -clip, clip)
    bar = T.Z_BAR * sigma
    err = float(np.abs(eps.astype(np.float64) - want).max())
    print("%s noise at n=%d (%d x %d): max |eps - restated| %.3e (bar %.3e)" % (what, n, B, A, err, bar))
    assert err <= bar, (what, n, err, bar)
    binds = np.abs(sigma * z) >= clip + bar              # beyond doubt: there the device holds +-clip itself
    assert np.array_equal(eps[binds], (np.sign(z) * np.float32(clip)).astype(np.float32)[binds]), what
    assert np.abs(eps).max() <= np.float32(clip)
    return err


def _noise_of(agent, B):
    return agent.trainer.last_target_noise(B)


# ---- 1. the noise the kernels leave, at every instance of the heads kernel and on the GEMM levels
@pytest.mark.parametrize("B,A,actor_hidden,path", [
    (5, 2, DEFAULT_ACTOR, "heads+pre"),        # two workgroups, three teams without a row
    (1, 2, DEFAULT_ACTOR, "heads+pre"),        # a single row
    (16, 3, DEFAULT_ACTOR, "heads+pre"),       # the padded 4-wide instance
    (16, 8, DEFAULT_ACTOR, "heads+pre"),       # eight components
    (16, 9, DEFAULT_ACTOR, "gemm"),            # one component past the heads kernel: tps_smooth_kernel
    (16, 2, [100, 100, 65], "gemm"),           # one lane past it
], ids=["B5-A2", "B1-A2", "A3-padded", "A8", "A9-gemm", "actor-65-gemm"])
def test_noise_readback_matches_the_restatement(B, A, actor_hidden, path):
    agent, (aspec, cspec) = _agent(B, A, actor_hidden=actor_hidden)
    try:
        assert ddpg_path(agent, B, aspec.hidden, cspec.hidden, True) == path      # (one eager minibatch: n = 0)
        eps, n = _noise_of(agent, B)
        assert n == 0
        assert_noise(eps, 0, what="%s eager" % path)
        agent.train_step(B, 1)
        eps, n = _noise_of(agent, B)
        assert n == 1
        assert_noise(eps, 1, what="%s second step" % path)
        if B * A >= 32:
            assert (np.abs(eps) == np.float32(CLIP)).any() and (np.abs(eps) < np.float32(CLIP)).any()
    finally:
        agent.close()


def test_noise_readback_lowdim():
    B, A = 16, 3
    agent, (aspec, cspec) = _agent(B, A, shape=LOWDIM, pixel=False)
    try:
        assert ddpg_path(agent, B, aspec.hidden, cspec.hidden, False) == "gemm"
        for want_n in (0, 1, 2):
            if want_n:
                agent.train_step(B, 1)
            eps, n = _noise_of(agent, B)
            assert n == want_n
            assert_noise(eps, n, what="lowdim")
    finally:
        agent.close()


# ---- 2. the fused step against SmoothedDDPG(float64)
def _smoothed_step_against_f64_oracle(B, A, path, graph, host_seed=None, actor_hidden=None, per=False, nstep=0, seed=0,
                                      atol=1e-5, grad_rel=2e-5, param_rel=2e-6, flip_tol=1e-5, **pair_kw):
    """ONE minibatch of cpp_ddpg_train_step with smoothing on -- graph: its hipGraph replay on device-drawn rows, else eager on the
    caller's rows -- against tps_np.SmoothedDDPG(float64) on the same rows, parameters and the restated noise of the count the device
    reports.  host_seed: parameters, episodes and rows are host_case's, the target actor saturated on two components
    (tps_np.saturate_target_actor), so that tests/test_tps_host.py plants its faults in the same numbers.  per / nstep: a prioritized
    memory (the critic's gradient against the oracle's backward pass of w * td_dev) / an n-step memory."""
    from cartpoleplusplus_amd import ddpg_cartpole as D
    from tests import per_np as P
    lib, check, ptr = _abi()
    kw = dict(prioritized_replay=True, priority_alpha=0.6, priority_beta=0.4, priority_eps=1e-6) if per else {}
    kw.update(pair_kw)
    case = None
    if host_seed is not None:
        case = host_case(PIX, B, 1, host_seed, rows=ROWS, action_dim=A)
        kw["perturb"] = False
    agent, _ref, (aspec, cspec) = make_pair(PIX, B, True, seed=seed, replay_size=ROWS + 50, action_dim=A, actor_hidden=actor_hidden, **kw)
    steps = 0                                              # target-forming passes (= training-mode forwards) before the one checked
    try:
        rm = agent.replay_memory
        if case is not None:
            start = list(case[1])
            start[2] = T.saturate_target_actor(start[2], aspec)
            for net, p in zip(agent.networks(), start):
                assert net.get_params().shape == p.shape
                net.set_params(p)
            for ep in case[2]:
                rm.add_episode(*ep)
            assert rm.size() == ROWS
        else:
            rm.fill_synthetic(ROWS, seed=21 + seed)
        if nstep:
            rm.enable_n_step(nstep, D.opts.discount)
        agent.trainer.set_target_smoothing(SIGMA, CLIP, SEED)
        got_path = ddpg_path(agent, B, aspec.hidden, cspec.hidden, True)
        steps += 1
        assert got_path == path, (got_path, path)
        if graph:
            agent.train_step(B, 1)                        # eager pass + capture
            steps += 1
        if per:
            rm.update_priorities(np.arange(ROWS), np.random.default_rng(seed + 9).lognormal(0.0, 2.0, ROWS).astype(np.float32))
        nets = (agent.actor, agent.critic, agent.target_actor, agent.target_critic)
        Pm = [n.get_params() for n in nets]
        if graph or per:
            agent.train_step(B, 1)                        # hipGraph replay (per, eager: the same sequence on rows drawn by priority)
            idxs = np.empty(B, np.int32)
            check(lib.cpp_replay_last_indexes(rm.handle, B, ptr(idxs)))
        else:
            idxs = case[3] if case is not None else np.random.default_rng(seed + 5).integers(0, ROWS, B).astype(np.int32)
            agent.train_step(B, 1, idxs=idxs)
        eps, n = agent.trainer.last_target_noise(B)
        assert n == steps, (n, steps)
        if case is not None and not graph:
            assert n == T.ORACLE_CASES["A%d" % A][3]      # (the count tests/test_tps_host.py plants its faults at)
        assert_noise(eps, n, what="%s A=%d graph=%s" % (path, A, graph))
        w = rm.last_weights(B) if per else None
        actions, dq_da, q, td = agent.trainer.last_values(B)
        g_a, g_c = agent.actor.get_grads(), agent.critic.get_grads()
        stats = agent.trainer.last_stats()
        Pn = [x.get_params() for x in nets]
        codes_a, codes_c = device_pool_codes(agent.actor, B), device_pool_codes(agent.critic, B)
        relu_a, relu_c = device_relu_active(agent.actor, B), device_relu_active(agent.critic, B)
        hb = rm.batch(idxs=idxs)
        s1, s2 = rm.state[hb.state_1_idx], rm.state[hb.state_2_idx]
        a, r, m = hb.action, hb.reward, hb.terminal_mask
    finally:
        agent.close()
    ref = T.SmoothedDDPG(aspec, cspec, Pm[0], Pm[1], np.float64)
    ref.set_targets(Pm[2], Pm[3])
    if aspec.dropout:
        ref.actor.drop_masks = dropout_masks("actor", aspec.hidden, B, steps)
        ref.target_actor.drop_masks = dropout_masks("target_actor", aspec.hidden, B, steps)
    ref.actor.amax_override, ref.critic.amax_override = codes_a, codes_c
    ref.actor.relu_override, ref.critic.relu_override = relu_a, relu_c
    t = (s1, a, r, m, s2)
    noise = T.target_noise(SEED, n, B, A, SIGMA, CLIP)
    ag = ref.actor_gradients(s1)
    cg = ref.critic_gradients(t, noise)
    pool_flips_are_near_ties(ag["cache_actor"], codes_a, flip_tol, what="actor")
    pool_flips_are_near_ties(cg["cache_critic"], codes_c, flip_tol, what="critic")
    relu_flips_are_at_the_boundary(ag["cache_actor"], relu_a, flip_tol, what="actor")
    relu_flips_are_at_the_boundary(cg["cache_critic"], relu_c, flip_tol, what="critic")
    bar = T.td_bar(ref.hp.discount, SIGMA, cg["target_dq_da"], atol)
    err = {"actions": float(np.abs(actions - ag["actions"]).max()), "dq_da": float(np.abs(dq_da - ag["dq_da"]).max()),
           "q": float(np.abs(q - cg["q"]).max()), "td": float(np.abs(td - cg["td"]).max())}
    w64 = w.astype(np.float64).reshape(-1, 1) if per else 1.0
    loss = float(np.mean(w64 * cg["td"] ** 2))
    err["loss"] = abs(float(stats[0]) - loss)
    unsmoothed = float(np.abs(ref.critic_gradients(t, None)["td"] - cg["td"]).max())
    print("%s A=%d graph=%s per=%s nstep=%d n=%d: %s; TD bar %.3e; the smoothing moves TD by %.3e" % (path, A, graph, per, nstep, n, err, bar, unsmoothed))
    assert unsmoothed > 100 * bar
    assert err["actions"] < atol and err["dq_da"] < atol and err["q"] < atol, err
    assert err["td"] < bar and err["loss"] < bar, (err, bar)
    assert_flat_close(aspec, g_a, ag["grads"], rel=grad_rel, what="actor pre-clip grads vs f64 oracle")
    if per:
        c_grads = ref.critic_gradients(t, noise, td_override=w64 * td.astype(np.float64))["grads"]
        assert_flat_close(cspec, g_c, c_grads, rel=grad_rel, what="weighted critic pre-clip grads vs f64 oracle at w * td_dev")
    else:
        c_grads = cg["grads"]
        try:
            assert_flat_close(cspec, g_c, c_grads, rel=grad_rel, what="critic pre-clip grads vs f64 oracle", abs_floor=2.0 * err["td"])
        except AssertionError:
            # (tests/helpers.py, fused_step_against_f64_oracle: the gradients are linear in TD -- the backward arithmetic alone, at the device's TD)
            c_grads = ref.critic_gradients(t, noise, td_override=td)["grads"]
            assert_flat_close(cspec, g_c, c_grads, rel=grad_rel, what="critic pre-clip grads vs f64 oracle's backward pass of the device's TD")
    hp = ref.hp
    ca, _ = O.clip_by_global_norm(ag["grads"], hp.gradient_clip, np.float64)
    cc, _ = O.clip_by_global_norm(c_grads, hp.gradient_clip, np.float64)
    want_a, want_c = Pm[0] - hp.actor_lr * ca, Pm[1] - hp.critic_lr * cc
    assert_flat_close(aspec, Pn[0], want_a, rel=param_rel, what="actor params after the step")
    assert_flat_close(cspec, Pn[1], want_c, rel=param_rel, what="critic params after the step")
    assert_flat_close(aspec, Pn[2], O.soft_update(Pm[2], want_a, hp.target_update_rate, np.float64), rel=1e-6, what="target actor")
    assert_flat_close(cspec, Pn[3], O.soft_update(Pm[3], want_c, hp.target_update_rate, np.float64), rel=1e-6, what="target critic")
    for name, new, old, want in (("actor", Pn[0], Pm[0], want_a), ("critic", Pn[1], Pm[1], want_c)):
        d_got, d_want = new.astype(np.float64) - old, want - old
        assert np.linalg.norm(d_got - d_want) < 2.0 ** -23 * np.linalg.norm(old) + 5e-5 * np.linalg.norm(d_want), name
    return cg, noise


@pytest.mark.parametrize("A,actor_hidden,path,graph", [
    (2, None, "heads+pre", False), (2, None, "heads+pre", True),
    (2, [100, 100, 63], "heads", False), (2, [100, 100, 63], "heads", True),
    (9, None, "gemm", False)], ids=["heads+pre-eager", "heads+pre-graph", "heads-eager", "heads-graph", "A9-gemm-eager"])
def test_fused_step_against_the_smoothed_f64_oracle(A, actor_hidden, path, graph):
    B, _A, host_seed, _n = T.ORACLE_CASES["A%d" % A]
    # (host_case's networks are the default widths: the 'heads' cases take their own parameters and synthetic rows)
    cg, noise = _smoothed_step_against_f64_oracle(B, A, path, graph, host_seed=host_seed if actor_hidden is None else None,
                                                  actor_hidden=actor_hidden)
    if actor_hidden is None:      # both clamps at work, as tests/test_tps_host.py requires of these cases
        raw = cg["target_actions"] + noise
        assert (np.abs(noise) == CLIP).mean() >= 0.25 and (raw > 1).any(axis=1).sum() >= 2 and (raw < -1).any(axis=1).sum() >= 2


# ---- 3. the count
def test_graph_replays_count_and_a_reconfigured_stream_starts_over():
    B, A = 16, 2
    agent, _ = _agent(B, A)
    try:
        seen = []
        for _ in range(4):                                 # eager pass + capture, then three replays
            agent.train_step(B, 1)
            eps, n = _noise_of(agent, B)
            assert_noise(eps, n, what="replay")
            seen.append((n, eps))
        assert [n for n, _e in seen] == [0, 1, 2, 3]
        assert not np.array_equal(seen[0][1], seen[1][1])
        agent.trainer.set_target_smoothing(SIGMA, CLIP, SEED)
        agent.train_step(B, 1)
        eps, n = _noise_of(agent, B)
        assert n == 0 and np.array_equal(eps, seen[0][1])
        agent.train_step(B, 1)
        eps, n = _noise_of(agent, B)
        assert n == 1 and np.array_equal(eps, seen[1][1])
        agent.trainer.set_target_smoothing(SIGMA, CLIP, SEED + 1)      # another seed: another stream
        agent.train_step(B, 1)
        eps, n = _noise_of(agent, B)
        assert n == 0 and not np.array_equal(eps, seen[0][1])
        assert_noise(eps, 0, seed=SEED + 1, what="other seed")
    finally:
        agent.close()


def test_every_target_forming_entry_point_advances_the_count_by_one():
    """cpp_ddpg_compute_gradients, cpp_ddpg_train_critic, cpp_ddpg_sample_and_compute (eager, then its graph), every minibatch of
    cpp_ddpg_dp_train_step (one graph; then the half-step form of sync_every = 2) and of cpp_ddpg_train_step, cpp_ddpg_train_rows;
    cpp_ddpg_check_loss and cpp_ddpg_train_actor in between do not"""
    lib, check, ptr = _abi()
    B, A = 8, 2
    agent, _ = _agent(B, A)
    try:
        t, rm = agent.trainer, agent.replay_memory
        count = [0]

        def expect(passes, what):
            count[0] += passes
            eps, n = _noise_of(agent, B)
            assert n == count[0] - 1, (what, n, count[0] - 1)
            assert_noise(eps, n, what=what)
        HostBatch = collections.namedtuple("HostBatch", "state_1 action reward terminal_mask state_2")
        hb = rm.batch(idxs=np.arange(B, dtype=np.int32))
        host = HostBatch(np.asarray(hb.state_1), hb.action, hb.reward, hb.terminal_mask, np.asarray(hb.state_2))
        dev = t.device_batch_for(host)
        check(lib.cpp_ddpg_compute_gradients(t.handle, dev.handle)); expect(1, "compute_gradients")
        agent.critic.train(host); expect(1, "train_critic")
        agent.critic.check_loss(host); expect(0, "check_loss")
        agent.actor.train(host.state_1); expect(0, "train_actor")
        check(lib.cpp_ddpg_sample_and_compute(t.handle, rm.handle, B, 5)); expect(1, "sample_and_compute, eager")
        check(lib.cpp_ddpg_sample_and_compute(t.handle, rm.handle, B, 5)); expect(1, "sample_and_compute, graph")
        check(lib.cpp_ddpg_dp_train_step(t.handle, rm.handle, None, B, 2, 7, 1, 0)); expect(2, "dp_train_step, eager")
        check(lib.cpp_ddpg_dp_train_step(t.handle, rm.handle, None, B, 2, 7, 1, 0)); expect(2, "dp_train_step, graph")
        check(lib.cpp_ddpg_dp_train_step(t.handle, rm.handle, None, B, 2, 7, 2, 0)); expect(2, "dp_train_step, sync_every 2")
        agent.train_step(B, 3); expect(3, "train_step, eager")
        agent.train_step(B, 3); expect(3, "train_step, graph")
        agent.train_step(B, 2, idxs=np.arange(2 * B)); expect(2, "train_step on rows")
        for k in range(3):
            b = rm.batch(idxs=np.arange(k, k + B, dtype=np.int32))
            agent.actor.train(b.state_1); agent.critic.train(b); expect(1, "train_rows %d" % k)
        assert t.fused_pairs == 3
    finally:
        agent.close()


# ---- 4. the reference's loop
def test_reference_loop_is_the_fused_minibatch():
    """`actor.train(batch.state_1); critic.train(batch)` on the same rows at the same count: the noise bits and the parameters of
    agent.train_step(B, 1, idxs).  The agents are built from the command line's options."""
    B = 8
    kw = dict(target_policy_noise=0.3, target_policy_noise_clip=0.4, target_policy_noise_seed=77)
    lit, _ = _agent(B, smooth=False, **kw)
    fused, _ = _agent(B, smooth=False, **kw)
    try:
        assert lit.trainer.target_smoothing == (0.3, 0.4, 77)
        np.random.seed(99)
        for step in range(4):
            batch = lit.replay_memory.batch(B)
            lit.actor.train(batch.state_1)
            lit.critic.train(batch)
            lit.target_actor.update_weights()
            lit.target_critic.update_weights()
            fused.train_step(B, 1, idxs=batch.idxs)
            (e1, n1), (e2, n2) = _noise_of(lit, B), _noise_of(fused, B)
            assert n1 == n2 == step and np.array_equal(e1, e2)
            assert_noise(e1, step, sigma=0.3, clip=0.4, seed=77, what="literal loop")
            for x, y in zip(lit.networks(), fused.networks()):
                assert np.array_equal(x.get_params(), y.get_params()), (step, x.namespace)
        assert lit.trainer.fused_pairs == 4
    finally:
        lit.close(); fused.close()


# ---- 5. check_loss is an evaluation
def test_check_loss_adds_no_noise_and_leaves_the_count():
    B = 16
    agent, _ = _agent(B)
    try:
        agent.train_step(B, 1)
        batch = agent.replay_memory.batch(idxs=np.arange(B, dtype=np.int32))
        on = agent.critic.check_loss(batch)
        assert _noise_of(agent, B)[1] == 0
        agent.train_step(B, 1)
        assert _noise_of(agent, B)[1] == 1                 # (consecutive: check_loss took no count)
        on2 = agent.critic.check_loss(batch)
        agent.trainer.set_target_smoothing(0.0, 0.0, SEED)
        off = agent.critic.check_loss(batch)
        for x, y in zip(on2, off):
            assert np.array_equal(np.asarray(x), np.asarray(y))
        assert not np.array_equal(on[1], on2[1])           # (the parameters moved in between: the comparison is not vacuous)
    finally:
        agent.close()


# ---- 6. off means off
def test_switched_off_is_a_trainer_that_never_had_it():
    B = 16
    was_on, _ = _agent(B)
    never, _ = _agent(B, smooth=False)
    try:
        start = [n.get_params() for n in never.networks()]
        for _ in range(2):
            was_on.train_step(B, 1)
        was_on.trainer.set_target_smoothing(0.0, 0.0, SEED)
        with pytest.raises(RuntimeError, match="smoothing is off"):
            was_on.trainer.last_target_noise(B)
        with pytest.raises(RuntimeError, match="smoothing is off"):
            never.trainer.last_target_noise(B)
        for net, p in zip(was_on.networks(), start):
            net.set_params(p)
        idxs = np.random.default_rng(4).integers(0, ROWS, 2 * B).astype(np.int32)
        for agent in (was_on, never):
            agent.train_step(B, 2, idxs=idxs)
        for x, y in zip(was_on.networks(), never.networks()):
            assert np.array_equal(x.get_params(), y.get_params()), x.namespace
        assert np.array_equal(was_on.trainer.last_stats(), never.trainer.last_stats())
        # ... and on again moves them apart
        was_on.trainer.set_target_smoothing(SIGMA, CLIP, SEED)
        for agent in (was_on, never):
            agent.train_step(B, 1, idxs=idxs[:B])
        assert not np.array_equal(was_on.critic.get_params(), never.critic.get_params())
    finally:
        was_on.close(); never.close()


# ---- 7, 8. with the other opt-in extensions
def test_prioritized_replay_on_the_padded_weighted_instance():
    _smoothed_step_against_f64_oracle(32, 3, "heads+pre", True, per=True)


def test_n_step_returns():
    _smoothed_step_against_f64_oracle(16, 2, "heads+pre", True, nstep=3, seed=1)


def test_dropout_keeps_the_folded_layer_out():
    _smoothed_step_against_f64_oracle(16, 2, "heads", False, actor_hidden=[100, 97, 50], use_dropout=True, seed=2)


# ---- 9. the data-parallel step as a world of one
def test_data_parallel_step_draws_the_fused_steps_noise():
    lib, check, _ptr = _abi()
    B = 16
    dp, _ = _agent(B)
    one, _ = _agent(B)
    try:
        for step in range(3):                              # eager + capture, then replays
            check(lib.cpp_ddpg_dp_train_step(dp.trainer.handle, dp.replay_memory.handle, None, B, 2, 0, 1, 0))
            one.train_step(B, 2)
            (e1, n1), (e2, n2) = _noise_of(dp, B), _noise_of(one, B)
            assert n1 == n2 == 2 * step + 1 and np.array_equal(e1, e2)
            assert_noise(e1, n1, what="data-parallel step")
    finally:
        dp.close(); one.close()


# ---- 10. determinism
def test_three_runs_are_identical():
    B, out = 16, []
    for _ in range(3):
        agent, _ = _agent(B)
        try:
            for _step in range(3):
                agent.train_step(B, 2)
            out.append([n.get_params() for n in agent.networks()] + [_noise_of(agent, B)[0]])
        finally:
            agent.close()
    for other in out[1:]:
        for x, y in zip(out[0], other):
            assert np.array_equal(x, y)


# ---- 11. refusals
def test_refusals_through_the_abi():
    lib, _check, _ptr = _abi()
    B = 4
    agent, _ = _agent(B, smooth=False, rows=40)
    try:
        h = agent.trainer.handle
        for sigma, clip in ((-0.1, 0.5), (float("nan"), 0.5), (float("inf"), 0.5), (0.2, -0.5), (0.2, float("nan")), (0.2, float("inf")),
                            (0.2, 0.0)):
            assert lib.cpp_ddpg_set_target_smoothing(h, ctypes.c_float(sigma), ctypes.c_float(clip), 1) == 1, (sigma, clip)      # CPP_ERR_ARG
            assert b"cpp_ddpg_set_target_smoothing" in lib.cpp_last_error()
        assert lib.cpp_ddpg_last_target_noise(h, B, None, None) == 3                                                              # CPP_ERR_STATE
        assert lib.cpp_ddpg_set_target_smoothing(h, ctypes.c_float(0.2), ctypes.c_float(0.5), 1) == 0
        assert lib.cpp_ddpg_last_target_noise(h, 0, None, None) == 1 and lib.cpp_ddpg_last_target_noise(h, B + 1, None, None) == 1
        agent.train_step(B, 1)
        assert np.isfinite(agent.critic.get_params()).all()
    finally:
        agent.close()
