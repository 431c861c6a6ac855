"""Delayed policy updates on the device (--policy-delay; cpp_ddpg_set_policy_delay: the hold word of csrc/optim.hip's segments, written
by csrc/heads.hip's last thread or by pd_tick_kernel) against the float64 restatement tests/td3_np.py.  The cases, their tolerances
and what they can see are that module's and tests/test_policy_delay_host.py's: every case's float32 twin stays inside the bounds used
here on the float64 routes, and every planted fault leaves them by more than ten times.

Tolerances: tests/ddpg_opt_np.py's, unchanged -- per vector (the four parameter vectors, m, v) 2^-23 * nb * |theta| + r * |delta_f64| with
r = 5e-5 (tests.helpers.delta_bound), parameters and targets besides at rel 2e-5 of the vector.  Step counts, the count n, the
schedule and every bit identity, exactly."""
import collections
import ctypes

import numpy as np
import pytest

from tests import ddpg_opt_np as R
from tests import td3_np as T3
from tests.helpers import _profiled_calls, hyper_options, make_pair
from tests.test_gpu_hyperparameters import _pair_from_host_case, _params

pytestmark = pytest.mark.gpu
HostBatch = collections.namedtuple("HostBatch", "state_1 action reward terminal_mask state_2")
CPP_ERR_ARG = 1          # include/cartpolepp_abi.h


def _abi():
    from cartpoleplusplus_amd._lib import lib, check, ptr
    return lib, check, ptr


def _state(agent):
    """(m, v as float64 -- zeros under GradientDescent, which has no slots --, [actor's count, critic's count] or None)"""
    if not agent.trainer.has_optimiser_slots():
        n = sum(len(p) for p in _params(agent)[:2])
        return [np.zeros(n), np.zeros(n)], None
    st = agent.trainer.get_optimiser_state()
    return [st["m"].astype(np.float64), st["v"].astype(np.float64)], [int(x) for x in st["step"]]


def _actor_bits(agent):
    """everything a held minibatch must leave alone: the actor's parameters, its share of both slot vectors, its count"""
    slots, steps = _state(agent)
    nA = len(agent.actor.get_params())
    return [agent.actor.get_params(), slots[0][:nA].copy(), slots[1][:nA].copy()], (steps[0] if steps else None)


def _compare(cid, opt, P, got, want, nb):
    bad = []
    for name, g, w, b in zip(T3.VECTORS, got, want, T3.bounds(P, want, nb)):
        if (name == "v" and opt != "adam") or (name == "m" and opt == "gradient-descent"):
            assert not np.asarray(g).any()
            continue
        err = float(np.linalg.norm(np.asarray(g, np.float64) - w))
        print("  %s %-13s |err| %.3e  bound %.3e  (%.2f of it)" % (cid, name, err, b, err / b))
        if not err <= b:
            bad.append((name, err, b))
        if name in T3.VECTORS[:4] and not err <= R.PARAM_REL * float(np.linalg.norm(w)):
            bad.append((name, "rel", err / float(np.linalg.norm(w))))
    assert not bad, (cid, bad)


def _agent(shape_name, hp, opt, delay=None, rows=24, nb=T3.MAX_MINIBATCHES, **kw):
    """host_case's parameters and episodes of the shape on the device; delay: through the command line's option"""
    shape, B, seed = T3.SHAPES[shape_name]
    if delay is not None:
        kw["policy_delay"] = delay
    agent, case = _pair_from_host_case(shape, B, nb, seed, hp, rows=rows, **dict(T3.opt_kw(opt), **kw))
    return agent, B, case


# ---- 1. against the float64 restatement, the caller's rows (the eager launch sequence)
def _ends_held(case):
    _cid, _opt, _sn, d, nb, steps, _clip, _tau = case
    return any((s * nb) % d != 0 for s in range(1, steps + 1))


_OUTER = [(c, "rider") for c in T3.grid()] + [(c, "own-launch") for c in T3.grid() if _ends_held(c)]


@pytest.mark.parametrize("case,targets", _OUTER, ids=["%s-%s" % (c[0], t) for c, t in _OUTER])
def test_outer_steps_against_the_float64_restatement(case, targets):
    """targets = own-launch (the cases with an outer step that ends on a held minibatch): the same minibatches one per call through
    cpp_ddpg_train_rows, the target updates by cpp_ddpg_update_targets behind each outer step"""
    cid, opt, shape_name, d, nb, steps, clip, tau = case
    lib, check, ptr = _abi()
    hp = T3.hyper_of(opt, clip, tau)
    agent, B, (specs, P, _ep, idxs, batches) = _agent(shape_name, hp, opt, d)
    idxs, batches = T3.case_batches(case, idxs, batches, B)
    try:
        assert agent.trainer.policy_delay == d and agent.trainer.policy_delay_status() == (d, 0, False)
        for s in range(steps):
            rows = idxs[s * nb * B:(s + 1) * nb * B]
            if targets == "rider":
                agent.train_step(B, nb, idxs=rows)
            else:
                for k in range(nb):
                    r = np.ascontiguousarray(rows[k * B:(k + 1) * B], dtype=np.int32)
                    check(lib.cpp_ddpg_train_rows(agent.trainer.handle, agent.replay_memory.handle, B, ptr(r)))
                check(lib.cpp_ddpg_update_targets(agent.trainer.handle))
        got, stats = _params(agent), agent.trainer.last_stats()
        slots, counts = _state(agent)
        status = agent.trainer.policy_delay_status()
    finally:
        agent.close()
    want, wcounts, outs, ref = T3.run_case(specs, P, batches, hp, opt, d, nb, steps)
    na, nc = outs[-1]["actor_norm"], outs[-1]["critic_norm"]
    # (the held actor's gradient is still computed, its pre-clip norm still reported)
    assert abs(stats[1] - na) < 1e-4 * max(1.0, na) and abs(stats[2] - nc) < 1e-4 * max(1.0, nc), (stats, na, nc)
    assert status == (d, steps * nb, ref.held), status
    if counts is not None:
        assert counts == [int(x) for x in wcounts] == [steps * nb // d, steps * nb], counts
    _compare(cid + "-" + targets, opt, P, got + slots, want, steps * nb)


def test_a_held_minibatch_still_draws_masks_and_is_counted():
    """--use-dropout under --policy-delay 2, four minibatches in one eager call on a 16x16x6 render at B = 6 (applied at 2 and 4, held at
    1 and 3): the hold reaches the optimiser alone, so minibatch k draws the masks of forward count k in the actor and in the target
    actor, held or not (include/cartpolepp_abi.h, cpp_net_spec.use_dropout; the restatement's DelayedDDPG._draw_masks).  A device that
    skipped the count on held minibatches would draw counts 0, 0, 1, 1 in the actor."""
    from tests.helpers import DROP_B, DROP_PIX, DROP_ROWS, DROP_SEED, LOUD, host_case
    opt, d, nb = "gradient-descent", 2, 4
    agent, (_specs, P, _ep, idxs, batches) = _pair_from_host_case(DROP_PIX, DROP_B, nb, DROP_SEED, LOUD, rows=DROP_ROWS, policy_delay=d,
                                                                  use_dropout=True)
    try:
        agent.train_step(DROP_B, nb, idxs=idxs)
        got, stats = _params(agent), agent.trainer.last_stats()
        slots, _counts = _state(agent)
        status = agent.trainer.policy_delay_status()
    finally:
        agent.close()
    specs = host_case(DROP_PIX, DROP_B, nb, DROP_SEED, rows=DROP_ROWS, dropout=True)[0]          # (the same numbers, an actor spec that asks for masks)
    want, _wc, outs, ref = T3.run_case(specs, P, batches, LOUD, opt, d, nb, 1)
    assert ref.drop_n == {"actor": nb, "target_actor": nb} and [o["applied"] for o in outs] == [False, True, False, True]
    na, nc = outs[-1]["actor_norm"], outs[-1]["critic_norm"]
    assert abs(stats[1] - na) < 1e-4 * max(1.0, na) and abs(stats[2] - nc) < 1e-4 * max(1.0, nc), (stats, na, nc)
    assert status == (d, nb, False), status
    _compare("dropout-d2-1x4", opt, P, got + slots, want, nb)


# ---- 1b / 4. graph replay on the rows the device draws; the first case is "one graph, a schedule that does not divide it"
@pytest.mark.parametrize("case", T3.GRAPH_CASES, ids=[c[0] for c in T3.GRAPH_CASES])
def test_graph_replays_against_the_float64_restatement(case):
    """the first outer step is the eager pass and the capture, the others replay ONE graph; under d = 2 with 5 minibatches the applied
    positions are 2, 4 in the odd outer steps and 1, 3, 5 in the even ones: only a predicate on the device passes this"""
    cid, opt, shape_name, d, nb, steps, sample_seed = case
    lib, check, ptr = _abi()
    hp = T3.hyper_of(opt, T3.GRAPH_CLIP, T3.GRAPH_TAU)
    specs, P, _ep, rows, batches = T3.graph_case(cid)
    agent, B, _case = _agent(shape_name, hp, opt, d, rows=T3.GRAPH_ROWS, nb=1, sample_seed=sample_seed)
    try:
        for _s in range(steps):
            agent.train_step(B, nb)
        last = np.empty(B, np.int32)
        check(lib.cpp_replay_last_indexes(agent.replay_memory.handle, B, ptr(last)))
        got = _params(agent)
        slots, counts = _state(agent)
        status = agent.trainer.policy_delay_status()
    finally:
        agent.close()
    assert np.array_equal(last, rows[-B:]), "the rows of the last minibatch are not the restated draw"
    want, wcounts, _outs, ref = T3.run_case(specs, P, batches, hp, opt, d, nb, steps)
    assert status == (d, steps * nb, ref.held), status
    if counts is not None:
        assert counts == [int(x) for x in wcounts] == [steps * nb // d, steps * nb], counts
    if cid == "adam-16x16x6-d2-4x5":
        assert status[1] == 20 and counts == [10, 20]
        assert ref.schedule[:5] == [False, True, False, True, False] and ref.schedule[5:10] == [True, False, True, False, True]
    _compare(cid, opt, P, got + slots, want, steps * nb)


# ---- 2. held means untouched, to the bit
@pytest.mark.parametrize("opt,shape_name", [("adam", "16x16x6"), ("momentum-0.5", "64x64x18"), ("gradient-descent", "16x16x6")])
def test_a_held_minibatch_leaves_every_bit_of_the_actor(opt, shape_name):
    """one minibatch per call (the target rider rides in every one of them: tau = 0.25), d = 3, six calls"""
    d = 3
    hp = T3.hyper_of(opt, 0.5, 0.25)
    agent, B, (_s, _P, _ep, idxs, _b) = _agent(shape_name, hp, opt, d)
    try:
        for k in range(1, 7):
            before, t0 = _actor_bits(agent)
            c0, ta0 = agent.critic.get_params(), agent.target_actor.get_params()
            agent.train_step(B, 1, idxs=idxs[(k - 1) * B:k * B])
            after, t1 = _actor_bits(agent)
            dd, n, held = agent.trainer.policy_delay_status()
            assert (dd, n, held) == (d, k, k % d != 0), (k, dd, n, held)
            same = [np.array_equal(x, y) for x, y in zip(before, after)]
            used = [True, opt != "gradient-descent", opt == "adam"]
            if held:
                assert all(same), (k, same)
                assert t1 == t0
            else:
                assert not any(s for s, u in zip(same, used) if u), (k, same)
                assert t0 is None or t1 == t0 + 1
            assert not np.array_equal(agent.critic.get_params(), c0)
            assert not np.array_equal(agent.target_actor.get_params(), ta0)      # (the target follows every outer step, from the actor as it is)
            assert agent.trainer.last_stats()[1] > 0
    finally:
        agent.close()


# ---- 3. the critic does not know
@pytest.mark.parametrize("per", [False, True], ids=["uniform", "prioritized"])
def test_the_critic_does_not_know(per):
    """one outer step of three minibatches, d = 3 against a twin with the delay off: the critic's update never reads the live actor, so
    its parameters, slots and count hold the same bits.  uniform: through cpp_ddpg_train_rows, which runs no target update -- the target
    critic is untouched in both; prioritized: through train_step, whose target critic follows the same critic, and whose sum tree
    (the priorities come from the TD values) must not know either"""
    lib, check, ptr = _abi()
    opt, shape, B, rows = "adam", (32, 32, 3, 2, 3), 16, 120
    hp = T3.hyper_of(opt, 0.5, 0.25)
    kw = dict(prioritized_replay=True, priority_alpha=0.6, priority_beta=0.4, priority_eps=1e-6) if per else {}
    out = []
    for delay in (3, 1):
        agent, _ref, _specs = make_pair(shape, B, True, seed=5, replay_size=rows + 40, **dict(hyper_options(hp), **dict(T3.opt_kw(opt), **kw)))
        try:
            agent.replay_memory.fill_synthetic(rows, seed=31)
            if delay > 1:
                agent.trainer.set_policy_delay(delay)
            tc0 = agent.target_critic.get_params()
            if per:
                agent.train_step(B, 3)
                tree = agent.replay_memory.priority_tree()
            else:
                idxs = np.random.default_rng(7).integers(0, rows, 3 * B).astype(np.int32)
                for k in range(3):
                    r = np.ascontiguousarray(idxs[k * B:(k + 1) * B])
                    check(lib.cpp_ddpg_train_rows(agent.trainer.handle, agent.replay_memory.handle, B, ptr(r)))
                assert np.array_equal(agent.target_critic.get_params(), tc0)      # (no target update yet)
                tree = None
            slots, counts = _state(agent)
            nA = len(agent.actor.get_params())
            out.append(dict(critic=agent.critic.get_params(), tcritic=agent.target_critic.get_params(), m=slots[0][nA:], v=slots[1][nA:],
                            count=counts[1], acount=counts[0], actor=agent.actor.get_params(), tree=tree))
        finally:
            agent.close()
    a, b = out
    assert a["count"] == b["count"] == 3 and (a["acount"], b["acount"]) == (1, 3)
    assert not np.array_equal(a["actor"], b["actor"])
    for k in ("critic", "tcritic", "m", "v"):
        assert np.array_equal(a[k], b[k]), k
    if per:
        assert np.array_equal(a["tree"], b["tree"])


# ---- 5. every entry point
def _n(agent):
    return agent.trainer.policy_delay_status()[1:]


def test_every_entry_point_counts_as_specified():
    lib, check, ptr = _abi()
    opt, d = "adam", 2
    hp = T3.hyper_of(opt, 0.5, 0.25)
    agent, B, (_s, _P, _ep, idxs, batches) = _agent("16x16x6", hp, opt, d)
    try:
        t, rm = agent.trainer, agent.replay_memory
        hb = [HostBatch(*[np.asarray(x) for x in b]) for b in batches]
        r0 = np.ascontiguousarray(idxs[:B], dtype=np.int32)
        agent.train_step(B, 3, idxs=idxs[:3 * B])
        assert _n(agent) == (3, True) and _state(agent)[1] == [1, 3]
        check(lib.cpp_ddpg_train_rows(t.handle, rm.handle, B, ptr(r0)))
        assert _n(agent) == (4, False) and _state(agent)[1] == [2, 4]
        # the literal loop, paired through defer_actor: one fused minibatch
        batch = rm.batch(idxs=r0)
        agent.actor.train(batch.state_1)
        agent.critic.train(batch)
        assert t.fused_pairs == 1 and _n(agent) == (5, True) and _state(agent)[1] == [2, 5]
        # ... and unpaired with host arrays: the actor's op looks one ahead and counts nothing, the critic's counts
        a0 = agent.actor.get_params()
        agent.actor.train(hb[0].state_1)
        assert _n(agent) == (5, False) and _state(agent)[1] == [3, 5] and not np.array_equal(agent.actor.get_params(), a0)
        agent.critic.train(hb[0])
        assert _n(agent) == (6, False) and _state(agent)[1] == [3, 6]
        a0 = agent.actor.get_params()
        agent.actor.train(hb[1].state_1)
        assert _n(agent) == (6, True) and _state(agent)[1] == [3, 6] and np.array_equal(agent.actor.get_params(), a0)
        agent.critic.train(hb[1])
        assert _n(agent) == (7, True) and _state(agent)[1] == [3, 7]
        # compute_gradients alone counts nothing; apply_gradients (both lists) counts and applies the predicate
        dev = t.device_batch_for(hb[2])
        check(lib.cpp_ddpg_compute_gradients(t.handle, dev.handle))
        assert _n(agent) == (7, True) and _state(agent)[1] == [3, 7]
        check(lib.cpp_ddpg_apply_gradients(t.handle, 1.0))
        assert _n(agent) == (8, False) and _state(agent)[1] == [4, 8]
        check(lib.cpp_ddpg_compute_gradients(t.handle, dev.handle))
        a0 = agent.actor.get_params()
        check(lib.cpp_ddpg_apply_gradients(t.handle, 1.0))
        assert _n(agent) == (9, True) and _state(agent)[1] == [4, 9] and np.array_equal(agent.actor.get_params(), a0)
        # check_loss and q_gradients_wrt_actions touch nothing
        loss = np.zeros(1, np.float32)
        check(lib.cpp_ddpg_check_loss(t.handle, dev.handle, ptr(loss), None, None))
        check(lib.cpp_ddpg_q_gradients_wrt_actions(t.handle, dev.handle, None, None, None))
        assert _n(agent) == (9, True) and _state(agent)[1] == [4, 9]
        # the data-parallel step as a world of one: one graph, and half steps followed by apply()
        check(lib.cpp_ddpg_dp_train_step(t.handle, rm.handle, None, B, 3, 7, 1, 0))
        assert _n(agent) == (12, False) and _state(agent)[1] == [6, 12]
        check(lib.cpp_ddpg_dp_train_step(t.handle, rm.handle, None, B, 3, 7, 2, 0))
        assert _n(agent) == (15, True) and _state(agent)[1] == [7, 15]
        check(lib.cpp_ddpg_sample_and_compute(t.handle, rm.handle, B, 7))
        assert _n(agent) == (15, True) and _state(agent)[1] == [7, 15]
        # the configuring call zeroes the count
        t.set_policy_delay(3)
        assert t.policy_delay_status() == (3, 0, False)
        for p in _params(agent) + _state(agent)[0]:
            assert np.isfinite(p).all()
    finally:
        agent.close()


@pytest.mark.parametrize("opt", ["gradient-descent", "adam"])
def test_the_unpaired_literal_loop_against_the_float64_restatement(opt):
    """ddpg_cartpole.py:332-337 with host arrays, four minibatches, d = 2 (tests/test_policy_delay_host.py: a counting actor op shows
    here): cpp_ddpg_train_actor, cpp_ddpg_train_critic, both target updates"""
    hp = T3.hyper_of(opt, 0.5, 0.25)
    agent, B, (specs, P, _ep, _idxs, batches) = _agent("16x16x6", hp, opt, 2)
    try:
        for b in batches[:4]:
            hb = HostBatch(*[np.asarray(x) for x in b])
            agent.actor.train(hb.state_1)
            agent.critic.train(hb)
            agent.target_actor.update_weights()
            agent.target_critic.update_weights()
        got = _params(agent)
        slots, counts = _state(agent)
        assert agent.trainer.policy_delay_status() == (2, 4, False)
    finally:
        agent.close()
    want, wcounts, _ref = T3.run_literal(specs, P, batches[:4], hp, opt, 2)
    if counts is not None:
        assert counts == [int(x) for x in wcounts] == [2, 4]
    _compare("literal-" + opt, opt, P, got + slots, want, 4)


@pytest.mark.parametrize("shape_name", ["16x16x6", "64x64x18"])
def test_the_paired_literal_loop_is_the_fused_step_bit_for_bit(shape_name):
    """one minibatch per outer step, as tests/test_gpu_literal_loop.py holds the plain step: actor.train(batch.state_1); critic.train(batch)
    against train_step(B, 1, idxs) on the same rows, d = 2, four outer steps"""
    hp = T3.hyper_of("adam", 0.5, 0.25)
    lit, B, _c = _agent(shape_name, hp, "adam", 2, rows=60)
    fused, _B, _c2 = _agent(shape_name, hp, "adam", 2, rows=60)
    try:
        np.random.seed(99)
        for step in range(1, 5):
            batch = lit.replay_memory.batch(B)
            lit.actor.train(batch.state_1)
            lit.critic.train(batch)
            lit.target_actor.update_weights()
            lit.target_critic.update_weights()
            fused.train_step(B, 1, idxs=batch.idxs)
            for a, b in zip(_params(lit), _params(fused)):
                assert np.array_equal(a, b), step
            assert lit.trainer.policy_delay_status() == fused.trainer.policy_delay_status() == (2, step, step % 2 != 0)
        assert lit.trainer.fused_pairs == 4
        (sl, tl), (sf, tf) = _state(lit), _state(fused)
        assert tl == tf == [2, 4] and np.array_equal(sl[0], sf[0]) and np.array_equal(sl[1], sf[1])
    finally:
        lit.close(); fused.close()


# ---- 6. off means off
@pytest.mark.parametrize("shape_name", ["16x16x6", "64x64x18"])
def test_switched_off_is_a_trainer_that_never_had_it(shape_name):
    """both twins run the same prelude (an eager outer step and a device-drawn one), one of them under d = 3; then the delay is set back
    to 1, both start over from the same parameters and zeroed slots, and run an eager outer step and three graph replays"""
    hp = T3.hyper_of("adam", 0.5, 0.25)
    runs = []
    for was_on in (True, False):
        agent, B, (_s, P, _ep, idxs, _b) = _agent(shape_name, hp, "adam", rows=60)
        try:
            if was_on:
                agent.trainer.set_policy_delay(3)
            agent.train_step(B, 2, idxs=idxs[:2 * B])
            agent.train_step(B, 2)
            if was_on:
                assert agent.trainer.policy_delay_status() == (3, 4, True) and _state(agent)[1] == [1, 4]
                agent.trainer.set_policy_delay(1)
                assert agent.trainer.policy_delay_status() == (1, 0, False)
            for net, p in zip(agent.networks(), P):
                net.set_params(p)
            n = len(P[0]) + len(P[1])
            agent.trainer.set_optimiser_state({"m": np.zeros(n, np.float32), "v": np.zeros(n, np.float32), "step": np.zeros(2, np.uint64)})
            agent.train_step(B, 3, idxs=idxs[:3 * B])
            for _ in range(3):
                agent.train_step(B, 2)
            slots, counts = _state(agent)
            assert counts == [9, 9]
            runs.append(np.concatenate(_params(agent) + slots))
        finally:
            agent.close()
    assert np.isfinite(runs[0]).all() and np.array_equal(runs[0], runs[1])


def test_the_launch_census_of_an_outer_step():
    """one profiled outer step of three minibatches at 64x64x18 (the heads path, the statistics, image and target riders): the same
    launches with the delay never configured, set to 1 and set to 2 -- the hold costs the fused path no launch; on the stand-alone ops
    d = 2 adds exactly the tick launch in place of the two counter launches"""
    hp = T3.hyper_of("adam", 0.5, 0.25)
    census = {}
    for name, delay in (("off", None), ("d=1", 1), ("d=2", 2)):
        agent, B, (_s, _P, _ep, idxs, _b) = _agent("64x64x18", hp, "adam")
        try:
            assert agent.trainer.policy_delay == 1      # (the trainer exists before the profile starts: its creation launches a fill)
            if delay is not None:
                agent.trainer.set_policy_delay(delay)
            census[name] = _profiled_calls(agent.actor.ctx, lambda: agent.train_step(B, 3, idxs=idxs[:3 * B]))
        finally:
            agent.close()
    print("launches per outer step:", census)
    assert census["off"] == census["d=1"] == census["d=2"], census
    assert census["off"].get("heads", 0) == 3 and census["off"].get("clip_sgd", 0) == 3, census


# ---- 7. TD3 minus the twin critics: smoothing + Adam + d = 2 against the composed restatement
SMOOTHING = (0.5, 0.5, 0x5EEDF00D12345)


def test_smoothing_adam_and_the_delay_together():
    """three minibatches on the caller's rows (held, applied, held): the noise of the last pass at tps_np.Z_BAR * sigma, its TD at
    tps_np.td_bar, the six vectors at the plain bounds"""
    from tests import tps_np as T
    opt, d, nb = "adam", 2, 3
    hp = T3.hyper_of(opt, 0.5, 0.25)
    agent, B, (specs, P, _ep, idxs, batches) = _agent("16x16x6", hp, opt, d, target_policy_noise=SMOOTHING[0],
                                                      target_policy_noise_clip=SMOOTHING[1], target_policy_noise_seed=SMOOTHING[2])
    try:
        agent.train_step(B, nb, idxs=idxs[:nb * B])
        got = _params(agent)
        slots, counts = _state(agent)
        eps, n_noise = agent.trainer.last_target_noise(B)
        _a, _dq, _q, td = agent.trainer.last_values(B)
        status = agent.trainer.policy_delay_status()
    finally:
        agent.close()
    want, wcounts, outs, ref = T3.run_case(specs, P, batches, hp, opt, d, nb, 1, smoothing=SMOOTHING)
    plain, _c, _o, _r = T3.run_case(specs, P, batches, hp, opt, d, nb, 1)
    assert status == (d, nb, True) and counts == [int(x) for x in wcounts] == [1, 3] and n_noise == nb - 1 and ref.tps_n == nb
    want_eps = T.target_noise(SMOOTHING[2], nb - 1, B, eps.shape[1], SMOOTHING[0], SMOOTHING[1])
    assert float(np.abs(eps - want_eps).max()) <= T.Z_BAR * SMOOTHING[0]
    bar = T.td_bar(hp.discount, SMOOTHING[0], outs[-1]["target_dq_da"])
    err_td = float(np.abs(td - outs[-1]["td"]).max())
    print("  TD of the last minibatch: |err| %.3e, smoothing's bar %.3e" % (err_td, bar))
    assert err_td < bar
    assert float(np.linalg.norm(want[1] - plain[1])) > 100 * T3.bounds(P, want, nb)[1]      # (the smoothing is in the numbers compared)
    _compare("td3-minus-twin-critics", opt, P, got + slots, want, nb)


def _rows(agent, B):
    lib, check, ptr = _abi()
    rows = np.empty(B, np.int32)
    check(lib.cpp_replay_last_indexes(agent.replay_memory.handle, B, ptr(rows)))
    return rows


def _one_replay_feature(what, prepare, shift=False):
    """smoothing + Adam + d = 2 with a replay feature on, one minibatch per call on device-drawn rows: two warm calls (n = 2), then a HELD
    minibatch (n = 3) and an APPLIED one (n = 4), each rebuilt on the host as tests/test_gpu_ddpg_optimisers.py rebuilds its checked
    minibatch -- the rows read back, the feature's own restatement of the minibatch, the float64 oracle's gradients on the device's
    routes with the restated noise of the count the device reports, tests/ddpg_opt_np.py's rule from the device's slots and counts as
    they stood before the call: applied to the critic's list always, to the actor's only when n' % d == 0 (held: every bit kept).
    The float32 evaluation of the same update must itself sit inside the bound (else the case is void, not the device wrong)."""
    from oracle import ddpg_np as O
    from tests import tps_np as T
    from tests.helpers import delta_bound, device_pool_codes, device_relu_active
    from tests.test_gpu_random_shift import _shifted_minibatch
    opt, d, shape, B, rows, seed = "adam", 2, (32, 32, 3, 2, 3), 32, 300, 4
    hp = T3.hyper_of(opt, 0.5, 0.25)
    agent, _ref, (aspec, cspec) = make_pair(shape, B, True, seed=seed, replay_size=rows + 50, policy_delay=d,
                                            target_policy_noise=SMOOTHING[0], target_policy_noise_clip=SMOOTHING[1],
                                            target_policy_noise_seed=SMOOTHING[2], **dict(hyper_options(hp), **T3.opt_kw(opt)))
    checked = []
    try:
        rm = agent.replay_memory
        rm.fill_synthetic(rows, seed=21 + seed)
        prepare(agent)
        agent.train_step(B, 1)
        agent.train_step(B, 1)
        for k in (3, 4):
            P = _params(agent)
            S0, t0 = _state(agent)
            agent.train_step(B, 1)
            idxs = _rows(agent, B)
            eps, n_noise = agent.trainer.last_target_noise(B)
            codes = (device_pool_codes(agent.actor, B), device_pool_codes(agent.critic, B))
            relus = (device_relu_active(agent.actor, B), device_relu_active(agent.critic, B))
            if shift:
                t, _un, _sh = _shifted_minibatch(rm, idxs)
            else:
                hb = rm.batch(idxs=idxs)
                t = (rm.state[hb.state_1_idx], hb.action, hb.reward, hb.terminal_mask, rm.state[hb.state_2_idx])
            S1, t1 = _state(agent)
            assert agent.trainer.policy_delay_status() == (d, k, k % d != 0) and n_noise == k - 1
            checked.append((k, P, S0, t0, _params(agent), S1, t1, t, eps, codes, relus))
    finally:
        agent.close()
    name, args = T3.OPTIMISERS[opt]
    for k, P, S0, t0, got, S1, t1, t, eps, codes, relus in checked:
        applied = k % d == 0
        nA = len(P[0])
        assert t1 == [t0[0] + int(applied), t0[1] + 1], (k, t0, t1)
        if not applied:
            assert np.array_equal(got[0], P[0]) and np.array_equal(S1[0][:nA], S0[0][:nA]) and np.array_equal(S1[1][:nA], S0[1][:nA]), what
        noise = T.target_noise(SMOOTHING[2], k - 1, B, eps.shape[1], SMOOTHING[0], SMOOTHING[1])
        assert float(np.abs(eps - noise).max()) <= T.Z_BAR * SMOOTHING[0]
        upd = {}
        for dt in (np.float64, np.float32):
            ref = T.SmoothedDDPG(aspec, cspec, P[0], P[1], dt, hyper=hp)
            ref.set_targets(P[2], P[3])
            ref.actor.amax_override, ref.critic.amax_override = codes
            ref.actor.relu_override, ref.critic.relu_override = relus
            ga = ref.actor_gradients(t[0])["grads"]
            gc = ref.critic_gradients(t, noise)["grads"]
            vec = []
            for which, flat, g, sl in (("actor", P[0], ga, slice(0, nA)), ("critic", P[1], gc, slice(nA, None))):
                sl_ = R.Slots(0, dt)
                sl_.m, sl_.v, sl_.t = S0[0][sl].astype(dt), S0[1][sl].astype(dt), t0[0 if which == "actor" else 1]
                new = flat.astype(dt)
                if which == "critic" or applied:
                    o = R.N.make_optimiser(name, dict(args, learning_rate=getattr(hp, which + "_lr")))
                    new, _norm = R.apply_rule(o, new, g, hp.gradient_clip, sl_, dt)
                vec.append((np.asarray(new, np.float64), np.asarray(sl_.m, np.float64), np.asarray(sl_.v, np.float64)))
            upd[dt] = [vec[0][0], vec[1][0], np.concatenate([vec[0][1], vec[1][1]]), np.concatenate([vec[0][2], vec[1][2]])]
        want, twin = upd[np.float64], upd[np.float32]
        bad = []
        for nm, g, w_, tw, p in zip(("actor", "critic", "m", "v"), [got[0], got[1], S1[0], S1[1]], want, twin, [P[0], P[1], S0[0], S0[1]]):
            bound = delta_bound(p, w_ - p, R.R[nm], 1)
            e_twin, err = float(np.linalg.norm(tw - w_)), float(np.linalg.norm(np.asarray(g, np.float64) - w_))
            print("  %s n=%d (%s) %-7s |err| %.3e  twin %.3e  bound %.3e" % (what, k, "applied" if applied else "held", nm, err, e_twin, bound))
            assert e_twin <= bound, "the float32 evaluation of this update leaves the bound itself: the case is void (%s %s)" % (what, nm)
            if not err <= bound:
                bad.append((nm, err, bound))
        assert not bad, (what, k, bad)
        # the targets: the soft update of the parameters the device holds -- the held actor's too --, to f32 rounding
        for j in (0, 1):
            wt = O.soft_update(P[2 + j], got[j], hp.target_update_rate, np.float64)
            assert float(np.linalg.norm(got[2 + j] - wt)) <= 2.0 ** -23 * float(np.linalg.norm(wt)), (what, "target", j)
        if not applied:
            assert not np.array_equal(got[2], P[2])


def test_with_n_step_returns():
    from cartpoleplusplus_amd import ddpg_cartpole as D
    _one_replay_feature("n-step", lambda a: a.replay_memory.enable_n_step(3, D.opts.discount))


def test_with_random_shift():
    _one_replay_feature("random-shift", lambda a: a.replay_memory.enable_random_shift(4, seed=11), shift=True)


# ---- 8. three identical runs
@pytest.mark.parametrize("opt", ["gradient-descent", "momentum-0.5", "adam"])
def test_three_identical_runs_give_identical_bits(opt):
    """idxs=None at 64x64x18: the eager pass, the capture and the replays, 5 minibatches under d = 2 -- the count lives on the device, so
    a replayed graph advances it"""
    hp = T3.hyper_of(opt, 0.5, 0.25)
    runs = []
    for _ in range(3):
        agent, B, _case = _agent("64x64x18", hp, opt, 2, rows=60, nb=1)
        try:
            for _k in range(3):
                agent.train_step(B, 5)
            slots, counts = _state(agent)
            assert agent.trainer.policy_delay_status() == (2, 15, True) and (counts is None or counts == [7, 15])
            runs.append(np.concatenate(_params(agent) + slots))
        finally:
            agent.close()
    assert np.isfinite(runs[0]).all()
    assert np.array_equal(runs[0], runs[1]) and np.array_equal(runs[0], runs[2])


# ---- 9. refusals through the raw ABI
def test_refusals_through_the_abi():
    lib, check, ptr = _abi()
    hp = T3.hyper_of("adam", 0.5, 0.25)
    agent, _B, _case = _agent("16x16x6", hp, "gradient-descent")
    try:
        h = agent.trainer.handle
        lib.cpp_last_error.restype = ctypes.c_char_p
        for bad in (0, -1, 65537):
            assert lib.cpp_ddpg_set_policy_delay(h, bad) == CPP_ERR_ARG, bad
            assert b"cpp_ddpg_set_policy_delay" in lib.cpp_last_error()
            assert agent.trainer.policy_delay_status() == (1, 0, False)
        assert lib.cpp_ddpg_set_policy_delay(None, 2) == CPP_ERR_ARG and b"cpp_ddpg_set_policy_delay" in lib.cpp_last_error()
        assert lib.cpp_ddpg_policy_delay_status(None, None, None, None) == CPP_ERR_ARG
        assert b"cpp_ddpg_policy_delay_status" in lib.cpp_last_error()
        check(lib.cpp_ddpg_set_policy_delay(h, 65536))
        assert agent.trainer.policy_delay_status() == (65536, 0, False)
        check(lib.cpp_ddpg_policy_delay_status(h, None, None, None))
    finally:
        agent.close()
