"""The quantile critic on the device (--quantile-critic; cpp_net_create_quantile: csrc/quant.hip on the GEMM levels of the gradient pass)
against the float64 restatement tests/quant_np.py.  The cases, their bars and what they can see are that module's and
tests/test_quantile_host.py's: every case puts at least a tenth of its pairs on either Huber branch, its float32 evaluation stays inside
the bounds used here on the float64 routes, no route is closer to a tie than float32 can decide, and every planted fault leaves a bar by
more than ten times.

Bars: theta, the sorted theta', y, Q, td and dQ/da at tests.quant_np.bar(...) -- the float32 restatement's worst error against float64
times 8, which is below the suite's 1e-5 for every one of them, so each is 1e-5 --, actions at 1e-5, both pre-clip gradient lists at rel
2e-5, the loss at 1e-5 relative; per vector (the four parameter vectors, m, v) tests/ddpg_opt_np.py's 2^-23 * nb * |theta| +
r * |delta_f64| with r = 5e-5, parameters and targets besides at rel 2e-5 of the vector.  With smoothing the restatement is fed the
device's own noise, which is held to the restated draw at tests.tps_np.Z_BAR * sigma."""
import collections
import ctypes
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import ddpg_opt_np as R
from tests import quant_np as W
from tests import td3_np as T3
from tests import tps_np as T
from tests.helpers import FakeEnv, _profiled_calls, assert_flat_close, hyper_options, make_opts, set_actor_masks

pytestmark = pytest.mark.gpu
CPP_ERR_ARG, CPP_ERR_STATE = 1, 3          # include/cartpolepp_abi.h
HostBatch = collections.namedtuple("HostBatch", "state_1 action reward terminal_mask state_2")
PER_KW = dict(prioritized_replay=True, priority_alpha=0.6, priority_beta=0.4, priority_eps=1e-6)


def _abi():
    from cartpoleplusplus_amd._lib import lib, check, ptr
    return lib, check, ptr


def _build(shape, B, A, hp, quant, P=None, episodes=None, rows=W.ROWS, seed=1, capacity=None, **kw):
    """a device agent (quantile critics unless quant is None; quant: (N, kappa, drop_top)) holding the case's parameters and episodes;
    capacity: the batch size it is built with (None: B)"""
    from cartpoleplusplus_amd import ddpg_cartpole as D
    pixel = len(shape) == 5
    if quant is not None:
        kw = dict(kw, quantile_critic=True, num_quantiles=quant[0], quantile_huber_kappa=quant[1], drop_top_quantiles=quant[2])
    make_opts(D, shape, B if capacity is None else int(capacity), pixel, replay_memory_size=rows, **dict(hyper_options(hp), **kw))
    agent = D.DeepDeterministicPolicyGradientAgent(FakeEnv(shape, A))
    try:
        agent.initialise_variables(seed=seed)
        agent.post_var_init_setup()
        if P is not None:
            for net, p in zip(agent.networks(), P):
                assert net.get_params().shape == p.shape, (net.namespace, net.get_params().shape, p.shape)
                net.set_params(p)
        for ep in episodes or ():
            agent.replay_memory.add_episode(*ep)
    except Exception:
        agent.close()
        raise
    return agent


def _case_kw(case):
    kw = dict(T3.opt_kw(case[8]))
    if case[9] > 1:
        kw["policy_delay"] = case[9]
    if case[10] is not None:
        sm = case[10]
        kw.update(target_policy_noise=sm[0], target_policy_noise_clip=sm[1], target_policy_noise_seed=sm[2])
    if case[13] > 1:
        kw["n_step"] = case[13]
    if "weighted" in case[0]:
        kw.update(PER_KW)
    return kw


def _case_agent(case, inputs, quant="case", **kw):
    specs, P, episodes, _idxs, _b = inputs
    return _build(W.SHAPES[case[1]], case[3], case[2], W.hyper_of(case), W.quant_of(case) if quant == "case" else quant, P, episodes,
                  **dict(_case_kw(case), **kw))


def _params(agent):
    return [n.get_params() for n in agent.networks()]


def _slots(agent):
    if not agent.trainer.has_optimiser_slots():
        n = sum(len(p) for p in _params(agent)[:2])
        return [np.zeros(n), np.zeros(n)], None
    st = agent.trainer.get_optimiser_state()
    return [st["m"].astype(np.float64), st["v"].astype(np.float64)], [int(x) for x in st["step"]]


def _compare(cid, opt, P, got, want, nb):
    bad = []
    for name, g, w, b in zip(T3.VECTORS, got, want, W.bounds(P, want, nb)):
        if (name == "v" and opt != "adam") or (name == "m" and opt == "gradient-descent"):
            assert not np.asarray(g).any()
            continue
        assert np.asarray(g).shape == w.shape, (name, np.asarray(g).shape, w.shape)
        err = float(np.linalg.norm(np.asarray(g, np.float64) - w))
        print("  %s %-13s |err| %.3e  bound %.3e  (%.2f of it)" % (cid, name, err, b, err / b))
        if not err <= b:
            bad.append((name, err, b))
        if name in T3.VECTORS[:4] and not err <= R.PARAM_REL * float(np.linalg.norm(w)):
            bad.append((name, "rel", err / float(np.linalg.norm(w))))
    assert not bad, (cid, bad)


def _set_priorities(agent):
    agent.replay_memory.update_priorities(np.arange(W.ROWS), np.random.default_rng(9).lognormal(0.0, 1.0, W.ROWS).astype(np.float32))


def _device_noise(agent, case, B, n):
    """the clipped noise of the last target-forming pass, held to the restated draw number n; None without smoothing"""
    if case[10] is None:
        return None
    sigma, clip, seed = case[10]
    eps, count = agent.trainer.last_target_noise(B)
    assert count == n, (count, n)
    want = T.target_noise(seed, n, B, case[2], sigma, clip, np.float64)
    assert np.abs(eps - want).max() <= T.Z_BAR * sigma, float(np.abs(eps - want).max())
    return eps.astype(np.float64)


def _row_errors(dev, cg, ag=None):
    """|device - restatement| of what job (b) leaves, and of job (a)'s chain where ag is given"""
    actions, dq_da, q, td, theta, srt, y = dev
    err = {"q": np.abs(q - cg["q"]).max(), "td": np.abs(td - cg["td"]).max(), "theta": np.abs(theta - cg["theta"]).max(),
           "sorted": np.abs(srt - cg["sorted"]).max(), "y": np.abs(y - cg["y"]).max()}
    if ag is not None:
        err.update(actions=np.abs(actions - ag["actions"]).max(), dq_da=np.abs(dq_da - ag["dq_da"]).max())
    return {k: float(v) for k, v in err.items()}


def _assert_rows(err):
    for k, v in err.items():
        assert v < (W.ATOL if k == "actions" else W.bar(k)), (k, err)


# ---- 1. one minibatch: the atoms, the sorted and truncated targets, every per-row value, the loss, both gradient sets
@pytest.mark.parametrize("cid", [c[0] for c in W.CASES])
def test_one_minibatch_against_the_float64_restatement(cid):
    _one_minibatch(cid)


def test_a_minibatch_with_dropout_against_the_float64_restatement():
    """--use-dropout under the quantile critic (quant.hip behind the GEMM levels), forward count 1: the actor and the target actor draw masks, the backward takes the GEMM x2 epilogue"""
    _one_minibatch("A2-B8-N25-d0-sgd", use_dropout=True, warm=1, launches={"quant": 2, "heads": 0, "td": 0})


def _one_minibatch(cid, use_dropout=False, warm=0, launches=None, capacity=None):
    """use_dropout: --use-dropout, the restatement's actor and target actor drawing the masks of forward count `warm` -- `warm` training
    calls on the same rows run first and the parameters are put back behind them (plain gradient descent only: no slots, no noise count).
    launches: {kernel family: count} the checked minibatch, profiled, must show.  capacity=C > B: the agent is built for C rows and a
    C-row minibatch (the last C of the case's rows) runs first, then one warm call at B; behind the checked minibatch the parameters
    are put back once more and the C-row minibatch is held to the restatement at the same bars."""
    case = W.case_of(cid)
    A, B, N, drop, opt, d, sm = case[2], case[3], case[4], case[5], case[8], case[9], case[10]
    inputs = W.case_inputs(case, **(dict(dropout=True) if use_dropout else {}))
    specs, P, episodes, idxs, batches = inputs
    weighted = "weighted" in cid
    big = None
    if capacity is not None:
        assert capacity > B and len(idxs) >= capacity
        big, warm = np.ascontiguousarray(idxs[-capacity:], dtype=np.int32), max(warm, 1)
    assert warm == 0 or (opt == "gradient-descent" and sm is None and d == 1 and not weighted and case[13] == 1)
    agent = _case_agent(case, inputs, capacity=capacity, **(dict(use_dropout=True) if use_dropout else {}))
    forwards = 0

    def put_back():
        for net, p in zip(agent.networks(), P):
            net.set_params(p)

    def read(Bx, weighted):
        return {"rows": tuple(agent.trainer.last_values(Bx)) + tuple(agent.trainer.last_quantiles(Bx)), "stats": agent.trainer.last_stats(),
                "grads": (agent.actor.get_grads(), agent.critic.get_grads()), "forwards": forwards - 1,
                "w": agent.replay_memory.last_weights(Bx).astype(np.float64).reshape(Bx, 1) if weighted else None,
                "noise": _device_noise(agent, case, Bx, 0)}
    try:
        if weighted:
            _set_priorities(agent)
        if big is not None:
            agent.train_step(capacity, 1, idxs=big)
            forwards += 1
        for _ in range(warm):
            agent.train_step(B, 1, idxs=idxs[:B])
            forwards += 1
        if warm:
            put_back()
        seen = _profiled_calls(agent.actor.ctx, lambda: agent.train_step(B, 1, idxs=idxs[:B])) if launches is not None else \
            agent.train_step(B, 1, idxs=idxs[:B])
        forwards += 1
        if launches is not None:
            assert {k: seen.get(k, 0) for k in launches} == launches, seen
        dev = read(B, weighted)
        back = None
        if big is not None:
            put_back()
            agent.train_step(capacity, 1, idxs=big)
            forwards += 1
            back = read(capacity, False)
        n_q, n_atoms = ctypes.c_int(-1), ctypes.c_int(-1)
        lib, check, _ptr = _abi()
        check(lib.cpp_net_quantile_info(agent.critic.handle, ctypes.byref(n_q)))
        check(lib.cpp_net_distribution_info(agent.critic.handle, ctypes.byref(n_atoms), None, None))
        assert (n_q.value, n_atoms.value) == (N, 0)          # (a quantile network has no support)
        check(lib.cpp_net_quantile_info(agent.actor.handle, ctypes.byref(n_q)))
        assert n_q.value == 0 and agent.trainer.quantile_target == (float(np.float32(case[6])), drop)
    finally:
        agent.close()
    _check_minibatch(cid, case, specs, P, dev, batches[0], weighted)
    if back is not None:
        from tests.helpers import minibatch_of_rows
        _check_minibatch(cid + " back at capacity %d" % capacity, case, specs, P, back,
                         minibatch_of_rows(W.ROWS, W.SHAPES[case[1]], A, episodes, big), False)


def _check_minibatch(cid, case, specs, P, got, batch, weighted):
    """what _one_minibatch read back from one minibatch against the float64 restatement on `batch` from the parameters P"""
    N, drop, opt, d, sm = case[4], case[5], case[8], case[9], case[10]
    B = int(np.asarray(batch[1]).shape[0])
    dev, stats, (g_a, g_c), w, noise = got["rows"], got["stats"], got["grads"], got["w"], got["noise"]
    ref = W.restatement(specs, P, W.quant_of(case), np.float64, W.hyper_of(case), opt, d, sm)
    set_actor_masks(ref, B, got["forwards"])
    ag = ref.actor_gradients(batch[0])
    cg = ref.critic_gradients(batch, noise=noise, w=w)
    if weighted:
        assert w.min() < 0.9 and abs(w.max() - 1.0) < 1e-6, w.ravel()
    err = _row_errors(dev, cg, ag)
    err["loss"] = abs(float(stats[0]) - float(cg["loss"])) / max(1.0, abs(float(cg["loss"])))
    print("%s: %s" % (cid, {k: "%.2e" % v for k, v in err.items()}))
    theta, srt, y = dev[4:]
    assert theta.shape == srt.shape == y.shape == (B, N)
    assert err.pop("loss") < W.ATOL, err
    _assert_rows(err)
    assert (np.diff(srt, axis=1) >= 0).all() and not y[:, N - drop:].any()          # ascending; the dropped columns are zero
    assert np.array_equal(np.sort(srt, axis=1), srt) and np.abs(np.sort(cg["target_theta"], axis=1) - srt).max() < W.bar("sorted")
    assert_flat_close(specs[0], g_a, ag["grads"], rel=W.GRAD_REL, what="actor pre-clip grads vs f64 restatement")
    assert len(g_c) == specs[1].num_params()
    assert_flat_close(specs[1], g_c, cg["grads"], rel=W.GRAD_REL, what="critic pre-clip grads vs f64 restatement")


def test_a_minibatch_below_the_capacity_against_the_float64_restatement():
    """(C, B) = (8, 5), two top quantiles dropped: the atoms, the sorted and truncated targets and the loss partials at B behind a C-row
    minibatch, and back"""
    _one_minibatch("A2-B5-N33-d2", capacity=8)


# ---- 2. the cases' outer steps: parameters, targets, slots, counts
def _run_outer(case, inputs, **kw):
    cid, B = case[0], case[3]
    nb, steps = W.structure(case)
    idxs = inputs[3]
    weighted = "weighted" in cid
    agent = _case_agent(case, inputs, **kw)
    weights = []
    try:
        if weighted:
            _set_priorities(agent)
        for s in range(steps):
            agent.train_step(B, nb, idxs=idxs[s * nb * B:(s + 1) * nb * B])
            if weighted:
                weights.append(agent.replay_memory.last_weights(B).astype(np.float64).reshape(B, 1))
        got, stats = _params(agent), agent.trainer.last_stats()
        slots, counts = _slots(agent)
    finally:
        agent.close()
    return got, slots, counts, stats, weights or None


@pytest.mark.parametrize("cid", [c[0] for c in W.CASES])
def test_outer_steps_against_the_float64_restatement(cid):
    case = W.case_of(cid)
    opt, d = case[8], case[9]
    inputs = W.case_inputs(case)
    got, slots, counts, stats, weights = _run_outer(case, inputs)
    want, wcounts, outs, _ref = W.run_case(case, inputs, weights=weights)
    na, nc = outs[-1]["actor_norm"], outs[-1]["critic_norm"]
    assert abs(stats[1] - na) < 1e-4 * max(1.0, na) and abs(stats[2] - nc) < 1e-4 * max(1.0, nc), (stats, na, nc)
    assert abs(stats[0] - outs[-1]["loss"]) < 1e-4 * max(1.0, outs[-1]["loss"]), (stats, outs[-1]["loss"])
    if counts is not None:
        assert counts == [int(x) for x in wcounts] == [W.NB // d, W.NB], counts
    _compare(cid, opt, inputs[1], got + slots, want, W.NB)


def test_priorities_come_from_the_truncated_targets_td():
    """a prioritized memory's leaves behind a quantile minibatch are (|td| + eps)^alpha with td = Q - mean_{j<M} y_j (the weighted
    instance of job (b))"""
    case = W.case_of("A2-B5-N33-d2-weighted")
    B, N, drop = case[3], case[4], case[5]
    inputs = W.case_inputs(case)
    specs, P, _ep, _idxs, batches = inputs
    lib, check, ptr = _abi()
    agent = _case_agent(case, inputs)
    try:
        _set_priorities(agent)
        rows = np.ascontiguousarray(inputs[3][:B], dtype=np.int32)
        agent.train_step(B, 1, idxs=rows)
        q, td = [x.ravel().astype(np.float64) for x in agent.trainer.last_values(B)[2:]]
        y = agent.trainer.last_quantiles(B)[2].astype(np.float64)
        pri = np.empty(B, np.float32)
        check(lib.cpp_replay_read_priorities(agent.replay_memory.handle, ptr(rows), B, ptr(pri)))
        w = agent.replay_memory.last_weights(B).astype(np.float64).reshape(B, 1)
    finally:
        agent.close()
    ref = W.restatement(specs, P, W.quant_of(case), np.float64, W.hyper_of(case))
    cg = ref.critic_gradients(batches[0], w=w)
    assert np.abs(td - cg["td"].ravel()).max() < W.bar("td")
    assert np.abs(td - (q - y[:, :N - drop].mean(axis=1))).max() < 2 * W.ATOL          # (the device's own figures: the mean of the KEPT targets)
    full = W.restatement(specs, P, (N, case[6], 0), np.float64, W.hyper_of(case)).critic_gradients(batches[0], w=w)
    assert np.abs(td - full["td"].ravel()).max() > 100 * W.bar("td")                 # (not the untruncated one)
    want = (np.abs(td) + 1e-6) ** 0.6
    # (a row drawn twice keeps the value of one of its occurrences)
    ok = [any(abs(pri[i] - want[j]) <= 1e-5 * max(1.0, want[j]) for j in range(B) if rows[j] == rows[i]) for i in range(B)]
    assert all(ok), (pri, want)
    assert np.abs(td).min() > 1e-3 and np.ptp(want) > 1e-2


# ---- 3. graph replays on the rows the device draws; the same bits eager, replayed, paired and repeated
def _graph_agent(**kw):
    case, _nb, _steps, sample_seed = W.GRAPH_CASE
    return _case_agent(case, W.graph_inputs(), sample_seed=sample_seed, **kw)


def _state(agent, B):
    return _params(agent) + _slots(agent)[0] + list(agent.trainer.last_quantiles(B)) + list(agent.trainer.last_values(B)) + \
        [np.asarray(agent.trainer.last_stats())]


def test_graph_replays_against_the_float64_restatement():
    """four outer steps of three minibatches (n-step rows, smoothing, --policy-delay 2, Adam): the eager pass and the capture, then three
    replays of one graph"""
    case, nb, steps, _ss = W.GRAPH_CASE
    cid, B, opt, d = case[0], case[3], case[8], case[9]
    lib, check, ptr = _abi()
    inputs = W.graph_inputs()
    agent = _graph_agent()
    try:
        for _s in range(steps):
            agent.train_step(B, nb)
        last = np.empty(B, np.int32)
        check(lib.cpp_replay_last_indexes(agent.replay_memory.handle, B, ptr(last)))
        got = _params(agent)
        slots, counts = _slots(agent)
        status = agent.trainer.policy_delay_status()
        _eps, n_noise = agent.trainer.last_target_noise(B)
    finally:
        agent.close()
    assert np.array_equal(last, inputs[3][-B:]), "the rows of the last minibatch are not the restated draw"
    want, wcounts, _outs, ref = W.run_case(case, inputs, nb=nb, steps=steps)
    assert status == (d, steps * nb, ref.held) and n_noise == steps * nb - 1
    assert counts == [int(x) for x in wcounts] == [steps * nb // d, steps * nb], counts
    _compare(cid, opt, inputs[1], got + slots, want, steps * nb)


def test_eager_runs_graph_replays_and_repeated_runs_are_bit_identical():
    """train_step on the device's draws (the eager pass and the capture, then replays) twice, and on the same rows handed in (eager
    launches throughout): one set of bits"""
    case, nb, _steps, _ss = W.GRAPH_CASE
    B = case[3]
    rows = W.graph_inputs()[3]
    runs = []
    for mode in ("graph", "graph", "eager"):
        agent = _graph_agent()
        try:
            for s in range(3):
                if mode == "graph":
                    agent.train_step(B, nb)
                else:
                    agent.train_step(B, nb, idxs=rows[s * nb * B:(s + 1) * nb * B])
            runs.append(_state(agent, B))
        finally:
            agent.close()
    for k, other in enumerate(runs[1:]):
        for i, (x, y) in enumerate(zip(runs[0], other)):
            assert np.array_equal(x, y), ("run", k + 1, "item", i)


def test_the_paired_literal_loop_is_the_fused_step_bit_for_bit():
    """actor.train(batch.state_1); critic.train(batch) on device-resident batches run as ONE cpp_ddpg_train_rows, both target updates
    behind them -- against train_step(B, 1, idxs) on the same rows, per minibatch, to the bit"""
    case, _nb, _steps, _ss = W.GRAPH_CASE
    B, d = case[3], case[9]
    lit, fused = _graph_agent(), _graph_agent()
    try:
        np.random.seed(99)
        for step in range(1, 5):
            batch = lit.replay_memory.batch(B)
            lit.actor.train(batch.state_1)
            lit.critic.train(batch)
            lit.target_actor.update_weights()
            lit.target_critic.update_weights()
            assert batch._states is None, "a state column crossed PCIe"
            fused.train_step(B, 1, idxs=batch.idxs)
            for i, (a, b) in enumerate(zip(_state(lit, B), _state(fused, B))):
                assert np.array_equal(a, b), (step, i)
            assert lit.trainer.policy_delay_status() == fused.trainer.policy_delay_status() == (d, step, step % d != 0)
        assert lit.trainer.fused_pairs == 4 and fused.trainer.fused_pairs == 0
    finally:
        lit.close()
        fused.close()


def test_set_quantile_target_between_replays_takes_effect():
    """(kappa, d) are captured by value: the call drops the graph, the next step is captured again with the new values, and the trainer
    ends, to the bit, where a fresh trainer built with the new values ends that starts from the parameters at the switch and is handed
    the same rows; the restatement follows with the same switch.  Plain gradient descent without smoothing or delay, so that the four
    parameter vectors are the whole state."""
    gcase, nb, _steps, sample_seed = W.GRAPH_CASE
    case = ("switch",) + gcase[1:8] + ("gradient-descent", 1, None) + gcase[11:]
    B, N = case[3], case[4]
    new = (W.SMALL_KAPPA, 5)
    inputs = W.graph_inputs()
    specs, P, episodes, rows, batches = inputs
    agent = _case_agent(case, inputs, sample_seed=sample_seed)
    try:
        for _s in range(2):
            agent.train_step(B, nb)                       # the eager pass and the capture, one replay
        mid = _params(agent)
        y_old = agent.trainer.last_quantiles(B)[2]
        agent.trainer.set_quantile_target(*new)
        for _s in range(2):
            agent.train_step(B, nb)                       # captured again, one replay
        assert agent.trainer.quantile_target == (float(np.float32(new[0])), new[1])
        switched = _params(agent) + list(agent.trainer.last_quantiles(B)) + list(agent.trainer.last_values(B)) + [np.asarray(agent.trainer.last_stats())]
    finally:
        agent.close()
    y_new = switched[6]
    assert not y_old[:, N - case[5]:].any() and y_old[:, N - case[5] - 1].any()
    assert not y_new[:, N - new[1]:].any() and y_new[:, N - new[1] - 1].any(), "the replayed graph still drops the old count"
    fresh_case = case[:5] + (new[1], new[0]) + case[7:]
    agent = _case_agent(fresh_case, (specs, mid, episodes, None, None), sample_seed=sample_seed)
    try:
        for s in (2, 3):
            agent.train_step(B, nb, idxs=rows[s * nb * B:(s + 1) * nb * B])
        fresh = _params(agent) + list(agent.trainer.last_quantiles(B)) + list(agent.trainer.last_values(B)) + [np.asarray(agent.trainer.last_stats())]
    finally:
        agent.close()
    for i, (x, y) in enumerate(zip(switched, fresh)):
        assert np.array_equal(x, y), ("the switched trainer against a fresh one", i)
    ref = W.restatement(specs, P, W.quant_of(case), np.float64, W.hyper_of(case))
    for s in range(4):
        if s == 2:
            ref.quant = (N, float(np.float32(new[0])), new[1])
        for k in range(s * nb, (s + 1) * nb):
            ref.train_minibatch(batches[k])
        ref.update_targets()
    _compare("switched", case[8], P, switched[:4] + _zero_slots(switched), R.vectors(ref), 4 * nb)
    kept = W.run_case(case, inputs, nb=nb, steps=4)[0]
    assert np.linalg.norm(kept[1] - R.vectors(ref)[1]) > 100 * W.bounds(P, kept, 4 * nb)[1]          # (the switch is not lost in the bound)


def _zero_slots(state):
    n = sum(len(p) for p in state[:2])
    return [np.zeros(n), np.zeros(n)]


# ---- 4. the reference's loop on host arrays: the stand-alone train ops (cpp_ddpg_train_actor, cpp_ddpg_train_critic)
@pytest.mark.parametrize("cid", ["A2-B8-N25-d0-sgd", "A9-B8-N64-d2-momentum", "lowdim-A3-B8-N25-d2-tqc"])
def test_the_literal_loop_on_host_arrays(cid):
    case = W.case_of(cid)
    opt, d, sm = case[8], case[9], case[10]
    inputs = W.case_inputs(case)
    specs, P, _ep, _idxs, batches = inputs
    agent = _case_agent(case, inputs)
    try:
        for b in batches:
            hb = HostBatch(*b)
            agent.actor.train(hb.state_1)
            agent.critic.train(hb)
            agent.target_actor.update_weights()
            agent.target_critic.update_weights()
        got = _params(agent)
        slots, counts = _slots(agent)
    finally:
        agent.close()
    ref = W.restatement(specs, P, W.quant_of(case), np.float64, W.hyper_of(case), opt, d, sm)
    for b in batches:
        ref.train_actor(b[0])
        ref.train_critic(b)
        ref.update_targets()
    if counts is not None:
        assert counts == [int(x) for x in ref.state()["step"]], counts
    _compare(cid + "-literal", opt, P, got + slots, R.vectors(ref), len(batches))


# ---- 5. n-step returns and random shift: both change the gathered minibatch, below everything the quantile critic does
def test_n_step_returns_reach_the_targets():
    """the n-step case's y is r_n + g_n s_j with the folded reward and mask of the device's gather (not the one-step columns)"""
    case = W.case_of("A2-B8-N25-d2-nstep3")
    B, N, drop = case[3], case[4], case[5]
    inputs = W.case_inputs(case)
    specs, P, _ep, idxs, batches = inputs
    one_step = W.case_inputs(case[:13] + (1,))[4]
    agent = _case_agent(case, inputs)
    try:
        agent.train_step(B, 1, idxs=idxs[:B])
        dev = tuple(agent.trainer.last_values(B)) + tuple(agent.trainer.last_quantiles(B))
    finally:
        agent.close()
    ref = W.restatement(specs, P, W.quant_of(case), np.float64, W.hyper_of(case))
    cg = ref.critic_gradients(batches[0])
    err = _row_errors(dev, cg)
    print("n-step: %s" % {k: "%.2e" % v for k, v in err.items()})
    _assert_rows(err)
    g = np.ravel(cg["g"])
    assert ((g > 0) & (g < 0.9 * 0.999)).any() and (g == 0).any()
    plain = ref.critic_gradients(one_step[0])
    assert np.abs(dev[6] - plain["y"]).max() > 100 * W.bar("y")


def test_with_random_shift():
    from oracle import ddpg_np as O
    from tests.test_gpu_random_shift import _shifted_minibatch
    lib, check, ptr = _abi()
    shape, B, A, rows, quant = (32, 32, 3, 2, 3), 8, 2, 120, (25, 1.0, 2)
    hp = T3.hyper_of("gradient-descent", 0.5, 0.25)
    agent = _build(shape, B, A, hp, quant, rows=rows + 50, seed=4)
    kw = dict(pixel=True, H=shape[0], W=shape[1], C=int(np.prod(shape[2:])))
    specs = (O.NetSpec("actor", A, [100, 100, 50], **kw), W.quant_spec(O.NetSpec("critic", A, [100, 100, 50], **kw), quant[0]))
    try:
        rng = np.random.default_rng(104)
        for net, sd in ((agent.actor, 0.05), (agent.critic, 0.05), (agent.target_actor, 0.01), (agent.target_critic, 0.01)):
            p = net.get_params()
            net.set_params(p + rng.normal(0, sd, p.shape).astype(np.float32))
        rm = agent.replay_memory
        rm.fill_synthetic(rows, seed=25)
        rm.enable_random_shift(4, seed=11)
        agent.train_step(B, 1)
        P = _params(agent)
        agent.train_step(B, 1)
        idxs = np.empty(B, np.int32)
        check(lib.cpp_replay_last_indexes(rm.handle, B, ptr(idxs)))
        t, unshifted, _sh = _shifted_minibatch(rm, idxs)
        dev = tuple(agent.trainer.last_values(B)) + tuple(agent.trainer.last_quantiles(B))
    finally:
        agent.close()
    ref = W.restatement(specs, P, quant, np.float64, hp)
    ag, cg = ref.actor_gradients(t[0]), ref.critic_gradients(t)
    err = _row_errors(dev, cg, ag)
    print("random shift: %s" % {k: "%.2e" % v for k, v in err.items()})
    _assert_rows(err)
    plain = ref.critic_gradients(unshifted)
    assert np.abs(dev[4] - plain["theta"]).max() > 100 * W.bar("theta")      # (the stored pixels miss it)


# ---- 6. the readers
def test_check_loss_forward_and_dq_da_read_q():
    case = W.case_of("A2-B8-N25-d2-smoothed")
    B, N, opt, d, sm = case[3], case[4], case[8], case[9], case[10]
    inputs = W.case_inputs(case)
    specs, P, _ep, _idxs, batches = inputs
    agent = _case_agent(case, inputs)
    try:
        hb = HostBatch(*batches[0])
        loss, td, q = agent.critic.check_loss(hb)
        assert agent.trainer.last_target_noise(B)[1] == 0              # (an evaluation: no draw, no count)
        theta, srt, y = agent.trainer.last_quantiles(B)
        q_fwd = agent.critic.forward(hb.state_1, hb.action)
        dq = agent.critic.q_gradients_wrt_actions(hb)
        names = [(v.name, tuple(v.shape)) for v in agent.critic.trainable_model_vars()]
    finally:
        agent.close()
    n_in = specs[1].fc[-1][1]
    assert names[-2:] == [("critic/q_value/weights:0", (n_in, N)), ("critic/q_value/biases:0", (N,))]
    ref = W.restatement(specs, P, W.quant_of(case), np.float64, W.hyper_of(case), opt, d, sm)
    wl, wtd, wq = ref.check_loss(batches[0])
    cg = ref.last_cg
    err = (abs(loss - wl), np.abs(td - wtd).max(), np.abs(q - wq).max(), np.abs(theta - cg["theta"]).max(), np.abs(srt - cg["sorted"]).max(),
           np.abs(y - cg["y"]).max())
    print("check_loss: |loss| %.2e |td| %.2e |q| %.2e |theta| %.2e |sorted| %.2e |y| %.2e" % err)
    assert err[0] < W.ATOL * max(1.0, wl) and err[1] < W.bar("td") and err[2] < W.bar("q")
    assert err[3] < W.bar("theta") and err[4] < W.bar("sorted") and err[5] < W.bar("y")
    assert q.shape == q_fwd.shape == (B, 1)
    # CriticNetwork.forward is inference mode on its own batch statistics: the mean of the restatement's atoms
    c = ref.critic.forward(hb.state_1, action=hb.action, training=False)
    want_q = c["out"].mean(axis=1, keepdims=True)
    assert np.abs(q_fwd - want_q).max() < W.bar("q") and np.ptp(want_q) > 0.05
    ag = ref.actor_gradients(hb.state_1)
    assert np.abs(dq - ag["dq_da"]).max() < W.bar("dq_da") and np.abs(ag["dq_da"]).max() > 1e-3


def test_checkpoints_round_trip_and_the_layout_check_refuses_both_ways(tmp_path):
    from cartpoleplusplus_amd import util
    case = W.case_of("A2-B5-N64-d63-adam")
    B = case[3]
    inputs = W.case_inputs(case)
    agent = _case_agent(case, inputs)
    try:
        agent.train_step(B, 2, idxs=inputs[3][:2 * B])
        util.SaverUtil(agent, str(tmp_path / "quant"), 3600).force_save()
        want = _params(agent) + _slots(agent)[0]
    finally:
        agent.close()
    bare = (inputs[0], None, None, None, None)
    agent = _case_agent(case, bare, seed=7)
    try:
        assert not np.array_equal(agent.critic.get_params(), want[1])
        util.SaverUtil(agent, str(tmp_path / "quant"), 3600)
        got = _params(agent) + _slots(agent)[0]
        assert all(np.array_equal(x, y) for x, y in zip(got, want))
    finally:
        agent.close()
    plain = _case_agent(case, bare, quant=None)
    try:
        util.SaverUtil(plain, str(tmp_path / "plain"), 3600).force_save()
        with pytest.raises(AssertionError, match="checkpoint does not match critic"):
            util.SaverUtil(plain, str(tmp_path / "quant"), 3600)
    finally:
        plain.close()
    for quant in ("case", (33, 1.0, 0)):          # a plain checkpoint into a quantile agent; another N
        agent = _case_agent(case, bare, quant=quant)
        try:
            with pytest.raises(AssertionError, match="checkpoint does not match critic"):
                util.SaverUtil(agent, str(tmp_path / ("plain" if quant == "case" else "quant")), 3600)
        finally:
            agent.close()


# ---- 7. the data-parallel step as a world of one
def test_the_data_parallel_step_as_a_world_of_one():
    case, nb, _steps, sample_seed = W.GRAPH_CASE
    cid, B, opt = case[0], case[3], case[8]
    lib, check, _ptr = _abi()
    inputs = W.graph_inputs()
    steps = 2
    agent = _graph_agent()
    try:
        for _s in range(steps):
            check(lib.cpp_ddpg_dp_train_step(agent.trainer.handle, agent.replay_memory.handle, None, B, nb, sample_seed, 1, 0))
        got = _params(agent)
        slots, counts = _slots(agent)
    finally:
        agent.close()
    short = (inputs[0], inputs[1], inputs[2], inputs[3][:steps * nb * B], inputs[4][:steps * nb])
    want, wcounts, _outs, _ref = W.run_case(case, short, nb=nb, steps=steps)
    assert counts == [int(x) for x in wcounts], counts
    _compare(cid + "-dp", opt, inputs[1], got + slots, want, steps * nb)


# ---- 8. off means off: a plain trainer's bits, ABI calls and launches; the census of a quantile step
_PLAIN_SNIPPET = r"""
import json, sys
sys.path.insert(0, %(root)r)
from tests import test_gpu_quantile as G
print("RESULT " + json.dumps(G._plain_run(%(quant_first)r)))
"""


def _plain_inputs():
    """the graph case with plain critics: tests.helpers.host_case's own q_value layer"""
    from tests.helpers import host_case
    case = W.GRAPH_CASE[0]
    specs, P, episodes, _i, _b = host_case(W.SHAPES[case[1]], case[3], 1, W.GRAPH_SEED, rows=W.ROWS, action_dim=case[2])
    return specs, P, episodes, None, None


class _CallLog(object):
    """counts the calls of the named ABI functions made through cartpoleplusplus_amd._lib.lib while it is installed"""
    def __init__(self, names):
        self.names, self.calls = names, collections.Counter()

    def __enter__(self):
        from cartpoleplusplus_amd import _lib
        self._saved = {n: getattr(_lib.lib, n) for n in self.names}
        for n, f in self._saved.items():
            setattr(_lib.lib, n, self._wrap(n, f))
        return self

    def _wrap(self, name, f):
        def call(*a):
            self.calls[name] += 1
            return f(*a)
        return call

    def __exit__(self, *exc):
        from cartpoleplusplus_amd import _lib
        for n, f in self._saved.items():
            setattr(_lib.lib, n, f)


NEW_CALLS = ("cpp_net_create_quantile", "cpp_net_quantile_info", "cpp_ddpg_set_quantile_target", "cpp_ddpg_last_quantiles")


def _plain_run(quant_first):
    """three graph-replayed outer steps of a PLAIN trainer (after a quantile one has lived and died in the process, if asked): the digest
    of its parameters and slots, the launch census of one more outer step, and how often it called the new entry points"""
    case, nb, _steps, sample_seed = W.GRAPH_CASE
    B = case[3]
    if quant_first:
        agent = _graph_agent()
        try:
            agent.train_step(B, nb)
            agent.train_step(B, nb)
        finally:
            agent.close()
    with _CallLog(NEW_CALLS) as log:
        agent = _case_agent(case, _plain_inputs(), quant=None, sample_seed=sample_seed)
        try:
            lib, check, _ptr = _abi()
            for _s in range(3):
                agent.train_step(B, nb)
            h = hashlib.sha256()
            for x in _params(agent) + _slots(agent)[0]:
                h.update(np.ascontiguousarray(x).tobytes())
            census = _profiled_calls(agent.actor.ctx, lambda: agent.train_step(B, nb))
            new_calls = sum(log.calls.values())
            n_q = ctypes.c_int(-1)
            check(lib.cpp_net_quantile_info(agent.critic.handle, ctypes.byref(n_q)))
            assert n_q.value == 0
        finally:
            agent.close()
    return {"digest": h.hexdigest(), "census": census, "new_calls": new_calls}


def test_off_means_off():
    """a plain trainer created after a quantile one in the same process ends with the bits, and launches the kernels, of one in a process
    that never made one: the fused heads launch, no quant launch; it calls none of the new entry points"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = subprocess.run([sys.executable, "-c", _PLAIN_SNIPPET % dict(root=root, quant_first=False)], cwd=root, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    fresh = json.loads([l for l in out.stdout.splitlines() if l.startswith("RESULT ")][0][len("RESULT "):])
    here = _plain_run(True)
    assert here["census"] == fresh["census"], (here["census"], fresh["census"])
    assert here["digest"] == fresh["digest"]
    assert here["new_calls"] == fresh["new_calls"] == 0
    c = here["census"]
    assert c.get("heads", 0) == W.GRAPH_CASE[1] and c.get("quant", 0) == 0 and c.get("dist", 0) == 0 and c.get("td", 0) == 0


def test_the_launches_of_a_quantile_outer_step_are_the_categorical_steps_with_quant_where_dist_stands():
    """the GEMM levels with quant.hip's two launches per minibatch; no td_kernel, no heads launch, no dist launch -- family by family the
    census of the same learner with categorical critics of the same width"""
    case, nb, _steps, sample_seed = W.GRAPH_CASE
    B, N = case[3], case[4]
    agent = _graph_agent()
    try:
        agent.train_step(B, nb)
        n = _profiled_calls(agent.actor.ctx, lambda: agent.train_step(B, nb))
    finally:
        agent.close()
    specs, P, episodes, _r, _b = W.graph_inputs()
    cat = _build(W.SHAPES[case[1]], B, case[2], W.hyper_of(case), None, P, episodes, sample_seed=sample_seed,
                 **dict(_case_kw(case), distributional_critic=True, num_atoms=N, v_min=-10.0, v_max=10.0))
    try:
        cat.train_step(B, nb)
        m = _profiled_calls(cat.actor.ctx, lambda: cat.train_step(B, nb))
    finally:
        cat.close()
    print("launches per outer step: quantile %s, categorical %s" % (n, m))
    assert n.get("quant", 0) == 2 * nb and n.get("heads", 0) == 0 and n.get("td", 0) == 0 and n.get("dist", 0) == 0, n
    assert m.get("dist", 0) == 2 * nb and m.get("quant", 0) == 0
    swapped = {("quant" if k == "dist" else k): v for k, v in m.items() if v}
    assert {k: v for k, v in n.items() if v} == swapped


# ---- 9. the refusals
def test_the_refusals():
    from cartpoleplusplus_amd import _lib
    lib, check, ptr = _abi()
    case = W.case_of("A2-B8-N25-d0-sgd")
    inputs = W.case_inputs(case)
    hpy = W.hyper_of(case)
    shape = W.SHAPES["16x16x3"]
    quant = _case_agent(case, inputs)
    try:
        plain = _build(shape, 8, 2, hpy, None)
        other_n = _build(shape, 8, 2, hpy, (33, 1.0, 0))
        twin = _build(shape, 8, 2, hpy, None, twin_q=True)
        cat = _build(shape, 8, 2, hpy, None, distributional_critic=True, num_atoms=25, v_min=-10.0, v_max=10.0)
        try:
            ctx = quant.actor.ctx.handle
            hp = _lib.DdpgHyper(1e-3, 1e-2, 0.9, 5.0, 0.1)
            h = ctypes.c_void_p()
            # mismatched critic / target critic: plain against quantile both ways, another N, a categorical one of the same width both ways,
            # a twin one both ways
            for critic, target in ((quant.critic, plain.target_critic), (plain.critic, quant.target_critic), (quant.critic, other_n.target_critic),
                                   (quant.critic, cat.target_critic), (cat.critic, quant.target_critic),
                                   (quant.critic, twin.target_critic), (twin.critic, quant.target_critic)):
                rc = lib.cpp_ddpg_create(ctx, plain.actor.handle, critic.handle, plain.target_actor.handle, target.handle, ctypes.byref(hp), ctypes.byref(h))
                assert rc == CPP_ERR_ARG, (rc, lib.cpp_last_error())
            # N out of range, not a critic
            spec = _lib.NetSpec()
            ctypes.memmove(ctypes.byref(spec), ctypes.byref(quant.critic.spec), ctypes.sizeof(spec))
            for n in (1, 65, 0, -3):
                rc = lib.cpp_net_create_quantile(ctx, ctypes.byref(spec), 8, n, ctypes.byref(h))
                assert rc == CPP_ERR_ARG and b"cpp_net_create_quantile" in lib.cpp_last_error(), (n, rc)
            ctypes.memmove(ctypes.byref(spec), ctypes.byref(quant.actor.spec), ctypes.sizeof(spec))
            rc = lib.cpp_net_create_quantile(ctx, ctypes.byref(spec), 8, 25, ctypes.byref(h))
            assert rc == CPP_ERR_ARG and b"cpp_net_create_quantile" in lib.cpp_last_error()
            # a quantile trainer takes batches up to 1024 (256 loss partials): a 1025-row pair of networks is refused, 1024 is not
            big = []
            try:
                for rows_, want_rc in ((1025, CPP_ERR_ARG), (1024, 0)):
                    for src in (quant.actor, quant.critic, quant.target_actor, quant.target_critic):
                        ctypes.memmove(ctypes.byref(spec), ctypes.byref(src.spec), ctypes.sizeof(spec))
                        n = ctypes.c_void_p()
                        if src in (quant.actor, quant.target_actor):
                            check(lib.cpp_net_create(ctx, ctypes.byref(spec), rows_, ctypes.byref(n)))
                        else:
                            check(lib.cpp_net_create_quantile(ctx, ctypes.byref(spec), rows_, 25, ctypes.byref(n)))
                        big.append(n)
                    a_, c_, ta_, tc_ = big[-4:]
                    t = ctypes.c_void_p()
                    rc = lib.cpp_ddpg_create(ctx, a_, c_, ta_, tc_, ctypes.byref(hp), ctypes.byref(t))
                    assert rc == want_rc, (rows_, rc, lib.cpp_last_error())
                    if rc == 0:
                        check(lib.cpp_ddpg_destroy(t))
                    else:
                        assert b"1024" in lib.cpp_last_error()
            finally:
                for n in big:
                    lib.cpp_net_destroy(n)
            # a quantile critic in an actor's place
            rc = lib.cpp_ddpg_create(ctx, quant.critic.handle, quant.critic.handle, plain.target_actor.handle, quant.target_critic.handle,
                                     ctypes.byref(hp), ctypes.byref(h))
            assert rc == CPP_ERR_ARG
            # NAF refuses such networks
            nh = _lib.NafHyper(0.9, 5.0, 0.1, 0, 1e-3, 0.0, 0.9, 0.999, 1e-8)
            rc = lib.cpp_naf_create(ctx, quant.critic.handle, quant.target_critic.handle, quant.critic.handle, quant.critic.handle, 0, ctypes.byref(nh), ctypes.byref(h))
            assert rc == CPP_ERR_ARG and b"quantile" in lib.cpp_last_error()
            # cpp_ddpg_set_quantile_target: kappa not finite or not positive, d outside [0, N - 1]; the trainer keeps what it had
            th = quant.trainer.handle
            for kappa, drop in ((0.0, 0), (-1.0, 0), (float("inf"), 0), (float("nan"), 0), (1.0, -1), (1.0, 25), (1.0, 64)):
                rc = lib.cpp_ddpg_set_quantile_target(th, kappa, drop)
                assert rc == CPP_ERR_ARG and b"cpp_ddpg_set_quantile_target" in lib.cpp_last_error(), (kappa, drop, rc)
            check(lib.cpp_ddpg_set_quantile_target(th, 0.5, 24))
            check(lib.cpp_ddpg_set_quantile_target(th, 1.0, 0))
            # ... and the read-back, on trainers without quantile critics (plain and categorical), and their argument checks
            buf = np.empty(8 * 25, np.float32)
            for other in (plain, cat):
                rc = lib.cpp_ddpg_set_quantile_target(other.trainer.handle, 1.0, 0)
                assert rc == CPP_ERR_STATE and b"cpp_ddpg_set_quantile_target" in lib.cpp_last_error()
                rc = lib.cpp_ddpg_last_quantiles(other.trainer.handle, 8, ptr(buf), None, None)
                assert rc == CPP_ERR_STATE and b"cpp_ddpg_last_quantiles" in lib.cpp_last_error()
            rc = lib.cpp_ddpg_last_distribution(quant.trainer.handle, 8, ptr(buf), None, None)          # (no support: not a categorical trainer)
            assert rc == CPP_ERR_STATE
            assert lib.cpp_ddpg_last_quantiles(None, 8, None, None, None) == CPP_ERR_ARG
            assert lib.cpp_ddpg_last_quantiles(th, 9, None, None, None) == CPP_ERR_ARG
            assert lib.cpp_ddpg_last_quantiles(th, 8, None, None, None) == 0
            assert lib.cpp_net_quantile_info(None, None) == CPP_ERR_ARG
        finally:
            for a in (plain, other_n, twin, cat):
                a.close()
    finally:
        quant.close()
    # the agent refuses the flags together before anything exists on the device
    with pytest.raises(SystemExit):
        _build(shape, 8, 2, hpy, (25, 1.0, 0), twin_q=True)
    with pytest.raises(SystemExit):
        _build(shape, 8, 2, hpy, (25, 1.0, 0), distributional_critic=True, v_min=0.0, v_max=1.0)
    with pytest.raises(SystemExit):
        _build(shape, 8, 2, hpy, (25, 1.0, 25))


def test_tqc_trains_through_main(capsys):
    """--quantile-critic --drop-top-quantiles 2 --n-step 3 --prioritized-replay through ddpg_cartpole.main on the stand-in environment"""
    from cartpoleplusplus_amd import ddpg_cartpole as D
    D.main(["--synthetic-env", "--use-raw-pixels", "--render-width", "16", "--render-height", "16", "--max-episode-len", "12", "--batch-size", "8",
            "--batches-per-step", "2", "--replay-memory-size", "200", "--replay-memory-burn-in", "20", "--max-num-actions", "60",
            "--quantile-critic", "--drop-top-quantiles", "2", "--n-step", "3", "--prioritized-replay"])
    out = capsys.readouterr()
    stats = [l for l in out.out.splitlines() if l.startswith("STATS")]
    assert stats and "q_value" in out.err
