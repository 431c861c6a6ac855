"""The actor on the minimum head on the device (--actor-min-q; cpp_ddpg_set_actor_min_q: csrc/heads_twin_min.hip on the fused path, the
GEMM levels with csrc/actor_min.hip elsewhere) against the float64 restatement tests/actor_min_np.py.  The cases, their seeds and what they
can see are that module's and tests/test_actor_min_host.py's: in every compared minibatch each head is followed on at least a quarter of
the rows, no row is closer to a tie than 1e-4 (ten times the bar on Q: the device cannot choose differently, no row is left out), the
float32 twin stays inside the bars used here and every planted fault leaves them by more than ten times.

Every minibatch is compared from a common start: the restatement takes over the device's parameters, slots and counts before it.
Bars: a, Q1 and Q2 at mu(s1), dQ/da, Q and td at the project's 1e-5 (td under smoothing plus tests.tps_np.td_bar's propagated noise term,
as tests/test_gpu_twin_q.py); sel exactly; pre-clip lists at rel 2e-5, norms at 1e-4; parameter, target and slot deltas at
tests.ddpg_opt_np's 2^-23 |theta| + 5e-5 |delta|, parameters and targets besides at rel 2e-5."""
import hashlib
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import actor_min_np as M
from tests import ddpg_opt_np as R
from tests import sac_np as S
from tests import td3_np as T3
from tests import twin_np as W
from tests.helpers import _profiled_calls, assert_flat_close, delta_bound
from tests.test_gpu_twin_q import PER_KW, HostBatch, _build, _params, _set_priorities, _slots

pytestmark = pytest.mark.gpu
CPP_ERR_ARG, CPP_ERR_STATE = 1, 3          # include/cartpolepp_abi.h
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _abi():
    from cartpoleplusplus_amd._lib import lib, check, ptr
    return lib, check, ptr


def _case_kw(case):
    _cid, _sn, _A, _B, opt, d, sm, _clip, _tau, extra = case
    kw = dict(T3.opt_kw(opt))
    if d > 1:
        kw["policy_delay"] = d
    if sm is not None:
        kw.update(target_policy_noise=sm[0], target_policy_noise_clip=sm[1], target_policy_noise_seed=sm[2])
    if extra.get("weighted"):
        kw.update(PER_KW)
    if extra.get("actor_hidden"):
        kw["actor_hidden_layers"] = ",".join(str(int(h)) for h in extra["actor_hidden"])
    return kw


def _agent(case, inputs, on=True, **kw):
    _cid, shape_name, A, B = case[:4]
    specs, P, episodes, _idxs, _b = inputs
    opts = dict(_case_kw(case), **kw)
    if on:
        opts["actor_min_q"] = True
    return _build(M.SHAPES[shape_name], B, A, M.hyper_of(case), P, episodes, rows=M.ROWS, **opts)


def _take_over(ref, case, P, slots, counts, k):
    """the restatement at the device's state in front of minibatch k (from 0) of a trainer that has run k minibatches"""
    na = len(P[0])
    for w, sl in (("actor", slice(0, na)), ("critic", slice(na, None))):
        ref.slots[w].m, ref.slots[w].v = np.asarray(slots[0][sl], np.float64).copy(), np.asarray(slots[1][sl], np.float64).copy()
    if counts is not None:
        ref.slots["actor"].t, ref.slots["critic"].t = counts
    ref.n, ref.tps_n = k, k
    return ref


def _read(agent, B, weighted):
    t = agent.trainer
    actions, dq_da, q, td = t.last_values(B)
    q2f, tq1, tq2, td2 = t.last_twin_values(B)
    mq1, mq2, sel = t.last_actor_min(B)
    stats = t.last_stats()
    got = {"actions": actions, "dq_da": dq_da, "q": q, "td": td, "q2": q2f, "tq1": tq1, "tq2": tq2, "td2": td2, "q1m": mq1, "q2m": mq2, "sel": sel,
           "loss": float(stats[0]), "actor_norm": float(stats[1]), "critic_norm": float(stats[2]), "g_a": agent.actor.get_grads(),
           "g_c": agent.critic.get_grads()}
    got["w"] = agent.replay_memory.last_weights(B).astype(np.float64).reshape(B, 1) if weighted else None
    return got


def _compare_minibatch(case, specs, start, got, after, k, batch):
    """one minibatch from the common start `start` = (the four parameter vectors, [m, v], counts)"""
    cid, _sn, _A, B, opt, d, sm, _clip, _tau, _x = case
    P, slots, counts = start
    ref = _take_over(M.restatement(case, specs, P), case, P, slots, counts, k)
    ref.weights, ref.fed = got["w"], batch[1]
    out = ref.train_minibatch(batch)
    ag, cg = ref.last_ag, ref.last_cg
    ref.update_targets()
    share, margin = float((ag["sel"] == 1).mean()), float(np.abs(ag["q1"] - ag["q2"]).min())
    assert margin >= M.TIE_MARGIN, (cid, k, margin)
    atol = M.P_BAR
    bar = W.td_bar(ref.hp.discount, sm[0], cg, atol) if sm is not None else atol
    err = {"actions": np.abs(got["actions"] - ag["actions"]).max(), "q1m": np.abs(got["q1m"] - ag["q1"]).max(),
           "q2m": np.abs(got["q2m"] - ag["q2"]).max(), "dq_da": np.abs(got["dq_da"] - ag["dq_da"]).max(), "q": np.abs(got["q"] - cg["q"]).max(),
           "q2": np.abs(got["q2"] - cg["q2"]).max(), "tq1": np.abs(got["tq1"] - cg["target_q"]).max(),
           "tq2": np.abs(got["tq2"] - cg["target_q2"]).max(), "td": np.abs(got["td"] - cg["td"]).max(), "td2": np.abs(got["td2"] - cg["td2"]).max(),
           "loss": abs(got["loss"] - float(cg["loss"]))}
    print("%s minibatch %d: %s; TD bar %.3e; head 1 followed on %.2f of the rows, smallest |Q1 - Q2| %.2e, sel %s" %
          (cid, k, {a: "%.2e" % b for a, b in err.items()}, bar, share, margin, got["sel"]))
    assert np.array_equal(got["sel"], ag["sel"]), (cid, k, got["sel"], ag["sel"])
    for key in ("actions", "q1m", "q2m", "dq_da", "q", "q2"):
        assert err[key] < atol, (cid, k, key, err)
    for key in ("tq1", "tq2", "td", "td2", "loss"):
        assert err[key] < bar, (cid, k, key, err, bar)
    assert_flat_close(specs[0], got["g_a"], ag["grads"], rel=2e-5, what="%s minibatch %d actor pre-clip grads" % (cid, k))
    floor = 2.0 * max(err["td"], err["td2"])
    try:
        assert_flat_close(W.TwinLayoutSpec(specs[1]), got["g_c"], cg["grads"], rel=2e-5, what="%s minibatch %d critic pre-clip grads" % (cid, k),
                          abs_floor=floor)
    except AssertionError:
        if sm is None:
            raise
        # (linear in the TDs, and the device's noise sits up to Z_BAR * sigma from the restated one: the backward arithmetic at the device's
        # TDs -- tests/test_gpu_twin_q.py)
        ww = np.ones((B, 1)) if got["w"] is None else got["w"]
        grads, _ = ref_backward(case, specs, P, batch, got, ww)
        assert_flat_close(W.TwinLayoutSpec(specs[1]), got["g_c"], grads, rel=2e-5, what="%s minibatch %d critic grads at the device's TDs" % (cid, k),
                          abs_floor=floor)
    na, nc = out["actor_norm"], out["critic_norm"]
    assert abs(got["actor_norm"] - na) < 1e-4 * max(1.0, na) and abs(got["critic_norm"] - nc) < 1e-4 * max(1.0, nc), (cid, k, got["actor_norm"], na, nc)
    # the deltas from the common start
    want = W.vectors(ref)
    have = list(after[0]) + list(after[1])
    begin = list(P) + [np.asarray(slots[0], np.float64), np.asarray(slots[1], np.float64)]
    bad = []
    for name, g, w, p in zip(T3.VECTORS, have, want, begin):
        if (name == "v" and opt != "adam") or (name == "m" and opt == "gradient-descent"):
            assert not np.asarray(g).any()
            continue
        e, b = float(np.linalg.norm(np.asarray(g, np.float64) - w)), delta_bound(p, w - p, R.R[name], 1)
        if not e <= b:
            bad.append((name, e, b))
        if name in T3.VECTORS[:4] and not e <= R.PARAM_REL * float(np.linalg.norm(w)):
            bad.append((name, "rel", e))
    assert not bad, (cid, k, bad)
    if not out["applied"]:      # a held actor keeps its bits
        assert d > 1 and np.array_equal(after[0][0], P[0]), (cid, k)
    if after[2] is not None:
        assert after[2] == [int(x) for x in ref.state()["step"]], (cid, k, after[2])
    return share


def ref_backward(case, specs, P, batch, got, ww):
    B = case[3]
    ref = M.restatement(case, specs, P)
    cb = ref.critic.forward(batch[0], action=np.asarray(batch[1], np.float64))
    grads, da = ref.critic.backward(cb, 2.0 * got["td"].astype(np.float64) * ww / B, 2.0 * got["td2"].astype(np.float64) * ww / B)
    return W.flatten_grads(specs[1], grads, np.float64), da


def partial_plan(case, inputs, capacity):
    """tests.helpers.capacity_plan of a case"""
    from tests.helpers import capacity_plan
    _cid, shape_name, A, B = case[:4]
    return capacity_plan(M.ROWS, M.SHAPES[shape_name], A, inputs[2], inputs[3], inputs[4], B, capacity)


def _run_case(cid, capacity=None, **kw):
    """capacity=C > B: the agent is built for C rows and walks partial_plan's minibatches -- C rows, B, B, C -- each held to the
    restatement from the device's own state in front of it, at the same bars"""
    case = M.case_of(cid)
    B, weighted = case[3], bool(case[9].get("weighted"))
    inputs = M.case_inputs(case)
    specs, _P, _ep, idxs, batches = inputs
    plan = [(idxs[k * B:(k + 1) * B], batches[k]) for k in range(M.NB)] if capacity is None else partial_plan(case, inputs, capacity)
    agent = _agent(case, inputs, capacity=capacity, **kw)
    shares, sels = [], []
    try:
        assert agent.trainer.actor_min_q
        if weighted:
            _set_priorities(agent)
        for k, (rows, batch) in enumerate(plan):
            sl, counts = _slots(agent)
            start = (_params(agent), sl, counts)
            agent.train_step(len(rows), 1, idxs=rows)
            got = _read(agent, len(rows), weighted)
            sl2, counts2 = _slots(agent)
            shares.append(_compare_minibatch(case, specs, start, got, (_params(agent), sl2, counts2), k, batch))
            sels.append(int(got["sel"][0]))
    finally:
        agent.close()
    if B == 1:
        assert len(set(sels)) == 2, sels
    else:
        assert all(M.MIN_SHARE <= s <= 1 - M.MIN_SHARE for s in shares), shares


# ---- 1. every case, minibatch by minibatch
@pytest.mark.parametrize("cid", [c[0] for c in M.CASES])
def test_minibatches_against_the_float64_restatement(cid):
    _run_case(cid)


def test_minibatches_below_the_capacity_against_the_float64_restatement():
    """(C, B) = (8, 5), twin heads with the actor on the minimum: the rows of both heads, actor_min's selection and the gradient lists at B
    behind a C-row minibatch, and at C again behind the B-row ones"""
    _run_case("A1-B5-sgd", capacity=8)


def test_the_eight_bit_store_changes_nothing():
    _run_case("A3-B5-smoothed", replay_store="u8")          # (the cases' frames are pixel codes: the same minibatches)


@pytest.mark.parametrize("cid,heads,added", [("A1-B5-sgd", 1, {}), ("A5-B7-weighted-smoothed", 1, {}), ("A2-B5-no-pre", 1, {}),
                                             ("A9-B5-sgd", 0, {"gemm": 1, "elementwise": 1}), ("lowdim-A3-B5-td3", 0, {"gemm": 2, "elementwise": 1})])
def test_the_launch_census(cid, heads, added):
    """the fused step launches what the twin step launches, kernel family by kernel family; on the GEMM levels head 2's forward and dX GEMMs
    ride in head 1's levels and the added launches are: actor_min_kernel, the GEMM level that adds head 2's action columns and, where the
    actor's chain is the pass's longest (the low-dimensional pair), one more GEMM level -- the kernel's level holds no GEMM, and the levels
    behind it no longer coincide with the critic's"""
    case = M.case_of(cid)
    B = case[3]
    inputs = M.case_inputs(case)
    census = {}
    for on in (False, True):
        agent = _agent(case, inputs, on=on)
        try:
            if case[9].get("weighted"):
                _set_priorities(agent)
            agent.train_step(B, 1, idxs=inputs[3][:B])
            census[on] = _profiled_calls(agent.actor.ctx, lambda: agent.train_step(B, 1, idxs=inputs[3][B:2 * B]))
        finally:
            agent.close()
    print(cid, census)
    assert census[True].get("heads", 0) == census[False].get("heads", 0) == heads
    diff = {k: census[True].get(k, 0) - census[False].get(k, 0) for k in set(census[True]) | set(census[False])}
    assert {k: v for k, v in diff.items() if v} == added, diff


# ---- 2. soft actor-critic: tests/test_gpu_sac_composed.py's comparison, the restatement's actor on the minimum
@pytest.mark.parametrize("cid", [c[0] for c in M.SAC_CASES])
def test_soft_actor_critic_against_the_float64_restatement(cid):
    from tests import test_gpu_sac_composed as G
    case = M.sac_case_of(cid)
    B = case[3]
    inputs = M.sac_inputs(case)
    agent = G._agent(case, inputs, actor_min_q=True)
    refs = (M.sac_restatement(case, inputs), M.sac_restatement(case, inputs, np.float32))
    shares = []
    try:
        assert agent.trainer.actor_min_q
        start = G._state(agent)
        for k in range(M.SAC_NB):
            rows = np.ascontiguousarray(inputs[3][k * B:(k + 1) * B], dtype=np.int32)
            agent.train_step(B, 1, idxs=rows)
            got, sac, routes = G._read_minibatch(agent, case, k)
            q1, q2, sel = agent.trainer.last_actor_min(B)
            got_vec = G._state(agent)
            batch = S.composed_batches(case, inputs[2], rows)[0]
            for ref in refs:
                ref.fed = batch[1]
            _want, ref = G._compare(case, inputs, refs, start, k, got, sac, routes, got_vec, batch, None, run=" (actor on the minimum)")
            ag = ref.last_ag
            margin = float(np.abs(ag["q1"] - ag["q2"]).min())
            e1, e2 = float(np.abs(q1 - ag["q1"]).max()), float(np.abs(q2 - ag["q2"]).max())
            print("%s minibatch %d: |Q1| %.2e |Q2| %.2e at the sample; sel %s; smallest |Q1 - Q2| %.2e" % (cid, k, e1, e2, sel, margin))
            assert margin >= M.TIE_MARGIN and np.array_equal(sel, ag["sel"]), (cid, k, sel, ag["sel"])
            assert e1 < M.P_BAR and e2 < M.P_BAR and np.abs(got["dq_da"] - ag["dq_da"]).max() < M.P_BAR
            shares.append(float((ag["sel"] == 1).mean()))
            start = got_vec
    finally:
        agent.close()
    assert all(M.MIN_SHARE <= s <= 1 - M.MIN_SHARE for s in shares), shares


# ---- 3. a tie is head 1's
@pytest.mark.parametrize("cid", ["A2-B7-weighted", "lowdim-A3-B5-td3"])
def test_a_tie_is_head_ones(cid):
    """head 2 a copy of head 1 (the fused instances; the GEMM levels): the two sums are the same arithmetic, every row ties, sel is 1"""
    case = M.case_of(cid)
    B = case[3]
    inputs = M.tie_inputs(case, M.case_inputs(case))
    agent = _agent(case, inputs)
    try:
        if case[9].get("weighted"):
            _set_priorities(agent)
        agent.train_step(B, 1, idxs=inputs[3][:B])
        q1, q2, sel = agent.trainer.last_actor_min(B)
    finally:
        agent.close()
    assert np.array_equal(q1, q2) and (sel == 1).all(), (q1, q2, sel)


# ---- 4. the bit identities
def _digest(agent):
    h = hashlib.sha256()
    for x in _params(agent) + _slots(agent)[0]:
        h.update(np.ascontiguousarray(x).tobytes())
    return h.hexdigest()


GRAPH = ("A3-B5-smoothed", 3, 3, 0)          # case, minibatches per outer step, outer steps, sample seed


def _graph_run(mode, on=True, toggle=False):
    """three outer steps of three minibatches on the rows the device draws (the eager pass and the capture, two replays); mode 'rows': the same
    rows handed in, which runs every minibatch eagerly; 'dp': the data-parallel step as a world of one"""
    cid, nb, steps, seed = GRAPH
    case = M.case_of(cid)
    B = case[3]
    inputs = M.case_inputs(case)
    lib, check, _ptr = _abi()
    agent = _agent(case, inputs, on=on, sample_seed=seed)
    try:
        if toggle:
            agent.trainer.set_actor_min_q(True)
            agent.trainer.set_actor_min_q(False)
        for s in range(steps):
            if mode == "graph":
                agent.train_step(B, nb)
            elif mode == "rows":
                rows = np.concatenate([T3.device_rows(seed, k, B, M.ROWS) for k in range(s * nb, (s + 1) * nb)])
                agent.train_step(B, nb, idxs=rows)
            else:
                check(lib.cpp_ddpg_dp_train_step(agent.trainer.handle, agent.replay_memory.handle, None, B, nb, seed, 1, 0))
        out = _digest(agent)
        vals = agent.trainer.last_actor_min(B) if on else None
    finally:
        agent.close()
    return out, vals


def test_graph_replays_eager_steps_repeated_runs_and_the_data_parallel_step_agree_to_the_bit():
    graph = [_graph_run("graph") for _ in range(3)]
    assert graph[0][0] == graph[1][0] == graph[2][0]
    assert all(np.array_equal(a, b) for a, b in zip(graph[0][1], graph[1][1]))
    eager, dp = _graph_run("rows"), _graph_run("dp")
    assert eager[0] == graph[0][0], "a replayed graph leaves other bits than the eager step on the same rows"
    assert dp[0] == graph[0][0], "the data-parallel step as a world of one leaves other bits"
    assert set(graph[0][1][2].tolist()) <= {1, 2}


def test_off_means_off():
    """a --twin-q trainer that had the switch on and then off: the bits of one that never had it, parameters, targets and slots over three
    minibatches (and three replayed outer steps); the switch on leaves other bits"""
    never, toggled, on = _graph_run("graph", on=False), _graph_run("graph", on=False, toggle=True), _graph_run("graph")
    assert never[0] == toggled[0] and never[0] != on[0]
    assert _graph_run("rows", on=False)[0] == _graph_run("rows", on=False, toggle=True)[0] == never[0]


def test_a_trainer_without_the_flag_makes_neither_call(monkeypatch):
    from cartpoleplusplus_amd import ddpg_cartpole as D
    calls = []
    for name in ("cpp_ddpg_set_actor_min_q", "cpp_ddpg_last_actor_min"):
        real = getattr(D.lib, name)
        monkeypatch.setattr(D.lib, name, lambda *a, _n=name, _r=real: calls.append(_n) or _r(*a))
    case = M.case_of("A1-B5-sgd")
    inputs = M.case_inputs(case)
    agent = _agent(case, inputs, on=False)
    try:
        agent.train_step(case[3], 1, idxs=inputs[3][:case[3]])
        assert not agent.trainer.actor_min_q
    finally:
        agent.close()
    assert calls == []
    agent = _agent(case, inputs)
    try:
        agent.train_step(case[3], 1, idxs=inputs[3][:case[3]])
    finally:
        agent.close()
    assert calls == ["cpp_ddpg_set_actor_min_q"]


def test_the_paired_literal_loop_is_the_fused_step_bit_for_bit():
    """actor.train(batch.state_1); critic.train(batch) on a device-resident batch run as ONE cpp_ddpg_train_rows -- against
    train_step(B, 1, idxs) on the same rows, per minibatch, to the bit"""
    case = M.case_of("A3-B5-smoothed")
    B = case[3]
    inputs = M.case_inputs(case)
    lit, fused = _agent(case, inputs), _agent(case, inputs)
    try:
        np.random.seed(99)
        for step in range(1, 4):
            batch = lit.replay_memory.batch(B)
            lit.actor.train(batch.state_1)
            lit.critic.train(batch)
            lit.target_actor.update_weights()
            lit.target_critic.update_weights()
            fused.train_step(B, 1, idxs=batch.idxs)
            for a, b in zip(_params(lit) + list(lit.trainer.last_actor_min(B)) + list(lit.trainer.last_values(B)),
                            _params(fused) + list(fused.trainer.last_actor_min(B)) + list(fused.trainer.last_values(B))):
                assert np.array_equal(a, b), step
        assert lit.trainer.fused_pairs == 3 and _digest(lit) == _digest(fused)
    finally:
        lit.close(); fused.close()


@pytest.mark.parametrize("cid", ["A2-B7-weighted", "A9-B5-sgd", "lowdim-A3-B5-td3"])
def test_the_single_ops_are_the_pass_byte_for_byte(cid):
    """cpp_ddpg_q_gradients_wrt_actions and cpp_ddpg_train_actor run the actor's half alone (head 2's forward with it) on the GEMM levels:
    dq_da, a, Q1, Q2 and sel are cpp_ddpg_compute_gradients' on the same minibatch, byte for byte where that pass takes the GEMM levels too
    (at the project's bar where it takes the fused heads); q stays Q1; and the actor's list of train_actor is the pass's"""
    case = M.case_of(cid)
    B = case[3]
    inputs = M.case_inputs(case)
    specs, P, _ep, _idxs, batches = inputs
    lib, check, ptr = _abi()
    hb = HostBatch(*batches[0])
    agent = _agent(case, inputs, **({"prioritized_replay": False} if case[9].get("weighted") else {}))
    try:
        t = agent.trainer
        dev = t.device_batch_for(hb)
        check(lib.cpp_ddpg_compute_gradients(t.handle, dev.handle))
        whole = list(t.last_values(B)[:2]) + list(t.last_actor_min(B)) + [agent.actor.get_grads()]
        dq = agent.critic.q_gradients_wrt_actions(hb)
        half = [t.last_values(B)[0], dq] + list(t.last_actor_min(B)) + [agent.actor.get_grads()]
        A = case[2]
        dq2, acts, q = np.empty((B, A), np.float32), np.empty((B, A), np.float32), np.empty((B, 1), np.float32)
        check(lib.cpp_ddpg_q_gradients_wrt_actions(t.handle, dev.handle, ptr(dq2), ptr(acts), ptr(q)))
        assert np.array_equal(q, half[2]) and np.array_equal(dq2, dq)          # (q stays Q1)
    finally:
        agent.close()
    gemm = cid in ("A9-B5-sgd", "lowdim-A3-B5-td3")
    for name, a, b in zip(("actions", "dq_da", "q1", "q2", "sel", "actor's list"), whole, half):
        if gemm or name == "sel":
            assert np.array_equal(a, b), (cid, name)
        elif name != "actor's list":
            assert np.abs(a - b).max() < M.P_BAR, (cid, name)
    ref = M.restatement(case, specs, P)
    ag = ref.actor_gradients(batches[0][0])
    assert np.array_equal(half[4], ag["sel"]) and np.abs(half[1] - ag["dq_da"]).max() < M.P_BAR
    assert np.abs(half[1] - ref.critic.d_action(ref.critic.forward(hb.state_1, action=ag["actions"]), 1)).max() > 10 * M.P_BAR


def test_the_literal_loop_on_host_arrays():
    """the stand-alone train ops (cpp_ddpg_train_actor, cpp_ddpg_train_critic) under a policy delay of 2: a held actor keeps its bits, an
    applied one is the restatement's"""
    case = M.case_of("lowdim-A3-B5-td3")
    _c, _sn, _A, B, opt, d, sm, _clip, _tau, _x = case
    inputs = M.case_inputs(case)
    specs, P, _ep, _idxs, batches = inputs
    agent = _agent(case, inputs)
    held = []
    try:
        for b in batches:
            hb = HostBatch(*b)
            before = agent.actor.get_params()
            agent.actor.train(hb.state_1)
            agent.critic.train(hb)
            held.append(np.array_equal(before, agent.actor.get_params()))
            agent.target_actor.update_weights()
            agent.target_critic.update_weights()
        got = _params(agent)
        slots, counts = _slots(agent)
    finally:
        agent.close()
    ref = M.restatement(case, specs, P)
    for b in batches:
        ref.train_actor(b[0])
        ref.train_critic(b)
        ref.update_targets()
    assert held == [not a for a in ref.schedule] == [True, False, True], (held, ref.schedule)
    assert counts == [int(x) for x in ref.state()["step"]], counts
    for name, g, w, b in zip(T3.VECTORS, got + slots, W.vectors(ref), W.bounds(P, W.vectors(ref), len(batches))):
        err = float(np.linalg.norm(np.asarray(g, np.float64) - w))
        assert err <= b, (name, err, b)


# ---- 5. the ablation library: the GEMM levels and the heads kernel without its `pre` layer on the fused cases' shapes
@pytest.mark.parametrize("switch", ["CPP_FUSED_HEADS", "CPP_HEADS_PRE"])
def test_the_fused_cases_hold_on_the_other_paths_when_selected(switch):
    env = dict(os.environ, CARTPOLEPP_ABLATION="1")
    env[switch] = "0"
    pick = "minibatches_against and (A1-B5-sgd or A3-B5-smoothed or A5-B7-weighted-smoothed or A8-B5-adam or A2-B1-sgd)"
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.join(ROOT, "tests", "test_gpu_actor_min.py"), "-q", "-x", "-m", "gpu", "-p", "no:cacheprovider",
                        "-k", pick], cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=600)
    tail = r.stdout.decode()[-1500:]
    assert r.returncode == 0 and "5 passed" in tail, tail


# ---- 6. batch norm composes
def test_batch_norm_composes():
    """--use-batch-norm with the actor on the minimum head, one minibatch (batch statistics of the four trunks): the choice exactly, the
    per-row values at the project's bar"""
    shape, A, B, rows = (16, 16, 3, 1, 2), 2, 5, 64          # (six channels: the batch-norm kernels' dense dW rows come in 16-byte chunks)
    case = ("bn-A2-B5", "16x16x6", A, B, "gradient-descent", 1, None, 0.5, 0.25, {})
    for seed in range(1, 40):          # the first seed whose rows meet the conditions (asserted below)
        specs, P, episodes, idxs, batches = W.host_case(shape, B, 1, seed, rows=rows, action_dim=A, batch_norm=True)
        ref = M.restatement(case, specs, P)
        ag = ref.actor_gradients(batches[0][0])
        P[1][-1] += M.midpoint_shift(ag["q1"] - ag["q2"])
        ref = M.restatement(case, specs, P)
        ag = ref.actor_gradients(batches[0][0])
        if M.MIN_SHARE <= (ag["sel"] == 1).mean() <= 1 - M.MIN_SHARE and np.abs(ag["q1"] - ag["q2"]).min() >= M.TIE_MARGIN:
            break
    assert seed == 1, seed
    agent = _build(shape, B, A, M.hyper_of(case), P, episodes, rows=rows, use_batch_norm=True, actor_min_q=True)
    try:
        agent.train_step(B, 1, idxs=idxs[:B])
        actions, dq_da, _q, _td = agent.trainer.last_values(B)
        q1, q2, sel = agent.trainer.last_actor_min(B)
    finally:
        agent.close()
    err = {"actions": np.abs(actions - ag["actions"]).max(), "dq_da": np.abs(dq_da - ag["dq_da"]).max(), "q1": np.abs(q1 - ag["q1"]).max(),
           "q2": np.abs(q2 - ag["q2"]).max()}
    print("batch norm: %s; sel %s" % ({k: "%.2e" % v for k, v in err.items()}, sel))
    assert np.array_equal(sel, ag["sel"]) and len(set(sel.tolist())) == 2
    assert max(err.values()) < M.P_BAR, err


# ---- 7. the refusals
def test_the_refusals():
    lib, _check, ptr = _abi()
    case = M.case_of("A1-B5-sgd")
    inputs = M.case_inputs(case)
    specs, P = inputs[0], inputs[1]
    n1 = specs[1].num_params()
    twin = _agent(case, inputs, on=False)
    try:
        plain = _build(M.SHAPES["8x8x6"], 5, 1, M.hyper_of(case), twin=False)
        try:
            for on in (1, 0):      # plain critics
                assert lib.cpp_ddpg_set_actor_min_q(plain.trainer.handle, on) == CPP_ERR_ARG and b"twin" in lib.cpp_last_error()
            # one twin critic only: no such trainer exists (cpp_ddpg_create refuses the pair), so neither does the switch
            import ctypes
            from cartpoleplusplus_amd import _lib
            hp, h = _lib.DdpgHyper(1e-3, 1e-2, 0.9, 5.0, 0.1), ctypes.c_void_p()
            rc = lib.cpp_ddpg_create(twin.actor.ctx.handle, plain.actor.handle, twin.critic.handle, plain.target_actor.handle, plain.target_critic.handle,
                                     ctypes.byref(hp), ctypes.byref(h))
            assert rc == CPP_ERR_ARG
            assert lib.cpp_ddpg_set_actor_min_q(None, 1) == CPP_ERR_ARG
            buf, sel = np.empty(5, np.float32), np.empty(5, np.int32)
            assert lib.cpp_ddpg_last_actor_min(twin.trainer.handle, 5, ptr(buf), None, ptr(sel)) == CPP_ERR_STATE          # (off)
            assert lib.cpp_ddpg_last_actor_min(plain.trainer.handle, 5, ptr(buf), None, None) == CPP_ERR_STATE
            twin.trainer.set_actor_min_q(True)
            assert lib.cpp_ddpg_last_actor_min(twin.trainer.handle, 6, None, None, None) == CPP_ERR_ARG
            assert lib.cpp_ddpg_last_actor_min(twin.trainer.handle, 5, None, None, None) == 0          # (NULL pointers are skipped)
        finally:
            plain.close()
    finally:
        twin.close()
    from cartpoleplusplus_amd import ddpg_cartpole as D
    with pytest.raises(SystemExit):
        D.main(["--synthetic-env", "--use-raw-pixels", "--render-width", "16", "--render-height", "16", "--actor-min-q"])
    assert n1 < len(P[1])


def test_the_recipe_trains_through_main(capsys):
    """--twin-q --actor-min-q --n-step 3 --target-policy-noise 0.2 through ddpg_cartpole.main on the stand-in environment"""
    from cartpoleplusplus_amd import ddpg_cartpole as D
    D.main(["--synthetic-env", "--use-raw-pixels", "--render-width", "16", "--render-height", "16", "--max-episode-len", "12", "--batch-size", "8",
            "--batches-per-step", "2", "--replay-memory-size", "200", "--replay-memory-burn-in", "20", "--max-num-actions", "60", "--twin-q",
            "--actor-min-q", "--n-step", "3", "--target-policy-noise", "0.2", "--ddpg-optimiser", "Adam"])
    out = capsys.readouterr()
    assert [l for l in out.out.splitlines() if l.startswith("STATS")] and "actor_min_q=True" in out.err


# ---- 8. the DrQ-v2 stack: 64x64x18, feature layer norm, twin heads, smoothing, n-step 3, random shift -- and the actor on the minimum
def test_the_drq_v2_stack_against_the_float64_restatement():
    """two warm minibatches on device-drawn rows, head 2's online q_valueb bias balanced on the rows of the next draw (unshifted pixels: an
    estimate of the midpoint is enough, the conditions are asserted on the minibatch as formed), then the checked minibatch rebuilt on the
    host -- its rows and shifts read back, the memory's n-step columns, tests/shift_np.py's images -- and the float64 restatement
    (tests.layer_norm_np's networks under tests.actor_min_np.MinTwinDDPG) on the device's routes, the noise count at 2"""
    from oracle import ddpg_np as O
    from tests import layer_norm_np as L
    from tests import test_gpu_layer_norm as GL
    from tests.test_gpu_random_shift import _shifted_minibatch
    lib, check, ptr = _abi()
    B, rows, hidden, seed, sample_seed = 8, 64, (65, 20, 10), 4, 5
    hp = O.Hyper(1e-2, 5e-2, 0.9, 0.5, 0.25)
    sm = W.SMOOTHING
    specs, P0, episodes, _i, _b = L.host_case(GL.SHAPE, B, 1, seed, hidden, "tanh", rows=rows)
    on, tg = W.twin_tail(specs[1], np.random.default_rng(5000 + seed))
    P0 = [P0[0], np.concatenate([P0[1], on]), P0[2], np.concatenate([P0[3], tg])]          # (tests.twin_np's order: [plain | gamma beta | twin])
    dev = lambda v: L.twin_to_device(specs[1], np.asarray(v))
    back = lambda v: L.twin_from_device(specs[1], np.asarray(v))

    def restated(P, dt=np.float64):
        ref = L.with_feature_norm(M.MinTwinDDPG)(specs[0], specs[1], P[0], P[1], dt, hp, "GradientDescent", {}, 1, sm)
        ref.set_targets(P[2], P[3])
        return ref
    agent = GL._agent(B, hidden, "tanh", hp, [P0[0], dev(P0[1]), P0[2], dev(P0[3])], episodes, rows=rows, sample_seed=sample_seed, n_step=3,
                      twin_q=True, actor_min_q=True, target_policy_noise=sm[0], target_policy_noise_clip=sm[1], target_policy_noise_seed=sm[2])
    try:
        rm = agent.replay_memory
        rm.enable_random_shift(2, seed=9)
        census = _profiled_calls(agent.actor.ctx, lambda: agent.train_step(B, 1))
        assert (census.get("heads", 0), census.get("ln_fwd", 0), census.get("ln_bwd", 0), census.get("td", 0)) == (1, 1, 2, 0), census
        agent.train_step(B, 1)
        nxt = T3.device_rows(sample_seed, 2, B, rows)
        a, c, ta, tc = GL._params(agent)
        est = restated([a, back(c), ta, back(tc)]).actor_gradients(rm.state[rm.batch(idxs=nxt).state_1_idx])
        c = back(c)
        c[-1] += M.midpoint_shift(est["q1"] - est["q2"])
        agent.critic.set_params(dev(c))
        P = [a, c, ta, back(tc)]
        agent.train_step(B, 1)
        idxs = np.empty(B, np.int32)
        check(lib.cpp_replay_last_indexes(rm.handle, B, ptr(idxs)))
        assert np.array_equal(idxs, nxt)
        t, _un, _sh = _shifted_minibatch(rm, idxs)
        actions, dq_da, q, td = agent.trainer.last_values(B)
        q1, q2, sel = agent.trainer.last_actor_min(B)
        g_a = agent.actor.get_grads()
        got = GL._params(agent)
        routes = GL._routes(agent, B)
        assert agent.trainer.last_target_noise(B)[1] == 2
    finally:
        agent.close()
    m = np.asarray(t[3]).ravel()
    assert ((m > 0) & (m < 1)).any(), m          # (folded masks: discount^2)
    upd = {}
    for dt in (np.float64, np.float32):
        ref = restated(P, dt)
        (ref.actor.amax_override, ref.actor.relu_override), (ref.critic.amax_override, ref.critic.relu_override) = routes
        ref.tps_n = 2
        ag, cg = ref.actor_gradients(t[0]), ref.critic_gradients(t)
        ca, _na = O.clip_by_global_norm(ag["grads"], hp.gradient_clip, dt)
        upd[dt] = np.asarray(np.asarray(P[0], dt) - dt(hp.actor_lr) * ca, np.float64)
        if dt is np.float64:
            share, margin = float((ag["sel"] == 1).mean()), float(np.abs(ag["q1"] - ag["q2"]).min())
            bar = W.td_bar(hp.discount, sm[0], cg, M.P_BAR)
            err = {"actions": np.abs(actions - ag["actions"]).max(), "q1": np.abs(q1 - ag["q1"]).max(), "q2": np.abs(q2 - ag["q2"]).max(),
                   "dq_da": np.abs(dq_da - ag["dq_da"]).max(), "q": np.abs(q - cg["q"]).max(), "td": np.abs(td - cg["td"]).max()}
            print("DrQ-v2 stack: %s; TD bar %.3e; head 1 followed on %.2f of the rows, smallest |Q1 - Q2| %.2e, sel %s" %
                  ({k: "%.2e" % v for k, v in err.items()}, bar, share, margin, sel))
            assert M.MIN_SHARE <= share <= 1 - M.MIN_SHARE and margin >= M.TIE_MARGIN, (share, margin)
            assert np.array_equal(sel, ag["sel"]), (sel, ag["sel"])
            assert max(err[k] for k in ("actions", "q1", "q2", "dq_da", "q")) < M.P_BAR and err["td"] < bar, (err, bar)
            assert_flat_close(specs[0], g_a, ag["grads"], rel=2e-5, what="actor pre-clip grads vs f64")
            assert np.abs(ag["dq_da"] - ref.critic.d_action(ref.critic.forward(t[0], action=ag["actions"]), 1)).max() > 10 * M.P_BAR
    e, e32 = float(np.linalg.norm(got[0].astype(np.float64) - upd[np.float64])), float(np.linalg.norm(upd[np.float32] - upd[np.float64]))
    bound = delta_bound(P[0], upd[np.float64] - P[0], R.R["actor"], 1)
    print("  actor |err| %.3e  float32 evaluation %.3e  bound %.3e" % (e, e32, bound))
    assert e32 <= bound, "the float32 evaluation of this update leaves the bound itself: the case is void"
    assert e <= bound, (e, bound)
