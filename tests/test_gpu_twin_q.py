"""Twin Q heads on the device (--twin-q; cpp_net_create_twin_q: csrc/heads_twin.hip on the fused paths, the GEMM levels with td_twin_kernel
elsewhere) against the float64
restatement tests/twin_np.py.  The cases, their tolerances and what they can see are that module's and tests/test_twin_q_host.py's: every
case's float32 evaluation stays inside the bounds used here on the float64 routes, each head is the minimum on at least a quarter of the
rows of every compared minibatch, and every planted fault leaves the bounds by more than ten times.

Tolerances: tests/ddpg_opt_np.py's, unchanged -- per vector (the four parameter vectors, m, v) 2^-23 * nb * |theta| + r * |delta_f64| with
r = 5e-5, parameters and targets besides at rel 2e-5 of the vector.  Per-row values of one minibatch (Q1, Q2, Q1', Q2', dQ/da) at the
suite's 1e-5; td_1, td_2 and the loss at 1e-5, with smoothing plus tests.tps_np.td_bar's propagated noise term; gradients at rel 2e-5."""
import collections
import ctypes
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle import ddpg_np as O
from tests import ddpg_opt_np as R
from tests import td3_np as T3
from tests import twin_np as W
from tests.helpers import FakeEnv, _profiled_calls, assert_flat_close, hyper_options, make_opts, set_actor_masks

pytestmark = pytest.mark.gpu
CPP_ERR_ARG, CPP_ERR_STATE = 1, 3          # include/cartpolepp_abi.h
HostBatch = collections.namedtuple("HostBatch", "state_1 action reward terminal_mask state_2")
PER_KW = dict(prioritized_replay=True, priority_alpha=0.6, priority_beta=0.4, priority_eps=1e-6)


def _abi():
    from cartpoleplusplus_amd._lib import lib, check, ptr
    return lib, check, ptr


def _build(shape, B, A, hp, P=None, episodes=None, rows=W.ROWS, twin=True, seed=1, capacity=None, **kw):
    """a device agent (twin critics unless told otherwise) holding the case's parameters and episodes; capacity: the batch size it is
    built with (None: B)"""
    from cartpoleplusplus_amd import ddpg_cartpole as D
    pixel = len(shape) == 5
    make_opts(D, shape, B if capacity is None else int(capacity), pixel, replay_memory_size=rows, twin_q=twin, **dict(hyper_options(hp), **kw))
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
    _cid, _sn, _A, _B, opt, d, sm, _clip, _tau = case
    kw = dict(T3.opt_kw(opt))
    if d > 1:
        kw["policy_delay"] = d
    if sm is not None:
        kw.update(target_policy_noise=sm[0], target_policy_noise_clip=sm[1], target_policy_noise_seed=sm[2])
    if "weighted" in case[0]:
        kw.update(PER_KW)
    return kw


def _case_agent(case, inputs, **kw):
    _cid, shape_name, A, B, _opt, _d, _sm, _clip, _tau = case
    specs, P, episodes, _idxs, _b = inputs
    return _build(W.SHAPES[shape_name], B, A, W.hyper_of(case), P, episodes, **dict(_case_kw(case), **kw))


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


# ---- 1. one minibatch: every per-row value, the loss, both gradient sets
@pytest.mark.parametrize("cid", [c[0] for c in W.CASES])
def test_one_minibatch_against_the_float64_restatement(cid):
    _one_minibatch(cid)


def _one_minibatch(cid, use_dropout=False, actor_hidden=None, warm=0, launches=None):
    """use_dropout: --use-dropout, the restatement's actor and target actor drawing the masks of forward count `warm` -- `warm` training
    calls on the same rows run first and the parameters are put back behind them (plain gradient descent only: no slots, no noise count).
    actor_hidden: --actor-hidden-layers.  launches: {kernel family: count} the checked minibatch, profiled, must show."""
    case = W.case_of(cid)
    _c, shape_name, A, B, opt, d, sm, _clip, _tau = case
    plain_kw, agent_kw = {}, {}
    if use_dropout:
        plain_kw, agent_kw = dict(dropout=True, drop_count=warm), dict(use_dropout=True)
    if actor_hidden is not None:
        plain_kw["actor_hidden"] = actor_hidden
        agent_kw["actor_hidden_layers"] = ",".join(str(int(h)) for h in actor_hidden)
    inputs = W.case_inputs(case, **plain_kw)
    specs, P, _ep, idxs, batches = inputs
    weighted = "weighted" in cid
    assert warm == 0 or (opt == "gradient-descent" and sm is None and d == 1 and not weighted)
    agent = _case_agent(case, inputs, **agent_kw)
    try:
        if weighted:
            _set_priorities(agent)
        for _ in range(warm):
            agent.train_step(B, 1, idxs=idxs[:B])
        if warm:
            for net, p in zip(agent.networks(), P):
                net.set_params(p)
        seen = _profiled_calls(agent.actor.ctx, lambda: agent.train_step(B, 1, idxs=idxs[:B])) if launches is not None else \
            agent.train_step(B, 1, idxs=idxs[:B])
        if launches is not None:
            assert {k: seen.get(k, 0) for k in launches} == launches, seen
        actions, dq_da, q1, td1 = agent.trainer.last_values(B)
        q2, tq1, tq2, td2 = agent.trainer.last_twin_values(B)
        stats = agent.trainer.last_stats()
        g_a, g_c = agent.actor.get_grads(), agent.critic.get_grads()
        w = agent.replay_memory.last_weights(B).astype(np.float64).reshape(B, 1) if weighted else None
    finally:
        agent.close()
    ref = W.restatement(specs, P, np.float64, W.hyper_of(case), opt, d, sm)
    set_actor_masks(ref, B, warm)
    ag = ref.actor_gradients(batches[0][0])
    cg = ref.critic_gradients(batches[0], w=w)
    if weighted:
        assert w.min() < 0.9 and abs(w.max() - 1.0) < 1e-6, w.ravel()
    share = ref.min_share[-1]
    assert W.MIN_SHARE <= share <= 1 - W.MIN_SHARE, share
    atol = 1e-5
    bar = W.td_bar(ref.hp.discount, sm[0], cg, atol) if sm is not None else atol
    err = {"actions": np.abs(actions - ag["actions"]).max(), "dq_da": np.abs(dq_da - ag["dq_da"]).max(), "q1": np.abs(q1 - cg["q"]).max(),
           "q2": np.abs(q2 - cg["q2"]).max(), "tq1": np.abs(tq1 - cg["target_q"]).max(), "tq2": np.abs(tq2 - cg["target_q2"]).max(),
           "td1": np.abs(td1 - cg["td"]).max(), "td2": np.abs(td2 - cg["td2"]).max(), "loss": abs(float(stats[0]) - float(cg["loss"]))}
    print("%s: %s; TD bar %.3e; min(Q1', Q2') is head 1's on %.2f of the rows" % (cid, {k: "%.2e" % v for k, v in err.items()}, bar, share))
    for k in ("actions", "dq_da", "q1", "q2"):
        assert err[k] < atol, (k, err)
    for k in ("tq1", "tq2", "td1", "td2", "loss"):
        assert err[k] < bar, (k, err, bar)
    assert np.abs(q1 - q2).max() > 1e-2 and np.abs(td1 - td2).max() > 1e-2      # (two heads)
    assert_flat_close(specs[0], g_a, ag["grads"], rel=2e-5, what="actor pre-clip grads vs f64 restatement")
    assert len(g_c) == W.num_params(specs[1])
    floor = 2.0 * max(err["td1"], err["td2"])
    try:
        assert_flat_close(W.TwinLayoutSpec(specs[1]), g_c, cg["grads"], rel=2e-5, what="twin critic pre-clip grads vs f64 restatement", abs_floor=floor)
    except AssertionError:
        if sm is None:
            raise
        # (the gradients are linear in the TDs, and the device's noise sits up to Z_BAR * sigma from the restated one: the backward
        # arithmetic alone, at the device's TDs -- tests/test_gpu_target_smoothing.py)
        c = cg["cache_critic"]
        ww = np.ones((B, 1)) if w is None else w
        grads, _ = ref.critic.backward(c, 2.0 * td1.astype(np.float64) * ww / B, 2.0 * td2.astype(np.float64) * ww / B)
        assert_flat_close(W.TwinLayoutSpec(specs[1]), g_c, W.flatten_grads(specs[1], grads, np.float64), rel=2e-5,
                          what="twin critic pre-clip grads vs the restatement's backward pass of the device's TDs", abs_floor=floor)


@pytest.mark.parametrize("actor_hidden,launches", [(None, {"heads": 1, "td": 0}), ([100, 100, 65], {"heads": 0, "td": 1})],
                         ids=["heads_twin-relu_x2", "100-100-65-td_twin_kernel"])
def test_a_minibatch_with_dropout_against_the_float64_restatement(actor_hidden, launches):
    """--use-dropout under twin critics, forward count 1: heads_twin.hip's x2 ReLU gradient into the actor's last hidden layer, and one
    lane past the heads kernel the GEMM x2 epilogue in front of td_twin_kernel; the target actor drops out in both"""
    _one_minibatch("A2-B8-sgd", use_dropout=True, actor_hidden=actor_hidden, warm=1, launches=launches)


# ---- 2. the cases' outer steps: parameters, targets, slots, counts
def _run_outer(case, inputs, **kw):
    cid, _sn, _A, B, opt, d, _sm, _clip, _tau = case
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
        tree = agent.replay_memory.priority_tree() if weighted else None
        td1 = agent.trainer.last_values(B)[3]
    finally:
        agent.close()
    return got, slots, counts, stats, weights or None, tree, td1


@pytest.mark.parametrize("cid", [c[0] for c in W.CASES])
def test_outer_steps_against_the_float64_restatement(cid):
    case = W.case_of(cid)
    opt, d = case[4], case[5]
    inputs = W.case_inputs(case)
    got, slots, counts, stats, weights, _tree, _td = _run_outer(case, inputs)
    want, wcounts, outs, ref = W.run_case(case, inputs, weights=weights)
    assert all(W.MIN_SHARE <= s <= 1 - W.MIN_SHARE for s in ref.min_share), ref.min_share
    na, nc = outs[-1]["actor_norm"], outs[-1]["critic_norm"]
    assert abs(stats[1] - na) < 1e-4 * max(1.0, na) and abs(stats[2] - nc) < 1e-4 * max(1.0, nc), (stats, na, nc)
    assert abs(stats[0] - outs[-1]["loss"]) < 1e-4 * max(1.0, outs[-1]["loss"]), (stats, outs[-1]["loss"])
    if counts is not None:
        assert counts == [int(x) for x in wcounts] == [W.NB // d, W.NB], counts
    _compare(cid, opt, inputs[1], got + slots, want, W.NB)


def _sum_tree_against_the_restatement(case, inputs, rows, w, tree):
    """the whole sum tree behind one twin minibatch -- leaves, every inner node, the total -- against tests.per_np's tree: the priorities
    _set_priorities wrote, then (|td_1| + eps)^alpha of the RESTATEMENT's float64 td_1 on the minibatch's rows (duplicate rule: the last
    occurrence).  A leaf may sit as far from the restated one as a td 1e-5 away (the suite's bar on td) moves it, plus 4 ulps of f32 for
    the device's powf; an inner node the sum of its leaves' allowances.  The tree rebuilt from td_2 must leave that allowance."""
    from tests import per_np as PN
    specs, P, _ep, _idxs, batches = inputs
    B = case[3]
    ref = W.restatement(specs, P, np.float64, W.hyper_of(case), case[4], case[5], case[6])
    cg = ref.critic_gradients(batches[0], w=w)
    L = PN.levels(W.ROWS)
    assert len(tree) == 2 << L
    start = PN.priority(np.random.default_rng(9).lognormal(0.0, 1.0, W.ROWS).astype(np.float32), 0.6, 1e-6).astype(np.float64)

    def rebuilt(td):
        a = np.abs(np.asarray(td, np.float64).ravel())
        t = PN.write(PN.build(start, L), L, rows, PN.priority(a, 0.6, 1e-6))
        leaf_tol = 4 * 2.0 ** -23 * t[1 << L:(1 << L) + W.ROWS].copy()
        last = {int(r): k for k, r in enumerate(rows)}
        for r, k in last.items():
            hi, lo = PN.priority(a[k] + 1e-5, 0.6, 1e-6), PN.priority(max(a[k] - 1e-5, 0.0), 0.6, 1e-6)
            leaf_tol[r] += float(hi) - float(lo)
        return t, PN.build(leaf_tol, L)
    want, tol = rebuilt(cg["td"])
    err = np.abs(tree - want)
    print("sum tree: total %.6f (restated %.6f), largest |err| / allowance %.3f over %d nodes" %
          (tree[1], want[1], float((err[1:] / np.maximum(tol[1:], 1e-300))[tol[1:] > 0].max()), len(tree) - 1))
    assert tree[0] == 0 and (err <= tol).all(), (np.flatnonzero(err > tol), err.max())
    other, _t = rebuilt(cg["td2"])
    assert (np.abs(tree - other) > tol).any() and abs(tree[1] - other[1]) > tol[1]


def test_priorities_come_from_td_1():
    """a prioritized memory's leaves behind a twin minibatch are (|td_1| + eps)^alpha of its rows: the restated values of head 1's TD, and
    not head 2's"""
    case = W.case_of("A2-B7-weighted")
    B = case[3]
    inputs = W.case_inputs(case)
    lib, check, ptr = _abi()
    agent = _case_agent(case, inputs)
    try:
        _set_priorities(agent)
        rows = np.ascontiguousarray(inputs[3][:B], dtype=np.int32)
        agent.train_step(B, 1, idxs=rows)
        td1 = agent.trainer.last_values(B)[3].ravel().astype(np.float64)
        td2 = agent.trainer.last_twin_values(B)[3].ravel().astype(np.float64)
        pri = np.empty(B, np.float32)
        check(lib.cpp_replay_read_priorities(agent.replay_memory.handle, ptr(rows), B, ptr(pri)))
        tree = agent.replay_memory.priority_tree()
        w = agent.replay_memory.last_weights(B).astype(np.float64).reshape(B, 1)
    finally:
        agent.close()
    _sum_tree_against_the_restatement(case, inputs, rows, w, tree)
    want1, want2 = (np.abs(td1) + 1e-6) ** 0.6, (np.abs(td2) + 1e-6) ** 0.6
    # (a row drawn twice keeps the value of one of its occurrences)
    ok1 = [any(abs(pri[i] - want1[j]) <= 1e-5 * max(1.0, want1[j]) for j in range(B) if rows[j] == rows[i]) for i in range(B)]
    ok2 = [any(abs(pri[i] - want2[j]) <= 1e-5 * max(1.0, want2[j]) for j in range(B) if rows[j] == rows[i]) for i in range(B)]
    assert all(ok1) and not all(ok2), (pri, want1, want2)


# ---- 3. graph replays on the rows the device draws: TD3 whole through one graph
def test_graph_replays_against_the_float64_restatement():
    """five outer steps of three minibatches: the eager pass and the capture, then FOUR replays -- 4 x 3 minibatches through one graph"""
    case, nb, steps, sample_seed = W.GRAPH_CASE
    assert steps - 1 >= 4 and nb >= 3
    cid, _sn, _A, B, opt, d, _sm, _clip, _tau = case
    lib, check, ptr = _abi()
    inputs = W.graph_inputs()
    agent = _case_agent(case, inputs, sample_seed=sample_seed)
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


def test_three_identical_runs_are_bit_identical():
    case, nb, _steps, sample_seed = W.GRAPH_CASE
    B = case[3]
    inputs = W.graph_inputs()
    runs = []
    for _k in range(3):
        agent = _case_agent(case, inputs, sample_seed=sample_seed)
        try:
            for _s in range(3):                       # eager pass + capture, two replays
                agent.train_step(B, nb)
            runs.append(_params(agent) + _slots(agent)[0] + [np.concatenate(agent.trainer.last_twin_values(B))])
        finally:
            agent.close()
    for other in runs[1:]:
        assert all(np.array_equal(x, y) for x, y in zip(runs[0], other))


# ---- 4. the reference's loop on host arrays: the stand-alone train ops (cpp_ddpg_train_actor, cpp_ddpg_train_critic) and the targets' own launches
@pytest.mark.parametrize("cid", ["A2-B8-sgd", "A4-B8-smoothed", "lowdim-A3-B16-td3"])
def test_the_literal_loop_on_host_arrays(cid):
    case = W.case_of(cid)
    _c, _sn, _A, B, opt, d, sm, _clip, _tau = case
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
    ref = W.restatement(specs, P, np.float64, W.hyper_of(case), opt, d, sm)
    for b in batches:
        ref.train_actor(b[0])
        ref.train_critic(b)
        ref.update_targets()
    assert all(W.MIN_SHARE <= s <= 1 - W.MIN_SHARE for s in ref.min_share[:1]), ref.min_share
    if counts is not None:
        assert counts == [int(x) for x in ref.state()["step"]], counts
    _compare(cid + "-literal", opt, P, got + slots, W.vectors(ref), len(batches))


def test_the_paired_literal_loop_is_the_fused_step_bit_for_bit():
    """the reference's loop on device-resident batches, as tests/test_gpu_literal_loop.py pairs it: actor.train(batch.state_1);
    critic.train(batch) run as ONE cpp_ddpg_train_rows (the twin heads launch), both target updates behind them -- against
    train_step(B, 1, idxs) on the same rows, per minibatch, to the bit; TD3 whole (Adam, smoothing, d = 2), four outer steps"""
    case, _nb, _steps, _ss = W.GRAPH_CASE
    B, d = case[3], case[5]
    inputs = W.graph_inputs()
    lit, fused = _case_agent(case, inputs), _case_agent(case, inputs)
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
            for a, b in zip(_params(lit), _params(fused)):
                assert np.array_equal(a, b), step
            for a, b in zip(lit.trainer.last_twin_values(B) + lit.trainer.last_values(B), fused.trainer.last_twin_values(B) + fused.trainer.last_values(B)):
                assert np.array_equal(a, b), step
            assert np.array_equal(lit.trainer.last_stats(), fused.trainer.last_stats())
            assert lit.trainer.policy_delay_status() == fused.trainer.policy_delay_status() == (d, step, step % d != 0)
        assert lit.trainer.fused_pairs == 4 and fused.trainer.fused_pairs == 0
        (sl, tl), (sf, tf) = _slots(lit), _slots(fused)
        assert tl == tf == [2, 4] and np.array_equal(sl[0], sf[0]) and np.array_equal(sl[1], sf[1])
        assert np.abs(lit.trainer.last_twin_values(B)[0] - lit.trainer.last_values(B)[2]).max() > 1e-2      # (two heads)
    finally:
        lit.close(); fused.close()


# ---- 4b. the layout the device reports
@pytest.mark.parametrize("cid", ["A2-B8-sgd", "lowdim-A3-B16-td3"])
def test_the_prefix_of_the_device_layout_is_the_plain_critics(cid):
    """cpp_net_var_info of a twin critic: the plain critic's variables first -- names, shapes, offsets --, then the twin variables in
    creation order, contiguous; cpp_net_num_params the restated figure"""
    case = W.case_of(cid)
    _c, shape_name, A, B, _opt, _d, _sm, _clip, _tau = case
    specs = W.case_inputs(case)[0]
    layouts = {}
    for twin in (False, True):
        agent = _build(W.SHAPES[shape_name], B, A, W.hyper_of(case), twin=twin)
        try:
            layouts[twin] = [[(v.name.split("/", 1)[1], tuple(v.shape), int(v.offset)) for v in net.trainable_model_vars()] + [net.num_params]
                             for net in (agent.critic, agent.target_critic)]
            if twin:
                assert agent.actor.num_params == specs[0].num_params()
        finally:
            agent.close()
    for plain, twin in zip(layouts[False], layouts[True]):
        n_plain, n_twin = plain.pop(), twin.pop()
        assert twin[:len(plain)] == plain and n_plain == specs[1].num_params() and n_twin == W.num_params(specs[1])
        off = n_plain
        for (name, shape, offset), (wname, wshape) in zip(twin[len(plain):], W.twin_layout(specs[1])):
            assert (name, shape, offset) == (wname + ":0", tuple(wshape), off), (name, shape, offset, wname, wshape, off)
            off += int(np.prod(shape))
        assert off == n_twin and len(twin) - len(plain) == len(W.twin_layout(specs[1]))
    if shape_name != "lowdim":
        assert W.num_params(specs[1]) - specs[1].num_params() == (50 + A + 1) * 50 + 51


# ---- 4c. n-step returns and random shift: they change the gathered minibatch, below everything twin
def _one_replay_feature(what, prepare, shift=False):
    """twin heads with a replay feature on, one minibatch per call on device-drawn rows: two warm calls, the q_valueb biases shifted by the
    median of Q1' - Q2' on the rows of the next draw (so that both heads take their share of the min), then the checked
    minibatch rebuilt on the host as tests/test_gpu_policy_delay.py rebuilds its own -- the rows read back, the feature's restatement
    of the minibatch, the float64 restatement on the device's routes: every per-row value at 1e-5, both updated parameter vectors at
    tests.ddpg_opt_np's bound, the targets at f32 rounding of their soft update.  The float32 evaluation of the same update must itself
    sit inside the bound (else the case is void, not the device wrong)."""
    from tests.helpers import delta_bound, device_pool_codes, device_relu_active
    from tests.test_gpu_random_shift import _shifted_minibatch
    lib, check, ptr = _abi()
    shape, B, A, rows = (32, 32, 3, 2, 3), 32, 2, 300
    hp = T3.hyper_of("gradient-descent", 0.5, 0.25)
    agent = _build(shape, B, A, hp, rows=rows + 50, seed=4)
    kw = dict(pixel=True, H=shape[0], W=shape[1], C=int(np.prod(shape[2:])))
    specs = (O.NetSpec("actor", A, [100, 100, 50], **kw), O.NetSpec("critic", A, [100, 100, 50], **kw))
    try:
        rng = np.random.default_rng(104)
        for net, sd in ((agent.actor, 0.05), (agent.critic, 0.05), (agent.target_actor, 0.01), (agent.target_critic, 0.01)):
            p = net.get_params()
            net.set_params(p + rng.normal(0, sd, p.shape).astype(np.float32))
        rm = agent.replay_memory
        rm.fill_synthetic(rows, seed=25)
        prepare(agent)
        agent.train_step(B, 1)
        agent.train_step(B, 1)
        # the rows of the next draw are known (sample seed 0, the sampler's counter = the minibatch's number): the shift from the float64
        # restatement's two target heads on that minibatch as the memory folds it (unshifted pixels: an estimate of the median is enough)
        nxt = T3.device_rows(0, 2, B, rows)
        hb = rm.batch(idxs=nxt)
        est = W.restatement(specs, _params(agent), np.float64, hp)
        cg0 = est.critic_gradients((rm.state[hb.state_1_idx], hb.action, hb.reward, hb.terminal_mask, rm.state[hb.state_2_idx]))
        shift_q = np.float32(np.median(cg0["target_q"] - cg0["target_q2"]))
        for net in (agent.critic, agent.target_critic):
            p = net.get_params()
            p[-1] += shift_q
            net.set_params(p)
        P = _params(agent)
        agent.train_step(B, 1)
        idxs = np.empty(B, np.int32)
        check(lib.cpp_replay_last_indexes(rm.handle, B, ptr(idxs)))
        assert np.array_equal(idxs, nxt)
        codes = (device_pool_codes(agent.actor, B), device_pool_codes(agent.critic, B))
        relus = (device_relu_active(agent.actor, B), device_relu_active(agent.critic, B))
        if shift:
            t, _un, _sh = _shifted_minibatch(rm, idxs)
        else:
            hb = rm.batch(idxs=idxs)
            t = (rm.state[hb.state_1_idx], hb.action, hb.reward, hb.terminal_mask, rm.state[hb.state_2_idx])
        got = _params(agent)
        _a, dq_da, q1, td1 = agent.trainer.last_values(B)
        q2, tq1, tq2, td2 = agent.trainer.last_twin_values(B)
        loss = float(agent.trainer.last_stats()[0])
    finally:
        agent.close()
    upd = {}
    for dt in (np.float64, np.float32):
        ref = W.restatement(specs, P, dt, hp)
        ref.actor.amax_override, ref.critic.amax_override = codes
        ref.actor.relu_override, ref.critic.relu_override = relus
        ag, cg = ref.actor_gradients(t[0]), ref.critic_gradients(t)
        if dt is np.float64:
            share = ref.min_share[-1]
            err = {"dq_da": np.abs(dq_da - ag["dq_da"]).max(), "q1": np.abs(q1 - cg["q"]).max(), "q2": np.abs(q2 - cg["q2"]).max(),
                   "tq1": np.abs(tq1 - cg["target_q"]).max(), "tq2": np.abs(tq2 - cg["target_q2"]).max(), "td1": np.abs(td1 - cg["td"]).max(),
                   "td2": np.abs(td2 - cg["td2"]).max(), "loss": abs(loss - float(cg["loss"]))}
        ref._apply("actor", ag["grads"])
        ref._apply("critic", cg["grads"])
        upd[dt] = [np.asarray(ref.actor.flat(), np.float64), np.asarray(ref.critic.flat(), np.float64)]
    print("%s: %s; min(Q1', Q2') is head 1's on %.2f of the rows" % (what, {k: "%.2e" % v for k, v in err.items()}, share))
    assert W.MIN_SHARE <= share <= 1 - W.MIN_SHARE, share
    assert max(err.values()) < 1e-5, err
    bad = []
    for nm, g, w_, tw, p in zip(("actor", "critic"), got[:2], upd[np.float64], upd[np.float32], P[:2]):
        bound = delta_bound(p, w_ - p, R.R[nm], 1)
        e_twin, e = float(np.linalg.norm(tw - w_)), float(np.linalg.norm(np.asarray(g, np.float64) - w_))
        print("  %s %-7s |err| %.3e  float32 evaluation %.3e  bound %.3e" % (what, nm, e, e_twin, bound))
        assert e_twin <= bound, "the float32 evaluation of this update leaves the bound itself: the case is void (%s %s)" % (what, nm)
        if not e <= bound:
            bad.append((nm, e, bound))
    assert not bad, (what, bad)
    for j in (0, 1):
        wt = O.soft_update(P[2 + j], got[j], hp.target_update_rate, np.float64)
        assert float(np.linalg.norm(got[2 + j] - wt)) <= 2.0 ** -23 * float(np.linalg.norm(wt)), (what, "target", j)
    return t


def test_with_n_step_returns():
    from cartpoleplusplus_amd import ddpg_cartpole as D
    t = _one_replay_feature("n-step", lambda a: a.replay_memory.enable_n_step(3, D.opts.discount))
    m = np.asarray(t[3]).ravel()
    assert ((m > 0) & (m < 1)).any()                            # (folded masks: discount^2 on the rows whose walk took three steps)


def test_with_random_shift():
    _one_replay_feature("random-shift", lambda a: a.replay_memory.enable_random_shift(4, seed=11), shift=True)


# ---- 5. the readers
def test_check_loss_forward_and_dq_da_are_head_1s():
    case = W.case_of("A4-B8-smoothed")
    _c, _sn, A, B, opt, d, sm, _clip, _tau = case
    inputs = W.case_inputs(case)
    specs, P, _ep, _idxs, batches = inputs
    lib, check, ptr = _abi()
    agent = _case_agent(case, inputs)
    try:
        hb = HostBatch(*batches[0])
        loss, td, q = agent.critic.check_loss(hb)
        assert agent.trainer.last_target_noise(B)[1] == 0              # (an evaluation: no draw, no count)
        q_fwd = agent.critic.forward(hb.state_1, hb.action)
        dq = agent.critic.q_gradients_wrt_actions(hb)
        before = _params(agent)
        assert all(np.array_equal(x, y) for x, y in zip(before, _params(agent)))
        assert lib.cpp_net_is_twin_q(agent.critic.handle) == 1 and lib.cpp_net_is_twin_q(agent.target_critic.handle) == 1
        assert lib.cpp_net_is_twin_q(agent.actor.handle) == 0 and lib.cpp_net_is_twin_q(None) == 0
        names = [v.name for v in agent.critic.trainable_model_vars()]
    finally:
        agent.close()
    assert names[-4:] == ["critic/hidden3b/weights:0", "critic/hidden3b/biases:0", "critic/q_valueb/weights:0", "critic/q_valueb/biases:0"]
    ref = W.restatement(specs, P, np.float64, W.hyper_of(case), opt, d, sm)
    wl, wtd, wq = ref.check_loss(batches[0])
    err = (abs(loss - wl), np.abs(td - wtd).max(), np.abs(q - wq).max())
    print("check_loss: |loss| %.2e |td| %.2e |q| %.2e" % err)
    assert max(err) < 1e-5
    cg = ref.last_cg
    assert abs(wl - float(np.mean(cg["td"] ** 2 + cg["td2"] ** 2))) < 1e-12 and abs(wl - float(np.mean(cg["td"] ** 2))) > 1e-3
    # CriticNetwork.forward is inference mode on its own batch statistics: head 1 of the restatement
    c = ref.critic.forward(hb.state_1, action=hb.action, training=False)
    assert np.abs(q_fwd - c["out"]).max() < 1e-5 and np.abs(q_fwd - c["out2"]).max() > 1e-2
    ag = ref.actor_gradients(hb.state_1)
    assert np.abs(dq - ag["dq_da"]).max() < 1e-5
    assert np.abs(dq - ref.critic.d_action(ref.critic.forward(hb.state_1, action=ag["actions"]), 2)).max() > 1e-3


def test_a_checkpoint_round_trip_and_a_plain_checkpoint_is_refused(tmp_path):
    from cartpoleplusplus_amd import util
    case = W.case_of("A8-B7-adam")
    B = case[3]
    inputs = W.case_inputs(case)
    agent = _case_agent(case, inputs)
    try:
        agent.train_step(B, 2, idxs=inputs[3][:2 * B])
        saver = util.SaverUtil(agent, str(tmp_path / "twin"), 3600)
        saver.force_save()
        want = _params(agent) + _slots(agent)[0]
    finally:
        agent.close()
    agent = _case_agent(case, (inputs[0], None, None, None, None), seed=7)
    try:
        assert not np.array_equal(agent.critic.get_params(), want[1])
        util.SaverUtil(agent, str(tmp_path / "twin"), 3600)
        got = _params(agent) + _slots(agent)[0]
        assert all(np.array_equal(x, y) for x, y in zip(got, want))
    finally:
        agent.close()
    plain = _case_agent(case, (inputs[0], None, None, None, None), twin=False)
    try:
        util.SaverUtil(plain, str(tmp_path / "plain"), 3600).force_save()
        with pytest.raises(AssertionError, match="checkpoint does not match critic"):
            util.SaverUtil(plain, str(tmp_path / "twin"), 3600)
    finally:
        plain.close()
    agent = _case_agent(case, (inputs[0], None, None, None, None))
    try:
        with pytest.raises(AssertionError, match="checkpoint does not match critic"):      # (the four extra variables are missing)
            util.SaverUtil(agent, str(tmp_path / "plain"), 3600)
    finally:
        agent.close()


# ---- 6. the data-parallel step as a world of one
def test_the_data_parallel_step_as_a_world_of_one():
    case, nb, _steps, sample_seed = W.GRAPH_CASE
    cid, _sn, _A, B, opt, d, _sm, _clip, _tau = case
    lib, check, ptr = _abi()
    inputs = W.graph_inputs()
    steps = 2
    agent = _case_agent(case, inputs, sample_seed=sample_seed)
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


# ---- 7. compositions: the 8-bit store (the cases' frames are pixel codes: the same minibatches), batch norm
def test_the_eight_bit_store_changes_nothing():
    case = W.case_of("A2-B8-32x32x6-td3")
    inputs = W.case_inputs(case)
    a = _run_outer(case, inputs)
    b = _run_outer(case, inputs, replay_store="u8")
    want, _wc, _outs, _ref = W.run_case(case, inputs)
    _compare(case[0] + "-u8", case[4], inputs[1], b[0] + b[1], want, W.NB)
    assert np.array_equal(a[6], b[6]) or np.abs(a[6] - b[6]).max() < 1e-5


@pytest.mark.parametrize("B", [5, 56])
def test_batch_norm_composes(B):
    """--use-batch-norm with twin heads, one minibatch (batch statistics of the four trunks) at the batch-norm suite's small and large
    batch: per-row values at its bars"""
    shape, A, rows = (16, 16, 3, 1, 2), 2, 64          # (six channels: the batch-norm kernels' dense dW rows come in 16-byte chunks)
    specs, P, episodes, idxs, batches = W.host_case(shape, B, 1, 3, rows=rows, action_dim=A, batch_norm=True)
    hp = T3.hyper_of("gradient-descent", 0.5, 0.25)
    agent = _build(shape, B, A, hp, P, episodes, rows=rows, use_batch_norm=True)
    try:
        agent.train_step(B, 1, idxs=idxs[:B])
        _actions, dq_da, q1, td1 = agent.trainer.last_values(B)
        q2, tq1, tq2, td2 = agent.trainer.last_twin_values(B)
        loss = float(agent.trainer.last_stats()[0])
    finally:
        agent.close()
    ref = W.restatement(specs, P, np.float64, hp)
    ag, cg = ref.actor_gradients(batches[0][0]), ref.critic_gradients(batches[0])
    err = {"dq_da": np.abs(dq_da - ag["dq_da"]).max(), "q1": np.abs(q1 - cg["q"]).max(), "q2": np.abs(q2 - cg["q2"]).max(),
           "tq1": np.abs(tq1 - cg["target_q"]).max(), "tq2": np.abs(tq2 - cg["target_q2"]).max(), "td1": np.abs(td1 - cg["td"]).max(),
           "td2": np.abs(td2 - cg["td2"]).max(), "loss": abs(loss - float(cg["loss"]))}
    print("batch norm B=%d: %s" % (B, {k: "%.2e" % v for k, v in err.items()}))
    assert max(err.values()) < 2e-5, err          # (tests/test_gpu_batchnorm.py's bar for values behind batch statistics)


# ---- 8. off means off
_PLAIN_SNIPPET = r"""
import hashlib, json, sys
import numpy as np
sys.path.insert(0, %(root)r)
from tests import test_gpu_twin_q as G
print("RESULT " + json.dumps(G._plain_run(%(twin_first)r)))
"""


def _plain_run(twin_first):
    """two graph-replayed outer steps of a PLAIN trainer (after a twin one has lived and died in the process, if asked): the digest of its
    parameters and slots, and the launch census of one more outer step"""
    case, nb, _steps, sample_seed = W.GRAPH_CASE
    B = case[3]
    inputs = W.graph_inputs()
    n1 = inputs[0][1].num_params()
    plain_inputs = (inputs[0], [inputs[1][0], inputs[1][1][:n1], inputs[1][2], inputs[1][3][:n1]], inputs[2], None, None)
    if twin_first:
        agent = _case_agent(case, inputs, sample_seed=sample_seed)
        try:
            agent.train_step(B, nb)
            agent.train_step(B, nb)
        finally:
            agent.close()
    agent = _case_agent(case, plain_inputs, sample_seed=sample_seed, twin=False)
    try:
        lib, _check, _ptr = _abi()
        assert lib.cpp_net_is_twin_q(agent.critic.handle) == 0
        for _s in range(3):
            agent.train_step(B, nb)
        h = hashlib.sha256()
        for x in _params(agent) + _slots(agent)[0]:
            h.update(np.ascontiguousarray(x).tobytes())
        census = _profiled_calls(agent.actor.ctx, lambda: agent.train_step(B, nb))
    finally:
        agent.close()
    return {"digest": h.hexdigest(), "census": census}


def test_off_means_off():
    """a plain trainer created after a twin one in the same process ends with the bits, and launches the kernels, of one in a process
    that never made a twin"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = subprocess.run([sys.executable, "-c", _PLAIN_SNIPPET % dict(root=root, twin_first=False)], cwd=root, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    fresh = json.loads([l for l in out.stdout.splitlines() if l.startswith("RESULT ")][0][len("RESULT "):])
    here = _plain_run(True)
    assert here["census"] == fresh["census"], (here["census"], fresh["census"])
    assert here["digest"] == fresh["digest"]
    assert here["census"].get("heads", 0) == W.GRAPH_CASE[1]          # (the plain pixel trainer keeps the fused heads launch)


# ---- 8b. the launches: a twin outer step is the plain step's, kernel id by kernel id; which kernel ran the heads
def _census(twin, nb=3):
    case, _nb, _steps, sample_seed = W.GRAPH_CASE
    B = case[3]
    inputs = W.graph_inputs()
    if not twin:
        n1 = inputs[0][1].num_params()
        inputs = (inputs[0], [inputs[1][0], inputs[1][1][:n1], inputs[1][2], inputs[1][3][:n1]], inputs[2], None, None)
    agent = _case_agent(case, inputs, sample_seed=sample_seed, twin=twin)
    try:
        agent.train_step(B, nb)
        return _profiled_calls(agent.actor.ctx, lambda: agent.train_step(B, nb))
    finally:
        agent.close()


def test_the_launch_census_of_a_twin_outer_step_is_the_plain_steps():
    plain, twin = _census(False), _census(True)
    print("launches per outer step:", twin)
    assert twin == plain, (twin, plain)
    assert twin.get("heads", 0) == 3 and twin.get("td", 0) == 0


@pytest.mark.parametrize("cid,heads", [("A1-B5-sgd", 1), ("A3-B7-momentum", 1), ("A5-B5-smoothed", 1), ("A8-B7-adam", 1), ("A2-B7-weighted", 1),
                                       ("A9-B8-sgd", 0), ("lowdim-A3-B16-td3", 0)])
def test_which_kernel_runs_the_twin_heads(cid, heads):
    """the fused heads launch up to eight action components (the weighted, smoothed and padded instances among them), the GEMM levels
    with td_twin_kernel past it and for a low-dimensional critic"""
    case = W.case_of(cid)
    B = case[3]
    inputs = W.case_inputs(case)
    agent = _case_agent(case, inputs)
    try:
        if "weighted" in cid:
            _set_priorities(agent)
        n = _profiled_calls(agent.actor.ctx, lambda: agent.train_step(B, 1, idxs=inputs[3][:B]))
    finally:
        agent.close()
    assert n.get("heads", 0) == heads and n.get("td", 0) == 1 - heads, n


@pytest.mark.parametrize("switch", ["CPP_FUSED_HEADS", "CPP_HEADS_PRE"])
def test_the_gemm_levels_hold_the_same_cases_when_selected(switch):
    """the ablation library with CPP_FUSED_HEADS=0 (twin heads as GEMM levels + td_twin_kernel at the widths the heads kernel covers) and
    CPP_HEADS_PRE=0 (the actors' last hidden layer outside it): the one-minibatch cases of this module at the same bars"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, CARTPOLEPP_ABLATION="1")
    env[switch] = "0"
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.join(root, "tests", "test_gpu_twin_q.py"), "-q", "-x", "-m", "gpu", "-p", "no:cacheprovider",
                        "-k", "one_minibatch and (A2-B8-sgd or A4-B5-weighted-smoothed or A8-B7-adam or A5-B5-smoothed)"],
                       cwd=root, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=600)
    tail = r.stdout.decode()[-1500:]
    assert r.returncode == 0 and "4 passed" in tail, tail


# ---- 9. the refusals
def test_the_refusals():
    from cartpoleplusplus_amd import _lib
    lib, check, ptr = _abi()
    case = W.case_of("A2-B8-sgd")
    inputs = W.case_inputs(case)
    twin = _case_agent(case, inputs)
    try:
        plain = _build(W.SHAPES["16x16x3"], 8, 2, W.hyper_of(case), twin=False)
        try:
            hp = _lib.DdpgHyper(1e-3, 1e-2, 0.9, 5.0, 0.1)
            h = ctypes.c_void_p()
            # mixed plain / twin critic and target, both ways
            for critic, target in ((twin.critic, plain.target_critic), (plain.critic, twin.target_critic)):
                rc = lib.cpp_ddpg_create(twin.actor.ctx.handle, plain.actor.handle, critic.handle, plain.target_actor.handle, target.handle,
                                         ctypes.byref(hp), ctypes.byref(h))
                assert rc == CPP_ERR_ARG and b"twin" in lib.cpp_last_error(), (rc, lib.cpp_last_error())
            # a twin actor cannot be made ...
            spec = _lib.NetSpec()
            ctypes.memmove(ctypes.byref(spec), ctypes.byref(twin.actor.spec), ctypes.sizeof(spec))
            rc = lib.cpp_net_create_twin_q(twin.actor.ctx.handle, ctypes.byref(spec), 8, ctypes.byref(h))
            assert rc == CPP_ERR_ARG and b"cpp_net_create_twin_q" in lib.cpp_last_error()
            # ... and a twin critic in an actor's place is refused
            rc = lib.cpp_ddpg_create(twin.actor.ctx.handle, twin.critic.handle, twin.critic.handle, plain.target_actor.handle,
                                     twin.target_critic.handle, ctypes.byref(hp), ctypes.byref(h))
            assert rc == CPP_ERR_ARG
            # NAF refuses twin networks
            nh = _lib.NafHyper(0.9, 5.0, 0.1, 0, 1e-3, 0.0, 0.9, 0.999, 1e-8)
            rc = lib.cpp_naf_create(twin.actor.ctx.handle, twin.critic.handle, twin.target_critic.handle, twin.critic.handle, twin.critic.handle,
                                    0, ctypes.byref(nh), ctypes.byref(h))
            assert rc == CPP_ERR_ARG and b"twin" in lib.cpp_last_error()
            # the twin read-back on a plain trainer
            buf = np.empty(8, np.float32)
            rc = lib.cpp_ddpg_last_twin_values(plain.trainer.handle, 8, ptr(buf), None, None, None)
            assert rc == CPP_ERR_STATE and b"cpp_ddpg_last_twin_values" in lib.cpp_last_error()
            assert lib.cpp_ddpg_last_twin_values(None, 8, None, None, None, None) == CPP_ERR_ARG
            assert lib.cpp_ddpg_last_twin_values(twin.trainer.handle, 9, None, None, None, None) == CPP_ERR_ARG
        finally:
            plain.close()
    finally:
        twin.close()


def test_td3_trains_through_main(tmp_path, capsys):
    """--twin-q --target-policy-noise 0.2 --policy-delay 2 --ddpg-optimiser Adam through ddpg_cartpole.main on the stand-in environment"""
    from cartpoleplusplus_amd import ddpg_cartpole as D
    D.main(["--synthetic-env", "--use-raw-pixels", "--render-width", "16", "--render-height", "16", "--max-episode-len", "12", "--batch-size", "8",
            "--batches-per-step", "2", "--replay-memory-size", "200", "--replay-memory-burn-in", "20", "--max-num-actions", "60", "--twin-q",
            "--target-policy-noise", "0.2", "--policy-delay", "2", "--ddpg-optimiser", "Adam"])
    out = capsys.readouterr()
    stats = [l for l in out.out.splitlines() if l.startswith("STATS")]
    assert stats and "hidden3b" in out.err and "q_valueb" in out.err
