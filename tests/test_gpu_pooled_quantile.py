"""Pooled twin quantile critics on the device (--pooled-quantile-critics; cpp_net_create_pooled_quantile: csrc/quant_pool.hip on the GEMM
levels of the gradient pass), also under soft actor-critic, against the float64 restatement tests/pool_np.py.  The cases, their bars and
what they can see are that module's and tests/test_pooled_quantile_host.py's: every compared minibatch pools differently from per-head
truncation on a quarter of its rows, takes a quarter of the kept atoms from each target head and puts a tenth of each head's u on either
side of kappa; the float32 twin stays inside the bars used here, and every planted fault leaves one by more than ten times.

Every minibatch is compared from a common start: the restatement takes over the device's state before it and is fed the device's own
noise (itself held to the restated draw), importance weights and pool / ReLU routes.  Bars: the rows at tests.pool_np.bar(...) -- the
float32 twin's worst error against float64 over these cases times 8, the suite's 1e-5 where that is below a quarter of it --; lists,
norms, deltas, slots, counts and the temperature at tests.sac_np.ratios' and tests.ddpg_opt_np's, unchanged."""
import collections
import ctypes
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import pool_np as P
from tests import sac_np as S
from tests import td3_np as T3
from tests import tps_np as T
from tests.helpers import (FakeEnv, _profiled_calls, device_pool_codes, device_relu_active, hyper_options, make_opts, pool_flips_are_near_ties,
                           relu_flips_are_at_the_boundary)

pytestmark = pytest.mark.gpu
CPP_ERR_ARG, CPP_ERR_STATE = 1, 3          # include/cartpolepp_abi.h
HostBatch = collections.namedtuple("HostBatch", "state_1 action reward terminal_mask state_2")
HIDDEN = ",".join(str(h) for h in P.HIDDEN)
GRAPH_SAMPLE_SEED = 0


def _abi():
    from cartpoleplusplus_amd._lib import lib, check, ptr
    return lib, check, ptr


def _build(shape, B, A, hp, pool, P_=None, episodes=None, rows=P.ROWS, seed=1, **kw):
    """a device agent (pooled quantile critics unless pool is None; pool: (N, kappa, d per head)) with hidden widths 8"""
    from cartpoleplusplus_amd import ddpg_cartpole as D
    pixel = len(shape) == 5
    if pool is not None:
        kw = dict(kw, pooled_quantile_critics=True, pooled_num_quantiles=pool[0], pooled_huber_kappa=pool[1], pooled_drop_per_head=pool[2])
    kw.setdefault("actor_hidden_layers", HIDDEN)
    kw.setdefault("critic_hidden_layers", HIDDEN)
    make_opts(D, shape, B, pixel, replay_memory_size=rows, **dict(hyper_options(hp), **kw))
    agent = D.DeepDeterministicPolicyGradientAgent(FakeEnv(shape, A))
    try:
        agent.initialise_variables(seed=seed)
        agent.post_var_init_setup()
        if P_ is not None:
            for net, p in zip(agent.networks(), P_):
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
    if case[1] == "sac":
        kw.update(soft_actor_critic=True, sac_init_temperature=P.TEMPERATURE, sac_temperature_learning_rate=P.TEMPERATURE_LR, sac_seed=P.NOISE_SEED)
    if case[11] > 1:
        kw["policy_delay"] = case[11]
    if case[12] is not None:
        sm = case[12]
        kw.update(target_policy_noise=sm[0], target_policy_noise_clip=sm[1], target_policy_noise_seed=sm[2])
    if case[13]:
        kw.update(prioritized_replay=True, priority_alpha=P.PER["alpha"], priority_eps=P.PER["eps"], priority_beta=P.PER["beta"],
                  priority_beta_final=P.PER["beta"], sample_seed=P.PER["sample_seed"])
    if case[14] > 1:
        kw["n_step"] = case[14]
    if P.is_stack(case):
        hidden = ",".join(str(h) for h in P.STACK_HIDDEN)
        kw.update(shared_encoder=True, feature_layer_norm=True, replay_store="u8", random_shift=P.STACK_SHIFT[0], random_shift_seed=P.STACK_SHIFT[1],
                  actor_hidden_layers=hidden, critic_hidden_layers=hidden)
    return kw


def _case_agent(case, inputs, pool="case", **kw):
    params = inputs[1]
    if params is not None:      # (the critics in the device's order)
        params = [p if i % 2 == 0 else P.critic_to_device(case, inputs[0], p) for i, p in enumerate(params)]
    agent = _build(P.SHAPES[case[2]], case[4], case[3], P.hyper_of(case), P.pool_of(case) if pool == "case" else pool, params, inputs[2],
                   **dict(_case_kw(case), **kw))
    if case[13] and inputs[2]:
        agent.replay_memory.update_priorities(np.arange(P.ROWS), S.per_priorities())
    return agent


def _params(agent):
    return [n.get_params() for n in agent.networks()]


def _state(agent, case, specs=None):
    """tests.pool_np's vectors() of the device (the critic's vectors and slots in the restatement's order: specs, for the stack)"""
    t = agent.trainer
    f = lambda v: np.asarray(v, np.float64)
    conv = lambda v: f(P.critic_from_device(case, specs, v))
    pa, pc, pta, ptc = _params(agent)
    out = {"actor": f(pa), "critic": conv(pc), "target_actor": f(pta), "target_critic": conv(ptc)}
    n = len(out["actor"]) + len(out["critic"])
    if t.has_optimiser_slots():
        st = t.get_optimiser_state()
        na = len(pa)
        out.update(m=np.concatenate([f(st["m"][:na]), conv(st["m"][na:])]), v=np.concatenate([f(st["v"][:na]), conv(st["v"][na:])]),
                   step=[int(x) for x in st["step"]])
    else:
        out.update(m=np.zeros(n), v=np.zeros(n), step=[0, 0])
    out["n"] = 0
    if case[1] == "sac":
        sac = t.get_sac_state()
        out.update(log_alpha=float(sac["log_alpha"]), alpha_m=float(sac["m"]), alpha_v=float(sac["v"]), alpha_step=int(sac["step"]))
    return out


def _last_rows(agent, B):
    lib, check, ptr = _abi()
    rows = np.empty(B, np.int32)
    check(lib.cpp_replay_last_indexes(agent.replay_memory.handle, B, ptr(rows)))
    return rows


def _read(agent, case, k, B, specs=None):
    """what the last minibatch left on the device, in the shape tests.pool_np.ratios takes; the device's noise, held to the restated draw"""
    A = case[3]
    t = agent.trainer
    acts, dq, q, td = t.last_values(B)
    q2, tq1, tq2, td2 = t.last_twin_values(B)
    th1, th2, srt, y = t.last_pooled_quantiles(B)
    stats = t.last_stats()
    got = {"actions": acts, "dq_da": dq, "q": q, "q2": q2, "td": td, "td2": td2, "target_q": tq1, "target_q2": tq2, "theta1": th1, "theta2": th2,
           "sorted": srt, "y": y, "loss": float(stats[0]), "actor_norm": float(stats[1]), "critic_norm": float(stats[2]),
           "actor_grads": agent.actor.get_grads(), "critic_grads": P.critic_from_device(case, specs, agent.critic.get_grads())}
    if case[1] == "sac":
        sac = t.last_sac(B)
        assert sac["n"] == k, (sac["n"], k)
        for key, stream in (("eps", S.STREAM_S1), ("eps2", S.STREAM_S2)):
            assert float(np.max(np.abs(sac[key] - S.noise(P.NOISE_SEED, k, B, A, stream)))) <= S.eps_bar(), key
        np.testing.assert_array_equal(acts, sac["a"])
        got.update(target_actions=sac["a2"], logp=sac["logp"], logp2=sac["logp2"], r_soft=sac["r_soft"], g_alpha=sac["g_alpha"])
        noise = (sac["eps"], sac["eps2"])
    elif case[12] is not None:
        sigma, clip, seed = case[12]
        eps, count = t.last_target_noise(B)
        assert count == k, (count, k)
        assert np.abs(eps - T.target_noise(seed, k, B, A, sigma, clip, np.float64)).max() <= T.Z_BAR * sigma
        noise = eps.astype(np.float64)
    else:
        noise = None
    routes = None
    if P.is_stack(case):          # (the actor has no conv layers: the encoder's routes are the critic's)
        routes = (None, device_pool_codes(agent.critic, B), None, device_relu_active(agent.critic, B))
    elif case[2] != "lowdim":
        routes = (device_pool_codes(agent.actor, B), device_pool_codes(agent.critic, B), device_relu_active(agent.actor, B),
                  device_relu_active(agent.critic, B))
    return got, noise, routes


def _check_shapes(case, got, B):
    N, d = case[5], case[6]
    M = 2 * N - 2 * d
    assert got["theta1"].shape == got["theta2"].shape == (B, N) and got["sorted"].shape == got["y"].shape == (B, 2 * N)
    assert (np.diff(got["sorted"], axis=1) >= 0).all() and not got["y"][:, M:].any()          # ascending; the dropped columns are zero


# ---- 1. the kernel against its own inputs: the restatement on the atoms the device read back
def _kernel_rows(agent, case_like, B, rows, weights, N, kappa, d, discount, ref, start, episodes):
    got, _noise, _routes = _read(agent, case_like, 0, B)
    hb = agent.replay_memory.batch(idxs=rows)
    # what the kernel READ: the restatement from the device's state before the step -- the sorted pool against np.sort of the restated target
    # critic's raw atoms, the target heads' means (taken before the sort) and both online heads' atoms
    ref.set_state(start)
    ref.pool = (N, kappa, d)
    cg = ref.critic_gradients(P.batches_of(case_like, episodes, rows)[0], noise=None, w=weights)
    raw = np.sort(np.concatenate([cg["target_theta1"], cg["target_theta2"]], axis=1), axis=1)
    assert np.abs(got["sorted"] - raw).max() < P.bar("sorted"), (N, d, B)
    for k in ("theta1", "theta2", "target_q", "target_q2"):
        assert np.abs(np.asarray(got[k], np.float64).reshape(cg[k].shape) - cg[k]).max() < P.bar(k), (k, N, d, B)
    pool = got["sorted"].astype(np.float64)
    want = P.rows(got["theta1"], got["theta2"], pool[:, :N], pool[:, N:], np.asarray(hb.reward), np.asarray(hb.terminal_mask), discount, kappa, d,
                  np.float64, weights)
    _check_shapes(("", "", "", 0, B, N, d), got, B)
    err = {k: float(np.max(np.abs(np.asarray(got[k], np.float64).reshape(want[k].shape) - want[k]))) for k in ("y", "q", "q2", "td", "td2")}
    err["loss"] = abs(got["loss"] - float(want["loss"])) / max(1.0, abs(float(want["loss"])))
    # d theta of both heads through the q layers' bias gradients: db = sum_b dz_b
    grads, db = got["critic_grads"], {}
    for v in agent.critic.trainable_model_vars():
        name = v.name.split("/", 1)[1]
        if name in ("q_value/biases:0", "q_valueb/biases:0"):
            db[name] = grads[v.offset:v.offset + int(np.prod(v.shape))]
    err["dz1"] = float(np.max(np.abs(db["q_value/biases:0"] - want["dz1"].sum(axis=0))))
    err["dz2"] = float(np.max(np.abs(db["q_valueb/biases:0"] - want["dz2"].sum(axis=0))))
    # the expect job: Q_1 and Q_2 at mu(s1) are the means of atoms the device does not report; the tops show in dQbar/da (section 2)
    for k, v in err.items():
        bar = P.ATOL if k == "loss" else P.bar("dz") if k.startswith("dz") else P.bar(k)
        assert v < bar, (k, N, d, B, err)
    return err


@pytest.mark.parametrize("weighted", [False, True], ids=["uniform", "weighted"])
@pytest.mark.parametrize("N", [2, 5, 25, 32])
def test_the_kernel_against_its_own_inputs(N, weighted):
    """N in {2, 5, 25, 32} x d in {0, 1, 2, N - 1} x B in {1, 5, 7, 8} (a partial workgroup), the uniform and the weighted instance"""
    case = P.case_of("A2-B8-N25-d2-per-nstep3" if weighted else "A2-B8-N25-d2-sgd")
    case = case[:5] + (N, min(2, N - 1)) + case[7:14] + (1,) + case[15:]
    inputs = P.case_inputs(case, seed=1)
    hp = P.hyper_of(case)
    agent = _case_agent(case, inputs)
    ref = P.restatement(case, inputs)
    worst = {}
    try:
        idxs = inputs[3]
        for d in sorted({0, 1, min(2, N - 1), N - 1}):
            agent.trainer.set_quantile_target(1.0, d)
            for B in (1, 5, 7, 8):
                start = _state(agent, case)
                if weighted:
                    agent.train_step(B, 1)
                    rows = _last_rows(agent, B)
                    w = agent.replay_memory.last_weights(B).astype(np.float64).reshape(B, 1)
                    assert abs(w.max() - 1.0) < 1e-6 and (B == 1 or w.min() < 1.0)
                else:
                    rows, w = np.ascontiguousarray(idxs[:B], dtype=np.int32), None
                    agent.train_step(B, 1, idxs=rows)
                err = _kernel_rows(agent, case, B, rows, w, N, 1.0, d, hp.discount, ref, start, inputs[2])
                worst = {k: max(v, worst.get(k, 0.0)) for k, v in err.items()}
        print("N %d %s: worst %s" % (N, "weighted" if weighted else "uniform", {k: "%.2e" % v for k, v in worst.items()}))
    finally:
        agent.close()


# ---- 2. whole minibatches from a common start
def _run_case(cid):
    case = P.case_of(cid)
    form, B, weighted = case[1], case[4], case[13]
    inputs = P.case_inputs(case)
    agent = _case_agent(case, inputs)
    refs = (P.restatement(case, inputs), P.restatement(case, inputs, np.float32))
    per = S.RestatedPer() if weighted else None
    worst = (0.0, None, None)
    try:
        rm = agent.replay_memory
        start = _state(agent, case, inputs[0])
        want0 = P.initial_state(case, inputs)
        for key in ("actor", "critic", "target_actor", "target_critic"):
            np.testing.assert_array_equal(start[key], want0[key])
        for k in range(P.nb_of(case)):
            weights = None
            if weighted:
                agent.train_step(B, 1)
                rows = _last_rows(agent, B)
                weights = rm.last_weights(B).astype(np.float64).reshape(B, 1)
                # the draw against tests.per_np's tree, kept with the device's own td_1: the priorities come from head 1's td
                r_rows, r_w = per.draw(k, B)
                assert np.array_equal(rows, r_rows), (cid, k, rows, r_rows)
                assert float(np.max(np.abs(weights.ravel() / r_w.ravel().astype(np.float64) - 1.0))) <= 8 * 2.0 ** -23 + 2.0 ** -24
            else:
                rows = np.ascontiguousarray(inputs[3][k * B:(k + 1) * B], dtype=np.int32)
                agent.train_step(B, 1, idxs=rows)
            got, noise, routes = _read(agent, case, k, B, inputs[0])
            _check_shapes(case, got, B)
            got_vec = _state(agent, case, inputs[0])
            if P.is_stack(case):      # the shifted images of the device's own gather, its shifts held to the restated draw
                from tests.test_gpu_random_shift import _shifted_minibatch
                from tests import shift_np
                batch, _unshifted, sh = _shifted_minibatch(rm, rows)
                assert np.array_equal(sh, shift_np.shifts(P.STACK_SHIFT[1], k, B, P.STACK_SHIFT[0]))
                for x, y in zip(batch[1:4], inputs[4][k][1:4]):          # (the states are the store's own decoding of the u8 codes)
                    np.testing.assert_array_equal(np.asarray(x), np.asarray(y))
            else:
                batch = P.batches_of(case, inputs[2], rows)[0]
                hb = rm.batch(idxs=rows)      # (the memory's own columns: the n-step fold is the restated one)
                np.testing.assert_array_equal(np.asarray(hb.reward), batch[2])
                np.testing.assert_array_equal(np.asarray(hb.terminal_mask), batch[3])
            outs, vecs = [], []
            for ref in refs:
                o, v = P.step(ref, case, batch, k, noise=noise, weights=weights, routes=routes, start=start)
                outs.append(o)
                vecs.append(v)
            want = outs[0]
            if routes is not None:
                if routes[0] is not None:
                    pool_flips_are_near_ties(want["cache_actor"], routes[0], what="actor")
                    relu_flips_are_at_the_boundary(want["cache_actor"], routes[2], what="actor")
                pool_flips_are_near_ties(want["cache_critic"], routes[1], what="critic")
                relu_flips_are_at_the_boundary(want["cache_critic"], routes[3], what="critic")
            r = P.ratios(case, inputs[0], start, got, got_vec, want, vecs[0], outs[1], vecs[1])
            key = max(r, key=lambda x: r[x])
            print("%s minibatch %d: worst %s at %.3f of its bar; %s" % (cid, k, key, r[key], {a: "%.2f" % b for a, b in sorted(r.items())}))
            if r[key] > worst[0]:
                worst = (float(r[key]), k, key)
            bad = {a: b for a, b in r.items() if not b <= 1.0}
            assert not bad, (cid, k, bad)
            # the conditions of tests/test_pooled_quantile_host.py, on what the device ran
            for name, (value, floor) in P.conditions(case, want).items():
                assert value >= floor, (cid, k, name, value)
            if case[15]:
                for n, side in zip((got["actor_norm"], got["critic_norm"]), case[15]):
                    assert n >= P.CLIP_SIDE_FACTOR * case[9] if side == "above" else n <= case[9] / P.CLIP_SIDE_FACTOR, (cid, k, side, n)
            if case[11] > 1:
                assert agent.trainer.policy_delay_status() == (case[11], k + 1, not want["applied"])
            if form == "sac":
                np.testing.assert_array_equal(agent.target_actor.get_params(), agent.actor.get_params())
            if per is not None:
                per.update(rows, got["td"])
            start = got_vec
        print("%s: worst error / bar %.3f (minibatch %s, %s)" % ((cid,) + worst))
    finally:
        agent.close()


@pytest.mark.parametrize("cid", [c[0] for c in P.CASES])
def test_minibatches_from_a_common_start_against_the_float64_restatement(cid):
    _run_case(cid)


# ---- 3. the readers
def test_check_loss_forward_and_dq_da():
    """check_loss and CriticNetwork.forward read head 1 (Q_1, td_1), q_gradients_wrt_actions returns dQbar/da"""
    case = P.case_of("A2-B8-N5-d1-smoothed-delay2")
    B, N = case[4], case[5]
    inputs = P.case_inputs(case)
    agent = _case_agent(case, inputs)
    try:
        hb = HostBatch(*inputs[4][0])
        loss, td, q = agent.critic.check_loss(hb)
        assert agent.trainer.last_target_noise(B)[1] == 0              # (an evaluation: no draw, no count)
        q_fwd = agent.critic.forward(hb.state_1, hb.action)
        dq = agent.critic.q_gradients_wrt_actions(hb)
        names = [(v.name, tuple(v.shape)) for v in agent.critic.trainable_model_vars()]
        n_q, n_p, n_atoms = ctypes.c_int(-1), ctypes.c_int(-1), ctypes.c_int(-1)
        lib, check, _ptr = _abi()
        check(lib.cpp_net_quantile_info(agent.critic.handle, ctypes.byref(n_q)))
        check(lib.cpp_net_pooled_quantile_info(agent.critic.handle, ctypes.byref(n_p)))
        check(lib.cpp_net_distribution_info(agent.critic.handle, ctypes.byref(n_atoms), None, None))
        assert (n_q.value, n_p.value, n_atoms.value, lib.cpp_net_is_twin_q(agent.critic.handle)) == (0, N, 0, 1)
        check(lib.cpp_net_pooled_quantile_info(agent.actor.handle, ctypes.byref(n_p)))
        assert n_p.value == 0 and agent.trainer.quantile_target == (float(np.float32(case[7])), case[6])
    finally:
        agent.close()
    n_in = inputs[0][1].fc[-1][1]
    assert names[-2:] == [("critic/q_valueb/weights:0", (n_in, N)), ("critic/q_valueb/biases:0", (N,))]
    assert ("critic/q_value/weights:0", (n_in, N)) in names
    ref = P.restatement(case, inputs)
    wl, wtd, wq = ref.check_loss(inputs[4][0])
    assert abs(loss - wl) < P.ATOL * max(1.0, wl) and np.abs(td - wtd).max() < P.bar("td") and np.abs(q - wq).max() < P.bar("q")
    c = ref.critic.forward(hb.state_1, action=hb.action, training=False)
    assert np.abs(q_fwd - c["out"].mean(axis=1, keepdims=True)).max() < P.bar("q") and q_fwd.shape == (B, 1)
    ag = ref.actor_gradients(hb.state_1)
    assert np.abs(dq - ag["dq_da"]).max() < P.bar("dq_da") and np.abs(ag["dq_da"]).max() > 1e-3
    head1 = P.restatement(case, inputs, fault="actor_head1_only").actor_gradients(hb.state_1)
    assert np.abs(dq - head1["dq_da"]).max() > 100 * P.bar("dq_da")          # (not head 1's alone)


# ---- 4. the same bits: graph replays, eager steps, repeated runs, the literal loop's pairs, the single ops, the data-parallel step
BITS_CASE = {"td3": "A2-B8-N5-d1-smoothed-delay2", "sac": "sac-A2-B8-N25-d2-adam"}


def _bits_agent(form):
    case = P.case_of(BITS_CASE[form])
    return case, _case_agent(case, P.case_inputs(case), sample_seed=GRAPH_SAMPLE_SEED)


def _bits(agent, case):
    B = case[4]
    t = agent.trainer
    st = _state(agent, case)
    out = [st[k] for k in ("actor", "critic", "target_actor", "target_critic", "m", "v")] + [np.asarray(st["step"])]
    out += list(t.last_pooled_quantiles(B)) + list(t.last_values(B)) + list(t.last_twin_values(B)) + [np.asarray(t.last_stats())]
    if case[1] == "sac":
        out += [np.asarray([st["log_alpha"], st["alpha_m"], st["alpha_v"], st["alpha_step"]])]
    return out


def _same(runs):
    for k, other in enumerate(runs[1:]):
        for i, (x, y) in enumerate(zip(runs[0], other)):
            assert np.array_equal(x, y), ("run", k + 1, "item", i)


@pytest.mark.parametrize("form", ["td3", "sac"])
def test_eager_steps_graph_replays_and_repeated_runs_are_bit_identical(form):
    nb, steps = 2, 3
    runs = []
    for mode in ("graph", "graph", "eager"):
        case, agent = _bits_agent(form)
        B = case[4]
        try:
            for _s in range(steps):
                if mode == "graph":
                    agent.train_step(B, nb)
                else:
                    _profiled_calls(agent.actor.ctx, lambda: agent.train_step(B, nb))      # (profiling keeps the call on stream launches)
            runs.append(_bits(agent, case))
        finally:
            agent.close()
    _same(runs)


@pytest.mark.parametrize("form", ["td3", "sac"])
def test_the_paired_literal_loop_is_the_fused_step_bit_for_bit(form):
    """actor.train(batch.state_1); critic.train(batch) on device-resident batches run as ONE cpp_ddpg_train_rows -- against
    train_step(B, 1, idxs) on the same rows, per minibatch, to the bit"""
    case, lit = _bits_agent(form)
    _c, fused = _bits_agent(form)
    B = case[4]
    try:
        np.random.seed(99)
        for _step in range(4):
            batch = lit.replay_memory.batch(B)
            lit.actor.train(batch.state_1)
            lit.critic.train(batch)
            lit.target_actor.update_weights()
            lit.target_critic.update_weights()
            fused.train_step(B, 1, idxs=batch.idxs)
            _same([_bits(lit, case), _bits(fused, case)])
        assert lit.trainer.fused_pairs == 4 and fused.trainer.fused_pairs == 0
    finally:
        lit.close()
        fused.close()


def test_the_single_ops_are_the_pass():
    """actor.train(s1), then critic.train(batch), on host arrays (each one half of the gradient pass and its own apply) against the fused
    minibatch on the same rows: plain gradient descent, so that the four parameter vectors are the whole state -- to the bit"""
    case = P.case_of("A2-B8-N25-d2-sgd")
    B = case[4]
    inputs = P.case_inputs(case)
    single, fused = _case_agent(case, inputs), _case_agent(case, inputs)
    try:
        for k in range(P.NB):
            rows = np.ascontiguousarray(inputs[3][k * B:(k + 1) * B], dtype=np.int32)
            hb = HostBatch(*inputs[4][k])
            single.actor.train(hb.state_1)
            dq = single.trainer.last_values(B)[1]
            single.critic.train(hb)
            single.target_actor.update_weights()
            single.target_critic.update_weights()
            fused.train_step(B, 1, idxs=rows)
            for x, y in zip(_params(single), _params(fused)):
                np.testing.assert_array_equal(x, y)
            np.testing.assert_array_equal(dq, fused.trainer.last_values(B)[1])
            for x, y in zip(single.trainer.last_pooled_quantiles(B), fused.trainer.last_pooled_quantiles(B)):
                np.testing.assert_array_equal(x, y)
        assert single.trainer.fused_pairs == 0
    finally:
        single.close()
        fused.close()


def test_the_data_parallel_step_as_a_world_of_one():
    """without SAC: cpp_ddpg_dp_train_step with no communicator ends where train_step ends on the same draws, to the bit; under SAC the
    entry point refuses"""
    lib, check, _ptr = _abi()
    nb, steps = 2, 2
    runs = []
    for mode in ("dp", "step"):
        case, agent = _bits_agent("td3")
        B = case[4]
        try:
            for _s in range(steps):
                if mode == "dp":
                    check(lib.cpp_ddpg_dp_train_step(agent.trainer.handle, agent.replay_memory.handle, None, B, nb, GRAPH_SAMPLE_SEED, 1, 0))
                else:
                    agent.train_step(B, nb)
            runs.append(_bits(agent, case)[:7])
        finally:
            agent.close()
    _same(runs)
    case, agent = _bits_agent("sac")
    try:
        rc = lib.cpp_ddpg_dp_train_step(agent.trainer.handle, agent.replay_memory.handle, None, case[4], nb, GRAPH_SAMPLE_SEED, 1, 0)
        assert rc == CPP_ERR_ARG and b"soft actor-critic" in lib.cpp_last_error()
    finally:
        agent.close()


def test_the_drq_stack_with_pooled_critics_runs_and_replays_to_the_bit():
    """one stack at 64x64x18, B = 8: SAC, the shared encoder, the feature layer norm (cpp_net_create_pooled_quantile_norm), the u8 store and
    random shift 4 under pooled critics -- graph replays, eager steps and a repeated run leave the same bits, the pool is sorted, the
    dropped columns are zero and both heads' tds share one truncated mean.  (The stack against float64: the case
    sac-drq-64x64x18-A2-B8-N25-d2-adam above.)"""
    shape, B, A, rows, pool, nb = (64, 64, 3, 2, 3), 8, 2, 60, (25, 1.0, 2), 2
    hp = T3.hyper_of("adam", 0.5, 0.25)
    kw = dict(T3.opt_kw("adam"), soft_actor_critic=True, sac_temperature_learning_rate=1e-2, sac_seed=5, shared_encoder=True, feature_layer_norm=True,
              replay_store="u8", random_shift=4, random_shift_seed=3, sample_seed=11, actor_hidden_layers="100,100,50", critic_hidden_layers="100,100,50")
    runs = []
    for mode in ("graph", "graph", "eager"):
        agent = _build(shape, B, A, hp, pool, rows=rows, seed=4, **kw)
        try:
            agent.replay_memory.fill_synthetic(rows, seed=25)
            for _s in range(3):
                if mode == "graph":
                    agent.train_step(B, nb)
                else:
                    _profiled_calls(agent.actor.ctx, lambda: agent.train_step(B, nb))
            t = agent.trainer
            th1, th2, srt, y = t.last_pooled_quantiles(B)
            _a, _dq, q, td = t.last_values(B)
            q2, _tq1, _tq2, td2 = t.last_twin_values(B)
            names = [v.name for v in agent.critic.trainable_model_vars()]
            runs.append(_params(agent) + [th1, th2, srt, y, q, td, q2, td2, np.asarray(t.last_stats())])
        finally:
            agent.close()
    _same(runs)
    assert names[-2:] == ["critic/hidden1/LayerNorm/gamma:0", "critic/hidden1/LayerNorm/beta:0"] and "critic/q_valueb/weights:0" in names
    assert all(np.isfinite(x).all() for x in runs[0])
    M = 2 * pool[0] - 2 * pool[2]
    assert (np.diff(srt, axis=1) >= 0).all() and not y[:, M:].any() and np.ptp(srt) > 0
    assert np.abs((q - td) - (q2 - td2)).max() < 2 * P.ATOL and np.abs((q - td).ravel() - y[:, :M].mean(axis=1)).max() < 2 * P.ATOL


# ---- 5. checkpoints
def test_checkpoints_round_trip_and_the_layout_check_refuses_across_kinds(tmp_path):
    from cartpoleplusplus_amd import util
    case = P.case_of("A2-B8-N25-d2-adam-clipped")
    B = case[4]
    inputs = P.case_inputs(case)
    agent = _case_agent(case, inputs)
    try:
        agent.train_step(B, 2, idxs=inputs[3][:2 * B])
        util.SaverUtil(agent, str(tmp_path / "pool"), 3600).force_save()
        want = _params(agent) + [agent.trainer.get_optimiser_state()[k] for k in ("m", "v")]
    finally:
        agent.close()
    bare = (inputs[0], None, None, None, None)
    agent = _case_agent(case, bare, seed=7)
    try:
        assert not np.array_equal(agent.critic.get_params(), want[1])
        util.SaverUtil(agent, str(tmp_path / "pool"), 3600)
        got = _params(agent) + [agent.trainer.get_optimiser_state()[k] for k in ("m", "v")]
        assert all(np.array_equal(x, y) for x, y in zip(got, want))
    finally:
        agent.close()
    # a twin scalar, a single-head quantile and a plain critic, and pooled critics of another N: refused in both directions
    kinds = {"twin": dict(pool=None, twin_q=True), "quant": dict(pool=None, quantile_critic=True, num_quantiles=25), "plain": dict(pool=None),
             "n24": dict(pool=(24, 1.0, 2))}
    for name, kw in kinds.items():
        other = _case_agent(case, bare, **kw)
        try:
            with pytest.raises(AssertionError, match="checkpoint does not match critic"):
                util.SaverUtil(other, str(tmp_path / "pool"), 3600)
            util.SaverUtil(other, str(tmp_path / name), 3600).force_save()
        finally:
            other.close()
        agent = _case_agent(case, bare)
        try:
            with pytest.raises(AssertionError, match="checkpoint does not match critic"):
                util.SaverUtil(agent, str(tmp_path / name), 3600)
        finally:
            agent.close()


# ---- 6. the census; off means off
NEW_CALLS = ("cpp_net_create_pooled_quantile", "cpp_net_create_pooled_quantile_norm", "cpp_net_pooled_quantile_info", "cpp_ddpg_last_pooled_quantiles",
             "cpp_ddpg_set_quantile_target")


def test_the_launches_of_a_pooled_outer_step():
    """quant_pool.hip's two launches per minibatch (the td job and the expect job, counted in the quantile critic's family) on the GEMM
    levels, 13 `gemm` launches per minibatch and 14 under SAC; no td_kernel, no heads, dist or bc launch"""
    case = P.case_of("A2-B8-N25-d2-sgd")
    B, nb = case[4], 2
    inputs = P.case_inputs(case)
    agent = _case_agent(case, inputs, sample_seed=GRAPH_SAMPLE_SEED)
    try:
        agent.train_step(B, nb)
        n = _profiled_calls(agent.actor.ctx, lambda: agent.train_step(B, nb))
    finally:
        agent.close()
    print("launches per outer step: %s" % n)
    assert n.get("quant", 0) == 2 * nb, n          # (the pooled launches are counted in the quantile critic's family: a trainer has one kind or the other)
    assert all(n.get(k, 0) == 0 for k in ("dist", "heads", "td", "bc", "sac")) and n.get("gemm", 0) == 13 * nb, n
    case = P.case_of("sac-A2-B8-N25-d2-adam")
    agent = _case_agent(case, P.case_inputs(case), sample_seed=GRAPH_SAMPLE_SEED)
    try:
        agent.train_step(B, nb)
        m = _profiled_calls(agent.actor.ctx, lambda: agent.train_step(B, nb))
    finally:
        agent.close()
    print("launches per outer step under SAC: %s" % m)
    assert m.get("quant", 0) == 2 * nb and m.get("sac", 0) == 4 * nb and m.get("gemm", 0) == 14 * nb and all(m.get(k, 0) == 0 for k in ("dist", "heads", "td", "bc")), m


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


_PLAIN_SNIPPET = r"""
import json, sys
sys.path.insert(0, %(root)r)
from tests import test_gpu_pooled_quantile as G
print("RESULT " + json.dumps(G._plain_run(%(pooled_first)r)))
"""


def _plain_run(pooled_first):
    """three graph-replayed outer steps of a PLAIN trainer (after a pooled one has lived and died in the process, if asked): the digest of
    its parameters, the launch census of one more outer step, and how often it called the new entry points"""
    from tests.helpers import host_case
    case = P.case_of("A2-B8-N25-d2-sgd")
    B, A, nb = case[4], case[3], 2
    if pooled_first:
        agent = _case_agent(case, P.case_inputs(case), sample_seed=GRAPH_SAMPLE_SEED)
        try:
            agent.train_step(B, nb)
            agent.train_step(B, nb)
        finally:
            agent.close()
    specs, Pp, episodes, _i, _b = host_case(P.SHAPES["lowdim"], B, 1, 1, rows=P.ROWS, action_dim=A)
    with _CallLog(NEW_CALLS) as log:
        agent = _build(P.SHAPES["lowdim"], B, A, P.hyper_of(case), None, Pp, episodes, sample_seed=GRAPH_SAMPLE_SEED,
                       actor_hidden_layers="100,100,50", critic_hidden_layers="100,100,50")
        try:
            for _s in range(3):
                agent.train_step(B, nb)
            h = hashlib.sha256()
            for x in _params(agent):
                h.update(np.ascontiguousarray(x).tobytes())
            census = _profiled_calls(agent.actor.ctx, lambda: agent.train_step(B, nb))
            new_calls = sum(log.calls.values())
        finally:
            agent.close()
    return {"digest": h.hexdigest(), "census": census, "new_calls": new_calls}


def test_off_means_off():
    """a plain trainer created after a pooled one in the same process ends with the bits, and launches the kernels, of one in a process that
    never made one; it calls none of the new entry points"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = subprocess.run([sys.executable, "-c", _PLAIN_SNIPPET % dict(root=root, pooled_first=False)], cwd=root, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    fresh = json.loads([l for l in out.stdout.splitlines() if l.startswith("RESULT ")][0][len("RESULT "):])
    here = _plain_run(True)
    assert here["census"] == fresh["census"], (here["census"], fresh["census"])
    assert here["digest"] == fresh["digest"]
    assert here["new_calls"] == fresh["new_calls"] == 0
    assert here["census"].get("quant", 0) == 0


# ---- 7. the refusals
def test_the_refusals():
    from cartpoleplusplus_amd import _lib
    lib, check, ptr = _abi()
    case = P.case_of("A2-B8-N25-d2-sgd")
    inputs = P.case_inputs(case)
    hpy, shape = P.hyper_of(case), P.SHAPES["lowdim"]
    pooled = _case_agent(case, inputs)
    try:
        plain = _build(shape, 8, 2, hpy, None)
        other_n = _build(shape, 8, 2, hpy, (24, 1.0, 2))
        twin = _build(shape, 8, 2, hpy, None, twin_q=True)
        quant = _build(shape, 8, 2, hpy, None, quantile_critic=True, num_quantiles=25)
        try:
            ctx = pooled.actor.ctx.handle
            hp = _lib.DdpgHyper(1e-3, 1e-2, 0.9, 5.0, 0.1)
            h = ctypes.c_void_p()
            # mismatched critic / target critic: against a plain, a twin scalar, a single-head quantile critic and another N, both ways
            for other in (plain, twin, quant, other_n):
                for critic, target in ((pooled.critic, other.target_critic), (other.critic, pooled.target_critic)):
                    rc = lib.cpp_ddpg_create(ctx, plain.actor.handle, critic.handle, plain.target_actor.handle, target.handle, ctypes.byref(hp), ctypes.byref(h))
                    assert rc == CPP_ERR_ARG, (rc, lib.cpp_last_error())
            # N out of range (33: the pool would not fit a wave), not a critic
            spec = _lib.NetSpec()
            ctypes.memmove(ctypes.byref(spec), ctypes.byref(pooled.critic.spec), ctypes.sizeof(spec))
            for n in (33, 64, 1, 0, -3):
                rc = lib.cpp_net_create_pooled_quantile(ctx, ctypes.byref(spec), 8, n, ctypes.byref(h))
                assert rc == CPP_ERR_ARG and b"cpp_net_create_pooled_quantile" in lib.cpp_last_error(), (n, rc)
            rc = lib.cpp_net_create_pooled_quantile_norm(ctx, ctypes.byref(spec), 8, 25, _lib.CPP_NORM_TANH, 1e-5, ctypes.byref(h))
            assert rc == CPP_ERR_ARG and b"low-dimensional" in lib.cpp_last_error()
            ctypes.memmove(ctypes.byref(spec), ctypes.byref(pooled.actor.spec), ctypes.sizeof(spec))
            rc = lib.cpp_net_create_pooled_quantile(ctx, ctypes.byref(spec), 8, 25, ctypes.byref(h))
            assert rc == CPP_ERR_ARG and b"cpp_net_create_pooled_quantile" in lib.cpp_last_error()
            # a pooled critic in NAF
            nh = _lib.NafHyper(0.9, 5.0, 0.1, 0, 1e-3, 0.0, 0.9, 0.999, 1e-8)
            rc = lib.cpp_naf_create(ctx, pooled.critic.handle, pooled.target_critic.handle, pooled.critic.handle, pooled.critic.handle, 0, ctypes.byref(nh), ctypes.byref(h))
            assert rc == CPP_ERR_ARG and b"cpp_naf_create" in lib.cpp_last_error()
            # cpp_ddpg_set_quantile_target: d per head outside [0, N - 1] (d = N: nothing stays); the trainer keeps what it had
            th = pooled.trainer.handle
            for kappa, drop in ((0.0, 0), (-1.0, 0), (float("inf"), 0), (float("nan"), 0), (1.0, -1), (1.0, 25), (1.0, 50)):
                rc = lib.cpp_ddpg_set_quantile_target(th, kappa, drop)
                assert rc == CPP_ERR_ARG and b"cpp_ddpg_set_quantile_target" in lib.cpp_last_error(), (kappa, drop, rc)
            check(lib.cpp_ddpg_set_quantile_target(th, 0.5, 24))
            check(lib.cpp_ddpg_set_quantile_target(th, 1.0, 2))
            # the actor on the minimum head and the behaviour-cloning term are not this trainer's
            assert lib.cpp_ddpg_set_actor_min_q(th, 1) == CPP_ERR_ARG and b"pooled" in lib.cpp_last_error()
            assert lib.cpp_ddpg_set_behaviour_cloning(th, 2.5, 1e-3) == CPP_ERR_ARG
            # the read-backs across kinds
            buf = np.empty(8 * 50, np.float32)
            for other in (plain, twin, quant):
                rc = lib.cpp_ddpg_last_pooled_quantiles(other.trainer.handle, 8, ptr(buf), None, None, None)
                assert rc == CPP_ERR_STATE and b"cpp_ddpg_last_pooled_quantiles" in lib.cpp_last_error()
            assert lib.cpp_ddpg_last_quantiles(th, 8, ptr(buf), None, None) == CPP_ERR_STATE
            assert lib.cpp_ddpg_last_distribution(th, 8, ptr(buf), None, None) == CPP_ERR_STATE
            assert lib.cpp_ddpg_last_pooled_quantiles(None, 8, None, None, None, None) == CPP_ERR_ARG
            assert lib.cpp_ddpg_last_pooled_quantiles(th, 9, None, None, None, None) == CPP_ERR_ARG
            assert lib.cpp_ddpg_last_pooled_quantiles(th, 8, None, None, None, None) == 0
            assert lib.cpp_net_pooled_quantile_info(None, None) == CPP_ERR_ARG
        finally:
            for a in (plain, other_n, twin, quant):
                a.close()
    finally:
        pooled.close()
    with pytest.raises(SystemExit):
        _build(shape, 8, 2, hpy, (25, 1.0, 2), twin_q=True)
    with pytest.raises(SystemExit):
        _build(shape, 8, 2, hpy, (25, 1.0, 25))
    with pytest.raises(SystemExit):
        _build(shape, 8, 2, hpy, (33, 1.0, 2))


def test_tqc_trains_through_main(capsys):
    """the recipe, --soft-actor-critic --pooled-quantile-critics, through ddpg_cartpole.main on the stand-in environment"""
    from cartpoleplusplus_amd import ddpg_cartpole as D
    D.main(["--synthetic-env", "--use-raw-pixels", "--render-width", "16", "--render-height", "16", "--max-episode-len", "12", "--batch-size", "8",
            "--batches-per-step", "2", "--replay-memory-size", "200", "--replay-memory-burn-in", "20", "--max-num-actions", "60",
            "--soft-actor-critic", "--pooled-quantile-critics"])
    out = capsys.readouterr()
    stats = [l for l in out.out.splitlines() if l.startswith("STATS")]
    assert stats and "q_value" in out.err
