"""Soft actor-critic as the trainer composes it -- twin critics, Adam and Momentum, the clip on both sides, importance weights, n-step
memories, random shift, the operand-image rider's geometry -- against tests.sac_np.ComposedSac (float64), minibatch by minibatch.

Every minibatch is compared from a common start: the restatement takes over the device's state (parameters, slots, counts, temperature)
before it, is fed the device's own eps (itself checked against the restated draw), importance weights, shifts and pool / ReLU routes
(a differing route accepted only at a near tie), and then both pre-clip norms, both pre-clip lists per variable, every per-row value,
the loss, the parameter, target and slot deltas, the counts and the temperature's Adam element must sit inside tests.sac_np.ratios'
bars.  tests/test_sac_host.py holds the cases to their conditions, the float32 twin inside the same bars and every planted fault
outside them by ten times."""
import collections

import numpy as np
import pytest

from tests import sac_np as S
from tests import td3_np as T3
from tests.helpers import (FakeEnv, assert_flat_close, device_pool_codes, device_relu_active, hyper_options, make_opts,
                           pool_flips_are_near_ties, relu_flips_are_at_the_boundary)

pytestmark = pytest.mark.gpu
HostBatch = collections.namedtuple("HostBatch", "state_1 action reward terminal_mask state_2")
WORST = {}          # run -> (ratio, minibatch, quantity): the largest error / bar seen (printed per case)


def _abi():
    from cartpoleplusplus_amd._lib import lib, check, ptr
    return lib, check, ptr


def _agent(case, inputs, capacity=None, **kw):
    """capacity: the batch size the agent is built with (None: the case's)"""
    from cartpoleplusplus_amd import ddpg_cartpole as D
    _cid, shape_name, A, B, opt, _clip, _tau, twin, weighted, n_step, pad = case
    shape = S.C_SHAPES[shape_name]
    opts = dict(hyper_options(S.composed_hyper(case)), soft_actor_critic=True, sac_init_temperature=S.C_TEMPERATURE,
                sac_temperature_learning_rate=S.C_TEMPERATURE_LR, sac_seed=S.C_NOISE_SEED, twin_q=twin, replay_memory_size=S.C_ROWS)
    opts.update(T3.opt_kw(opt))
    if weighted:
        opts.update(prioritized_replay=True, priority_alpha=S.PER["alpha"], priority_eps=S.PER["eps"], priority_beta=S.PER["beta"],
                    priority_beta_final=S.PER["beta"], sample_seed=S.PER["sample_seed"])
    if n_step > 1:
        opts["n_step"] = n_step
    if pad:
        opts["replay_store"] = "u8"
    opts.update(kw)
    make_opts(D, shape, B if capacity is None else int(capacity), len(shape) == 5, **opts)
    agent = D.DeepDeterministicPolicyGradientAgent(FakeEnv(shape, A))
    try:
        agent.initialise_variables(seed=1)
        agent.post_var_init_setup()
        specs, P, episodes = inputs[0], inputs[1], inputs[2]
        for net, p in zip(agent.networks(), P):
            assert net.get_params().shape == p.shape, (net.namespace, net.get_params().shape, p.shape)
            net.set_params(p)
        for ep in episodes:
            agent.replay_memory.add_episode(*ep)
        assert agent.replay_memory.size() == S.C_ROWS
        if weighted:
            agent.replay_memory.update_priorities(np.arange(S.C_ROWS), S.per_priorities())
        if pad:
            agent.replay_memory.enable_random_shift(pad, seed=S.C_SHIFT_SEED)
    except Exception:
        agent.close()
        raise
    return agent


def _state(agent):
    """tests.sac_np.ComposedSac.vectors() of the device"""
    t = agent.trainer
    f = lambda v: np.asarray(v, np.float64)
    out = {"actor": f(agent.actor.get_params()), "critic": f(agent.critic.get_params()), "target_critic": f(agent.target_critic.get_params())}
    n = len(out["actor"]) + len(out["critic"])
    if t.has_optimiser_slots():
        st = t.get_optimiser_state()
        assert len(st["m"]) == n
        out.update(m=f(st["m"]), v=f(st["v"]), step=[int(x) for x in st["step"]])
    else:
        out.update(m=np.zeros(n), v=np.zeros(n), step=[0, 0])
    sac = t.get_sac_state()
    out.update(log_alpha=float(sac["log_alpha"]), alpha_m=float(sac["m"]), alpha_v=float(sac["v"]), alpha_step=int(sac["step"]))
    return out


def _last_rows(agent, B):
    lib, check, ptr = _abi()
    rows = np.empty(B, np.int32)
    check(lib.cpp_replay_last_indexes(agent.replay_memory.handle, B, ptr(rows)))
    return rows


def _read_minibatch(agent, case, k, fused=True, rows=None):
    """what the last minibatch left on the device, in the shape tests.sac_np.ratios takes.  fused=False: behind critic.train of the single
    ops (the actor's half was read behind actor.train).  rows: the minibatch's row count (None: the case's)"""
    _cid, shape_name, A, B, _opt, _clip, _tau, twin, _w, _n, _pad = case
    B = B if rows is None else int(rows)
    t = agent.trainer
    sac = t.last_sac(B)
    assert sac["n"] == k, (sac["n"], k)
    for key, stream in (("eps", S.STREAM_S1), ("eps2", S.STREAM_S2)) if fused else (("eps2", S.STREAM_S2),):
        z = S.noise(S.C_NOISE_SEED, k, B, A, stream)
        assert float(np.max(np.abs(sac[key] - z))) <= S.eps_bar(), key
    acts, dq, q, td = t.last_values(B)
    if fused:
        np.testing.assert_array_equal(acts, sac["a"])
    q2, td2 = (None, td)
    if twin:
        q2, _tq1, _tq2, td2 = t.last_twin_values(B)
    stats = t.last_stats()
    got = {"actions": sac["a"], "target_actions": sac["a2"], "q": q, "q2": q2, "td": td, "td2": td2, "dq_da": dq, "logp": sac["logp"],
           "logp2": sac["logp2"], "r_soft": sac["r_soft"], "g_alpha": sac["g_alpha"], "loss": float(stats[0]), "actor_norm": float(stats[1]),
           "critic_norm": float(stats[2]), "actor_grads": agent.actor.get_grads(), "critic_grads": agent.critic.get_grads()}
    routes = None
    if shape_name != "lowdim":
        routes = (device_pool_codes(agent.actor, B), device_pool_codes(agent.critic, B), device_relu_active(agent.actor, B),
                  device_relu_active(agent.critic, B))
    return got, sac, routes


def _compare(case, inputs, refs, start, k, got, sac, routes, got_vec, batch, weights, run=""):
    """one minibatch from the common start `start`: refs = (float64 restatement, float32 twin)"""
    cid = case[0]
    outs, vecs = [], []
    for ref in refs:
        if k > 0:
            ref.set_state(start)
        outs.append(ref.train_minibatch(batch, sac["eps"], sac["eps2"], weights=weights, routes=routes))
        ref.update_targets()
        vecs.append(ref.vectors())
    want, want_vec = outs[0], vecs[0]
    flips = 0
    if routes is not None:
        flips += pool_flips_are_near_ties(want["cache_actor"], routes[0], what="actor") + pool_flips_are_near_ties(want["cache_critic"], routes[1], what="critic")
        flips += relu_flips_are_at_the_boundary(want["cache_actor"], routes[2], what="actor") + relu_flips_are_at_the_boundary(want["cache_critic"], routes[3], what="critic")
    r = S.ratios(case, inputs[0], start, got, got_vec, want, want_vec, outs[1], vecs[1])
    key = max(r, key=lambda x: r[x])
    print("%s minibatch %d: worst %s at %.3f of its bar; norms %.3f %.3f; %d route flips; %s" %
          (cid, k, key, r[key], got["actor_norm"], got["critic_norm"], flips, {a: "%.2f" % b for a, b in sorted(r.items())}))
    if r[key] > WORST.get(cid + run, (0.0,))[0]:
        WORST[cid + run] = (float(r[key]), k, key)
    # the lists once more through the project's own assertion, the float32 twin's distance where it is the larger tolerance
    cspec = S.critic_layout(case, inputs[0])
    f = lambda v: np.asarray(v, np.float64).reshape(-1)
    floor = 2.0 * max(float(np.max(np.abs(f(got["td"]) - f(want["td"])))), float(np.max(np.abs(f(got["td2"]) - f(want["td2"])))))
    assert_flat_close(inputs[0][0], got["actor_grads"], want["actor_grads"], rel=2e-5, what="%s minibatch %d actor pre-clip grads" % (cid, k),
                      rel_of=S.f32_rel_of(inputs[0][0], outs[1]["actor_grads"], want["actor_grads"]))
    assert_flat_close(cspec, got["critic_grads"], want["critic_grads"], rel=2e-5, what="%s minibatch %d critic pre-clip grads" % (cid, k),
                      abs_floor=floor, rel_of=S.f32_rel_of(cspec, outs[1]["critic_grads"], want["critic_grads"]))
    bad = {a: b for a, b in r.items() if not b <= 1.0}
    assert not bad, (cid, k, bad)
    return want, refs[0]


def _run(case, inputs, device_rows, capacity=None):
    """C_MINIBATCHES calls of one minibatch each (the weights, the shifts and eps can be read for the last minibatch of a call only).
    device_rows: the device draws (the first call is the eager pass and the capture, the others replay the graph).  capacity=C > B (the
    caller's rows, no shift): the agent is built for C rows and the four minibatches have C, B, B and C rows -- the last C of the case's
    rows in front and behind, its first two minibatches between them -- each from the device's own state, at the same bars."""
    cid, shape_name, A, B, _opt, clip, _tau, twin, weighted, n_step, pad = case
    sizes = None
    if capacity is not None:
        assert not device_rows and not pad
        sizes = S.partial_rows(case, inputs, capacity)
    agent = _agent(case, inputs, capacity=capacity, **({} if weighted or not device_rows else {"sample_seed": GRAPH_SAMPLE_SEED}))
    refs = (S.composed_restatement(case, inputs), S.composed_restatement(case, inputs, np.float32))
    restated_per = S.RestatedPer() if weighted else None
    try:
        rm = agent.replay_memory
        start = _state(agent)
        want0 = S.initial_state(inputs)
        for key in ("actor", "critic", "target_critic", "log_alpha"):
            np.testing.assert_array_equal(start[key], want0[key])
        for k in range(S.C_MINIBATCHES):
            weights = None
            if device_rows:
                agent.train_step(B, 1)
                rows = _last_rows(agent, B)
                if weighted:
                    weights = rm.last_weights(B).astype(np.float64).reshape(B, 1)
                    assert weights.min() > 0 and abs(weights.max() - 1.0) < 1e-6 and weights.max() - weights.min() > 1e-3, weights.ravel()
                    # the draw and its weights against tests.per_np on a tree kept with the device's own td_1: the rows equal; a leaf is
                    # the device's powf, 4 ulps of float32 from numpy's (tests/test_gpu_twin_q.py), so leaf / total is within 8 x 2^-23,
                    # its power -beta = -0.5 within half of that, the ratio to the batch maximum within twice that again, and the
                    # float32 store adds 2^-24: 1.0e-6 relative
                    r_rows, r_w = restated_per.draw(k, B)
                    assert np.array_equal(rows, r_rows), (cid, k, rows, r_rows)
                    rel = float(np.max(np.abs(weights.ravel() / r_w.ravel().astype(np.float64) - 1.0)))
                    print("%s minibatch %d: the restated draw; weights within %.1e relative" % (cid, k, rel))
                    assert rel <= 8 * 2.0 ** -23 + 2.0 ** -24, (cid, k, rel)
                else:
                    assert np.array_equal(rows, T3.device_rows(GRAPH_SAMPLE_SEED, k, B, S.C_ROWS)), "the rows are not the restated draw"
            elif sizes is not None:
                rows = np.ascontiguousarray(sizes[k], dtype=np.int32)
                agent.train_step(len(rows), 1, idxs=rows)
            else:
                rows = np.ascontiguousarray(inputs[3][k * B:(k + 1) * B], dtype=np.int32)
                agent.train_step(B, 1, idxs=rows)
            got, sac, routes = _read_minibatch(agent, case, k, rows=len(rows))
            got_vec = _state(agent)
            np.testing.assert_array_equal(agent.target_actor.get_params(), agent.actor.get_params())
            if pad:
                from tests.test_gpu_random_shift import _shifted_minibatch
                from tests import shift_np
                batch, _unshifted, sh = _shifted_minibatch(rm, rows)
                assert np.array_equal(sh, shift_np.shifts(S.C_SHIFT_SEED, k, B, pad))
            else:
                batch = S.composed_batches(case[:3] + (len(rows),) + case[4:], inputs[2], rows)[0]
                hb = rm.batch(idxs=rows)      # (the memory's own columns: the n-step fold is the restated one)
                np.testing.assert_array_equal(np.asarray(hb.reward), batch[2])
                np.testing.assert_array_equal(np.asarray(hb.terminal_mask), batch[3])
            want, ref = _compare(case, inputs, refs, start, k, got, sac, routes, got_vec, batch, weights, run=" (device-drawn rows)" if device_rows else "")
            if restated_per is not None:
                restated_per.update(rows, got["td"])
            if not device_rows or weighted:      # the conditions of tests/test_sac_host.py, on what the device ran
                for n, side in zip((got["actor_norm"], got["critic_norm"]), S.C_SIDES[cid]):
                    assert n >= 1.2 * clip if side == "above" else n <= clip / 1.2, (cid, k, side, n, clip)
                if twin:
                    assert 0.25 <= ref.min_share[-1] <= 0.75, (cid, k, ref.min_share)
            start = got_vec
        if got_vec["step"] != [0, 0]:
            assert got_vec["step"] == [S.C_MINIBATCHES] * 2
        assert got_vec["alpha_step"] == S.C_MINIBATCHES
        run = cid + (" (device-drawn rows)" if device_rows else "")
        print("%s: worst error / bar %.3f (minibatch %d, %s)" % ((run,) + WORST[run]))
    finally:
        agent.close()


GRAPH_SAMPLE_SEED = 0


# ---- 1. every case: four minibatches, one per call (each call an outer step: the critic's target update behind it), so that eps,
# the weights and the shifts of every minibatch can be read back
@pytest.mark.parametrize("cid", [c[0] for c in S.C_CASES])
def test_outer_steps_of_every_composed_case_against_the_float64_restatement(cid):
    case = S.composed_case(cid)
    _run(case, S.composed_inputs(case), device_rows=bool(case[8]))


def test_minibatches_below_the_capacity_against_the_float64_restatement():
    """(C, B) = (8, 5), scalar critic, Adam, both lists clipped (tests.sac_np.C_PARTIAL_CASE; its side of the clip over the four
    minibatches: tests/test_partial_batch_host.py): the policy's noise by row, log pi, the soft reward and the temperature's gradient at
    B behind a C-row minibatch, and at C again behind the B-row ones"""
    case = S.C_PARTIAL_CASE
    _run(case, S.composed_inputs(case), device_rows=False, capacity=S.C_PARTIAL_CAPACITY)


# ---- 2. graph replays on the rows the device draws
def test_graph_replays_on_device_drawn_rows_against_the_float64_restatement():
    """a uniform memory (twin, Adam, n-step 3) on the rows the device draws: one eager call (the capture), then three calls at the same
    key, which the trainer serves from its cached graph (tests/test_gpu_graph_cache.py; the runtime reports the form of a call only for
    the data-parallel step, so it is not asserted here); the noise count advances once per call (_read_minibatch).  The weighted case
    runs the same way above: a prioritized memory always draws on the device"""
    case = S.composed_case("twin-adam-nstep3-A2-B8")
    _run(case, S.composed_inputs(case), device_rows=True)


# ---- 3. the forms agree under composition
COMPOSED_FORM = dict(twin_q=True, ddpg_optimiser="Adam", gradient_clip=0.5)


def test_under_composition_eager_runs_graph_replays_and_repeated_runs_are_bit_identical():
    from tests.test_gpu_sac import _run_form
    eager, _ = _run_form("eager", **COMPOSED_FORM)
    graph, sac = _run_form("graph", **COMPOSED_FORM)
    again, _ = _run_form("graph", **COMPOSED_FORM)
    for x, y, z in zip(eager, graph, again):
        np.testing.assert_array_equal(x, y)
        np.testing.assert_array_equal(y, z)
    assert [o["n"] for o in sac] == [1, 3, 5]
    np.testing.assert_array_equal(graph[0], graph[2])                # target actor == actor


def test_under_composition_the_literal_loops_deferred_pairs_are_the_fused_minibatch_on_rows_bit_for_bit():
    from tests.test_gpu_sac import _run_form
    literal, sac_l = _run_form("literal", **COMPOSED_FORM)
    rows, sac_r = _run_form("rows", **COMPOSED_FORM)
    for x, y in zip(literal, rows):
        np.testing.assert_array_equal(x, y)
    assert [o["n"] for o in sac_l] == list(range(6)) == [o["n"] for o in sac_r]
    np.testing.assert_array_equal(literal[0], literal[2])


# ---- 4. the single ops on host arrays
def test_the_single_ops_under_twin_heads_and_momentum_with_the_clip_engaged():
    """actor.train(s1) then critic.train(batch) on host arrays, three minibatches: each op advances its own list's count only, and the
    pair is the restated minibatch"""
    case, seed, nb = S.C_SINGLE_OPS
    cid, _sn, A, B, _opt, clip, _tau, _twin, _w, _n, _pad = case
    inputs = S.composed_inputs(case, seed=seed, nb=nb)
    agent = _agent(case, inputs)
    refs = (S.composed_restatement(case, inputs), S.composed_restatement(case, inputs, np.float32))
    try:
        t = agent.trainer
        start = _state(agent)
        for k in range(nb):
            hb = HostBatch(*inputs[4][k])
            agent.actor.train(hb.state_1)
            assert [int(x) for x in t.get_optimiser_state()["step"]] == [k + 1, k]
            first, a_norm, g_a = t.last_sac(B), float(t.last_stats()[1]), agent.actor.get_grads()
            dq = t.last_values(B)[1]
            assert float(np.max(np.abs(first["eps"] - S.noise(S.C_NOISE_SEED, k, B, A, S.STREAM_S1)))) <= S.eps_bar()
            agent.critic.train(hb)
            assert [int(x) for x in t.get_optimiser_state()["step"]] == [k + 1, k + 1]
            agent.target_actor.update_weights()
            agent.target_critic.update_weights()
            got, sac, routes = _read_minibatch(agent, case, k, fused=False)
            got.update(actor_norm=a_norm, actor_grads=g_a, actions=first["a"], logp=first["logp"], g_alpha=first["g_alpha"], dq_da=dq)
            sac = dict(sac, eps=first["eps"])
            got_vec = _state(agent)
            np.testing.assert_array_equal(agent.target_actor.get_params(), agent.actor.get_params())
            _compare(case, inputs, refs, start, k, got, sac, routes, got_vec, inputs[4][k], None)
            assert got["actor_norm"] >= 1.2 * clip and got["critic_norm"] >= 1.2 * clip, (got["actor_norm"], got["critic_norm"])
            assert 0.25 <= refs[0].min_share[-1] <= 0.75, refs[0].min_share
            start = got_vec
        print("%s: worst error / bar %.3f (minibatch %d, %s)" % ((cid,) + WORST[cid]))
    finally:
        agent.close()
