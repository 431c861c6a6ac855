"""Feature layer norm on the device (--feature-layer-norm; cpp_net_create_feature_norm, csrc/ln.hip) against the float64 restatement
tests/layer_norm_np.py.  The cases, their bars and what they can see are that module's and tests/test_layer_norm_host.py's: every
kernel-edge quantity is held to the bar its float32 twin derives (8 x the twin's own error, or the ordinary 1e-5), every whole
minibatch to the ordinary bars of tests.helpers.fused_step_against_f64_oracle and to tests.helpers.delta_bound.

16x16x6 images, replay memories of 24 - 64 rows: every case is seconds."""
import ctypes
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle import ddpg_np as O
from tests import layer_norm_np as L
from tests.helpers import (FakeEnv, _profiled_calls, assert_flat_close, ddpg_path, delta_bound, device_pool_codes, device_relu_active,
                           hyper_options, make_opts, pool_flips_are_near_ties, relu_flips_are_at_the_boundary, twin_rs)

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPP_ERR_ARG, CPP_ERR_STATE = 1, 3
SHAPE = L.WHOLE_SHAPE


def _abi():
    from cartpoleplusplus_amd._lib import lib, check, ptr
    return lib, check, ptr


def _agent(B, hidden, act, hp, P=None, episodes=None, rows=24, norm=True, opt=None, seed=0, capacity=None, **kw):
    """a device agent through the public Python surface, holding P and the episodes (None: its own initialisation, an empty memory);
    capacity: the batch size it is built with (None: B)"""
    from cartpoleplusplus_amd import ddpg_cartpole as D
    from tests import ddpg_opt_np as R
    if opt is not None:
        name, args = R.OPTIMISERS[opt]
        kw.update(ddpg_optimiser=name, ddpg_optimiser_args=json.dumps(args))
    if norm:
        kw.update(feature_layer_norm=True, feature_norm_activation=act)
    kw.update(hyper_options(hp))
    make_opts(D, SHAPE, B if capacity is None else int(capacity), True, replay_memory_size=rows,
              actor_hidden_layers=",".join(str(h) for h in hidden), **kw)
    agent = D.DeepDeterministicPolicyGradientAgent(FakeEnv(SHAPE, 2))
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


def _params(agent):
    return [n.get_params() for n in agent.networks()]


def _routes(agent, B):
    return ((device_pool_codes(agent.actor, B), device_relu_active(agent.actor, B)),
            (device_pool_codes(agent.critic, B), device_relu_active(agent.critic, B)))


def _pinned_oracle(specs, P, hp, routes):
    ref = L.restatement(specs, P, np.float64, hp)
    (ref.actor.amax_override, ref.actor.relu_override), (ref.critic.amax_override, ref.critic.relu_override) = routes
    return ref


def _flips(ag, cg, routes):
    (ca, ra), (cc, rc) = routes
    return (pool_flips_are_near_ties(ag["cache_actor"], ca, what="actor") + pool_flips_are_near_ties(cg["cache_critic"], cc, what="critic")
            + relu_flips_are_at_the_boundary(ag["cache_actor"], ra, what="actor") + relu_flips_are_at_the_boundary(cg["cache_critic"], rc, what="critic"))


# ---- 1. kernel edges, through last_feature_norm: widths 5 .. 1024 (the critic's: 200), B = 1 .. 33, both activations
def wide_edge_case(case, capacity):
    """an edge case with its minibatch replaced by rows 0 .. capacity-1 of its memory: (the case, the rows)"""
    from tests.helpers import minibatch_of_rows
    rows = np.arange(capacity, dtype=np.int32)
    return case[:3] + (rows, [minibatch_of_rows(L.EDGE_ROWS, SHAPE, 2, case[2], rows)]) + case[5:], rows


def _edge(case, act, B, hidden, capacity=None):
    """capacity=C > B: the agent is built for C rows; a C-row minibatch (rows 0 .. C-1) and one at B run first and the parameters are put
    back, the checked minibatch follows, the parameters are put back once more and the C-row minibatch is held to its own bars"""
    specs, P, episodes, idxs, batches = case[:5]
    hp = O.DEFAULT_HYPER
    agent = _agent(B, hidden, act, hp, P, episodes, rows=L.EDGE_ROWS, capacity=capacity)
    wide = back = None
    try:
        if capacity is not None:
            assert capacity > B
            wide, rows = wide_edge_case(case, capacity)
            agent.train_step(capacity, 1, idxs=rows)
            agent.train_step(B, 1, idxs=idxs)
            for net, p in zip(agent.networks(), P):
                net.set_params(p)
        agent.train_step(B, 1, idxs=idxs)
        got = agent.trainer.last_feature_norm(B)
        routes = _routes(agent, B)
        if capacity is not None:
            for net, p in zip(agent.networks(), P):
                net.set_params(p)
            agent.train_step(capacity, 1, idxs=rows)
            back = (agent.trainer.last_feature_norm(capacity), _routes(agent, capacity))
    finally:
        agent.close()
    q = _check_edge(case, got, routes)
    if back is not None:
        _check_edge(wide, back[0], back[1])
    return got, q


def _check_edge(case, got, routes):
    specs, P, _episodes, _idxs, batches = case[:5]
    hp = O.DEFAULT_HYPER
    q, ag, cg = L.ln_quantities(_pinned_oracle(specs, P, hp, routes), batches[0])
    flips = _flips(ag, cg, routes)
    bars, _q = L.edge_bars(case)
    bad = []
    for net in ("actor", "critic"):
        for k in L.LN_QUANTITIES:
            e, (e32, bar) = L.rel_err(got[net][k], q[net][k]), bars[(net, k)]
            print("  %-6s %-6s err %.2e  twin %.2e  bar %.2e" % (net, k, e, e32, bar))
            assert np.isfinite(got[net][k]).all()
            if not e <= bar:
                bad.append((net, k, e, bar))
    print("  (%d route flips at ties)" % flips)
    assert not bad, bad
    return q


def test_a_kernel_edge_below_the_capacity_against_float64():
    """(C, B) = (8, 5), width 65, ReLU: the per-row statistics, xhat, y and the dgamma / dbeta partials of both feature layers at B behind
    a C-row minibatch, and at C again behind the B-row ones (tests.layer_norm_np.conditions hold on the C-row minibatch too:
    tests/test_partial_batch_host.py)"""
    _edge(L.edge_case("w65-b5-relu"), "relu", 5, (65,) + L.EDGE_TAIL, capacity=8)


@pytest.mark.parametrize("cid", [c[0] for c in L.EDGE_CASES])
def test_kernel_edges_against_float64(cid):
    _cid, width, B, act = [c for c in L.EDGE_CASES if c[0] == cid][0]
    _edge(L.edge_case(cid), act, B, (width,) + L.EDGE_TAIL)


def test_a_dead_feature_layer():
    """layer-0 weights zero, biases one constant: var = 0 exactly, xhat = 0, y = act(beta), rstd = 1 / sqrt(eps), dz finite"""
    case = L.edge_case("w65-b5-relu", dead=True)
    got, q = _edge(case, "relu", 5, (65,) + L.EDGE_TAIL)
    for net in ("actor", "critic"):
        assert not got[net]["xhat"].any() and not got[net]["dgamma"].any()
        assert np.array_equal(got[net]["rstd"], np.full(5, np.float32(1.0) / np.sqrt(np.float32(L.EPS)), np.float32))
    beta = case[1][0][-65:]
    assert np.array_equal(got["actor"]["y"], np.maximum(beta, 0)[None].repeat(5, 0))


# ---- 2. whole minibatches against the float64 restatement
@pytest.mark.parametrize("cid", list(L.WHOLE_CASES))
def test_whole_minibatches_against_the_float64_restatement(cid):
    hidden, act, nb, opt, clip, route = L.WHOLE_CASES[cid]
    specs, P, episodes, idxs, batches, seed, want, outs, twin = L.whole_case(cid)
    hp, B = L.whole_hyper(cid), L.WHOLE_B
    agent = _agent(B, hidden, act, hp, P, episodes, rows=L.WHOLE_ROWS, opt=opt)
    try:
        if opt is None:      # the route of this shape: one profiled minibatch, then the case's parameters again
            path = ddpg_path(agent, B, list(hidden), [], True)
            assert route in path.split("|"), (cid, path)
            for net, p in zip(agent.networks(), P):
                net.set_params(p)
        agent.train_step(B, nb, idxs=idxs)
        actions, dq_da, q, td = agent.trainer.last_values(B)
        g_a, g_c = agent.actor.get_grads(), agent.critic.get_grads()
        stats = agent.trainer.last_stats()
        got = _params(agent)
        slots = None
        if opt is not None:
            st = agent.trainer.get_optimiser_state()
            slots, steps = [st["m"].astype(np.float64), st["v"].astype(np.float64)], [int(x) for x in st["step"]]
            assert steps == [nb, nb]
        routes = _routes(agent, B)
    finally:
        agent.close()
    print("%s (seed %d): device norms %.4f %.4f, oracle %s" % (cid, seed, stats[1], stats[2], [(round(o["actor_norm"], 4), round(o["critic_norm"], 4)) for o in outs]))
    if nb == 1:      # the per-row values and both lists per variable, on the device's routes (accepted only at ties)
        ref = _pinned_oracle(specs, P, hp, routes)
        _q, ag, cg = L.ln_quantities(ref, batches[0])
        flips = _flips(ag, cg, routes)
        err = {"actions": np.abs(actions - ag["actions"]).max(), "dq_da": np.abs(dq_da - ag["dq_da"]).max(), "q": np.abs(q - cg["q"]).max(),
               "td": np.abs(td - cg["td"]).max(), "loss": abs(stats[0] - cg["loss"]) / max(1.0, abs(cg["loss"]))}
        print("  %s, %d route flips at ties" % ({k: "%.2e" % v for k, v in err.items()}, flips))
        assert max(err.values()) < 1e-5, err
        assert_flat_close(specs[0], g_a, ag["grads"], rel=2e-5, what="actor pre-clip grads vs f64")
        assert_flat_close(specs[1], g_c, cg["grads"], rel=2e-5, what="critic pre-clip grads vs f64", abs_floor=2.0 * float(err["td"]))
        if flips:
            want, outs = L.run_whole(specs, P, batches, hp, opt, pin=[routes])
    else:
        assert np.abs(td - outs[-1]["td"]).max() < 1e-5
    na, nc = outs[-1]["actor_norm"], outs[-1]["critic_norm"]
    assert abs(stats[1] - na) < 1e-4 * max(1.0, na) and abs(stats[2] - nc) < 1e-4 * max(1.0, nc), (stats, na, nc)
    start = list(P) + [np.zeros_like(want[4]), np.zeros_like(want[5])]
    rs = twin_rs(want, twin, start)
    bad = []
    for name, g, w, p, r in zip(("actor", "critic", "target_actor", "target_critic", "m", "v"), got + (slots or []), want, start, rs):
        errn, bound = float(np.linalg.norm(np.asarray(g, np.float64) - w)), delta_bound(p, w - p, r, nb)
        print("  %-13s |err| %.3e  bound %.3e" % (name, errn, bound))
        if not errn <= bound:
            bad.append((name, errn, bound))
        # (gamma and beta on their own: the tail of the vector moved, and as the restatement says)
        k = specs[0].num_plain() if "actor" in name else specs[1].num_plain() if "critic" in name else None
        if k is not None and not np.linalg.norm(np.asarray(g[k:], np.float64) - w[k:]) <= delta_bound(p[k:], w[k:] - p[k:], max(r, 5e-5), nb):
            bad.append((name + " gamma/beta", float(np.linalg.norm(g[k:] - w[k:]))))
        if k is not None:
            assert np.abs(w[k:] - p[k:]).max() > 0
    assert not bad, (cid, bad)


# ---- 2b. twin Q heads against tests.twin_np's restatement composed with the norm
@pytest.mark.parametrize("cid", list(L.TWIN_CASES))
def test_twin_q_minibatches_against_the_float64_restatement(cid):
    from tests import twin_np as W
    opt, nb, _clip = L.TWIN_CASES[cid]
    specs, P, episodes, idxs, batches, seed, want, outs, twin = L.twin_case(cid)
    hp, B = L.twin_hyper(cid), L.WHOLE_B
    dev = lambda v: L.twin_to_device(specs[1], v)
    back = lambda v: L.twin_from_device(specs[1], np.asarray(v))
    agent = _agent(B, (65, 20, 10), "tanh", hp, [P[0], dev(P[1]), P[2], dev(P[3])], episodes, rows=L.WHOLE_ROWS,
                   opt=None if opt == "gradient-descent" else opt, twin_q=True)
    try:
        names = [v.name.split("/", 1)[1] for v in agent.critic.trainable_model_vars()]
        assert names[-6:] == ["hidden3b/weights:0", "hidden3b/biases:0", "q_valueb/weights:0", "q_valueb/biases:0", "hidden1/LayerNorm/gamma:0", "hidden1/LayerNorm/beta:0"]
        census = _profiled_calls(agent.actor.ctx, lambda: agent.train_step(B, 1, idxs=idxs[:B]))
        assert (census.get("heads", 0), census.get("ln_fwd", 0), census.get("ln_bwd", 0), census.get("sumsq", 0)) == (1, 1, 2, 0), census
        for net, p in zip(agent.networks(), [P[0], dev(P[1]), P[2], dev(P[3])]):
            net.set_params(p)
        if opt != "gradient-descent":
            st = agent.trainer.get_optimiser_state()
            agent.trainer.set_optimiser_state({"m": np.zeros_like(st["m"]), "v": np.zeros_like(st["v"]), "step": np.zeros(2, np.uint64)})
        agent.train_step(B, nb, idxs=idxs)
        actions, dq_da, q, td = agent.trainer.last_values(B)
        q2, tq1, tq2, td2 = agent.trainer.last_twin_values(B)
        g_a, g_c = agent.actor.get_grads(), back(agent.critic.get_grads())
        stats = agent.trainer.last_stats()
        a, c, ta, tc = _params(agent)
        got = [a, back(c), ta, back(tc)]
        if opt != "gradient-descent":
            st = agent.trainer.get_optimiser_state()
            nA = len(a)
            got += [np.concatenate([st[k][:nA], back(st[k][nA:])]).astype(np.float64) for k in ("m", "v")]
            assert [int(x) for x in st["step"]] == [nb, nb]
        routes = _routes(agent, B)
    finally:
        agent.close()
    if nb == 1:
        want, outs, _ref = L.run_twin(specs, P, batches, hp, opt, pin=[routes])
    ag, cg = outs[-1]["ag"], outs[-1]["cg"]
    if nb == 1:
        flips = _flips(ag, cg, routes)
        print("  %d route flips at ties" % flips)
    err = {"actions": np.abs(actions - ag["actions"]).max(), "dq_da": np.abs(dq_da - ag["dq_da"]).max(), "q": np.abs(q - cg["q"]).max(),
           "q2": np.abs(q2 - cg["q2"]).max(), "tq1": np.abs(tq1 - cg["target_q"]).max(), "tq2": np.abs(tq2 - cg["target_q2"]).max(),
           "td": np.abs(td - cg["td"]).max(), "td2": np.abs(td2 - cg["td2"]).max(), "loss": abs(stats[0] - cg["loss"]) / max(1.0, abs(cg["loss"]))}
    print("%s (seed %d): %s" % (cid, seed, {k: "%.2e" % v for k, v in err.items()}))
    assert max(err.values()) < 1e-5, err
    assert_flat_close(specs[0], g_a, ag["grads"], rel=2e-5, what="actor pre-clip grads vs f64")
    assert_flat_close(W.TwinLayoutSpec(specs[1]), g_c, cg["grads"], rel=2e-5, what="twin critic pre-clip grads vs f64", abs_floor=2.0 * float(max(err["td"], err["td2"])))
    na, nc = outs[-1]["actor_norm"], outs[-1]["critic_norm"]
    assert abs(stats[1] - na) < 1e-4 * max(1.0, na) and abs(stats[2] - nc) < 1e-4 * max(1.0, nc), (stats, na, nc)
    start = list(P) + [np.zeros_like(want[4]), np.zeros_like(want[5])]
    rs = twin_rs(want, twin, start)
    bad = []
    for name, g, w, p, r in zip(("actor", "critic", "target_actor", "target_critic", "m", "v"), got, want, start, rs):
        errn, bound = float(np.linalg.norm(np.asarray(g, np.float64) - w)), delta_bound(p, w - p, r, nb)
        print("  %-13s |err| %.3e  bound %.3e" % (name, errn, bound))
        if not errn <= bound:
            bad.append((name, errn, bound))
    assert not bad, (cid, bad)


# ---- 2b'. the categorical and the quantile critic (the GEMM levels) against tests.dist_np / tests.quant_np composed with the norm
@pytest.mark.parametrize("cid", list(L.VALUE_CASES))
def test_distributional_and_quantile_minibatches_against_the_float64_restatement(cid):
    kind, opt, nb, _clip = L.VALUE_CASES[cid]
    specs, P, episodes, idxs, batches, seed, want, outs, twin = L.value_case(cid)
    hp, B = L.value_hyper(cid), L.WHOLE_B
    kw = dict(distributional_critic=True, num_atoms=L.DIST[0], v_min=L.DIST[1], v_max=L.DIST[2]) if kind == "dist" else \
        dict(quantile_critic=True, num_quantiles=L.QUANT[0], quantile_huber_kappa=L.QUANT[1], drop_top_quantiles=L.QUANT[2])
    agent = _agent(B, (65, 20, 10), "tanh", hp, P, episodes, rows=L.WHOLE_ROWS, opt=opt, **kw)
    try:
        census = _profiled_calls(agent.actor.ctx, lambda: agent.train_step(B, 1, idxs=idxs[:B]))
        assert (census.get("heads", 0), census.get("ln_fwd", 0), census.get("ln_bwd", 0), census.get("sumsq", 0)) == (0, 1, 2, 0), census
        for net, p in zip(agent.networks(), P):
            net.set_params(p)
        st = agent.trainer.get_optimiser_state()
        agent.trainer.set_optimiser_state({"m": np.zeros_like(st["m"]), "v": np.zeros_like(st["v"]), "step": np.zeros(2, np.uint64)})
        agent.train_step(B, nb, idxs=idxs)
        actions, dq_da, q, td = agent.trainer.last_values(B)
        g_a, g_c = agent.actor.get_grads(), agent.critic.get_grads()
        stats = agent.trainer.last_stats()
        st = agent.trainer.get_optimiser_state()
        got = _params(agent) + [st["m"].astype(np.float64), st["v"].astype(np.float64)]
        assert [int(x) for x in st["step"]] == [nb, nb]
        fn = agent.trainer.last_feature_norm(B)
    finally:
        agent.close()
    ag, cg = outs[-1]["ag"], outs[-1]["cg"]
    err = {"actions": np.abs(actions - ag["actions"]).max(), "dq_da": np.abs(dq_da - ag["dq_da"]).max(), "q": np.abs(q - cg["q"]).max(),
           "td": np.abs(td - cg["td"]).max(), "loss": abs(stats[0] - cg["loss"]) / max(1.0, abs(cg["loss"]))}
    for name, cache in (("actor", ag["cache_actor"]), ("critic", cg["cache_critic"])):
        for k in ("dz", "dgamma", "dbeta"):
            err["%s %s" % (name, k)] = L.rel_err(fn[name][k], cache["ln"][k])
    print("%s (seed %d): %s" % (cid, seed, {k: "%.2e" % v for k, v in err.items()}))
    assert max(err.values()) < 1e-5, err
    assert_flat_close(specs[0], g_a, ag["grads"], rel=2e-5, what="actor pre-clip grads vs f64")
    assert_flat_close(specs[1], g_c, cg["grads"], rel=2e-5, what="critic pre-clip grads vs f64")
    na, nc = outs[-1]["actor_norm"], outs[-1]["critic_norm"]
    assert abs(stats[1] - na) < 1e-4 * max(1.0, na) and abs(stats[2] - nc) < 1e-4 * max(1.0, nc), (stats, na, nc)
    start = list(P) + [np.zeros_like(want[4]), np.zeros_like(want[5])]
    bad = []
    for name, g, w, p, r in zip(("actor", "critic", "target_actor", "target_critic", "m", "v"), got, want, start, twin_rs(want, twin, start)):
        errn, bound = float(np.linalg.norm(np.asarray(g, np.float64) - w)), delta_bound(p, w - p, r, nb)
        print("  %-13s |err| %.3e  bound %.3e" % (name, errn, bound))
        if not errn <= bound and np.linalg.norm(w - p) > 0:
            bad.append((name, errn, bound))
    assert not bad, (cid, bad)


# ---- 2b''. prioritized replay + n-step 3 + the u8 store + random shift: the minibatch the device formed, rebuilt on the host
def test_per_nstep_u8_and_random_shift_against_the_float64_restatement():
    """two warm minibatches on device-drawn rows (the priorities and with them the weights move), then the checked one: its rows, weights
    and shifts read back, the minibatch rebuilt by the features' own restatements (the memory's n-step columns, tests/shift_np.py), the
    float64 restatement on the device's routes with the weights on the critic's loss -- per-row values, both lists per variable, both
    norms, the clipped update at delta_bound, the targets at f32 rounding of their soft update of the device's new parameters"""
    from tests.test_gpu_random_shift import _shifted_minibatch
    lib, check, ptr = _abi()
    B, rows, hidden = 8, 64, (65, 20, 10)
    hp = O.Hyper(1e-2, 5e-2, 0.9, 0.5, 0.25)
    specs, P0, episodes, _i, _b = L.host_case(SHAPE, B, 1, 4, hidden, "tanh", rows=rows)
    u8 = lambda x: np.rint(np.asarray(x, np.float32) * 255).astype(np.uint8)
    episodes = [(u8(f), [(a, r, u8(s2)) for a, r, s2 in seq]) for f, seq in episodes]
    agent = _agent(B, hidden, "tanh", hp, P0, episodes, rows=rows, sample_seed=5, prioritized_replay=True, priority_alpha=0.6, priority_beta=0.4,
                   priority_eps=1e-6, n_step=3, replay_store="u8")
    try:
        rm = agent.replay_memory
        rm.enable_random_shift(2, seed=9)
        agent.train_step(B, 1)
        agent.train_step(B, 1)
        P = _params(agent)
        agent.train_step(B, 1)
        idxs = np.empty(B, np.int32)
        check(lib.cpp_replay_last_indexes(rm.handle, B, ptr(idxs)))
        w = rm.last_weights(B).astype(np.float64).reshape(B, 1)
        t, _un, _sh = _shifted_minibatch(rm, idxs)
        actions, dq_da, q, td = agent.trainer.last_values(B)
        g_a, g_c = agent.actor.get_grads(), agent.critic.get_grads()
        stats = agent.trainer.last_stats()
        got = _params(agent)
        routes = _routes(agent, B)
        fn = agent.trainer.last_feature_norm(B)
    finally:
        agent.close()
    m = np.asarray(t[3]).ravel()
    assert np.ptp(w) > 1e-3 and ((m > 0) & (m < 1)).any(), (w.ravel(), m)      # (weights that differ; folded masks: discount^2)
    upd = {}
    for dt in (np.float64, np.float32):
        ref = _pinned_oracle(specs, P, hp, routes) if dt is np.float64 else L.restatement(specs, P, dt, hp)
        if dt is np.float32:
            (ref.actor.amax_override, ref.actor.relu_override), (ref.critic.amax_override, ref.critic.relu_override) = routes
        ag, cg = ref.actor_gradients(t[0]), ref.critic_gradients(t)
        cgw = ref.critic_gradients(t, td_override=w.astype(dt) * cg["td"])
        ca, na = O.clip_by_global_norm(ag["grads"], hp.gradient_clip, dt)
        cc, nc = O.clip_by_global_norm(cgw["grads"], hp.gradient_clip, dt)
        upd[dt] = [np.asarray(P[0].astype(dt) - dt(hp.actor_lr) * ca, np.float64), np.asarray(P[1].astype(dt) - dt(hp.critic_lr) * cc, np.float64)]
        if dt is np.float64:
            flips = _flips(ag, cg, routes)
            err = {"actions": np.abs(actions - ag["actions"]).max(), "dq_da": np.abs(dq_da - ag["dq_da"]).max(), "q": np.abs(q - cg["q"]).max(),
                   "td": np.abs(td - cg["td"]).max(), "loss": abs(stats[0] - float((w * cg["td"] ** 2).mean()))}
            for name, cache in (("actor", ag["cache_actor"]), ("critic", cgw["cache_critic"])):
                for k in ("xhat", "y", "dz", "dgamma", "dbeta"):
                    err["%s %s" % (name, k)] = L.rel_err(fn[name][k], cache["ln"][k])
            print("per + n-step + u8 + shift: %s, %d route flips at ties" % ({k: "%.2e" % v for k, v in err.items()}, flips))
            assert max(err.values()) < 1e-5, err
            assert_flat_close(specs[0], g_a, ag["grads"], rel=2e-5, what="actor pre-clip grads vs f64")
            assert_flat_close(specs[1], g_c, cgw["grads"], rel=2e-5, what="critic pre-clip grads vs f64", abs_floor=2.0 * float(err["td"]))
            assert min(na, nc) > 1.2 * hp.gradient_clip
            assert abs(stats[1] - na) < 1e-4 * max(1.0, na) and abs(stats[2] - nc) < 1e-4 * max(1.0, nc), (stats, na, nc)
    rs = twin_rs(upd[np.float64], upd[np.float32], P[:2])
    for name, g, wv, p, r in zip(("actor", "critic"), got[:2], upd[np.float64], P[:2], rs):
        e, bound = float(np.linalg.norm(g.astype(np.float64) - wv)), delta_bound(p, wv - p, r, 1)
        print("  %-7s |err| %.3e  bound %.3e" % (name, e, bound))
        assert e <= bound, (name, e, bound)
    for j in (0, 1):
        wt = O.soft_update(P[2 + j], got[j], hp.target_update_rate, np.float64)
        assert float(np.linalg.norm(got[2 + j] - wt)) <= 2.0 ** -23 * float(np.linalg.norm(wt)), ("target", j)


# ---- 2b-sac. soft actor-critic (the GEMM levels, sac.hip's jobs above the norm) against tests.sac_np composed with the norm
def test_a_soft_actor_critic_minibatch_against_the_float64_restatement():
    """one minibatch under gradient descent with the clip engaged; the device's own noise of both draws (last_sac) feeds the restatement"""
    specs, P, episodes, idxs, batches = L.sac_case()
    hp, B = L.sac_hyper(), L.WHOLE_B
    agent = _agent(B, (65, 20, 10), "tanh", hp, P, episodes, rows=L.WHOLE_ROWS, soft_actor_critic=True)
    try:
        census = _profiled_calls(agent.actor.ctx, lambda: agent.train_step(B, 1, idxs=idxs))
        assert (census.get("heads", 0), census.get("ln_fwd", 0), census.get("ln_bwd", 0), census.get("sumsq", 0)) == (0, 1, 2, 0) and census.get("sac", 0) >= 3, census
        for net, p in zip(agent.networks(), P):
            net.set_params(p)
        sc = agent.trainer.sac
        agent.trainer.set_sac(sc["init_temperature"], sc["target_entropy"], sc["temperature_learning_rate"], sc["seed"])
        assert np.array_equal(agent.target_actor.get_params(), P[0])
        agent.train_step(B, 1, idxs=idxs)
        sac = agent.trainer.last_sac(B)
        _a, dq_da, q, td = agent.trainer.last_values(B)
        g_a, g_c = agent.actor.get_grads(), agent.critic.get_grads()
        stats = agent.trainer.last_stats()
        got = _params(agent)
        routes = _routes(agent, B)
        fn = agent.trainer.last_feature_norm(B)
    finally:
        agent.close()
    assert np.abs(sac["eps"]).max() > 0 and np.abs(sac["eps2"]).max() > 0
    want, out, ag, cg = L.run_sac(specs, P, batches[0], sac["eps"], sac["eps2"], np.float64, routes)
    twin, _o, _a32, _c32 = L.run_sac(specs, P, batches[0], sac["eps"], sac["eps2"], np.float32, routes)
    flips = _flips(ag, cg, routes)
    err = {"a": np.abs(sac["a"] - ag["actions"]).max(), "logp": np.abs(sac["logp"] - np.asarray(ag["logp"]).ravel()).max(), "a2": np.abs(sac["a2"] - cg["target_actions"]).max(),
           "r_soft": np.abs(sac["r_soft"] - np.asarray(cg["r_soft"]).ravel()).max(), "dq_da": np.abs(dq_da - ag["dq_da"]).max(), "q": np.abs(q - cg["q"]).max(),
           "td": np.abs(td - cg["td"]).max(), "loss": abs(stats[0] - cg["loss"]) / max(1.0, abs(cg["loss"])),
           "head dz": np.abs(sac["dz"] - np.concatenate([ag["dm"], ag["dx"]], axis=1)).max()}
    for name, cache in (("actor", ag["cache_actor"]), ("critic", cg["cache_critic"])):
        for k in ("xhat", "y", "dz", "dgamma", "dbeta"):
            err["%s %s" % (name, k)] = L.rel_err(fn[name][k], cache["ln"][k])
    print("soft actor-critic: %s, %d route flips at ties" % ({k: "%.2e" % v for k, v in err.items()}, flips))
    assert max(err.values()) < 1e-5, err
    assert_flat_close(specs[0], g_a, ag["grads"], rel=2e-5, what="actor pre-clip grads vs f64")
    assert_flat_close(specs[1], g_c, cg["grads"], rel=2e-5, what="critic pre-clip grads vs f64", abs_floor=2.0 * float(err["td"]))
    na, nc = float(out["actor_norm"]), float(out["critic_norm"])
    assert min(na, nc) > 1.2 * L.SAC_CLIP
    assert abs(stats[1] - na) < 1e-4 * max(1.0, na) and abs(stats[2] - nc) < 1e-4 * max(1.0, nc), (stats, na, nc)
    start = [P[0], P[1], P[3]]
    for name, g, w, p, r in zip(("actor", "critic", "target_critic"), (got[0], got[1], got[3]), want, start, twin_rs(want, twin, start)):
        e, bound = float(np.linalg.norm(g.astype(np.float64) - w)), delta_bound(p, w - p, r, 1)
        print("  %-13s |err| %.3e  bound %.3e" % (name, e, bound))
        assert e <= bound, (name, e, bound)
    k = specs[0].num_plain()
    assert np.array_equal(got[2], got[0]) and np.abs(got[0][k:] - P[0][k:]).max() > 0      # the target actor is the actor, gamma / beta included


# ---- 2c. the single train ops are the pass's halves: the same bits on the GEMM levels (tests/test_gpu_single_ops_are_the_pass.py's form)
@pytest.mark.parametrize("hidden,A", [((65,), 2), ((65, 20, 10), 9)], ids=["one-hidden-A2", "default-A9"])
def test_the_single_ops_leave_the_bits_the_pass_leaves(hidden, A):
    """two trainers from the same numbers, one host batch: cpp_ddpg_compute_gradients (both halves; the GEMM levels: one hidden layer, or
    nine actions) against q_gradients_wrt_actions, check_loss, train_actor and train_critic, whose ln launches carry one, three, one and
    three jobs where the pass's carry four and two.  Byte for byte: dq_da, td, every last_feature_norm quantity, the fully connected
    slices of both lists with gamma and beta (the conv slices come from other launches on the two sides)"""
    import collections
    from cartpoleplusplus_amd import ddpg_cartpole as D
    lib, check, ptr = _abi()
    B = 8
    HostBatch = collections.namedtuple("HostBatch", "state_1 action reward terminal_mask state_2")
    hb = HostBatch(*O.synthetic_batch(np.random.default_rng(5), B, SHAPE, A, True))

    def make():
        make_opts(D, SHAPE, B, True, replay_memory_size=8, feature_layer_norm=True, actor_hidden_layers=",".join(str(h) for h in hidden))
        agent = D.DeepDeterministicPolicyGradientAgent(FakeEnv(SHAPE, A))
        agent.initialise_variables(seed=0)
        rng = np.random.default_rng(100)
        for nets, sd, hook in (((agent.actor, agent.critic), 0.05, agent.post_var_init_setup), ((agent.target_actor, agent.target_critic), 0.01, None)):
            for net in nets:
                p = net.get_params()
                net.set_params(p + rng.normal(0, sd, p.shape).astype(np.float32))
            if hook:
                hook()
        return agent
    whole, single = make(), make()
    try:
        tr = whole.trainer
        dev = tr.device_batch_for(hb)
        seen = _profiled_calls(whole.actor.ctx, lambda: check(lib.cpp_ddpg_compute_gradients(tr.handle, dev.handle)))
        assert (seen.get("heads", 0), seen.get("ln_fwd", 0), seen.get("ln_bwd", 0)) == (0, 1, 2), seen
        _a, dq_da, _q, td = tr.last_values(B)
        ga, gc, fn = whole.actor.get_grads(), whole.critic.get_grads(), tr.last_feature_norm(B)
        dq_da1 = single.critic.q_gradients_wrt_actions(hb)
        _loss, td1, _q1 = single.critic.check_loss(hb)
        single.actor.train(hb.state_1)
        ga1, fa = single.actor.get_grads(), single.trainer.last_feature_norm(B)["actor"]
        single.critic.train(hb)
        gc1, fc = single.critic.get_grads(), single.trainer.last_feature_norm(B)["critic"]
        conv = sum(int(np.prod(v.shape)) for v in whole.actor.trainable_model_vars() if "/conv" in v.name)
    finally:
        whole.close(); single.close()
    assert np.abs(dq_da).max() > 0 and np.abs(td).max() > 0
    assert dq_da1.tobytes() == dq_da.tobytes() and td1.tobytes() == td.tobytes()
    for name, one in (("actor", fa), ("critic", fc)):
        for k in L.LN_QUANTITIES:
            assert np.abs(fn[name][k]).max() > 0 and one[k].tobytes() == fn[name][k].tobytes(), (name, k, np.abs(one[k] - fn[name][k]).max())
    assert 0 < conv < len(ga) and ga1[conv:].tobytes() == ga[conv:].tobytes() and gc1[conv:].tobytes() == gc[conv:].tobytes()


# ---- 3. identities
def _run(B, nb, calls, how, opt="adam", act="tanh", hidden=(65, 20, 10), **kw):
    """`calls` outer steps of nb minibatches on one memory, device-drawn rows of one seed; how: 'graph' (the eager pass, the capture, the
    replays) or 'dp' (the data-parallel step at world size 1)"""
    lib, check, ptr = _abi()
    specs, P, episodes, _idxs, _batches = L.host_case(SHAPE, B, 1, 4, hidden, act, rows=64)
    hp = L._R().hyper_of("adam", 0.5, 0.25)
    agent = _agent(B, hidden, act, hp, P, episodes, rows=64, opt=opt, sample_seed=5, seed=3, **kw)
    try:
        rows = []
        for _c in range(calls):
            if how == "graph":
                agent.train_step(B, nb)
            elif how == "dp":
                check(lib.cpp_ddpg_dp_train_step(agent.trainer.handle, agent.replay_memory.handle, None, B, nb, 5, 1, 0))
            last = np.empty(B, np.int32)
            check(lib.cpp_replay_last_indexes(agent.replay_memory.handle, B, ptr(last)))
            rows.append(last)
        st = agent.trainer.get_optimiser_state() if opt else {"m": np.zeros(1), "v": np.zeros(1)}
        out = _params(agent) + [st["m"], st["v"]]
        assert all(np.isfinite(x).all() for x in out)
        return out, rows, agent.trainer.last_feature_norm(B)
    finally:
        agent.close()


def test_three_repeated_runs_and_the_data_parallel_step_are_bit_identical():
    """three runs of (eager pass, capture, two replays) give the same bits; so does the data-parallel step at world size 1 (whose norms
    come from the sumsq kernel over the reduced buffer instead of the folded partials: both are float64 sums rounded once to float32)"""
    B, nb = 8, 2
    runs = [_run(B, nb, 4, "graph") for _ in range(3)]
    for other in runs[1:]:
        assert all(np.array_equal(x, y) for x, y in zip(runs[0][0], other[0]))
        assert all(np.array_equal(other[2][n][k], runs[0][2][n][k]) for n in ("actor", "critic") for k in L.LN_QUANTITIES)
    dp = _run(B, nb, 4, "dp")
    assert all(np.array_equal(x, y) for x, y in zip(runs[0][1], dp[1])), "the data-parallel step drew other rows"
    print("  fused against data-parallel, largest |difference| per vector:", ["%.1e" % np.abs(x.astype(np.float64) - y).max() for x, y in zip(runs[0][0], dp[0])])
    assert all(np.array_equal(x, y) for x, y in zip(runs[0][0], dp[0]))


def test_the_literal_loop_is_the_fused_step_bit_for_bit_and_the_single_ops_follow_the_restatement():
    """the reference's loop on device-resident batches (actor.train(batch.state_1); critic.train(batch): ONE cpp_ddpg_train_rows, graph
    replayed) against train_step(B, 1, idxs) on the same rows, to the bit; then the stand-alone ops on host arrays -- each half of the
    pass on its own, the ln launches with one job -- against the float64 restatement's train_actor / train_critic"""
    B, hidden, act = 8, (65, 20, 10), "tanh"
    specs, P, episodes, _idxs, batches = L.host_case(SHAPE, B, 2, 4, hidden, act, rows=64)
    hp = L._R().hyper_of("adam", 0.5, 0.25)
    lit, fused = (_agent(B, hidden, act, hp, P, episodes, rows=64, opt="adam") for _ in range(2))
    try:
        np.random.seed(99)
        for step in range(4):
            batch = lit.replay_memory.batch(B)
            lit.actor.train(batch.state_1)
            lit.critic.train(batch)
            lit.target_actor.update_weights()
            lit.target_critic.update_weights()
            fused.train_step(B, 1, idxs=batch.idxs)
            for a, b in zip(_params(lit), _params(fused)):
                assert np.array_equal(a, b), step
            fl, ff = lit.trainer.last_feature_norm(B), fused.trainer.last_feature_norm(B)
            assert all(np.array_equal(fl[n][k], ff[n][k]) for n in ("actor", "critic") for k in L.LN_QUANTITIES)
        assert lit.trainer.fused_pairs == 4
    finally:
        lit.close(); fused.close()
    import collections
    HostBatch = collections.namedtuple("HostBatch", "state_1 action reward terminal_mask state_2")
    agent = _agent(B, hidden, act, hp, P, None, rows=64, opt="adam")
    try:
        for b in batches:
            hb = HostBatch(*[np.asarray(x) for x in b])
            agent.actor.train(hb.state_1)
            agent.critic.train(hb)
        got = _params(agent)
        loss, td, q = agent.critic.check_loss(HostBatch(*[np.asarray(x) for x in batches[0]]))
    finally:
        agent.close()
    R = L._R()
    name, args = R.OPTIMISERS["adam"]
    ref = L.with_feature_norm(R.DDPGWithOptimiser)(specs[0], specs[1], P[0], P[1], np.float64, hp, name, args)
    ref.set_targets(P[2], P[3])
    for b in batches:
        ref.train_actor(b[0])
        ref.train_critic(b)
    for g, w, p in zip(got[:2], (ref.actor.flat(), ref.critic.flat()), P[:2]):
        assert np.linalg.norm(g - w) <= delta_bound(p, w - p, 5e-5, 2)
    wl, wtd, wq = ref.check_loss(batches[0])      # (no training / inference distinction: the same normalisation)
    assert np.abs(td - wtd).max() < 1e-5 and np.abs(q - wq).max() < 1e-5 and abs(loss - wl) < 1e-5 * max(1.0, wl)


def test_targets_at_rate_one_equal_the_trained_networks_gamma_and_beta_included():
    """the target update is fma(-rate, t - s, t) per element (csrc/common.h, soft_update_value; base_network.py:31): at rate 1 that is s
    bit for bit wherever t - s is exact in float32 -- Sterbenz: t / 2 <= s <= 2 t, which is where a run's targets live -- and s up to one
    rounding elsewhere (an element near zero whose target sits a perturbation away).  Held, over the whole buffers with gamma and beta:
    every element is that formula's bits, and the trained network's own bits wherever the difference is exact"""
    B, hidden = 8, (65, 20, 10)
    specs, P, episodes, idxs, _b = L.host_case(SHAPE, B, 2, 4, hidden, "tanh", rows=64)
    agent = _agent(B, hidden, "tanh", O.Hyper(1e-2, 5e-2, 0.9, 0.5, 1.0), P, episodes, rows=64)
    try:
        agent.train_step(B, 2, idxs=idxs)
        a, c, ta, tc = _params(agent)
        fwd = agent.actor.forward(np.asarray(episodes[0][0])[None])
        tfwd = agent.target_actor.forward(np.asarray(episodes[0][0])[None])
    finally:
        agent.close()
    for name, src, tgt, old, spec in (("actor", a, ta, P[2], specs[0]), ("critic", c, tc, P[3], specs[1])):
        d = old - src                                           # float32: one rounding
        assert np.array_equal(tgt, (old.astype(np.float64) - d.astype(np.float64)).astype(np.float32)), name
        exact = d.astype(np.float64) == old.astype(np.float64) - src.astype(np.float64)
        k = spec.num_plain()
        print("  %s: t - s exact in %d of %d elements (gamma / beta: %d of %d)" % (name, exact.sum(), exact.size, exact[k:].sum(), exact.size - k))
        assert np.array_equal(tgt[exact], src[exact]) and exact.mean() > 0.9 and exact[k:].mean() > 0.9
        assert np.abs(tgt - src).max() <= 2.0 ** -23 * np.abs(old).max()
        assert np.abs(src[k:] - P[0 if name == "actor" else 1][k:]).max() > 0
    assert np.abs(fwd - tfwd).max() < 1e-5
    ref = L.LnNet(specs[0], a, np.float64)      # (the inference path normalises as the train ops do)
    assert np.abs(fwd - ref.forward(np.asarray(episodes[0][0])[None])["out"]).max() < 1e-5


# ---- 3b. the collectives over the longer buffers: real RCCL calls on a communicator of one rank, and the replica broadcast
@pytest.mark.parametrize("mode", ["gradient-allreduce", "overlap", "periodic-3"])
def test_the_rccl_collectives_cover_gamma_and_beta(mode):
    """tests/test_gpu_distributed.py's form on normalised networks under Adam: the all-reduce of the whole gradient buffer, the
    overlapped all-reduce of the fully connected tails (which end in gamma and beta) and the parameter / slot averaging of the periodic
    mode walk the fused step's minibatches to its parameters and slots, gamma and beta having moved"""
    from cartpoleplusplus_amd import ddpg_cartpole as D
    from cartpoleplusplus_amd.distributed import Communicator, NativeLearner
    B, hidden = 8, (65, 20, 10)
    specs, P, episodes, _i, _b = L.host_case(SHAPE, B, 1, 4, hidden, "tanh", rows=64)
    hp = L._R().hyper_of("adam", 0.5, 0.25)
    res = []
    for which in ("fused", "dp"):
        agent = _agent(B, hidden, "tanh", hp, P, episodes, rows=64, opt="adam", sample_seed=5)
        try:
            if which == "fused":
                for _ in range(4):
                    agent.train_step(B, 3)
            else:
                comm = Communicator.single(agent.trainer.ctx)
                learner = NativeLearner(agent, B, int(D.opts.sample_seed), comm, sync_every=3 if mode == "periodic-3" else 1, overlap=mode == "overlap")
                for _ in range(4):
                    learner.train_step(3)
                learner.close()
            agent.actor.ctx.sync()
            st = agent.trainer.get_optimiser_state()
            res.append(_params(agent) + [st["m"], st["v"]])
        finally:
            agent.close()
    for x, y in zip(res[0], res[1]):
        assert np.abs(x - y).max() < 1e-6, float(np.abs(x - y).max())
    for i, k in ((0, specs[0].num_plain()), (1, specs[1].num_plain()), (2, specs[0].num_plain()), (3, specs[1].num_plain())):
        assert np.abs(res[1][i][k:] - P[i][k:]).min() > 0


def test_the_replica_broadcast_carries_gamma_beta_and_their_slots():
    """distributed.sync_replicas_from_rank0 between two agents of one process, torch.distributed stood in for by an object that hands
    rank 0's payload to rank 1: parameters, targets and slots arrive bit for bit over the longer buffers"""
    from cartpoleplusplus_amd.distributed import sync_replicas_from_rank0
    B, hidden = 8, (65, 20, 10)
    specs, P, episodes, idxs, _b = L.host_case(SHAPE, B, 2, 4, hidden, "tanh", rows=64)
    hp = L._R().hyper_of("adam", 0.5, 0.25)

    class Wire(object):
        box = None

        def __init__(self, rank):
            self.rank = rank

        def get_rank(self):
            return self.rank

        def get_backend(self):
            return "gloo"

        def broadcast_object_list(self, payload, src=0, **_kw):
            if self.rank == src:
                Wire.box = payload[0]
            else:
                payload[0] = Wire.box
    zero = _agent(B, hidden, "tanh", hp, P, episodes, rows=64, opt="adam")
    try:
        zero.train_step(B, 2, idxs=idxs)
        one = _agent(B, hidden, "tanh", hp, None, None, rows=64, opt="adam", seed=7)
        try:
            assert not np.array_equal(one.actor.get_params(), zero.actor.get_params())
            sync_replicas_from_rank0(zero, Wire(0))
            sync_replicas_from_rank0(one, Wire(1))
            s0, s1 = zero.trainer.get_optimiser_state(), one.trainer.get_optimiser_state()
            for x, y in zip(_params(zero) + [s0["m"], s0["v"], s0["step"]], _params(one) + [s1["m"], s1["v"], s1["step"]]):
                assert np.array_equal(x, y)
            k = specs[0].num_plain()
            assert np.abs(s1["m"][k:len(P[0])]).min() > 0 and np.abs(one.actor.get_params()[k:] - P[0][k:]).min() > 0
        finally:
            one.close()
    finally:
        zero.close()


# ---- 4. compositions that take the GEMM levels, and the replay features: they run, stay finite, replay to the same bits as a second run,
# ---- move gamma and beta, and (soft actor-critic) copy them into the target actor
VARIANTS = {"twin-q": (dict(twin_q=True), "heads"),
            "distributional": (dict(distributional_critic=True, num_atoms=11, v_min=-2.0, v_max=12.0), "gemm"),
            "quantile": (dict(quantile_critic=True, num_quantiles=7), "gemm"),
            "sac": (dict(soft_actor_critic=True), "gemm"),
            "per-nstep-u8-shift": (dict(prioritized_replay=True, n_step=3, replay_store="u8"), "heads")}


@pytest.mark.parametrize("name", list(VARIANTS))
def test_the_other_learners_compose(name):
    kw, route = VARIANTS[name]
    B, nb = 8, 2
    runs = []
    for _k in range(2):
        lib, check, ptr = _abi()
        _specs, _P, episodes, _i, _b = L.host_case(SHAPE, B, 1, 4, (65, 20, 10), "tanh", rows=64)
        if name == "per-nstep-u8-shift":
            episodes = [(np.rint(np.asarray(f, np.float32) * 255).astype(np.uint8), [(a, r, np.rint(np.asarray(s2, np.float32) * 255).astype(np.uint8)) for a, r, s2 in seq])
                        for f, seq in episodes]
        agent = _agent(B, (65, 20, 10), "tanh", L._R().hyper_of("adam", 0.5, 0.25), None, episodes, rows=64, opt="adam", sample_seed=5, seed=3, **kw)
        try:
            if name == "per-nstep-u8-shift":
                agent.replay_memory.enable_random_shift(2, seed=9)
            start = _params(agent)
            census = _profiled_calls(agent.actor.ctx, lambda: agent.train_step(B, 1))
            assert census.get("heads", 0) == (1 if route == "heads" else 0), census
            assert (census.get("ln_fwd", 0), census.get("ln_bwd", 0)) == (1, 2), census
            for _c in range(3):
                agent.train_step(B, nb)
            end = _params(agent)
            runs.append(end)
            ka, kc = start[0].size - 2 * 65, start[1].size - 2 * 200
            assert all(np.isfinite(x).all() for x in end)
            for i, k in ((0, ka), (1, kc), (2, ka), (3, kc)):
                assert np.abs(end[i][k:] - start[i][k:]).min() > 0, (name, i)      # every gamma and every beta moved
            if name == "sac":
                assert np.array_equal(end[0], end[2])      # the target actor is the actor, gamma / beta included
            names = [v.name for v in agent.critic.trainable_model_vars()]
            assert names[-2:] == ["critic/hidden1/LayerNorm/gamma:0", "critic/hidden1/LayerNorm/beta:0"]
        finally:
            agent.close()
    assert all(np.array_equal(x, y) for x, y in zip(runs[0], runs[1]))


# ---- 5. the launch census, and off means off
def _census(norm, nb=3):
    specs, P, episodes, _idxs, _b = L.host_case(SHAPE, 8, 1, 4, (65, 20, 10), "tanh", rows=64)
    if not norm:
        P = [p[:s.num_plain()] for p, s in zip(P, (specs[0], specs[1], specs[0], specs[1]))]
    agent = _agent(8, (65, 20, 10), "tanh", O.DEFAULT_HYPER, P, episodes, rows=64, norm=norm, sample_seed=5)
    try:
        agent.train_step(8, nb)
        return _profiled_calls(agent.actor.ctx, lambda: agent.train_step(8, nb))
    finally:
        agent.close()


def test_the_launch_census_is_the_plain_steps_plus_the_ln_launches():
    nb = 3
    plain, norm = _census(False, nb), _census(True, nb)
    print("launches per outer step:", norm)
    assert plain.get("ln_fwd", 0) == 0 and plain.get("ln_bwd", 0) == 0
    assert norm.pop("ln_fwd") == nb and norm.pop("ln_bwd") == 2 * nb      # one forward, two backward launches per minibatch
    assert norm == plain, (norm, plain)
    assert norm["heads"] == nb and norm.get("sumsq", 0) == 0      # the heads launch stays; the norms stay folded


_PLAIN_SNIPPET = r"""
import json, sys
sys.path.insert(0, %(root)r)
from tests import test_gpu_layer_norm as G
print("RESULT " + json.dumps(G._plain_run(%(norm_first)r)))
"""


def _plain_run(norm_first):
    specs, P, episodes, _idxs, _b = L.host_case(SHAPE, 8, 1, 4, (65, 20, 10), "tanh", rows=64)
    if norm_first:
        agent = _agent(8, (65, 20, 10), "tanh", O.DEFAULT_HYPER, P, episodes, rows=64, sample_seed=5)
        try:
            agent.train_step(8, 2)
            agent.train_step(8, 2)
        finally:
            agent.close()
    plainP = [p[:s.num_plain()] for p, s in zip(P, (specs[0], specs[1], specs[0], specs[1]))]
    agent = _agent(8, (65, 20, 10), "tanh", O.DEFAULT_HYPER, plainP, episodes, rows=64, norm=False, sample_seed=5)
    try:
        lib, _check, _ptr = _abi()
        on = ctypes.c_int(7)
        assert lib.cpp_net_feature_norm_info(agent.actor.handle, ctypes.byref(on), None, None) == 0 and on.value == 0
        for _s in range(3):
            agent.train_step(8, 2)
        h = hashlib.sha256()
        for x in _params(agent):
            h.update(np.ascontiguousarray(x).tobytes())
        census = _profiled_calls(agent.actor.ctx, lambda: agent.train_step(8, 2))
    finally:
        agent.close()
    return {"digest": h.hexdigest(), "census": census}


def test_off_means_off():
    """a plain trainer created after a normalised one in the same process ends with the bits, and launches the kernels, of one in a
    process that never made one"""
    out = subprocess.run([sys.executable, "-c", _PLAIN_SNIPPET % dict(root=ROOT, norm_first=False)], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    fresh = json.loads([l for l in out.stdout.splitlines() if l.startswith("RESULT ")][0][len("RESULT "):])
    here = _plain_run(True)
    assert here["census"] == fresh["census"], (here["census"], fresh["census"])
    assert here["digest"] == fresh["digest"] and "ln_fwd" not in here["census"] and "ln_bwd" not in here["census"]


# ---- 6. the layout, checkpoints, refusals
def test_the_layout_a_checkpoint_round_trip_and_both_layout_refusals(tmp_path):
    from cartpoleplusplus_amd import util
    specs, P, episodes, idxs, _b = L.host_case(SHAPE, 8, 2, 4, (65, 20, 10), "tanh", rows=64)
    hp = L._R().hyper_of("adam", 0.5, 0.25)
    layouts = {}
    for norm in (False, True):
        agent = _agent(8, (65, 20, 10), "tanh", hp, None, None, rows=64, norm=norm, opt="adam", twin_q=True)
        try:
            layouts[norm] = [[(v.name.split("/", 1)[1], tuple(v.shape), int(v.offset)) for v in net.trainable_model_vars()] for net in agent.networks()]
            if norm:      # gamma = 1, beta = 0 as created
                for net, width in zip(agent.networks(), (65, 200, 65, 200)):
                    tail = net.get_params()[-2 * width:]
                    assert np.array_equal(tail[:width], np.ones(width, np.float32)) and not tail[width:].any()
        finally:
            agent.close()
    for plain, norm, layer0, width in zip(layouts[False], layouts[True], ("h0", "hidden1", "h0", "hidden1"), (65, 200, 65, 200)):
        assert norm[:len(plain)] == plain      # the plain prefix -- twin variables included -- keeps names, shapes and offsets
        end = plain[-1][2] + int(np.prod(plain[-1][1]))
        assert norm[len(plain):] == [(layer0 + "/LayerNorm/gamma:0", (width,), end), (layer0 + "/LayerNorm/beta:0", (width,), end + width)]
    agent = _agent(8, (65, 20, 10), "tanh", hp, P, episodes, rows=64, opt="adam")
    try:
        agent.train_step(8, 2, idxs=idxs)
        util.SaverUtil(agent, str(tmp_path / "norm"), 3600).force_save()
        st = agent.trainer.get_optimiser_state()
        want = _params(agent) + [st["m"], st["v"]]
    finally:
        agent.close()
    agent = _agent(8, (65, 20, 10), "tanh", hp, None, None, rows=64, opt="adam", seed=7)
    try:
        assert not np.array_equal(agent.actor.get_params(), want[0])
        util.SaverUtil(agent, str(tmp_path / "norm"), 3600)
        st = agent.trainer.get_optimiser_state()
        assert all(np.array_equal(x, y) for x, y in zip(_params(agent) + [st["m"], st["v"]], want))
    finally:
        agent.close()
    plain = _agent(8, (65, 20, 10), "tanh", hp, None, None, rows=64, norm=False, opt="adam")
    try:
        util.SaverUtil(plain, str(tmp_path / "plain"), 3600).force_save()
        with pytest.raises(AssertionError, match="checkpoint does not match"):
            util.SaverUtil(plain, str(tmp_path / "norm"), 3600)
    finally:
        plain.close()
    agent = _agent(8, (65, 20, 10), "tanh", hp, None, None, rows=64, opt="adam")
    try:
        with pytest.raises(AssertionError, match="checkpoint does not match"):
            util.SaverUtil(agent, str(tmp_path / "plain"), 3600)
    finally:
        agent.close()


def test_the_refusals():
    from cartpoleplusplus_amd import _lib
    lib, check, ptr = _abi()
    hp = O.DEFAULT_HYPER
    norm = _agent(8, (65, 20, 10), "tanh", hp, None, None)
    try:
        relu = _agent(8, (65, 20, 10), "relu", hp, None, None)
        plain = _agent(8, (65, 20, 10), "tanh", hp, None, None, norm=False)
        try:
            ctx = norm.actor.ctx.handle
            h = ctypes.c_void_p()
            hy = _lib.DdpgHyper(1e-3, 1e-2, 0.9, 5.0, 0.1)

            def create(a, c, ta, tc):
                return lib.cpp_ddpg_create(ctx, a.handle, c.handle, ta.handle, tc.handle, ctypes.byref(hy), ctypes.byref(h))
            # some but not all four networks normalised
            for nets in ((norm.actor, plain.critic, norm.target_actor, plain.target_critic), (plain.actor, plain.critic, plain.target_actor, norm.target_critic)):
                assert create(*nets) == CPP_ERR_ARG and b"some of the four" in lib.cpp_last_error(), lib.cpp_last_error()
            # differing activations
            assert create(norm.actor, norm.critic, relu.target_actor, norm.target_critic) == CPP_ERR_ARG and b"differ in activation" in lib.cpp_last_error()

            def spec_of(net, **kw):
                s = _lib.NetSpec()
                ctypes.memmove(ctypes.byref(s), ctypes.byref(net.spec), ctypes.sizeof(s))
                for k, v in kw.items():
                    setattr(s, k, v)
                return s

            def make(spec, act=_lib.CPP_NORM_TANH, eps=1e-5, variant=None):
                rc = lib.cpp_net_create_feature_norm(ctx, ctypes.byref(spec), 8, ctypes.byref(variant) if variant is not None else None, act, eps, ctypes.byref(h))
                return rc, lib.cpp_last_error()
            low = spec_of(norm.actor, pixel=0, state_elems=14)
            for spec, word in ((low, b"low-dimensional"), (spec_of(norm.actor, use_batch_norm=1), b"use_batch_norm"), (spec_of(norm.actor, use_dropout=1), b"use_dropout"),
                               (spec_of(norm.actor, kind=_lib.CPP_HEAD, head_out=1), b"kind 2")):
                rc, msg = make(spec)
                assert rc == CPP_ERR_ARG and word in msg, (word, msg)
            rc, msg = make(spec_of(norm.actor), act=2)
            assert rc == CPP_ERR_ARG and b"activation 2" in msg
            rc, msg = make(spec_of(norm.actor), eps=0.0)
            assert rc == CPP_ERR_ARG and b"epsilon" in msg
            v = _lib.NetVariant()
            v.twin_q, v.n_quantiles = 1, 5
            rc, msg = make(spec_of(norm.critic), variant=v)
            assert rc == CPP_ERR_ARG and b"at most one" in msg
            v = _lib.NetVariant()
            v.twin_q = 1
            rc, msg = make(spec_of(norm.actor), variant=v)
            assert rc == CPP_ERR_ARG and b"belong to a critic" in msg
            # differing epsilon: a second target critic with another one
            rc, msg = make(spec_of(norm.critic), eps=1e-3)
            assert rc == 0
            other = ctypes.c_void_p(h.value)
            try:
                rc = lib.cpp_ddpg_create(ctx, norm.actor.handle, norm.critic.handle, norm.target_actor.handle, other, ctypes.byref(hy), ctypes.byref(h))
                assert rc == CPP_ERR_ARG and b"differ in activation or epsilon" in lib.cpp_last_error()
                on, act, eps = ctypes.c_int(), ctypes.c_int(), ctypes.c_float()
                check(lib.cpp_net_feature_norm_info(other, ctypes.byref(on), ctypes.byref(act), ctypes.byref(eps)))
                assert (on.value, act.value) == (1, _lib.CPP_NORM_TANH) and eps.value == np.float32(1e-3)
            finally:
                lib.cpp_net_destroy(other)
            # NAF refuses normalised networks
            nh = _lib.NafHyper(0.9, 5.0, 0.1, 0, 1e-3, 0.0, 0.9, 0.999, 1e-8)
            rc = lib.cpp_naf_create(ctx, norm.critic.handle, norm.target_critic.handle, norm.critic.handle, norm.critic.handle, 0, ctypes.byref(nh), ctypes.byref(h))
            assert rc == CPP_ERR_ARG and b"feature layer norm" in lib.cpp_last_error()
            # the read-back on a plain trainer, and its argument checks
            assert lib.cpp_ddpg_last_feature_norm(plain.trainer.handle, 8, 0, None, None, None, None, None, None) == CPP_ERR_STATE
            assert b"cpp_ddpg_last_feature_norm" in lib.cpp_last_error()
            assert lib.cpp_ddpg_last_feature_norm(None, 8, 0, None, None, None, None, None, None) == CPP_ERR_ARG
            assert lib.cpp_ddpg_last_feature_norm(norm.trainer.handle, 9, 0, None, None, None, None, None, None) == CPP_ERR_ARG
            assert lib.cpp_ddpg_last_feature_norm(norm.trainer.handle, 8, 2, None, None, None, None, None, None) == CPP_ERR_ARG
        finally:
            relu.close(); plain.close()
    finally:
        norm.close()
