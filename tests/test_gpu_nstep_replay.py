"""n-step returns in the device gather (csrc/gather_body.h nstep_walk; semantics in include/cartpolepp_abi.h) against the row-by-row
restatement tests/nstep_np.py: the gathered reward, mask, state_2 pixels and slots bit for bit (caller rows and Philox draws, f16 and
8-bit stores, a memory filled by add_episode that has wrapped), the literal loop's host columns against the device's, n = 1 set
explicitly against a memory that never set it, one fused minibatch at n = 3 against the unmodified float64 oracles fed the n-step
columns (DDPG cfg3, the low-dimensional agent, NAF cfg4, prioritized + n-step), the literal loop against the fused step, a captured
step graph that follows n, the data-parallel step at world size 1, and the discount refusals."""
import ctypes

import numpy as np
import pytest

from oracle import ddpg_np as O
from oracle import naf_np as N
from tests import nstep_np as NS
from tests import per_np as P
from tests.helpers import (assert_flat_close, device_pool_codes, device_relu_active, make_pair, pool_flips_are_near_ties,
                           relu_flips_are_at_the_boundary)
from tests.test_gpu_naf_prioritized_replay import CatSpec, last_rows, make_naf, MOMENTUM

pytestmark = pytest.mark.gpu

LOWDIM = (2, 2, 7)
PIX = (32, 32, 3, 2, 3)
SMALL = (16, 16, 3, 1, 2)
CODES = (np.arange(256) / 255.0).astype(np.float16)


def _lib():
    from cartpoleplusplus_amd._lib import lib, check, ptr
    return lib, check, ptr


def _bits(x):
    x = np.ascontiguousarray(x)
    return x.view(np.uint32) if x.dtype == np.float32 else x.view(np.uint16) if x.dtype == np.float16 else x


def _same(a, b, what=""):
    a, b = np.asarray(a), np.asarray(b)
    assert a.shape == b.shape, (what, a.shape, b.shape)
    assert np.array_equal(_bits(a), _bits(b)), what


def _want(rm, idxs):
    return NS.columns(idxs, rm.state_1_idx, rm.state_2_idx, rm.reward, rm.terminal_mask, rm.size(), rm.buffer_size, rm.n_step,
                      rm.n_step_discount)


def _download(rm, B):
    lib, check, ptr = _lib()
    dev = rm._batches[B]
    s1, s2 = np.empty((B,) + rm.state_shape, np.float16), np.empty((B,) + rm.state_shape, np.float16)
    a, r, m = np.empty((B, rm.action_dim), np.float32), np.empty((B, 1), np.float32), np.empty((B, 1), np.float32)
    check(lib.cpp_batch_download(dev.handle, ptr(s1), ptr(s2), ptr(a), ptr(r), ptr(m)))
    return s1, s2, a, r, m


def _episode_memory(store, R=120, seed=0):
    """a memory filled by add_episode with episode lengths 1..12 until it has wrapped at least twice; random rewards, 8-bit codes"""
    from cartpoleplusplus_amd.replay_memory import ReplayMemory
    rng = np.random.default_rng(seed)
    rm = ReplayMemory(R, SMALL, 2, store_dtype=store)
    written = 0
    while written < 2 * R + 17:
        L = int(rng.integers(1, 13))
        frames = [CODES[rng.integers(0, 256, SMALL)] for _ in range(L + 1)]
        seq = [(rng.uniform(-1, 1, 2).astype(np.float32), float(np.float32(rng.normal())), frames[k + 1]) for k in range(L)]
        rm.add_episode(frames[0], seq)
        written += L
    assert rm.full
    return rm


@pytest.mark.parametrize("store", ["f16", "u8"])
def test_gather_matches_numpy_bit_for_bit(store):
    rm = _episode_memory(store, seed=1 if store == "u8" else 0)
    try:
        rng = np.random.default_rng(2)
        B = 64
        for n in (1, 2, 3, 5, 64):
            rm.enable_n_step(n, 0.97)
            for draw in ("rows", "philox"):
                if draw == "rows":
                    idxs = rng.integers(0, rm.size(), B)
                    b = rm.batch(idxs=idxs)
                    b.device                                     # cpp_replay_sample on the caller's rows
                else:
                    b = rm.sample_on_device(B, seed=5, counter=n)
                idxs = b.idxs
                r, m, s2_idx = _want(rm, idxs)
                s1g, s2g, ag, rg, mg = _download(rm, B)
                _same(rg, r, "reward n=%d %s" % (n, draw))
                _same(mg, m, "mask n=%d %s" % (n, draw))
                _same(s2g, rm.state[s2_idx], "state_2 n=%d %s" % (n, draw))
                _same(s1g, rm.state[rm.state_1_idx[idxs]], "state_1")
                _same(ag, rm.action[idxs], "action")
                # the literal loop's Batch: its host columns are the device's, bit for bit
                _same(b.reward, rg, "host reward")
                _same(b.terminal_mask, mg, "host mask")
                _same(b.state_2_idx, s2_idx, "host state_2 slots")
                if n > 1:
                    assert (s2_idx != rm.state_2_idx[idxs]).any()          # (the walk went somewhere)
    finally:
        rm.close()


def test_explicit_n1_is_the_one_step_memory():
    B = 32
    a, _r, _ = make_pair(PIX, B, True, seed=3, replay_size=240)
    b, _r, _ = make_pair(PIX, B, True, seed=3, replay_size=240)
    try:
        for x in (a, b):
            x.replay_memory.fill_synthetic(200, seed=21)
        b.replay_memory.enable_n_step(1, 0.5)                 # (n = 1: the discount plays no part)
        for _ in range(3):
            a.train_step(B, 3)
            b.train_step(B, 3)
        for x, y in zip(a.networks(), b.networks()):
            assert np.array_equal(x.get_params(), y.get_params()), x.namespace
    finally:
        a.close()
        b.close()


def _ddpg_nstep_against_f64_oracle(shape, B, rows, pixel=True, seed=0, per=False, atol=1e-5, grad_rel=2e-5, flip_tol=1e-5, hyper=None,
                                   capacity=None, **pair_kw):
    """ONE graph-replayed minibatch of the fused DDPG step on an n = 3 memory against oracle.DDPG(float64), unmodified, on the n-step
    columns (reward, terminal_mask, state_2 of the last row walked): actions / Q / TD at `atol`, the pre-clip gradients at `grad_rel`.
    per: a prioritized memory as well -- the critic's gradient against the oracle's backward pass of w * td_dev, and the priorities
    written from the n-step TD.  hyper: an O.Hyper for the agent and the oracle (None: the defaults).  pair_kw: make_pair's options
    (use_batch_norm).  capacity=C > B: the agent is built for C rows; a C-row step and its replay run first, and behind the checked
    B-row replay one more C-row step is held to the same bars."""
    kw = dict(prioritized_replay=True, priority_alpha=0.6, priority_beta=0.4, priority_eps=1e-6) if per else {}
    if hyper is not None:
        from tests.helpers import hyper_options
        kw.update(hyper_options(hyper))
    kw.update(pair_kw)
    agent, _ref, (aspec, cspec) = make_pair(shape, B, pixel, seed=seed, replay_size=rows + 50, capacity=capacity, **kw)
    from cartpoleplusplus_amd import ddpg_cartpole as D
    try:
        rm = agent.replay_memory
        rm.fill_synthetic(rows, seed=21 + seed)
        rm.enable_n_step(3, D.opts.discount)
        C = B if capacity is None else int(capacity)
        for _ in range(2 if C > B else 0):
            agent.train_step(C, 1)                            # eager pass + capture, its replay
        agent.train_step(B, 1)                                # eager pass + capture
        if per:
            rm.update_priorities(np.arange(rows), np.random.default_rng(seed + 9).lognormal(0.0, 2.0, rows).astype(np.float32))
        nets = (agent.actor, agent.critic, agent.target_actor, agent.target_critic)
        lib, check, ptr = _lib()

        def step_and_read(Bx):
            d = {"Pm": [n.get_params() for n in nets]}
            agent.train_step(Bx, 1)                           # hipGraph replay where this key's graph is held
            idxs = np.empty(Bx, np.int32)
            check(lib.cpp_replay_last_indexes(rm.handle, Bx, ptr(idxs)))
            d["w"] = rm.last_weights(Bx) if per else None
            d["values"] = agent.trainer.last_values(Bx)
            d["grads"] = (agent.actor.get_grads(), agent.critic.get_grads())
            if per:
                last = {int(r): i for i, r in enumerate(idxs)}
                keys = np.array(sorted(last), np.int32)
                d["last"], d["keys"], d["written"] = last, keys, rm.priorities(keys)
            if pixel:
                d["codes"] = (device_pool_codes(agent.actor, Bx), device_pool_codes(agent.critic, Bx))
                d["relu"] = (device_relu_active(agent.actor, Bx), device_relu_active(agent.critic, Bx))
            hb = rm.batch(idxs=idxs)
            s1, s2 = rm.state[hb.state_1_idx], rm.state[hb.state_2_idx]
            a, r, m = hb.action, hb.reward, hb.terminal_mask
            assert (hb.state_2_idx != rm.state_2_idx[idxs]).any() and (m != rm.terminal_mask[idxs]).any()
            d["batch"] = (s1, a, r, m, s2)
            return d
        checked = step_and_read(B)
        back = step_and_read(C) if C > B else None
    finally:
        agent.close()
    for d in (checked, back):
        if d is not None:
            _check_nstep(d, aspec, cspec, pixel, per, atol, grad_rel, flip_tol, hyper)


def _check_nstep(d, aspec, cspec, pixel, per, atol, grad_rel, flip_tol, hyper):
    """what _ddpg_nstep_against_f64_oracle's step_and_read() brought back from one minibatch"""
    Pm, w = d["Pm"], d["w"]
    actions, _dq, q, td = d["values"]
    g_a, g_c = d["grads"]
    s1, a, r, m, s2 = d["batch"]
    ref = O.DDPG(aspec, cspec, Pm[0], Pm[1], np.float64, **({} if hyper is None else {"hyper": hyper}))
    ref.set_targets(Pm[2], Pm[3])
    if pixel:
        (codes_a, codes_c), (relu_a, relu_c) = d["codes"], d["relu"]
        ref.actor.amax_override, ref.critic.amax_override = codes_a, codes_c
        ref.actor.relu_override, ref.critic.relu_override = relu_a, relu_c
    t = (s1, a, r, m, s2)
    ag = ref.actor_gradients(s1)
    cg = ref.critic_gradients(t)
    if pixel:
        pool_flips_are_near_ties(ag["cache_actor"], codes_a, flip_tol, what="actor")
        pool_flips_are_near_ties(cg["cache_critic"], codes_c, flip_tol, what="critic")
        relu_flips_are_at_the_boundary(ag["cache_actor"], relu_a, flip_tol, what="actor")
        relu_flips_are_at_the_boundary(cg["cache_critic"], relu_c, flip_tol, what="critic")
    assert np.abs(actions - ag["actions"]).max() < atol
    assert np.abs(q - cg["q"]).max() < atol and np.abs(td - cg["td"]).max() < atol
    assert_flat_close(aspec, g_a, ag["grads"], rel=grad_rel, what="actor pre-clip grads vs f64 oracle")
    if per:
        last, keys, written = d["last"], d["keys"], d["written"]
        w64 = w.astype(np.float64).reshape(-1, 1)
        cw = ref.critic_gradients(t, td_override=w64 * td.astype(np.float64))
        assert_flat_close(cspec, g_c, cw["grads"], rel=grad_rel, what="weighted critic pre-clip grads vs f64 oracle (n-step)")
        want = P.priority(td.reshape(-1)[[last[k] for k in keys]], 0.6, 1e-6)
        assert np.abs(written / want - 1).max() < 2e-6
    else:
        assert_flat_close(cspec, g_c, cg["grads"], rel=grad_rel, what="critic pre-clip grads vs f64 oracle (n-step)")


def test_nstep_step_below_the_capacity_against_f64_oracle():
    """(C, B) = (8, 5), n = 3: the gather's n-step walk for B rows behind C-row steps, and back"""
    _ddpg_nstep_against_f64_oracle((16, 16, 3, 1, 2), 5, 300, capacity=8)


def test_nstep_fused_step_against_f64_oracle_cfg3():
    _ddpg_nstep_against_f64_oracle((64, 64, 3, 2, 3), 256, 2500)


def test_nstep_lowdim_step_against_f64_oracle():
    _ddpg_nstep_against_f64_oracle(LOWDIM, 64, 2000, pixel=False, seed=4)


def test_prioritized_nstep_step_against_f64_oracle():
    _ddpg_nstep_against_f64_oracle((64, 64, 3, 2, 3), 256, 2500, seed=2, per=True)


def test_nstep_naf_step_against_f64_oracle_cfg4():
    """one graph-replayed minibatch of the fused NAF step (cfg4: shared trunk, Momentum) on an n = 3 memory against oracle.naf_np.NAF
    (float64, unmodified) fed the n-step columns: the loss at 1e-5, the pre-clip gradients at 2e-5"""
    from cartpoleplusplus_amd import naf_cartpole as F
    shape, B, share, rows = (64, 64, 3, 2, 3), 256, True, 2500
    agent, specs = make_naf(shape, B, share, seed=0, replay_size=rows + 50)
    try:
        rm = agent.replay_memory
        rm.fill_synthetic(rows, seed=33)
        rm.enable_n_step(3, F.opts.discount)
        agent.train_step(B, 1)                                # eager pass + capture
        nets = (agent.value_net, agent.naf.mu_net, agent.naf.l_net, agent.target_value_net)
        Pm = [n.get_params() for n in nets]
        opt = agent.naf.get_optimiser_state()
        agent.train_step(B, 1)                                # hipGraph replay
        idxs = last_rows(agent, B)
        grads, stats = agent.naf.get_grads(), agent.naf.last_stats()
        codes, relu = [device_pool_codes(agent.value_net, B)], [device_relu_active(agent.value_net, B)]
        hb = rm.batch(idxs=idxs)
        s1, s2 = rm.state[hb.state_1_idx], rm.state[hb.state_2_idx]
        batch = (s1, hb.action, hb.reward, hb.terminal_mask, s2)
        assert (hb.state_2_idx != rm.state_2_idx[idxs]).any()
    finally:
        agent.close()
    vspec, mspec, lspec = specs
    ref = N.NAF(vspec, mspec, lspec, Pm[0], Pm[1], Pm[2], share, 2, np.float64, discount=F.opts.discount, gradient_clip=5.0,
                optimiser=N.make_optimiser(*MOMENTUM))
    ref.target_value = O.Net(vspec, Pm[3], np.float64)
    ref.m = opt["m"].astype(np.float64)
    ref.value.amax_override, ref.value.relu_override = codes[0], relu[0]
    out = ref.forward_backward(batch)
    cache = ref.value.forward(s1, white=ref._white(ref.value, s1), training=True)
    pool_flips_are_near_ties(cache, codes[0], what="value trunk")
    relu_flips_are_at_the_boundary(cache, relu[0], what="value trunk")
    assert stats[2] == 0
    assert abs(stats[0] - out["loss"]) < 1e-5 * max(1.0, abs(out["loss"])), (stats[0], out["loss"])
    assert_flat_close(CatSpec(specs), grads, out["grads"], rel=2e-5, what="NAF pre-clip grads vs f64 oracle (n-step)")


@pytest.mark.parametrize("shape,pixel", [(PIX, True), (LOWDIM, False)], ids=["32x32x18", "lowdim"])
def test_reference_loop_is_the_fused_step(shape, pixel):
    """ddpg_cartpole.py:331-337 verbatim on an n = 3 memory (batch() draws with numpy's RNG; the device trains on the draw's rows,
    whose n-step columns the Batch also carries) against agent.train_step on the same rows: bit for bit, one minibatch per step"""
    from cartpoleplusplus_amd import ddpg_cartpole as D
    B = 32

    def agent():
        a, _ref, _ = make_pair(shape, B, pixel, seed=3, replay_size=240)
        a.replay_memory.fill_synthetic(200, seed=21)
        a.replay_memory.enable_n_step(3, D.opts.discount)
        return a
    lit, fused = agent(), agent()
    try:
        np.random.seed(11)
        for step in range(6):
            batch = lit.replay_memory.batch(B)
            lit.actor.train(batch.state_1)
            lit.critic.train(batch)
            lit.target_actor.update_weights()
            lit.target_critic.update_weights()
            fused.train_step(B, 1, idxs=batch.idxs)
            for a, b in zip(lit.networks(), fused.networks()):
                assert np.array_equal(a.get_params(), b.get_params()), (step, a.namespace)
        assert lit.trainer.fused_pairs == 6
    finally:
        lit.close()
        fused.close()


def test_captured_graph_follows_n():
    """a captured step graph on a memory switched 3 -> 1 -> 3 (device words, no capture again) against an agent that trains on the
    same rows through the eager path at each setting: the same parameters at every step"""
    from cartpoleplusplus_amd import ddpg_cartpole as D
    B = 32
    lib, check, ptr = _lib()

    def agent():
        a, _ref, _ = make_pair(PIX, B, True, seed=5, replay_size=240)
        a.replay_memory.fill_synthetic(200, seed=23)
        return a
    g, e = agent(), agent()
    try:
        for n in (3, 3, 1, 1, 3, 3):
            for x in (g, e):
                x.replay_memory.enable_n_step(n, D.opts.discount)
            g.train_step(B, 1)                                   # (captured at the first step, replayed after)
            rows = np.empty(B, np.int32)
            check(lib.cpp_replay_last_indexes(g.replay_memory.handle, B, ptr(rows)))
            e.train_step(B, 1, idxs=rows)                        # (eager: a stream of launches, no graph)
            for a, b in zip(g.networks(), e.networks()):
                assert np.array_equal(a.get_params(), b.get_params()), (n, a.namespace)
    finally:
        g.close()
        e.close()


def test_data_parallel_step_at_world_size_one_trains_on_nstep_targets():
    from cartpoleplusplus_amd import ddpg_cartpole as D
    B, rows = 32, 400
    agent, _ref, (aspec, cspec) = make_pair(PIX, B, True, seed=6, replay_size=rows + 40)
    lib, check, ptr = _lib()
    try:
        rm, t = agent.replay_memory, agent.trainer
        rm.fill_synthetic(rows, seed=25)
        rm.enable_n_step(3, D.opts.discount)
        nets = (agent.actor, agent.critic, agent.target_actor, agent.target_critic)
        Pm = [n.get_params() for n in nets]
        check(lib.cpp_ddpg_dp_train_step(t.handle, rm.handle, None, B, 1, 7, 1, 0))
        idxs = np.empty(B, np.int32)
        check(lib.cpp_replay_last_indexes(rm.handle, B, ptr(idxs)))
        _a, _dq, q, td = t.last_values(B)
        codes_c, relu_c = device_pool_codes(agent.critic, B), device_relu_active(agent.critic, B)
        hb = rm.batch(idxs=idxs)
        s1, s2 = rm.state[hb.state_1_idx], rm.state[hb.state_2_idx]
        batch = (s1, hb.action, hb.reward, hb.terminal_mask, s2)
    finally:
        agent.close()
    ref = O.DDPG(aspec, cspec, Pm[0], Pm[1], np.float64)
    ref.set_targets(Pm[2], Pm[3])
    ref.critic.amax_override, ref.critic.relu_override = codes_c, relu_c
    cg = ref.critic_gradients(batch)
    assert np.abs(q - cg["q"]).max() < 1e-5 and np.abs(td - cg["td"]).max() < 1e-5
    assert (hb.reward > 1).any()                               # (synthetic rewards are 1: the n-step returns are larger)


def test_discount_mismatch_is_refused():
    """every trainer entry point refuses an n > 1 memory folded with another discount, writing nothing: parameters, the sampler's
    counter (the next draw is a fresh agent's first) and the priority tree stay as they were"""
    from cartpoleplusplus_amd import ddpg_cartpole as D
    lib, check, ptr = _lib()
    B = 32
    kw = dict(prioritized_replay=True, priority_alpha=0.6, priority_beta=0.4, priority_eps=1e-6)
    agent, _r, _ = make_pair(PIX, B, True, seed=8, replay_size=240, **kw)
    fresh, _r, _ = make_pair(PIX, B, True, seed=8, replay_size=240, **kw)
    try:
        rm, t = agent.replay_memory, agent.trainer
        for x in (agent, fresh):
            x.replay_memory.fill_synthetic(200, seed=27)
        rm.enable_n_step(3, 0.5)
        before, tree = [n.get_params() for n in agent.networks()], rm.priority_tree()
        rows = np.arange(B, dtype=np.int32)
        with pytest.raises(RuntimeError, match="discount"):
            agent.train_step(B, 1)
        for name, args in (("cpp_ddpg_train_step", (t.handle, rm.handle, B, 1, None, 0)),
                           ("cpp_ddpg_train_rows", (t.handle, rm.handle, B, ptr(rows))),
                           ("cpp_ddpg_sample_and_compute", (t.handle, rm.handle, B, 0)),
                           ("cpp_ddpg_dp_train_step", (t.handle, rm.handle, None, B, 1, 0, 1, 0))):
            assert getattr(lib, name)(*args) == 1, name
            assert b"discount" in lib.cpp_last_error() or b"prioritized" in lib.cpp_last_error(), name
        for x, y in zip(before, agent.networks()):
            assert np.array_equal(x, y.get_params())
        assert np.array_equal(tree, rm.priority_tree())
        n, d = ctypes.c_int(), ctypes.c_float()
        check(lib.cpp_replay_get_n_step(rm.handle, ctypes.byref(n), ctypes.byref(d)))
        assert (n.value, d.value) == (3, 0.5)
        # the counter has not moved: after the discount is put right, the step draws the rows of a fresh agent's first step
        rm.enable_n_step(3, D.opts.discount)
        fresh.replay_memory.enable_n_step(3, D.opts.discount)
        agent.train_step(B, 1)
        fresh.train_step(B, 1)
        for x, y in zip(agent.networks(), fresh.networks()):
            assert np.array_equal(x.get_params(), y.get_params()), x.namespace
        assert np.array_equal(rm.priority_tree(), fresh.replay_memory.priority_tree())
    finally:
        agent.close()
        fresh.close()
    # the NAF learner's five entry points, on a uniform memory (no prioritized refusal in the way)
    from cartpoleplusplus_amd import naf_cartpole as F
    naf, _specs = make_naf(LOWDIM, B, True, seed=1, replay_size=240)
    try:
        rm, h = naf.replay_memory, naf.naf.handle
        rm.fill_synthetic(200, seed=29)
        rm.enable_n_step(2, 0.25)
        before = [n.get_params() for n in (naf.value_net, naf.naf.mu_net, naf.naf.l_net, naf.target_value_net)]
        ticket, loss = ctypes.c_uint64(), ctypes.c_float()
        for name, args in (("cpp_naf_train_step", (h, rm.handle, B, 1, None, 0)),
                           ("cpp_naf_train_rows", (h, rm.handle, B, ptr(rows), ctypes.byref(loss))),
                           ("cpp_naf_train_rows_async", (h, rm.handle, B, ptr(rows), ctypes.byref(ticket))),
                           ("cpp_naf_sample_and_compute", (h, rm.handle, B, 0)),
                           ("cpp_naf_dp_train_step", (h, rm.handle, None, B, 1, 0, 1))):
            assert getattr(lib, name)(*args) == 1, name
            assert b"discount" in lib.cpp_last_error(), name
        after = [n.get_params() for n in (naf.value_net, naf.naf.mu_net, naf.naf.l_net, naf.target_value_net)]
        for x, y in zip(before, after):
            assert np.array_equal(x, y)
        rm.enable_n_step(2, F.opts.discount)
        naf.train_step(B, 1)                                     # (the matching discount trains)
    finally:
        naf.close()
