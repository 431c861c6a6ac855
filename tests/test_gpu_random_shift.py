"""Random shift (DrQ) in the device gather (csrc/gather_body.h ShiftVec / shift_draw; semantics in include/cartpolepp_abi.h) against
the numpy restatement tests/shift_np.py: the shifted gather bit for bit (f16 and 8-bit stores, square, non-square and full-size
images, every pad up to the largest), the augmentation counter on every path, one fused minibatch against the unmodified float64
oracles fed the shifted minibatch rebuilt on the host (DDPG cfg3, n-step + prioritized, NAF cfg4, the 8-bit store), the literal loop
against the fused step, a captured step graph that follows the switch, never-enabled = the parent's behaviour, determinism, the
data-parallel step at world size 1 and the refusals."""
import ctypes

import numpy as np
import pytest

from oracle import ddpg_np as O
from oracle import naf_np as N
from tests import shift_np as S
from tests.helpers import (assert_flat_close, device_pool_codes, device_relu_active, make_pair, pool_flips_are_near_ties,
                           relu_flips_are_at_the_boundary)
from tests.test_gpu_naf_prioritized_replay import CatSpec, last_rows, make_naf, MOMENTUM

pytestmark = pytest.mark.gpu

LOWDIM = (2, 2, 7)
PIX = (32, 32, 3, 2, 3)
CFG = (64, 64, 3, 2, 3)
ATOL, GRAD_REL = 1e-5, 2e-5            # (the tolerances of the n-step and prioritized-replay oracle tests)
SEED = 11


def _lib():
    from cartpoleplusplus_amd._lib import lib, check, ptr
    return lib, check, ptr


def _same(a, b, what=""):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.shape == b.shape and a.dtype == b.dtype, (what, a.shape, b.shape)
    assert np.array_equal(a.view(np.uint16) if a.dtype == np.float16 else a, b.view(np.uint16) if b.dtype == np.float16 else b), what


def _rows(agent, B):
    lib, check, ptr = _lib()
    rows = np.empty(B, np.int32)
    check(lib.cpp_replay_last_indexes(agent.replay_memory.handle, B, ptr(rows)))
    return rows


def _shifted_minibatch(rm, idxs):
    """the minibatch the last augmented gather of rows `idxs` formed, rebuilt on the host: (s1, a, r, m, s2) shifted, and unshifted"""
    hb = rm.batch(idxs=idxs)                     # (the n-step columns, if the memory folds them)
    sh = rm.last_shifts(len(idxs))
    s1u, s2u = rm.state[hb.state_1_idx], rm.state[hb.state_2_idx]
    s1, s2 = S.shift_images(s1u, sh[0]), S.shift_images(s2u, sh[1])
    assert (np.abs(sh).max(axis=(1, 2)) > 0).all() and not np.array_equal(s1, s1u)
    return (s1, hb.action, hb.reward, hb.terminal_mask, s2), (s1u, hb.action, hb.reward, hb.terminal_mask, s2u), sh


# ---- 1. the gather, bit for bit ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("store", ["f16", "u8"])
@pytest.mark.parametrize("shape,B", [(PIX, 64), ((12, 10, 3, 3, 1), 48), (CFG, 256)], ids=["32x32x18", "12x10x9", "64x64x18-B256"])
def test_gather_shifted_matches_numpy_bit_for_bit(store, shape, B):
    from cartpoleplusplus_amd.replay_memory import ReplayMemory
    rows = 300
    rm = ReplayMemory(rows + 20, shape, 2, store_dtype=store)
    try:
        rm.fill_synthetic(rows, seed=5)
        rng = np.random.default_rng(3)
        for pad in (1, 4, min(16, min(shape[:2]) - 1)):
            seed = SEED + pad + (1 << 40)
            rm.enable_random_shift(pad, seed=seed)
            assert rm.random_shift == (pad, seed) and rm.shift_counter() == 0
            for k in range(2):
                idxs = rng.integers(0, rows, B).astype(np.int32)
                idxs[1], idxs[B - 1] = idxs[0], idxs[0]                       # duplicate rows: every copy draws its own shift
                s1, s2, sh = rm.gather_shifted(idxs)
                assert sh.shape == (2, B, 2) and sh.dtype == np.int32
                assert np.array_equal(sh, S.shifts(seed, k, B, pad)), (pad, k)
                assert np.array_equal(sh, rm.last_shifts(B))
                _same(s1, S.shift_images(rm.state[rm.state_1_idx[idxs]], sh[0]), "state_1 pad=%d" % pad)
                _same(s2, S.shift_images(rm.state[rm.state_2_idx[idxs]], sh[1]), "state_2 pad=%d" % pad)
                assert rm.shift_counter() == k + 1
            assert len({tuple(x) for x in sh[0]}) > 1
    finally:
        rm.close()


# ---- 2. the counter ---------------------------------------------------------------------------------------------------------------
def test_counter_moves_once_per_augmented_minibatch_and_never_otherwise():
    B, rows, pad = 32, 200, 4
    lib, check, ptr = _lib()
    agent, _ref, _ = make_pair(PIX, B, True, seed=3, replay_size=rows + 60)
    try:
        rm, t = agent.replay_memory, agent.trainer
        rm.fill_synthetic(rows, seed=21)
        rm.enable_random_shift(pad, seed=SEED)
        assert rm.shift_counter() == 0
        rm.gather_shifted(np.arange(B))
        assert rm.shift_counter() == 1
        agent.train_step(B, 3)                                 # eager (and captured)
        assert rm.shift_counter() == 4
        assert np.array_equal(rm.last_shifts(B), S.shifts(SEED, 3, B, pad))
        agent.train_step(B, 3)                                 # replayed from the captured graph
        assert rm.shift_counter() == 7
        first = rm.last_shifts(B)
        assert np.array_equal(first, S.shifts(SEED, 6, B, pad))
        agent.train_step(B, 3)
        assert rm.shift_counter() == 10
        assert np.array_equal(rm.last_shifts(B), S.shifts(SEED, 9, B, pad)) and not np.array_equal(first, rm.last_shifts(B))
        # the literal loop: one minibatch, its rows from the host
        np.random.seed(5)
        for k in range(2):
            batch = rm.batch(B)
            agent.actor.train(batch.state_1)
            agent.critic.train(batch)
            assert rm.shift_counter() == 11 + k
            assert np.array_equal(rm.last_shifts(B), S.shifts(SEED, 10 + k, B, pad))
            assert np.array_equal(_rows(agent, B), batch.idxs)
        check(lib.cpp_ddpg_sample_and_compute(t.handle, rm.handle, B, 0))
        assert rm.shift_counter() == 13
        check(lib.cpp_ddpg_sample_and_compute(t.handle, rm.handle, B, 0))
        assert rm.shift_counter() == 14
        # draws, inspection gathers and host reads leave it alone and show the stored pixels
        b = rm.batch(B)
        dev = b.device
        s1d, s2d = np.empty((B,) + PIX, np.float16), np.empty((B,) + PIX, np.float16)
        check(lib.cpp_batch_download(dev.handle, ptr(s1d), ptr(s2d), None, None, None))
        _same(s1d, rm.state[b.state_1_idx], "Batch.device state_1")
        _same(s2d, rm.state[b.state_2_idx], "Batch.device state_2")
        d = rm.sample_on_device(B, seed=1, counter=0)
        _same(np.asarray(d.state_1), rm.state[d.state_1_idx], "sample_on_device")
        b2 = rm.batch(B)
        stored1, stored2 = rm.state[b2.state_1_idx], rm.state[b2.state_2_idx]
        _same(np.asarray(b2.state_1), stored1, "host read of state_1")
        b3 = rm.batch(B)                                        # never read before the memory is written: preserved by add_episode
        stored3 = rm.state[b3.state_2_idx]
        rng = np.random.default_rng(9)
        codes = (np.arange(256) / 255.0).astype(np.float16)
        frames = [codes[rng.integers(0, 256, PIX)] for _ in range(4)]
        rm.add_episode(frames[0], [(rng.uniform(-1, 1, 2).astype(np.float32), 1.0, f) for f in frames[1:]])
        _same(np.asarray(b3.state_2), stored3, "preserved Batch, state_2")
        _same(np.asarray(b2.state_1), stored1, "read Batch after the write")
        _same(np.asarray(b2.state_2), stored2, "read Batch after the write, state_2")
        assert rm.shift_counter() == 14
    finally:
        agent.close()


# ---- 3. one fused minibatch against the float64 oracles ---------------------------------------------------------------------------
def _ddpg_shift_against_f64_oracle(shape, B, rows, seed=0, per=False, nstep=1, store="f16", pad=4, grad_rel=None, capacity=None, **pair_kw):
    """ONE graph-replayed minibatch of the fused DDPG step on a memory with random shift on against oracle.DDPG(float64), unmodified,
    fed the shifted minibatch rebuilt on the host: actions / Q / TD at ATOL, the pre-clip gradients at GRAD_REL; the same oracle fed
    the stored (unshifted) pixels must miss the device's Q by more than 100 x ATOL.  grad_rel (None: GRAD_REL), pair_kw: the bar of the
    gradient lists and make_pair's options for other networks (use_batch_norm).  capacity=C > B: the agent is built for C rows; a C-row
    step and its replay run first (two draws of C shifts), and behind the checked B-row replay one more C-row step is held to the same
    bars."""
    grad_rel = GRAD_REL if grad_rel is None else grad_rel
    from cartpoleplusplus_amd import ddpg_cartpole as D
    from tests import per_np as P
    kw = dict(prioritized_replay=True, priority_alpha=0.6, priority_beta=0.4, priority_eps=1e-6) if per else {}
    kw.update(pair_kw)
    agent, _ref, (aspec, cspec) = make_pair(shape, B, True, seed=seed, replay_size=rows + 50, replay_store=store, capacity=capacity, **kw)
    try:
        rm = agent.replay_memory
        rm.fill_synthetic(rows, seed=21 + seed)
        if nstep > 1:
            rm.enable_n_step(nstep, D.opts.discount)
        rm.enable_random_shift(pad, seed=SEED + seed)
        C = B if capacity is None else int(capacity)
        draws = 0
        for _ in range(2 if C > B else 0):
            agent.train_step(C, 1)                            # eager pass + capture, its replay
            draws += 1
        agent.train_step(B, 1)                                # eager pass + capture
        draws += 1
        if per:
            rm.update_priorities(np.arange(rows), np.random.default_rng(seed + 9).lognormal(0.0, 2.0, rows).astype(np.float32))
        nets = (agent.actor, agent.critic, agent.target_actor, agent.target_critic)

        def step_and_read(Bx):
            d = {"Pm": [n.get_params() for n in nets]}
            assert rm.shift_counter() == draws
            agent.train_step(Bx, 1)                           # hipGraph replay where this key's graph is held
            assert rm.shift_counter() == draws + 1
            idxs = _rows(agent, Bx)
            d["w"] = rm.last_weights(Bx) if per else None
            d["values"] = agent.trainer.last_values(Bx)
            d["grads"] = (agent.actor.get_grads(), agent.critic.get_grads())
            d["codes"] = (device_pool_codes(agent.actor, Bx), device_pool_codes(agent.critic, Bx))
            d["relu"] = (device_relu_active(agent.actor, Bx), device_relu_active(agent.critic, Bx))
            d["t"], d["t_unshifted"], sh = _shifted_minibatch(rm, idxs)
            assert np.array_equal(sh, S.shifts(SEED + seed, draws, Bx, pad))
            return d
        checked = step_and_read(B)
        draws += 1
        back = step_and_read(C) if C > B else None
    finally:
        agent.close()
    for d in (checked, back):
        if d is not None:
            _check_shifted(d, aspec, cspec, per, grad_rel)


def _check_shifted(d, aspec, cspec, per, grad_rel):
    """what _ddpg_shift_against_f64_oracle's step_and_read() brought back from one minibatch"""
    Pm, w, t, t_unshifted = d["Pm"], d["w"], d["t"], d["t_unshifted"]
    actions, _dq, q, td = d["values"]
    g_a, g_c = d["grads"]
    (codes_a, codes_c), (relu_a, relu_c) = d["codes"], d["relu"]
    ref = O.DDPG(aspec, cspec, Pm[0], Pm[1], np.float64)
    ref.set_targets(Pm[2], Pm[3])
    ref.actor.amax_override, ref.critic.amax_override = codes_a, codes_c
    ref.actor.relu_override, ref.critic.relu_override = relu_a, relu_c
    ag = ref.actor_gradients(t[0])
    cg = ref.critic_gradients(t)
    pool_flips_are_near_ties(ag["cache_actor"], codes_a, 1e-5, what="actor")
    pool_flips_are_near_ties(cg["cache_critic"], codes_c, 1e-5, what="critic")
    relu_flips_are_at_the_boundary(ag["cache_actor"], relu_a, 1e-5, what="actor")
    relu_flips_are_at_the_boundary(cg["cache_critic"], relu_c, 1e-5, what="critic")
    err = (np.abs(actions - ag["actions"]).max(), np.abs(q - cg["q"]).max(), np.abs(td - cg["td"]).max())
    miss = np.abs(q - ref.critic_gradients(t_unshifted)["q"]).max()
    print("random shift vs f64 oracle: |actions| %.2e |q| %.2e |td| %.2e; unshifted oracle misses q by %.2e" % (err + (miss,)))
    assert max(err) < ATOL, err
    assert miss > 100 * ATOL, miss
    assert_flat_close(aspec, g_a, ag["grads"], rel=grad_rel, what="actor pre-clip grads vs f64 oracle (random shift)")
    if per:
        cw = ref.critic_gradients(t, td_override=w.astype(np.float64).reshape(-1, 1) * td.astype(np.float64))
        assert_flat_close(cspec, g_c, cw["grads"], rel=grad_rel, what="weighted critic pre-clip grads vs f64 oracle (random shift)")
    else:
        assert_flat_close(cspec, g_c, cg["grads"], rel=grad_rel, what="critic pre-clip grads vs f64 oracle (random shift)")


def test_shifted_step_below_the_capacity_against_f64_oracle():
    """(C, B) = (8, 5): B shifts per image set drawn and applied behind C-row steps, and back"""
    _ddpg_shift_against_f64_oracle((16, 16, 3, 1, 2), 5, 300, capacity=8)


def test_shifted_fused_step_against_f64_oracle_cfg3():
    _ddpg_shift_against_f64_oracle(CFG, 256, 2500)


def test_shifted_prioritized_nstep_step_against_f64_oracle():
    _ddpg_shift_against_f64_oracle(CFG, 256, 2500, seed=2, per=True, nstep=3)


def test_shifted_u8_store_step_against_f64_oracle():
    _ddpg_shift_against_f64_oracle(CFG, 256, 2500, seed=1, store="u8")


def test_shifted_naf_step_against_f64_oracle_cfg4():
    """one graph-replayed minibatch of the fused NAF step (cfg4: shared trunk, Momentum) with random shift on against
    oracle.naf_np.NAF (float64, unmodified) fed the shifted minibatch: the loss at 1e-5, the pre-clip gradients at 2e-5; fed the
    stored pixels it misses the loss by more than 100 x that"""
    from cartpoleplusplus_amd import naf_cartpole as F
    shape, B, share, rows, pad = CFG, 256, True, 2500, 4
    agent, specs = make_naf(shape, B, share, seed=0, replay_size=rows + 50)
    try:
        rm = agent.replay_memory
        rm.fill_synthetic(rows, seed=33)
        rm.enable_random_shift(pad, seed=SEED)
        agent.train_step(B, 1)                                # eager pass + capture
        nets = (agent.value_net, agent.naf.mu_net, agent.naf.l_net, agent.target_value_net)
        Pm = [n.get_params() for n in nets]
        opt = agent.naf.get_optimiser_state()
        agent.train_step(B, 1)                                # hipGraph replay
        assert rm.shift_counter() == 2
        idxs = last_rows(agent, B)
        grads, stats = agent.naf.get_grads(), agent.naf.last_stats()
        codes, relu = device_pool_codes(agent.value_net, B), device_relu_active(agent.value_net, B)
        batch, unshifted, sh = _shifted_minibatch(rm, idxs)
        assert np.array_equal(sh, S.shifts(SEED, 1, B, pad))
    finally:
        agent.close()
    vspec, mspec, lspec = specs
    ref = N.NAF(vspec, mspec, lspec, Pm[0], Pm[1], Pm[2], share, 2, np.float64, discount=F.opts.discount, gradient_clip=5.0,
                optimiser=N.make_optimiser(*MOMENTUM))
    ref.target_value = O.Net(vspec, Pm[3], np.float64)
    ref.m = opt["m"].astype(np.float64)
    ref.value.amax_override, ref.value.relu_override = codes, relu
    out = ref.forward_backward(batch)
    cache = ref.value.forward(batch[0], white=ref._white(ref.value, batch[0]), training=True)
    pool_flips_are_near_ties(cache, codes, what="value trunk")
    relu_flips_are_at_the_boundary(cache, relu, what="value trunk")
    miss = abs(stats[0] - ref.forward_backward(unshifted)["loss"])
    print("random shift NAF: loss %.8f oracle %.8f; unshifted oracle misses by %.2e" % (stats[0], out["loss"], miss))
    assert stats[2] == 0
    assert abs(stats[0] - out["loss"]) < 1e-5 * max(1.0, abs(out["loss"])), (stats[0], out["loss"])
    assert miss > 100 * 1e-5 * max(1.0, abs(out["loss"])), miss
    assert_flat_close(CatSpec(specs), grads, out["grads"], rel=2e-5, what="NAF pre-clip grads vs f64 oracle (random shift)")


# ---- 4. the literal loop is the fused step ----------------------------------------------------------------------------------------
def test_reference_loop_is_the_fused_step_ddpg():
    """ddpg_cartpole.py:331-337 verbatim with random shift on (the train calls gather the draw's rows, shifted) against
    agent.train_step on the same rows, the same seed and the same starting counter: bit for bit after each of 3 minibatches"""
    B = 32

    def agent():
        a, _ref, _ = make_pair(PIX, B, True, seed=3, replay_size=240)
        a.replay_memory.fill_synthetic(200, seed=21)
        a.replay_memory.enable_random_shift(4, seed=SEED)
        return a
    lit, fused = agent(), agent()
    try:
        np.random.seed(11)
        for step in range(3):
            batch = lit.replay_memory.batch(B)
            lit.actor.train(batch.state_1)
            lit.critic.train(batch)
            lit.target_actor.update_weights()
            lit.target_critic.update_weights()
            fused.train_step(B, 1, idxs=batch.idxs)
            assert np.array_equal(lit.replay_memory.last_shifts(B), fused.replay_memory.last_shifts(B))
            for a, b in zip(lit.networks(), fused.networks()):
                assert np.array_equal(a.get_params(), b.get_params()), (step, a.namespace)
        assert lit.trainer.fused_pairs == 3
        assert lit.replay_memory.shift_counter() == 3 and fused.replay_memory.shift_counter() == 3
    finally:
        lit.close()
        fused.close()


def test_reference_loop_is_the_fused_step_naf():
    """naf_cartpole.py:365-373 verbatim with random shift on against agent.train_step on the same rows: bit for bit"""
    B = 32

    def agent():
        a, _ = make_naf(PIX, B, True, seed=5, replay_size=240)
        a.replay_memory.fill_synthetic(200, seed=4)
        a.replay_memory.enable_random_shift(4, seed=SEED)
        return a
    lit, fused = agent(), agent()
    try:
        np.random.seed(12)
        for step in range(3):
            batch = lit.replay_memory.batch(B)
            loss = lit.naf.train(batch)
            lit.target_value_net.update_weights()
            fused.train_step(B, 1, idxs=batch.idxs)
            assert np.isfinite(float(loss))
            assert np.array_equal(lit.replay_memory.last_shifts(B), fused.replay_memory.last_shifts(B))
            for a, b in zip(lit.networks(), fused.networks()):
                assert np.array_equal(a.get_params(), b.get_params()), (step, a.namespace)
        assert lit.replay_memory.shift_counter() == 3 and fused.replay_memory.shift_counter() == 3
    finally:
        lit.close()
        fused.close()


# ---- 5. a captured graph follows the switch ---------------------------------------------------------------------------------------
def test_captured_graph_follows_the_switch():
    B, pad = 32, 4

    def agent():
        a, _ref, _ = make_pair(PIX, B, True, seed=5, replay_size=240)
        a.replay_memory.fill_synthetic(200, seed=23)
        return a
    g, twin = agent(), agent()
    try:
        for _ in range(3):                                       # captured at the first step, replayed after
            g.train_step(B, 2)
            twin.train_step(B, 2)
        for a, b in zip(g.networks(), twin.networks()):
            assert np.array_equal(a.get_params(), b.get_params()), a.namespace
        rm = g.replay_memory
        rm.enable_random_shift(pad, seed=SEED)
        before = [n.get_params() for n in g.networks()]
        g.train_step(B, 2)
        twin.train_step(B, 2)                                    # (keeps the twin's sampler in step)
        assert rm.shift_counter() == 2
        assert np.array_equal(rm.last_shifts(B), S.shifts(SEED, 1, B, pad))
        assert any(not np.array_equal(x, n.get_params()) for x, n in zip(before, g.networks()))
        assert any(not np.array_equal(a.get_params(), b.get_params()) for a, b in zip(g.networks(), twin.networks()))
        g.train_step(B, 2)                                       # (the shifting form, replayed from its own graph)
        twin.train_step(B, 2)
        assert rm.shift_counter() == 4
        rm.enable_random_shift(0)
        assert rm.random_shift == (0, 0) and rm.shift_counter() == 0
        for a, b in zip(g.networks(), twin.networks()):          # the twin takes g's parameters: from here on the two must agree again
            b.set_params(a.get_params())
        for _ in range(2):
            g.train_step(B, 2)
            twin.train_step(B, 2)
            for a, b in zip(g.networks(), twin.networks()):
                assert np.array_equal(a.get_params(), b.get_params()), a.namespace
    finally:
        g.close()
        twin.close()


# ---- 6. never enabled = the parent's behaviour ------------------------------------------------------------------------------------
def test_enabled_then_disabled_is_the_memory_that_never_had_it():
    B = 32
    a, _r, _ = make_pair(PIX, B, True, seed=3, replay_size=240)
    b, _r, _ = make_pair(PIX, B, True, seed=3, replay_size=240)
    try:
        for x in (a, b):
            x.replay_memory.fill_synthetic(200, seed=21)
        b.replay_memory.enable_random_shift(4, seed=SEED)
        b.replay_memory.enable_random_shift(0)
        for _ in range(3):
            a.train_step(B, 3)
            b.train_step(B, 3)
        for x, y in zip(a.networks(), b.networks()):
            assert np.array_equal(x.get_params(), y.get_params()), x.namespace
        assert b.replay_memory.shift_counter() == 0
        with pytest.raises(RuntimeError):
            a.replay_memory.last_shifts(B)                       # (never enabled: there is no augmented gather to report)
    finally:
        a.close()
        b.close()


# ---- 7. determinism ---------------------------------------------------------------------------------------------------------------
def test_two_runs_are_identical():
    B = 64

    def run():
        a, _r, _ = make_pair(CFG, B, True, seed=7, replay_size=340)
        try:
            a.replay_memory.fill_synthetic(300, seed=31)
            a.replay_memory.enable_random_shift(4, seed=SEED)
            for _ in range(3):
                a.train_step(B, 3)
            return [n.get_params() for n in a.networks()], a.replay_memory.last_shifts(B), a.replay_memory.shift_counter()
        finally:
            a.close()
    (p0, s0, c0), (p1, s1, c1) = run(), run()
    assert c0 == c1 == 9 and np.array_equal(s0, s1)
    for x, y in zip(p0, p1):
        assert np.array_equal(x, y)


# ---- 8. the data-parallel step at world size 1 ------------------------------------------------------------------------------------
def test_data_parallel_step_at_world_size_one_trains_on_shifted_minibatches():
    B, rows, pad = 32, 400, 4
    agent, _ref, (aspec, cspec) = make_pair(PIX, B, True, seed=6, replay_size=rows + 40)
    lib, check, ptr = _lib()
    try:
        rm, t = agent.replay_memory, agent.trainer
        rm.fill_synthetic(rows, seed=25)
        rm.enable_random_shift(pad, seed=SEED)
        check(lib.cpp_ddpg_dp_train_step(t.handle, rm.handle, None, B, 2, 7, 1, 0))
        assert rm.shift_counter() == 2
        nets = (agent.actor, agent.critic, agent.target_actor, agent.target_critic)
        Pm = [n.get_params() for n in nets]
        check(lib.cpp_ddpg_dp_train_step(t.handle, rm.handle, None, B, 1, 7, 1, 0))
        assert rm.shift_counter() == 3
        idxs = _rows(agent, B)
        _a, _dq, q, td = t.last_values(B)
        codes_c, relu_c = device_pool_codes(agent.critic, B), device_relu_active(agent.critic, B)
        batch, unshifted, sh = _shifted_minibatch(rm, idxs)
        assert np.array_equal(sh, S.shifts(SEED, 2, B, pad))
    finally:
        agent.close()
    ref = O.DDPG(aspec, cspec, Pm[0], Pm[1], np.float64)
    ref.set_targets(Pm[2], Pm[3])
    ref.critic.amax_override, ref.critic.relu_override = codes_c, relu_c
    cg = ref.critic_gradients(batch)
    assert np.abs(q - cg["q"]).max() < ATOL and np.abs(td - cg["td"]).max() < ATOL
    assert np.abs(q - ref.critic_gradients(unshifted)["q"]).max() > 100 * ATOL


# ---- 9. refusals ------------------------------------------------------------------------------------------------------------------
def test_refusals_write_nothing():
    from cartpoleplusplus_amd.replay_memory import ReplayMemory
    lib, check, ptr = _lib()

    def state(rm):
        p, s, n = ctypes.c_int(-1), ctypes.c_uint64(99), ctypes.c_uint64(99)
        check(lib.cpp_replay_get_random_shift(rm.handle, ctypes.byref(p), ctypes.byref(s), ctypes.byref(n)))
        return p.value, s.value, n.value
    low = ReplayMemory(40, LOWDIM, 2)
    pix = ReplayMemory(40, (12, 10, 3, 1, 3), 2)
    try:
        low.fill_synthetic(30)
        pix.fill_synthetic(30)
        with pytest.raises(ValueError):
            low.enable_random_shift(1)
        assert lib.cpp_replay_set_random_shift(low.handle, 2, 14, 1, 0) == 1 and b"pixel" in lib.cpp_last_error()
        assert state(low) == (0, 0, 0) and low.random_shift == (0, 0)
        for pad in (-1, 17, 10, 11):
            with pytest.raises(ValueError):
                pix.enable_random_shift(pad)
            assert lib.cpp_replay_set_random_shift(pix.handle, 12, 10, pad, 5) == 1, pad
            assert b"pad" in lib.cpp_last_error()
        for H, W in ((12, 11), (11, 10), (6, 21), (0, 10)):
            assert lib.cpp_replay_set_random_shift(pix.handle, H, W, 2, 5) == 1, (H, W)
        assert state(pix) == (0, 0, 0)
        assert lib.cpp_replay_last_shifts(pix.handle, 8, ptr(np.empty((2, 8, 2), np.int32))) != 0      # (nothing to report)
        # ... and an enabled memory keeps its setting and its counter through a refused call
        pix.enable_random_shift(3, seed=77)
        pix.gather_shifted(np.arange(8))
        assert state(pix) == (3, 77, 1)
        assert lib.cpp_replay_set_random_shift(pix.handle, 12, 10, 10, 5) == 1
        assert lib.cpp_replay_set_random_shift(pix.handle, 11, 10, 3, 5) == 1
        assert state(pix) == (3, 77, 1) and pix.random_shift == (3, 77)
        sh = pix.last_shifts(8)
        assert np.array_equal(sh, S.shifts(77, 0, 8, 3))
        pix.enable_random_shift(9, seed=78)                      # (the largest pad a 12 x 10 image allows; the counter starts again)
        assert state(pix) == (9, 78, 0)
    finally:
        low.close()
        pix.close()
