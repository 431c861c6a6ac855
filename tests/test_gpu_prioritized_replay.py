"""Prioritized experience replay on the device (csrc/per.hip; semantics in include/cartpolepp_abi.h) against the numpy restatement
tests/per_np.py: the sum tree bit for bit, the stratified draw bit for bit (its top-end guard included), the importance weights, the
weighted critic loss and the priorities the DDPG step writes, the literal loop against the fused step, reproducibility, the
refusals and the command line."""
import ctypes
import json

import numpy as np
import pytest

from oracle import ddpg_np as O
from tests import per_np as P
from tests.helpers import (assert_flat_close, device_pool_codes, device_relu_active, make_pair, pool_flips_are_near_ties,
                           relu_flips_are_at_the_boundary)

pytestmark = pytest.mark.gpu

LOWDIM = (2, 2, 7)
PIX = (32, 32, 3, 2, 3)
PARTIAL_PER_SEED = 3          # (test_prioritized_step_below_the_capacity_against_f64_oracle: of seeds 0 .. 11 one whose priorities give the five-row
#                               and the eight-row draw a weight below 0.5 at every sampler counter 0 .. 7 -- tests/per_np.py's draw over the known tree)


def _memory(n, alpha=0.6, eps=1e-6):
    from cartpoleplusplus_amd.replay_memory import ReplayMemory
    rm = ReplayMemory(n, LOWDIM, 2)
    rm.enable_priorities(alpha, eps)
    return rm


def _leaves(rm):
    t = rm.priority_tree()
    L = P.levels(rm.buffer_size)
    return t, L, t[1 << L:(1 << L) + rm.buffer_size]


@pytest.mark.parametrize("n", [22000, 1000000])
def test_tree_matches_numpy_bit_for_bit(n):
    rm = _memory(n)
    try:
        rm.fill_synthetic(n, seed=3)                      # a full memory: the next episode overwrites the oldest rows
        t, L, leaves = _leaves(rm)
        assert (leaves == 1.0).all() and np.array_equal(t, P.build(leaves, L))
        rng = np.random.default_rng(n)
        rows = rng.integers(0, n, 3000).astype(np.int32)
        rows[100:110] = rows[0]                           # duplicates: the last occurrence wins
        td = rng.normal(0, 3, 3000).astype(np.float32)
        rm.update_priorities(rows, np.abs(td))
        p = P.priority(td, 0.6, 1e-6)
        last = {int(r): float(v) for r, v in zip(rows, p)}
        keys = np.array(sorted(last), np.int32)
        got = rm.priorities(keys)
        assert np.abs(got / np.array([last[k] for k in keys], np.float32) - 1).max() < 2e-6       # (device powf against numpy's)
        lastpos = int(np.nonzero(rows == rows[0])[0][-1])   # rows[0] occurs 11+ times: it holds the priority of its last position
        dup = rm.priorities(rows[:1])[0]
        assert lastpos >= 109 and abs(dup / p[lastpos] - 1) < 2e-6 and abs(p[0] / p[lastpos] - 1) > 1e-3
        t, L, leaves = _leaves(rm)
        assert np.array_equal(t, P.build(leaves, L))      # every inner node left + right, bit for bit
        untouched = np.setdiff1d(np.arange(n), keys)
        assert (leaves[untouched] == 1.0).all()
        # new rows (FIFO overwrites of rows 0..11) take the running maximum of every priority written so far
        pmax = max(1.0, float(p.max()))                  # (duplicates' earlier values included)
        seq = [(np.zeros(2, np.float32), 1.0, np.full(LOWDIM, k, np.float32)) for k in range(12)]
        rm.add_episode(np.zeros(LOWDIM, np.float32), seq)
        new = rm.priorities(np.arange(12))
        assert (new == new[0]).all() and abs(new[0] / pmax - 1) < 2e-6
        t, L, leaves = _leaves(rm)
        assert np.array_equal(t, P.build(leaves, L))
    finally:
        rm.close()


def test_draws_and_weights_match_numpy():
    n = 22000
    rm = _memory(n)
    try:
        rm.fill_synthetic(n - 500, seed=4)
        size = n - 500
        rng = np.random.default_rng(5)
        rm.update_priorities(np.arange(size), np.abs(rng.standard_cauchy(size)).astype(np.float32))
        rm.set_priority_beta(0.4)
        t, L, _ = _leaves(rm)
        for B in (256, 512):
            for ctr in (0, 7, 2 ** 33 + 5):
                b = rm.sample_on_device(B, seed=11, counter=ctr)
                rows, _g = P.draw(t, L, size, B, 11, ctr)
                assert np.array_equal(b.idxs, rows), (B, ctr)
                w = rm.last_weights(B)
                want = P.weights(t, L, size, rows, 0.4)
                assert np.abs(w / want - 1).max() < 1e-6 and w.max() == 1.0
        # the top-end guard: rows written past `size` (their leaves hold the maximum) draw the strata above it onto row size - 1
        from cartpoleplusplus_amd._lib import lib, check, ptr
        extra = np.arange(size, size + 200, dtype=np.int32)
        z = np.zeros(200, np.int32)
        check(lib.cpp_replay_write_rows(rm.handle, ptr(extra), 200, ptr(z), ptr(z), ptr(np.zeros((200, 2), np.float32)),
                                        ptr(np.zeros(200, np.float32)), ptr(np.zeros(200, np.float32))))
        t, L, _ = _leaves(rm)
        b = rm.sample_on_device(512, seed=11, counter=3)
        rows, guarded = P.draw(t, L, size, 512, 11, 3)
        assert guarded.any() and np.array_equal(b.idxs, rows)
        assert np.abs(rm.last_weights(512) / P.weights(t, L, size, rows, 0.4) - 1).max() < 1e-6
    finally:
        rm.close()


def _agent(B=32, rows=200, seed=3, **per):
    kw = dict(prioritized_replay=True, priority_alpha=0.6, priority_beta=0.4, priority_eps=1e-6)
    kw.update(per)
    agent, _ref, _ = make_pair(PIX, B, True, seed=seed, replay_size=rows + 40, **kw)
    agent.replay_memory.fill_synthetic(rows, seed=21)
    return agent


def test_weighted_loss_and_written_priorities():
    """the fused step's critic loss is mean(w td^2) with the draw's weights, and its rows' priorities are (|td| + eps)^alpha"""
    B = 32
    agent = _agent(B)
    try:
        rm = agent.replay_memory
        for _ in range(3):
            agent.train_step(B, 1)
        from cartpoleplusplus_amd._lib import lib, check, ptr
        rows = np.empty(B, np.int32)
        check(lib.cpp_replay_last_indexes(rm.handle, B, ptr(rows)))
        _a, _dq, _q, td = agent.trainer.last_values(B)
        td = td.reshape(-1)
        w = rm.last_weights(B)
        assert w.max() == 1.0 and w.min() < 1.0
        loss = float(agent.trainer.last_stats()[0])
        want = float(np.mean(w.astype(np.float64) * td.astype(np.float64) ** 2))
        assert abs(loss - want) <= 1e-5 * abs(want), (loss, want)
        last = {int(r): float(v) for r, v in zip(rows, P.priority(td, 0.6, 1e-6))}
        got = rm.priorities(np.array(sorted(last), np.int32))
        ref = np.array([last[k] for k in sorted(last)], np.float32)
        assert np.abs(got / ref - 1).max() < 2e-6
    finally:
        agent.close()


def test_only_the_weight_differs():
    """alpha = 0, beta = 0: every weight is 1 and a prioritized minibatch is cpp_ddpg_train_rows on the same rows, bit for bit"""
    from cartpoleplusplus_amd._lib import lib, check, ptr
    B = 32
    per = _agent(B, priority_alpha=0.0, priority_beta=0.0, priority_beta_final=0.0)
    uni = _agent(B, prioritized_replay=False)
    try:
        per.train_step(B, 1)
        rows = np.empty(B, np.int32)
        check(lib.cpp_replay_last_indexes(per.replay_memory.handle, B, ptr(rows)))
        assert np.array_equal(per.replay_memory.last_weights(B), np.ones(B, np.float32))
        check(lib.cpp_ddpg_train_rows(uni.trainer.handle, uni.replay_memory.handle, B, ptr(rows)))
        for a, b in zip(per.networks()[:2], uni.networks()[:2]):
            assert np.array_equal(a.get_params(), b.get_params()), a.namespace
        assert per.trainer.last_stats()[0] == uni.trainer.last_stats()[0]
    finally:
        per.close()
        uni.close()


def _rows_of_last_minibatch(agent, B):
    from cartpoleplusplus_amd._lib import lib, check, ptr
    rows = np.empty(B, np.int32)
    check(lib.cpp_replay_last_indexes(agent.replay_memory.handle, B, ptr(rows)))
    return rows


@pytest.mark.parametrize("shape,B,pixel,per_step", [(PIX, 32, True, 1), (LOWDIM, 32, False, 5), (PIX, 32, True, 5)],
                         ids=["32x32x18-1-per-step", "lowdim-5-per-step", "32x32x18-5-per-step"])
def test_reference_loop_is_the_fused_step(shape, B, pixel, per_step):
    """ddpg_cartpole.py:331-337 verbatim on a prioritized memory (batch() draws by priority on the device) against agent.train_step
    with the same seed.  With 5 minibatches per step the fused step draws minibatches 2..5 itself, in the launch behind each
    minibatch's heads (counter + 1, after the priorities are in the tree) -- the literal loop draws them with batch() after each
    critic.train: the rows must be the same.  Bit for bit (parameters, tree) wherever the uniform step is bit for bit the literal loop:
    one minibatch per step, and the low-dimensional agent (no sample pass riding in the backward kernels); the pixel agent at 5
    minibatches per step is held to the uniform step's own bar against the literal loop (tests/test_gpu_literal_loop.py: the riding
    sample pass moves last bits) and its rows must still be the literal loop's."""
    def agent():
        a, _ref, _ = make_pair(shape, B, pixel, seed=3, replay_size=240, prioritized_replay=True, priority_alpha=0.6,
                               priority_beta=0.4, priority_eps=1e-6)
        a.replay_memory.fill_synthetic(200, seed=21)
        return a
    lit, fused = agent(), agent()
    exact = per_step == 1 or not pixel
    try:
        steps = 10 if per_step == 1 else 4 if exact else 2      # (the pixel agent at 5 per step: the uniform test's 10 minibatches)
        for step in range(steps):
            for _ in range(per_step):
                batch = lit.replay_memory.batch(B)
                assert batch.weights is not None and batch.weights.max() == 1.0
                lit.actor.train(batch.state_1)
                lit.critic.train(batch)
            lit.target_actor.update_weights()
            lit.target_critic.update_weights()
            fused.train_step(B, per_step)
            assert np.array_equal(_rows_of_last_minibatch(fused, B), batch.idxs), step
            assert np.array_equal(fused.replay_memory.last_weights(B), batch.weights) or not exact, step
            tl, tf = lit.replay_memory.priority_tree(), fused.replay_memory.priority_tree()
            for a, b in zip(lit.networks(), fused.networks()):
                pa, pb = a.get_params(), b.get_params()
                if exact:
                    assert np.array_equal(pa, pb), (step, a.namespace)
                else:
                    assert float(np.abs(pa - pb).max() / np.abs(pb).max()) < 2e-6, (step, a.namespace)
            if exact:
                assert np.array_equal(tl, tf), step
            else:
                assert np.allclose(tl, tf, rtol=1e-4, atol=1e-4), (step, float(np.abs(tl - tf).max()))
        assert lit.trainer.fused_pairs == steps * per_step
    finally:
        lit.close()
        fused.close()


def _per_step_against_f64_oracle(shape, B, rows, pixel=True, replay_store="f16", seed=0, alpha=0.6, beta=0.4, eps=1e-6,
                                 atol=1e-5, grad_rel=2e-5, flip_tol=1e-5, probe=False, capacity=None, **pair_kw):
    """ONE graph-replayed minibatch of the fused step on a prioritized memory (rows drawn by priority, importance weights w) against
    oracle.DDPG(float64) on the same rows and parameters: actions / Q / TD at `atol`, the actor's pre-clip gradients at `grad_rel`
    (unweighted), the critic's at `grad_rel` against the oracle's backward pass of w * td_dev -- the weighted gradient, the critic's
    gradient being linear in TD --, the weighted loss mean(w td^2), and the priorities written: (|td_dev| + eps)^alpha.
    capacity=C > B: the agent is built for C rows; a C-row step and its replay run first, the checked B-row replay behind them and one
    more C-row step behind it are both held to the same bars, and besides to tests/per_np.py: the weights of the rows drawn from the
    tree as it stood (1e-6, tests' bar for last_weights) and the tree behind the step, every inner node left + right bit for bit."""
    agent, _ref, (aspec, cspec) = make_pair(shape, B, pixel, seed=seed, replay_size=rows + 50, replay_store=replay_store, capacity=capacity,
                                           prioritized_replay=True, priority_alpha=alpha, priority_beta=beta, priority_eps=eps, **pair_kw)
    path = None
    try:
        rm = agent.replay_memory
        rm.fill_synthetic(rows, seed=21 + seed)
        C = B if capacity is None else int(capacity)
        for _ in range(2 if C > B else 0):
            agent.train_step(C, 1)                        # eager pass + capture, its replay
        if probe:
            from tests.helpers import ddpg_path
            path = ddpg_path(agent, B, aspec.hidden, cspec.hidden, pixel)
        agent.train_step(B, 1)                            # eager pass + capture
        nets = (agent.actor, agent.critic, agent.target_actor, agent.target_critic)

        def step_and_read(Bx, salt):
            # priorities spread over three decades: the next draw's importance weights are far from 1
            rm.update_priorities(np.arange(rows), np.random.default_rng(seed + salt).lognormal(0.0, 2.0, rows).astype(np.float32))
            d = {"B": Bx, "Pm": [n.get_params() for n in nets], "tree": rm.priority_tree()}
            agent.train_step(Bx, 1)                       # hipGraph replay where this key's graph is held, rows drawn by priority
            idxs = _rows_of_last_minibatch(agent, Bx)
            d["idxs"], d["w"] = idxs, rm.last_weights(Bx)
            d["values"] = agent.trainer.last_values(Bx)
            d["grads"] = (agent.actor.get_grads(), agent.critic.get_grads())
            d["stats"] = agent.trainer.last_stats()
            last = {int(r): i for i, r in enumerate(idxs)}
            keys = np.array(sorted(last), np.int32)
            d["last"], d["keys"], d["written"], d["tree_after"] = last, keys, rm.priorities(keys), rm.priority_tree()
            if pixel:
                d["codes"] = (device_pool_codes(agent.actor, Bx), device_pool_codes(agent.critic, Bx))
                d["relu"] = (device_relu_active(agent.actor, Bx), device_relu_active(agent.critic, Bx))
            s1, s2 = rm.state[rm.state_1_idx[idxs]], rm.state[rm.state_2_idx[idxs]]
            hb = rm.batch(idxs=idxs)
            d["batch"] = (s1, hb.action, hb.reward, hb.terminal_mask, s2)
            return d
        checked = step_and_read(B, 9)
        back = step_and_read(C, 10) if C > B else None
        L, size = P.levels(rm.buffer_size), rm.size()
    finally:
        agent.close()
    for d in (checked, back):
        if d is not None:
            _check_per_step(d, aspec, cspec, pixel, alpha, beta, eps, atol, grad_rel, flip_tol, (L, size) if C > B else None)
    return path


def _check_per_step(d, aspec, cspec, pixel, alpha, beta, eps, atol, grad_rel, flip_tol, tree_shape):
    """what _per_step_against_f64_oracle's step_and_read() brought back from one minibatch"""
    Pm, w, idxs, stats, last, keys, written = d["Pm"], d["w"], d["idxs"], d["stats"], d["last"], d["keys"], d["written"]
    actions, _dq_da, q, td = d["values"]
    g_a, g_c = d["grads"]
    s1, a, r, m, s2 = d["batch"]
    assert w.max() == 1.0 and w.min() < 0.5, (w.min(), w.max())
    if tree_shape is not None:
        L, size = tree_shape
        want_w = P.weights(d["tree"], L, size, idxs, beta)
        assert np.abs(w / want_w - 1).max() < 1e-6, (w, want_w)
        assert np.array_equal(d["tree_after"], P.build(d["tree_after"][1 << L:], L))
    ref = O.DDPG(aspec, cspec, Pm[0], Pm[1], np.float64)
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
    w64 = w.astype(np.float64).reshape(-1, 1)
    loss = float(np.mean(w64 * cg["td"] ** 2))
    assert abs(stats[0] - loss) < atol * max(1.0, loss), (stats[0], loss)
    assert_flat_close(aspec, g_a, ag["grads"], rel=grad_rel, what="actor pre-clip grads vs f64 oracle")
    cw = ref.critic_gradients(t, td_override=w64 * td.astype(np.float64))
    assert_flat_close(cspec, g_c, cw["grads"], rel=grad_rel, what="weighted critic pre-clip grads vs f64 oracle at w * td_dev")
    # (and the weights matter: the unweighted gradient is far from the device's)
    assert float(np.linalg.norm(g_c - cg["grads"]) / np.linalg.norm(cg["grads"])) > 100 * grad_rel
    want = P.priority(td.reshape(-1)[[last[k] for k in keys]], alpha, eps)
    assert np.abs(written / want - 1).max() < 2e-6
    if tree_shape is not None:
        # which leaves the step wrote: the rows of THIS minibatch hold the priorities of its TD (a repeated row its last occurrence's),
        # every other leaf the bits it held in front of the step.  An update that walked the entries of an earlier, larger minibatch
        # (n_up following the capacity) would rewrite rows this minibatch never drew -- and leave the tree as self-consistent as before
        L, _size = tree_shape
        before, after = d["tree"][1 << L:], d["tree_after"][1 << L:]
        others = np.ones(len(after), bool)
        others[keys] = False
        changed = np.nonzero(others & (after != before))[0]
        assert changed.size == 0, "leaves of rows %s changed, the minibatch drew %s" % (changed[:16], keys)
        assert np.abs(after[keys] / want - 1).max() < 2e-6 and np.array_equal(after[keys].astype(np.float32), written)
        assert (after[keys] != before[keys]).any()


def test_prioritized_step_below_the_capacity_against_f64_oracle():
    """(C, B) = (8, 5): n_up (the leaves a step writes are its own rows' and no others), the weights and the weighted loss partials at B
    behind C-row steps, and back"""
    _per_step_against_f64_oracle((16, 16, 3, 1, 2), 5, 300, seed=PARTIAL_PER_SEED, capacity=8)


@pytest.mark.parametrize("shape,store,seed", [((64, 64, 3, 2, 3), "f16", 0), ((64, 64, 3, 2, 3), "u8", 2), ((64, 64, 3, 1, 3), "f16", 1)],
                         ids=["cfg3", "cfg3-u8", "cfg2"])
def test_prioritized_fused_step_against_f64_oracle(shape, store, seed):
    _per_step_against_f64_oracle(shape, 256, 2500, replay_store=store, seed=seed)


def test_prioritized_lowdim_step_against_f64_oracle():
    """the low-dimensional critic has no fused heads: its weighted TD runs in td_weighted_kernel"""
    _per_step_against_f64_oracle(LOWDIM, 64, 2000, pixel=False, seed=4)


def test_three_runs_are_identical():
    B, out = 32, []
    for _ in range(3):
        agent = _agent(B)
        try:
            for _step in range(10):
                agent.train_step(B, 5)
            out.append([n.get_params() for n in agent.networks()] + [agent.replay_memory.priority_tree()])
        finally:
            agent.close()
    L = P.levels(240)
    assert (out[0][-1][1 << L:(1 << L) + 200] != 1.0).any()      # (the priorities moved)
    for run in out[1:]:
        for x, y in zip(out[0], run):
            assert np.array_equal(x, y)


def test_refusals():
    from cartpoleplusplus_amd._lib import lib
    B = 32
    agent = _agent(B)
    try:
        rm, t = agent.replay_memory, agent.trainer
        before = [n.get_params() for n in agent.networks()]
        tree = rm.priority_tree()
        assert lib.cpp_ddpg_dp_train_step(t.handle, rm.handle, None, B, 1, 0, 1, 0) != 0
        assert b"prioritized" in lib.cpp_last_error()
        assert lib.cpp_ddpg_sample_and_compute(t.handle, rm.handle, B, 0) != 0
        for name, args in (("cpp_naf_train_step", (None, rm.handle, B, 1, None, 0)), ("cpp_naf_train_rows", (None, rm.handle, B, None, None)),
                           ("cpp_naf_sample_and_compute", (None, rm.handle, B, 0)),
                           ("cpp_naf_dp_train_step", (None, rm.handle, None, B, 1, 0, 1))):
            assert getattr(lib, name)(*args) != 0, name
            assert b"prioritized" in lib.cpp_last_error(), name
        for x, y in zip(before, agent.networks()):
            assert np.array_equal(x, y.get_params())
        assert np.array_equal(tree, rm.priority_tree())
        with pytest.raises(RuntimeError):
            rm.enable_priorities(-0.5, 1e-6)
        with pytest.raises(RuntimeError):
            rm.enable_priorities(0.6, 0.0)
        rm.enable_priorities(0.0, 0.0)            # (alpha == 0 needs no eps)
    finally:
        agent.close()


def test_cli_prioritized_replay(capsys, monkeypatch):
    from cartpoleplusplus_amd import ddpg_cartpole as D
    seen = {}
    close = D.DeepDeterministicPolicyGradientAgent.close

    def spy(self):
        rm = self.replay_memory
        if rm.handle is not None and rm.prioritized:
            seen["p"] = rm.priorities(np.arange(rm.size()))
        close(self)
    monkeypatch.setattr(D.DeepDeterministicPolicyGradientAgent, "close", spy)
    D.main(["--synthetic-env", "--use-raw-pixels", "--render-width", "16", "--render-height", "16", "--batch-size", "8",
            "--replay-memory-size", "120", "--replay-memory-burn-in", "20", "--max-episode-len", "12", "--max-num-actions", "70",
            "--prioritized-replay", "--priority-beta-steps", "5"])
    out = capsys.readouterr().out
    stats = [json.loads(l.split("\t", 1)[1]) for l in out.splitlines() if l.startswith("STATS")]
    assert len(stats) >= 4 and any(np.isfinite(s["mean_losses"]) for s in stats), out[-400:]
    assert not any(np.isinf(s["mean_losses"]) for s in stats)
    assert "p" in seen and (seen["p"] != 1.0).any() and (seen["p"] > 0).all()
