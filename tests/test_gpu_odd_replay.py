"""The device replay memory at states whose element count is no multiple of 8: 15 x 15 x 3 (675 elements: store rows 2-byte aligned),
9 x 9 x 9 (729: 2 bytes), 13 x 11 x 6 (858: 4 bytes), 9 x 68 x 9 (5508: 8 bytes).  replay_gather_args and cpp_replay_set_stats_channels
then set C = 0: the gather takes gather_stats_body's copy-only branch -- Vec8 loads and stores of 16 bytes at addresses that are only
element aligned, then the tail loop nvec * 8 .. elems -- for the store rows AND for the gathered copy (row b starts at b * elems), and
the minibatch's whitening tables come from stats_generic_kernel through batch_ensure_stats.  Every other pixel memory of the suite has
elems % 8 == 0.

Bit for bit against oracle/replay_np.py and the store's own rows (caller's rows and Philox draws, a one-step and an n = 3 memory); the
tables the sample pass leaves, through conv1's pooled output, Q and TD on that very device batch, against float64 moments of the same pixels;
and the random shift's refusal, which names the element count."""
import ctypes

import numpy as np
import pytest

from oracle.replay_np import OracleReplayMemory
from tests.test_gpu_nstep_replay import _download, _same, _want

pytestmark = pytest.mark.gpu

SHAPES = [(15, 15, 3, 1, 1), (9, 9, 3, 1, 3), (13, 11, 3, 1, 2), (9, 68, 3, 1, 3)]
IDS = ["15x15x3-675", "9x9x9-729", "13x11x6-858", "9x68x9-5508"]
ROWS, SLOTS = 40, 60


def _episodes(shape, seed=4):
    """test_gather_and_statistics_match_oracle_bitwise's stream: 14 episodes of 1 .. 7 steps, f32 frames cast to f16 on store; the 40
    rows wrap, and with this seed the first and the last state slot are both in use at the end"""
    from cartpoleplusplus_amd.replay_memory import ReplayMemory
    rng = np.random.default_rng(seed)
    rm, orm = ReplayMemory(ROWS, shape, 2), OracleReplayMemory(ROWS, shape, 2)
    for _ in range(14):
        n = int(rng.integers(1, 8))
        mk = lambda: rng.uniform(0, 1, shape).astype(np.float32)
        s0, seq = mk(), [(rng.uniform(-1, 1, (1, 2)), float(rng.integers(0, 9)), mk()) for _ in range(n)]
        rm.add_episode(s0, seq); orm.add_episode(s0, seq)
    return rm, orm, rng


def _edge_rows(rm):
    """rows whose state_1 / state_2 lie in the first slot, in the last slot (the last row of the store), in odd and in even slots, the
    first and the last row of the memory, each twice over and out of order"""
    s1, s2 = rm.state_1_idx, rm.state_2_idx
    pick = [0, ROWS - 1]
    for slot in (0, SLOTS - 1):
        hit = np.flatnonzero((s1 == slot) | (s2 == slot))
        assert len(hit), "slot %d is not in use: choose another seed" % slot
        pick += [int(hit[0]), int(hit[-1])]
    pick += [int(np.flatnonzero(s1 % 2 == 1)[0]), int(np.flatnonzero(s1 % 2 == 0)[0]), int(np.flatnonzero(s2 % 2 == 1)[-1]), int(np.flatnonzero(s2 % 2 == 0)[-1])]
    return np.array(pick + pick[::-1] + [7, 7, 8], np.int32)


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_gather_matches_the_oracle_memory_bit_for_bit(shape):
    assert int(np.prod(shape)) % 8 != 0
    rm, orm, rng = _episodes(shape)
    try:
        assert rm.full and np.array_equal(rm.state_1_idx, orm.state_1_idx) and np.array_equal(rm.state_2_idx, orm.state_2_idx)
        assert list(rm.state_free_slots) == list(orm.state_free_slots) and rm.state_buffer_size == SLOTS
        for idxs in (_edge_rows(rm), rng.integers(0, ROWS, 33).astype(np.int32), np.arange(ROWS, dtype=np.int32)):
            B = len(idxs)
            want = orm.batch(idxs=idxs)
            # the draw read where it lies (cpp_replay_read_states) ...
            got = rm.batch(idxs=idxs)
            for g, w in zip(got, want):
                g = np.asarray(g)
                assert g.dtype == w.dtype, (g.dtype, w.dtype)
                _same(g, w, "batch(idxs) B=%d" % B)
            assert np.array_equal(got.state_1_idx, orm.state_1_idx[idxs])
            # ... and gathered by the device into a minibatch (cpp_replay_sample on the caller's rows: the copy-only branch)
            b = rm.batch(idxs=idxs)
            b.device
            s1, s2, a, r, m = _download(rm, B)
            for g, w, what in zip((s1, a, r, m, s2), want, ("state_1", "action", "reward", "terminal_mask", "state_2")):
                assert g.dtype == w.dtype, (what, g.dtype, w.dtype)
                _same(g, w, "gathered %s B=%d" % (what, B))
            _same(np.asarray(b.state_1), want.state_1, "state_1 column of the gathered draw")
        # the device's own Philox draw: the rows it reports, and their states from the store
        for B, counter in ((5, 0), (33, 1), (64, 2)):
            b = rm.sample_on_device(B, seed=9, counter=counter)
            idxs = b.idxs
            assert idxs.dtype == np.int32 and idxs.min() >= 0 and idxs.max() < ROWS and len(np.unique(idxs)) > 1
            s1, s2, a, r, m = _download(rm, B)
            _same(s1, rm.state[rm.state_1_idx[idxs]], "sampled state_1")
            _same(s2, rm.state[rm.state_2_idx[idxs]], "sampled state_2")
            want = orm.batch(idxs=idxs)
            for g, w, what in zip((s1, a, r, m, s2), want, ("state_1", "action", "reward", "terminal_mask", "state_2")):
                assert g.dtype == w.dtype, (what, g.dtype, w.dtype)
                _same(g, w, "sampled %s B=%d" % (what, B))
            _same(np.asarray(b.state_2), want.state_2, "state_2 column of the sampled draw")
    finally:
        rm.close()


def test_n_step_gather_at_675_elements_matches_numpy_bit_for_bit():
    """the n = 3 walk (gather_body.h nstep_walk) in front of the copy-only branch: reward, mask and the state in the slot the walk ends
    on against tests/nstep_np.py, the host's columns of the same draw against the device's"""
    shape = SHAPES[0]
    rm, _orm, rng = _episodes(shape)
    try:
        rm.enable_n_step(3, 0.97)
        walked = 0
        for draw in ("edges", "rows", "philox"):
            if draw == "philox":
                b = rm.sample_on_device(33, seed=5, counter=3)
            else:
                b = rm.batch(idxs=_edge_rows(rm) if draw == "edges" else rng.integers(0, ROWS, 33).astype(np.int32))
                b.device
            idxs, B = b.idxs, len(b.idxs)
            r, m, s2_idx = _want(rm, idxs)
            s1g, s2g, ag, rg, mg = _download(rm, B)
            _same(rg, r, "reward %s" % draw)
            _same(mg, m, "mask %s" % draw)
            _same(s2g, rm.state[s2_idx], "state_2 %s" % draw)
            _same(s1g, rm.state[rm.state_1_idx[idxs]], "state_1 %s" % draw)
            _same(ag, rm.action[idxs], "action %s" % draw)
            _same(b.reward, rg, "host reward")
            _same(b.terminal_mask, mg, "host mask")
            _same(b.state_2_idx, s2_idx, "host state_2 slots")
            walked += int((s2_idx != rm.state_2_idx[idxs]).sum())
        assert walked > 0
    finally:
        rm.close()


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_sampled_minibatch_carries_the_f64_whitening_tables(shape):
    """cpp_replay_sample on such a memory leaves the minibatch's two whitening tables -- state_1's for the live networks, state_2's for
    the targets -- to stats_generic_kernel (replay_sample_finish -> batch_ensure_stats -> batch_stats' else arm).  No call returns the
    tables; cpp_ddpg_check_loss on that very device batch reads both.  Nearest to the tables is conv1's pooled output, one whitened 5 x 5
    window away from them: the critic's pool1 (state_1's table) and the target critic's (state_2's) against the float64 oracle's conv1
    under float64 numpy moments of the same f16 pixels, at the 1e-5 that
    tests/test_gpu_fullsize.py::test_full_size_whitening_statistics_and_forward_against_f64_oracle_slice holds the vector path's tables
    to through the same quantity (stats_generic_kernel accumulates in f64 like the vector path); then Q, TD and the loss at 1e-5.  The
    checks have power over the tables: with one image's statistics in place of the batch's the oracle's own pool1 and Q move by more
    than a hundred times the bar."""
    from oracle import ddpg_np as O
    from tests.helpers import _profiled_calls, make_pair
    B, rows = 5, 40
    agent, ref, _specs = make_pair(shape, B, True, seed=13, replay_size=rows + 20)
    try:
        rm = agent.replay_memory
        rm.fill_synthetic(rows, seed=31)
        held = {}
        calls = _profiled_calls(agent.actor.ctx, lambda: held.update(b=rm.sample_on_device(B, seed=3, counter=1)))
        b = held["b"]
        assert calls.get("stats_generic", 0) == 2, calls                    # one launch per state column, none from the vector path
        assert calls.get("stats_finalize", 0) == 0, calls
        idxs = b.idxs
        s1, s2 = rm.state[rm.state_1_idx[idxs]], rm.state[rm.state_2_idx[idxs]]
        loss, td, q = agent.critic.check_loss(b)                            # b.device: the buffer the sample pass filled, tables included
        t = (s1, rm.action[idxs], rm.reward[idxs], rm.terminal_mask[idxs], s2)
        w_loss, w_td, w_q = ref.check_loss(t)
        print("TABLES %s: |q - f64| %.2e  |td - f64| %.2e  (|q| <= %.2f)" % (shape, np.abs(q - w_q).max(), np.abs(td - w_td).max(), np.abs(w_q).max()))
        assert np.abs(q - w_q).max() < 1e-5 and np.abs(td - w_td).max() < 1e-5
        assert abs(loss - w_loss) < 1e-5 * max(1.0, abs(w_loss))
        sp = ref.critic.spec
        act = np.asarray(t[1], np.float64)
        want_1 = ref.critic.forward(s1, action=act, white=O.whiten_stats(np.asarray(s1).reshape(B, sp.H, sp.W, sp.C), np.float64), training=False)
        want_2 = ref.target_critic.forward(s2, action=act, white=O.whiten_stats(np.asarray(s2).reshape(B, sp.H, sp.W, sp.C), np.float64), training=False)
        pool_1, pool_2 = agent.critic.pool1.eval(B), agent.target_critic.pool1.eval(B)      # (conv1 does not see the action)
        err_1 = np.abs(pool_1.reshape(want_1["conv1"][1].shape) - want_1["conv1"][1]).max()
        err_2 = np.abs(pool_2.reshape(want_2["conv1"][1].shape) - want_2["conv1"][1]).max()
        print("TABLES %s: |pool1 - f64| %.2e (state_1) %.2e (state_2)  (|pool1| <= %.2f)" % (shape, err_1, err_2, np.abs(want_1["conv1"][1]).max()))
        assert pool_1.size > 0 and err_1 < 1e-5 and err_2 < 1e-5
        one = O.whiten_stats(np.asarray(s1[:1]).reshape(1, sp.H, sp.W, sp.C), np.float64)
        f_one = ref.critic.forward(s1, action=act, white=one, training=False)
        assert np.abs(f_one["out"] - w_q).max() > 1e-3 and np.abs(f_one["conv1"][1] - want_1["conv1"][1]).max() > 1e-3
    finally:
        agent.close()


def test_random_shift_is_refused_at_675_elements_before_anything_trains():
    """a 15 x 15 x 3 memory: cpp_replay_set_stats_channels turned the vector path off (675 % 8 = 3) and the shifted gather moves whole
    vectors of 8 elements.  ReplayMemory.enable_random_shift raises, the message names the element count and the multiple-of-8 rule,
    nothing is written or launched, the agent trains unshifted, and the context serves a default agent afterwards."""
    from cartpoleplusplus_amd import _lib
    from tests.helpers import make_pair
    lib, check = _lib.lib, _lib.check
    shape = SHAPES[0]
    agent, _ref, _specs = make_pair(shape, 4, True, seed=2, replay_size=60)
    ctx = agent.actor.ctx
    try:
        rm = agent.replay_memory
        rm.fill_synthetic(40, seed=1)
        before = [n.get_params() for n in agent.networks()]
        ctx.sync()
        ctx.prof_reset()
        ctx.prof_enable(True)
        try:
            with pytest.raises(RuntimeError, match=r"675 elements.*multiple of 8"):
                rm.enable_random_shift(2, seed=5)
            assert lib.cpp_replay_set_random_shift(rm.handle, 15, 15, 2, 5) == 1
            msg = lib.cpp_last_error()
            assert b"675" in msg and b"multiple of 8" in msg and b"not a pixel memory" not in msg, msg
            ctx.sync()
        finally:
            ctx.prof_enable(False)
        launched = {k: v for k, v in ctx.prof_read().items() if v[1] > 0}
        assert not launched, launched
        ctx.prof_reset()
        p, s, n = ctypes.c_int(-1), ctypes.c_uint64(99), ctypes.c_uint64(99)
        check(lib.cpp_replay_get_random_shift(rm.handle, ctypes.byref(p), ctypes.byref(s), ctypes.byref(n)))
        assert (p.value, s.value, n.value) == (0, 0, 0) and rm.random_shift == (0, 0)
        for x, y in zip(before, (n_.get_params() for n_ in agent.networks())):
            assert np.array_equal(x, y)
        agent.train_step(4, 2)
        assert rm.shift_counter() == 0
        assert np.isfinite(agent.critic.get_params()).all() and not np.array_equal(before[1], agent.critic.get_params())
    finally:
        agent.close()
    default, _ref, _specs = make_pair((16, 16, 3, 1, 2), 4, True)
    try:
        default.replay_memory.fill_synthetic(40, seed=1)
        default.train_step(4, 2)
        default.actor.ctx.sync()
        assert np.isfinite(default.actor.get_params()).all() and np.isfinite(default.critic.get_params()).all()
    finally:
        default.close()
