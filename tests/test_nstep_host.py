"""n-step returns on the host: the product's vectorised fold (replay_memory.n_step_columns, what batch() hands the literal loop) held
bit for bit to the row-by-row restatement tests/nstep_np.py, on hand-built and random tables; batch() on the n-step columns; and the
argument refusals of ReplayMemory.enable_n_step."""
import collections
import weakref

import numpy as np
import pytest

from cartpoleplusplus_amd import replay_memory as RM
from tests import nstep_np as NS


def _same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    assert a.shape == b.shape and a.dtype == b.dtype, (a.shape, b.shape, a.dtype, b.dtype)
    assert np.array_equal(a.view(np.uint32) if a.dtype == np.float32 else a, b.view(np.uint32) if b.dtype == np.float32 else b)


def _check(idxs, s1, s2, r, m, size, R, n, d):
    got = RM.n_step_columns(idxs, s1, s2, r.reshape(-1, 1), m.reshape(-1, 1), size, R, n, d)
    want = NS.columns(idxs, s1, s2, r, m, size, R, n, d)
    for g, w in zip(got, want):
        _same(g, w)
    return got


def _chain(R, ends, size=None):
    """rows 0..R-1 as consecutive transitions of one slot chain; the rows in `ends` are episode ends (mask 0, the next row starts a
    new episode with a fresh slot)"""
    s1, s2 = np.zeros(R, np.int32), np.zeros(R, np.int32)
    slot = 0
    for i in range(R):
        s1[i] = slot
        slot += 1
        s2[i] = slot
        if i in ends:
            slot += 1
    r = (np.arange(R, dtype=np.float32) + np.float32(1)) * np.float32(0.5)
    m = np.array([0.0 if i in ends else 1.0 for i in range(R)], np.float32)
    return s1, s2, r, m, R if size is None else size


def test_episode_end_stops_the_walk():
    s1, s2, r, m, size = _chain(10, {3, 7})
    rew, msk, s2g = _check(np.arange(10), s1, s2, r, m, size, 10, 3, 0.9)
    d = np.float32(0.9)
    # row 2: rows 2, 3 (end) -> r2 + r3 d, mask 0, s2 of row 3
    assert rew[2, 0] == np.float32(r[2] + np.float32(r[3] * d)) and msk[2, 0] == 0.0 and s2g[2] == s2[3]
    # row 3 is an episode end itself: its own row only
    assert rew[3, 0] == r[3] and msk[3, 0] == 0.0 and s2g[3] == s2[3]
    # row 4: three rows inside the episode; the mask carries discount^2
    g2 = np.float32(d * d)
    assert msk[4, 0] == g2 and s2g[4] == s2[6]


def test_slot_mismatch_stops_the_walk():
    s1, s2, r, m, size = _chain(8, set())
    s1[5] = 99                                     # row 4's s2 is not row 5's s1 (a row written by another episode)
    rew, msk, s2g = _check(np.arange(8), s1, s2, r, m, size, 8, 4, 0.5)
    assert s2g[3] == s2[4] and msk[3, 0] == np.float32(0.5) and rew[3, 0] == np.float32(r[3] + np.float32(r[4] * np.float32(0.5)))


def test_memory_that_is_not_full_does_not_wrap():
    s1, s2, r, m, _ = _chain(16, set())
    size = 9                                       # rows >= 9 are not in the memory yet
    rew, msk, s2g = _check(np.arange(size), s1, s2, r, m, size, 16, 5, 0.75)
    assert s2g[8] == s2[8] and rew[8, 0] == r[8] and msk[8, 0] == 1.0
    assert s2g[6] == s2[8]


def test_wrap_at_the_write_head():
    """a full memory: the walk continues from row R-1 to row 0 where the episode goes on, and stops at the write head"""
    R = 12
    s1, s2, r, m, _ = _chain(R, set())
    # rows 9, 10, 11, 0, 1 are one episode written across the end of the buffer; row 2 is the oldest row (the write head is at 2)
    s1[0], s2[0] = s2[11], s2[11] + 1
    s1[1], s2[1] = s2[0], s2[0] + 1
    s1[2] = 500                                    # the oldest row's s1: a live slot, never the newest row's s2
    rew, msk, s2g = _check(np.arange(R), s1, s2, r, m, R, R, 4, 0.9)
    assert s2g[10] == s2[1] and s2g[11] == s2[1] and s2g[1] == s2[1]
    _check(np.arange(R), s1, s2, r, m, R, R, 64, 0.9)
    # a circular chain (every row continues into the next): the walk stops before it comes back to the drawn row
    s1c = np.arange(R, dtype=np.int32)
    s2c = np.roll(s1c, -1).astype(np.int32)
    _, mc, s2gc = _check(np.arange(R), s1c, s2c, r, np.ones(R, np.float32), R, R, 64, 1.0)
    assert (s2gc == s2c[(np.arange(R) + R - 1) % R]).all() and (mc == 1.0).all()


def test_n_larger_than_the_episode():
    s1, s2, r, m, size = _chain(6, {2, 5})
    rew, msk, s2g = _check(np.arange(6), s1, s2, r, m, size, 6, 64, 0.99)
    assert s2g[0] == s2[2] and msk[0, 0] == 0.0 and s2g[3] == s2[5]


def test_n_one_is_the_stored_columns():
    rng = np.random.default_rng(0)
    s1, s2, r, m, size = NS.episodes_table(rng.integers(1, 13, 60), 100, rng=rng)
    idxs = rng.integers(0, size, 256)
    rew, msk, s2g = _check(idxs, s1, s2, r, m, size, 100, 1, 0.3)
    _same(rew, r[idxs].reshape(-1, 1))
    _same(msk, m[idxs].reshape(-1, 1))
    _same(s2g, s2[idxs])


@pytest.mark.parametrize("n", [2, 3, 5, 64])
def test_random_episode_tables(n):
    rng = np.random.default_rng(n)
    for trial in range(6):
        R = int(rng.integers(5, 200))
        lengths = rng.integers(1, 13, int(rng.integers(1, 3 * R)))
        s1, s2, r, m, size = NS.episodes_table(lengths, R, rng=rng)
        d = float(np.float32(rng.uniform(0.0, 1.0)))
        _check(rng.integers(0, size, 300), s1, s2, r, m, size, R, n, d)


def test_random_columns():
    """arbitrary columns (slots, masks and rewards of any value, as cpp_replay_write_rows may leave them)"""
    rng = np.random.default_rng(7)
    for trial in range(20):
        R = int(rng.integers(1, 80))
        size = R if trial % 2 else int(rng.integers(1, R + 1))
        s1 = rng.integers(0, 6, R).astype(np.int32)
        s2 = rng.integers(0, 6, R).astype(np.int32)
        m = rng.choice(np.array([0.0, 1.0, 0.5, -0.0], np.float32), R)
        r = rng.normal(size=R).astype(np.float32) * np.float32(1e3)
        _check(rng.integers(0, size, 200), s1, s2, r, m, size, R, int(rng.integers(1, 65)), float(rng.uniform(0, 2)))


def _host_memory(s1, s2, r, m, size, R):
    """a ReplayMemory's host side only (mirrors and bookkeeping, no device memory): batch() of it needs no GPU"""
    rm = RM.ReplayMemory.__new__(RM.ReplayMemory)
    rm.buffer_size, rm.state_shape, rm.action_dim = R, (3,), 2
    rm.state_1_idx, rm.state_2_idx = s1, s2
    rm.reward, rm.terminal_mask = r.reshape(-1, 1), m.reshape(-1, 1)
    rm.action = np.arange(2 * R, dtype=np.float32).reshape(R, 2)
    rm.insert, rm.full = (0, True) if size == R else (size, False)
    rm.stats, rm.prioritized, rm._write_gen, rm._drawn = collections.Counter(), False, 0, weakref.WeakSet()
    rm.n_step, rm.n_step_discount = 1, 0.0
    return rm


def test_batch_carries_the_n_step_columns():
    rng = np.random.default_rng(3)
    R = 90
    s1, s2, r, m, size = NS.episodes_table(rng.integers(1, 13, 40), R, rng=rng)
    rm = _host_memory(s1, s2, r, m, size, R)
    idxs = rng.integers(0, size, 64)
    one = rm.batch(idxs=idxs)
    _same(one.reward, r[idxs].reshape(-1, 1))
    _same(one.state_2_idx, s2[idxs])
    rm.n_step, rm.n_step_discount = 3, float(np.float32(0.95))     # (what enable_n_step(3, 0.95) leaves on the host)
    b = rm.batch(idxs=idxs)
    want = NS.columns(idxs, s1, s2, r, m, size, R, 3, 0.95)
    _same(b.reward, want[0])
    _same(b.terminal_mask, want[1])
    _same(b.state_2_idx, want[2])
    _same(b.state_1_idx, s1[idxs])
    _same(b.action, rm.action[idxs])
    assert not np.array_equal(b.reward, one.reward)


@pytest.mark.parametrize("n, d", [(0, 0.9), (65, 0.9), (-1, 0.9), (3, -0.5), (3, float("nan")), (3, float("inf"))])
def test_enable_n_step_refuses_bad_arguments(n, d):
    rm = RM.ReplayMemory.__new__(RM.ReplayMemory)
    rm.handle, rm.n_step, rm.n_step_discount = None, 1, 0.0
    with pytest.raises(ValueError):
        rm.enable_n_step(n, d)
    assert rm.n_step == 1
