"""n-step returns, restated row by row in plain Python (include/cartpolepp_abi.h "n-step returns"): the walk along a drawn row's
episode and the f32 fold of its rewards.  Independent of the product's vectorised host function and of the device gather, both of
which the tests hold to it bit for bit.  Test-only: product code never imports it."""
import numpy as np


def walk(i, s1_idx, s2_idx, mask, size, R, n):
    """the rows j_0 = i, j_1, ... the walk visits (1 <= len <= n)"""
    rows = [int(i)]
    for _k in range(n - 1):
        j = rows[-1]
        if mask[j] == 0:
            break
        if j + 1 < size:
            nxt = j + 1
        elif size == R:
            nxt = (j + 1) % R
        else:
            break
        if nxt == i or s2_idx[j] != s1_idx[nxt]:
            break
        rows.append(nxt)
    return rows


def transition(i, s1_idx, s2_idx, reward, mask, size, R, n, discount):
    """(reward, terminal_mask, state_2 slot) of row i's n-step transition: f32, every operation rounded on its own"""
    s1_idx, s2_idx = [int(x) for x in np.ravel(s1_idx)], [int(x) for x in np.ravel(s2_idx)]
    reward, mask = np.ravel(np.asarray(reward, np.float32)), np.ravel(np.asarray(mask, np.float32))
    d = np.float32(discount)
    rows = walk(i, s1_idx, s2_idx, mask, size, R, n)
    g, ret = np.float32(1.0), np.float32(reward[rows[0]])
    for j in rows[1:]:
        g = np.float32(g * d)
        ret = np.float32(ret + np.float32(reward[j] * g))
    last = rows[-1]
    return ret, np.float32(mask[last] * g), s2_idx[last]


def columns(idxs, s1_idx, s2_idx, reward, mask, size, R, n, discount):
    """the three gathered columns of a draw: (B, 1) reward, (B, 1) terminal_mask, (B,) state_2 slots"""
    out = [transition(i, s1_idx, s2_idx, reward, mask, size, R, n, discount) for i in np.ravel(idxs)]
    r = np.array([o[0] for o in out], np.float32).reshape(-1, 1)
    m = np.array([o[1] for o in out], np.float32).reshape(-1, 1)
    return r, m, np.array([o[2] for o in out], np.int32)


def episodes_table(lengths, R, slots_factor=1.5, rng=None):
    """the event columns a ReplayMemory(R) holds after add_episode() of episodes of the given lengths (its FIFO slot bookkeeping,
    replay_memory.py:63-118): (s1_idx, s2_idx, reward, mask, size).  Rewards are drawn from rng (N(0, 1) f32), or 1."""
    import collections
    S = int(R * slots_factor)
    free = collections.deque(range(S))
    s1, s2 = np.zeros(R, np.int32), np.zeros(R, np.int32)
    rew, msk = np.zeros(R, np.float32), np.zeros(R, np.float32)
    insert, full = 0, False
    for L in lengths:
        slot = free.popleft()
        for k in range(L):
            row = insert
            if full:
                free.append(int(s1[row]))
                if msk[row] == 0:
                    free.append(int(s2[row]))
            s1[row] = slot
            rew[row] = np.float32(rng.normal()) if rng is not None else np.float32(1.0)
            msk[row] = 0.0 if k == L - 1 else 1.0
            slot = free.popleft()
            s2[row] = slot
            insert += 1
            if insert >= R:
                insert, full = 0, True
    return s1, s2, rew, msk, (R if full else insert)
