"""numpy restatement of the device's prioritized replay (csrc/per.hip; semantics in include/cartpolepp_abi.h): the sum tree, the
duplicate rule, the stratified draw with its top-end guard and the importance weights."""
import numpy as np

from tests.helpers import philox4x32_10_np


def levels(buffer_size):
    """L with 2^L >= buffer_size (leaves at [2^L, 2^(L+1)))"""
    return max(0, int(buffer_size - 1).bit_length())


def priority(abs_td, alpha, eps):
    """p = powf(|td| + eps, alpha) in f32; alpha == 1: |td| + eps; alpha == 0: 1"""
    x = np.abs(np.asarray(abs_td, np.float32)) + np.float32(eps)
    if alpha == 0:
        return np.ones_like(x)
    if alpha == 1:
        return x
    return np.power(x, np.float32(alpha), dtype=np.float32)


def build(leaves, L):
    """the whole tree from its leaves (f64): every inner node is left + right"""
    t = np.zeros(2 << L, np.float64)
    t[1 << L:(1 << L) + len(leaves)] = leaves
    for k in range(L - 1, -1, -1):
        lo = 1 << k
        t[lo:2 * lo] = t[2 * lo:4 * lo:2] + t[2 * lo + 1:4 * lo:2]
    return t


def write(tree, L, rows, p):
    """leaf writes in list order (a duplicate row keeps its LAST value) and the sums above them"""
    for i, v in zip(rows, p):
        tree[(1 << L) + int(i)] = np.float64(np.float32(v))
    for i in set(int(r) for r in rows):
        node = ((1 << L) + i) >> 1
        while node >= 1:
            tree[node] = tree[2 * node] + tree[2 * node + 1]
            node >>= 1
    return tree


def draw(tree, L, size, B, seed, counter):
    """the stratified draw: rows and whether each one went through the top-end guard"""
    b = np.arange(B, dtype=np.uint64)
    c = np.uint64(counter)
    r = philox4x32_10_np(b, np.ones_like(b), np.full_like(b, int(c) & 0xFFFFFFFF), np.full_like(b, int(c) >> 32),
                         seed & 0xFFFFFFFF, seed >> 32)
    U = ((r[0] << np.uint64(32) | r[1]) >> np.uint64(11)).astype(np.float64) * 2.0 ** -53
    total = tree[1]
    rows, guarded = np.empty(B, np.int64), np.zeros(B, bool)
    for k in range(B):
        u = (float(k) + U[k]) * (total / float(B))
        node = 1
        for _ in range(L):
            left = tree[2 * node]
            if u < left:
                node = 2 * node
            else:
                u -= left
                node = 2 * node + 1
        row = node - (1 << L)
        if row >= size:
            row, guarded[k] = size - 1, True
        rows[k] = row
    return rows, guarded


def weights(tree, L, size, rows, beta):
    """w = (size * leaf / total)^-beta in f64, over the batch maximum, as f32"""
    leaf = tree[(1 << L) + np.asarray(rows, np.int64)]
    w = np.power(float(size) * leaf / tree[1], -float(beta))
    return (w / w.max()).astype(np.float32)
