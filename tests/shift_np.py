"""numpy restatement of the random shift of the device gather (include/cartpolepp_abi.h "Random shift"; csrc/gather_body.h):
the Philox draw of every image's (dy, dx) and the clamp rule out[y, x, c] = in[clamp(y + dy), clamp(x + dx), c]."""
import numpy as np

from tests.helpers import philox4x32_10_np


def shifts(seed, counter, B, pad):
    """(2, B, 2) int32 [which][b][dy, dx]: r = philox4x32_10({b, 2 + which, n_lo, n_hi}, {seed_lo, seed_hi}),
    dy = ((r.x * (2 pad + 1)) >> 32) - pad, dx the same from r.y"""
    seed, counter, B, pad = int(seed), int(counter), int(B), int(pad)
    b = np.arange(B, dtype=np.uint64)
    span = np.uint64(2 * pad + 1)
    out = np.empty((2, B, 2), np.int32)
    for which in (0, 1):
        r = philox4x32_10_np(b, np.full(B, 2 + which, np.uint64), np.full(B, counter & 0xFFFFFFFF, np.uint64),
                             np.full(B, counter >> 32, np.uint64), seed & 0xFFFFFFFF, seed >> 32)
        out[which, :, 0] = ((r[0] * span) >> np.uint64(32)).astype(np.int64) - pad
        out[which, :, 1] = ((r[1] * span) >> np.uint64(32)).astype(np.int64) - pad
    return out


def shift_images(x, sh):
    """x: (B, H, W, ...) images, sh: (B, 2) [dy, dx] -> the shifted images (same shape and dtype)"""
    x, sh = np.asarray(x), np.asarray(sh)
    B, H, W = x.shape[:3]
    out = np.empty_like(x)
    for b in range(B):
        ys = np.clip(np.arange(H) + int(sh[b, 0]), 0, H - 1)
        xs = np.clip(np.arange(W) + int(sh[b, 1]), 0, W - 1)
        out[b] = x[b][ys][:, xs]
    return out
