"""Census of tests/test_gpu_odd_geometry.py's table (no GPU: the table is imported, the dispatchers' instance lists are parsed, the
classes are computed from shapes alone).

What decides the route of an image of H x W pixels and C = 3 x cameras x repeats f16 channels:
  * the parity of H and of W (conv_fwd_k16_dispatch, conv_dw16_dispatch, conv_fwd_rs16_dispatch, the (ky,o)-column dW);
  * the staging chunk of chunk_bytes_for (conv.hip): the largest of 16, 8, 4 bytes that divides the row length R = W * C * 2 and the
    image stride H * R -- the stride is a multiple of the row, so the row decides -- or none;
  * whether H * W * C is a multiple of 8 (the replay's vector statistics and its 16-byte gather; else stats_generic_kernel);
  * which kernel holds an instance for (C, width class, chunk), in the order launch_conv_fwd_multi / launch_conv_dw_multi ask:
    conv1 forward K16_CASE (conv_fwd_k16.hip: even W only), then KYO1_CASE / KYO1_CASE_CHB (conv_fwd_kyo_l1.hip), else conv_impl.h;
    conv1 dW DW16_CASE never (it refuses an odd side), DWKYO_CASE / DWKYO_CASE_CHB (conv_dw_kyo_l1.hip: even H only), else conv_impl.h.
    The profiler cannot tell conv_kyo.h from conv_impl.h, so this file is what keeps a (ky,o) instance that an odd image can reach --
    12 channels at 33 <= W <= 63: 24 W-byte rows are multiples of 8 at every W -- from going without a row.
Not every combination exists.  C is a multiple of 3.  An even W gives R = 4 (W / 2) C: 4-byte rows at least.  An odd W with an odd C gives
R = 2 x odd: no chunk; with an even C, 4 bytes at least.  H * W * C % 8 == 0 means 16 | H * R: always with 16-byte rows, with 8-byte rows
iff H is even, with 4-byte rows iff 4 | H, with no chunk iff 8 | H.  An odd element count therefore has no chunk.  `possible()` below
enumerates (H, W, C) instead of trusting that argument; the test fails for a class without a row."""
import numpy as np

from tests import test_gpu_odd_geometry as T
from tests.test_conv_instance_census import _calls


def chunk_bytes(nbytes_row, nbytes_image):
    for chb in (16, 8, 4):
        if nbytes_row % chb == 0 and nbytes_image % chb == 0:
            return chb
    return 0


def _lists():
    """the instance lists of the three dispatchers an image with an odd side can reach, f16 pixels in: K16 (channels, xt, ipw), KYO1
    (channels, xt, ipw, chunk), DWKYO (channels, ns, chunk)"""
    k16 = set((int(c), int(xt), int(ipw)) for c, xt, ipw, plain in _calls("conv_fwd_k16.hip", "K16_CASE") if plain == "false")
    kyo1 = set((int(c), int(xt), int(ipw), 16) for c, xt, ipw in _calls("conv_fwd_kyo_l1.hip", "KYO1_CASE"))
    kyo1 |= set((int(c), int(xt), int(ipw), int(chb)) for c, xt, ipw, chb in _calls("conv_fwd_kyo_l1.hip", "KYO1_CASE_CHB"))
    dwkyo = set((int(c), int(ns), 16) for c, ns, mode in _calls("conv_dw_kyo_l1.hip", "DWKYO_CASE") if mode == "IN_F16_WHITEN")
    dwkyo |= set((int(c), int(ns), int(chb)) for c, ns, mode, chb in _calls("conv_dw_kyo_l1.hip", "DWKYO_CASE_CHB") if mode == "IN_F16_WHITEN")
    return k16, kyo1, dwkyo


K16_LIST, KYO1_LIST, DWKYO_LIST = _lists()


def kernels(H, W, C):
    """(conv1 forward, conv1 dW) of a minibatch (B >= 2, batch statistics, no batch norm) of H x W x C f16 images, H or W odd, W <= 128"""
    assert (H % 2 == 1 or W % 2 == 1) and 4 <= H and W <= 128
    chb = chunk_bytes(W * C * 2, H * W * C * 2)
    # conv_fwd_k16_dispatch: xt = W > 16 ? 2 : 1, ipw = W > 64 ? 1 : (W > 32 ? 2 : 4); an even W has an even image stride
    if W % 2 == 0 and (C, 2 if W > 16 else 1, 1 if W > 64 else (2 if W > 32 else 4)) in K16_LIST:
        fwd = T.K16
    # conv_fwd_kyo_dispatch_l1: xt = W > 64 ? 2 : 1, ipw = W > 32 ? 1 : (W > 16 ? 2 : 4)
    elif chb and (C, 2 if W > 64 else 1, 1 if W > 32 else (2 if W > 16 else 4), chb) in KYO1_LIST:
        fwd = T.KYO
    else:
        fwd = T.IMPL
    # launch_conv_dw_multi: kyo needs H % 2 == 0 and a chunk; conv_dw_kyo_dispatch: ns = W > 64 ? 32 : (W > 32 ? 16 : 8)
    dw = T.KYO if H % 2 == 0 and chb and (C, 32 if W > 64 else (16 if W > 32 else 8), chb) in DWKYO_LIST else T.IMPL
    return fwd, dw


def klass(shape):
    H, W = shape[0], shape[1]
    C = int(np.prod(shape[2:]))
    return (H % 2, W % 2, chunk_bytes(W * C * 2, H * W * C * 2), (H * W * C) % 8 == 0) + kernels(H, W, C)


def possible():
    """the classes of every H in 8 .. 40 (8: the smallest side with a pool3 output), every W in 8 .. 72 (all four width classes of the
    dispatchers) and every channel count the command line can ask for up to 30, where H or W is odd"""
    out = set()
    for H in range(8, 41):
        for W in range(8, 73):
            if H % 2 == 0 and W % 2 == 0:
                continue
            for C in range(3, 31, 3):
                out.add(klass((H, W, C)))
    return out


def test_the_parser_sees_the_three_lists():
    assert len(K16_LIST) >= 15 and len(KYO1_LIST) >= 13 and len(DWKYO_LIST) >= 8, (K16_LIST, KYO1_LIST, DWKYO_LIST)
    assert (18, 2, 2) in K16_LIST and (12, 1, 1, 8) in KYO1_LIST and (9, 1, 4, 4) in KYO1_LIST and (12, 16, 8) in DWKYO_LIST


def test_the_table_states_the_classes_its_shapes_have():
    for row in T.ROWS:
        H, W = row.shape[:2]
        assert H % 2 == 1 or W % 2 == 1, row
        k = klass(row.shape)
        assert k[2] == row.chunk, (row, k)
        assert k[3] == (row.stats == T.VECTOR), (row, k)
        assert k[4:] == (row.fwd, row.dw), (row, k)                       # the kernel the instance lists give this geometry
        assert row.fwd != T.K16 or W % 2 == 0, row                        # conv_fwd_k16_dispatch refuses an odd W
    assert all(int(np.prod(r.shape)) % 8 == 0 for r in T.ROWS if r.stats == T.VECTOR)


def test_every_class_that_can_exist_has_a_row():
    have = set(klass(r.shape) for r in T.ROWS)
    want = possible()
    # (what the module docstring derives)
    for hp, wp, chunk, vec, fwd, dw in want:
        assert chunk >= 4 or wp == 1, "an even W has 4-byte rows at least"
        assert vec or chunk != 16
        assert not (hp == 1 and vec) or chunk == 16, "an odd H has whole vectors of 8 only with 16-byte rows"
        assert fwd != T.K16 or wp == 0
        assert dw != T.KYO or hp == 0
    assert len(set(k[:4] for k in want)) == 13, sorted(want)
    # an odd W on the (ky,o)-column kernels: forward and dW at an even H, the forward alone at an odd H
    assert (0, 1, 8, True, T.KYO, T.KYO) in want and (1, 1, 8, False, T.KYO, T.IMPL) in want
    missing = sorted(want - have)
    assert not missing, ("no row in tests/test_gpu_odd_geometry.py for (H odd, W odd, row chunk, elements %% 8 == 0, conv1 forward, conv1 dW)"
                         " = %s" % (missing,))
    assert have <= want
    # every row runs at the default precision, the f16-pipe forwards also with exact products, and graph replay alternates with the
    # eager call
    plain = [r for r, exact, _g in T.TABLE if not exact]
    assert plain == T.ROWS
    assert [r for r, exact, _g in T.TABLE if exact] == [r for r in T.ROWS if r.fwd == T.K16]
    graphs = [g for _r, _e, g in T.TABLE]
    assert all(a != b for a, b in zip(graphs, graphs[1:]))
    assert any(r.B % 2 == 1 for r in T.ROWS if r.fwd == T.K16) and any(r.B % 4 in (1, 3) for r in T.ROWS)      # images-per-workgroup remainders


def test_every_row_runs_through_the_f64_oracle_with_a_pool3_output_and_gradients():
    """host_case's parameters and episodes at every row's shape and batch size: the oracle's trunk leaves a non-empty pool3 (VALID pooling
    drops the partial last row and column three times) and both gradient lists are finite and non-zero"""
    from tests.helpers import host_case, oracle_of
    from oracle import ddpg_np as O
    for row in T.ROWS:
        specs, P, _episodes, _idxs, batches = host_case(row.shape, row.B, 1, 5, rows=12)
        ref = oracle_of(specs, P, np.float64, O.DEFAULT_HYPER)
        ag, cg = ref.actor_gradients(batches[0][0]), ref.critic_gradients(batches[0])
        pool3 = cg["cache_critic"]["conv3"][1]
        H, W = row.shape[:2]
        assert pool3.shape[1:3] == (H // 8, W // 8) and pool3.size > 0, (row, pool3.shape)
        for g in (ag["grads"], cg["grads"]):
            assert np.isfinite(g).all() and np.linalg.norm(g) > 0, row
