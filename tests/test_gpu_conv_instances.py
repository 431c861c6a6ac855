"""Every instance of conv1's two hand-written tables -- conv_fwd_k16.hip's K16_CASE list (channels x columns per tile x images per
workgroup) and conv_dw16.hip's DW16_CASE list (channels x chunks per row) -- and every geometry next to them that falls back to the
f32-input kernels, through the fused step against oracle.DDPG(float64) at the suite's bars.  Each row first profiles one eager
minibatch (tests/helpers.py conv_routes) and asserts WHICH route ran conv1's forward and conv1's dW: a cell that silently fell back to
the f32 kernels would stay parity-green, the fallback being exact.

The dispatchers key on the width class of the image: W <= 16 (one column per tile, four images per workgroup, one chunk per row),
18..32 (two columns, four images, one chunk), 34..64 (two columns, two images, two chunks), 66..128 (two columns, one image, four
chunks).  The two tables do not hold the same cells: 3 channels at 18..32 wide run the forward on the f32 kernel and dW on conv_dw16.h,
9 channels at 66..128 wide run the forward on conv_k16.h (which leaves bf16 planes for conv2) and dW on the f32 kernel -- the two
MIXED cells.  tests/test_conv_instance_census.py (CPU) parses the two lists and fails when one of their instances has no row here.

Shapes: 8 rows (conv_dw16.h needs an even H >= 4) by the narrowest width of the class above 16: 16, 24, 40, 68.  64-wide images run on
conv_rs16.h / conv_dw16_rs.h and have files of their own (test_gpu_conv1_rs16_channels.py, test_gpu_backward_rs.py)."""
import collections

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

F16, F32 = "f16", "f32"
WIDTH_CLASSES = ("<=16", "18..32", "34..64", "66..128")
CLASS_SHAPE = {"<=16": (8, 16), "18..32": (8, 24), "34..64": (8, 40), "66..128": (8, 68)}
CLASS_BATCHES = {"<=16": (2, 5, 7), "18..32": (2, 5, 7), "34..64": (2, 3), "66..128": (2, 3)}      # images per workgroup: 4, 4, 2, 1
CAMERAS_REPEATS = {3: (1, 1), 6: (1, 2), 9: (1, 3), 12: (2, 2), 15: (1, 5), 18: (2, 3), 24: (2, 4), 30: (2, 5)}
# conv1 forward / conv1 dW per width class, as the two instance lists read (Y: the f16 pipes, N: the f32-input kernels)
EXPECTED = collections.OrderedDict([
    (3, ("Y/Y", "N/Y", "Y/Y", "N/N")),
    (6, ("Y/Y", "Y/Y", "Y/Y", "N/N")),
    (9, ("Y/Y", "Y/Y", "Y/Y", "Y/N")),
    (12, ("N/N", "N/N", "Y/Y", "N/N")),
    (18, ("Y/Y", "Y/Y", "Y/Y", "Y/Y")),
    (30, ("N/N", "N/N", "N/N", "Y/Y")),
    (15, ("N/N", "N/N", "N/N", "N/N")),
    (24, ("N/N", "N/N", "N/N", "N/N")),
])
MIXED_CELLS = ((3, "18..32"), (9, "66..128"))

Row = collections.namedtuple("Row", "id channels wclass shape B graph exact fwd dw also")


def _shape(channels, H, W):
    cams, reps = CAMERAS_REPEATS[channels]
    return (H, W, 3, cams, reps)


def _table():
    rows, turn = [], collections.Counter()

    def add(tag, channels, wclass, hw, B, exact, fwd, dw, also=None):
        rows.append(Row("%s%dch-%dx%d-B%d-%s%s%s" % (tag, channels, hw[0], hw[1], B, fwd, dw, "-exact" if exact else ""), channels, wclass,
                        _shape(channels, *hw), B, len(rows) % 2 == 0, exact, fwd, dw, also or {}))

    def next_b(wclass):
        bs = CLASS_BATCHES[wclass]
        turn[wclass] += 1
        return bs[(turn[wclass] - 1) % len(bs)]

    route = {"Y": F16, "N": F32}
    for exact in (False, True):
        for channels, per_class in EXPECTED.items():
            for wclass, cell in zip(WIDTH_CLASSES, per_class):
                fwd, dw = route[cell[0]], route[cell[2]]
                if exact and not (cell == "Y/Y" or (channels, wclass) in MIXED_CELLS):
                    continue
                add("", channels, wclass, CLASS_SHAPE[wclass], next_b(wclass), exact, fwd, dw)
    # B = 1: the FORWARD stays on the f32 kernel whatever the tables hold (conv.hip: action_given is bit-identical to a row of
    # forward_each; conv1_f16_pipes_ok says no at B < 2, so the minibatch is a gathered copy).  The table reading "B = 1 runs conv1 on the
    # f32 route" holds for the forward only: launch_conv_dw_multi has no batch-size rule and conv_dw16.h takes the dW of one image as it
    # takes any other (observed: conv1_fwd + conv1_dw_f16) -- the dispatcher is as designed, the expectation here follows it
    add("one-image-", 18, "34..64", (8, 40), 1, False, F32, F16)
    # one image per workgroup / four chunks per row at even heights far below cfg5's 128.  32 x 128: conv2 is 16 x 64 and conv3 8 x 32 --
    # neither is a geometry of the pair launches (conv2_bwd_pair.hip: 32-wide conv2 rows; conv3_bwd_pair.hip: 16-wide conv3 rows), so dX
    # and dW of both layers leave on their own
    add("short-", 30, "66..128", (16, 128), 3, False, F16, F16)
    add("short-", 18, "66..128", (32, 128), 3, False, F16, F16, {"conv2_bwd": "conv2_dx+conv2_dw", "conv3_bwd": "conv3_dx+conv3_dw"})
    return rows


TABLE = _table()
FWD_FAMILY = {F16: ("conv1_fwd_f16",), F32: ("conv1_fwd",)}
DW_FAMILY = {F16: ("conv1_dw_f16", "conv1_dw_gather"), F32: ("conv1_dw",)}


def _reset_precision():
    from cartpoleplusplus_amd import _lib
    if _lib.default_context().precision != "fast":
        _lib.default_context().set_precision("fast")


@pytest.mark.parametrize("row", TABLE, ids=[r.id for r in TABLE])
def test_conv1_instance_takes_its_route_and_holds_the_f64_oracle(row):
    from tests.helpers import fused_step_against_f64_oracle
    kw = {"exact_products": True} if row.exact else {}
    try:
        rep = fused_step_against_f64_oracle(row.shape, row.B, rows=60, graph=row.graph, probe_conv=True, seed=17, **kw)
    finally:
        if row.exact:
            _reset_precision()
    print("ROUTES %s: %s  err_q %.2e grads %.2e / %.2e" % (row.id, rep["conv"], rep["err_q"], rep["rel_actor_grads"], rep["rel_critic_grads"]))
    assert rep["conv"]["conv1_fwd"] in FWD_FAMILY[row.fwd], (row.id, rep["conv"])
    assert rep["conv"]["conv1_dw"] in DW_FAMILY[row.dw], (row.id, rep["conv"])
    for part, want in row.also.items():
        assert rep["conv"][part] == want, (row.id, part, rep["conv"])


# The mixed cells in depth.  (3, 18..32): the smallest shape and the 32 x 32 render with one camera and no repeat.  (9, 66..128): 8 x 66
# pools to 33 columns -- conv12_b16_ok refuses odd widths, no bf16 planes, conv2 runs from f32 -- 8 x 68 pools to 34 and conv2 reads
# conv1's planes, and at 32 x 128 conv2 is 64 wide: conv_dx_rs.h leaves its per-image bound of |dpool1| for a conv_dw16.h that does not
# run there -- the f32 dW kernel must not scale by it.
MIXED_DEPTH = [
    pytest.param(3, (8, 24), 5, F32, F16, id="3ch-8x24"),
    pytest.param(3, (32, 32), 3, F32, F16, id="3ch-32x32-render-geometry"),
    pytest.param(9, (8, 66), 3, F16, F32, id="9ch-8x66-odd-pool1-no-planes"),
    pytest.param(9, (8, 68), 2, F16, F32, id="9ch-8x68-conv2-from-planes"),
    pytest.param(9, (32, 128), 3, F16, F32, id="9ch-32x128-dx-rs-bound"),
]
MIXED_ROWS, MIXED_SEED = 60, 3


@pytest.mark.parametrize("channels,hw,B,fwd,dw", MIXED_DEPTH)
def test_mixed_cell_as_the_fused_step(channels, hw, B, fwd, dw):
    from tests.helpers import fused_step_against_f64_oracle
    rep = fused_step_against_f64_oracle(_shape(channels, *hw), B, rows=MIXED_ROWS, graph=False, probe_conv=True, seed=MIXED_SEED)
    print("ROUTES mixed fused %dch %dx%d: %s" % (channels, hw[0], hw[1], rep["conv"]))
    assert rep["conv"]["conv1_fwd"] in FWD_FAMILY[fwd] and rep["conv"]["conv1_dw"] in DW_FAMILY[dw], rep["conv"]


@pytest.mark.parametrize("channels,hw,B,fwd,dw", MIXED_DEPTH)
def test_mixed_cell_op_by_op_on_the_same_rows(channels, hw, B, fwd, dw):
    """actor.train + critic.train (cpp_ddpg_train_actor / cpp_ddpg_train_critic on the gathered f16 minibatch) on the rows the fused
    case above trains on -- the same agent, the same replay rows, the same draw -- with both launch sequences profiled: the single
    network launches must take the routes the four-network launches took, and both pre-clip gradient lists sit at rel 2e-5 of the
    float64 oracle (pool routes: the device's, accepted at near ties only)."""
    from oracle import ddpg_np as O
    from tests.helpers import make_pair, assert_grads_close_modulo_pool_ties, conv_routes_of, _profiled_calls
    shape, rows, seed = _shape(channels, *hw), MIXED_ROWS, MIXED_SEED
    agent, _ref, (aspec, cspec) = make_pair(shape, B, True, seed=seed, replay_size=rows + 50, replay_store="f16")
    try:
        rm = agent.replay_memory
        rm.fill_synthetic(rows, seed=21 + seed)
        idxs = np.random.default_rng(seed + 5).integers(0, rows, B).astype(np.int32)      # (fused_step_against_f64_oracle's eager draw)
        P = [n.get_params() for n in agent.networks()]
        hb = rm.batch(idxs=idxs)
        s1, s2 = rm.state[rm.state_1_idx[idxs]], rm.state[rm.state_2_idx[idxs]]
        t = (s1, hb.action, hb.reward, hb.terminal_mask, s2)
        ref = O.DDPG(aspec, cspec, P[0], P[1], np.float64)
        ref.set_targets(P[2], P[3])
        ctx, got = agent.actor.ctx, {}

        def actor_op():
            agent.actor.train(hb)
            got["actor"] = agent.actor.get_grads()

        def critic_op():
            agent.critic.train(hb)
            got["critic"] = agent.critic.get_grads()

        calls_a = _profiled_calls(ctx, actor_op)
        held = {}

        def actor_grads():
            held["ag"] = ref.actor_gradients(s1)
            return held["ag"]["grads"]

        def critic_grads():
            held["cg"] = ref.critic_gradients(t)
            return held["cg"]["grads"]

        assert_grads_close_modulo_pool_ties(aspec, agent.actor, B, ref.actor, lambda: held["ag"]["cache_actor"], actor_grads, got["actor"],
                                            what="actor.train grads", rel=2e-5)
        calls_c = _profiled_calls(ctx, critic_op)
        assert_grads_close_modulo_pool_ties(cspec, agent.critic, B, ref.critic, lambda: held["cg"]["cache_critic"], critic_grads, got["critic"],
                                            what="critic.train grads", rel=2e-5)
        routes_a, routes_c = conv_routes_of(calls_a), conv_routes_of(calls_c)
        print("ROUTES mixed op-by-op %dch %dx%d: actor %s critic %s" % (channels, hw[0], hw[1], routes_a, routes_c))
        for routes in (routes_a, routes_c):
            assert routes["conv1_fwd"] in FWD_FAMILY[fwd] and routes["conv1_dw"] in DW_FAMILY[dw], (routes_a, routes_c)
    finally:
        agent.close()


@pytest.mark.parametrize("shape,B", [((32, 40, 3, 1, 2), 6), ((50, 50, 3, 2, 3), 7), ((42, 24, 3, 1, 3), 9)],
                         ids=["32x40x6-B6", "50x50x18-B7", "42x24x9-B9-r0-22"])
def test_k16_two_bands_of_rows_per_image_are_an_arrangement_not_arithmetic(tmp_path, shape, B):
    """conv_fwd_k16.hip walks every image as TWO bands of output rows when whole images would fill at most one workgroup slot per CU
    (k16_with_bands: H >= 32, networks x ceil(B / images per workgroup) <= CUs, a first band of r0 rows with r0 even and r0 - 2 a
    multiple of 5: 12 of 32, 22 of 50, 22 of 42; `CPP_CONV_BANDS=0` in the ablation build: whole images).  A band's walk starts two
    input rows above its first output row; its unstored first steps are the only difference, so every pooled value, arg-max code and
    both gradient lists must hold the SAME BITS (conv_rs16.h's bands: test_gpu_conv1_rs16_channels.py)."""
    from tests.test_gpu_conv1_rs16_channels import _run
    new = _run(tmp_path, "bands", shape, B, {})
    old = _run(tmp_path, "whole", shape, B, {"CPP_CONV_BANDS": "0"})
    assert sorted(new) == sorted(old)
    for k in new:
        assert np.isfinite(new[k]).all() and np.array_equal(new[k], old[k]), (k, np.abs(new[k].astype(np.float64) - old[k]).max())
    assert np.abs(new["actor_pool1"]).max() > 0 and np.abs(new["grads"]).max() > 0
