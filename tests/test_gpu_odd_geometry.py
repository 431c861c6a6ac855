"""Images whose height or width is odd, through the fused DDPG step against oracle.DDPG(float64) at the suite's bars -- one row per
class of (H parity, W parity, staging chunk of an image row, vector or generic whitening statistics, conv1 kernels).  --render-height /
--render-width take any integer; every other conv1 geometry of the suite has an even H, an even W and 16-byte rows (the 50 x 50 render reaches odd
sizes only as conv2's 25 x 25 and conv3's 12 x 12 inputs: the f32-plain-input kernels, not conv1's).

What parity decides, as the dispatchers read (each row asserts the profiler's families, so a silent fallback cannot stay green):

* conv_fwd_k16_dispatch refuses an odd W (and an odd image stride), not an odd H; conv_dw16_dispatch refuses both.  An odd-H, even-W
  image runs conv1's forward on the f16 pipes (Hp = H >> 1: the last row completes no pool pair; two bands of rows at H >= 32) and
  conv1's dW on the f32 kernels -- a third mixed cell next to the two of tests/test_gpu_conv_instances.py.  conv_fwd_rs16_dispatch
  refuses an odd H: 64-wide images of odd height take K16_CASE(18, 2, 2).  conv1_f16_pipes_ok needs both dispatchers, so the step reads
  a gathered copy of the minibatch, not the replay store through slots.
* chunk_bytes_for (conv.hip) picks 16, 8 or 4 bytes from the row length W * C * 2 (the image stride is a multiple of it) or none, and
  the (ky,o)-column kernels (conv_kyo.h, conv_dw_kyo.h) take a geometry only where they hold an instance for (channels, width class,
  chunk); their dW also needs an even H.  An odd W reaches exactly one pair of them: 12 channels have rows of 24 W bytes -- a multiple
  of 8 for every W -- and at 33 <= W <= 63 KYO1_CASE_CHB(12, 1, 1, 8) and DWKYO_CASE_CHB(12, 16, IN_F16_WHITEN, 8) take the image: a
  partial last pool column, a last column tile that is not full and a dY column that must stay zero on the reduced-chunk (ky,o)
  kernels (16 x 33 x 12: forward and dW; 15 x 35 x 12: that forward next to the first implementation's dW).  The other reduced-chunk
  instances (18 / 6 channels at 8 bytes, 9 at 4) need row lengths only an even W has, where conv_k16.h comes first.  Every other
  f32-family row runs the first implementation's kernels (conv_fwd_dispatch_l1 / conv_dw_dispatch_l1, conv_impl.h), whose row staging
  has two forms: 16-byte chunks cut at aligned addresses around rows that start anywhere (vec_ok: the image stride H * W * C * 2 is a
  multiple of 16 -- the 16 x 15 and 9 x 15 x 24 rows) and element by element (the others); an even W whose channel count has no
  conv_k16.h instance (15, or 12 at W <= 32) lands there too.  The profiler's conv1_fwd / conv1_dw families do not tell conv_kyo.h from
  conv_impl.h: the table names the kernel per row and tests/test_odd_geometry_census.py derives it from the dispatchers' instance lists.
  The 4-byte (ky,o) forward at an odd height is reached through per-image statistics (test_inference_at_odd_sizes, 9 x 10 x 9).
* H * W * C % 8 != 0 switches the replay's vector statistics off (replay_gather_args: C = 0): the gather copies with 16-byte loads from
  2-, 4- or 8-byte aligned store rows plus an element tail, the whitening tables come from stats_generic_kernel.

tests/test_odd_geometry_census.py enumerates every combination of (H parity, W parity, row chunk, vector or generic statistics, conv1
forward kernel, conv1 dW kernel) that an image with an odd side can have and fails for one without a row here.
Measured figures per row: DESIGN.md section 4, "Odd geometries"."""
import collections

import pytest

pytestmark = pytest.mark.gpu

K16, KYO, IMPL = "k16", "kyo", "impl"         # conv_k16.h (f16 pipes); conv_kyo.h / conv_dw_kyo.h; conv_impl.h (both f32 MFMA)
VECTOR, GENERIC = "vector", "stats_generic"
Row = collections.namedtuple("Row", "shape B chunk fwd dw stats")
# shape (H, W, 3, cameras, repeats), B (odd where the images-per-workgroup remainder is wanted), row chunk in bytes (0: none),
# conv1 forward kernel, conv1 dW kernel, statistics
ROWS = [
    Row((9, 16, 3, 2, 3), 5, 16, K16, IMPL, VECTOR),         # K16_CASE(18, 1, 4)
    Row((33, 40, 3, 1, 2), 3, 16, K16, IMPL, VECTOR),        # K16_CASE(6, 2, 2), two bands of rows (12 + 21) at this B
    Row((17, 72, 3, 1, 3), 2, 16, K16, IMPL, VECTOR),        # K16_CASE(9, 2, 1)
    Row((33, 64, 3, 2, 3), 2, 16, K16, IMPL, VECTOR),        # conv_k16.h, not conv_rs16.h; two bands
    Row((15, 64, 3, 2, 3), 3, 16, K16, IMPL, VECTOR),        # conv_k16.h (H < 16)
    Row((9, 68, 3, 1, 3), 3, 8, K16, IMPL, GENERIC),         # 5508 elements
    Row((16, 15, 3, 2, 4), 3, 16, IMPL, IMPL, VECTOR),
    Row((16, 15, 3, 2, 2), 5, 8, IMPL, IMPL, VECTOR),
    Row((16, 15, 3, 2, 3), 5, 4, IMPL, IMPL, VECTOR),
    Row((16, 15, 3, 1, 1), 7, 0, IMPL, IMPL, VECTOR),        # no chunk: the first implementation's kernels
    Row((13, 11, 3, 1, 2), 5, 4, IMPL, IMPL, GENERIC),       # odd H: dW not on the (ky,o)-column kernel
    Row((15, 15, 3, 1, 1), 5, 0, IMPL, IMPL, GENERIC),       # 675 elements
    Row((9, 9, 3, 1, 3), 7, 0, IMPL, IMPL, GENERIC),         # 729 elements
    Row((51, 51, 3, 1, 2), 2, 4, IMPL, IMPL, GENERIC),
    # one image per workgroup at 12 channels: the reduced-chunk (ky,o) kernels at an odd W (792- and 840-byte rows)
    Row((16, 33, 3, 2, 2), 3, 8, KYO, KYO, VECTOR),          # KYO1_CASE_CHB(12, 1, 1, 8) and DWKYO_CASE_CHB(12, 16, IN_F16_WHITEN, 8)
    Row((15, 35, 3, 2, 2), 3, 8, KYO, IMPL, GENERIC),        # that forward, dW on conv_impl.h (odd H): 6300 elements
    # an odd H at an even W whose channel count has no conv_k16.h instance: forward and dW on conv_impl.h
    Row((9, 10, 3, 1, 5), 3, 4, IMPL, IMPL, GENERIC),        # 15 channels: 1350 elements
    Row((9, 12, 3, 1, 5), 5, 8, IMPL, IMPL, GENERIC),        # 1620 elements
    Row((9, 8, 3, 2, 2), 5, 16, IMPL, IMPL, VECTOR),         # 12 channels at W <= 16
    # the remaining combinations of parity, chunk and statistics
    Row((10, 15, 3, 1, 2), 3, 4, IMPL, IMPL, GENERIC),       # even H that is no multiple of 4: 900 elements
    Row((10, 15, 3, 1, 1), 5, 0, IMPL, IMPL, GENERIC),       # 450 elements
    Row((9, 10, 3, 1, 1), 5, 4, K16, IMPL, GENERIC),         # K16_CASE(3, 1, 4) at 4-byte rows: 270 elements
    Row((9, 15, 3, 2, 4), 3, 16, IMPL, IMPL, VECTOR),        # both odd, 16-byte rows
    Row((9, 15, 3, 2, 2), 5, 8, IMPL, IMPL, GENERIC),        # both odd, 8-byte rows: 1620 elements
]


def row_id(row, exact=False):
    h, w, _three, cams, reps = row.shape
    pipes = "f16" if row.fwd == K16 else "f32"          # (conv1 forward, then dW: always the f32 kernels)
    return "%dx%dx%d-B%d-chunk%d-%sf32-%s%s" % (h, w, 3 * cams * reps, row.B, row.chunk, pipes, row.stats, "-exact" if exact else "")


def _table():
    """(row, exact_products, graph): every row at the default precision, the rows whose forward runs on the f16 pipes once more with
    --exact-products (three f16 pieces per weight), graph replay and the eager call alternating down the table"""
    cases = [(row, False) for row in ROWS] + [(row, True) for row in ROWS if row.fwd == K16]
    return [(row, exact, i % 2 == 0) for i, (row, exact) in enumerate(cases)]


TABLE = _table()
FWD_FAMILY = {K16: "conv1_fwd_f16", KYO: "conv1_fwd", IMPL: "conv1_fwd"}      # the profiler's families
DW_FAMILY = {KYO: "conv1_dw", IMPL: "conv1_dw"}                               # (conv_dw16.h takes no image with an odd side)


def _reset_precision():
    from cartpoleplusplus_amd import _lib
    if _lib.default_context().precision != "fast":
        _lib.default_context().set_precision("fast")


@pytest.mark.parametrize("row,exact,graph", TABLE, ids=[row_id(r, e) for r, e, _g in TABLE])
def test_odd_geometry_takes_its_route_and_holds_the_f64_oracle(row, exact, graph):
    """one minibatch of the fused step (graph: the hipGraph replay on device-drawn rows) against oracle.DDPG(float64) at the helper's own
    bars -- 1e-5 on actions / Q / TD / dQ/da, rel 2e-5 per variable on both pre-clip gradient lists, 2e-6 on the parameters; pool and
    ReLU routes are the device's and accepted at near ties only -- and the families the profiler saw for conv1's forward, conv1's dW and
    the sample pass's statistics"""
    from tests.helpers import fused_step_against_f64_oracle
    kw = {"exact_products": True} if exact else {}
    try:
        rep = fused_step_against_f64_oracle(row.shape, row.B, rows=40, probe_conv=True, seed=23, graph=graph, **kw)
    finally:
        if exact:
            _reset_precision()
    print("ROUTES %s: %s  err_q %.2e grads %.2e / %.2e  near-tie pool windows %d / %d" % (
        row_id(row, exact), rep["conv"], rep["err_q"], rep["rel_actor_grads"], rep["rel_critic_grads"], rep["flips_actor"], rep["flips_critic"]))
    assert rep["conv"]["conv1_fwd"] == FWD_FAMILY[row.fwd], (row_id(row, exact), rep["conv"])
    assert rep["conv"]["conv1_dw"] == DW_FAMILY[row.dw], (row_id(row, exact), rep["conv"])
    stats = rep["conv"]["stats"].split("+")
    assert stats != [""], (row_id(row, exact), rep["conv"])                # a sample pass ran
    assert ("stats_generic" in stats) == (row.stats == GENERIC), (row_id(row, exact), rep["conv"])


# ---- inference: a host batch (one table for the batch: batch_stats), a batch of independent states (cpp_net_forward_each: per-image
# ---- tables -- one stats_generic launch per row where the elements are no multiple of 8 -- and the f32-input kernels, the f16 pipes
# ---- having no per-image weights) and batches of one.  9 x 10 x 9: an even W whose rows are 4-byte multiples -- the per-image forward
# ---- runs on conv_kyo.h's KYO1_CASE_CHB(9, 1, 4, 4) at an odd height
INFERENCE = [pytest.param((9, 16, 3, 2, 3), "gather_stats", id="9x16x18"), pytest.param((15, 15, 3, 1, 1), "stats_generic", id="15x15x3"),
             pytest.param((9, 10, 3, 1, 3), "stats_generic", id="9x10x9")]


@pytest.mark.parametrize("shape,stats", INFERENCE)
def test_inference_at_odd_sizes(shape, stats):
    import numpy as np
    from cartpoleplusplus_amd import _lib
    from cartpoleplusplus_amd._lib import lib, check, ptr
    from tests.helpers import _profiled_calls, make_pair
    B, ATOL = 5, 1e-5
    agent, ref, _specs = make_pair(shape, B, True, seed=7)
    rng = np.random.default_rng(17)
    s = rng.integers(0, 256, (B,) + shape).astype(np.float16) / np.float16(255)
    a = rng.uniform(-1, 1, (B, 2)).astype(np.float32)
    ctx = agent.actor.ctx
    try:
        for dtype in (np.float16, np.float32):
            x = s.astype(dtype)
            # one table for the batch
            want_a, want_q = ref.actor.forward(s), ref.critic.forward(s, action=a)
            got = {}
            calls = _profiled_calls(ctx, lambda: got.update(a=agent.actor.forward(x)))
            assert calls.get(stats, 0) >= 1 and (stats == "stats_generic") == (calls.get("stats_generic", 0) > 0), calls
            got_q = agent.critic.forward(x, a)
            pools = [getattr(agent.critic, "pool%d" % i).eval(B) for i in (1, 2, 3)]
            assert np.abs(got["a"] - want_a["out"]).max() < ATOL and np.abs(got_q - want_q["out"]).max() < ATOL
            for i, name in enumerate(("conv1", "conv2", "conv3")):
                assert pools[i].size > 0 and np.abs(pools[i].reshape(want_q[name][1].shape) - want_q[name][1]).max() < ATOL, name
            # every image with its own statistics
            calls = _profiled_calls(ctx, lambda: got.update(each=agent.actor.actions_given(x)))
            if stats == "stats_generic":
                assert calls.get("stats_generic", 0) == B, calls                    # forward_each's loop: one launch per image
            else:
                assert calls.get("stats_generic", 0) == 0 and calls.get("gather_stats", 0) == 1, calls
            assert calls.get("conv1_fwd", 0) == 1 and calls.get("conv1_fwd_f16", 0) == 0, calls      # the f32-input kernels
            want_each = np.concatenate([ref.actor.forward(s[i:i + 1])["out"] for i in range(B)], axis=0)
            assert got["each"].shape == (B, 2) and np.abs(got["each"] - want_each).max() < ATOL
            one = np.concatenate([agent.actor.action_given(x[i]) for i in range(B)], axis=0)
            assert np.array_equal(got["each"], one), np.abs(got["each"] - one).max()       # (conv.hip: B = 1 stays off the f16 pipes for this)
            assert np.abs(one[:1] - ref.action_given(s[0])).max() < ATOL
            assert np.abs(got["each"] - got["a"]).max() > 0                                 # ... and it is not the batch-statistics forward
            # the critic the same way (cpp_net_forward_each with an action batch)
            q_each = np.empty((B, 1), np.float32)
            xs, dt = _lib.as_state_array(x)
            check(lib.cpp_net_forward_each(agent.critic.handle, ptr(xs), dt, B, ptr(a), ptr(q_each)))
            want_q_each = np.concatenate([ref.critic.forward(s[i:i + 1], action=a[i:i + 1])["out"] for i in range(B)], axis=0)
            assert np.abs(q_each - want_q_each).max() < ATOL
            q_one = np.concatenate([agent.critic.forward(x[i:i + 1], a[i:i + 1]) for i in range(B)], axis=0)
            assert np.array_equal(q_each, q_one)
    finally:
        agent.close()


# ---- NAF: the op-by-op body of tests/test_gpu_naf.py and one fused cpp_naf_train_step minibatch (graph replay, Momentum 0.5, the
# ---- hyperparameters of tests/test_gpu_hyperparameters.py's NAF cases) at an odd height on a shared trunk and at an odd height and width
# ---- on three trunks of their own
NAF = [pytest.param((9, 16, 3, 1, 2), 4, True, id="9x16x6-B4-shared-trunk"), pytest.param((15, 13, 3, 1, 3), 3, False, id="15x13x9-B3-own-trunks")]


@pytest.mark.parametrize("shape,B,share", NAF)
def test_naf_forward_gradients_and_sgd_step_at_odd_sizes(shape, B, share):
    from tests.test_gpu_naf import test_naf_forward_gradients_and_sgd_step as body
    body(shape, B, share)


@pytest.mark.parametrize("shape,B,share", NAF)
def test_naf_fused_minibatch_at_odd_sizes(shape, B, share):
    from tests.test_gpu_hyperparameters import _naf_step
    from tests.helpers import NAF_HYPER
    rep = _naf_step(shape, B, share, "momentum-0.5")
    assert rep["norm"] > NAF_HYPER["clip"]


# ---- batch norm: launch_conv_dw_multi's dense arm has no parity rule of its own (dense => the (ky,o)-column kernel; conv_dw16.h refuses
# ---- the odd side) -- what decides is whether conv_dw_kyo_dispatch_dense holds an instance for (channels, columns, chunk):
# ---- 9 x 16 x 6: DWD_CASE(6, 5, 8, F16, 16); 33 x 64 x 18: DWD_CASE(18, 5, 16, F16, 16), the forward on K16_CASE(18, 2, 2, plain);
# ---- 16 x 15 x 6: 180-byte rows, a 4-byte chunk, no instance -- refused like tests/test_gpu_batchnorm_training.py's REFUSED rows
BN_PARITY = [(9, 16, 3, 1, 2), (33, 64, 3, 2, 3)]
BN_REFUSED = [((16, 15, 3, 1, 2), r"no kernel for 16x15, 6 channels, 5x5 taps, 4-byte")]


@pytest.mark.parametrize("shape", BN_PARITY, ids=["9x16x6", "33x64x18"])
def test_batch_norm_fused_minibatch_at_odd_sizes(shape):
    from tests.test_gpu_batchnorm_training import _fused
    _fused(shape, 3, 40, graph=True, seed=2)


@pytest.mark.parametrize("shape,msg", BN_REFUSED, ids=["16x15x6"])
def test_batch_norm_refuses_an_odd_width_without_an_instance_and_names_it(shape, msg):
    import numpy as np
    from tests.helpers import make_pair
    from tests.test_gpu_batchnorm_training import test_a_refused_geometry_says_so_and_leaves_the_context_usable as refused
    B = 3
    agent, _ref, _specs = make_pair(shape, B, True, replay_size=60, use_batch_norm=True)
    try:
        agent.replay_memory.fill_synthetic(40, seed=1)
        before = [n.get_params() for n in agent.networks()]
        with pytest.raises(RuntimeError, match=msg):        # the geometry by name
            agent.train_step(B, 1)
        for x, n in zip(before, agent.networks()):
            assert np.array_equal(x, n.get_params()), n.namespace
    finally:
        agent.close()
    refused(shape, "f16")                                   # op by op and fused, and a batch-norm agent on the context afterwards


# ---- what surrounds the step.  9 x 16 x 18: conv1 forward on the f16 pipes, dW on the f32 kernels, a gathered copy (no direct replay),
# ---- vector statistics; 15 x 15 x 3: the first implementation's kernels, the copy-only gather and stats_generic tables
AROUND = [pytest.param((9, 16, 3, 2, 3), 6, id="9x16x18-B6"), pytest.param((15, 15, 3, 1, 1), 5, id="15x15x3-B5")]
AROUND_SEED = 1          # host_case seed: the float32 twin keeps the float64 oracle's routes over three LOUD minibatches at both shapes


@pytest.mark.parametrize("shape,B", AROUND)
def test_three_minibatches_in_one_call_as_deltas_at_odd_sizes(shape, B):
    """train_step(B, 3) at LOUD hyperparameters: the sample rider and the `next` minibatch without direct replay; the four parameter
    vectors as deltas against the float64 restatement, delta_bound as it stands (tests/test_gpu_hyperparameters.py)"""
    from tests.test_gpu_hyperparameters import test_several_minibatches_in_one_call_as_deltas as body
    body(shape, B, AROUND_SEED, "LOUD", 3)


@pytest.mark.parametrize("shape,B", AROUND)
def test_the_literal_loop_is_the_fused_step_at_odd_sizes(shape, B):
    import numpy as np
    from tests.helpers import LOUD, hyper_options
    from tests.test_gpu_literal_loop import _twin_agents
    lit, fused = _twin_agents(shape, B, True, rows=60, **hyper_options(LOUD))
    try:
        np.random.seed(99)
        for step in range(4):
            batch = lit.replay_memory.batch(B)            # ddpg_cartpole.py:331-337, one minibatch per step
            lit.actor.train(batch.state_1)
            lit.critic.train(batch)
            lit.target_actor.update_weights()
            lit.target_critic.update_weights()
            fused.train_step(B, 1, idxs=batch.idxs)
            for x, y in zip(lit.networks(), fused.networks()):
                assert np.array_equal(x.get_params(), y.get_params()), (x.namespace, step)
        assert lit.trainer.fused_pairs == 4
        assert np.array_equal(lit.trainer.last_stats(), fused.trainer.last_stats())
    finally:
        lit.close(); fused.close()


@pytest.mark.parametrize("shape,B", AROUND)
def test_graph_replay_is_the_eager_call_on_the_same_rows_at_odd_sizes(shape, B):
    import numpy as np
    from tests.helpers import LOUD, hyper_options
    from tests.test_gpu_batchnorm_training import _last_rows
    from tests.test_gpu_literal_loop import _twin_agents
    replayed, eager = _twin_agents(shape, B, True, rows=60, **hyper_options(LOUD))
    try:
        for step in range(4):          # the first call runs eagerly and captures, the later ones replay
            replayed.train_step(B, 1)
            eager.train_step(B, 1, idxs=_last_rows(replayed, B))
            for x, y in zip(replayed.networks(), eager.networks()):
                assert np.array_equal(x.get_params(), y.get_params()), (x.namespace, step)
        assert np.array_equal(replayed.trainer.last_stats(), eager.trainer.last_stats())
        assert np.array_equal(replayed.actor.get_grads(), eager.actor.get_grads())
        assert np.array_equal(replayed.critic.get_grads(), eager.critic.get_grads())
    finally:
        replayed.close(); eager.close()


@pytest.mark.parametrize("shape,B", AROUND)
def test_three_runs_from_one_seed_are_identical_at_odd_sizes(shape, B):
    import numpy as np
    from tests.helpers import LOUD, hyper_options, make_pair
    runs = []
    for _ in range(3):
        agent, _ref, _specs = make_pair(shape, B, True, replay_size=100, **hyper_options(LOUD))
        try:
            agent.replay_memory.fill_synthetic(60, seed=11)
            for _step in range(3):
                agent.train_step(B, 3)
            agent.actor.ctx.sync()
            runs.append([n.get_params() for n in agent.networks()] + [agent.actor.get_grads(), agent.critic.get_grads()])
        finally:
            agent.close()
    assert all(np.isfinite(x).all() for x in runs[0])
    for other in runs[1:]:
        for x, y in zip(runs[0], other):
            assert np.array_equal(x, y)


@pytest.mark.parametrize("shape,B", AROUND)
def test_native_learner_at_world_size_one_reaches_the_fused_step_at_odd_sizes(shape, B):
    from cartpoleplusplus_amd import ddpg_cartpole as D
    from cartpoleplusplus_amd.distributed import Communicator, NativeLearner
    from tests.helpers import make_pair
    from tests.test_gpu_distributed import _close_params
    res = []
    for which in ("fused", "dp"):
        agent, _ref, _specs = make_pair(shape, B, True, replay_size=100)
        try:
            agent.replay_memory.fill_synthetic(60, seed=11)
            if which == "fused":
                for _ in range(3):
                    agent.train_step(B, 3)
            else:
                comm = Communicator.single(agent.trainer.ctx)
                assert (comm.rank, comm.world) == (0, 1)
                learner = NativeLearner(agent, B, int(D.opts.sample_seed), comm, sync_every=1, overlap=False)
                for _ in range(3):
                    learner.train_step(3)
                assert "dp1" in learner.describe()
                learner.close()
            agent.actor.ctx.sync()
            res.append([n.get_params() for n in agent.networks()])
        finally:
            agent.close()
    _close_params(res[0], res[1])
