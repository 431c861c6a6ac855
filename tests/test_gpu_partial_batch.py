"""Batches below the capacity the agent was built with.  Every training and inference entry point takes any B in [1, capacity]
(--batch-size, cpp_net_spec.max_batch), workspaces, partial lists and noise buffers are sized by the capacity, and the graph caches key
on B.  Each case here builds the agent at capacity C, runs a C-row batch first, so that every row and slot beyond B holds real data
of a batch that is over, and then holds a B-row batch to the float64 oracle at the bars the same quantity has at B = C in its own
runner (tests.helpers.fused_step_against_f64_oracle, tests/test_gpu_naf.py, tests/test_gpu_parity.py, tests/test_gpu_ddpg_optimisers.py,
tests/test_gpu_distributed.py); one more C-row batch follows, so that no count cached from the small one survives either.

What a device that followed C where it should follow B would show against these bars is tests/test_partial_batch_host.py's (CPU, the
oracle alone).  No case compares a capacity-C agent at B with a capacity-B agent bit for bit: the dW slice plan may differ."""
import collections
import ctypes
import time

import numpy as np
import pytest

from oracle import ddpg_np as O
from tests import ddpg_opt_np as R
from tests.helpers import (PARTIAL_B, PARTIAL_C, PARTIAL_LOWDIM, PARTIAL_PIX, assert_flat_close, fused_step_against_f64_oracle, hyper_options,
                           make_pair, naf_partial_case, oracle_minibatch, oracle_of, partial_case, partial_sizes)

pytestmark = pytest.mark.gpu
PIX, LOWDIM, CFG3 = PARTIAL_PIX, PARTIAL_LOWDIM, (64, 64, 3, 2, 3)
ATOL = 1e-5
HostBatch = collections.namedtuple("HostBatch", "state_1 action reward terminal_mask state_2")
ADAM = ("Adam", {"learning_rate": 0.01, "beta1": 0.8, "beta2": 0.9, "epsilon": 1e-3})        # tests.helpers.NAF_OPTIMISERS' "adam-third-step":
# with this epsilon an element whose gradient is float32 noise moves by lr g / epsilon, not by +-lr (tests/test_gpu_dropout.py uses it so)


def _figures(rep):
    return {k: ("%.2e" % v if isinstance(v, float) else v) for k, v in sorted(rep.items()) if k.startswith(("err_", "rel_", "path", "conv", "flips", "critic_grads_checked"))}


def _fused(what, shape, C, B, graph, pixel=True, **kw):
    t0 = time.time()
    rep = fused_step_against_f64_oracle(shape, B, max(300, 3 * C), graph=graph, probe=True, probe_conv=pixel, pixel=pixel, capacity=C, **kw)
    print("%s capacity %d, B = %d (%s): path %s, conv %s, %.1f s\n  at B: %s\n  back at capacity: %s" % (
        what, C, B, "graph replay" if graph else "eager", rep["path"], rep.get("conv"), time.time() - t0, _figures(rep), _figures(rep["back"])))
    return rep


# ---- 1. DDPG, plain ---------------------------------------------------------------------------------------------------------------
# (8, 5) and (8, 1): both sides of the heads kernel's four rows per workgroup, and B = 1 takes conv1 off the f16 pipes; (16, 4): exactly
# one workgroup; (64, 33), (256, 100): many
@pytest.mark.parametrize("graph", [True, False], ids=["graph-replay", "eager"])
@pytest.mark.parametrize("C,B", [(8, 5), (8, 1), (16, 4), (64, 33), (256, 100)])
def test_ddpg_pixel_step_below_capacity(C, B, graph):
    _fused("DDPG 16x16x6", PIX, C, B, graph)


def test_ddpg_release_conv_kernels_below_capacity():
    _fused("DDPG 64x64x18", CFG3, 32, 9, True)


# (1025, 16): the capacity lies past the heads kernel's limit of 1024 rows, the batch inside it
@pytest.mark.parametrize("graph", [True, False], ids=["graph-replay", "eager"])
@pytest.mark.parametrize("C,B", [(16, 5), (1025, 16)])
def test_ddpg_lowdim_step_below_capacity(C, B, graph):
    _fused("DDPG low-dimensional", LOWDIM, C, B, graph, pixel=False)


def _agent_of_case(shape, C, case, hyper, **kw):
    """a device agent of capacity C holding the case's parameters and episodes"""
    specs, P, episodes = case[:3]
    rows = sum(len(ep[1]) for ep in episodes)
    agent, _ref, (aspec, _c) = make_pair(shape, C, len(shape) == 5, replay_size=rows, perturb=False, **dict(hyper_options(hyper), **kw))
    try:
        assert list(aspec.hidden) == list(specs[0].hidden)
        for net, p in zip(agent.networks(), P):
            assert net.get_params().shape == p.shape
            net.set_params(p)
        for ep in episodes:
            agent.replay_memory.add_episode(*ep)
        assert agent.replay_memory.size() == rows
    except Exception:
        agent.close()
        raise
    return agent


@pytest.mark.parametrize("opt", ["momentum-0.5", "adam"])
def test_optimiser_slots_over_the_four_steps(opt):
    """Momentum and Adam at (8, 5): C, B, B and C rows, each a fused step on the caller's rows with its target update.  Parameters,
    targets, m, v and both step counts against tests/ddpg_opt_np.py's restatement walking the same four minibatches, at
    tests/test_gpu_ddpg_optimisers.py's bounds for four stores."""
    from tests.test_gpu_ddpg_optimisers import _compare, _opt_kw, _state
    C, B = PARTIAL_C, PARTIAL_B
    case = partial_case(PIX, C, B)
    specs, P, _ep, idxs, batches = case
    hp = R.hyper_of(opt, 0.5, 0.25)
    agent = _agent_of_case(PIX, C, case, hp, **_opt_kw(opt))
    try:
        for rows in idxs:
            agent.train_step(len(rows), 1, idxs=rows)
        got = [n.get_params() for n in agent.networks()]
        slots, steps = _state(agent)
        stats = agent.trainer.last_stats()
    finally:
        agent.close()
    name, args = R.OPTIMISERS[opt]
    ref = R.restatement(specs, P, np.float64, hp, name, args)
    outs = []
    for b in batches:
        outs.append(ref.train_minibatch(b))
        ref.update_targets()
    na, nc = outs[-1]["actor_norm"], outs[-1]["critic_norm"]
    assert abs(stats[1] - na) < 1e-4 * max(1.0, na) and abs(stats[2] - nc) < 1e-4 * max(1.0, nc), (stats, na, nc)
    assert min(min(o["actor_norm"], o["critic_norm"]) for o in outs) > hp.gradient_clip          # (every list of every step is clipped)
    assert steps == [int(x) for x in ref.state()["step"]] == [4, 4]
    _compare("%s-capacity-%d-B-%d" % (opt, C, B), opt, P, got + slots, R.vectors(ref), 4)


@pytest.mark.parametrize("opt", ["gradient-descent", "adam"])
def test_target_smoothing_and_policy_delay_over_the_four_steps(opt):
    """--target-policy-noise with --policy-delay 2 at (8, 5): the four minibatches C, B, B, C are held, applied, held, applied -- the held
    step falls on a B-row minibatch once and off it once.  The noise of every target-forming pass at its own row count against the
    restated draw (tests/test_gpu_target_smoothing.py's bar), a held minibatch leaving every bit of the actor, and parameters, targets,
    slots and counts against tests/td3_np.py's restatement at tests/test_gpu_policy_delay.py's bounds for four stores."""
    from tests import td3_np as T3
    from tests import tps_np as T
    from tests.test_gpu_policy_delay import _actor_bits, _compare, _state
    from tests.test_gpu_target_smoothing import assert_noise
    C, B, d = PARTIAL_C, PARTIAL_B, 2
    sigma, clip, seed = T.SIGMA, T.CLIP, T.NOISE_SEED
    case = partial_case(PIX, C, B)
    specs, P, _ep, idxs, batches = case
    hp = T3.hyper_of(opt, 0.5, 0.25)
    agent = _agent_of_case(PIX, C, case, hp, policy_delay=d, target_policy_noise=sigma, target_policy_noise_clip=clip,
                           target_policy_noise_seed=seed, **T3.opt_kw(opt))
    try:
        assert agent.trainer.policy_delay == d
        for k, rows in enumerate(idxs):
            before, t0 = _actor_bits(agent)
            agent.train_step(len(rows), 1, idxs=rows)
            eps, n = agent.trainer.last_target_noise(len(rows))
            assert n == k and eps.shape == (len(rows), 2)
            assert_noise(eps, k, sigma, clip, seed, what="%d rows" % len(rows))
            after, t1 = _actor_bits(agent)
            assert agent.trainer.policy_delay_status() == (d, k + 1, (k + 1) % d != 0)
            if (k + 1) % d:
                assert all(np.array_equal(x, y) for x, y in zip(before, after)) and t1 == t0, k
            else:
                assert not np.array_equal(before[0], after[0]), k
        got = [n.get_params() for n in agent.networks()]
        slots, counts = _state(agent)
        stats = agent.trainer.last_stats()
    finally:
        agent.close()
    ref = T3.restatement(specs, P, np.float64, hp, opt, d, (sigma, clip, seed))
    outs = []
    for b in batches:
        outs.append(ref.train_minibatch(b))
        ref.update_targets()
    assert ref.schedule == [False, True, False, True] and min(o["tie"] for o in outs) > T3.TIE_FLOOR
    na, nc = outs[-1]["actor_norm"], outs[-1]["critic_norm"]
    assert abs(stats[1] - na) < 1e-4 * max(1.0, na) and abs(stats[2] - nc) < 1e-4 * max(1.0, nc), (stats, na, nc)
    if counts is not None:
        assert counts == [int(x) for x in ref.state()["step"]] == [2, 4], counts
    _compare("%s-smoothed-d2-capacity-%d-B-%d" % (opt, C, B), opt, P, got + slots, R.vectors(ref), 4)


# ---- 2. the single ops and the literal loop on host batches: the cpp_batch of capacity C carries B rows ---------------------------
@pytest.mark.parametrize("shape", [PIX, LOWDIM], ids=["16x16x6", "low-dimensional"])
def test_single_ops_on_a_host_batch_below_capacity(shape):
    """The single ops on one cpp_batch of capacity C (replay_memory.DeviceBatch, the buffer actor.train / critic.train upload a host
    batch into): a C-row host batch, then a B-row one uploaded into the SAME buffer, its rows B .. C-1 still the first batch's --
    cpp_ddpg_check_loss, cpp_ddpg_q_gradients_wrt_actions, cpp_ddpg_train_actor, cpp_ddpg_train_critic, then both target updates.
    Gradients of the B-row calls at tests/test_gpu_parity.py's bar (rel 2e-5 per variable), both reported norms at 1e-4, the parameters
    after both pairs and the target update at its 1e-5 / 1e-6, check_loss on the B rows at 1e-5 -- against tests.helpers.oracle_minibatch."""
    from cartpoleplusplus_amd import replay_memory
    from cartpoleplusplus_amd._lib import lib, check, ptr
    C, B = PARTIAL_C, PARTIAL_B
    case = partial_case(shape, C, B)
    specs, P, _ep, _idxs, batches = case
    hp = O.DEFAULT_HYPER
    agent = _agent_of_case(shape, C, case, hp)
    ref = oracle_of(specs, P, np.float64, hp)
    dev = None
    try:
        trainer = agent.trainer
        dev = replay_memory.DeviceBatch(C, trainer.state_elems, trainer.action_dim, trainer.ctx)
        assert dev.max_batch == C
        dev.upload(*batches[0])
        assert dev.size == C
        check(lib.cpp_ddpg_train_actor(trainer.handle, dev.handle))
        check(lib.cpp_ddpg_train_critic(trainer.handle, dev.handle))
        oracle_minibatch(ref, batches[0])
        dev.upload(*batches[1])
        assert dev.size == B
        ag, cg = ref.actor_gradients(batches[1][0]), ref.critic_gradients(batches[1])
        loss, td, q = np.zeros(1, np.float32), np.empty((B, 1), np.float32), np.empty((B, 1), np.float32)
        check(lib.cpp_ddpg_check_loss(trainer.handle, dev.handle, ptr(loss), ptr(td), ptr(q)))
        assert np.abs(q - cg["q"]).max() < ATOL and np.abs(td - cg["td"]).max() < ATOL
        assert abs(loss[0] - cg["loss"]) < ATOL * max(1.0, abs(cg["loss"]))
        dq = np.empty((B, 2), np.float32)
        check(lib.cpp_ddpg_q_gradients_wrt_actions(trainer.handle, dev.handle, ptr(dq), None, None))
        assert np.abs(dq - ag["dq_da"]).max() < ATOL
        check(lib.cpp_ddpg_train_actor(trainer.handle, dev.handle))
        assert_flat_close(specs[0], agent.actor.get_grads(), ag["grads"], what="actor grads, B rows in a C-row batch")
        na = float(np.linalg.norm(ag["grads"]))
        assert abs(trainer.last_stats()[1] - na) < 1e-4 * max(1.0, na), (trainer.last_stats(), na)
        check(lib.cpp_ddpg_train_critic(trainer.handle, dev.handle))
        assert_flat_close(specs[1], agent.critic.get_grads(), cg["grads"], what="critic grads, B rows in a C-row batch")
        nc = float(np.linalg.norm(cg["grads"]))
        assert abs(trainer.last_stats()[2] - nc) < 1e-4 * max(1.0, nc), (trainer.last_stats(), nc)
        agent.target_actor.update_weights()
        agent.target_critic.update_weights()
        oracle_minibatch(ref, batches[1])
        ref.update_targets()
        got = [n.get_params() for n in agent.networks()]
    finally:
        if dev is not None:
            dev.close()
        agent.close()
    assert_flat_close(specs[0], got[0], ref.actor.flat(), rel=1e-5, what="actor params")
    assert_flat_close(specs[1], got[1], ref.critic.flat(), rel=1e-5, what="critic params")
    assert_flat_close(specs[0], got[2], ref.target_actor.flat(), rel=1e-6, what="target actor")
    assert_flat_close(specs[1], got[3], ref.target_critic.flat(), rel=1e-6, what="target critic")


# ---- 3. NAF -----------------------------------------------------------------------------------------------------------------------
# (share, widths): the three head paths of the shared trunk by their widths (tests/test_gpu_head_shapes.py) and trunks of their own
NAF_PATHS = [pytest.param(True, [100, 50], "mlp", id="shared-mlp"), pytest.param(True, [100, 52], "heads", id="shared-heads"),
             pytest.param(True, [100, 64], "gemm", id="shared-gemm"), pytest.param(False, [32, 16], "gemm", id="own-trunks-gemm")]


@pytest.mark.parametrize("C,B", [(8, 5), (64, 33)])
@pytest.mark.parametrize("share,hidden,path", NAF_PATHS)
def test_naf_fused_step_below_capacity(share, hidden, path, C, B):
    from tests.test_gpu_naf import naf_fused_step_against_f64_oracle
    t0 = time.time()
    got = naf_fused_step_against_f64_oracle(PIX, B, share, rows=300, probe=True, optimiser=ADAM[0], optimiser_args=ADAM[1], hidden=hidden,
                                            capacity=C)
    print("NAF share=%s hidden %s capacity %d, B = %d: path %s (%.1f s)" % (share, hidden, C, B, got, time.time() - t0))
    assert got == path, (got, path)


@pytest.mark.parametrize("entry", ["train_rows", "train_rows_async"])
@pytest.mark.parametrize("share,C,B", [(True, 8, 5), (False, 8, 5), (True, 64, 33)], ids=["shared-8-5", "own-trunks-8-5", "shared-64-33"])
def test_naf_train_rows_below_capacity(entry, share, C, B):
    """cpp_naf_train_rows and cpp_naf_train_rows_async (naf.train on a replay draw) on C, B, B and C rows under Adam: every loss at 1e-5,
    the parameters after the four updates and the target update at tests/test_gpu_naf.py's rel 2e-5 / 1e-6, Adam's count"""
    from cartpoleplusplus_amd._lib import lib, check, ptr
    from oracle import naf_np as N
    from tests.test_gpu_naf import CatSpec, make_naf, params_of
    hidden = [100, 50] if share else [32, 16]
    specs, flats, episodes, idxs, batches = naf_partial_case(PIX, C, B, rows=120, hidden=hidden, share=share)
    agent, _ref, aspecs = make_naf(PIX, B, share, ADAM[0], ADAM[1], replay_size=120, hidden=hidden, capacity=C)
    losses = []
    try:
        nets = (agent.value_net, agent.naf.mu_net, agent.naf.l_net, agent.target_value_net)
        for net, p in zip(nets, flats):
            assert net.get_params().shape == p.shape
            net.set_params(p)
        for ep in episodes:
            agent.replay_memory.add_episode(*ep)
        for rows in idxs:
            if entry == "train_rows":
                loss = ctypes.c_float()
                check(lib.cpp_naf_train_rows(agent.naf.handle, agent.replay_memory.handle, len(rows), ptr(rows), ctypes.byref(loss)))
                losses.append(loss.value)
            else:
                losses.append(agent.naf.train(agent.replay_memory.batch(idxs=rows)))
        losses = [float(x) for x in losses]
        agent.target_value_net.update_weights()
        got, target = params_of(agent), agent.target_value_net.get_params()
        count = int(agent.naf.get_optimiser_state()["step"])
    finally:
        agent.close()
    ref = N.NAF(specs[0], specs[1], specs[2], flats[0], flats[1], flats[2], share, 2, np.float64, optimiser=N.make_optimiser(*ADAM),
                gradient_clip=5.0, discount=0.99, target_update_rate=1e-4)
    ref.target_value = O.Net(specs[0], flats[3], np.float64)
    want = [float(ref.train(b)["loss"]) for b in batches]
    ref.update_targets()
    print("NAF %s share=%s sizes %s: losses %s, oracle %s" % (entry, share, partial_sizes(C, B), losses, want))
    for g, w in zip(losses, want):
        assert abs(g - w) < ATOL * max(1.0, abs(w)), (losses, want)
    assert count == 4
    assert_flat_close(CatSpec(specs), got, ref.flat(), rel=2e-5, what="NAF params after C, B, B, C rows")
    assert_flat_close(specs[0], target, ref.target_value.flat(), rel=1e-6, what="target value")


# ---- 4. inference at 1 < B < C, behind a full-capacity call of the same entry point ------------------------------------------------
INFER = [(8, 3), (64, 33)]


def _states(shape, n, seed):
    pixel = len(shape) == 5
    return O.synthetic_batch(np.random.default_rng(seed), n, shape, 2, pixel)


@pytest.mark.parametrize("C,B", INFER)
def test_ddpg_inference_uses_the_statistics_of_its_own_rows(C, B):
    """actor.forward, critic.forward and check_loss whiten with the statistics of the B images they are given, actions_given with each
    row's own: against the oracle's rows at tests/test_gpu_parity.py's 1e-5"""
    agent, ref, _ = make_pair(PIX, B, True, capacity=C)
    big, small = _states(PIX, C, 11), _states(PIX, B, 12)
    try:
        for dtype in (np.float16, np.float32):
            agent.actor.forward(big[0].astype(dtype))
            got = agent.actor.forward(small[0].astype(dtype))
            assert got.shape == (B, 2) and np.abs(got - ref.actor.forward(small[0])["out"]).max() < ATOL
            agent.critic.forward(big[0].astype(dtype), big[1])
            got = agent.critic.forward(small[0].astype(dtype), small[1])
            wq = ref.critic.forward(small[0], action=small[1])
            assert got.shape == (B, 1) and np.abs(got - wq["out"]).max() < ATOL
            for i, name in enumerate(("conv1", "conv2", "conv3")):
                assert np.abs(getattr(agent.critic, "pool%d" % (i + 1)).eval(B) - wq[name][1]).max() < ATOL, name
        # (the batch statistics matter at this bar: the oracle's first B rows of the C-row forward are not the B-row forward)
        mixed = ref.actor.forward(np.concatenate([small[0], big[0][B:]]))["out"][:B]
        assert np.abs(mixed - ref.actor.forward(small[0])["out"]).max() > 10 * ATOL
        agent.critic.check_loss(HostBatch(*big))
        loss, td, q = agent.critic.check_loss(HostBatch(*small))
        cg = ref.critic_gradients(small)
        assert np.abs(q - cg["q"]).max() < ATOL and np.abs(td - cg["td"]).max() < ATOL
        assert abs(loss - cg["loss"]) < ATOL * max(1.0, abs(cg["loss"]))
        agent.actor.actions_given(big[0])
        each = agent.actor.actions_given(small[0])
        one = np.concatenate([agent.actor.action_given(small[0][i]) for i in range(B)], axis=0)
        assert each.shape == (B, 2) and np.array_equal(each, one)
        want = np.concatenate([ref.actor.forward(small[0][i:i + 1])["out"] for i in range(B)], axis=0)
        assert np.abs(each - want).max() < 1e-5
    finally:
        agent.close()


@pytest.mark.parametrize("C,B", INFER)
def test_naf_inference_uses_the_statistics_of_its_own_rows(C, B):
    """naf.forward, value_given, action_given per row and debug_values at tests/test_gpu_naf.py's 1e-5"""
    from tests.test_gpu_naf import HB, make_naf
    agent, ref, _specs = make_naf(PIX, B, True, capacity=C)
    big, small = _states(PIX, C, 3), _states(PIX, B, 4)
    try:
        out = ref.forward_backward(small, backward=False)
        agent.naf.debug_values(HB(big))
        l_values, loss, v, a, vp = agent.naf.debug_values(HB(small))
        adv = out["advantage"][:, 0]
        assert l_values.shape[0] == B and np.abs(l_values - out["l_values"]).max() < ATOL
        assert np.abs(v - out["value"][:, 0]).max() < ATOL and (np.abs(a - adv) <= ATOL * np.maximum(1.0, np.abs(adv))).all()
        assert np.abs(vp - out["target_value"][:, 0]).max() < ATOL and abs(loss - out["loss"]) < ATOL * max(1.0, abs(out["loss"]))
        agent.naf.forward(big[0])
        assert np.abs(agent.naf.forward(small[0]) - out["mu"]).max() < ATOL
        agent.value_net.value_given(big[0])
        assert np.abs(agent.value_net.value_given(small[0]) - out["value"]).max() < ATOL
        for i in range(B):
            one = agent.naf.action_given(small[0][i].astype(np.float32), add_noise=False)
            assert np.abs(one - ref.action_given(small[0][i])).max() < ATOL, i
    finally:
        agent.close()


# ---- 5. the data-parallel step as a world of one ------------------------------------------------------------------------------------
def test_data_parallel_world_of_one_below_capacity():
    """tests/test_gpu_distributed.py's comparison at (8, 5): C-row steps, B-row steps and C-row steps again through NativeLearner over a
    communicator of one rank end on the fused step's parameters (1e-6: the dW reductions may sum in other slices)"""
    from cartpoleplusplus_amd import ddpg_cartpole as D
    from cartpoleplusplus_amd.distributed import Communicator, NativeLearner
    from tests.test_gpu_distributed import _close_params, _params
    C, B = PARTIAL_C, PARTIAL_B
    res = []
    for which in ("fused", "dp"):
        agent, _ref, _ = make_pair(PIX, B, True, replay_size=300, capacity=C)
        learners, comm = {}, None
        try:
            agent.replay_memory.fill_synthetic(200, seed=11)
            if which == "dp":
                comm = Communicator.single(agent.trainer.ctx)
            for n, times in ((C, 2), (B, 3), (C, 2)):
                for _ in range(times):
                    if which == "fused":
                        agent.train_step(n, 2)
                    else:
                        if n not in learners:
                            learners[n] = NativeLearner(agent, n, int(D.opts.sample_seed), comm)
                        learners[n].train_step(2)
            agent.actor.ctx.sync()
            res.append(_params(agent))
        finally:
            for l in learners.values():
                l.close()
            if comm is not None:
                comm.close()
            agent.close()
    print("data-parallel world of one, sizes 8, 5, 8: largest difference from the fused step %.3e" % max(
        float(np.abs(x - y).max()) for x, y in zip(*res)))
    _close_params(res[0], res[1])


# ---- 6. variants through tests.helpers.fused_step_against_f64_oracle at (8, 5) -------------------------------------------------------
@pytest.mark.parametrize("graph", [True, False], ids=["graph-replay", "eager"])
def test_batch_norm_moments_are_taken_over_the_rows_of_the_batch(graph):
    """--use-batch-norm in training: the batch moments of all four networks over B rows (stale rows B .. C-1 would move every mean), at
    tests/test_gpu_batchnorm_training.py's bars"""
    from tests.test_gpu_batchnorm_training import POOL_ATOL, _fused as bn_fused
    rep = bn_fused(PIX, PARTIAL_B, 300, graph=graph, probe=True, capacity=PARTIAL_C)
    print("batch norm capacity 8, B = 5: path %s; critic list checked at the device's TD: %s at B, %s back at capacity; back at capacity %s" % (
        rep["path"], rep.get("critic_grads_checked_at_device_td", False), rep["back"].get("critic_grads_checked_at_device_td", False),
        _figures(rep["back"])))
    for i in (1, 2, 3):
        assert rep["back"]["err_pool%d" % i] < POOL_ATOL


@pytest.mark.parametrize("graph", [True, False], ids=["graph-replay", "eager"])
@pytest.mark.parametrize("shape", [PIX, LOWDIM], ids=["16x16x6", "low-dimensional"])
def test_dropout_masks_follow_the_row_not_the_capacity(shape, graph):
    """--use-dropout: the oracle draws the masks of the count the device is at (every C-row and B-row step before the checked one is a
    training-mode forward) and of row b at pitch `units`, whatever the capacity"""
    _fused("DDPG --use-dropout", shape, PARTIAL_C, PARTIAL_B, graph, pixel=len(shape) == 5, use_dropout=True)


@pytest.mark.parametrize("share", [True, False], ids=["shared-trunk", "own-trunks"])
def test_naf_dropout_masks_follow_the_row_not_the_capacity(share):
    """the NAF step with --use-dropout at (8, 5): the oracle draws the masks of the count the device is at, row b at pitch `units`"""
    from tests.test_gpu_naf import naf_fused_step_against_f64_oracle
    got = naf_fused_step_against_f64_oracle(PIX, PARTIAL_B, share, rows=300, probe=True, optimiser=ADAM[0], optimiser_args=ADAM[1],
                                            hidden=[100, 50] if share else [32, 16], use_dropout=True, capacity=PARTIAL_C)
    print("NAF --use-dropout share=%s capacity 8, B = 5: path %s" % (share, got))
    assert got == ("heads" if share else "gemm")          # (naf_mlp_kernel knows no masks: tests/test_gpu_dropout.py)


def test_naf_batch_norm_moments_are_taken_over_the_rows_of_the_batch():
    """the NAF step with --use-batch-norm at (8, 5), the gradient list at batch norm's 5e-5 (tests/test_gpu_batchnorm.py)"""
    from tests.test_gpu_naf import naf_fused_step_against_f64_oracle
    got = naf_fused_step_against_f64_oracle(PIX, PARTIAL_B, True, rows=300, probe=True, use_batch_norm=True, grad_rel=5e-5, capacity=PARTIAL_C)
    print("NAF --use-batch-norm capacity 8, B = 5: path %s" % got)


# ---- 7. inference of the variants' networks at 1 < B < C ---------------------------------------------------------------------------
@pytest.mark.parametrize("C,B", INFER)
def test_forward_gaussian_uses_the_statistics_of_its_own_rows(C, B):
    """a --soft-actor-critic actor's head (m, log sigma) on B states behind a C-row call, with the batch's statistics and with each
    row's own, at tests/test_gpu_sac.py's 1e-5 against tests/sac_np.py's networks"""
    from tests import sac_np as S
    from tests.test_gpu_sac import _agent as sac_agent, _ref as sac_ref
    A = 2
    agent = sac_agent(PIX, C, True, A)
    big, small = _states(PIX, C, 21)[0], _states(PIX, B, 22)[0]
    try:
        ref = sac_ref(agent, PIX, True, A)
        for each in (False, True):
            agent.actor.forward_gaussian(big, each=each)
            m, ls = agent.actor.forward_gaussian(small, each=each)
            if each:
                want = np.concatenate([ref.actor.forward(small[i:i + 1], training=False)["out"] for i in range(B)], axis=0)
            else:
                want = ref.actor.forward(small, training=False)["out"]
            assert m.shape == ls.shape == (B, A)
            assert np.abs(m - want[:, :A]).max() <= 1e-5 and np.abs(ls - S.log_std(want[:, A:])).max() <= 1e-5, each
            agent.actor.forward(big) if not each else agent.actor.actions_given(big)
            a = agent.actor.forward(small) if not each else agent.actor.actions_given(small)
            assert np.abs(a - np.tanh(want[:, :A])).max() <= 1e-5, each
    finally:
        agent.close()


@pytest.mark.parametrize("C,B", INFER)
@pytest.mark.parametrize("kind", ["distributional", "quantile"])
def test_a_distribution_critics_forward_uses_its_own_rows(kind, C, B):
    """CriticNetwork.forward of a categorical / a quantile critic on B rows behind a C-row call: Q from dist_expect / quant_expect over
    B rows, at the bar the variant's own test holds forward to (1e-5 x max(1, max |z|); tests.quant_np.bar('q'))"""
    if kind == "distributional":
        from tests import dist_np as W
        from tests.test_gpu_distributional import _build
        case = W.case_of("A2-B8-N51-sgd")
        head = W.dist_of(case)
        bar = W.ATOL * W.zmax_of(case)
    else:
        from tests import quant_np as W
        from tests.test_gpu_quantile import _build
        case = W.case_of("A2-B8-N25-d0-sgd")
        head = W.quant_of(case)
        bar = W.bar("q")
    shape, A = W.SHAPES[case[1]], case[2]
    specs, P, episodes, _idxs, _b = W.case_inputs(case)
    agent = _build(shape, B, A, W.hyper_of(case), head, P, episodes, capacity=C)
    big, small = _states(shape, C, 31), _states(shape, B, 32)
    try:
        agent.critic.forward(big[0], big[1])
        got = agent.critic.forward(small[0], small[1])
    finally:
        agent.close()
    ref = W.restatement(specs, P, head, np.float64, W.hyper_of(case), case[8], case[9], case[10])
    c = ref.critic.forward(small[0], action=small[1], training=False)
    if kind == "distributional":
        want = (W.softmax(c["out"])[0] * W.support(*head)[0]).sum(axis=1, keepdims=True)
    else:
        want = c["out"].mean(axis=1, keepdims=True)
    print("%s critic forward, %d rows behind %d: max |Q - restated| %.2e (bar %.2e), Q spans %.3f" % (kind, B, C, np.abs(got - want).max(), bar, np.ptp(want)))
    assert got.shape == (B, 1) and np.abs(got - want).max() < bar and np.ptp(want) > 0.05
