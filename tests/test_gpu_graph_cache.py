"""The cached step graphs of the DDPG and NAF training entry points (rt_ddpg.cpp / rt_naf.cpp: StepGraph) against the same calls as
plain stream launches.  Every entry point keeps one captured graph per key (batch size, minibatches per step, sampling seed, replay
memory, communicator) and everything else a captured launch holds by value (the optimiser's rule, target policy smoothing, the memory's
random shift) must drop it: agent G takes the default path (capture at a new key, replay at a held one), agent E runs with the
context's profiler on, which forces every call onto the eager path.  Same seeds, same calls: same parameters.

Only the public Python surface is used, so the file is independent of how the caches are kept.

Measured on the commit before the caches became one type: the largest difference G against E was 0 in every case (bit for bit) but
`test_ddpg_half_steps_after_a_replayed_fused_step` (see there), so every comparison is np.array_equal."""
import ctypes
import json

import numpy as np
import pytest

from tests.helpers import FakeEnv, make_pair

pytestmark = pytest.mark.gpu

PIXEL, LOWDIM = (16, 16, 3, 2, 3), (2, 2, 7)
ROWS = 150


def _abi():
    from cartpoleplusplus_amd import _lib
    return _lib, _lib.lib, _lib.check, _lib.ptr


def _second_memory(agent, rows=ROWS, seed=23):
    from cartpoleplusplus_amd import replay_memory
    rm = agent.replay_memory
    other = replay_memory.ReplayMemory(rm.buffer_size, rm.state_shape, rm.action_dim)
    other.fill_synthetic(rows, seed=seed)
    return other


def _ddpg_agent(shape, maxB=8):
    agent, _ref, _ = make_pair(shape, maxB, len(shape) == 5, replay_size=300)
    agent.replay_memory.fill_synthetic(ROWS, seed=11)
    return agent


def _naf_agent(shape, maxB=8):
    from cartpoleplusplus_amd import naf_cartpole as F
    kw = dict(use_raw_pixels=True, render_height=shape[0], render_width=shape[1], num_cameras=shape[3], action_repeats=shape[4]) \
        if len(shape) == 5 else dict(use_raw_pixels=False, action_repeats=shape[0])
    F.set_opts(F.default_opts(batch_size=maxB, replay_memory_size=300, share_input_state_representation=len(shape) == 5,
                              optimiser="Adam", optimiser_args=json.dumps({"learning_rate": 0.001}), **kw))
    agent = F.NormalizedAdvantageFunctionAgent(FakeEnv(shape))
    agent.initialise_variables(seed=4)
    agent.post_var_init_setup()
    agent.replay_memory.fill_synthetic(ROWS, seed=9)
    return agent


def _graph_and_eager(make_agent, script):
    """[what `script(agent)` returns + the networks' parameters] for agent G (cached graphs) and agent E (every call eager)"""
    _lib = _abi()[0]
    out = []
    for eager in (False, True):
        agent = make_agent()
        ctx = _lib.default_context()
        try:
            ctx.prof_enable(eager)
            got = list(script(agent) or [])
            ctx.sync()
            out.append(got + [n.get_params() for n in agent.networks()])
        finally:
            ctx.prof_enable(False)
            agent.close()
    return out


def _assert_equal(res, what=""):
    G, E = res
    assert len(G) == len(E)
    worst = 0.0
    for x, y in zip(G, E):
        x, y = np.asarray(x), np.asarray(y)
        assert x.shape == y.shape
        if x.size:
            worst = max(worst, float(np.abs(x.astype(np.float64) - y.astype(np.float64)).max()))
    print("graph vs eager %s: largest difference %.3e" % (what, worst))
    for x, y in zip(G, E):
        assert np.array_equal(np.asarray(x), np.asarray(y)), worst
    for x in G:
        assert np.all(np.isfinite(np.asarray(x, dtype=np.float64)))


# ---------------------------------------------------------------------------------------------------------------------
# 1. the DDPG fused step: every component of the key, and every setter whose values the captured launches hold
# ---------------------------------------------------------------------------------------------------------------------
def ddpg_fused_script(agent, pixel=True):
    _lib, lib, check, ptr = _abi()
    t = agent.trainer
    state = {"B": 8, "n": 2, "seed": 1234, "rm": agent.replay_memory}
    others = []

    def step(times, **change):
        state.update(change)
        for _ in range(times):
            check(lib.cpp_ddpg_train_step(t.handle, state["rm"].handle, state["B"], state["n"], None, state["seed"]))
    try:
        step(3)                          # capture, replay, replay
        step(2, n=3)
        step(2, B=4)
        step(2, B=8, n=2)                # (one graph per entry point: the first key again is a new capture)
        step(2, seed=77)
        check(lib.cpp_ddpg_set_optimiser(t.handle, _lib.CPP_OPT_ADAM, 0.0, 0.9, 0.999, 1e-8))
        t.optimiser_kind = _lib.CPP_OPT_ADAM
        step(2)
        t.set_target_smoothing(0.2, 0.5, 9)
        step(2)
        t.set_target_smoothing(0.0, 0.0, 9)
        step(2)
        if pixel:                        # (the memory takes a new uid with each setting)
            agent.replay_memory.enable_random_shift(2, seed=5)
            step(2)
            agent.replay_memory.enable_random_shift(0)
            step(2)
        others.append(_second_memory(agent))
        step(2, rm=others[0])
        step(2, rm=agent.replay_memory)
        agent.replay_memory.fill_synthetic(250, seed=11)      # (the sampler's range is a device word: the graph stays)
        step(2)
        slots = t.get_optimiser_state()
        return [slots["m"], slots["v"], slots["step"], t.last_stats()]
    finally:
        _lib.default_context().sync()
        for o in others:
            o.close()


@pytest.mark.parametrize("shape", [PIXEL, LOWDIM], ids=["pixel", "low-dimensional"])
def test_ddpg_fused_step_recaptures_whenever_a_captured_value_changes(shape):
    pixel = len(shape) == 5
    res = _graph_and_eager(lambda: _ddpg_agent(shape), lambda a: ddpg_fused_script(a, pixel))
    _assert_equal(res, "ddpg fused step")
    assert res[0][2][0] > 0 and np.abs(res[0][0]).max() > 0          # (Adam ran: counts and slots moved)


# ---------------------------------------------------------------------------------------------------------------------
# 2. DDPG on host-drawn rows
# ---------------------------------------------------------------------------------------------------------------------
def _row_draws(count, B, rows=ROWS, seed=5):
    rng = np.random.default_rng(seed + B)
    return [np.ascontiguousarray(rng.integers(0, rows, B), dtype=np.int32) for _ in range(count)]


def test_ddpg_train_rows_across_batch_sizes_and_memories():
    def script(agent):
        _lib, lib, check, ptr = _abi()
        t, other = agent.trainer, _second_memory(agent)
        try:
            for rm, B, times in ((agent.replay_memory, 8, 3), (agent.replay_memory, 4, 2), (agent.replay_memory, 8, 2), (other, 8, 2),
                                 (agent.replay_memory, 8, 2)):
                for idxs in _row_draws(times, B):
                    check(lib.cpp_ddpg_train_rows(t.handle, rm.handle, B, ptr(idxs)))
                check(lib.cpp_ddpg_update_targets(t.handle))
            return [t.last_stats()]
        finally:
            _lib.default_context().sync()
            other.close()
    _assert_equal(_graph_and_eager(lambda: _ddpg_agent(PIXEL), script), "ddpg train_rows")


# ---------------------------------------------------------------------------------------------------------------------
# 3. NAF: the four cached entry points
# ---------------------------------------------------------------------------------------------------------------------
def naf_script(agent, entry):
    _lib, lib, check, ptr = _abi()
    h, other, losses = agent.naf.handle, _second_memory(agent), []
    try:
        for rm, B, times in ((agent.replay_memory, 8, 3), (agent.replay_memory, 4, 2), (agent.replay_memory, 8, 2), (other, 8, 2),
                             (agent.replay_memory, 8, 2)):
            for idxs in _row_draws(times, B):
                loss = ctypes.c_float()
                if entry == "train_step":
                    check(lib.cpp_naf_train_step(h, rm.handle, B, 2, None, 1234))
                elif entry == "train_rows":
                    check(lib.cpp_naf_train_rows(h, rm.handle, B, ptr(idxs), ctypes.byref(loss)))
                elif entry == "train_rows_async":
                    ticket = ctypes.c_uint64()
                    check(lib.cpp_naf_train_rows_async(h, rm.handle, B, ptr(idxs), ctypes.byref(ticket)))
                    check(lib.cpp_naf_loss_wait(h, ticket.value, ctypes.byref(loss)))
                else:
                    check(lib.cpp_naf_sample_and_compute(h, rm.handle, B, 1234))
                    check(lib.cpp_naf_apply_gradients(h, 1.0))
                losses.append(loss.value)
        slots = agent.naf.get_optimiser_state()
        return [np.array(losses, np.float32), slots["m"], slots["v"], agent.naf.last_stats()]
    finally:
        _lib.default_context().sync()
        other.close()


@pytest.mark.parametrize("entry", ["train_step", "train_rows", "train_rows_async", "sample_and_compute"])
def test_naf_entry_points_across_batch_sizes_and_memories(entry):
    res = _graph_and_eager(lambda: _naf_agent(PIXEL), lambda a: naf_script(a, entry))
    _assert_equal(res, "naf " + entry)
    assert res[0][3][2] == 0          # (check_numerics never fired)


def test_naf_fused_step_low_dimensional():
    _assert_equal(_graph_and_eager(lambda: _naf_agent(LOWDIM), lambda a: naf_script(a, "train_step")), "naf low-dimensional")


# ---------------------------------------------------------------------------------------------------------------------
# 4. the data-parallel step at world size 1
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_comm", [True, False], ids=["communicator", "no-communicator"])
@pytest.mark.parametrize("which,mode", [("ddpg", "default"), ("ddpg", "overlap"), ("ddpg", "periodic-2"), ("naf", "default"),
                                        ("naf", "periodic-2")])
def test_data_parallel_step_at_world_size_one(which, mode, with_comm):
    from cartpoleplusplus_amd.distributed import Communicator, NativeLearner
    status = []

    def script(agent):
        _lib = _abi()[0]
        comm = Communicator.single(_lib.default_context()) if with_comm else None
        try:
            for B, times in ((8, 3), (4, 2), (8, 2)):
                learner = NativeLearner(agent, B, 1234, comm, sync_every=2 if mode == "periodic-2" else 1, overlap=mode == "overlap")
                for _ in range(times):
                    learner.train_step(3)
                status.append(learner.dp_status())
            return []
        finally:
            _lib.default_context().sync()
            if comm is not None:
                comm.close()
    make = (lambda: _ddpg_agent(PIXEL)) if which == "ddpg" else (lambda: _naf_agent(PIXEL))
    _assert_equal(_graph_and_eager(make, script), "%s data-parallel %s" % (which, mode))
    graph_runs, eager_runs = status[:3], status[3:]
    if mode == "default":
        assert [s["path"] for s in graph_runs] == ["hipgraph"] * 3, graph_runs       # (asked after the second call at each key)
    else:
        assert [s["path"] for s in graph_runs] == ["none"] * 3, graph_runs
    assert [s["path"] for s in eager_runs] == ["none"] * 3, eager_runs


# ---------------------------------------------------------------------------------------------------------------------
# 5. half steps and fused steps on one trainer: both use the trainer's one minibatch buffer and its two sets of sampled slots
# ---------------------------------------------------------------------------------------------------------------------
def _mixed_script(agent, order):
    _lib, lib, check, ptr = _abi()
    t, rm = agent.trainer, agent.replay_memory
    for what, times in order:
        for _ in range(times):
            if what == "half":
                check(lib.cpp_ddpg_sample_and_compute(t.handle, rm.handle, 8, 1234))
                check(lib.cpp_ddpg_apply_gradients(t.handle, 1.0))
            else:
                check(lib.cpp_ddpg_train_step(t.handle, rm.handle, 8, 2, None, 1234))
    return [t.last_stats()]


def test_ddpg_half_steps_around_fused_steps():
    order = (("half", 2), ("fused", 3), ("half", 2))
    _assert_equal(_graph_and_eager(lambda: _ddpg_agent(PIXEL), lambda a: _mixed_script(a, order)), "ddpg half / fused / half")


def test_ddpg_half_steps_after_a_replayed_fused_step():
    """The fused step's graph is captured BEFORE the half steps leave a presampled minibatch behind: the fused step that follows them is
    a replay, and it overwrites the slots that minibatch lives in exactly as the eager step does -- the next half step must draw again.

    This is the one case that fails on the commit before the caches became one type: the replay branch of cpp_ddpg_train_step did not
    reset the half steps' `pre_variant` as the eager body does, so the half step behind it consumed slots the fused step had written
    (measured there: G against E differ by up to 4.1e-1 over everything compared here, the parameters of the four networks and the
    loss and gradient norms of the last call; with the reset in place they agree bit for bit, like every other case of this file)."""
    order = (("fused", 2), ("half", 2), ("fused", 1), ("half", 2))
    _assert_equal(_graph_and_eager(lambda: _ddpg_agent(PIXEL), lambda a: _mixed_script(a, order)), "ddpg fused / half / replayed fused / half")


# ---------------------------------------------------------------------------------------------------------------------
# 6. --use-dropout: every entry point assembles or captures the step on its own, and each must advance every dropout counter exactly
# once per training-mode forward -- a replay that drew the masks of its capture's count, or an entry point that counted twice, leaves
# the eager sequence of masks at once.  (tests/test_gpu_dropout.py pins the eager counts to the float64 oracle; here the replays are
# pinned to the eager counts, bit for bit.)
# ---------------------------------------------------------------------------------------------------------------------
def _ddpg_dropout_agent(shape, maxB=8):
    agent, _ref, _ = make_pair(shape, maxB, len(shape) == 5, replay_size=300, use_dropout=True)
    agent.replay_memory.fill_synthetic(ROWS, seed=11)
    return agent


def _naf_dropout_agent(shape, share, maxB=8):
    from tests.test_gpu_naf import make_naf
    agent, _ref, _ = make_naf(shape, maxB, share, "Adam", {"learning_rate": 0.001}, seed=4, replay_size=300, use_dropout=True)
    agent.replay_memory.fill_synthetic(ROWS, seed=9)
    return agent


_DP_PATHS = []          # the data-parallel step's path per learner, in call order (agent G's two, then agent E's two)


def _dp_steps(agent, B=8):
    from cartpoleplusplus_amd.distributed import NativeLearner
    for sync_every in (1, 2):
        learner = NativeLearner(agent, B, 1234, None, sync_every=sync_every)
        for _ in range(2):
            learner.train_step(3)
        _DP_PATHS.append(learner.dp_status()["path"])


def _assert_dp_paths():
    """agent G replayed a captured graph at sync_every 1 (at 2, without a communicator, it may hold on to that graph or launch eagerly:
    not asserted); agent E never did"""
    paths = list(_DP_PATHS)
    del _DP_PATHS[:]
    assert len(paths) == 4 and paths[0] == "hipgraph" and paths[2:] == ["none", "none"], paths


def ddpg_dropout_script(agent):
    _lib, lib, check, ptr = _abi()
    t, rm, B = agent.trainer, agent.replay_memory, 8

    def fused(times, n):
        for _ in range(times):
            check(lib.cpp_ddpg_train_step(t.handle, rm.handle, B, n, None, 1234))
    fused(3, 2)                          # capture, replay, replay
    fused(2, 3)
    for idxs in _row_draws(3, B):
        check(lib.cpp_ddpg_train_rows(t.handle, rm.handle, B, ptr(idxs)))
    check(lib.cpp_ddpg_update_targets(t.handle))
    for _ in range(2):
        check(lib.cpp_ddpg_sample_and_compute(t.handle, rm.handle, B, 1234))
        check(lib.cpp_ddpg_apply_gradients(t.handle, 1.0))
    _dp_steps(agent, B)
    fused(2, 2)
    return [t.last_stats(), agent.actor.get_grads(), agent.critic.get_grads()]


def naf_dropout_script(agent):
    _lib, lib, check, ptr = _abi()
    h, rm, B, losses = agent.naf.handle, agent.replay_memory, 8, []

    def fused(times, n):
        for _ in range(times):
            check(lib.cpp_naf_train_step(h, rm.handle, B, n, None, 1234))
    fused(3, 2)
    fused(2, 3)
    for idxs in _row_draws(3, B):
        loss = ctypes.c_float()
        check(lib.cpp_naf_train_rows(h, rm.handle, B, ptr(idxs), ctypes.byref(loss)))
        losses.append(loss.value)
    for idxs in _row_draws(3, B, seed=6):
        loss, ticket = ctypes.c_float(), ctypes.c_uint64()
        check(lib.cpp_naf_train_rows_async(h, rm.handle, B, ptr(idxs), ctypes.byref(ticket)))
        check(lib.cpp_naf_loss_wait(h, ticket.value, ctypes.byref(loss)))
        losses.append(loss.value)
    for _ in range(2):
        check(lib.cpp_naf_sample_and_compute(h, rm.handle, B, 1234))
        check(lib.cpp_naf_apply_gradients(h, 1.0))
    _dp_steps(agent, B)
    fused(2, 2)
    slots = agent.naf.get_optimiser_state()
    return [np.array(losses, np.float32), slots["m"], slots["v"], agent.naf.last_stats(), agent.naf.get_grads()]


@pytest.mark.parametrize("shape", [PIXEL, LOWDIM], ids=["pixel", "low-dimensional"])
def test_ddpg_entry_points_with_dropout(shape):
    del _DP_PATHS[:]
    res = _graph_and_eager(lambda: _ddpg_dropout_agent(shape), ddpg_dropout_script)
    _assert_equal(res, "ddpg --use-dropout, every entry point")
    _assert_dp_paths()


@pytest.mark.parametrize("shape,share", [(PIXEL, True), (PIXEL, False), (LOWDIM, True), (LOWDIM, False)],
                         ids=["pixel-shared", "pixel-own-trunks", "low-dimensional-shared", "low-dimensional-own-trunks"])
def test_naf_entry_points_with_dropout(shape, share):
    del _DP_PATHS[:]
    res = _graph_and_eager(lambda: _naf_dropout_agent(shape, share), naf_dropout_script)
    _assert_equal(res, "naf --use-dropout, every entry point")
    _assert_dp_paths()
    assert res[0][3][2] == 0          # (check_numerics never fired)
