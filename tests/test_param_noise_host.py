"""Parameter-space exploration noise (--param-noise-stddev; include/cartpolepp_abi.h, cpp_ddpg_set_param_noise), everything that needs no
GPU: the reader of the flags and its refusals, the ABI's names, the draw's moments, the training loop's begin_episode hook -- and the power
of the bars tests/test_gpu_param_noise.py holds the device to: each planted fault of tests/param_noise_np.py, switched on in the float32
twin that stands in for the device, leaves at least one of them.

Smallest factor by which a fault leaves its bar (test_every_planted_fault_leaves_a_bar; three faults break a bit comparison, which has no
factor): 5.5e5, `adapt_on_current_copy` at alpha 1.5 -- the copy's step is half as large again, against bars of sigma 4e-6 + 2^-24 |pt|.  The
other perturbation faults leave by 1.1e6 to 1.6e6, the two distance faults by 1.6e7 and 5.4e7."""
import io
import os
import re

import numpy as np
import pytest

from tests import param_noise_np as PN

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("cpp_ddpg_set_param_noise", "cpp_ddpg_param_noise_resample", "cpp_ddpg_param_noise_status", "cpp_ddpg_param_noise_state",
               "cpp_ddpg_last_param_noise")
FLAG_KEYS = ("param_noise_stddev", "param_noise_target", "param_noise_adapt", "param_noise_adapt_rounds", "param_noise_seed")


def _parse(*argv):
    from cartpoleplusplus_amd import ddpg_cartpole as D
    return D, D.build_parser().parse_args(list(argv))


# ---- 1. the flags
def test_the_options_are_absent_unless_given_and_the_defaults_are_the_issues():
    D, o = _parse()
    for key in FLAG_KEYS:
        assert not hasattr(o, key), key
    assert D.param_noise(o) is None
    D, o = _parse("--param-noise-stddev", "0.2")
    assert D.param_noise(o) == {"stddev": float(np.float32(0.2)), "target": float(np.float32(0.1)), "adapt": float(np.float32(1.01)), "rounds": 1, "seed": 0}
    D, o = _parse("--param-noise-stddev", "0", "--param-noise-target", "0.3", "--param-noise-adapt", "1", "--param-noise-adapt-rounds", "4",
                  "--param-noise-seed", str(2 ** 64 - 1))
    assert D.param_noise(o) == {"stddev": 0.0, "target": float(np.float32(0.3)), "adapt": 1.0, "rounds": 4, "seed": 2 ** 64 - 1}


def test_default_opts_leave_the_feature_off():
    from cartpoleplusplus_amd import ddpg_cartpole as D
    d = D.default_opts()
    for key in FLAG_KEYS:
        assert hasattr(d, key) and getattr(d, key) is None, key
    assert D.param_noise(d) is None
    assert D.param_noise(D.default_opts(param_noise_stddev=0.05))["stddev"] == float(np.float32(0.05))


@pytest.mark.parametrize("argv,word", [
    (("--param-noise-target", "0.2"), "--param-noise-target needs --param-noise-stddev"),
    (("--param-noise-adapt", "1.5"), "--param-noise-adapt needs --param-noise-stddev"),
    (("--param-noise-adapt-rounds", "2"), "--param-noise-adapt-rounds needs --param-noise-stddev"),
    (("--param-noise-seed", "3"), "--param-noise-seed needs --param-noise-stddev"),
    (("--param-noise-stddev", "-0.1"), "not a standard deviation >= 0"),
    (("--param-noise-stddev", "nan"), "not a finite number"),
    (("--param-noise-stddev", "0.1", "--param-noise-target", "0"), "not a distance > 0"),
    (("--param-noise-stddev", "0.1", "--param-noise-target", "inf"), "not a finite number"),
    (("--param-noise-stddev", "0.1", "--param-noise-adapt", "0.99"), "not a factor >= 1"),
    (("--param-noise-stddev", "0.1", "--param-noise-adapt-rounds", "0"), "not a whole number in [1, 64]"),
    (("--param-noise-stddev", "0.1", "--param-noise-adapt-rounds", "65"), "not a whole number in [1, 64]"),
    (("--param-noise-stddev", "0.1", "--param-noise-seed", "-1"), "not in [0, 2^64)"),
    (("--param-noise-stddev", "0.1", "--param-noise-seed", str(2 ** 64)), "not in [0, 2^64)"),
    (("--param-noise-stddev", "0.1", "--soft-actor-critic"), "--soft-actor-critic (its policy explores by itself)"),
    (("--param-noise-stddev", "0.1", "--use-raw-pixels", "--use-batch-norm"), "cannot be combined with --use-batch-norm")])
def test_the_refusals_of_the_reader(argv, word):
    D, o = _parse(*argv)
    with pytest.raises(SystemExit) as e:
        D.param_noise(o)
    assert word in str(e.value), str(e.value)


def test_the_naf_learner_does_not_know_the_options():
    from cartpoleplusplus_amd import naf_cartpole as NAF
    for flag in ("--param-noise-stddev", "--param-noise-target", "--param-noise-adapt", "--param-noise-adapt-rounds", "--param-noise-seed"):
        with pytest.raises(SystemExit):
            NAF.build_parser().parse_args([flag, "1"])
    for key in FLAG_KEYS:
        assert not hasattr(NAF.default_opts(), key)


# ---- 2. the ABI
def test_the_entry_points_are_declared_bound_and_exported():
    import ctypes
    from cartpoleplusplus_amd import _lib
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "cartpolepp_abi.h")).read(), flags=re.S)
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for s in NEW_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % s, header), s
        assert s in _lib.SIGNATURES and hasattr(raw, s), s
    names = [_lib.lib.cpp_prof_kernel_name(k).decode() for k in range(_lib.lib.cpp_prof_num_kernels())]
    assert names[-1] == "param_noise" and names.count("param_noise") == 1      # (appended: every earlier id keeps its name)
    # every entry point cites the lines of the reference it extends
    full = open(os.path.join(ROOT, "include", "cartpolepp_abi.h")).read()
    for s in NEW_SYMBOLS:
        comment = full[:full.index("int %s(" % s)].rsplit("/*", 1)[1]
        assert "ddpg_cartpole.py:" in comment or "util.py:" in comment, s


# ---- 3. the draw
def test_the_moments_of_the_draw_over_2_16_elements():
    """65536 standard normals: the mean within 4 / sqrt(N) of 0, the variance within 4 sqrt(2 / N) of 1 (four standard errors of each),
    and no value beyond Box-Muller's reach on 24-bit uniforms, sqrt(-2 log 2^-24) = 5.77"""
    N = 1 << 16
    for seed, n in ((0, 0), (0x5EEDF00D12345, 1), (7, 1 << 32)):
        for dt in (np.float64, np.float32):
            z = PN.normals(seed, n, N, dt).astype(np.float64)
            assert abs(z.mean()) < 4.0 / np.sqrt(N), (seed, n, z.mean())
            assert abs(z.var() - 1.0) < 4.0 * np.sqrt(2.0 / N), (seed, n, z.var())
            assert np.abs(z).max() <= 5.77 and np.isfinite(z).all()
    a, b = PN.normals(3, 5, 64), PN.normals(3, 6, 64)
    assert not np.array_equal(a, b) and not np.array_equal(a, PN.normals(4, 5, 64))
    assert np.array_equal(PN.normals(3, 5, 64)[10:20], PN.normals(3, 5, 10, first=10))      # (the counter is the element's index)
    assert not np.array_equal(PN.normals(3, 0, 64), PN.normals(3, 1 << 32, 64))


# ---- 4. the power of the bars.  A stand-in for the device: the float32 twin, with a fault or without
N_PLAIN, N_TAIL = (1 << 16) + 37, 6          # elements beyond 2^16, a count that is no multiple of 4, a layer norm's tail
SEED, DELTA, ALPHA, SIGMA0 = 0x5EEDF00D12345, 0.1, 1.5, 0.05
STATES = 9


def _scenario():
    rng = np.random.default_rng(11)
    p = rng.normal(0, 0.3, N_PLAIN + N_TAIL).astype(np.float32)
    p[N_PLAIN:N_PLAIN + N_TAIL // 2] = 1.0
    X = rng.normal(0, 1, (STATES, 7)).astype(np.float64)
    return p, X


def _actions_of(p, X):
    """a small tanh policy over the head of the flat vector AND its end (so that every region of it moves the actions)"""
    def policy(v):
        v = np.asarray(v, np.float64)
        W = v[:14].reshape(7, 2) + v[N_PLAIN - 14:N_PLAIN].reshape(7, 2)
        return np.tanh(X @ W).astype(np.float32)
    return lambda pt: (policy(p), policy(pt))


def _run(fault):
    """the stand-in's resamples, each held to every bar: a first one without a batch, two measured ones, and -- the count set to 2^32 - 1 --
    two more across the word boundary.  Returns the worst ratio per bar."""
    p, X = _scenario()
    dev = PN.Restated(SIGMA0, DELTA, ALPHA, SEED, np.float32, fault)
    worst = {}
    for k, measured in enumerate((False, True, True, None, True, True)):
        if measured is None:
            dev.n = (1 << 32) - 1
            continue
        before = (dev.sigma, dev.d, dev.n)
        pt = dev.resample(p, N_PLAIN, _actions_of(p, X) if measured else None)
        r = PN.resample_ratios(pt, (dev.sigma, dev.d, dev.n, dev.adapted), p, N_PLAIN, before, SEED, DELTA, ALPHA, dev.last if measured else None)
        if measured:
            assert PN.decided(dev.d, DELTA, dev.last[0].size), (k, dev.d)
        for key, v in r.items():
            worst[key] = max(worst.get(key, 0.0), v)
    return worst


def test_the_float32_twin_is_inside_every_bar():
    w = _run(None)
    assert set(w) == {"perturbation", "count", "adapted_flag", "left_alone", "distance", "sigma"}
    assert max(w.values()) <= 1.0, w


@pytest.mark.parametrize("fault", PN.FAULTS)
def test_every_planted_fault_leaves_a_bar(fault):
    w = _run(fault)
    assert max(w.values()) > 1e3, (fault, w)
    print("%s: leaves %s by %.3g" % (fault, max(w, key=w.get), max(w.values())))


def test_the_faults_are_the_issues_ten():
    assert len(PN.FAULTS) == 10 and len(set(PN.FAULTS)) == 10


def test_a_sigma_of_zero_is_a_bit_copy_and_the_bars_say_so():
    p, _X = _scenario()
    pt = PN.perturbed(p, 0.0, SEED, 3, N_PLAIN, np.float32)
    assert np.array_equal(pt.view(np.uint32), p.view(np.uint32)) and PN.perturbation_ratio(pt, p, 0.0, SEED, 3, N_PLAIN) == 0.0
    off = pt.copy()
    off[5] = np.nextafter(off[5], np.float32(9))
    assert PN.perturbation_ratio(off, p, 0.0, SEED, 3, N_PLAIN) == float("inf")


# ---- 5. the training loop's hook
class _Env(object):
    def __init__(self, episode_len, log):
        self.t, self.n, self.log = 0, episode_len, log

    def reset(self):
        self.t = 0
        self.log.append("reset")
        return np.zeros(3, np.float32)

    def step(self, action):
        self.t += 1
        return np.full(3, self.t, np.float32), 1.0, self.t >= self.n, {}


class _Agent(object):
    def __init__(self, episode_len, log):
        import collections

        class Mem(object):
            def __init__(self):
                self.rows, self.stats = 0, collections.Counter()

            def add_episode(self, s0, seq):
                self.rows += len(seq)

            def size(self):
                return self.rows

            def current_stats(self):
                return {}
        self.env, self.replay_memory, self.evals = _Env(episode_len, log), Mem(), 0

    def run_eval(self, n, add_noise=False):
        self.evals += n


def _opts(**kw):
    import types
    o = types.SimpleNamespace(dont_do_rollouts=False, replay_memory_burn_in=10, async_rollouts=False)
    o.__dict__.update(kw)
    return o


def test_the_training_loop_calls_begin_episode_before_every_reset_and_never_without_one():
    from cartpoleplusplus_amd.training_loop import TrainingLoop, play_episode
    log = []
    agent = _Agent(4, log)
    loop = TrainingLoop(agent, _opts(), act=lambda s: np.zeros((1, 2), np.float32), train=lambda b, n: [0.0], out=io.StringIO(),
                        begin_episode=lambda: log.append("begin"))
    loop.run(max_num_actions=21, max_run_time=0, batch_size=8, batches_per_step=1, saver_util=None)
    assert loop.iterations == 6 and log == ["begin", "reset"] * 6      # (the evaluation episodes are the agent's: none here)
    # the default: no hook, the loop of before
    log2 = []
    loop = TrainingLoop(_Agent(4, log2), _opts(), act=lambda s: np.zeros((1, 2), np.float32), train=lambda b, n: [0.0], out=io.StringIO())
    loop.run(21, 0, 8, 1, None)
    assert log2 == ["reset"] * 6
    log3 = []
    play_episode(_Env(2, log3), lambda s: 0)
    assert log3 == ["reset"]


def test_the_rollout_thread_calls_begin_episode_too():
    from cartpoleplusplus_amd.training_loop import TrainingLoop
    log = []
    agent = _Agent(5, log)
    loop = TrainingLoop(agent, _opts(async_rollouts=True), act=lambda s: np.zeros((1, 2), np.float32), train=lambda b, n: [0.0],
                        out=io.StringIO(), begin_episode=lambda: log.append("begin"))
    loop.run(max_num_actions=30, max_run_time=0, batch_size=8, batches_per_step=1, saver_util=None)
    assert len(log) >= 12 and all(log[i] == ("begin", "reset")[i % 2] for i in range(len(log) - len(log) % 2))


def test_begin_episode_is_a_no_op_for_an_agent_without_the_feature():
    from cartpoleplusplus_amd import ddpg_cartpole as D
    agent = object.__new__(D.DeepDeterministicPolicyGradientAgent)      # (no device: nothing may be touched)
    assert agent.begin_episode() is None
    agent.param_noise = None
    assert agent.begin_episode() is None and agent.checkpoint_extras.__func__ is D.DeepDeterministicPolicyGradientAgent.checkpoint_extras
