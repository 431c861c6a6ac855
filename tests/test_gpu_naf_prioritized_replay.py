"""Prioritized replay for the NAF learner (csrc/rt_naf.cpp, the weighted instances of the NAF head kernels in csrc/gemm.hip; semantics
in include/cartpolepp_abi.h): one graph-replayed prioritized minibatch against the weighted float64 reference (tests/naf_per_np.py) on
every head path, the weight as the only difference, the literal loop against the fused step, a non-finite minibatch that must leave
the parameters and the tree alone, reproducibility and the training loop."""
import ctypes
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle import ddpg_np as O
from oracle import naf_np as N
from tests import per_np as P
from tests.helpers import FakeEnv, assert_flat_close
from tests.naf_per_np import WeightedNAF

pytestmark = pytest.mark.gpu
ATOL = 1e-5
LOWDIM = (2, 2, 7)
PER = dict(prioritized_replay=True, priority_alpha=0.6, priority_beta=0.4, priority_eps=1e-6)
MOMENTUM = ("Momentum", {"learning_rate": 0.01, "momentum": 0.9})


def make_naf(shape, B, share, optimiser="Momentum", optimiser_args=None, seed=0, replay_size=64, hidden=None, action_dim=2, **extra):
    """tests/test_gpu_naf.py's make_naf with options of its own (the prioritized-replay keys)"""
    from cartpoleplusplus_amd import naf_cartpole as F
    pixel = len(shape) == 5
    hidden, A = ([100, 50] if hidden is None else [int(h) for h in hidden]), int(action_dim)
    extra.setdefault("hidden_layers", ",".join(str(h) for h in hidden))
    kw = dict(batch_size=B, replay_memory_size=replay_size, share_input_state_representation=share, optimiser=optimiser,
              optimiser_args=json.dumps(optimiser_args or MOMENTUM[1]), gradient_clip=5.0)
    if pixel:
        kw.update(use_raw_pixels=True, render_height=shape[0], render_width=shape[1], num_cameras=shape[3], action_repeats=shape[4])
    else:
        kw.update(use_raw_pixels=False, action_repeats=shape[0])
    kw.update(extra)
    F.set_opts(F.default_opts(**kw))
    agent = F.NormalizedAdvantageFunctionAgent(FakeEnv(shape, A))
    agent.initialise_variables(seed=seed)
    rng = np.random.default_rng(seed + 5)
    for net in (agent.value_net, agent.naf.mu_net, agent.naf.l_net):
        p = net.get_params()
        net.set_params(p + rng.normal(0, 0.05, p.shape).astype(np.float32))
    agent.post_var_init_setup()
    p = agent.target_value_net.get_params()
    agent.target_value_net.set_params(p + rng.normal(0, 0.01, p.shape).astype(np.float32))
    skw = dict(pixel=True, H=shape[0], W=shape[1], C=int(np.prod(shape[2:]))) if pixel else dict(pixel=False, state_elems=int(np.prod(shape)))
    vspec = N.HeadSpec(1, "linear", hidden, **skw)
    if share:
        mspec = N.HeadSpec(A, "tanh", [], False, state_elems=hidden[-1], head_only=True)
        lspec = N.HeadSpec(N.num_l_values(A), "linear", [], False, state_elems=hidden[-1], head_only=True)
    else:
        mspec, lspec = N.HeadSpec(A, "tanh", hidden, **skw), N.HeadSpec(N.num_l_values(A), "linear", hidden, **skw)
    return agent, (vspec, mspec, lspec)


def params_of(agent):
    return np.concatenate([agent.value_net.get_params(), agent.naf.mu_net.get_params(), agent.naf.l_net.get_params()])


class CatSpec(object):
    def __init__(self, specs):
        self.specs = specs

    def layout(self):
        out = []
        for tag, sp in zip(("value/", "mu/", "l/"), self.specs):
            out += [(tag + n, s) for n, s in sp.layout()]
        return out


def last_rows(agent, B):
    from cartpoleplusplus_amd import _lib
    rows = np.empty(B, np.int32)
    _lib.check(_lib.lib.cpp_replay_last_indexes(agent.replay_memory.handle, B, rows.ctypes.data_as(ctypes.c_void_p)))
    return rows


def per_naf_step_against_f64_oracle(shape, B, share, rows=2500, replay_store="f16", seed=0, alpha=0.6, eps=1e-6, grad_rel=2e-5,
                                    probe=False, **naf_kw):
    """ONE hipGraph-replayed minibatch of the fused NAF step on a prioritized memory (rows drawn by priority, priorities spread over three
    decades) against WeightedNAF(float64) on the same rows, parameters and Momentum slots: w.max() == 1 and w.min() < 0.5, the loss
    mean(w td^2) at 1e-5, the pre-clip gradients at 2e-5 (the trunk's pool routes and ReLUs taken from the device, accepted only at
    rounding-level ties), the unweighted gradient far away, the priorities written (|td| + eps)^alpha (held to the oracle's td, which
    the device's matches at 1e-5 relative to max(1, |td|): the tolerance carries alpha times that), and the clipped Momentum update."""
    from cartpoleplusplus_amd import naf_cartpole as F
    from tests.helpers import device_pool_codes, device_relu_active, naf_path, pool_flips_are_near_ties, relu_flips_are_at_the_boundary
    pixel = len(shape) == 5
    agent, specs = make_naf(shape, B, share, seed=seed, replay_size=rows + 50, replay_store=replay_store, priority_alpha=alpha,
                            priority_eps=eps, **dict({k: v for k, v in PER.items() if k not in ("priority_alpha", "priority_eps")}, **naf_kw))
    path = None
    try:
        rm = agent.replay_memory
        rm.fill_synthetic(rows, seed=33 + seed)
        if probe:
            path = naf_path(agent, B, specs[0].hidden, share)
        agent.train_step(B, 1)                                    # eager pass + capture (also fills the Momentum slots)
        rm.update_priorities(np.arange(rows), np.random.default_rng(seed + 9).lognormal(0.0, 2.0, rows).astype(np.float32))
        nets = (agent.value_net, agent.naf.mu_net, agent.naf.l_net, agent.target_value_net)
        Pm = [n.get_params() for n in nets]
        opt = agent.naf.get_optimiser_state()
        agent.train_step(B, 1)                                    # hipGraph replay, rows drawn by priority
        idxs = last_rows(agent, B)
        w = rm.last_weights(B)
        assert w.max() == 1.0 and w.min() < 0.5, (w.min(), w.max())
        grads, stats = agent.naf.get_grads(), agent.naf.last_stats()
        Pn = [n.get_params() for n in nets]
        keys = np.array(sorted(set(int(r) for r in idxs)), np.int32)
        written = rm.priorities(keys)
        trunks = [agent.value_net] if share else [agent.value_net, agent.naf.mu_net, agent.naf.l_net]
        if pixel:
            codes, relu = [device_pool_codes(n, B) for n in trunks], [device_relu_active(n, B) for n in trunks]
        s1, s2 = rm.state[rm.state_1_idx[idxs]], rm.state[rm.state_2_idx[idxs]]
        hb = rm.batch(idxs=idxs)
        batch = (s1, hb.action, hb.reward, hb.terminal_mask, s2)
    finally:
        agent.close()
    vspec, mspec, lspec = specs
    ref = WeightedNAF(vspec, mspec, lspec, Pm[0], Pm[1], Pm[2], share, mspec.head_out, np.float64, gradient_clip=5.0,
                      optimiser=N.make_optimiser(*MOMENTUM))
    ref.target_value = O.Net(vspec, Pm[3], np.float64)
    ref.m = opt["m"].astype(np.float64)
    rnets = [ref.value] if share else [ref.value, ref.mu, ref.l]
    if pixel:
        for net, cd, rl in zip(rnets, codes, relu):
            net.amax_override, net.relu_override = cd, rl
    out = ref.forward_backward(batch, w=w.astype(np.float64))
    if pixel:
        for net, cd, rl, what in zip(rnets, codes, relu, ("value", "mu", "l")):
            cache = net.forward(s1, white=ref._white(net, s1), training=True)
            pool_flips_are_near_ties(cache, cd, what=what + " trunk")
            relu_flips_are_at_the_boundary(cache, rl, what=what + " trunk")
    assert stats[2] == 0
    assert abs(stats[0] - out["loss"]) < ATOL * max(1.0, abs(out["loss"])), (stats[0], out["loss"])
    cat = CatSpec(specs)
    assert_flat_close(cat, grads, out["grads"], rel=grad_rel, what="weighted NAF pre-clip grads vs f64 oracle")
    plain = N.NAF.forward_backward(ref, batch)
    assert float(np.linalg.norm(grads - plain["grads"]) / np.linalg.norm(plain["grads"])) > 100 * grad_rel
    td = np.abs(out["td"].reshape(-1))
    pos = {int(r): i for i, r in enumerate(idxs)}                 # (a row drawn twice holds its last position's priority)
    tdk = td[[pos[k] for k in keys]]
    want = P.priority(tdk, alpha, eps).astype(np.float64)
    assert (np.abs(written / want - 1) <= 2e-6 + alpha * ATOL * np.maximum(1.0, tdk) / (tdk + eps)).all()
    before = ref.flat()
    ref.apply(out["grads"])
    ref.update_targets()
    assert_flat_close(cat, np.concatenate(Pn[:3]), ref.flat(), rel=2e-6, what="NAF params after the prioritized step")
    assert_flat_close(vspec, Pn[3], ref.target_value.flat(), rel=1e-6, what="target value net")
    assert np.abs(ref.flat() - before).max() > 0
    return path


PARITY = [
    pytest.param((64, 64, 3, 2, 3), 256, True, "f16", 0, id="cfg4-64x64x18-B256-shared-trunk"),
    pytest.param((50, 50, 3, 1, 2), 128, False, "f16", 1, id="reference-defaults-50x50x6-B128-own-trunks"),
    pytest.param((64, 64, 3, 2, 3), 256, True, "u8", 2, id="cfg4-u8-store"),
    pytest.param(LOWDIM, 64, True, "f16", 3, id="lowdim-share"),
]


@pytest.mark.parametrize("shape,B,share,store,seed", PARITY)
def test_prioritized_naf_step_against_f64_oracle(shape, B, share, store, seed):
    per_naf_step_against_f64_oracle(shape, B, share, replay_store=store, seed=seed)


@pytest.mark.parametrize("switch", ["CPP_NAF_MLP", "CPP_NAF_HEADS"])
def test_the_other_naf_head_paths_are_weighted_too(switch):
    """CPP_NAF_MLP=0: naf_heads_kernel's weighted instances; CPP_NAF_HEADS=0: GEMM levels + naf_head_kernel's (ablation build)"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.join(root, "tests", "test_gpu_naf_prioritized_replay.py"), "-q", "-x",
                        "-m", "gpu", "-k", "against_f64_oracle"], cwd=root,
                       env=dict(os.environ, CARTPOLEPP_ABLATION="1", **{switch: "0"}), stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, timeout=900)
    tail = r.stdout.decode()[-1500:]
    assert r.returncode == 0 and " passed" in tail, tail


@pytest.mark.parametrize("shape,B", [((32, 32, 3, 2, 3), 32), (LOWDIM, 32)], ids=["32x32x18-shared", "lowdim-shared"])
def test_only_the_weight_differs(shape, B):
    """beta = 0 (every weight exactly 1): a prioritized NAF step on caller-given rows is the uniform step on them, bit for bit"""
    per, _ = make_naf(shape, B, True, seed=4, replay_size=240, priority_beta=0.0, priority_beta_final=0.0,
                      **{k: v for k, v in PER.items() if k != "priority_beta"})
    uni, _ = make_naf(shape, B, True, seed=4, replay_size=240)
    try:
        for a in (per, uni):
            a.replay_memory.fill_synthetic(200, seed=6)
        rows = np.random.default_rng(1).integers(0, 200, B).astype(np.int32)
        per.train_step(B, 1, idxs=rows)
        uni.train_step(B, 1, idxs=rows)
        assert np.array_equal(per.replay_memory.last_weights(B), np.ones(B, np.float32))
        for a, b in zip(per.networks(), uni.networks()):
            assert np.array_equal(a.get_params(), b.get_params()), a.namespace
        assert per.naf.last_stats()[0] == uni.naf.last_stats()[0]
        assert (per.replay_memory.priorities(rows) != 1.0).any()
    finally:
        per.close()
        uni.close()


@pytest.mark.parametrize("per_step,steps", [(1, 4), (5, 2)], ids=["1-per-step", "5-per-step"])
def test_literal_loop_is_the_fused_step(per_step, steps):
    """naf_cartpole.py:365-373 verbatim on a prioritized memory (batch() draws by priority; naf.train(batch) recomputes the rows'
    weights and writes their priorities) against agent.train_step: the same rows; at one minibatch per step the parameters and the
    trees bit for bit, at five the parameters at 2e-6 (the sample pass riding in the backward kernels moves last bits)."""
    shape, B = (32, 32, 3, 2, 3), 32
    lit, _ = make_naf(shape, B, True, seed=5, replay_size=240, **PER)
    fused, _ = make_naf(shape, B, True, seed=5, replay_size=240, **PER)
    try:
        for a in (lit, fused):
            a.replay_memory.fill_synthetic(200, seed=4)
        for step in range(steps):
            losses = []
            for _ in range(per_step):
                batch = lit.replay_memory.batch(B)
                assert batch.weights is not None and batch.weights.max() == 1.0
                losses.append(lit.naf.train(batch))
            lit.target_value_net.update_weights()
            fused.train_step(B, per_step)
            assert np.isfinite([float(l) for l in losses]).all()
            assert np.array_equal(last_rows(fused, B), batch.idxs), step
            tl, tf = lit.replay_memory.priority_tree(), fused.replay_memory.priority_tree()
            for a, b in zip(lit.networks(), fused.networks()):
                pa, pb = a.get_params(), b.get_params()
                if per_step == 1:
                    assert np.array_equal(pa, pb), (step, a.namespace)
                else:
                    assert float(np.abs(pa - pb).max() / np.abs(pb).max()) < 2e-6, (step, a.namespace)
            if per_step == 1:
                assert np.array_equal(tl, tf), step
            else:
                assert np.allclose(tl, tf, rtol=1e-4, atol=1e-4), (step, float(np.abs(tl - tf).max()))
        L = P.levels(240)
        assert (tf[1 << L:(1 << L) + 200] != 1.0).any()
    finally:
        lit.close()
        fused.close()


@pytest.mark.parametrize("path", ["fused-step", "async-literal-loop"])
def test_a_non_finite_minibatch_leaves_the_parameters_and_the_tree_alone(path):
    """l_values at 1e4 (exp overflows, naf_cartpole.py:208): check_numerics raises, and neither the optimiser nor the priority writes
    ran -- the parameters and the whole sum tree are what they were (a NaN priority would poison every later draw)"""
    B = 16
    agent, _ = make_naf(LOWDIM, B, True, seed=2, replay_size=240, **PER)
    try:
        rm = agent.replay_memory
        rm.fill_synthetic(200, seed=3)
        agent.train_step(B, 5)                                    # a good step first (eager pass + capture)
        float(agent.naf.last_stats()[0])
        agent.naf.l_net.set_params(agent.naf.l_net.get_params() * 0 + 1e4)
        before, tree = params_of(agent), rm.priority_tree()
        if path == "fused-step":
            with pytest.raises(FloatingPointError):
                agent._train_once(B, 5)
            with pytest.raises(FloatingPointError):          # (sticky: the next step stands down as well)
                agent._train_once(B, 5)
        else:
            losses = [agent.naf.train(rm.batch(B)) for _ in range(2)]      # the bad one and one more (sticky flag), nobody looks
            for l in losses:
                with pytest.raises(FloatingPointError):
                    float(l)
        assert np.array_equal(before, params_of(agent)), "an optimiser step ran behind a non-finite minibatch"
        after = rm.priority_tree()
        assert np.isfinite(after).all() and np.array_equal(tree, after), "a non-finite minibatch reached the priority tree"
        if path != "fused-step":
            with pytest.raises(FloatingPointError):         # (close() re-raises the losses it finds non-finite)
                agent.naf.close()
            agent.naf = None
    finally:
        if agent.naf is not None:
            agent.close()
        else:
            agent.value_net.close(); agent.target_value_net.close(); agent.replay_memory.close()


def test_three_runs_are_identical():
    """cfg4 (64x64x18, B = 256, shared trunk, Momentum): 10 outer steps x 5 minibatches, parameters and trees bit for bit"""
    shape, B, runs = (64, 64, 3, 2, 3), 256, []
    for _ in range(3):
        agent, _ = make_naf(shape, B, True, seed=9, replay_size=2 * B + 64, **PER)
        try:
            agent.replay_memory.fill_synthetic(2 * B, seed=12)
            for _ in range(10):
                agent.train_step(B, 5)
            agent.value_net.ctx.sync()
            runs.append([params_of(agent), agent.target_value_net.get_params(), agent.replay_memory.priority_tree()])
        finally:
            agent.close()
    L = P.levels(2 * B + 64)
    assert (runs[0][2][1 << L:(1 << L) + 2 * B] != 1.0).any()
    for other in runs[1:]:
        for x, y in zip(runs[0], other):
            assert np.array_equal(x, y), float(np.abs(x - y).max())


def test_run_training_on_a_prioritized_memory(capsys):
    from cartpoleplusplus_amd import naf_cartpole as F
    from cartpoleplusplus_amd.ddpg_cartpole import make_env
    F.set_opts(F.default_opts(synthetic_env=True, use_raw_pixels=True, render_width=16, render_height=16, batch_size=8,
                              replay_memory_size=120, replay_memory_burn_in=20, max_episode_len=12, share_input_state_representation=True,
                              prioritized_replay=True, priority_beta_steps=5))
    env = make_env(F.opts)
    agent = F.NormalizedAdvantageFunctionAgent(env=env)
    try:
        agent.initialise_variables(seed=1)
        agent.post_var_init_setup()
        agent.run_training(70, 0, 8, F.opts.batches_per_step, None)
        rm = agent.replay_memory
        p = rm.priorities(np.arange(rm.size()))
        assert agent.train_steps > 0
    finally:
        agent.close()
    out = capsys.readouterr().out
    stats = [json.loads(l.split("\t", 1)[1]) for l in out.splitlines() if l.startswith("STATS")]
    assert len(stats) >= 2 and any(np.isfinite(s["mean_losses"]) for s in stats), out[-400:]
    assert not any(np.isinf(s["mean_losses"]) for s in stats)
    assert (p != 1.0).any() and (p > 0).all() and np.isfinite(p).all()
