"""--use-batch-norm training beyond batch size 4: bn.hip's five kernels, the dense-dY instances of the conv dW / dX kernels and the
batch-norm branches of rt_ddpg_pass.cpp / rt_ddpg.cpp / rt_naf.cpp (nets_forward_trunk_bn, launch_sumsq for the clip norms, dbeta written by the BN
backward kernels) against oracle.DDPG(float64) / oracle.naf_np on the same rows and starting parameters.

Bars (the ones tests/test_gpu_batchnorm.py and the helpers already use for this mode): actions, Q, TD, dQ/da 1e-5; pools 2e-5;
pre-clip gradient lists per variable rel 5e-5; parameters after a step, deltas and targets at the helpers' defaults; parameters after
several minibatches 2e-5 / the delta bound of tests/test_gpu_hyperparameters.py.  What a device with a planted fault would show
against these bars is tests/test_batchnorm_sensitivity.py's (CPU, the same inputs).

Loop thresholds of bn.hip at 64x64 (10 output channels; DESIGN.md, batch norm): bn_stats wraps its grid at B >= 2, bn_bwd_reduce at
B >= 7, bn_bwd_dz at B >= 52, bn_relu_pool at B >= 103 -- the batch-size ladder below crosses each with the smallest batch that does."""
import numpy as np
import pytest

from oracle import ddpg_np as O
from tests.helpers import (BN_B1_CASE, BN_B7_CASE, BN_HYPER_CASES, BN_PER_CASE, HYPER_SETS, assert_grads_close_modulo_pool_ties, delta_bound,
                           f32_twin_case, fused_step_against_f64_oracle, make_pair)

pytestmark = pytest.mark.gpu

SIX, CFG3, SMALL, EDGE = (64, 64, 3, 1, 2), (64, 64, 3, 2, 3), (16, 16, 3, 1, 2), (32, 32, 3, 2, 3)
ATOL, POOL_ATOL, GRAD_REL = 1e-5, 2e-5, 5e-5
B1_CASE, B7_CASE, C_CASES = BN_B1_CASE, BN_B7_CASE, BN_HYPER_CASES          # (shared with tests/test_batchnorm_sensitivity.py)
VECTORS = ("actor", "critic", "target_actor", "target_critic")


class HB(object):
    def __init__(self, t):
        self.state_1, self.action, self.reward, self.terminal_mask, self.state_2 = t


def _fused(shape, B, rows, **kw):
    """one minibatch of the fused step on batch-norm networks at this module's bars; prints every figure as a fraction of its bar"""
    rep = fused_step_against_f64_oracle(shape, B, rows, atol=ATOL, grad_rel=GRAD_REL, use_batch_norm=True, **kw)
    fr = {k[4:]: rep[k] / ATOL for k in ("err_actions", "err_dq_da", "err_q", "err_td")}
    fr.update({"pool%d" % i: rep["err_pool%d" % i] / POOL_ATOL for i in (1, 2, 3)})
    fr.update({"grads_" + n: rep["rel_%s_grads" % n] / GRAD_REL for n in ("actor", "critic")})
    print("BN %s B=%d: worst %.2f of its bar; %s flips %s norms %s deltas (relative error; the helper holds them to 2^-23 |theta| + 5e-5 |delta|) %s" % (
        shape, B, max(fr.values()), {k: round(v, 3) for k, v in fr.items()},
        [rep[k] for k in ("flips_actor", "flips_critic", "relu_flips_actor", "relu_flips_critic")], rep["norms"],
        ["%.1e" % rep["rel_delta_" + n] for n in VECTORS]))
    for i in (1, 2, 3):
        assert rep["err_pool%d" % i] < POOL_ATOL, (i, rep["err_pool%d" % i])
    return rep


# ---- a. the batch-size ladder ------------------------------------------------------------------------------------------------------
def test_one_image_leaves_four_samples_per_channel_in_conv3():
    """16x16x6, B = 1: conv3's output is 2 x 2, its batch statistics are taken over four values per channel (and a minibatch of one row)"""
    shape, B, rows, seed = B1_CASE
    _fused(shape, B, rows, graph=False, host_seed=seed)


def test_an_odd_batch_in_the_paired_dense_launches():
    """64x64x18, B = 5: the dense-dY dW and dX launches of actor and critic run side by side over an odd number of images"""
    _fused(CFG3, 5, 60, graph=True, seed=3)


def test_the_backward_reductions_second_pass():
    """64x64x6, B = 7: 7 * 32 * 32 * 10 = 71 680 pooled cells > 64 000, bn_bwd_reduce_kernel's loop runs a second time"""
    shape, B, rows, seed = B7_CASE
    _fused(shape, B, rows, graph=False, host_seed=seed)


@pytest.mark.parametrize("graph", [True, False], ids=["graph-replay", "eager"])
def test_the_dz_kernels_second_pass(graph):
    """64x64x6, B = 56: 56 * 64 * 64 * 10 = 2 293 760 > 8192 * 256, bn_bwd_dz_kernel's loop runs a second time (idx -> (b, y, x, o)
    on the later pass, images past the 51st)"""
    _fused(SIX, 56, 160, graph=graph, seed=5)


def test_the_relu_pool_kernels_second_pass():
    """64x64x6, B = 104: 104 * 32 * 32 * 10 = 1 064 960 > 4096 * 256 pooled cells, bn_relu_pool_kernel's loop runs a second time.  One
    network's forward and backward (actor.train on host states): gradients with the device's pool routes accepted only at near ties,
    and the three pools against the oracle's forward"""
    B = 104
    agent, ref, (aspec, _cspec) = make_pair(SIX, B, True, seed=6, use_batch_norm=True)
    s1 = O.synthetic_batch(np.random.default_rng(16), B, SIX, 2, True)[0]
    try:
        agent.actor.train(s1)
        got = agent.actor.get_grads()
        pools = [getattr(agent.actor, "pool%d" % i).eval(B) for i in (1, 2, 3)]
        held = {}

        def grads():
            held["ag"] = ref.actor_gradients(s1)
            return held["ag"]["grads"]
        flips = assert_grads_close_modulo_pool_ties(aspec, agent.actor, B, ref.actor, lambda: held["ag"]["cache_actor"], grads, got,
                                                    what="actor grads (batch norm, B = 104)", rel=GRAD_REL)
    finally:
        agent.close()
    cache = held["ag"]["cache_actor"]
    for i, (name, _k, _co) in enumerate(O.CONV_DEFS):
        err = float(np.abs(pools[i].reshape(cache[name][1].shape) - cache[name][1]).max())
        print("B=104 %s: |pool - oracle| %.2e (%.2f of the bar), %d near-tie flips" % (name, err, err / POOL_ATOL, flips))
        assert err < POOL_ATOL, (name, err)
    # (images on the second pass of the grid are not all-zero: the loop wrote them)
    assert np.abs(pools[0][103]).max() > 0 and np.abs(pools[2][103]).max() > 0


# ---- b. every dense-dY instance a geometry can reach ---------------------------------------------------------------------------------
# (shape, B, dtype of the host states): what profiles/diag/geometry_sweep.py's batch-norm column and the same sweep with float32 host
# states print "ok" for ...
PARITY = [((64, 64, 3, 1, 3), 3, "f16"), ((64, 64, 3, 1, 4), 2, "f16"), ((50, 50, 3, 1, 2), 3, "f16"), ((96, 96, 3, 2, 3), 2, "f16"),
          ((128, 128, 3, 2, 5), 2, "f16"), ((100, 100, 3, 2, 3), 2, "f16"), ((28, 28, 3, 2, 3), 3, "f16"), ((96, 96, 3, 1, 2), 2, "f16"),
          ((20, 20, 3, 1, 2), 3, "f16"),
          ((64, 64, 3, 1, 2), 3, "f32"), ((64, 64, 3, 2, 3), 2, "f32"), ((40, 30, 3, 1, 2), 3, "f32")]
# ... and what they refuse with "no kernel for" (the dense-dY dW dispatch has no instance; DESIGN.md, batch norm, has the sweep's whole
# table): the 40x30 render from f16 states (it runs from float32 ones), 9 channels from float32 states, 30 channels at 64 columns,
# 12 channels at 32 and at 96 columns, 9 channels at 50 and at 100 columns, a 33x33 conv3 input, 3 channels
REFUSED = [((40, 30, 3, 1, 2), "f16"), ((64, 64, 3, 1, 3), "f32"), ((64, 64, 3, 2, 5), "f16"), ((32, 32, 3, 1, 4), "f16"),
           ((96, 96, 3, 1, 4), "f16"), ((50, 50, 3, 1, 3), "f16"), ((100, 100, 3, 1, 3), "f16"), ((132, 132, 3, 1, 2), "f16"),
           ((64, 64, 3, 1, 1), "f16")]


def _gid(shape, dtype):
    return "%dx%dx%d-%s" % (shape[0], shape[1], int(np.prod(shape[2:])), dtype)


def _host_batch(shape, B, dtype):
    t = O.synthetic_batch(np.random.default_rng(5), B, shape, 2, True)
    if dtype == "f32":       # (k / 255 in f16, widened: the same numbers through the IN_F32_WHITEN instances)
        t = (t[0].astype(np.float32),) + t[1:4] + (t[4].astype(np.float32),)
    return t


@pytest.mark.parametrize("shape,B,dtype", PARITY, ids=[_gid(s, d) for s, _b, d in PARITY])
def test_geometry_op_by_op_gradients(shape, B, dtype):
    """actor.train / critic.train on host states, as tests/test_gpu_batchnorm.py::test_training_mode_gradients"""
    agent, ref, (aspec, cspec) = make_pair(shape, B, True, use_batch_norm=True)
    t = _host_batch(shape, B, dtype)
    try:
        pa = agent.actor.get_params()
        agent.actor.train(t[0])
        assert_grads_close_modulo_pool_ties(
            aspec, agent.actor, B, ref.actor, lambda: ref.actor.forward(t[0]),
            lambda: ref.actor_gradients(t[0])["grads"], agent.actor.get_grads(), what="actor grads (batch norm)", rel=GRAD_REL)
        agent.actor.set_params(pa)
        agent.critic.train(HB(t))
        assert_grads_close_modulo_pool_ties(
            cspec, agent.critic, B, ref.critic, lambda: ref.critic.forward(t[0], action=np.asarray(t[1])),
            lambda: ref.critic_gradients(t)["grads"], agent.critic.get_grads(), what="critic grads (batch norm)", rel=GRAD_REL)
    finally:
        agent.close()


@pytest.mark.parametrize("shape,B", [(s, b) for s, b, d in PARITY if d == "f16"], ids=[_gid(s, d) for s, _b, d in PARITY if d == "f16"])
def test_geometry_fused_minibatch(shape, B):
    _fused(shape, B, 40, graph=True, seed=2)


@pytest.mark.parametrize("shape,dtype", REFUSED, ids=[_gid(s, d) for s, d in REFUSED])
def test_a_refused_geometry_says_so_and_leaves_the_context_usable(shape, dtype):
    B = 3
    agent, _ref, _ = make_pair(shape, B, True, replay_size=60, use_batch_norm=True)
    t = _host_batch(shape, B, dtype)
    try:
        before = agent.critic.get_params()
        with pytest.raises(RuntimeError, match="no kernel for"):
            agent.actor.train(t[0])
            agent.critic.train(HB(t))
        if dtype == "f16":
            agent.replay_memory.fill_synthetic(40, seed=1)
            with pytest.raises(RuntimeError, match="no kernel for"):
                agent.train_step(B, 2)
        assert np.array_equal(before, agent.critic.get_params())
    finally:
        agent.close()
    agent, _ref, _ = make_pair(SMALL, 4, True, replay_size=60, use_batch_norm=True)      # the next agent on the context
    try:
        agent.replay_memory.fill_synthetic(40, seed=1)
        agent.train_step(4, 2); agent.train_step(4, 2)
        agent.actor.ctx.sync()
        assert np.isfinite(agent.critic.get_params()).all() and np.isfinite(agent.actor.get_params()).all()
    finally:
        agent.close()


# ---- c. away from the default hyperparameters: the clip norms come from launch_sumsq --------------------------------------------------
@pytest.mark.parametrize("hyper_name", ["LOUD", "SPLIT", "UNCLIPPED_NONE"])
@pytest.mark.parametrize("shape_name", sorted(C_CASES))
def test_three_minibatches_at_loud_hyperparameters_as_deltas(shape_name, hyper_name):
    from tests.test_gpu_hyperparameters import _pair_from_host_case, _params
    (shape, B, seed), hp, nb = C_CASES[shape_name], HYPER_SETS[hyper_name], 3
    agent, (specs, P, _ep, idxs, batches) = _pair_from_host_case(shape, B, nb, seed, hp, use_batch_norm=True)
    try:
        agent.train_step(B, nb, idxs=idxs)
        got, stats = _params(agent), agent.trainer.last_stats()
    finally:
        agent.close()
    assert specs[0].batch_norm and specs[1].batch_norm
    want, rs, outs, same_routes = f32_twin_case(specs, P, batches, hp)
    assert same_routes, "the float32 twin and the float64 oracle take different pool / ReLU routes: the comparison is void, choose another seed"
    print("BN %s %s: oracle norms %s, device's last (%.4f, %.4f)" % (
        hyper_name, shape_name, [(round(o["actor_norm"], 3), round(o["critic_norm"], 3)) for o in outs], stats[1], stats[2]))
    na, nc = outs[-1]["actor_norm"], outs[-1]["critic_norm"]
    assert abs(stats[1] - na) < 1e-4 * max(1.0, na) and abs(stats[2] - nc) < 1e-4 * max(1.0, nc), (stats, na, nc)
    if hyper_name == "LOUD":
        assert all(min(o["actor_norm"], o["critic_norm"]) > hp.gradient_clip for o in outs)
    elif hyper_name == "SPLIT":
        assert any(min(o["actor_norm"], o["critic_norm"]) < hp.gradient_clip < max(o["actor_norm"], o["critic_norm"]) for o in outs)
    bad = []
    for name, g, w, p, r in zip(VECTORS, got, want, P, rs):
        err, bound = float(np.linalg.norm(g.astype(np.float64) - w)), delta_bound(p, w - p, r, nb)
        print("  %-13s r %.2e  device %.2e of its delta  (|err| %.3e, bound %.3e: %.2f of it)" % (
            name, r, err / np.linalg.norm(w - p), err, bound, err / bound))
        if not err <= bound:
            bad.append((name, err, bound))
    assert not bad, bad


# ---- d. the features merged since, on batch-norm networks ---------------------------------------------------------------------------
PIX = (32, 32, 3, 2, 3)


def test_prioritized_replay_weights_enter_both_bn_reductions():
    from tests.test_gpu_prioritized_replay import _per_step_against_f64_oracle
    shape, B, rows, seed = BN_PER_CASE
    _per_step_against_f64_oracle(shape, B, rows, seed=seed, atol=ATOL, grad_rel=GRAD_REL, use_batch_norm=True)


def test_three_step_returns():
    from tests.test_gpu_nstep_replay import _ddpg_nstep_against_f64_oracle
    _ddpg_nstep_against_f64_oracle(SMALL, 8, 200, seed=1, atol=ATOL, grad_rel=GRAD_REL, use_batch_norm=True)


def test_random_shift_with_pad_two():
    from tests.test_gpu_random_shift import _ddpg_shift_against_f64_oracle
    _ddpg_shift_against_f64_oracle(PIX, 8, 200, seed=1, pad=2, grad_rel=GRAD_REL, use_batch_norm=True)


def test_the_eight_bit_store():
    _fused(PIX, 8, 120, graph=True, seed=4, replay_store="u8")


def test_dropout_together_with_batch_norm():
    _fused((8, 8, 3, 1, 2), 4, 60, graph=True, seed=4, use_dropout=True)


@pytest.mark.parametrize("opt", ["momentum-0.5", "adam"])
def test_three_minibatches_under_momentum_and_adam(opt):
    """tests/test_gpu_ddpg_optimisers.py's first case on batch-norm networks; besides, the slots of every BatchNorm/beta variable
    (dbeta comes from bn_bwd_finalize_kernel, not from a conv epilogue) are non-zero and within the slots' bound"""
    from tests import ddpg_opt_np as R
    from tests.test_gpu_ddpg_optimisers import _compare, _opt_kw, _state
    from tests.test_gpu_hyperparameters import _pair_from_host_case, _params
    shape, B, seed = SMALL, 8, 3
    hp = R.hyper_of(opt, 0.5, 0.25)
    agent, (specs, P, _ep, idxs, batches) = _pair_from_host_case(shape, B, R.NB, seed, hp, use_batch_norm=True, **_opt_kw(opt))
    try:
        names = [v.name for v in agent.actor.trainable_model_vars()]
        assert "actor/conv1/BatchNorm/beta:0" in names
        agent.train_step(B, R.NB, idxs=idxs)
        got, stats = _params(agent), agent.trainer.last_stats()
        slots, steps = _state(agent)
    finally:
        agent.close()
    want, wsteps, outs = R.run_case(specs, P, batches, hp, opt)
    na, nc = outs[-1]["actor_norm"], outs[-1]["critic_norm"]
    assert abs(stats[1] - na) < 1e-4 * max(1.0, na) and abs(stats[2] - nc) < 1e-4 * max(1.0, nc), (stats, na, nc)
    assert steps == [int(x) for x in wsteps] == [R.NB, R.NB]
    _compare("bn-" + opt, opt, P, got + slots, want, R.NB)
    off = 0
    for spec in specs:
        for name, shp in spec.layout():
            n = int(np.prod(shp))
            if name.startswith("conv") and name.endswith("/biases"):          # the BatchNorm/beta slot
                for which, g, w in (("m", slots[0], want[4]), ("v", slots[1], want[5]))[:2 if opt == "adam" else 1]:
                    gs, ws = g[off:off + n], w[off:off + n]
                    err, bound = float(np.linalg.norm(gs - ws)), R.R[which] * float(np.linalg.norm(ws))
                    print("  %s %s of %s/BatchNorm/beta: |slot| %.3e |err| %.3e (%.2f of the bound)" % (spec.kind, which, name[:5], np.linalg.norm(gs), err, err / bound))
                    assert np.all(gs != 0) and err <= bound, (spec.kind, name, which, err, bound)
            off += n
    assert off == len(slots[0])


# ---- e. bit identities ---------------------------------------------------------------------------------------------------------------
E_CASES = [pytest.param(SMALL, 8, id="16x16x6-B8"), pytest.param(CFG3, 8, id="64x64x18-B8")]


def _all_params(agent):
    return [n.get_params() for n in agent.networks()]


def _last_rows(agent, B):
    from cartpoleplusplus_amd._lib import lib, check, ptr
    rows = np.empty(B, np.int32)
    check(lib.cpp_replay_last_indexes(agent.replay_memory.handle, B, ptr(rows)))
    return rows


@pytest.mark.parametrize("shape,B", E_CASES)
def test_graph_replay_is_the_eager_call_on_the_same_rows(shape, B):
    from tests.test_gpu_literal_loop import _twin_agents
    replayed, eager = _twin_agents(shape, B, True, rows=120, use_batch_norm=True)
    try:
        for step in range(4):          # the first call runs eagerly and captures, the later ones replay
            replayed.train_step(B, 1)
            eager.train_step(B, 1, idxs=_last_rows(replayed, B))
            for a, b in zip(replayed.networks(), eager.networks()):
                assert np.array_equal(a.get_params(), b.get_params()), (a.namespace, step)
        assert np.array_equal(replayed.trainer.last_stats(), eager.trainer.last_stats())
        assert np.array_equal(replayed.actor.get_grads(), eager.actor.get_grads())
        assert np.array_equal(replayed.critic.get_grads(), eager.critic.get_grads())
    finally:
        replayed.close(); eager.close()


@pytest.mark.parametrize("shape,B", E_CASES)
def test_the_literal_loop_is_the_fused_step(shape, B):
    from tests.test_gpu_literal_loop import _twin_agents
    lit, fused = _twin_agents(shape, B, True, rows=120, use_batch_norm=True)
    try:
        np.random.seed(99)
        for step in range(4):
            batch = lit.replay_memory.batch(B)            # ddpg_cartpole.py:331-337, one minibatch per step
            lit.actor.train(batch.state_1)
            lit.critic.train(batch)
            lit.target_actor.update_weights()
            lit.target_critic.update_weights()
            fused.train_step(B, 1, idxs=batch.idxs)
            for a, b in zip(lit.networks(), fused.networks()):
                assert np.array_equal(a.get_params(), b.get_params()), (a.namespace, step)
        assert lit.trainer.fused_pairs == 4
        assert np.array_equal(lit.trainer.last_stats(), fused.trainer.last_stats())
    finally:
        lit.close(); fused.close()


@pytest.mark.parametrize("shape,B", E_CASES)
def test_the_data_parallel_step_at_world_size_one_is_the_fused_step(shape, B):
    from cartpoleplusplus_amd import ddpg_cartpole as D
    from cartpoleplusplus_amd.distributed import Communicator, NativeLearner
    res = []
    for which in ("fused", "dp"):
        agent, _ref, _ = make_pair(shape, B, True, replay_size=160, use_batch_norm=True)
        try:
            agent.replay_memory.fill_synthetic(120, seed=11)
            if which == "fused":
                for _ in range(3):
                    agent.train_step(B, 3)
            else:
                learner = NativeLearner(agent, B, int(D.opts.sample_seed), Communicator.single(agent.trainer.ctx), sync_every=1, overlap=False)
                for _ in range(3):
                    learner.train_step(3)
                learner.close()
            agent.actor.ctx.sync()
            res.append(_all_params(agent))
        finally:
            agent.close()
    for name, x, y in zip(VECTORS, res[0], res[1]):
        print("dp vs fused %s: max |diff| %.3e" % (name, float(np.abs(x - y).max())))
    for name, x, y in zip(VECTORS, res[0], res[1]):
        assert np.array_equal(x, y), name


@pytest.mark.parametrize("shape,B", E_CASES)
def test_two_runs_from_one_seed_are_identical(shape, B):
    runs = []
    for _ in range(2):
        agent, _ref, _ = make_pair(shape, B, True, replay_size=160, use_batch_norm=True)
        try:
            agent.replay_memory.fill_synthetic(120, seed=11)
            for _ in range(4):
                agent.train_step(B, 3)
            agent.actor.ctx.sync()
            runs.append(_all_params(agent) + [agent.actor.get_grads(), agent.critic.get_grads()])
        finally:
            agent.close()
    assert all(np.isfinite(x).all() for x in runs[0])
    for x, y in zip(*runs):
        assert np.array_equal(x, y)


# ---- f. edge inputs ------------------------------------------------------------------------------------------------------------------
def _beta_slices(spec):
    out, off = {}, 0
    for name, shp in spec.layout():
        n = int(np.prod(shp))
        if name.startswith("conv"):
            out[name] = (off, shp)
        off += n
    return out


def test_a_dead_conv1_channel_has_exactly_zero_gradients():
    """beta = -50 in one conv1 channel of the actor (channel 3) and of the critic (channel 7): every pooled value of that channel is
    0, no gradient enters it -- the filter's dW and its dbeta are exactly 0, everything else stays at the bars"""
    dead = {"actor": 3, "critic": 7}

    def prepare(agent):
        for net in agent.networks():
            sl = _beta_slices(O.NetSpec(net.namespace.replace("target_", ""), 2, [], True, 32, 32, 18, batch_norm=True))
            p = net.get_params()
            p[sl["conv1/biases"][0] + dead[net.namespace.replace("target_", "")]] = -50.0
            net.set_params(p)
    rep = _fused(EDGE, 6, 80, graph=True, seed=7, prepare=prepare)
    for kind, g in zip(("actor", "critic"), rep["grads"]):
        sl = _beta_slices(O.NetSpec(kind, 2, [], True, 32, 32, 18, batch_norm=True))
        off, shp = sl["conv1/weights"]
        w = g[off:off + int(np.prod(shp))].reshape(shp)
        b = g[sl["conv1/biases"][0]:sl["conv1/biases"][0] + 10]
        assert np.all(w[..., dead[kind]] == 0) and b[dead[kind]] == 0, (kind, np.abs(w[..., dead[kind]]).max(), b[dead[kind]])
        live = [c for c in range(10) if c != dead[kind]]
        assert np.all(np.abs(w[..., live]).max(axis=(0, 1, 2)) > 0) and np.all(b[live] != 0)


def test_betas_as_large_as_the_pooled_values():
    """every beta drawn from U(-1, 3): bn_bwd_reduce_kernel recovers zhat as pooled - beta, which rounds at the size of pooled"""
    def prepare(agent):
        rng = np.random.default_rng(77)
        for net in agent.networks():
            sl = _beta_slices(O.NetSpec(net.namespace.replace("target_", ""), 2, [], True, 32, 32, 18, batch_norm=True))
            p = net.get_params()
            for name in ("conv1/biases", "conv2/biases", "conv3/biases"):
                p[sl[name][0]:sl[name][0] + 10] = rng.uniform(-1, 3, 10).astype(np.float32)
            net.set_params(p)
    _fused(EDGE, 6, 80, graph=True, seed=8, prepare=prepare)


def test_constant_input_channels():
    """rendered episodes seen by a blind camera: constant input channels, conv outputs whose batch variance is near the 1e-3 epsilon"""
    _fused(EDGE, 6, 80, graph=True, seed=9, fill="render-blind")


# ---- g. NAF --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["momentum-0.5", "adam-third-step"])
@pytest.mark.parametrize("share", [True, False], ids=["shared-trunk", "own-trunks"])
def test_naf_at_batch_56(share, name):
    """64x64x18, B = 56: bn_bwd_dz wraps (56 * 64 * 64 * 10 > 8192 * 256) in one network (shared trunk) or in three (own trunks)"""
    from tests.test_gpu_hyperparameters import _naf_step
    _naf_step(CFG3, 56, share, name, use_batch_norm=True, grad_rel=GRAD_REL)


@pytest.mark.parametrize("share", [True, False], ids=["shared-trunk", "own-trunks"])
def test_naf_at_batch_one(share):
    from tests.test_gpu_hyperparameters import _naf_step
    _naf_step(SMALL, 1, share, "momentum-0.5", use_batch_norm=True, grad_rel=GRAD_REL)
