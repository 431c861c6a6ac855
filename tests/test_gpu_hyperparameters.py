"""The update path away from the reference's default hyperparameters.  Every other GPU test runs at learning rates 1e-3 / 1e-2,
discount 0.99, clip 5, target update rate 1e-4, Momentum 0.9 and Adam's defaults, where a stale target, a stale conv1 operand image or
a hard-coded discount are below float32 rounding.  These numbers are kernel arguments of opt_apply_kernel (clip by global norm, the
optimiser, the conv1 image rider, the targets' soft update), of the TD / heads kernels and of the n-step gather; here they take values
at which such faults are 10x .. 1000x the tolerances -- tests/test_hyper_sensitivity.py checks that with the oracle alone, on the
same inputs (tests.helpers.host_case)."""
import ctypes

import numpy as np
import pytest

from oracle import ddpg_np as O
from tests.helpers import (HYPER_SETS, LOUD, NAF_HYPER, NAF_OPTIMISERS, NAF_RIDER_CASE, RIDER_CASES, SENS_B, SENS_SEED, SENS_SHAPE, STALE_TARGET_CASE, delta_bound,
                           f32_twin_case, fused_step_against_f64_oracle, host_case, hyper_options, make_pair, naf_host_case,
                           naf_twin_case, oracle_of)

pytestmark = pytest.mark.gpu

CFG3, NINE, REF50, SMALL, LOWDIM = (64, 64, 3, 2, 3), (64, 64, 3, 1, 3), (50, 50, 3, 1, 2), (16, 16, 3, 1, 2), (2, 2, 7)
VECTORS = ("actor", "critic", "target_actor", "target_critic")


def _pair_from_host_case(shape, B, nb, seed, hyper, rows=24, fill=True, **kw):
    """a device agent holding host_case's parameters and episodes, and the case itself"""
    from cartpoleplusplus_amd import ddpg_cartpole as D
    specs, P, episodes, idxs, batches = host_case(shape, B, nb, seed, rows=rows, batch_norm=bool(kw.get("use_batch_norm", False)))
    agent, _ref, (aspec, _cspec) = make_pair(shape, B, len(shape) == 5, seed=seed, replay_size=rows, perturb=False,
                                             **dict(hyper_options(hyper), **kw))
    try:
        assert list(aspec.hidden) == list(specs[0].hidden) and D.opts.discount == hyper.discount
        for net, p in zip(agent.networks(), P):
            assert net.get_params().shape == p.shape
            net.set_params(p)
        if fill:
            for ep in episodes:
                agent.replay_memory.add_episode(*ep)
            assert agent.replay_memory.size() == rows
    except Exception:
        agent.close()
        raise
    return agent, (specs, P, episodes, idxs, batches)


def _params(agent):
    return [n.get_params() for n in agent.networks()]


# ---- a. one minibatch, graph replay, against the float64 oracle at the helper's ordinary bars
@pytest.mark.parametrize("shape,B,rows,pixel", [(CFG3, 8, 120, True), (NINE, 6, 100, True), (REF50, 5, 100, True), (LOWDIM, 16, 300, False)],
                         ids=["64x64x18-B8", "64x64x9-B6", "50x50x6-B5-no-rs16", "lowdim-B16"])
def test_one_graph_replayed_minibatch_at_loud_hyperparameters(shape, B, rows, pixel):
    rep = fused_step_against_f64_oracle(shape, B, rows, graph=True, seed=31, pixel=pixel, hyper=LOUD)
    print("LOUD %s B=%d:" % (shape, B), {k: v for k, v in rep.items() if k.startswith(("err_", "rel_", "norm"))})
    assert min(rep["norms"]) > LOUD.gradient_clip, rep["norms"]        # both lists clipped


@pytest.mark.parametrize("name", ["UNCLIPPED_NONE", "UNCLIPPED_1E4"])
def test_one_graph_replayed_minibatch_without_clipping(name):
    hp = HYPER_SETS[name]
    rep = fused_step_against_f64_oracle(SMALL, 16, 200, graph=True, seed=32, hyper=hp)
    print("%s:" % name, {k: v for k, v in rep.items() if k.startswith(("err_", "rel_", "norm"))})
    if hp.gradient_clip is not None:
        assert max(rep["norms"]) < hp.gradient_clip, rep["norms"]      # clip > 0 with a scale of exactly 1


def test_one_graph_replayed_minibatch_with_one_list_clipped():
    """SPLIT's clip lies between the two lists' norms in tests/test_hyper_sensitivity.py's minibatches (host_case); this case starts
    from make_pair's parameters, so which side each list falls on is asserted from the step's own statistics"""
    hp = HYPER_SETS["SPLIT"]
    rep = fused_step_against_f64_oracle(SMALL, 16, 200, graph=True, seed=32, hyper=hp)
    print("SPLIT:", {k: v for k, v in rep.items() if k.startswith(("err_", "rel_", "norm"))})
    assert min(rep["norms"]) < hp.gradient_clip < max(rep["norms"]), rep["norms"]


# ---- b. several minibatches in one call: the conv1 image rider and the `next` minibatch exist
@pytest.mark.parametrize("shape,B,seed,hyper_name", [RIDER_CASES["LOUD"][:3] + ("LOUD",), RIDER_CASES["ACTOR_LOUD"][:3] + ("ACTOR_LOUD",), (NINE, 6, 1, "LOUD"), (SMALL, SENS_B, SENS_SEED, "LOUD"),
                                                     (SMALL, SENS_B, SENS_SEED, "SPLIT"), (SMALL, SENS_B, SENS_SEED, "UNCLIPPED_NONE"),
                                                     (SMALL, SENS_B, SENS_SEED, "UNCLIPPED_1E4")],
                         ids=["64x64x18-B8", "64x64x18-B8-actor-loud", "64x64x9-B6", "16x16x6-B16", "16x16x6-B16-split", "16x16x6-B16-clip-none", "16x16x6-B16-clip-1e4"])
@pytest.mark.parametrize("nb", [3, 5])
def test_several_minibatches_in_one_call_as_deltas(shape, B, seed, hyper_name, nb):
    hp = RIDER_CASES["ACTOR_LOUD"][3] if hyper_name == "ACTOR_LOUD" else HYPER_SETS[hyper_name]
    agent, (specs, P, _ep, idxs, batches) = _pair_from_host_case(shape, B, nb, seed, hp)
    try:
        agent.train_step(B, nb, idxs=idxs)
        got = _params(agent)
        stats = agent.trainer.last_stats()
    finally:
        agent.close()
    want, rs, outs, same_routes = f32_twin_case(specs, P, batches, hp)
    assert same_routes, "the float32 twin and the float64 oracle take different pool / ReLU routes: the comparison is void, choose another seed"
    print("%s %s nb=%d: oracle norms %s" % (hyper_name, shape, nb, [(round(o["actor_norm"], 3), round(o["critic_norm"], 3)) for o in outs]))
    na, nc = outs[-1]["actor_norm"], outs[-1]["critic_norm"]
    assert abs(stats[1] - na) < 1e-4 * max(1.0, na) and abs(stats[2] - nc) < 1e-4 * max(1.0, nc), (stats, na, nc)
    if hyper_name == "LOUD":
        assert all(min(o["actor_norm"], o["critic_norm"]) > hp.gradient_clip for o in outs)
    elif hyper_name == "UNCLIPPED_1E4":
        assert all(max(o["actor_norm"], o["critic_norm"]) < hp.gradient_clip for o in outs)
    elif hyper_name == "SPLIT":       # (one list clipped, the other not, in at least one minibatch; the device's last norms are the oracle's, above)
        assert any(min(o["actor_norm"], o["critic_norm"]) < hp.gradient_clip < max(o["actor_norm"], o["critic_norm"]) for o in outs)
    bad = []
    for name, g, w, p, r in zip(VECTORS, got, want, P, rs):
        err, bound = float(np.linalg.norm(g.astype(np.float64) - w)), delta_bound(p, w - p, r, nb)
        print("  %-13s r %.2e  device %.2e of its delta  (|err| %.3e, bound %.3e)" % (name, r, err / np.linalg.norm(w - p), err, bound))
        if not err <= bound:
            bad.append((name, err, bound))
    assert not bad, bad


@pytest.mark.parametrize("shape,B", [(CFG3, 8), (SMALL, 16)], ids=["64x64x18-B8", "16x16x6-B16"])
def test_captured_steps_carry_the_hyperparameters_and_repeat_bit_for_bit(shape, B):
    """idxs=None: capture + replay; two fresh agents end on the same bits, and not on the bits of an agent at the default hyperparameters
    (they are arguments of the captured kernels)"""
    runs = []
    for hp in (LOUD, LOUD, O.DEFAULT_HYPER):
        agent, _case = _pair_from_host_case(shape, B, 3, 1, hp, rows=60)
        try:
            for _ in range(3):
                agent.train_step(B, 3)
            runs.append(np.concatenate(_params(agent)))
        finally:
            agent.close()
    assert np.isfinite(runs[0]).all()
    assert np.array_equal(runs[0], runs[1])
    assert not np.array_equal(runs[0], runs[2])


# ---- c. bit-exact invariants
def _conv1_len(spec):
    return int(np.prod(spec.layout()[0][1])) + int(np.prod(spec.layout()[1][1]))


@pytest.mark.parametrize("shape,B", [(CFG3, 8), (SMALL, 16)], ids=["64x64x18-B8-rider", "16x16x6-B16"])
@pytest.mark.parametrize("frozen", ["actor", "critic"])
def test_a_learning_rate_of_zero_leaves_that_network_bit_identical(shape, B, frozen):
    hp = LOUD._replace(actor_lr=0.0) if frozen == "actor" else LOUD._replace(critic_lr=0.0)
    agent, (specs, P, _ep, idxs, _b) = _pair_from_host_case(shape, B, 3, 1, hp)
    try:
        agent.train_step(B, 3, idxs=idxs)
        got = _params(agent)
    finally:
        agent.close()
    k, other = (0, 1) if frozen == "actor" else (1, 0)
    c1 = _conv1_len(specs[k])
    assert np.array_equal(got[k][:c1], P[k][:c1]), "conv1 (the rider's own update) moved at learning rate 0"
    assert np.array_equal(got[k][c1:], P[k][c1:]), "the main loop's variables moved at learning rate 0"
    c1 = _conv1_len(specs[other])
    assert not np.array_equal(got[other][:c1], P[other][:c1]) and not np.array_equal(got[other][c1:], P[other][c1:])


@pytest.mark.parametrize("shape,B", [(CFG3, 8), (SMALL, 16)], ids=["64x64x18-B8-rider", "16x16x6-B16"])
def test_target_update_rates_of_zero_and_one_are_exact(shape, B):
    """soft_update_value is fmaf(-coeff, t - s, t): coeff 0 returns t; coeff 1 returns f32(t - f32(t - s)) exactly (the product is
    the rounded difference itself) -- which is s only where t and s lie within a factor of two of each other"""
    for tau in (0.0, 1.0):
        agent, (specs, P, _ep, idxs, _b) = _pair_from_host_case(shape, B, 3, 1, LOUD._replace(target_update_rate=tau))
        try:
            agent.train_step(B, 3, idxs=idxs)
            got = _params(agent)
        finally:
            agent.close()
        for k in (0, 1):
            t, s = P[2 + k], got[k]
            want = t if tau == 0.0 else (t.astype(np.float64) - (t - s).astype(np.float64)).astype(np.float32)
            c1 = _conv1_len(specs[k])
            assert not np.array_equal(s, P[k])
            assert np.array_equal(got[2 + k][:c1], want[:c1]), (VECTORS[2 + k], "conv1", tau)
            assert np.array_equal(got[2 + k][c1:], want[c1:]), (VECTORS[2 + k], "past conv1", tau)


# ---- d. the target networks' conv1 operand image after a target update
def test_the_second_call_reads_the_updated_target_networks():
    """tau = 0.25: the first call's target update moves the target networks' conv1 weights by a quarter of their distance to the live
    ones.  The second call's TD against the oracle at the parameters read back in between: a target conv1 image that missed the
    update is >= 10x the 1e-5 allowed here (tests/test_hyper_sensitivity.py)"""
    shape, B, seed = STALE_TARGET_CASE
    agent, (specs, P, _ep, idxs, batches) = _pair_from_host_case(shape, B, 2, seed, LOUD, rows=40)
    try:
        agent.train_step(B, 1, idxs=idxs[:B])
        mid = _params(agent)
        agent.train_step(B, 1, idxs=idxs[B:])
        _a, _dq, q, td = agent.trainer.last_values(B)
    finally:
        agent.close()
    assert not np.array_equal(mid[2], P[2]) and not np.array_equal(mid[3], P[3])
    cg = oracle_of(specs, mid, np.float64, LOUD).critic_gradients(batches[1])
    print("second call: |q - oracle| %.3e  |td - oracle| %.3e" % (np.abs(q - cg["q"]).max(), np.abs(td - cg["td"]).max()))
    assert np.abs(q - cg["q"]).max() < 1e-5 and np.abs(td - cg["td"]).max() < 1e-5


# ---- e. the reference's loop as the reference writes it
@pytest.mark.parametrize("shape,B", [(CFG3, 8), (SMALL, 16)], ids=["64x64x18-B8", "16x16x6-B16"])
def test_the_literal_loop_is_the_fused_step_at_loud_hyperparameters(shape, B):
    from tests.test_gpu_literal_loop import _twin_agents
    lit, fused = _twin_agents(shape, B, True, rows=120, **hyper_options(LOUD))
    try:
        np.random.seed(99)
        for _step in range(4):
            batch = lit.replay_memory.batch(B)            # ddpg_cartpole.py:331-337, one minibatch per step
            lit.actor.train(batch.state_1)
            lit.critic.train(batch)
            lit.target_actor.update_weights()
            lit.target_critic.update_weights()
            fused.train_step(B, 1, idxs=batch.idxs)
            for a, b in zip(lit.networks(), fused.networks()):
                assert np.array_equal(a.get_params(), b.get_params()), (a.namespace, _step)
        assert lit.trainer.fused_pairs == 4
        assert np.array_equal(lit.trainer.last_stats(), fused.trainer.last_stats())
    finally:
        lit.close(); fused.close()


# ---- f. the data-parallel half steps with a gradient scale other than 1
def _scaled_clip(g, scale, clip):
    return O.clip_by_global_norm(scale * np.asarray(g, np.float64), clip, np.float64)


@pytest.mark.parametrize("clip", [0.5, None])
def test_ddpg_apply_gradients_with_a_scale_of_one_half(clip):
    from cartpoleplusplus_amd import ddpg_cartpole as D
    from cartpoleplusplus_amd.distributed import AgentOps
    hp, B = LOUD._replace(gradient_clip=clip), 16
    agent, (specs, P, _ep, _idxs, _b) = _pair_from_host_case(SMALL, B, 1, SENS_SEED, hp, rows=60)
    try:
        ops = AgentOps(agent, B, int(D.opts.sample_seed))
        ops.sample_and_compute()
        g = [agent.actor.get_grads(), agent.critic.get_grads()]
        ops.apply(0.5)
        got, stats = _params(agent), agent.trainer.last_stats()
    finally:
        agent.close()
    assert np.array_equal(got[2], P[2]) and np.array_equal(got[3], P[3])          # (the targets move in update_targets only)
    for k, lr in ((0, hp.actor_lr), (1, hp.critic_lr)):
        clipped, norm = _scaled_clip(g[k], 0.5, clip)
        d_want, d_got = -lr * clipped, got[k].astype(np.float64) - P[k]
        err, bound = float(np.linalg.norm(d_got - d_want)), delta_bound(P[k], d_want, 5e-5)
        print("clip %s %s: scaled norm %.4f (device %.4f), delta error %.2e of the delta" % (clip, VECTORS[k], norm, stats[1 + k], err / np.linalg.norm(d_want)))
        assert abs(stats[1 + k] - norm) < 1e-4 * max(1.0, norm), (stats, norm)     # the norm of the SCALED list
        assert clip is None or norm > clip
        assert err < bound, (VECTORS[k], err, bound)


@pytest.mark.parametrize("clip", [0.5, None])
def test_naf_apply_gradients_with_a_scale_of_one_half(clip):
    from cartpoleplusplus_amd import _lib
    from cartpoleplusplus_amd import naf_cartpole as F
    from tests.test_gpu_naf import make_naf, params_of
    B = 16
    agent, _ref, _specs = make_naf(SMALL, B, True, "Momentum", {"learning_rate": 0.01, "momentum": 0.5}, seed=6, replay_size=100, clip=clip,
                                   discount=NAF_HYPER["discount"], target_update_rate=NAF_HYPER["target_update_rate"])
    try:
        agent.replay_memory.fill_synthetic(60, seed=5)
        lib, check = _lib.lib, _lib.check
        for _ in range(2):          # (the second step starts from a Momentum slot that is not zero)
            check(lib.cpp_naf_sample_and_compute(agent.naf.handle, agent.replay_memory.handle, B, int(F.opts.sample_seed)))
            before, m = params_of(agent), agent.naf.get_optimiser_state()["m"].astype(np.float64)
            g = agent.naf.get_grads()
            check(lib.cpp_naf_apply_gradients(agent.naf.handle, ctypes.c_float(0.5)))
            got, stats = params_of(agent), agent.naf.last_stats()
            m_got = agent.naf.get_optimiser_state()["m"]
        assert np.abs(m).max() > 0
    finally:
        agent.close()
    clipped, norm = _scaled_clip(g, 0.5, clip)
    m_want = 0.5 * m + clipped
    d_want, d_got = -0.01 * m_want, got.astype(np.float64) - before
    err, bound = float(np.linalg.norm(d_got - d_want)), delta_bound(before, d_want, 5e-5)
    print("NAF clip %s: scaled norm %.4f (device %.4f), delta error %.2e of the delta" % (clip, norm, stats[1], err / np.linalg.norm(d_want)))
    assert abs(stats[1] - norm) < 1e-4 * max(1.0, norm), (stats, norm)
    assert clip is None or norm > clip
    assert err < bound, (err, bound)
    assert np.linalg.norm(m_got - m_want) < 2.0 ** -23 * np.linalg.norm(m) + 5e-5 * np.linalg.norm(m_want - m)


# ---- g. NAF: the optimisers away from Momentum 0.9 / Adam's defaults
NAF_SHAPES = [pytest.param(CFG3, 8, True, id="64x64x18-B8-shared-trunk"), pytest.param(SMALL, 16, False, id="16x16x6-B16-own-trunks")]


def _naf_step(shape, B, share, name, report=None, **kw):
    from tests.test_gpu_naf import naf_fused_step_against_f64_oracle
    oname, oargs, warm = NAF_OPTIMISERS[name]
    report = {} if report is None else report
    naf_fused_step_against_f64_oracle(shape, B, share, rows=150, optimiser=oname, optimiser_args=oargs, warm_steps=warm, clip=NAF_HYPER["clip"],
                                      discount=NAF_HYPER["discount"], target_update_rate=NAF_HYPER["target_update_rate"], report=report, **kw)
    print("NAF %s %s: norm %.4f (device %.4f), delta error %.2e (params) %.2e (target) of the delta" % (
        name, shape, report["norm"], report["device_norm"], report["rel_delta_params"], report["rel_delta_target"]))
    return report


@pytest.mark.parametrize("shape,B,share", NAF_SHAPES)
def test_naf_momentum_one_half(shape, B, share):
    rep = _naf_step(shape, B, share, "momentum-0.5")
    assert rep["norm"] > NAF_HYPER["clip"]


@pytest.mark.parametrize("shape,B,share", NAF_SHAPES)
def test_naf_momentum_zero_is_gradient_descent(shape, B, share):
    """momentum_accum is fmaf(momentum, m, g): at momentum 0 the slot is the clipped gradient itself and momentum_step is sgd_update's
    fmaf(-lr, g, p), so the two runs end on the same bits"""
    from tests.test_gpu_naf import naf_fused_step_against_f64_oracle
    rep = _naf_step(shape, B, share, "momentum-0.0")
    sgd = {}
    naf_fused_step_against_f64_oracle(shape, B, share, rows=150, optimiser="GradientDescent", optimiser_args={"learning_rate": 0.01},
                                      clip=NAF_HYPER["clip"], discount=NAF_HYPER["discount"],
                                      target_update_rate=NAF_HYPER["target_update_rate"], report=sgd)
    assert np.array_equal(rep["params"], sgd["params"]) and np.array_equal(rep["target"], sgd["target"])


@pytest.mark.parametrize("shape,B,share", NAF_SHAPES)
def test_naf_adam_third_step(shape, B, share):
    """t = 3 in the bias correction, betas and epsilon away from the defaults (one minibatch per call: no conv1 image rider under any
    optimiser; what Adam does to the rider is test_naf_adam_builds_the_conv1_image_by_a_launch_of_its_own_every_minibatch's)"""
    _naf_step(shape, B, share, "adam-third-step")


def _naf_agent_from_host_case(name):
    """a shared-trunk NAF agent holding naf_host_case's parameters and episodes"""
    from tests.test_gpu_naf import make_naf
    oname, oargs, _warm = NAF_OPTIMISERS[name]
    shape, B, nb, rows, seed = NAF_RIDER_CASE
    specs, flats, episodes, idxs, batches = naf_host_case(shape, B, nb, rows, seed)
    agent, _ref, _specs = make_naf(shape, B, True, oname, oargs, seed=11, replay_size=rows, clip=NAF_HYPER["clip"], discount=NAF_HYPER["discount"],
                                   target_update_rate=NAF_HYPER["target_update_rate"])
    try:
        for net, p in zip((agent.value_net, agent.naf.mu_net, agent.naf.l_net, agent.target_value_net), flats):
            assert net.get_params().shape == p.shape
            net.set_params(p)
        for ep in episodes:
            agent.replay_memory.add_episode(*ep)
    except Exception:
        agent.close()
        raise
    return agent, (specs, flats, idxs, batches)


@pytest.mark.parametrize("name", ["momentum-0.5", "momentum-0.0", "adam-third-step"])
def test_naf_several_minibatches_in_one_call_as_deltas(name):
    """the shared trunk at 64x64x18: minibatches 2 and 3 read conv1 through the operand image.  Under SGD / Momentum the optimiser
    launch's rider built it, from conv1 weights the rider updated itself with Momentum slots of its own (mw / mb); under Adam the rider
    stands down and the image is rebuilt from the Adam-updated weights by a launch of its own.  Deltas of the parameters and of the
    target value network against the float64 oracle, r from the float32 numpy twin as in the DDPG case above (inputs:
    tests.helpers.naf_host_case, checked with a planted stale image in tests/test_hyper_sensitivity.py)."""
    from tests.test_gpu_naf import params_of
    oname, oargs, _warm = NAF_OPTIMISERS[name]
    B, nb = NAF_RIDER_CASE[1], NAF_RIDER_CASE[2]
    agent, (specs, flats, idxs, batches) = _naf_agent_from_host_case(name)
    try:
        agent.train_step(B, nb, idxs=idxs)
        got, stats = (params_of(agent), agent.target_value_net.get_params()), agent.naf.last_stats()
    finally:
        agent.close()
    want, rs, norms, same = naf_twin_case(specs, flats, batches, oname, oargs)
    assert same, "float32 twin and float64 oracle take different routes: the comparison is void, choose another seed"
    print("NAF %s nb=%d: oracle norms %s, device's last %.4f" % (name, nb, norms, stats[1]))
    assert min(norms) > NAF_HYPER["clip"] and abs(stats[1] - norms[-1]) < 1e-4 * max(1.0, norms[-1])
    for what, g, w, r, p in zip(("params", "target"), got, want, rs, (np.concatenate(flats[:3]), flats[3])):
        err, bound = float(np.linalg.norm(g.astype(np.float64) - w)), delta_bound(p, w - p, r, nb)
        print("  %-7s r %.2e  device %.2e of its delta  (|err| %.3e, bound %.3e)" % (what, r, err / np.linalg.norm(w - p), err, bound))
        assert err <= bound, (what, err, bound)


def test_naf_adam_builds_the_conv1_image_by_a_launch_of_its_own_every_minibatch():
    """one profiled train_step(B, 3) per optimiser on the same rows: under Momentum the images of minibatches 2 and 3 ride in the
    optimiser launch (conv1_image launches for the first minibatch only), under Adam every minibatch launches conv1_image"""
    from tests.helpers import _profiled_calls
    B, nb = NAF_RIDER_CASE[1], NAF_RIDER_CASE[2]
    counts = {}
    for name in ("momentum-0.5", "adam-third-step"):
        agent, (_specs, _flats, idxs, _b) = _naf_agent_from_host_case(name)
        try:
            counts[name] = _profiled_calls(agent.value_net.ctx, lambda: agent.train_step(B, nb, idxs=idxs)).get("conv1_image", 0)
        finally:
            agent.close()
    print("conv1_image launches in train_step(B, %d):" % nb, counts)
    assert counts["momentum-0.5"] >= 1
    assert counts["adam-third-step"] > counts["momentum-0.5"], counts


# ---- h. n-step returns with another discount
def test_nstep_returns_with_a_discount_of_nine_tenths():
    from tests.test_gpu_nstep_replay import _ddpg_nstep_against_f64_oracle
    _ddpg_nstep_against_f64_oracle(CFG3, 8, 200, seed=5, hyper=LOUD)


def test_a_discount_mismatch_names_both_values():
    agent, _ref, _ = make_pair(SMALL, 8, True, seed=8, replay_size=120, **hyper_options(LOUD))
    try:
        agent.replay_memory.fill_synthetic(100, seed=27)
        agent.replay_memory.enable_n_step(3, 0.75)
        before = _params(agent)
        with pytest.raises(RuntimeError, match=r"discount 0\.75\b.*discount is 0\.(9|89999)"):
            agent.train_step(8, 1)
        for x, y in zip(before, _params(agent)):
            assert np.array_equal(x, y)
        agent.replay_memory.enable_n_step(3, LOUD.discount)
        agent.train_step(8, 1)
        assert not np.array_equal(before[1], agent.critic.get_params())
    finally:
        agent.close()
