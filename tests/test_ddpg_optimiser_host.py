"""Momentum and Adam for the DDPG learner, without a GPU: the command line, the float64 restatement (tests/ddpg_opt_np.py) against its
parent oracle, and what tests/test_gpu_ddpg_optimisers.py can see -- on that module's own cases (the same parameters, episodes and rows,
tests.helpers.host_case) each planted fault must move a compared vector by more than the tolerance the GPU test applies to it, and
the oracle's own float32 run must stay inside that tolerance (a case that rests on elements float32 cannot decide is replaced, not
loosened)."""
import functools

import numpy as np
import pytest

from oracle import ddpg_np as O
from tests import ddpg_opt_np as R
from tests.helpers import host_case, oracle_of


# ---- the command line
def test_the_parser_takes_both_flags_and_the_default_is_gradient_descent():
    from cartpoleplusplus_amd import ddpg_cartpole as D
    o = D.build_parser().parse_args([])
    assert D.ddpg_optimiser(o) == (0, 0.0, 0.9, 0.999, 1e-8) and D.default_opts().ddpg_optimiser == "GradientDescent"
    o = D.build_parser().parse_args(["--ddpg-optimiser", "Adam", "--ddpg-optimiser-args", '{"beta1": 0.8, "epsilon": 1e-3}'])
    assert D.ddpg_optimiser(o) == (2, 0.0, 0.8, 0.999, 1e-3)
    o = D.build_parser().parse_args(["--ddpg-optimiser", "Momentum", "--ddpg-optimiser-args", '{"momentum": 0.5}'])
    assert D.ddpg_optimiser(o) == (1, 0.5, 0.9, 0.999, 1e-8)
    assert D.ddpg_optimiser(D.default_opts(ddpg_optimiser="Adam")) == (2, 0.0, 0.9, 0.999, 1e-8)
    with pytest.raises(SystemExit):
        D.build_parser().parse_args(["--ddpg-optimiser", "RMSProp"])


def test_a_learning_rate_among_the_optimiser_args_is_refused_by_name():
    from cartpoleplusplus_amd import ddpg_cartpole as D
    o = D.default_opts(ddpg_optimiser="Adam", ddpg_optimiser_args='{"learning_rate": 0.001}')
    with pytest.raises(SystemExit) as e:
        D.ddpg_optimiser(o)
    assert "--actor-learning-rate" in str(e.value) and "--critic-learning-rate" in str(e.value)
    with pytest.raises(SystemExit):
        D.ddpg_optimiser(D.default_opts(ddpg_optimiser="Adam", ddpg_optimiser_args='{"beta3": 1}'))
    with pytest.raises(SystemExit):
        D.ddpg_optimiser(D.default_opts(ddpg_optimiser="Adam", ddpg_optimiser_args='[1]'))


def test_the_optimiser_flag_of_the_shared_options_still_means_nothing_to_ddpg():
    from cartpoleplusplus_amd import ddpg_cartpole as D
    o = D.build_parser().parse_args(["--optimiser", "Adam"])
    assert D.ddpg_optimiser(o)[0] == 0


# ---- the restatement against its parent
@functools.lru_cache(maxsize=None)
def _case(shape_name):
    shape, B, seed = R.SHAPES[shape_name]
    return host_case(shape, B, R.NB, seed)


def test_momentum_zero_is_the_parent_oracles_step_bit_for_bit():
    specs, P, _ep, _idxs, batches = _case("16x16x6")
    hp = R.hyper_of("momentum-0.0", 0.5, 0.25)
    got, steps, _outs = R.run_case(specs, P, batches, hp, "momentum-0.0")
    parent = oracle_of(specs, P, np.float64, hp)
    parent.train_step(batches)
    for g, n in zip(got[:4], (parent.actor, parent.critic, parent.target_actor, parent.target_critic)):
        assert np.array_equal(g, np.asarray(n.flat(), np.float64))
    assert list(steps) == [R.NB, R.NB]


def test_each_list_counts_its_own_applies():
    specs, P, _ep, _idxs, batches = _case("16x16x6")
    name, args = R.OPTIMISERS["adam"]
    ref = R.restatement(specs, P, np.float64, R.hyper_of("adam", 0.5, 0.25), name, args)
    c0 = ref.critic.flat().copy()
    ref.train_actor(batches[0][0])
    assert list(ref.state()["step"]) == [1, 0] and np.array_equal(ref.critic.flat(), c0)
    assert not ref.slots["critic"].m.any() and ref.slots["actor"].m.any()
    a1 = ref.actor.flat().copy()
    ref.train_critic(batches[1])
    ref.train_critic(batches[2])
    assert list(ref.state()["step"]) == [1, 2] and np.array_equal(ref.actor.flat(), a1)
    ref.train_minibatch(batches[0])
    assert list(ref.state()["step"]) == [2, 3]


# ---- conditioning and power, on the GPU module's cases
@functools.lru_cache(maxsize=None)
def _run(shape_name, opt, clip, tau, dt_name="f64", fault=None, actor_first=False):
    specs, P, _ep, _idxs, batches = _case(shape_name)
    first = batches[-1][0] if actor_first else None
    return R.run_case(specs, P, batches, R.hyper_of(opt, clip, tau), opt, np.float64 if dt_name == "f64" else np.float32, fault, first)


@pytest.mark.parametrize("cid,opt,shape_name,clip,tau", R.grid(), ids=[c[0] for c in R.grid()])
def test_the_float32_twin_stays_inside_the_gpu_tolerance(cid, opt, shape_name, clip, tau):
    """the cap on a case: the oracle's own float32 run within the GPU test's bounds of its float64 run, on the same routes, with every
    norm on the side of the clip the case is named for"""
    _specs, P, _ep, _idxs, _b = _case(shape_name)
    want, steps, o64 = _run(shape_name, opt, clip, tau)
    twin, _s, o32 = _run(shape_name, opt, clip, tau, "f32")
    assert all(np.isfinite(w).all() for w in want) and list(steps) == [R.NB, R.NB]
    assert all(np.array_equal(x, y) for a, b in zip(o64, o32) for x, y in zip(a["routes"], b["routes"])), \
        "the float32 twin and the float64 restatement take different pool / ReLU routes: choose another case"
    norms = [n for o in o64 for n in (o["actor_norm"], o["critic_norm"])]
    print("%s: norms %s" % (cid, [round(n, 3) for n in norms]))
    assert (min(norms) > clip) if clip < 1 else (max(norms) < clip), norms
    for name, w, t, b in zip(R.VECTORS, want, twin, R.bounds(P, want)):
        if name == "v" and not opt.startswith("adam"):
            continue
        err = float(np.linalg.norm(t - w))
        print("  %-13s twin |err| %.3e  bound %.3e  (%.2f of it)" % (name, err, b, err / b))
        assert err <= b, (cid, name, err, b)
        if name in R.VECTORS[:4]:
            assert float(np.linalg.norm(t - w)) <= R.PARAM_REL * float(np.linalg.norm(w)), (cid, name)


def _applicable(opt, clip):
    faults = []
    if opt.startswith("adam"):
        faults += ["shared_t", "no_bias_correction", "eps_in_sqrt"]
    if clip < 1:                       # (above the norms every scale is 1: where the clip sits changes nothing)
        faults.append("clip_after_moments")
    return faults


@pytest.mark.parametrize("cid,opt,shape_name,clip,tau", R.grid(), ids=[c[0] for c in R.grid()])
def test_each_planted_fault_moves_a_vector_by_more_than_the_gpu_tolerance(cid, opt, shape_name, clip, tau):
    _specs, P, _ep, _idxs, _b = _case(shape_name)
    for fault in _applicable(opt, clip):
        first = fault == "shared_t"           # (the counts differ only after a call that trains one list: the GPU module's actor-first case)
        want, _s, _o = _run(shape_name, opt, clip, tau, "f64", None, first)
        got, _s2, _o2 = _run(shape_name, opt, clip, tau, "f64", fault, first)
        ratios = {name: float(np.linalg.norm(g - w)) / b for name, g, w, b in zip(R.VECTORS, got, want, R.bounds(P, want, R.NB + int(first)))
                  if b > 0}                   # (Momentum has no v)
        print("%s %-20s %s" % (cid, fault, {k: round(v, 1) for k, v in ratios.items()}))
        assert max(ratios.values()) > 1.0, (cid, fault, ratios)
        if fault != "clip_after_moments":     # (the slots are the same under these three: it is the parameters that must show them)
            assert max(ratios[k] for k in R.VECTORS[:4]) > 1.0, (cid, fault, ratios)
