"""The behaviour-cloning actor term, on the host: what tests/test_gpu_behaviour_cloning.py's comparisons can see.  Everything here is asserted
on the float64 restatement tests/bc_np.py alone (and its float32 twin): the restatement against torch autograd, the cases' conditions, the
twin inside the GPU test's bars, every planted fault outside at least one of them, and the command line's flags."""
import numpy as np
import pytest

from tests import actor_min_np as AM
from tests import bc_np as Bc
from tests import twin_np as W

_RUNS = {}
SMALL = [c[0] for c in Bc.CASES if c[0] not in Bc.BIG]


def _run(cid):
    """the case's float64 run with every fault probed on each minibatch's starting state, computed once and shared, left unchanged"""
    if cid not in _RUNS:
        case = Bc.case_of(cid)
        inputs = Bc.case_inputs(case)
        vec, ags, cgs, outs, ref, probed = Bc.run_case(case, inputs, weights=Bc.case_weights(case), probe=Bc.FAULTS)
        _RUNS[cid] = (case, inputs, vec, ags, outs, ref, probed)
    return _RUNS[cid]


# ---- the restatement is the gradient of the loss it names
@pytest.mark.parametrize("floor", [Bc.Q_FLOOR, Bc.HIGH_FLOOR])
def test_the_restatement_against_torch_autograd(floor):
    """B times the paper's loss, -lambda.detach() * Q.sum() + B * mse(mu, a), differentiated by torch on a small actor / critic pair whose
    weights are the restatement's: grad_ys at the actor's output, and the actor's list through tanh"""
    import torch
    case = Bc.case_of("lowdim-A3-B5")
    specs, P, _ep, _idxs, batches = Bc.case_inputs(case)
    ref = Bc.restatement(case, specs, P)
    ref.bc_floor = floor
    s1, a = np.asarray(batches[0][0], np.float64), np.asarray(batches[0][1], np.float64)
    ref.fed = a
    ag = ref.actor_gradients(s1)
    B, A = a.shape
    # the actor's pre-activation of its last layer, so that torch differentiates through the tanh the restatement's backward applies
    z = torch.tensor(np.arctanh(np.clip(ag["actions"], -1 + 1e-15, 1 - 1e-15)), dtype=torch.float64, requires_grad=True)
    mu = torch.tanh(z)
    mu.retain_grad()

    def critic(action):      # the restatement's critic as a torch function of the action (the state's path is a constant)
        sp = specs[1]
        x = torch.tensor(s1.reshape(B, -1))
        for name, _ni, _no, act, cat in sp.fc:
            w = torch.tensor(np.asarray(ref.critic.p[name + "/weights"], np.float64))
            b = torch.tensor(np.asarray(ref.critic.p[name + "/biases"], np.float64))
            if cat:
                x = torch.cat([x, action], dim=1)
            x = x @ w + b
            if act == "relu":
                x = torch.relu(x)
        return x
    q = critic(mu)
    assert np.abs(q.detach().numpy() - ag["q_mu"]).max() < 1e-12
    lam = Bc.ALPHA / max(float(q.detach().abs().mean()), floor)
    loss = -lam * q.sum() + B * ((mu - torch.tensor(a)) ** 2).mean()
    loss.backward()
    assert abs(lam - ag["lambda"]) <= 1e-12 * lam
    assert np.abs(mu.grad.numpy() - ag["g"]).max() < 1e-11, np.abs(mu.grad.numpy() - ag["g"]).max()
    assert np.abs(z.grad.numpy() - ag["adz"]).max() < 1e-11
    assert np.abs(ag["bc_rows"] - ((ag["actions"] - a) ** 2).mean(axis=1)).max() < 1e-15


# ---- the cases' conditions, asserted and not assumed
@pytest.mark.parametrize("cid", SMALL)
def test_the_conditions_hold_in_every_compared_minibatch(cid):
    case, inputs, _vec, ags, _outs, _ref, _p = _run(cid)
    floor = Bc.floor_of(case)
    ms = [a["m"] for a in ags]
    print(cid, "m", ms, "lambda", [a["lambda"] for a in ags], "rows with Q > 0", [int((a["q_mu"] > 0).sum()) for a in ags])
    for k, (a, b) in enumerate(zip(ags, inputs[4])):
        assert a["g"].shape == np.asarray(b[1]).shape and a["bc_rows"].shape == (case[3],), (cid, k)      # no row is ever left out
        assert abs(a["m"] - floor) >= Bc.FLOOR_GAP * floor, (cid, k, a["m"])
        on_floor = a["m"] < floor
        assert on_floor or a["m"] >= Bc.M_MIN, (cid, k, a["m"])
        assert on_floor == ("floor" in case[9]), (cid, k, a["m"])
        assert a["lambda"] == Bc.ALPHA / (floor if on_floor else a["m"])
        if "sel" in a:
            assert float(np.abs(a["q1"] - a["q2"]).min()) >= AM.TIE_MARGIN, (cid, k)
            assert AM.MIN_SHARE <= float((a["sel"] == 1).mean()) <= 1 - AM.MIN_SHARE, (cid, k, a["sel"])


def test_both_branches_of_the_max_and_both_signs_of_q_are_among_the_cases():
    on_floor, signs = set(), set()
    for cid in SMALL:
        case, _i, _v, ags, _o, _r, _p = _run(cid)
        for a in ags:
            on_floor.add(a["m"] < Bc.floor_of(case))
            if (a["q_mu"] > 0).any() and (a["q_mu"] < 0).any():
                signs.add(cid)
    assert on_floor == {True, False} and signs, (on_floor, signs)


@pytest.mark.parametrize("cid", SMALL)
def test_the_float32_twin_stays_inside_the_bars(cid):
    case, inputs, vec, ags, outs, _ref, _p = _run(cid)
    A = case[2]
    vec32, a32, _c, o32, _r, _p32 = Bc.run_case(case, inputs, np.float32, weights=Bc.case_weights(case))
    for name, g, w, b in zip(W.T3.VECTORS, vec32, vec, W.bounds(inputs[1], vec, Bc.NB)):
        err = float(np.linalg.norm(np.asarray(g, np.float64) - w))
        assert err <= b, (cid, name, err, b)
    for k, (a, b) in enumerate(zip(ags, a32)):
        if "sel" in a:
            assert np.array_equal(a["sel"], b["sel"]), (cid, k)
        for key in ("actions", "q_mu", "dq_da"):
            assert float(np.abs(a[key] - b[key]).max()) < Bc.P_BAR, (cid, k, key)
        assert abs(b["lambda"] - a["lambda"]) <= Bc.lambda_bar(a["lambda"], a["m"]), (cid, k)
        assert (np.abs(b["g"] - a["g"]) <= Bc.g_bar(a["lambda"], a["m"], a["dq_da"], A)).all(), (cid, k)
        g, w = np.asarray(b["grads"], np.float64), a["grads"]
        assert np.linalg.norm(g - w) <= 2e-5 * np.linalg.norm(w), (cid, k)
    for a, b in zip(outs, o32):      # the float64 pool / ReLU routes
        assert all(np.array_equal(x, y) for x, y in zip(a["routes"], b["routes"])), cid


# ---- every fault leaves at least one bar on at least one case
@pytest.mark.parametrize("fault", Bc.FAULTS)
def test_every_fault_exceeds_a_bar_on_some_case(fault):
    """on the cases' own minibatches, each from the state the unfaulted run reaches: by how many bars (lambda, g, the reported dq_da, the
    actor's pre-clip list) the GPU test's comparison would see the fault, the largest over the cases' minibatches"""
    worst = {}
    for cid in SMALL:
        case, _inputs, _vec, ags, _outs, _ref, probed = _run(cid)
        worst[cid] = max(Bc.seen(a, p, case[2]) for p, a in zip(probed[fault], ags))
    print(fault, {k: "%.3g" % v for k, v in worst.items()})
    assert max(worst.values()) > 10.0, (fault, worst)
    if fault == "follows_q1_under_min":      # only the cases whose actor follows the minimum can show it
        assert all(v == 0.0 for k, v in worst.items() if Bc.case_of(k)[9].get("critic") != "min")
        assert all(v > 10.0 for k, v in worst.items() if Bc.case_of(k)[9].get("critic") == "min")
    if fault == "no_floor":                  # ... and only the floor branch this one
        assert all((v > 10.0) == ("floor" in Bc.case_of(k)[9]) for k, v in worst.items())


def test_the_restatement_with_alpha_zero_grad_ys_is_the_plain_learners():
    """the cloning term and lambda taken out by hand: -dq_da, the class the restatement derives from"""
    case = Bc.case_of("A2-B7-adam-clipped")
    specs, P, _ep, _idxs, batches = Bc.case_inputs(case)
    ref = Bc.restatement(case, specs, P)
    ref.fed = batches[0][1]
    ag = ref.actor_gradients(batches[0][0])
    plain = Bc.T3.DelayedDDPG.actor_gradients(ref, batches[0][0])
    assert np.array_equal(ag["dq_da"], plain["dq_da"]) and np.array_equal(ag["actions"], plain["actions"])
    A = case[2]
    assert np.allclose(ag["g"], -ag["lambda"] * plain["dq_da"] + (2.0 / A) * (ag["actions"] - batches[0][1]), rtol=0, atol=1e-13)


# ---- the command line
def test_the_flags_are_absent_unless_given_and_refuse_what_cannot_be_meant():
    from cartpoleplusplus_amd import ddpg_cartpole as D
    p = D.build_parser()
    o = p.parse_args([])
    assert not hasattr(o, "bc_alpha") and not hasattr(o, "bc_q_floor") and D.behaviour_cloning(o) == (0.0, 1e-3)
    assert D.behaviour_cloning(p.parse_args(["--bc-alpha", "2.5"])) == (2.5, 1e-3)
    assert D.behaviour_cloning(p.parse_args(["--bc-alpha", "2.5", "--bc-q-floor", "0.5"])) == (2.5, 0.5)
    assert D.behaviour_cloning(p.parse_args(["--bc-alpha", "1", "--twin-q", "--actor-min-q"])) == (1.0, 1e-3)
    d = D.default_opts()
    assert d.bc_alpha is None and d.bc_q_floor is None and D.behaviour_cloning(d) == (0.0, 1e-3)
    assert D.behaviour_cloning(D.default_opts(bc_alpha=2.5)) == (2.5, 1e-3)
    for args, word in ((["--bc-q-floor", "0.5"], "--bc-alpha"),
                       (["--bc-alpha", "-1"], "--bc-alpha"), (["--bc-alpha", "nan"], "--bc-alpha"), (["--bc-alpha", "inf"], "--bc-alpha"),
                       (["--bc-alpha", "1", "--bc-q-floor", "0"], "--bc-q-floor"), (["--bc-alpha", "1", "--bc-q-floor", "-2"], "--bc-q-floor"),
                       (["--bc-alpha", "1", "--bc-q-floor", "nan"], "--bc-q-floor"),
                       (["--bc-alpha", "1", "--soft-actor-critic"], "--soft-actor-critic"),
                       (["--bc-alpha", "1", "--distributional-critic"], "--distributional-critic"),
                       (["--bc-alpha", "1", "--quantile-critic"], "--quantile-critic")):
        with pytest.raises(SystemExit) as e:
            D.behaviour_cloning(p.parse_args(args))
        assert word in str(e.value), (args, str(e.value))
    text = " ".join(p.format_help().split())
    assert "2.5" in text.split("--bc-alpha ALPHA")[-1][:300] and "--bc-q-floor F " in text


def test_the_agent_refuses_the_flags_before_anything_exists_on_the_device(monkeypatch):
    from cartpoleplusplus_amd import ddpg_cartpole as D
    from tests.helpers import FakeEnv
    made = []
    monkeypatch.setattr(D.replay_memory, "ReplayMemory", lambda *a, **k: made.append("replay") or (_ for _ in ()).throw(AssertionError("built")))
    old = D.opts
    try:
        D.set_opts(D.default_opts(bc_q_floor=0.5))
        with pytest.raises(SystemExit):
            D.DeepDeterministicPolicyGradientAgent(FakeEnv((2, 2, 7), 2))
        assert not made
    finally:
        D.set_opts(old)


def test_the_abi_names_both_calls():
    import os
    import re
    from cartpoleplusplus_amd import _lib
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "cartpolepp_abi.h")).read()
    for name in ("cpp_ddpg_set_behaviour_cloning", "cpp_ddpg_last_behaviour_cloning"):
        assert name in _lib.SIGNATURES and re.search(r"\bint %s\(" % name, header), name
    assert "ddpg_cartpole.py:111-113" in header.split("cpp_ddpg_last_actor_min(")[1].split("cpp_ddpg_set_behaviour_cloning(")[0]
