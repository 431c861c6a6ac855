"""The actor on the minimum head, on the host: what tests/test_gpu_actor_min.py's comparisons can see.  Everything here is asserted on the
float64 restatement tests/actor_min_np.py alone (and its float32 twin): the cases' conditions, the twin inside the GPU test's bars, every
planted fault outside them by more than ten times, and the command line's flag."""
import numpy as np
import pytest

from tests import actor_min_np as M
from tests import twin_np as W

_RUNS = {}


def _run(cid):
    """the case's float64 run with every fault probed on each minibatch's starting state, computed once and shared, left unchanged"""
    if cid not in _RUNS:
        if cid.startswith("sac"):
            case = M.sac_case_of(cid)
            inputs = M.sac_inputs(case)
            vec, ags, outs, ref, probed = M.run_sac(case, inputs, probe=M.FAULTS)
        else:
            case = M.case_of(cid)
            inputs = M.case_inputs(case)
            vec, ags, _cgs, outs, ref, probed = M.run_case(case, inputs, weights=M.case_weights(case), probe=M.FAULTS)
        _RUNS[cid] = (case, inputs, vec, ags, outs, ref, probed)
    return _RUNS[cid]


ALL = [c[0] for c in M.CASES] + [c[0] for c in M.SAC_CASES]


@pytest.mark.parametrize("cid", ALL)
def test_the_conditions_hold_in_every_compared_minibatch(cid):
    case, _inputs, _vec, ags, _outs, _ref, _p = _run(cid)
    share, margin = M.shares(ags)
    print(cid, "share of head 1:", share, "smallest |Q1 - Q2|:", margin)
    assert min(margin) >= M.TIE_MARGIN, margin          # no row is ever left out of a comparison
    if case[3] == 1:      # one row: a quarter of it has no meaning -- both heads are followed among the case's minibatches
        assert len(set(int(a["sel"][0]) for a in ags)) == 2, share
    else:
        assert all(M.MIN_SHARE <= s <= 1 - M.MIN_SHARE for s in share), share


@pytest.mark.parametrize("cid", ALL)
def test_the_seed_is_the_first_that_meets_the_conditions(cid):
    """the share and the margin of every earlier seed (the float32 twin's part of the choice is test_the_float32_twin's, on the seed kept)"""
    sac = cid.startswith("sac")
    case = M.sac_case_of(cid) if sac else M.case_of(cid)
    kept = (M.SAC_SEEDS if sac else M.SEEDS)[cid]
    for seed in range(1, min(kept, 6)):      # (the five first: a case that needed eighty seeds is not searched again on every run)
        if sac:
            inputs = M.sac_inputs(case, seed)
            _v, ags, _o, ref, _p = M.run_sac(case, inputs)
            tshare = all(M.MIN_SHARE <= s <= 1 - M.MIN_SHARE for s in ref.min_share)
        else:
            inputs = M.case_inputs(case, seed)
            _v, ags, _c, _o, _r, _p = M.run_case(case, inputs, weights=M.case_weights(case))
            tshare = True
        share, margin = M.shares(ags)
        ok = min(margin) >= M.TIE_MARGIN and tshare and (len(set(int(a["sel"][0]) for a in ags)) == 2 if case[3] == 1 else
                                                         all(M.MIN_SHARE <= s <= 1 - M.MIN_SHARE for s in share))
        if ok and not sac:      # ... then the float32 twin rejected it: routes, the choice or a bar
            _v32, a32, _c32, o32, _r32, _p32 = M.run_case(case, inputs, np.float32, weights=M.case_weights(case))
            _v, ags, _c, outs, _r, _p = M.run_case(case, inputs, weights=M.case_weights(case))
            ok = all(np.array_equal(a["sel"], b["sel"]) for a, b in zip(ags, a32)) and \
                all(np.array_equal(x, y) for a, b in zip(outs, o32) for x, y in zip(a["routes"], b["routes"])) and \
                all(np.abs(a[k] - b[k]).max() < M.P_BAR for a, b in zip(ags, a32) for k in ("actions", "q1", "q2", "dq_da"))
        if ok and case[3] == 1:      # ... or, with three rows in all, a fault that chooses by other values chose the same
            probed = M.run_case(case, inputs, probe=M.FAULTS)[5]
            ok = all(max(float(np.abs(p[0] - a["dq_da"]).max()) for p, a in zip(probed[f], ags)) > 10 * M.P_BAR
                     for f in M.FAULTS if f != "tie_goes_to_q2" and (cid, f) not in BLIND)
        assert not ok, (cid, seed)


@pytest.mark.parametrize("cid", ALL)
def test_the_float32_twin_stays_inside_the_bars(cid):
    case, inputs, vec, ags, outs, _ref, _p = _run(cid)
    if cid.startswith("sac"):
        vec32, a32, o32, _r, _p32 = M.run_sac(case, inputs, np.float32)
    else:
        vec32, a32, _c, o32, _r, _p32 = M.run_case(case, inputs, np.float32, weights=M.case_weights(case))
        for name, g, w, b in zip(W.T3.VECTORS, vec32, vec, W.bounds(inputs[1], vec, M.NB)):
            err = float(np.linalg.norm(np.asarray(g, np.float64) - w))
            assert err <= b, (cid, name, err, b)
    for k, (a, b) in enumerate(zip(ags, a32)):
        assert np.array_equal(a["sel"], b["sel"]), (cid, k)
        for key in ("actions", "q1", "q2", "dq_da"):
            err = float(np.abs(a[key] - b[key]).max())
            assert err < M.P_BAR, (cid, k, key, err)
        g, w = np.asarray(b["grads"], np.float64), a["grads"]
        assert np.linalg.norm(g - w) <= 2e-5 * np.linalg.norm(w), (cid, k)
    for a, b in zip(outs, o32):
        assert all(np.array_equal(x, y) for x, y in zip(a["routes"], b["routes"])), cid


# which faults a case cannot see, and why: with one row per minibatch the batch means are the row's values
BLIND = {("A2-B1-sgd", "one_choice_per_batch")}


@pytest.mark.parametrize("fault", [f for f in M.FAULTS if f != "tie_goes_to_q2"])
@pytest.mark.parametrize("cid", ALL)
def test_every_fault_moves_dq_da_by_ten_bars(cid, fault):
    """on the case's own minibatches, each from the state the unfaulted run reaches: the largest move of dQ/da over the case's minibatches"""
    _case, _inputs, _vec, ags, _outs, _ref, probed = _run(cid)
    move = max(float(np.abs(p[0] - a["dq_da"]).max()) for p, a in zip(probed[fault], ags))
    print(cid, fault, "moves dq_da by %.3e" % move)
    if (cid, fault) in BLIND:
        assert move == 0.0
        return
    assert move > 10 * M.P_BAR, (cid, fault, move)


@pytest.mark.parametrize("cid", ["A2-B7-weighted", "lowdim-A3-B5-td3"])
def test_a_tie_is_head_ones(cid):
    """head 2 a copy of head 1: every row ties, every row follows head 1 -- and head 2 under the planted fault"""
    case = M.case_of(cid)
    inputs = M.tie_inputs(case, M.case_inputs(case))
    specs, P, _ep, _idxs, batches = inputs
    ref = M.restatement(case, specs, P)
    ag = ref.actor_gradients(batches[0][0])
    assert np.array_equal(ag["q1"], ag["q2"]) and (ag["sel"] == 1).all()
    bad = M.restatement(case, specs, P, fault="tie_goes_to_q2").actor_gradients(batches[0][0])
    assert (bad["sel"] == 2).all()
    assert np.array_equal(ag["dq_da"], bad["dq_da"])      # (the copy's gradient: only sel can show this fault)


def test_the_restatement_with_the_switch_off_is_the_twin_learners():
    """follows_q1 is tests.twin_np.TwinDDPG, bit for bit: the subclass changes the actor's objective and nothing else"""
    case = M.case_of("A3-B5-smoothed")
    inputs = M.case_inputs(case)
    off = M.run_case(case, inputs, fault="follows_q1")[0]
    want = W.run_case(case[:9], inputs, nb=1, steps=M.NB)[0]
    assert all(np.array_equal(a, b) for a, b in zip(off, want))
    on = M.run_case(case, inputs)[0]
    assert not np.array_equal(on[0], want[0]) and not np.array_equal(on[1], want[1])      # (the critic's trunk is not touched by the actor's list,
    # but its later minibatches see other actions only through the target actor: the critic differs from the second minibatch on)


# ---- the command line
def test_the_flag_is_absent_unless_given_and_refused_without_twin_q():
    from cartpoleplusplus_amd import ddpg_cartpole as D
    p = D.build_parser()
    assert not hasattr(p.parse_args([]), "actor_min_q") and not D.actor_min_q(p.parse_args([]))
    o = p.parse_args(["--twin-q", "--actor-min-q"])
    assert o.actor_min_q is True and D.actor_min_q(o)
    assert not D.actor_min_q(p.parse_args(["--twin-q"]))
    with pytest.raises(SystemExit) as e:
        D.actor_min_q(p.parse_args(["--actor-min-q"]))
    assert "--twin-q" in str(e.value)
    assert D.default_opts().actor_min_q is False
    for combo in (["--distributional-critic", "--v-min", "0", "--v-max", "1"], ["--quantile-critic"]):
        with pytest.raises(SystemExit):      # (neither critic can be twin)
            D.actor_min_q(p.parse_args(combo + ["--actor-min-q"]))
    assert "unless --actor-min-q" in " ".join(p.format_help().split())


def test_the_agent_refuses_the_flag_before_anything_exists_on_the_device(monkeypatch):
    from cartpoleplusplus_amd import ddpg_cartpole as D
    from tests.helpers import FakeEnv
    made = []
    monkeypatch.setattr(D.replay_memory, "ReplayMemory", lambda *a, **k: made.append("replay") or (_ for _ in ()).throw(AssertionError("built")))
    old = D.opts
    try:
        D.set_opts(D.default_opts(actor_min_q=True))
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
    for name in ("cpp_ddpg_set_actor_min_q", "cpp_ddpg_last_actor_min"):
        assert name in _lib.SIGNATURES and re.search(r"\bint %s\(" % name, header), name
