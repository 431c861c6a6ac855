"""Twin Q heads without a GPU: the float64 restatement (tests/twin_np.py) against torch autograd, the command line, the layout, the
conditioning of the cases tests/test_gpu_twin_q.py shares -- each head is the minimum on at least a quarter of the rows of every compared
minibatch, the float32 evaluation stays inside the GPU test's bounds on the float64 routes, no route is closer to a tie than float32 can
decide -- and the power of that comparison: every planted fault moves a compared vector by at least ten times the GPU test's bound."""
import functools

import numpy as np
import pytest

from oracle import ddpg_np as O
from tests import ddpg_opt_np as R
from tests import td3_np as T3
from tests import twin_np as W

POWER = 10.0          # the smallest factor the earlier feature tests accepted (tests/test_policy_delay_host.py)


# ---- the restatement against torch autograd, float64
@pytest.mark.parametrize("pixel", [True, False], ids=["pixel", "lowdim"])
def test_the_twin_critics_gradients_against_torch_autograd(pixel):
    import torch
    from oracle.ddpg_torch import TorchDDPG
    rng = np.random.default_rng(3)
    A, B = 3, 6
    kw = dict(pixel=True, H=8, W=8, C=3) if pixel else dict(pixel=False, state_elems=11)
    aspec, cspec = O.NetSpec("actor", A, [7], **kw), O.NetSpec("critic", A, [9, 6], **kw)
    plain = O.init_params(cspec, rng)
    plain = plain + rng.normal(0, 0.05, plain.shape).astype(np.float32)
    flat = np.concatenate([plain, W.twin_tail(cspec, rng)[0]]).astype(np.float64)
    net = W.TwinCritic(cspec, flat, np.float64)
    state = rng.uniform(0, 1, (B, 8, 8, 3)) if pixel else rng.standard_normal((B, 11))
    a, y, w = rng.uniform(-1, 1, (B, A)), rng.standard_normal((B, 1)), rng.uniform(0.2, 1, (B, 1))
    c = net.forward(state, action=a)
    td1, td2 = c["out"] - y, c["out2"] - y
    grads, d_action = net.backward(c, 2.0 * td1 * w / B, 2.0 * td2 * w / B)
    got = W.flatten_grads(cspec, grads, np.float64)
    # torch: the same loss, by autograd
    t = TorchDDPG(aspec, cspec, O.init_params(aspec, rng), plain, dtype=torch.float64)
    p1 = {n: torch.tensor(np.asarray(v), dtype=torch.float64, requires_grad=True) for n, v in net.h1.p.items()}
    p2 = {n: torch.tensor(np.asarray(v), dtype=torch.float64, requires_grad=True) for n, v in net.p2.items()}
    ta = torch.tensor(a, requires_grad=True)
    feat = t._trunk(cspec, p1, torch.tensor(state))
    h = feat
    k = W.cat_index(cspec)
    for name, _i, _o, act, cat in cspec.fc[:k]:
        h = torch.relu(h @ p1[name + "/weights"] + p1[name + "/biases"])
    x = torch.cat([h, ta], dim=1)

    def tail(p, suffix):
        z = x
        for name, _i, _o, act, _cat in cspec.fc[k:]:
            z = z @ p[name + suffix + "/weights"] + p[name + suffix + "/biases"]
            z = torch.relu(z) if act == "relu" else z
        return z
    q1, q2 = tail(p1, ""), tail(p2, "b")
    assert np.allclose(q1.detach().numpy(), c["out"], rtol=1e-12, atol=1e-12) and np.allclose(q2.detach().numpy(), c["out2"], rtol=1e-12, atol=1e-12)
    loss = (torch.tensor(w) * ((q1 - torch.tensor(y)) ** 2 + (q2 - torch.tensor(y)) ** 2)).mean()
    names = [n for n, _s in W.full_layout(cspec)]
    allp = dict(p1, **p2)
    tg = torch.autograd.grad(loss, [allp[n] for n in names], retain_graph=True)
    want = np.concatenate([g.numpy().ravel() for g in tg])
    assert got.shape == want.shape == (W.num_params(cspec),)
    assert np.allclose(got, want, rtol=1e-9, atol=1e-12 * np.abs(want).max()), float(np.abs(got - want).max())
    dq1, = torch.autograd.grad(q1.sum(), ta)
    assert np.allclose(d_action * 0 + net.d_action(c, 1), dq1.numpy(), rtol=1e-9, atol=1e-14)
    # (head 2 matters: the plain critic's gradient of td_1 alone is another vector below the concat layer)
    alone, _ = net.backward(c, 2.0 * td1 * w / B, 0.0 * td2, share_head2=False)
    first = cspec.fc[0][0] + "/weights"
    if k > 0:
        assert np.abs(alone[first] - grads[first]).max() > 1e-3 * np.abs(grads[first]).max()


# ---- the command line
def test_the_parser_takes_the_flag_and_the_default_is_off():
    from cartpoleplusplus_amd import ddpg_cartpole as D
    o = D.build_parser().parse_args([])
    assert not hasattr(o, "twin_q") and D.twin_q(o) is False and D.default_opts().twin_q is False
    assert D.twin_q(D.build_parser().parse_args(["--twin-q"])) is True
    assert D.twin_q(D.default_opts(twin_q=True)) is True
    with pytest.raises(SystemExit):
        D.build_parser().parse_args(["--twin-q", "2"])


def test_naf_does_not_take_the_flag():
    from cartpoleplusplus_amd import naf_cartpole as F
    assert "twin_q" not in vars(F.build_parser().parse_args([]))
    with pytest.raises(SystemExit):
        F.build_parser().parse_args(["--twin-q"])


# ---- the layout
@pytest.mark.parametrize("pixel", [True, False], ids=["pixel", "lowdim"])
def test_the_prefix_of_the_layout_is_the_plain_critics(pixel):
    kw = dict(pixel=True, H=16, W=16, C=3) if pixel else dict(pixel=False, state_elems=28)
    spec = O.NetSpec("critic", 2, [100, 100, 50], **kw)
    full, plain = W.full_layout(spec), spec.layout()
    assert full[:len(plain)] == plain and W.num_params(spec) > spec.num_params()
    tail = [n for n, _s in full[len(plain):]]
    if pixel:
        assert tail == ["hidden3b/weights", "hidden3b/biases", "q_valueb/weights", "q_valueb/biases"]
        assert W.num_params(spec) - spec.num_params() == 2650 + 51
    else:
        assert tail == ["h0b/weights", "h0b/biases", "h1b/weights", "h1b/biases", "h2b/weights", "h2b/biases", "q_valueb/weights", "q_valueb/biases"]
        assert W.num_params(spec) == 2 * spec.num_params()
    flat = np.arange(W.num_params(spec), dtype=np.float64)
    net = W.TwinCritic(spec, flat, np.float64)
    assert np.array_equal(net.flat(), flat) and np.array_equal(net.h1.flat(), flat[:spec.num_params()])


# ---- conditioning and power, on the GPU module's cases
@functools.lru_cache(maxsize=None)
def _inputs(cid):
    return W.case_inputs(W.case_of(cid))


def _weights(cid):
    return W.case_weights(W.case_of(cid)) if "weighted" in cid else None


@functools.lru_cache(maxsize=None)
def _run(cid, dt_name="f64", fault=None):
    got, counts, outs, ref = W.run_case(W.case_of(cid), _inputs(cid), np.float64 if dt_name == "f64" else np.float32, fault, weights=_weights(cid))
    return got, counts, outs, ref.min_share


def _compared(opt):
    return [n for n in T3.VECTORS if not (n == "v" and opt != "adam") and not (n == "m" and opt == "gradient-descent")]


IDS = [c[0] for c in W.CASES]


@pytest.mark.parametrize("cid", IDS)
def test_each_head_is_the_minimum_on_a_quarter_of_the_rows(cid):
    _got, _counts, _outs, share = _run(cid)
    print("%s  share of rows whose minimum is head 1's, per minibatch: %s" % (cid, ["%.2f" % s for s in share]))
    assert len(share) == W.NB
    assert all(W.MIN_SHARE <= s <= 1.0 - W.MIN_SHARE for s in share), "one head is the minimum on nearly every row: replace the case"


@pytest.mark.parametrize("cid", IDS)
def test_the_float32_evaluation_stays_inside_the_gpu_bounds(cid):
    case = W.case_of(cid)
    opt, d, clip = case[4], case[5], case[7]
    P = _inputs(cid)[1]
    want, counts, o64, _s = _run(cid)
    twin, _c, o32, _s2 = _run(cid, "f32")
    nb_, steps_ = W.structure(case)
    assert list(counts) == [W.NB // d, W.NB] and nb_ * steps_ == W.NB
    assert all(np.array_equal(x, y) for a, b in zip(o64, o32) for x, y in zip(a["routes"], b["routes"])), \
        "the float32 evaluation and the float64 restatement take different pool / ReLU routes: choose another case"
    norms = [n for o in o64 for n in (o["actor_norm"], o["critic_norm"])]
    assert (min(norms) > clip) if clip < 1 else (max(norms) < clip), norms
    ties = [o["tie"] for o in o64]
    print("%s  closest call per minibatch %s (floor %.2e)" % (cid, ["%.2e" % t for t in ties], T3.TIE_FLOOR))
    assert min(ties) > T3.TIE_FLOOR, "a route of this case is closer to a tie than float32 can decide: choose another case"
    for name, w, t, b in zip(T3.VECTORS, want, twin, W.bounds(P, want, W.NB)):
        if name not in _compared(opt):
            continue
        err = float(np.linalg.norm(t - w))
        print("%s  %-13s float32 |err| %.3e  bound %.3e  (%.2f of it)" % (cid, name, err, b, err / b))
        assert err <= b, (cid, name, err, b)
        if name in T3.VECTORS[:4]:
            assert err <= R.PARAM_REL * float(np.linalg.norm(w)), (cid, name)


def test_the_graph_case_meets_the_same_conditions():
    case, nb, steps, _ss = W.GRAPH_CASE
    inp = W.graph_inputs()
    P, rows = inp[1], inp[3]
    assert len(inp[4]) == steps * nb and rows.min() >= 0 and rows.max() < W.ROWS
    want, counts, o64, ref = W.run_case(case, inp, nb=nb, steps=steps)
    twin, _c, o32, _r = W.run_case(case, inp, np.float32, nb=nb, steps=steps)
    assert list(counts) == [steps * nb // 2, steps * nb] and ref.schedule == T3.expected_schedule(2, steps * nb)
    print("graph case: share of rows whose minimum is head 1's %s; closest calls %s" % (ref.min_share, ["%.2e" % o["tie"] for o in o64]))
    assert all(W.MIN_SHARE <= s <= 1.0 - W.MIN_SHARE for s in ref.min_share)
    assert min(o["tie"] for o in o64) > T3.TIE_FLOOR
    assert all(np.array_equal(x, y) for a, b in zip(o64, o32) for x, y in zip(a["routes"], b["routes"]))
    for name, w, t, b in zip(T3.VECTORS, want, twin, W.bounds(P, want, steps * nb)):
        err = float(np.linalg.norm(t - w))
        print("graph case  %-13s float32 |err| %.3e  bound %.3e  (%.2f of it)" % (name, err, b, err / b))
        assert err <= b and (name not in T3.VECTORS[:4] or err <= R.PARAM_REL * float(np.linalg.norm(w))), (name, err, b)


def _applicable(case):
    cid, shape_name, _A, _B, _opt, _d, sm, clip, _tau = case
    faults = ["max_for_min", "target_q1_only", "loss_td1_only", "head2_own_target", "actor_follows_q2", "actor_follows_min",
              "target_head2_not_updated"]
    if shape_name != "lowdim":                      # (a low-dimensional critic has no layer below the concat layer)
        faults.append("head2_missing_from_shared_grad")
    if sm is not None:
        faults.append("two_noise_draws")
    if "weighted" in cid:
        faults.append("weight_on_td1_only")
    if clip < 1:
        faults.append("head2_outside_clip_norm")
    return faults


@pytest.mark.parametrize("cid", IDS)
def test_each_planted_fault_moves_a_vector_by_ten_times_the_gpu_bound(cid):
    case = W.case_of(cid)
    opt = case[4]
    P = _inputs(cid)[1]
    want, _c, _o, _s = _run(cid)
    for fault in _applicable(case):
        got, _c2, _o2, _s2 = _run(cid, "f64", fault)
        ratios = {name: float(np.linalg.norm(g - w)) / b for name, g, w, b in zip(T3.VECTORS, got, want, W.bounds(P, want, W.NB))
                  if name in _compared(opt) and b > 0}
        print("%s %-32s %s" % (cid, fault, {k: round(v, 1) for k, v in ratios.items()}))
        assert max(ratios.values()) > POWER, (cid, fault, ratios)
        if fault.startswith("actor_follows"):
            assert ratios["actor"] > POWER, (cid, fault, ratios)
        if fault == "target_head2_not_updated":
            assert ratios["target_critic"] > POWER, (cid, fault, ratios)


def test_every_fault_is_seen_by_some_case():
    seen = set()
    for case in W.CASES:
        seen.update(_applicable(case))
    assert seen == set(W.FAULTS)


def test_check_loss_is_the_twin_formula_without_noise():
    cid = "A4-B8-smoothed"
    specs, P, _ep, _idxs, batches = _inputs(cid)
    ref = W.restatement(specs, P, np.float64, W.hyper_of(W.case_of(cid)), smoothing=W.SMOOTHING)
    loss, td, q = ref.check_loss(batches[0])
    cg = ref.last_cg
    assert ref.tps_n == 0 and cg["noise"] is None
    assert abs(loss - float(np.mean(cg["td"] ** 2 + cg["td2"] ** 2))) < 1e-15 and np.array_equal(td, cg["td"]) and np.array_equal(q, cg["q"])
