"""The distributional critic without a GPU: the float64 restatement (tests/dist_np.py) against torch autograd -- the loss, the logit
gradient, dQ/da through the expectation --, the triangular projection against the floor / ceil scatter, its invariants, the command line,
the derivation of the two bars tests/test_gpu_distributional.py holds p, p' and m to, the conditioning of the cases the two modules
share, and the power of the GPU comparison: every planted fault moves a compared quantity by at least ten times its GPU bar."""
import functools

import numpy as np
import pytest

from oracle import ddpg_np as O
from tests import ddpg_opt_np as R
from tests import dist_np as W
from tests import td3_np as T3

POWER = 10.0          # the smallest factor the earlier feature tests accepted (tests/test_policy_delay_host.py)


# ---- the restatement against torch autograd, float64
@pytest.mark.parametrize("pixel", [True, False], ids=["pixel", "lowdim"])
def test_loss_logit_gradient_and_dq_da_against_torch_autograd(pixel):
    import torch
    from oracle.ddpg_torch import TorchDDPG
    rng = np.random.default_rng(4)
    A, B, N, v_min, v_max = 3, 6, 7, -1.5, 2.0
    kw = dict(pixel=True, H=8, W=8, C=3) if pixel else dict(pixel=False, state_elems=11)
    aspec, plain = O.NetSpec("actor", A, [7], **kw), O.NetSpec("critic", A, [9, 6], **kw)
    cspec = W.dist_spec(plain, N)
    assert cspec.layout()[-2:] == [("q_value/weights", (plain.fc[-1][1], N)), ("q_value/biases", (N,))] and plain.fc[-1][2] == 1
    flat = O.init_params(cspec, rng).astype(np.float64)
    flat = flat + rng.normal(0, 0.05, flat.shape)
    aflat = (O.init_params(aspec, rng) + rng.normal(0, 0.05, aspec.num_params())).astype(np.float64)
    ref = W.DistDDPG(aspec, cspec, aflat, flat, (N, v_min, v_max), np.float64)
    state = rng.uniform(0, 1, (B, 8, 8, 3)) if pixel else rng.standard_normal((B, 11))
    s2 = rng.uniform(0, 1, (B, 8, 8, 3)) if pixel else rng.standard_normal((B, 11))
    a, r = rng.uniform(-1, 1, (B, A)), rng.integers(0, 3, (B, 1)).astype(np.float64)
    mask, w = (rng.uniform(0, 1, (B, 1)) > 0.3).astype(np.float64), rng.uniform(0.2, 1, (B, 1))
    cg = ref.critic_gradients((state, a, r, mask, s2), w=w)
    ag = ref.actor_gradients(state)
    # torch: the critic from the same parameters, the loss by autograd with the projected target held constant
    t = TorchDDPG(aspec, plain, O.init_params(aspec, rng), O.init_params(plain, rng), dtype=torch.float64)
    p = {n: torch.tensor(np.asarray(v), dtype=torch.float64, requires_grad=True) for n, v in ref.critic.p.items()}
    z = torch.tensor(W.support(N, v_min, v_max)[0])

    def logits_of(st, act):
        h = t._trunk(cspec, p, torch.tensor(st))
        for name, _i, _o, kind, cat in cspec.fc:
            if cat:
                h = torch.cat([h, act], dim=1)
            h = h @ p[name + "/weights"] + p[name + "/biases"]
            h = torch.relu(h) if kind == "relu" else h
        return h
    ta = torch.tensor(a, requires_grad=True)
    lg = logits_of(state, ta)
    assert np.allclose(lg.detach().numpy(), cg["logits"], rtol=1e-11, atol=1e-11)
    logp = torch.log_softmax(lg, dim=1)
    lg.retain_grad()
    loss = (torch.tensor(w) * -(torch.tensor(cg["m"]) * logp).sum(dim=1, keepdim=True)).mean()
    names = [n for n, _s in cspec.layout()]
    tg = torch.autograd.grad(loss, [p[n] for n in names] + [lg], retain_graph=True)
    assert abs(float(loss.detach()) - float(cg["loss"])) < 1e-12 * max(1.0, abs(float(loss.detach())))
    assert np.allclose(cg["dz"], tg[-1].numpy(), rtol=1e-10, atol=1e-15), "logit gradient (w / B)(p - m)"
    want = np.concatenate([g.numpy().ravel() for g in tg[:-1]])
    assert np.allclose(cg["grads"], want, rtol=1e-9, atol=1e-12 * np.abs(want).max()), float(np.abs(cg["grads"] - want).max())
    # dQ/da through the expectation, at the actor's action
    act = torch.tensor(ag["actions"], requires_grad=True)
    q = (torch.softmax(logits_of(state, act), dim=1) * z).sum(dim=1, keepdim=True)
    assert np.allclose(q.detach().numpy(), ag["q"], rtol=1e-11, atol=1e-12)
    dq, = torch.autograd.grad(q.sum(), act)
    assert np.allclose(ag["dq_da"], dq.numpy(), rtol=1e-9, atol=1e-13), float(np.abs(ag["dq_da"] - dq.numpy()).max())
    assert np.abs(dq.numpy()).max() > 1e-3


# ---- the projection
SUPPORTS = ((51, -10.0, 10.0), (64, 0.0, 63.0), (2, 0.5, 1.5), (33, 0.0, 8.0), (7, -1.5, 2.0))


def _projection_rows(n_atoms, v_min, v_max, B=64, seed=0):
    """rows with rewards beyond both ends, terminal rows, n-step scales and -- where the support allows -- integer b"""
    rng = np.random.default_rng(seed + n_atoms)
    tp = W.softmax(rng.normal(0, 2.0, (B, n_atoms)))[0]
    span = v_max - v_min
    r = rng.uniform(v_min - 0.6 * span, v_max + 0.6 * span, (B, 1))
    r[::4] = np.round(r[::4])
    g = rng.choice([0.0, 1.0, 0.9, 0.9 ** 3], (B, 1))
    return tp, r, g


@pytest.mark.parametrize("sup", SUPPORTS, ids=lambda s: "N%d[%g,%g]" % s)
def test_the_triangular_form_is_the_floor_ceil_scatter_and_keeps_the_mass(sup):
    n_atoms, v_min, v_max = sup
    tp, r, g = _projection_rows(*sup)
    m = W.project(tp, r, g, n_atoms, v_min, v_max)
    want = W.scatter_projection(tp, r, g, n_atoms, v_min, v_max)
    assert np.abs(m - want).max() < 1e-15
    assert np.abs(m.sum(axis=1) - 1.0).max() < 1e-14 and m.min() >= 0.0
    z = W.support(n_atoms, v_min, v_max)[0]
    tz = r + g * z[None, :]
    free = ((tz > v_min) & (tz < v_max)).all(axis=1)           # no clamp binds: y = r + g Q'
    y, tq = (m * z).sum(axis=1), (tp * z).sum(axis=1)
    if free.any():
        assert np.abs(y[free] - (r[:, 0] + g[:, 0] * tq)[free]).max() < 1e-12 * max(1.0, abs(v_min), abs(v_max))
    assert (~free).any() and ((r[:, 0] > v_max).any() and (r[:, 0] < v_min).any())
    below, above = r[:, 0] + g[:, 0] * v_max <= v_min, r[:, 0] + g[:, 0] * v_min >= v_max      # the whole distribution beyond an end
    assert np.abs(m[below, 0] - 1.0).max(initial=0.0) < 1e-14 and np.abs(m[above, -1] - 1.0).max(initial=0.0) < 1e-14


def test_an_integer_b_keeps_its_whole_mass_where_the_scatter_as_often_coded_loses_it():
    n_atoms, v_min, v_max = 33, 0.0, 8.0          # delta = 1/4: b = 4 r + j on rows with g = 1
    rng = np.random.default_rng(2)
    tp = W.softmax(rng.normal(0, 2.0, (6, n_atoms)))[0]
    r, g = np.array([[0.0], [1.0], [2.0], [1.0], [0.0], [2.0]]), np.array([[1.0], [1.0], [1.0], [0.0], [0.0], [0.0]])
    m = W.project(tp, r, g, n_atoms, v_min, v_max)
    assert np.array_equal(m[0], tp[0])
    assert np.array_equal(m[1][4:-1], tp[1][:-5]) and abs(m[1][-1] - tp[1][-5:].sum()) < 1e-15      # shifted by 4 atoms, the top clamped
    assert m[3][4] == pytest.approx(1.0, abs=1e-15) and m[5][8] == pytest.approx(1.0, abs=1e-15)   # terminal rows: everything on atom 4 r
    lost = W.project(tp, r, g, n_atoms, v_min, v_max, fault="integer_b_loses_mass")
    assert np.abs(lost).max() == 0.0
    # continuity in b: a reward a hair off the integer moves m by that hair
    near = W.project(tp, r + 1e-9, g, n_atoms, v_min, v_max)
    assert np.abs(near - m).max() < 1e-8


def test_the_float32_row_functions_follow_float64():
    rng = np.random.default_rng(5)
    for n_atoms, v_min, v_max in SUPPORTS[:4]:
        lg, tl = rng.normal(0, 2.0, (9, n_atoms)), rng.normal(0, 2.0, (9, n_atoms))
        r, mask = rng.integers(0, 3, (9, 1)).astype(np.float64), (rng.uniform(0, 1, (9, 1)) > 0.3).astype(np.float64)
        a, b = W.rows(lg, tl, r, mask, 0.9, n_atoms, v_min, v_max), W.rows_f32(lg, tl, r, mask, 0.9, n_atoms, v_min, v_max)
        zmax = max(1.0, abs(v_min), abs(v_max))
        assert b["p"].dtype == np.float32 and b["m"].shape == (9, n_atoms)
        assert np.abs(a["p"] - b["p"]).max() < W.P_BAR and np.abs(a["m"] - b["m"]).max() < W.M_BAR
        for k in ("q", "tq", "y", "td"):
            assert np.abs(a[k] - b[k]).max() < W.ATOL * zmax, (k, n_atoms)


# ---- the command line
def test_the_parser_takes_the_options_and_they_are_absent_unless_given():
    from cartpoleplusplus_amd import ddpg_cartpole as D
    o = D.build_parser().parse_args([])
    for k in ("distributional_critic", "num_atoms", "v_min", "v_max", "n_step"):
        assert not hasattr(o, k), k
    assert D.distributional_critic(o) is None and D.distributional_critic(D.default_opts()) is None and D.n_step(o) == 1
    o = D.build_parser().parse_args(["--distributional-critic", "--v-min", "-10", "--v-max", "10"])
    assert D.distributional_critic(o) == (51, -10.0, 10.0)
    o = D.build_parser().parse_args(["--distributional-critic", "--num-atoms", "33", "--v-min", "0", "--v-max", "8", "--n-step", "3"])
    assert D.distributional_critic(o) == (33, 0.0, 8.0) and D.n_step(o) == 3
    assert D.distributional_critic(D.default_opts(distributional_critic=True, num_atoms=2, v_min=0.5, v_max=1.5)) == (2, 0.5, 1.5)


@pytest.mark.parametrize("argv", [["--distributional-critic"],                                              # no support
                                  ["--distributional-critic", "--v-min", "0"],
                                  ["--distributional-critic", "--v-max", "1"],
                                  ["--v-min", "0", "--v-max", "1"],                                         # options without the flag
                                  ["--num-atoms", "51"],
                                  ["--distributional-critic", "--v-min", "1", "--v-max", "1"],              # v_min >= v_max
                                  ["--distributional-critic", "--v-min", "2", "--v-max", "1"],
                                  ["--distributional-critic", "--v-min", "0", "--v-max", "inf"],
                                  ["--distributional-critic", "--v-min", "0", "--v-max", "1", "--num-atoms", "1"],
                                  ["--distributional-critic", "--v-min", "0", "--v-max", "1", "--num-atoms", "65"],
                                  ["--distributional-critic", "--v-min", "0", "--v-max", "1", "--twin-q"],
                                  ["--n-step", "0"], ["--n-step", "65"]],
                         ids=lambda a: " ".join(a))
def test_the_parsers_refusals(argv):
    from cartpoleplusplus_amd import ddpg_cartpole as D
    with pytest.raises(SystemExit):
        o = D.build_parser().parse_args(argv)
        D.distributional_critic(o)
        D.n_step(o)


def test_naf_does_not_take_the_options():
    from cartpoleplusplus_amd import naf_cartpole as F
    assert not {"distributional_critic", "num_atoms", "v_min", "v_max", "n_step"} & set(vars(F.build_parser().parse_args([])))
    with pytest.raises(SystemExit):
        F.build_parser().parse_args(["--distributional-critic"])


# ---- the cases the GPU module shares
@functools.lru_cache(maxsize=None)
def _inputs(cid):
    return W.case_inputs(W.case_of(cid))


def _weights(cid):
    return W.case_weights(W.case_of(cid)) if "weighted" in cid else None


@functools.lru_cache(maxsize=None)
def _run(cid, dt_name="f64", fault=None):
    return W.run_case(W.case_of(cid), _inputs(cid), np.float64 if dt_name == "f64" else np.float32, fault, weights=_weights(cid))[:3]


def _compared(opt):
    return [n for n in T3.VECTORS if not (n == "v" and opt != "adam") and not (n == "m" and opt == "gradient-descent")]


IDS = [c[0] for c in W.CASES]


def test_the_cases_hold_what_the_issue_asks_for():
    cases = W.CASES
    assert {c[3] for c in cases} >= {1, 5, 8} and {c[4] for c in cases} >= {2, 33, 51, 64} and {c[2] for c in cases} >= {1, 2, 9}
    assert {c[1] for c in cases} == {"16x16x3", "lowdim"}
    wide = [c for c in cases if W.zmax_of(c) > 10.0]
    assert [c[0] for c in wide] == ["A2-B8-N51-wide"]
    seen = set()
    for c in cases:
        b = _inputs(c[0])[4][0]
        r, mask = np.ravel(b[2]), np.ravel(b[3])
        g = mask * np.float32(c[7])
        z = W.support(*W.dist_of(c))[0]
        if (mask == 0).any():
            seen.add("terminal")
        tz = r[:, None] + g[:, None] * z[None, :]
        if (r > c[6]).any() and (tz > c[6]).any():          # a reward beyond the end, and the clamp binds there
            seen.add("beyond the top")
        if (r < c[5]).any() and (tz < c[5]).any():
            seen.add("beyond the bottom")
        bj = (np.clip(r[:, None] + g[:, None] * z[None, :], c[5], c[6]) - c[5]) / ((c[6] - c[5]) / (c[4] - 1))
        if "integer" in c[0]:
            assert (bj == np.round(bj)).all() and (g == 1).any(), c[0]
            seen.add("integer b")
        if c[13] > 1:
            assert ((g > 0) & (g < np.float32(c[7]) * 0.999)).any(), (c[0], g)
            seen.add("n-step")
    assert seen == {"terminal", "beyond the top", "beyond the bottom", "integer b", "n-step"}, seen


def test_the_two_bars_are_the_float32_restatements_error_times_eight():
    worst_p = worst_m = 0.0
    for case in W.CASES:
        c64, r32 = W.f32_rows_of(case, _inputs(case[0]))
        e = {k: float(np.abs(r32[k] - c64[k]).max()) for k in ("p", "tp", "m", "q", "y", "td")}
        print("%-28s %s" % (case[0], {k: "%.2e" % v for k, v in e.items()}))
        for k in ("q", "y", "td"):
            assert e[k] < W.ATOL * W.zmax_of(case), (case[0], k, e[k])
        print("%-28s dQ/da float32 |err| %.2e, bar %.2e" % (case[0], c64["dq_da_f32_err"], W.dqda_bar(case)))
        if W.zmax_of(case) <= 10.0:          # the ordinary bar, with room for the device's own order
            assert W.dqda_bar(case) == W.ATOL and c64["dq_da_f32_err"] < W.ATOL / 4, (case[0], c64["dq_da_f32_err"])
        else:                                # the wide case's own: the recorded figure is the measured one, rounded up by less than a tenth
            assert 0.9 * W.F32_ERR_DQDA_WIDE <= c64["dq_da_f32_err"] <= W.F32_ERR_DQDA_WIDE and W.dqda_bar(case) == 8.0 * W.F32_ERR_DQDA_WIDE
        if W.zmax_of(case) <= 10.0:
            worst_p, worst_m = max(worst_p, e["p"], e["tp"]), max(worst_m, e["m"])
    print("worst |p32 - p64| %.3e, worst |m32 - m64| %.3e" % (worst_p, worst_m))
    # the recorded figures are the measured ones, rounded up by less than a tenth
    assert 0.9 * W.F32_ERR_P <= worst_p <= W.F32_ERR_P and 0.9 * W.F32_ERR_M <= worst_m <= W.F32_ERR_M
    assert W.P_BAR == 8.0 * W.F32_ERR_P and W.M_BAR == 8.0 * W.F32_ERR_M


@pytest.mark.parametrize("cid", IDS)
def test_the_float32_evaluation_stays_inside_the_gpu_bounds(cid):
    case = W.case_of(cid)
    opt, d, clip = case[8], case[9], case[11]
    P = _inputs(cid)[1]
    want, counts, o64 = _run(cid)
    twin, _c, o32 = _run(cid, "f32")
    nb_, steps_ = W.structure(case)
    assert list(counts) == [W.NB // d, W.NB] and nb_ * steps_ == W.NB
    assert all(np.array_equal(x, y) for a, b in zip(o64, o32) for x, y in zip(a["routes"], b["routes"])), \
        "the float32 evaluation and the float64 restatement take different pool / ReLU routes: choose another case"
    norms = [n for o in o64 for n in (o["actor_norm"], o["critic_norm"])]
    print("%s  pre-clip norms %s" % (cid, ["%.2f" % n for n in norms]))
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


def _applicable(case):
    cid, shape_name = case[0], case[1]
    faults = ["target_p_from_online_critic", "log_of_wrong_evaluation", "actor_fed_ones", "support_off_by_one", "target_q_value_not_updated"]
    z = W.support(*W.dist_of(case))[0][None, :]

    def tz(b, g):
        return np.clip(np.asarray(b[2], np.float64).reshape(-1, 1) + g * z, case[5], case[6])
    # (a terminal or an n-step row among the compared minibatches whose clamped Tz the mask moves)
    if any(np.abs(tz(b, case[7]) - tz(b, np.asarray(b[3], np.float64).reshape(-1, 1) * case[7])).max() > 0.01 for b in _inputs(cid)[4]):
        faults.append("discount_without_mask")
    if case[3] > 1:
        faults.append("mean_missing")
    if "ends" in cid:
        faults.append("projection_unclamped")
    if "integer" in cid:
        faults.append("integer_b_loses_mass")
    if case[10] is not None:
        faults.append("m_from_unsmoothed_action")
    if "weighted" in cid:
        faults.append("weight_missing")
    return faults


def _quantity_bars(case):
    zmax = W.zmax_of(case)
    return {"p": W.P_BAR, "tp": W.P_BAR, "m": W.M_BAR, "q": W.ATOL * zmax, "td": W.ATOL * zmax, "dq_da": W.dqda_bar(case), "actions": W.ATOL}


@pytest.mark.parametrize("cid", IDS)
def test_each_planted_fault_moves_a_compared_quantity_by_ten_times_its_gpu_bar(cid):
    """the compared quantities: the first minibatch's p, p', m, Q, td, dQ/da and actions at their bars, both pre-clip gradient lists at
    GRAD_REL of the list's norm, and the six vectors behind the case's minibatches at tests.ddpg_opt_np's bounds"""
    case = W.case_of(cid)
    opt = case[8]
    P = _inputs(cid)[1]
    want, _c, o64 = _run(cid)
    bars = _quantity_bars(case)
    for fault in _applicable(case):
        got, _c2, of = _run(cid, "f64", fault)
        ratios = {name: float(np.linalg.norm(g - w)) / b for name, g, w, b in zip(T3.VECTORS, got, want, W.bounds(P, want, W.NB))
                  if name in _compared(opt) and b > 0}
        for k, bar in bars.items():
            ratios[k] = float(np.abs(np.asarray(of[0][k]) - np.asarray(o64[0][k])).max()) / bar
        for k in ("actor_grads", "critic_grads"):
            ratios[k] = float(np.linalg.norm(of[0][k] - o64[0][k]) / (W.GRAD_REL * np.linalg.norm(o64[0][k])))
        print("%s %-30s %s" % (cid, fault, {k: round(v, 1) for k, v in ratios.items() if v > 0}))
        assert max(ratios.values()) > POWER, (cid, fault, ratios)
        if fault == "actor_fed_ones":
            assert ratios["dq_da"] > POWER and ratios["actor_grads"] > POWER, (cid, fault, ratios)
        if fault == "target_q_value_not_updated":
            assert ratios["target_critic"] > POWER, (cid, fault, ratios)
        if fault == "integer_b_loses_mass":
            assert ratios["m"] > POWER, (cid, fault, ratios)


def test_every_fault_is_seen_by_some_case():
    seen = set()
    for case in W.CASES:
        seen.update(_applicable(case))
    assert seen == set(W.FAULTS)


def test_check_loss_is_the_formula_without_noise_or_weights():
    cid = "A2-B8-N51-smoothed"
    case = W.case_of(cid)
    specs, P, _ep, _idxs, batches = _inputs(cid)
    ref = W.restatement(specs, P, W.dist_of(case), np.float64, W.hyper_of(case), smoothing=W.SMOOTHING)
    ref.weights = W.case_weights(case)[0]
    loss, td, q = ref.check_loss(batches[0])
    cg = ref.last_cg
    assert ref.tps_n == 0 and cg["noise"] is None and np.array_equal(cg["w"], np.ones_like(cg["w"]))
    assert abs(loss - float(cg["ce"].mean())) < 1e-15 and np.array_equal(td, cg["q"] - cg["y"]) and np.array_equal(q, cg["q"])


def test_the_graph_case_meets_the_same_conditions():
    case, nb, steps, _ss = W.GRAPH_CASE
    inp = W.graph_inputs()
    P, rows = inp[1], inp[3]
    assert len(inp[4]) == steps * nb and rows.min() >= 0 and rows.max() < W.ROWS
    want, counts, o64, ref = W.run_case(case, inp, nb=nb, steps=steps)
    twin, _c, o32, _r = W.run_case(case, inp, np.float32, nb=nb, steps=steps)
    assert list(counts) == [steps * nb // 2, steps * nb] and ref.schedule == T3.expected_schedule(2, steps * nb)
    g = np.concatenate([np.ravel(b[3]) for b in inp[4]])
    assert ((g > 0) & (g < 1)).any() and (g == 0).any()                 # (folded n-step masks and terminal rows)
    print("graph case: closest calls %s" % ["%.2e" % o["tie"] for o in o64])
    assert min(o["tie"] for o in o64) > T3.TIE_FLOOR
    assert all(np.array_equal(x, y) for a, b in zip(o64, o32) for x, y in zip(a["routes"], b["routes"]))
    for name, w, t, b in zip(T3.VECTORS, want, twin, W.bounds(P, want, steps * nb)):
        err = float(np.linalg.norm(t - w))
        print("graph case  %-13s float32 |err| %.3e  bound %.3e  (%.2f of it)" % (name, err, b, err / b))
        assert err <= b and (name not in T3.VECTORS[:4] or err <= R.PARAM_REL * float(np.linalg.norm(w))), (name, err, b)
