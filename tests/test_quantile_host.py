"""The quantile critic without a GPU: the float64 restatement (tests/quant_np.py) against torch autograd -- the loss, the gradient into
the atoms, dQ/da through the mean --, the sort and the truncation against np.sort, d = 0 against plain quantile regression, the command
line, the entry points' citations, the conditioning of the cases the two modules share (both Huber branches, routes, ties), the derivation
of the bars tests/test_gpu_quantile.py uses, and the power of the GPU comparison: every planted fault moves a compared quantity by at
least ten times its GPU bar."""
import functools
import os
import re

import numpy as np
import pytest

from oracle import ddpg_np as O
from tests import ddpg_opt_np as R
from tests import quant_np as W
from tests import td3_np as T3

POWER = 10.0          # the smallest factor the earlier feature tests accepted (tests/test_policy_delay_host.py)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the restatement against torch autograd, float64
@pytest.mark.parametrize("pixel,drop,kappa", [(True, 0, 1.0), (True, 2, 0.3), (False, 6, 1.0), (False, 3, 0.1)],
                         ids=["pixel-d0", "pixel-d2-k0.3", "lowdim-M1", "lowdim-d3-k0.1"])
def test_loss_atom_gradient_and_dq_da_against_torch_autograd(pixel, drop, kappa):
    import torch
    from oracle.ddpg_torch import TorchDDPG
    rng = np.random.default_rng(4)
    A, B, N = 3, 6, 7
    kappa = float(np.float32(kappa))          # (the ABI takes kappa as a float)
    kw = dict(pixel=True, H=8, W=8, C=3) if pixel else dict(pixel=False, state_elems=11)
    aspec, plain = O.NetSpec("actor", A, [7], **kw), O.NetSpec("critic", A, [9, 6], **kw)
    cspec = W.quant_spec(plain, N)
    assert cspec.layout()[-2:] == [("q_value/weights", (plain.fc[-1][1], N)), ("q_value/biases", (N,))] and plain.fc[-1][2] == 1
    flat = O.init_params(cspec, rng).astype(np.float64)
    flat = flat + rng.normal(0, 0.05, flat.shape)
    tail = plain.fc[-1][1] * N + N                     # the q_value layer spread out: atoms on the scale of the returns, on both sides of kappa
    flat[-tail:] += rng.normal(0, 0.7, tail)
    aflat = (O.init_params(aspec, rng) + rng.normal(0, 0.05, aspec.num_params())).astype(np.float64)
    ref = W.QuantDDPG(aspec, cspec, aflat, flat, (N, kappa, drop), np.float64)
    state = rng.uniform(0, 1, (B, 8, 8, 3)) if pixel else rng.standard_normal((B, 11))
    s2 = rng.uniform(0, 1, (B, 8, 8, 3)) if pixel else rng.standard_normal((B, 11))
    a, r = rng.uniform(-1, 1, (B, A)), rng.integers(0, 3, (B, 1)).astype(np.float64)
    mask, w = (rng.uniform(0, 1, (B, 1)) > 0.3).astype(np.float64), rng.uniform(0.2, 1, (B, 1))
    cg = ref.critic_gradients((state, a, r, mask, s2), w=w)
    ag = ref.actor_gradients(state)
    au = np.abs(cg["u"])
    assert (au <= kappa).any() and (au > kappa).any() and (cg["u"] < 0).any() and (cg["u"] > 0).any()
    # torch: the critic from the same parameters, the loss written out from the definition with the targets held constant
    t = TorchDDPG(aspec, plain, O.init_params(aspec, rng), O.init_params(plain, rng), dtype=torch.float64)
    p = {n: torch.tensor(np.asarray(v), dtype=torch.float64, requires_grad=True) for n, v in ref.critic.p.items()}

    def atoms_of(st, act):
        h = t._trunk(cspec, p, torch.tensor(st))
        for name, _i, _o, kind, cat in cspec.fc:
            if cat:
                h = torch.cat([h, act], dim=1)
            h = h @ p[name + "/weights"] + p[name + "/biases"]
            h = torch.relu(h) if kind == "relu" else h
        return h
    ta = torch.tensor(a, requires_grad=True)
    th = atoms_of(state, ta)
    assert np.allclose(th.detach().numpy(), cg["theta"], rtol=1e-11, atol=1e-11)
    M = N - drop
    y = torch.tensor(cg["y"][:, :M])
    want_y = r + mask * ref.hp.discount * np.sort(cg["target_theta"], axis=1)[:, :M]
    assert np.abs(cg["y"][:, :M] - want_y).max() < 1e-14 and not cg["y"][:, M:].any()
    u = y[:, None, :] - th[:, :, None]
    tau = torch.tensor((2.0 * np.arange(N) + 1.0) / (2.0 * N))[None, :, None]
    hub = torch.where(u.abs() <= kappa, 0.5 * u * u, kappa * (u.abs() - 0.5 * kappa))
    rho = (tau - (u.detach() < 0).double()).abs() * hub / kappa
    loss = (torch.tensor(w) * rho.sum(dim=(1, 2), keepdim=False).reshape(B, 1) / (N * M)).mean()
    names = [n for n, _s in cspec.layout()]
    tg = torch.autograd.grad(loss, [p[n] for n in names] + [th], retain_graph=True)
    assert abs(float(loss.detach()) - float(cg["loss"])) < 1e-12 * max(1.0, abs(float(loss.detach())))
    assert np.allclose(cg["dz"], tg[-1].numpy(), rtol=1e-10, atol=1e-15), "the gradient into the atoms"
    assert np.abs(tg[-1].numpy()).max() > 1e-4
    want = np.concatenate([g.numpy().ravel() for g in tg[:-1]])
    assert np.allclose(cg["grads"], want, rtol=1e-9, atol=1e-12 * np.abs(want).max()), float(np.abs(cg["grads"] - want).max())
    # td and Q
    assert np.abs(cg["q"] - cg["theta"].mean(axis=1, keepdims=True)).max() < 1e-14
    assert np.abs(cg["td"] - (cg["q"] - want_y.mean(axis=1, keepdims=True))).max() < 1e-14
    # dQ/da through the mean of the atoms, at the actor's action
    act = torch.tensor(ag["actions"], requires_grad=True)
    q = atoms_of(state, act).mean(dim=1, keepdim=True)
    assert np.allclose(q.detach().numpy(), ag["q"], rtol=1e-11, atol=1e-12)
    dq, = torch.autograd.grad(q.sum(), act)
    assert np.allclose(ag["dq_da"], dq.numpy(), rtol=1e-9, atol=1e-13), float(np.abs(ag["dq_da"] - dq.numpy()).max())
    assert np.abs(dq.numpy()).max() > 1e-3


# ---- the sort and the truncation
def _tied_rows(n, B=12, seed=0):
    """target atoms with ties (a row of one value, rows drawn from three values, a pair of equal atoms), signs mixed, and rows with mask 0"""
    rng = np.random.default_rng(seed + n)
    tt = rng.normal(0, 2.0, (B, n))
    tt[0] = 1.25
    tt[1] = rng.choice([-1.0, 0.0, 2.5], n)
    tt[2] = rng.choice([-0.0, 0.0], n)
    tt[3, -1] = tt[3, 0]
    tt[4] = np.sort(tt[4])[::-1]
    r = rng.integers(0, 3, (B, 1)).astype(np.float64)
    mask = (rng.uniform(0, 1, (B, 1)) > 0.3).astype(np.float64)
    mask[5], mask[1] = 0.0, 0.0
    return tt.astype(np.float32), r, mask


@pytest.mark.parametrize("n", [2, 25, 33, 64])
def test_the_sort_and_the_truncation_against_np_sort(n):
    tt, r, mask = _tied_rows(n)
    want = np.sort(tt, axis=1)
    lanes = W.bitonic_sort(W._lanes(tt, np.inf))
    assert np.array_equal(lanes[:, :n], want) and np.isinf(lanes[:, n:]).all()          # (ties included: the values, bit for bit up to the sign of zero)
    theta = np.random.default_rng(n).normal(0, 2.0, tt.shape).astype(np.float32)
    for drop in sorted({0, min(2, n - 1), n - 1}):
        m = n - drop
        s, y = W.sort_truncate(tt, r, mask * 0.9, drop)
        assert np.array_equal(s, want) and y.shape == (tt.shape[0], m)
        assert np.array_equal(y, r + mask * 0.9 * want[:, :m].astype(np.float64))
        assert np.array_equal(y[mask[:, 0] == 0], np.repeat(r[mask[:, 0] == 0], m, axis=1))          # (mask 0: every kept target is r)
        f64, f32 = W.rows(theta, tt, r, mask, 0.9, 1.0, drop), W.rows_f32(theta, tt, r, mask, 0.9, 1.0, drop)
        assert np.array_equal(f32["sorted"], want) and not f32["y"][:, m:].any() and not f64["y"][:, m:].any()
        for k in ("theta", "sorted", "y", "q", "tq", "td"):
            assert np.abs(f32[k] - f64[k]).max() < W.ATOL, (k, n, drop)
        assert np.abs(f32["L"] - f64["L"]).max() < 1e-6
        assert np.abs(f32["dz"] - (-f64["G"] / tt.shape[0])).max() < 1e-7
        # truncation works on values: a permutation of the target atoms changes nothing
        perm = np.random.default_rng(drop).permutation(n)
        again = W.rows(theta, tt[:, perm], r, mask, 0.9, 1.0, drop)
        assert all(np.array_equal(again[k], f64[k]) for k in ("sorted", "y", "L", "G")) and np.abs(again["td"] - f64["td"]).max() < 1e-14


def test_without_dropped_atoms_it_is_plain_quantile_regression():
    """d = 0 against QR-DQN's loss written the usual way: every (i, j) pair of the UNSORTED targets, mean over j, sum over i, over N"""
    rng = np.random.default_rng(3)
    B, n, kappa = 7, 25, 1.0
    theta, tt = rng.normal(1, 2.0, (B, n)), rng.normal(1, 2.0, (B, n))
    r, g = rng.integers(0, 3, (B, 1)).astype(np.float64), rng.choice([0.0, 0.9], (B, 1))
    _s, y = W.sort_truncate(tt, r, g, 0)
    L, G = W.pair_loss(theta, y, kappa)
    tau = (np.arange(n) + 0.5) / n
    want = np.zeros((B, 1))
    for b in range(B):
        for i in range(n):
            for j in range(n):
                u = r[b, 0] + g[b, 0] * tt[b, j] - theta[b, i]
                h = 0.5 * u * u if abs(u) <= kappa else kappa * (abs(u) - 0.5 * kappa)
                want[b, 0] += abs(tau[i] - (1.0 if u < 0 else 0.0)) * h / kappa / n / n
    assert np.abs(L - want).max() < 1e-13
    eps = 1e-6                                             # the gradient by central differences (the loss is C1)
    for i in (0, 7, n - 1):
        d = np.zeros_like(theta)
        d[:, i] = eps
        num = (W.pair_loss(theta + d, y, kappa)[0] - W.pair_loss(theta - d, y, kappa)[0]) / (2 * eps)
        assert np.abs(-G[:, i:i + 1] - num).max() < 1e-8
    assert np.abs(W.rows(theta, tt, r, g / 0.9, 0.9, kappa, 0)["td"] - (theta.mean(axis=1, keepdims=True) - y.mean(axis=1, keepdims=True))).max() < 1e-14


def test_the_loss_and_its_gradient_are_continuous_where_the_branches_meet():
    theta = np.zeros((1, 2))
    for kappa in (1.0, 0.25):
        for at in (0.0, kappa, -kappa):
            lo, hi = (W.pair_loss(theta, np.array([[at + e]]), kappa) for e in (-1e-9, 1e-9))
            assert np.abs(lo[0] - hi[0]).max() < 1e-8 and np.abs(lo[1] - hi[1]).max() < 1e-8, (kappa, at)


# ---- the command line
OPTION_KEYS = ("quantile_critic", "num_quantiles", "quantile_huber_kappa", "drop_top_quantiles")


def test_the_parser_takes_the_options_and_they_are_absent_unless_given():
    from cartpoleplusplus_amd import ddpg_cartpole as D
    o = D.build_parser().parse_args([])
    for k in OPTION_KEYS:
        assert not hasattr(o, k), k
    d = D.default_opts()
    assert [getattr(d, k) for k in OPTION_KEYS] == [False, None, None, None]
    assert D.quantile_critic(o) is None and D.quantile_critic(d) is None
    assert D.quantile_critic(D.build_parser().parse_args(["--quantile-critic"])) == (25, 1.0, 0)
    o = D.build_parser().parse_args(["--quantile-critic", "--num-quantiles", "33", "--quantile-huber-kappa", "0.25", "--drop-top-quantiles", "2",
                                     "--n-step", "3", "--prioritized-replay", "--policy-delay", "2", "--target-policy-noise", "0.2"])
    assert D.quantile_critic(o) == (33, 0.25, 2) and D.distributional_critic(o) is None
    assert D.quantile_critic(D.default_opts(quantile_critic=True, num_quantiles=2, drop_top_quantiles=1)) == (2, 1.0, 1)
    assert D.quantile_critic(D.default_opts(quantile_critic=True, num_quantiles=64, drop_top_quantiles=63)) == (64, 1.0, 63)


@pytest.mark.parametrize("argv", [["--num-quantiles", "25"],                                                # options without the flag
                                  ["--quantile-huber-kappa", "1"],
                                  ["--drop-top-quantiles", "2"],
                                  ["--quantile-critic", "--twin-q"],
                                  ["--quantile-critic", "--distributional-critic", "--v-min", "0", "--v-max", "1"],
                                  ["--quantile-critic", "--num-quantiles", "1"],
                                  ["--quantile-critic", "--num-quantiles", "65"],
                                  ["--quantile-critic", "--num-quantiles", "0"],
                                  ["--quantile-critic", "--drop-top-quantiles", "-1"],
                                  ["--quantile-critic", "--drop-top-quantiles", "25"],                      # d = N: nothing stays
                                  ["--quantile-critic", "--num-quantiles", "8", "--drop-top-quantiles", "8"],
                                  ["--quantile-critic", "--quantile-huber-kappa", "0"],
                                  ["--quantile-critic", "--quantile-huber-kappa", "-1"],
                                  ["--quantile-critic", "--quantile-huber-kappa", "inf"],
                                  ["--quantile-critic", "--quantile-huber-kappa", "nan"]],
                         ids=lambda a: " ".join(a))
def test_the_parsers_refusals(argv):
    from cartpoleplusplus_amd import ddpg_cartpole as D
    o = D.build_parser().parse_args(argv)
    with pytest.raises(SystemExit):
        D.quantile_critic(o)


def test_the_agent_refuses_before_anything_exists_on_the_device():
    """quantile_critic() runs at the top of the agent's constructor: the refusal needs no device (this test has none)"""
    from cartpoleplusplus_amd import ddpg_cartpole as D
    from tests.helpers import FakeEnv
    for kw in (dict(quantile_critic=True, twin_q=True), dict(quantile_critic=True, distributional_critic=True, v_min=0.0, v_max=1.0),
               dict(num_quantiles=25), dict(quantile_critic=True, num_quantiles=8, drop_top_quantiles=8)):
        D.set_opts(D.default_opts(use_raw_pixels=False, **kw))
        with pytest.raises(SystemExit):
            D.DeepDeterministicPolicyGradientAgent(FakeEnv((2, 2, 7), 2))
    D.set_opts(D.default_opts())


def test_naf_does_not_take_the_options():
    from cartpoleplusplus_amd import naf_cartpole as F
    assert not set(OPTION_KEYS) & set(vars(F.build_parser().parse_args([])))
    with pytest.raises(SystemExit):
        F.build_parser().parse_args(["--quantile-critic"])


NEW_ENTRY_POINTS = ("cpp_net_create_quantile", "cpp_net_quantile_info", "cpp_ddpg_set_quantile_target", "cpp_ddpg_last_quantiles")


def test_every_new_entry_point_is_bound_and_cites_the_reference_lines_it_extends():
    from cartpoleplusplus_amd import _lib
    header = open(os.path.join(ROOT, "include", "cartpolepp_abi.h")).read()
    csrc = os.path.join(ROOT, "cartpoleplusplus_amd", "csrc")
    source = "".join(open(os.path.join(csrc, f)).read() for f in sorted(os.listdir(csrc)) if f.startswith("rt_") and f.endswith(".cpp"))
    for name in NEW_ENTRY_POINTS:
        assert name in _lib.SIGNATURES, name
        # the comment that ends where the declaration / the definition begins
        for text, pattern in ((header, r"/\*((?:(?!\*/).)*)\*/\s*int %s\(" % name), (source, r"((?://[^\n]*\n)+)extern \"C\" int %s\(" % name)):
            m = re.search(pattern, text, flags=re.S)
            assert m and re.search(r"ddpg_cartpole\.py:\d+", m.group(1)), name


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
    assert {c[3] for c in cases} >= {1, 5, 8} and {c[4] for c in cases} >= {2, 25, 33, 64} and {c[2] for c in cases} >= {2, 9}
    assert {c[1] for c in cases} == {"16x16x3", "lowdim"}
    assert {c[5] for c in cases} >= {0, 2} and any(c[5] == c[4] - 1 for c in cases) and any(c[4] == 64 and c[5] == 63 for c in cases)
    assert {c[6] for c in cases} == {1.0, W.SMALL_KAPPA} and W.SMALL_KAPPA < 1.0
    assert {c[8] for c in cases} >= {"gradient-descent", "momentum-0.5", "adam"}
    assert any(c[9] == 2 and c[10] is not None for c in cases) and any(c[13] == 3 for c in cases) and any("weighted" in c[0] for c in cases)
    seen = set()
    for c in cases:
        b = _inputs(c[0])[4][0]
        mask = np.ravel(b[3])
        if (mask == 0).any():
            seen.add("terminal")
        if c[13] > 1:
            g = mask * np.float32(c[7])
            assert ((g > 0) & (g < np.float32(c[7]) * 0.999)).any(), (c[0], g)
            seen.add("n-step")
    assert seen == {"terminal", "n-step"}, seen


@pytest.mark.parametrize("cid", IDS)
def test_every_case_exercises_both_huber_branches(cid):
    """a condition on the case, met by the float64 restatement alone: at least a tenth of the u_ij of the first minibatch on either side
    of kappa (and, where the kappa is the small one, most of them on the linear branch); both signs; target atoms that arrive unsorted"""
    case = W.case_of(cid)
    o = _run(cid)[2][0]
    au = np.abs(o["u"])
    quad = float((au <= case[6]).mean())
    print("%s: %d pairs, %.3f on the quadratic branch" % (cid, au.size, quad))
    assert 0.1 <= quad <= 0.9, (cid, quad)
    if case[6] == W.SMALL_KAPPA:
        assert quad < 0.5
    assert (o["u"] < 0).mean() >= 0.1 and (o["u"] > 0).mean() >= 0.1
    ref = W.restatement(_inputs(cid)[0], _inputs(cid)[1], W.quant_of(case), np.float64, W.hyper_of(case), case[8], case[9], case[10])
    tt = ref.critic_gradients(_inputs(cid)[4][0])["target_theta"]
    assert (np.diff(tt, axis=1) < 0).any(), "the target atoms arrive sorted: the sort would not be seen"


def test_the_bars_are_the_float32_restatements_error_times_eight():
    worst = {k: 0.0 for k in W.F32_ERR}
    for case in W.CASES:
        c64, r32 = W.f32_rows_of(case, _inputs(case[0]))
        e = {k: float(np.abs(np.asarray(r32[k], np.float64) - c64[k]).max()) for k in worst}
        print("%-28s %s" % (case[0], {k: "%.2e" % v for k, v in e.items()}))
        assert float(np.abs(r32["L"] - c64["L"]).max()) < 1e-6 * max(1.0, float(c64["L"].max())), case[0]
        for k in worst:
            worst[k] = max(worst[k], e[k])
    print("worst: %s" % {k: "%.3e" % v for k, v in worst.items()})
    for k, v in worst.items():
        # the recorded figures are the measured ones, rounded up by less than a tenth
        assert 0.9 * W.F32_ERR[k] <= v <= W.F32_ERR[k], (k, v, W.F32_ERR[k])
        # each bar is the figure times eight; the ordinary ATOL is kept wherever the figure is below ATOL / 4
        if W.F32_ERR[k] < W.ATOL / 4:
            assert W.bar(k) == W.ATOL
        else:
            assert W.bar(k) == 8.0 * W.F32_ERR[k]
    assert W.BAR_FACTOR == 8.0 and set(worst) == {"theta", "sorted", "y", "dz", "q", "td", "dq_da"}


@pytest.mark.parametrize("cid", IDS)
def test_the_float32_evaluation_stays_inside_the_gpu_bounds(cid):
    case = W.case_of(cid)
    opt, d = case[8], case[9]
    P = _inputs(cid)[1]
    want, counts, o64 = _run(cid)
    twin, _c, o32 = _run(cid, "f32")
    nb_, steps_ = W.structure(case)
    assert list(counts) == [W.NB // d, W.NB] and nb_ * steps_ == W.NB
    assert all(np.array_equal(x, y) for a, b in zip(o64, o32) for x, y in zip(a["routes"], b["routes"])), \
        "the float32 evaluation and the float64 restatement take different pool / ReLU routes: choose another case"
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
    for k in range(W.NB):      # both pre-clip gradient lists of every minibatch at the GPU test's relative bar
        for key in ("actor_grads", "critic_grads"):
            rel = float(np.linalg.norm(o32[k][key] - o64[k][key]) / np.linalg.norm(o64[k][key]))
            assert rel < W.GRAD_REL, (cid, k, key, rel)


def _applicable(case):
    cid = case[0]
    faults = ["targets_not_sorted", "tau_i_over_n", "indicator_on_theta_minus_y", "plain_l2", "nm_missing", "target_theta_from_online_critic",
              "actor_fed_ones", "target_q_value_not_updated"]
    if case[5] > 0:
        faults.append("smallest_dropped")
    if case[6] != 1.0:
        faults.append("huber_without_kappa")
    # (a terminal or an n-step row among the compared minibatches)
    if any((np.abs(np.ravel(b[3]) - 1.0) > 0.01).any() for b in _inputs(cid)[4]):
        faults.append("discount_without_mask")
    if case[3] > 1:
        faults.append("mean_missing")
    if case[10] is not None:
        faults.append("unsmoothed_target_action")
    if "weighted" in cid:
        faults.append("weight_missing")
    return faults


QUANTITY_BARS = {"theta": W.bar("theta"), "sorted": W.bar("sorted"), "y": W.bar("y"), "q": W.bar("q"), "td": W.bar("td"),
                 "dq_da": W.bar("dq_da"), "actions": W.ATOL}


@pytest.mark.parametrize("cid", IDS)
def test_each_planted_fault_moves_a_compared_quantity_by_ten_times_its_gpu_bar(cid):
    """the compared quantities: the first minibatch's theta, sorted theta', y, Q, td, dQ/da and actions at their bars, both pre-clip
    gradient lists at GRAD_REL of the list's norm, the loss at ATOL relative, and the six vectors behind the case's minibatches at
    tests.ddpg_opt_np's bounds"""
    case = W.case_of(cid)
    opt = case[8]
    P = _inputs(cid)[1]
    want, _c, o64 = _run(cid)
    for fault in _applicable(case):
        got, _c2, of = _run(cid, "f64", fault)
        ratios = {name: float(np.linalg.norm(g - w)) / b for name, g, w, b in zip(T3.VECTORS, got, want, W.bounds(P, want, W.NB))
                  if name in _compared(opt) and b > 0}
        for k, bar in QUANTITY_BARS.items():
            ratios[k] = float(np.abs(np.asarray(of[0][k]) - np.asarray(o64[0][k])).max()) / bar
        for k in ("actor_grads", "critic_grads"):
            ratios[k] = float(np.linalg.norm(of[0][k] - o64[0][k]) / (W.GRAD_REL * np.linalg.norm(o64[0][k])))
        ratios["loss"] = abs(of[0]["loss"] - o64[0]["loss"]) / (W.ATOL * max(1.0, abs(o64[0]["loss"])))
        print("%s %-32s %s" % (cid, fault, {k: round(v, 1) for k, v in ratios.items() if v > 0}))
        assert max(ratios.values()) > POWER, (cid, fault, ratios)
        if fault == "actor_fed_ones":
            assert ratios["dq_da"] > POWER and ratios["actor_grads"] > POWER, (cid, fault, ratios)
        if fault == "target_q_value_not_updated":
            assert ratios["target_critic"] > POWER, (cid, fault, ratios)
        if fault in ("targets_not_sorted", "smallest_dropped"):
            assert ratios["y"] > POWER and (case[5] == 0 or ratios["td"] > POWER), (cid, fault, ratios)      # (d = 0: the mean keeps td)
        if fault in ("tau_i_over_n", "indicator_on_theta_minus_y", "plain_l2", "nm_missing", "huber_without_kappa", "mean_missing", "weight_missing"):
            assert ratios["critic_grads"] > POWER, (cid, fault, ratios)


def test_every_fault_is_seen_by_some_case():
    seen = set()
    for case in W.CASES:
        seen.update(_applicable(case))
    assert seen == set(W.FAULTS) and len(W.FAULTS) == 14


def test_check_loss_is_the_formula_without_noise_or_weights():
    cid = "A2-B8-N25-d2-smoothed"
    case = W.case_of(cid)
    specs, P, _ep, _idxs, batches = _inputs(cid)
    ref = W.restatement(specs, P, W.quant_of(case), np.float64, W.hyper_of(case), smoothing=W.SMOOTHING)
    ref.weights = W.case_weights(case)[0]
    loss, td, q = ref.check_loss(batches[0])
    cg = ref.last_cg
    assert ref.tps_n == 0 and cg["noise"] is None and np.array_equal(cg["w"], np.ones_like(cg["w"]))
    assert abs(loss - float(cg["L"].mean())) < 1e-15 and np.array_equal(q, cg["q"])
    assert np.array_equal(td, cg["q"] - cg["y"][:, :case[4] - case[5]].mean(axis=1, keepdims=True))


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
    quad = float((np.abs(o64[0]["u"]) <= case[6]).mean())
    assert 0.1 <= quad <= 0.9, quad
    print("graph case: closest calls %s" % ["%.2e" % o["tie"] for o in o64])
    assert min(o["tie"] for o in o64) > T3.TIE_FLOOR
    assert all(np.array_equal(x, y) for a, b in zip(o64, o32) for x, y in zip(a["routes"], b["routes"]))
    for name, w, t, b in zip(T3.VECTORS, want, twin, W.bounds(P, want, steps * nb)):
        err = float(np.linalg.norm(t - w))
        print("graph case  %-13s float32 |err| %.3e  bound %.3e  (%.2f of it)" % (name, err, b, err / b))
        assert err <= b and (name not in T3.VECTORS[:4] or err <= R.PARAM_REL * float(np.linalg.norm(w))), (name, err, b)
