"""Pooled twin quantile critics on the host (--pooled-quantile-critics; include/cartpolepp_abi.h, cpp_net_create_pooled_quantile): the command
line and its refusals, the restatement tests/pool_np.py against torch autograd, the pooled bitonic network against np.sort, the conditions
the shared cases meet, the bars of tests/test_gpu_pooled_quantile.py re-measured from the float32 twin, the twin inside those bars, and
every planted fault outside them by ten times.  No test here needs a device."""
import functools
import os
import re

import numpy as np
import pytest

from oracle import ddpg_np as O
from tests import pool_np as P
from tests import quant_np as Q
from tests import twin_np as W

POWER = 10.0          # the smallest factor the earlier feature tests accepted (tests/test_policy_delay_host.py)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the restatement against torch autograd, float64
@pytest.mark.parametrize("pixel,drop,kappa", [(True, 0, 1.0), (True, 2, 0.3), (False, 6, 1.0), (False, 3, 0.1)],
                         ids=["pixel-d0", "pixel-d2-k0.3", "lowdim-M2", "lowdim-d3-k0.1"])
def test_loss_atom_gradients_and_dqbar_da_against_torch_autograd(pixel, drop, kappa):
    import torch
    from oracle.ddpg_torch import TorchDDPG
    rng = np.random.default_rng(5)
    A, B, N = 3, 6, 7
    kappa = float(np.float32(kappa))          # (the ABI takes kappa as a float)
    kw = dict(pixel=True, H=8, W=8, C=3) if pixel else dict(pixel=False, state_elems=11)
    aspec, plain = O.NetSpec("actor", A, [7], **kw), O.NetSpec("critic", A, [9, 6], **kw)
    cspec = Q.quant_spec(plain, N)
    layout = W.full_layout(cspec)
    assert layout[-2:] == [("q_valueb/weights", (plain.fc[-1][1], N)), ("q_valueb/biases", (N,))]
    flat = rng.uniform(-0.4, 0.4, W.num_params(cspec))
    off = 0
    for name, shape in layout:                 # both q layers spread out: atoms on the scale of the returns, the heads interleaved
        n = int(np.prod(shape))
        if name.startswith("q_value"):
            flat[off:off + n] += rng.normal(0, 0.7, n)
        off += n
    aflat = (O.init_params(aspec, rng) + rng.normal(0, 0.05, aspec.num_params())).astype(np.float64)
    ref = P.PoolDDPG(aspec, cspec, aflat, flat, (N, kappa, drop), np.float64)
    tflat = flat + rng.normal(0, 0.1, flat.shape)
    ref.set_targets(aflat + rng.normal(0, 0.05, aflat.shape), tflat)
    state = rng.uniform(0, 1, (B, 8, 8, 3)) if pixel else rng.standard_normal((B, 11))
    s2 = rng.uniform(0, 1, (B, 8, 8, 3)) if pixel else rng.standard_normal((B, 11))
    a, r = rng.uniform(-1, 1, (B, A)), rng.integers(0, 3, (B, 1)).astype(np.float64)
    mask, w = (rng.uniform(0, 1, (B, 1)) > 0.3).astype(np.float64), rng.uniform(0.2, 1, (B, 1))
    cg = ref.critic_gradients((state, a, r, mask, s2), noise=None, w=w)
    ag = ref.actor_gradients(state)
    for u in (cg["u1"], cg["u2"]):
        assert (np.abs(u) <= kappa).any() and (np.abs(u) > kappa).any() and (u < 0).any() and (u > 0).any()
    t = TorchDDPG(aspec, plain, O.init_params(aspec, rng), O.init_params(plain, rng), dtype=torch.float64)
    p = {n: torch.tensor(np.asarray(v), dtype=torch.float64, requires_grad=True) for n, v in list(ref.critic.h1.p.items()) + list(ref.critic.p2.items())}
    k = W.cat_index(cspec)

    def atoms_of(st, act):
        h = t._trunk(cspec, p, torch.tensor(st))
        for name, _i, _o, kind, _cat in cspec.fc[:k]:
            h = torch.relu(h @ p[name + "/weights"] + p[name + "/biases"]) if kind == "relu" else h @ p[name + "/weights"] + p[name + "/biases"]
        h = torch.cat([h, act], dim=1)
        heads = []
        for suffix in ("", "b"):
            x = h
            for name, _i, _o, kind, _cat in cspec.fc[k:]:
                x = x @ p[name + suffix + "/weights"] + p[name + suffix + "/biases"]
                x = torch.relu(x) if kind == "relu" else x
            heads.append(x)
        return heads
    th = atoms_of(state, torch.tensor(a))
    assert np.allclose(th[0].detach().numpy(), cg["theta1"], rtol=1e-11, atol=1e-11) and np.allclose(th[1].detach().numpy(), cg["theta2"], rtol=1e-11, atol=1e-11)
    M = 2 * N - 2 * drop
    pool = np.concatenate([cg["target_theta1"], cg["target_theta2"]], axis=1)
    want_y = r + mask * ref.hp.discount * np.sort(pool, axis=1)[:, :M]
    assert np.abs(cg["y"][:, :M] - want_y).max() < 1e-14 and not cg["y"][:, M:].any() and cg["y"].shape == (B, 2 * N)
    y = torch.tensor(want_y)
    tau = torch.tensor((2.0 * np.arange(N) + 1.0) / (2.0 * N))[None, :, None]
    loss = 0.0
    for head in th:
        u = y[:, None, :] - head[:, :, None]
        hub = torch.where(u.abs() <= kappa, 0.5 * u * u, kappa * (u.abs() - 0.5 * kappa))
        rho = (tau - (u.detach() < 0).double()).abs() * hub / kappa
        loss = loss + (torch.tensor(w) * rho.sum(dim=(1, 2)).reshape(B, 1) / (N * M)).mean()
    names = [n for n, _s in layout]
    tg = torch.autograd.grad(loss, [p[n] for n in names] + th, retain_graph=True)
    assert abs(float(loss.detach()) - float(cg["loss"])) < 1e-12 * max(1.0, abs(float(loss.detach())))
    assert np.allclose(cg["dz1"], tg[-2].numpy(), rtol=1e-9, atol=1e-15) and np.allclose(cg["dz2"], tg[-1].numpy(), rtol=1e-9, atol=1e-15)
    assert min(np.abs(tg[-2].numpy()).max(), np.abs(tg[-1].numpy()).max()) > 1e-4
    want = np.concatenate([g.numpy().ravel() for g in tg[:-2]])
    assert np.allclose(cg["grads"], want, rtol=1e-9, atol=1e-12 * np.abs(want).max()), float(np.abs(cg["grads"] - want).max())
    # both tds from the one truncated mean; Q_k the heads' means
    ym = want_y.mean(axis=1, keepdims=True)
    assert np.abs(cg["td"] - (cg["theta1"].mean(axis=1, keepdims=True) - ym)).max() < 1e-14
    assert np.abs(cg["td2"] - (cg["theta2"].mean(axis=1, keepdims=True) - ym)).max() < 1e-14
    # dQbar/da through the mean over all atoms of both heads, at the actor's action
    act = torch.tensor(ag["actions"], requires_grad=True)
    h1, h2 = atoms_of(state, act)
    qbar = 0.5 * (h1.mean(dim=1, keepdim=True) + h2.mean(dim=1, keepdim=True))
    assert np.allclose(h1.mean(dim=1, keepdim=True).detach().numpy(), ag["q"], rtol=1e-11, atol=1e-12)
    assert np.allclose(h2.mean(dim=1, keepdim=True).detach().numpy(), ag["q2"], rtol=1e-11, atol=1e-12)
    dq, = torch.autograd.grad(qbar.sum(), act)
    assert np.allclose(ag["dq_da"], dq.numpy(), rtol=1e-9, atol=1e-13), float(np.abs(ag["dq_da"] - dq.numpy()).max())
    assert np.abs(dq.numpy()).max() > 1e-3


# ---- the pooled sort and the truncation
def _tied_heads(n, B=12, seed=0):
    """two target heads with ties inside and across the heads (a row of one value, rows drawn from three values, signed zeros, equal
    atoms in both heads), signs mixed, and rows with mask 0"""
    rng = np.random.default_rng(seed + n)
    t1, t2 = rng.normal(0, 2.0, (B, n)), rng.normal(0.3, 2.0, (B, n))
    t1[0], t2[0] = 1.25, 1.25
    t1[1], t2[1] = rng.choice([-1.0, 0.0, 2.5], n), rng.choice([-1.0, 0.0, 2.5], n)
    t1[2], t2[2] = rng.choice([-0.0, 0.0], n), rng.choice([-0.0, 0.0], n)
    t2[3] = t1[3]
    t1[4], t2[4] = np.sort(t1[4])[::-1], np.sort(t2[4])
    t2[6, 0] = t1[6, -1]
    r = rng.integers(0, 3, (B, 1)).astype(np.float64)
    mask = (rng.uniform(0, 1, (B, 1)) > 0.3).astype(np.float64)
    mask[5], mask[1] = 0.0, 0.0
    return t1.astype(np.float32), t2.astype(np.float32), r, mask


@pytest.mark.parametrize("n", [2, 25, 32])
def test_the_pooled_sort_and_the_truncation_against_np_sort(n):
    t1, t2, r, mask = _tied_heads(n)
    B = t1.shape[0]
    want = np.sort(np.concatenate([t1, t2], axis=1), axis=1)
    lanes = Q.bitonic_sort(P.pool_lanes(t1, t2))
    assert np.array_equal(lanes[:, :2 * n], want) and np.isinf(lanes[:, 2 * n:]).all()          # (ties included: the values; N = 32: no idle lane)
    rng = np.random.default_rng(n)
    th1, th2 = rng.normal(0, 2.0, t1.shape).astype(np.float32), rng.normal(0, 2.0, t1.shape).astype(np.float32)
    for drop in sorted({0, 1, min(2, n - 1), n - 1}):
        m = 2 * n - 2 * drop
        s, y, _from1 = P.pool_target(t1, t2, r, mask * 0.9, drop)
        assert np.array_equal(s, want) and y.shape == (B, m)
        assert np.array_equal(y, r + mask * 0.9 * want[:, :m].astype(np.float64))
        assert np.array_equal(y[mask[:, 0] == 0], np.repeat(r[mask[:, 0] == 0], m, axis=1))          # (mask 0: every kept target is r)
        f64, f32 = P.rows(th1, th2, t1, t2, r, mask, 0.9, 1.0, drop), P.rows_f32(th1, th2, t1, t2, r, mask, 0.9, 1.0, drop)
        assert np.array_equal(f32["sorted"], want) and not f32["y"][:, m:].any() and not f64["y"][:, m:].any()
        for k in P.ROW_KEYS:
            assert np.abs(f32[k] - f64[k]).max() < P.ATOL, (k, n, drop)
        assert max(np.abs(f32["L1"] - f64["L1"]).max(), np.abs(f32["L2"] - f64["L2"]).max()) < 1e-6
        assert abs(float(f32["loss"]) - float(f64["loss"])) < 1e-6 * max(1.0, float(f64["loss"]))
        assert max(np.abs(f32["dz1"] - f64["dz1"]).max(), np.abs(f32["dz2"] - f64["dz2"]).max()) < 1e-7
        # truncation works on values: a permutation of the pool across the heads changes nothing behind the sort
        perm = np.random.default_rng(drop).permutation(2 * n)
        z = np.concatenate([t1, t2], axis=1)[:, perm]
        again = P.rows(th1, th2, z[:, :n], z[:, n:], r, mask, 0.9, 1.0, drop)
        assert all(np.array_equal(again[k], f64[k]) for k in ("sorted", "y", "L1", "L2", "dz1", "dz2"))
        assert max(np.abs(again["td"] - f64["td"]).max(), np.abs(again["td2"] - f64["td2"]).max()) < 1e-14


def test_pooling_differs_from_truncating_each_head():
    """two heads of which one is the larger everywhere: the pool drops 2d of ITS atoms, per-head truncation d of each"""
    t1, t2 = np.arange(5.0)[None, :], np.arange(5.0)[None, :] + 10.0
    r, g = np.zeros((1, 1)), np.ones((1, 1))
    _s, y, from1 = P.pool_target(t1, t2, r, g, 2)
    assert np.array_equal(y, np.array([[0, 1, 2, 3, 4, 10.0]])) and from1[0] == 0
    _s, yf, _ = P.pool_target(t1, t2, r, g, 2, fault="truncation_per_head")
    assert np.array_equal(yf, np.array([[0, 1, 2, 10.0, 11.0, 12.0]]))


# ---- the command line
OPTION_KEYS = ("pooled_quantile_critics", "pooled_num_quantiles", "pooled_drop_per_head", "pooled_huber_kappa")


def test_the_parser_takes_the_options_and_they_are_absent_unless_given():
    from cartpoleplusplus_amd import ddpg_cartpole as D
    o = D.build_parser().parse_args([])
    for k in OPTION_KEYS:
        assert not hasattr(o, k), k
    d = D.default_opts()
    assert [getattr(d, k) for k in OPTION_KEYS] == [False, None, None, None]
    assert D.pooled_quantile_critics(o) is None and D.pooled_quantile_critics(d) is None
    assert D.pooled_quantile_critics(D.build_parser().parse_args(["--pooled-quantile-critics"])) == (25, 1.0, 2)
    o = D.build_parser().parse_args(["--pooled-quantile-critics", "--pooled-num-quantiles", "32", "--pooled-huber-kappa", "0.25", "--pooled-drop-per-head", "3",
                                     "--soft-actor-critic", "--shared-encoder", "--use-raw-pixels", "--random-shift", "4", "--n-step", "3",
                                     "--prioritized-replay"])
    assert D.pooled_quantile_critics(o) == (32, 0.25, 3) and D.quantile_critic(o) is None and not D.twin_q(o)
    assert D.soft_actor_critic(o, 2) is not None and D.shared_encoder(o) and D.random_shift(o) == (4, 0)
    o = D.build_parser().parse_args(["--pooled-quantile-critics", "--target-policy-noise", "0.2", "--policy-delay", "2", "--ddpg-optimiser", "Adam",
                                     "--param-noise-stddev", "0.1"])
    assert D.pooled_quantile_critics(o) == (25, 1.0, 2) and D.policy_delay(o) == 2 and D.param_noise(o) is not None
    assert D.pooled_quantile_critics(D.default_opts(pooled_quantile_critics=True, pooled_num_quantiles=2, pooled_drop_per_head=1)) == (2, 1.0, 1)
    assert D.pooled_quantile_critics(D.default_opts(pooled_quantile_critics=True, pooled_num_quantiles=32, pooled_drop_per_head=31)) == (32, 1.0, 31)


@pytest.mark.parametrize("argv", [["--pooled-num-quantiles", "25"],                                                # options without the flag
                                  ["--pooled-huber-kappa", "1"],
                                  ["--pooled-drop-per-head", "2"],
                                  ["--pooled-quantile-critics", "--quantile-critic"],
                                  ["--pooled-quantile-critics", "--distributional-critic", "--v-min", "0", "--v-max", "1"],
                                  ["--pooled-quantile-critics", "--twin-q"],
                                  ["--pooled-quantile-critics", "--twin-q", "--actor-min-q"],
                                  ["--pooled-quantile-critics", "--actor-min-q"],
                                  ["--pooled-quantile-critics", "--bc-alpha", "2.5"],
                                  ["--pooled-quantile-critics", "--pooled-num-quantiles", "1"],
                                  ["--pooled-quantile-critics", "--pooled-num-quantiles", "33"],
                                  ["--pooled-quantile-critics", "--pooled-num-quantiles", "0"],
                                  ["--pooled-quantile-critics", "--pooled-drop-per-head", "-1"],
                                  ["--pooled-quantile-critics", "--pooled-drop-per-head", "25"],                      # d = N: nothing stays
                                  ["--pooled-quantile-critics", "--pooled-num-quantiles", "8", "--pooled-drop-per-head", "8"],
                                  ["--pooled-quantile-critics", "--pooled-huber-kappa", "0"],
                                  ["--pooled-quantile-critics", "--pooled-huber-kappa", "-1"],
                                  ["--pooled-quantile-critics", "--pooled-huber-kappa", "inf"],
                                  ["--pooled-quantile-critics", "--pooled-huber-kappa", "nan"]],
                         ids=lambda a: " ".join(a))
def test_the_parsers_refusals(argv):
    from cartpoleplusplus_amd import ddpg_cartpole as D
    o = D.build_parser().parse_args(argv)
    with pytest.raises(SystemExit):
        D.pooled_quantile_critics(o)


def test_the_agent_refuses_before_anything_exists_on_the_device():
    """pooled_quantile_critics() runs at the top of the agent's constructor: the refusal needs no device (this test has none)"""
    from cartpoleplusplus_amd import ddpg_cartpole as D
    from tests.helpers import FakeEnv
    for kw in (dict(pooled_quantile_critics=True, twin_q=True), dict(pooled_quantile_critics=True, quantile_critic=True),
               dict(pooled_quantile_critics=True, distributional_critic=True, v_min=0.0, v_max=1.0), dict(pooled_quantile_critics=True, bc_alpha=2.5),
               dict(pooled_num_quantiles=25), dict(pooled_quantile_critics=True, pooled_num_quantiles=33),
               dict(pooled_quantile_critics=True, pooled_num_quantiles=8, pooled_drop_per_head=8),
               dict(pooled_quantile_critics=True, soft_actor_critic=True, data_parallel=True)):
        D.set_opts(D.default_opts(use_raw_pixels=False, **kw))
        with pytest.raises(SystemExit):
            D.DeepDeterministicPolicyGradientAgent(FakeEnv((2, 2, 7), 2))
    D.set_opts(D.default_opts())


def test_naf_does_not_take_the_options():
    from cartpoleplusplus_amd import naf_cartpole as F
    assert not set(OPTION_KEYS) & set(vars(F.build_parser().parse_args([])))
    for flag in ("--pooled-quantile-critics", "--pooled-num-quantiles"):
        with pytest.raises(SystemExit):
            F.build_parser().parse_args([flag] + (["25"] if flag.endswith("quantiles") else []))


NEW_ENTRY_POINTS = ("cpp_net_create_pooled_quantile", "cpp_net_create_pooled_quantile_norm", "cpp_net_pooled_quantile_info", "cpp_ddpg_last_pooled_quantiles")


def test_every_new_entry_point_is_bound_and_cites_the_reference_lines_it_extends():
    from cartpoleplusplus_amd import _lib
    header = open(os.path.join(ROOT, "include", "cartpolepp_abi.h")).read()
    csrc = os.path.join(ROOT, "cartpoleplusplus_amd", "csrc")
    source = "".join(open(os.path.join(csrc, f)).read() for f in sorted(os.listdir(csrc)) if f.startswith("rt_") and f.endswith(".cpp"))
    for name in NEW_ENTRY_POINTS:
        assert name in _lib.SIGNATURES, name
        for text, pattern in ((header, r"/\*((?:(?!\*/).)*)\*/\s*int %s\(" % name), (source, r"((?://[^\n]*\n)+)extern \"C\" int %s\(" % name)):
            m = re.search(pattern, text, flags=re.S)
            assert m and re.search(r"ddpg_cartpole\.py:\d+", m.group(1)), name
    assert "quant_pool.hip" in open(os.path.join(csrc, "Makefile")).read()


# ---- the cases the GPU module shares
IDS = [c[0] for c in P.CASES]


@functools.lru_cache(maxsize=None)
def _inputs(cid):
    return P.case_inputs(P.case_of(cid))


@functools.lru_cache(maxsize=None)
def _run(cid, dt_name="f64", fault=None):
    """the float64 run; every other run takes each minibatch from the float64 run's state, as the GPU test takes it from the device's"""
    case = P.case_of(cid)
    if dt_name == "f64" and fault is None:
        return P.run_case(case, _inputs(cid))[:2]
    return P.run_case(case, _inputs(cid), np.float64 if dt_name == "f64" else np.float32, fault, states=_run(cid)[1])[:2]


def test_the_cases_hold_what_the_issue_asks_for():
    cases = P.CASES
    assert {c[3] for c in cases if c[1] == "td3" and c[8] == "gradient-descent" and c[2] == "lowdim"} == {1, 2, 9}
    assert {c[15] for c in cases if c[8] == "adam" and c[15]} == {("above", "above"), ("below", "below")}
    assert any(c[12] is not None and c[11] == 2 for c in cases) and any(c[13] and c[14] == 3 for c in cases)
    assert any(c[2] == "8x8x6" and c[4] == 5 for c in cases) and {c[3] for c in cases if c[1] == "sac" and c[2] == "lowdim"} == {2, 9}
    assert any(P.is_stack(c) and c[1] == "sac" and c[4] == 8 for c in cases)          # the one stack at 64x64x18, B = 8
    assert all(2 <= c[5] <= 32 and 0 <= c[6] <= c[5] - 1 for c in cases) and any(c[5] == 32 for c in cases)
    assert {c[4] for c in cases} >= {5, 7, 8}          # a partial workgroup and whole ones


@pytest.mark.parametrize("cid", IDS)
def test_every_compared_minibatch_meets_the_conditions(cid):
    """on the float64 restatement alone: pooling differs from per-head truncation on a quarter of the rows, each target head supplies a
    quarter of the kept atoms, a tenth of each head's u on either side of kappa; the registered side of the clip by a factor of 1.2"""
    case = P.case_of(cid)
    outs, _vecs = _run(cid)
    assert len(outs) == P.nb_of(case)
    for k, o in enumerate(outs):
        for name, (value, floor) in P.conditions(case, o).items():
            assert value >= floor, (cid, k, name, value)
        if case[15]:
            for n, side in zip((o["actor_norm"], o["critic_norm"]), case[15]):
                assert n >= P.CLIP_SIDE_FACTOR * case[9] if side == "above" else n <= case[9] / P.CLIP_SIDE_FACTOR, (cid, k, side, n)
    if case[11] > 1:
        assert [o["applied"] for o in outs] == [(k + 1) % case[11] == 0 for k in range(len(outs))]


def test_the_seeds_are_the_first_on_which_the_conditions_hold():
    for case in P.CASES:
        for seed in range(1, P.SEEDS[case[0]]):
            outs = P.run_case(case, P.case_inputs(case, seed=seed))[0]
            assert any(v < fl for o in outs for v, fl in P.conditions(case, o).values()), (case[0], seed)


def test_the_bars_are_the_float32_restatements_error_times_eight():
    measured = P.measure_f32()
    print({k: "%.3e" % v for k, v in measured.items()})
    for a, b in P.PAIRS:
        measured[a] = measured[b] = max(measured[a], measured[b])
    for k, v in measured.items():
        assert v <= P.F32_ERR[k] <= 1.1 * v + 1e-10, (k, v, P.F32_ERR[k])
        assert P.bar(k) == (P.ATOL if 8.0 * P.F32_ERR[k] < P.ATOL / 4 else 8.0 * P.F32_ERR[k])


def _as_device(case, o32, batch, weights):
    """the float32 twin's minibatch as the device would report it: its atoms through rows_f32"""
    r32 = P.f32_twin_rows(case, o32, batch, weights)
    return dict(o32, loss=float(r32["loss"]), **{k: r32[k] for k in P.ROW_KEYS})


def _ratios(cid, dt_name, fault):
    case = P.case_of(cid)
    inputs = _inputs(cid)
    want, want_vecs = _run(cid)
    twin, twin_vecs = _run(cid, "f32")
    got, got_vecs = _run(cid, dt_name, fault)
    wts = P.case_weights(case, P.nb_of(case)) if case[13] else None
    out = []
    for k in range(P.nb_of(case)):
        start = P.initial_state(case, inputs) if k == 0 else want_vecs[k - 1]
        g = _as_device(case, got[k], inputs[4][k], None if wts is None else wts[k]) if dt_name == "f32" else got[k]
        out.append(P.ratios(case, inputs[0], start, g, got_vecs[k], want[k], want_vecs[k], twin[k], twin_vecs[k]))
    return out


@pytest.mark.parametrize("cid", IDS)
def test_the_float32_twin_stays_inside_the_gpu_bars(cid):
    for k, r in enumerate(_ratios(cid, "f32", None)):
        bad = {a: b for a, b in r.items() if not b <= 1.0}
        assert not bad, (cid, k, bad)


def _applies(case, fault):
    if fault in P.SAC_ONLY_FAULTS:
        return case[1] == "sac"
    if fault in P.NOISE_FAULTS:
        return case[1] == "sac" or case[12] is not None
    if fault in P.WEIGHT_FAULTS:
        return bool(case[13])
    return True


@pytest.mark.parametrize("fault", P.FAULTS)
def test_each_planted_fault_moves_a_compared_quantity_by_ten_times_its_bar(fault):
    seen = 0
    for case in P.CASES:
        if not _applies(case, fault):
            continue
        worst = max(max(r.values()) for r in _ratios(case[0], "f64", fault))
        print("%s on %s: %.1f bars" % (fault, case[0], worst))
        assert worst > POWER, (fault, case[0], worst)
        seen += 1
    assert seen >= 1, fault


def test_check_loss_is_the_formula_without_noise_or_weights():
    case = P.case_of("A2-B8-N5-d1-smoothed-delay2")
    inputs = _inputs(case[0])
    ref = P.restatement(case, inputs)
    loss, td, q = ref.check_loss(inputs[4][0])
    again = P.restatement(case, inputs).critic_gradients(inputs[4][0], noise=None, training=False)
    assert loss == again["loss"] and np.array_equal(td, again["td"]) and np.array_equal(q, again["q"]) and ref.tps_n == 0
