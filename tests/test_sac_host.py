"""Soft actor-critic on the host (no GPU): tests/sac_np.py against torch autograd and torch.distributions, the command line, the ABI
table, the derivation of the GPU bars, the conditions on the GPU test's cases and the power of every planted fault."""
import functools
import os
import re

import numpy as np
import pytest
import torch

from oracle import ddpg_np as O
from tests import sac_np as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the formulas against autograd
def _torch_policy(m, x, eps, lo, hi):
    ls = lo + 0.5 * (hi - lo) * (torch.tanh(x) + 1.0)
    u = m + torch.exp(ls) * eps
    return ls, u, torch.tanh(u)


@pytest.mark.parametrize("B,A", [(1, 1), (3, 2), (5, 8), (7, 16)])
def test_logp_head_gradient_dq_da_chain_and_g_alpha_against_torch_autograd(B, A):
    c = S.head_case(B, A)
    lo, hi, alpha, hbar = S.LO, S.HI, float(c["alpha"]), c["hbar"]
    m = torch.tensor(c["m"], dtype=torch.float64, requires_grad=True)
    x = torch.tensor(c["x"], dtype=torch.float64, requires_grad=True)
    eps = torch.tensor(c["eps1"], dtype=torch.float64)
    log_alpha = torch.tensor(np.log(alpha), dtype=torch.float64, requires_grad=True)
    ls, u, a = _torch_policy(m, x, eps, lo, hi)
    # the second opinion: Normal(m, exp(ls)) under a tanh, evaluated at the pre-tanh sample (no atanh of a saturated action)
    base = torch.distributions.Normal(m, torch.exp(ls))
    tanh = torch.distributions.transforms.TanhTransform()
    logp_t = (base.log_prob(u) - tanh.log_abs_det_jacobian(u, a)).sum(dim=1)
    want = S.policy(c["m"], c["x"], c["eps1"], lo, hi, np.float64)
    # (Normal.log_prob recovers eps as (u - m) / exp(ls), a cancellation at the small standard deviations of the lower tail: its own
    # error is |u| 2^-52 / (exp(ls) |eps|) relative to eps^2 -- 1e-9 of logp covers it, the restatement never forms that difference)
    np.testing.assert_allclose(want["logp"], logp_t.detach().numpy(), rtol=1e-9, atol=1e-10)
    np.testing.assert_allclose(want["a"], a.detach().numpy(), rtol=0, atol=1e-14)
    # a critic: any smooth Q(s, a); dq = dQ/da by autograd, the chain the device walks with its GEMMs
    g = torch.Generator().manual_seed(B * 100 + A)
    W1 = torch.randn(A, 6, dtype=torch.float64, generator=g)
    w2 = torch.randn(6, dtype=torch.float64, generator=g)
    q = (torch.tanh(a @ W1) @ w2)
    dq = torch.autograd.grad(q.sum(), a, retain_graph=True)[0]
    loss = (torch.exp(log_alpha).detach() * logp_t - q).sum()
    gm, gx = torch.autograd.grad(loss, (m, x), retain_graph=True)
    dm, dx = S.head_gradient(c["x"], want["a"], c["eps1"], dq.numpy(), alpha, lo, hi, np.float64)
    np.testing.assert_allclose(dm, gm.numpy(), rtol=1e-9, atol=1e-9)
    np.testing.assert_allclose(dx, gx.numpy(), rtol=1e-9, atol=1e-9)
    ga = torch.autograd.grad((-log_alpha * (logp_t.detach() + hbar)).mean(), log_alpha)[0]
    assert abs(float(S.temperature_gradient(want["logp"], hbar)) - float(ga)) <= 2.0 ** -23 * abs(float(ga)) + 1e-12


def test_the_stable_correction_is_the_naive_one_where_the_naive_one_is_accurate():
    u = np.linspace(-3.0, 3.0, 241)
    stable = 2.0 * (np.log(2.0) - u - S.softplus(-2.0 * u))
    np.testing.assert_allclose(stable, np.log(1.0 - np.tanh(u) ** 2), rtol=0, atol=1e-12)


def test_logp_is_continuous_and_finite_up_to_u_of_twelve():
    """log(1 - tanh(u)^2) = 2 (log 2 - |u|) + O(exp(-2 |u|)): the stable form follows it in float32 where 1 - a^2 has long been 0"""
    u = np.linspace(-12.0, 12.0, 4801).reshape(-1, 1)
    z = np.zeros_like(u)
    x0 = np.full_like(u, -20.0)        # ls = lo: the noise term is 0, u = m
    f64 = S.policy(u, x0, z, dt=np.float64)["logp"]
    f32 = S.policy(u, x0, z, dt=np.float32)["logp"]
    assert np.all(np.isfinite(f32))
    assert np.max(np.abs(f64 - f32)) < 2e-5
    assert np.max(np.abs(np.diff(f64))) < 2 * 0.005 + 1e-9                       # |d logp / du| = 2 |tanh u| <= 2: no jump anywhere
    asym = -S.LO - 0.5 * np.log(2 * np.pi) - 2.0 * (np.log(2.0) - np.abs(u[:, 0]))
    far = np.abs(u[:, 0]) > 10.0
    np.testing.assert_allclose(f64[far], asym[far], rtol=0, atol=1e-8)
    naive = S.policy(u, x0, z, dt=np.float32, fault="correction_1e-6")["logp"]   # ... and the 1e-6 form does not
    assert np.max(np.abs(naive[far] - f64[far])) > 1.0


def test_the_restated_draw_is_standard_normal_and_the_streams_differ():
    z1, z2 = S.noise(3, 5, 4096, 8, S.STREAM_S1), S.noise(3, 5, 4096, 8, S.STREAM_S2)
    assert abs(z1.mean()) < 0.02 and abs(z1.std() - 1.0) < 0.02 and np.abs(z1).max() < 5.8
    assert np.abs(z1 - z2).max() > 1.0 and np.abs(z1 - S.noise(3, 6, 4096, 8, S.STREAM_S1)).max() > 1.0
    from tests import tps_np
    np.testing.assert_array_equal(S.noise(3, 5, 16, 4, 0x100), tps_np.standard_normals(3, 5, 16, 4))      # one generator, three streams


def test_adam_element_against_torch():
    p = torch.tensor([np.log(0.1)], dtype=torch.float32, requires_grad=True)
    opt = torch.optim.Adam([p], lr=1e-2, betas=(0.9, 0.999), eps=1e-8)
    la, m, v = np.float32(np.log(0.1)), np.float32(0), np.float32(0)
    for t, g in enumerate([0.7, -1.3, 2.1, 0.05], 1):
        p.grad = torch.tensor([g], dtype=torch.float32)
        opt.step()
        la, m, v = S.adam(la, g, m, v, t, 1e-2)
        # (TensorFlow folds the bias corrections into the rate and keeps epsilon outside: the two agree to epsilon's weight)
        assert abs(float(la) - float(p.detach()[0])) < 1e-6, t


# ---- the command line
OPTION_KEYS = ("soft_actor_critic", "sac_init_temperature", "sac_target_entropy", "sac_temperature_learning_rate", "sac_log_std_min",
               "sac_log_std_max", "sac_seed")


def test_the_parser_takes_the_options_and_they_are_absent_unless_given():
    from cartpoleplusplus_amd import ddpg_cartpole as D
    o = D.build_parser().parse_args([])
    for k in OPTION_KEYS:
        assert not hasattr(o, k), k
    d = D.default_opts()
    assert [getattr(d, k) for k in OPTION_KEYS] == [False] + [None] * 6
    assert D.soft_actor_critic(o) is None and D.soft_actor_critic(d) is None
    v = D.soft_actor_critic(D.build_parser().parse_args(["--soft-actor-critic"]), 3)
    assert v == {"init_temperature": float(np.float32(0.1)), "target_entropy": -3.0, "temperature_learning_rate": float(np.float32(1e-4)),
                 "log_std_min": -10.0, "log_std_max": 2.0, "seed": 0}
    o = D.build_parser().parse_args(["--soft-actor-critic", "--sac-init-temperature", "0.5", "--sac-target-entropy", "-1.5",
                                     "--sac-temperature-learning-rate", "0", "--sac-log-std-min", "-5", "--sac-log-std-max", "1", "--sac-seed", "9",
                                     "--twin-q", "--n-step", "3", "--prioritized-replay", "--ddpg-optimiser", "Adam"])
    assert D.soft_actor_critic(o, 2) == {"init_temperature": 0.5, "target_entropy": -1.5, "temperature_learning_rate": 0.0, "log_std_min": -5.0,
                                         "log_std_max": 1.0, "seed": 9}


@pytest.mark.parametrize("argv", [["--sac-init-temperature", "0.1"], ["--sac-target-entropy", "-2"], ["--sac-temperature-learning-rate", "1e-3"],
                                  ["--sac-log-std-min", "-5"], ["--sac-log-std-max", "1"], ["--sac-seed", "1"],      # options without the flag
                                  ["--soft-actor-critic", "--target-policy-noise", "0.2"],
                                  ["--soft-actor-critic", "--policy-delay", "2"],
                                  ["--soft-actor-critic", "--distributional-critic", "--v-min", "0", "--v-max", "1"],
                                  ["--soft-actor-critic", "--quantile-critic"],
                                  ["--soft-actor-critic", "--use-batch-norm"],
                                  ["--soft-actor-critic", "--use-dropout"],
                                  ["--soft-actor-critic", "--data-parallel"],
                                  ["--soft-actor-critic", "--sac-init-temperature", "0"],
                                  ["--soft-actor-critic", "--sac-init-temperature", "-1"],
                                  ["--soft-actor-critic", "--sac-init-temperature", "inf"],
                                  ["--soft-actor-critic", "--sac-target-entropy", "nan"],
                                  ["--soft-actor-critic", "--sac-temperature-learning-rate=-1e-3"],
                                  ["--soft-actor-critic", "--sac-log-std-min", "2", "--sac-log-std-max", "2"],
                                  ["--soft-actor-critic", "--sac-log-std-min", "3"],
                                  ["--soft-actor-critic", "--sac-log-std-max", "inf"],
                                  ["--soft-actor-critic", "--sac-seed", "-1"]],
                         ids=lambda a: " ".join(a))
def test_the_parsers_refusals(argv):
    from cartpoleplusplus_amd import ddpg_cartpole as D
    o = D.build_parser().parse_args(argv)
    with pytest.raises(SystemExit):
        D.soft_actor_critic(o, 2)


def test_the_agent_refuses_before_anything_exists_on_the_device():
    """soft_actor_critic() runs at the top of the agent's constructor: the refusal needs no device (this test has none)"""
    from cartpoleplusplus_amd import ddpg_cartpole as D
    from tests.helpers import FakeEnv
    for kw in (dict(soft_actor_critic=True, policy_delay=2), dict(soft_actor_critic=True, target_policy_noise=0.2),
               dict(soft_actor_critic=True, quantile_critic=True), dict(sac_seed=3), dict(soft_actor_critic=True, use_batch_norm=True),
               dict(soft_actor_critic=True, sac_log_std_min=1.0, sac_log_std_max=0.0)):
        D.set_opts(D.default_opts(use_raw_pixels=False, **kw))
        with pytest.raises(SystemExit):
            D.DeepDeterministicPolicyGradientAgent(FakeEnv((2, 2, 7), 2))
    D.set_opts(D.default_opts(use_raw_pixels=False, soft_actor_critic=True))
    with pytest.raises(SystemExit):
        D.DeepDeterministicPolicyGradientAgent(FakeEnv((2, 2, 7), 65))
    D.set_opts(D.default_opts())


def test_naf_does_not_take_the_options():
    from cartpoleplusplus_amd import naf_cartpole as F
    assert not set(OPTION_KEYS) & set(vars(F.build_parser().parse_args([])))
    with pytest.raises(SystemExit):
        F.build_parser().parse_args(["--soft-actor-critic"])


NEW_ENTRY_POINTS = ("cpp_net_create_gaussian", "cpp_net_gaussian_info", "cpp_net_forward_gaussian", "cpp_ddpg_set_sac", "cpp_ddpg_last_sac",
                    "cpp_ddpg_sac_temperature")


def test_every_new_entry_point_is_bound_and_cites_the_reference_lines_it_extends():
    from cartpoleplusplus_amd import _lib
    header = open(os.path.join(ROOT, "include", "cartpolepp_abi.h")).read()
    csrc = os.path.join(ROOT, "cartpoleplusplus_amd", "csrc")
    source = "".join(open(os.path.join(csrc, f)).read() for f in sorted(os.listdir(csrc)) if f.startswith("rt_") and f.endswith(".cpp"))
    for name in NEW_ENTRY_POINTS:
        assert name in _lib.SIGNATURES, name
        for text, pattern in ((header, r"/\*((?:(?!\*/).)*)\*/\s*int %s\(" % name), (source, r"((?://[^\n]*\n)+)extern \"C\" int %s\(" % name)):
            m = re.search(pattern, text, flags=re.S)
            assert m and re.search(r"(ddpg_cartpole|util)\.py:\d+", m.group(1)), name


# ---- the cases the GPU module shares
@functools.lru_cache(maxsize=None)
def _rows(B, A, dt_name="f64", fault=None):
    return S.rows_of(S.head_case(B, A), np.float64 if dt_name == "f64" else np.float32, fault)


@pytest.mark.parametrize("B,A", S.CASES)
def test_the_cases_hold_what_the_issue_asks_for(B, A):
    """on the float64 restatement alone: a tenth of the action components saturated, a tenth small, x in both tails of the bound"""
    c, r = S.head_case(B, A), _rows(B, A)
    a = np.abs(np.concatenate([r["a"].ravel(), r["a2"].ravel()]))
    assert (a > 0.99).mean() >= 0.1 and (a < 0.5).mean() >= 0.1, ((a > 0.99).mean(), (a < 0.5).mean())
    if B * A >= 2:
        assert np.tanh(c["x"].max()) > 0.98 and np.tanh(c["x"].min()) < -0.98
    assert np.abs(r["u"]).max() > 3.0


def test_the_cases_cover_the_shapes_off_the_wave_and_workgroup_multiples():
    assert {b for b, _ in S.CASES} == {1, 3, 5, 64, 65, 257} and {a for _, a in S.CASES} == {1, 2, 3, 8, 16}


def test_the_bars_are_the_float32_restatements_error_times_eight():
    """re-measured here; DESIGN records the figures.  The ordinary 1e-5 wherever 8x the error is below a quarter of it"""
    for k in ("a", "a2", "q", "td", "dq_da"):
        assert S.bar(k) == 1e-5
    for k in S.ROW_KEYS:
        e, b = S.measured_error(k), S.bar(k)
        assert b == (1e-5 if 8 * e < 2.5e-6 else 8 * e), (k, e, b)
        assert b < 1e-3, (k, b)
        print("bar %-10s f32 error %.3e bar %.3e" % (k, e, b))
    assert S.eps_bar() <= 1e-4
    print("bar eps        %.3e" % S.eps_bar())


@pytest.mark.parametrize("B,A", S.CASES)
def test_the_float32_evaluation_stays_inside_the_gpu_bounds(B, A):
    f64, f32 = _rows(B, A), _rows(B, A, "f32")
    for k in ("a", "a2") + S.ROW_KEYS:
        assert np.max(np.abs(np.asarray(f64[k], np.float64) - np.asarray(f32[k], np.float64))) <= S.bar(k) / 8 + 1e-12 or S.bar(k) == 1e-5, k


ROW_FAULTS = ("correction_1e-6", "correction_missing", "entropy_sign", "entropy_unmasked", "one_eps_for_both_draws", "bounds_swapped",
              "no_2_alpha_a", "no_minus_alpha_in_dx", "no_std_eps_in_dx", "gradient_wrt_alpha", "g_alpha_summed", "adam_bias_one_step_off")
COMPARED = ("a", "a2", "logp", "logp2", "r_soft", "dm", "dx", "g_alpha", "log_alpha")


def _bar(k):
    return S.bar("logp" if k == "logp2" else k)


@pytest.mark.parametrize("fault", ROW_FAULTS)
def test_each_row_local_fault_moves_a_compared_quantity_by_ten_times_its_gpu_bar(fault):
    best = 0.0
    for B, A in S.CASES:
        good, bad = _rows(B, A), _rows(B, A, "f64", fault)
        for k in COMPARED:
            best = max(best, float(np.max(np.abs(np.asarray(good[k], np.float64) - np.asarray(bad[k], np.float64)))) / _bar(k))
    assert best > 10.0, (fault, best)


def test_the_noise_faults_move_eps_by_far_more_than_its_bar():
    for B, A in S.CASES:
        if B * A < 4:
            continue
        z = S.noise(7, 3, B, A, S.STREAM_S2)
        assert np.abs(z - S.noise(7, 3, B, A, S.STREAM_S2, fault="eps_not_refreshed")).max() > 10 * S.eps_bar()
        assert np.abs(z - S.noise(7, 3, B, A, S.STREAM_S2, fault="one_eps_for_both_draws")).max() > 10 * S.eps_bar()


# ---- the learner-level faults: a small low-dimensional learner over three minibatches
def _learner(fault=None, B=5, A=2, nb=3):
    rng = np.random.default_rng(11)
    kw = dict(pixel=False, state_elems=6)
    aspec, cspec = S.gaussian_spec(A, [12, 8], **kw), O.NetSpec("critic", A, [12, 8], **kw)
    pa = (O.init_params(aspec, rng) + rng.normal(0, 0.3, aspec.num_params())).astype(np.float32)
    pc = (O.init_params(cspec, rng) + rng.normal(0, 0.1, cspec.num_params())).astype(np.float32)
    hyper = O.Hyper(actor_lr=0.05, critic_lr=0.05, discount=0.9, gradient_clip=None, target_update_rate=0.01) if hasattr(O, "Hyper") else O.DEFAULT_HYPER
    ref = S.SacDDPG(aspec, cspec, pa, pc, np.float64, hyper, state=S.SacState(0.2, -float(A), 1e-2, 7))
    outs = []
    for i in range(nb):
        s1, s2 = rng.normal(0, 1, (B, 6)).astype(np.float32), rng.normal(0, 1, (B, 6)).astype(np.float32)
        batch = (s1, rng.uniform(-1, 1, (B, A)).astype(np.float32), rng.normal(0, 1, (B, 1)).astype(np.float32), np.ones((B, 1), np.float32), s2)
        n = 0 if fault == "eps_not_refreshed" else i
        e1 = S.noise(7, n, B, A, S.STREAM_S1)
        e2 = e1 if fault == "one_eps_for_both_draws" else S.noise(7, n, B, A, S.STREAM_S2)
        outs.append(ref.train_minibatch(batch, e1, e2, fault if fault in S.FAULTS else None))
        ref.update_targets()
    return outs


@pytest.mark.parametrize("fault", ("target_actor_soft_updated", "copy_before_update", "temperature_updated_first", "eps_not_refreshed"))
def test_each_learner_level_fault_moves_a_compared_quantity_by_ten_times_its_gpu_bar(fault):
    good, bad = _learner(), _learner(fault)
    best = 0.0
    for g, b in zip(good, bad):
        for k, bark in (("target_actions", 1e-5), ("r_soft", S.bar("r_soft")), ("td", 1e-5), ("logp2", S.bar("logp")), ("actions", 1e-5)):
            best = max(best, float(np.max(np.abs(np.asarray(g[k], np.float64) - np.asarray(b[k], np.float64)))) / bark)
    assert best > 10.0, (fault, best)


def test_every_fault_is_tested():
    assert set(S.FAULTS) == set(ROW_FAULTS) | {"target_actor_soft_updated", "copy_before_update", "temperature_updated_first", "eps_not_refreshed"} | set(S.COMPOSED_FAULTS)
    assert len(S.FAULTS) == 27 and len(S.COMPOSED_FAULTS) == 11      # (every composed fault: test_each_composed_fault_... below)


def test_the_learner_copies_the_actor_into_the_target_and_reads_the_temperature_before_its_update():
    outs = _learner(nb=2)
    assert outs[0]["alpha"] == pytest.approx(0.2, rel=1e-6) and outs[1]["alpha"] != outs[0]["alpha"]
    assert abs(float(outs[1]["alpha"]) - float(np.exp(np.float64(outs[0]["log_alpha"])))) < 1e-12


# ---- the composed learner (tests.sac_np.ComposedSac): twin critics, the optimisers' rules, importance weights, n-step memories
def _torch_net(layout, flat):
    p, off = {}, 0
    for name, shape in layout:
        n = int(np.prod(shape))
        p[name] = torch.tensor(np.asarray(flat[off:off + n], np.float64).reshape(shape), requires_grad=True)
        off += n
    assert off == len(flat)
    return p


def _torch_forward(spec, p, s, a=None, suffix="", first=0, h=None):
    """the fully connected stack of a low-dimensional net from layer `first` on (suffix 'b': the twin variables)"""
    h = s.reshape(s.shape[0], -1) if h is None else h
    for name, _n_in, _n_out, act, cat in spec.fc[first:]:
        if cat:
            h = torch.cat([h, a], dim=1)
        y = h @ p[name + suffix + "/weights"] + p[name + suffix + "/biases"]
        h = {"relu": torch.relu, "tanh": torch.tanh}.get(act, lambda t: t)(y)
    return h


def _torch_logp(out, eps, A):
    m, x = out[:, :A], out[:, A:]
    ls = S.LO + 0.5 * (S.HI - S.LO) * (torch.tanh(x) + 1.0)
    u = m + torch.exp(ls) * eps
    a = torch.tanh(u)
    corr = 2.0 * (np.log(2.0) - u - torch.nn.functional.softplus(-2.0 * u))
    return a, (-0.5 * eps * eps - ls - 0.5 * np.log(2.0 * np.pi) - corr).sum(dim=1)


def test_one_composed_minibatch_against_torch_autograd():
    """float64, low-dimensional (the whole critic stack twinned), twin heads, importance weights, the clip engaged on both lists, gradient
    descent: both pre-clip lists, both norms, g_alpha, the loss and both updated parameter vectors against autograd of
    sum_b (alpha logp_b - Q1(s1, a_b)) and mean_b w_b (td_1^2 + td_2^2), as tests/test_torch_twin_step.py holds the plain step"""
    from tests import twin_np as W
    case = S.composed_case("lowdim-twin-adam-A3-B16")
    A, B = case[2], case[3]
    specs, P, _ep, _idxs, batches = S.composed_inputs(case)
    hyper = S.composed_hyper(case)._replace(actor_lr=1e-2, critic_lr=5e-2, gradient_clip=0.5)
    ref = S.ComposedSac(specs[0], specs[1], P[0], P[1], np.float64, hyper, S.SacState(S.C_TEMPERATURE, -float(A), S.C_TEMPERATURE_LR, 0))
    ref.set_target_critic(P[3])
    w = W.case_weights((None, None, None, B), 1)[0].astype(np.float64)
    e1, e2 = S.noise(5, 0, B, A, S.STREAM_S1), S.noise(5, 0, B, A, S.STREAM_S2)
    want = ref.train_minibatch(batches[0], e1, e2, weights=w)
    T = lambda v: torch.tensor(np.asarray(v, np.float64))
    s1, a, r, mask, s2 = (T(v) for v in batches[0])
    alpha = float(np.exp(np.float64(np.float32(np.log(np.float32(S.C_TEMPERATURE))))))
    pa, pc, ptc = (_torch_net(lay, flat) for lay, flat in ((specs[0].layout(), P[0]), (W.full_layout(specs[1]), P[1]),
                                                                 (W.full_layout(specs[1]), P[3])))
    # the actor's list
    act, logp = _torch_logp(_torch_forward(specs[0], pa, s1), T(e1), A)
    q1 = _torch_forward(specs[1], pc, s1, act)
    g_a = torch.autograd.grad((alpha * logp - q1[:, 0]).sum(), list(pa.values()))
    g_a = np.concatenate([g.numpy().ravel() for g in g_a])
    np.testing.assert_allclose(want["actor_grads"], g_a, rtol=1e-8, atol=1e-10)
    log_alpha = torch.tensor(np.log(alpha), requires_grad=True)
    ga = torch.autograd.grad((-log_alpha * (logp.detach() + (-float(A)))).mean(), log_alpha)[0]
    assert abs(float(want["g_alpha"]) - float(ga)) <= 2.0 ** -23 * abs(float(ga)) + 1e-12
    # the critic's: one a' for both target heads, the minimum, both heads onto it
    with torch.no_grad():
        a2, logp2 = _torch_logp(_torch_forward(specs[0], pa, s2), T(e2), A)
        tq1, tq2 = _torch_forward(specs[1], ptc, s2, a2), _torch_forward(specs[1], ptc, s2, a2, suffix="b")
        y = r - mask * hyper.discount * alpha * logp2[:, None] + mask * hyper.discount * torch.minimum(tq1, tq2)
    td1, td2 = _torch_forward(specs[1], pc, s1, a) - y, _torch_forward(specs[1], pc, s1, a, suffix="b") - y
    loss = (T(w) * (td1 * td1 + td2 * td2)).mean()
    g_c = np.concatenate([g.numpy().ravel() for g in torch.autograd.grad(loss, list(pc.values()))])
    np.testing.assert_allclose(want["critic_grads"], g_c, rtol=1e-8, atol=1e-10)
    np.testing.assert_allclose(want["loss"], loss.item(), rtol=1e-10)
    np.testing.assert_allclose(want["td"], td1.detach().numpy(), rtol=1e-9, atol=1e-12)
    np.testing.assert_allclose(want["td2"], td2.detach().numpy(), rtol=1e-9, atol=1e-12)
    assert 0.25 <= ref.min_share[0] <= 0.75 and float(w.max() - w.min()) > 1e-3
    for got, g, p0, lr, norm in ((ref.actor.flat(), g_a, P[0], 1e-2, want["actor_norm"]), (ref.critic.flat(), g_c, P[1], 5e-2, want["critic_norm"])):
        n = float(np.sqrt((g * g).sum()))
        assert n > 1.2 * 0.5 and abs(norm - n) <= 1e-9 * n
        np.testing.assert_allclose(got, p0.astype(np.float64) - lr * g * 0.5 / n, rtol=1e-9, atol=1e-12)
    np.testing.assert_array_equal(ref.target_actor.flat(), ref.actor.flat())


@functools.lru_cache(maxsize=None)
def _composed(cid):
    """the float64 run of a case and its float32 twin, every minibatch of the twin from the float64 state before it"""
    case = S.composed_case(cid)
    inp = S.composed_inputs(case)
    o64, v64, ref = S.run_composed(case, inp)
    rows, weights = [o["rows"] for o in o64], [o["weights"] for o in o64]
    o32, v32, _ = S.run_composed(case, inp, np.float32, states=v64, rows=rows, weights=weights)
    return case, inp, o64, v64, ref, o32, v32


def _composed_ratios(cid, got, got_vec):
    case, inp, o64, v64, _ref, o32, v32 = _composed(cid)
    starts = [S.initial_state(inp)] + v64[:-1]
    return [S.ratios(case, inp[0], starts[k], got[k], got_vec[k], o64[k], v64[k], o32[k], v32[k]) for k in range(S.C_MINIBATCHES)]


COMPOSED_IDS = [c[0] for c in S.C_CASES]


def test_the_single_ops_case_meets_its_conditions():
    case, seed, nb = S.C_SINGLE_OPS
    inp = S.composed_inputs(case, seed=seed, nb=nb)
    o64, v64, ref = S.run_composed(case, inp)
    o32, _v32, _ = S.run_composed(case, inp, np.float32, states=v64)
    assert len(o64) == nb == 3 and all(0.25 <= s <= 0.75 for s in ref.min_share), ref.min_share
    assert all(min(o["actor_norm"], o["critic_norm"]) >= 1.2 * case[5] for o in o64)
    assert v64[-1]["step"] == [3, 3] and v64[-1]["alpha_step"] == 3


def test_the_composed_cases_are_the_ones_the_issue_lists():
    assert [(c[1], c[2], c[3], c[4], c[7], c[8], c[9], c[10]) for c in S.C_CASES] == [
        ("16x16x6", 2, 8, "gradient-descent", True, False, 1, 0), ("16x16x6", 1, 5, "adam", True, False, 1, 0),
        ("16x16x6", 3, 7, "momentum-0.5", True, False, 1, 0), ("16x16x6", 9, 8, "adam", True, False, 1, 0),
        ("16x16x6", 2, 8, "adam", False, False, 1, 0), ("16x16x6", 2, 8, "adam", True, True, 1, 0), ("16x16x6", 2, 8, "adam", True, False, 3, 0),
        ("lowdim", 3, 16, "adam", True, False, 1, 0), ("64x64x18", 2, 8, "adam", True, False, 1, 0), ("16x16x6", 2, 8, "adam", True, False, 1, 2)]
    assert S.composed_case("twin-sgd-clip0.5-A2-B8")[5:7] == (0.5, 0.25) and S.composed_case("twin-adam-unclipped-A1-B5")[5:7] == (1e4, 1.0)
    assert S.C_TEMPERATURE_LR == 1e-2


@pytest.mark.parametrize("cid", COMPOSED_IDS)
def test_the_composed_cases_meet_their_conditions(cid):
    """on the float64 restatement: each list's norm on its side of the clip by a factor of 1.2, each target head the minimum on a quarter
    of the rows, weights that weigh, n-step masks outside {0, 1}, and the float32 twin on the float64 routes of the conv trunks (pool
    arg-max and ReLU decision per window; the low-dimensional case has none) in every minibatch"""
    case, inp, o64, _v64, ref, o32, _v32 = _composed(cid)
    clip = case[5]
    for o in o64:
        for n, side in zip((o["actor_norm"], o["critic_norm"]), S.C_SIDES[cid]):
            assert n >= 1.2 * clip if side == "above" else n <= clip / 1.2, (cid, side, n, clip)
    if case[7]:
        assert len(ref.min_share) == S.C_MINIBATCHES and all(0.25 <= s <= 0.75 for s in ref.min_share), ref.min_share
    if case[8]:
        assert all(float(o["weights"].max() - o["weights"].min()) > 1e-3 for o in o64)
    if case[9] > 1:
        masks = np.concatenate([o["batch"][3].ravel() for o in o64])
        assert int(((masks != 0) & (masks != 1)).sum()) >= 2, masks
    if case[10]:
        from tests import shift_np
        # (every minibatch shifts some state_1 image and some state_2 image)
        assert all(np.abs(shift_np.shifts(S.C_SHIFT_SEED, k, case[3], case[10])).max(axis=(1, 2)).min() > 0 for k in range(S.C_MINIBATCHES))
        assert not np.array_equal(o64[0]["batch"][0], S.composed_batches(case[:10] + (0,), inp[2], o64[0]["rows"])[0][0])
    assert all(np.array_equal(x, y) for a, b in zip(o64, o32) for x, y in zip(a["routes"], b["routes"]))
    # (the temperature moves, and an update is not hidden behind the parameters)
    assert abs(float(o64[-1]["log_alpha"]) - float(np.log(np.float32(S.C_TEMPERATURE)))) > 1e-3


ROW_OWN_BARS = ("logp", "logp2", "r_soft", "g_alpha", "log_alpha", "alpha_m", "alpha_v", "loss", "actor_norm", "critic_norm")


@pytest.mark.parametrize("cid", COMPOSED_IDS)
def test_the_float32_composed_restatement_stays_inside_every_gpu_bar(cid):
    """bar / 8 on the quantities whose bars are derived ones, the bar itself where it is the project's 1e-5 (as
    test_the_float32_evaluation_stays_inside_the_gpu_bounds has it), bar / F32_GRAD_FACTOR on the lists, the deltas and the slots"""
    from tests.helpers import F32_GRAD_FACTOR
    _case, _inp, _o64, _v64, _ref, o32, v32 = _composed(cid)
    for k, r in enumerate(_composed_ratios(cid, o32, v32)):
        for key, v in r.items():
            lim = 1.0 / 8 if key in ROW_OWN_BARS else 1.0 if key in S.ROW_BARS else 1.0 / F32_GRAD_FACTOR + 1e-9
            assert v <= lim, (cid, k, key, v, lim)


def test_the_log_alpha_bar_of_the_composed_cases_is_re_measured():
    worst = 0.0
    for cid in COMPOSED_IDS:
        _case, _inp, _o64, v64, _ref, _o32, v32 = _composed(cid)
        worst = max(worst, max(abs(a["log_alpha"] - b["log_alpha"]) for a, b in zip(v64, v32)))
    print("composed cases: float32 restatement's worst |log_alpha error| %.3e, bar %.3e" % (worst, S.composed_bar("log_alpha")))
    assert worst <= S.C_LOG_ALPHA_F32_ERROR + 1e-12
    assert S.composed_bar("log_alpha") == (1e-5 if 8 * S.C_LOG_ALPHA_F32_ERROR < 2.5e-6 else 8 * S.C_LOG_ALPHA_F32_ERROR)


POWER_IDS = [c for c in COMPOSED_IDS if "64x64" not in c]      # (the 16x16x6 and low-dimensional cases show every fault; 64x64x18 costs seconds per run)


@pytest.mark.parametrize("fault", S.COMPOSED_FAULTS)
def test_each_composed_fault_moves_a_compared_quantity_by_ten_times_its_gpu_bar(fault):
    """in the restatement alone, over the GPU cases, every minibatch from the common start the device comparison uses"""
    best, where = 0.0, None
    for cid in POWER_IDS:
        case, inp, o64, v64, _ref, _o32, _v32 = _composed(cid)
        if (fault in ("weights_missing", "weights_on_actor") and not case[8]) or (fault == "entropy_discount_only" and case[9] == 1) \
                or (fault in ("target_q1_only", "actor_follows_q2", "actor_follows_min") and not case[7]):
            continue
        bad, bad_vec, _r = S.run_composed(case, inp, fault=fault, states=v64, rows=[o["rows"] for o in o64], weights=[o["weights"] for o in o64])
        for k, r in enumerate(_composed_ratios(cid, bad, bad_vec)):
            key = max(r, key=lambda x: r[x])
            if r[key] > best:
                best, where = float(r[key]), (cid, k, key)
        if best > 10.0:
            break
    print("%s: %.3g x the bar at %s" % (fault, best, where))
    assert best > 10.0, (fault, best, where)
