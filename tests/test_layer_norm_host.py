"""Feature layer norm on the host: tests/layer_norm_np.py (the float64 restatement tests/test_gpu_layer_norm.py holds the device to)
against torch autograd, the bars its cases derive from the float32 twin, the conditions under which those cases can see anything, the
faults they catch, and the command line's flags and refusals.  No GPU."""
import argparse

import numpy as np
import pytest

from oracle import ddpg_np as O
from tests import layer_norm_np as L
from tests.helpers import delta_bound, twin_rs


# ---- a. the restatement against torch autograd, float64
@pytest.mark.parametrize("act", ["tanh", "relu"])
@pytest.mark.parametrize("kind", ["actor", "critic"])
def test_restatement_matches_torch_autograd(kind, act):
    import torch
    import torch.nn.functional as F
    specs, P, _ep, _idxs, batches = L.host_case(L.EDGE_SHAPE, 6, 1, 5, (37, 20, 10), act)
    spec, flat = (specs[0], P[0]) if kind == "actor" else (specs[1], P[1])
    net = L.LnNet(spec, flat, np.float64)
    s1, a = batches[0][0], batches[0][1]
    c = net.forward(s1, action=a if kind == "critic" else None)
    rng = np.random.default_rng(0)
    dout = rng.normal(size=c["out"].shape)
    grads, d_action = net.backward(c, dout)
    # torch: the fully connected stack from the oracle's conv features, which are a leaf
    t = lambda x: torch.tensor(np.asarray(x, np.float64), requires_grad=True)
    feat = t(c["fc"][0][0])
    W = {n: t(v) for n, v in net.p.items() if not n.startswith("conv")}
    name0 = spec.fc[0][0]
    z = feat @ W[name0 + "/weights"] + W[name0 + "/biases"]
    z.retain_grad()
    u = F.layer_norm(z, (spec.fc[0][2],), W[name0 + "/LayerNorm/gamma"], W[name0 + "/LayerNorm/beta"], spec.eps)
    h = torch.tanh(u) if act == "tanh" else torch.relu(u)
    assert np.abs(h.detach().numpy() - c["ln"]["y"]).max() < 1e-12
    ta = t(a)
    for name, _ni, _no, lact, cat in spec.fc[1:]:
        if cat:
            h = torch.cat([h, ta], dim=1)
        h = h @ W[name + "/weights"] + W[name + "/biases"]
        h = torch.relu(h) if lact == "relu" else torch.tanh(h) if lact == "tanh" else h
    assert np.abs(h.detach().numpy() - c["out"]).max() < 1e-12
    (h * torch.tensor(dout)).sum().backward()
    close = lambda got, want, what: np.testing.assert_allclose(got, want.numpy(), rtol=1e-9, atol=1e-12, err_msg=what)
    close(c["ln"]["dz"], z.grad, "dz")
    close(c["d_flat"], feat.grad, "d flat")
    for n, v in W.items():
        close(grads[n], v.grad, n)
    if kind == "critic":
        close(d_action, ta.grad, "dQ/da")
    # ... and the flat list is in layout order, gamma and beta behind every plain variable
    names = [n for n, _s in spec.layout()]
    assert names[-2:] == [name0 + "/LayerNorm/gamma", name0 + "/LayerNorm/beta"] and names[:-2] == [n for n, _s in spec.plain_layout()]
    assert list(grads) == names


def test_the_restatement_composes_with_the_optimiser_and_delay_restatements():
    """every network tests.ddpg_opt_np / tests.td3_np build for an LnSpec normalises, and their slots cover gamma and beta"""
    from tests import ddpg_opt_np as R
    from tests import td3_np as T3
    specs, P, _ep, _idxs, batches = L.host_case(L.WHOLE_SHAPE, 4, 2, 2, (33, 20, 10))
    hp = O.Hyper(1e-2, 5e-2, 0.9, 0.5, 0.25)
    ref = L.with_feature_norm(R.DDPGWithOptimiser)(specs[0], specs[1], P[0], P[1], np.float64, hp, "Adam", {"beta1": 0.8})
    ref.set_targets(P[2], P[3])
    for b in batches:
        ref.train_minibatch(b)
    ref.update_targets()
    for net in (ref.actor, ref.critic, ref.target_actor, ref.target_critic):
        assert type(net) is L.LnNet
    st = ref.state()
    nA, kA = len(P[0]), specs[0].num_plain()
    assert len(st["m"]) == len(P[0]) + len(P[1]) and np.abs(st["m"][kA:nA]).min() > 0 and np.abs(st["v"][kA:nA]).min() > 0
    assert np.abs(ref.actor.flat()[kA:] - P[0][kA:]).min() > 0 and np.abs(ref.target_actor.flat()[kA:] - P[2][kA:]).min() > 0
    d = L.with_feature_norm(T3.DelayedDDPG)(specs[0], specs[1], P[0], P[1], np.float64, hp, delay=2, smoothing=(0.2, 0.5, 3))
    d.set_targets(P[2], P[3])
    for b in batches:
        d.train_minibatch(b)
    assert type(d.actor) is L.LnNet and d.schedule == [False, True]


def test_the_restatement_composes_with_the_twin_restatement():
    """tests.twin_np.TwinDDPG on normalised networks: both critics are the twin critic over the norm, the critic's whole list -- gamma and
    beta of the shared layer, which both heads feed -- against torch autograd, the twin's slots and targets cover the longer buffer"""
    import torch
    import torch.nn.functional as F
    from tests import twin_np as W
    specs, P, _ep, _idxs, batches, _seed, want, outs, twin = L.twin_case("twin-adam")
    ref = L.with_feature_norm(W.TwinDDPG)(specs[0], specs[1], P[0], P[1], np.float64)
    ref.set_targets(P[2], P[3])
    assert type(ref.actor) is L.LnNet and isinstance(ref.critic, W.TwinCritic) and type(ref.critic.h1) is L.LnNet and type(ref.target_critic.h1) is L.LnNet
    s1, a = batches[0][0], batches[0][1]
    c = ref.critic.forward(s1, action=a)
    rng = np.random.default_rng(0)
    d1, d2 = rng.normal(size=c["out"].shape), rng.normal(size=c["out2"].shape)
    grads, _da = ref.critic.backward(c, d1, d2)
    t = lambda x: torch.tensor(np.asarray(x, np.float64), requires_grad=True)
    spec = specs[1]
    Wt = {n: t(v) for n, v in list(ref.critic.h1.p.items()) + list(ref.critic.p2.items()) if not n.startswith("conv")}
    feat, ta = t(c["fc"][0][0]), t(a)
    h = torch.tanh(F.layer_norm(feat @ Wt["hidden1/weights"] + Wt["hidden1/biases"], (200,), Wt["hidden1/LayerNorm/gamma"], Wt["hidden1/LayerNorm/beta"], spec.eps))
    h = torch.cat([torch.relu(h @ Wt["hidden2/weights"] + Wt["hidden2/biases"]), ta], dim=1)
    qs = [(torch.relu(h @ Wt["hidden3" + sfx + "/weights"] + Wt["hidden3" + sfx + "/biases"]) @ Wt["q_value" + sfx + "/weights"] + Wt["q_value" + sfx + "/biases"]) for sfx in ("", "b")]
    assert np.abs(qs[0].detach().numpy() - c["out"]).max() < 1e-12 and np.abs(qs[1].detach().numpy() - c["out2"]).max() < 1e-12
    ((qs[0] * torch.tensor(d1)).sum() + (qs[1] * torch.tensor(d2)).sum()).backward()
    for n, v in Wt.items():
        np.testing.assert_allclose(grads[n], v.grad.numpy(), rtol=1e-9, atol=1e-12, err_msg=n)
    assert list(grads) == [n for n, _s in W.full_layout(spec)]
    # the case itself: clipped, each head the minimum on a quarter of the rows, slots and targets over the longer buffer, the twin inside the bounds
    k, n = spec.num_plain(), 400
    assert len(want[1]) == len(P[1]) and np.abs(want[1][k:k + n] - P[1][k:k + n]).min() > 0 and np.abs(want[3][k:k + n] - P[3][k:k + n]).min() > 0
    assert np.abs(want[4][len(P[0]) + k:len(P[0]) + k + n]).min() > 0
    start = list(P) + [np.zeros_like(want[4]), np.zeros_like(want[5])]
    for w, tw, p, r in zip(want, twin, start, twin_rs(want, twin, start)):
        assert np.linalg.norm(tw - w) <= delta_bound(p, w - p, r, 3)
    v = np.arange(len(P[1]), dtype=np.float64)
    assert np.array_equal(L.twin_from_device(spec, L.twin_to_device(spec, v)), v) and np.array_equal(L.twin_to_device(spec, v)[-n:], v[k:k + n])


@pytest.mark.parametrize("cid", list(L.VALUE_CASES))
def test_the_restatement_composes_with_the_distributional_and_quantile_restatements(cid):
    """tests.dist_np.DistDDPG / tests.quant_np.QuantDDPG on normalised networks: every network normalises, gamma and beta sit behind the
    N-wide q_value, the lists, slots and targets cover them, the critic's gamma gradient is the loss's finite difference, the float32
    twin stays inside the bounds the GPU test uses"""
    kind, _opt, nb, clip = L.VALUE_CASES[cid]
    specs, P, _ep, _idxs, batches, _seed, want, outs, twin = L.value_case(cid)
    N = (L.DIST if kind == "dist" else L.QUANT)[0]
    names = [n for n, _s in specs[1].layout()]
    assert names[-4:] == ["q_value/weights", "q_value/biases", "hidden1/LayerNorm/gamma", "hidden1/LayerNorm/beta"] and dict(specs[1].layout())["q_value/weights"] == (50, N)
    assert min(n for o in outs for n in (o["actor_norm"], o["critic_norm"])) > 1.2 * clip
    from tests import dist_np, quant_np
    Base, par = (dist_np.DistDDPG, L.DIST) if kind == "dist" else (quant_np.QuantDDPG, L.QUANT)

    def loss(p):
        r = L.with_feature_norm(Base)(specs[0], specs[1], P[0], p, par, np.float64)
        r.set_targets(P[2], P[3])
        assert type(r.critic) is L.LnNet and type(r.target_critic) is L.LnNet and type(r.target_actor) is L.LnNet
        return r.critic_gradients(batches[0])
    g = loss(P[1])["grads"]
    k = specs[1].num_plain()
    for i in (k + 3, k + 200 + 7, 5):      # a gamma, a beta, a conv1 weight
        hi, lo = P[1].astype(np.float64).copy(), P[1].astype(np.float64).copy()
        hi[i] += 1e-6
        lo[i] -= 1e-6
        fd = (float(loss(hi)["loss"]) - float(loss(lo)["loss"])) / 2e-6
        assert abs(fd - g[i]) <= 1e-6 * max(1.0, abs(g[i])), (i, fd, g[i])
    start = list(P) + [np.zeros_like(want[4]), np.zeros_like(want[5])]
    for w, tw, p, r in zip(want, twin, start, twin_rs(want, twin, start)):
        if np.linalg.norm(w - p) > 0:
            assert np.linalg.norm(tw - w) <= delta_bound(p, w - p, r, nb)
    assert np.abs(want[1][k:] - P[1][k:]).min() > 0 and np.abs(want[3][k:] - P[3][k:]).min() > 0 and np.abs(want[4][len(P[0]) + k:]).min() > 0


def test_the_restatement_composes_with_the_soft_actor_critic_restatement():
    """tests.sac_np.SacDDPG on normalised networks with a 2A-wide linear head: every network normalises, gamma and beta sit behind the
    head, the actor's gamma gradient is the finite difference of its objective sum_b (alpha logp - Q), the clip is engaged"""
    from tests import sac_np as S
    specs, P, _ep, _idxs, batches = L.sac_case()
    assert [n for n, _s in specs[0].layout()][-3:] == ["output_action/biases", "h0/LayerNorm/gamma", "h0/LayerNorm/beta"] and dict(specs[0].layout())["output_action/biases"] == (4,)
    rng = np.random.default_rng(0)
    e1, e2 = rng.normal(size=(L.WHOLE_B, 2)), rng.normal(size=(L.WHOLE_B, 2))
    want, out, ag, cg = L.run_sac(specs, P, batches[0], e1, e2)
    assert min(float(out["actor_norm"]), float(out["critic_norm"])) > 1.2 * L.SAC_CLIP
    k = specs[0].num_plain()
    assert np.abs(want[0][k:] - P[0][k:]).min() > 0 and np.abs(want[1][specs[1].num_plain():] - P[1][specs[1].num_plain():]).min() > 0

    def objective(p):
        r = L.with_feature_norm(S.SacDDPG)(specs[0], specs[1], p, P[1], np.float64, L.sac_hyper())
        assert type(r.actor) is L.LnNet and type(r.target_actor) is L.LnNet and type(r.critic) is L.LnNet
        a = r.actor_gradients(batches[0][0], e1)
        return float((a["alpha"] * np.asarray(a["logp"]).ravel() - a["q"].ravel()).sum()), a["grads"]
    g = objective(P[0])[1]
    for i in (k + 3, k + 65 + 7):
        hi, lo = P[0].astype(np.float64).copy(), P[0].astype(np.float64).copy()
        hi[i] += 1e-6
        lo[i] -= 1e-6
        fd = (objective(hi)[0] - objective(lo)[0]) / 2e-6
        assert abs(fd - g[i]) <= 1e-5 * max(1.0, abs(g[i])), (i, fd, g[i])


# ---- b. the kernel-edge cases: conditions, and the bars the float32 twin derives
@pytest.mark.parametrize("cid", [c[0] for c in L.EDGE_CASES])
def test_edge_cases_meet_their_conditions_and_derive_their_bars(cid):
    case = L.edge_case(cid)
    act = [c for c in L.EDGE_CASES if c[0] == cid][0][3]
    bars, q = L.edge_bars(case)
    assert L.conditions(q, act) is None
    print("%s (seed %d):" % (cid, case[-1]), "  ".join("%s/%s %.1e->%.1e" % (n, k, e, b) for (n, k), (e, b) in sorted(bars.items())))
    for (_net, _k), (e, bar) in bars.items():
        assert bar == (8.0 * e if 8.0 * e >= 0.25 * 1e-5 else 1e-5)      # the house rule, restated
        assert bar < 1e-3                                                 # (a twin that far off could not referee anything)


def test_a_dead_feature_layer_has_zero_variance_in_both_precisions():
    case = L.edge_case("w65-b5-relu", dead=True)
    q, _ag, _cg, q32, _a, _c = L.pinned_twin(case[0], case[1], case[4][0])
    for qq, dt in ((q, np.float64), (q32, np.float32)):
        for net in ("actor", "critic"):
            assert not qq[net]["xhat"].any() and not qq[net]["sd"].any()
            assert np.allclose(qq[net]["rstd"], 1.0 / np.sqrt(dt(L.EPS)), rtol=1e-6) and np.isfinite(qq[net]["dz"]).all()
            assert not qq[net]["dgamma"].any()
    beta = case[1][0][-65:]
    assert np.allclose(q["actor"]["y"], np.maximum(beta, 0)[None].repeat(5, 0))
    bars, _q = L.edge_bars(case)
    print("dead layer:", "  ".join("%s/%s %.1e->%.1e" % (n, k, e, b) for (n, k), (e, b) in sorted(bars.items())))


# ---- c. the whole-minibatch cases: clipped or not by a margin, routes kept by the float32 twin, the twin inside the bounds
@pytest.mark.parametrize("cid", list(L.WHOLE_CASES))
def test_whole_cases_meet_their_conditions_and_their_twin_stays_inside_the_bounds(cid):
    _hidden, act, nb, _opt, clip, _route = L.WHOLE_CASES[cid]
    specs, P, _ep, _idxs, batches, seed, want, outs, twin = L.whole_case(cid)
    norms = [n for o in outs for n in (o["actor_norm"], o["critic_norm"])]
    assert (min(norms) > 1.2 * clip) if clip < 1 else (1.2 * max(norms) < clip), (cid, norms)
    start = list(P) + [np.zeros_like(want[4]), np.zeros_like(want[5])]
    rs = twin_rs(want, twin, start)
    print("%s (seed %d): norms %s, r %s" % (cid, seed, [round(n, 2) for n in norms], ["%.1e" % r for r in rs]))
    for w, t, p, r in zip(want, twin, start, rs):
        if np.linalg.norm(w - p) > 0:
            assert np.linalg.norm(t - w) <= delta_bound(p, w - p, r, nb)


# ---- d. planted faults: each moves a compared quantity by more than 10 x its bar
def _edge_moves(case, fault):
    """the largest (error / bar) over the compared quantities of an edge case when `fault` is planted in the float64 evaluation"""
    bars, _q = L.edge_bars(case)
    q, _ag, _cg, qf, _a, _c = L.pinned_twin(case[0], case[1], case[4][0], fault=fault, dt=np.float64)
    return max(L.rel_err(qf[net][k], q[net][k]) / bars[(net, k)][1] for net in ("actor", "critic") for k in L.LN_QUANTITIES)


@pytest.mark.parametrize("fault", L.NET_FAULTS)
def test_a_planted_fault_in_the_layer_moves_a_compared_quantity(fault):
    moved = {}
    for cid, _w, _B, act in L.EDGE_CASES:
        if fault == "relu_mask_for_tanh" and act != "tanh":
            continue
        moved[cid] = _edge_moves(L.edge_case(cid), fault)
    print(fault, {k: "%.0f" % v for k, v in moved.items()})
    # where the variance is of the order of 1 an epsilon of 1e-5 on either side of the root is below the bars: the quiet case is there for it
    need = ["w64-b5-tanh-quiet"] if fault == "eps_outside_root" else list(moved)
    for cid in need:
        assert moved[cid] > 10.0, (fault, cid, moved[cid])


@pytest.mark.parametrize("fault", ["norm_vars_outside_clip_norm", "norm_vars_not_in_target_update"])
def test_a_planted_fault_above_the_networks_moves_a_vector(fault):
    cid = "default-sgd"                                   # clipped: both norms above 1.2 x the clip
    specs, P, _ep, _idxs, batches, _seed, want, _outs, twin = L.whole_case(cid)
    hp = L.whole_hyper(cid)
    ref = L.restatement(specs, P, np.float64, hp, fault=fault)
    for b in batches:
        ref.train_minibatch(b)
    ref.update_targets()
    got = [np.asarray(n.flat(), np.float64) for n in (ref.actor, ref.critic, ref.target_actor, ref.target_critic)]
    rs = twin_rs(want[:4], twin[:4], P)
    ratios = [float(np.linalg.norm(g - w)) / delta_bound(p, w - p, r, 1) for g, w, p, r in zip(got, want[:4], P, rs)]
    print(fault, ["%.1f" % x for x in ratios])
    assert max(ratios) > 10.0, (fault, ratios)
    # (and without a fault the plain restatement is tests.ddpg_opt_np's GradientDescent, bit for bit)
    ok = L.restatement(specs, P, np.float64, hp)
    for b in batches:
        ok.train_minibatch(b)
    ok.update_targets()
    assert all(np.array_equal(np.asarray(n.flat(), np.float64), w) for n, w in zip((ok.actor, ok.critic, ok.target_actor, ok.target_critic), want))


# ---- e. the command line
def test_flags_are_absent_unless_given_and_every_refusal_names_its_reason():
    from cartpoleplusplus_amd import ddpg_cartpole as D
    parser = D.build_parser()
    o = parser.parse_args([])
    assert not hasattr(o, "feature_layer_norm") and not hasattr(o, "feature_norm_activation")
    assert D.feature_layer_norm(o) is None and D.feature_layer_norm(D.default_opts()) is None
    o = parser.parse_args(["--feature-layer-norm", "--use-raw-pixels"])
    assert o.feature_layer_norm is True and not hasattr(o, "feature_norm_activation")
    assert D.feature_layer_norm(o) == ("tanh", 1e-5)
    o = parser.parse_args(["--feature-layer-norm", "--use-raw-pixels", "--feature-norm-activation", "relu"])
    assert D.feature_layer_norm(o) == ("relu", 1e-5)
    with pytest.raises(SystemExit):
        parser.parse_args(["--feature-layer-norm", "--feature-norm-activation", "gelu"])
    for argv, word in ((["--feature-norm-activation", "relu"], "needs --feature-layer-norm"),
                       (["--feature-layer-norm"], "low-dimensional"),
                       (["--feature-layer-norm", "--use-raw-pixels", "--use-batch-norm"], "--use-batch-norm"),
                       (["--feature-layer-norm", "--use-raw-pixels", "--use-dropout"], "--use-dropout")):
        with pytest.raises(SystemExit) as e:
            D.feature_layer_norm(parser.parse_args(argv))
        assert word in str(e.value), (argv, str(e.value))
    # it composes with the other learners' flags, and the NAF parser does not know it
    o = parser.parse_args(["--feature-layer-norm", "--use-raw-pixels", "--twin-q", "--n-step", "3", "--target-policy-noise", "0.2"])
    assert D.feature_layer_norm(o) == ("tanh", 1e-5) and D.twin_q(o) and D.n_step(o) == 3
    from cartpoleplusplus_amd import naf_cartpole as NAF
    naf_parser = NAF.build_parser() if hasattr(NAF, "build_parser") else None
    if naf_parser is not None:
        with pytest.raises(SystemExit):
            naf_parser.parse_args(["--feature-layer-norm"])
    assert isinstance(parser, argparse.ArgumentParser)
