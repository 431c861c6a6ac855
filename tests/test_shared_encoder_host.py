"""The shared conv encoder on the host: tests/shared_encoder_np.py against torch autograd in float64, its float32 twin inside the bars of
tests/test_gpu_shared_encoder.py on that test's own cases, every planted fault outside them by more than ten times, and the option parser."""
import copy

import numpy as np
import pytest

from oracle import ddpg_np as O
from tests import shared_encoder_np as S

CASE_IDS = [c[0] for c in S.CASES]
_runs = {}


def _run(cid, dt=np.float64, fault=None):
    """NB minibatches of a case, each from the clean float64 run's state before it (what the GPU test does with the device's state):
    [(start, out, vectors)]"""
    key = (cid, np.dtype(dt).name, fault)
    if key in _runs:
        return _runs[key]
    case = S.case_of(cid)
    specs, P, _ep, _idxs, batches = S.case_inputs(case)
    ref = S.restatement(specs, P, dt, S.hyper_of(case), case[4], fault=fault)
    clean = _run(cid) if (fault is not None or dt is not np.float64) else None
    out = []
    start = S.initial_state(P)
    for k, b in enumerate(batches):
        if clean is not None:
            start = clean[k][0]
        if k > 0 or clean is not None:
            ref.set_state(start)
        o = ref.train_minibatch(b)
        ref.update_targets()
        vec = ref.vectors()
        out.append((start, o, vec))
        start = vec
    _runs[key] = out
    return out


def _specs(cid):
    return S.case_inputs(S.case_of(cid))[0]


# ---- 1. the restatement against torch autograd (float64, 8x8x6)
def test_the_restatement_against_torch_autograd():
    import torch
    from tests.test_oracle_vs_torch import torch_forward, tparams
    case = S.case_of("8x8x6-A2-B5-sgd")
    specs, P, _ep, _idxs, batches = S.case_inputs(case)
    aspec, cspec = specs
    ref = S.restatement(specs, P, np.float64, S.hyper_of(case)._replace(gradient_clip=None), case[4])
    s1, a, r, mask, s2 = batches[0]
    ag, cg = ref.actor_gradients(s1), ref.critic_gradients(batches[0])
    assert not [n for n, _s in aspec.layout() if n.startswith("conv")]
    assert len(ag["grads"]) == len(P[0]) == aspec.num_params()

    trunk, head = copy.copy(cspec), copy.copy(cspec)
    trunk.fc = []                                            # states -> flattened pool3
    head.pixel, low = False, O.NetSpec("actor", aspec.action_dim, aspec.hidden, pixel=False, state_elems=cspec.flat)
    t = lambda x: torch.tensor(np.asarray(x, np.float64))
    pa, pc = tparams(low, P[0]), tparams(cspec, P[1])
    pta, ptc = tparams(low, P[2]), tparams(cspec, P[3])
    conv_names = [n for n, _s in cspec.layout() if n.startswith("conv")]
    # the actor's objective: -sum_b Q(s1, mu(features.detach())) w.r.t. the actor's variables
    f1 = torch_forward(trunk, pc, t(s1))
    act = torch_forward(low, pa, f1.detach())
    q = torch_forward(head, pc, f1, action=act)
    np.testing.assert_allclose(act.detach().numpy(), ag["actions"], rtol=0, atol=1e-12)
    np.testing.assert_allclose(q.detach().numpy(), ag["q"], rtol=0, atol=1e-12)
    g_actor = torch.autograd.grad(-q.sum(), [pa[n] for n, _s in low.layout()], retain_graph=True)
    want = np.concatenate([g.numpy().ravel() for g in g_actor])
    assert np.abs(want - ag["grads"]).max() <= 1e-10 * max(1.0, np.abs(want).max())
    # ... nothing of the actor reaches a conv variable: d(actions)/d(conv) is identically zero under the stop gradient
    g_conv = torch.autograd.grad(act.sum(), [pc[n] for n in conv_names], allow_unused=True)
    assert all(g is None or not g.abs().max() for g in g_conv)
    # the critic's loss at the target actor's action on the TARGET critic's features
    f2 = torch_forward(trunk, ptc, t(s2))
    a2 = torch_forward(low, pta, f2)
    tq = torch_forward(head, ptc, f2, action=a2)
    np.testing.assert_allclose(a2.detach().numpy(), cg["target_actions"], rtol=0, atol=1e-12)
    y = (t(r) + t(mask) * ref.hp.discount * tq).detach()
    qb = torch_forward(cspec, pc, t(s1), action=t(a))
    loss = ((qb - y) ** 2).mean()
    g_critic = torch.autograd.grad(loss, [pc[n] for n, _s in cspec.layout()])
    want_c = np.concatenate([g.numpy().ravel() for g in g_critic])
    assert abs(float(loss.detach()) - cg["loss"]) <= 1e-12 * max(1.0, float(loss.detach()))
    assert np.abs(want_c - cg["grads"]).max() <= 1e-10 * max(1.0, np.abs(want_c).max())
    # ... which is the PLAIN critic's gradient at the same a': the encoder's gradient is the critic's loss gradient and nothing else
    plain = O.DDPG(O.NetSpec("actor", 2, list(aspec.hidden), pixel=True, H=cspec.H, W=cspec.W, C=cspec.C), cspec,
                   np.zeros(O.NetSpec("actor", 2, list(aspec.hidden), pixel=True, H=cspec.H, W=cspec.W, C=cspec.C).num_params()), P[1], np.float64, ref.hp)
    plain.set_targets(plain.actor.flat(), P[3])
    w2 = plain._white(plain.critic, s2)
    tqp = plain.target_critic.forward(s2, action=cg["target_actions"], white=w2)
    yp = np.asarray(r, np.float64) + np.asarray(mask, np.float64) * ref.hp.discount * tqp["out"]
    cb = plain.critic.forward(s1, action=np.asarray(a, np.float64))
    gp, _ = plain.critic.backward(cb, 2.0 * (cb["out"] - yp) / len(yp))
    np.testing.assert_array_equal(O.flatten(cspec, gp, np.float64), cg["grads"])
    # the withheld gradient is not small: a leak would show
    leak = S.encoder_leak(ag["cache_actor"])
    assert np.linalg.norm(leak) > 0.1 * np.linalg.norm(cg["grads"][:len(leak)])


# ---- 2. the float32 twin inside the bars, on the GPU test's cases
@pytest.mark.parametrize("cid", CASE_IDS)
def test_the_float32_twin_is_inside_the_bars(cid):
    specs = _specs(cid)
    clean, twin = _run(cid), _run(cid, np.float32)
    for k, ((start, want, want_vec), (_s, got, got_vec)) in enumerate(zip(clean, twin)):
        r = S.ratios(specs, start, got, got_vec, want, want_vec)
        # (the gradient lists: the GPU test's bar per variable is the larger of GRAD_REL and F32_GRAD_FACTOR x this twin's own distance)
        grads = {key: r.pop(key) for key in ("actor_grads", "critic_grads")}
        worst = max(r, key=lambda x: r[x])
        print("%s minibatch %d: float32 twin's worst %s at %.3f of its bar; gradient lists at %s of GRAD_REL" % (cid, k, worst, r[worst], grads))
        assert r[worst] <= 1.0, (cid, k, {a: b for a, b in r.items() if b > 1.0})
        assert got_vec["step"] == want_vec["step"]


@pytest.mark.parametrize("cid", CASE_IDS)
def test_the_clip_sits_where_the_case_says(cid):
    case = S.case_of(cid)
    clip = case[5]
    for _start, out, _vec in _run(cid):
        na, nc = out["actor_norm"], out["critic_norm"]
        side = S.SIDES[cid]
        if side == "below":      # the clip below both norms: both lists scaled
            assert min(na, nc) >= 1.2 * clip, (cid, na, nc, clip)
        elif side == "above":
            assert max(na, nc) <= clip / 1.2, (cid, na, nc, clip)
        else:                    # between: the critic's list scaled, the actor's (fully connected layers only) not
            assert na <= clip / 1.2 and nc >= 1.2 * clip, (cid, na, nc, clip)


# ---- 3. every planted fault leaves a bar by more than ten times, on each of the GPU test's cases
@pytest.mark.parametrize("fault", S.FAULTS)
@pytest.mark.parametrize("cid", CASE_IDS)
def test_every_planted_fault_leaves_a_bar_by_more_than_ten_times(cid, fault):
    specs = _specs(cid)
    clean, bad = _run(cid), _run(cid, fault=fault)
    worst = 0.0
    for (start, want, want_vec), (_s, got, got_vec) in zip(clean, bad):
        r = S.ratios(specs, start, got, got_vec, want, want_vec)
        key = max(r, key=lambda x: r[x])
        worst = max(worst, r[key])
    print("%s / %s: %.1f x a bar (%s)" % (cid, fault, worst, key))
    assert worst > 10.0, (cid, fault, worst)


# ---- 4. the option parser
def _parse(*argv):
    from cartpoleplusplus_amd import ddpg_cartpole as D
    return D, D.build_parser().parse_args(list(argv))


def test_the_options_are_absent_unless_given():
    D, o = _parse()
    for key in ("shared_encoder", "random_shift", "random_shift_seed"):
        assert not hasattr(o, key), key
    assert D.shared_encoder(o) is False and D.random_shift(o) == (0, 0)
    D, o = _parse("--use-raw-pixels", "--shared-encoder", "--random-shift", "4", "--random-shift-seed", "7")
    assert o.shared_encoder is True and D.shared_encoder(o) is True and D.random_shift(o) == (4, 7)
    d = D.default_opts()
    assert d.shared_encoder is False and D.shared_encoder(d) is False and D.random_shift(d) == (0, 0)


@pytest.mark.parametrize("argv,word", [(("--shared-encoder",), "--use-raw-pixels"),
                                       (("--shared-encoder", "--use-raw-pixels", "--use-batch-norm"), "--use-batch-norm"),
                                       (("--shared-encoder", "--use-raw-pixels", "--use-dropout"), "--use-dropout"),
                                       (("--random-shift", "4"), "--use-raw-pixels"),
                                       (("--use-raw-pixels", "--random-shift-seed", "3"), "--random-shift PAD"),
                                       (("--use-raw-pixels", "--random-shift", "-1"), ">= 0")])
def test_the_refusals_of_the_readers(argv, word):
    D, o = _parse(*argv)
    with pytest.raises(SystemExit) as e:
        D.shared_encoder(o)
        D.random_shift(o)
    assert word in str(e.value), str(e.value)


def test_the_naf_learner_does_not_know_the_option():
    from cartpoleplusplus_amd import naf_cartpole as NAF
    with pytest.raises(SystemExit):
        NAF.build_parser().parse_args(["--shared-encoder"])


# ---- 5. the compositions: the float32 twin inside the bars, either wrong encoder outside them by more than ten times
_comp_runs = {}


def _comp_run(name, dt=np.float64, fault=None):
    """S.NB minibatches of a composition, each from the clean float64 run's state before it: [(start, out, vectors)]"""
    key = (name, np.dtype(dt).name, fault)
    if key in _comp_runs:
        return _comp_runs[key]
    inputs = S.comp_inputs(name)
    _kind, _sn, A, B = S.COMPOSITIONS[name][:4]
    clean = None if (fault is None and dt is np.float64) else _comp_run(name)
    ref = S.comp_restatement(name, inputs, dt, fault)
    out, start = [], S.comp_initial_state(inputs)
    for k, b in enumerate(inputs["batches"]):
        if clean is not None:
            start = clean[k][0]
        S.comp_set_state(ref, name, inputs, start, k)
        o = S.comp_minibatch(ref, name, inputs, b, eps=S.comp_noise(name, k, B, A))
        vec = S.comp_vectors(ref, name, inputs)
        out.append((start, o, vec))
        start = vec
    _comp_runs[key] = out
    return out


@pytest.mark.parametrize("name", list(S.COMPOSITIONS))
def test_a_compositions_float32_twin_is_inside_the_bars(name):
    """(the host runs every composition on its one-step, unshifted minibatches: an n-step memory and the random shift change the data the
    GPU test feeds, not the arithmetic)"""
    layout = S.comp_inputs(name)["layout"]
    for k, ((start, want, want_vec), (_s, got, got_vec)) in enumerate(zip(_comp_run(name), _comp_run(name, np.float32))):
        r = S.ratios(layout, start, got, got_vec, want, want_vec)
        grads = {key: r.pop(key) for key in ("actor_grads", "critic_grads")}
        worst = max(r, key=lambda x: r[x])
        print("%s minibatch %d: float32 twin's worst %s at %.3f of its bar; gradient lists at %s of GRAD_REL" % (name, k, worst, r[worst], grads))
        assert r[worst] <= 1.0, (name, k, {a: b for a, b in r.items() if b > 1.0})
    if S.COMPOSITIONS[name][6] > 1:      # the delay: held, then applied
        assert [o["applied"] for _s, o, _v in _comp_run(name)] == [False, True]


@pytest.mark.parametrize("fault", S.FAULTS[1:3])
@pytest.mark.parametrize("name", list(S.COMPOSITIONS))
def test_in_a_composition_either_wrong_encoder_leaves_a_bar_by_more_than_ten_times(name, fault):
    layout = S.comp_inputs(name)["layout"]
    worst = 0.0
    for (start, want, want_vec), (_s, got, got_vec) in zip(_comp_run(name), _comp_run(name, fault=fault)):
        r = S.ratios(layout, start, got, got_vec, want, want_vec)
        worst = max(worst, max(r.values()))
    print("%s / %s: %.1f x a bar" % (name, fault, worst))
    assert worst > 10.0, (name, fault, worst)


def _sac_run(dt=np.float64, fault=None, nb=2):
    from tests import sac_np as SAC
    case, inputs = S.sac_inputs()
    A, B = case[2], case[3]
    ref, clean = S.sac_restatement(case, inputs, dt, fault), S.sac_restatement(case, inputs)
    out, start = [], SAC.initial_state(inputs)
    for k in range(nb):
        batch = SAC.composed_batches(case, inputs[2], inputs[3][k * B:(k + 1) * B])[0]
        e1, e2 = (SAC.noise(SAC.C_NOISE_SEED, k, B, A, s) for s in (SAC.STREAM_S1, SAC.STREAM_S2))
        res = []
        for r in (clean, ref):
            if k > 0:
                r.set_state(start)
            o = r.train_minibatch(batch, e1, e2)
            r.update_targets()
            res.append((o, r.vectors()))
        out.append((start, res[0], res[1]))
        start = res[0][1]
    return case, inputs, out


def test_soft_actor_critic_on_a_shared_encoder_twin_inside_the_bars_and_either_wrong_encoder_outside():
    from tests import sac_np as SAC
    case, inputs, out = _sac_run(np.float32)
    for k, (start, (want, want_vec), (got, got_vec)) in enumerate(out):
        r = SAC.ratios(case, inputs[0], start, got, got_vec, want, want_vec, got, got_vec)
        worst = max(r, key=lambda x: r[x])
        print("sac minibatch %d: float32 twin's worst %s at %.3f of its bar" % (k, worst, r[worst]))
        assert r[worst] <= 1.0, (k, {a: b for a, b in r.items() if b > 1.0})
    for fault in S.FAULTS[1:3]:
        case, inputs, out = _sac_run(fault=fault)
        worst = 0.0
        for start, (want, want_vec), (got, got_vec) in out:
            r = SAC.ratios(case, inputs[0], start, got, got_vec, want, want_vec, want, want_vec)
            worst = max(worst, max(r.values()))
        print("sac / %s: %.1f x a bar" % (fault, worst))
        assert worst > 10.0, (fault, worst)
