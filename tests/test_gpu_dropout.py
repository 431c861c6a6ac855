"""--use-dropout (base_network.py:69-70): slim.dropout (keep 0.5) after the ReLU of the actor's / NAF networks' hidden
layers.  TensorFlow's random bits cannot be reproduced; the device draws its keep bits from Philox4x32-10 keyed by
(network, layer, forward count), and the oracle is fed the same masks."""
import numpy as np
import pytest

from oracle import ddpg_np as O
from tests.helpers import (DROP_B, DROP_CALLS, DROP_LOWDIM, DROP_NAF_HIDDEN, DROP_NAF_OPTIMISER, DROP_NB, DROP_PIX, DROP_ROWS, DROP_SEED, LOUD,
                           NAF_HYPER, assert_flat_close, ddpg_dropout_calls, ddpg_dropout_case, delta_bound, dropout_masks,
                           fused_step_against_f64_oracle, hyper_options, make_pair, naf_dropout_calls, naf_dropout_case, naf_oracle, oracle_of,
                           twin_rs)

pytestmark = pytest.mark.gpu
VECTORS = ("actor", "critic", "target_actor", "target_critic")


class HB(object):
    def __init__(self, t):
        self.state_1, self.action, self.reward, self.terminal_mask, self.state_2 = t


@pytest.mark.parametrize("shape,B", [((2, 2, 7), 5), ((8, 8, 3, 1, 2), 4)], ids=["lowdim-28-B5", "8x8x6-B4"])
def test_dropout_training_and_inference(shape, B):
    pixel = len(shape) == 5
    agent, ref, (aspec, cspec) = make_pair(shape, B, pixel, use_dropout=True)
    rng = np.random.default_rng(21)
    t = O.synthetic_batch(rng, B, shape, 2, pixel)
    hidden = [100, 100, 50]
    try:
        # inference (action_given / check_loss): no dropout
        want = ref.actor.forward(t[0], training=False)["out"]
        assert np.abs(agent.actor.forward(t[0]) - want).max() < 1e-5
        loss, td, q = agent.critic.check_loss(HB(t))
        wl, wtd, wq = ref.check_loss(t)
        assert np.abs(q - wq).max() < 1e-5 and np.abs(td - wtd).max() < 1e-5
        # the train ops: forward count 0 of the actor (actor.train) and of the target actor (critic.train)
        ref.actor.drop_masks = dropout_masks("actor", hidden, B, 0)
        ag = ref.actor_gradients(t[0])
        pa, pc = agent.actor.get_params(), agent.critic.get_params()
        agent.actor.train(HB(t).state_1)
        assert_flat_close(aspec, agent.actor.get_grads(), ag["grads"], what="actor grads (dropout)")
        agent.actor.set_params(pa)
        ref.target_actor.drop_masks = dropout_masks("target_actor", hidden, B, 0)
        cg = ref.critic_gradients(t)
        agent.critic.train(HB(t))
        assert_flat_close(cspec, agent.critic.get_grads(), cg["grads"], what="critic grads (dropout in the target actor)")
        agent.critic.set_params(pc)
        # a second actor update draws new masks (forward count 1)
        ref.actor.drop_masks = dropout_masks("actor", hidden, B, 1)
        ag1 = ref.actor_gradients(t[0])
        agent.actor.train(HB(t).state_1)
        assert_flat_close(aspec, agent.actor.get_grads(), ag1["grads"], what="actor grads (dropout, second forward)")
        assert np.abs(ag1["grads"] - ag["grads"]).max() > 1e-6
    finally:
        agent.close()


def _print_bounds(what, names, got, want, start, rs, stores):
    bad = []
    for name, g, w, p, r, nb in zip(names, got, want, start, rs, stores):
        err, bound = float(np.linalg.norm(g.astype(np.float64) - w)), delta_bound(p, w - p, r, nb)
        print("  %s %-13s r %.2e  device %.2e of its delta  (|err| %.3e, bound %.3e)" % (what, name, r, err / np.linalg.norm(w - p), err, bound))
        if not err <= bound:
            bad.append((what, name, err, bound))
    return bad


@pytest.mark.parametrize("shape", [DROP_LOWDIM, DROP_PIX], ids=["lowdim", "16x16x6"])
def test_fused_train_step_with_dropout(shape):
    """cpp_ddpg_train_step on the caller's rows, two calls of three minibatches (tests.helpers.ddpg_dropout_case, LOUD): minibatch k of
    call c draws the masks of forward count 3 c + k in the actor and in the target actor; the targets are updated between the calls.
    Parameters and targets after each call as deltas (delta_bound, r from the float32 numpy twin with the same masks).  Between the
    calls the inference entry points run -- actor.forward, action_given, critic.check_loss: none of them drops a unit (the oracle's
    training=False forward on the device's own parameters, 1e-5) and none advances a counter (the second call must match counts 3..5;
    tests/test_dropout_sensitivity.py: a count one behind moves these vectors by far more than their bounds)."""
    pixel = len(shape) == 5
    B, nb = DROP_B, DROP_NB
    specs, P, episodes, idxs, batches = ddpg_dropout_case(shape)
    agent, _ref, (aspec, _cspec) = make_pair(shape, B, pixel, seed=DROP_SEED, replay_size=DROP_ROWS, perturb=False, use_dropout=True,
                                             **hyper_options(LOUD))
    got, stats = [], []
    try:
        assert list(aspec.hidden) == list(specs[0].hidden) and aspec.dropout
        for net, p in zip(agent.networks(), P):
            assert net.get_params().shape == p.shape
            net.set_params(p)
        for ep in episodes:
            agent.replay_memory.add_episode(*ep)
        for c in range(DROP_CALLS):
            agent.train_step(B, nb, idxs=idxs[c * nb * B:(c + 1) * nb * B])
            got.append([n.get_params() for n in agent.networks()])
            stats.append(agent.trainer.last_stats())
            if c == 0:      # inference between the training calls, against the oracle on the parameters the device holds now
                refi = oracle_of(specs, got[0], np.float64, LOUD)
                t = batches[1]
                want = refi.actor.forward(t[0], training=False)["out"]
                assert np.abs(agent.actor.forward(t[0]) - want).max() < 1e-5
                one = agent.actor.action_given(np.asarray(t[0][2], np.float32), add_noise=False)
                assert np.abs(one - refi.action_given(t[0][2])).max() < 1e-5
                loss, td, q = agent.critic.check_loss(HB(t))
                wl, wtd, wq = refi.check_loss(t)
                assert np.abs(q - wq).max() < 1e-5 and np.abs(td - wtd).max() < 1e-5 and abs(loss - wl) < 1e-5 * max(1.0, abs(wl))
                for net, p in zip(agent.networks(), got[0]):
                    assert np.array_equal(net.get_params(), p)
    finally:
        agent.close()
    r64 = ddpg_dropout_calls(specs, P, batches)
    r32 = ddpg_dropout_calls(specs, P, batches, dt=np.float32)
    bad = []
    for c in range(DROP_CALLS):
        want, outs = r64[c][0], r64[c][1]
        same = all(np.array_equal(x, y) for a, b in zip(outs, r32[c][1]) for x, y in zip(a["routes"], b["routes"]))
        assert same, "the float32 twin and the float64 oracle take different pool / ReLU routes: the comparison is void"
        na, nc = outs[-1]["actor_norm"], outs[-1]["critic_norm"]
        print("call %d: oracle norms %s, device's last (%.4f, %.4f)" % (c, [(round(o["actor_norm"], 3), round(o["critic_norm"], 3)) for o in outs],
                                                                       stats[c][1], stats[c][2]))
        assert abs(stats[c][1] - na) < 1e-4 * max(1.0, na) and abs(stats[c][2] - nc) < 1e-4 * max(1.0, nc), (stats[c], na, nc)
        stores = [nb * (c + 1)] * 2 + [c + 1] * 2
        bad += _print_bounds("call %d" % c, VECTORS, got[c], want, P, twin_rs(want, r32[c][0], P), stores)
    assert not bad, bad


@pytest.mark.parametrize("shape", [DROP_LOWDIM, DROP_PIX], ids=["lowdim", "16x16x6"])
@pytest.mark.parametrize("share", [True, False], ids=["shared-representation", "own-trunks"])
def test_naf_fused_train_step_with_dropout(shape, share):
    """the same for cpp_naf_train_step (tests.helpers.naf_dropout_case, NAF_HYPER, Momentum 0.5): the value and the target value
    network -- with trunks of their own also mu and l_values, four counters -- draw count 3 c + k; naf.forward, value_given,
    action_given and debug_values between the calls."""
    from tests.test_gpu_naf import make_naf, HB as NHB, params_of, ATOL
    B, nb = DROP_B, DROP_NB
    specs, flats, episodes, idxs, batches = naf_dropout_case(shape, share)
    oname, oargs = DROP_NAF_OPTIMISER
    agent, _ref, aspecs = make_naf(shape, B, share, oname, oargs, seed=11, replay_size=DROP_ROWS, clip=NAF_HYPER["clip"],
                                   discount=NAF_HYPER["discount"], target_update_rate=NAF_HYPER["target_update_rate"], use_dropout=True,
                                   hidden=DROP_NAF_HIDDEN[share])
    got, stats = [], []
    nets = lambda: (agent.value_net, agent.naf.mu_net, agent.naf.l_net, agent.target_value_net)
    try:
        assert all(list(x.hidden) == list(y.hidden) for x, y in zip(aspecs, specs))
        for net, p in zip(nets(), flats):
            assert net.get_params().shape == p.shape
            net.set_params(p)
        for ep in episodes:
            agent.replay_memory.add_episode(*ep)
        for c in range(DROP_CALLS):
            agent.train_step(B, nb, idxs=idxs[c * nb * B:(c + 1) * nb * B])
            got.append((params_of(agent), agent.target_value_net.get_params()))
            stats.append(agent.naf.last_stats())
            if c == 0:
                now = [n.get_params() for n in nets()]
                refi = naf_oracle(specs, now, share, np.float64)
                t = batches[1]
                out = refi.forward_backward(t, backward=False)
                assert np.abs(agent.naf.forward(t[0]) - out["mu"]).max() < ATOL
                assert np.abs(agent.value_net.value_given(t[0]) - out["value"]).max() < ATOL
                one = agent.naf.action_given(np.asarray(t[0][2], np.float32), add_noise=False)
                assert np.abs(one - refi.action_given(t[0][2])).max() < ATOL
                l_values, loss, v, a, vp = agent.naf.debug_values(NHB(t))
                adv = out["advantage"][:, 0]
                assert np.abs(l_values - out["l_values"]).max() < ATOL and np.abs(v - out["value"][:, 0]).max() < ATOL
                assert (np.abs(a - adv) <= ATOL * np.maximum(1.0, np.abs(adv))).all()
                assert np.abs(vp - out["target_value"][:, 0]).max() < ATOL and abs(loss - out["loss"]) < ATOL * max(1.0, abs(out["loss"]))
                for net, p in zip(nets(), now):
                    assert np.array_equal(net.get_params(), p)
    finally:
        agent.close()
    r64 = naf_dropout_calls(specs, flats, batches, share)
    r32 = naf_dropout_calls(specs, flats, batches, share, dt=np.float32)
    start = (np.concatenate(flats[:3]), flats[3])
    bad = []
    for c in range(DROP_CALLS):
        want, norms, routes = r64[c][0], r64[c][1], r64[c][2]
        assert all(np.array_equal(x, y) for x, y in zip(routes, r32[c][2])), "float32 twin and float64 oracle take different routes"
        print("call %d: oracle norms %s, device's last %.6g" % (c, norms, stats[c][1]))
        assert stats[c][2] == 0 and abs(stats[c][1] - norms[-1]) < 1e-4 * max(1.0, norms[-1]), (stats[c], norms)
        bad += _print_bounds("call %d" % c, ("params", "target"), got[c], want, start, twin_rs(want, r32[c][0], start), [nb * (c + 1), c + 1])
    assert not bad, bad


@pytest.mark.parametrize("share", [True, False], ids=["shared-representation", "own-trunks"])
def test_naf_with_dropout(share):
    """NAF: the value / target-value (and, with their own trunks, mu / l_values) hidden stacks drop out in the train op
    (naf_cartpole.py:271), not in the debug fetch (:282)."""
    from tests.test_gpu_naf import make_naf, HB as NHB, CatSpec, params_of, ATOL
    shape, B = (2, 2, 7), 6
    agent, ref, specs = make_naf(shape, B, share, use_dropout=True)
    rng = np.random.default_rng(8)
    t = O.synthetic_batch(rng, B, shape, 2, False)
    hidden = [100, 50]
    try:
        dbg = ref.forward_backward(t, backward=False)
        l_values, loss, v, a, vp = agent.naf.debug_values(NHB(t))
        assert np.abs(l_values - dbg["l_values"]).max() < ATOL and np.abs(v - dbg["value"][:, 0]).max() < ATOL
        ref.value.drop_masks = dropout_masks("value", hidden, B, 0)
        ref.target_value.drop_masks = dropout_masks("target_value", hidden, B, 0)
        if not share:
            ref.mu.drop_masks = dropout_masks("naf/output_action", hidden, B, 0)
            ref.l.drop_masks = dropout_masks("naf/l_values", hidden, B, 0)
        out = ref.forward_backward(t)
        got_loss = agent.naf.train(NHB(t))
        assert abs(got_loss - out["loss"]) < ATOL * max(1.0, abs(out["loss"]))
        assert_flat_close(CatSpec(specs), agent.naf.get_grads(), out["grads"], what="naf grads (dropout)")
    finally:
        agent.close()


# ---- one minibatch of the fused step -- with graph=True its hipGraph replay, on rows the device drew -- against the float64 oracle at
# ---- the helpers' ordinary bars, the oracle drawing the masks of the count the device is at (the probe and the capture pass are
# ---- training-mode forwards).  16x16x6 renders, 300 rows; every case asserts the head path its probe saw.
PIX, ROWS = DROP_PIX, 300
DEFAULT_ACTOR = [100, 100, 50]
DDPG_REPLAYED = [
    # --use-dropout keeps the actor's last hidden layer out of the heads kernel ('heads', not 'heads+pre'): its masks come from the
    # GEMM epilogue, its backward from heads_body.h's relu_x2.  graph=True: the checked minibatch is forward count 2
    pytest.param(DEFAULT_ACTOR, 2, 16, True, "heads", id="defaults-B16-replay"),
    pytest.param(DEFAULT_ACTOR, 2, 1, False, "heads", id="B1-idle-lanes"),
    pytest.param(DEFAULT_ACTOR, 2, 5, True, "heads", id="B5-idle-lanes-replay"),
    pytest.param(DEFAULT_ACTOR, 2, 17, True, "heads", id="B17-second-M-tile-replay"),
    pytest.param([100, 100, 65], 2, 16, True, "gemm", id="100-100-65-gemm-x2-epilogue-replay"),
    pytest.param(DEFAULT_ACTOR, 9, 16, False, "gemm", id="A9-gemm-x2-epilogue"),
    pytest.param([400, 300], 2, 17, True, "gemm", id="400-300-B17-replay"),
]


def _print_report(what, rep):
    print(what, {k: v for k, v in sorted(rep.items()) if k.startswith(("err_", "rel_", "path", "f32_"))})


@pytest.mark.parametrize("actor_hidden,A,B,graph,path", DDPG_REPLAYED)
def test_ddpg_minibatch_with_dropout_against_f64_oracle(actor_hidden, A, B, graph, path):
    rep = fused_step_against_f64_oracle(PIX, B, ROWS, graph=graph, probe=True, use_dropout=True, actor_hidden=actor_hidden, action_dim=A)
    _print_report("DDPG dropout actor %s A=%d B=%d graph=%s:" % (actor_hidden, A, B, graph), rep)
    assert rep["path"] == path, (rep["path"], path)


def test_ddpg_lowdim_replayed_minibatch_with_dropout_against_f64_oracle():
    rep = fused_step_against_f64_oracle(DROP_LOWDIM, 16, ROWS, graph=True, probe=True, pixel=False, use_dropout=True)
    _print_report("DDPG dropout low-dimensional B=16 replay:", rep)
    assert rep["path"] == "gemm"


ADAM = ("Adam", {"learning_rate": 0.01, "beta1": 0.8, "beta2": 0.9, "epsilon": 1e-3})        # tests.helpers.NAF_OPTIMISERS' "adam-third-step"
NAF_REPLAYED = [
    # naf_mlp_kernel knows no masks: at the reference's widths the step must leave it for naf_heads_kernel (its x2 d(representation))
    pytest.param(True, [100, 50], 2, 16, "heads", {}, id="shared-100-50-not-mlp"),
    pytest.param(True, [100, 100, 50], 2, 17, "heads", {}, id="shared-100-100-50-B17"),
    pytest.param(True, [100, 64], 2, 16, "gemm", {}, id="shared-100-64-gemm"),
    pytest.param(True, [100, 50], 5, 16, "gemm", {}, id="shared-A5-gemm"),
    pytest.param(False, [32, 16], 2, 16, "gemm", {}, id="own-trunks-four-counters"),
    pytest.param(True, [100, 50], 2, 16, "heads", dict(optimiser=ADAM[0], optimiser_args=ADAM[1], warm_steps=2), id="shared-adam-count-3"),
]


@pytest.mark.parametrize("share,hidden,A,B,path,kw", NAF_REPLAYED)
def test_naf_replayed_minibatch_with_dropout_against_f64_oracle(share, hidden, A, B, path, kw):
    from tests.test_gpu_naf import naf_fused_step_against_f64_oracle
    report = {}
    got = naf_fused_step_against_f64_oracle(PIX, B, share, rows=ROWS, probe=True, use_dropout=True, hidden=hidden, action_dim=A,
                                            report=report, **kw)
    print("NAF dropout share=%s hidden %s A=%d B=%d: path %s, delta error %.2e (params) %.2e (target)" % (
        share, hidden, A, B, got, report["rel_delta_params"], report["rel_delta_target"]))
    assert got == path, (got, path)


def test_batch_norm_and_dropout_replayed_at_B17():
    """nets_forward_trunk_bn in front of the dropout stack, the first row of a second M-tile (the gradient list at batch norm's 5e-5)"""
    from tests.test_gpu_batchnorm_training import _fused
    rep = _fused(PIX, 17, ROWS, graph=True, probe=True, use_dropout=True)
    _print_report("DDPG batch norm + dropout B=17 replay:", rep)
    assert rep["path"] == "heads", rep["path"]
