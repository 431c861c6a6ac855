"""What tests/test_gpu_dropout.py's multi-call tests can see, established with the float64 oracle alone (no GPU): every fault below is
PLANTED IN THE ORACLE (other masks handed to it, or a subclass of oracle.ddpg_np.Net that edits the forward cache; oracle/ has no switch
for any of them) and must move at least one of the quantities the GPU tests compare by at least 10x the tolerance they apply to it, on
those tests' own inputs (tests.helpers.ddpg_dropout_case / naf_dropout_case: two calls of three minibatches at B = 6, DDPG at LOUD, NAF
at NAF_HYPER under Momentum 0.5; a 16x16x6 render and the low-dimensional state; NAF with a shared trunk and with trunks of their own).

Tolerances (the GPU tests'): after each call every parameter vector at delta_bound(theta, delta_f64, r, stores) -- r from the float32
numpy twin drawing the same masks, stores = minibatches so far (the targets: calls so far); the pre-clip norms the device reports for a
call's last minibatch at 1e-4 relative; the inference outputs between the calls (actions, Q, TD; mu, V, l_values) at 1e-5.

Planted faults:
  stale_count        the masks of count k - 1 re-used at k >= 1 (a counter not advanced, a replay holding its capture's count, an
                     inference call in between that advanced nothing but was believed to)
  transposed_index   element index unit * B + row instead of row * units + unit
  next_layer_stream  layer l draws layer l + 1's stream
  target_draws_online  the target network (target actor / target value network) draws the online network's masks
  backward_no_x2     the backward pass through a dropout layer without the factor 1 / keep_prob = 2
  backward_pre_gate  the backward pass gated on the activation in front of the mask: active-but-dropped units pass gradient
  inference_drops    the inference forward (IS_TRAINING False) drops units
  held_not_counted   --policy-delay 2: a minibatch whose actor update is held does not advance the actor's count (tests/test_gpu_policy_delay.py's
                     case of four minibatches, at tests/ddpg_opt_np.py's bounds)

Seen where: the first six through the parameter vectors and norms of the training calls; inference_drops through the inference
outputs only -- by construction it leaves every training call alone (ratio 0 there).  stale_count leaves minibatch 0 of call 0 alone by
construction (there is no count -1) and is found from minibatch 1 on.  Nothing else is excused.

The vectorised mask generator of tests.helpers is held to the scalar Philox4x32-10 statement of record bit for bit at the end."""
import zlib

import numpy as np
import pytest

from oracle import ddpg_np as O
from tests.helpers import (DROP_B, DROP_CALLS, DROP_LOWDIM, DROP_NB, DROP_PIX, LOUD, ddpg_dropout_calls, ddpg_dropout_case, delta_bound,
                           dropout_masks, naf_dropout_calls, naf_dropout_case, naf_oracle, oracle_of, philox4x32_10, philox4x32_10_np, twin_rs)

ATOL, NORM_REL = 1e-5, 1e-4
MASK_FAULTS = ("stale_count", "transposed_index", "next_layer_stream", "target_draws_online")
NET_FAULTS = ("backward_no_x2", "backward_pre_gate")
TARGET_OF = {"target_actor": "actor", "target_value": "value"}


def _masks_by(namespace, hidden, B, step, layer_shift=0, transposed=False):
    """dropout_masks with the element index or the layer word changed"""
    seed = zlib.crc32(namespace.encode()) & 0xffffffff
    out = {}
    for layer, units in enumerate(hidden):
        rows, cols = np.meshgrid(np.arange(B, dtype=np.uint64), np.arange(units, dtype=np.uint64), indexing="ij")
        idx = (cols * np.uint64(B) + rows) if transposed else (rows * np.uint64(units) + cols)
        w0 = philox4x32_10_np(idx, np.full_like(idx, layer + layer_shift), np.full_like(idx, step & 0xFFFFFFFF), np.full_like(idx, step >> 32), seed, 0)[0]
        out["h%d" % layer] = (w0 & np.uint64(1)).astype(np.float64)
    return out


def faulty_masks(fault):
    if fault == "stale_count":
        return lambda ns, hidden, B, step: dropout_masks(ns, hidden, B, max(step - 1, 0))
    if fault == "transposed_index":
        return lambda ns, hidden, B, step: _masks_by(ns, hidden, B, step, transposed=True)
    if fault == "next_layer_stream":
        return lambda ns, hidden, B, step: _masks_by(ns, hidden, B, step, layer_shift=1)
    if fault == "target_draws_online":
        return lambda ns, hidden, B, step: dropout_masks(TARGET_OF.get(ns, ns), hidden, B, step)
    return dropout_masks


class FaultyNet(O.Net):
    """oracle.ddpg_np.Net with a backward fault planted through the forward cache the backward pass reads (fault=None: the oracle)"""

    def __init__(self, net, fault=None):
        super(FaultyNet, self).__init__(net.spec, net.flat(), net.dt)
        self.fault, self.drop_masks = fault, net.drop_masks

    def forward(self, state, action=None, white=None, training=True):
        c = super(FaultyNet, self).forward(state, action=action, white=white, training=training)
        dropped = c.get("dropped", set())
        if self.fault == "backward_pre_gate":        # the gate sees relu(z), not relu(z) * mask * 2
            for i, ((name, _i, _o, act, _cat), (h, y)) in enumerate(zip(self.spec.fc, c["fc"])):
                if name in dropped:
                    c["fc"][i] = (h, O._act(h @ self.p[name + "/weights"] + self.p[name + "/biases"], act))
        if self.fault == "backward_no_x2":
            c["dropped"] = set()
        return c


def _wrap_ddpg(fault):
    def wrap(ref):
        ref.actor, ref.target_actor = FaultyNet(ref.actor, fault), FaultyNet(ref.target_actor, fault)
    return wrap


def _wrap_naf(fault):
    def wrap(ref):
        for k in ("value", "target_value", "mu", "l"):
            setattr(ref, k, FaultyNet(getattr(ref, k), fault))
    return wrap


def _planted(fault, wrap_of):
    kw = {}
    if fault in MASK_FAULTS:
        kw["masks"] = faulty_masks(fault)
    if fault in NET_FAULTS or fault == "restated":
        kw["wrap"] = wrap_of(None if fault == "restated" else fault)
    return kw


def _ddpg_ratios(right, twin, wrong, P):
    """the largest (|wrong - right| / the GPU test's tolerance) over the calls: parameter vectors, reported norms"""
    worst = 0.0
    for c in range(DROP_CALLS):
        want = right[c][0]
        rs = twin_rs(want, twin[c][0], P)
        stores = [DROP_NB * (c + 1)] * 2 + [c + 1] * 2
        for w, g, p, r, nb in zip(want, wrong[c][0], P, rs, stores):
            worst = max(worst, float(np.linalg.norm(g - w)) / delta_bound(p, w - p, r, nb))
        for k in ("actor_norm", "critic_norm"):
            n, m = right[c][1][-1][k], wrong[c][1][-1][k]
            worst = max(worst, abs(m - n) / (NORM_REL * max(1.0, n)))
    return worst


@pytest.mark.parametrize("shape", [DROP_LOWDIM, DROP_PIX], ids=["lowdim", "16x16x6"])
def test_every_planted_fault_moves_the_ddpg_calls_by_ten_times_their_tolerance(shape):
    specs, P, _ep, _idxs, batches = ddpg_dropout_case(shape)
    assert specs[0].dropout and not specs[1].dropout
    right = ddpg_dropout_calls(specs, P, batches)
    twin = ddpg_dropout_calls(specs, P, batches, dt=np.float32)
    assert all(np.isfinite(v).all() for c in right for v in c[0])
    Pd = [np.asarray(p, np.float64) for p in P]
    for fault in MASK_FAULTS + NET_FAULTS:
        ratio = _ddpg_ratios(right, twin, ddpg_dropout_calls(specs, P, batches, **_planted(fault, _wrap_ddpg)), Pd)
        print("DDPG %s %-20s %.3gx" % (shape, fault, ratio))
        assert ratio >= 10.0, (fault, ratio)
    # the restatement with no fault is the oracle: the faults are measured from the right place
    same = ddpg_dropout_calls(specs, P, batches, **_planted("restated", _wrap_ddpg))
    for c in range(DROP_CALLS):
        for a, b in zip(right[c][0], same[c][0]):
            assert np.array_equal(a, b)
    # stale_count leaves the first minibatch alone and shows in the second
    one = ddpg_dropout_calls(specs, P, batches[:1], nb=1)
    stale = ddpg_dropout_calls(specs, P, batches[:1], nb=1, masks=faulty_masks("stale_count"))
    assert all(np.array_equal(a, b) for a, b in zip(one[0][0], stale[0][0]))
    # inference between the calls: a forward that drops units leaves the outputs the GPU test holds to 1e-5
    ref = right[0][2]
    t = batches[1]
    clean = ref.actor.forward(t[0], training=False)["out"]
    ref.actor.drop_masks = dropout_masks("actor", specs[0].hidden, DROP_B, DROP_NB)
    ref.target_actor.drop_masks = dropout_masks("target_actor", specs[0].hidden, DROP_B, DROP_NB)
    moved = float(np.abs(ref.actor.forward(t[0], training=True)["out"] - clean).max()) / ATOL
    _l, td0, _q = ref.check_loss(t)
    moved_td = float(np.abs(ref.critic_gradients(t, training=True)["td"] - td0).max()) / ATOL
    print("DDPG %s inference_drops: actions %.3gx, TD %.3gx" % (shape, moved, moved_td))
    assert moved >= 10.0 and moved_td >= 10.0


def test_held_minibatches_left_uncounted_show_in_the_policy_delay_case():
    from tests import ddpg_opt_np as R
    from tests import td3_np as T3
    from tests.helpers import DROP_ROWS, DROP_SEED, host_case

    class SkipsHeld(T3.DelayedDDPG):
        def _draw_masks(self, B, *which):
            super(SkipsHeld, self)._draw_masks(B, *which)
            if "actor" in which and not self._applies(self.n + 1):
                self.drop_n["actor"] -= 1
    opt, d, nb = "gradient-descent", 2, 4
    specs, P, _ep, _idxs, batches = host_case(DROP_PIX, DROP_B, nb, DROP_SEED, rows=DROP_ROWS, dropout=True)
    want, _c, outs, ref = T3.run_case(specs, P, batches, LOUD, opt, d, nb, 1)
    assert [o["applied"] for o in outs] == [False, True, False, True] and min(o["tie"] for o in outs) > T3.TIE_FLOOR
    name, args = T3.OPTIMISERS[opt]
    bad = SkipsHeld(specs[0], specs[1], P[0], P[1], np.float64, LOUD, name, args, d)
    bad.set_targets(P[2], P[3])
    for b in batches:
        bad.train_minibatch(b)
    bad.update_targets()
    assert bad.drop_n == {"actor": 2, "target_actor": 4}
    moved = [float(np.linalg.norm(g - w)) / b for g, w, b in zip(R.vectors(bad)[:4], want[:4], T3.bounds(P, want, nb)[:4])]
    print("held_not_counted: %s x the bounds" % ["%.3g" % m for m in moved])
    assert max(moved) >= 10.0, moved


def _naf_ratios(right, twin, wrong, start):
    worst = 0.0
    for c in range(DROP_CALLS):
        want = right[c][0]
        rs = twin_rs(want, twin[c][0], start)
        for w, g, p, r, nb in zip(want, wrong[c][0], start, rs, (DROP_NB * (c + 1), c + 1)):
            worst = max(worst, float(np.linalg.norm(g - w)) / delta_bound(p, w - p, r, nb))
        n, m = right[c][1][-1], wrong[c][1][-1]
        worst = max(worst, abs(m - n) / (NORM_REL * max(1.0, n)))
    return worst


@pytest.mark.parametrize("shape", [DROP_LOWDIM, DROP_PIX], ids=["lowdim", "16x16x6"])
@pytest.mark.parametrize("share", [True, False], ids=["shared-representation", "own-trunks"])
def test_every_planted_fault_moves_the_naf_calls_by_ten_times_their_tolerance(shape, share):
    specs, flats, _ep, _idxs, batches = naf_dropout_case(shape, share)
    assert specs[0].dropout and specs[1].dropout == (not share)
    right = naf_dropout_calls(specs, flats, batches, share)
    twin = naf_dropout_calls(specs, flats, batches, share, dt=np.float32)
    start = (np.concatenate(flats[:3]).astype(np.float64), np.asarray(flats[3], np.float64))
    assert all(np.isfinite(v).all() for c in right for v in c[0])
    for fault in MASK_FAULTS + NET_FAULTS:
        ratio = _naf_ratios(right, twin, naf_dropout_calls(specs, flats, batches, share, **_planted(fault, _wrap_naf)), start)
        print("NAF %s share=%s %-20s %.3gx" % (shape, share, fault, ratio))
        assert ratio >= 10.0, (fault, ratio)
    same = naf_dropout_calls(specs, flats, batches, share, **_planted("restated", _wrap_naf))
    for c in range(DROP_CALLS):
        for a, b in zip(right[c][0], same[c][0]):
            assert np.array_equal(a, b)
    ref = right[0][3]
    t = batches[1]
    clean = ref.forward_backward(t, backward=False)
    nets = (ref.value, ref.target_value) + (() if share else (ref.mu, ref.l))
    for net, ns in zip(nets, ("value", "target_value", "naf/output_action", "naf/l_values")):
        net.drop_masks = dropout_masks(ns, specs[0].hidden, DROP_B, DROP_NB)
    cv, cm, cl = ref._forward(t[0], training=True)
    moved = {"value": float(np.abs(cv["out"] - clean["value"]).max()) / ATOL, "mu": float(np.abs(cm["out"] - clean["mu"]).max()) / ATOL,
             "l_values": float(np.abs(cl["out"] - clean["l_values"]).max()) / ATOL}
    print("NAF %s share=%s inference_drops:" % (shape, share), {k: "%.3gx" % v for k, v in moved.items()})
    assert min(moved.values()) >= 10.0, moved


@pytest.mark.parametrize("namespace,hidden,B,step", [("actor", [100, 100, 50], 5, 0), ("target_actor", [7], 3, 1), ("value", [400, 300], 17, 2 ** 32),
                                                     ("naf/l_values", [4000, 3], 17, 2 ** 32 + 5), ("target_value", [1, 2], 1, 2 ** 40 + 3)],
                         ids=["actor-defaults", "one-layer", "paper-widths-high-word", "B-x-units-past-2^16", "high-word-tiny"])
def test_the_vectorised_masks_are_the_scalar_philox_bit_for_bit(namespace, hidden, B, step):
    got = dropout_masks(namespace, hidden, B, step)
    seed = zlib.crc32(namespace.encode()) & 0xffffffff
    assert sorted(got) == ["h%d" % i for i in range(len(hidden))]
    for layer, units in enumerate(hidden):
        want = np.array([[philox4x32_10([b * units + j, layer, step & 0xFFFFFFFF, step >> 32], [seed, 0])[0] & 1 for j in range(units)]
                         for b in range(B)], np.float64)
        m = got["h%d" % layer]
        assert m.shape == (B, units) and m.dtype == np.float64 and np.array_equal(m, want)
    big = [k for k in got if got[k].size >= 64]
    if step >= 2 ** 32 and big:      # the counter's high word is part of the draw
        low = dropout_masks(namespace, hidden, B, step & 0xFFFFFFFF)
        assert all(not np.array_equal(low[k], got[k]) for k in big)
