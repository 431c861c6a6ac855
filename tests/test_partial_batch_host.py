"""What tests/test_gpu_partial_batch.py can see, established with the float64 oracle alone (no GPU).  An agent built for batches of
C rows runs a C-row minibatch and then a B-row one; a device that lets a quantity follow C where it should follow B computes the B-row
minibatch with one of the faults below.  Each is PLANTED IN THE ORACLE here (patches inside this file; oracle/ has no switch for any
of them), on tests.helpers.partial_case / naf_partial_case at (C, B) = (8, 5) -- the C-row minibatch, its update, then the B-row one --
and must move at least one quantity the GPU runners assert by at least 10x that quantity's bar.

Bars (the runners': tests.helpers.fused_step_against_f64_oracle, tests/test_gpu_naf.py naf_fused_step_against_f64_oracle): actions, dQ/da,
Q, TD 1e-5 absolute; the loss 1e-5 of max(1, |loss|); both pre-clip gradient lists per variable at rel 2e-5 (batch norm: 5e-5), a
variable counting as moved the way assert_flat_close counts it bad; the reported pre-clip norms at 1e-4 of max(1, norm).

Planted faults:
  stale_rows       (a) dW and db summed over the B rows plus rows B .. C-1 of the C-row minibatch before it: their layer inputs and
                       their dz (seeded with 1/C, at the parameters of that minibatch) are still in the workspace
  inv_capacity     (b) the loss and the dz seeds scaled by 1/C instead of 1/B
  bn_rows          (c) batch-norm moments over the B rows' conv outputs and the stale ones of rows B .. C-1
  norm_partials    (d) the squared norm summed over the partial slots of the C-row pass: the stale rows' partials are added
  whiten_count     (e) the whitening moments divided by the pixel count of C images
  mask_pitch       (f) the dropout keep bit of row b, unit u read at u * C + b of the mask buffer instead of b * units + u
"""
import contextlib

import numpy as np
import pytest

from oracle import ddpg_np as O
from oracle import naf_np as N
from tests.helpers import (PARTIAL_B, PARTIAL_C, PARTIAL_LOWDIM, PARTIAL_PIX, dropout_masks, naf_partial_case, oracle_minibatch, oracle_of,
                           partial_case)
from tests.test_batchnorm_sensitivity import grads_moved

C, B = PARTIAL_C, PARTIAL_B
ATOL, NORM_REL = 1e-5, 1e-4
FAULTS = ("stale_rows", "inv_capacity", "bn_rows", "norm_partials", "whiten_count", "mask_pitch")
ADAM = ("Adam", {"learning_rate": 0.01, "beta1": 0.8, "beta2": 0.9, "epsilon": 1e-3})
NAF_NAMESPACES = ("value", "target_value", "naf/output_action", "naf/l_values")


class CatSpec(object):
    """the layout of the NAF gradient list: value | mu | l (tests/test_gpu_naf.py)"""

    def __init__(self, specs):
        self.specs = specs

    def layout(self):
        out = []
        for tag, sp in zip(("value/", "mu/", "l/"), self.specs):
            out += [(tag + n, s) for n, s in sp.layout()]
        return out


class _Moments(object):
    """O.bn_stats and O.whiten_stats as the faults see them.  record: keep rows B .. C-1 of every conv output whose batch moments are
    taken, in call order; bn_rows: take the moments of call k over the rows given and the rows kept at k; whiten_count: divide the
    whitening sums by C / B times the pixel count."""

    def __init__(self):
        self.kept, self.mode, self.k = [], None, 0
        self.bn, self.white = O.bn_stats, O.whiten_stats

    def bn_stats(self, z, dt, training):
        if not training or self.mode not in ("record", "bn_rows"):
            return self.bn(z, dt, training)
        if self.mode == "record":
            self.kept.append(np.array(z[B:C]))
            return self.bn(z, dt, training)
        stale = self.kept[self.k]
        self.k += 1
        assert z.shape[0] == B and stale.shape[1:] == z.shape[1:]
        return self.bn(np.concatenate([z, stale]), dt, training)

    def whiten_stats(self, x, dt):
        if self.mode != "whiten_count":
            return self.white(x, dt)
        x64 = np.asarray(x, np.float64)
        flat = x64.reshape(-1, x64.shape[3])
        n = flat.shape[0] * C // B
        mean, sq = flat.sum(axis=0) / n, (flat * flat).sum(axis=0) / n
        inv = 1.0 / np.sqrt(sq - mean * mean + O.WHITEN_EPS)
        return inv.astype(dt), (-mean * inv).astype(dt)

    @contextlib.contextmanager
    def __call__(self, mode):
        self.mode, self.k = mode, 0
        O.bn_stats, O.whiten_stats = self.bn_stats, self.whiten_stats
        try:
            yield
        finally:
            O.bn_stats, O.whiten_stats = self.bn, self.white
            self.mode = None


def _masks(namespace, hidden, rows, step, fault):
    right = dropout_masks(namespace, hidden, rows, step)
    if fault != "mask_pitch":
        return right
    out = {}
    for name, units in zip(sorted(right), hidden):
        buf = right[name].reshape(-1)          # what the B-row forward wrote: row b, unit u at b * units + u
        b, u = np.meshgrid(np.arange(rows), np.arange(units), indexing="ij")
        out[name] = buf[(u * C + b) % buf.size]
    return out


def _rows_from(n):
    return (np.arange(C) >= n).astype(np.float64).reshape(C, 1)


# ---- DDPG -------------------------------------------------------------------------------------------------------------------------
def ddpg_checked_minibatch(case, fault, restate=True):
    """what the fused runner compares of the B-row minibatch behind the C-row one.  restate=False: the plain oracle calls the GPU
    runner makes, nothing of this file in between"""
    specs, P, _ep, _idxs, batches = case
    ref = oracle_of(specs, P, np.float64, O.DEFAULT_HYPER)
    hidden = specs[0].hidden
    big, small = batches[0], batches[1]

    def set_masks(rows, step, f):
        if specs[0].dropout:
            ref.actor.drop_masks = _masks("actor", hidden, rows, step, f)
            ref.target_actor.drop_masks = _masks("target_actor", hidden, rows, step, f)
    set_masks(C, 0, None)
    if not restate:
        oracle_minibatch(ref, big)
        ref.update_targets()
        set_masks(B, 1, None)
        ag, cg = ref.actor_gradients(small[0]), ref.critic_gradients(small)
        stale_a = stale_c = None
    else:
        moments = _Moments()
        with moments("record"):
            ag0, cg0 = ref.actor_gradients(big[0]), ref.critic_gradients(big)
        # the C-row pass's contribution of rows B .. C-1 to both lists: its own seeds (1 / C in the critic's), its own layer inputs
        stale_a = O.flatten(specs[0], ref.actor.backward(ag0["cache_actor"], -ag0["dq_da"] * _rows_from(B))[0], np.float64)
        stale_c = ref.critic_gradients(big, td_override=cg0["td"] * _rows_from(B))["grads"]
        oracle_minibatch(ref, big)
        ref.update_targets()
        set_masks(B, 1, fault)
        with moments(fault):
            ag, cg = ref.actor_gradients(small[0]), ref.critic_gradients(small)
    out = {"actions": ag["actions"], "dq_da": ag["dq_da"], "q": cg["q"], "td": cg["td"], "loss": float(cg["loss"]),
           "actor_grads": np.array(ag["grads"]), "critic_grads": np.array(cg["grads"])}
    if fault == "stale_rows":
        out["actor_grads"] += stale_a
        out["critic_grads"] += stale_c
    if fault == "inv_capacity":
        out["loss"] *= B / C
        out["critic_grads"] *= B / C
    out["actor_norm"], out["critic_norm"] = float(np.linalg.norm(out["actor_grads"])), float(np.linalg.norm(out["critic_grads"]))
    if fault == "norm_partials":
        out["actor_norm"] = float(np.sqrt(out["actor_norm"] ** 2 + np.linalg.norm(stale_a) ** 2))
        out["critic_norm"] = float(np.sqrt(out["critic_norm"] ** 2 + np.linalg.norm(stale_c) ** 2))
    return out


def ddpg_ratios(specs, right, wrong, grad_rel):
    out = {k: float(np.abs(wrong[k] - right[k]).max()) / ATOL for k in ("actions", "dq_da", "q", "td")}
    out["loss"] = abs(wrong["loss"] - right["loss"]) / (ATOL * max(1.0, abs(right["loss"])))
    out["actor_grads"] = grads_moved(specs[0], wrong["actor_grads"], right["actor_grads"], grad_rel)
    out["critic_grads"] = grads_moved(specs[1], wrong["critic_grads"], right["critic_grads"], grad_rel)
    for k in ("actor_norm", "critic_norm"):
        out[k] = abs(wrong[k] - right[k]) / (NORM_REL * max(1.0, right[k]))
    return out


# fault -> (shape, host_case's switches, the gradient lists' bar)
DDPG_CASES = {"stale_rows": (PARTIAL_PIX, {}, 2e-5), "inv_capacity": (PARTIAL_PIX, {}, 2e-5), "bn_rows": (PARTIAL_PIX, dict(batch_norm=True), 5e-5),
              "norm_partials": (PARTIAL_PIX, {}, 2e-5), "whiten_count": (PARTIAL_PIX, {}, 2e-5), "mask_pitch": (PARTIAL_PIX, dict(dropout=True), 2e-5)}


@pytest.mark.parametrize("fault", FAULTS)
def test_every_planted_fault_moves_a_ddpg_quantity_by_ten_times_its_bar(fault):
    shape, kw, grad_rel = DDPG_CASES[fault]
    case = partial_case(shape, C, B, **kw)
    right = ddpg_checked_minibatch(case, None)
    r = ddpg_ratios(case[0], right, ddpg_checked_minibatch(case, fault), grad_rel)
    print("DDPG %-14s largest %.3gx: " % (fault, max(r.values())) + "  ".join("%s %.3gx" % kv for kv in sorted(r.items())))
    assert max(r.values()) >= 10.0, (fault, r)
    if fault in ("stale_rows", "norm_partials", "inv_capacity"):          # (backward faults: the forward values stay)
        assert max(r[k] for k in ("actions", "dq_da", "q", "td")) == 0.0
    if fault == "norm_partials":
        assert r["actor_grads"] == r["critic_grads"] == 0.0 and min(r["actor_norm"], r["critic_norm"]) >= 10.0


def test_stale_rows_and_masks_show_in_a_low_dimensional_state_too():
    for fault, kw in (("stale_rows", {}), ("inv_capacity", {}), ("norm_partials", {}), ("mask_pitch", dict(dropout=True))):
        case = partial_case(PARTIAL_LOWDIM, C, B, **kw)
        r = ddpg_ratios(case[0], ddpg_checked_minibatch(case, None), ddpg_checked_minibatch(case, fault), 2e-5)
        print("DDPG low-dimensional %-14s largest %.3gx" % (fault, max(r.values())))
        assert max(r.values()) >= 10.0, (fault, r)


@pytest.mark.parametrize("kw", [{}, dict(batch_norm=True), dict(dropout=True)], ids=["plain", "batch-norm", "dropout"])
def test_the_unfaulted_ddpg_restatement_is_the_oracle(kw):
    """the clean oracle passes every bar by construction: with no fault the restatement above computes the plain oracle's numbers"""
    case = partial_case(PARTIAL_PIX, C, B, **kw)
    a, b = ddpg_checked_minibatch(case, None), ddpg_checked_minibatch(case, None, restate=False)
    for k in a:
        assert np.array_equal(a[k], b[k]), k


# ---- NAF --------------------------------------------------------------------------------------------------------------------------
def naf_checked_minibatch(case, share, fault, restate=True):
    specs, flats, _ep, _idxs, batches = case
    ref = N.NAF(specs[0], specs[1], specs[2], flats[0], flats[1], flats[2], share, 2, np.float64, gradient_clip=5.0, discount=0.99,
                target_update_rate=1e-4, optimiser=N.make_optimiser(*ADAM))
    ref.target_value = O.Net(specs[0], flats[3], np.float64)
    hidden = specs[0].hidden
    big, small = batches[0], batches[1]

    def set_masks(rows, step, f):
        if specs[0].dropout:
            nets = (ref.value, ref.target_value) + (() if share else (ref.mu, ref.l))
            for net, ns in zip(nets, NAF_NAMESPACES):
                net.drop_masks = _masks(ns, hidden, rows, step, f)
    moments = _Moments()
    stale = None
    set_masks(C, 0, None)
    if restate:
        with moments("record"):
            out0 = ref.forward_backward(big)
        # rows 0 .. B-1 given the reward at which their temporal difference is zero: what is left of the C-row pass's list is the
        # contribution of rows B .. C-1, seeded with 1 / C
        r0 = np.where(_rows_from(B) > 0, np.asarray(big[2], np.float64),
                      out0["q"] - np.asarray(big[3], np.float64) * ref.discount * out0["target_value"])
        only = ref.forward_backward((big[0], big[1], r0, big[3], big[4]))
        assert np.abs(only["td"][:B]).max() < 1e-12 and np.array_equal(only["td"][B:], out0["td"][B:])
        stale = only["grads"]
    ref.train(big)
    ref.update_targets()
    set_masks(B, 1, fault)
    with moments(fault if restate else None):
        out = ref.forward_backward(small)
    res = {"loss": float(out["loss"]), "grads": np.array(out["grads"])}
    if fault == "stale_rows":
        res["grads"] += stale
    if fault == "inv_capacity":
        res["loss"] *= B / C
        res["grads"] *= B / C
    res["norm"] = float(np.linalg.norm(res["grads"]))
    if fault == "norm_partials":
        res["norm"] = float(np.sqrt(res["norm"] ** 2 + np.linalg.norm(stale) ** 2))
    return res


def naf_ratios(specs, right, wrong, grad_rel):
    return {"loss": abs(wrong["loss"] - right["loss"]) / (ATOL * max(1.0, abs(right["loss"]))),
            "grads": grads_moved(CatSpec(specs), wrong["grads"], right["grads"], grad_rel),
            "norm": abs(wrong["norm"] - right["norm"]) / (NORM_REL * max(1.0, right["norm"]))}


NAF_FAULTS = FAULTS


@pytest.mark.parametrize("share", [True, False], ids=["shared-trunk", "own-trunks"])
@pytest.mark.parametrize("fault", NAF_FAULTS)
def test_every_planted_fault_moves_a_naf_quantity_by_ten_times_its_bar(fault, share):
    hidden = (100, 50) if share else (32, 16)
    case = naf_partial_case(PARTIAL_PIX, C, B, hidden=hidden, share=share, dropout=fault == "mask_pitch", batch_norm=fault == "bn_rows")
    assert case[0][0].batch_norm == (fault == "bn_rows")
    right = naf_checked_minibatch(case, share, None)
    r = naf_ratios(case[0], right, naf_checked_minibatch(case, share, fault), 5e-5 if fault == "bn_rows" else 2e-5)
    print("NAF share=%s %-14s largest %.3gx: " % (share, fault, max(r.values())) + "  ".join("%s %.3gx" % kv for kv in sorted(r.items())))
    assert max(r.values()) >= 10.0, (fault, r)


@pytest.mark.parametrize("kw", [dict(dropout=True), dict(batch_norm=True)], ids=["dropout", "batch-norm"])
@pytest.mark.parametrize("share", [True, False], ids=["shared-trunk", "own-trunks"])
def test_the_unfaulted_naf_restatement_is_the_oracle(share, kw):
    case = naf_partial_case(PARTIAL_PIX, C, B, hidden=(100, 50) if share else (32, 16), share=share, **kw)
    a, b = naf_checked_minibatch(case, share, None), naf_checked_minibatch(case, share, None, restate=False)
    for k in a:
        assert np.array_equal(a[k], b[k]), k



# ---- the variants' cases below the capacity: the conditions their own host tests place on a case's inputs, on the minibatches of the
# ---- capacity plans (C rows, B, B, C) as the float64 restatements walk them
def test_the_min_head_actors_plan_keeps_both_heads_in_play():
    from tests import actor_min_np as M
    from tests.test_gpu_actor_min import partial_plan
    case = M.case_of("A1-B5-sgd")
    inputs = M.case_inputs(case)
    ref = M.restatement(case, inputs[0], inputs[1])
    for rows, batch in partial_plan(case, inputs, C):
        ref.weights, ref.fed = None, batch[1]
        ref.train_minibatch(batch)
        ag = ref.last_ag
        ref.update_targets()
        assert float(np.abs(ag["q1"] - ag["q2"]).min()) >= M.TIE_MARGIN and M.MIN_SHARE <= float((ag["sel"] == 1).mean()) <= 1 - M.MIN_SHARE, len(rows)


def test_the_cloning_plan_stays_clear_of_the_floor():
    from tests import bc_np as Bc
    from tests.test_gpu_behaviour_cloning import partial_plan
    case = Bc.case_of("A1-B5-sgd")
    inputs = Bc.case_inputs(case)
    ref, floor = Bc.restatement(case, inputs[0], inputs[1]), Bc.floor_of(case)
    for rows, batch in partial_plan(case, inputs, C):
        ref.train_minibatch(batch)
        m = ref.last_ag["m"]
        ref.update_targets()
        assert abs(m - floor) >= Bc.FLOOR_GAP * floor and (m < floor or m >= Bc.M_MIN), (len(rows), m)


def test_the_shared_encoders_plan_stays_on_its_side_of_the_clip():
    from tests import shared_encoder_np as S
    from tests.test_gpu_shared_encoder import partial_plan
    cid = "8x8x6-A2-B5-sgd"
    case = S.case_of(cid)
    inputs = S.case_inputs(case)
    ref = S.restatement(inputs[0], inputs[1], np.float64, S.hyper_of(case), case[4])
    assert S.SIDES[cid] == "below"
    for rows, batch in partial_plan(case, inputs, C):
        out = ref.train_minibatch(batch, weights=None)
        ref.update_targets()
        assert min(out["actor_norm"], out["critic_norm"]) >= 1.2 * case[5], len(rows)


def test_the_layer_norm_edge_holds_its_conditions_on_the_wide_minibatch():
    from tests import layer_norm_np as L
    from tests.test_gpu_layer_norm import wide_edge_case
    wide, rows = wide_edge_case(L.edge_case("w65-b5-relu"), C)
    q, _ag, _cg = L.ln_quantities(L.restatement(wide[0], wide[1]), wide[4][0])
    assert len(rows) == C and L.conditions(q, "relu") is None


def test_the_smoothed_delayed_plan_is_decidable_in_float32():
    """tests/test_gpu_partial_batch.py's smoothing + delay case: no route of the four minibatches closer to a tie than float32 decides,
    the schedule held, applied, held, applied, and the float32 twin inside the bounds the device is held to"""
    from tests import ddpg_opt_np as R
    from tests import td3_np as T3
    from tests import tps_np as T
    case = partial_case(PARTIAL_PIX, C, B)
    specs, P, _ep, _idxs, batches = case
    for opt in ("gradient-descent", "adam"):
        hp = T3.hyper_of(opt, 0.5, 0.25)
        refs = [T3.restatement(specs, P, dt, hp, opt, 2, (T.SIGMA, T.CLIP, T.NOISE_SEED)) for dt in (np.float64, np.float32)]
        for b in batches:
            for ref in refs:
                out = ref.train_minibatch(b)
                ref.update_targets()
                assert out["tie"] > T3.TIE_FLOOR
        assert refs[0].schedule == [False, True, False, True]
        want, twin = R.vectors(refs[0]), R.vectors(refs[1])
        for name, w, t, bound in zip(T3.VECTORS, want, twin, T3.bounds(P, want, 4)):
            if np.any(w):
                assert float(np.linalg.norm(np.asarray(t, np.float64) - w)) <= bound, (opt, name)


def test_the_soft_actor_critic_plan_stays_on_its_side_of_the_clip():
    """tests.sac_np.C_PARTIAL_CASE over its four minibatches of C, B, B and C rows, the float64 restatement and its float32 twin fed the
    restated noise: both pre-clip norms on the registered side of the clip by 1.2 x, as tests/test_sac_host.py asks of C_CASES"""
    from tests import sac_np as S
    case = S.C_PARTIAL_CASE
    cid, A, clip = case[0], case[2], case[5]
    assert S.composed_case(cid) is case and case not in S.C_CASES
    inputs = S.composed_inputs(case)
    refs = [S.composed_restatement(case, inputs, dt) for dt in (np.float64, np.float32)]
    for k, rows in enumerate(S.partial_rows(case, inputs)):
        n = len(rows)
        batch = S.composed_batches(case[:3] + (n,) + case[4:], inputs[2], np.asarray(rows))[0]
        for ref in refs:
            out = ref.train_minibatch(batch, S.noise(S.C_NOISE_SEED, k, n, A, S.STREAM_S1), S.noise(S.C_NOISE_SEED, k, n, A, S.STREAM_S2),
                                      weights=None, routes=None)
            ref.update_targets()
            for norm, side in zip((float(out["actor_norm"]), float(out["critic_norm"])), S.C_SIDES[cid]):
                assert norm >= 1.2 * clip if side == "above" else norm <= clip / 1.2, (k, n, side, norm)
    assert [len(r) for r in S.partial_rows(case, inputs)] == [S.C_PARTIAL_CAPACITY, case[3], case[3], S.C_PARTIAL_CAPACITY]
