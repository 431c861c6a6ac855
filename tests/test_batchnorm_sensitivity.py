"""What tests/test_gpu_batchnorm_training.py can see, established with the float64 oracle alone (no GPU): every fault below is PLANTED
IN THE ORACLE (a subclass of oracle.ddpg_np.Net / a patch of bn_stats inside the test; oracle/ has no switch for any of them) and must
move at least one of the vectors the GPU module compares by at least 10x the tolerance it applies to that vector, on that module's own
inputs (tests.helpers.host_case with batch_norm=True: the B = 1 case, the 64x64x6 case at B = 7, the prioritized-replay case's shape,
batch and row count -- the device draws that case's rows by priority, here they are host_case's with weights from lognormal(0, 2)
priorities as in the GPU helper -- and the 16x16x6 case of the hyperparameter group at LOUD).

Tolerances (the GPU module's): actions, Q, TD, dQ/da 1e-5 absolute; both pre-clip gradient lists per variable at rel 5e-5 (a variable
counts as moved the way assert_flat_close counts it bad: relative L2 error AND largest absolute error over rel x the list's RMS); the
reported pre-clip norms at 1e-4 relative; after three minibatches each of the four parameter vectors at
2^-23 * nb * |theta| + r * |delta_f64| with r from the float32 numpy twin (tests.helpers.f32_twin_case).

Planted faults:
  targets_moving_stats   the target networks normalise with the moving statistics (mean 0, variance 1) instead of the batch moments
  no_mean_dy             dz = inv * (dy - zhat * mean(dy * zhat)): the mean(dy) term dropped
  no_zhat_term           dz = inv * (dy - mean(dy)): the zhat * mean(dy * zhat) term dropped
  pooled_count           both means divided by the pooled count B (H/2) (W/2) instead of B H W
  first_image_stats      forward statistics taken over the first image only
  dbeta_out_of_clip      the BatchNorm/beta gradients left out of the clip norm (LOUD: both lists clipped)
  per_after_reductions   prioritized replay: the BN backward reductions (dbeta, mean(dy), mean(dy * zhat)) taken over the UNWEIGHTED
                         gradient, the importance weights applied to dz afterwards

NOT SEEN by construction: first_image_stats at B = 1 (the first image is the batch); the B = 7 case and the PER case see it."""
import contextlib

import numpy as np
import pytest

from oracle import ddpg_np as O
from tests.helpers import (BN_B1_CASE, BN_B7_CASE, BN_HYPER_CASES, BN_PER_CASE, LOUD, delta_bound, f32_twin_case, four_vectors, host_case,
                           oracle_of, oracle_train_step, per_var_report)

ATOL, GRAD_REL, NORM_REL = 1e-5, 5e-5, 1e-4
BACKWARD_FAULTS = ("no_mean_dy", "no_zhat_term", "pooled_count")
FAULTS = ("targets_moving_stats",) + BACKWARD_FAULTS + ("first_image_stats",)


class FaultyNet(O.Net):
    """oracle.ddpg_np.Net with one fault planted (fault=None: the oracle itself, test_the_unfaulted_restatement_is_the_oracle)"""

    def __init__(self, net, fault=None, inference=False, sample_w=None):
        super(FaultyNet, self).__init__(net.spec, net.flat(), net.dt)
        self.fault, self.inference, self.sample_w = fault, inference, sample_w

    def forward(self, state, action=None, white=None, training=True):
        return super(FaultyNet, self).forward(state, action=action, white=white, training=training and not self.inference)

    def backward_trunk(self, c, dp):
        sp, dt, fault = self.spec, self.dt, self.fault
        assert sp.batch_norm
        g = {}
        for idx in range(len(O.CONV_DEFS) - 1, -1, -1):
            name = O.CONV_DEFS[idx][0]
            x, pooled, amax, h, w = c[name]
            dz = O.relu_pool_bwd(dp, pooled, amax, h, w, None)
            zhat, inv, training = c[name + ":bn"]
            assert training
            wb = None
            if fault == "per_after_reductions" and self.sample_w is not None:      # (the actor's list carries no weights)
                wb = np.asarray(self.sample_w, dt).reshape(-1, 1, 1, 1)
                dz = dz / wb                                   # what the reductions see: the gradient without the importance weights
            dbeta = dz.sum(axis=(0, 1, 2))
            m1 = dz.mean(axis=(0, 1, 2), dtype=np.float64).astype(dt)
            m2 = (dz * zhat).mean(axis=(0, 1, 2), dtype=np.float64).astype(dt)
            if fault == "pooled_count":
                scale = dt(h * w) / dt((h // 2) * (w // 2))
                m1, m2 = m1 * scale, m2 * scale
            if fault == "no_mean_dy":
                m1 = np.zeros_like(m1)
            if fault == "no_zhat_term":
                m2 = np.zeros_like(m2)
            dz = (inv * (dz - m1 - zhat * m2)).astype(dt)
            if wb is not None:
                dz = dz * wb
            dW, _db, dp = O.conv_bwd(x, self.p[name + "/weights"], dz, need_dx=idx > 0)
            g[name + "/weights"], g[name + "/biases"] = dW, dbeta
        return g


@contextlib.contextmanager
def _statistics_over_the_first_image(on):
    orig = O.bn_stats
    if on:
        O.bn_stats = lambda z, dt, training: orig(z[:1] if training else z, dt, training)
    try:
        yield
    finally:
        O.bn_stats = orig


def planted(specs, P, fault, hyper=O.DEFAULT_HYPER, sample_w=None, restate=True):
    """oracle.DDPG(float64) on P with `fault` in all four networks (restate=False, fault None: the plain oracle)"""
    ref = oracle_of(specs, P, np.float64, hyper)
    if restate:
        net_fault = fault if fault in BACKWARD_FAULTS + ("per_after_reductions",) else None
        ref.actor, ref.critic = FaultyNet(ref.actor, net_fault), FaultyNet(ref.critic, net_fault, sample_w=sample_w)
        ref.target_actor = FaultyNet(ref.target_actor, None, inference=fault == "targets_moving_stats")
        ref.target_critic = FaultyNet(ref.target_critic, None, inference=fault == "targets_moving_stats")
    return ref


def one_minibatch(specs, P, batch, fault, weights=None, restate=True):
    """what the fused helper compares: actions, dQ/da, Q, TD and the two pre-clip gradient lists (weights: the critic's list is the
    backward pass of w * td, as tests/test_gpu_prioritized_replay.py's helper takes it)"""
    ref = planted(specs, P, fault, sample_w=weights, restate=restate)
    with _statistics_over_the_first_image(fault == "first_image_stats"):
        ag = ref.actor_gradients(batch[0])
        cg = ref.critic_gradients(batch)
        if weights is not None:
            cg = dict(cg, grads=ref.critic_gradients(batch, td_override=np.asarray(weights, np.float64).reshape(-1, 1) * cg["td"])["grads"])
    return {"actions": ag["actions"], "dq_da": ag["dq_da"], "q": cg["q"], "td": cg["td"], "actor_grads": ag["grads"], "critic_grads": cg["grads"]}


def grads_moved(spec, got, want, rel=GRAD_REL):
    """the largest factor by which a variable of the list leaves assert_flat_close's bar: it is bad there when its relative L2 error
    exceeds rel AND its largest absolute error exceeds rel x the list's RMS (one-element variables, which that function may excuse
    through abs_floor, are left out)"""
    scale = float(np.linalg.norm(np.asarray(want, np.float64))) / np.sqrt(len(want)) + 1e-30
    single = set(name for name, shp in spec.layout() if int(np.prod(shp)) == 1)
    return max(min(r / rel, m / (rel * scale)) for name, m, r in per_var_report(spec, got, want) if name not in single)


def ratios(specs, right, wrong):
    out = {k: float(np.abs(wrong[k] - right[k]).max()) / ATOL for k in ("actions", "dq_da", "q", "td")}
    out["actor_grads"] = grads_moved(specs[0], wrong["actor_grads"], right["actor_grads"])
    out["critic_grads"] = grads_moved(specs[1], wrong["critic_grads"], right["critic_grads"])
    return out


def _case(case, nb=1):
    shape, B, rows, seed = case
    return host_case(shape, B, nb, seed, rows=rows, batch_norm=True)


def _per_weights(rows, idxs, seed, beta=0.4):
    """importance weights of rows `idxs` under priorities lognormal(0, 2) (tests/test_gpu_prioritized_replay.py's spread; tests/per_np.py)"""
    p = np.random.default_rng(seed + 9).lognormal(0.0, 2.0, rows).astype(np.float32).astype(np.float64)
    w = np.power(rows * p[idxs] / p.sum(), -beta)
    return (w / w.max()).astype(np.float32)


SEEN = {"B1": set(FAULTS) - {"first_image_stats"}, "B7": set(FAULTS), "PER": set(FAULTS) | {"per_after_reductions"}}


@pytest.mark.parametrize("which", ["B1", "B7", "PER"])
def test_every_planted_fault_moves_a_compared_vector_by_ten_times_its_tolerance(which):
    case = {"B1": BN_B1_CASE, "B7": BN_B7_CASE, "PER": BN_PER_CASE}[which]
    specs, P, _ep, idxs, batches = _case(case)
    assert specs[0].batch_norm and specs[1].batch_norm
    weights = _per_weights(case[2], idxs, case[3]) if which == "PER" else None
    if weights is not None:
        assert weights.max() == 1.0 and weights.min() < 0.5, weights
    right = one_minibatch(specs, P, batches[0], None, weights)
    assert all(np.isfinite(v).all() for v in right.values())
    for fault in FAULTS + (("per_after_reductions",) if which == "PER" else ()):
        r = ratios(specs, right, one_minibatch(specs, P, batches[0], fault, weights))
        print("%-3s %-22s " % (which, fault) + "  ".join("%s %.3gx" % kv for kv in sorted(r.items())))
        if fault in SEEN[which]:
            assert max(r.values()) >= 10.0, (which, fault, r)
        else:
            assert max(r.values()) == 0.0, (which, fault, r)          # (B = 1: the first image is the batch)
    # the backward faults leave the forward values alone and are found through the gradient lists only
    r = ratios(specs, right, one_minibatch(specs, P, batches[0], "no_mean_dy", weights))
    assert max(r[k] for k in ("actions", "q", "td")) == 0.0 and r["dq_da"] == 0.0


def test_the_unfaulted_restatement_is_the_oracle():
    """FaultyNet(fault=None) computes oracle.ddpg_np.Net's numbers: the faults above are measured from the right place"""
    specs, P, _ep, _idxs, batches = _case(BN_B1_CASE)
    a, b = one_minibatch(specs, P, batches[0], None), one_minibatch(specs, P, batches[0], None, restate=False)
    for k in a:
        assert np.array_equal(a[k], b[k]), k
    specs, P, _ep, idxs, batches = _case((BN_PER_CASE[0], 3, 24, 5))
    w = _per_weights(24, idxs, 5)
    a, b = one_minibatch(specs, P, batches[0], None, w), one_minibatch(specs, P, batches[0], None, w, restate=False)
    for k in a:
        assert np.allclose(a[k], b[k], rtol=0, atol=1e-13 * max(1.0, float(np.abs(b[k]).max()))), k


def _beta_mask(spec):
    mask, off = np.zeros(spec.num_params(), bool), 0
    for name, shp in spec.layout():
        n = int(np.prod(shp))
        if name.startswith("conv") and name.endswith("/biases"):       # the BatchNorm/beta slot
            mask[off:off + n] = True
        off += n
    return mask


def test_dbeta_left_out_of_the_clip_norm_shows_at_loud():
    """the hyperparameter group's 16x16x6 case, three minibatches at LOUD (both lists clipped in every minibatch): a clip norm taken
    without the BatchNorm/beta gradients -- a launch_sumsq over the conv and fully connected weights only -- moves a reported norm
    or a parameter vector by >= 10x its tolerance (measured: the critic's reported norm by 13x, the critic's parameters by 6.8x)"""
    shape, B, seed = BN_HYPER_CASES["16x16x6"]
    nb, hp = 3, LOUD
    specs, P, _ep, _idxs, batches = host_case(shape, B, nb, seed, batch_norm=True)
    want, rs, outs, same = f32_twin_case(specs, P, batches, hp)
    assert same and all(np.isfinite(w).all() for w in want)
    assert all(min(o["actor_norm"], o["critic_norm"]) > hp.gradient_clip for o in outs)
    cur = [np.asarray(p, np.float64) for p in P]
    masks = [_beta_mask(specs[0]), _beta_mask(specs[1])]
    norms = []
    for b in batches:
        work = oracle_of(specs, cur, np.float64, hp)
        g = [work.actor_gradients(b[0])["grads"], work.critic_gradients(b)["grads"]]
        n = [float(np.linalg.norm(g[k][~masks[k]])) for k in (0, 1)]
        norms.append(n)
        for k, lr in ((0, hp.actor_lr), (1, hp.critic_lr)):
            cur[k] = cur[k] - lr * hp.gradient_clip * min(1.0 / n[k], 1.0 / hp.gradient_clip) * g[k]
    for k in (0, 1):
        cur[2 + k] = O.soft_update(cur[2 + k], cur[k], hp.target_update_rate, np.float64)
    tol = [delta_bound(p, w - p, r, nb) for p, w, r in zip(P, want, rs)]
    moved = [float(np.linalg.norm(c - w)) / t for c, w, t in zip(cur, want, tol)]
    right = (outs[-1]["actor_norm"], outs[-1]["critic_norm"])
    norm_moved = [abs(n - r) / (NORM_REL * max(1.0, r)) for n, r in zip(norms[-1], right)]
    print("dbeta_out_of_clip at LOUD: vectors %s, reported norms %s x their tolerances" % (
        ["%.3g" % m for m in moved], ["%.3g" % m for m in norm_moved]))
    assert max(moved + norm_moved) >= 10.0, (moved, norm_moved)
    # (and the oracle_train_step the GPU module's expectation comes from is the loop restated above when nothing is left out)
    ref = oracle_of(specs, P, np.float64, hp)
    oracle_train_step(ref, batches)
    for g, w in zip(four_vectors(ref), want):
        assert np.array_equal(g, w)
