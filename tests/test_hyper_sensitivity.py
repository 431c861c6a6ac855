"""What tests/test_gpu_hyperparameters.py can see, established with the float64 oracle alone (no GPU): for every hyperparameter set
of that module and every fault the set is meant to expose, the fault is PLANTED IN THE ORACLE and must move at least one of the
compared vectors by at least 10x the tolerance the GPU test applies to that vector.  The inputs are the GPU test's own
(tests.helpers.host_case: the same parameters, episodes and rows), so a pass here says that a device with that fault fails there.

Tolerances (the GPU module's): several minibatches -- per vector (actor, critic, target actor, target critic)
    2^-23 * nb * |theta| + r * |delta_f64|,  r = max(5e-5, F32_GRAD_FACTOR x the float32 numpy twin's own relative delta error);
NAF, one step after warm-up -- naf_fused_step_against_f64_oracle's 2^-23 * |theta| + 5e-5 * |delta_f64|, parameters and target;
the loss at 1e-5 * max(1, |loss|); the second call's TD after a target update -- 1e-5 absolute.

Planted faults: targets updated from the values before the last minibatch; conv1's forward reading weights one minibatch old (a
stale operand image); the discount fixed at 0.99; the clip ignored; the clip scales swapped between the two lists; the clip as a
plain normalisation clip / norm (no min with 1: scales a short list UP); clip None taken as the default 5; the two learning rates
swapped; Momentum / Adam slots not carried over; Adam's bias correction with t - 1; the target conv1 image not rebuilt after a
target update.

NOT COVERED at 10x by any set (by construction, not by measurement):
  * a stale conv1 image of the ACTOR alone at LOUD: the actor's clipped update is lr * clip = 5e-3 per minibatch, as at the defaults;
    the fault moves the actor by 0.4x (16x16) .. 9x (64x64x18) of its tolerance and is found through the critic.  The 64x64x18 row
    ACTOR_LOUD (actor learning rate 0.1) is there for it: test_a_stale_conv1_image_shows_where_the_rider_runs.
  * Momentum 0.0: 'slot not carried over' changes nothing (the slot is multiplied by zero); that case exists to be compared with
    GradientDescent, not to find this fault.  Momentum 0.5 and Adam find it.
  * gradient_clip None and 1e4: 'clip ignored' and 'clip scales swapped' change nothing (every scale is 1).  Those two sets are
    there for 'None taken as 5' and 'clip / norm without the min', which they do expose; LOUD and SPLIT expose the other two.
"""
import numpy as np
import pytest

from oracle import ddpg_np as O
from oracle import naf_np as N
from tests.helpers import (HYPER_SETS, LOUD, NAF_HYPER, NAF_OPTIMISERS, NAF_RIDER_CASE, RIDER_CASES, SENS_SHAPE, SENS_B, SENS_SEED, STALE_TARGET_CASE, delta_bound,
                           f32_twin_case, four_vectors, host_case, naf_host_case, naf_twin_case, oracle_of, oracle_train_step)

VECTORS = ("actor", "critic", "target_actor", "target_critic")
COMMON = ("targets_from_old_values", "stale_conv1", "discount_0.99", "lr_swapped")
FAULTS = {"LOUD": COMMON + ("clip_ignored", "clip_swapped"),
          "UNCLIPPED_NONE": COMMON + ("none_is_default_clip",),
          "UNCLIPPED_1E4": COMMON + ("clip_over_norm",),
          "SPLIT": COMMON + ("clip_ignored", "clip_swapped", "clip_over_norm")}


def _scale(clip, norm):
    return 1.0 if clip is None or norm == 0 else clip * min(1.0 / norm, 1.0 / clip)      # (norm 0: a dead network, nothing to scale)


def faulty_train_step(specs, P, batches, hp, fault):
    """oracle.DDPG.train_step in float64 with one fault planted"""
    cur = [np.asarray(p, np.float64) for p in P]
    prev_conv1 = None
    n1 = [int(np.prod(s.layout()[0][1])) for s in specs]            # conv1/weights lead both flat vectors
    for i, b in enumerate(batches):
        seen = [c.copy() for c in cur]
        if fault == "stale_conv1" and prev_conv1 is not None:
            for k in (0, 1):
                seen[k][:n1[k]] = prev_conv1[k]
        work = oracle_of(specs, seen, np.float64, hp._replace(discount=0.99) if fault == "discount_0.99" else hp)
        ga, gc = work.actor_gradients(b[0])["grads"], work.critic_gradients(b)["grads"]
        na, nc = float(np.linalg.norm(ga)), float(np.linalg.norm(gc))
        clip = hp.gradient_clip
        sa, sc = _scale(clip, na), _scale(clip, nc)
        if fault == "clip_ignored":
            sa = sc = 1.0
        elif fault == "clip_swapped":
            sa, sc = sc, sa
        elif fault == "clip_over_norm":
            sa, sc = (clip / na if na > 0 else 1.0), (clip / nc if nc > 0 else 1.0)      # (a dead network has no gradient left)
        elif fault == "none_is_default_clip":
            sa, sc = _scale(5.0, na), _scale(5.0, nc)
        la, lc = (hp.critic_lr, hp.actor_lr) if fault == "lr_swapped" else (hp.actor_lr, hp.critic_lr)
        prev_conv1 = [cur[k][:n1[k]].copy() for k in (0, 1)]
        if fault == "targets_from_old_values" and i == len(batches) - 1:
            src = [cur[0].copy(), cur[1].copy()]
        cur[0], cur[1] = cur[0] - la * sa * ga, cur[1] - lc * sc * gc
    if fault != "targets_from_old_values":
        src = cur[:2]
    for k in (0, 1):
        cur[2 + k] = O.soft_update(cur[2 + k], src[k], hp.target_update_rate, np.float64)
    return cur


@pytest.mark.parametrize("name", sorted(HYPER_SETS))
def test_each_hyperparameter_set_exposes_its_faults_at_ten_times_the_gpu_tolerance(name):
    hp, nb = HYPER_SETS[name], 3
    specs, P, _ep, _idxs, batches = host_case(SENS_SHAPE, SENS_B, nb, SENS_SEED)
    want, rs, outs, same_routes = f32_twin_case(specs, P, batches, hp)
    assert all(np.isfinite(w).all() for w in want)
    assert same_routes, "the float32 twin and the float64 oracle disagree on a pool / ReLU route: choose another seed"
    for i, o in enumerate(outs):
        print("%s minibatch %d: actor norm %.4g critic norm %.4g (clip %s)" % (name, i, o["actor_norm"], o["critic_norm"], hp.gradient_clip))
    tol = [delta_bound(p, w - p, r, nb) for p, w, r in zip(P, want, rs)]
    print("%s r = %s" % (name, ", ".join("%s %.2e" % (v, r) for v, r in zip(VECTORS, rs))))
    if name == "SPLIT":       # exactly one list clipped in the first minibatch
        assert outs[0]["actor_norm"] < hp.gradient_clip < outs[0]["critic_norm"]
    elif name == "LOUD":
        assert all(min(o["actor_norm"], o["critic_norm"]) > hp.gradient_clip for o in outs)
    elif name == "UNCLIPPED_1E4":
        assert all(max(o["actor_norm"], o["critic_norm"]) < hp.gradient_clip for o in outs)
    for fault in FAULTS[name]:
        got = faulty_train_step(specs, P, batches, hp, fault)
        ratios = [float(np.linalg.norm(g - w)) / t for g, w, t in zip(got, want, tol)]
        print("%-15s %-24s " % (name, fault) + "  ".join("%s %.3e / tol %.3e = %.0fx" % (v, ra * t, t, ra) for v, ra, t in zip(VECTORS, ratios, tol)))
        assert max(ratios) >= 10.0, (name, fault, ratios)


def test_the_unfaulted_restatement_is_the_oracle():
    """faulty_train_step(fault=None) is oracle.DDPG.train_step: the faults above are measured from the right place"""
    specs, P, _ep, _idxs, batches = host_case(SENS_SHAPE, SENS_B, 2, SENS_SEED)
    ref = oracle_of(specs, P, np.float64, LOUD)
    ref.train_step(batches)
    for g, w in zip(faulty_train_step(specs, P, batches, LOUD, None), four_vectors(ref)):
        assert np.allclose(g, w, rtol=0, atol=1e-12)
    # ... and so is tests.helpers.oracle_train_step, where the expected values of the GPU module come from (it exists to get at the routes)
    ref2 = oracle_of(specs, P, np.float64, LOUD)
    oracle_train_step(ref2, batches)
    for g, w in zip(four_vectors(ref2), four_vectors(ref)):
        assert np.array_equal(g, w)


@pytest.mark.parametrize("name", sorted(RIDER_CASES))
def test_a_stale_conv1_image_shows_where_the_rider_runs(name):
    """the conv1 operand image and its rider exist at 64x64 only.  On the GPU module's 64x64x18 inputs a conv1 forward that reads
    weights one minibatch old moves the critic by >= 10x its tolerance at LOUD (the actor, whose clipped update is lr * clip = 5e-3 per
    minibatch as at the defaults, by less); ACTOR_LOUD (actor learning rate 0.1) is there so that the ACTOR moves by >= 10x too -- a
    stale image of the actor alone is seen"""
    shape, B, seed, hp = RIDER_CASES[name]
    specs, P, _ep, _idxs, batches = host_case(shape, B, 3, seed)
    want, rs, _outs, same_routes = f32_twin_case(specs, P, batches, hp)
    assert same_routes and all(np.isfinite(w).all() for w in want)
    tol = [delta_bound(p, w - p, r, 3) for p, w, r in zip(P, want, rs)]
    got = faulty_train_step(specs, P, batches, hp, "stale_conv1")
    ratios = [float(np.linalg.norm(g - w)) / t for g, w, t in zip(got, want, tol)]
    print("%s 64x64x18 stale_conv1: " % name + "  ".join("%s %.1fx" % (v, ra) for v, ra in zip(VECTORS, ratios)))
    assert ratios[1] >= 10.0 and (name != "ACTOR_LOUD" or ratios[0] >= 10.0), ratios


@pytest.mark.parametrize("name", sorted(NAF_OPTIMISERS))
def test_a_stale_conv1_image_shows_in_the_naf_rider_case(name):
    """the GPU module's shared-trunk NAF case (three minibatches in one call, tests.helpers.naf_host_case): the oracles stay finite and
    agree on the routes, and a value-network conv1 forward on weights one minibatch old -- a rider that missed the Momentum update, an
    image not rebuilt after Adam's -- moves the parameters by >= 10x the tolerance"""
    oname, oargs, _warm = NAF_OPTIMISERS[name]
    shape, B, nb, rows, seed = NAF_RIDER_CASE
    specs, flats, _ep, _idxs, batches = naf_host_case(shape, B, nb, rows, seed)
    want, rs, norms, same = naf_twin_case(specs, flats, batches, oname, oargs)
    assert same and np.isfinite(want[0]).all() and np.isfinite(want[1]).all()
    print("NAF %s: norms %s (clip %s), r %s" % (name, norms, NAF_HYPER["clip"], rs))
    assert min(norms) > NAF_HYPER["clip"]
    ref = _naf(specs, flats, N.make_optimiser(oname, oargs))
    ref.share = True
    prev = None
    for b in batches:
        fresh = ref.value.p["conv1/weights"]
        if prev is not None:
            ref.value.p["conv1/weights"] = prev
        out = ref.forward_backward(b)
        ref.value.p["conv1/weights"] = fresh
        ref.apply(out["grads"])
        prev = fresh
    ref.update_targets()
    p0 = np.concatenate(flats[:3])
    ratio = float(np.linalg.norm(ref.flat() - want[0])) / delta_bound(p0, want[0] - p0, rs[0], nb)
    print("NAF %s stale conv1 image: params off by %.0fx the tolerance" % (name, ratio))
    assert ratio >= 10.0


def test_a_target_conv1_image_that_missed_the_update_shows_in_the_second_calls_td():
    """case d of the GPU module: after one train_step at tau = 0.25 the second call's TD, computed with target networks whose
    conv1 weights are still the ones from before the update, is off by >= 10 x the 1e-5 the GPU test allows"""
    shape, B, seed = STALE_TARGET_CASE
    specs, P, _ep, _idxs, batches = host_case(shape, B, 2, seed, rows=40)
    ref = oracle_of(specs, P, np.float64, LOUD)
    oracle_train_step(ref, batches[:1])
    right = ref.critic_gradients(batches[1])["td"]
    now = four_vectors(ref)
    for k in (2, 3):
        n1 = int(np.prod(specs[k - 2].layout()[0][1]))
        now[k][:n1] = np.asarray(P[k][:n1], np.float64)
    wrong = oracle_of(specs, now, np.float64, LOUD).critic_gradients(batches[1])["td"]
    err = float(np.abs(wrong - right).max())
    print("stale target conv1 image: TD off by %.3e (tolerance 1e-5)" % err)
    assert np.isfinite(right).all() and err >= 10 * 1e-5


# ---- NAF: one checked step after warm-up, as naf_fused_step_against_f64_oracle does
def _naf(specs, flats, opt, m=None, v=None, t=0, discount=None):
    vspec, mspec, lspec = specs
    ref = N.NAF(vspec, mspec, lspec, flats[0], flats[1], flats[2], False, 2, np.float64, discount=NAF_HYPER["discount"] if discount is None else discount,
                gradient_clip=NAF_HYPER["clip"], target_update_rate=NAF_HYPER["target_update_rate"], optimiser=opt)
    ref.target_value = O.Net(vspec, flats[3], np.float64)
    if m is not None:
        ref.m, ref.v, ref.t = m.copy(), v.copy(), t
    return ref


NAF_FAULTS = {"momentum-0.5": ("slot_not_carried", "discount_0.99"), "momentum-0.0": ("discount_0.99",),
              "adam-third-step": ("slot_not_carried", "bias_correction_t_minus_1", "discount_0.99")}


@pytest.mark.parametrize("name", sorted(NAF_OPTIMISERS))
def test_naf_optimiser_cases_expose_their_faults(name):
    oname, oargs, warm = NAF_OPTIMISERS[name]
    opt = N.make_optimiser(oname, oargs)
    shape, B = SENS_SHAPE, 8
    kw = dict(pixel=True, H=shape[0], W=shape[1], C=int(np.prod(shape[2:])))
    specs = (N.HeadSpec(1, "linear", [100, 50], **kw), N.HeadSpec(2, "tanh", [100, 50], **kw), N.HeadSpec(3, "linear", [100, 50], **kw))
    rng = np.random.default_rng(17)
    flats = []
    for sp in specs:
        p = N.init_head_params(sp, rng)
        flats.append(p + rng.normal(0, 0.05, p.shape).astype(np.float32))
    flats.append(flats[0] + rng.normal(0, 0.01, flats[0].shape).astype(np.float32))
    ref = _naf(specs, flats, opt)
    for _ in range(warm):
        ref.train(O.synthetic_batch(rng, B, shape, 2, True))
    batch = O.synthetic_batch(rng, B, shape, 2, True)
    start = [ref.value.flat(), ref.mu.flat(), ref.l.flat(), ref.target_value.flat()]
    m, v, t = ref.m, ref.v, ref.t
    assert t == warm

    def step(fault):
        r = _naf(specs, start, opt, m, v, t, discount=0.99 if fault == "discount_0.99" else None)
        if fault == "slot_not_carried":
            r.m, r.v = np.zeros_like(m), np.zeros_like(v)
        if fault == "bias_correction_t_minus_1":
            r.t = t - 1
        out = r.train(batch)
        r.update_targets()
        return r.flat(), r.target_value.flat(), out
    want_p, want_t, out = step(None)
    assert np.isfinite(want_p).all() and np.isfinite(want_t).all()
    print("%s: gradient norm %.4g (clip %s), step %d" % (name, out["norm"], NAF_HYPER["clip"], t + 1))
    p0 = np.concatenate(start[:3])
    tol_p, tol_t = delta_bound(p0, want_p - p0, 5e-5), delta_bound(start[3], want_t - start[3], 5e-5)
    for fault in NAF_FAULTS[name]:
        got_p, got_t, bad = step(fault)
        rp, rt = float(np.linalg.norm(got_p - want_p)) / tol_p, float(np.linalg.norm(got_t - want_t)) / tol_t
        rl = abs(bad["loss"] - out["loss"]) / (1e-5 * max(1.0, abs(out["loss"])))       # (the helper holds the loss to 1e-5 as well)
        print("%-16s %-26s params %.0fx  target %.0fx  loss %.0fx of the tolerance (%.3e, %.3e)" % (name, fault, rp, rt, rl, tol_p, tol_t))
        assert max(rp, rt, rl) >= 10.0, (name, fault, rp, rt, rl)
