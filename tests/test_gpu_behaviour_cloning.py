"""The behaviour-cloning actor term on the device (--bc-alpha; cpp_ddpg_set_behaviour_cloning: csrc/bc.hip behind the action-columns dX GEMM
of the GEMM levels) against (1) the kernel's own float32 inputs recomputed in float64 and (2) the float64 restatement tests/bc_np.py.  The
cases, their seeds, the bars with their derivations and what they can see are that module's and tests/test_bc_host.py's.

Every minibatch of (2) is compared from a common start: the restatement takes over the device's parameters, slots and counts before it.
Bars: a, Q, td and dQ/da at the project's 1e-5 (td under smoothing plus tests.tps_np.td_bar's propagated noise term); lambda at
lambda64 (1e-5 / m64 + 2^-22); g at |dlambda| |dq_da| + (lambda + 2/A) 1e-5; sel exactly; pre-clip lists at rel 2e-5, norms at 1e-4;
parameter, target and slot deltas at tests.ddpg_opt_np's 2^-23 |theta| + 5e-5 |delta|, parameters and targets besides at rel 2e-5."""
import hashlib

import numpy as np
import pytest

from oracle import ddpg_np as O
from tests import actor_min_np as AM
from tests import bc_np as Bc
from tests import ddpg_opt_np as R
from tests import td3_np as T3
from tests import tps_np as TP
from tests import twin_np as W
from tests.helpers import _profiled_calls, assert_flat_close, delta_bound, host_case
from tests.test_gpu_twin_q import PER_KW, HostBatch, _build, _params, _slots

pytestmark = pytest.mark.gpu
CPP_ERR_ARG, CPP_ERR_STATE = 1, 3          # include/cartpolepp_abi.h


def _abi():
    from cartpoleplusplus_amd._lib import lib, check, ptr
    return lib, check, ptr


def _kind(case):
    return case[9].get("critic", "plain")


def _case_kw(case):
    _cid, _sn, _A, _B, opt, d, sm, _clip, _tau, extra = case
    kw = dict(T3.opt_kw(opt))
    if d > 1:
        kw["policy_delay"] = d
    if sm is not None:
        kw.update(target_policy_noise=sm[0], target_policy_noise_clip=sm[1], target_policy_noise_seed=sm[2])
    if extra.get("weighted"):
        kw.update(PER_KW)
    if _kind(case) == "min":
        kw["actor_min_q"] = True
    return kw


def _agent(case, inputs, on=True, **kw):
    _cid, shape_name, A, B = case[:4]
    specs, P, episodes, _idxs, _b = inputs
    opts = dict(_case_kw(case), **kw)
    if on:
        opts.update(bc_alpha=Bc.ALPHA, bc_q_floor=Bc.floor_of(case))
    return _build(Bc.SHAPES[shape_name], B, A, Bc.hyper_of(case), P, episodes, rows=Bc.rows_of(case), twin=_kind(case) != "plain", **opts)


# ---- 1. the kernel against its own inputs
KERNEL_B = (1, 5, 7, 64, 65, 257)      # one row, a partial wave, a wave boundary, more than one 256-thread workgroup each re-deriving m


def _kernel_pass(agent, hb, B, A, amin):
    """the actor's half on the minibatch (cpp_ddpg_q_gradients_wrt_actions: dq_da, mu and Q(s1, mu) of head 1 as the kernel read them), what
    the kernel left, the output layer's bias gradient (the column sums of adz: the [dW; db] GEMM's last row)"""
    lib, check, ptr = _abi()
    t = agent.trainer
    dev = t.device_batch_for(hb)
    dq, mu, q = np.empty((B, A), np.float32), np.empty((B, A), np.float32), np.empty((B, 1), np.float32)
    check(lib.cpp_ddpg_q_gradients_wrt_actions(t.handle, dev.handle, ptr(dq), ptr(mu), ptr(q)))
    lam, m, g, rows = t.last_behaviour_cloning(B)
    sel = None
    if amin:
        q1, q2, sel = t.last_actor_min(B)
        assert np.array_equal(q1, q)
        q = np.where((sel == 1).reshape(B, 1), q1, q2)
    db = O.unflatten(agent_spec(agent, A), agent.actor.get_grads(), np.float32)["output_action/biases"]
    return dq, mu, q, lam, m, g, rows, np.asarray(db, np.float64).ravel(), sel


def agent_spec(agent, A):
    return O.NetSpec("actor", A, (100, 100, 50), pixel=False, state_elems=28)


def _check_kernel(what, B, A, a, dq, mu, q, lam, m, g, rows, db, floor):
    m64, lam64, g64, adz64, rows64, gb, ab = Bc.kernel_reference(q, dq, mu, a, Bc.ALPHA, floor)
    err = {"m": abs(m - m64) / m64, "lambda": abs(lam - lam64) / lam64, "g / bar": float((np.abs(g - g64) / np.maximum(gb, 1e-300)).max()),
           "rows": float(np.abs(rows - rows64).max())}
    # the bias gradient: B additions of adz in float32, each at most 2^-24 of a partial sum that is at most sum |adz|; factor 2 as the bars'
    db_bar = ab.sum(axis=0) + 2.0 * B * 2.0 ** -24 * np.abs(adz64).sum(axis=0)
    err["db / bar"] = float((np.abs(db - adz64.sum(axis=0)) / np.maximum(db_bar, 1e-300)).max())
    print("%s: m %.6f lambda %.4f  %s" % (what, m64, lam64, {k: "%.2e" % v for k, v in err.items()}))
    assert err["m"] <= Bc.M_REL and err["lambda"] <= Bc.LAMBDA_REL, (what, err)
    assert (np.abs(g - g64) <= gb).all(), (what, err)
    assert (np.abs(db - adz64.sum(axis=0)) <= db_bar).all(), (what, err)          # (B = 1: adz itself, element by element)
    # (1/A) sum (mu - a)^2 in float32: A roundings of the squares' sum, the difference's and the division's, on values below 4
    assert (np.abs(rows - rows64) <= (A + 3) * 2.0 ** -24 * np.maximum(rows64, 2.0 ** -100)).all(), (what, err)
    return m64


@pytest.mark.parametrize("A", [1, 2, 3, 5, 8, 9, 16])
def test_the_kernel_against_its_own_inputs(A):
    """the low-dimensional pair (28,), every B of KERNEL_B on one agent; B = 5 once more on the floor branch"""
    Bmax = max(KERNEL_B)
    hp = O.Hyper(1e-2, 5e-2, 0.9, 0.5, 0.25)
    specs, P, _ep, _idxs, batches = host_case((28,), Bmax, 1, 1, rows=2 * Bmax, action_dim=A)
    agent = _build((28,), Bmax, A, hp, P, None, rows=2 * Bmax, twin=False, bc_alpha=Bc.ALPHA)
    try:
        for floor in (Bc.Q_FLOOR, Bc.HIGH_FLOOR):
            agent.trainer.set_behaviour_cloning(Bc.ALPHA, floor)
            for B in KERNEL_B if floor == Bc.Q_FLOOR else (5,):
                hb = HostBatch(*[np.ascontiguousarray(x[:B]) for x in batches[0]])
                dq, mu, q, lam, m, g, rows, db, _sel = _kernel_pass(agent, hb, B, A, False)
                m64 = _check_kernel("A%d B%d floor %g" % (A, B, floor), B, A, hb.action, dq, mu, q, lam, m, g, rows, db, floor)
                assert (m64 < floor) == (floor == Bc.HIGH_FLOOR) and abs(m64 - floor) >= Bc.FLOOR_GAP * floor
    finally:
        agent.close()


def test_the_kernel_reads_the_selected_head_under_actor_min_q():
    """--twin-q --actor-min-q on the low-dimensional pair: q is the row's selected head's, both heads followed, at B = 7 and 65"""
    case = Bc.case_of("lowdim-A3-B7-td3-min")
    A = case[2]
    specs, P, _ep, _idxs, _b = Bc.case_inputs(case)
    _s, _P, _e, _i, batches = host_case((28,), 65, 1, 3, rows=130, action_dim=A)
    agent = _build((28,), 65, A, Bc.hyper_of(case), P, None, rows=130, twin=True, actor_min_q=True, bc_alpha=Bc.ALPHA)
    try:
        for B in (7, 65):
            hb = HostBatch(*[np.ascontiguousarray(x[:B]) for x in batches[0]])
            dq, mu, q, lam, m, g, rows, db, sel = _kernel_pass(agent, hb, B, A, True)
            assert set(sel.tolist()) == {1, 2}, sel
            _check_kernel("min A%d B%d" % (A, B), B, A, hb.action, dq, mu, q, lam, m, g, rows, db, Bc.Q_FLOOR)
            q1 = agent.trainer.last_actor_min(B)[0]
            assert abs(np.abs(q1.astype(np.float64)).mean() - m) > 1e-4 * m          # (head 1 alone gives another m)
    finally:
        agent.close()


# ---- 2. whole minibatches against the restatement from a common start
def _take_over(ref, P, slots, counts, k):
    na = len(P[0])
    for w, sl in (("actor", slice(0, na)), ("critic", slice(na, None))):
        ref.slots[w].m, ref.slots[w].v = np.asarray(slots[0][sl], np.float64).copy(), np.asarray(slots[1][sl], np.float64).copy()
    if counts is not None:
        ref.slots["actor"].t, ref.slots["critic"].t = counts
    ref.n, ref.tps_n = k, k
    return ref


def _read(agent, case, B=None):
    B, kind, t = case[3] if B is None else B, _kind(case), agent.trainer
    actions, dq_da, q, td = t.last_values(B)
    lam, m, g, rows = t.last_behaviour_cloning(B)
    stats = t.last_stats()
    got = {"actions": actions, "dq_da": dq_da, "q": q, "td": td, "lambda": lam, "m": m, "g": g, "bc_rows": rows, "loss": float(stats[0]),
           "actor_norm": float(stats[1]), "critic_norm": float(stats[2]), "g_a": agent.actor.get_grads(), "g_c": agent.critic.get_grads()}
    if kind != "plain":
        got["q2"], got["tq1"], got["tq2"], got["td2"] = t.last_twin_values(B)
    if kind == "min":
        got["q1m"], got["q2m"], got["sel"] = t.last_actor_min(B)
    got["w"] = agent.replay_memory.last_weights(B).astype(np.float64).reshape(B, 1) if case[9].get("weighted") else None
    return got


def _compare_minibatch(case, specs, start, got, after, k, batch):
    """one minibatch from the common start `start` = (the four parameter vectors, [m, v], counts)"""
    cid, _sn, A, B, opt, d, sm, _clip, _tau, _x = case
    kind = _kind(case)
    P, slots, counts = start
    ref = _take_over(Bc.restatement(case, specs, P), P, slots, counts, k)
    if got["w"] is not None:
        ref.weights = got["w"]
    out = ref.train_minibatch(batch)
    ag, cg = ref.last_ag, ref.last_cg
    ref.update_targets()
    atol = Bc.P_BAR
    bar = atol
    if sm is not None:
        bar = W.td_bar(ref.hp.discount, sm[0], cg, atol) if kind != "plain" else TP.td_bar(ref.hp.discount, sm[0], cg["target_dq_da"], atol)
    floor = Bc.floor_of(case)
    assert abs(ag["m"] - floor) >= Bc.FLOOR_GAP * floor and (ag["m"] < floor or ag["m"] >= Bc.M_MIN), (cid, k, ag["m"])
    lam_bar, g_bar = Bc.lambda_bar(ag["lambda"], ag["m"]), Bc.g_bar(ag["lambda"], ag["m"], ag["dq_da"], A)
    err = {"actions": np.abs(got["actions"] - ag["actions"]).max(), "dq_da": np.abs(got["dq_da"] - ag["dq_da"]).max(),
           "q": np.abs(got["q"] - cg["q"]).max(), "td": np.abs(got["td"] - cg["td"]).max(), "loss": abs(got["loss"] - float(cg["loss"])),
           "m": abs(got["m"] - ag["m"]), "lambda / bar": abs(got["lambda"] - ag["lambda"]) / lam_bar,
           "g / bar": float((np.abs(got["g"] - ag["g"]) / g_bar).max()), "bc_rows": np.abs(got["bc_rows"] - ag["bc_rows"]).max()}
    if kind != "plain":
        err.update({"q2": np.abs(got["q2"] - cg["q2"]).max(), "td2": np.abs(got["td2"] - cg["td2"]).max()})
    if kind == "min":
        err.update({"q1m": np.abs(got["q1m"] - ag["q1"]).max(), "q2m": np.abs(got["q2m"] - ag["q2"]).max()})
        assert float(np.abs(ag["q1"] - ag["q2"]).min()) >= AM.TIE_MARGIN and np.array_equal(got["sel"], ag["sel"]), (cid, k, got["sel"], ag["sel"])
    print("%s minibatch %d: m %.4f lambda %.4f (%s the floor) applied %s; %s; TD bar %.3e" %
          (cid, k, ag["m"], ag["lambda"], "on" if ag["m"] < floor else "off", out["applied"], {a: "%.2e" % b for a, b in err.items()}, bar))
    for key in ("actions", "dq_da", "q", "q2", "q1m", "q2m"):
        assert key not in err or err[key] < atol, (cid, k, key, err)
    assert err["m"] <= atol + Bc.M_REL * ag["m"], (cid, k, err)          # (the mean of B errors of Q, then one rounding)
    for key in ("td", "td2", "loss"):
        assert key not in err or err[key] < bar, (cid, k, key, err, bar)
    # ((1/A) sum (mu - a)^2 moves by at most 2 max|mu - a| <= 4 times the actions' bar)
    assert err["lambda / bar"] <= 1.0 and err["g / bar"] <= 1.0 and err["bc_rows"] < 4 * atol, (cid, k, err)
    assert_flat_close(specs[0], got["g_a"], ag["grads"], rel=2e-5, what="%s minibatch %d actor pre-clip grads" % (cid, k))
    cspec = W.TwinLayoutSpec(specs[1]) if kind != "plain" else specs[1]
    tds = max(err["td"], err.get("td2", 0.0))
    try:
        assert_flat_close(cspec, got["g_c"], cg["grads"], rel=2e-5, what="%s minibatch %d critic pre-clip grads" % (cid, k), abs_floor=2.0 * tds)
    except AssertionError:
        if sm is None or kind == "plain":
            raise
        # (linear in the TDs, and the device's noise sits up to Z_BAR * sigma from the restated one: the backward arithmetic at the device's
        # TDs -- tests/test_gpu_twin_q.py)
        ww = np.ones((B, 1)) if got["w"] is None else got["w"]
        fresh = Bc.restatement(case, specs, P)
        cb = fresh.critic.forward(batch[0], action=np.asarray(batch[1], np.float64))
        grads, _da = fresh.critic.backward(cb, 2.0 * got["td"].astype(np.float64) * ww / B, 2.0 * got["td2"].astype(np.float64) * ww / B)
        assert_flat_close(cspec, got["g_c"], W.flatten_grads(specs[1], grads, np.float64), rel=2e-5,
                          what="%s minibatch %d critic grads at the device's TDs" % (cid, k), abs_floor=2.0 * tds)
    na, nc = out["actor_norm"], out["critic_norm"]
    assert abs(got["actor_norm"] - na) < 1e-4 * max(1.0, na) and abs(got["critic_norm"] - nc) < 1e-4 * max(1.0, nc), (cid, k, got["actor_norm"], na, nc)
    want = W.vectors(ref)
    have = list(after[0]) + list(after[1])
    begin = list(P) + [np.asarray(slots[0], np.float64), np.asarray(slots[1], np.float64)]
    bad = []
    for name, g, w, p in zip(T3.VECTORS, have, want, begin):
        if (name == "v" and opt != "adam") or (name == "m" and opt == "gradient-descent"):
            assert not np.asarray(g).any()
            continue
        e, b = float(np.linalg.norm(np.asarray(g, np.float64) - w)), delta_bound(p, w - p, R.R[name], 1)
        if not e <= b:
            bad.append((name, e, b))
        if name in T3.VECTORS[:4] and not e <= R.PARAM_REL * float(np.linalg.norm(w)):
            bad.append((name, "rel", e))
    assert not bad, (cid, k, bad)
    if not out["applied"]:      # a held actor keeps its bits
        assert d > 1 and np.array_equal(after[0][0], P[0]), (cid, k)
    if after[2] is not None:
        assert after[2] == [int(x) for x in ref.state()["step"]], (cid, k, after[2])
    return out


def partial_plan(case, inputs, capacity):
    """tests.helpers.capacity_plan of a case"""
    from tests.helpers import capacity_plan
    _cid, shape_name, A, B = case[:4]
    return capacity_plan(Bc.rows_of(case), Bc.SHAPES[shape_name], A, inputs[2], inputs[3], inputs[4], B, capacity)


def _run_case(cid, nb=Bc.NB, capacity=None, **kw):
    """capacity=C > B: the agent is built for C rows and walks partial_plan's minibatches -- C rows, B, B, C -- each held to the
    restatement from the device's own state in front of it, at the same bars"""
    case = Bc.case_of(cid)
    B = case[3]
    inputs = Bc.case_inputs(case, nb=nb)
    specs, _P, _ep, idxs, batches = inputs
    plan = [(idxs[k * B:(k + 1) * B], batches[k]) for k in range(nb)] if capacity is None else partial_plan(case, inputs, capacity)
    agent = _agent(case, inputs, capacity=capacity, **kw)
    outs = []
    try:
        assert agent.trainer.behaviour_cloning == (Bc.ALPHA, Bc.floor_of(case))
        if case[9].get("weighted"):
            agent.replay_memory.update_priorities(np.arange(Bc.rows_of(case)),
                                                  np.random.default_rng(9).lognormal(0.0, 1.0, Bc.rows_of(case)).astype(np.float32))
        for k, (rows, batch) in enumerate(plan):
            sl, counts = _slots(agent)
            start = (_params(agent), sl, counts)
            census = _profiled_calls(agent.actor.ctx, lambda: agent.train_step(len(rows), 1, idxs=rows))
            assert census.get("bc", 0) == 1 and census.get("heads", 0) == 0, census
            got = _read(agent, case, len(rows))
            sl2, counts2 = _slots(agent)
            outs.append(_compare_minibatch(case, specs, start, got, (_params(agent), sl2, counts2), k, batch))
    finally:
        agent.close()
    return case, outs


def test_minibatches_below_the_capacity_against_the_float64_restatement():
    """(C, B) = (8, 5): the batch mean m of |Q| behind lambda, the term's rows and both gradient lists at B behind a C-row minibatch, and at C
    again behind the B-row ones"""
    _run_case("A1-B5-sgd", capacity=8)


@pytest.mark.parametrize("cid", [c[0] for c in Bc.CASES if c[0] not in Bc.BIG])
def test_minibatches_against_the_float64_restatement(cid):
    case, outs = _run_case(cid)
    if case[5] == 2:
        assert [o["applied"] for o in outs] == [False, True, False]          # --policy-delay 2: held and applied
    if case[4] == "adam":      # both sides of the clip, as the case's name says
        clip = case[7]
        assert all((o["actor_norm"] > clip) == (clip < 1) and (o["critic_norm"] > clip) == (clip < 1) for o in outs), (clip, outs)


def test_the_offline_td3_stack_at_64x64x18():
    """--twin-q --target-policy-noise 0.2 --policy-delay 2 --ddpg-optimiser Adam with --bc-alpha 2.5, B = 8: a held and an applied minibatch"""
    _case, outs = _run_case(Bc.BIG[0], nb=2)
    assert [o["applied"] for o in outs] == [False, True]


def test_feature_layer_norm_per_nstep_u8_and_random_shift_against_the_float64_restatement():
    """--feature-layer-norm with prioritized replay, n-step 3, the u8 store and random shift at 64x64x18, B = 8 (tests/test_gpu_layer_norm.py's
    stack, the term on top): two warm minibatches on device-drawn rows, then the checked one -- its rows, weights and shifts read back, the
    minibatch rebuilt on the host (the memory's n-step columns, tests/shift_np.py's images), the float64 restatement (tests.layer_norm_np's
    networks under tests.bc_np.BcDDPG) on the device's routes.  The stored actions are the rows' own: the cloning term reads what the gather
    left, under every one of these features"""
    from tests import layer_norm_np as L
    from tests import test_gpu_layer_norm as GL
    from tests.helpers import twin_rs
    from tests.test_gpu_random_shift import _shifted_minibatch
    lib, check, ptr = _abi()
    B, rows, hidden, A = 8, 64, (65, 20, 10), 2
    hp = O.Hyper(1e-2, 5e-2, 0.9, 0.5, 0.25)
    specs, P0, episodes, _i, _b = L.host_case(GL.SHAPE, B, 1, 4, hidden, "tanh", rows=rows)
    u8 = lambda x: np.rint(np.asarray(x, np.float32) * 255).astype(np.uint8)
    episodes = [(u8(f), [(a, r, u8(s2)) for a, r, s2 in seq]) for f, seq in episodes]

    def restated(P, dt):
        ref = L.with_feature_norm(Bc.BcDDPG)(specs[0], specs[1], P[0], P[1], dt, hp, "GradientDescent", {}, 1, None, alpha=Bc.ALPHA, q_floor=Bc.Q_FLOOR)
        ref.set_targets(P[2], P[3])
        return ref
    agent = GL._agent(B, hidden, "tanh", hp, P0, episodes, rows=rows, sample_seed=5, prioritized_replay=True, priority_alpha=0.6, priority_beta=0.4,
                      priority_eps=1e-6, n_step=3, replay_store="u8", bc_alpha=Bc.ALPHA)
    try:
        rm = agent.replay_memory
        rm.enable_random_shift(2, seed=9)
        agent.train_step(B, 1)
        agent.train_step(B, 1)
        P = GL._params(agent)
        census = _profiled_calls(agent.actor.ctx, lambda: agent.train_step(B, 1))
        assert (census.get("heads", 0), census.get("bc", 0), census.get("ln_fwd", 0), census.get("ln_bwd", 0)) == (0, 1, 1, 2), census
        idxs = np.empty(B, np.int32)
        check(lib.cpp_replay_last_indexes(rm.handle, B, ptr(idxs)))
        w = rm.last_weights(B).astype(np.float64).reshape(B, 1)
        t, _un, _sh = _shifted_minibatch(rm, idxs)
        actions, dq_da, q, td = agent.trainer.last_values(B)
        lam, m, g, bc_rows = agent.trainer.last_behaviour_cloning(B)
        g_a = agent.actor.get_grads()
        stats = agent.trainer.last_stats()
        got = GL._params(agent)
        routes = GL._routes(agent, B)
    finally:
        agent.close()
    mask = np.asarray(t[3]).ravel()
    assert np.ptp(w) > 1e-3 and ((mask > 0) & (mask < 1)).any(), (w.ravel(), mask)      # (weights that differ; folded masks: discount^2)
    upd = {}
    for dt in (np.float64, np.float32):
        ref = restated(P, dt)
        (ref.actor.amax_override, ref.actor.relu_override), (ref.critic.amax_override, ref.critic.relu_override) = routes
        ref.fed = t[1]
        ag, cg = ref.actor_gradients(t[0]), ref.critic_gradients(t)
        ca, na = O.clip_by_global_norm(ag["grads"], hp.gradient_clip, dt)
        upd[dt] = [np.asarray(P[0].astype(dt) - dt(hp.actor_lr) * ca, np.float64)]
        if dt is np.float64:
            assert ag["m"] >= Bc.M_MIN and abs(ag["m"] - Bc.Q_FLOOR) >= Bc.FLOOR_GAP * Bc.Q_FLOOR, ag["m"]
            err = {"actions": np.abs(actions - ag["actions"]).max(), "dq_da": np.abs(dq_da - ag["dq_da"]).max(), "q": np.abs(q - cg["q"]).max(),
                   "td": np.abs(td - cg["td"]).max(), "loss": abs(stats[0] - float((w * cg["td"] ** 2).mean())), "m": abs(m - ag["m"]),
                   "bc_rows": np.abs(bc_rows - ag["bc_rows"]).max(),
                   "lambda / bar": abs(lam - ag["lambda"]) / Bc.lambda_bar(ag["lambda"], ag["m"]),
                   "g / bar": float((np.abs(g - ag["g"]) / Bc.g_bar(ag["lambda"], ag["m"], ag["dq_da"], A)).max())}
            print("layer norm + per + n-step + u8 + shift: m %.4f lambda %.4f %s" % (ag["m"], ag["lambda"], {k: "%.2e" % v for k, v in err.items()}))
            assert max(err[k] for k in ("actions", "dq_da", "q", "td", "loss")) < Bc.P_BAR and err["bc_rows"] < 4 * Bc.P_BAR, err
            assert err["m"] <= Bc.P_BAR + Bc.M_REL * ag["m"] and err["lambda / bar"] <= 1.0 and err["g / bar"] <= 1.0, err
            assert_flat_close(specs[0], g_a, ag["grads"], rel=2e-5, what="actor pre-clip grads vs f64")
            assert na > 1.2 * hp.gradient_clip and abs(stats[1] - na) < 1e-4 * max(1.0, na), (stats, na)
    rs = twin_rs(upd[np.float64], upd[np.float32], P[:1])
    e, bound = float(np.linalg.norm(got[0].astype(np.float64) - upd[np.float64][0])), delta_bound(P[0], upd[np.float64][0] - P[0], rs[0], 1)
    print("  actor |err| %.3e  bound %.3e" % (e, bound))
    assert e <= bound, (e, bound)


def test_the_eight_bit_store_changes_nothing():
    _run_case("A2-B5-smoothed", replay_store="u8")          # (the cases' frames are pixel codes: the same minibatches)


# ---- 3. the bit identities
def _digest(agent):
    h = hashlib.sha256()
    for x in _params(agent) + _slots(agent)[0]:
        h.update(np.ascontiguousarray(x).tobytes())
    return h.hexdigest()


GRAPH = ("A2-B7-delay2", 3, 3, 0)          # case, minibatches per outer step, outer steps, sample seed


def _graph_run(mode, on=True, census=False):
    """three outer steps of three minibatches on the rows the device draws (the eager pass and the capture, two replays); mode 'rows': the same
    rows handed in, which runs every minibatch eagerly; 'dp': the data-parallel step as a world of one"""
    cid, nb, steps, seed = GRAPH
    case = Bc.case_of(cid)
    B = case[3]
    inputs = Bc.case_inputs(case)
    lib, check, _ptr = _abi()
    agent = _agent(case, inputs, on=on, sample_seed=seed)
    counts = None
    try:
        for s in range(steps):
            if census and s == steps - 1:
                counts = _profiled_calls(agent.actor.ctx, lambda: agent.train_step(B, nb))
            elif mode == "graph":
                agent.train_step(B, nb)
            elif mode == "rows":
                rows = np.concatenate([T3.device_rows(seed, k, B, Bc.rows_of(case)) for k in range(s * nb, (s + 1) * nb)])
                agent.train_step(B, nb, idxs=rows)
            else:
                check(lib.cpp_ddpg_dp_train_step(agent.trainer.handle, agent.replay_memory.handle, None, B, nb, seed, 1, 0))
        out = _digest(agent)
        vals = agent.trainer.last_behaviour_cloning(B) if on else None
    finally:
        agent.close()
    return out, vals, counts


def test_graph_replays_eager_steps_repeated_runs_and_the_data_parallel_step_agree_to_the_bit():
    graph = [_graph_run("graph") for _ in range(2)]
    assert graph[0][0] == graph[1][0]
    assert graph[0][1][:2] == graph[1][1][:2] and all(np.array_equal(a, b) for a, b in zip(graph[0][1][2:], graph[1][1][2:]))
    eager, dp = _graph_run("rows"), _graph_run("dp")
    assert eager[0] == graph[0][0], "a replayed graph leaves other bits than the eager step on the same rows"
    assert eager[1][:2] == graph[0][1][:2] and np.array_equal(eager[1][2], graph[0][1][2])
    assert dp[0] == graph[0][0], "the data-parallel step as a world of one leaves other bits"


def test_off_means_off_and_the_launch_census():
    """a trainer switched on and off again before its first step against one that never had the switch: bit for bit over three outer steps
    (the eager pass and the capture, two replays), and launch for launch; with the switch on: no heads launch, one bc launch per minibatch"""
    cid, nb, steps, seed = GRAPH
    case = Bc.case_of(cid)
    B = case[3]
    inputs = Bc.case_inputs(case)

    def run(first_on):
        agent = _agent(case, inputs, on=False, sample_seed=seed)
        try:
            if first_on:
                agent.trainer.set_behaviour_cloning(Bc.ALPHA, Bc.Q_FLOOR)
                agent.trainer.set_behaviour_cloning(0.0, Bc.Q_FLOOR)
                assert agent.trainer.behaviour_cloning[0] == 0.0
            for _ in range(steps - 1):
                agent.train_step(B, nb)
            census = _profiled_calls(agent.actor.ctx, lambda: agent.train_step(B, nb))
            return _digest(agent), census
        finally:
            agent.close()
    never, toggled = run(False), run(True)
    assert never == toggled
    on = _graph_run("graph", census=True)
    assert on[0] != never[0]
    print("off:", never[1], "\non:", on[2])
    assert never[1].get("heads", 0) == nb and never[1].get("bc", 0) == 0
    assert on[2].get("heads", 0) == 0 and on[2]["bc"] == nb


def test_the_census_is_the_gemm_level_steps_plus_one_launch_and_one_level_per_minibatch():
    """the low-dimensional pair takes the GEMM levels with the term off as well: with it on every kernel family launches what it launched,
    bc once per minibatch (the action-columns GEMM runs with GE_NONE in place of GE_ACTOR_HEAD: the same launch), and the batched GEMM
    launches are one more per minibatch: bc's level holds none of the actor's GEMMs while the critic's backward still fills it, and the
    actor's backward, the pass's longest chain, ends one level later"""
    case = Bc.case_of("lowdim-A3-B5")
    B, nb = case[3], 3
    inputs = Bc.case_inputs(case)
    census = {}
    for on in (False, True):
        agent = _agent(case, inputs, on=on, sample_seed=0)
        try:
            agent.train_step(B, nb)
            census[on] = _profiled_calls(agent.actor.ctx, lambda: agent.train_step(B, nb))
        finally:
            agent.close()
    print(census)
    assert census[False].get("heads", 0) == 0 and census[True].pop("bc") == nb
    assert census[True].pop("gemm") == census[False].pop("gemm") + nb and census[True] == census[False], census


def test_an_enabled_run_leaves_nothing_behind():
    """enabled, one outer step, switched off, parameters, targets and slots put back: the following steps are those of a trainer that never
    had the switch, bit for bit (the graphs captured with the term are dropped, the buffers it allocated are not read)"""
    cid, nb, _steps, seed = GRAPH
    case = Bc.case_of(cid)
    B = case[3]
    inputs = Bc.case_inputs(case)
    digests = []
    for enabled_first in (False, True):
        agent = _agent(case, inputs, on=False, sample_seed=seed)
        try:
            t = agent.trainer
            if enabled_first:
                t.set_behaviour_cloning(Bc.ALPHA, Bc.Q_FLOOR)
            agent.train_step(B, nb)
            if enabled_first:
                assert t.last_behaviour_cloning(B)[0] > 0
                t.set_behaviour_cloning(0.0, Bc.Q_FLOOR)
            for net, p in zip(agent.networks(), inputs[1]):
                net.set_params(p)
            st = t.get_optimiser_state()
            t.set_optimiser_state(dict(st, m=np.zeros_like(st["m"]), v=np.zeros_like(st["v"]), step=np.zeros_like(st["step"])))
            t.set_policy_delay(2)          # (zeroes the delay's count)
            agent.train_step(B, nb)
            agent.train_step(B, nb)
            digests.append(_digest(agent))
        finally:
            agent.close()
    assert digests[0] == digests[1]


def test_the_paired_literal_loop_is_the_fused_step_bit_for_bit():
    """actor.train(batch.state_1); critic.train(batch) on a device-resident batch run as ONE cpp_ddpg_train_rows -- against
    train_step(B, 1, idxs) on the same rows, per minibatch, to the bit; the Batch's device copy carries the actions"""
    case = Bc.case_of("A2-B5-smoothed")
    B = case[3]
    inputs = Bc.case_inputs(case)
    lit, fused = _agent(case, inputs), _agent(case, inputs)
    try:
        np.random.seed(99)
        for step in range(1, 4):
            batch = lit.replay_memory.batch(B)
            lit.actor.train(batch.state_1)
            lit.critic.train(batch)
            lit.target_actor.update_weights()
            lit.target_critic.update_weights()
            fused.train_step(B, 1, idxs=batch.idxs)
            for a, b in zip(_params(lit) + list(lit.trainer.last_behaviour_cloning(B)) + list(lit.trainer.last_values(B)),
                            _params(fused) + list(fused.trainer.last_behaviour_cloning(B)) + list(fused.trainer.last_values(B))):
                assert np.array_equal(a, b), step
        assert lit.trainer.fused_pairs == 3 and _digest(lit) == _digest(fused)
        # ... and flushed: the actor's op alone on the state column of a Batch, whose device copy carries the actions -- against the op on
        # the same columns as host arrays
        batch = lit.replay_memory.batch(B)
        lit.actor.train(batch.state_1)
        lit.trainer.flush()
        lam = lit.trainer.last_behaviour_cloning(B)
        fused.actor.train(HostBatch(np.asarray(batch.state_1), np.asarray(batch.action), np.asarray(batch.reward), np.asarray(batch.terminal_mask),
                                    np.asarray(batch.state_2)))
        assert lit.trainer.fused_pairs == 3
        # (the gathered copy and the uploaded one take their whitening tables from different kernels: each within its bar of the truth)
        other = fused.trainer.last_behaviour_cloning(B)
        dq = np.abs(fused.trainer.last_values(B)[1]).astype(np.float64)
        assert abs(lam[0] - other[0]) <= 2 * Bc.lambda_bar(other[0], other[1])
        assert (np.abs(lam[2] - other[2]) <= 2 * Bc.g_bar(other[0], other[1], dq, case[2])).all()
        assert not np.array_equal(lit.actor.get_params(), _params(fused)[1]) and lit.trainer.fused_pairs == 3
    finally:
        lit.close(); fused.close()


@pytest.mark.parametrize("cid", ["A2-B7-adam-clipped", "A2-B7-twin-min", "lowdim-A3-B5"])
def test_the_single_ops_are_the_pass_byte_for_byte(cid):
    """cpp_ddpg_q_gradients_wrt_actions and cpp_ddpg_train_actor run the actor's half alone: lambda, m, g, the rows, dq_da, a and the actor's
    list are cpp_ddpg_compute_gradients' on the same minibatch, byte for byte; the reported dq_da is the unscaled dQ/da"""
    case = Bc.case_of(cid)
    A, B = case[2], case[3]
    inputs = Bc.case_inputs(case)
    specs, P, _ep, _idxs, batches = inputs
    lib, check, ptr = _abi()
    hb = HostBatch(*batches[0])
    agent = _agent(case, inputs)
    try:
        t = agent.trainer
        dev = t.device_batch_for(hb)
        check(lib.cpp_ddpg_compute_gradients(t.handle, dev.handle))
        whole = list(t.last_values(B)[:2]) + list(t.last_behaviour_cloning(B)) + [agent.actor.get_grads()]
        dq = agent.critic.q_gradients_wrt_actions(hb)
        half = [t.last_values(B)[0], dq] + list(t.last_behaviour_cloning(B)) + [agent.actor.get_grads()]
        before = agent.actor.get_params()
        agent.actor.train(hb)          # (a Batch-like with its actions; the host STATE array is refused: test_the_refusals)
        trained = list(t.last_behaviour_cloning(B)) + [agent.actor.get_grads()]
        assert not np.array_equal(before, agent.actor.get_params())
    finally:
        agent.close()
    for name, a, b in zip(("actions", "dq_da", "lambda", "m", "g", "bc_rows", "actor's list"), whole, half):
        assert np.array_equal(a, b), (cid, name)
    for name, a, b in zip(("lambda", "m", "g", "bc_rows", "actor's list"), whole[2:], trained):
        assert np.array_equal(a, b), (cid, name)
    ref = Bc.restatement(case, specs, P)
    ref.fed = batches[0][1]
    ag = ref.actor_gradients(batches[0][0])
    assert np.abs(half[1] - ag["dq_da"]).max() < Bc.P_BAR          # unscaled: lambda is far from 1 on these cases
    assert abs(ag["lambda"] - 1.0) > 0.5 and np.abs(ag["lambda"] * ag["dq_da"] - ag["dq_da"]).max() > 10 * Bc.P_BAR


# ---- 4. the refusals
def test_the_refusals():
    lib, _check, ptr = _abi()
    case = Bc.case_of("lowdim-A3-B5")
    A, B = case[2], case[3]
    inputs = Bc.case_inputs(case)
    agent = _agent(case, inputs, on=False)
    try:
        t = agent.trainer
        h = t.handle
        buf = np.empty(B * A, np.float32)
        assert lib.cpp_ddpg_last_behaviour_cloning(h, B, ptr(buf), None, None, None) == CPP_ERR_STATE          # (off)
        bad = ((-1.0, 1e-3), (2.5, 0.0), (2.5, -1.0), (float("nan"), 1e-3), (float("inf"), 1e-3), (2.5, float("nan")), (2.5, float("inf")))
        for alpha, floor in bad:
            assert lib.cpp_ddpg_set_behaviour_cloning(h, alpha, floor) == CPP_ERR_ARG, (alpha, floor)
        assert lib.cpp_ddpg_last_behaviour_cloning(h, B, ptr(buf), None, None, None) == CPP_ERR_STATE          # nothing was written
        assert lib.cpp_ddpg_set_behaviour_cloning(None, 2.5, 1e-3) == CPP_ERR_ARG
        t.set_behaviour_cloning(2.5, 1e-3)
        for alpha, floor in bad:      # ... nor now: the trainer keeps 2.5 and 1e-3
            assert lib.cpp_ddpg_set_behaviour_cloning(h, alpha, floor) == CPP_ERR_ARG, (alpha, floor)
        assert lib.cpp_ddpg_last_behaviour_cloning(h, B + 1, None, None, None, None) == CPP_ERR_ARG
        assert lib.cpp_ddpg_last_behaviour_cloning(h, B, None, None, None, None) == 0          # (NULL pointers are skipped)
        hb = HostBatch(*inputs[4][0])
        with pytest.raises(ValueError) as e:
            agent.actor.train(hb.state_1)
        assert "actions" in str(e.value)
        agent.actor.train(hb)
        lam = t.last_behaviour_cloning(B)[0]
        ref = Bc.restatement(case, inputs[0], inputs[1])
        ref.fed = hb.action
        want = ref.actor_gradients(hb.state_1)
        assert abs(lam - want["lambda"]) <= Bc.lambda_bar(want["lambda"], want["m"])          # (2.5 and 1e-3 survived the refused calls)
    finally:
        agent.close()
    from cartpoleplusplus_amd import ddpg_cartpole as D
    for kw in (dict(soft_actor_critic=True), dict(distributional_critic=True, v_min=0.0, v_max=1.0), dict(quantile_critic=True)):
        other = _build(Bc.SHAPES["lowdim28"], B, A, Bc.hyper_of(case), twin=False, **kw)
        try:
            assert lib.cpp_ddpg_set_behaviour_cloning(other.trainer.handle, 2.5, 1e-3) == CPP_ERR_ARG, kw
            assert lib.cpp_ddpg_set_behaviour_cloning(other.trainer.handle, 0.0, 1e-3) == CPP_ERR_ARG, kw
        finally:
            other.close()
    with pytest.raises(SystemExit):
        D.main(["--synthetic-env", "--use-raw-pixels", "--render-width", "16", "--render-height", "16", "--bc-q-floor", "0.5"])


def test_a_critic_whose_q_is_zero_leaves_every_parameter_finite():
    """the q layer zeroed: Q is exactly 0 on every row, m = 0, lambda = alpha / q_floor; dQ/da is 0 too, so the step is the cloning term's"""
    case = Bc.case_of("A2-B5-smoothed")
    B = case[3]
    inputs = Bc.case_inputs(case)
    specs, P, _ep, idxs, _b = inputs
    P = [p.copy() for p in P]
    nq = 50 + 1          # q_value's weights and bias: the last variables of the pixel critic's layout
    assert [n for n, _s in specs[1].layout()][-2:] == ["q_value/weights", "q_value/biases"]
    P[1][-nq:] = 0.0
    agent = _agent(case, (specs, P) + tuple(inputs[2:]))
    try:
        agent.train_step(B, 1, idxs=idxs[:B])
        lam, m, g, _rows = agent.trainer.last_behaviour_cloning(B)
        actions, dq_da, _q, _td = agent.trainer.last_values(B)
        assert m == 0.0 and abs(lam - Bc.ALPHA / Bc.Q_FLOOR) <= Bc.LAMBDA_REL * Bc.ALPHA / Bc.Q_FLOOR and not dq_da.any()
        assert all(np.isfinite(p).all() for p in _params(agent)) and np.isfinite(g).all()
        assert not np.array_equal(agent.actor.get_params(), P[0])
    finally:
        agent.close()


def test_a_trainer_without_the_flag_makes_neither_call(monkeypatch):
    from cartpoleplusplus_amd import ddpg_cartpole as D
    calls = []
    for name in ("cpp_ddpg_set_behaviour_cloning", "cpp_ddpg_last_behaviour_cloning"):
        real = getattr(D.lib, name)
        monkeypatch.setattr(D.lib, name, lambda *a, _n=name, _r=real: calls.append(_n) or _r(*a))
    case = Bc.case_of("A1-B5-sgd")
    inputs = Bc.case_inputs(case)
    for on, want in ((False, []), (True, ["cpp_ddpg_set_behaviour_cloning"])):
        del calls[:]
        agent = _agent(case, inputs, on=on)
        try:
            agent.train_step(case[3], 1, idxs=inputs[3][:case[3]])
        finally:
            agent.close()
        assert calls == want


def test_the_offline_recipe_trains_through_main(capsys, tmp_path):
    """the README's offline command line: an event log written by a short run on the stand-in environment, then TD3+BC from it alone"""
    from cartpoleplusplus_amd import ddpg_cartpole as D
    log = str(tmp_path / "events.log")
    common = ["--synthetic-env", "--use-raw-pixels", "--render-width", "16", "--render-height", "16", "--max-episode-len", "12", "--batch-size", "8",
              "--batches-per-step", "2", "--replay-memory-size", "200", "--replay-memory-burn-in", "20"]
    D.main(common + ["--max-num-actions", "60", "--event-log-out", log])
    capsys.readouterr()
    D.main(common + ["--event-log-in", log, "--dont-do-rollouts", "--twin-q", "--target-policy-noise", "0.2",
                     "--policy-delay", "2", "--ddpg-optimiser", "Adam", "--bc-alpha", "2.5"])
    out = capsys.readouterr()
    assert "bc_alpha=2.5" in out.err
