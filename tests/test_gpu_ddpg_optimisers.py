"""Momentum and Adam for the DDPG learner on the device (--ddpg-optimiser; cpp_ddpg_set_optimiser) against the float64 restatement
tests/ddpg_opt_np.py.  The cases, their tolerances and what they can see are that module's and tests/test_ddpg_optimiser_host.py's:
every case's float32 twin stays inside the bounds used here, and every planted fault leaves them.

Tolerances: per vector (the four parameter vectors, m, v) 2^-23 * nb * |theta| + r * |delta_f64| with r = 5e-5, the
delta-relative bound of tests/test_gpu_hyperparameters.py at its floor; parameters and targets besides at rel 2e-5 of the vector
(tests/test_gpu_naf.py).  Step counts, and every bit identity, exactly."""
import ctypes
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle import ddpg_np as O
from tests import ddpg_opt_np as R
from tests.helpers import (_profiled_calls, delta_bound, device_pool_codes, device_relu_active, hyper_options, make_pair)
from tests.test_gpu_hyperparameters import _pair_from_host_case, _params

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _opt_kw(opt):
    name, args = R.OPTIMISERS[opt]
    return dict(ddpg_optimiser=name, ddpg_optimiser_args=json.dumps(args))


def _state(agent):
    st = agent.trainer.get_optimiser_state()
    return [st["m"].astype(np.float64), st["v"].astype(np.float64)], [int(x) for x in st["step"]]


def _compare(cid, opt, P, got, want, nb):
    bad = []
    for name, g, w, b in zip(R.VECTORS, got, want, R.bounds(P, want, nb)):
        if name == "v" and not opt.startswith("adam"):
            assert not np.asarray(g).any()
            continue
        err = float(np.linalg.norm(np.asarray(g, np.float64) - w))
        print("  %-13s |err| %.3e  bound %.3e  (%.2f of it)" % (name, err, b, err / b))
        if not err <= b:
            bad.append((name, err, b))
        if name in R.VECTORS[:4] and not err <= R.PARAM_REL * float(np.linalg.norm(w)):
            bad.append((name, "rel", err / float(np.linalg.norm(w))))
    assert not bad, (cid, bad)


# ---- a. three minibatches in one call against the float64 restatement: parameters, targets, slots, both step counts
@pytest.mark.parametrize("cid,opt,shape_name,clip,tau", R.grid(), ids=[c[0] for c in R.grid()])
def test_three_minibatches_against_the_float64_restatement(cid, opt, shape_name, clip, tau):
    shape, B, seed = R.SHAPES[shape_name]
    hp = R.hyper_of(opt, clip, tau)
    agent, (specs, P, _ep, idxs, batches) = _pair_from_host_case(shape, B, R.NB, seed, hp, **_opt_kw(opt))
    try:
        agent.train_step(B, R.NB, idxs=idxs)
        got, stats = _params(agent), agent.trainer.last_stats()
        slots, steps = _state(agent)
    finally:
        agent.close()
    want, wsteps, outs = R.run_case(specs, P, batches, hp, opt)
    na, nc = outs[-1]["actor_norm"], outs[-1]["critic_norm"]
    print("%s: oracle norms %s" % (cid, [(round(o["actor_norm"], 3), round(o["critic_norm"], 3)) for o in outs]))
    assert abs(stats[1] - na) < 1e-4 * max(1.0, na) and abs(stats[2] - nc) < 1e-4 * max(1.0, nc), (stats, na, nc)
    assert steps == [int(x) for x in wsteps] == [R.NB, R.NB]
    _compare(cid, opt, P, got + slots, want, R.NB)


# ---- b. the literal calls: each list's own count
@pytest.mark.parametrize("shape_name", ["16x16x6", "64x64x18"])
def test_an_actor_only_call_advances_the_actors_count_alone(shape_name):
    """actor.train on host states (cpp_ddpg_train_actor: the critic's list has n = 0), then the three fused minibatches: the counts
    end at (4, 3), and the critic's third apply is corrected with t = 3, not 4 (tests/test_ddpg_optimiser_host.py: 'shared_t')"""
    shape, B, seed = R.SHAPES[shape_name]
    opt, clip, tau = "adam", 0.5, 0.25
    hp = R.hyper_of(opt, clip, tau)
    agent, (specs, P, _ep, idxs, batches) = _pair_from_host_case(shape, B, R.NB, seed, hp, **_opt_kw(opt))
    try:
        c0 = agent.critic.get_params()
        agent.actor.train(np.asarray(batches[-1][0]))
        _slots, steps = _state(agent)
        assert steps == [1, 0] and np.array_equal(agent.critic.get_params(), c0)
        nC = len(c0)
        assert not _slots[0][-nC:].any() and not _slots[1][-nC:].any() and _slots[0][:-nC].any()
        agent.train_step(B, R.NB, idxs=idxs)
        got = _params(agent)
        slots, steps = _state(agent)
    finally:
        agent.close()
    want, wsteps, _outs = R.run_case(specs, P, batches, hp, opt, actor_first=batches[-1][0])
    assert steps == [int(x) for x in wsteps] == [R.NB + 1, R.NB]
    _compare("actor-first-" + shape_name, opt, P, got + slots, want, R.NB + 1)


def test_a_critic_only_call_advances_the_critics_count_alone():
    shape, B, seed = R.SHAPES["16x16x6"]
    hp = R.hyper_of("adam", 0.5, 0.25)
    agent, (specs, P, _ep, idxs, batches) = _pair_from_host_case(shape, B, R.NB, seed, hp, **_opt_kw("adam"))
    import collections
    HostBatch = collections.namedtuple("HostBatch", "state_1 action reward terminal_mask state_2")
    try:
        a0 = agent.actor.get_params()
        for b in batches[:2]:
            agent.critic.train(HostBatch(*[np.asarray(x) for x in b]))
        got = _params(agent)
        slots, steps = _state(agent)
        assert np.array_equal(got[0], a0)
    finally:
        agent.close()
    name, args = R.OPTIMISERS["adam"]
    ref = R.restatement(specs, P, np.float64, hp, name, args)
    for b in batches[:2]:
        ref.train_critic(b)
    assert steps == [0, 2]
    want = R.vectors(ref)
    _compare("critic-only", "adam", P, got + slots, want, 2)


# ---- c. bit identities
@pytest.mark.parametrize("shape_name", ["16x16x6", "64x64x18"])
def test_momentum_zero_is_gradient_descent_bit_for_bit(shape_name):
    """momentum_accum is fmaf(0, m, g * scale) = g * scale and momentum_step is sgd_update's fmaf(-lr, ., p) -- in the update's
    workgroups, in the conv1 image rider and in the target update that rides behind both"""
    shape, B, seed = R.SHAPES[shape_name]
    hp = R.hyper_of("momentum-0.0", 0.5, 0.25)
    runs = []
    for kw in (_opt_kw("momentum-0.0"), {}):
        agent, (_s, _P, _ep, idxs, _b) = _pair_from_host_case(shape, B, R.NB, seed, hp, **kw)
        try:
            agent.train_step(B, R.NB, idxs=idxs)
            for _ in range(2):
                agent.train_step(B, 2)
            runs.append(np.concatenate(_params(agent)))
        finally:
            agent.close()
    assert np.isfinite(runs[0]).all() and np.array_equal(runs[0], runs[1])


@pytest.mark.parametrize("shape_name", ["16x16x6", "64x64x18"])
def test_the_literal_loop_is_the_fused_step_under_adam(shape_name):
    """ddpg_cartpole.py:331-337 verbatim, one minibatch per step, against train_step(B, 1, idxs) on the same rows: the same bits in
    every parameter, slot and count (tests/test_gpu_literal_loop.py shows it for GradientDescent)"""
    shape, B, seed = R.SHAPES[shape_name]
    hp = R.hyper_of("adam", 0.5, 0.25)
    lit, _c = _pair_from_host_case(shape, B, R.NB, seed, hp, **_opt_kw("adam"))
    fused, _c2 = _pair_from_host_case(shape, B, R.NB, seed, hp, **_opt_kw("adam"))
    try:
        np.random.seed(99)
        for _step in range(4):
            batch = lit.replay_memory.batch(B)
            lit.actor.train(batch.state_1)
            lit.critic.train(batch)
            lit.target_actor.update_weights()
            lit.target_critic.update_weights()
            fused.train_step(B, 1, idxs=batch.idxs)
        assert lit.trainer.fused_pairs == 4
        for a, b in zip(_params(lit), _params(fused)):
            assert np.array_equal(a, b)
        (sl, tl), (sf, tf) = _state(lit), _state(fused)
        assert tl == tf == [4, 4] and np.array_equal(sl[0], sf[0]) and np.array_equal(sl[1], sf[1])
    finally:
        lit.close(); fused.close()


@pytest.mark.parametrize("opt", ["momentum-0.5", "adam"])
def test_three_identical_runs_give_identical_bits(opt):
    """idxs=None: the eager pass, the capture and the replays -- the counts live on the device, so a replayed graph advances them"""
    shape, B, seed = R.SHAPES["64x64x18"]
    hp = R.hyper_of(opt, 0.5, 0.25)
    runs = []
    for _ in range(3):
        agent, _case = _pair_from_host_case(shape, B, 3, seed, hp, rows=60, **_opt_kw(opt))
        try:
            for _k in range(3):
                agent.train_step(B, 3)
            slots, steps = _state(agent)
            assert steps == [9, 9]
            runs.append(np.concatenate(_params(agent) + slots))
        finally:
            agent.close()
    assert np.isfinite(runs[0]).all()
    assert np.array_equal(runs[0], runs[1]) and np.array_equal(runs[0], runs[2])


_RIDER_SNIPPET = r"""
import hashlib, json, sys
import numpy as np
from tests.helpers import make_pair
shape, B = (64, 64, 3, 2, 3), 16
agent, _ref, _ = make_pair(shape, B, True, replay_size=8 * B, ddpg_optimiser="Adam",
                           ddpg_optimiser_args=json.dumps({"beta1": 0.8, "beta2": 0.9, "epsilon": 1e-3}),
                           actor_learning_rate=2e-3, critic_learning_rate=5e-3, gradient_clip=0.5, target_update_rate=0.25)
agent.replay_memory.fill_synthetic(6 * B, seed=11)
for _ in range(3):
    agent.train_step(B, 3)
agent.actor.ctx.sync()
st = agent.trainer.get_optimiser_state()
assert list(st["step"]) == [9, 9]
for name, arr in [(n.namespace, n.get_params()) for n in agent.networks()] + [("m", st["m"]), ("v", st["v"])]:
    assert np.isfinite(arr).all()
    print("DIGEST", name, hashlib.sha256(np.ascontiguousarray(arr).tobytes()).hexdigest())
agent.close()
"""


def test_the_conv1_image_rider_under_adam_is_an_arrangement_not_arithmetic():
    """nine minibatches in three calls at 64x64x18 under Adam, three arrangements of the ablation library: the rider as built;
    CPP_RIDE_IMAGE=0, conv1's forward builds its image by a launch of its own from the parameters the rider wrote (the switch of
    tests/test_gpu_fused_fullsize.py's GradientDescent / Momentum test); CPP_RIDE_IMAGE_UPDATE=0, no rider workgroups at all -- conv1's
    parameters and moments are advanced by the update's plain workgroups.  Parameters, targets and both slot vectors: the same bits."""
    got = {}
    for name, extra in (("rider", {}), ("own-launch", {"CPP_RIDE_IMAGE": "0"}), ("no-rider", {"CPP_RIDE_IMAGE_UPDATE": "0"})):
        r = subprocess.run([sys.executable, "-c", _RIDER_SNIPPET], cwd=ROOT, env=dict(os.environ, CARTPOLEPP_ABLATION="1", **extra),
                           stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=600)
        out = r.stdout.decode()
        assert r.returncode == 0, out[-1500:]
        got[name] = [l for l in out.splitlines() if l.startswith("DIGEST")]
        assert len(got[name]) == 6, out[-1500:]
    assert got["rider"] == got["own-launch"], got
    assert got["rider"] == got["no-rider"], got


# ---- d. launches
def test_adam_builds_the_conv1_image_in_the_optimisers_launch():
    """one profiled train_step(B, 3) at 64x64x18: conv1_image launches for the first minibatch only, under Adam as under
    GradientDescent (for NAF, whose gate stays, tests/test_gpu_hyperparameters.py pins the opposite)"""
    shape, B, seed = R.SHAPES["64x64x18"]
    counts = {}
    for name, kw in (("GradientDescent", {}), ("adam", _opt_kw("adam"))):
        agent, (_s, _P, _ep, idxs, _b) = _pair_from_host_case(shape, B, R.NB, seed, R.hyper_of("adam", 0.5, 0.25), **kw)
        try:
            counts[name] = _profiled_calls(agent.actor.ctx, lambda: agent.train_step(B, R.NB, idxs=idxs))
        finally:
            agent.close()
    print("conv1_image launches in train_step(B, 3):", {k: v.get("conv1_image", 0) for k, v in counts.items()})
    # 'the first minibatch only': as many as ONE profiled minibatch of a fresh agent launches, not three times that
    agent, (_s, _P, _ep, idxs, _b) = _pair_from_host_case(shape, B, R.NB, seed, R.hyper_of("adam", 0.5, 0.25), **_opt_kw("adam"))
    try:
        first = _profiled_calls(agent.actor.ctx, lambda: agent.train_step(B, 1, idxs=idxs[:B])).get("conv1_image", 0)
    finally:
        agent.close()
    assert first >= 1 and counts["adam"].get("conv1_image", 0) == first, (first, counts)
    assert counts["adam"].get("conv1_image", 0) == counts["GradientDescent"].get("conv1_image", 0), counts
    # ... and the step counts cost the fused step no launch: the same number of launches in all as under GradientDescent
    assert sum(counts["adam"].values()) == sum(counts["GradientDescent"].values()), counts


# ---- e. Adam with the replay features and on the data-parallel path: ONE minibatch against the restatement's rule
def _rows(agent, B):
    from cartpoleplusplus_amd._lib import lib, check, ptr
    rows = np.empty(B, np.int32)
    check(lib.cpp_replay_last_indexes(agent.replay_memory.handle, B, ptr(rows)))
    return rows


def _one_step_under_adam(what, step, prepare=None, per=False, shift=False, shape=(32, 32, 3, 2, 3), B=32, rows=300, seed=4):
    """warm call(s), then ONE checked minibatch of `step(agent)`: its rows read back, the minibatch rebuilt on the host by the feature's
    own restatement (tests/shift_np.py, the memory's n-step columns, the drawn weights), the float64 oracle's gradients on the device's
    routes, and tests/ddpg_opt_np.py's rule applied to them from the device's slots and counts as they stood before the step.  The
    float32 evaluation of the same update must itself sit inside the bound (else the case is void, not the device wrong)."""
    from tests.test_gpu_random_shift import _shifted_minibatch
    opt = "adam"
    hp = R.hyper_of(opt, 0.5, 0.25)
    kw = dict(prioritized_replay=True, priority_alpha=0.6, priority_beta=0.4, priority_eps=1e-6) if per else {}
    agent, _ref, (aspec, cspec) = make_pair(shape, B, True, seed=seed, replay_size=rows + 50, **dict(hyper_options(hp), **kw), **_opt_kw(opt))
    try:
        rm = agent.replay_memory
        rm.fill_synthetic(rows, seed=21 + seed)
        if prepare:
            prepare(agent)
        step(agent)
        step(agent)
        P = _params(agent)
        S0, t0 = _state(agent)
        step(agent)
        idxs = _rows(agent, B)
        w = rm.last_weights(B) if per else None
        _a, _dq, _q, td = agent.trainer.last_values(B)
        codes_a, codes_c = device_pool_codes(agent.actor, B), device_pool_codes(agent.critic, B)
        relu_a, relu_c = device_relu_active(agent.actor, B), device_relu_active(agent.critic, B)
        if shift:
            t, _un, _sh = _shifted_minibatch(rm, idxs)
        else:
            hb = rm.batch(idxs=idxs)
            t = (rm.state[hb.state_1_idx], hb.action, hb.reward, hb.terminal_mask, rm.state[hb.state_2_idx])
        got = _params(agent)
        S1, t1 = _state(agent)
    finally:
        agent.close()
    assert t0 == [2, 2] and t1 == [3, 3], (t0, t1)
    name, args = R.OPTIMISERS[opt]
    nA = len(P[0])
    upd = {}
    for dt in (np.float64, np.float32):
        ref = O.DDPG(aspec, cspec, P[0], P[1], dt, hyper=hp)
        ref.set_targets(P[2], P[3])
        ref.actor.amax_override, ref.critic.amax_override = codes_a, codes_c
        ref.actor.relu_override, ref.critic.relu_override = relu_a, relu_c
        ga = ref.actor_gradients(t[0])["grads"]
        cg = ref.critic_gradients(t)
        gc = cg["grads"] if not per else ref.critic_gradients(t, td_override=w.astype(dt).reshape(-1, 1) * cg["td"])["grads"]
        vec = []
        for which, flat, g, sl in (("actor", P[0], ga, slice(0, nA)), ("critic", P[1], gc, slice(nA, None))):
            o = R.N.make_optimiser(name, dict(args, learning_rate=getattr(hp, which + "_lr")))
            s = R.Slots(0, dt)
            s.m, s.v, s.t = S0[0][sl].astype(dt), S0[1][sl].astype(dt), t0[0 if which == "actor" else 1]
            new, _norm = R.apply_rule(o, flat.astype(dt), g, hp.gradient_clip, s, dt)
            vec.append((np.asarray(new, np.float64), np.asarray(s.m, np.float64), np.asarray(s.v, np.float64)))
        upd[dt] = [vec[0][0], vec[1][0], np.concatenate([vec[0][1], vec[1][1]]), np.concatenate([vec[0][2], vec[1][2]])]
    want, twin = upd[np.float64], upd[np.float32]
    start = [P[0], P[1], S0[0], S0[1]]
    bad = []
    for nm, g, w_, tw, p in zip(("actor", "critic", "m", "v"), [got[0], got[1], S1[0], S1[1]], want, twin, start):
        bound = delta_bound(p, w_ - p, R.R[nm], 1)
        e_twin, err = float(np.linalg.norm(tw - w_)), float(np.linalg.norm(np.asarray(g, np.float64) - w_))
        print("  %s %-7s |err| %.3e  twin %.3e  bound %.3e" % (what, nm, err, e_twin, bound))
        assert e_twin <= bound, "the float32 evaluation of this update leaves the bound itself: the case is void (%s %s)" % (what, nm)
        if not err <= bound:
            bad.append((nm, err, bound))
    assert not bad, (what, bad)
    # the targets: the soft update of the parameters the device holds (soft_update_value on the new bits), to f32 rounding
    for k in (0, 1):
        wt = O.soft_update(P[2 + k], got[k], hp.target_update_rate, np.float64)
        assert float(np.linalg.norm(got[2 + k] - wt)) <= 2.0 ** -23 * float(np.linalg.norm(wt)), (what, "target", k)


def test_adam_with_prioritized_replay():
    _one_step_under_adam("prioritized", lambda a: a.train_step(32, 1), per=True)


def test_adam_with_n_step_returns():
    from cartpoleplusplus_amd import ddpg_cartpole as D
    _one_step_under_adam("n-step", lambda a: a.train_step(32, 1), prepare=lambda a: a.replay_memory.enable_n_step(3, D.opts.discount))


def test_adam_with_random_shift():
    _one_step_under_adam("random-shift", lambda a: a.train_step(32, 1), prepare=lambda a: a.replay_memory.enable_random_shift(4, seed=11),
                         shift=True)


def _dp_step(sync_every):
    from cartpoleplusplus_amd._lib import lib, check

    def step(a):
        check(lib.cpp_ddpg_dp_train_step(a.trainer.handle, a.replay_memory.handle, None, 32, 1, 7, sync_every, 0))
    return step


def test_adam_in_the_data_parallel_step_as_a_world_of_one():
    """cpp_ddpg_dp_train_step without a communicator, gradient all-reduce mode: the captured step, whose heads kernel advances the counts"""
    _one_step_under_adam("dp-1", _dp_step(1))


def test_adam_in_the_periodic_data_parallel_step_follows_the_all_reduce_mode():
    """sync_every = 2 without a communicator: half steps followed by apply(), where a launch in front of the optimiser's advances the
    counts.  Its half steps presample the next minibatch, so the rows of the one just trained cannot be read back; the run is held to
    the all-reduce mode's (checked against the restatement above) on the same seed instead: the same rows through the same gradient
    kernels in another arrangement -- the delta bound between the two runs, the counts exactly."""
    opt, B = "adam", 32
    hp = R.hyper_of(opt, 0.5, 0.25)
    runs = []
    for sync_every in (1, 2):
        agent, _ref, _specs = make_pair((32, 32, 3, 2, 3), B, True, seed=4, replay_size=350, **dict(hyper_options(hp), **_opt_kw(opt)))
        try:
            agent.replay_memory.fill_synthetic(300, seed=25)
            P = _params(agent)
            for _ in range(3):
                _dp_step(sync_every)(agent)
            slots, steps = _state(agent)
            assert steps == [3, 3]
            runs.append(_params(agent) + slots)
        finally:
            agent.close()
    start = P + [np.zeros_like(runs[0][4]), np.zeros_like(runs[0][5])]
    for name, a, b, p in zip(R.VECTORS, runs[0], runs[1], start):
        err, bound = float(np.linalg.norm(a.astype(np.float64) - b)), delta_bound(p, a.astype(np.float64) - p, R.R[name], 3)
        print("  periodic vs all-reduce %-13s |diff| %.3e  bound %.3e" % (name, err, bound))
        assert err <= bound, (name, err, bound)


# ---- f. checkpoints
def test_a_checkpoint_under_adam_resumes_on_the_same_bits(tmp_path, capfd):
    from cartpoleplusplus_amd import util
    shape, B, seed = R.SHAPES["16x16x6"]
    hp = R.hyper_of("adam", 0.5, 0.25)

    def fresh(**kw):
        agent, case = _pair_from_host_case(shape, B, R.NB, seed, hp, rows=60, **kw)
        return agent, case[3]
    whole, idxs = fresh(**_opt_kw("adam"))
    try:
        for _ in range(3):
            whole.train_step(B, 2, idxs=idxs[:2 * B])
        saver = util.SaverUtil.__new__(util.SaverUtil)
        saver.agent, saver.ckpt_dir, saver.save_freq = whole, str(tmp_path / "adam"), 3600
        os.makedirs(saver.ckpt_dir)
        saver.force_save()
        whole.train_step(B, 2, idxs=idxs[B:3 * B])
        want = _params(whole) + _state(whole)[0]
        wsteps = _state(whole)[1]
    finally:
        whole.close()
    resumed, _ = fresh(**_opt_kw("adam"))
    try:
        util.SaverUtil(resumed, str(tmp_path / "adam"), 3600)
        assert _state(resumed)[1] == [6, 6]
        resumed.train_step(B, 2, idxs=idxs[B:3 * B])
        got = _params(resumed) + _state(resumed)[0]
        assert _state(resumed)[1] == wsteps == [8, 8]
        for g, w in zip(got, want):
            assert np.array_equal(g, w)
    finally:
        resumed.close()
    # GradientDescent: today's keys, no optimiser::*; restored under Adam it warns and the slots start from zero
    plain, _ = fresh()
    try:
        plain.train_step(B, 2, idxs=idxs[:2 * B])
        saver = util.SaverUtil.__new__(util.SaverUtil)
        saver.agent, saver.ckpt_dir, saver.save_freq = plain, str(tmp_path / "sgd"), 3600
        os.makedirs(saver.ckpt_dir)
        saver.force_save()
        pp = _params(plain)
    finally:
        plain.close()
    name = [l for l in open(str(tmp_path / "sgd" / "checkpoint"))][0].split(":", 1)[1].strip().strip('"')
    keys = list(np.load(str(tmp_path / "sgd" / (name + ".npz"))).keys())
    assert keys and not [k for k in keys if k.startswith("optimiser::")], keys
    capfd.readouterr()
    late, _ = fresh(**_opt_kw("adam"))
    try:
        util.SaverUtil(late, str(tmp_path / "sgd"), 3600)
        assert "holds no optimiser slots" in capfd.readouterr().err
        slots, steps = _state(late)
        assert steps == [0, 0] and not slots[0].any() and not slots[1].any()
        for g, w in zip(_params(late), pp):
            assert np.array_equal(g, w)
    finally:
        late.close()


def test_bad_kinds_and_ranges_are_refused():
    from cartpoleplusplus_amd._lib import lib
    shape, B, seed = R.SHAPES["16x16x6"]
    agent, _case = _pair_from_host_case(shape, B, R.NB, seed, R.hyper_of("adam", 0.5, 0.25), fill=False)
    try:
        h = agent.trainer.handle
        for bad in ((3, 0.0, 0.9, 0.999, 1e-8), (-1, 0.0, 0.9, 0.999, 1e-8), (1, -0.5, 0.9, 0.999, 1e-8), (2, 0.0, 1.0, 0.999, 1e-8),
                    (2, 0.0, 0.9, -0.1, 1e-8), (2, 0.0, 0.9, 0.999, 0.0)):
            assert lib.cpp_ddpg_set_optimiser(h, *bad) != 0, bad
        buf = np.zeros(4, np.float32)
        steps = np.zeros(2, np.uint64)
        assert lib.cpp_ddpg_get_opt_state(h, buf.ctypes.data_as(ctypes.c_void_p), None, 4, steps.ctypes.data_as(ctypes.c_void_p)) != 0      # GradientDescent: no slots
    finally:
        agent.close()
