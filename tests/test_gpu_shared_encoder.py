"""The shared conv encoder on the device (--shared-encoder; cpp_net_create_encoderless, cpp_net_set_encoder) against the float64
restatement tests/shared_encoder_np.py, minibatch by minibatch from a common start: the restatement takes over the device's parameters,
targets, slots and counts before each minibatch and is fed the device's pool / ReLU routes (a differing route accepted only at a near
tie); then a, a', Q, td, dq_da, the loss, both pre-clip norms, both pre-clip lists per variable and the parameter, target and slot
deltas must sit inside tests.shared_encoder_np's bars.  tests/test_shared_encoder_host.py holds the float32 twin inside the same bars
and every planted fault outside them by ten times, on the same cases.

Measured on an MI355X (this file's own prints; error / bar of the worst quantity per case): 8x8x6-A2-B5-sgd 0.116 (the actor's delta),
8x8x6-A1-B1-sgd 0.100, 8x8x6-A2-B7-momentum 0.130, 8x8x6-A1-B5-adam 0.038, 8x8x6-A2-B5-adam-split 0.034, 12x10x9-A2-B3-momentum 0.104,
64x64x18-A2-B8-sgd 0.205 (td), 64x64x18-A2-B8-adam-split 0.205 (td); the ablation library's GEMM levels 0.117.
The compositions (section 6): twin-actor-min 0.115, feature-layer-norm 0.157, smoothing-policy-delay-2 0.115, bc-alpha-2.5 0.115, quantile
0.114, drq-v2-64x64x18 0.102 (td), soft actor-critic with twin heads 0.115 (tests.sac_np.ratios).

Section 6 holds one whole-minibatch case of each composition the same way -- --twin-q --actor-min-q, --feature-layer-norm, smoothing
with --policy-delay 2, --bc-alpha 2.5, the quantile critic, the DrQ-v2 stack whole at 64x64x18 and soft actor-critic with twin heads --
to the existing restatement of that composition with its actors adopted onto the critics' encoders.  Section 7 is an extra: each
composition once more against the separate-trunk trainer at tied conv weights."""
import collections
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle import ddpg_np as O
from tests import shared_encoder_np as S
from tests import td3_np as T3
from tests.helpers import (FakeEnv, _profiled_calls, assert_flat_close, device_pool_codes, device_relu_active, hyper_options, make_opts,
                           pool_flips_are_near_ties, relu_flips_are_at_the_boundary)

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HostBatch = collections.namedtuple("HostBatch", "state_1 action reward terminal_mask state_2")


def _abi():
    from cartpoleplusplus_amd._lib import lib, check, ptr
    return lib, check, ptr


def _opt_kw(opt):
    name, args = S.OPTIMISERS[opt]
    return {} if name == "GradientDescent" else dict(ddpg_optimiser=name, ddpg_optimiser_args=json.dumps(args))


def _agent(case, inputs, shared=True, capacity=None, **kw):
    """a device agent holding the case's parameters and episodes (a separate-trunk agent: the episodes, its own initial parameters);
    capacity: the batch size it is built with (None: the case's)"""
    from cartpoleplusplus_amd import ddpg_cartpole as D
    _cid, shape_name, A, B, opt, _clip, hidden = case
    shape = S.SHAPES[shape_name]
    opts = dict(hyper_options(S.hyper_of(case)), replay_memory_size=S.ROWS, actor_hidden_layers=",".join(str(h) for h in hidden))
    opts.update(_opt_kw(opt))
    if shared:
        opts["shared_encoder"] = True
    opts.update(kw)
    make_opts(D, shape, B if capacity is None else int(capacity), True, **opts)
    agent = D.DeepDeterministicPolicyGradientAgent(FakeEnv(shape, A))
    try:
        agent.initialise_variables(seed=1)
        agent.post_var_init_setup()
        if inputs is not None:
            for net, p in zip(agent.networks(), inputs[1] if shared else ()):
                assert net.get_params().shape == p.shape, (net.namespace, net.get_params().shape, p.shape)
                net.set_params(p)
            for ep in inputs[2]:
                agent.replay_memory.add_episode(*ep)
            assert agent.replay_memory.size() == S.ROWS
    except Exception:
        agent.close()
        raise
    return agent


def _state(agent):
    """tests.shared_encoder_np.SharedDDPG.vectors() of the device"""
    t = agent.trainer
    f = lambda v: np.asarray(v, np.float64)
    out = {n.namespace: f(n.get_params()) for n in agent.networks()}
    n = len(out["actor"]) + len(out["critic"])
    if t.has_optimiser_slots():
        st = t.get_optimiser_state()
        assert len(st["m"]) == n
        out.update(m=f(st["m"]), v=f(st["v"]), step=[int(x) for x in st["step"]])
    else:
        out.update(m=np.zeros(n), v=np.zeros(n), step=[0, 0])
    return out


def _digest(agent):
    st = _state(agent)
    return np.concatenate([st[k] for k in S.VECTORS])


def partial_plan(case, inputs, capacity):
    """tests.helpers.capacity_plan of a case"""
    from tests.helpers import capacity_plan
    _c, shape_name, A, B, _opt, _clip, _h = case
    return capacity_plan(S.ROWS, S.SHAPES[shape_name], A, inputs[2], inputs[3], inputs[4], B, capacity)


def _minibatches(cid, batches_of=None, prepare=None, capacity=None, **kw):
    """S.NB calls of one minibatch each against the restatement and its float32 twin.  capacity=C > B: the agent is built for C rows
    and walks partial_plan's minibatches -- C rows, B, B, C -- each from the device's own state in front of it, at the same bars."""
    case = S.case_of(cid)
    _c, _sn, A, B, opt, clip, _h = case
    inputs = S.case_inputs(case)
    specs, P, _episodes, idxs, batches = inputs
    plan = [(idxs[k * B:(k + 1) * B], batches[k]) for k in range(S.NB)] if capacity is None else partial_plan(case, inputs, capacity)
    assert capacity is None or batches_of is None
    agent = _agent(case, inputs, capacity=capacity, **kw)
    if prepare is not None:
        prepare(agent)
    refs = [S.restatement(specs, P, dt, S.hyper_of(case), opt) for dt in (np.float64, np.float32)]
    worst = (0.0, None, None)
    try:
        start = _state(agent)
        want0 = S.initial_state(P)
        for key in S.VECTORS[:4]:
            np.testing.assert_array_equal(start[key], want0[key])
        for k in range(len(plan)):
            weights = None
            if batches_of is None:
                rows, batch = np.ascontiguousarray(plan[k][0], dtype=np.int32), plan[k][1]
                B = len(rows)
                # a' of the common start: the target actor's inference forward on state_2 (the target critic's trunk, then its stack)
                a2_forward = agent.target_actor.forward(np.asarray(batch[4]))
                agent.train_step(B, 1, idxs=rows)
            else:
                a2_forward = None
                agent.train_step(B, 1)
                batch, weights = batches_of(agent, k, B)
            t = agent.trainer
            acts, dq, q, td = t.last_values(B)
            stats = t.last_stats()
            got = {"actions": acts, "dq_da": dq, "q": q, "td": td, "loss": float(stats[0]), "actor_norm": float(stats[1]),
                   "critic_norm": float(stats[2]), "actor_grads": agent.actor.get_grads(), "critic_grads": agent.critic.get_grads()}
            routes = (device_pool_codes(agent.critic, B), device_relu_active(agent.critic, B))
            got_vec = _state(agent)
            outs, vecs = [], []
            for ref in refs:
                ref.set_state(start)
                ref.critic.amax_override, ref.critic.relu_override = routes
                outs.append(ref.train_minibatch(batch, weights=weights))
                ref.update_targets()
                vecs.append(ref.vectors())
            want, want_vec = outs[0], vecs[0]
            # (the device keeps no a' of a deterministic actor: its inference forward stands in where the caller's rows allow one; on the
            # device's own draw the rows are not known before the step, and a' is not among the compared keys -- Q' and td carry it)
            if a2_forward is not None:
                got["target_actions"] = a2_forward
            flips = pool_flips_are_near_ties(want["cache_critic"], routes[0], what="critic") + relu_flips_are_at_the_boundary(want["cache_critic"], routes[1], what="critic")
            r = S.ratios(specs, start, got, got_vec, want, want_vec)
            grads = {key: r.pop(key) for key in ("actor_grads", "critic_grads")}
            key = max(r, key=lambda x: r[x])
            print("%s minibatch %d: worst %s at %.3f of its bar; norms %.3f %.3f; %d route flips; gradient lists at %s of GRAD_REL; %s" %
                  (cid, k, key, r[key], got["actor_norm"], got["critic_norm"], flips, {a: "%.2f" % b for a, b in grads.items()},
                   {a: "%.2f" % b for a, b in sorted(r.items())}))
            if r[key] > worst[0]:
                worst = (float(r[key]), k, key)
            floor = 2.0 * float(np.max(np.abs(np.asarray(got["td"], np.float64).reshape(-1) - np.asarray(want["td"], np.float64).reshape(-1))))
            assert_flat_close(specs[0], got["actor_grads"], want["actor_grads"], rel=S.GRAD_REL, what="%s minibatch %d actor pre-clip grads" % (cid, k),
                              rel_of=S.f32_rel_of(specs[0], outs[1]["actor_grads"], want["actor_grads"]))
            assert_flat_close(specs[1], got["critic_grads"], want["critic_grads"], rel=S.GRAD_REL, what="%s minibatch %d critic pre-clip grads" % (cid, k),
                              abs_floor=floor, rel_of=S.f32_rel_of(specs[1], outs[1]["critic_grads"], want["critic_grads"]))
            bad = {a: b for a, b in r.items() if not b <= 1.0}
            assert not bad, (cid, k, bad)
            assert got_vec["step"] == want_vec["step"] or not agent.trainer.has_optimiser_slots()
            side = S.SIDES.get(cid)
            na, nc = got["actor_norm"], got["critic_norm"]
            if side == "below":
                assert min(na, nc) >= 1.2 * clip
            elif side == "above":
                assert max(na, nc) <= clip / 1.2
            elif side == "between":
                assert na <= clip / 1.2 and nc >= 1.2 * clip
            start = got_vec
        print("%s: worst error / bar %.3f (minibatch %s, %s)" % ((cid,) + worst))
    finally:
        agent.close()


# ---- 1. whole minibatches against the float64 restatement
@pytest.mark.parametrize("cid", [c[0] for c in S.CASES])
def test_minibatches_against_the_float64_restatement(cid):
    _minibatches(cid)


def test_minibatches_below_the_capacity_against_the_float64_restatement():
    """(C, B) = (8, 5): the critic's trunk feeding both networks at B behind a C-row minibatch, and at C again behind the B-row ones"""
    _minibatches("8x8x6-A2-B5-sgd", capacity=8)


PER = dict(alpha=0.6, eps=1e-3, beta=0.5, sample_seed=5)
SHIFT = (2, 77)


def test_prioritized_n_step_u8_random_shift_minibatches_against_the_float64_restatement():
    """a prioritized n-step 3 memory on a u8 store with --random-shift: the rows and weights are the device's draw, the images the shifted
    gather's (rebuilt on the host from the recorded shifts), the reward and mask columns the memory's n-step fold"""
    from tests.test_gpu_random_shift import _shifted_minibatch
    cid = "8x8x6-A2-B5-sgd"
    B = S.case_of(cid)[3]
    prios = 0.05 + np.random.default_rng(9).uniform(0, 2, S.ROWS)

    def batches_of(agent, k, B_):
        rm = agent.replay_memory
        lib, check, ptr = _abi()
        rows = np.empty(B_, np.int32)
        check(lib.cpp_replay_last_indexes(rm.handle, B_, ptr(rows)))
        weights = rm.last_weights(B_).astype(np.float64).reshape(B_, 1)
        assert weights.min() > 0 and abs(weights.max() - 1.0) < 1e-6
        batch, _unshifted, sh = _shifted_minibatch(rm, rows)
        assert rm.random_shift == SHIFT and sh.shape == (2, B_, 2)
        return batch, weights

    def prepare(agent):
        assert agent.replay_memory.random_shift == SHIFT      # --random-shift / --random-shift-seed reached the memory
        agent.replay_memory.update_priorities(np.arange(S.ROWS), prios)
    _minibatches(cid, batches_of=batches_of, prepare=prepare, prioritized_replay=True, priority_alpha=PER["alpha"], priority_eps=PER["eps"],
                 priority_beta=PER["beta"], priority_beta_final=PER["beta"], sample_seed=PER["sample_seed"], n_step=3, replay_store="u8",
                 random_shift=SHIFT[0], random_shift_seed=SHIFT[1])


def test_the_gemm_levels_of_the_ablation_library_against_the_float64_restatement():
    """CPP_FUSED_HEADS=0 on the ablation library (chosen at import: a process of its own): the same case on the GEMM levels"""
    env = dict(os.environ, CARTPOLEPP_ABLATION="1", CPP_FUSED_HEADS="0", PYTHONPATH=ROOT)
    cid = "8x8x6-A2-B5-sgd"
    r = subprocess.run([sys.executable, "-m", "pytest", "-q", "-x", "-s", "-p", "no:cacheprovider",
                        "%s::test_minibatches_against_the_float64_restatement[%s]" % (os.path.abspath(__file__), cid)],
                       cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True, timeout=300)
    print(r.stdout[-3000:])
    assert r.returncode == 0 and "1 passed" in r.stdout


# ---- 2. identities to the bit
FORM_CASE = "64x64x18-A2-B8-adam-split"
FORM_SEED = 11


def _run_form(form, cid=FORM_CASE, nb=2, steps=3, **kw):
    case = S.case_of(cid)
    B = case[3]
    inputs = S.case_inputs(case)
    agent = _agent(case, inputs, sample_seed=FORM_SEED, **kw)
    lib, check, ptr = _abi()
    try:
        rng = np.random.default_rng(3)
        for s in range(steps):
            if form == "graph":
                agent.train_step(B, nb)
            elif form == "eager":
                _profiled_calls(agent.actor.ctx, lambda: agent.train_step(B, nb))      # (profiling keeps the call on stream launches)
            elif form == "dp":
                check(lib.cpp_ddpg_dp_train_step(agent.trainer.handle, agent.replay_memory.handle, None, B, nb, FORM_SEED, 1, 0))
            elif form == "device-rows":
                rows = np.concatenate([T3.device_rows(FORM_SEED, k, B, S.ROWS) for k in range(s * nb, (s + 1) * nb)])
                agent.train_step(B, nb, idxs=rows)
            elif form == "literal":
                for _k in range(nb):
                    batch = agent.replay_memory.batch(B, idxs=rng.integers(0, S.ROWS, B))
                    agent.actor.train(batch.state_1)
                    agent.critic.train(batch)
                agent.target_actor.update_weights()
                agent.target_critic.update_weights()
            elif form == "rows":
                for _k in range(nb):
                    rows = rng.integers(0, S.ROWS, B).astype(np.int32)
                    check(lib.cpp_ddpg_train_rows(agent.trainer.handle, agent.replay_memory.handle, B, ptr(rows)))
                check(lib.cpp_ddpg_update_targets(agent.trainer.handle))
        if form == "literal":
            assert agent.trainer.fused_pairs == steps * nb
        out = _digest(agent)
        assert np.isfinite(out).all()
        return out
    finally:
        agent.close()


def test_graph_replays_eager_steps_repeated_runs_the_callers_rows_and_the_data_parallel_step_agree_to_the_bit():
    graph, again = _run_form("graph"), _run_form("graph")
    np.testing.assert_array_equal(graph, again)
    np.testing.assert_array_equal(graph, _run_form("eager"))
    np.testing.assert_array_equal(graph, _run_form("device-rows"))
    np.testing.assert_array_equal(graph, _run_form("dp"))


def test_the_literal_loops_deferred_pairs_are_the_fused_minibatch_on_rows_bit_for_bit():
    np.testing.assert_array_equal(_run_form("literal"), _run_form("rows"))


def test_the_single_ops_leave_the_bits_the_pass_leaves():
    """tests/test_gpu_single_ops_are_the_pass.py's comparison for a shared-encoder trainer (its agents, its batch; nine actions: the pass
    takes the GEMM levels, as the halves always do).  Byte for byte: dq_da, a, td, the actor's WHOLE list (it is fully connected) and the
    fully connected slices of the critic's.  The critic's conv slices come from other launches on the two sides (one network per launch
    against the pair's batched launch): both sides are held to the float64 restatement at tests.helpers' bar, not to each other.  The
    actor's half alone leaves the critic -- and with it the encoder -- as it was."""
    from tests import test_gpu_single_ops_are_the_pass as T
    lib, check, ptr = _abi()
    shape, A, B = T.PIXEL
    t = O.synthetic_batch(np.random.default_rng(5), B, shape, A, True)
    hb = T.HostBatch(t)
    whole, single = T._agent(shape, A, B, dict(shared_encoder=True)), T._agent(shape, A, B, dict(shared_encoder=True))
    try:
        P = [n.get_params() for n in whole.networks()]
        for p, q in zip(P, [n.get_params() for n in single.networks()]):
            assert p.tobytes() == q.tobytes()
        tr = whole.trainer
        dev = tr.device_batch_for(hb)
        seen = _profiled_calls(whole.actor.ctx, lambda: check(lib.cpp_ddpg_compute_gradients(tr.handle, dev.handle)))
        assert seen.get("heads", 0) == 0 and seen.get("gemm", 0) > 0, seen      # (the GEMM levels)
        act, dq_da, _q, td = tr.last_values(B)
        ga, gc = whole.actor.get_grads(), whole.critic.get_grads()
        dq_da1 = single.critic.q_gradients_wrt_actions(hb)
        _loss, td1, _q1 = single.critic.check_loss(hb)
        c0 = single.critic.get_params()
        half = _profiled_calls(single.actor.ctx, lambda: single.actor.train(hb.state_1))
        assert not [k for k, n in half.items() if n and ("_dw" in k or "_bwd" in k or "_dx" in k or k == "dw_reduce")], half      # no conv backward
        act1 = single.trainer.last_values(B)[0]
        ga1 = single.actor.get_grads()
        assert single.critic.get_params().tobytes() == c0.tobytes()
        single.critic.train(hb)
        gc1 = single.critic.get_grads()
    finally:
        whole.close()
        single.close()
    assert np.abs(dq_da).max() > 0 and np.abs(td).max() > 0 and np.abs(ga).max() > 0 and np.abs(gc).max() > 0
    assert dq_da1.tobytes() == dq_da.tobytes(), np.abs(dq_da1 - dq_da).max()
    assert td1.tobytes() == td.tobytes(), np.abs(td1 - td).max()
    assert act1.tobytes() == act.tobytes(), np.abs(act1 - act).max()
    assert ga1.tobytes() == ga.tobytes(), np.abs(ga1 - ga).max()
    specs = S.specs_for(shape, A)
    fc0 = S.conv_params(specs[1])
    assert gc1[fc0:].tobytes() == gc[fc0:].tobytes(), np.abs(gc1[fc0:] - gc[fc0:]).max()
    ref = S.restatement(specs, P)
    want_c = ref.critic_gradients(t)["grads"]
    for side, g in (("the pass", gc), ("critic.train", gc1)):
        T._conv_slices_against_oracle(specs[1], g, want_c, "%s: the critic's conv slices" % side)
    print("conv slices: |single - pass| max %.3e (held to the restatement each, not to each other)" % float(np.abs(gc1[:fc0] - gc[:fc0]).max()))


# ---- 3. structure
def test_the_actors_name_no_conv_variable_and_read_their_own_critics_encoder():
    case = S.case_of("8x8x6-A2-B5-sgd")
    inputs = S.case_inputs(case)
    agent = _agent(case, inputs)
    try:
        for net, p in zip((agent.actor, agent.target_actor), (inputs[1][0], inputs[1][2])):
            names = [v.name for v in net.trainable_model_vars()]
            assert names and not [n for n in names if "conv" in n], names
            assert names[0] == net.namespace + "/h0/weights:0" and net.trainable_model_vars()[0].offset == 0
            assert net.num_params == len(p) == inputs[0][0].num_params()
        assert [v.name.split("/", 1)[1] for v in agent.critic.trainable_model_vars()][:2] == ["conv1/weights:0", "conv1/biases:0"]
        s = np.asarray(inputs[4][0][0])
        a0, t0 = agent.actor.forward(s), agent.target_actor.forward(s)
        # the restatement's inference forward (the same whitening: the batch's own statistics)
        ref = S.restatement(inputs[0], inputs[1])
        np.testing.assert_allclose(a0, ref.actor.forward(s)["out"], rtol=0, atol=S.ROW_ATOL)
        np.testing.assert_allclose(t0, ref.target_actor.forward(s)["out"], rtol=0, atol=S.ROW_ATOL)
        each = agent.actor.actions_given(s)
        for i in range(len(s)):
            np.testing.assert_allclose(each[i], ref.actor.forward(s[i:i + 1])["out"][0], rtol=0, atol=S.ROW_ATOL)
        w = agent.critic.trainable_model_vars()[0]
        v = w.eval()
        v.reshape(-1)[::7] += 0.25
        w.load(v)
        assert np.abs(agent.actor.forward(s) - a0).max() > 1e-4
        np.testing.assert_array_equal(agent.target_actor.forward(s), t0)
        a1 = agent.actor.forward(s)
        w = agent.target_critic.trainable_model_vars()[0]
        v = w.eval()
        v.reshape(-1)[::7] += 0.25
        w.load(v)
        assert np.abs(agent.target_actor.forward(s) - t0).max() > 1e-4
        np.testing.assert_array_equal(agent.actor.forward(s), a1)
    finally:
        agent.close()


def test_an_actor_that_is_not_bound_refuses_to_run_and_the_abi_refuses_what_the_definition_excludes():
    from cartpoleplusplus_amd import _lib, ddpg_cartpole as D, base_network
    import ctypes as C
    lib, check, ptr = _abi()
    make_opts(D, S.SHAPES["8x8x6"], 4, True, shared_encoder=True)
    s1 = base_network.Placeholder([None] + list(S.SHAPES["8x8x6"]))
    actor = D.ActorNetwork("actor", s1, 2)
    other = D.ActorNetwork("target_actor", s1, 2)
    critic = None
    try:
        with pytest.raises(RuntimeError) as e:
            actor.forward(np.zeros((2,) + S.SHAPES["8x8x6"], np.float32))
        assert "not bound" in str(e.value) and "cpp_net_set_encoder" in str(e.value)
        enc, bound = C.c_int(), C.c_int()
        check(lib.cpp_net_encoder_info(actor.handle, C.byref(enc), C.byref(bound)))
        assert (enc.value, bound.value) == (1, 0)
        critic = D.CriticNetwork("critic", actor)
        check(lib.cpp_net_encoder_info(actor.handle, C.byref(enc), C.byref(bound)))
        assert (enc.value, bound.value) == (1, 1)
        assert actor.forward(np.zeros((2,) + S.SHAPES["8x8x6"], np.float32)).shape == (2, 2)
        # a trainer takes encoder-less actors as a pair, each bound to the critic it is created with
        hp = _lib.DdpgHyper(1e-3, 1e-2, 0.99, 5.0, 1e-3)
        h = C.c_void_p()
        assert lib.cpp_ddpg_create(actor.ctx.handle, actor.handle, critic.handle, other.handle, critic.handle, C.byref(hp), C.byref(h)) != 0
        assert "pair" in lib.cpp_last_error().decode()
        # the constructor's refusals, by name, before anything is allocated
        for change, word in ((dict(pixel=0, state_elems=28), "low-dimensional"), (dict(use_batch_norm=1), "use_batch_norm"),
                             (dict(use_dropout=1), "use_dropout"), (dict(kind=_lib.CPP_CRITIC), "kind")):
            spec = _lib.NetSpec()
            C.memmove(C.byref(spec), C.byref(actor.spec), C.sizeof(spec))
            for k, v in change.items():
                setattr(spec, k, v)
            assert lib.cpp_net_create_encoderless(actor.ctx.handle, C.byref(spec), 4, None, _lib.CPP_NORM_NONE, 0.0, C.byref(h)) != 0
            assert word in lib.cpp_last_error().decode(), (word, lib.cpp_last_error().decode())
        # binding checks geometry and max_batch
        make_opts(D, S.SHAPES["8x8x6"], 8, True, shared_encoder=True)
        big = D.ActorNetwork("big", s1, 2)
        try:
            assert lib.cpp_net_set_encoder(big.handle, critic.handle) != 0 and "max_batch" in lib.cpp_last_error().decode()
        finally:
            big.close()
        # ... action_dim, geometry, a critic with batch norm, another context, an actor with conv layers, a second binding
        make_opts(D, S.SHAPES["8x8x6"], 4, True, shared_encoder=True)
        wide = D.ActorNetwork("wide", s1, 3)
        odd = D.ActorNetwork("odd", base_network.Placeholder([None] + list(S.SHAPES["12x10x9"])), 2)
        make_opts(D, S.SHAPES["8x8x6"], 4, True)
        plain_actor = D.ActorNetwork("plain_actor", s1, 2)
        plain_critic = D.CriticNetwork("plain_critic", plain_actor)
        make_opts(D, S.SHAPES["8x8x6"], 4, True, use_batch_norm=True)
        bn_actor = D.ActorNetwork("bn_actor", s1, 2)
        bn_critic = D.CriticNetwork("bn_critic", bn_actor)
        ctx2 = _lib.Context(0)
        far = C.c_void_p()
        try:
            for a_net, c_net, word in ((wide, critic, "action_dim"), (odd, critic, "geometry"), (other, bn_critic, "batch norm"),
                                       (plain_actor, critic, "conv layers of its own"), (actor, plain_critic, "bound already")):
                assert lib.cpp_net_set_encoder(a_net.handle, c_net.handle) != 0
                assert word in lib.cpp_last_error().decode(), (word, lib.cpp_last_error().decode())
            check(lib.cpp_net_create_encoderless(ctx2.handle, C.byref(actor.spec), 4, None, _lib.CPP_NORM_NONE, 0.0, C.byref(far)))
            assert lib.cpp_net_set_encoder(far, critic.handle) != 0 and "contexts" in lib.cpp_last_error().decode()
            # one encoder-less actor beside a full one; NAF takes none
            assert lib.cpp_ddpg_create(actor.ctx.handle, actor.handle, critic.handle, plain_actor.handle, plain_critic.handle, C.byref(hp), C.byref(h)) != 0
            assert "one encoder-less actor" in lib.cpp_last_error().decode(), lib.cpp_last_error().decode()
            nhp = _lib.NafHyper(0.9, 5.0, 1e-3, _lib.CPP_OPT_SGD, 1e-3, 0.0, 0.9, 0.999, 1e-8)
            assert lib.cpp_naf_create(actor.ctx.handle, actor.handle, actor.handle, actor.handle, actor.handle, 0, C.byref(nhp), C.byref(h)) != 0
            assert "encoder-less" in lib.cpp_last_error().decode(), lib.cpp_last_error().decode()
            # a destroyed critic leaves its actor unbound: the next forward refuses instead of reading freed memory
            check(lib.cpp_net_set_encoder(other.handle, plain_critic.handle))
            plain_critic.close()
            check(lib.cpp_net_encoder_info(other.handle, C.byref(enc), C.byref(bound)))
            assert (enc.value, bound.value) == (1, 0)
            with pytest.raises(RuntimeError) as e:
                other.forward(np.zeros((2,) + S.SHAPES["8x8x6"], np.float32))
            assert "not bound" in str(e.value)
        finally:
            if far:
                lib.cpp_net_destroy(far)
            for n in (wide, odd, plain_actor, plain_critic, bn_actor, bn_critic):
                n.close()
            ctx2.close() if hasattr(ctx2, "close") else None
    finally:
        actor.close(); other.close()
        if critic is not None:
            critic.close()


@pytest.mark.parametrize("kw,word", [(dict(use_batch_norm=True), "--use-batch-norm"), (dict(use_dropout=True), "--use-dropout")])
def test_the_command_line_refuses_before_anything_exists_on_the_device(kw, word):
    from cartpoleplusplus_amd import ddpg_cartpole as D
    make_opts(D, S.SHAPES["8x8x6"], 4, True, shared_encoder=True, **kw)
    with pytest.raises(SystemExit) as e:
        D.DeepDeterministicPolicyGradientAgent(FakeEnv(S.SHAPES["8x8x6"], 2))
    assert word in str(e.value)
    make_opts(D, (2, 2, 7), 4, False, shared_encoder=True)
    with pytest.raises(SystemExit) as e:
        D.DeepDeterministicPolicyGradientAgent(FakeEnv((2, 2, 7), 2))
    assert "--use-raw-pixels" in str(e.value)


def test_a_checkpoint_round_trip_and_a_restore_across_the_option_fails_in_both_directions(tmp_path):
    from cartpoleplusplus_amd import util
    case = S.case_of("8x8x6-A2-B5-adam-split")
    inputs = S.case_inputs(case)
    B = case[3]
    shared_dir, plain_dir = str(tmp_path / "shared"), str(tmp_path / "plain")
    a = _agent(case, inputs)
    try:
        saver = util.SaverUtil(a, shared_dir, 3600)      # (no checkpoint there yet: it initialises the variables and saves)
        for net, p in zip(a.networks(), inputs[1]):
            net.set_params(p)
        a.train_step(B, 2, idxs=np.ascontiguousarray(inputs[3][:2 * B], dtype=np.int32))
        saver.force_save()
        want = _digest(a)
    finally:
        a.close()
    b = _agent(case, inputs)
    try:
        util.SaverUtil(b, shared_dir, 3600)
        np.testing.assert_array_equal(_digest(b), want)
    finally:
        b.close()
    p = _agent(case, None, shared=False)
    try:
        with pytest.raises(AssertionError) as e:
            util.SaverUtil(p, shared_dir, 3600)
        assert "does not match actor" in str(e.value)
        util.SaverUtil(p, plain_dir, 3600)
    finally:
        p.close()
    c = _agent(case, inputs)
    try:
        with pytest.raises(AssertionError) as e:
            util.SaverUtil(c, plain_dir, 3600)
        assert "does not match actor" in str(e.value)
    finally:
        c.close()


# ---- 4. the census of an outer step against the plain step
def _census(cid, nb=3, shared=True, **kw):
    case = S.case_of(cid)
    B = case[3]
    agent = _agent(case, None, shared=shared, sample_seed=3, **kw)      # (its own initial parameters: a census reads no value)
    try:
        for ep in S.case_inputs(case)[2]:
            agent.replay_memory.add_episode(*ep)
        agent.train_step(B, nb)      # (the first call builds what later calls find built)
        calls = _profiled_calls(agent.actor.ctx, lambda: agent.train_step(B, nb))
        return {k: n for k, n in calls.items() if n}, _digest(agent)
    finally:
        agent.close()


@pytest.mark.parametrize("cid", ["8x8x6-A2-B5-sgd", "64x64x18-A2-B8-sgd"])
def test_no_kernel_family_launches_more_than_in_the_plain_step(cid):
    plain, _d = _census(cid, shared=False)
    shared, _d = _census(cid)
    print("%s: plain %s\n%s: shared %s" % (cid, sorted(plain.items()), cid, sorted(shared.items())))
    more = {k: (n, plain.get(k, 0)) for k, n in shared.items() if n > plain.get(k, 0)}
    assert not more, more
    assert sum(shared.values()) <= sum(plain.values())


def test_soft_actor_critic_builds_one_conv1_image_per_outer_step():
    """the separate-trunk SAC step rebuilds the target actor's conv1 operand image in every minibatch (its parameters are copied behind
    every optimiser launch); with a shared encoder the target actor has no conv1"""
    cid, nb = "64x64x18-A2-B8-sgd", 3
    kw = dict(soft_actor_critic=True, twin_q=True, actor_min_q=True)
    plain, _d = _census(cid, nb=nb, shared=False, **kw)
    shared, _d = _census(cid, nb=nb, **kw)
    print("plain SAC %s\nshared SAC %s" % (sorted(plain.items()), sorted(shared.items())))
    image = [k for k in plain if "image" in k]
    assert image, sorted(plain)
    assert sum(plain[k] for k in image) >= nb and sum(shared.get(k, 0) for k in image) <= 1


# ---- 5. off means off
_OFF_SNIPPET = r"""
import hashlib, json, sys
import numpy as np
from tests import shared_encoder_np as S
from tests.test_gpu_shared_encoder import _agent, _census
cid = "64x64x18-A2-B8-sgd"
if sys.argv[1] == "after":
    case = S.case_of(cid)
    a = _agent(case, S.case_inputs(case))
    a.train_step(case[3], 2)
    a.train_step(case[3], 2)
    a.close()
calls, digest = _census(cid, shared=False)
print("RESULT " + json.dumps({"calls": sorted(calls.items()), "bits": hashlib.sha256(np.asarray(digest, np.float64).tobytes()).hexdigest()}))
"""


def test_a_plain_trainer_behind_a_shared_encoder_trainer_is_a_fresh_processs_plain_trainer():
    out = []
    for mode in ("fresh", "after"):
        r = subprocess.run([sys.executable, "-c", _OFF_SNIPPET, mode], cwd=ROOT, env=dict(os.environ, PYTHONPATH=ROOT), stdout=subprocess.PIPE,
                           stderr=subprocess.STDOUT, universal_newlines=True, timeout=300)
        assert r.returncode == 0, r.stdout[-3000:]
        out.append(json.loads([l for l in r.stdout.splitlines() if l.startswith("RESULT ")][-1][7:]))
    assert out[0] == out[1], out


# ---- 6. the compositions, each against its float64 restatement on a shared encoder
def _comp_agent(name, inputs):
    _kind, shape_name, A, B, opt, clip, _d, _sm, kw = S.COMPOSITIONS[name]
    agent = _agent((name, shape_name, A, B, opt, clip, S.DEFAULT_ACTOR_HIDDEN), None, **kw)
    try:
        for net, p in zip(agent.networks(), inputs["P"]):
            assert net.get_params().shape == p.shape, (net.namespace, net.get_params().shape, p.shape)
            net.set_params(p)
        for ep in inputs["episodes"]:
            agent.replay_memory.add_episode(*ep)
        assert agent.replay_memory.size() == S.ROWS
    except Exception:
        agent.close()
        raise
    return agent


@pytest.mark.parametrize("name", list(S.COMPOSITIONS))
def test_a_composition_against_its_float64_restatement(name):
    """S.NB calls of one minibatch each on the caller's rows, from a common start: the existing restatement of the composition with its
    actors adopted onto the critics' encoders (tests.shared_encoder_np.comp_restatement) takes over the device's state and is fed the
    device's routes and -- where the target is smoothed -- the device's clipped noise, itself held to the restated draw.  Compared: a, a'
    (the target actor's inference forward on the minibatch's state_2 -- the shifted images where the memory shifts -- before the step),
    Q, td, dq_da, the loss, both pre-clip norms and lists, the four parameter vectors' and both slots' deltas, at section 1's bars."""
    from tests import shift_np
    kind, _sn, A, B, _opt, _clip, delay, smoothing, kw = S.COMPOSITIONS[name]
    inputs = S.comp_inputs(name)
    specs, idxs = inputs["layout"], inputs["idxs"]
    pad = kw.get("random_shift", 0)
    agent = _comp_agent(name, inputs)
    refs = [S.comp_restatement(name, inputs, dt) for dt in (np.float64, np.float32)]
    worst = (0.0, None, None)
    try:
        rm, t = agent.replay_memory, agent.trainer
        start = _state(agent)
        want0 = S.comp_initial_state(inputs)
        for key in S.VECTORS[:4]:
            np.testing.assert_array_equal(start[key], want0[key])
        for k in range(S.NB):
            rows = np.ascontiguousarray(idxs[k * B:(k + 1) * B], dtype=np.int32)
            hb = rm.batch(idxs=rows)      # (the memory's own columns: an n-step memory folds them)
            s1, s2 = rm.state[hb.state_1_idx], rm.state[hb.state_2_idx]
            if pad:
                sh = shift_np.shifts(S.COMP_SHIFT[1], k, B, pad)
                s1, s2 = shift_np.shift_images(s1, sh[0]), shift_np.shift_images(s2, sh[1])
            batch = (s1, hb.action, hb.reward, hb.terminal_mask, s2)
            if not pad and kw.get("n_step", 1) == 1:
                for x, y in zip(batch, inputs["batches"][k]):
                    np.testing.assert_array_equal(np.asarray(x, np.float32).reshape(-1), np.asarray(y, np.float32).reshape(-1))
            a2_forward = agent.target_actor.forward(np.asarray(s2))
            agent.train_step(B, 1, idxs=rows)
            if pad:
                assert np.array_equal(rm.last_shifts(B), sh)
            eps = None
            if smoothing is not None:
                eps, n = t.last_target_noise(B)
                assert n == k and float(np.max(np.abs(eps - S.comp_noise(name, k, B, A)))) <= S.ROW_ATOL, (n, k)
            acts, dq, q, td = t.last_values(B)
            stats = t.last_stats()
            got = {"actions": acts, "target_actions": a2_forward, "dq_da": dq, "q": q, "td": td, "loss": float(stats[0]), "actor_norm": float(stats[1]),
                   "critic_norm": float(stats[2]), "actor_grads": agent.actor.get_grads(),
                   "critic_grads": S.comp_critic_to_ref(name, inputs, agent.critic.get_grads())}
            routes = (device_pool_codes(agent.critic, B), device_relu_active(agent.critic, B))
            got_vec = _state(agent)
            outs, vecs = [], []
            for ref in refs:
                S.comp_set_state(ref, name, inputs, start, k)
                outs.append(S.comp_minibatch(ref, name, inputs, batch, eps=eps, routes=routes))
                vecs.append(S.comp_vectors(ref, name, inputs))
            want, want_vec = outs[0], vecs[0]
            if delay > 1:
                assert t.policy_delay_status()[2] == (not want["applied"]), (k, t.policy_delay_status(), want["applied"])
            flips = pool_flips_are_near_ties(want["cache_critic"], routes[0], what="critic") + relu_flips_are_at_the_boundary(want["cache_critic"], routes[1], what="critic")
            r = S.ratios(specs, start, got, got_vec, want, want_vec)
            grads = {key: r.pop(key) for key in ("actor_grads", "critic_grads")}
            key = max(r, key=lambda x: r[x])
            print("%s minibatch %d: worst %s at %.3f of its bar; norms %.3f %.3f; %d route flips; gradient lists at %s of GRAD_REL; %s" %
                  (name, k, key, r[key], got["actor_norm"], got["critic_norm"], flips, {a: "%.2f" % b for a, b in grads.items()},
                   {a: "%.2f" % b for a, b in sorted(r.items())}))
            if r[key] > worst[0]:
                worst = (float(r[key]), k, key)
            floor = 2.0 * float(np.max(np.abs(np.asarray(got["td"], np.float64).reshape(-1) - np.asarray(want["td"], np.float64).reshape(-1))))
            assert_flat_close(specs[0], got["actor_grads"], want["actor_grads"], rel=S.GRAD_REL, what="%s minibatch %d actor pre-clip grads" % (name, k),
                              rel_of=S.f32_rel_of(specs[0], outs[1]["actor_grads"], want["actor_grads"]))
            assert_flat_close(specs[1], got["critic_grads"], want["critic_grads"], rel=S.GRAD_REL, what="%s minibatch %d critic pre-clip grads" % (name, k),
                              abs_floor=floor, rel_of=S.f32_rel_of(specs[1], outs[1]["critic_grads"], want["critic_grads"]))
            bad = {a: b for a, b in r.items() if not b <= 1.0}
            assert not bad, (name, k, bad)
            if t.has_optimiser_slots():
                assert got_vec["step"] == want_vec["step"]
            start = got_vec
        print("%s: worst error / bar %.3f (minibatch %s, %s)" % ((name,) + worst))
    finally:
        agent.close()


def test_soft_actor_critic_with_twin_heads_against_its_float64_restatement():
    """tests/test_gpu_sac_composed.py's run of its case 'twin-sgd-clip0.5-A2-B8' with --shared-encoder: tests.sac_np.ComposedSac with the
    two actors adopted, its bars (tests.sac_np.ratios: a, a', logp, logp', r_soft, Q1, Q2, td1, td2, dq_da, g_alpha, the loss, norms,
    lists, deltas, counts, the temperature).  (a', logp') are sampled on the TARGET critic's features: the target critic's encoder
    differs from the critic's here, and tests/test_shared_encoder_host.py shows either wrong encoder 20 000 bars away."""
    from tests import sac_np as SAC
    from tests import test_gpu_sac_composed as G
    case, inputs = S.sac_inputs()
    _cid, _sn, A, B = case[:4]
    agent = G._agent(case, inputs, shared_encoder=True)
    refs = (S.sac_restatement(case, inputs), S.sac_restatement(case, inputs, np.float32))
    try:
        assert not [v for v in agent.target_actor.trainable_model_vars() if "conv" in v.name]
        t = agent.trainer
        start = G._state(agent)
        for k in range(SAC.C_MINIBATCHES):
            rows = np.ascontiguousarray(inputs[3][k * B:(k + 1) * B], dtype=np.int32)
            agent.train_step(B, 1, idxs=rows)
            sac = t.last_sac(B)
            assert sac["n"] == k
            for key, stream in (("eps", SAC.STREAM_S1), ("eps2", SAC.STREAM_S2)):
                assert float(np.max(np.abs(sac[key] - SAC.noise(SAC.C_NOISE_SEED, k, B, A, stream)))) <= SAC.eps_bar(), key
            acts, dq, q, td = t.last_values(B)
            q2, _tq1, _tq2, td2 = t.last_twin_values(B)
            stats = t.last_stats()
            got = {"actions": sac["a"], "target_actions": sac["a2"], "q": q, "q2": q2, "td": td, "td2": td2, "dq_da": dq, "logp": sac["logp"],
                   "logp2": sac["logp2"], "r_soft": sac["r_soft"], "g_alpha": sac["g_alpha"], "loss": float(stats[0]), "actor_norm": float(stats[1]),
                   "critic_norm": float(stats[2]), "actor_grads": agent.actor.get_grads(), "critic_grads": agent.critic.get_grads()}
            codes, active = device_pool_codes(agent.critic, B), device_relu_active(agent.critic, B)
            got_vec = G._state(agent)
            np.testing.assert_array_equal(agent.target_actor.get_params(), agent.actor.get_params())
            batch = SAC.composed_batches(case, inputs[2], rows)[0]
            G._compare(case, inputs, refs, start, k, got, sac, (codes, codes, active, active), got_vec, batch, None, run=" (shared encoder)")
            start = got_vec
        print("%s with a shared encoder: worst error / bar %.3f (minibatch %d, %s)" % ((case[0],) + G.WORST[case[0] + " (shared encoder)"]))
    finally:
        agent.close()


# ---- 7. an extra: the compositions against the separate-trunk trainer at tied conv weights
COMPOSITIONS = {
    "twin-actor-min": dict(twin_q=True, actor_min_q=True),
    "feature-layer-norm": dict(feature_layer_norm=True),
    "smoothing-policy-delay-2": dict(target_policy_noise=0.2, target_policy_noise_clip=0.5, target_policy_noise_seed=7, policy_delay=2),
    "bc-alpha-2.5": dict(bc_alpha=2.5),
    "quantile": dict(quantile_critic=True, num_quantiles=8),
    "sac-twin": dict(soft_actor_critic=True, twin_q=True, actor_min_q=True, sac_seed=5),
    "drq-v2-64x64x18": dict(twin_q=True, actor_min_q=True, feature_layer_norm=True, n_step=3, target_policy_noise=0.2, target_policy_noise_seed=7,
                            random_shift=4, random_shift_seed=3, replay_store="u8", ddpg_optimiser="Adam"),
}


@pytest.mark.parametrize("name", list(COMPOSITIONS))
def test_a_composition_is_the_separate_trunk_trainer_at_tied_conv_weights(name):
    """With the actor's conv variables set to the critic's and the target actor's to the target critic's, the separate-trunk trainer
    computes the same a, a', Q, td, dq_da and loss, the same critic list (its whole update and target update), and an actor list whose
    fully connected part is the shared-encoder trainer's whole list.  Both run in float32 on the same kernels' arithmetic; each is
    inside tests.shared_encoder_np's bars around the exact values, so they are held to twice those bars of each other."""
    kw = dict(COMPOSITIONS[name])
    cid = "64x64x18-A2-B8-sgd" if name.startswith("drq-v2") else "8x8x6-A2-B5-sgd"
    case = S.case_of(cid)
    B = case[3]
    inputs = S.case_inputs(case)
    rows = np.ascontiguousarray(inputs[3][:B], dtype=np.int32)
    shared, plain = _agent(case, None, **kw), _agent(case, None, shared=False, **kw)
    try:
        nconv = S.conv_params(inputs[0][1])
        rng = np.random.default_rng(4)
        for live, target in ((shared.critic, shared.target_critic),):
            p = live.get_params()
            p = (p + rng.normal(0, 0.05, p.shape)).astype(np.float32)
            live.set_params(p)
            t = (p + rng.normal(0, 0.01, p.shape)).astype(np.float32)
            if kw.get("soft_actor_critic"):      # (the separate-trunk target actor is a copy of the actor, conv layers included: the tie needs
                t[:nconv] = p[:nconv]            # the target critic's encoder to be the critic's as well)
            target.set_params(t)
        pa = shared.actor.get_params()
        pa = (pa + rng.normal(0, 0.05, pa.shape)).astype(np.float32)
        shared.actor.set_params(pa)
        shared.target_actor.set_params(pa if kw.get("soft_actor_critic") else (pa + rng.normal(0, 0.01, pa.shape)).astype(np.float32))
        for s_net, p_net in ((shared.critic, plain.critic), (shared.target_critic, plain.target_critic)):
            p_net.set_params(s_net.get_params())
        for s_net, p_net, enc in ((shared.actor, plain.actor, shared.critic), (shared.target_actor, plain.target_actor, shared.target_critic)):
            full = p_net.get_params()
            assert len(full) == nconv + s_net.num_params
            full[:nconv], full[nconv:] = enc.get_params()[:nconv], s_net.get_params()
            p_net.set_params(full)
        if kw.get("soft_actor_critic"):
            plain.target_actor.set_params(plain.actor.get_params())
        for agent in (shared, plain):
            for ep in inputs[2]:
                agent.replay_memory.add_episode(*ep)
            agent.train_step(B, 1, idxs=rows)
        vs, vp = shared.trainer.last_values(B), plain.trainer.last_values(B)
        for what, x, y in zip(("actions", "dq_da", "q", "td"), vs, vp):
            err = float(np.max(np.abs(x.astype(np.float64) - y) / np.maximum(1.0, np.abs(y))))
            print("%s %-8s |shared - plain| %.3e (twice the bar: %.1e)" % (name, what, err, 2 * S.ROW_ATOL))
            assert err <= 2 * S.ROW_ATOL, (name, what, err)
        ss, sp = shared.trainer.last_stats(), plain.trainer.last_stats()
        assert abs(ss[0] - sp[0]) <= 2 * S.ROW_ATOL * max(1.0, abs(sp[0])) and abs(ss[2] - sp[2]) <= 2 * S.NORM_RTOL * max(1.0, sp[2]), (ss, sp)
        gs, gp = shared.actor.get_grads().astype(np.float64), plain.actor.get_grads().astype(np.float64)
        fc_norm = float(np.linalg.norm(gp[nconv:]))
        assert abs(ss[1] - fc_norm) <= 2 * S.NORM_RTOL * max(1.0, fc_norm), (ss[1], fc_norm, sp[1])      # the actor's norm is of its fully connected layers
        assert np.linalg.norm(gp[:nconv]) > 1e-3 * fc_norm                                               # (... and the plain actor's conv gradient is not nothing)
        for what, x, y in (("actor list", gs, gp[nconv:]), ("critic list", shared.critic.get_grads().astype(np.float64), plain.critic.get_grads().astype(np.float64))):
            rel = float(np.linalg.norm(x - y) / np.linalg.norm(y))
            print("%s %-11s |shared - plain| / |plain| %.3e" % (name, what, rel))
            assert rel <= 2 * S.GRAD_REL, (name, what, rel)
        for what, s_net, p_net in (("critic", shared.critic, plain.critic), ("target critic", shared.target_critic, plain.target_critic)):
            x, y = s_net.get_params().astype(np.float64), p_net.get_params().astype(np.float64)
            rel = float(np.linalg.norm(x - y) / np.linalg.norm(y))
            print("%s %-13s parameters |shared - plain| / |plain| %.3e" % (name, what, rel))
            assert rel <= 2 * S.GRAD_REL, (name, what, rel)
        # and three graph-replayed outer steps of the composition stay finite and repeat
        for _ in range(3):
            shared.train_step(B, 2)
        assert np.isfinite(_digest(shared)).all()
    finally:
        shared.close(); plain.close()
