"""Delayed policy updates without a GPU: the command line, the schedule of the float64 restatement (tests/td3_np.py), and what
tests/test_gpu_policy_delay.py can see -- on that module's own cases (the same parameters, episodes and rows, tests.helpers.host_case)
every planted fault must move a compared vector by a large multiple of the bound the GPU test applies to it, and the restatement's own
float32 run must stay inside that bound on the float64 routes (a case that does not is replaced here, on the CPU, not loosened)."""
import functools

import numpy as np
import pytest

from tests import td3_np as T3
from tests.helpers import host_case

POWER = 10.0          # "a large multiple": a fault the GPU test sees at less than ten times its bound is not counted as seen


# ---- the command line
def test_the_parser_takes_the_flag_and_the_default_is_off():
    from cartpoleplusplus_amd import ddpg_cartpole as D
    o = D.build_parser().parse_args([])
    assert not hasattr(o, "policy_delay") and D.policy_delay(o) == 1 and D.default_opts().policy_delay == 1
    assert D.policy_delay(D.build_parser().parse_args(["--policy-delay", "2"])) == 2
    assert D.policy_delay(D.default_opts(policy_delay=65536)) == 65536


@pytest.mark.parametrize("bad", [0, -1, 65537, 2.5, "2", None, True])
def test_the_parser_refuses_what_cannot_be_meant(bad):
    from cartpoleplusplus_amd import ddpg_cartpole as D
    with pytest.raises(SystemExit) as e:
        D.policy_delay(D.default_opts(policy_delay=bad))
    assert "--policy-delay" in str(e.value)


def test_the_command_line_refuses_a_delay_that_is_not_a_number():
    from cartpoleplusplus_amd import ddpg_cartpole as D
    with pytest.raises(SystemExit):
        D.build_parser().parse_args(["--policy-delay", "two"])


# ---- the schedule
@functools.lru_cache(maxsize=None)
def _case(shape_name):
    shape, B, seed = T3.SHAPES[shape_name]
    return host_case(shape, B, T3.MAX_MINIBATCHES, seed)


@pytest.mark.parametrize("d", [2, 3, 5])
@pytest.mark.parametrize("nb", [3, 5])
def test_the_schedule_over_outer_steps(d, nb):
    """three outer steps of nb minibatches: the actor's list moves with every d-th critic update, counted across the outer steps; a held
    minibatch leaves the actor, its slots and its count as they were, to the bit; the targets follow every outer step"""
    specs, P, _ep, _idxs, batches = _case("16x16x6")
    ref = T3.restatement(specs, P, np.float64, T3.hyper_of("adam", 0.5, 0.25), "adam", d)
    k = 0
    for _s in range(3):
        ta0 = ref.target_actor.flat().copy()
        for _i in range(nb):
            a0, m0, v0, t0 = ref.actor.flat().copy(), ref.slots["actor"].m.copy(), ref.slots["actor"].v.copy(), ref.slots["actor"].t
            c0 = ref.critic.flat().copy()
            out = ref.train_minibatch(batches[k % len(batches)])
            k += 1
            assert out["applied"] == (k % d == 0) and ref.held == (not out["applied"]) and out["actor_norm"] > 0
            same = np.array_equal(ref.actor.flat(), a0) and np.array_equal(ref.slots["actor"].m, m0) and np.array_equal(ref.slots["actor"].v, v0)
            assert same == (not out["applied"]) and ref.slots["actor"].t == t0 + int(out["applied"])
            assert not np.array_equal(ref.critic.flat(), c0) and ref.slots["critic"].t == k
        ref.update_targets()
        assert not np.array_equal(ref.target_actor.flat(), ta0)      # (the target actor differs from the actor: it moves even when the actor did not)
    assert ref.n == 3 * nb and ref.schedule == T3.expected_schedule(d, 3 * nb) and list(ref.state()["step"]) == [3 * nb // d, 3 * nb]


def test_a_delay_of_one_is_the_parent_restatement_bit_for_bit():
    from tests import ddpg_opt_np as R
    specs, P, _ep, _idxs, batches = _case("16x16x6")
    hp = T3.hyper_of("adam", 0.5, 0.25)
    got, steps, _o, _r = T3.run_case(specs, P, batches, hp, "adam", 1, 3, 1)
    want, wsteps, _o2 = R.run_case(specs, P, batches[:3], hp, "adam")
    assert list(steps) == list(wsteps) and all(np.array_equal(g, w) for g, w in zip(got, want))


def test_the_stand_alone_ops_keep_the_fused_schedule():
    """actor.train looks one minibatch ahead and counts nothing; critic.train counts"""
    specs, P, _ep, _idxs, batches = _case("16x16x6")
    hp = T3.hyper_of("adam", 0.5, 0.25)
    _v, steps, ref = T3.run_literal(specs, P, batches[:4], hp, "adam", 2)
    assert ref.n == 4 and list(steps) == [2, 4] and ref.schedule == [False, True, False, True]


# ---- conditioning and power, on the GPU module's cases
@functools.lru_cache(maxsize=None)
def _run(cid, dt_name="f64", fault=None):
    case = [c for c in T3.grid() if c[0] == cid][0]
    _cid, opt, shape_name, d, nb, steps, clip, tau = case
    specs, P, _ep, idxs, batches = _case(shape_name)
    _rows, batches = T3.case_batches(case, idxs, batches, T3.SHAPES[shape_name][1])
    got, counts, outs, _ref = T3.run_case(specs, P, batches, T3.hyper_of(opt, clip, tau), opt, d, nb, steps,
                                          np.float64 if dt_name == "f64" else np.float32, fault)
    return got, counts, outs


def _compared(opt):
    return [n for n in T3.VECTORS if not (n == "v" and opt != "adam") and not (n == "m" and opt == "gradient-descent")]


@pytest.mark.parametrize("case", T3.grid(), ids=[c[0] for c in T3.grid()])
def test_the_float32_twin_stays_inside_the_gpu_tolerance(case):
    cid, opt, shape_name, d, nb, steps, clip, tau = case
    _specs, P, _ep, _idxs, _b = _case(shape_name)
    want, counts, o64 = _run(cid)
    twin, _c, o32 = _run(cid, "f32")
    assert list(counts) == [steps * nb // d, steps * nb]
    assert all(np.array_equal(x, y) for a, b in zip(o64, o32) for x, y in zip(a["routes"], b["routes"])), \
        "the float32 twin and the float64 restatement take different pool / ReLU routes: choose another case"
    norms = [n for o in o64 for n in (o["actor_norm"], o["critic_norm"])]
    assert (min(norms) > clip) if clip < 1 else (max(norms) < clip), norms
    ties = [o["tie"] for o in o64]
    print("%s  closest call per minibatch %s (floor %.2e)" % (cid, ["%.2e" % t for t in ties], T3.TIE_FLOOR))
    assert min(ties) > T3.TIE_FLOOR, "a route of this case is closer to a tie than float32 can decide: choose another case"
    from tests import ddpg_opt_np as R
    for name, w, t, b in zip(T3.VECTORS, want, twin, T3.bounds(P, want, steps * nb)):
        if name not in _compared(opt):
            continue
        err = float(np.linalg.norm(t - w))
        print("%s  %-13s twin |err| %.3e  bound %.3e  (%.2f of it)" % (cid, name, err, b, err / b))
        assert err <= b, (cid, name, err, b)
        if name in T3.VECTORS[:4]:
            assert err <= R.PARAM_REL * float(np.linalg.norm(w)), (cid, name)


@pytest.mark.parametrize("case", T3.GRAPH_CASES, ids=[c[0] for c in T3.GRAPH_CASES])
def test_the_float32_twin_stays_inside_the_gpu_tolerance_on_the_rows_the_device_draws(case):
    from tests import ddpg_opt_np as R
    cid, opt, shape_name, d, nb, steps, _sample_seed = case
    specs, P, _ep, rows, batches = T3.graph_case(cid)
    assert len(batches) == steps * nb and rows.min() >= 0 and rows.max() < T3.GRAPH_ROWS
    hp = T3.hyper_of(opt, T3.GRAPH_CLIP, T3.GRAPH_TAU)
    want, counts, o64, ref = T3.run_case(specs, P, batches, hp, opt, d, nb, steps)
    twin, _c, o32, _r = T3.run_case(specs, P, batches, hp, opt, d, nb, steps, np.float32)
    assert list(counts) == [steps * nb // d, steps * nb] and ref.schedule == T3.expected_schedule(d, steps * nb)
    ties = [o["tie"] for o in o64]
    print("%s  closest call per minibatch %s (floor %.2e)" % (cid, ["%.2e" % t for t in ties], T3.TIE_FLOOR))
    assert min(ties) > T3.TIE_FLOOR, "a route of this case is closer to a tie than float32 can decide: choose another case"
    assert all(np.array_equal(x, y) for a, b in zip(o64, o32) for x, y in zip(a["routes"], b["routes"])), \
        "the float32 twin and the float64 restatement take different pool / ReLU routes: choose another case"
    for name, w, t, b in zip(T3.VECTORS, want, twin, T3.bounds(P, want, steps * nb)):
        if name not in _compared(opt):
            continue
        err = float(np.linalg.norm(t - w))
        print("%s  %-13s twin |err| %.3e  bound %.3e  (%.2f of it)" % (cid, name, err, b, err / b))
        assert err <= b, (cid, name, err, b)
        if name in T3.VECTORS[:4]:
            assert err <= R.PARAM_REL * float(np.linalg.norm(w)), (cid, name)


def _applicable(opt, d, nb, steps):
    faults = ["actor_every_minibatch", "phase_off_by_one", "critic_held_too"]
    if opt == "adam":
        faults.append("adam_count_on_hold")          # (GradientDescent and Momentum read no count: the GPU test compares the counts themselves)
    if opt != "gradient-descent":
        faults.append("slots_on_hold")
    if any((s * nb) % d != 0 for s in range(1, steps + 1)):      # (an outer step that ends on a held minibatch)
        faults.append("target_actor_skips_when_held")
    return faults


@pytest.mark.parametrize("case", T3.grid(), ids=[c[0] for c in T3.grid()])
def test_each_planted_fault_moves_a_vector_by_a_large_multiple_of_the_gpu_bound(case):
    cid, opt, shape_name, d, nb, steps, clip, tau = case
    _specs, P, _ep, _idxs, _b = _case(shape_name)
    want, wcounts, _o = _run(cid)
    for fault in _applicable(opt, d, nb, steps):
        got, counts, _o2 = _run(cid, "f64", fault)
        ratios = {name: float(np.linalg.norm(g - w)) / b for name, g, w, b in zip(T3.VECTORS, got, want, T3.bounds(P, want, steps * nb))
                  if name in _compared(opt) and b > 0}
        print("%s %-30s %s counts %s (want %s)" % (cid, fault, {k: round(v, 1) for k, v in ratios.items()}, list(counts), list(wcounts)))
        assert max(ratios.values()) > POWER, (cid, fault, ratios)
        if fault == "target_actor_skips_when_held":
            assert ratios["target_actor"] > POWER, (cid, ratios)
        if fault == "adam_count_on_hold":
            assert list(counts) != list(wcounts)


def test_every_fault_is_seen_by_some_case():
    seen = set()
    for _cid, opt, _sn, d, nb, steps, _clip, _tau in T3.grid():
        seen.update(_applicable(opt, d, nb, steps))
    assert seen | {"train_actor_advances_n"} == set(T3.FAULTS)


@pytest.mark.parametrize("opt", ["gradient-descent", "adam"])
def test_a_counting_actor_op_shows_in_the_literal_loop(opt):
    """the GPU module's unpaired literal loop (four minibatches, d = 2): with cpp_ddpg_train_actor counting, the actor never meets an
    even count and never moves"""
    from tests import ddpg_opt_np as R
    specs, P, _ep, _idxs, batches = _case("16x16x6")
    hp = T3.hyper_of(opt, 0.5, 0.25)
    want, wcounts, _r = T3.run_literal(specs, P, batches[:4], hp, opt, 2)
    got, counts, _r2 = T3.run_literal(specs, P, batches[:4], hp, opt, 2, fault="train_actor_advances_n")
    ratios = {name: float(np.linalg.norm(g - w)) / b for name, g, w, b in zip(T3.VECTORS, got, want, R.bounds(P, want, 4))
              if name in _compared(opt) and b > 0}
    print("literal %s train_actor_advances_n %s" % (opt, {k: round(v, 1) for k, v in ratios.items()}))
    assert ratios["actor"] > POWER and list(counts)[0] == 0 and list(wcounts) == [2, 4]
