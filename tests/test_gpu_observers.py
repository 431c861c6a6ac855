"""Training is held to the same bits when observers run between its calls ("Observers").

Per case and entry point of tests/observers.py, four runs from the same seed, parameters and memory, each behind a reset route and each
synchronising after every call (so the route's "k - 1 or k - 2" rule decides alike in all of them):
  A    the training calls only, state read once at the end
  A2   A again: A2 == A is the precondition -- the variant is deterministic from run to run
  A'   A with after_call and snapshot behind every call: A' == A shows that the test's own reads observe
  B    A' with an observer block between every two calls -- every applicable observer in catalogue order, and a seeded random subset in
       random order -- and a second snapshot behind each block: no difference behind any call or block, and none at the end against A
The reference is the run without the observers and the bar is bit identity: there is no tolerance anywhere in this module.  Three
positive controls slip a documented mutator among the observers and must be told which call and which key it moved."""
import collections

import numpy as np
import pytest

from tests import observers as OB

pytestmark = pytest.mark.gpu
SUBSET_SEED = 11
_REFERENCE = {}


def reference(rid):
    """runs A, A2 and A' of a record, once per process: (first difference A2 / A, first difference A' / A, A''s trace, A's end)"""
    if rid not in _REFERENCE:
        rec = OB.RECORD[rid]
        _t, end_a = OB.run(rec, "A")
        _t, end_a2 = OB.run(rec, "A")
        trace, end_ap = OB.run(rec, "A'")
        _REFERENCE[rid] = (OB.first_difference(end_a2, end_a), OB.first_difference(end_ap, end_a), trace, end_a)
    return _REFERENCE[rid]


@pytest.mark.parametrize("rid", [r.id for r in OB.RECORDS])
def test_the_run_repeats_itself_and_the_tests_own_reads_observe(rid):
    again, reads, trace, end = reference(rid)
    assert again is None, "%s: two runs of the same calls differ (call, key, elements, max |difference|): %s" % (rid, again)
    assert reads is None, "%s: reading after_call and snapshot behind every call changed the end: %s" % (rid, reads)
    assert len(trace) == 4 and any(k.startswith("params.") for k in end) and "route" in end


@pytest.mark.parametrize("which", ["all", "subset-seed%d" % SUBSET_SEED])
@pytest.mark.parametrize("rid", [r.id for r in OB.RECORDS])
def test_observers_between_the_training_calls_change_nothing(rid, which, tmp_path):
    rec = OB.RECORD[rid]
    again, reads, trace_ref, end_a = reference(rid)
    assert again is None and reads is None, (again, reads)
    observers = OB.applicable(rec) if which == "all" else OB.subset(rec, SUBSET_SEED)
    trace_b, end_b = OB.run(rec, "B", tmp_path=tmp_path, observers=observers)
    found = OB.compare_with_observers(trace_b, trace_ref)
    names = [o.name for o in observers]
    assert found is None, "%s: behind the %s of call %d, %r differs in %d element(s), max |difference| %g; observers %s" % (
        rid, found[1], found[0][0], found[0][1], found[0][2], found[0][3], names)
    end = OB.first_difference(end_b, end_a)
    assert end is None, "%s: the end differs from the run without observers: %s; observers %s" % (rid, end, names)
    print("%s %s: identical (%d observers, route %s)" % (rid, which, len(names), end_b["route"].tolist()))


def test_the_large_cases_run_the_row_streaming_forward_and_the_operand_image_rider():
    """OB.BIG_B is the smallest batch at 64x64x18 whose minibatch runs conv1's forward on the f16 pipes' row-streaming kernel and whose
    optimiser launch builds the next minibatch's operand images: one row does neither"""
    from tests.helpers import _profiled_calls, conv_routes_of, make_pair
    seen = {}
    for B in (OB.BIG_B - 1, OB.BIG_B):
        OB.reset_route()
        agent, _ref, _ = make_pair(OB.BIG_SHAPE, B, True, seed=3, replay_size=OB.REPLAY_SIZE, capacity=4)
        try:
            agent.replay_memory.fill_synthetic(OB.ROWS, seed=24)
            calls = _profiled_calls(agent.actor.ctx, lambda: agent.train_step(B, 2))
            seen[B] = (conv_routes_of(calls)["conv1_fwd"], calls.get("conv1_image", 0))
        finally:
            agent.close()
    print("conv1 forward family and conv1_image launches of train_step(B, 2) at 64x64x18:", seen)
    assert seen[OB.BIG_B][0] == "conv1_fwd_f16" and seen[OB.BIG_B][1] >= 1, seen
    assert seen[OB.BIG_B - 1][0] == "conv1_fwd" and seen[OB.BIG_B - 1][1] == 0, seen


# ---- positive controls: the comparison can fail, and says where
def _control(rid, slip, tmp_path):
    rec = OB.RECORD[rid]
    again, reads, trace_ref, _end = reference(rid)
    assert again is None and reads is None, (again, reads)
    trace_b, _end_b = OB.run(rec, "B", tmp_path=tmp_path, observers=OB.applicable(rec), slip=(1, slip))
    return trace_b, trace_ref, OB.compare_with_observers(trace_b, trace_ref)


def _differing(trace_b, trace_ref, k):
    return [key for key in trace_ref[k] if OB.first_difference({key: trace_b[k][0][key]}, {key: trace_ref[k][key]}) is not None]


def test_control_a_shifted_gather_among_the_observers_moves_the_shift_counter(tmp_path):
    B = OB.RECORD["drqv2-fused"].B
    trace_b, trace_ref, found = _control("drqv2-fused", lambda env: env.agent.replay_memory.gather_shifted(np.arange(B)), tmp_path)
    assert found == ((1, "shift_counter", 1, 1.0), "observers"), found
    assert not _differing(trace_b, trace_ref, 0) and not _differing(trace_b, trace_ref, 1)
    for k in (2, 3):          # the next call gathered under another count: other shifts, other parameters
        moved = _differing(trace_b, trace_ref, k)
        assert "shift_counter" in moved and "last_shifts" in moved and "params.critic" in moved and "params.actor" in moved, (k, moved)


def test_control_a_resample_among_the_observers_moves_the_draw_count_and_the_perturbed_copy_alone(tmp_path):
    trace_b, trace_ref, found = _control("param-noise-fused", lambda env: env.trainer.param_noise_resample(None), tmp_path)
    assert found == ((1, "param_noise.n", 1, 1.0), "observers"), found
    assert not _differing(trace_b, trace_ref, 0) and not _differing(trace_b, trace_ref, 1)
    for k in (2, 3):          # "no launch of a training call reads or writes any of this": the copy differs, nothing that trains does
        moved = _differing(trace_b, trace_ref, k)
        assert {"param_noise.n", "param_noise.state", "params.perturbed_actor"} <= set(moved), (k, moved)
        assert all(key.startswith("param_noise.") or key == "params.perturbed_actor" for key in moved), (k, moved)


def test_control_an_episode_added_among_the_observers_moves_the_priority_tree(tmp_path):
    def add_episode(env):
        rm = env.agent.replay_memory
        state = np.full(rm.state_shape, 0.25, np.float16)
        rm.add_episode(state, [(np.zeros((1, rm.action_dim), np.float32), 1.0, state)] * 2)
    trace_b, trace_ref, found = _control("per-nstep-fused", add_episode, tmp_path)
    assert found is not None and found[0][:2] == (1, "priority_tree") and found[1] == "observers", found
    assert not _differing(trace_b, trace_ref, 0) and not _differing(trace_b, trace_ref, 1)
    for k in (2, 3):          # new rows at the running maximum priority, a larger range: other draws, other parameters
        moved = _differing(trace_b, trace_ref, k)
        assert "priority_tree" in moved and "last_indexes" in moved and "params.critic" in moved, (k, moved)
