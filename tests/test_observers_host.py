"""The tables of tests/observers.py, held without a GPU: every symbol of include/cartpolepp_abi.h is classified exactly once (a new ABI
entry fails here until someone reads its comment and decides), every observer-class symbol is reached by a catalogue entry, every
entry applies somewhere, and first_difference sees what a bit comparison must see."""
import collections

import numpy as np
import pytest

from tests import observers as OB


def test_every_declared_symbol_has_exactly_one_class_and_nothing_else_is_named():
    declared = OB.declared_symbols()
    assert len(declared) > 150 and len(set(declared)) == len(declared), [s for s, n in collections.Counter(declared).items() if n > 1]
    named = [s for syms in OB.CLASS_LISTS.values() for s in syms]
    twice = [s for s, n in collections.Counter(named).items() if n > 1]
    assert not twice, "classified more than once: %s" % twice
    assert not set(declared) - set(named), "declared in the header, in no class: %s" % sorted(set(declared) - set(named))
    assert not set(named) - set(declared), "classified, not declared in the header: %s" % sorted(set(named) - set(declared))
    assert set(OB.CLASS_LISTS) == {OB.TRAINING, OB.OBSERVER, OB.MUTATOR, OB.CONFIGURATION, OB.LIFECYCLE}


def test_the_header_and_the_ctypes_table_name_the_same_symbols():
    """(the parser of this module against the table the package loads the library with)"""
    import ast
    import os
    src = open(os.path.join(OB.ROOT, "cartpoleplusplus_amd", "_lib.py")).read()
    keys = set()
    for node in ast.walk(ast.parse(src)):
        if isinstance(node, ast.Assign) and getattr(node.targets[0], "id", None) == "SIGNATURES":
            keys = {k.value for k in node.value.keys}
    assert keys == set(OB.declared_symbols()), sorted(keys ^ set(OB.declared_symbols()))


@pytest.mark.parametrize("change", ["one-removed", "one-undeclared"])
def test_the_symbol_check_fails_when_the_table_is_wrong(change, monkeypatch):
    lists = {k: list(v) for k, v in OB.CLASS_LISTS.items()}
    if change == "one-removed":
        lists[OB.OBSERVER].remove("cpp_net_get_pool")
    else:
        lists[OB.MUTATOR].append("cpp_net_scramble_params")
    monkeypatch.setattr(OB, "CLASS_LISTS", {k: tuple(v) for k, v in lists.items()})
    with pytest.raises(AssertionError):
        test_every_declared_symbol_has_exactly_one_class_and_nothing_else_is_named()


def test_the_catalogue_reaches_exactly_the_observer_class():
    reached = set(s for o in OB.CATALOGUE for s in o.symbols)
    observers = set(OB.CLASS_LISTS[OB.OBSERVER])
    assert not reached - observers, "a catalogue entry declares a symbol that is no observer: %s" % sorted(reached - observers)
    assert not observers - reached, "observer-class symbols no catalogue entry reaches: %s" % sorted(observers - reached)
    names = [o.name for o in OB.CATALOGUE]
    assert len(set(names)) == len(names)


def test_every_predicate_evaluates_on_every_record_and_every_entry_applies_somewhere():
    assert len(OB.RECORDS) == len(OB.RECORD) and len(OB.CASES) == len(OB.CASE)
    for o in OB.CATALOGUE:
        where = [r.id for r in OB.RECORDS if bool(o.applies(r))]
        assert where, "%s applies to no case" % o.name
    for r in OB.RECORDS:
        assert len(OB.applicable(r)) >= 8, r.id
        picked = OB.subset(r, 11)
        assert picked and set(o.name for o in picked) <= set(o.name for o in OB.applicable(r))
        assert [o.name for o in picked] == [o.name for o in OB.subset(r, 11)]


def test_the_cases_are_the_issues():
    ids = [c.id for c in OB.CASES]
    assert ids == ["plain", "capacity16", "lowdim", "adam-td3", "momentum", "categorical", "quantile", "pooled-sac", "twin-sac", "drqv2", "bc",
                   "per-nstep", "param-noise", "dropout", "batch-norm", "naf-adam", "naf-per", "big-plain", "big-shared"]
    dp = sorted(r.case.id for r in OB.RECORDS if r.comm)
    assert dp == ["adam-td3"] * 3 + ["plain"] * 3          # the data-parallel step refuses a prioritized memory; two cases carry the modes
    assert [r.id for r in OB.RECORDS if r.entry == "literal-mid"] == ["plain-literal-mid"]
    for c in OB.CASES:
        big = c.id.startswith("big")
        assert (c.shape == OB.BIG_SHAPE) == big and (big or c.shape in (OB.DEFAULT_SHAPE, OB.LOWDIM))
        assert c.B == (OB.BIG_B if big else 8) and c.capacity >= c.B
    r = OB.RECORD["drqv2-fused"]
    assert r.shift and r.shared and r.feature_norm and r.n_step == 3 and not r.actor_conv and r.case.kw["replay_store"] == "u8"
    r = OB.RECORD["adam-td3-dp"]
    assert r.twin and r.actor_min and r.delay == 2 and r.smoothing and r.slots and r.comm
    assert OB.RECORD["pooled-sac-ops"].gaussian and OB.RECORD["pooled-sac-ops"].pooled and OB.RECORD["pooled-sac-ops"].twin


# ---- first_difference
def _snap(**kw):
    return collections.OrderedDict((k, np.asarray(v)) for k, v in kw.items())


def test_first_difference_is_none_on_equal_bytes_nan_included():
    a = [_snap(n=np.uint64(3), p=np.array([1.0, np.nan, -0.0], np.float32))]
    b = [_snap(n=np.uint64(3), p=np.array([1.0, np.nan, -0.0], np.float32))]
    assert OB.first_difference(a, b) is None
    assert OB.first_difference(a[0], b[0]) is None


def test_first_difference_tells_minus_zero_from_zero_and_one_nan_from_another():
    a = _snap(p=np.array([0.0, 1.0, 2.0], np.float32))
    b = _snap(p=np.array([-0.0, 1.0, 2.0], np.float32))
    assert OB.first_difference(a, b) == (0, "p", 1, 0.0)
    quiet = np.array([np.nan], np.float32)
    other = (quiet.view(np.uint32) | np.uint32(1)).view(np.float32)
    call, key, n, worst = OB.first_difference(_snap(p=quiet), _snap(p=other))
    assert (call, key, n) == (0, "p", 1) and np.isnan(worst)


def test_first_difference_names_the_first_call_and_the_first_key_and_counts():
    a = [_snap(n=1, p=np.zeros(4, np.float32)), _snap(n=2, p=np.zeros(4, np.float32)), _snap(n=3, p=np.zeros(4, np.float32))]
    b = [_snap(n=1, p=np.zeros(4, np.float32)), _snap(n=2, p=np.array([0, 0.5, 0, -2.0], np.float32)), _snap(n=4, p=np.ones(4, np.float32))]
    assert OB.first_difference(a, b) == (1, "p", 2, 2.0)
    b[1]["n"] = np.asarray(7)
    assert OB.first_difference(a, b) == (1, "n", 1, 5.0)


def test_first_difference_reports_a_missing_key_a_shape_change_a_type_change_and_a_short_trace():
    a, b = _snap(n=1, p=np.zeros(4, np.float32)), _snap(n=1)
    call, key, n, worst = OB.first_difference(a, b)
    assert (call, key, n) == (0, "p", 4) and np.isnan(worst)
    assert OB.first_difference(b, a)[:3] == (0, "p", 4)
    call, key, n, worst = OB.first_difference(_snap(p=np.zeros(4, np.float32)), _snap(p=np.zeros((2, 2), np.float32)))
    assert (call, key, n) == (0, "p", 4) and np.isnan(worst)
    assert OB.first_difference(_snap(p=np.zeros(2, np.float32)), _snap(p=np.zeros(2, np.float64)))[:3] == (0, "p", 2)
    assert OB.first_difference([a, a], [a])[:2] == (1, None)


def test_compare_with_observers_says_whether_the_call_or_the_block_differs():
    ref = [_snap(n=1, p=np.zeros(2, np.float32), seen=5), _snap(n=2, p=np.ones(2, np.float32), seen=6)]
    same = [(ref[0], _snap(n=1, p=np.zeros(2, np.float32))), (ref[1], None)]
    assert OB.compare_with_observers(same, ref) is None
    moved = [(ref[0], _snap(n=9, p=np.zeros(2, np.float32))), (ref[1], None)]
    assert OB.compare_with_observers(moved, ref) == ((0, "n", 1, 8.0), "observers")
    late = [(ref[0], _snap(n=1, p=np.zeros(2, np.float32))), (_snap(n=2, p=np.array([1, 3], np.float32), seen=6), None)]
    assert OB.compare_with_observers(late, ref) == ((1, "p", 1, 2.0), "call")
