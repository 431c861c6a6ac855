"""Prioritized replay for the NAF agent, host side: the float64 weighted NAF reference (tests/naf_per_np.py) proven against the unmodified
oracle, and the NAF options (the DDPG parser's six keys and defaults, no command-line flag yet, the same refusals)."""
import numpy as np
import pytest

from oracle import ddpg_np as O
from oracle import naf_np as N
from tests.naf_per_np import WeightedNAF

LOWDIM = (2, 2, 7)


def _naf(share, seed, cls=WeightedNAF):
    rng = np.random.default_rng(seed)
    skw = dict(pixel=False, state_elems=int(np.prod(LOWDIM)))
    vspec = N.HeadSpec(1, "linear", [100, 50], **skw)
    if share:
        mspec = N.HeadSpec(2, "tanh", [], False, state_elems=50, head_only=True)
        lspec = N.HeadSpec(3, "linear", [], False, state_elems=50, head_only=True)
    else:
        mspec, lspec = N.HeadSpec(2, "tanh", [100, 50], **skw), N.HeadSpec(3, "linear", [100, 50], **skw)
    # (perturbed away from the zero biases and the tiny mu head, as the GPU tests do: every path carries signal)
    flats = [N.init_head_params(sp, rng) for sp in (vspec, mspec, lspec)]
    flats = [f + rng.normal(0, 0.05, f.shape).astype(np.float32) for f in flats]
    naf = cls(vspec, mspec, lspec, flats[0], flats[1], flats[2], share, 2, np.float64)
    naf.target_value = O.Net(vspec, flats[0] + rng.normal(0, 0.01, flats[0].shape).astype(np.float32), np.float64)
    return naf


def _batch(B, seed):
    return O.synthetic_batch(np.random.default_rng(seed), B, LOWDIM, 2, False)


@pytest.mark.parametrize("share", [True, False], ids=["share", "own-trunks"])
def test_weighted_reference_with_unit_weights_is_the_oracle_bit_for_bit(share):
    naf, t = _naf(share, 1), _batch(16, 2)
    want = N.NAF.forward_backward(naf, t)
    got = naf.forward_backward(t, w=np.ones(16))
    assert np.array_equal(got["grads"], want["grads"]) and got["loss"] == want["loss"]
    assert np.array_equal(got["td"], want["td"])


@pytest.mark.parametrize("share", [True, False], ids=["share", "own-trunks"])
def test_weighted_gradient_is_the_weighted_mean_of_one_row_gradients(share):
    """no batch whitening in the low-dimensional NAF: the batch's gradient is the mean of its rows' -- the weighted one
    (1/B) sum_b w_b grad(row b), each row's gradient from the UNMODIFIED oracle as a batch of one"""
    B = 12
    naf, t = _naf(share, 3), _batch(B, 4)
    w = np.random.default_rng(5).uniform(0.05, 1.0, B)
    w[0] = 1.0
    got = naf.forward_backward(t, w=w)
    plain = _naf(share, 3, cls=N.NAF)
    rows = [plain.forward_backward(tuple(np.asarray(x)[b:b + 1] for x in t)) for b in range(B)]
    want = sum(w[b] * rows[b]["grads"] for b in range(B)) / B
    assert np.abs(got["grads"] - want).max() <= 1e-12 * max(1.0, np.abs(want).max())
    assert abs(got["loss"] - sum(w[b] * rows[b]["loss"] for b in range(B)) / B) <= 1e-12 * max(1.0, abs(got["loss"]))
    # (and the weights matter)
    assert np.abs(got["grads"] - N.NAF.forward_backward(plain, t)["grads"]).max() > 1e-3 * np.abs(want).max()


def test_naf_options_carry_the_ddpg_per_keys_and_defaults():
    from cartpoleplusplus_amd import ddpg_cartpole as D
    from cartpoleplusplus_amd import naf_cartpole as F
    keys = ("prioritized_replay", "priority_alpha", "priority_beta", "priority_beta_final", "priority_beta_steps", "priority_eps")
    d, n = vars(D.build_parser().parse_args([])), vars(F.build_parser().parse_args([]))
    for k in keys:
        assert n[k] == d[k] and type(n[k]) is type(d[k]), k
    o = F.default_opts(prioritized_replay=True, priority_beta_steps=5)
    assert o.prioritized_replay and o.priority_beta_steps == 5
    assert F.priority_beta(o, 0) == 0.4 and F.priority_beta(o, 5) == 1.0


def test_naf_command_line_still_has_no_per_flag():
    from cartpoleplusplus_amd import naf_cartpole as F
    for flag in ("--prioritized-replay", "--priority-alpha"):
        with pytest.raises(SystemExit):
            F.build_parser().parse_args([flag] if flag == "--prioritized-replay" else [flag, "0.5"])


@pytest.mark.parametrize("extra", [dict(host_rng_sampling=True), dict(data_parallel=True)], ids=["host-rng", "data-parallel"])
def test_naf_refuses_per_with_host_rng_or_data_parallel(extra):
    from cartpoleplusplus_amd import naf_cartpole as F
    o = F.default_opts(prioritized_replay=True, **extra)
    with pytest.raises(SystemExit):
        F.check_prioritized_opts(o)
    F.check_prioritized_opts(F.default_opts(**extra))          # (uniform replay: nothing to refuse)
