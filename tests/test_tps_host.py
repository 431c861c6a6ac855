"""Target policy smoothing, what can be established without a GPU: the numpy restatement of the noise (tests/tps_np.py) against
its own float64 evaluation and against the normal distribution, the independence of its streams, the command-line surface, and
the power of tests/test_gpu_target_smoothing.py's oracle comparison -- every planted fault moves a float64 TD by more than 10x
the bar that test applies, on that test's own cases."""
import math

import numpy as np
import pytest

from tests import tps_np as T
from tests.helpers import host_case

SEED = 0xC0FFEE1234567


def test_f32_restatement_against_float64():
    """2^20 draws before the clip: the float32 evaluation within Z_BAR of the float64 one (24-bit uniforms are exact in both)"""
    B, A = 1 << 17, 8
    z32 = T.standard_normals(SEED, 3, B, A, np.float32)
    z64 = T.standard_normals(SEED, 3, B, A, np.float64)
    assert z32.dtype == np.float32 and z32.size == 1 << 20
    err = float(np.abs(z32.astype(np.float64) - z64).max())
    print("max |z32 - z64| over 2^20 draws: %.3e (bar %.1e); max |z| %.3f" % (err, T.Z_BAR, float(np.abs(z64).max())))
    assert err <= T.Z_BAR
    assert np.abs(z64).max() <= 5.77 and np.isfinite(z64).all()


def test_moments():
    """N = 2^16 draws: mean and variance within four standard errors of N(0, 1)'s (1 / sqrt N and sqrt(2 / N))"""
    N = 1 << 16
    z = T.standard_normals(SEED, 0, N // 4, 4).ravel()
    assert abs(z.mean()) < 4.0 / math.sqrt(N), z.mean()
    assert abs(z.var() - 1.0) < 4.0 * math.sqrt(2.0 / N), z.var()


def test_clip_fraction():
    """sigma = c: the clip binds where |z| >= 1, a fraction erfc(1 / sqrt 2) of the draws, to four binomial standard errors"""
    N = 1 << 16
    eps = T.target_noise(SEED, 5, N // 2, 2, 0.3, 0.3).ravel()
    p = math.erfc(1.0 / math.sqrt(2.0))
    frac = float((np.abs(eps) == 0.3).mean())
    assert abs(frac - p) < 4.0 * math.sqrt(p * (1.0 - p) / N), (frac, p)
    assert np.abs(eps).max() == 0.3


def test_streams_are_independent():
    B, A = 64, 8
    base = T.standard_normals(SEED, 7, B, A)
    assert np.array_equal(base, T.standard_normals(SEED, 7, B, A))
    for other in (T.standard_normals(SEED, 8, B, A), T.standard_normals(SEED, 7 + (1 << 32), B, A),
                  T.standard_normals(SEED + 1, 7, B, A), T.standard_normals(SEED + (1 << 32), 7, B, A)):
        assert not (other == base).any()
    assert len(np.unique(base)) == B * A                                # rows and components
    assert np.array_equal(T.standard_normals(SEED, 7, B // 2, A), base[:B // 2])      # a draw depends on (b, i) alone, not on B
    assert np.array_equal(T.standard_normals(SEED, 7, B, A // 2), base[:, :A // 2])   # ... nor on A
    for f in T.NOISE_FAULTS:
        assert not np.array_equal(T.target_noise(SEED, 7, B, A, 0.5, 0.5, fault=f), T.target_noise(SEED, 7, B, A, 0.5, 0.5)), f


# ---- the command line
KEYS = ("target_policy_noise", "target_policy_noise_clip", "target_policy_noise_seed")


def test_parser_keeps_the_options_of_a_plain_command_line():
    from cartpoleplusplus_amd import ddpg_cartpole as D
    plain = vars(D.build_parser().parse_args([]))
    assert not set(KEYS) & set(plain)
    o = D.default_opts()
    assert (o.target_policy_noise, o.target_policy_noise_clip, o.target_policy_noise_seed) == (0.0, 0.5, 0)
    assert D.target_policy_smoothing(D.build_parser().parse_args([])) == (0.0, 0.5, 0)
    assert D.target_policy_smoothing(o) == (0.0, 0.5, 0)
    o = D.build_parser().parse_args(["--target-policy-noise", "0.2", "--target-policy-noise-clip", "0.4", "--target-policy-noise-seed", "9"])
    assert D.target_policy_smoothing(o) == (0.2, 0.4, 9)
    assert D.target_policy_smoothing(D.build_parser().parse_args(["--target-policy-noise", "0.2"])) == (0.2, 0.5, 0)


@pytest.mark.parametrize("argv", [["--target-policy-noise-clip", "0.3"], ["--target-policy-noise-seed", "4"],
                                  ["--target-policy-noise", "-0.1"], ["--target-policy-noise", "nan"], ["--target-policy-noise", "inf"],
                                  ["--target-policy-noise", "0.2", "--target-policy-noise-clip", "0"],
                                  ["--target-policy-noise", "0.2", "--target-policy-noise-clip", "-1"],
                                  ["--target-policy-noise", "0.2", "--target-policy-noise-clip", "nan"],
                                  ["--target-policy-noise", "0.2", "--target-policy-noise-seed", "-1"],
                                  ["--target-policy-noise", "0.2", "--target-policy-noise-seed", str(2 ** 64)]],
                         ids=lambda a: " ".join(a))
def test_parser_refusals(argv):
    from cartpoleplusplus_amd import ddpg_cartpole as D
    o = D.build_parser().parse_args(argv)
    with pytest.raises(SystemExit):
        D.target_policy_smoothing(o)


def test_naf_does_not_take_the_flags():
    from cartpoleplusplus_amd import naf_cartpole as F
    assert not set(KEYS) & set(vars(F.build_parser().parse_args([])))
    with pytest.raises(SystemExit):
        F.build_parser().parse_args(["--target-policy-noise", "0.2"])


# ---- sensitivity of the GPU test's oracle comparison
def _oracle_case(name):
    B, A, seed, n = T.ORACLE_CASES[name]
    (aspec, cspec), P, _ep, _idxs, batches = host_case(T.CASE_SHAPE, B, 1, seed, rows=T.CASE_ROWS, action_dim=A)
    ref = T.SmoothedDDPG(aspec, cspec, P[0], P[1], np.float64)
    ref.set_targets(T.saturate_target_actor(P[2], aspec), P[3])
    return ref, batches[0], B, A, n


@pytest.mark.parametrize("name", sorted(T.ORACLE_CASES))
def test_every_planted_fault_moves_td_by_ten_times_the_gpu_bar(name):
    ref, batch, B, A, n = _oracle_case(name)
    assert n >= 1, "a count that does not advance shows only past the first minibatch"
    noise = T.target_noise(T.NOISE_SEED, n, B, A, T.SIGMA, T.CLIP)
    good = ref.critic_gradients(batch, noise)
    # both clamps are at work in the reference restatement itself
    inner = float((np.abs(noise) == T.CLIP).mean())
    raw = good["target_actions"] + noise
    up, down = int((raw > 1.0).any(axis=1).sum()), int((raw < -1.0).any(axis=1).sum())
    print("%s: inner clip on %.2f of the draws; +1 clamp on %d rows, -1 clamp on %d rows" % (name, inner, up, down))
    assert inner >= 0.25 and up >= 2 and down >= 2, (inner, up, down)
    assert np.abs(good["smoothed_actions"]).max() <= 1.0
    bar = T.td_bar(ref.hp.discount, T.SIGMA, good["target_dq_da"])
    plain = ref.critic_gradients(batch, None)
    assert np.abs(plain["td"] - good["td"]).max() > 10 * bar, "the smoothing itself is below the bar"
    for fault in T.FAULTS:
        if fault in T.NOISE_FAULTS:
            bad = ref.critic_gradients(batch, T.target_noise(T.NOISE_SEED, n, B, A, T.SIGMA, T.CLIP, fault=fault))
        else:
            bad = ref.critic_gradients(batch, noise, fault=fault)
        moved = float(np.abs(bad["td"] - good["td"]).max())
        print("%s %-28s max |dTD| %.3e = %.0f x the bar %.3e" % (name, fault, moved, moved / bar, bar))
        assert moved > 10 * bar, (fault, moved, bar)
