"""Prioritized replay on the host side: the numpy restatement (tests/per_np.py) of the device's sum tree, draw and weights, and the
command line's new options (PER off by default, nothing else in `opts` changes)."""
import numpy as np
import pytest

from tests import per_np as P


def test_tree_inner_nodes_are_sums_of_their_children():
    rng = np.random.default_rng(0)
    L = P.levels(1000)
    assert (1 << L) >= 1000 and (1 << (L - 1)) < 1000
    tree = P.build(P.priority(rng.normal(size=1000), 0.6, 1e-6).astype(np.float64), L)
    P.write(tree, L, rng.integers(0, 1000, 300), P.priority(rng.normal(size=300), 0.6, 1e-6))
    for node in range(1, 1 << L):
        assert tree[node] == tree[2 * node] + tree[2 * node + 1]


def test_priority_special_cases():
    td = np.array([-2.5, 0.0, 1e-3], np.float32)
    assert np.array_equal(P.priority(td, 1.0, 1e-6), np.abs(td) + np.float32(1e-6))
    assert np.array_equal(P.priority(td, 0.0, 0.0), np.ones(3, np.float32))


def test_duplicate_row_keeps_its_last_priority():
    L = P.levels(8)
    tree = P.build(np.ones(8), L)
    P.write(tree, L, [3, 5, 3, 3], [2.0, 4.0, 7.0, 0.5])
    assert tree[(1 << L) + 3] == 0.5 and tree[(1 << L) + 5] == 4.0
    assert tree[1] == 6 + 0.5 + 4.0


def test_draw_frequencies_follow_the_priorities():
    """10^5 draws against p^alpha / sum: chi-square well inside its bound (stratified draws are, if anything, closer than multinomial)"""
    rng = np.random.default_rng(1)
    n, alpha = 50, 0.6
    p = P.priority(rng.exponential(size=n), alpha, 1e-6)
    L = P.levels(n)
    tree = P.build(p.astype(np.float64), L)
    B, counts = 1000, np.zeros(n)
    for ctr in range(100):
        rows, _g = P.draw(tree, L, n, B, seed=7, counter=ctr)
        counts += np.bincount(rows, minlength=n)
    expect = 100 * B * p.astype(np.float64) / p.astype(np.float64).sum()
    chi2 = float(((counts - expect) ** 2 / expect).sum())
    assert chi2 < 2 * n + 50, chi2       # (49 degrees of freedom: mean 49, sd 10)


def test_top_end_guard_takes_the_last_row():
    """a tree whose root sum exceeds the sum of the leaves below `size` (as rounding can leave it): u past them lands on size - 1"""
    L = P.levels(8)
    tree = P.build(np.array([1.0, 1, 1, 1, 1, 0, 0, 0]), L)
    tree[1] = 6.0                             # total 6, leaves only 5: the last stratum walks past row 4
    rows, guarded = P.draw(tree, L, 5, 6, seed=0, counter=0)
    assert guarded.any() and (rows[guarded] == 4).all() and rows.max() == 4


def test_weights_peak_at_one():
    rng = np.random.default_rng(2)
    L = P.levels(100)
    tree = P.build(P.priority(rng.normal(size=100), 0.6, 1e-6).astype(np.float64), L)
    rows, _ = P.draw(tree, L, 100, 64, seed=3, counter=5)
    w = P.weights(tree, L, 100, rows, 0.4)
    assert w.max() == 1.0 and (w > 0).all()
    assert np.array_equal(P.weights(tree, L, 100, rows, 0.0), np.ones(64, np.float32))


# the parser's defaults before prioritized replay existed (every option name and value): nothing but the PER keys may be added
DEFAULTS_BEFORE_PER = {
    "action_force": 50.0, "action_noise_sigma": 0.05, "action_noise_theta": 0.01, "action_repeats": 2, "actor_hidden_layers": "100,100,50",
    "actor_learning_rate": 0.001, "async_rollouts": False, "batch_size": 128, "batches_per_step": 5, "ckpt_dir": None, "ckpt_freq": 3600,
    "critic_hidden_layers": "100,100,50", "critic_learning_rate": 0.01, "data_parallel": False, "delay": 0.0, "discount": 0.99,
    "dont_do_rollouts": False, "eval_action_noise": False, "event_log_in": None, "event_log_out": None, "exact_products": False,
    "gradient_clip": 5, "gui": False, "host_rng_sampling": False, "initial_force": 55.0, "max_episode_len": 200, "max_num_actions": 0,
    "max_run_time": 0, "no_random_theta": False, "num_cameras": 1, "num_eval": 0, "optimiser": "GradientDescent",
    "optimiser_args": '{"learning_rate": 0.001}', "overlap_allreduce": False, "print_gradients": False, "render_height": 50,
    "render_width": 50, "replay_memory_burn_in": 1000, "replay_memory_size": 22000, "replay_store": "f16", "reward_calc": "fixed",
    "sample_seed": 0, "steps_per_repeat": 5, "sync_every": 1, "synthetic_env": False, "target_update_rate": 0.0001,
    "use_batch_norm": False, "use_dropout": False, "use_raw_pixels": False,
}


def test_cli_defaults_unchanged_plus_per_keys():
    from cartpoleplusplus_amd import ddpg_cartpole as D
    o = vars(D.build_parser().parse_args([]))
    new = {"prioritized_replay": False, "priority_alpha": 0.6, "priority_beta": 0.4, "priority_beta_final": 1.0,
           "priority_beta_steps": 100000, "priority_eps": 1e-6}
    for k, v in new.items():
        assert o.pop(k) == v, k
    assert o == DEFAULTS_BEFORE_PER
    assert all(type(o[k]) is type(v) for k, v in DEFAULTS_BEFORE_PER.items())


def test_cli_accepts_the_per_flags_and_schedules_beta():
    from cartpoleplusplus_amd import ddpg_cartpole as D
    o = D.build_parser().parse_args(["--prioritized-replay", "--priority-alpha", "0.7", "--priority-beta", "0.5",
                                     "--priority-beta-final", "0.9", "--priority-beta-steps", "4", "--priority-eps", "1e-5"])
    assert o.prioritized_replay and o.priority_alpha == 0.7 and o.priority_eps == 1e-5
    assert D.priority_beta(o, 0) == 0.5 and abs(D.priority_beta(o, 2) - 0.7) < 1e-12 and D.priority_beta(o, 10) == 0.9
    D.check_prioritized_opts(o)


@pytest.mark.parametrize("extra", [["--host-rng-sampling"], ["--data-parallel"]])
def test_cli_refuses_per_with_host_rng_or_data_parallel(extra):
    from cartpoleplusplus_amd import ddpg_cartpole as D
    o = D.build_parser().parse_args(["--prioritized-replay"] + extra)
    with pytest.raises(SystemExit):
        D.check_prioritized_opts(o)


def test_naf_cli_has_no_per():
    from cartpoleplusplus_amd import naf_cartpole as F
    with pytest.raises(SystemExit):
        F.build_parser().parse_args(["--prioritized-replay"])
