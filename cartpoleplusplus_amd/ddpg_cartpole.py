#!/usr/bin/env python
"""DDPG agent for cartpole++ with the interface of the reference's ddpg_cartpole.py, running on
hand-written HIP kernels (MI355X) behind include/cartpolepp_abi.h.

Reference surface kept (paths relative to /root/reference/ddpg_cartpole.py): the flag set :18-57
(`opts` is a module global read by the network classes, as in the reference), ActorNetwork :78-145
(`init_ops_for_training`, `action_given`, `train`, attrs `input_state`, `output_action`,
`exploration_noise`, `train_op`), CriticNetwork :148-248 (`init_ops_for_training`,
`q_gradients_wrt_actions`, `train`, `check_loss`, attrs `input_state`, `input_action`, `q_value`,
`reward`, `terminal_mask`, `input_state_2`, `temporal_difference`, `temporal_difference_loss`),
DeepDeterministicPolicyGradientAgent :251-409 (`post_var_init_setup`, `run_training`, `run_eval`) and
the STATS / EVAL stdout lines :352-361, :396-399.

Decisions on reference defects: B1 low-dim critic = flatten|action -> hidden stack;
B2 pixel critic flattens pool3 before hidden1; B4 the np.clip(1, -1, actions) quirk is reproduced
(upper bound only); B10 mean_losses is filled from the last minibatch's TD loss.
"""
import argparse
import ctypes as C
import os
import sys
import time

import numpy as np

from . import _lib, base_network, replay_memory, util
from ._lib import lib, check, ptr

np.set_printoptions(precision=5, threshold=10000, suppress=True, linewidth=10000)

VERBOSE_DEBUG = False


def toggle_verbose_debug(signal, frame):           # SIGUSR1 (the reference installs the same two handlers at import)
    global VERBOSE_DEBUG
    VERBOSE_DEBUG = not VERBOSE_DEBUG


DUMP_WEIGHTS = False


def set_dump_weights(signal, frame):               # SIGUSR2: run_training dumps the weights after the current episode
    global DUMP_WEIGHTS
    DUMP_WEIGHTS = True


def _install_signal_handlers():
    import signal
    try:
        signal.signal(signal.SIGUSR1, toggle_verbose_debug)
        signal.signal(signal.SIGUSR2, set_dump_weights)
    except ValueError:                             # not the main thread (an embedding application): the toggles stay callable
        pass


def build_parser():
    parser = argparse.ArgumentParser(formatter_class=argparse.ArgumentDefaultsHelpFormatter)
    a = parser.add_argument
    a('--num-eval', type=int, default=0, help="if >0 just run this many episodes with no training")
    a('--max-num-actions', type=int, default=0,
      help="train for (at least) this number of actions (always finish current episode) ignore if <=0")
    a('--max-run-time', type=int, default=0,
      help="train for (at least) this number of seconds (always finish current episode) ignore if <=0")
    a('--ckpt-dir', type=str, default=None, help="if set save ckpts to this dir")
    a('--ckpt-freq', type=int, default=3600, help="freq (sec) to save ckpts")
    a('--batch-size', type=int, default=128, help="training batch size")
    a('--batches-per-step', type=int, default=5, help="number of batches to train per step")
    a('--dont-do-rollouts', action="store_true", help="train from the replay memory only")
    a('--target-update-rate', type=float, default=0.0001,
      help="affine combo for updating target networks each time we run a training step")
    a('--use-batch-norm', action='store_true', help="whether to use batch norm on conv layers")
    a('--actor-hidden-layers', type=str, default="100,100,50", help="actor hidden layer sizes")
    a('--critic-hidden-layers', type=str, default="100,100,50", help="critic hidden layer sizes")
    a('--actor-learning-rate', type=float, default=0.001, help="learning rate for actor")
    a('--critic-learning-rate', type=float, default=0.01, help="learning rate for critic")
    a('--discount', type=float, default=0.99, help="discount for RHS of critic bellman equation update")
    a('--event-log-in', type=str, default=None, help="prepopulate replay memory from this event log")
    a('--replay-memory-size', type=int, default=22000, help="max size of replay memory")
    a('--replay-memory-burn-in', type=int, default=1000,
      help="dont train from replay memory until it reaches this size")
    a('--eval-action-noise', action='store_true', help="whether to use noise during eval")
    a('--action-noise-theta', type=float, default=0.01, help="OrnsteinUhlenbeckNoise theta")
    a('--action-noise-sigma', type=float, default=0.05, help="OrnsteinUhlenbeckNoise sigma")
    util.add_opts(parser)
    # the subset of bullet_cartpole.add_opts (bullet_cartpole.py:13-38) that shapes the observations
    a('--action-repeats', type=int, default=2, help="number of action repeats")
    a('--num-cameras', type=int, default=1, help="how many camera points to render; 1 or 2")
    a('--max-episode-len', type=int, default=200, help="maximum episode len for cartpole")
    a('--use-raw-pixels', action='store_true', help="use raw pixels as state instead of poses")
    a('--render-width', type=int, default=50, help="if --use-raw-pixels render with this width")
    a('--render-height', type=int, default=50, help="if --use-raw-pixels render with this height")
    # the rest of bullet_cartpole.add_opts (bullet_cartpole.py:13-38): read by the reference's pybullet environment when it is on
    # sys.path (make_env); --event-log-out is also honoured by the stand-in environment
    a('--gui', action='store_true', help="pybullet GUI")
    a('--delay', type=float, default=0.0, help="seconds to sleep per simulation step")
    a('--action-force', type=float, default=50.0, help="magnitude of action force applied per step")
    a('--initial-force', type=float, default=55.0, help="magnitude of initial push, in random direction")
    a('--no-random-theta', action='store_true', help="initial push always in the same direction")
    a('--steps-per-repeat', type=int, default=5, help="number of sim steps per repeat")
    a('--event-log-out', type=str, default=None, help="path to record event log.")
    a('--reward-calc', type=str, default='fixed',
      help="'fixed': 1 per step. 'angle': 2*max_angle - ox - oy. 'action': 1.5 - |action|. 'angle_action': both")
    # additions of this build
    a('--host-rng-sampling', action='store_true',
      help="draw minibatch rows with numpy's RNG on the host like the reference (default: Philox on the GPU)")
    a('--sample-seed', type=int, default=0, help="seed of the device-side minibatch sampler")
    a('--exact-products', action='store_true',
      help="conv1 / conv2 on the f16 / bf16 matrix pipes with EVERY operand bit (three f16 pieces, nine bf16 products) instead of "
           "operands to within one f32 ulp (two / six): ~0.87 x the speed (cpp_ctx_set_precision)")
    a('--replay-store', type=str, default="f16", choices=["f16", "u8"],
      help="element type of the replay memory's state store: f16 as the reference, or u8 pixel codes "
           "(identical batches for rendered frames, half the memory)")
    a('--data-parallel', action='store_true',
      help="one actor-learner per GPU (launch with torch.distributed.run): own environment and replay shard per process, the "
           "gradients of every minibatch all-reduced over RCCL (cartpoleplusplus_amd/distributed.py)")
    a('--sync-every', type=int, default=1,
      help="--data-parallel: 1 = gradient all-reduce per minibatch; k > 1 = k local minibatch updates, then parameter averaging")
    a('--overlap-allreduce', action='store_true',
      help="--data-parallel: reduce the fully connected layers' gradients beside the conv backward")
    a('--async-rollouts', action='store_true',
      help="play the episodes on a rollout thread while the learner trains back to back (training_loop.py): the learner -- and, with "
           "--data-parallel, every other rank -- never waits for this process's environment once it is past burn-in")
    a('--synthetic-env', action='store_true', help="random-frame stand-in env (pybullet stays optional)")
    # prioritized experience replay (an extension beyond the reference: Schaul et al. 2016, proportional; the sum tree on the GPU)
    a('--prioritized-replay', action='store_true',
      help="draw minibatches by priority (|td| + eps)^alpha and weight the critic's loss by the importance weights")
    a('--priority-alpha', type=float, default=0.6, help="--prioritized-replay: priority exponent alpha")
    a('--priority-beta', type=float, default=0.4, help="--prioritized-replay: importance-weight exponent beta at the start")
    a('--priority-beta-final', type=float, default=1.0, help="--prioritized-replay: beta after --priority-beta-steps train steps")
    a('--priority-beta-steps', type=int, default=100000,
      help="--prioritized-replay: outer train steps over which beta moves linearly to --priority-beta-final")
    a('--priority-eps', type=float, default=1e-6, help="--prioritized-replay: added to |td| before the exponent")
    # the update rule of the actor's and the critic's train ops (an extension beyond the reference, whose DDPG is GradientDescent only,
    # ddpg_cartpole.py:118-119, :218): TensorFlow's Momentum / Adam per list, each with its own slots and step count
    # (both are absent from the parsed options unless given -- the options of a command line that does not name them are exactly what they
    # were, key for key; ddpg_optimiser() reads them with their defaults, default_opts() fills them in)
    a('--ddpg-optimiser', type=str, default=argparse.SUPPRESS, choices=list(DDPG_OPTIMISERS),
      help="update rule of both DDPG train ops (default GradientDescent); the learning rates stay --actor-learning-rate and "
           "--critic-learning-rate")
    a('--ddpg-optimiser-args', type=str, default=argparse.SUPPRESS,
      help="json object with any of momentum (0.0), beta1 (0.9), beta2 (0.999), epsilon (1e-8) for --ddpg-optimiser")
    # target policy smoothing of the critic's target (an extension beyond the reference, ddpg_cartpole.py:199-209: TD3, Fujimoto et al.
    # 2018; DrQ-v2's critic target): a' = clip(mu'(s2) + clip(N(0, sigma^2), -c, c), -1, 1), drawn on the device per row and component
    # (absent from the parsed options unless given, like --ddpg-optimiser; target_policy_smoothing() reads them with their defaults)
    a('--target-policy-noise', type=float, default=argparse.SUPPRESS,
      help="standard deviation sigma of the noise added to the target actor's action in the critic's target (default 0: none)")
    a('--target-policy-noise-clip', type=float, default=argparse.SUPPRESS,
      help="--target-policy-noise: the noise is clipped to +- this (default 0.5)")
    a('--target-policy-noise-seed', type=int, default=argparse.SUPPRESS,
      help="--target-policy-noise: seed of the device's noise stream (default 0)")
    # delayed policy updates (an extension beyond the reference, ddpg_cartpole.py:332-337: TD3, Fujimoto et al. 2018, Algorithm 1): the
    # actor's list is applied with every D-th critic update only, decided on the device (absent from the parsed options unless given,
    # like --ddpg-optimiser; policy_delay() reads it with its default)
    a('--policy-delay', type=int, default=argparse.SUPPRESS,
      help="apply the actor's update with every D-th critic update only (default 1: every minibatch); with --batches-per-step D the "
           "actor moves in the outer step's last minibatch and the targets follow it: TD3's schedule")
    # twin Q heads (an extension beyond the reference, ddpg_cartpole.py:166-171, :199-209: TD3's clipped double-Q, Fujimoto et al. 2018,
    # on a shared representation as in DrQ-v2): the critic's layers from the concat layer upward exist twice, the target takes the smaller
    # of the two target heads (absent from the parsed options unless given, like --ddpg-optimiser; twin_q() reads it with its default)
    a('--twin-q', action='store_true', default=argparse.SUPPRESS,
      help="critics with two Q heads on one representation; both regress onto r + discount * min(Q1', Q2'), the actor follows Q1 unless --actor-min-q")
    # the actor on the minimum head (an extension beyond the reference, ddpg_cartpole.py:111-113, :220-222: the actor's objective of TD3's
    # descendants on twin critics -- DrQ-v2, SAC, DrQ): the actor ascends min(Q1, Q2) at its own action, chosen per row (absent from the
    # parsed options unless given, like --twin-q; actor_min_q() reads it with its default)
    a('--actor-min-q', action='store_true', default=argparse.SUPPRESS,
      help="--twin-q: the actor follows the smaller of Q1 and Q2 at its own action, row by row (default: Q1)")
    # the behaviour-cloning actor term (an extension beyond the reference, ddpg_cartpole.py:111-113: TD3+BC, Fujimoto & Gu 2021, the cure for
    # extrapolation error when the memory is a fixed data set -- --event-log-in .. --dont-do-rollouts): the actor ascends lambda * Q with
    # lambda = alpha / mean|Q| of the minibatch and regresses onto the minibatch's stored action (absent from the parsed options unless
    # given, like --actor-min-q; behaviour_cloning() reads them with their defaults)
    a('--bc-alpha', type=float, metavar='ALPHA', default=argparse.SUPPRESS,
      help="TD3+BC: the actor's grad_ys become -(alpha / mean|Q|) dQ/da + (2/A)(mu - a) with a the stored action; the paper's value is 2.5 (default: off)")
    a('--bc-q-floor', type=float, metavar='F', default=argparse.SUPPRESS,
      help="--bc-alpha: lambda = alpha / max(mean|Q|, F), so that a critic whose Q is 0 gives a finite step (default 1e-3)")
    # distributional critic (an extension beyond the reference, ddpg_cartpole.py:166-177, :199-214: the categorical value distribution of
    # Bellemare et al. 2017 as D4PG uses it, Barth-Maron et al. 2018): the critic's last layer emits logits over a fixed support, trained
    # with the projected Bellman target and cross-entropy; the actor ascends the distribution's mean (absent from the parsed options
    # unless given, like --twin-q; distributional_critic() reads them)
    a('--distributional-critic', action='store_true', default=argparse.SUPPRESS,
      help="critics that emit a categorical value distribution over --num-atoms atoms on [--v-min, --v-max] (both required)")
    a('--num-atoms', type=int, default=argparse.SUPPRESS, help="--distributional-critic: atoms of the support (default 51; 2 .. 64)")
    a('--v-min', type=float, default=argparse.SUPPRESS, help="--distributional-critic: the support's lower end (no default fits every reward scale)")
    a('--v-max', type=float, default=argparse.SUPPRESS, help="--distributional-critic: the support's upper end")
    # quantile critic (an extension beyond the reference, ddpg_cartpole.py:166-177, :199-214: quantile regression, Dabney et al. 2018, with
    # the truncated targets of Kuznetsov et al. 2020 inside one network): the critic's last layer emits N quantile atoms, trained with the
    # quantile Huber loss against the sorted target atoms without their largest D; the actor ascends their mean (absent from the parsed
    # options unless given, like --twin-q; quantile_critic() reads them)
    a('--quantile-critic', action='store_true', default=argparse.SUPPRESS,
      help="critics that emit --num-quantiles quantiles of the return (no support to configure), trained by quantile regression")
    a('--num-quantiles', type=int, default=argparse.SUPPRESS, help="--quantile-critic: quantiles per critic (default 25; 2 .. 64)")
    a('--quantile-huber-kappa', type=float, default=argparse.SUPPRESS, help="--quantile-critic: the Huber threshold of the quantile loss (default 1.0)")
    a('--drop-top-quantiles', type=int, default=argparse.SUPPRESS,
      help="--quantile-critic: drop the D largest target quantiles before the regression (overestimation control; default 0; 0 .. N - 1)")
    # pooled twin quantile critics (an extension beyond the reference, ddpg_cartpole.py:166-177, :199-214: Truncated Quantile Critics, Kuznetsov
    # et al. 2020, with two heads on one representation): each critic has two heads of N quantile atoms; the atoms of both target heads are
    # pooled and sorted and the 2d largest dropped, both heads regress onto the kept ones and the actor ascends the mean over all atoms of both
    # heads.  With --soft-actor-critic this is TQC (absent from the parsed options unless given, like --twin-q; pooled_quantile_critics() reads them)
    a('--pooled-quantile-critics', action='store_true', default=argparse.SUPPRESS,
      help="critics with two heads of --pooled-num-quantiles quantiles each; the target pools both target heads' atoms and drops the largest")
    a('--pooled-num-quantiles', type=int, default=argparse.SUPPRESS, help="--pooled-quantile-critics: quantiles per head (default 25; 2 .. 32)")
    a('--pooled-drop-per-head', type=int, default=argparse.SUPPRESS,
      help="--pooled-quantile-critics: drop the 2 d largest atoms of the pool of 2 N before the regression (default 2; 0 .. N - 1)")
    a('--pooled-huber-kappa', type=float, default=argparse.SUPPRESS, help="--pooled-quantile-critics: the Huber threshold of the quantile loss (default 1.0)")
    # soft actor-critic (an extension beyond the reference, ddpg_cartpole.py:95-119, :199-214: Haarnoja et al. 2018): a stochastic
    # tanh-Gaussian actor, an entropy term in the critic's target and a learned temperature; with --twin-q and random shift this is DrQ
    # (absent from the parsed options unless given, like --twin-q; soft_actor_critic() reads them)
    a('--soft-actor-critic', action='store_true', default=argparse.SUPPRESS,
      help="maximum-entropy learner: the actor emits a tanh-Gaussian policy, the target carries -alpha log pi, alpha is learned")
    a('--sac-init-temperature', type=float, default=argparse.SUPPRESS, help="--soft-actor-critic: the initial temperature alpha (default 0.1)")
    a('--sac-target-entropy', type=float, default=argparse.SUPPRESS, help="--soft-actor-critic: the target entropy (default: -action_dim)")
    a('--sac-temperature-learning-rate', type=float, default=argparse.SUPPRESS,
      help="--soft-actor-critic: Adam's rate for log alpha (default 1e-4; 0: a fixed temperature)")
    a('--sac-log-std-min', type=float, default=argparse.SUPPRESS, help="--soft-actor-critic: lower bound of the policy's log std (default -10)")
    a('--sac-log-std-max', type=float, default=argparse.SUPPRESS, help="--soft-actor-critic: upper bound of the policy's log std (default 2)")
    a('--sac-seed', type=int, default=argparse.SUPPRESS, help="--soft-actor-critic: seed of the policy noise on the device (default 0)")
    # feature layer norm (an extension beyond the reference, ddpg_cartpole.py:95, :168: the trunk of DrQ-v2, Yarats et al. 2021):
    # Linear -> LayerNorm -> tanh on the first fully connected layer of actor and critic, between the conv features and the MLP; with
    # --twin-q, --n-step 3, --target-policy-noise and random shift this is DrQ-v2 (absent unless given; feature_layer_norm() reads them)
    a('--feature-layer-norm', action='store_true', default=argparse.SUPPRESS,
      help="pixel networks: layer-normalise the first fully connected layer of actor and critic (Linear -> LayerNorm -> tanh)")
    a('--feature-norm-activation', type=str, default=argparse.SUPPRESS, choices=list(FEATURE_NORM_ACTIVATIONS),
      help="--feature-layer-norm: the activation behind the normalisation (default tanh)")
    # n-step returns for this learner (ReplayMemory.enable_n_step; absent unless given): with --prioritized-replay, --data-parallel and
    # --distributional-critic this is D4PG from the command line
    a('--n-step', type=int, default=argparse.SUPPRESS,
      help="train on n-step returns: reward = sum_k discount^k r_k, bootstrap with discount^n (default 1: one-step transitions)")
    # shared conv encoder (an extension beyond the reference, ddpg_cartpole.py:78-100, :148-171, whose four networks each own three conv
    # layers: SAC-AE, DrQ, DrQ-v2): the actors have no conv layers and read the critics' conv features, which only the critic's loss
    # trains (absent from the parsed options unless given, like --twin-q; shared_encoder() reads it)
    a('--shared-encoder', action='store_true', default=argparse.SUPPRESS,
      help="pixel networks: actor and target actor read the conv features of critic and target critic; only the critic's loss trains the encoder")
    # DrQ's random shift from the command line (ReplayMemory.enable_random_shift; absent unless given; random_shift() reads them)
    a('--random-shift', type=int, metavar='PAD', default=argparse.SUPPRESS,
      help="--use-raw-pixels: pad every gathered image by PAD pixels of its own edge and crop it back at a random offset (default 0: off)")
    a('--random-shift-seed', type=int, metavar='N', default=argparse.SUPPRESS, help="--random-shift: seed of the shifts (default 0)")
    # parameter-space exploration noise (an extension beyond the reference, ddpg_cartpole.py:127-134, whose exploration is one
    # Ornstein-Uhlenbeck process added to the action: Plappert et al. 2018): the actor's weights are perturbed once per episode on the
    # device, the episode is played with the perturbed copy, and the perturbation's scale adapts until it moves the actions by DELTA
    # (absent from the parsed options unless given, like --random-shift; param_noise() reads them)
    a('--param-noise-stddev', type=float, metavar='S', default=argparse.SUPPRESS,
      help="explore with a copy of the actor whose weights carry N(0, S^2) noise, redrawn at every episode boundary, instead of the "
           "Ornstein-Uhlenbeck action noise; S is the initial standard deviation (default: off)")
    a('--param-noise-target', type=float, metavar='DELTA', default=argparse.SUPPRESS,
      help="--param-noise-stddev: the root-mean-square distance between the actor's and the perturbed actor's actions that the standard "
           "deviation is adapted towards (default 0.1)")
    a('--param-noise-adapt', type=float, metavar='ALPHA', default=argparse.SUPPRESS,
      help="--param-noise-stddev: the standard deviation is multiplied (distance below DELTA) or divided by ALPHA at every measured resample "
           "(default 1.01; 1 keeps it fixed)")
    a('--param-noise-adapt-rounds', type=int, metavar='R', default=argparse.SUPPRESS,
      help="--param-noise-stddev: resamples per episode boundary, each adapting; the last is the exploring copy (default 1)")
    a('--param-noise-seed', type=int, metavar='N', default=argparse.SUPPRESS,
      help="--param-noise-stddev: seed of the device's noise stream (default 0; --data-parallel: rank r draws with N + r)")
    return parser


def shared_encoder(o):
    """--shared-encoder; off unless given; refuses what cannot be meant"""
    if not bool(getattr(o, "shared_encoder", False)):
        return False
    if not bool(getattr(o, "use_raw_pixels", False)):
        raise SystemExit("--shared-encoder needs --use-raw-pixels: a low-dimensional network has no conv encoder to share")
    if bool(getattr(o, "use_batch_norm", False)):
        raise SystemExit("--shared-encoder cannot be combined with --use-batch-norm")
    if bool(getattr(o, "use_dropout", False)):
        raise SystemExit("--shared-encoder cannot be combined with --use-dropout")
    return True


def random_shift(o):
    """(pad, seed) of --random-shift / --random-shift-seed; (0, 0) is off; refuses what cannot be meant"""
    pad, seed = getattr(o, "random_shift", None), getattr(o, "random_shift_seed", None)
    if pad is None or (not isinstance(pad, bool) and pad == 0):
        if seed is not None:
            raise SystemExit("--random-shift-seed %r needs --random-shift PAD" % (seed,))
        return (0, 0)
    if isinstance(pad, bool) or not isinstance(pad, (int, np.integer)) or int(pad) < 0:
        raise SystemExit("--random-shift %r is not a whole number of pixels >= 0" % (pad,))
    seed = 0 if seed is None else seed
    if isinstance(seed, bool) or not isinstance(seed, (int, np.integer)) or not 0 <= int(seed) < 2 ** 64:
        raise SystemExit("--random-shift-seed %r is not in [0, 2^64)" % (seed,))
    if not bool(getattr(o, "use_raw_pixels", False)):
        raise SystemExit("--random-shift needs --use-raw-pixels: a low-dimensional state has no image to shift")
    return (int(pad), int(seed))


_PARAM_NOISE_DEFAULTS = {"param_noise_target": 0.1, "param_noise_adapt": 1.01, "param_noise_adapt_rounds": 1, "param_noise_seed": 0}
PARAM_NOISE_ROUNDS_MAX = 64


def param_noise(o):
    """{stddev, target, adapt, rounds, seed} of --param-noise-stddev and its --param-noise-* flags, or None (off); refuses what cannot be
    meant"""
    import math
    s = getattr(o, "param_noise_stddev", None)
    given = [k for k in _PARAM_NOISE_DEFAULTS if getattr(o, k, None) is not None]
    if s is None:
        if given:
            raise SystemExit("--%s needs --param-noise-stddev" % given[0].replace("_", "-"))
        return None
    v = {}
    for k, name in (("param_noise_stddev", "stddev"), ("param_noise_target", "target"), ("param_noise_adapt", "adapt")):
        x = getattr(o, k, None)
        x = _PARAM_NOISE_DEFAULTS.get(k) if x is None else x
        try:
            x = float(np.float32(x))
        except (TypeError, ValueError) as e:
            raise SystemExit("--%s: %s" % (k.replace("_", "-"), e))
        if isinstance(getattr(o, k, None), bool) or not math.isfinite(x):
            raise SystemExit("--%s %r is not a finite number" % (k.replace("_", "-"), getattr(o, k, None)))
        v[name] = x
    if v["stddev"] < 0.0:
        raise SystemExit("--param-noise-stddev %r is not a standard deviation >= 0" % (s,))
    if not v["target"] > 0.0:
        raise SystemExit("--param-noise-target %r is not a distance > 0" % (getattr(o, "param_noise_target"),))
    if v["adapt"] < 1.0:
        raise SystemExit("--param-noise-adapt %r is not a factor >= 1 (1 keeps the standard deviation fixed)" % (getattr(o, "param_noise_adapt"),))
    r = getattr(o, "param_noise_adapt_rounds", None)
    r = _PARAM_NOISE_DEFAULTS["param_noise_adapt_rounds"] if r is None else r
    if isinstance(r, bool) or not isinstance(r, (int, np.integer)) or not 1 <= int(r) <= PARAM_NOISE_ROUNDS_MAX:
        raise SystemExit("--param-noise-adapt-rounds %r is not a whole number in [1, %d]" % (r, PARAM_NOISE_ROUNDS_MAX))
    seed = getattr(o, "param_noise_seed", None)
    seed = _PARAM_NOISE_DEFAULTS["param_noise_seed"] if seed is None else seed
    if isinstance(seed, bool) or not isinstance(seed, (int, np.integer)) or not 0 <= int(seed) < 2 ** 64:
        raise SystemExit("--param-noise-seed %r is not in [0, 2^64)" % (seed,))
    v["rounds"], v["seed"] = int(r), int(seed)
    if bool(getattr(o, "soft_actor_critic", False)):
        raise SystemExit("--param-noise-stddev cannot be combined with --soft-actor-critic (its policy explores by itself)")
    if bool(getattr(o, "use_batch_norm", False)):
        raise SystemExit("--param-noise-stddev cannot be combined with --use-batch-norm (the perturbed copy would be measured in inference "
                         "mode against statistics its weights never shaped; the paper's normalisation is --feature-layer-norm)")
    return v


FEATURE_NORM_ACTIVATIONS = ("tanh", "relu")
FEATURE_NORM_EPSILON = 1e-5      # torch.nn.LayerNorm's default, which DrQ-v2 uses (there is no flag for it)


def feature_layer_norm(o):
    """(activation, epsilon) of --feature-layer-norm / --feature-norm-activation, or None (off); refuses what cannot be meant."""
    on = bool(getattr(o, "feature_layer_norm", False))
    act = getattr(o, "feature_norm_activation", None)
    if not on:
        if act is not None:
            raise SystemExit("--feature-norm-activation needs --feature-layer-norm")
        return None
    act = "tanh" if act is None else act
    if act not in FEATURE_NORM_ACTIVATIONS:
        raise SystemExit("--feature-norm-activation %r is not one of %s" % (act, ", ".join(FEATURE_NORM_ACTIVATIONS)))
    if not bool(getattr(o, "use_raw_pixels", False)):
        raise SystemExit("--feature-layer-norm needs --use-raw-pixels: a low-dimensional network has no conv features to normalise")
    if bool(getattr(o, "use_batch_norm", False)):
        raise SystemExit("--feature-layer-norm cannot be combined with --use-batch-norm")
    if bool(getattr(o, "use_dropout", False)):
        raise SystemExit("--feature-layer-norm cannot be combined with --use-dropout")
    return (act, FEATURE_NORM_EPSILON)


DDPG_OPTIMISERS = {"GradientDescent": _lib.CPP_OPT_SGD, "Momentum": _lib.CPP_OPT_MOMENTUM, "Adam": _lib.CPP_OPT_ADAM}
_DDPG_OPTIMISER_DEFAULTS = {"momentum": 0.0, "beta1": 0.9, "beta2": 0.999, "epsilon": 1e-8}      # tf.train.AdamOptimizer's defaults


def ddpg_optimiser(o):
    """(kind, momentum, beta1, beta2, epsilon) of --ddpg-optimiser / --ddpg-optimiser-args; refuses what cannot be meant."""
    import json
    name = getattr(o, "ddpg_optimiser", "GradientDescent")
    if name not in DDPG_OPTIMISERS:
        raise SystemExit("--ddpg-optimiser %r is not one of %s" % (name, ", ".join(DDPG_OPTIMISERS)))
    try:
        args = json.loads(getattr(o, "ddpg_optimiser_args", None) or "{}")
    except ValueError as e:
        raise SystemExit("--ddpg-optimiser-args is not json: %s" % e)
    if not isinstance(args, dict):
        raise SystemExit("--ddpg-optimiser-args must be a json object")
    if "learning_rate" in args:
        raise SystemExit("--ddpg-optimiser-args takes no learning_rate: the two lists' rates are --actor-learning-rate and "
                         "--critic-learning-rate")
    unknown = sorted(set(args) - set(_DDPG_OPTIMISER_DEFAULTS))
    if unknown:
        raise SystemExit("--ddpg-optimiser-args: unknown key(s) %s (momentum, beta1, beta2, epsilon)" % ", ".join(unknown))
    v = dict(_DDPG_OPTIMISER_DEFAULTS)
    v.update({k: float(x) for k, x in args.items()})
    return (DDPG_OPTIMISERS[name], v["momentum"], v["beta1"], v["beta2"], v["epsilon"])


_TARGET_SMOOTHING_DEFAULTS = (0.0, 0.5, 0)      # sigma, clip, seed


def target_policy_smoothing(o):
    """(sigma, clip, seed) of --target-policy-noise / -clip / -seed; refuses what cannot be meant.  sigma == 0: off."""
    import math
    given_clip, given_seed = hasattr(o, "target_policy_noise_clip"), hasattr(o, "target_policy_noise_seed")
    try:
        sigma = float(getattr(o, "target_policy_noise", _TARGET_SMOOTHING_DEFAULTS[0]))
        clip = float(getattr(o, "target_policy_noise_clip", _TARGET_SMOOTHING_DEFAULTS[1]))
        seed = int(getattr(o, "target_policy_noise_seed", _TARGET_SMOOTHING_DEFAULTS[2]))
    except (TypeError, ValueError) as e:
        raise SystemExit("--target-policy-noise: %s" % e)
    if not math.isfinite(sigma) or sigma < 0.0:
        raise SystemExit("--target-policy-noise %r is not a finite standard deviation >= 0" % sigma)
    if not math.isfinite(clip) or clip < 0.0:
        raise SystemExit("--target-policy-noise-clip %r is not a finite bound >= 0" % clip)
    if not 0 <= seed < 2 ** 64:
        raise SystemExit("--target-policy-noise-seed %r is not in [0, 2^64)" % seed)
    if sigma == 0.0:
        # (default_opts() fills the defaults in: a clip or seed that IS the default says nothing)
        if (given_clip and clip != _TARGET_SMOOTHING_DEFAULTS[1]) or (given_seed and seed != _TARGET_SMOOTHING_DEFAULTS[2]):
            raise SystemExit("--target-policy-noise-clip / --target-policy-noise-seed need a noise: give --target-policy-noise SIGMA")
        return (0.0, clip, seed)
    if clip == 0.0:
        raise SystemExit("--target-policy-noise %g with --target-policy-noise-clip 0 would clip the noise away" % sigma)
    return (sigma, clip, seed)


_POLICY_DELAY_DEFAULT, POLICY_DELAY_MAX = 1, 65536


def policy_delay(o):
    """D of --policy-delay; refuses what cannot be meant.  1: off."""
    d = getattr(o, "policy_delay", _POLICY_DELAY_DEFAULT)
    if isinstance(d, bool) or not isinstance(d, (int, np.integer)):
        if isinstance(d, float) and d == int(d):
            d = int(d)
        else:
            raise SystemExit("--policy-delay %r is not a whole number of critic updates" % (d,))
    d = int(d)
    if not 1 <= d <= POLICY_DELAY_MAX:
        raise SystemExit("--policy-delay %d is outside [1, %d] (1: the actor is updated in every minibatch)" % (d, POLICY_DELAY_MAX))
    return d


def twin_q(o):
    """--twin-q; off unless given"""
    return bool(getattr(o, "twin_q", False))


def actor_min_q(o):
    """--actor-min-q; off unless given; refused without --twin-q"""
    on = bool(getattr(o, "actor_min_q", False))
    if on and not twin_q(o):
        raise SystemExit("--actor-min-q needs --twin-q (the minimum is over the two heads of twin critics)")
    return on


_BC_Q_FLOOR_DEFAULT = 1e-3


def behaviour_cloning(o):
    """(alpha, q_floor) of --bc-alpha / --bc-q-floor; (0.0, default floor) is off; refuses what cannot be meant"""
    import math
    alpha, floor = getattr(o, "bc_alpha", None), getattr(o, "bc_q_floor", None)
    if alpha is None or alpha == 0:
        if floor is not None:
            raise SystemExit("--bc-q-floor %r needs --bc-alpha (the floor is of the behaviour-cloning term's lambda)" % (floor,))
        return 0.0, _BC_Q_FLOOR_DEFAULT
    alpha, floor = float(alpha), float(_BC_Q_FLOOR_DEFAULT if floor is None else floor)
    if not (math.isfinite(alpha) and alpha > 0.0):
        raise SystemExit("--bc-alpha %r is not a finite weight >= 0" % (alpha,))
    if not (math.isfinite(floor) and floor > 0.0):
        raise SystemExit("--bc-q-floor %r is not a finite value > 0" % (floor,))
    for flag, name in (("soft_actor_critic", "--soft-actor-critic"), ("distributional_critic", "--distributional-critic"),
                       ("quantile_critic", "--quantile-critic")):
        if getattr(o, flag, False):
            raise SystemExit("--bc-alpha with %s (the behaviour-cloning term is of a deterministic actor on a scalar critic)" % name)
    return alpha, floor


_NUM_ATOMS_DEFAULT, NUM_ATOMS_MAX = 51, 64


def distributional_critic(o):
    """(n_atoms, v_min, v_max) of --distributional-critic / --num-atoms / --v-min / --v-max, or None (off); refuses what cannot be meant."""
    import math
    on = bool(getattr(o, "distributional_critic", False))
    given = [k for k in ("num_atoms", "v_min", "v_max") if getattr(o, k, None) is not None]
    if not on:
        if given:
            raise SystemExit("--%s needs --distributional-critic" % given[0].replace("_", "-"))
        return None
    if twin_q(o):
        raise SystemExit("--distributional-critic cannot be combined with --twin-q (one value distribution, one head)")
    if "v_min" not in given or "v_max" not in given:
        raise SystemExit("--distributional-critic needs --v-min and --v-max: no default support fits every reward scale")
    n = getattr(o, "num_atoms", None)
    n = _NUM_ATOMS_DEFAULT if n is None else n
    if isinstance(n, bool) or not isinstance(n, (int, np.integer)) or not 2 <= int(n) <= NUM_ATOMS_MAX:
        raise SystemExit("--num-atoms %r is not a whole number in [2, %d]" % (n, NUM_ATOMS_MAX))
    try:
        v_min, v_max = float(np.float32(o.v_min)), float(np.float32(o.v_max))
    except (TypeError, ValueError) as e:
        raise SystemExit("--v-min / --v-max: %s" % e)
    if not (math.isfinite(v_min) and math.isfinite(v_max) and v_min < v_max):
        raise SystemExit("--v-min %r, --v-max %r: both finite, --v-min below --v-max" % (o.v_min, o.v_max))
    return (int(n), v_min, v_max)


_NUM_QUANTILES_DEFAULT, NUM_QUANTILES_MAX, _QUANTILE_KAPPA_DEFAULT = 25, 64, 1.0


def quantile_critic(o):
    """(n_quantiles, kappa, drop_top) of --quantile-critic / --num-quantiles / --quantile-huber-kappa / --drop-top-quantiles, or None
    (off); refuses what cannot be meant."""
    import math
    on = bool(getattr(o, "quantile_critic", False))
    given = [k for k in ("num_quantiles", "quantile_huber_kappa", "drop_top_quantiles") if getattr(o, k, None) is not None]
    if not on:
        if given:
            raise SystemExit("--%s needs --quantile-critic" % given[0].replace("_", "-"))
        return None
    if twin_q(o):
        raise SystemExit("--quantile-critic cannot be combined with --twin-q (--drop-top-quantiles is its overestimation control)")
    if bool(getattr(o, "distributional_critic", False)):
        raise SystemExit("--quantile-critic cannot be combined with --distributional-critic (one value distribution per critic)")
    n = getattr(o, "num_quantiles", None)
    n = _NUM_QUANTILES_DEFAULT if n is None else n
    if isinstance(n, bool) or not isinstance(n, (int, np.integer)) or not 2 <= int(n) <= NUM_QUANTILES_MAX:
        raise SystemExit("--num-quantiles %r is not a whole number in [2, %d]" % (n, NUM_QUANTILES_MAX))
    d = getattr(o, "drop_top_quantiles", None)
    d = 0 if d is None else d
    if isinstance(d, bool) or not isinstance(d, (int, np.integer)) or not 0 <= int(d) <= int(n) - 1:
        raise SystemExit("--drop-top-quantiles %r is not a whole number in [0, %d] (at least one target quantile stays)" % (d, int(n) - 1))
    k = getattr(o, "quantile_huber_kappa", None)
    try:
        k = _QUANTILE_KAPPA_DEFAULT if k is None else float(np.float32(k))
    except (TypeError, ValueError) as e:
        raise SystemExit("--quantile-huber-kappa: %s" % e)
    if not (math.isfinite(k) and k > 0.0):
        raise SystemExit("--quantile-huber-kappa %r is not finite and positive" % (getattr(o, "quantile_huber_kappa", None),))
    return (int(n), k, int(d))


_POOLED_NUM_QUANTILES_DEFAULT, POOLED_NUM_QUANTILES_MAX, _POOLED_DROP_DEFAULT, _POOLED_KAPPA_DEFAULT = 25, 32, 2, 1.0


def pooled_quantile_critics(o):
    """(n_quantiles per head, kappa, drop per head) of --pooled-quantile-critics / --pooled-num-quantiles / --pooled-huber-kappa /
    --pooled-drop-per-head, or None (off); refuses what cannot be meant."""
    import math
    on = bool(getattr(o, "pooled_quantile_critics", False))
    given = [k for k in ("pooled_num_quantiles", "pooled_drop_per_head", "pooled_huber_kappa") if getattr(o, k, None) is not None]
    if not on:
        if given:
            raise SystemExit("--%s needs --pooled-quantile-critics" % given[0].replace("_", "-"))
        return None
    for flag, name, why in (("quantile_critic", "--quantile-critic", "it makes its own two quantile heads"),
                            ("distributional_critic", "--distributional-critic", "one value distribution per head"),
                            ("twin_q", "--twin-q", "it makes its own two heads"),
                            ("actor_min_q", "--actor-min-q", "its actor ascends the mean over all atoms of both heads")):
        if bool(getattr(o, flag, False)):
            raise SystemExit("--pooled-quantile-critics cannot be combined with %s (%s)" % (name, why))
    alpha = getattr(o, "bc_alpha", None)
    if alpha is not None and alpha != 0:
        raise SystemExit("--pooled-quantile-critics cannot be combined with --bc-alpha (the behaviour-cloning term is of a scalar critic)")
    n = getattr(o, "pooled_num_quantiles", None)
    n = _POOLED_NUM_QUANTILES_DEFAULT if n is None else n
    if isinstance(n, bool) or not isinstance(n, (int, np.integer)) or not 2 <= int(n) <= POOLED_NUM_QUANTILES_MAX:
        raise SystemExit("--pooled-num-quantiles %r is not a whole number in [2, %d] (the pool of both heads fills one wave)" % (n, POOLED_NUM_QUANTILES_MAX))
    d = getattr(o, "pooled_drop_per_head", None)
    d = min(_POOLED_DROP_DEFAULT, int(n) - 1) if d is None else d
    if isinstance(d, bool) or not isinstance(d, (int, np.integer)) or not 0 <= int(d) <= int(n) - 1:
        raise SystemExit("--pooled-drop-per-head %r is not a whole number in [0, %d] (at least two atoms of the pool stay)" % (d, int(n) - 1))
    k = getattr(o, "pooled_huber_kappa", None)
    try:
        k = _POOLED_KAPPA_DEFAULT if k is None else float(np.float32(k))
    except (TypeError, ValueError) as e:
        raise SystemExit("--pooled-huber-kappa: %s" % e)
    if isinstance(getattr(o, "pooled_huber_kappa", None), bool) or not (math.isfinite(k) and k > 0.0):
        raise SystemExit("--pooled-huber-kappa %r is not finite and positive" % (getattr(o, "pooled_huber_kappa", None),))
    return (int(n), k, int(d))


_SAC_DEFAULTS = {"sac_init_temperature": 0.1, "sac_target_entropy": None, "sac_temperature_learning_rate": 1e-4,
                 "sac_log_std_min": -10.0, "sac_log_std_max": 2.0, "sac_seed": 0}
SAC_ACTION_DIM_MAX = 64


def soft_actor_critic(o, action_dim=None):
    """{init_temperature, target_entropy (None: -action_dim, filled in when action_dim is given), temperature_learning_rate, log_std_min,
    log_std_max, seed} of --soft-actor-critic and its --sac-* flags, or None (off); refuses what cannot be meant."""
    import math
    on = bool(getattr(o, "soft_actor_critic", False))
    given = [k for k in _SAC_DEFAULTS if getattr(o, k, None) is not None]
    if not on:
        if given:
            raise SystemExit("--%s needs --soft-actor-critic" % given[0].replace("_", "-"))
        return None
    if float(getattr(o, "target_policy_noise", 0.0) or 0.0) > 0.0:
        raise SystemExit("--soft-actor-critic cannot be combined with --target-policy-noise (its target action is a sample already)")
    if policy_delay(o) > 1:
        raise SystemExit("--soft-actor-critic cannot be combined with --policy-delay above 1")
    if bool(getattr(o, "distributional_critic", False)):
        raise SystemExit("--soft-actor-critic cannot be combined with --distributional-critic")
    if bool(getattr(o, "quantile_critic", False)):
        raise SystemExit("--soft-actor-critic cannot be combined with --quantile-critic")
    if bool(getattr(o, "use_batch_norm", False)):
        raise SystemExit("--soft-actor-critic cannot be combined with --use-batch-norm")
    if bool(getattr(o, "use_dropout", False)):
        raise SystemExit("--soft-actor-critic cannot be combined with --use-dropout")
    if bool(getattr(o, "data_parallel", False)):
        raise SystemExit("--soft-actor-critic is not supported by the data-parallel step (the temperature's gradient is not reduced): drop --data-parallel")
    v = {}
    for k, dflt in _SAC_DEFAULTS.items():
        x = getattr(o, k, None)
        x = dflt if x is None else x
        if k == "sac_seed":
            if isinstance(x, bool) or not isinstance(x, (int, np.integer)) or not 0 <= int(x) < 2 ** 64:
                raise SystemExit("--sac-seed %r is not in [0, 2^64)" % (x,))
            v[k[4:]] = int(x)
            continue
        if x is None:
            v[k[4:]] = None
            continue
        try:
            x = float(np.float32(x))
        except (TypeError, ValueError) as e:
            raise SystemExit("--%s: %s" % (k.replace("_", "-"), e))
        if not math.isfinite(x):
            raise SystemExit("--%s %r is not finite" % (k.replace("_", "-"), getattr(o, k, None)))
        v[k[4:]] = x
    if not v["init_temperature"] > 0.0:
        raise SystemExit("--sac-init-temperature %r is not positive" % v["init_temperature"])
    if v["temperature_learning_rate"] < 0.0:
        raise SystemExit("--sac-temperature-learning-rate %r is negative (0: a fixed temperature)" % v["temperature_learning_rate"])
    if not v["log_std_min"] < v["log_std_max"]:
        raise SystemExit("--sac-log-std-min %r is not below --sac-log-std-max %r" % (v["log_std_min"], v["log_std_max"]))
    if action_dim is not None:
        if not 1 <= int(action_dim) <= SAC_ACTION_DIM_MAX:
            raise SystemExit("--soft-actor-critic takes action dimensions up to %d (got %d)" % (SAC_ACTION_DIM_MAX, int(action_dim)))
        if v["target_entropy"] is None:
            v["target_entropy"] = -float(action_dim)
    return v


def n_step(o):
    """n of --n-step; 1 (off) unless given"""
    n = getattr(o, "n_step", 1)
    if isinstance(n, bool) or not isinstance(n, (int, np.integer)) or not 1 <= int(n) <= 64:
        raise SystemExit("--n-step %r is not a whole number in [1, 64]" % (n,))
    return int(n)


def priority_beta(o, train_steps):
    """beta of the outer train step `train_steps` (linear from --priority-beta to --priority-beta-final)"""
    n = max(1, int(o.priority_beta_steps))
    f = min(1.0, max(0, int(train_steps)) / float(n))
    return float(o.priority_beta) + f * (float(o.priority_beta_final) - float(o.priority_beta))


def check_prioritized_opts(o):
    """--prioritized-replay's refusals at startup"""
    if not getattr(o, "prioritized_replay", False):
        return
    if o.host_rng_sampling:
        raise SystemExit("--prioritized-replay draws minibatches by priority on the device: it cannot be combined with --host-rng-sampling")
    if o.data_parallel:
        raise SystemExit("--prioritized-replay is not supported by the data-parallel step (per-shard trees): drop --data-parallel")


def default_opts(**overrides):
    o = build_parser().parse_args([])
    o.ddpg_optimiser, o.ddpg_optimiser_args = "GradientDescent", "{}"
    o.target_policy_noise, o.target_policy_noise_clip, o.target_policy_noise_seed = _TARGET_SMOOTHING_DEFAULTS
    o.policy_delay = _POLICY_DELAY_DEFAULT
    o.twin_q = False
    o.actor_min_q = False
    o.bc_alpha, o.bc_q_floor = None, None
    o.distributional_critic, o.num_atoms, o.v_min, o.v_max = False, None, None, None
    o.quantile_critic, o.num_quantiles, o.quantile_huber_kappa, o.drop_top_quantiles = False, None, None, None
    o.pooled_quantile_critics, o.pooled_num_quantiles, o.pooled_drop_per_head, o.pooled_huber_kappa = False, None, None, None
    o.n_step = 1
    o.soft_actor_critic = False
    o.feature_layer_norm, o.feature_norm_activation = False, None
    o.shared_encoder = False
    o.random_shift, o.random_shift_seed = None, None
    o.param_noise_stddev = None
    for k in _PARAM_NOISE_DEFAULTS:
        setattr(o, k, None)
    for k in _SAC_DEFAULTS:
        setattr(o, k, None)
    for k, v in overrides.items():
        assert hasattr(o, k), k
        setattr(o, k, v)
    return o


opts = default_opts()        # module global, as in the reference (ddpg_cartpole.py:56)


def set_opts(o):
    global opts
    opts = o


def _hidden(spec):
    return [int(s) for s in str(spec).split(",")]


class _OpHandle(object):
    """names a fetchable 'tensor' of a network (output_action, q_value, train_op ...)."""

    def __init__(self, name):
        self.name = name

    def __repr__(self):
        return "<op %s>" % self.name


class ActorNetwork(base_network.Network):
    """ the actor represents the learnt policy mapping states to actions"""

    def __init__(self, namespace, input_state, action_dim):
        super(ActorNetwork, self).__init__(namespace)
        self.input_state = input_state
        self.action_dim = int(action_dim)
        self.exploration_noise = util.OrnsteinUhlenbeckNoise(action_dim, opts.action_noise_theta,
                                                             opts.action_noise_sigma)
        opts.hidden_layers = opts.actor_hidden_layers                 # ddpg_cartpole.py:91
        # --shared-encoder: no simple_conv_net_on -- the hidden stack starts at the conv features of the critic this actor is given to
        # (CriticNetwork.__init__ binds it; until then forward refuses)
        self.shared_encoder = shared_encoder(opts)
        if self.shared_encoder:
            shape = self.input_state.get_shape()
            self._state_elems = int(np.prod([int(d) for d in shape[1:]]))
            self._conv_input = (int(shape[1]), int(shape[2]), int(np.prod([int(d) for d in shape[3:]])))
            self.hidden_layers_starting_at(self.input_state, opts.hidden_layers, opts)
        else:
            self.input_state_network(self.input_state, opts)
        # --soft-actor-critic: output_action emits (m | x), 2A wide; forward returns tanh(m), exploration samples on the host
        self.sac = soft_actor_critic(opts, action_dim)
        # --feature-layer-norm: h0 is Linear -> LayerNorm -> tanh (the same in every forward: there is no training / inference distinction)
        self.feature_norm = feature_layer_norm(opts)
        self._build_native(_lib.CPP_ACTOR, action_dim, max(int(opts.batch_size), 1),
                           gaussian=(self.sac["log_std_min"], self.sac["log_std_max"]) if self.sac else None, feature_norm=self.feature_norm,
                           encoderless=self.shared_encoder)
        self._sac_rng = np.random.default_rng(self.sac["seed"]) if self.sac else None
        self.output_action = _OpHandle(namespace + "/output_action")
        self.train_op = None
        self.critic = None
        # --param-noise-stddev: the copy of this actor that explores in its place (the agent's 'perturbed_actor'); None: this actor itself,
        # with the Ornstein-Uhlenbeck process
        self.perturbed = None

    def init_ops_for_training(self, critic):
        # gradients of output_action w.r.t. the actor's variables with grad_ys = -dQ/da from the critic
        # (sum over the batch), clipped by global norm, applied with plain SGD (ddpg_cartpole.py:102-119)
        self.critic = critic
        critic._register_actor_training(self)
        self.train_op = _OpHandle(self.namespace + "/optimiser/train_op")

    def forward(self, states):
        """output_action for a host batch of states (B, ...) -> (B, action_dim)."""
        s, dt = _lib.as_state_array(states)
        B = s.shape[0]
        out = np.empty((B, self.action_dim), np.float32)
        check(lib.cpp_net_forward(self.handle, ptr(s), dt, B, None, ptr(out)))
        return out

    def actions_given(self, states, add_noise=False):
        """`action_given` for many env workers at once: states (B, ...) -> actions (B, action_dim),
        row i identical to action_given(states[i]) -- every image is whitened with its own statistics.  With
        add_noise each row gets its own Ornstein-Uhlenbeck process (one per worker, created on first use)."""
        s, dt = _lib.as_state_array(states)
        B = s.shape[0]
        if self.sac and add_noise:
            return self._sample_gaussian(s, dt, B, each=True)
        if add_noise and self.perturbed is not None:      # --param-noise-stddev: the perturbed copy's own actions; tanh bounds them
            return self.perturbed.actions_given(s)
        actions = np.empty((B, self.action_dim), np.float32)
        check(lib.cpp_net_forward_each(self.handle, ptr(s), dt, B, None, ptr(actions)))
        if add_noise:
            procs = self.__dict__.setdefault("_worker_noise", [])
            while len(procs) < B:
                procs.append(util.OrnsteinUhlenbeckNoise(self.action_dim, opts.action_noise_theta, opts.action_noise_sigma))
            for i in range(B):
                actions[i] += procs[i].sample()
            actions = np.minimum(1, actions)     # the reference's clip quirk, per row (:134)
        return actions

    def forward_gaussian(self, states, each=False):
        """(m, ls), each (B, action_dim): the head of a --soft-actor-critic actor on a host batch of states (cpp_net_forward_gaussian)"""
        s, dt = _lib.as_state_array(states)
        B = s.shape[0]
        m, ls = np.empty((B, self.action_dim), np.float32), np.empty((B, self.action_dim), np.float32)
        check(lib.cpp_net_forward_gaussian(self.handle, ptr(s), dt, B, 1 if each else 0, ptr(m), ptr(ls)))
        return m, ls

    def _sample_gaussian(self, s, dt, B, each):
        # tanh(m + exp(ls) z), z from numpy's generator: the policy's own exploration replaces the Ornstein-Uhlenbeck process; like it,
        # the noise stays outside the device graph (:127-134)
        m, ls = self.forward_gaussian(s, each)
        z = self._sac_rng.standard_normal((B, self.action_dim)).astype(np.float32)
        return np.tanh(m + np.exp(ls) * z).astype(np.float32)

    def action_given(self, state, add_noise=False):
        # feed explicitly provided state (batch of one; whitening uses this image's own statistics)
        if self.sac and add_noise:
            s, dt = _lib.as_state_array(np.asarray(state)[None])
            return self._sample_gaussian(s, dt, 1, each=False)
        if add_noise and self.perturbed is not None:
            # --param-noise-stddev: the exploration is in the weights of the perturbed copy (redrawn by agent.begin_episode, consistent
            # within the episode); no Ornstein-Uhlenbeck sample, and no clip: tanh bounds the action
            actions = self.perturbed.forward(np.asarray(state)[None])
            if VERBOSE_DEBUG:
                print("TRAIN action_given pre_noise %s post_noise %s" % (self.forward(np.asarray(state)[None]), actions))
            return actions
        actions = self.forward(np.asarray(state)[None])
        # NOTE: noise is added outside the device graph, as in the reference (:127-134)
        if add_noise:
            if VERBOSE_DEBUG:
                pre_noise = str(actions)
            actions[0] += self.exploration_noise.sample()
            actions = np.minimum(1, actions)     # np.clip(1, -1, actions): upper bound only (:134)
            if VERBOSE_DEBUG:
                print("TRAIN action_given pre_noise %s post_noise %s" % (pre_noise, actions))
        return actions

    def train(self, state):
        # training actor only requires state since we are trying to maximise the q_value according
        # to the critic (ddpg_cartpole.py:140-145).  `state` may be a host array or a device Batch.
        if self.critic is None:
            raise Exception("init_ops_for_training not called")
        trainer = self.critic._trainer()
        # the reference's loop calls `actor.train(batch.state_1)` and then `critic.train(batch)` (:333-334).  When `state` is the
        # state_1 COLUMN of a replay Batch, the update is deferred: if the critic's call on the same Batch follows, both run as the
        # fused device sequence of train_step on those rows (legal: the critic's update never reads the live actor and the actor's
        # never writes the critic); anything else that touches the actor or the trainer first runs it on its own (_Trainer.flush).
        if (isinstance(state, replay_memory.StateColumn) and state.field == "state_1" and state.batch.in_replay()
                and self.critic.target_critic is not None):
            trainer.defer_actor(self, state.batch)
            return
        if trainer.behaviour_cloning[0] > 0.0:
            # --bc-alpha: the update regresses onto the minibatch's stored actions, which only a Batch carries (its device copy, or its
            # columns uploaded whole)
            b = state.batch if isinstance(state, replay_memory.StateColumn) else state
            if not hasattr(b, "action"):
                raise ValueError("actor.train(state) on a host array has no actions to clone: with --bc-alpha pass a Batch or its state_1 column")
            dev = trainer.device_batch_for(b)
        else:
            dev = trainer.device_batch_for(state, state_only=True)
        check(lib.cpp_ddpg_train_actor(trainer.handle, dev.handle))
        if opts.print_gradients:
            print("gradient %s l2_norm %s" % (self.namespace, trainer.last_stats()[1]))


class _Trainer(object):
    """owns the cpp_ddpg handle that binds (actor, critic, target_actor, target_critic) and the
    hyper-parameters -- the 'optimiser' variable scope of the reference."""

    def __init__(self, actor, critic, target_actor, target_critic):
        hp = _lib.DdpgHyper(float(opts.actor_learning_rate), float(opts.critic_learning_rate),
                            float(opts.discount), util.gradient_clip_value(opts),
                            float(opts.target_update_rate))
        h = C.c_void_p()
        check(lib.cpp_ddpg_create(actor.ctx.handle, actor.handle, critic.handle, target_actor.handle,
                                  target_critic.handle, C.byref(hp), C.byref(h)))
        self._h, self.ctx = h, actor.ctx
        # (the default rule needs no call: cpp_ddpg_create's trainer is GradientDescent, and stays what it was before the rule could be chosen;
        # the rule is the one parsed when the critic's train op was declared, not whatever the module's options say by now)
        rule = getattr(critic, "_optimiser", None) or ddpg_optimiser(opts)
        self.optimiser_kind = rule[0]
        if self.optimiser_kind != _lib.CPP_OPT_SGD:
            check(lib.cpp_ddpg_set_optimiser(h, *rule))
        self.nets = (actor, critic, target_actor, target_critic)
        self.state_elems = int(actor._state_elems)
        self.action_dim = int(actor.action_dim)
        self._upload = {}
        self._pending = None         # (actor network, Batch) of a deferred actor.train(batch.state_1)
        self.fused_pairs = 0         # actor.train + critic.train pairs that ran as one fused sequence (tests, profiles)
        # target policy smoothing, as parsed when the critic's train op was declared (off, the trainer's state as created, needs no call)
        smoothing = getattr(critic, "_target_smoothing", None) or target_policy_smoothing(opts)
        self.target_smoothing = (0.0, 0.0, 0)
        if smoothing[0] > 0.0:
            self.set_target_smoothing(*smoothing)
        # delayed policy updates, as parsed when the critic's train op was declared (1: off, the trainer's state as created, needs no call)
        delay = getattr(critic, "_policy_delay", None) or policy_delay(opts)
        self.policy_delay = 1
        if delay > 1:
            self.set_policy_delay(delay)
        # --quantile-critic: the Huber threshold and the dropped top target quantiles, as parsed when the critic was built
        quantiles = getattr(critic, "quantiles", None)
        if quantiles:
            self.set_quantile_target(quantiles[1], quantiles[2])
        # --pooled-quantile-critics: the Huber threshold and the atoms dropped per head, as parsed when the critic was built
        pooled = getattr(critic, "pooled", None)
        if pooled:
            self.set_quantile_target(pooled[1], pooled[2])
        # --soft-actor-critic: temperature, target entropy, rate and seed, as parsed when the actor was built
        self.sac = getattr(actor, "sac", None)
        if self.sac:
            self.set_sac(self.sac["init_temperature"], self.sac["target_entropy"], self.sac["temperature_learning_rate"], self.sac["seed"])
        # --actor-min-q, as parsed when the critic's train op was declared (off, the trainer's state as created, needs no call)
        self.actor_min_q = False
        amin = getattr(critic, "_actor_min_q", None)
        if actor_min_q(opts) if amin is None else amin:
            self.set_actor_min_q(True)
        # --bc-alpha / --bc-q-floor, as parsed when the critic's train op was declared (off, the trainer's state as created, needs no call)
        self.behaviour_cloning = (0.0, _BC_Q_FLOOR_DEFAULT)
        bc = getattr(critic, "_behaviour_cloning", None) or behaviour_cloning(opts)
        if bc[0] > 0.0:
            self.set_behaviour_cloning(*bc)
        # --param-noise-stddev: off until the agent hands over its perturbed copy (set_param_noise); the trainer's state as created
        self.param_noise = None

    @property
    def handle(self):
        """the cpp_ddpg; a deferred actor update lands first (every trainer op but the fused pair goes through here)."""
        self.flush()
        return self._h

    def defer_actor(self, actor, batch):
        self.flush()
        self._pending = (actor, batch)
        actor._before_use = self.flush

    def flush(self):
        """run a deferred actor.train now, on its own (ddpg_cartpole.py:140-145)."""
        if self._pending is None:
            return
        (actor, batch), self._pending = self._pending, None
        actor._before_use = None
        check(lib.cpp_ddpg_train_actor(self._h, batch.device.handle))
        if opts.print_gradients:
            print("gradient %s l2_norm %s" % (actor.namespace, self.last_stats()[1]))

    def train_pair(self, batch):
        """critic.train(batch) arriving right behind the deferred actor.train(batch.state_1) of the SAME draw: both updates as the
        fused minibatch of cpp_ddpg_train_step on the draw's rows (cpp_ddpg_train_rows); False if that is not the situation."""
        if self._pending is None or self._pending[1] is not batch or not batch.in_replay():
            return False
        (actor, _), self._pending = self._pending, None
        actor._before_use = None
        rm = batch._memory
        check(lib.cpp_ddpg_train_rows(self._h, rm.handle, len(batch.idxs), ptr(batch.idxs)))
        self.fused_pairs += 1
        if opts.print_gradients:
            st = self.last_stats()
            print("gradient %s l2_norm %s" % (actor.namespace, st[1]))
            print("gradient %s l2_norm %s" % (self.nets[1].namespace, st[2]))
        return True

    def device_batch_for(self, batch, state_only=False):
        self.flush()          # (a deferred actor update gathers ITS draw into the shared minibatch buffer: before this one's, not after)
        if isinstance(batch, replay_memory.StateColumn):          # a state column of a replay Batch: its rows, gathered on the device
            batch = batch.batch
        if isinstance(batch, replay_memory.Batch) and batch.device is not None:
            return batch.device
        if state_only:
            s1 = np.asarray(batch.state_1 if hasattr(batch, "state_1") else batch)
            B = s1.shape[0]
            args = (s1, None, None, None, None)
        else:
            s1 = np.asarray(batch.state_1)
            B = s1.shape[0]
            args = (s1, batch.action, batch.reward, batch.terminal_mask, batch.state_2)
        if B not in self._upload:
            self._upload[B] = replay_memory.DeviceBatch(B, self.state_elems, self.action_dim, self.ctx)
        return self._upload[B].upload(*args)

    def last_stats(self):
        out = np.zeros(3, np.float32)
        check(lib.cpp_ddpg_last_stats(self.handle, ptr(out)))
        return out

    def last_values(self, B):
        """(actions, dq_da, q, td) of the last minibatch's gradient pass, as the device left them -- the values the
        reference dumps under VERBOSE_DEBUG (ddpg_cartpole.py:339-349); also after a fused / graph-replayed train_step."""
        B, A = int(B), self.action_dim
        actions, dq_da = np.empty((B, A), np.float32), np.empty((B, A), np.float32)
        q, td = np.empty((B, 1), np.float32), np.empty((B, 1), np.float32)
        check(lib.cpp_ddpg_last_values(self.handle, B, ptr(actions), ptr(dq_da), ptr(q), ptr(td)))
        return actions, dq_da, q, td

    def last_twin_values(self, B):
        """(q2, target_q1, target_q2, td2) of the last minibatch's gradient pass of a --twin-q trainer, each (B, 1): head 2 on the fed
        action, the two target heads at the (smoothed) target action, head 2's temporal difference (last_values has head 1's)"""
        B = int(B)
        out = [np.empty((B, 1), np.float32) for _ in range(4)]
        check(lib.cpp_ddpg_last_twin_values(self.handle, B, *[ptr(x) for x in out]))
        return tuple(out)

    def last_distribution(self, B):
        """(p, target_p, m) of the last minibatch's gradient pass of a --distributional-critic trainer, each (B, num_atoms): the fed
        evaluation's distribution, the target critic's at the (smoothed) target action, the projected Bellman target"""
        B = int(B)
        dist = getattr(self.nets[1], "distribution", None)
        n = dist[0] if dist else 1
        out = [np.empty((B, n), np.float32) for _ in range(3)]
        check(lib.cpp_ddpg_last_distribution(self.handle, B, *[ptr(x) for x in out]))
        return tuple(out)

    def last_quantiles(self, B):
        """(theta, sorted_target_theta, y) of the last minibatch's gradient pass of a --quantile-critic trainer, each (B, num_quantiles):
        the fed evaluation's quantiles, the target critic's at the (smoothed) target action sorted ascending, and y_j = r + g s_j with
        the columns of the dropped quantiles zero"""
        B = int(B)
        q = getattr(self.nets[1], "quantiles", None)
        n = q[0] if q else 1
        out = [np.empty((B, n), np.float32) for _ in range(3)]
        check(lib.cpp_ddpg_last_quantiles(self.handle, B, *[ptr(x) for x in out]))
        return tuple(out)

    def last_pooled_quantiles(self, B):
        """(theta1, theta2, sorted_pool, y) of the last minibatch's gradient pass of a --pooled-quantile-critics trainer: both heads' quantiles
        of the fed evaluation, each (B, N); both target heads' atoms at the one target action pooled and sorted ascending, and
        y_j = r* + g s_j with the columns j >= 2N - 2d zero, each (B, 2N)"""
        B = int(B)
        p = getattr(self.nets[1], "pooled", None)
        n = p[0] if p else 1
        out = [np.empty((B, n), np.float32), np.empty((B, n), np.float32), np.empty((B, 2 * n), np.float32), np.empty((B, 2 * n), np.float32)]
        check(lib.cpp_ddpg_last_pooled_quantiles(self.handle, B, *[ptr(x) for x in out]))
        return tuple(out)

    def set_sac(self, init_temperature, target_entropy, temperature_lr, seed):
        """soft actor-critic's temperature, target entropy, temperature rate (0: fixed) and noise seed (include/cartpolepp_abi.h,
        cpp_ddpg_set_sac); zeroes the noise count and the temperature's Adam state, drops the captured graphs."""
        check(lib.cpp_ddpg_set_sac(self.handle, float(init_temperature), float(target_entropy), float(temperature_lr), int(seed)))

    def last_sac(self, B):
        """what the last gradient pass of a --soft-actor-critic trainer left: dict of eps, a (B, A), logp (B) of the draw at state_1,
        eps2, a2, logp2 of the draw at state_2, r_soft (B), alpha, g_alpha, the noise count n and dz, the head gradient (d m | d x), (B, 2A)"""
        B, A = int(B), self.action_dim
        o = {k: np.empty((B, A), np.float32) for k in ("eps", "a", "eps2", "a2")}
        o.update({k: np.empty(B, np.float32) for k in ("logp", "logp2", "r_soft")})
        o["dz"] = np.empty((B, 2 * A), np.float32)
        alpha, g, n = C.c_float(), C.c_float(), C.c_uint64()
        check(lib.cpp_ddpg_last_sac(self.handle, B, ptr(o["eps"]), ptr(o["a"]), ptr(o["logp"]), ptr(o["eps2"]), ptr(o["a2"]), ptr(o["logp2"]),
                                    ptr(o["r_soft"]), C.byref(alpha), C.byref(g), C.byref(n), ptr(o["dz"])))
        o.update(alpha=float(alpha.value), g_alpha=float(g.value), n=int(n.value))
        return o

    def last_feature_norm(self, B):
        """what the last gradient pass of a --feature-layer-norm trainer left of the normalised layer: {"actor": .., "critic": ..}, each a
        dict of xhat, y, dz (B, n), rstd (B) and dgamma, dbeta (n) before the clip, n the width of that network's first fully connected layer"""
        B, out = int(B), {}
        for which, (name, net) in enumerate((("actor", self.nets[0]), ("critic", self.nets[1]))):
            n = [v for v in net.trainable_model_vars() if v.name.endswith("/LayerNorm/gamma:0")]
            n = n[0].shape[0] if n else 1
            o = {k: np.empty((B, n), np.float32) for k in ("xhat", "y", "dz")}
            o["rstd"] = np.empty(B, np.float32)
            o.update({k: np.empty(n, np.float32) for k in ("dgamma", "dbeta")})
            check(lib.cpp_ddpg_last_feature_norm(self.handle, B, which, ptr(o["xhat"]), ptr(o["rstd"]), ptr(o["y"]), ptr(o["dz"]),
                                                 ptr(o["dgamma"]), ptr(o["dbeta"])))
            out[name] = o
        return out

    def get_sac_state(self):
        """{log_alpha, m, v, step}: the temperature and its Adam state (checkpoints; the noise count is not part of it)"""
        la, m, v, t = C.c_float(), C.c_float(), C.c_float(), C.c_uint64()
        check(lib.cpp_ddpg_sac_temperature(self.handle, 0, C.byref(la), C.byref(m), C.byref(v), C.byref(t)))
        return {"log_alpha": np.float32(la.value), "m": np.float32(m.value), "v": np.float32(v.value), "step": np.uint64(t.value)}

    def set_sac_state(self, state):
        la, m, v = (C.c_float(float(np.asarray(state[k]).reshape(()))) for k in ("log_alpha", "m", "v"))
        t = C.c_uint64(int(np.asarray(state["step"]).reshape(())))
        check(lib.cpp_ddpg_sac_temperature(self.handle, 1, C.byref(la), C.byref(m), C.byref(v), C.byref(t)))

    def set_quantile_target(self, kappa, drop_top):
        """the quantile Huber threshold and the number of largest target quantiles dropped (include/cartpolepp_abi.h,
        cpp_ddpg_set_quantile_target); drops the captured graphs."""
        check(lib.cpp_ddpg_set_quantile_target(self.handle, float(kappa), int(drop_top)))
        self.quantile_target = (float(kappa), int(drop_top))

    def set_target_smoothing(self, sigma, clip, seed):
        """target policy smoothing of the critic's target (include/cartpolepp_abi.h, cpp_ddpg_set_target_smoothing): sigma > 0 switches
        it on, (0, 0, seed) off; zeroes the count of target-forming passes and drops the captured graphs."""
        check(lib.cpp_ddpg_set_target_smoothing(self.handle, float(sigma), float(clip), int(seed)))
        self.target_smoothing = (float(sigma), float(clip), int(seed))

    def last_target_noise(self, B):
        """((B, action_dim) clipped noise of the last target-forming pass, the count n it was drawn at)"""
        eps, n = np.empty((int(B), self.action_dim), np.float32), C.c_uint64()
        check(lib.cpp_ddpg_last_target_noise(self.handle, int(B), ptr(eps), C.byref(n)))
        return eps, int(n.value)

    def set_policy_delay(self, delay):
        """delayed policy updates (include/cartpolepp_abi.h, cpp_ddpg_set_policy_delay): the actor's list is applied with every
        delay-th critic update; 1 switches it off; zeroes the count of critic updates and drops the captured graphs."""
        check(lib.cpp_ddpg_set_policy_delay(self.handle, int(delay)))
        self.policy_delay = int(delay)

    def set_actor_min_q(self, on):
        """the actor on the minimum head (include/cartpolepp_abi.h, cpp_ddpg_set_actor_min_q; twin critics only): dq_da and the actor's
        list follow the smaller of Q1 and Q2 at mu(state_1), row by row; off restores the actor on Q1; drops the captured graphs."""
        check(lib.cpp_ddpg_set_actor_min_q(self.handle, 1 if on else 0))
        self.actor_min_q = bool(on)

    def last_actor_min(self, B):
        """(q1, q2, sel) of the last gradient pass of an --actor-min-q trainer: Q1 and Q2 at mu(state_1), each (B, 1) float32, and the
        head each row followed, (B,) int32, 1 or 2"""
        B = int(B)
        q1, q2, sel = np.empty((B, 1), np.float32), np.empty((B, 1), np.float32), np.empty(B, np.int32)
        check(lib.cpp_ddpg_last_actor_min(self.handle, B, ptr(q1), ptr(q2), ptr(sel)))
        return q1, q2, sel

    def set_behaviour_cloning(self, alpha, q_floor=_BC_Q_FLOOR_DEFAULT):
        """the behaviour-cloning actor term (include/cartpolepp_abi.h, cpp_ddpg_set_behaviour_cloning; TD3+BC): the actor's grad_ys become
        -lambda dQ/da + (2/A)(mu - a) with lambda = alpha / max(mean|Q|, q_floor) of each minibatch and a its stored action; alpha 0 is off;
        drops the captured graphs."""
        check(lib.cpp_ddpg_set_behaviour_cloning(self.handle, float(alpha), float(q_floor)))
        self.behaviour_cloning = (float(alpha), float(q_floor))

    def last_behaviour_cloning(self, B):
        """(lambda, m, g, bc_rows) of the last gradient pass of a --bc-alpha trainer that ran the actor's half: two floats, the grad_ys at
        the actor's output, (B, A) float32, and (1/A) sum_i (mu - a)^2 per row, (B,) float32"""
        B = int(B)
        lam, m = np.empty(1, np.float32), np.empty(1, np.float32)
        g, rows = np.empty((B, self.action_dim), np.float32), np.empty(B, np.float32)
        check(lib.cpp_ddpg_last_behaviour_cloning(self.handle, B, ptr(lam), ptr(m), ptr(g), ptr(rows)))
        return float(lam[0]), float(m[0]), g, rows

    def set_param_noise(self, perturbed_actor, stddev=0.0, target=0.1, adapt=1.0, seed=0):
        """parameter-space exploration noise (include/cartpolepp_abi.h, cpp_ddpg_set_param_noise): `perturbed_actor`, an ActorNetwork with
        the actor's layout, becomes the actor plus N(0, stddev^2) noise on every weight, is redrawn by param_noise_resample and answers
        the actor's action_given(.., add_noise=True); set_param_noise(None) switches it off.  Ends with one resample without a batch;
        drops no captured graph."""
        h = perturbed_actor.handle if perturbed_actor is not None else None
        check(lib.cpp_ddpg_set_param_noise(self.handle, h, float(stddev), float(target), float(adapt), int(seed)))
        self.param_noise = None if perturbed_actor is None else (float(stddev), float(target), float(adapt), int(seed))
        self.nets[0].perturbed = perturbed_actor

    def param_noise_resample(self, device_batch=None):
        """one resample (cpp_ddpg_param_noise_resample): perturb; with a DeviceBatch also measure the action distance on its state_1 and
        adapt the standard deviation of the next resample; count.  Nothing waits for the device."""
        check(lib.cpp_ddpg_param_noise_resample(self.handle, device_batch.handle if device_batch is not None else None))

    def param_noise_status(self):
        """(sigma the next resample reads, distance of the last measured resample, draw count n, whether the last resample adapted)"""
        s, d, n, ad = C.c_float(), C.c_float(), C.c_uint64(), C.c_int()
        check(lib.cpp_ddpg_param_noise_status(self.handle, C.byref(s), C.byref(d), C.byref(n), C.byref(ad)))
        return np.float32(s.value), np.float32(d.value), int(n.value), bool(ad.value)

    def get_param_noise_state(self):
        """{sigma, n}: what a checkpoint carries of the noise (the perturbed copy itself is redrawn)"""
        s, n = C.c_float(), C.c_uint64()
        check(lib.cpp_ddpg_param_noise_state(self.handle, 0, C.byref(s), C.byref(n)))
        return {"sigma": np.float32(s.value), "n": np.uint64(n.value)}

    def set_param_noise_state(self, state):
        s = C.c_float(float(np.asarray(state["sigma"]).reshape(())))
        n = C.c_uint64(int(np.asarray(state["n"]).reshape(())))
        check(lib.cpp_ddpg_param_noise_state(self.handle, 1, C.byref(s), C.byref(n)))

    def last_param_noise(self, B):
        """(a, at), each (B, action_dim): the actor's and the perturbed actor's actions on the rows of the last measured resample"""
        B = int(B)
        a, at = np.empty((B, self.action_dim), np.float32), np.empty((B, self.action_dim), np.float32)
        check(lib.cpp_ddpg_last_param_noise(self.handle, B, ptr(a), ptr(at)))
        return a, at

    def policy_delay_status(self):
        """(delay, critic updates counted since it was set, whether the last minibatch held the actor)"""
        d, n, held = C.c_int(), C.c_uint64(), C.c_int()
        check(lib.cpp_ddpg_policy_delay_status(self.handle, C.byref(d), C.byref(n), C.byref(held)))
        return int(d.value), int(n.value), bool(held.value)

    def grad_buffer(self):
        p, n = C.c_void_p(), C.c_int64()
        check(lib.cpp_ddpg_grad_buffer(self.handle, C.byref(p), C.byref(n)))
        return p.value, n.value

    def has_optimiser_slots(self):
        return self.optimiser_kind != _lib.CPP_OPT_SGD

    def get_optimiser_state(self):
        """the two optimisers' slot variables {m, v, step} (what tf.train.Saver checkpoints besides the weights, util.py:88-90): m and v
        hold the actor's list, then the critic's; step = (actor's count, critic's count).  Momentum leaves v zero."""
        assert self.has_optimiser_slots(), "GradientDescent has no slots"
        n = int(lib.cpp_ddpg_opt_state_size(self.handle))
        m, v, step = np.zeros(n, np.float32), np.zeros(n, np.float32), np.zeros(2, np.uint64)
        check(lib.cpp_ddpg_get_opt_state(self.handle, ptr(m), ptr(v), n, ptr(step)))
        return {"m": m, "v": v, "step": step}

    def set_optimiser_state(self, state):
        assert self.has_optimiser_slots(), "GradientDescent has no slots"
        m = np.ascontiguousarray(state["m"], dtype=np.float32)
        v = np.ascontiguousarray(state["v"], dtype=np.float32)
        step = np.ascontiguousarray(np.asarray(state["step"]).reshape(2), dtype=np.uint64)
        assert len(m) == len(v)
        check(lib.cpp_ddpg_set_opt_state(self.handle, ptr(m), ptr(v), len(m), ptr(step)))

    def close(self):
        if self._h:
            self.flush()
        for b in self._upload.values():
            b.close()
        if self._h:
            lib.cpp_ddpg_destroy(self._h)
            self._h = None


class CriticNetwork(base_network.Network):
    """ the critic represents a mapping from state & actors action to a quality score."""

    def __init__(self, namespace, actor):
        super(CriticNetwork, self).__init__(namespace)
        # input state to the critic is the _same_ state given to the actor; input action is the
        # (gradient-stopped) output action of the actor unless one is fed (ddpg_cartpole.py:161-162)
        self.actor = actor
        self.input_state = actor.input_state
        self.input_action = _OpHandle(namespace + "/input_action")
        self.action_dim = actor.action_dim
        self._state_elems = int(np.prod([int(d) for d in self.input_state.get_shape()[1:]]))
        if opts.use_raw_pixels:
            # conv trunk -> (flatten) -> 200 -> 50 -> concat action -> 50  (:166-171, intent; B2)
            self.simple_conv_net_on(self.input_state, opts)
            self._hidden = []
        else:
            # flatten(state) | action -> hidden stack (:172-177; B1: opts=None means no dropout)
            self.hidden_layers_starting_at(self.input_state, opts.critic_hidden_layers)
        # --twin-q: hidden3 / q_value (low-dimensional: the whole stack) twice; q_value, forward and dQ/da stay head 1's
        self.twin_q = twin_q(opts)
        # --distributional-critic: q_value emits num_atoms logits; q_value, forward and dQ/da are the distribution's mean
        self.distribution = distributional_critic(opts)
        # --quantile-critic: q_value emits num_quantiles quantile atoms; q_value, forward and dQ/da are their mean
        self.quantiles = quantile_critic(opts)
        # --pooled-quantile-critics: two heads of N quantile atoms each; q_value and forward are head 1's mean, dQ/da the mean over both heads'
        self.pooled = pooled_quantile_critics(opts)
        # --feature-layer-norm: hidden1 is Linear -> LayerNorm -> tanh
        self.feature_norm = feature_layer_norm(opts)
        if self.pooled:
            self._build_native(_lib.CPP_CRITIC, self.action_dim, max(int(opts.batch_size), 1), pooled=self.pooled[0], feature_norm=self.feature_norm)
        else:
            self._build_native(_lib.CPP_CRITIC, self.action_dim, max(int(opts.batch_size), 1), twin_q=self.twin_q, distribution=self.distribution,
                               quantiles=self.quantiles[0] if self.quantiles else None, feature_norm=self.feature_norm)
        # --shared-encoder: this critic's conv trunk is its actor's encoder from here on
        if getattr(actor, "shared_encoder", False):
            check(lib.cpp_net_set_encoder(actor.handle, self.handle))
        self.q_value = _OpHandle(namespace + "/q_value")
        self.target_critic = None
        self._ddpg = None
        self._actor_for_training = None
        self.train_op = None

    def _register_actor_training(self, actor):
        self._actor_for_training = actor

    def init_ops_for_training(self, target_critic):
        # bellman: Q(s1, a) = reward + terminal_mask * discount * Q'(s2, A'(s2)); squared TD loss;
        # clip by global norm; SGD (ddpg_cartpole.py:186-218)
        self.target_critic = target_critic
        self._optimiser = ddpg_optimiser(opts)      # (kind, momentum, beta1, beta2, epsilon) of this train op and the actor's
        self._target_smoothing = target_policy_smoothing(opts)      # (sigma, clip, seed) of this train op's target
        self._policy_delay = policy_delay(opts)      # critic updates per actor update (the actor's train op is bound to this one)
        self._actor_min_q = actor_min_q(opts)      # whether the actor's train op follows min(Q1, Q2)
        self._behaviour_cloning = behaviour_cloning(opts)      # (alpha, q_floor) of the actor's train op; alpha 0: off
        self.reward = base_network.Placeholder([None, 1], name="critic_reward")
        self.terminal_mask = base_network.Placeholder([None, 1], name="critic_terminal_mask")
        self.input_state_2 = target_critic.input_state
        self.temporal_difference = _OpHandle(self.namespace + "/temporal_difference")
        self.temporal_difference_loss = _OpHandle(self.namespace + "/temporal_difference_loss")
        self.train_op = _OpHandle(self.namespace + "/optimiser/train_op")

    def _trainer(self):
        if self._ddpg is None:
            actor = self._actor_for_training or self.actor
            if self.target_critic is not None:
                self._ddpg = _Trainer(actor, self, self.target_critic.actor, self.target_critic)
            else:   # actor-only training does not touch the targets; bind the live nets as stand-ins
                self._ddpg = _Trainer(actor, self, actor, self)
        return self._ddpg

    def forward(self, states, actions):
        s, dt = _lib.as_state_array(states)
        B = s.shape[0]
        a = np.ascontiguousarray(np.asarray(actions, np.float32).reshape(B, self.action_dim))
        out = np.empty((B, 1), np.float32)
        check(lib.cpp_net_forward(self.handle, ptr(s), dt, B, ptr(a), ptr(out)))
        return out

    def q_gradients_wrt_actions(self, batch=None):
        """ gradients for the q.value w.r.t just input_action; used for actor training.  With no
        argument returns the op handle (graph-building use, :111); with a batch / state array returns
        dQ/da evaluated at a = actor(state_1), shape (B, action_dim)."""
        if batch is None:
            return _OpHandle(self.namespace + "/q_gradients_wrt_actions")
        trainer = self._trainer()
        # (--bc-alpha: the pass's cloning term reads the stored actions of a batch that carries them; dQ/da itself never does)
        dev = trainer.device_batch_for(batch, state_only=not (trainer.behaviour_cloning[0] > 0.0 and hasattr(batch, "action")))
        out = np.empty((dev.size, self.action_dim), np.float32)
        check(lib.cpp_ddpg_q_gradients_wrt_actions(trainer.handle, dev.handle, ptr(out), None, None))
        return out

    def train(self, batch):
        if self.target_critic is None:
            raise Exception("init_ops_for_training not called")
        trainer = self._trainer()
        if isinstance(batch, replay_memory.Batch) and trainer.train_pair(batch):
            return                  # ran together with the actor's deferred update (ActorNetwork.train)
        if isinstance(batch, replay_memory.Batch) and batch.weights is not None:
            raise RuntimeError("a prioritized Batch trains as the reference's pair: actor.train(batch.state_1), then critic.train(batch) "
                               "on the same draw (the weights and the priority updates belong to that fused minibatch)")
        dev = trainer.device_batch_for(batch)
        check(lib.cpp_ddpg_train_critic(trainer.handle, dev.handle))
        if opts.print_gradients:
            print("gradient %s l2_norm %s" % (self.namespace, trainer.last_stats()[2]))

    def check_loss(self, batch):
        if self.target_critic is None:
            raise Exception("init_ops_for_training not called")
        trainer = self._trainer()
        dev = trainer.device_batch_for(batch)
        B = dev.size
        loss = np.zeros(1, np.float32)
        td = np.empty((B, 1), np.float32)
        q = np.empty((B, 1), np.float32)
        check(lib.cpp_ddpg_check_loss(trainer.handle, dev.handle, ptr(loss), ptr(td), ptr(q)))
        return [loss[0], td, q]


class DeepDeterministicPolicyGradientAgent(object):
    def __init__(self, env):
        self.env = env
        state_shape = self.env.observation_space.shape
        action_dim = self.env.action_space.shape[1]
        # (the refusals of --distributional-critic and --n-step come before anything exists on the device, as check_prioritized_opts')
        pooled_quantile_critics(opts)
        distributional_critic(opts)
        quantile_critic(opts)
        soft_actor_critic(opts, action_dim)
        feature_layer_norm(opts)
        n_step(opts)
        actor_min_q(opts)
        behaviour_cloning(opts)
        shared_encoder(opts)
        shift = random_shift(opts)
        self.param_noise = param_noise(opts)
        # (--exact-products asks for the exact arithmetic contract; without the flag the context keeps whatever mode its owner chose --
        # an explicit Context.set_precision("exact") is not undone, and a second agent on the shared context does not fight the first)
        if getattr(opts, "exact_products", False) and _lib.default_context().precision != "exact":
            _lib.default_context().set_precision("exact")
        # replay memory: f16 state store resident in HBM (ddpg_cartpole.py:257-261)
        self.replay_memory = replay_memory.ReplayMemory(opts.replay_memory_size, state_shape, action_dim,
                                                       store_dtype=opts.replay_store)
        if getattr(opts, "prioritized_replay", False):
            check_prioritized_opts(opts)
            self.replay_memory.enable_priorities(opts.priority_alpha, opts.priority_eps, seed=opts.sample_seed)
            self.replay_memory.set_priority_beta(priority_beta(opts, 0))
        if n_step(opts) > 1:
            self.replay_memory.enable_n_step(n_step(opts), opts.discount)
        if shift[0] > 0:
            try:
                self.replay_memory.enable_random_shift(*shift)
            except ValueError as e:
                raise SystemExit("--random-shift: %s" % e)
        # s1 and s2 placeholders
        batched_state_shape = [None] + list(state_shape)
        s1 = base_network.Placeholder(batched_state_shape)
        s2 = base_network.Placeholder(batched_state_shape)
        # base models for actor / critic and their corresponding target networks
        self.actor = ActorNetwork("actor", s1, action_dim)
        self.critic = CriticNetwork("critic", self.actor)
        self.target_actor = ActorNetwork("target_actor", s2, action_dim)
        self.target_critic = CriticNetwork("target_critic", self.target_actor)
        # training ops
        self.actor.init_ops_for_training(self.critic)
        self.critic.init_ops_for_training(self.target_critic)
        self.ddpg_optimiser_kind = self.critic._optimiser[0]      # (util.optimiser_slot_owner: who holds slots is a fact about this agent)
        self.train_steps = 0
        # --param-noise-stddev: one more actor, the copy that explores.  Not one of networks(): it is a function of the actor, sigma and the
        # draw count, so it is neither checkpointed nor broadcast; under --shared-encoder it reads the critic's conv features as the actor does
        self.perturbed_actor = None
        if self.param_noise is not None:
            self.perturbed_actor = ActorNetwork("perturbed_actor", s1, action_dim)
            if self.perturbed_actor.shared_encoder:
                check(lib.cpp_net_set_encoder(self.perturbed_actor.handle, self.critic.handle))

    def initialise_variables(self, seed=None):
        """tf.initialize_all_variables() (ddpg_cartpole.py:424)."""
        rng = np.random.RandomState(seed) if seed is not None else np.random
        for net in (self.actor, self.critic, self.target_actor, self.target_critic):
            net.initialise_variables(rng)

    def networks(self):
        return [self.actor, self.critic, self.target_actor, self.target_critic]

    def checkpoint_extras(self):
        """(prefix, get, set) of state a checkpoint carries by name besides the networks and the optimiser slots: the temperature of a
        --soft-actor-critic agent ('sac::log_alpha', 'sac::m', 'sac::v', 'sac::step'), the standard deviation and the draw count of a
        --param-noise-stddev agent ('param_noise::sigma', 'param_noise::n'); nothing for any other agent"""
        if getattr(self, "param_noise", None) is not None:
            return [("param_noise::", lambda: self._param_noise_trainer().get_param_noise_state(),
                     lambda st: self._param_noise_trainer().set_param_noise_state(st))]
        if not self.actor.sac:
            return []
        return [("sac::", lambda: self.trainer.get_sac_state(), lambda st: self.trainer.set_sac_state(st))]

    def _param_noise_trainer(self):
        """the trainer with the perturbed copy handed over (once: cpp_ddpg_set_param_noise zeroes the draw count).  Under --data-parallel
        rank r draws with seed + r, so that the replicas explore differently."""
        t = self.trainer
        if t.param_noise is None:
            pn = self.param_noise
            rank = int(os.environ.get("RANK", "0")) if getattr(opts, "data_parallel", False) else 0
            t.set_param_noise(self.perturbed_actor, pn["stddev"], pn["target"], pn["adapt"], (pn["seed"] + rank) % 2 ** 64)
        return t

    def begin_episode(self):
        """--param-noise-stddev: redraw the perturbed copy for the episode about to start (Plappert et al. 2018: the perturbation is held
        for a whole episode) -- --param-noise-adapt-rounds resamples, each on its own device minibatch of opts.batch_size rows (the
        inspection sampler: the training sampler's counter stays where it is; the stored pixels, no random shift) once the memory holds
        that many, without a batch before that.  A no-op for every other agent.  Under --async-rollouts the rollout thread calls it: it
        takes the device lock, as _action does."""
        if getattr(self, "param_noise", None) is None:
            return
        lock = getattr(self, "device_lock", None)
        if lock is None:
            return self._begin_episode()
        with lock:
            return self._begin_episode()

    def _begin_episode(self):
        t, B = self._param_noise_trainer(), int(opts.batch_size)
        for _ in range(self.param_noise["rounds"]):
            dev = None
            if self.replay_memory.size() >= B:
                dev = self.replay_memory.sample_on_device(B, seed=self.param_noise["seed"]).device
            t.param_noise_resample(dev)

    def post_var_init_setup(self):
        if opts.event_log_in:
            self.replay_memory.reset_from_event_log(opts.event_log_in)
        # hook networks up to their targets ( one off clobber of all vars in target network )
        self.target_actor.set_as_target_network_for(self.actor, opts.target_update_rate)
        self.target_critic.set_as_target_network_for(self.critic, opts.target_update_rate)
        if getattr(self, "param_noise", None) is not None:      # the actor's variables exist: the perturbed copy can be drawn, and acts from here on
            self._param_noise_trainer()

    @property
    def trainer(self):
        return self.critic._trainer()

    def train_step(self, batch_size, batches_per_step, idxs=None):
        """the inner train step ddpg_cartpole.py:331-337 as ONE device-side sequence (hipGraph after
        the first call): batches_per_step x {sample+gather, actor update, critic update}, then both
        target soft updates.  idxs: optional (batches_per_step*batch_size) rows instead of Philox."""
        t = self.trainer
        if idxs is None and getattr(opts, "data_parallel", False):      # one learner of N: the collective step (distributed.py)
            self._dp_learner(batch_size).train_step(batches_per_step)
            self.train_steps += 1
            return
        rows = None
        if idxs is not None:
            rows = np.ascontiguousarray(np.asarray(idxs).reshape(-1), dtype=np.int32)
            assert len(rows) == batch_size * batches_per_step
        self.replay_memory.stats[">batch"] += batches_per_step
        check(lib.cpp_ddpg_train_step(t.handle, self.replay_memory.handle, int(batch_size),
                                      int(batches_per_step), ptr(rows), int(opts.sample_seed)))
        self.train_steps += 1

    def _dp_learner(self, batch_size):
        from . import distributed
        return distributed.setup_data_parallel(self, opts, batch_size)

    def _action(self, state, add_noise):
        """action_given under the context lock of --async-rollouts (the rollout thread and the learner thread share one stream)."""
        lock = getattr(self, "device_lock", None)
        if lock is None:
            return self.actor.action_given(state, add_noise)
        with lock:
            return self.actor.action_given(state, add_noise)

    def _train_once(self, batch_size, batches_per_step):
        """the inner step ddpg_cartpole.py:331-337; returns the losses it logs (B10: the last minibatch's TD loss)."""
        if getattr(opts, "prioritized_replay", False):
            self.replay_memory.set_priority_beta(priority_beta(opts, self.train_steps))
        if opts.host_rng_sampling:
            for _ in range(batches_per_step):
                batch = self.replay_memory.batch(batch_size)
                self.actor.train(batch.state_1)
                self.critic.train(batch)
            self.target_actor.update_weights()
            self.target_critic.update_weights()
        else:
            self.train_step(batch_size, batches_per_step)
        return [float(self.trainer.last_stats()[0])]

    def _verbose_after_train(self, batch_size):
        if VERBOSE_DEBUG:                          # ddpg_cartpole.py:339-349
            batch = self.replay_memory.batch(batch_size)
            td_loss, td, q_value = self.critic.check_loss(batch)
            print("-----")
            print("temporal_difference_loss", td_loss)
            print("temporal_difference", td.T)
            print("q_value", q_value.T)

    def run_training(self, max_num_actions, max_run_time, batch_size, batches_per_step, saver_util):
        """ddpg_cartpole.py:291-383.  The loop itself -- episode, add_episode, train after burn-in, STATS, checkpoint, eval every 10th,
        exit tests -- is training_loop.TrainingLoop, shared with the NAF agent; under --data-parallel it takes the train / stop
        decisions collectively, with --async-rollouts the episodes come from a rollout thread."""
        from . import training_loop
        agreement = None
        if getattr(opts, "data_parallel", False):
            agreement = self._dp_learner(batch_size).agreement()
        if getattr(opts, "async_rollouts", False) and getattr(self, "device_lock", None) is None:
            self.device_lock = training_loop.FairLock()

        def dump_requested():
            global DUMP_WEIGHTS
            if DUMP_WEIGHTS:
                DUMP_WEIGHTS = False
                return True
            return False
        loop = training_loop.TrainingLoop(self, opts, act=lambda s: self._action(s, True), train=self._train_once,
                                          agreement=agreement, verbose=lambda: VERBOSE_DEBUG,
                                          after_train=self._verbose_after_train, dump_weights_requested=dump_requested,
                                          begin_episode=self.begin_episode if getattr(self, "param_noise", None) is not None else None)
        loop.run(max_num_actions, max_run_time, batch_size, batches_per_step, saver_util)
        return loop

    def debug_dump_network_weights(self):
        fn = "/tmp/weights.%s" % time.time()
        with open(fn, "w") as f:
            f.write("DUMP time %s\n" % time.time())
            for net in self.networks():
                for var in net.trainable_model_vars():
                    f.write("VAR %s %s\n" % (var.name, tuple(var.get_shape())))
                    f.write("%s\n" % var.eval())
        print("weights written to", fn)
        return fn

    def run_eval(self, num_episodes, add_noise=False):
        """ run num_episodes of eval and output episode length and rewards """
        for i in range(num_episodes):
            state = self.env.reset()
            total_reward = 0
            steps = 0
            done = False
            while not done:
                action = self._action(state, add_noise)
                state, reward, done, _ = self.env.step(action)
                print("EVALSTEP r%s %s %s %s %s" % (i, steps, np.squeeze(action), np.linalg.norm(action), reward))
                total_reward += reward
                steps += 1
            print("EVAL", i, steps, total_reward)
        sys.stdout.flush()

    def close(self):
        if getattr(self, "_learner", None) is not None:
            self._learner.close()
            self._learner = None
        if self.critic._ddpg is not None:
            self.critic._ddpg.close()
        if getattr(self, "perturbed_actor", None) is not None:
            self.perturbed_actor.close()
        for net in (self.actor, self.critic, self.target_actor, self.target_critic):
            net.close()
        self.replay_memory.close()


def make_env(o):
    if o.synthetic_env:
        from .synthetic_env import SyntheticCartpole
        return SyntheticCartpole(o)
    try:
        import bullet_cartpole      # the reference's pybullet env, if the user has it on sys.path
    except ImportError as e:
        raise ImportError("bullet_cartpole / pybullet not importable (%s); physics stays on the host "
                          "CPU and is not part of this package -- use --synthetic-env for a stand-in" % e)
    return bullet_cartpole.BulletCartpole(opts=o, discrete_actions=False)


def main(argv=None):
    _install_signal_handlers()
    set_opts(build_parser().parse_args(argv))
    if opts.data_parallel and opts.host_rng_sampling:
        # the host-RNG path is the reference's literal loop: local actor.train / critic.train calls with no all-reduce -- N learners
        # would agree on when to train (LoopAgreement) and silently train N different networks
        raise SystemExit("--data-parallel draws minibatches with the device sampler inside the collective step: it cannot be combined with --host-rng-sampling")
    check_prioritized_opts(opts)
    sys.stderr.write("%s\n" % opts)
    env = make_env(opts)
    agent = DeepDeterministicPolicyGradientAgent(env=env)
    # either load the latest ckpt or init variables (ddpg_cartpole.py:419-424)
    saver_util = None
    if opts.ckpt_dir is not None and not (opts.data_parallel and int(os.environ.get("RANK", "0")) != 0):      # rank 0 keeps the checkpoints
        saver_util = util.SaverUtil(agent, opts.ckpt_dir, opts.ckpt_freq)
    else:
        agent.initialise_variables()
    for net in (agent.actor, agent.critic, agent.target_actor, agent.target_critic):
        for v in net.trainable_model_vars():
            sys.stderr.write("%s %s\n" % (v.name, util.shape_and_product_of(v.shape)))
    agent.post_var_init_setup()
    if opts.data_parallel and opts.num_eval <= 0:
        # process group, rank 0's parameters to every rank, RCCL communicator: collective, so at the same point on every rank
        from . import distributed
        distributed.setup_data_parallel(agent, opts, opts.batch_size)
    if opts.num_eval > 0:
        agent.run_eval(opts.num_eval, opts.eval_action_noise)
    else:
        agent.run_training(opts.max_num_actions, opts.max_run_time, opts.batch_size,
                           opts.batches_per_step, saver_util)
        if saver_util is not None:
            saver_util.force_save()
    env.reset()
    agent.close()
    if opts.data_parallel:
        from . import distributed
        distributed.shutdown_data_parallel()
    if hasattr(env, "close"):
        env.close()


if __name__ == "__main__":
    main()
