#!/usr/bin/env python
"""The cost of a resample of the parameter-space exploration noise (--param-noise-stddev; csrc/param_noise.hip) beside the fused DDPG step:
cfg3 (64x64x18, B = 256, 5 minibatches per outer step, 22 000 synthetic rows), with and without --shared-encoder, ONE process.  Per agent:
    * a resample's two launches, event-timed: the library's profiling mode (an event pair around every launch of the eager sequence)
      books the perturbation and the distance / adapt / count launch under one family, so their mean; and one event pair around
      back-to-back resamples without a batch, the two launches together as the stream runs them;
    * a whole measured resample -- the device-side draw of 256 rows, the perturbation, both actors' inference forwards, the distance
      launch -- as agent.begin_episode() runs it, host clock around `reps` of them that end in a device synchronise;
    * the same without a batch (the perturbation and the count alone);
    * an outer step of the learner, hipGraph-replayed, timed the same way, and the measured resample as a share of it.
Prints one JSON line.  Usage: param_noise_rate.py [blocks] [reps per block]"""
import json, os, sys, time
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cartpoleplusplus_amd import ddpg_cartpole as D

shape, B, NB, ROWS = (64, 64, 3, 2, 3), 256, 5, 22000
blocks = int(sys.argv[1]) if len(sys.argv) > 1 else 8
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 40


class Env(object):
    class S(object):
        def __init__(self, s): self.shape = tuple(s)
    observation_space, action_space = S(shape), S((1, 2))


def agent(shared):
    D.set_opts(D.default_opts(use_raw_pixels=True, render_height=64, render_width=64, num_cameras=2, action_repeats=3, batch_size=B,
                              replay_memory_size=ROWS, param_noise_stddev=0.05, shared_encoder=shared))
    a = D.DeepDeterministicPolicyGradientAgent(Env())
    a.initialise_variables(seed=42)
    a.post_var_init_setup()
    a.replay_memory.fill_synthetic(ROWS, seed=1234)
    return a


def timed(ctx, fn, n):
    ctx.sync()
    t0 = time.perf_counter()
    for _ in range(n):
        fn()
    ctx.sync()
    return 1e6 * (time.perf_counter() - t0) / n


out = {"workload": "cfg3", "B": B, "batches_per_step": NB, "blocks": blocks, "reps_per_block": reps}
for name, shared in (("separate", False), ("shared_encoder", True)):
    a = agent(shared)
    ctx, t = a.actor.ctx, a.trainer
    for _ in range(4):
        a.train_step(B, NB)
        a.begin_episode()
    us = {"measured": [], "unmeasured": [], "outer_step": []}
    for _ in range(blocks):
        us["measured"].append(timed(ctx, a.begin_episode, reps))
        us["unmeasured"].append(timed(ctx, t.param_noise_resample, reps))
        us["outer_step"].append(timed(ctx, lambda: a.train_step(B, NB), reps))
    # the two launches: one profiled resample without a batch books the perturbation and the count launch, a measured one the
    # perturbation and the distance launch -- both launches of the family per resample
    ctx.sync(); ctx.prof_reset(); ctx.prof_enable(True)
    try:
        for _ in range(reps):
            a.begin_episode()
        ctx.sync()
    finally:
        ctx.prof_enable(False)
    prof = ctx.prof_read()
    ctx.prof_reset()
    ms, n = prof["param_noise"]
    assert n == 2 * reps, prof
    ctx.sync()
    ctx.timer_begin()
    for _ in range(reps):
        t.param_noise_resample()
    pair_us = 1e3 * ctx.timer_end() / reps      # (back to back on the stream: the perturbation and the count launch, launch gaps included)
    sigma, d, count, adapted = t.param_noise_status()
    out[name] = {"actor_parameters": int(a.actor.num_params), "param_noise_launch_us_mean_of_both": 1e3 * ms / n, "unmeasured_resample_event_us": pair_us,
                 "profiled_resample_launches": {k: int(v[1] // reps) for k, v in sorted(prof.items())},
                 "profiled_resample_us_by_family": {k: 1e3 * v[0] / reps for k, v in sorted(prof.items())},
                 "measured_resample_us": float(np.median(us["measured"])), "unmeasured_resample_us": float(np.median(us["unmeasured"])),
                 "outer_step_us": float(np.median(us["outer_step"])),
                 "measured_resample_over_outer_step": float(np.median(np.array(us["measured"]) / np.array(us["outer_step"]))),
                 "last_sigma": float(sigma), "last_distance": float(d), "resamples": int(count)}
    a.close()
print(json.dumps(out))
