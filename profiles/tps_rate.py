#!/usr/bin/env python
"""Target policy smoothing's cost in the fused DDPG step: cfg3 (64x64x18, B = 256, 5 minibatches per outer step, 22 000 synthetic
rows), a trainer with smoothing off (the default instances of the heads kernel) against one with sigma = 0.2, c = 0.5 (the SMOOTH
instances: one Philox call, one logf, one cospif per row and a lane broadcast per component), ONE process, two agents, alternating
timed blocks of hipGraph-replayed outer steps.  Then the heads launch alone, event-timed both ways (the library's profiling mode:
the eager launch sequence with an event pair around every launch), alternating as well.  Prints one JSON line: steps/s of each and
their ratio, microseconds per heads launch of each and their ratio (medians over the block pairs).
Usage: tps_rate.py [blocks] [steps per block]"""
import json, os, sys, time
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cartpoleplusplus_amd import ddpg_cartpole as D

shape, B, NB, ROWS = (64, 64, 3, 2, 3), 256, 5, 22000
SIGMA, CLIP = 0.2, 0.5
blocks = int(sys.argv[1]) if len(sys.argv) > 1 else 8
steps = int(sys.argv[2]) if len(sys.argv) > 2 else 40


class Env(object):
    class S(object):
        def __init__(self, s): self.shape = tuple(s)
    observation_space, action_space = S(shape), S((1, 2))


def agent(sigma):
    D.set_opts(D.default_opts(use_raw_pixels=True, render_height=64, render_width=64, num_cameras=2, action_repeats=3, batch_size=B,
                              replay_memory_size=ROWS, target_policy_noise=sigma, target_policy_noise_clip=CLIP))
    a = D.DeepDeterministicPolicyGradientAgent(Env())
    a.initialise_variables(seed=42)
    a.post_var_init_setup()
    a.replay_memory.fill_synthetic(ROWS, seed=1234)
    return a


agents = {"off": agent(0.0), "on": agent(SIGMA)}
assert agents["off"].trainer.target_smoothing[0] == 0.0 and agents["on"].trainer.target_smoothing[:2] == (SIGMA, CLIP)
ctx = agents["off"].actor.ctx
for a in agents.values():
    for _ in range(4):
        a.train_step(B, NB)
ctx.sync()
assert agents["on"].trainer.last_target_noise(B)[1] == 4 * NB - 1
rates = {k: [] for k in agents}
for _ in range(blocks):
    for k, a in agents.items():
        t0 = time.perf_counter()
        for _ in range(steps):
            a.train_step(B, NB)
        ctx.sync()
        rates[k].append(steps / (time.perf_counter() - t0))
heads = {k: [] for k in agents}
launches = {}
for _ in range(blocks):
    for k, a in agents.items():
        ctx.sync()
        ctx.prof_reset()
        ctx.prof_enable(True)
        try:
            for _ in range(4):
                a.train_step(B, NB)
            ctx.sync()
        finally:
            ctx.prof_enable(False)
        prof = ctx.prof_read()
        ms, n = prof["heads"]
        assert n == 4 * NB, prof
        heads[k].append(1e3 * ms / n)
        launches[k] = {name: cnt for name, (_ms, cnt) in prof.items()}
ctx.prof_reset()
assert launches["on"] == launches["off"], (launches["on"], launches["off"])      # (the count rides in the optimiser's launch)
print(json.dumps({"workload": "cfg3", "B": B, "batches_per_step": NB, "blocks": blocks, "steps_per_block": steps, "sigma": SIGMA, "clip": CLIP,
                  "off_steps_per_s": float(np.median(rates["off"])), "on_steps_per_s": float(np.median(rates["on"])),
                  "on_over_off": float(np.median(np.array(rates["on"]) / np.array(rates["off"]))),
                  "off_heads_us": float(np.median(heads["off"])), "on_heads_us": float(np.median(heads["on"])),
                  "heads_on_over_off": float(np.median(np.array(heads["on"]) / np.array(heads["off"]))),
                  "launches_per_outer_step": {k: int(v // 4) for k, v in sorted(launches["off"].items())}}))
for a in agents.values():
    a.close()
