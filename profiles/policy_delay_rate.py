#!/usr/bin/env python
"""Delayed policy updates' cost in the fused DDPG step: cfg3 (64x64x18, B = 256, 5 minibatches per outer step, 22 000 synthetic
rows), a trainer with the delay off against one with d = 2 (the heads kernel's last thread counts the minibatch and leaves the hold
word; the optimiser's launch leaves a held actor's parameters alone), ONE process, two agents, alternating timed blocks of
hipGraph-replayed outer steps.  Then the heads and the optimiser's launches alone, event-timed both ways (the library's profiling
mode: the eager launch sequence with an event pair around every launch), alternating as well.  Prints one JSON line: steps/s of each
and the median of the pairs' ratios, microseconds per heads / optimiser launch of each and their ratios, the launches per outer step
(identical on and off on this path: no tick launch).
Usage: policy_delay_rate.py [blocks] [steps per block]"""
import json, os, sys, time
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cartpoleplusplus_amd import ddpg_cartpole as D

shape, B, NB, ROWS = (64, 64, 3, 2, 3), 256, 5, 22000
DELAY = 2
blocks = int(sys.argv[1]) if len(sys.argv) > 1 else 8
steps = int(sys.argv[2]) if len(sys.argv) > 2 else 40


class Env(object):
    class S(object):
        def __init__(self, s): self.shape = tuple(s)
    observation_space, action_space = S(shape), S((1, 2))


def agent(delay):
    D.set_opts(D.default_opts(use_raw_pixels=True, render_height=64, render_width=64, num_cameras=2, action_repeats=3, batch_size=B,
                              replay_memory_size=ROWS, policy_delay=delay))
    a = D.DeepDeterministicPolicyGradientAgent(Env())
    a.initialise_variables(seed=42)
    a.post_var_init_setup()
    a.replay_memory.fill_synthetic(ROWS, seed=1234)
    return a


agents = {"off": agent(1), "on": agent(DELAY)}
assert agents["off"].trainer.policy_delay == 1 and agents["on"].trainer.policy_delay == DELAY
ctx = agents["off"].actor.ctx
for a in agents.values():
    for _ in range(4):
        a.train_step(B, NB)
ctx.sync()
assert agents["on"].trainer.policy_delay_status() == (DELAY, 4 * NB, (4 * NB) % DELAY != 0)
rates = {k: [] for k in agents}
for _ in range(blocks):
    for k, a in agents.items():
        t0 = time.perf_counter()
        for _ in range(steps):
            a.train_step(B, NB)
        ctx.sync()
        rates[k].append(steps / (time.perf_counter() - t0))
heads = {k: [] for k in agents}
optim = {k: [] for k in agents}
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
        ms, n = prof["clip_sgd"]
        assert n == 4 * NB, prof
        optim[k].append(1e3 * ms / n)
        launches[k] = {name: cnt for name, (_ms, cnt) in prof.items()}
ctx.prof_reset()
assert launches["on"] == launches["off"], (launches["on"], launches["off"])      # (the count rides in the heads kernel: no tick launch on this path)
print(json.dumps({"workload": "cfg3", "B": B, "batches_per_step": NB, "blocks": blocks, "steps_per_block": steps, "policy_delay": DELAY,
                  "off_steps_per_s": float(np.median(rates["off"])), "on_steps_per_s": float(np.median(rates["on"])),
                  "on_over_off": float(np.median(np.array(rates["on"]) / np.array(rates["off"]))),
                  "off_heads_us": float(np.median(heads["off"])), "on_heads_us": float(np.median(heads["on"])),
                  "heads_on_over_off": float(np.median(np.array(heads["on"]) / np.array(heads["off"]))),
                  "off_optimiser_us": float(np.median(optim["off"])), "on_optimiser_us": float(np.median(optim["on"])),
                  "optimiser_on_over_off": float(np.median(np.array(optim["on"]) / np.array(optim["off"]))),
                  "launches_per_outer_step": {k: int(v // 4) for k, v in sorted(launches["off"].items())}}))
for a in agents.values():
    a.close()
