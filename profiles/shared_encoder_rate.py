#!/usr/bin/env python
"""The shared conv encoder's rate in the fused DDPG step: cfg3 (64x64x18, B = 256, 5 minibatches per outer step, 22 000 synthetic rows), a
trainer of four full networks against one whose actors read the critics' conv features (--shared-encoder: conv forward of {critic,
target critic} instead of four networks, conv backward of {critic} instead of two), ONE process, two agents, alternating timed blocks of
hipGraph-replayed outer steps.  Then the conv launches alone, event-timed both ways (the library's profiling mode: the eager launch
sequence with an event pair around every launch), alternating as well.  Prints one JSON line: outer steps/s of each and their ratio
(median of the block pairs' ratios), microseconds per launch of each conv family of both and their ratios, and the launch census of an
outer step of both.
Usage: shared_encoder_rate.py [blocks] [steps per block]"""
import json, os, sys, time
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cartpoleplusplus_amd import ddpg_cartpole as D

shape, B, NB, ROWS = (64, 64, 3, 2, 3), 256, 5, 22000
blocks = int(sys.argv[1]) if len(sys.argv) > 1 else 8
steps = int(sys.argv[2]) if len(sys.argv) > 2 else 40
PROF_STEPS = 4


class Env(object):
    class S(object):
        def __init__(self, s): self.shape = tuple(s)
    observation_space, action_space = S(shape), S((1, 2))


def agent(shared):
    D.set_opts(D.default_opts(use_raw_pixels=True, render_height=64, render_width=64, num_cameras=2, action_repeats=3, batch_size=B,
                              replay_memory_size=ROWS, shared_encoder=shared))
    a = D.DeepDeterministicPolicyGradientAgent(Env())
    a.initialise_variables(seed=42)
    a.post_var_init_setup()
    a.replay_memory.fill_synthetic(ROWS, seed=1234)
    return a


agents = {"plain": agent(False), "shared": agent(True)}
assert not [v for v in agents["shared"].actor.trainable_model_vars() if "conv" in v.name]
ctx = agents["plain"].actor.ctx
for a in agents.values():
    for _ in range(4):
        a.train_step(B, NB)
ctx.sync()
rates = {k: [] for k in agents}
for _ in range(blocks):
    for k, a in agents.items():
        t0 = time.perf_counter()
        for _ in range(steps):
            a.train_step(B, NB)
        ctx.sync()
        rates[k].append(steps / (time.perf_counter() - t0))
us = {k: {} for k in agents}
launches = {}
for _ in range(blocks):
    for k, a in agents.items():
        ctx.sync()
        ctx.prof_reset()
        ctx.prof_enable(True)
        try:
            for _ in range(PROF_STEPS):
                a.train_step(B, NB)
            ctx.sync()
        finally:
            ctx.prof_enable(False)
        prof = ctx.prof_read()
        for f, (ms, n) in prof.items():
            if n and f.startswith("conv"):
                us[k].setdefault(f, []).append(1e3 * ms / n)
        launches[k] = {name: int(cnt // PROF_STEPS) for name, (_ms, cnt) in prof.items() if cnt}
ctx.prof_reset()
out = {"workload": "cfg3", "B": B, "batches_per_step": NB, "blocks": blocks, "steps_per_block": steps,
       "plain_steps_per_s": float(np.median(rates["plain"])), "shared_steps_per_s": float(np.median(rates["shared"])),
       "shared_over_plain": float(np.median(np.array(rates["shared"]) / np.array(rates["plain"])))}
for f in sorted(set(us["plain"]) | set(us["shared"])):
    p, s = us["plain"].get(f), us["shared"].get(f)
    out["plain_%s_us" % f] = float(np.median(p)) if p else None
    out["shared_%s_us" % f] = float(np.median(s)) if s else None
    if p and s and len(p) == len(s):
        out["%s_shared_over_plain" % f] = float(np.median(np.array(s) / np.array(p)))
out["launches_per_outer_step"] = {k: dict(sorted(v.items())) for k, v in launches.items()}
print(json.dumps(out))
for a in agents.values():
    a.close()
