#!/usr/bin/env python
"""Soft actor-critic's cost in the fused DDPG step: cfg3 (64x64x18, B = 256, 5 minibatches per outer step, 22 000 synthetic rows), three
trainers in ONE process on alternating timed blocks of hipGraph-replayed outer steps:
    plain      the scalar trainer (the route the environment chooses, see below)
    sac        --soft-actor-critic                     (csrc/sac.hip: four launches per minibatch, two copy nodes)
    sac_twin   --soft-actor-critic --twin-q            (DrQ's learner without its augmentation)
Then the launches alone, event-timed (the library's profiling mode: the eager launch sequence with an event pair around every launch),
alternating as well.  Two runs say two things:
    sac_rate.py                                             the plain trainer on its default route (the fused heads launch): what a user pays
    CARTPOLEPP_ABLATION=1 CPP_FUSED_HEADS=0 sac_rate.py     the plain trainer on the SAME GEMM levels (td_kernel): the kernels' own price
Prints one JSON line: steps/s of each and the ratios of the SAC steps to the plain one, microseconds per launch of the sac / td / heads /
gemm / clip_sgd families (medians over the block pairs), and the launch census of an outer step of each.
Usage: sac_rate.py [blocks] [steps per block]"""
import json, os, sys, time
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cartpoleplusplus_amd import ddpg_cartpole as D

shape, B, NB, ROWS = (64, 64, 3, 2, 3), 256, 5, 22000
blocks = int(sys.argv[1]) if len(sys.argv) > 1 else 8
steps = int(sys.argv[2]) if len(sys.argv) > 2 else 40
FAMILIES = ("sac", "td", "heads", "gemm", "clip_sgd")
KINDS = {"plain": {}, "sac": dict(soft_actor_critic=True), "sac_twin": dict(soft_actor_critic=True, twin_q=True)}


class Env(object):
    class S(object):
        def __init__(self, s): self.shape = tuple(s)
    observation_space, action_space = S(shape), S((1, 2))


def agent(kw):
    D.set_opts(D.default_opts(use_raw_pixels=True, render_height=64, render_width=64, num_cameras=2, action_repeats=3, batch_size=B,
                              replay_memory_size=ROWS, **kw))
    a = D.DeepDeterministicPolicyGradientAgent(Env())
    a.initialise_variables(seed=42)
    a.post_var_init_setup()
    a.replay_memory.fill_synthetic(ROWS, seed=1234)
    return a


agents = {k: agent(kw) for k, kw in KINDS.items()}
assert agents["plain"].actor.sac is None and agents["sac"].actor.sac is not None
assert agents["sac"].actor.num_params - agents["plain"].actor.num_params == 51 * 2
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
us = {k: {f: [] for f in FAMILIES} for k in agents}
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
        for f in FAMILIES:
            ms, n = prof.get(f, (0.0, 0))
            if n:
                us[k][f].append(1e3 * ms / n)
        launches[k] = {name: cnt for name, (_ms, cnt) in prof.items()}
ctx.prof_reset()
for k in ("sac", "sac_twin"):
    assert launches[k]["sac"] == 4 * 4 * NB and not launches[k].get("heads", 0), launches[k]
assert launches["plain"].get("sac", 0) == 0, launches["plain"]


def ratio(a, b):
    return float(np.median(np.array(rates[a]) / np.array(rates[b])))


out = {"workload": "cfg3", "B": B, "batches_per_step": NB, "blocks": blocks, "steps_per_block": steps,
       "plain_route": "fused heads" if launches["plain"].get("heads", 0) else "gemm levels"}
for k in agents:
    out["%s_steps_per_s" % k] = float(np.median(rates[k]))
for k in ("sac", "sac_twin"):
    out["%s_over_plain" % k] = ratio(k, "plain")
for k in agents:
    for f in FAMILIES:
        if us[k][f]:
            out["%s_%s_us" % (k, f)] = float(np.median(us[k][f]))
for k in agents:
    out["%s_launches_per_outer_step" % k] = {name: int(v // 4) for name, v in sorted(launches[k].items()) if v}
print(json.dumps(out))
for a in agents.values():
    a.close()
