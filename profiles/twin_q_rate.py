#!/usr/bin/env python
"""Twin Q heads' cost in the fused DDPG step: cfg3 (64x64x18, B = 256, 5 minibatches per outer step, 22 000 synthetic rows), a trainer of
plain critics (ddpg_heads_kernel) against one of twin critics (--twin-q: ddpg_heads_twin_kernel, two more dW GEMMs in the level behind
it, a critic segment 2 701 floats longer for the optimiser), ONE process, two agents, alternating timed blocks of hipGraph-replayed
outer steps.  Then the launches alone, event-timed both ways (the library's profiling mode: the eager launch sequence with an event
pair around every launch), alternating as well: the heads launch, the GEMM launches (the profiler books all levels of a minibatch in
one family: the mean over them -- the level behind the heads launch is one of four) and the optimiser's launch.  Prints one JSON line:
steps/s of each and their ratio, microseconds per launch of each family and their ratios (medians over the block pairs), and the
launch census of an outer step, which must be the same for both.
Usage: twin_q_rate.py [blocks] [steps per block]"""
import json, os, sys, time
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cartpoleplusplus_amd import ddpg_cartpole as D

shape, B, NB, ROWS = (64, 64, 3, 2, 3), 256, 5, 22000
blocks = int(sys.argv[1]) if len(sys.argv) > 1 else 8
steps = int(sys.argv[2]) if len(sys.argv) > 2 else 40
FAMILIES = ("heads", "gemm", "clip_sgd")


class Env(object):
    class S(object):
        def __init__(self, s): self.shape = tuple(s)
    observation_space, action_space = S(shape), S((1, 2))


def agent(twin):
    D.set_opts(D.default_opts(use_raw_pixels=True, render_height=64, render_width=64, num_cameras=2, action_repeats=3, batch_size=B,
                              replay_memory_size=ROWS, twin_q=twin))
    a = D.DeepDeterministicPolicyGradientAgent(Env())
    a.initialise_variables(seed=42)
    a.post_var_init_setup()
    a.replay_memory.fill_synthetic(ROWS, seed=1234)
    return a


agents = {"plain": agent(False), "twin": agent(True)}
assert not agents["plain"].critic.twin_q and agents["twin"].critic.twin_q
assert agents["twin"].critic.num_params - agents["plain"].critic.num_params == 2650 + 51
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
        assert prof["heads"][1] == 4 * NB, prof
        for f in FAMILIES:
            ms, n = prof[f]
            us[k][f].append(1e3 * ms / n)
        launches[k] = {name: cnt for name, (_ms, cnt) in prof.items()}
ctx.prof_reset()
assert launches["twin"] == launches["plain"], (launches["twin"], launches["plain"])      # (no launch added: kernel id by kernel id)
out = {"workload": "cfg3", "B": B, "batches_per_step": NB, "blocks": blocks, "steps_per_block": steps,
       "plain_steps_per_s": float(np.median(rates["plain"])), "twin_steps_per_s": float(np.median(rates["twin"])),
       "twin_over_plain": float(np.median(np.array(rates["twin"]) / np.array(rates["plain"])))}
for f in FAMILIES:
    out["plain_%s_us" % f] = float(np.median(us["plain"][f]))
    out["twin_%s_us" % f] = float(np.median(us["twin"][f]))
    out["%s_twin_over_plain" % f] = float(np.median(np.array(us["twin"][f]) / np.array(us["plain"][f])))
out["launches_per_outer_step"] = {k: int(v // 4) for k, v in sorted(launches["plain"].items())}
print(json.dumps(out))
for a in agents.values():
    a.close()
