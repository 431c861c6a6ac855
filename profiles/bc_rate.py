#!/usr/bin/env python
"""The cost of the behaviour-cloning actor term (--bc-alpha; csrc/bc.hip) in the fused DDPG step: cfg3 (64x64x18, B = 256, 5 minibatches per
outer step, 22 000 synthetic rows), a plain trainer against one with --bc-alpha 2.5, ONE process, two agents, alternating timed blocks of
hipGraph-replayed outer steps.  A trainer with the term always takes the GEMM levels (lambda needs every row of the minibatch, the heads
kernel spreads the rows over workgroups), so the two comparisons are two runs of this script:
    python profiles/bc_rate.py                                              the BC step against the default fused-heads step
    CARTPOLEPP_ABLATION=1 CPP_FUSED_HEADS=0 python profiles/bc_rate.py      ... against the scalar step on the same GEMM levels
Then the launches alone, event-timed both ways (the library's profiling mode: the eager launch sequence with an event pair around every
launch), alternating as well.  Prints one JSON line: steps/s of each and their ratio, microseconds per launch of each family (the bc
launch among them) and both launch censuses of an outer step.
Usage: bc_rate.py [blocks] [steps per block]"""
import json, os, sys, time
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cartpoleplusplus_amd import ddpg_cartpole as D

shape, B, NB, ROWS = (64, 64, 3, 2, 3), 256, 5, 22000
blocks = int(sys.argv[1]) if len(sys.argv) > 1 else 8
steps = int(sys.argv[2]) if len(sys.argv) > 2 else 40
gemm_levels = os.environ.get("CARTPOLEPP_ABLATION") == "1" and os.environ.get("CPP_FUSED_HEADS") == "0"
FAMILIES = ("bc", "gemm", "elementwise", "td", "heads", "clip_sgd")


class Env(object):
    class S(object):
        def __init__(self, s): self.shape = tuple(s)
    observation_space, action_space = S(shape), S((1, 2))


def agent(alpha):
    D.set_opts(D.default_opts(use_raw_pixels=True, render_height=64, render_width=64, num_cameras=2, action_repeats=3, batch_size=B,
                              replay_memory_size=ROWS, bc_alpha=alpha))
    a = D.DeepDeterministicPolicyGradientAgent(Env())
    a.initialise_variables(seed=42)
    a.post_var_init_setup()
    a.replay_memory.fill_synthetic(ROWS, seed=1234)
    return a


agents = {"plain": agent(None), "bc": agent(2.5)}
assert agents["plain"].trainer.behaviour_cloning[0] == 0.0 and agents["bc"].trainer.behaviour_cloning[0] == 2.5
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
assert launches["bc"]["bc"] == 4 * NB and not launches["bc"].get("heads", 0) and not launches["plain"].get("bc", 0), launches
assert launches["plain"].get("heads", 0) == (0 if gemm_levels else 4 * NB), launches["plain"]
lam, m, _g, _rows = agents["bc"].trainer.last_behaviour_cloning(B)
out = {"workload": "cfg3", "against": "gemm-levels" if gemm_levels else "fused-heads", "B": B, "batches_per_step": NB, "blocks": blocks,
       "steps_per_block": steps, "plain_steps_per_s": float(np.median(rates["plain"])), "bc_steps_per_s": float(np.median(rates["bc"])),
       "bc_over_plain": float(np.median(np.array(rates["bc"]) / np.array(rates["plain"]))), "last_lambda": lam, "last_m": m}
for k in agents:
    for f in FAMILIES:
        if us[k][f]:
            out["%s_%s_us" % (k, f)] = float(np.median(us[k][f]))
    out["launches_per_outer_step_" + k] = {name: int(v // 4) for name, v in sorted(launches[k].items())}
print(json.dumps(out))
for a in agents.values():
    a.close()
