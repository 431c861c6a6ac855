#!/usr/bin/env python
"""The feature layer norm's cost in the fused DDPG step: cfg3 (64x64x18, B = 256, 5 minibatches per outer step, 22 000 synthetic rows), a
trainer of plain networks against one of normalised networks (--feature-layer-norm: layer 0 of the four networks without an epilogue,
one ln forward launch behind that GEMM level, two ln backward launches in front of layer 0's dW / dX level; 2 x 100 and 2 x 200 more
floats for the optimiser), ONE process, two agents, alternating timed blocks of hipGraph-replayed outer steps.  Then the launches alone,
event-timed both ways (the library's profiling mode: the eager launch sequence with an event pair around every launch), alternating as
well: the ln forward launch, the ln backward launches (the profiler books the column sums' and the row-local launch in one family: the
mean over the two), the heads launch, the GEMM launches and the optimiser's launch.  Prints one JSON line: steps/s of each and their ratio, microseconds per launch
of each family (medians over the block pairs), and the launch census of an outer step of each -- which must differ by the ln family
alone.
Usage: feature_norm_rate.py [blocks] [steps per block]"""
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


def agent(norm):
    D.set_opts(D.default_opts(use_raw_pixels=True, render_height=64, render_width=64, num_cameras=2, action_repeats=3, batch_size=B,
                              replay_memory_size=ROWS, feature_layer_norm=norm))
    a = D.DeepDeterministicPolicyGradientAgent(Env())
    a.initialise_variables(seed=42)
    a.post_var_init_setup()
    a.replay_memory.fill_synthetic(ROWS, seed=1234)
    return a


agents = {"plain": agent(False), "norm": agent(True)}
assert agents["plain"].actor.feature_norm is None and agents["norm"].critic.feature_norm == ("tanh", 1e-5)
assert agents["norm"].actor.num_params - agents["plain"].actor.num_params == 200
assert agents["norm"].critic.num_params - agents["plain"].critic.num_params == 400
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
LN = ("ln_fwd", "ln_bwd")
us = {k: {f: [] for f in FAMILIES + LN} for k in agents}
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
        for f in FAMILIES + (LN if k == "norm" else ()):
            ms, n = prof[f]
            us[k][f].append(1e3 * ms / n)
        launches[k] = {name: cnt for name, (_ms, cnt) in prof.items()}
ctx.prof_reset()
census = dict(launches["norm"])
assert census.pop("ln_fwd") == 4 * NB and census.pop("ln_bwd") == 2 * 4 * NB and census == launches["plain"], (launches["norm"], launches["plain"])
out = {"workload": "cfg3", "B": B, "batches_per_step": NB, "blocks": blocks, "steps_per_block": steps,
       "plain_steps_per_s": float(np.median(rates["plain"])), "norm_steps_per_s": float(np.median(rates["norm"])),
       "norm_over_plain": float(np.median(np.array(rates["norm"]) / np.array(rates["plain"]))),
       "ln_fwd_us": float(np.median(us["norm"]["ln_fwd"])), "ln_bwd_us_per_launch": float(np.median(us["norm"]["ln_bwd"]))}
for f in FAMILIES:
    out["plain_%s_us" % f] = float(np.median(us["plain"][f]))
    out["norm_%s_us" % f] = float(np.median(us["norm"][f]))
out["launches_per_outer_step"] = {k: {n: int(v // 4) for n, v in sorted(launches[k].items())} for k in ("plain", "norm")}
print(json.dumps(out))
for a in agents.values():
    a.close()
