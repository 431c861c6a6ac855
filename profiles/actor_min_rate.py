#!/usr/bin/env python
"""The cost of the actor on the minimum head in the fused DDPG step: cfg3 (64x64x18, B = 256, 5 minibatches per outer step, 22 000
synthetic rows), a trainer of twin critics (--twin-q: ddpg_heads_twin_kernel) against one with --actor-min-q as well
(ddpg_heads_twin_min_kernel: one more accumulator, two more team sums, three more stores per row -- no launch added), ONE process, two
agents, alternating timed blocks of hipGraph-replayed outer steps.  Then the launches alone, event-timed both ways (the library's profiling
mode: the eager launch sequence with an event pair around every launch), alternating as well.  Prints one JSON line: steps/s of each and
their ratio, microseconds per launch of each family and their ratios (medians over the block pairs), and both launch censuses of an outer
step.

The GEMM-level form against the twin GEMM-level form is the same script on the ablation library with the heads kernel switched off:
    CARTPOLEPP_ABLATION=1 CPP_FUSED_HEADS=0 python profiles/actor_min_rate.py
(the census then differs by the launches DESIGN lists: actor_min_kernel and the GEMM level of head 2's action columns).
Usage: actor_min_rate.py [blocks] [steps per block]"""
import json, os, sys, time
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cartpoleplusplus_amd import ddpg_cartpole as D

shape, B, NB, ROWS = (64, 64, 3, 2, 3), 256, 5, 22000
blocks = int(sys.argv[1]) if len(sys.argv) > 1 else 8
steps = int(sys.argv[2]) if len(sys.argv) > 2 else 40
gemm_levels = os.environ.get("CARTPOLEPP_ABLATION") == "1" and os.environ.get("CPP_FUSED_HEADS") == "0"
FAMILIES = ("gemm", "elementwise", "td", "clip_sgd") if gemm_levels else ("heads", "gemm", "clip_sgd")


class Env(object):
    class S(object):
        def __init__(self, s): self.shape = tuple(s)
    observation_space, action_space = S(shape), S((1, 2))


def agent(amin):
    D.set_opts(D.default_opts(use_raw_pixels=True, render_height=64, render_width=64, num_cameras=2, action_repeats=3, batch_size=B,
                              replay_memory_size=ROWS, twin_q=True, actor_min_q=amin))
    a = D.DeepDeterministicPolicyGradientAgent(Env())
    a.initialise_variables(seed=42)
    a.post_var_init_setup()
    a.replay_memory.fill_synthetic(ROWS, seed=1234)
    return a


agents = {"twin": agent(False), "min": agent(True)}
assert not agents["twin"].trainer.actor_min_q and agents["min"].trainer.actor_min_q
ctx = agents["twin"].actor.ctx
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
        assert prof.get("heads", (0, 0))[1] == (0 if gemm_levels else 4 * NB), prof
        for f in FAMILIES:
            ms, n = prof[f]
            us[k][f].append(1e3 * ms / n)
        launches[k] = {name: cnt for name, (_ms, cnt) in prof.items()}
ctx.prof_reset()
if not gemm_levels:
    assert launches["min"] == launches["twin"], (launches["min"], launches["twin"])      # (no launch added: kernel id by kernel id)
out = {"workload": "cfg3", "form": "gemm-levels" if gemm_levels else "fused-heads", "B": B, "batches_per_step": NB, "blocks": blocks, "steps_per_block": steps,
       "twin_steps_per_s": float(np.median(rates["twin"])), "min_steps_per_s": float(np.median(rates["min"])),
       "min_over_twin": float(np.median(np.array(rates["min"]) / np.array(rates["twin"])))}
for f in FAMILIES:
    out["twin_%s_us" % f] = float(np.median(us["twin"][f]))
    out["min_%s_us" % f] = float(np.median(us["min"][f]))
    out["%s_min_over_twin" % f] = float(np.median(np.array(us["min"][f]) / np.array(us["twin"][f])))
for k in agents:
    out["launches_per_outer_step_" + k] = {name: int(v // 4) for name, v in sorted(launches[k].items())}
print(json.dumps(out))
for a in agents.values():
    a.close()
