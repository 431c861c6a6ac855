#!/usr/bin/env python
"""The pooled twin quantile critics' cost in the fused DDPG step: cfg3 (64x64x18, B = 256, 5 minibatches per outer step, 22 000 synthetic
rows), the trainers below in ONE process on alternating timed blocks of hipGraph-replayed outer steps:
    quant_d2     --quantile-critic --num-quantiles 25 --drop-top-quantiles 2          (csrc/quant.hip: one head)
    twin         --twin-q --actor-min-q                                               (the twin scalar step; see below)
    pooled       --pooled-quantile-critics (N = 25, d = 2 per head)                   (csrc/quant_pool.hip: two launches per minibatch)
    sac_twin     --soft-actor-critic --twin-q
    sac_pooled   --soft-actor-critic --pooled-quantile-critics                        (TQC)
Then the launches alone, event-timed (the library's profiling mode: the eager launch sequence with an event pair around every launch),
alternating as well.  Two runs say two things about `twin`:
    pooled_quantile_rate.py                                             the twin scalar trainer on its default route (the fused heads launch)
    CARTPOLEPP_ABLATION=1 CPP_FUSED_HEADS=0 pooled_quantile_rate.py     the twin scalar trainer on the SAME GEMM levels (td_kernel, actor_min)
Prints one JSON line: steps/s of each, the ratios of the pooled steps to their comparisons, microseconds per launch of the quant (a pooled
trainer's: quant_pool.hip's launches) / td / heads / sac / gemm families (medians over the block pairs), and the launch census of an outer step of each.
Usage: pooled_quantile_rate.py [blocks] [steps per block]"""
import json, os, sys, time
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cartpoleplusplus_amd import ddpg_cartpole as D

shape, B, NB, ROWS = (64, 64, 3, 2, 3), 256, 5, 22000
NQ, DROP = 25, 2
blocks = int(sys.argv[1]) if len(sys.argv) > 1 else 8
steps = int(sys.argv[2]) if len(sys.argv) > 2 else 40
FAMILIES = ("quant", "td", "heads", "sac", "gemm", "clip_sgd")
POOLED = dict(pooled_quantile_critics=True, pooled_num_quantiles=NQ, pooled_drop_per_head=DROP)
KINDS = {"quant_d2": dict(quantile_critic=True, num_quantiles=NQ, drop_top_quantiles=DROP),
         "twin": dict(twin_q=True, actor_min_q=True),
         "pooled": POOLED,
         "sac_twin": dict(soft_actor_critic=True, twin_q=True),
         "sac_pooled": dict(soft_actor_critic=True, **POOLED)}


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
assert agents["pooled"].critic.pooled == (NQ, 1.0, DROP) and agents["sac_pooled"].critic.pooled == (NQ, 1.0, DROP) and agents["twin"].critic.pooled is None
# (both q layers N wide: 51 (N - 1) more parameters per head than the twin scalar critic)
assert agents["pooled"].critic.num_params - agents["twin"].critic.num_params == 2 * 51 * (NQ - 1)
ctx = agents["pooled"].actor.ctx
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
# (the pooled launches are counted in the `quant` family: a trainer has quant.hip's launches or quant_pool.hip's, never both)
for k in ("pooled", "sac_pooled", "quant_d2"):
    assert launches[k]["quant"] == 2 * 4 * NB and not any(launches[k].get(f, 0) for f in ("heads", "td", "dist")), launches[k]
assert not any(launches[k].get("quant", 0) for k in ("twin", "sac_twin"))


def ratio(a, b):
    return float(np.median(np.array(rates[a]) / np.array(rates[b])))


out = {"workload": "cfg3", "B": B, "batches_per_step": NB, "blocks": blocks, "steps_per_block": steps, "quantiles_per_head": NQ, "drop_per_head": DROP,
       "twin_route": "fused heads" if launches["twin"].get("heads", 0) else "gemm levels"}
for k in agents:
    out["%s_steps_per_s" % k] = float(np.median(rates[k]))
out["pooled_over_quant_d2"], out["pooled_over_twin"] = ratio("pooled", "quant_d2"), ratio("pooled", "twin")
out["sac_pooled_over_sac_twin"] = ratio("sac_pooled", "sac_twin")
for k in agents:
    for f in FAMILIES:
        if us[k][f]:
            out["%s_%s_us" % (k, f)] = float(np.median(us[k][f]))
for k in agents:
    out["%s_launches_per_outer_step" % k] = {name: int(v // 4) for name, v in sorted(launches[k].items()) if v}
print(json.dumps(out))
for a in agents.values():
    a.close()
