#!/usr/bin/env python
"""n-step returns' cost in the fused DDPG step: cfg3 (64x64x18, B = 256, 5 minibatches per outer step, 22 000 synthetic rows), a
memory at n = 1 (never set: the uniform gather instances) against one at n = 3 (the walking instances; the synthetic fill's 50-step
episodes chain s2[i] == s1[i + 1], so the walk does real work), ONE process, two agents, alternating timed blocks of hipGraph-replayed
outer steps.  Prints one JSON line: steps/s of each and their ratio (median over the block pairs).
--naf: the fused NAF step at cfg4 instead (64x64x18, B = 256, shared trunk, Momentum, 5 minibatches per step, 22 000 rows).
Usage: nstep_rate.py [--naf] [blocks] [steps per block]"""
import json, os, sys, time
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cartpoleplusplus_amd import ddpg_cartpole as D
from cartpoleplusplus_amd import naf_cartpole as F

shape, B, NB, ROWS = (64, 64, 3, 2, 3), 256, 5, 22000
naf = "--naf" in sys.argv
args = [a for a in sys.argv[1:] if a != "--naf"]
blocks = int(args[0]) if len(args) > 0 else 8
steps = int(args[1]) if len(args) > 1 else 40


class Env(object):
    class S(object):
        def __init__(self, s): self.shape = tuple(s)
    observation_space, action_space = S(shape), S((1, 2))


def agent(n):
    if naf:          # cfg4: the shared trunk under Momentum (exps/run_93.sh)
        F.set_opts(F.default_opts(use_raw_pixels=True, render_height=64, render_width=64, num_cameras=2, action_repeats=3, batch_size=B,
                                  replay_memory_size=ROWS, share_input_state_representation=True, optimiser="Momentum",
                                  optimiser_args=json.dumps({"learning_rate": 0.01, "momentum": 0.9})))
        a = F.NormalizedAdvantageFunctionAgent(Env())
        discount = F.opts.discount
    else:
        D.set_opts(D.default_opts(use_raw_pixels=True, render_height=64, render_width=64, num_cameras=2, action_repeats=3, batch_size=B,
                                  replay_memory_size=ROWS))
        a = D.DeepDeterministicPolicyGradientAgent(Env())
        discount = D.opts.discount
    a.initialise_variables(seed=42)
    a.post_var_init_setup()
    a.replay_memory.fill_synthetic(ROWS, seed=1234)
    if n > 1:
        a.replay_memory.enable_n_step(n, discount)
    return a


agents = {"n1": agent(1), "n3": agent(3)}
ctx = agents["n1"].value_net.ctx if naf else agents["n1"].actor.ctx
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
ratio = float(np.median(np.array(rates["n3"]) / np.array(rates["n1"])))
print(json.dumps({"workload": "naf-cfg4" if naf else "cfg3", "B": B, "batches_per_step": NB, "blocks": blocks, "steps_per_block": steps,
                  "n1_steps_per_s": float(np.median(rates["n1"])), "n3_steps_per_s": float(np.median(rates["n3"])),
                  "n3_over_n1": ratio}))
for a in agents.values():
    a.close()
