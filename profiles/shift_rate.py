#!/usr/bin/env python
"""Random shift's cost in the fused DDPG step: cfg3 (64x64x18, B = 256, 5 minibatches per outer step, 22 000 synthetic rows), a
memory on which the augmentation was never enabled against one at pad = 4, ONE process, two agents, alternating timed blocks of
hipGraph-replayed outer steps.  Prints one JSON line: steps/s of each and their ratio (median over the block pairs).
Run as it is, "off" is the direct path (conv1 reads the replay store, no gathered copy): pad4 / off is the price of materialising
the minibatch.  Run on the ablation library with the copy kept,
    CARTPOLEPP_ABLATION=1 CPP_DIRECT_REPLAY=0 python profiles/shift_rate.py
"off" is the unshifted copying gather, which moves the same bytes as the shifted one: pad4 / off is then the price of the shift
itself (the kernels' own durations: the same command under rocprofv3 --kernel-trace --stats, gather_stats_kernel /
reduce_gather_kernel against gather_shift_kernel / reduce_gather_shift_kernel).
--naf: the fused NAF step at cfg4 instead (64x64x18, B = 256, shared trunk, Momentum, 5 minibatches per step, 22 000 rows).
Usage: shift_rate.py [--naf] [blocks] [steps per block]"""
import json, os, sys, time
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cartpoleplusplus_amd import ddpg_cartpole as D
from cartpoleplusplus_amd import naf_cartpole as F

shape, B, NB, ROWS, PAD = (64, 64, 3, 2, 3), 256, 5, 22000, 4
naf = "--naf" in sys.argv
args = [a for a in sys.argv[1:] if a != "--naf"]
blocks = int(args[0]) if len(args) > 0 else 8
steps = int(args[1]) if len(args) > 1 else 40
copy_kept = os.environ.get("CARTPOLEPP_ABLATION") == "1" and os.environ.get("CPP_DIRECT_REPLAY") == "0"


class Env(object):
    class S(object):
        def __init__(self, s): self.shape = tuple(s)
    observation_space, action_space = S(shape), S((1, 2))


def agent(pad):
    if naf:          # cfg4: the shared trunk under Momentum (exps/run_93.sh)
        F.set_opts(F.default_opts(use_raw_pixels=True, render_height=64, render_width=64, num_cameras=2, action_repeats=3, batch_size=B,
                                  replay_memory_size=ROWS, share_input_state_representation=True, optimiser="Momentum",
                                  optimiser_args=json.dumps({"learning_rate": 0.01, "momentum": 0.9})))
        a = F.NormalizedAdvantageFunctionAgent(Env())
    else:
        D.set_opts(D.default_opts(use_raw_pixels=True, render_height=64, render_width=64, num_cameras=2, action_repeats=3, batch_size=B,
                                  replay_memory_size=ROWS))
        a = D.DeepDeterministicPolicyGradientAgent(Env())
    a.initialise_variables(seed=42)
    a.post_var_init_setup()
    a.replay_memory.fill_synthetic(ROWS, seed=1234)
    if pad > 0:
        a.replay_memory.enable_random_shift(pad, seed=7)
    return a


agents = {"off": agent(0), "pad4": agent(PAD)}
ctx = agents["off"].value_net.ctx if naf else agents["off"].actor.ctx
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
per_block = np.array(rates["pad4"]) / np.array(rates["off"])
assert agents["pad4"].replay_memory.shift_counter() == (4 + blocks * steps) * NB
print(json.dumps({"workload": "naf-cfg4" if naf else "cfg3", "B": B, "batches_per_step": NB, "blocks": blocks, "steps_per_block": steps,
                  "off_is": "copy path (CPP_DIRECT_REPLAY=0, ablation library)" if copy_kept else "direct path",
                  "off_steps_per_s": float(np.median(rates["off"])), "pad4_steps_per_s": float(np.median(rates["pad4"])),
                  "pad4_over_off": float(np.median(per_block)), "pad4_over_off_min": float(per_block.min()),
                  "pad4_over_off_max": float(per_block.max()),
                  "off_spread": float((max(rates["off"]) - min(rates["off"])) / np.median(rates["off"]))}))
for a in agents.values():
    a.close()
