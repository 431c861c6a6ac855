#!/usr/bin/env python
"""What --ddpg-optimiser costs the fused DDPG step: cfg3 (64x64x18, B = 256, 5 minibatches per outer step, 22 000 synthetic rows),
ONE process, three agents -- GradientDescent, Momentum, Adam -- alternating timed blocks of hipGraph-replayed outer steps.  Prints one
JSON line: steps/s of each, Momentum's and Adam's as a fraction of GradientDescent's (median over the block triples), the optimiser
launch's duration per kind (one profiled outer step each: event-timed launches, mean over its 5 minibatches) and, with --rider, the
Adam step of the ablation library with the conv1 image rider on and off (CPP_RIDE_IMAGE_UPDATE=0: the image by a launch of its own, as
NAF under Adam pays it) in alternating child processes.
Usage: ddpg_opt_rate.py [--rider] [blocks] [steps per block]"""
import json, os, subprocess, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

shape, B, NB, ROWS = (64, 64, 3, 2, 3), 256, 5, 22000
rider = "--rider" in sys.argv
child = "--child" in sys.argv
args = [a for a in sys.argv[1:] if not a.startswith("--")]
blocks = int(args[0]) if len(args) > 0 else 8
steps = int(args[1]) if len(args) > 1 else 40
KINDS = {"sgd": ("GradientDescent", {}), "momentum": ("Momentum", {"momentum": 0.9}), "adam": ("Adam", {})}


class Env(object):
    class S(object):
        def __init__(self, s): self.shape = tuple(s)
    observation_space, action_space = S(shape), S((1, 2))


def agent(kind):
    from cartpoleplusplus_amd import ddpg_cartpole as D
    name, oargs = KINDS[kind]
    D.set_opts(D.default_opts(use_raw_pixels=True, render_height=64, render_width=64, num_cameras=2, action_repeats=3, batch_size=B,
                              replay_memory_size=ROWS, ddpg_optimiser=name, ddpg_optimiser_args=json.dumps(oargs)))
    a = D.DeepDeterministicPolicyGradientAgent(Env())
    a.initialise_variables(seed=42)
    a.post_var_init_setup()
    a.replay_memory.fill_synthetic(ROWS, seed=1234)
    return a


def measure(kinds):
    agents = {k: agent(k) for k in kinds}
    ctx = next(iter(agents.values())).actor.ctx
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
    launch_us = {}
    for k, a in agents.items():          # one profiled outer step: the optimiser launch's event time
        ctx.sync(); ctx.prof_reset(); ctx.prof_enable(True)
        a.train_step(B, NB)
        ctx.sync(); ctx.prof_enable(False)
        prof = ctx.prof_read(); ctx.prof_reset()
        ms, n = prof.get("clip_sgd", (0.0, 0))
        launch_us[k] = 1e3 * ms / max(n, 1)
        launch_us[k + "_conv1_image_launches"] = prof.get("conv1_image", (0.0, 0))[1]
    for a in agents.values():
        a.close()
    return rates, launch_us


if child:
    rates, launch_us = measure(["adam"])
    print(json.dumps({"adam_steps_per_s": float(np.median(rates["adam"])), "launch_us": launch_us}))
    sys.exit(0)

rates, launch_us = measure(list(KINDS))
sgd = np.array(rates["sgd"])
out = {"workload": "cfg3", "B": B, "batches_per_step": NB, "blocks": blocks, "steps_per_block": steps}
for k in KINDS:
    out[k + "_steps_per_s"] = float(np.median(rates[k]))
out["momentum_over_sgd"] = float(np.median(np.array(rates["momentum"]) / sgd))
out["adam_over_sgd"] = float(np.median(np.array(rates["adam"]) / sgd))
out["optimiser_launch_us"] = launch_us
if rider:
    res = {"on": [], "off": []}
    for _ in range(2):
        for name, extra in (("on", {}), ("off", {"CPP_RIDE_IMAGE_UPDATE": "0"})):
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", str(max(2, blocks // 2)), str(steps)], cwd=ROOT,
                               env=dict(os.environ, CARTPOLEPP_ABLATION="1", **extra), stdout=subprocess.PIPE, timeout=900)
            assert r.returncode == 0
            res[name].append(json.loads(r.stdout.decode().strip().splitlines()[-1]))
    out["adam_rider_on_steps_per_s"] = float(np.median([x["adam_steps_per_s"] for x in res["on"]]))
    out["adam_rider_off_steps_per_s"] = float(np.median([x["adam_steps_per_s"] for x in res["off"]]))
    out["adam_rider_off_over_on"] = out["adam_rider_off_steps_per_s"] / out["adam_rider_on_steps_per_s"]
    out["adam_rider_on_launch_us"], out["adam_rider_off_launch_us"] = res["on"][-1]["launch_us"], res["off"][-1]["launch_us"]
print(json.dumps(out))
