#!/usr/bin/env python3
"""A/B of solver options on the benchmark's workloads, one child process per run, variants interleaved:
    python tools/mask_free_time.py c3|c2 STEPS REPS "mask_free=0" "mask_free=1" "mask_free=1;chunk_cost=0" ...
Each run builds the workload as bench.py does (same grid, obstacles, iteration count), sets the options, runs 3 warm-up
steps and times STEPS steps (host clock around work that ends in a device synchronise).  Prints one JSON object: ms per
step of every run per variant.  Development tool."""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHILD = r'''
import json, os, sys, tempfile, time
sys.path.insert(0, %r)
import bench
import fluid_simulation_amd as F
cfg = bench.WORKLOADS[sys.argv[1]]
steps = int(sys.argv[2])
sim = F.Simulation(cfg["W"], cfg["H"], cfg["D"], steps, acc=cfg["acc"], quiet=1, dump_every=0)
for kv in filter(None, sys.argv[3].split(";")):
    k, v = kv.split("=", 1)
    sim.set_option(k, v)
with tempfile.TemporaryDirectory() as tmp:
    bench.add_obstacles(F, sim, cfg, tmp)
for _ in range(3):
    sim.run_one()
sim.sync()
t0 = time.perf_counter()
for _ in range(steps):
    sim.run_one()
sim.sync()
print(json.dumps({"ms_per_step": (time.perf_counter() - t0) * 1e3 / steps, "triple_plan": sim._geti("triple_plan")}))
''' % ROOT

work, steps, reps = sys.argv[1], sys.argv[2], int(sys.argv[3])
variants = sys.argv[4:]
out = {v: [] for v in variants}
for _ in range(reps):
    for v in variants:
        r = subprocess.run([sys.executable, "-c", CHILD, work, steps, v], capture_output=True, text=True, timeout=900)
        if r.returncode != 0:
            sys.stderr.write(r.stderr[-2000:])
            sys.exit("variant %r failed with %d" % (v, r.returncode))
        out[v].append(json.loads(r.stdout.strip().splitlines()[-1]))
print(json.dumps({"workload": work, "steps": int(steps), "runs": out}, indent=1))
