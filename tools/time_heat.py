#!/usr/bin/env python3
"""Cost of heat and buoyancy (fs_heat_params) on the benchmark's workload: bench.py's obstacles (sphere + plate through the STL
loader), fp32, acc 80 by default.
  python tools/time_heat.py [--grid 512] [--acc 80] [--steps 5] [--repeats 5] [--parent-lib OLD.so] [--out FILE.json]
Every measurement runs in a child process of its own (FLUIDSIM_LIB names the library it loads), the repeats interleaved:
  * "off": ms per step (wall clock around synchronised steps after two warm-up steps) of a handle that never hears of heat,
    with this tree's library and -- with --parent-lib -- with the library of the commit before, `repeats` times each; the two
    medians must agree within the spread of the repeats (reported, not asserted);
  * "on": ms per step in mode 2 (kappa, beta, alpha > 0, the bodies' walls held at 1), and with option "profile" the HIP-event
    times of pass A (fs_heat_apply, family "heat" alone) beside the gradient march of the same run -- the yardstick: pass A
    moves 21 B per cell against the march's 28 -- and of pass C (fs_heat_budget's three launches).
The expected whole-step cost of mode 2 is one more solve beside the step's seven and one more advection beside its five, plus
the two streaming passes; the measured ratio is printed next to it.  A tool, not a test: nothing here gates."""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHILD = r'''
import json, os, sys, tempfile, time
sys.path.insert(0, %r)
import fluid_simulation_amd as F
from fluid_simulation_amd import shapes
mode, N, acc, steps = sys.argv[1], int(sys.argv[2]), int(sys.argv[3]), int(sys.argv[4])

def steps_ms(sim, n):
    sim.sync()
    t0 = time.perf_counter()
    for _ in range(n):
        sim.run_one()
    sim.sync()
    return (time.perf_counter() - t0) * 1e3 / n

with tempfile.TemporaryDirectory() as tmp:
    sim = F.Simulation(N, N, N, 1, acc=acc, quiet=1, dump_every=0, profile=(1 if mode == "passes" else 0))
    sphere = shapes.write_binary_stl(os.path.join(tmp, "sphere.stl"), shapes.sphere_triangles(2.0, 48, 24))
    F.loadSTLIntoObstacles(sphere, sim, 0.3, 0.0, 0.0, 0.0, -N / 4.0, 0.0, 0.0)
    plate = shapes.write_binary_stl(os.path.join(tmp, "plate.stl"), shapes.box_triangles(0.2, 2.4, 1.6))
    F.loadSTLIntoObstacles(plate, sim, 0.45, 0.0, 0.0, 0.0, N / 8.0, 0.0, 0.0)
    out = {"mode": mode}
    if mode != "off":
        sim.set_heat(kappa=1e-5, beta=0.5, alpha=0.1, up="+y", inlet=0.0, wall=1.0, in_step=(mode == "on"))
    for _ in range(2):
        sim.run_one()
    if mode in ("off", "on"):
        out["ms_per_step"] = steps_ms(sim, steps)
    else:
        sim.heat_apply()
        sim.heat_budget()                                    # the kernels' code objects
        sim.reset_timing()
        for _ in range(steps):
            sim.heat_apply()
        sim.sync()
        ms, n = sim.timing("heat")
        out["pass_a_ms"] = ms / n
        sim.reset_timing()
        for _ in range(steps):
            sim.heat_budget()
        ms, n = sim.timing("heat")
        out["pass_c_ms"] = ms * 3 / n                        # three launches per budget
        sim.reset_timing()
        for _ in range(2):
            sim.run_one()
        sim.sync()
        ms, n = sim.timing("gradient")
        out["gradient_ms_per_launch"] = ms / n
        ms, n = sim.timing("advect")
        out["advect_ms_per_launch"] = ms / n
    print(json.dumps(out))
    sim.close()
''' % ROOT


def child(mode, lib, a):
    env = dict(os.environ)
    if lib:
        env["FLUIDSIM_LIB"] = os.path.abspath(lib)
    r = subprocess.run([sys.executable, "-c", CHILD, mode, str(a.grid), str(a.acc), str(a.steps)], env=env, capture_output=True,
                       text=True, timeout=900)
    if r.returncode != 0:
        raise SystemExit("child %s (%s) failed: %s" % (mode, lib or "this tree", r.stderr[-600:]))
    return json.loads(r.stdout.strip().splitlines()[-1])


def spread(v):
    return {"median": round(statistics.median(v), 3), "min": round(min(v), 3), "max": round(max(v), 3), "runs": [round(x, 3) for x in v]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--grid", type=int, default=512)
    ap.add_argument("--acc", type=int, default=80)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--parent-lib", default=None, help="libfluidsim.so of the commit before: its heat-off step time in the same run")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    off, parent, on = [], [], []
    for _ in range(a.repeats):
        if a.parent_lib:
            parent.append(child("off", a.parent_lib, a)["ms_per_step"])
        off.append(child("off", None, a)["ms_per_step"])
        on.append(child("on", None, a)["ms_per_step"])
    passes = child("passes", None, a)
    N = a.grid
    res = {"what": "heat", "grid": [N] * 3, "precision": "fp32", "acc": a.acc, "steps": a.steps, "repeats": a.repeats,
           "step_ms_heat_off": spread(off), "step_ms_heat_off_parent": spread(parent) if parent else None,
           "step_ms_mode_2": spread(on)}
    if parent:
        d = abs(res["step_ms_heat_off"]["median"] - res["step_ms_heat_off_parent"]["median"])
        width = max(res["step_ms_heat_off"]["max"] - res["step_ms_heat_off"]["min"],
                    res["step_ms_heat_off_parent"]["max"] - res["step_ms_heat_off_parent"]["min"])
        res["heat_off_vs_parent"] = {"median_difference_ms": round(d, 3), "run_to_run_spread_ms": round(width, 3),
                                     "within_spread": d <= width}
    ratio = res["step_ms_mode_2"]["median"] / res["step_ms_heat_off"]["median"]
    res["mode_2_over_off"] = round(ratio, 4)
    res["expected_note"] = "one more solve beside seven and one more advection beside five, plus two streaming passes"
    res["pass_a_ms"] = round(passes["pass_a_ms"], 4)
    res["pass_a_GB_per_s_at_21B_per_cell"] = round(21.0 * N ** 3 / passes["pass_a_ms"] / 1e6, 1)
    res["pass_c_ms"] = round(passes["pass_c_ms"], 4)
    res["gradient_march_ms_per_launch"] = round(passes["gradient_ms_per_launch"], 4)
    res["advect_ms_per_launch"] = round(passes["advect_ms_per_launch"], 4)
    res["pass_a_over_gradient_march"] = round(passes["pass_a_ms"] / passes["gradient_ms_per_launch"], 3)
    res["pass_a_within_yardstick"] = passes["pass_a_ms"] <= passes["gradient_ms_per_launch"]
    text = json.dumps(res, indent=1)
    print(text, flush=True)
    if a.out:
        with open(a.out, "w") as fp:
            fp.write(text + "\n")


if __name__ == "__main__":
    main()
