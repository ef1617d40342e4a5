#!/usr/bin/env python3
"""Cost of the per-step force log on bench.py's c3 workload (512^3, sphere + plate, 80 solver iterations): one handle,
timed in alternating blocks of steps with force_log off and on (ABBA order) (the same launch plans and arrays for both; one untimed
step after each switch takes the ring's allocation), then a few profiled steps with the log on for the "forces"
family's own time.  One JSON line.
    python tools/forces_time.py [--blocks 6] [--steps 5] [--grid 512]"""
import argparse
import json
import os
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import fluid_simulation_amd as F  # noqa: E402
from fluid_simulation_amd import shapes  # noqa: E402


def make(N, acc, tmp):
    sim = F.Simulation(N, N, N, 1, acc=acc, quiet=1, dump_every=0)
    # bench.py's c3 obstacles (a sphere and a plate through the STL loader)
    sphere = shapes.write_binary_stl(os.path.join(tmp, "sphere.stl"), shapes.sphere_triangles(2.0, 48, 24))
    F.loadSTLIntoObstacles(sphere, sim, 0.3, 0.0, 0.0, 0.0, -N / 4.0, 0.0, 0.0)
    plate = shapes.write_binary_stl(os.path.join(tmp, "plate.stl"), shapes.box_triangles(0.2, 2.4, 1.6))
    F.loadSTLIntoObstacles(plate, sim, 0.45, 0.0, 0.0, 0.0, N / 8.0, 0.0, 0.0)
    return sim


def block(sim, steps):
    sim.sync()
    t0 = time.perf_counter()
    for _ in range(steps):
        sim.run_one()
    sim.sync()
    return (time.perf_counter() - t0) * 1e3 / steps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=6)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--grid", type=int, default=512)
    ap.add_argument("--acc", type=int, default=80)
    a = ap.parse_args()
    with tempfile.TemporaryDirectory() as tmp:
        sim = make(a.grid, a.acc, tmp)
        block(sim, 2)                                    # warm-up: launch plans are timed on the first steps
        ms = {"off": [], "on": []}
        for b in range(a.blocks):                        # off, on, on, off, ...: a drift of the step time cancels
            order = (("off", 0), ("on", a.steps + 1))
            for mode, n in (order if b % 2 == 0 else order[::-1]):
                sim.set_option("force_log", n)
                block(sim, 1)
                ms[mode].append(block(sim, a.steps))
        sim.set_option("force_log", a.steps + 1)
        block(sim, 1)
        sim.set_option("profile", 1)
        sim.reset_timing()
        prof_step = block(sim, a.steps)
        fam_ms, launches = sim.timing("forces")
        rows = sim.force_log()
        med = {k: sorted(v)[len(v) // 2] for k, v in ms.items()}
        diff = sorted(y - x for x, y in zip(ms["off"], ms["on"]))
        print(json.dumps({
            "grid": [a.grid] * 3, "acc": a.acc, "steps_per_block": a.steps,
            "ms_per_step_off": [round(v, 3) for v in ms["off"]], "ms_per_step_on": [round(v, 3) for v in ms["on"]],
            "median_off": round(med["off"], 3), "median_on": round(med["on"], 3),
            "overhead_pct": round(100.0 * (med["on"] - med["off"]) / med["off"], 3),
            "paired_diff_ms": [round(v, 3) for v in diff], "mean_paired_diff_pct": round(100.0 * sum(diff) / len(diff) / med["off"], 3),
            "forces_ms_per_step": round(fam_ms / a.steps, 4), "forces_launches": launches,
            "forces_ms_per_launch": round(fam_ms / max(launches, 1), 4), "profiled_ms_per_step": round(prof_step, 3),
            "forces_pct_of_step": round(100.0 * fam_ms / a.steps / med["off"], 3),
            "log_rows": len(rows), "last_row": {k: float(rows[-1][k]) for k in ("s2x", "faces", "frontal", "cx")},
        }))
        sim.close()


if __name__ == "__main__":
    main()
