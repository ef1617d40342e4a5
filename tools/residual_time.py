#!/usr/bin/env python3
"""Cost of the residual of the linear solves on bench.py's c3 workload (512^3, sphere + plate, 80 solver iterations):
the yardstick (one Jacobi sweep of the two-sweep kernel, fs_time_sweeps under sweep_fuse=2, on a handle of its own), one
stepping handle timed in alternating blocks of steps with residual_log off and on (ABBA order; the same launch plans and
arrays for both; one untimed step after each switch takes the ring's allocation), then a few profiled steps with the log
on for the "residual" family's own time, and the on-demand query.  One JSON line.
    python tools/residual_time.py [--blocks 6] [--steps 5] [--grid 512] [--precision fp32]"""
import argparse
import json
import os
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import fluid_simulation_amd as F  # noqa: E402
from fluid_simulation_amd import shapes  # noqa: E402


def make(N, acc, tmp, **kw):
    sim = F.Simulation(N, N, N, 1, acc=acc, quiet=1, dump_every=0, **kw)
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
    ap.add_argument("--precision", default="fp32")
    a = ap.parse_args()
    with tempfile.TemporaryDirectory() as tmp:
        # the yardstick: a sweep of the two-sweep kernel on the same grid and mask
        ys = make(a.grid, a.acc, tmp, precision=a.precision, sweep_fuse=2)
        block(ys, 1)
        sweep_ms = [ys.time_sweeps(0, F.PRESSURE, F.DIVERGENCE, 1.0, 6.0, 40) for _ in range(3)]
        ys.close()

        sim = make(a.grid, a.acc, tmp, precision=a.precision)
        block(sim, 2)                                    # warm-up: launch plans are timed on the first steps
        ms = {"off": [], "on": []}
        for b in range(a.blocks):                        # off, on, on, off, ...: a drift of the step time cancels
            order = (("off", 0), ("on", a.steps + 1))
            for mode, n in (order if b % 2 == 0 else order[::-1]):
                sim.set_option("residual_log", n)
                block(sim, 1)
                ms[mode].append(block(sim, a.steps))
        sim.set_option("residual_log", a.steps + 1)
        block(sim, 1)
        sim.set_option("profile", 1)
        sim.reset_timing()
        prof_step = block(sim, a.steps)
        fam_ms, launches = sim.timing("residual")
        rows = sim.residual_log()
        # the on-demand query: launch, copy of the plane records, host sum
        sim.reset_timing()
        sim.sync()
        t0 = time.perf_counter()
        for _ in range(5):
            q = sim.pressure_residual()
        query_wall = (time.perf_counter() - t0) * 1e3 / 5
        q_ms, q_launches = sim.timing("residual")
        med = {k: sorted(v)[len(v) // 2] for k, v in ms.items()}
        diff = sorted(y - x for x, y in zip(ms["off"], ms["on"]))
        sweep = sorted(sweep_ms)[1]
        last = rows[-1]
        print(json.dumps({
            "grid": [a.grid] * 3, "acc": a.acc, "precision": a.precision, "steps_per_block": a.steps,
            "yardstick_ms_per_sweep": [round(v, 4) for v in sweep_ms],
            "ms_per_step_off": [round(v, 3) for v in ms["off"]], "ms_per_step_on": [round(v, 3) for v in ms["on"]],
            "median_off": round(med["off"], 3), "median_on": round(med["on"], 3),
            "overhead_pct": round(100.0 * (med["on"] - med["off"]) / med["off"], 3),
            "paired_diff_ms": [round(v, 3) for v in diff], "mean_paired_diff_pct": round(100.0 * sum(diff) / len(diff) / med["off"], 3),
            "residual_ms_per_step": round(fam_ms / a.steps, 4), "residual_launches": launches,
            "residual_ms_per_launch": round(fam_ms / max(launches, 1), 4),
            "residual_launch_over_sweep": round(fam_ms / max(launches, 1) / sweep, 3),
            "profiled_ms_per_step": round(prof_step, 3), "residual_pct_of_step": round(100.0 * fam_ms / a.steps / med["off"], 3),
            "query_ms_per_launch": round(q_ms / max(q_launches, 1), 4), "query_wall_ms": round(query_wall, 3),
            "pressure_relative_residual": q["relative"], "log_rows": len(rows),
            "last_row_reduction": [float(last["reduction_%d" % k]) for k in range(6)],
            "last_row_relative": [float((last["r_sq_%d" % k] / last["rhs_sq_%d" % k]) ** 0.5) for k in range(6)],
        }))
        sim.close()


if __name__ == "__main__":
    main()
