#!/usr/bin/env python3
"""Cost of the time-averaged flow statistics (option "flow_stats").  One JSON line per call.
  sample:  python tools/flow_stats_time.py sample [--grid 512] [--precision fp32] [--mode moments] [--samples 200]
           the accumulation kernel alone: a few steps give the fields a flow, 3 warm-up samples, then `samples` calls of
           fs_flow_stats_sample under option "profile" (HIP events on the handle's stream around each launch); reports ms
           per sample, the algorithmic bytes (include/fluidsim.h: 4 or 8 B per field read + 16 B per accumulator, per cell
           of the padded array the kernel walks) and TB/s, and one finalize + fetch.
  step:    python tools/flow_stats_time.py step [--grid 512] [--blocks 4] [--steps 5]
           bench.py's c3 workload (512^3, sphere + plate, 80 solver iterations) on one stepping handle, timed in
           alternating blocks of steps with the statistics off and "moments" every step (ABBA order; one untimed step
           after each switch takes the allocation); reports the added ms per step."""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np

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


def walked_cells(N):
    """cells of the pitched layout the kernel walks (csrc/flow_stats.h): rows of sy cells, planes 0 .. N + 1"""
    sy = (N + 5 + 3) // 4 * 4
    return sy * (N + 2) * (N + 2) + 4


def sample(a):
    elem = 8 if a.precision == "fp64" else 4
    nacc = 12 if a.mode == "moments" else 5
    with tempfile.TemporaryDirectory() as tmp:
        sim = make(a.grid, 4, tmp, precision=a.precision, flow_stats=a.mode, flow_stats_start=1 << 30)
        block(sim, 2)
        for _ in range(3):
            sim.flow_stats_sample()
        sim.set_option("profile", 1)
        sim.reset_timing()
        sim.sync()
        t0 = time.perf_counter()
        for _ in range(a.samples):
            sim.flow_stats_sample()
        sim.sync()
        wall = (time.perf_counter() - t0) * 1e3 / a.samples
        ms, launches = sim.timing("flow_stats")
        sim.set_option("profile", 0)
        per = ms / launches
        padded = (a.grid + 2) ** 3
        bytes_cell = 5 * elem + 16 * nacc
        t0 = time.perf_counter()
        mean_u = sim.flow_stats(F.STAT_MEAN_VX, dtype=np.float32)
        fetch = (time.perf_counter() - t0) * 1e3
        print(json.dumps({
            "what": "sample", "grid": [a.grid] * 3, "precision": a.precision, "mode": a.mode, "samples": launches,
            "ms_per_sample": round(per, 4), "wall_ms_per_sample": round(wall, 4), "bytes_per_cell": bytes_cell,
            "padded_cells": padded, "algorithmic_GB": round(bytes_cell * padded / 1e9, 3),
            "TB_per_s": round(bytes_cell * padded / per / 1e9, 3),
            "walked_cells": walked_cells(a.grid), "TB_per_s_walked": round(bytes_cell * walked_cells(a.grid) / per / 1e9, 3),
            "fetch_one_field_ms": round(fetch, 2), "mean_vx_max": float(mean_u.max()),
        }))
        sim.close()


def step(a):
    with tempfile.TemporaryDirectory() as tmp:
        sim = make(a.grid, a.acc, tmp, precision=a.precision)
        block(sim, 2)                                    # warm-up: launch plans are timed on the first steps
        ms = {"off": [], "moments": []}
        for b in range(a.blocks):                        # off, on, on, off, ...: a drift of the step time cancels
            order = ("off", "moments")
            for mode in (order if b % 2 == 0 else order[::-1]):
                sim.set_option("flow_stats", mode)
                block(sim, 1)
                ms[mode].append(block(sim, a.steps))
        sim.set_option("profile", 1)
        sim.reset_timing()
        sim.set_option("flow_stats", "moments")
        block(sim, a.steps)
        fam_ms, launches = sim.timing("flow_stats")
        med = {k: sorted(v)[len(v) // 2] for k, v in ms.items()}
        diff = [y - x for x, y in zip(ms["off"], ms["moments"])]
        print(json.dumps({
            "what": "step", "grid": [a.grid] * 3, "acc": a.acc, "precision": a.precision, "steps_per_block": a.steps,
            "ms_per_step_off": [round(v, 3) for v in ms["off"]], "ms_per_step_moments": [round(v, 3) for v in ms["moments"]],
            "median_off": round(med["off"], 3), "median_moments": round(med["moments"], 3),
            "added_ms_per_step": round(sum(diff) / len(diff), 3), "paired_diff_ms": [round(v, 3) for v in diff],
            "profiled_flow_stats_ms_per_sample": round(fam_ms / max(launches, 1), 4), "profiled_launches": launches,
        }))
        sim.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=["sample", "step"])
    ap.add_argument("--grid", type=int, default=512)
    ap.add_argument("--acc", type=int, default=80)
    ap.add_argument("--precision", default="fp32")
    ap.add_argument("--mode", default="moments", choices=["mean", "moments"])
    ap.add_argument("--samples", type=int, default=200)
    ap.add_argument("--blocks", type=int, default=4)
    ap.add_argument("--steps", type=int, default=5)
    a = ap.parse_args()
    (sample if a.what == "sample" else step)(a)


if __name__ == "__main__":
    main()
