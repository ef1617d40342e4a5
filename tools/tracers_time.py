#!/usr/bin/env python3
"""Cost of the tracer particles on bench.py's c3 workload (512^3, sphere + plate, 80 solver iterations).

One handle with "profile" on: `--warm` steps develop the flow, then 2^20 particles are seeded as 1024 rakes of 1024 points
across the tunnel upstream of the sphere and `--steps` more steps are timed -- the "tracers" family's HIP-event time per
advance (the first one, which moves every particle, on its own), the step as the host sees it, and how many particles are
still ALIVE after the first advance and at the end.  --off runs the same steps without
the feature (also what a library of the parent commit does, loaded through FLUIDSIM_LIB).  --shuffle seeds the same points in
a random order instead: what the move costs once neighbours in a wave no longer share cache lines (the case a cell sort
would repair).  One JSON line.
    python tools/tracers_time.py [--off | --shuffle] [--warm 20] [--steps 20] [--grid 512] [--acc 80]"""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import fluid_simulation_amd as F  # noqa: E402
from fluid_simulation_amd import shapes, viewer  # noqa: E402


def make(N, acc, tmp, **kw):
    sim = F.Simulation(N, N, N, 1, acc=acc, quiet=1, dump_every=0, profile=1, **kw)
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
    ap.add_argument("--off", action="store_true")
    ap.add_argument("--shuffle", action="store_true")
    ap.add_argument("--warm", type=int, default=20)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--grid", type=int, default=512)
    ap.add_argument("--acc", type=int, default=80)
    ap.add_argument("--rakes", type=int, default=1024)
    a = ap.parse_args()
    N, R = a.grid, a.rakes
    with tempfile.TemporaryDirectory() as tmp:
        sim = make(N, a.acc, tmp) if a.off else make(N, a.acc, tmp, tracers=R * R)
        warm_ms = block(sim, a.warm)
        if not a.off:
            # rake r spans the tunnel in y at height z_r, a tenth of the way down the tunnel
            z = np.linspace(1.0, float(N), R)
            pts = np.concatenate([viewer.rake((0.1 * N, 1.0, z[r]), (0.1 * N, float(N), z[r]), R) for r in range(R)])
            if a.shuffle:
                pts = pts[np.random.default_rng(1).permutation(len(pts))]
            sim.tracer_seed(pts)
        first = None
        sim.reset_timing()
        if not a.off:                                    # the first advance moves every particle: timed on its own
            first_ms = block(sim, 1)
            first = (sim.timing("tracers")[0], first_ms, int((sim.tracers()["status"] == F.TRACER_ALIVE).sum()))
            sim.reset_timing()
        step_ms = block(sim, a.steps - (0 if a.off else 1))
        out = {"grid": [N] * 3, "acc": a.acc, "warm_steps": a.warm, "steps": a.steps, "library": os.path.basename(os.path.dirname(F._lib.LIB_PATH)),
               "mode": "off" if a.off else ("random order" if a.shuffle else "rakes"), "warm_ms_per_step": round(warm_ms, 3),
               "ms_per_step": round(step_ms, 3)}
        if not a.off:
            ms, launches = sim.timing("tracers")
            status = sim.tracers()["status"]
            out.update({"first_advance_ms": round(first[0], 5), "first_step_ms": round(first[1], 3), "alive_after_first_advance": first[2]})
            out.update({"particles": int(len(status)), "tracers_launches": int(launches), "tracers_ms_per_advance": round(ms / max(launches, 1), 5),
                        "tracers_pct_of_step": round(100.0 * ms / max(launches, 1) / step_ms, 4),
                        "alive_at_end": int((status == F.TRACER_ALIVE).sum()), "out": int((status == F.TRACER_OUT).sum()),
                        "hit": int((status == F.TRACER_HIT).sum())})
        print(json.dumps(out))
        sim.close()


if __name__ == "__main__":
    main()
