#!/usr/bin/env python3
"""Cost of the per-body force and moment records on bench.py's c3 workload (512^3, sphere + plate, 80 solver iterations):
one handle, one run with profile=1 and both force_log and body_force_log on -- the "body_forces" family's time per
record next to the "forces" family's, the step time of that same run, and the time of one labelling.  One JSON line.
    python tools/bodies_time.py [--steps 5] [--grid 512]"""
import argparse
import json
import os
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import fluid_simulation_amd as F  # noqa: E402
from fluid_simulation_amd import shapes  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--grid", type=int, default=512)
    ap.add_argument("--acc", type=int, default=80)
    a = ap.parse_args()
    N = a.grid
    with tempfile.TemporaryDirectory() as tmp:
        sim = F.Simulation(N, N, N, 1, acc=a.acc, quiet=1, dump_every=0)
        # bench.py's c3 obstacles (a sphere and a plate through the STL loader)
        sphere = shapes.write_binary_stl(os.path.join(tmp, "sphere.stl"), shapes.sphere_triangles(2.0, 48, 24))
        F.loadSTLIntoObstacles(sphere, sim, 0.3, 0.0, 0.0, 0.0, -N / 4.0, 0.0, 0.0)
        plate = shapes.write_binary_stl(os.path.join(tmp, "plate.stl"), shapes.box_triangles(0.2, 2.4, 1.6))
        F.loadSTLIntoObstacles(plate, sim, 0.45, 0.0, 0.0, 0.0, N / 8.0, 0.0, 0.0)
        for _ in range(2):                               # warm-up: launch plans are timed on the first steps
            sim.run_one()
        sim.sync()
        t0 = time.perf_counter()
        info = sim.label_bodies()
        label_ms = (time.perf_counter() - t0) * 1e3
        sim.set_option("moment_origin", (N / 2.0, N / 2.0, N / 2.0))
        sim.set_option("force_log", a.steps + 1)
        sim.set_option("body_force_log", a.steps + 1)
        sim.run_one()                                    # takes the rings' allocation
        sim.set_option("profile", 1)
        sim.reset_timing()
        sim.sync()
        t0 = time.perf_counter()
        for _ in range(a.steps):
            sim.run_one()
        sim.sync()
        step_ms = (time.perf_counter() - t0) * 1e3 / a.steps
        body_ms, body_n = sim.timing("body_forces")
        force_ms, force_n = sim.timing("forces")
        rows = sim.body_force_log()
        total = sim.force_log()
        print(json.dumps({
            "grid": [N] * 3, "acc": a.acc, "steps": a.steps, "profiled_ms_per_step": round(step_ms, 3),
            "body_forces_records": body_n, "body_forces_ms_per_record": round(body_ms / max(body_n, 1), 4),
            "forces_records": force_n, "forces_ms_per_record": round(force_ms / max(force_n, 1), 4),
            "label_ms": round(label_ms, 2), "components": sim.body_components,
            "bodies": [{k: int(r[k]) for k in ("body", "cells", "xmin", "xmax", "ymin", "ymax", "zmin", "zmax", "frontal")} for r in info],
            "last_step": [{k: float(r[k]) for k in ("body", "s2x", "m2z", "faces", "cx", "cmz")} for r in rows[-len(info):]],
            "last_step_total_s2x": float(total[-1]["s2x"]), "last_step_total_faces": int(total[-1]["faces"]),
        }))
        sim.close()


if __name__ == "__main__":
    main()
