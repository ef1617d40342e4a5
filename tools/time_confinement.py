#!/usr/bin/env python3
"""Cost of the vorticity-confinement pass (option "vorticity_confinement") against the projection passes of the same run.
One JSON line per grid.
  python tools/time_confinement.py [--grids 256,512] [--eps 0.25] [--steps 4] [--acc 20]
bench.py's obstacles (sphere + plate through the STL loader), fp32, option "profile" (HIP events on the handle's stream
around each launch).  Per grid, on one handle: two warm-up steps (launch plans are timed on the first), `steps` steps with the
option off, then `steps` steps with it on.  Printed: the "confinement" family's ms per pass beside the "divergence" and
"gradient" families' ms per launch of the same (option-on) run, their ratio -- the yardstick: one pass should cost no more than
one projection's divergence plus gradient, which move 48 B per cell of algorithmic traffic against the pass's 24 -- and the
whole-step time off and on (wall clock around synchronised steps, profiling on in both)."""
import argparse
import json
import os
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import fluid_simulation_amd as F  # noqa: E402
from fluid_simulation_amd import shapes  # noqa: E402


def steps_ms(sim, n):
    sim.sync()
    t0 = time.perf_counter()
    for _ in range(n):
        sim.run_one()
    sim.sync()
    return (time.perf_counter() - t0) * 1e3 / n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--grids", default="256,512")
    ap.add_argument("--acc", type=int, default=20)
    ap.add_argument("--eps", type=float, default=0.25)
    ap.add_argument("--steps", type=int, default=4)
    a = ap.parse_args()
    for N in (int(t) for t in a.grids.split(",")):
        with tempfile.TemporaryDirectory() as tmp:
            sim = F.Simulation(N, N, N, 1, acc=a.acc, quiet=1, dump_every=0, profile=1)
            sphere = shapes.write_binary_stl(os.path.join(tmp, "sphere.stl"), shapes.sphere_triangles(2.0, 48, 24))
            F.loadSTLIntoObstacles(sphere, sim, 0.3, 0.0, 0.0, 0.0, -N / 4.0, 0.0, 0.0)
            plate = shapes.write_binary_stl(os.path.join(tmp, "plate.stl"), shapes.box_triangles(0.2, 2.4, 1.6))
            F.loadSTLIntoObstacles(plate, sim, 0.45, 0.0, 0.0, 0.0, N / 8.0, 0.0, 0.0)
            for _ in range(2):
                sim.run_one()
            off_ms = steps_ms(sim, a.steps)
            sim.set_option("vorticity_confinement", a.eps)
            sim.run_one()                                    # the kernel's code object
            sim.reset_timing()
            on_ms = steps_ms(sim, a.steps)
            conf_ms, conf_n = sim.timing("confinement")
            div_ms, div_n = sim.timing("divergence")
            grad_ms, grad_n = sim.timing("gradient")
            assert conf_n == a.steps and div_n > 0 and grad_n > 0
            conf, div, grad = conf_ms / conf_n, div_ms / div_n, grad_ms / grad_n
            print(json.dumps({
                "what": "confinement", "grid": [N] * 3, "precision": "fp32", "eps": a.eps, "steps": a.steps,
                "confinement_ms_per_pass": round(conf, 4), "divergence_ms_per_launch": round(div, 4),
                "gradient_ms_per_launch": round(grad, 4), "ratio_to_divergence_plus_gradient": round(conf / (div + grad), 3),
                "confinement_GB_per_s_at_24B_per_cell": round(24.0 * N ** 3 / conf / 1e6, 1),
                "step_ms_off": round(off_ms, 3), "step_ms_on": round(on_ms, 3),
                "step_overhead_percent": round(100.0 * (on_ms - off_ms) / off_ms, 2),
                "within_yardstick": conf <= div + grad}), flush=True)
            sim.close()


if __name__ == "__main__":
    main()
