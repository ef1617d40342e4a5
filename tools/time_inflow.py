#!/usr/bin/env python3
"""Cost of the inflow generator (option "inflow") against the step and the uniform inlet's launch of the same run.  One JSON
line per grid.
  python tools/time_inflow.py [--grids 256,512] [--sigma 8] [--steps 4] [--acc 20]
bench.py's obstacles (sphere + plate through the STL loader), fp32, option "profile" (HIP events on the handle's stream
around each launch).  Per grid N^3 (an N x N inlet plane), on one handle: two warm-up steps (launch plans are timed on the
first), `steps` steps with the option off -- which by construction are the steps of a build without the feature -- then
`steps` steps with it on: a power-law mean map, a fluctuation scale, a gust, and N_eddies = V / sigma^3 rounded (at most
65536) eddies of radius sigma, V the eddy box's volume.  Printed: the "inflow" family's ms per plane (the table kernel and
the plane kernel together), the "misc" family's ms per launch of the option-off run (the uniform inlet is one of its
launches), the whole-step time off and on (wall clock around synchronised steps, profiling on in both), and per timing
family whose time per step moved by more than 1 % of the step, its ms per step off and on: a turbulent inlet makes the
flow rough, and what the rest of the step then costs (the advection's gathers above all) is the flow's doing, not the
pass's."""
import argparse
import json
import os
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import fluid_simulation_amd as F  # noqa: E402
from fluid_simulation_amd import inflow, shapes  # noqa: E402


FAMILIES = ["sweep", "sweep_pair", "sweep_triple", "divergence", "gradient", "advect", "bounds", "misc", "multigrid", "inflow"]


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
    ap.add_argument("--sigma", type=float, default=8.0)
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
            sim.reset_timing()
            off_ms = steps_ms(sim, a.steps)
            misc_ms, misc_n = sim.timing("misc")
            fam_off = {f: sim.timing(f)[0] / a.steps for f in FAMILIES}
            assert sim.timing("inflow")[1] == 0 and misc_n > 0
            side = N - 1 + 2.0 * a.sigma
            eddies = min(65536, int(round(2.0 * a.sigma * side * side / a.sigma ** 3)))
            mean = inflow.power_law(N, N, sim.speed, 1.0 / 7.0, N / 2.0)
            sim.set_inflow(profile=mean, rms=inflow.intensity_profile(N, N, 0.1, N / 2.0, decay=0.25, mean=mean),
                           gust=[(0, 1.0), (1000, 1.2)], eddies=eddies, sigma=a.sigma, u_rms=1.0)
            sim.run_one()                                    # the kernels' code objects, the maps' upload
            sim.reset_timing()
            on_ms = steps_ms(sim, a.steps)
            in_ms, in_n = sim.timing("inflow")
            fam_on = {f: sim.timing(f)[0] / a.steps for f in FAMILIES}
            moved = {f: [round(fam_off[f], 3), round(fam_on[f], 3)] for f in FAMILIES if abs(fam_on[f] - fam_off[f]) > 0.01 * off_ms}
            assert in_n == a.steps
            print(json.dumps({
                "what": "inflow", "grid": [N] * 3, "precision": "fp32", "sigma": a.sigma, "eddies": eddies, "steps": a.steps,
                "inflow_ms_per_plane": round(in_ms / in_n, 4), "misc_ms_per_launch_off": round(misc_ms / misc_n, 4),
                "misc_launches_per_step_off": round(misc_n / a.steps, 2),
                "pairs_per_plane": eddies * N * N, "step_ms_off": round(off_ms, 3), "step_ms_on": round(on_ms, 3),
                "step_overhead_percent": round(100.0 * (on_ms - off_ms) / off_ms, 2),
                "families_ms_per_step_off_on": moved}), flush=True)
            sim.close()


if __name__ == "__main__":
    main()
