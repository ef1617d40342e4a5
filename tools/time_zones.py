#!/usr/bin/env python3
"""Cost of the momentum-zone pass (fs_zones) on the benchmark's workload: bench.py's obstacles (sphere + plate through the STL
loader), fp32, acc 80 by default.
  python tools/time_zones.py [--grid 512] [--acc 80] [--steps 20] [--out FILE.json]
One handle with option "profile", heat and zones both in mode 2: after two warm-up steps the HIP-event times of the families
"zones" (the pass: one launch per step) and "heat" (pass A: one launch per step) over `steps` steps of the same run -- the
yardstick: the zone pass moves 25 B per cell against pass A's 21.  The zones are a tunnel's: a porous slab across the section,
a rotor disk behind the bodies, a sponge of four layers in front of the outlet.  Then the worst case by fs_zone_apply alone:
one resistive zone over the whole domain, where every cell pays the square root and the three divisions; and the budget's
three launches.  A tool, not a test: nothing here gates."""
import argparse
import json
import os
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--grid", type=int, default=512)
    ap.add_argument("--acc", type=int, default=80)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import fluid_simulation_amd as F
    from fluid_simulation_amd import shapes, zones as Z
    N = a.grid
    grid = (N, N, N)
    with tempfile.TemporaryDirectory() as tmp:
        sim = F.Simulation(N, N, N, 1, acc=a.acc, quiet=1, dump_every=0, profile=1)
        sphere = shapes.write_binary_stl(os.path.join(tmp, "sphere.stl"), shapes.sphere_triangles(2.0, 48, 24))
        F.loadSTLIntoObstacles(sphere, sim, 0.3, 0.0, 0.0, 0.0, -N / 4.0, 0.0, 0.0)
        plate = shapes.write_binary_stl(os.path.join(tmp, "plate.stl"), shapes.box_triangles(0.2, 2.4, 1.6))
        F.loadSTLIntoObstacles(plate, sim, 0.45, 0.0, 0.0, 0.0, N / 8.0, 0.0, 0.0)
    tunnel = [Z.porous_box((N // 16, N // 16 + 3, 1, N, 1, N), D=20.0, F=5.0),
              Z.actuator_disk(0, (3 * N // 4, N / 2 + 0.5, N / 2 + 0.5), N / 8.0, 2, 1.33, grid=grid),
              Z.sponge(N - N // 16 + 1, N, 50.0, 4, grid=grid)]
    sim.set_heat(kappa=1e-5, beta=0.5, alpha=0.1, up="+y", inlet=0.0, wall=1.0)
    sim.set_zones(tunnel, mode="step")
    for _ in range(2):
        sim.run_one()
    sim.sync()
    sim.reset_timing()
    for _ in range(a.steps):
        sim.run_one()
    sim.sync()
    cells = float(N) ** 3
    res = {"what": "zones", "grid": list(grid), "precision": "fp32", "acc": a.acc, "steps": a.steps, "zones": int(sim.zones()[0].shape[0]),
           "cells_in_zones": int(sim.zone_budget()[:, 0].sum())}
    ms, n = sim.timing("zones")
    res["zone_pass_ms"] = round(ms / n, 4)
    res["zone_pass_GB_per_s_at_25B_per_cell"] = round(25.0 * cells / (ms / n) / 1e6, 1)
    ms, n = sim.timing("heat")
    res["heat_pass_a_ms"] = round(ms / n, 4)
    res["heat_pass_a_GB_per_s_at_21B_per_cell"] = round(21.0 * cells / (ms / n) / 1e6, 1)
    res["zone_pass_over_heat_pass_a"] = round(res["zone_pass_ms"] / res["heat_pass_a_ms"], 3)
    res["launches"] = {"zones": sim.timing("zones")[1], "heat": n}
    sim.reset_timing()
    for _ in range(a.steps):
        sim.zone_budget()
    ms, n = sim.timing("zones")
    res["budget_ms"] = round(ms * 3 / n, 4)                  # three launches per budget
    sim.set_zones([Z.porous_box((1, N, 1, N, 1, N), D=1.0, F=1.0)], mode="manual")
    sim.apply_zones()
    sim.sync()
    sim.reset_timing()
    for _ in range(a.steps):
        sim.apply_zones()
    sim.sync()
    ms, n = sim.timing("zones")
    res["whole_domain_resistive_pass_ms"] = round(ms / n, 4)
    sim.close()
    text = json.dumps(res, indent=1)
    print(text, flush=True)
    if a.out:
        with open(a.out, "w") as fp:
            fp.write(text + "\n")


if __name__ == "__main__":
    main()
