#!/usr/bin/env python3
"""Cost of one flow-monitor record (option "monitor_log", fs_flow_monitor) against kernels of the same run.  One JSON line
per grid.
  python tools/time_monitor.py [--grids 256,512] [--steps 4] [--acc 20]
bench.py's obstacles (sphere + plate through the STL loader), fp32, option "profile" (HIP events on the handle's stream around
each launch), one process.  Per grid, on one handle: two warm-up steps (launch plans are timed on the first), `steps` steps
with the log off, one step with it on (the kernels' code objects), then `steps` steps with it on.  Printed: the "monitor"
family's ms per record (three launches: the streaming pass and the two small reductions); the whole-step time off and on (wall
clock around synchronised steps, profiling on in both); and two yardsticks of the same run that are not the code under test:
one "mean" sample of the time-averaged flow statistics (reads the five fields, reads and writes five fp64 accumulators: 100 B
per cell in fp32) and the divergence launch of a projection (reads three velocities and the flag bytes, writes the divergence,
and the pressure where it is zeroed in memory: 17 to 21 B per cell).  The monitor's traffic floor is 21 B per cell (five fp32
fields and one flag byte, read once); floor_ms_at_divergence_rate is the time that floor takes at the bandwidth the divergence
launch reached, counted at 17 B per cell."""
import argparse
import json
import os
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import fluid_simulation_amd as F  # noqa: E402
from fluid_simulation_amd import shapes  # noqa: E402

MONITOR_BYTES = 21.0         # per cell: q, u, v, w, p in fp32 and the flag byte
DIVERGENCE_BYTES = 17.0      # per cell: three velocities and the flag byte in, the divergence out (p is not stored where the solve starts from zeros)
FLOW_STATS_BYTES = 100.0     # per cell: five fp32 fields in, five fp64 accumulators in and out


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
            sim.set_option("monitor_log", a.steps + 1)
            sim.set_option("monitor_stations", "%d,%d" % (N // 8, N // 2))
            sim.run_one()                                    # the kernels' code objects, the workspace
            sim.monitor_log()
            sim.reset_timing()
            on_ms = steps_ms(sim, a.steps)
            mon_ms, mon_n = sim.timing("monitor")
            div_ms, div_n = sim.timing("divergence")
            rows = sim.monitor_log()
            assert mon_n == a.steps == len(rows) and div_n > 0
            sim.set_option("monitor_log", 0)
            # the flow-statistics yardstick: one warm-up sample, then one timed
            sim.set_option("flow_stats", "mean")
            sim.flow_stats_sample()
            sim.reset_timing()
            sim.flow_stats_sample()
            sim.sync()
            fst_ms, fst_n = sim.timing("flow_stats")
            assert fst_n == 1
            mon, div = mon_ms / mon_n, div_ms / div_n
            cells = float(N) ** 3
            div_rate = DIVERGENCE_BYTES * cells / div / 1e6  # GB/s
            floor = MONITOR_BYTES * cells / div_rate / 1e6   # ms
            print(json.dumps({
                "what": "monitor", "grid": [N] * 3, "precision": "fp32", "steps": a.steps,
                "monitor_ms_per_record": round(mon, 4), "monitor_GB_per_s_at_21B_per_cell": round(MONITOR_BYTES * cells / mon / 1e6, 1),
                "divergence_ms_per_launch": round(div, 4), "divergence_GB_per_s_at_17B_per_cell": round(div_rate, 1),
                "flow_stats_mean_ms_per_sample": round(fst_ms, 4),
                "flow_stats_GB_per_s_at_100B_per_cell": round(FLOW_STATS_BYTES * cells / fst_ms / 1e6, 1),
                "floor_ms_at_divergence_rate": round(floor, 4), "monitor_over_floor": round(mon / floor, 2),
                "step_ms_off": round(off_ms, 3), "step_ms_on": round(on_ms, 3),
                "step_overhead_percent": round(100.0 * (on_ms - off_ms) / off_ms, 2),
                "nonfinite": int(rows[-1][2]), "cfl_x": round(F.monitor_cfl(sim.dt, N, N, N, *rows[-1][9:12])[0], 4)}), flush=True)
            sim.close()


if __name__ == "__main__":
    main()
