#!/usr/bin/env python3
"""Cost of the vortex-identification kernel (fs_vortex_field) against the projection's gradient pass.  One JSON line.
  python tools/vortex_time.py [--grid 512] [--precision fp32] [--steps 4] [--reps 10]
bench.py's c3 obstacles (sphere + plate through the STL loader); a few profiled steps give the fields a flow and the
"gradient" family its time per launch (a z-march over the same grid: 29 B per cell in fp32); then, in the same process
and on the same handle, `reps` fetches of every selector under option "profile" (HIP events on the handle's stream
around each launch; the copy to the host is outside them), for both values of "vortex_ry".  Bytes per cell: the
components a selector reads (2 for a vorticity component, 3 for |omega|^2 and Q) + the field written + the flag byte."""
import argparse
import json
import os
import sys
import tempfile

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import fluid_simulation_amd as F  # noqa: E402
from fluid_simulation_amd import shapes  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--grid", type=int, default=512)
    ap.add_argument("--acc", type=int, default=20)
    ap.add_argument("--precision", default="fp32")
    ap.add_argument("--steps", type=int, default=4)
    ap.add_argument("--reps", type=int, default=10)
    a = ap.parse_args()
    N, elem = a.grid, (8 if a.precision == "fp64" else 4)
    with tempfile.TemporaryDirectory() as tmp:
        sim = F.Simulation(N, N, N, 1, acc=a.acc, quiet=1, dump_every=0, precision=a.precision)
        sphere = shapes.write_binary_stl(os.path.join(tmp, "sphere.stl"), shapes.sphere_triangles(2.0, 48, 24))
        F.loadSTLIntoObstacles(sphere, sim, 0.3, 0.0, 0.0, 0.0, -N / 4.0, 0.0, 0.0)
        plate = shapes.write_binary_stl(os.path.join(tmp, "plate.stl"), shapes.box_triangles(0.2, 2.4, 1.6))
        F.loadSTLIntoObstacles(plate, sim, 0.45, 0.0, 0.0, 0.0, N / 8.0, 0.0, 0.0)
        sim.run_one()                                        # warm-up: launch plans are timed on the first step
        sim.set_option("profile", 1)
        sim.reset_timing()
        for _ in range(a.steps):
            sim.run_one()
        grad_ms, grad_n = sim.timing("gradient")
        cells = N ** 3
        out = {"what": "vortex", "grid": [N] * 3, "precision": a.precision, "interior_cells": cells,
               "gradient_us_per_launch": round(grad_ms / grad_n * 1e3, 1), "gradient_launches": grad_n, "vortex_us_per_launch": {},
               "TB_per_s": {}}
        out["gradient_TB_per_s"] = round((7 * elem + 1) * cells / (grad_ms / grad_n) / 1e9, 3)
        buf = None
        for ry in (2, 1):
            sim.set_option("vortex_ry", ry)
            for which, name in enumerate(F.VORTEX_NAMES):
                buf = sim.vortex(which, dtype=np.float32)    # warm-up: the code object, and at first the allocation
                sim.reset_timing()
                for _ in range(a.reps):
                    buf = sim.vortex(which, dtype=np.float32)
                ms, n = sim.timing("vortex")
                assert n == a.reps
                bytes_cell = ((2 if which < 3 else 3) + 1) * elem + 1
                key = "%s ry=%d" % (name, ry)
                out["vortex_us_per_launch"][key] = round(ms / n * 1e3, 1)
                out["TB_per_s"][key] = round(bytes_cell * cells / (ms / n) / 1e9, 3)
        out["q_max"] = float(buf.max())
        out["q_le_gradient"] = out["vortex_us_per_launch"]["q ry=2"] <= out["gradient_us_per_launch"]
        print(json.dumps(out))
        sim.close()


if __name__ == "__main__":
    main()
