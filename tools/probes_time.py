#!/usr/bin/env python3
"""Cost of the point probes and the field sampler on bench.py's c3 workload (512^3, sphere + plate, 80 solver iterations):
one handle, timed in alternating blocks of steps with the probe log off, on with 64 probes and on with 4096 probes (the
same launch plans and arrays for all three; one untimed step after each switch takes the ring's allocation), the launch
counts per timing family of a block with the log off and on, the "probes" family's own time per record, and one
fs_sample of a 512 x 512 cut plane (all three modes) and of the obstacle mesh's vertices (mode "fluid").  One JSON line.
    python tools/probes_time.py [--blocks 6] [--steps 5] [--grid 512]"""
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

FAMILIES = ["sweep", "sweep_pair", "sweep_triple", "divergence", "gradient", "advect", "bounds", "misc", "comm", "multigrid",
            "forces", "residual", "flow_stats", "vortex", "probes"]


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


def probe_cells(N, n, rng):
    """a wake rake behind the sphere first, random cells (ghosts included) for the rest"""
    rake = [(min(N, N // 2 + 8 * k), N // 2, N // 2) for k in range(min(n, 16))]
    rest = rng.integers(0, N + 2, size=(n - len(rake), 3))
    return np.concatenate([np.array(rake, dtype=np.int64).reshape(-1, 3), rest]).astype(np.intc)


def timed(fn, reps=5):
    fn()                                                 # the first call takes the allocations
    ms = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ms.append((time.perf_counter() - t0) * 1e3)
    return sorted(ms)[len(ms) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=6)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--grid", type=int, default=512)
    ap.add_argument("--acc", type=int, default=80)
    a = ap.parse_args()
    N = a.grid
    rng = np.random.default_rng(1)
    cells = {"on64": probe_cells(N, 64, rng), "on4096": probe_cells(N, F.PROBE_MAX, rng)}
    with tempfile.TemporaryDirectory() as tmp:
        sim = make(N, a.acc, tmp)
        block(sim, 2)                                    # warm-up: launch plans are timed on the first steps
        sim.set_option("probe_log", a.steps + 1)
        modes = ["off", "on64", "on4096"]
        ms = {m: [] for m in modes}
        for b in range(a.blocks):                        # off, 64, 4096, 4096, 64, off, ...: a drift of the step time cancels
            for mode in (modes if b % 2 == 0 else modes[::-1]):
                sim.set_probes(cells[mode] if mode != "off" else np.zeros((0, 3), dtype=np.intc))
                block(sim, 1)
                ms[mode].append(block(sim, a.steps))
        # launch counts per family with the log off and on, and the family's own time per record
        sim.set_option("profile", 1)
        counts, fam = {}, {}
        for mode in modes:
            sim.set_probes(cells[mode] if mode != "off" else np.zeros((0, 3), dtype=np.intc))
            block(sim, 1)
            sim.reset_timing()
            block(sim, a.steps)
            counts[mode] = {f: sim.timing(f)[1] for f in FAMILIES}
            fam[mode] = sim.timing("probes")[0]
        log = sim.probe_log()
        sim.set_option("profile", 0)
        sim.set_probes(np.zeros((0, 3), dtype=np.intc))
        # the sampler: a cut plane through the wake at an odd position, and the body's surface
        gx, gy = np.meshgrid(np.linspace(0.0, N + 1.0, 512), np.linspace(0.0, N + 1.0, 512), indexing="xy")
        cut = np.stack([gx.ravel(), gy.ravel(), np.full(gx.size, N / 2.0 + 0.37)], axis=1)
        sim.sample_points(cut)
        sample_ms = {m: timed(lambda m=m: sim.sample(F.PRESSURE, m)) for m in ("nearest", "linear", "fluid")}
        upload_ms = timed(lambda: sim.sample_points(cut))
        mesh = viewer.surface_pressure(sim)
        surf_ms = timed(lambda: sim.sample(F.PRESSURE, "fluid"))
        surf_all_ms = timed(lambda: viewer.surface_pressure(sim), reps=3)
        t0 = time.perf_counter()
        sim.get(F.PRESSURE)
        get_ms = (time.perf_counter() - t0) * 1e3
        med = {k: sorted(v)[len(v) // 2] for k, v in ms.items()}
        same = all(counts["off"][f] == counts[m][f] for m in modes for f in FAMILIES if f != "probes")
        print(json.dumps({
            "grid": [N] * 3, "acc": a.acc, "steps_per_block": a.steps,
            "ms_per_step": {m: [round(v, 3) for v in ms[m]] for m in modes},
            "median_ms_per_step": {m: round(med[m], 3) for m in modes},
            "overhead_pct": {m: round(100.0 * (med[m] - med["off"]) / med["off"], 3) for m in modes[1:]},
            "mean_paired_diff_pct": {m: round(100.0 * sum(y - x for x, y in zip(ms["off"], ms[m])) / len(ms[m]) / med["off"], 3)
                                     for m in modes[1:]},
            "launches_per_family": counts, "other_families_same_launches": same,
            "probes_ms_per_record": {m: round(fam[m] / max(counts[m]["probes"], 1), 5) for m in modes[1:]},
            "log_rows": int(len(log["step"])), "log_probes": int(log["values"].shape[1]),
            "cut_512x512_sample_ms": {k: round(v, 3) for k, v in sample_ms.items()}, "cut_512x512_upload_ms": round(upload_ms, 3),
            "surface_vertices": int(mesh["p"].shape[0]), "surface_sample_ms": round(surf_ms, 3),
            "surface_pressure_call_ms": round(surf_all_ms, 3), "cp_range": [float(np.nanmin(mesh["cp"])), float(np.nanmax(mesh["cp"]))],
            "get_field_pressure_ms": round(get_ms, 3),
        }))
        sim.close()


if __name__ == "__main__":
    main()
