#!/usr/bin/env python3
"""Cost of the slice and projection images on bench.py's c3 workload (512^3, sphere + plate, 80 solver iterations).

default: one handle, timed in alternating blocks of steps with the image log off, on with the two default views (density and
  v_x at the middle z-slice, a frame every step) and -- for scale -- off with a full frame dump after every step
  (fs_dump_frame, five volumes); the launch counts per timing family with the log off and on; the host-side way to one
  picture without the feature (fs_get_field of the whole field plus a numpy slice) against image_rgb of the same slice.
--kernels: every kind on every axis `--reps` times through image_values, for a run under
  `rocprofv3 --kernel-trace --stats` (the kernels' own times), with the call times as the host sees them.
One JSON line either way.
    python tools/images_time.py [--blocks 4] [--steps 4] [--grid 512] [--acc 80]
    rocprofv3 --kernel-trace --stats -d DIR --output-format csv -- python tools/images_time.py --kernels [--reps 5]"""
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
            "forces", "residual", "flow_stats", "vortex", "probes", "body_forces"]
KINDS = ["slice", "sum", "max", "min"]


def make(N, acc, tmp, **kw):
    sim = F.Simulation(N, N, N, 1, acc=acc, quiet=1, dump_every=0, **kw)
    # bench.py's c3 obstacles (a sphere and a plate through the STL loader)
    sphere = shapes.write_binary_stl(os.path.join(tmp, "sphere.stl"), shapes.sphere_triangles(2.0, 48, 24))
    F.loadSTLIntoObstacles(sphere, sim, 0.3, 0.0, 0.0, 0.0, -N / 4.0, 0.0, 0.0)
    plate = shapes.write_binary_stl(os.path.join(tmp, "plate.stl"), shapes.box_triangles(0.2, 2.4, 1.6))
    F.loadSTLIntoObstacles(plate, sim, 0.45, 0.0, 0.0, 0.0, N / 8.0, 0.0, 0.0)
    return sim


def block(sim, steps, dump=False):
    sim.sync()
    t0 = time.perf_counter()
    for _ in range(steps):
        sim.run_one()
        if dump:
            sim.dump_frame()
    sim.sync()
    return (time.perf_counter() - t0) * 1e3 / steps


def timed(fn, reps=5):
    fn()                                                 # the first call takes the allocations
    ms = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ms.append((time.perf_counter() - t0) * 1e3)
    return sorted(ms)[len(ms) // 2]


def kernels(a):
    N = a.grid
    with tempfile.TemporaryDirectory() as tmp:
        sim = make(N, 4, tmp)
        for _ in range(2):
            sim.run_one()
        calls = {}
        for axis in (0, 1, 2):
            for kind in KINDS:
                index = (N + 2) // 2 if kind == "slice" else 0
                calls["%s_%s" % (kind, "xyz"[axis])] = round(timed(lambda: sim.image_values(F.VX, kind, axis, index), a.reps), 3)
        rgb = round(timed(lambda: sim.image_rgb(F.VX, "sum", 2, 0, vmin=0.0, vmax=1.0e4, obstacle_alpha=0.2), a.reps), 3)
        print(json.dumps({"grid": [N] * 3, "reps": a.reps, "field_bytes": int(sim._L.fs_padded_size(sim._h)) * 4,
                          "image_values_call_ms": calls, "image_rgb_sum_z_call_ms": rgb}))
        sim.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=4)
    ap.add_argument("--steps", type=int, default=4)
    ap.add_argument("--grid", type=int, default=512)
    ap.add_argument("--acc", type=int, default=80)
    ap.add_argument("--kernels", action="store_true")
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    if a.kernels:
        return kernels(a)
    N = a.grid
    mid = (N + 2) // 2
    views = [(F.DENS, "slice", 2, mid, 0.0, 0.01, 0.2), (F.VX, "slice", 2, mid, -10.0, 10.0, 0.2)]
    with tempfile.TemporaryDirectory() as tmp:
        sim = make(N, a.acc, tmp, dump_dir=os.path.join(tmp, "frames"))
        os.makedirs(os.path.join(tmp, "frames"))
        block(sim, 2)                                    # warm-up: launch plans are timed on the first steps
        sim.set_option("image_log", a.steps + 1)
        modes = ["off", "images", "dump"]
        ms = {m: [] for m in modes}
        for b in range(a.blocks):                        # off, images, dump, dump, images, off, ...: a drift of the step time cancels
            for mode in (modes if b % 2 == 0 else modes[::-1]):
                sim.set_image_views(views if mode == "images" else [])
                block(sim, 1, dump=(mode == "dump"))     # takes the ring's allocation / opens the dump files
                ms[mode].append(block(sim, a.steps, dump=(mode == "dump")))
        sim.set_option("profile", 1)
        counts, fam = {}, {}
        for mode in ("off", "images"):
            sim.set_image_views(views if mode == "images" else [])
            block(sim, 1)
            sim.reset_timing()
            block(sim, a.steps)
            counts[mode] = {f: sim.timing(f)[1] for f in FAMILIES + ["images"]}
            fam[mode] = sim.timing("images")[0]
        steps, images = sim.image_log()
        sim.set_option("profile", 0)
        sim.set_image_views([])
        # one picture without the feature: the whole field to the host, a numpy slice (colouring not counted)
        get_ms = timed(lambda: sim.get(F.DENS)[mid], 3)
        rgb_ms = timed(lambda: viewer.slice_image(sim, "density"), 5)
        med = {k: sorted(v)[len(v) // 2] for k, v in ms.items()}
        same = all(counts["off"][f] == counts["images"][f] for f in FAMILIES)
        print(json.dumps({
            "grid": [N] * 3, "acc": a.acc, "steps_per_block": a.steps,
            "ms_per_step": {m: [round(v, 3) for v in ms[m]] for m in modes},
            "median_ms_per_step": {m: round(med[m], 3) for m in modes},
            "overhead_pct": {m: round(100.0 * (med[m] - med["off"]) / med["off"], 3) for m in modes[1:]},
            "mean_paired_diff_ms": {m: round(sum(y - x for x, y in zip(ms["off"], ms[m])) / len(ms[m]), 4) for m in modes[1:]},
            "launches_per_family": counts, "other_families_same_launches": same,
            "images_ms_per_view": round(fam["images"] / max(counts["images"]["images"], 1), 5),
            "log_frames": int(len(steps)), "frame_bytes": int(sum(im[0].size for im in images)) if len(steps) else 0,
            "get_field_plus_slice_ms": round(get_ms, 3), "slice_image_call_ms": round(rgb_ms, 3),
        }))
        sim.close()


if __name__ == "__main__":
    main()
