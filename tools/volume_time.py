#!/usr/bin/env python3
"""Cost of one volume-rendered view on bench.py's c3 workload (512^3, sphere + plate, 80 solver iterations).

After `--warm` steps (so that there is a plume to march through) one `--size` view of the density from the 3-D viewer's
orbit (azimuth 45, elevation 30; the distance is chosen so that the whole box is in view) is timed three ways:
  * the ray-march kernel itself: the "volume" timing family's HIP-event time per launch over `--reps` frames taken with
    fs_volume_sample (one launch per view, events on the handle's own stream);
  * volume_render as the host sees it: the call, its device-to-host copy of rgb and the synchronisation included (median);
  * the only way to the same picture without the feature: fetching that one volume to the host with fs_get_field (median;
    rendering it there is not counted).
Then the launch counts per timing family over `--steps` steps with the volume log off and on, and the step time of both.
One JSON line.
    python tools/volume_time.py [--grid 512] [--acc 80] [--warm 8] [--reps 10] [--steps 4] [--size 512x512] [--distance D]"""
import argparse
import json
import os
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import fluid_simulation_amd as F  # noqa: E402
from fluid_simulation_amd import shapes, viewer  # noqa: E402

FAMILIES = ["sweep", "sweep_pair", "sweep_triple", "divergence", "gradient", "advect", "bounds", "misc", "comm", "multigrid",
            "forces", "residual", "flow_stats", "vortex", "probes", "body_forces", "images", "tracers"]


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


def timed(fn, reps):
    fn()                                                 # the first call takes the allocations
    ms = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ms.append((time.perf_counter() - t0) * 1e3)
    return sorted(ms)[len(ms) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--grid", type=int, default=512)
    ap.add_argument("--acc", type=int, default=80)
    ap.add_argument("--warm", type=int, default=8)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--steps", type=int, default=4)
    ap.add_argument("--size", default="512x512")
    ap.add_argument("--distance", type=float, default=0.0)
    a = ap.parse_args()
    N = a.grid
    cols, rows = (int(t) for t in a.size.split("x"))
    dist = a.distance if a.distance > 0 else 2.75 * N        # the box diagonal subtends about 35 of the 45 degrees
    par = dict(vmin=0.0, vmax=0.01, opacity=0.05, step=0.5, t_min=0.01, obstacle=viewer.VOLUME_OBSTACLE,
               background=viewer.VOLUME_BACKGROUND)
    with tempfile.TemporaryDirectory() as tmp:
        sim = make(N, a.acc, tmp)
        block(sim, a.warm)                               # launch plans are timed on the first steps; the plume grows
        rgb = viewer.volume_image(sim, "density", distance=dist, size=(cols, rows), slot=0, **{k: par[k] for k in ("opacity", "step", "t_min")})
        colours = int(len({tuple(c) for c in rgb.reshape(-1, 3)}))
        background = float((rgb.reshape(-1, 3) == viewer.VOLUME_BACKGROUND).all(axis=1).mean())
        render_ms = timed(lambda: sim.volume_render(F.DENS, 0, **par), a.reps)
        fetch_ms = timed(lambda: sim.get(F.DENS), 3)
        # the kernel alone: frames of the log taken by hand
        sim.set_option("profile", 1)
        sim.set_volume_views([(F.DENS, 0, par)])
        sim.set_option("volume_log", a.reps + a.steps + 2)
        sim.volume_sample()
        sim.sync()
        sim.reset_timing()
        for _ in range(a.reps):
            sim.volume_sample()
        kernel_ms, launches = sim.timing("volume")
        # the step: launches per family, log off and on
        counts, step_ms = {}, {}
        for mode in ("off", "on"):
            sim.set_volume_views([(F.DENS, 0, par)] if mode == "on" else [])
            block(sim, 1)
            sim.reset_timing()
            step_ms[mode] = block(sim, a.steps)
            counts[mode] = {f: sim.timing(f)[1] for f in FAMILIES + ["volume"]}
        steps, images = sim.volume_log()
        print(json.dumps({
            "grid": [N] * 3, "acc": a.acc, "warm_steps": a.warm, "size": [cols, rows], "distance": dist, "params": {k: par[k] for k in ("vmin", "vmax", "opacity", "step", "t_min")},
            "distinct_colours": colours, "background_share": round(background, 4),
            "volume_kernel_ms": round(kernel_ms / max(launches, 1), 4), "kernel_launches": launches,
            "volume_render_call_ms": round(render_ms, 3), "rgb_bytes": 3 * cols * rows,
            "get_field_ms": round(fetch_ms, 3), "field_bytes": int(sim._L.fs_padded_size(sim._h)) * 4,
            "ms_per_step": {m: round(v, 3) for m, v in step_ms.items()},
            "launches_per_family": counts,
            "other_families_same_launches": all(counts["off"][f] == counts["on"][f] for f in FAMILIES),
            "log_frames": int(len(steps)), "frame_bytes": int(sim.volume_frame_bytes),
        }))
        sim.close()


if __name__ == "__main__":
    main()
