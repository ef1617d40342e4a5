"""One rank of a z-slab run with the residual log (spawned by tests/test_gpu_residual.py).
argv: rank nranks idfile outdir W H D steps solver overlap log"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import fluid_simulation_amd as F  # noqa: E402


def main():
    rank, nranks = int(sys.argv[1]), int(sys.argv[2])
    idfile, outdir = sys.argv[3], sys.argv[4]
    W, H, D, steps = (int(v) for v in sys.argv[5:9])
    solver, overlap, log = sys.argv[9], sys.argv[10], int(sys.argv[11])
    opts = {}
    if nranks > 1 and overlap != "auto":
        opts["overlap"] = overlap
    sim = F.Simulation(W, H, D, steps, acc=8, quiet=1, dump_every=0, solver=solver, residual_log=log, profile=1, **opts)
    if nranks > 1:
        sim.comm_init(rank, nranks, open(idfile, "rb").read())
    Dl, zoff = sim.local_depth, sim.z_offset
    # a ball around the middle of the depth: it straddles the boundary of 2 slabs and the inner boundaries of 4
    z, y, x = np.mgrid[0:D + 2, 0:H + 2, 0:W + 2]
    m = ((x - W / 2.0) ** 2 + (y - H / 2.0) ** 2 + (z - (D / 2.0 + 0.5)) ** 2) <= (min(W, H, D) * 9.0 / 32.0) ** 2
    m[0] = m[-1] = False
    m[:, 0] = m[:, -1] = False
    m[:, :, 0] = m[:, :, -1] = False
    sim.set_mask(m[zoff:zoff + Dl + 2])
    sim.run_one()                        # the schedules and launch plans are chosen (and their exchanges made) in here
    sim.sync()
    sim.reset_timing()
    for _ in range(steps - 1):
        sim.run_one()
    sim.sync()
    comm = sim.timing("comm")[1]         # exchanges and gathers of steps 2 .. `steps`, before any query adds its own
    launches = sim.timing("residual")[1]
    raw = np.zeros((0, 31))
    if log:
        rows = sim.residual_log()
        raw = np.stack([rows[k].astype(np.float64) for k in rows.dtype.names[:31]], axis=1)
    p = sim.pressure_residual(per_plane=True)
    v = sim.diffuse_residual(1, F.VX, F.VX, per_plane=True)
    np.savez(os.path.join(outdir, "rank%d.npz" % rank), raw=raw, comm=comm, launches=launches,
             p=np.array([p["r_sq"], p["rhs_sq"], p["r_max"], p["cells"]]), p_planes=p["per_plane"],
             v=np.array([v["r_sq"], v["rhs_sq"], v["r_max"], v["cells"]]), v_planes=v["per_plane"],
             plan=np.array([sim._geti("overlap_plan") if nranks > 1 else -1]))
    sim.close()


if __name__ == "__main__":
    main()
