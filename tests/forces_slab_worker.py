"""One rank of a z-slab run with the force log on (spawned by tests/test_gpu_forces.py).
argv: rank nranks idfile outdir W H D steps solver"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import fluid_simulation_amd as F  # noqa: E402


def main():
    rank, nranks = int(sys.argv[1]), int(sys.argv[2])
    idfile, outdir = sys.argv[3], sys.argv[4]
    W, H, D, steps = (int(v) for v in sys.argv[5:9])
    solver = sys.argv[9]
    sim = F.Simulation(W, H, D, steps, acc=8, quiet=1, dump_every=0, solver=solver, force_log=steps + 2)
    if nranks > 1:
        sim.comm_init(rank, nranks, open(idfile, "rb").read())
    Dl, zoff = sim.local_depth, sim.z_offset
    # a ball around the middle of the depth (radius 9 at D = 32): it straddles the boundary of 2 slabs and all three of 4
    z, y, x = np.mgrid[0:D + 2, 0:H + 2, 0:W + 2]
    m = ((x - W / 2.0) ** 2 + (y - H / 2.0) ** 2 + (z - (D / 2.0 + 0.5)) ** 2) <= (9.0 * D / 32.0) ** 2
    m[0] = m[-1] = False
    m[:, 0] = m[:, -1] = False
    m[:, :, 0] = m[:, :, -1] = False
    sim.set_mask(m[zoff:zoff + Dl + 2])
    for _ in range(steps):
        sim.run_one()
    rows = sim.force_log()
    q = sim.obstacle_force(per_plane=True)
    raw = np.stack([rows[k].astype(np.float64) for k in rows.dtype.names[:9]], axis=1)
    np.savez(os.path.join(outdir, "rank%d.npz" % rank), raw=raw, S=q["S"],
             counts=np.array([q["faces"], q["frontal"]]), per_plane=q["per_plane"])
    sim.close()


if __name__ == "__main__":
    main()
