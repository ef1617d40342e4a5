"""One rank of a z-slab run that fetches the vortex-identification fields (spawned by tests/test_gpu_vortex.py).
argv: rank nranks idfile outdir W H D steps"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import fluid_simulation_amd as F  # noqa: E402


def main():
    rank, nranks = int(sys.argv[1]), int(sys.argv[2])
    idfile, outdir = sys.argv[3], sys.argv[4]
    W, H, D, steps = (int(v) for v in sys.argv[5:9])
    sim = F.Simulation(W, H, D, steps, acc=8, quiet=1, dump_every=0)
    if nranks > 1:
        sim.comm_init(rank, nranks, open(idfile, "rb").read())
    Dl, zoff = sim.local_depth, sim.z_offset
    # a ball around the middle of the depth: it straddles the boundary of 2 slabs and reaches into all of 3 and 4
    z, y, x = np.mgrid[0:D + 2, 0:H + 2, 0:W + 2]
    m = ((x - W / 3.0) ** 2 + (y - H / 2.0) ** 2 + (z - (D / 2.0 + 0.5)) ** 2) <= (6.0 * D / 32.0) ** 2
    m[0] = m[-1] = False
    m[:, 0] = m[:, -1] = False
    m[:, :, 0] = m[:, :, -1] = False
    sim.set_mask(m[zoff:zoff + Dl + 2])
    out = {"zoff": np.array(zoff)}
    for k in range(steps):
        sim.run_one()
        if k == steps // 2:
            out["mid_q"] = sim.vortex(F.VORTEX_Q)          # a fetch between steps must not disturb the run
    # a host-side edit on both sides of every slab boundary (every rank issues the same calls): the fetch that follows
    # must see the neighbour's edited plane
    for zb in range(1, D + 1):
        sim.setVelocity(6, 5, zb, 1.5 + zb, -0.5, 2.0 - zb)
    for which, name in enumerate(F.VORTEX_NAMES):
        out[name] = sim.vortex(which)
    out["q_f32"] = sim.vortex(F.VORTEX_Q, dtype=np.float32)
    for f, name in ((F.VX, "vx"), (F.VY, "vy"), (F.VZ, "vz"), (F.OBS, "obs")):
        out[name] = sim.get(f)
    dump = os.path.join(outdir, "vortex")
    if rank == 0:
        os.makedirs(dump, exist_ok=True)
    sim.vortex_dump(dump)            # collective: rank 0's directory exists before any other rank opens a file
    np.savez(os.path.join(outdir, "rank%d.npz" % rank), **out)
    sim.close()


if __name__ == "__main__":
    main()
