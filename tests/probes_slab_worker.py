"""One rank of a z-slab run with the point-probe log on (spawned by tests/test_gpu_probes.py).
argv: rank nranks idfile outdir W H D steps"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import fluid_simulation_amd as F  # noqa: E402


def probe_cells(W, H, D):
    """Both sides of every boundary of 2, 3 and 4 slabs of a depth that 12 divides, the two z ghost planes, x / y ghost
    cells and corners: the same list whatever the split, so that every run has the same columns."""
    zs = sorted({0, 1, D, D + 1} | {D * k // n + s for n in (2, 3, 4) for k in range(1, n) for s in (0, 1)})
    cells = []
    for k, z in enumerate(zs):
        cells.append((1 + (5 * k) % W, 1 + (3 * k) % H, z))
        cells.append(((0, W + 1, 3, 7)[k % 4], (2, 5, 0, H + 1)[k % 4], z))
    cells += [(0, 0, 0), (W + 1, H + 1, D + 1), (W // 3 + 2, H // 2, D // 2), (W // 3 + 2, H // 2, D // 2 + 1)]
    return np.array(cells, dtype=np.intc)


def main():
    rank, nranks = int(sys.argv[1]), int(sys.argv[2])
    idfile, outdir = sys.argv[3], sys.argv[4]
    W, H, D, steps = (int(v) for v in sys.argv[5:9])
    sim = F.Simulation(W, H, D, steps, acc=8, quiet=1, dump_every=0)
    cells = probe_cells(W, H, D)
    sim.set_probes(cells)                                  # before the partition exists: legal at any time
    if nranks > 1:
        sim.comm_init(rank, nranks, open(idfile, "rb").read())
    sim.set_option("probe_log", steps)
    Dl, zoff = sim.local_depth, sim.z_offset
    z, y, x = np.mgrid[0:D + 2, 0:H + 2, 0:W + 2]
    m = ((x - W / 3.0) ** 2 + (y - H / 2.0) ** 2 + (z - (D / 2.0 + 0.5)) ** 2) <= (6.0 * D / 32.0) ** 2
    m[0] = m[-1] = False
    m[:, 0] = m[:, -1] = False
    m[:, :, 0] = m[:, :, -1] = False
    sim.set_mask(m[zoff:zoff + Dl + 2])
    steps_col, values, direct = [], [], []
    for k in range(steps):
        sim.run_one()
        if nranks == 1:                                    # what the definition says a record holds
            fields = [sim.get(f).astype(np.float64) for f in (F.DENS, F.VX, F.VY, F.VZ, F.PRESSURE)]
            direct.append(np.stack([f[cells[:, 2], cells[:, 1], cells[:, 0]] for f in fields], axis=1))
        if k == steps // 2:                                # a collective drain in the middle of the run
            log = sim.probe_log()
            steps_col.append(log["step"])
            values.append(log["values"])
    sim.probe_sample()                                     # one more record of the final state
    log, dropped = sim.probe_log(with_dropped=True)
    steps_col.append(log["step"])
    values.append(log["values"])
    out = {"step": np.concatenate(steps_col), "values": np.concatenate(values), "dropped": np.array(dropped),
           "count": np.array(sim.probe_count), "vx": sim.get(F.VX), "zoff": np.array(zoff)}
    if nranks == 1:
        out["direct"] = np.stack(direct)
    np.savez(os.path.join(outdir, "rank%d.npz" % rank), **out)
    sim.close()


if __name__ == "__main__":
    main()
