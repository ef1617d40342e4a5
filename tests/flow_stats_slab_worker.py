"""One rank of a z-slab run with the time-averaged flow statistics on (spawned by tests/test_gpu_flow_stats.py).
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
    sim = F.Simulation(W, H, D, steps, acc=8, quiet=1, dump_every=0, flow_stats="moments")
    if nranks > 1:
        sim.comm_init(rank, nranks, open(idfile, "rb").read())
    Dl, zoff = sim.local_depth, sim.z_offset
    # a ball around the middle of the depth: it straddles the boundary of 2 slabs and reaches into all of 4
    z, y, x = np.mgrid[0:D + 2, 0:H + 2, 0:W + 2]
    m = ((x - W / 3.0) ** 2 + (y - H / 2.0) ** 2 + (z - (D / 2.0 + 0.5)) ** 2) <= (6.0 * D / 32.0) ** 2
    m[0] = m[-1] = False
    m[:, 0] = m[:, -1] = False
    m[:, :, 0] = m[:, :, -1] = False
    sim.set_mask(m[zoff:zoff + Dl + 2])
    for k in range(steps):
        if k == steps // 2:
            # a host-side edit on both sides of a slab boundary (every rank issues the same calls)
            for zb in (D // 2, D // 2 + 1, max(1, D // 4)):
                sim.setVelocity(6, 5, zb, 1.5, -0.5, 2.0)
        sim.run_one()
    out = {"samples": np.array(sim.flow_stats_samples), "zoff": np.array(zoff)}
    for which, name in enumerate(F.STAT_NAMES):
        out[name] = sim.flow_stats(which)
        if which != F.STAT_TKE:
            out["raw_" + name] = sim.flow_stats(which, raw=True)
    out["tke_f32"] = sim.flow_stats(F.STAT_TKE, dtype=np.float32)
    out["stream_syncs"] = np.array(sim._geti("stream_syncs"))
    dump = os.path.join(outdir, "mean")
    if rank == 0:
        os.makedirs(dump, exist_ok=True)
    sim.flow_stats_dump(dump)        # collective: rank 0's directory exists before any other rank opens a file
    np.savez(os.path.join(outdir, "rank%d.npz" % rank), **out)
    sim.close()


if __name__ == "__main__":
    main()
