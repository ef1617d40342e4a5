"""One rank of a z-slab run of the advection under the rough flow of tests/advect_model.py (spawned by
tests/test_gpu_advect_rough.py).  argv: rank nranks idfile outdir W H D precision advect_kernels steps"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import fluid_simulation_amd as F  # noqa: E402

import advect_model as M  # noqa: E402

PASSES = ((0, F.DENS, F.BUFFER), (1, F.VX, F.VX_PREV), (2, F.VY, F.VY_PREV), (3, F.VZ, F.VZ_PREV))
STEP_FIELDS = (F.DENS, F.VX, F.VY, F.VZ, F.PRESSURE)


def main():
    rank, nranks = int(sys.argv[1]), int(sys.argv[2])
    idfile, outdir = sys.argv[3], sys.argv[4]
    W, H, D = (int(v) for v in sys.argv[5:8])
    precision, kernels, steps = sys.argv[8], sys.argv[9], int(sys.argv[10])
    sim = F.Simulation(W, H, D, steps, acc=4, quiet=1, dump_every=0, debug_poison_gather=1, precision=precision,
                       advect_kernels=kernels, advect_window=4)
    if nranks > 1:
        sim.comm_init(rank, nranks, open(idfile, "rb").read())
    Dl, zoff = sim.local_depth, sim.z_offset
    # the global state is the same on every rank; a rank keeps its planes (and the neighbours' boundary planes as halos)
    mine = slice(zoff, zoff + Dl + 2)
    ux, uy, uz, src = (a[mine] for a in M.rough_fields(W, H, D, M.SEED, sim.dtype))
    sim.set_mask(M.rough_mask(W, H, D, M.SEED)[mine])
    out = {"zoff": np.array(zoff), "Dl": np.array(Dl)}
    reach = []
    for b, field, prev in PASSES:
        for f, a in ((F.VX, ux), (F.VY, uy), (F.VZ, uz)):
            sim.set(f, a)
        sim.set(prev, src if b == 0 else (ux, uy, uz)[b - 1])
        sim.advect(b, field, prev)
        out["pass%d" % b] = sim.get(field)
        reach.append(sim._geti("last_advect_reach") if nranks > 1 else D)
    for f, a in ((F.VX, ux), (F.VY, uy), (F.VZ, uz), (F.DENS, np.abs(src))):
        sim.set(f, a)
    for k in range(steps):
        sim.run_one()
        for f in STEP_FIELDS:
            out["step%d_%s" % (k + 1, F.FIELD_NAMES[f])] = sim.get(f)
        reach.append(sim._geti("last_advect_reach") if nranks > 1 else D)
    out["reach"] = np.array(reach)
    np.savez(os.path.join(outdir, "rank%d.npz" % rank), **out)
    sim.close()


if __name__ == "__main__":
    main()
