"""The three-sweep kernel on lane-aligned fp32 rows (W = 256, 512) takes the x neighbours of a lane's cells from the
lanes beside it and only the cell beyond either end of a wave from memory or the LDS tile.  Wherever those cells
differ from the plain reading -- solids at x = 1 and x = W, at the two cells either side of a wave boundary (x = 256,
257 on 512-cell rows), one-plane-thin plates, obstacles near the z walls and in the rows two bands share -- a whole
step (boundary codes b = 0..3) must stay the oracle's Jacobi bit for bit."""
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import GOLDEN, ball_mask, bits_equal

pytestmark = pytest.mark.gpu

WORKER = os.path.join(os.path.dirname(os.path.abspath(__file__)), "slab_worker.py")


@pytest.fixture(scope="module")
def F():
    import fluid_simulation_amd as F
    return F


def _mask(kind, W, H, D):
    m = np.zeros((D + 2, H + 2, W + 2), dtype=bool)
    if kind == "x_walls":                       # solids against both ghost columns, in every row of a few planes
        m[2:D - 1, 1:H + 1, 1] = True
        m[3:D, 2:H, W] = True
        m[D // 2, :, 1:3] = True
    elif kind == "wave_seam":                   # the cells either side of the 256-cell wave boundary, and a lone cell on it
        m[2:D, 3:H - 2, 255:259] = True
        m[1, 1, 256] = m[D, H, 257] = True
        m[D // 2, H // 2, 254] = True
    elif kind == "thin_plate":                  # one plane thick, starting and ending inside a group of iterations
        m[D // 2, 2:H - 1, W // 4:3 * W // 4] = True
        m[D // 2 + 3, 1:H + 1, 1:W + 1:7] = True
    elif kind == "z_walls":                     # against the ghost planes z = 0 and D+1 (the general body's groups)
        m[1, 2:H - 1, 10:W - 10] = True
        m[D, 1:H, 1:W:3] = True
        m[2, H // 2, W - 1] = True
    elif kind == "band_overlap":                # rows 7..10: where the 12-row bands (8 productive) overlap
        m[3:D - 2, 7:11, W // 3:W // 3 + 40] = True
        m[5, 8, 1] = m[6, 9, W] = True
    elif kind == "ball":
        m = ball_mask(W, H, D, W / 3.0, H / 2.0, D / 2.0, min(H, D) / 3.0)
        m[1, 1, 1] = m[D, H, W] = True
    return m


KINDS = ["x_walls", "thin_plate", "z_walls", "band_overlap", "ball"]
CASES = [(512, 21, 26, k) for k in KINDS + ["wave_seam"]] + [(256, 30, 19, k) for k in KINDS]   # one wave per row at W = 256


@pytest.mark.parametrize("W,H,D,kind", CASES)
def test_three_sweeps_on_aligned_rows_match_oracle(F, oracle_mod, W, H, D, kind):
    O = oracle_mod
    acc = 9                                      # three passes of three sweeps per solve
    sim = F.Simulation(W, H, D, 1, acc=acc, quiet=1)
    sim.set_option("sweep_fuse", "4")            # three sweeps per pass wherever the kernel exists
    ora = O.Oracle(W, H, D, solver=O.JACOBI, threads=4, acc=acc)
    m = _mask(kind, W, H, D)
    sim.set_mask(m)
    ora.set_mask(m)
    for _ in range(2):
        sim.run_one()
        ora.run_one()
    for f in range(11):
        assert bits_equal(sim.get(f), ora.get(f)), "%s %dx%dx%d: %s" % (kind, W, H, D, F.FIELD_NAMES[f])
    sim.close()


@pytest.mark.parametrize("W", [256, 512])
def test_three_sweeps_on_aligned_rows_with_z_chunks(F, W):
    """Short z chunks (pair_zc): many chunk boundaries inside the obstacle, against the single-sweep kernels."""
    H, D = 17, 40
    out = []
    for fuse in ("4", "1"):
        sim = F.Simulation(W, H, D, 1, acc=6, quiet=1)
        sim.set_option("sweep_fuse", fuse)
        if fuse == "4":
            sim.set_option("pair_zc", 5)
        m = _mask("ball", W, H, D)
        m[10:16, 1:H + 1, W // 2 - 1:W // 2 + 2] = True
        sim.set_mask(m)
        sim.run_one()
        sim.run_one()
        out.append([sim.get(f) for f in range(11)])
        sim.close()
    for f in range(11):
        assert bits_equal(out[0][f], out[1][f]), "W=%d %s" % (W, F.FIELD_NAMES[f])


def _run_ranks(tmp, nranks, args):
    out = os.path.join(tmp, "n%d" % nranks)
    os.makedirs(os.path.join(out, "data"))
    idfile = os.path.join(out, "id.bin")
    if nranks > 1:
        import fluid_simulation_amd as F
        open(idfile, "wb").write(F.comm_unique_id("shm"))
    procs = [subprocess.Popen([sys.executable, WORKER, str(r), str(nranks), idfile, out] + [str(a) for a in args],
                              env=dict(os.environ, FS_IPC_TIMEOUT_S="60")) for r in range(nranks)]
    for p in procs:
        assert p.wait(timeout=600) == 0
    return out


def test_three_sweeps_on_aligned_rows_two_slabs(tmp_path):
    """Two z-slabs of 512-cell rows (the SLAB build of the three-sweep kernel) against one GPU."""
    W, H, D, nranks = 512, 14, 32, 2
    args = [W, H, D, 9, 2, os.path.join(GOLDEN, "plate_ascii.stl"), "fp32", "jacobi", ""]
    ref = np.load(os.path.join(_run_ranks(str(tmp_path), 1, args), "rank0.npz"))
    par_dir = _run_ranks(str(tmp_path), nranks, args)
    Dl = D // nranks
    for r in range(nranks):
        z = np.load(os.path.join(par_dir, "rank%d.npz" % r))
        zoff = int(z["zoff"])
        assert int(z["kernels"][0]) >= 0             # the three-sweep kernel ran
        for k in ("dens", "v_x", "v_y", "v_z", "obs"):
            assert np.array_equal(z[k].view(np.uint32), ref[k][zoff:zoff + Dl + 2].view(np.uint32)), (r, k)
