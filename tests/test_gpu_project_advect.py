"""Option "fuse_project_advect": on one GPU the gradient pass of a step's first projection runs inside the kernel of the
three velocity advections (the projected velocities never reach memory).  Nothing may change: one handle runs with
fuse_project_advect = 0 and zero_start = 0 (the launches as they were), another with both at 1, from the same start, and
the fields are compared bit for bit after every step.  fs_get_int "project_advect_steps" says which path a step took."""
import os

import numpy as np
import pytest

from conftest import GOLDEN, ball_mask, bits_equal, rel_l2
from test_gpu_slabs import run_ranks

pytestmark = pytest.mark.gpu

GRIDS = [(256, 20, 10), (512, 28, 13), (70, 18, 9)]
STEPS = 4
OFF = {"fuse_project_advect": "0", "zero_start": "0"}
ON = {"fuse_project_advect": "1", "zero_start": "1"}


@pytest.fixture(scope="module")
def F():
    import fluid_simulation_amd as F
    return F


def _mask(W, H, D):
    m = ball_mask(W, H, D, W / 3.0, H / 2.0, D / 2.0, min(H, D) / 4.0)
    m[D // 2, 1:H // 2, 2 * W // 3:2 * W // 3 + 9] = True       # a plate on the y = 1 wall
    m[2, H - 1, W] = m[D - 1, 2, 1] = True                       # single cells in the last / first column
    return m


def _run(F, W, H, D, opts, precision="fp32", rough=True, acc=5, solver="jacobi", steps=STEPS, **more):
    """Returns (fields after every step, the handle).  rough: random velocities of order one (dt W |u| is a dozen cells, so
    the traces do not all clamp to the inlet column); else the tunnel's own start."""
    sim = F.Simulation(W, H, D, steps, acc=acc, quiet=1, precision=precision, solver=solver, **opts, **more)
    sim.set_mask(_mask(W, H, D))
    if rough:
        rng = np.random.default_rng(W + 7 * H)
        for f in (F.VX, F.VY, F.VZ):
            sim.set(f, rng.standard_normal((D + 2, H + 2, W + 2)).astype(sim.dtype))
        sim.set(F.DENS, rng.random((D + 2, H + 2, W + 2)).astype(sim.dtype))
    out = []
    for _ in range(steps):
        sim.run_one()
        out.append([sim.get(f) for f in (F.DENS, F.VX, F.VY, F.VZ, F.PRESSURE, F.DIVERGENCE)])
    return out, sim


def _same(F, a, b, what):
    names = ("dens", "v_x", "v_y", "v_z", "pressure", "divergence")
    for k, (sa, sb) in enumerate(zip(a, b)):
        for n, x, y in zip(names, sa, sb):
            assert x.tobytes() == y.tobytes(), "%s: step %d %s" % (what, k + 1, n)


@pytest.mark.parametrize("rough", [True, False])
@pytest.mark.parametrize("precision", ["fp32", "fp64"])
@pytest.mark.parametrize("W,H,D", GRIDS)
def test_steps_are_bit_identical(F, W, H, D, precision, rough):
    a, sa = _run(F, W, H, D, OFF, precision, rough)
    b, sb = _run(F, W, H, D, ON, precision, rough)
    _same(F, a, b, "%dx%dx%d %s rough=%s" % (W, H, D, precision, rough))
    assert sa._geti("project_advect_steps") == 0 and sb._geti("project_advect_steps") == STEPS
    assert np.abs(b[-1][1]).max() > 0 and np.isfinite(b[-1][1]).all()
    sa.close()
    sb.close()


@pytest.mark.parametrize("W,H,D", GRIDS[:2])
def test_force_log_records_are_the_same(F, W, H, D):
    a, sa = _run(F, W, H, D, OFF, force_log=STEPS)
    b, sb = _run(F, W, H, D, ON, force_log=STEPS)
    _same(F, a, b, "force_log")
    la, lb = sa.force_log(), sb.force_log()
    assert len(la) == STEPS and la.tobytes() == lb.tobytes()
    assert np.abs(la["s1x"]).max() > 0                               # the records are not empty
    assert sb._geti("project_advect_steps") == STEPS
    sa.close()
    sb.close()


@pytest.mark.parametrize("W,H,D", GRIDS[:2])
def test_with_the_dead_density_solve_elided(F, W, H, D):
    a, sa = _run(F, W, H, D, OFF, elide_dead_density_solve="1")
    b, sb = _run(F, W, H, D, ON, elide_dead_density_solve="1")
    _same(F, a, b, "elide_dead_density_solve")
    assert sb._geti("project_advect_steps") == STEPS
    sa.close()
    sb.close()


@pytest.mark.parametrize("solver,acc", [("gs_lex", 5), ("jacobi", 0)])
@pytest.mark.parametrize("W,H,D", [GRIDS[0], GRIDS[2]])
def test_in_place_solver_and_acc_zero_take_the_fallback(F, W, H, D, solver, acc):
    a, sa = _run(F, W, H, D, OFF, acc=acc, solver=solver)
    b, sb = _run(F, W, H, D, ON, acc=acc, solver=solver)
    _same(F, a, b, "%s acc %d" % (solver, acc))
    assert sb._geti("project_advect_steps") == 0 and sb._geti("zero_start_projections") == 0
    sa.close()
    sb.close()


def test_slabs_keep_their_launches(tmp_path):
    """Two z-slab ranks over the shared-memory development transport, with the options at 1 and at 0: the same bits, and
    the same as one GPU with the options at 0."""
    W, H, D, acc, steps = 20, 12, 32, 5, 2
    stl = os.path.join(GOLDEN, "sphere_24x12.stl")
    off, on = "fuse_project_advect=0,zero_start=0", "fuse_project_advect=1,zero_start=1"
    ref = np.load(os.path.join(run_ranks(str(tmp_path / "ref"), 1, [W, H, D, acc, steps, stl, "fp32", "jacobi", off]), "rank0.npz"))
    dirs = [run_ranks(str(tmp_path / k), 2, [W, H, D, acc, steps, stl, "fp32", "jacobi", o]) for k, o in (("off", off), ("on", on))]
    for r in range(2):
        za, zb = (np.load(os.path.join(d, "rank%d.npz" % r)) for d in dirs)
        zoff, Dl = int(zb["zoff"]), D // 2
        for k in ("dens", "v_x", "v_y", "v_z", "pressure"):
            assert za[k].tobytes() == zb[k].tobytes(), (r, k)
            lo, hi = (0 if r == 0 else 1), (Dl + 2 if r == 1 else Dl + 1)
            assert zb[k][lo:hi].tobytes() == ref[k][zoff:zoff + Dl + 2][lo:hi].tobytes(), (r, k, "single GPU")


def test_against_the_cpu_oracle(F, oracle_mod):
    """64x24x20, acc = 7, three steps against the CPU restatement, held to what tests/test_gpu_parity.py holds a Jacobi run
    to: relative L2 within 1e-5 and bit-exact."""
    O = oracle_mod
    W, H, D, acc, steps = 64, 24, 20, 7, 3
    m = ball_mask(W, H, D, W / 3.0, H / 2.0, D / 2.0, 4.0)
    sim = F.Simulation(W, H, D, steps, acc=acc, solver="jacobi", quiet=1, **ON)
    ora = O.Oracle(W, H, D, solver=O.JACOBI, iter=steps, acc=acc)
    sim.set_mask(m)
    ora.set_mask(m)
    for s in range(steps):
        sim.run_one()
        ora.run_one()
        for f in range(11):
            got, want = sim.get(f), ora.get(f)
            r = rel_l2(got, want)
            assert r <= 1e-5, "step %d %s: relL2 %.3e" % (s + 1, F.FIELD_NAMES[f], r)
            assert bits_equal(np.asarray(got, dtype=want.dtype), want), "step %d %s: not bit-exact" % (s + 1, F.FIELD_NAMES[f])
    assert sim._geti("project_advect_steps") == steps
    sim.close()
