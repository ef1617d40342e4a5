"""Every form of the semi-Lagrangian advection kernels under rough flows, bit for bit against the CPU oracle.

csrc/advect.hip holds the advection in four forms (option advect_kernels) plus the kernel that fuses the first
projection's gradient into the velocity advection; DESIGN.md section 4 calls them bit-identical.  Which branch of a form a
back-trace takes depends on where it ends, and the tunnel's own start reaches few of them (tests/test_gpu_edge.py,
test_advection_row_kernels_match_cell_kernels_and_oracle).  The flow here is the seeded recipe of tests/advect_model.py;
its numpy classifier counts, per grid and window radius R, the fluid cells whose trace falls in each class, and a test
asserts those counts against the floor of 100 before it compares a single field, so a passing run has been through every
branch.  tests/test_advect_model_cpu.py asserts the same numbers without a GPU.

  class     the trace                                  branch it reaches
  lo_in     px == 0.5, corner rows / planes inside     back_trace_tab `lo`, side 0 of the tables (celltab, row); the staged
            the tile's window of radius R              LDS window of advect_tile_kernel
  lo_out    px == 0.5, a corner outside the window     advect_tile_kernel's fallback to back_trace_tab and the global table
  hi        px == W + 0.5                              back_trace_tab `hi`: side 1 of the tables (advect_columns_kernel)
  mid       no clamp in x                              the gather from the big array, in every form
  mid_int   mid with px integral                       tx == 0 exactly
  ylo..zhi  py == 0.5, H + 0.5, pz == 0.5, D + 0.5     rows 0 / H of the window and the tables, planes 0 / D
  corners   lo_ylo, hi_yhi, lo_zhi, hi_zlo             an x clamp with a y or z clamp: table rows 0 / H + 1, planes 0 / D + 1

Counts of the per-pass advections (seed 7, prev = the velocity itself; fp32 but for 12x80x11, fp64), R the radius the tile
form really runs at for advect_window = 1, 4, 24, 128 (advect_model.tile_window: one staged table; 59 / 40 cover the whole
table of the first two grids, so lo_out is empty there and no floor is asked):

  grid        fluid    R   lo_in  lo_out      hi     mid  mid_int  ylo / yhi / zlo / zhi          corners
  70x33x21    47068    1    6060    5884   11936   23188    11846   5110 / 5001 / 5347 / 5179     1289 1262 1267 1382
                       4    7638    4306
                      24   11784     160
  12x80x11    10259    1    1357    1495    2825    4582     2545   1078 / 1030 / 1265 / 1275      305  277  339  336
                      21    2331     521
                      24    2401     451
  256x9x70   156513    1   21667   17662   39194   77990    39054  20271 / 20511 / 15988 / 16014  5029 5138 4032 4010
                      24   34125    5204
                      32   36321    3008

The first whole step, traces of all three sources of the velocity advection (carried by v_x_prev and the projected v_y,
v_z; by the advected v_x, v_y_prev and the projected v_z; by the advected v_x, v_y and v_z_prev), R for three staged tables
(fp32: 1, 4, 24, 32; fp64: 1, 4, 21, 21); lo_out per source in brackets:

  70x33x21    R = 1: lo_in 22142 lo_out 16722 (5400 6299 5023)   4: 28779 / 10085 (3251 4178 2656)   24: 38648 / 216 (42 174 0)
  12x80x11    R = 1: 4947 / 4845 (2014 1343 1488)   21: 8916 / 876 (352 474 50)   24: 9063 / 729 (285 413 31)
  256x9x70    R = 1: 65139 / 64895 (19143 26225 19527)   24: 121033 / 9001 (1275 1692 6034)   32: 125467 / 4567 (412 577 3578)
  every other class holds at least 490 traces (hi_yhi on 12x80x11).

5x3x2 (30 fluid cells, the tile is larger than the grid) is exempt from the floor: hi > 0, lo_in > 0, lo_out == 0.

Every number above comes from the numpy model, every expected field from the oracle (solver JACOBI, at the field
precision), every expected window radius from the restated tile_window().  The bound is bit equality on all eleven fields,
ghost cells included."""
import os
import subprocess
import sys

import numpy as np
import pytest

import advect_model as M
from conftest import ROOT, bits_equal

pytestmark = pytest.mark.gpu
WORKER = os.path.join(ROOT, "tests", "advect_slab_worker.py")
ACC = 4
GRIDS = [((70, 33, 21), "fp32"), ((70, 33, 21), "fp64"), ((12, 80, 11), "fp64"), ((12, 80, 11), "fp32"), ((256, 9, 70), "fp32"),
         (M.TINY, "fp32"), (M.TINY, "fp64")]
FORMS = [("cell", None), ("celltab", None), ("row", None)] + [("tile", w) for w in M.WINDOWS]
OFF = {"fuse_project_advect": "0"}


@pytest.fixture(scope="module")
def F():
    import fluid_simulation_amd as F
    return F


def handle(F, shape, precision, kernels, window=None, **kw):
    if window is not None:
        kw["advect_window"] = window
    return F.Simulation(*shape, 1, acc=ACC, quiet=1, precision=precision, advect_kernels=kernels, **kw)


def oracle(O, shape, precision):
    return O.Oracle(*shape, solver=O.JACOBI, fp64=precision == "fp64", acc=ACC)


def same_state(F, sim, want, what):
    for f in range(11):
        assert bits_equal(sim.get(f), want[f]), "%s: %s" % (what, F.FIELD_NAMES[f])


def state_of(x):
    return [x.get(f) for f in range(11)]


def passes(F):
    return ((0, F.DENS, F.BUFFER), (1, F.VX, F.VX_PREV), (2, F.VY, F.VY_PREV), (3, F.VZ, F.VZ_PREV))


def run_pass(F, x, b, field, prev, ux, uy, uz, src):
    for f, a in ((F.VX, ux), (F.VY, uy), (F.VZ, uz)):
        x.set(f, a)
    x.set(prev, src if b == 0 else (ux, uy, uz)[b - 1])
    x.advect(b, field, prev)


def start(F, x, ux, uy, uz, src):
    for f, a in ((F.VX, ux), (F.VY, uy), (F.VZ, uz), (F.DENS, np.abs(src))):
        x.set(f, a)


def check_floors(shape, dtype, nf, count, what):
    """the class floors at every radius the tile form runs at with `nf` staged tables, where the grid lists that radius"""
    radii = sorted({M.tile_window(w, nf, np.dtype(dtype).itemsize) for w in M.WINDOWS})
    if shape == M.TINY:
        M.assert_tiny(count(1), what)
        return
    held = [R for R in radii if R in M.FLOOR_R[shape]]
    assert len(held) >= 2, (shape, radii)
    for R in held:
        c = count(R)
        print(what, "R", R, c)
        M.assert_floors(c, "%s R %d" % (what, R))


@pytest.mark.parametrize("shape,precision", GRIDS)
def test_per_pass_every_form(F, oracle_mod, shape, precision):
    """advect(b, field, prev) for b = 0..3 on one handle per form, from the rough state: the written field equals the
    oracle's and no other field moved."""
    O = oracle_mod
    W, H, D = shape
    dtype = np.float64 if precision == "fp64" else np.float32
    ux, uy, uz, src = M.rough_fields(W, H, D, M.SEED, dtype)
    mask = M.rough_mask(W, H, D, M.SEED)
    check_floors(shape, dtype, 1, lambda R: M.classify(W, H, D, ux, uy, uz, mask, R, dtype), "%s %s per pass" % (shape, precision))
    sims = [("%s window %s" % form, handle(F, shape, precision, *form)) for form in FORMS]
    ora = oracle(O, shape, precision)
    for _, x in sims + [("", ora)]:
        x.set_mask(mask)
    for b, field, prev in passes(F):
        run_pass(F, ora, b, field, prev, ux, uy, uz, src)
        want = state_of(ora)
        assert np.isfinite(want[field]).all() and np.abs(want[field]).max() > 0.5
        for name, sim in sims:
            run_pass(F, sim, b, field, prev, ux, uy, uz, src)
            same_state(F, sim, want, "%s %s b = %d, %s" % (shape, precision, b, name))
    for _, sim in sims:
        sim.close()


@pytest.mark.parametrize("shape,precision", GRIDS)
def test_whole_steps_fused_and_unfused(F, oracle_mod, shape, precision):
    """Three steps from the rough state: every form with the three velocity advections in one kernel and as three launches
    (the projection's gradient pass kept apart), and the per-cell form with the gradient pass inside the advection
    kernel, against the oracle after every step."""
    O = oracle_mod
    W, H, D = shape
    steps = 3
    dtype = np.float64 if precision == "fp64" else np.float32
    ux, uy, uz, src = M.rough_fields(W, H, D, M.SEED, dtype)
    mask = M.rough_mask(W, H, D, M.SEED)
    rep = oracle(O, shape, precision)
    carriers = M.step_carriers(rep, ux, uy, uz, mask)
    rep.close()
    check_floors(shape, dtype, 3, lambda R: M.classify_step(W, H, D, carriers, mask, R, dtype)[0],
                 "%s %s step 1" % (shape, precision))
    sims = [("%s window %s fuse_advect %d" % (form + (fuse,)), handle(F, shape, precision, *form, fuse_advect=fuse, **OFF))
            for form in FORMS for fuse in (0, 1)]
    # step(): the gradient pass runs inside the advection kernel where the option is on, on one GPU, under Jacobi with acc > 0,
    # with fuse_advect on and advect_kernels=cell -- no term depends on the grid, so every step of this handle takes it
    fused = handle(F, shape, precision, "cell", fuse_project_advect=1, zero_start=1)
    ora = oracle(O, shape, precision)
    for _, x in sims + [("", fused), ("", ora)]:
        x.set_mask(mask)
        start(F, x, ux, uy, uz, src)
    for step in range(steps):
        ora.run_one()
        want = state_of(ora)
        assert all(np.isfinite(a).all() for a in want) and np.abs(want[F.VY]).max() > 1.0
        for name, sim in sims + [("cell, gradient pass inside the advection", fused)]:
            sim.run_one()
            same_state(F, sim, want, "%s %s step %d, %s" % (shape, precision, step + 1, name))
    for _, sim in sims:
        assert sim._geti("project_advect_steps") == 0
        sim.close()
    assert fused._geti("project_advect_steps") == steps
    fused.close()


@pytest.mark.parametrize("shape,precision", [((70, 33, 21), "fp32"), ((12, 80, 11), "fp64")])
def test_outlet_side_alone(F, oracle_mod, shape, precision):
    """u_x = -2 / dt everywhere: every fluid trace clamps at the outlet side and reads side 1 of the clamp tables."""
    O = oracle_mod
    W, H, D = shape
    dtype = np.float64 if precision == "fp64" else np.float32
    ux, uy, uz, src = M.rough_fields(W, H, D, M.SEED, dtype)
    ux[~M.box_edges(W, H, D)] = -2 / M.DT                  # (the edges of the box stay 0, see rough_fields)
    mask = M.rough_mask(W, H, D, M.SEED)
    c = M.classify(W, H, D, ux, uy, uz, mask, 1, dtype)
    assert c["hi"] == c["fluid"] > 0 and c["hi_yhi"] >= M.FLOOR and c["hi_zlo"] >= M.FLOOR
    sims = [("%s window %s" % form, handle(F, shape, precision, *form)) for form in (("celltab", None), ("row", None), ("tile", 1), ("tile", 24))]
    ora = oracle(O, shape, precision)
    for _, x in sims + [("", ora)]:
        x.set_mask(mask)
    for b, field, prev in passes(F):
        run_pass(F, ora, b, field, prev, ux, uy, uz, src)
        want = state_of(ora)
        assert np.abs(want[field]).max() > 0.5
        for name, sim in sims:
            run_pass(F, sim, b, field, prev, ux, uy, uz, src)
            same_state(F, sim, want, "outlet only, %s %s b = %d, %s" % (shape, precision, b, name))
    for _, x in sims + [("", ora)]:
        start(F, x, ux, uy, uz, src)
    for step in range(2):
        ora.run_one()
        want = state_of(ora)
        for name, sim in sims:
            sim.run_one()
            same_state(F, sim, want, "outlet only, %s %s step %d, %s" % (shape, precision, step + 1, name))
    for _, sim in sims:
        sim.close()


def test_window_cap(F, oracle_mod):
    """12x80x11 fp64: advect_window = 24 and 128 run at the radius the 64 KB of LDS leave -- 21 both with three staged
    tables, 24 and 40 with one -- and traces still leave every one of those windows; the bits are those of the per-cell
    form, per pass and over whole steps."""
    O = oracle_mod
    shape, precision, dtype = (12, 80, 11), "fp64", np.float64
    W, H, D = shape
    assert [M.tile_window(w, 3, 8) for w in (24, 128)] == [21, 21] and [M.tile_window(w, 1, 8) for w in (24, 128)] == [24, 40]
    ux, uy, uz, src = M.rough_fields(W, H, D, M.SEED, dtype)
    mask = M.rough_mask(W, H, D, M.SEED)
    for R in (21, 24, 40):
        c = M.classify(W, H, D, ux, uy, uz, mask, R, dtype)
        assert c["lo_out"] >= M.FLOOR and c["lo_in"] >= M.FLOOR, (R, c)
    sims = [handle(F, shape, precision, "cell", **OFF), handle(F, shape, precision, "tile", 24), handle(F, shape, precision, "tile", 128)]
    ora = oracle(O, shape, precision)
    for x in sims + [ora]:
        x.set_mask(mask)
    for b, field, prev in passes(F):
        for x in sims + [ora]:
            run_pass(F, x, b, field, prev, ux, uy, uz, src)
        want = state_of(sims[0])
        same_state(F, ora, want, "b = %d, cell against the oracle" % b)
        for w, sim in zip((24, 128), sims[1:]):
            same_state(F, sim, want, "b = %d, advect_window %d against cell" % (b, w))
    for x in sims + [ora]:
        start(F, x, ux, uy, uz, src)
    for step in range(3):
        for x in sims + [ora]:
            x.run_one()
        want = state_of(sims[0])
        same_state(F, ora, want, "step %d, cell against the oracle" % (step + 1))
        for w, sim in zip((24, 128), sims[1:]):
            same_state(F, sim, want, "step %d, advect_window %d against cell" % (step + 1, w))
    for sim in sims:
        sim.close()


# ---- z-slabs ----------------------------------------------------------------------------------------------------------------

SLAB = (20, 12, 32)
SLAB_STEPS = 2
_SLAB_REF = {}


def run_ranks(tmp, nranks, transport, kernels):
    import fluid_simulation_amd as F
    out = os.path.join(tmp, "%s_%s_n%d" % (transport, kernels, nranks))
    os.makedirs(out)
    idfile = os.path.join(out, "id.bin")
    if nranks > 1:
        open(idfile, "wb").write(F.comm_unique_id(transport))
    procs = [subprocess.Popen([sys.executable, WORKER, str(r), str(nranks), idfile, out] + [str(v) for v in SLAB] +
                              ["fp32", kernels, str(SLAB_STEPS)], env=dict(os.environ, FS_IPC_TIMEOUT_S="60"))
             for r in range(nranks)]
    try:
        for p in procs:
            assert p.wait(timeout=300) == 0
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
    return [dict(np.load(os.path.join(out, "rank%d.npz" % r))) for r in range(nranks)]


def slab_reference(F, O, tmp):
    """the one-GPU run of the same worker, held to the oracle"""
    if "ref" in _SLAB_REF:
        return _SLAB_REF["ref"]
    W, H, D = SLAB
    (ref,) = run_ranks(tmp, 1, "single", "cell")
    ux, uy, uz, src = M.rough_fields(W, H, D, M.SEED, np.float32)
    ora = oracle(O, SLAB, "fp32")
    ora.set_mask(M.rough_mask(W, H, D, M.SEED))
    for b, field, prev in passes(F):
        run_pass(F, ora, b, field, prev, ux, uy, uz, src)
        assert bits_equal(ref["pass%d" % b], ora.get(field)), "one GPU against the oracle, b = %d" % b
    start(F, ora, ux, uy, uz, src)
    for k in range(SLAB_STEPS):
        ora.run_one()
        for f in (F.DENS, F.VX, F.VY, F.VZ, F.PRESSURE):
            key = "step%d_%s" % (k + 1, F.FIELD_NAMES[f])
            assert bits_equal(ref[key], ora.get(f)), "one GPU against the oracle, " + key
    ora.close()
    _SLAB_REF["ref"] = ref
    return ref


def model_reach(vz, D):
    """reach_of() of fluidsim.cpp for the largest |u_z| of the interior cells: ceil(dt D max|u_z|) + 2 planes, at most D"""
    planes = np.ceil(abs(float(np.float32(M.DT)) * D) * float(np.abs(vz[1:-1, 1:-1, 1:-1]).max())) + 2.0
    return D if planes >= D else int(planes)


@pytest.mark.parametrize("nranks,kernels,transport", [(2, "cell", "shm"), (2, "row", "shm"), (2, "tile", "shm"), (4, "cell", "shm"),
                                                      (2, "row", "ipc"), (4, "cell", "ipc")])
def test_slabs_under_the_rough_flow(F, oracle_mod, tmp_path, nranks, kernels, transport):
    """2 and 4 z-slab ranks on 20x12x32: |dt D u_z| reaches several D, so the traces of every slab end in every other
    slab, in both directions, and the gathered source must span the whole depth (the gather buffer is poisoned first).
    On slabs the clamp tables are dropped: `row` runs back_trace_tab without a table against the gathered array, `tile`
    falls through to the per-cell kernels."""
    if transport == "ipc":
        from test_gpu_slabs import ipc_usable
        ok, why = ipc_usable()
        if not ok:
            pytest.skip("FSIPC transport not usable on this box: " + why)
    W, H, D = SLAB
    ref = slab_reference(F, oracle_mod, str(tmp_path))
    uz = M.rough_fields(W, H, D, M.SEED, np.float32)[2]
    keys = ["pass%d" % b for b in range(4)] + ["step%d_%s" % (k + 1, F.FIELD_NAMES[f]) for k in range(SLAB_STEPS)
                                               for f in (F.DENS, F.VX, F.VY, F.VZ, F.PRESSURE)]
    # what each advection needs: the per-pass ones are carried by u_z, a step's last one (the density) by its final v_z
    need = [model_reach(uz, D)] * 4 + [model_reach(ref["step%d_v_z" % (k + 1)], D) for k in range(SLAB_STEPS)]
    assert need[:5] == [D] * 5                             # the rough state and the first step ask for the whole depth
    ranks = run_ranks(str(tmp_path), nranks, transport, kernels)
    Dl = D // nranks
    for r, z in enumerate(ranks):
        zoff = int(z["zoff"])
        assert zoff == r * Dl and int(z["Dl"]) == Dl
        lo = 0 if r == 0 else 1                            # the planes a rank owns, and the physical ghost planes it holds
        hi = Dl + 1 if r == nranks - 1 else Dl
        for k in keys:
            assert z[k].shape == (Dl + 2, H + 2, W + 2)
            assert bits_equal(z[k][lo:hi + 1], ref[k][zoff + lo:zoff + hi + 1]), (r, k)
        # the kernel's own maximum also sees ghost cells: never less than the interior asks for, the whole depth where it does
        got = [int(v) for v in z["reach"]]
        assert all(n <= g <= D for n, g in zip(need, got)), (r, got, need)
