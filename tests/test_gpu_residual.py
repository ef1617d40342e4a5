"""Residual of the linear solves on the MI355X (fs_solve_residual, fs_diffuse_residual, option "residual_log" /
fs_residual_log): integer-valued cases that fix the cell set and the formula of include/fluidsim.h with no tolerance at
all, real-valued fields against a numpy restatement within the bound of a reordered fp64 sum, real solves, the per-step
log against the on-demand query on a handle that replays the step by hand, no effect on the run, the ring, z-slab runs
bit-identical with one GPU, and the CSV of simulation.out."""
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import GOLDEN, ROOT, ball_mask, bits_equal

pytestmark = pytest.mark.gpu
WORKER = os.path.join(ROOT, "tests", "residual_slab_worker.py")
PRECISIONS = ["fp32", "fp64"]
SHAPES = [(13, 7, 5), (33, 16, 12), (64, 48, 40), (130, 9, 6)]
COEFFS = [(1.0, 6.0), (2.0, 13.0), (0.5, 4.0)]
U = 2.0 ** -53


def sim_of(W, H, D, precision="fp32", **kw):
    import fluid_simulation_amd as F
    kw.setdefault("quiet", 1)
    kw.setdefault("dump_every", 0)
    return F.Simulation(W, H, D, 1, precision=precision, **kw)


def restate(x, x0, obs, a, c, b):
    """numpy fp64 restatement of the definition in include/fluidsim.h: per z-plane {sum r^2, sum x0^2, max |r|, free
    cells}, and the free-cell mask.  r is evaluated in the header's order, so it carries the kernel's bits; the sums are
    numpy's (pairwise), another order."""
    D, H, W = (n - 2 for n in obs.shape)
    q = np.asarray(x, dtype=np.float64)
    rhs = np.asarray(x0, dtype=np.float64)[1:-1, 1:-1, 1:-1]
    a, c = np.float64(a), np.float64(c)
    nb = ((((q[1:-1, 1:-1, 2:] + q[1:-1, 1:-1, :-2]) + q[1:-1, 2:, 1:-1]) + q[1:-1, :-2, 1:-1]) + q[2:, 1:-1, 1:-1]) + q[:-2, 1:-1, 1:-1]
    r = (rhs + a * nb) - c * q[1:-1, 1:-1, 1:-1]
    solid = np.zeros(obs.shape, dtype=bool)
    solid[1:-1, 1:-1, 1:-1] = np.asarray(obs)[1:-1, 1:-1, 1:-1] == 1.0      # ghosts and walls are never bodies
    near = (solid[1:-1, 1:-1, 2:] | solid[1:-1, 1:-1, :-2] | solid[1:-1, 2:, 1:-1] | solid[1:-1, :-2, 1:-1] |
            solid[2:, 1:-1, 1:-1] | solid[:-2, 1:-1, 1:-1])
    free = ~solid[1:-1, 1:-1, 1:-1]
    if b != 0:
        free &= ~near
    rec = np.zeros((D, 4))
    rec[:, 0] = np.where(free, r * r, 0.0).sum(axis=(1, 2))
    rec[:, 1] = np.where(free, rhs * rhs, 0.0).sum(axis=(1, 2))
    rec[:, 2] = np.where(free, np.abs(r), 0.0).max(axis=(1, 2))
    rec[:, 3] = free.sum(axis=(1, 2))
    return rec, free


def total(rec):
    return np.array([rec[:, 0].sum(), rec[:, 1].sum(), rec[:, 2].max(), rec[:, 3].sum()])


def nasty_mask(rng, W, H, D):
    """Random solids plus solids on every wall, in corners and adjacent to each other."""
    obs = np.zeros((D + 2, H + 2, W + 2))
    obs[1:-1, 1:-1, 1:-1] = rng.random((D, H, W)) < 0.2
    obs[1, 1, 1] = obs[D, H, W] = obs[1, H, 1] = obs[D, 1, W] = 1.0          # corners
    obs[1, 1, 2] = 1.0                                                       # next to a corner solid
    obs[(D + 1) // 2, 1, 1:W + 1] = 1.0                                      # a whole row on the y = 1 wall
    obs[1:D + 1, (H + 1) // 2, W] = 1.0                                      # a column on the x = W wall
    obs[D, H, max(1, W - 3):W + 1] = 1.0                                     # the tail of the last row of the last plane
    return obs


def as_rec(q):
    return np.array([q["r_sq"], q["rhs_sq"], q["r_max"], q["cells"]], dtype=np.float64)


def load(sim, obs, x, x0):
    import fluid_simulation_amd as F
    sim.set(F.OBS, obs.astype(sim.dtype))
    sim.set(F.DENS, x.astype(sim.dtype))
    sim.set(F.BUFFER, x0.astype(sim.dtype))


# ---- 1. exact cases ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("shape", SHAPES)
def test_integer_fields_are_exact(precision, shape):
    """Fields of small integers (ghost cells included), dyadic a and c: every r, r^2 and partial sum is an integer or a
    dyadic value far below 2^53, so every order of summation is exact -- out and every per-plane record equal the numpy
    restatement bit for bit.  Pins the cell set (F_SOLID, F_NEAR for b != 0, x > W, ghosts) and the formula."""
    import fluid_simulation_amd as F
    W, H, D = shape
    rng = np.random.default_rng(7 + W * 1000 + H * 10 + D)
    obs = nasty_mask(rng, W, H, D)
    x = rng.integers(-8, 9, size=obs.shape).astype(np.float64)
    x0 = rng.integers(-8, 9, size=obs.shape).astype(np.float64)
    sim = sim_of(W, H, D, precision)
    load(sim, obs, x, x0)
    for a, c in COEFFS:
        for b in (0, 1, 2, 3):
            q = sim.solve_residual(b, F.DENS, F.BUFFER, a, c, per_plane=True)
            rec, free = restate(x, x0, obs, a, c, b)
            assert free.sum() > 0 and (b == 0 or free.sum() < (obs[1:-1, 1:-1, 1:-1] == 0).sum())
            assert np.array_equal(q["per_plane"], rec), (a, c, b)
            assert np.array_equal(as_rec(q), total(rec)), (a, c, b)
    # field == prev is legal: the state a diffusion solve starts from
    q = sim.solve_residual(0, F.DENS, F.DENS, 2.0, 13.0, per_plane=True)
    rec, _ = restate(x, x, obs, 2.0, 13.0, 0)
    assert np.array_equal(q["per_plane"], rec) and np.array_equal(as_rec(q), total(rec))
    # nothing was changed by any of it
    assert np.array_equal(sim.get(F.DENS, np.float64), x) and np.array_equal(sim.get(F.BUFFER, np.float64), x0)


# ---- 2. real-valued fields --------------------------------------------------------------------------------------------

@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("shape", SHAPES)
def test_real_fields_match_numpy(precision, shape):
    """Seeded normal fields: r is evaluated in a fixed fp64 order, so max |r| and the cell counts are equal exactly; the
    two sums against numpy's sum within a relative 2 N 2^-53, N the free cells summed -- two orders of a sum of N
    non-negative fp64 terms are each within (N - 1) u of the true sum."""
    import fluid_simulation_amd as F
    W, H, D = shape
    rng = np.random.default_rng(11 + W * 1000 + H * 10 + D)
    obs = nasty_mask(rng, W, H, D)
    dt = np.float32 if precision == "fp32" else np.float64
    x = (rng.standard_normal(obs.shape) * 3.0).astype(dt)
    x0 = rng.standard_normal(obs.shape).astype(dt)
    sim = sim_of(W, H, D, precision)
    load(sim, obs, x, x0)
    for a, c in COEFFS:
        for b in (0, 2):
            q = sim.solve_residual(b, F.DENS, F.BUFFER, a, c, per_plane=True)
            rec, _ = restate(x, x0, obs, a, c, b)
            got = q["per_plane"]
            print(precision, shape, a, c, b, "planes: max rel err", np.max(np.abs(got[:, :2] - rec[:, :2]) / np.maximum(rec[:, :2], 1e-300)),
                  "bound", 2 * rec[:, 3].max() * U)
            assert np.array_equal(got[:, 2:], rec[:, 2:]), (a, c, b)
            assert np.all(np.abs(got[:, :2] - rec[:, :2]) <= 2.0 * rec[:, 3:4] * U * rec[:, :2]), (a, c, b)
            tot, mine = total(rec), as_rec(q)
            assert np.array_equal(mine[2:], tot[2:])
            assert np.all(np.abs(mine[:2] - tot[:2]) <= 2.0 * tot[3] * U * tot[:2]), (a, c, b, mine, tot)
            # the whole-grid record is the planes' records added in increasing z in fp64
            s = np.zeros(2)
            for r in got:
                s = s + r[:2]
            assert bits_equal(mine[:2], s)
            assert q["relative"] == np.sqrt(q["r_sq"] / q["rhs_sq"])


# ---- 3. against a solve -------------------------------------------------------------------------------------------------

def tunnel(solver="jacobi", precision="fp32", N=48, **kw):
    import fluid_simulation_amd as F
    kw.setdefault("dump_every", 0)
    sim = F.Simulation(N, N, N, 1, acc=10, solver=solver, precision=precision, quiet=1, **kw)
    sim.set_mask(ball_mask(N, N, N, N / 2.0, N / 2.0, N / 2.0, N / 8.0))
    return sim


@pytest.mark.parametrize("solver", ["jacobi", "rbsor", "mg", "gs_lex"])
def test_pressure_residual_after_a_projection(solver):
    """After fs_project on a tunnel with a ball, pressure_residual() equals the numpy value on the fetched fields -- the
    sums within 2 N 2^-53, hence `relative` (a square root of their quotient: half the sum of the two errors, plus a
    rounding each for the quotient and the root on either side) within (2 N + 4) 2^-53 -- and it shrinks when the
    iteration count grows: `acc` for the relaxation solvers; the V-cycles of solver mg are counted by mg_cycles (its
    pressure solve does not read acc), so there mg_cycles grows from 1 to 4."""
    import fluid_simulation_amd as F
    rel = []
    for more in (False, True):
        sim = tunnel(solver)
        for _ in range(2):
            sim.run_one()
        if solver == "mg":
            sim.set_option("mg_cycles", 4 if more else 1)
        else:
            sim.acc = 40 if more else 10
        sim.project()
        q = sim.pressure_residual()
        p, div, obs = sim.get(F.PRESSURE), sim.get(F.DIVERGENCE), sim.get(F.OBS)
        rec, _ = restate(p, div, obs, 1.0, 6.0, 0)
        tot = total(rec)
        want = np.sqrt(tot[0] / tot[1])
        print(solver, "more" if more else "less", "relative", q["relative"], "host", want, "cells", q["cells"])
        assert q["cells"] == tot[3] > 0 and q["r_max"] == tot[2]
        assert abs(q["r_sq"] - tot[0]) <= 2 * tot[3] * U * tot[0] and abs(q["rhs_sq"] - tot[1]) <= 2 * tot[3] * U * tot[1]
        assert abs(q["relative"] - want) <= (2 * tot[3] + 4) * U * want
        assert q["relative"] > 0.0
        rel.append(q["relative"])
        sim.close()
    assert rel[1] < rel[0], rel


# ---- 4. the log is the query ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("solver", ["jacobi", "mg"])
def test_log_matches_query_on_a_replayed_step(solver, precision):
    """A second handle replays the fourth step by hand through the per-pass entry points -- inlet and prev copies from the
    host, fs_diffuse x 3, fs_project, fs_advect x 3, fs_project, fs_diffuse of the density -- with the query before and
    after each diffusion and after each projection: the numbers equal the stepping handle's log row bit for bit.  The
    projections start from p = 0, so there r0_sq == rhs_sq bit for bit."""
    import fluid_simulation_amd as F
    sim = tunnel(solver, precision, residual_log=8)
    for _ in range(3):
        sim.run_one()
    state = {f: sim.get(f) for f in (F.VX, F.VY, F.VZ, F.DENS)}
    sim.run_one()
    rows = sim.residual_log()
    assert list(rows["step"]) == [1, 2, 3, 4]
    last = rows[-1]

    def col(k):
        return np.array([last["r0_sq_%d" % k], last["r_sq_%d" % k], last["r_max_%d" % k], last["rhs_sq_%d" % k], last["cells_%d" % k]],
                        dtype=np.float64)

    rep = tunnel(solver, precision)
    vx, vy, vz = state[F.VX].copy(), state[F.VY].copy(), state[F.VZ].copy()
    vx[1:-1, 1:-1, 1] = rep.speed                              # the inlet, simulation.cpp:103-105
    vy[1:-1, 1:-1, 1] = 0.0
    vz[1:-1, 1:-1, 1] = 0.0
    dens = state[F.DENS].copy()
    dens[1:-1, 1:-1, 1] += rep.dtype(np.float32(0.001))        # run()'s inlet density, simulation.cpp:65-67
    for f, f0, a in ((F.VX, F.VX_PREV, vx), (F.VY, F.VY_PREV, vy), (F.VZ, F.VZ_PREV, vz), (F.DENS, F.BUFFER, dens)):
        rep.set(f, a)
        rep.set(f0, a)

    def around_diffusion(b, f, f0):
        before = rep.diffuse_residual(b, f, f0)
        rep.diffuse(b, f, f0)
        after = rep.diffuse_residual(b, f, f0)
        assert after["rhs_sq"] == before["rhs_sq"] and after["cells"] == before["cells"] > 0
        return np.array([before["r_sq"], after["r_sq"], after["r_max"], after["rhs_sq"], after["cells"]], dtype=np.float64)

    V = ((1, F.VX, F.VX_PREV), (2, F.VY, F.VY_PREV), (3, F.VZ, F.VZ_PREV))
    for k, (b, f, f0) in enumerate(V):
        want = around_diffusion(b, f, f0)
        assert bits_equal(col(k), want), (k, col(k), want)
        assert want[1] < want[0]                               # the sweeps reduce the residual of a diffusion system
    for k in (3, 4):
        rep.project()
        q = rep.solve_residual(0, F.PRESSURE, F.DIVERGENCE, 1, 6)
        got = col(k)
        assert bits_equal(got[1:], np.array([q["r_sq"], q["r_max"], q["rhs_sq"], q["cells"]], dtype=np.float64)), (k, got, q)
        assert bits_equal(got[0:1], got[3:4]) and got[0] > 0.0  # p = 0 at the start: r = div
        assert last["reduction_%d" % k] == np.sqrt(got[1] / got[0])
        if k == 3:
            for b, f, f0 in V:
                rep.advect(b, f, f0)
    want = around_diffusion(0, F.DENS, F.BUFFER)
    assert bits_equal(col(5), want), (col(5), want)


# ---- 5. the log changes nothing -----------------------------------------------------------------------------------------

def test_log_leaves_the_run_unchanged(tmp_path):
    """Every field and every dumped frame of a run with the log on is byte-identical with the run without it."""
    import fluid_simulation_amd as F
    out = {}
    for on in (0, 6):
        d = tmp_path / ("log%d" % on)
        d.mkdir()
        sim = tunnel(residual_log=on, dump_dir=str(d), dump_every=1)
        sim.iter = 4
        sim.run()
        out[on] = {f: sim.get(f) for f in range(11)}
        assert len(sim.residual_log()) == (4 if on else 0)
        sim.close()
    for f in range(11):
        assert bits_equal(out[0][f], out[6][f]), F.FIELD_NAMES[f]
    for name in ("data.bin", "obs.bin", "v_x.bin", "v_y.bin", "v_z.bin"):
        a = (tmp_path / "log0" / name).read_bytes()
        assert len(a) > 0 and a == (tmp_path / "log6" / name).read_bytes(), name


# ---- 6. the ring ----------------------------------------------------------------------------------------------------------

def test_log_wraps_and_reports_the_overwritten_steps():
    sim = tunnel(residual_log=3)
    for _ in range(5):
        sim.step()
    rows, dropped = sim.residual_log(with_dropped=True)
    assert list(rows["step"]) == [3, 4, 5] and dropped == 2
    assert np.all(rows["cells_3"] > 0) and np.all(rows["r_sq_3"] > 0.0)
    rows, dropped = sim.residual_log(with_dropped=True)         # drained
    assert len(rows) == 0 and dropped == 0
    sim.step()
    rows, dropped = sim.residual_log(with_dropped=True)
    assert list(rows["step"]) == [6] and dropped == 0
    sim.set_option("residual_log", 2)                           # re-setting clears
    assert len(sim.residual_log()) == 0
    import fluid_simulation_amd as F
    with pytest.raises(F.FluidsimError):
        sim.set_option("residual_log", 1048577)


def test_log_off_launches_nothing_and_on_twelve_records_per_step():
    """The "residual" timing family counts one launch per record: six solves, before and after = 12 per step; 10 where
    the dead density solve is elided; nothing with the log off."""
    for n, elide, want in ((0, 0, 0), (4, 0, 36), (4, 1, 30)):
        sim = tunnel(residual_log=n, profile=1, elide_dead_density_solve=elide)
        for _ in range(3):
            sim.step()
        sim.sync()
        assert sim.timing("residual")[1] == want
        sim.close()


def test_elided_and_empty_solves():
    """A solve the step does not run has NaN in its four real columns and 0 cells; a solve of zero sweeps leaves
    r_sq == r0_sq."""
    sim = tunnel(residual_log=2, elide_dead_density_solve=1)
    sim.run_one()
    row = sim.residual_log()[0]
    assert all(np.isnan(row[k]) for k in ("r0_sq_5", "r_sq_5", "r_max_5", "rhs_sq_5", "reduction_5")) and row["cells_5"] == 0
    assert row["cells_0"] > 0 and not np.isnan(row["r_sq_4"])
    sim.close()
    sim = tunnel(residual_log=2)
    sim.acc = 0
    sim.run_one()
    row = sim.residual_log()[0]
    for k in range(6):
        assert row["cells_%d" % k] > 0 and bits_equal(np.array([row["r_sq_%d" % k]]), np.array([row["r0_sq_%d" % k]])), k


def test_bad_arguments_and_fsnull():
    import fluid_simulation_amd as F
    sim = sim_of(16, 16, 16)
    for args in ((4, F.DENS, F.BUFFER), (-1, F.DENS, F.BUFFER), (0, 11, F.BUFFER), (0, F.DENS, -1)):
        with pytest.raises(F.FluidsimError) as e:
            sim.solve_residual(*args, 1.0, 6.0)
        assert e.value.code == -1
        with pytest.raises(F.FluidsimError):
            sim.diffuse_residual(*args)
    sim.close()
    sim = F.Simulation(16, 16, 16, 1, quiet=1, residual_log=2)
    sim.comm_init(0, 2, b"FSNULL:".ljust(128, b"\0"))
    with pytest.raises(F.FluidsimError) as e:
        sim.pressure_residual()
    assert e.value.code == -1 and "FSNULL" in str(e.value)


# ---- 7. z-slabs ------------------------------------------------------------------------------------------------------

def ipc_usable():
    exe = os.path.join(ROOT, "tools", "ipc_probe")
    if not os.path.exists(exe):
        return False, "tools/ipc_probe was not built"
    r = subprocess.run([exe, "2", "8", "1"], capture_output=True, text=True, timeout=120,
                       env=dict(os.environ, FS_IPC_TIMEOUT_S="20"))
    return r.returncode == 0, (r.stdout + r.stderr)[-400:]


_SINGLE = {}
# jacobi: 24 planes per rank of two (every schedule splits boundary and interior); mg: level 1 (16 x 16 x 64 / 128) stays
# distributed at the default mg_min_planes = 32, so the seam to the levels held whole lies below a distributed coarse level
CASES = {"jacobi": (32, 24, 48), "mg2": (32, 32, 128), "mg4": (32, 32, 256)}


def run_ranks(tmp, nranks, transport, case, overlap="auto", log=6, steps=3):
    import fluid_simulation_amd as F
    W, H, D = CASES[case]
    solver = "mg" if case.startswith("mg") else "jacobi"
    out = os.path.join(tmp, "%s_n%d_%s_%s_%d" % (transport, nranks, case, overlap, log))
    os.makedirs(out)
    idfile = os.path.join(out, "id.bin")
    if nranks > 1:
        open(idfile, "wb").write(F.comm_unique_id(transport))
    procs = [subprocess.Popen([sys.executable, WORKER, str(r), str(nranks), idfile, out, str(W), str(H), str(D), str(steps),
                               solver, overlap, str(log)], env=dict(os.environ, FS_IPC_TIMEOUT_S="60")) for r in range(nranks)]
    for p in procs:
        assert p.wait(timeout=600) == 0
    return [np.load(os.path.join(out, "rank%d.npz" % r)) for r in range(nranks)]


def single(tmp, case):
    if case not in _SINGLE:
        _SINGLE[case] = run_ranks(tmp, 1, "single", case)[0]
    ref = _SINGLE[case]
    assert ref["raw"].shape == (3, 31) and np.all(ref["raw"][:, 5::5] > 0) and ref["launches"] == 24
    return ref


def same_as_one_gpu(z, ref, who):
    assert bits_equal(z["raw"], ref["raw"]), (who, z["raw"], ref["raw"])
    for k in ("p", "p_planes", "v", "v_planes"):
        assert bits_equal(z[k], ref[k]), (who, k)


@pytest.mark.parametrize("nranks,transport,case", [(2, "shm", "jacobi"), (4, "shm", "jacobi"), (2, "shm", "mg2"), (4, "shm", "mg4"),
                                                   (2, "ipc", "jacobi"), (4, "ipc", "jacobi"), (2, "ipc", "mg2")])
def test_slabs_bit_identical_with_one_gpu(tmp_path, nranks, transport, case):
    """The drained log and the per-plane queries (pressure; a velocity system with field == prev) of every rank equal
    the one-GPU run bit for bit, under the schedule "auto" picks."""
    if transport == "ipc":
        ok, why = ipc_usable()
        if not ok:
            pytest.skip("FSIPC transport not usable on this box: " + why)
    ref = single(str(tmp_path), case)
    for r, z in enumerate(run_ranks(str(tmp_path), nranks, transport, case)):
        same_as_one_gpu(z, ref, r)


@pytest.mark.parametrize("transport,overlap", [("shm", "0"), ("shm", "1"), ("shm", "2"), ("ipc", "3")])
def test_every_schedule_leaves_current_halos_and_the_log_adds_no_exchange(tmp_path, transport, overlap):
    """Under each communication schedule the records of the boundary planes (they read the neighbour's plane of x) equal
    the one-GPU run, and steps with the log on issue exactly the exchanges of steps with it off ("comm" launches)."""
    if transport == "ipc":
        ok, why = ipc_usable()
        if not ok:
            pytest.skip("FSIPC transport not usable on this box: " + why)
    ref = single(str(tmp_path), "jacobi")
    on = run_ranks(str(tmp_path), 2, transport, "jacobi", overlap)
    off = run_ranks(str(tmp_path), 2, transport, "jacobi", overlap, log=0)
    for r in range(2):
        assert on[r]["plan"][0] == int(overlap)
        same_as_one_gpu(on[r], ref, r)
        print(transport, "overlap", overlap, "rank", r, "comm launches of two steps: log on", int(on[r]["comm"]), "off", int(off[r]["comm"]))
        assert on[r]["comm"] == off[r]["comm"] > 0 and off[r]["launches"] == 0 and on[r]["launches"] == 24
        for k in ("p", "p_planes", "v", "v_planes"):
            assert bits_equal(off[r][k], ref[k]), (r, k)


# ---- 8. simulation.out --residuals -----------------------------------------------------------------------------------

def test_cli_residuals_csv_matches_python(tmp_path):
    import fluid_simulation_amd as F
    exe = os.path.join(ROOT, "simulation.out")
    assert os.path.exists(exe), "simulation.out is built by __graft_entry__.build()"
    stl = os.path.join(GOLDEN, "sphere_24x12.stl")
    csv, fcsv = tmp_path / "r.csv", tmp_path / "f.csv"
    env = {k: v for k, v in os.environ.items() if not k.startswith("FS_")}
    subprocess.run([exe, "--grid", "64x32x32", "--steps", "5", "--residuals", str(csv), "--forces", str(fcsv), "--stl",
                    stl + ",0.5,0,0,0,0,0,0", "--dump-every", "0", "--dump-dir", str(tmp_path), "--quiet"], check=True,
                   cwd=str(tmp_path), env=env, timeout=600)
    lines = csv.read_text().splitlines()
    assert lines[0] == ",".join(F.RESIDUAL_LOG_DTYPE.names)
    got = np.array([[float(v) for v in ln.split(",")] for ln in lines[1:]])
    assert got.shape == (5, 37) and len(fcsv.read_text().splitlines()) == 6
    sim = F.Simulation(64, 32, 32, 5, quiet=1, dump_every=0, residual_log=5)
    F.loadSTLIntoObstacles(stl, sim, 0.5, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0)
    sim.run()
    rows = sim.residual_log()
    want = np.stack([rows[k].astype(np.float64) for k in rows.dtype.names], axis=1)
    assert np.all(want[:, 5::5][:, :6] > 0)
    assert np.array_equal(got[:, :31], want[:, :31])
    assert np.allclose(got[:, 31:], want[:, 31:], rtol=1e-15, atol=0, equal_nan=True)
