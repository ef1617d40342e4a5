"""Obstacle pressure force (fs_obstacle_force, option "force_log" / fs_force_log) on the MI355X: analytic cases
that fix the definition of include/fluidsim.h, a numpy restatement on random masks, the per-step log inside real
runs (bit-identical with the on-demand query and with a per-pass replay, no effect on the run), the direction of
the drag, z-slab runs bit-identical with one GPU, and the CSV of simulation.out."""
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import GOLDEN, ROOT, ball_mask, bits_equal

pytestmark = pytest.mark.gpu
WORKER = os.path.join(ROOT, "tests", "forces_slab_worker.py")
PRECISIONS = ["fp32", "fp64"]


def sim_of(W, H, D, precision="fp32", **kw):
    import fluid_simulation_amd as F
    kw.setdefault("quiet", 1)
    kw.setdefault("dump_every", 0)
    return F.Simulation(W, H, D, 1, precision=precision, **kw)


def restate(obs, p):
    """numpy fp64 restatement of the definition in include/fluidsim.h: per z-plane {Sx, Sy, Sz, faces, frontal}."""
    D, H, W = (n - 2 for n in obs.shape)
    o = np.asarray(obs, dtype=np.float64)
    inner = (slice(1, D + 1), slice(1, H + 1), slice(1, W + 1))
    upd = o[inner] != 1.0
    pc = np.asarray(p, dtype=np.float64)[inner]
    z, y, x = np.meshgrid(np.arange(1, D + 1), np.arange(1, H + 1), np.arange(1, W + 1), indexing="ij")
    rec = np.zeros((D, 5))
    mag = np.zeros(D)
    for comp, (dz, dy, dx) in enumerate(((0, 0, 1), (0, 1, 0), (1, 0, 0))):
        for sgn in (1, -1):
            nb = o[1 + sgn * dz:D + 1 + sgn * dz, 1 + sgn * dy:H + 1 + sgn * dy, 1 + sgn * dx:W + 1 + sgn * dx]
            zz, yy, xx = z + sgn * dz, y + sgn * dy, x + sgn * dx
            inr = (xx >= 1) & (xx <= W) & (yy >= 1) & (yy <= H) & (zz >= 1) & (zz <= D)
            blocked = upd & inr & (nb != 0.0)
            rec[:, comp] += sgn * np.where(blocked, pc, 0.0).sum(axis=(1, 2))
            rec[:, 3] += blocked.sum(axis=(1, 2))
            mag += np.where(blocked, np.abs(pc), 0.0).sum(axis=(1, 2))
    rec[:, 4] = (o[inner] == 1.0).any(axis=2).sum(axis=1)
    return rec, mag


def query(sim, obs, p):
    import fluid_simulation_amd as F
    sim.set(F.OBS, obs.astype(sim.dtype))
    sim.set(F.PRESSURE, p.astype(sim.dtype))
    return sim.obstacle_force(per_plane=True)


def box(shape, x0, x1, y0, y1, z0, z1):
    m = np.zeros(shape)
    m[z0:z1 + 1, y0:y1 + 1, x0:x1 + 1] = 1.0
    return m


# ---- 1. analytic, solver-free ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("precision", PRECISIONS)
def test_constant_pressure_on_closed_bodies_is_zero(precision):
    W, H, D = 40, 28, 24
    shape = (D + 2, H + 2, W + 2)
    bodies = {
        "ball": ball_mask(W, H, D, 14, 14, 12, 6).astype(np.float64),
        "box": box(shape, 20, 31, 5, 14, 6, 17),
        "column": box(shape, 8, 10, 9, 12, 2, 22),          # crosses 21 z-planes
    }
    bodies["all"] = np.maximum(np.maximum(bodies["ball"], box(shape, 30, 35, 18, 24, 3, 8)), bodies["column"])
    sim = sim_of(W, H, D, precision)
    p = np.full(shape, 0.75)
    for name, obs in bodies.items():
        q = query(sim, obs, p)
        assert q["faces"] > 0, name
        assert np.array_equal(q["S"], [0.0, 0.0, 0.0]), (name, q["S"])
        rec, _ = restate(obs, p)
        assert np.array_equal(q["per_plane"][:, 3:], rec[:, 3:]), name


@pytest.mark.parametrize("precision", PRECISIONS)
def test_body_on_the_wall_feels_the_unbalanced_side(precision):
    """A box resting on the y = 1 wall: its wall side has no blocked face, so S = -c * A * y_hat (A = contact cells)."""
    W, H, D = 32, 24, 20
    shape = (D + 2, H + 2, W + 2)
    c = 1.25
    obs = box(shape, 8, 13, 1, 4, 5, 11)                     # 6 x 4 x 7 cells, 6 * 7 of them on the wall
    q = query(sim_of(W, H, D, precision), obs, np.full(shape, c))
    assert np.array_equal(q["S"], [0.0, -c * 6 * 7, 0.0]), q["S"]
    assert q["faces"] == 2 * 4 * 7 + 6 * 7 + 2 * 6 * 4 and q["frontal"] == 4 * 7


@pytest.mark.parametrize("precision", PRECISIONS)
def test_linear_pressure_around_a_box(precision):
    """p = a + g . (x, y, z) around an Lx x Ly x Lz box away from the walls: Sx = -gx (Lx+1) Ly Lz (likewise y, z),
    faces = 2 (Lx Ly + Ly Lz + Lz Lx), frontal = Ly Lz -- exactly, with dyadic a and g."""
    W, H, D = 36, 30, 26
    shape = (D + 2, H + 2, W + 2)
    x0, y0, z0, Lx, Ly, Lz = 9, 7, 6, 11, 9, 13
    obs = box(shape, x0, x0 + Lx - 1, y0, y0 + Ly - 1, z0, z0 + Lz - 1)
    a, gx, gy, gz = 0.5, 0.25, -0.125, 0.0625
    z, y, x = np.mgrid[0:D + 2, 0:H + 2, 0:W + 2]
    p = a + gx * x + gy * y + gz * z
    q = query(sim_of(W, H, D, precision), obs, p)
    want = [-gx * (Lx + 1) * Ly * Lz, -gy * (Ly + 1) * Lx * Lz, -gz * (Lz + 1) * Lx * Ly]
    assert np.array_equal(q["S"], want), (q["S"], want)
    assert q["faces"] == 2 * (Lx * Ly + Ly * Lz + Lz * Lx)
    assert q["frontal"] == Ly * Lz
    assert np.array_equal(q["per_plane"][:, 4].sum(), Ly * Lz)


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("shape", [(37, 21, 18), (64, 48, 20), (5, 3, 4)])
def test_random_mask_matches_numpy(precision, shape):
    """Random masks with obs values outside {0, 1} (set through fs_set_field(FS_OBS)) and random p: the per-plane records
    and the totals match the numpy restatement (1e-12 of the summed magnitudes), the counts exactly."""
    W, H, D = shape
    rng = np.random.default_rng(W * 1000 + H * 10 + D)
    obs = np.zeros((D + 2, H + 2, W + 2))
    obs[1:-1, 1:-1, 1:-1] = rng.choice([0.0, 1.0, 0.5, 2.0, -1.0], size=(D, H, W), p=[0.6, 0.25, 0.05, 0.05, 0.05])
    p = rng.standard_normal(obs.shape) * 3.0
    if precision == "fp32":
        p = p.astype(np.float32)
    q = query(sim_of(W, H, D, precision), obs, p)
    rec, mag = restate(obs, p)
    got = q["per_plane"]
    assert np.array_equal(got[:, 3:], rec[:, 3:])
    assert np.all(np.abs(got[:, :3] - rec[:, :3]) <= 1e-12 * mag[:, None] + 1e-300)
    assert np.all(np.abs(q["S"] - rec[:, :3].sum(axis=0)) <= 1e-12 * mag.sum())
    assert q["faces"] == rec[:, 3].sum() and q["frontal"] == rec[:, 4].sum()
    # the totals are the planes' records added in increasing z in fp64
    tot = np.zeros(5)
    for r in got:
        tot = tot + r
    assert bits_equal(q["S"], tot[:3])


# ---- 2. in a run ---------------------------------------------------------------------------------------------------

def tunnel(solver="jacobi", **kw):
    import fluid_simulation_amd as F
    N = 64
    kw.setdefault("dump_every", 0)
    sim = F.Simulation(N, N, N, 1, acc=10, solver=solver, quiet=1, **kw)
    sim.set_mask(ball_mask(N, N, N, N / 2.0, N / 2.0, N / 2.0, 8))
    return sim


@pytest.mark.parametrize("solver", ["jacobi", "mg"])
def test_log_matches_query_and_per_pass_replay(solver):
    """S2 of a step's row = fs_obstacle_force right after that step; S1 = the query on a second handle that replays the
    step's first half through the per-pass entry points (inlet, prev copies, fs_diffuse x 3, fs_project)."""
    import fluid_simulation_amd as F
    sim = tunnel(solver, force_log=8)
    for _ in range(3):
        sim.run_one()
    state = {f: sim.get(f) for f in (F.VX, F.VY, F.VZ, F.OBS)}
    sim.run_one()
    after = sim.obstacle_force()
    rows = sim.force_log()
    assert list(rows["step"]) == [1, 2, 3, 4]
    last = rows[-1]
    assert bits_equal(np.array([last["s2x"], last["s2y"], last["s2z"]]), after["S"])
    assert last["faces"] == after["faces"] > 0 and last["frontal"] == after["frontal"] > 0

    rep = tunnel(solver)
    vx, vy, vz = state[F.VX].copy(), state[F.VY].copy(), state[F.VZ].copy()
    vx[1:-1, 1:-1, 1] = rep.speed                              # the inlet, simulation.cpp:103-105
    vy[1:-1, 1:-1, 1] = 0.0
    vz[1:-1, 1:-1, 1] = 0.0
    rep.set(F.OBS, state[F.OBS])
    for f, f0, a in ((F.VX, F.VX_PREV, vx), (F.VY, F.VY_PREV, vy), (F.VZ, F.VZ_PREV, vz)):
        rep.set(f, a)
        rep.set(f0, a)
    for b, f, f0 in ((1, F.VX, F.VX_PREV), (2, F.VY, F.VY_PREV), (3, F.VZ, F.VZ_PREV)):
        rep.diffuse(b, f, f0)
    rep.project()
    first = rep.obstacle_force()
    assert bits_equal(np.array([last["s1x"], last["s1y"], last["s1z"]]), first["S"])
    # the step's force applies both impulses
    force, coeff = F.pressure_force(first["S"] + after["S"], after["frontal"], sim.dt, sim.speed, 64, 64, 64)
    assert bits_equal(np.array([last["fx"], last["fy"], last["fz"]]), force)
    assert bits_equal(np.array([last["cx"], last["cy"], last["cz"]]), coeff)


def test_log_leaves_the_run_unchanged(tmp_path):
    """Every field and every dumped frame of a run with the log on is byte-identical with the run without it."""
    import fluid_simulation_amd as F
    out = {}
    for on in (0, 6):
        d = tmp_path / ("log%d" % on)
        d.mkdir()
        sim = tunnel(force_log=on, dump_dir=str(d), dump_every=1)
        sim.iter = 4
        sim.run()
        out[on] = {f: sim.get(f) for f in range(11)}
        if on:
            assert len(sim.force_log()) == 4
        sim.close()
    for f in range(11):
        assert bits_equal(out[0][f], out[6][f]), F.FIELD_NAMES[f]
    for name in ("data.bin", "obs.bin", "v_x.bin", "v_y.bin", "v_z.bin"):
        a = (tmp_path / "log0" / name).read_bytes()
        assert len(a) > 0 and a == (tmp_path / "log6" / name).read_bytes(), name


def test_log_wraps_and_reports_the_overwritten_steps():
    sim = tunnel(force_log=3)
    for _ in range(5):
        sim.step()
    rows, dropped = sim.force_log(with_dropped=True)
    assert list(rows["step"]) == [3, 4, 5] and dropped == 2
    rows, dropped = sim.force_log(with_dropped=True)            # drained
    assert len(rows) == 0 and dropped == 0
    sim.step()
    rows, dropped = sim.force_log(with_dropped=True)
    assert list(rows["step"]) == [6] and dropped == 0
    sim.set_option("force_log", 2)                              # re-setting clears
    rows = sim.force_log()
    assert len(rows) == 0


def test_log_off_launches_nothing_and_on_two_per_step():
    for n, want in ((0, 0), (4, 6)):
        sim = tunnel(force_log=n, profile=1)
        for _ in range(3):
            sim.step()
        sim.sync()
        assert sim.timing("forces")[1] == want
        sim.close()


def test_drag_points_downstream():
    """A centred ball after 20 steps of the default inlet: p > 0 upstream, p < 0 downstream of the body, so Sx > 0."""
    sim = tunnel(force_log=20)
    sim.acc = 15
    for _ in range(20):
        sim.run_one()
    q = sim.obstacle_force()
    rows = sim.force_log()
    assert q["S"][0] > 0.0 and q["force"][0] > 0.0 and q["coeff"][0] > 0.0, q
    assert np.all(rows["s2x"][-5:] > 0.0) and np.all(rows["fx"][-5:] > 0.0), rows


def test_fsnull_slab_handle_refuses():
    import fluid_simulation_amd as F
    sim = F.Simulation(16, 16, 16, 1, quiet=1, force_log=2)
    sim.comm_init(0, 2, b"FSNULL:".ljust(128, b"\0"))
    with pytest.raises(F.FluidsimError) as e:
        sim.obstacle_force()
    assert e.value.code == -1 and "FSNULL" in str(e.value)


# ---- 4. z-slabs ------------------------------------------------------------------------------------------------------

def ipc_usable():
    exe = os.path.join(ROOT, "tools", "ipc_probe")
    if not os.path.exists(exe):
        return False, "tools/ipc_probe was not built"
    r = subprocess.run([exe, "2", "8", "1"], capture_output=True, text=True, timeout=120,
                       env=dict(os.environ, FS_IPC_TIMEOUT_S="20"))
    return r.returncode == 0, (r.stdout + r.stderr)[-400:]


_SINGLE = {}


def run_ranks(tmp, nranks, transport, W, H, D, steps, solver):
    import fluid_simulation_amd as F
    out = os.path.join(tmp, "%s_n%d_%s" % (transport, nranks, solver))
    os.makedirs(out)
    idfile = os.path.join(out, "id.bin")
    if nranks > 1:
        open(idfile, "wb").write(F.comm_unique_id(transport))
    procs = [subprocess.Popen([sys.executable, WORKER, str(r), str(nranks), idfile, out, str(W), str(H), str(D), str(steps),
                               solver], env=dict(os.environ, FS_IPC_TIMEOUT_S="60")) for r in range(nranks)]
    for p in procs:
        assert p.wait(timeout=600) == 0
    return [np.load(os.path.join(out, "rank%d.npz" % r)) for r in range(nranks)]


@pytest.mark.parametrize("nranks,transport", [(2, "shm"), (4, "shm"), (2, "ipc"), (4, "ipc")])
def test_slabs_bit_identical_with_one_gpu(tmp_path, nranks, transport):
    if transport == "ipc":
        ok, why = ipc_usable()
        if not ok:
            pytest.skip("FSIPC transport not usable on this box: " + why)
    W, H, D, steps, solver = 32, 24, 32, 3, "jacobi"
    if "ref" not in _SINGLE:
        _SINGLE["ref"] = run_ranks(str(tmp_path), 1, "single", W, H, D, steps, solver)[0]
    ref = _SINGLE["ref"]
    assert ref["raw"].shape == (steps, 9) and ref["counts"][1] > 0
    assert np.all(ref["raw"][:, 7] > 0)
    for r, z in enumerate(run_ranks(str(tmp_path), nranks, transport, W, H, D, steps, solver)):
        assert bits_equal(z["raw"], ref["raw"]), (r, z["raw"], ref["raw"])
        assert bits_equal(z["S"], ref["S"]) and np.array_equal(z["counts"], ref["counts"]), r
        assert bits_equal(z["per_plane"], ref["per_plane"]), r


# ---- 5. simulation.out --forces ---------------------------------------------------------------------------------------

def test_cli_forces_csv_matches_python(tmp_path):
    import fluid_simulation_amd as F
    exe = os.path.join(ROOT, "simulation.out")
    assert os.path.exists(exe), "simulation.out is built by __graft_entry__.build()"
    stl = os.path.join(GOLDEN, "sphere_24x12.stl")
    csv = tmp_path / "f.csv"
    env = {k: v for k, v in os.environ.items() if not k.startswith("FS_")}
    subprocess.run([exe, "--grid", "64x32x32", "--steps", "5", "--forces", str(csv), "--stl", stl + ",0.5,0,0,0,0,0,0",
                    "--dump-every", "0", "--dump-dir", str(tmp_path), "--quiet"], check=True, cwd=str(tmp_path), env=env,
                   timeout=600)
    lines = csv.read_text().splitlines()
    assert lines[0] == "step,s1x,s1y,s1z,s2x,s2y,s2z,faces,frontal,fx,fy,fz,cx,cy,cz"
    got = np.array([[float(v) for v in ln.split(",")] for ln in lines[1:]])
    assert got.shape == (5, 15)
    sim = F.Simulation(64, 32, 32, 5, quiet=1, dump_every=0, force_log=5)
    F.loadSTLIntoObstacles(stl, sim, 0.5, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0)
    sim.run()
    rows = sim.force_log()
    want = np.stack([rows[k].astype(np.float64) for k in rows.dtype.names], axis=1)
    assert np.all(want[:, 8] > 0), "the sphere should give the tunnel a body"
    assert np.array_equal(got[:, :9], want[:, :9])
    assert np.allclose(got[:, 9:], want[:, 9:], rtol=1e-12, atol=0, equal_nan=True)
