"""The flow monitor on the MI355X (fs_flow_monitor, fs_monitor_sample, fs_monitor_log, options "monitor_log" /
"monitor_every" / "monitor_stations"), through the C ABI via the Python mirror: the three launches against the numpy
restatement of include/fluidsim.h (tests/monitor_model.py) on grids of one cell, of rows that are no multiple of four, of
rows across a wave and across a workgroup; non-finite values; no side effects; the log against the query; the ring; the
stations; the Courant numbers; the refusals; simulation.out --monitor.  Every comparison is bit for bit."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import monitor_model as M
from conftest import ROOT, GOLDEN, ball_mask, bits_equal

pytestmark = pytest.mark.gpu
FAMILIES = ["sweep", "sweep_pair", "sweep_triple", "divergence", "gradient", "advect", "bounds", "misc", "comm", "multigrid",
            "forces", "residual", "flow_stats", "vortex", "probes", "body_forces", "images", "tracers", "volume", "confinement"]
GRIDS = [(1, 1, 1), (3, 2, 1), (13, 7, 5), (65, 16, 3), (130, 9, 6), (257, 3, 2), (33, 16, 12)]
EMPTY = [0.0] * 12 + [np.inf, -np.inf, np.inf, -np.inf]


def sim_of(W, H, D, precision="fp32", **kw):
    import fluid_simulation_amd as F
    kw.setdefault("quiet", 1)
    kw.setdefault("dump_every", 0)
    return F.Simulation(W, H, D, 1, precision=precision, **kw)


def same(a, b):
    return bool(np.array_equal(np.asarray(a), np.asarray(b), equal_nan=True))


def nasty_mask(rng, W, H, D):
    """solids at random, on walls, in corners, a whole row, and the tail of the last row; ghosts clear"""
    m = np.zeros((D + 2, H + 2, W + 2), dtype=bool)
    m[1:-1, 1:-1, 1:-1] = rng.random((D, H, W)) < 0.2
    m[1:-1, 1, 1:-1] |= rng.random((D, W)) < 0.5             # the y = 1 wall
    m[1, 1:-1, 1:-1] |= rng.random((H, W)) < 0.5             # the z = 1 wall
    m[1:-1, 1:-1, W] |= rng.random((D, H)) < 0.5             # the x = W wall
    for z in (1, D):
        for y in (1, H):
            for x in (1, W):
                m[z, y, x] = (z + y + x) % 2 == 1            # the corners, some solid, some fluid
    m[(D + 1) // 2, (H + 1) // 2, 1:-1] = True               # a whole row
    m[D, H, W // 2 + 1:W + 1] = True                         # the tail of the last row
    return m


def load(sim, fields, mask):
    import fluid_simulation_amd as F
    sim.set_mask(mask)
    for f, a in zip((F.DENS, F.VX, F.VY, F.VZ, F.PRESSURE), fields):
        sim.set(f, a)


def expect_model(sim, fields, mask, context):
    got = sim.flow_monitor(per_plane=True, x_profile=True)
    whole, planes, profile = M.monitor(*fields, mask.astype(np.float32))
    assert same(got["values"], whole), (context, got["values"], whole)
    assert same(got["per_plane"], planes), (context, np.argwhere(~np.isclose(got["per_plane"], planes, rtol=0, atol=0, equal_nan=True))[:4])
    assert same(got["x_profile"], profile), (context, np.argwhere(~np.isclose(got["x_profile"], profile, rtol=0, atol=0, equal_nan=True))[:4])
    return whole, planes, profile


# ---- 1. the records against the model ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("precision", ["fp32", "fp64"])
@pytest.mark.parametrize("grid", GRIDS)
def test_records_match_the_model(grid, precision):
    W, H, D = grid
    sim = sim_of(W, H, D, precision)
    rng = np.random.default_rng([W, H, D, precision == "fp64"])
    shape = (D + 2, H + 2, W + 2)
    mask = nasty_mask(rng, W, H, D)
    fields = [(rng.standard_normal(shape) * 10.0 ** rng.integers(-2, 3)).astype(sim.dtype) for _ in range(5)]
    load(sim, fields, np.zeros(shape, dtype=bool))
    whole, planes, profile = expect_model(sim, fields, np.zeros(shape, dtype=bool), (grid, precision, "no solid"))
    assert whole[0] == W * H * D and np.all(profile[:, 0] == H * D) and np.all(np.isfinite(whole))
    load(sim, fields, mask)
    whole, planes, profile = expect_model(sim, fields, mask, (grid, precision, "real"))
    fluid = int((~mask[1:-1, 1:-1, 1:-1]).sum())
    assert whole[0] == fluid == planes[:, 0].sum() == profile[:, 0].sum() and whole[1] == 0
    # NaN and +-Inf in target, solid and ghost cells
    target = np.argwhere(~mask[1:-1, 1:-1, 1:-1]) + 1
    solid = np.argwhere(mask)
    planted = 0
    for k, bad in enumerate((np.nan, np.inf, -np.inf, np.nan, np.inf)):
        if len(target):
            z, y, x = target[rng.integers(len(target))]
            fields[k][z, y, x] = bad
            planted += 1
        if len(solid):
            z, y, x = solid[rng.integers(len(solid))]
            fields[(k + 1) % 5][z, y, x] = bad
        fields[k][0, 1:-1, 1:-1] = bad                       # ghost faces (the box edges stay as they are)
        fields[(k + 2) % 5][1:-1, H + 1, 1:-1] = bad
        fields[(k + 3) % 5][1:-1, 1:-1, 0] = bad
    load(sim, fields, mask)
    whole, planes, profile = expect_model(sim, fields, mask, (grid, precision, "non-finite"))
    assert whole[0] == fluid and (whole[1] >= 1) == (planted > 0) and whole[1] <= planted
    sim.close()


def test_a_plane_all_solid_gives_the_empty_record():
    W, H, D = 13, 7, 5
    sim = sim_of(W, H, D)
    rng = np.random.default_rng(5)
    shape = (D + 2, H + 2, W + 2)
    mask = np.zeros(shape, dtype=bool)
    mask[3, 1:-1, 1:-1] = True
    fields = [rng.standard_normal(shape).astype(np.float32) for _ in range(5)]
    fields[1][3] = np.nan                                    # whatever the solid plane holds
    load(sim, fields, mask)
    whole, planes, profile = expect_model(sim, fields, mask, "solid plane")
    assert same(planes[2], EMPTY) and whole[0] == W * H * (D - 1) and whole[1] == 0
    mask[1:-1, 1:-1, 1:-1] = True
    load(sim, fields, mask)
    whole, planes, profile = expect_model(sim, fields, mask, "all solid")
    assert same(whole, EMPTY) and not profile.any()
    sim.close()


# ---- 2. no side effects ------------------------------------------------------------------------------------------------------

def test_the_query_and_the_log_change_nothing():
    W, H, D = 24, 20, 12
    mask = ball_mask(W, H, D, 8, 10, 6, 3)
    counts, fields = {}, {}
    for how in ("off", "on"):
        sim = sim_of(W, H, D, acc=6, profile=1, sweep_fuse=2, two_sweep_kernel="pair", pair_shape=1)
        if how == "on":
            sim.set_option("monitor_log", 8)
        sim.set_mask(mask)
        for _ in range(3):
            sim.run_one()
        counts[how] = {f: sim.timing(f)[1] for f in FAMILIES + ["monitor"]}
        fields[how] = [sim.get(f) for f in range(11)]
        if how == "on":
            # the query changes no field either, and counts one record
            sim.flow_monitor(per_plane=True, x_profile=True)
            for f in range(11):
                assert bits_equal(sim.get(f), fields[how][f]), f
            assert sim.timing("monitor")[1] == 4
            sim.monitor_sample()
            assert sim.timing("monitor")[1] == 5
            assert [int(r[0]) for r in sim.monitor_log()] == [1, 2, 3, 3]
        sim.close()
    assert counts["off"]["monitor"] == 0 and counts["on"]["monitor"] == 3, counts
    for f in FAMILIES:
        assert counts["on"][f] == counts["off"][f], (f, counts)
    assert counts["off"]["advect"] > 0 and counts["off"]["gradient"] > 0, counts
    for f in range(11):
        assert bits_equal(fields["on"][f], fields["off"][f]), f


# ---- 3. the log -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("precision", ["fp32", "fp64"])
def test_log_rows_are_the_query_after_each_step(precision):
    W, H, D = 24, 20, 12
    mask = ball_mask(W, H, D, 8, 10, 6, 3)
    stations = [2, 23, 9]
    a = sim_of(W, H, D, precision, acc=6, monitor_log=8, monitor_stations="2,23,9")
    b = sim_of(W, H, D, precision, acc=6)
    c = sim_of(W, H, D, precision, acc=6, monitor_log=8, monitor_every=2, monitor_stations=stations)
    assert a._geti("monitor_stations") == 3 and b._geti("monitor_stations") == 0 and c._geti("monitor_every") == 2
    want = []
    for h in (a, b, c):
        h.set_mask(mask)
    for step in range(1, 5):
        for h in (a, b, c):
            h.run_one()
        r = b.flow_monitor(x_profile=True)
        want.append(M.log_row(step, r["values"], r["x_profile"], stations))
        # and the query is the model of the fetched state
        import fluid_simulation_amd as F
        whole, _, profile = M.monitor(*(b.get(f) for f in (F.DENS, F.VX, F.VY, F.VZ, F.PRESSURE)), b.get(F.OBS))
        assert same(r["values"], whole) and same(r["x_profile"], profile), step
    rows = a.monitor_log()
    assert rows.shape == (4, 57) and same(rows, np.array(want)), (rows, want)
    assert np.all(np.isnan(rows[:, 17 + 15:])) and not np.any(np.isnan(rows[:, :17 + 15]))
    assert rows[3, 1] == (~mask[1:-1, 1:-1, 1:-1]).sum() and rows[3, 2] == 0 and rows[3, 9] > 0
    rows = c.monitor_log()
    assert rows.shape == (2, 57) and same(rows, np.array([want[0], want[2]]))
    for h in (a, b, c):
        h.close()


def test_ring_behaviour():
    import fluid_simulation_amd as F
    sim = sim_of(13, 7, 5, acc=4, monitor_log=2)
    for _ in range(5):
        sim.run_one()
    n, dropped = C.c_long(), C.c_long()
    assert sim._L.fs_monitor_log(sim._h, None, 0, C.byref(n), C.byref(dropped)) == 0       # rows = NULL: reports, drains nothing
    assert (n.value, dropped.value) == (2, 3)
    buf = np.zeros((2, 57))
    assert sim._L.fs_monitor_log(sim._h, buf.ctypes.data, 1, C.byref(n), C.byref(dropped)) == F._lib.EINVAL   # too small
    assert (n.value, dropped.value) == (2, 3) and b"fs_monitor_log" in sim._L.fs_last_error()
    rows, dropped = sim.monitor_log(with_dropped=True)
    assert dropped == 3 and [int(r[0]) for r in rows] == [4, 5]
    assert same(rows[1, 1:17], sim.flow_monitor()["values"])
    rows, dropped = sim.monitor_log(with_dropped=True)      # a drain empties the log
    assert len(rows) == 0 and dropped == 0
    sim.run_one()
    assert [int(r[0]) for r in sim.monitor_log()] == [6]
    sim.set_option("monitor_log", 0)
    with pytest.raises(F.FluidsimError) as e:
        sim.monitor_sample()
    assert e.value.code == F._lib.EINVAL and "monitor_log" in str(e.value)
    sim.run_one()
    assert len(sim.monitor_log()) == 0
    for bad in ("-1", "1048577", "", "3x"):
        with pytest.raises(F.FluidsimError) as e:
            sim.set_option("monitor_log", bad)
        assert e.value.code == F._lib.EINVAL, bad
    for bad in ("0", "-2", "", "x"):
        with pytest.raises(F.FluidsimError) as e:
            sim.set_option("monitor_every", bad)
        assert e.value.code == F._lib.EINVAL, bad
    sim.close()


def test_stations():
    import fluid_simulation_amd as F
    W, H, D = 33, 16, 12
    sim = sim_of(W, H, D, acc=4, monitor_log=4, monitor_stations="1,33,10")
    sim.set_mask(ball_mask(W, H, D, 10, 8, 6, 3))
    sim.run_one()
    sim.run_one()
    prof = sim.flow_monitor(x_profile=True)["x_profile"]
    rows = sim.monitor_log()
    assert len(rows) == 2
    for k, x in enumerate((1, 33, 10)):
        assert same(rows[1, 17 + 5 * k:22 + 5 * k], prof[x - 1]), x
    assert np.all(np.isnan(rows[:, 32:]))
    assert rows[1, 17] == H * D and rows[1, 17 + 10] < H * D                  # cells of a clear plane, and of one through the ball
    sim.run_one()
    sim.set_option("monitor_stations", "5")                  # changing the stations clears the log
    assert sim._geti("monitor_stations") == 1 and len(sim.monitor_log()) == 0
    sim.monitor_sample()
    rows = sim.monitor_log()
    assert len(rows) == 1 and rows[0, 0] == 3 and same(rows[0, 17:22], sim.flow_monitor(x_profile=True)["x_profile"][4])
    assert np.all(np.isnan(rows[0, 22:]))
    for bad in ("0", str(W + 1), "1,2,3,4,5,6,7,8,9", "junk", "1,,2", "1,", "-3", "2;3"):
        with pytest.raises(F.FluidsimError) as e:
            sim.set_option("monitor_stations", bad)
        assert e.value.code == F._lib.EINVAL and "monitor_stations" in str(e.value), bad
        assert sim._geti("monitor_stations") == 1
    sim.set_option("monitor_stations", "1,2,3,4,5,6,7,8")
    assert sim._geti("monitor_stations") == 8
    sim.monitor_sample()
    assert not np.any(np.isnan(sim.monitor_log()))
    sim.set_option("monitor_stations", "")
    assert sim._geti("monitor_stations") == 0
    sim.monitor_sample()
    assert np.all(np.isnan(sim.monitor_log()[0, 17:]))
    sim.close()


# ---- 4. derived values -------------------------------------------------------------------------------------------------------

def test_cfl_is_dt_times_cells_times_the_largest_speed():
    import fluid_simulation_amd as F
    W, H, D = 24, 20, 12
    sim = sim_of(W, H, D, acc=6, dt=0.03)
    mask = ball_mask(W, H, D, 8, 10, 6, 3)
    sim.set_mask(mask)
    for _ in range(3):
        sim.run_one()
    r = sim.flow_monitor()
    dt = float(np.float32(0.03))
    assert float(sim.dt) == dt
    t = ~mask[1:-1, 1:-1, 1:-1]
    want = tuple((dt * n) * float(np.abs(sim.get(f)[1:-1, 1:-1, 1:-1].astype(np.float64))[t].max())
                 for f, n in ((F.VX, W), (F.VY, H), (F.VZ, D)))
    assert r["cfl"] == want and r["cfl"] == M.cfl(0.03, (W, H, D), r["values"]) and want[0] > 0
    h = 1.0 / float(np.cbrt(float(W * H * D)))
    assert r["kinetic_energy"] == 0.5 * r["sum_e"] * (h * h * h) and r["kinetic_energy"] > 0
    sim.close()


# ---- 5. refusals -------------------------------------------------------------------------------------------------------------

def test_fsnull_slab_handle_refuses():
    import fluid_simulation_amd as F
    sim = F.Simulation(16, 16, 16, 1, quiet=1)
    sim.comm_init(0, 2, b"FSNULL:".ljust(128, b"\0"))
    for call in (sim.flow_monitor, sim.monitor_sample, sim.monitor_log, lambda: sim.set_option("monitor_log", 4),
                 lambda: sim.set_option("monitor_every", 2), lambda: sim.set_option("monitor_stations", "3")):
        with pytest.raises(F.FluidsimError) as e:
            call()
        assert e.value.code == -1 and "single-GPU" in str(e.value)
    # the other order: a handle with the log on cannot become a slab
    sim = F.Simulation(16, 16, 16, 1, quiet=1, monitor_log=4)
    with pytest.raises(F.FluidsimError) as e:
        sim.comm_init(0, 2, b"FSNULL:".ljust(128, b"\0"))
    assert e.value.code == -1 and "monitor_log" in str(e.value)
    sim.set_option("monitor_log", 0)
    sim.comm_init(0, 2, b"FSNULL:".ljust(128, b"\0"))


def test_sample_with_the_log_off_is_refused():
    import fluid_simulation_amd as F
    sim = sim_of(8, 6, 5)
    with pytest.raises(F.FluidsimError) as e:
        sim.monitor_sample()
    assert e.value.code == F._lib.EINVAL and "monitor_log" in str(e.value)
    assert sim._L.fs_flow_monitor(sim._h, None, None, None) == F._lib.EINVAL
    assert len(sim.monitor_log()) == 0 and sim.timing("monitor")[1] == 0
    sim.close()


# ---- 6. simulation.out --monitor ---------------------------------------------------------------------------------------------

def test_cli_monitor_csv_reads_back_exactly(tmp_path):
    import fluid_simulation_amd as F
    exe = os.path.join(ROOT, "simulation.out")
    assert os.path.exists(exe), "simulation.out is built by __graft_entry__.build()"
    stl = os.path.join(GOLDEN, "sphere_24x12.stl")
    csv = tmp_path / "f.csv"
    env = {k: v for k, v in os.environ.items() if not k.startswith("FS_")}
    subprocess.run([exe, "--grid", "32x16x16", "--steps", "4", "--stl", stl + ",0.5,0,0,0,-4,0,0", "--dump-every", "0", "--quiet",
                    "--monitor", str(csv), "--monitor-stations", "2,31"], check=True, cwd=str(tmp_path), env=env, timeout=600)
    sim = F.Simulation(32, 16, 16, 4, quiet=1, dump_every=0, monitor_log=4, monitor_stations="2,31")
    assert F.loadSTLIntoObstacles(stl, sim, 0.5, 0.0, 0.0, 0.0, -4.0, 0.0, 0.0) > 0
    sim.run()
    sim.sync()
    rows = sim.monitor_log()
    sim.close()
    assert rows.shape == (4, 57) and list(rows[:, 0]) == [1, 2, 3, 4] and rows[3, 1] < 32 * 16 * 16
    lines = csv.read_text().splitlines()
    assert lines[0].split(",") == list(F.MONITOR_LOG_NAMES) + ["cfl_x", "cfl_y", "cfl_z"]
    got = np.array([[float(t) for t in line.split(",")] for line in lines[1:]])
    assert got.shape == (4, 60) and same(got[:, :57], rows)
    assert np.all(np.isnan(got[:, 27:57])) and not np.any(np.isnan(got[:, :27]))
    for i in range(4):
        assert tuple(got[i, 57:]) == M.cfl(0.05, (32, 16, 16), rows[i, 1:17]), i
    # --monitor-every, through the environment; a station the option refuses is refused here too
    env2 = dict(env, FS_MONITOR=str(tmp_path / "g.csv"), FS_MONITOR_EVERY="3")
    subprocess.run([exe, "--grid", "32x16x16", "--steps", "4", "--stl", stl + ",0.5,0,0,0,-4,0,0", "--dump-every", "0", "--quiet"],
                   check=True, cwd=str(tmp_path), env=env2, timeout=600)
    g = (tmp_path / "g.csv").read_text().splitlines()
    assert [ln.split(",")[0] for ln in g[1:]] == ["1", "4"] and g[1].split(",")[:17] == lines[1].split(",")[:17]
    r = subprocess.run([exe, "--grid", "32x16x16", "--steps", "1", "--stl", "none", "--dump-every", "0", "--quiet", "--monitor",
                        str(tmp_path / "h.csv"), "--monitor-stations", "33"], cwd=str(tmp_path), env=env, timeout=600,
                       capture_output=True, text=True)
    assert r.returncode != 0 and "monitor_stations" in r.stderr
