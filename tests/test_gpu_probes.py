"""The point-probe log on the MI355X (fs_set_probes, option "probe_log", fs_probe_sample, fs_probe_log), through the C
ABI via the Python mirror: a record is the stored value of dens, v_x, v_y, v_z and the pressure at each probe cell,
widened to fp64 -- so every comparison is bit for bit against fs_get_field.  Hand-set fields, real runs (rows, no effect
on the run, launch counts), the ring (wrap, sizes-only query, too-small buffer, clearing), the limits, z-slab runs
bit-identical with one GPU, and simulation.out --probes / --probe-log."""
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import GOLDEN, ROOT, ball_mask, bits_equal

pytestmark = pytest.mark.gpu
WORKER = os.path.join(ROOT, "tests", "probes_slab_worker.py")
FAMILIES = ["sweep", "sweep_pair", "sweep_triple", "divergence", "gradient", "advect", "bounds", "misc", "comm", "multigrid",
            "forces", "residual", "flow_stats", "vortex"]


def record_of(sim, cells):
    """what the definition says a record holds: (n, 5) float64"""
    import fluid_simulation_amd as F
    c = np.asarray(cells).reshape(-1, 3)
    return np.stack([sim.get(f).astype(np.float64)[c[:, 2], c[:, 1], c[:, 0]]
                     for f in (F.DENS, F.VX, F.VY, F.VZ, F.PRESSURE)], axis=1)


def tunnel(precision="fp32", **kw):
    import fluid_simulation_amd as F
    W, H, D = 24, 16, 12
    kw.setdefault("quiet", 1)
    kw.setdefault("dump_every", 0)
    # one launch plan whatever the clock says, so that launch counts compare between handles (the bits never depend on it)
    kw.update(sweep_fuse=2, two_sweep_kernel="pair", pair_shape=1)
    sim = F.Simulation(W, H, D, 8, acc=6, precision=precision, **kw)
    sim.set_mask(ball_mask(W, H, D, 8, 8, 6, 3))
    return sim


CELLS = np.array([(8, 8, 6), (4, 8, 6), (1, 1, 1), (24, 16, 12), (0, 0, 0), (25, 17, 13), (0, 5, 3), (25, 5, 3), (7, 0, 2),
                  (7, 17, 2), (9, 9, 0), (9, 9, 13), (12, 8, 6), (14, 9, 7), (8, 8, 6)], dtype=np.intc)   # first: a solid cell; last: a repeat


# ---- 1. hand-set fields ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("precision", ["fp32", "fp64"])
def test_hand_set_fields(precision):
    import fluid_simulation_amd as F
    W, H, D = 9, 7, 5
    rng = np.random.default_rng(3)
    sim = F.Simulation(W, H, D, 1, precision=precision, quiet=1, dump_every=0, probe_log=4)
    cells = np.array([(0, 0, 0), (W + 1, H + 1, D + 1), (1, 1, 1), (W, H, D), (4, 3, 2), (0, 3, 2), (4, 0, 2), (4, 3, 0),
                      (W + 1, 3, 2), (4, H + 1, 2), (4, 3, D + 1), (5, 3, 2)], dtype=np.intc)
    sim.set_probes(cells)
    assert sim.probe_count == len(cells)
    fields = {}
    for f in (F.DENS, F.VX, F.VY, F.VZ, F.PRESSURE):
        fields[f] = (rng.standard_normal((D + 2, H + 2, W + 2)) * 1e3).astype(sim.dtype)
        sim.set(f, fields[f])
    sim.probe_sample()
    fields[F.VY] = -fields[F.VY]
    sim.set(F.VY, fields[F.VY])
    sim.probe_sample()
    log, dropped = sim.probe_log(with_dropped=True)
    assert dropped == 0 and log["step"].dtype == np.int64 and list(log["step"]) == [0, 0]     # no step completed yet
    assert log["values"].shape == (2, len(cells), 5) and log["values"].dtype == np.float64
    want = np.stack([fields[f].astype(np.float64)[cells[:, 2], cells[:, 1], cells[:, 0]]
                     for f in (F.DENS, F.VX, F.VY, F.VZ, F.PRESSURE)], axis=1)
    assert bits_equal(log["values"][1], want)
    want[:, 2] = -want[:, 2]
    assert bits_equal(log["values"][0], want)
    sim.close()


# ---- 2. real runs ------------------------------------------------------------------------------------------------------------

_RUN = {}


def logged_run(precision):
    """8 steps with the log on; the rows, the values fs_get_field gave after each step, the final fields, launch counts"""
    if precision not in _RUN:
        sim = tunnel(precision, probe_log=8, profile=1)
        sim.set_probes(CELLS)
        direct = []
        for k in range(8):
            if k == 2:
                assert sim.timing("probes")[1] == 2
                sim.reset_timing()                                             # the launch plans are chosen by now
            sim.run_one()
            direct.append(record_of(sim, CELLS))
        sim.sync()
        launches = {fam: sim.timing(fam)[1] for fam in FAMILIES + ["probes"]}
        log, dropped = sim.probe_log(with_dropped=True)
        _RUN[precision] = dict(log=log, dropped=dropped, direct=np.stack(direct), launches=launches,
                               fields=[sim.get(f) for f in range(11)])
        sim.close()
    return _RUN[precision]


@pytest.mark.parametrize("precision", ["fp32", "fp64"])
def test_rows_are_the_stored_values_after_each_step(precision):
    run = logged_run(precision)
    assert list(run["log"]["step"]) == list(range(1, 9)) and run["dropped"] == 0
    assert run["log"]["values"].shape == (8, len(CELLS), 5)
    assert bits_equal(run["log"]["values"], run["direct"])
    v = run["log"]["values"]
    assert np.all(v[:, 0, 1:4] == 0.0) and np.all(v[:, 0] == v[:, -1])       # the solid cell holds no velocity; the repeat
    assert abs(v[-1, 1, 4]) > 0 and len(set(v[:, 13, 1])) > 1                  # pressure in front of the ball; a signal in the wake


@pytest.mark.parametrize("precision", ["fp32", "fp64"])
def test_run_is_unchanged_and_launch_counts(precision):
    import fluid_simulation_amd as F
    run = logged_run(precision)
    assert run["launches"]["probes"] == 6                                      # one launch per record (timing reset after two steps)
    off_configs = [dict(), dict(probe_log=8), dict(probe_log=0, probes=True), dict(probe_log=8, probes=True, cleared=True)]
    for cfg in off_configs:
        sim = tunnel(precision, profile=1, **({"probe_log": cfg["probe_log"]} if "probe_log" in cfg else {}))
        if cfg.get("probes"):
            sim.set_probes(CELLS)
        if cfg.get("cleared"):
            sim.set_probes(np.zeros((0, 3), dtype=np.intc))                    # n = 0 is off
        for k in range(8):
            if k == 2:
                assert sim.timing("probes")[1] == 0, cfg
                sim.reset_timing()
            sim.run_one()
        sim.sync()
        assert sim.timing("probes")[1] == 0, cfg
        for fam in FAMILIES:
            assert sim.timing(fam)[1] == run["launches"][fam], (cfg, fam)
        for f in range(11):
            assert bits_equal(sim.get(f), run["fields"][f]), (cfg, F.FIELD_NAMES[f])
        log = sim.probe_log()
        assert len(log["step"]) == 0 and log["values"].shape[0] == 0
        sim.close()


# ---- 3. the ring ---------------------------------------------------------------------------------------------------------------

def test_ring_wraps_and_drains_like_the_force_log():
    import ctypes as C
    import fluid_simulation_amd as F
    run = logged_run("fp32")
    sim = tunnel(probe_log=3)
    sim.set_probes(CELLS)
    for _ in range(8):
        sim.run_one()
    n, dropped = C.c_long(-1), C.c_long(-1)
    L, h = sim._L, sim._h
    cols = 1 + 5 * len(CELLS)
    # rows = NULL reports and drains nothing; a too-small buffer is refused and drains nothing
    assert L.fs_probe_log(h, None, 0, C.byref(n), C.byref(dropped)) == 0 and (n.value, dropped.value) == (3, 5)
    buf = np.full((3, cols), -7.0)
    assert L.fs_probe_log(h, buf.ctypes.data, 2, C.byref(n), C.byref(dropped)) == F._lib.EINVAL
    assert (n.value, dropped.value) == (3, 5) and np.all(buf == -7.0)
    assert L.fs_probe_log(h, None, 0, None, None) == 0
    log, dropped = sim.probe_log(with_dropped=True)
    assert list(log["step"]) == [6, 7, 8] and dropped == 5
    assert bits_equal(log["values"], run["direct"][5:8])
    log, dropped = sim.probe_log(with_dropped=True)                            # drained
    assert len(log["step"]) == 0 and dropped == 0
    sim.run_one()
    sim.probe_sample()
    log, dropped = sim.probe_log(with_dropped=True)
    assert list(log["step"]) == [9, 9] and dropped == 0 and bits_equal(log["values"][0], log["values"][1])
    assert bits_equal(log["values"][1], record_of(sim, CELLS))
    # fs_set_probes and the option clear the log
    sim.run_one()
    sim.set_probes(CELLS[:4])
    assert sim.probe_count == 4 and len(sim.probe_log()["step"]) == 0
    sim.run_one()
    log = sim.probe_log()
    assert list(log["step"]) == [11] and bits_equal(log["values"][0], record_of(sim, CELLS[:4]))
    sim.run_one()
    sim.set_option("probe_log", 5)
    assert len(sim.probe_log()["step"]) == 0
    for _ in range(2):
        sim.run_one()
    assert list(sim.probe_log()["step"]) == [13, 14]
    sim.close()


def test_limits():
    import fluid_simulation_amd as F
    EINVAL = F._lib.EINVAL
    W, H, D = 12, 10, 8
    sim = F.Simulation(W, H, D, 1, quiet=1, dump_every=0)
    L, h = sim._L, sim._h
    many = np.ones((F.PROBE_MAX + 1, 3), dtype=np.intc)
    assert L.fs_set_probes(h, many.ctypes.data, F.PROBE_MAX + 1) == EINVAL
    assert L.fs_set_probes(h, many.ctypes.data, -1) == EINVAL and L.fs_set_probes(h, None, 3) == EINVAL
    assert L.fs_set_probes(h, many.ctypes.data, F.PROBE_MAX) == 0 and sim.probe_count == F.PROBE_MAX
    for bad in ((-1, 1, 1), (W + 2, 1, 1), (1, -1, 1), (1, H + 2, 1), (1, 1, -1), (1, 1, D + 2)):
        with pytest.raises(F.FluidsimError) as e:
            sim.set_probes([(1, 1, 1), bad])
        assert e.value.code == EINVAL
    assert sim.probe_count == F.PROBE_MAX                                      # a refused list replaces nothing
    sim.set_probes([(0, 0, 0), (W + 1, H + 1, D + 1)])                         # the ghost corners are cells
    for bad in ("-1", "1048577", "x", "3.5", ""):
        with pytest.raises(F.FluidsimError):
            sim.set_option("probe_log", bad)
    # N * n * 40 bytes may not exceed 1 GiB, whichever of the two is set last
    sim.set_probes(np.ones((25, 3), dtype=np.intc))
    sim.set_option("probe_log", 1048576)                                       # 1 048 576 000 bytes
    with pytest.raises(F.FluidsimError) as e:
        sim.set_probes(np.ones((26, 3), dtype=np.intc))                        # 1 090 519 040 bytes
    assert e.value.code == EINVAL and sim.probe_count == 25
    sim.set_option("probe_log", 0)
    sim.set_probes(np.ones((26, 3), dtype=np.intc))
    with pytest.raises(F.FluidsimError) as e:
        sim.set_option("probe_log", 1048576)
    assert e.value.code == EINVAL
    sim.set_option("probe_log", 2)
    # fs_probe_sample needs probes and a ring
    sim.probe_sample()
    sim.set_probes(np.zeros((0, 3), dtype=np.intc))
    with pytest.raises(F.FluidsimError):
        sim.probe_sample()
    sim.set_probes([(1, 1, 1)])
    sim.set_option("probe_log", 0)
    with pytest.raises(F.FluidsimError):
        sim.probe_sample()
    assert L.fs_set_probes(None, many.ctypes.data, 1) == EINVAL and L.fs_probe_sample(None) == EINVAL
    assert L.fs_probe_log(None, None, 0, None, None) == EINVAL
    sim.close()


def test_fsnull_slab_handle_refuses():
    import fluid_simulation_amd as F
    sim = F.Simulation(16, 16, 16, 1, quiet=1, dump_every=0, probe_log=2)
    sim.comm_init(0, 2, b"FSNULL:".ljust(128, b"\0"))
    sim.set_probes([(3, 3, 3), (3, 3, 12)])
    sim.probe_sample()
    with pytest.raises(F.FluidsimError) as e:
        sim.probe_log()
    assert e.value.code == -1 and "FSNULL" in str(e.value)
    sim.close()


# ---- 4. z-slabs ----------------------------------------------------------------------------------------------------------------

def ipc_usable():
    exe = os.path.join(ROOT, "tools", "ipc_probe")
    if not os.path.exists(exe):
        return False, "tools/ipc_probe was not built"
    r = subprocess.run([exe, "2", "8", "1"], capture_output=True, text=True, timeout=120,
                       env=dict(os.environ, FS_IPC_TIMEOUT_S="20"))
    return r.returncode == 0, (r.stdout + r.stderr)[-400:]


_SINGLE = {}


def run_ranks(tmp, nranks, transport, W, H, D, steps):
    import fluid_simulation_amd as F
    out = os.path.join(tmp, "%s_n%d" % (transport, nranks))
    os.makedirs(out)
    idfile = os.path.join(out, "id.bin")
    if nranks > 1:
        open(idfile, "wb").write(F.comm_unique_id(transport))
    procs = [subprocess.Popen([sys.executable, WORKER, str(r), str(nranks), idfile, out, str(W), str(H), str(D), str(steps)],
                              env=dict(os.environ, FS_IPC_TIMEOUT_S="60")) for r in range(nranks)]
    for p in procs:
        assert p.wait(timeout=600) == 0
    return [dict(np.load(os.path.join(out, "rank%d.npz" % r))) for r in range(nranks)]


@pytest.mark.parametrize("nranks,transport", [(2, "shm"), (3, "shm"), (4, "shm"), (2, "ipc"), (3, "ipc"), (4, "ipc")])
def test_slabs_bit_identical_with_one_gpu(tmp_path, nranks, transport):
    if transport == "ipc":
        ok, why = ipc_usable()
        if not ok:
            pytest.skip("FSIPC transport not usable on this box: " + why)
    W, H, D, steps = 32, 16, 24, 8
    if "ref" not in _SINGLE:
        _SINGLE["ref"] = run_ranks(str(tmp_path), 1, "single", W, H, D, steps)[0]
    ref = _SINGLE["ref"]
    n = int(ref["count"])
    assert n == 32 and list(ref["step"]) == list(range(1, steps + 1)) + [steps] and int(ref["dropped"]) == 0
    assert ref["values"].shape == (steps + 1, n, 5)
    assert bits_equal(ref["values"][:steps], ref["direct"]) and bits_equal(ref["values"][steps], ref["direct"][-1])
    assert np.count_nonzero(ref["values"][-1]) > n
    Dl = D // nranks
    for r, z in enumerate(run_ranks(str(tmp_path), nranks, transport, W, H, D, steps)):
        assert int(z["zoff"]) == r * Dl and int(z["count"]) == n and int(z["dropped"]) == 0
        assert np.array_equal(z["step"], ref["step"]), r
        assert bits_equal(z["values"], ref["values"]), (r, np.argwhere(z["values"] != ref["values"])[:8])
        assert bits_equal(z["vx"][1:Dl + 1], ref["vx"][r * Dl + 1:r * Dl + Dl + 1]), r       # the run itself is the one-GPU run


# ---- 5. simulation.out --probes / --probe-log ---------------------------------------------------------------------------------------

def test_cli_probe_log_csv_matches_python(tmp_path):
    import fluid_simulation_amd as F
    exe = os.path.join(ROOT, "simulation.out")
    assert os.path.exists(exe), "simulation.out is built by __graft_entry__.build()"
    stl = os.path.join(GOLDEN, "sphere_24x12.stl")
    cells = [(20, 8, 8), (0, 0, 0), (33, 17, 17), (12, 9, 8), (28, 6, 10)]
    probes = tmp_path / "probes.txt"
    probes.write_text("# wake probes\n20 8 8\n0 0 0   # a ghost corner\n\n33 17 17\n  12 9 8\n28\t6 10\n")
    csv = tmp_path / "p.csv"
    env = {k: v for k, v in os.environ.items() if not k.startswith("FS_")}
    subprocess.run([exe, "--grid", "32x16x16", "--steps", "6", "--probes", str(probes), "--probe-log", str(csv), "--stl",
                    stl + ",0.5,0,0,0,-4,0,0", "--dump-every", "0", "--dump-dir", str(tmp_path), "--quiet"], check=True,
                   cwd=str(tmp_path), env=env, timeout=600)
    lines = csv.read_text().splitlines()
    assert lines[0] == "step," + ",".join("q_%d,u_%d,v_%d,w_%d,p_%d" % ((k,) * 5) for k in range(len(cells)))
    got = np.array([[float(v) for v in ln.split(",")] for ln in lines[1:]])
    assert got.shape == (6, 1 + 5 * len(cells))
    sim = F.Simulation(32, 16, 16, 6, quiet=1, dump_every=0, probe_log=6)
    assert F.loadSTLIntoObstacles(stl, sim, 0.5, 0.0, 0.0, 0.0, -4.0, 0.0, 0.0) > 0
    sim.set_probes(cells)
    sim.run()
    log = sim.probe_log()
    assert list(log["step"]) == [1, 2, 3, 4, 5, 6] and np.array_equal(got[:, 0], log["step"])
    assert bits_equal(got[:, 1:].reshape(6, len(cells), 5), log["values"])
    assert np.count_nonzero(log["values"][-1]) > len(cells)
    assert bits_equal(log["values"][-1], record_of(sim, cells))
    # the same through the environment, and a malformed file is refused
    csv2 = tmp_path / "p2.csv"
    subprocess.run([exe, "--grid", "32x16x16", "--steps", "6", "--stl", stl + ",0.5,0,0,0,-4,0,0", "--dump-every", "0",
                    "--dump-dir", str(tmp_path), "--quiet"], check=True, cwd=str(tmp_path), timeout=600,
                   env=dict(env, FS_PROBES=str(probes), FS_PROBE_LOG=str(csv2)))
    assert csv2.read_text() == csv.read_text()
    probes.write_text("1 2\n")
    r = subprocess.run([exe, "--grid", "32x16x16", "--steps", "1", "--probes", str(probes), "--stl", "none", "--dump-every", "0",
                        "--quiet"], cwd=str(tmp_path), env=env, timeout=600, capture_output=True, text=True)
    assert r.returncode != 0 and "x y z" in r.stderr
    sim.close()
