"""The inflow generator on the MI355X (option "inflow", fs_inflow_profile / _gust / _plane / _eddies), through the C ABI via the
Python mirror: the two kernels against the numpy restatement of include/fluidsim.h (tests/inflow_model.py) on planes that
take every path of the patch and tile loops, the plane a step writes, the neutral setting, "off means off", the query's side
effects, the gust against the flow monitor, the refusals, simulation.out --inflow-* and the stream's statelessness.  Every
comparison is bit for bit."""
import itertools
import os
import subprocess

import numpy as np
import pytest

import inflow_model as M
from conftest import ROOT, ball_mask, bits_equal

pytestmark = pytest.mark.gpu
FAMILIES = ["sweep", "sweep_pair", "sweep_triple", "divergence", "gradient", "advect", "bounds", "misc", "comm", "multigrid",
            "forces", "residual", "flow_stats", "vortex", "probes", "body_forces", "images", "tracers", "volume", "confinement",
            "monitor"]
SIGMAS = [1.0, 2.5, 8.0, 40.0]                       # 40: every eddy touches every cell of every plane here
CONVECTS = [0.0, 0.3, 7.75, 1000.5]                  # frozen, slow, crossing a rebirth, many rebirths per step
STEPS = [0, 1, 17, 10 ** 6]
COUNTS = [1, 63, 64, 65, 257, 1000]
SPEED = 30


def sim_of(W, H, D, precision="fp32", **kw):
    import fluid_simulation_amd as F
    kw.setdefault("quiet", 1)
    kw.setdefault("dump_every", 0)
    return F.Simulation(W, H, D, 1, speed=SPEED, precision=precision, **kw)


def same(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and bool(np.array_equal(a.view(np.uint64), b.view(np.uint64)))


def rough_map(rng, d, h):
    """+-0, huge and tiny magnitudes, ordinary numbers"""
    m = rng.standard_normal((d, h)) * 10.0 ** rng.integers(-30, 30, size=(d, h))
    m.flat[rng.integers(0, m.size)] = -0.0
    m.flat[rng.integers(0, m.size)] = 0.0
    return m


def check_case(sim, H, D, seed, n, sigma, c, t, U, r, gust, context):
    p = M.Params(seed, n, H, D, sigma, c, 1.5)
    sim.set_inflow(profile=U, rms=r, gust=gust, eddies=n, sigma=sigma, u_rms=1.5, convect=c, seed=seed)
    e, want = sim.inflow_eddies(t), M.eddies(p, t)
    assert e.shape == (n, 6)
    for col, key in enumerate(("ex", "ey", "ez")):
        assert same(e[:, col], want[key]), (context, key)
    assert same(e[:, 3:], want["sign"]), context
    plane = M.plane(p, U, r, gust, t, speed=SPEED)
    assert same(sim.inflow_plane(t), plane), context
    return plane


# ---- 1. the plane and the eddies against the model -----------------------------------------------------------------------

@pytest.mark.parametrize("precision", ["fp32", "fp64"])
@pytest.mark.parametrize("grid", [(3, 1, 1), (4, 3, 2), (5, 7, 5), (8, 65, 3)])
def test_small_planes_on_the_whole_grid(grid, precision):
    """sigma x c x t, the counts cycling so that each sigma meets each of them; maps, none, the mean only; a gust"""
    W, H, D = grid
    rng = np.random.default_rng(H * 1000 + D)
    sim = sim_of(W, H, D, precision)
    gust = [(0, 0.5), (10, 1.75), (100, 0.875), (2000000, 1.0)]
    for i, (sg, c, t) in enumerate(itertools.product(SIGMAS, CONVECTS, STEPS)):
        n = COUNTS[(i + i // 16) % 6]
        kind = i % 3
        U = rough_map(rng, D, H) if kind != 1 else None
        r = rough_map(rng, D, H) if kind == 0 else None
        check_case(sim, H, D, 77 + i, n, sg, c, t, U, r, gust if i % 2 else None, (grid, sg, c, t, n))
    sim.close()


@pytest.mark.parametrize("precision", ["fp32", "fp64"])
@pytest.mark.parametrize("grid", [(6, 130, 6), (3, 16, 70), (7, 33, 260)])
def test_planes_of_several_patches(grid, precision):
    """y across waves and patches, z across several patches; every sigma with every c, t and N cycling"""
    W, H, D = grid
    rng = np.random.default_rng(H * 1000 + D)
    sim = sim_of(W, H, D, precision)
    U, r = rough_map(rng, D, H), rough_map(rng, D, H)
    for i, (sg, c) in enumerate(itertools.product(SIGMAS, CONVECTS)):
        t, n = STEPS[(i + i // 4) % 4], COUNTS[i % 5]                          # up to 257 eddies: the model stays quick
        check_case(sim, H, D, 500 + i, n, sg, c, t, U, r, [(0, 1.0), (17, 0.25)], (grid, sg, c, t, n))
    sim.close()


def test_many_tiles_full_lists_and_empty_patches():
    # 4097 eddies = 17 tiles; at sigma = 40 every patch keeps every eddy, so the list fills and is summed every second tile
    W, H, D = 3, 16, 70
    rng = np.random.default_rng(4097)
    sim = sim_of(W, H, D)
    U, r = rough_map(rng, D, H), rough_map(rng, D, H)
    for sg, c, t, n in ((40.0, 7.75, 17, 4097), (2.5, 0.3, 10 ** 6, 4097), (8.0, 1000.5, 1, 1000)):
        check_case(sim, H, D, 9, n, sg, c, t, U, r, None, (sg, c, t, n))
    plane = check_case(sim, H, D, 9, 4097, 40.0, 0.0, 0, None, None, None, "sigma 40")
    assert np.all(plane[1:] != 0.0)                                           # every eddy touches every cell
    sim.close()
    # one eddy of radius 1 on 33 x 260: 50 of the 51 patches keep nothing
    W, H, D = 7, 33, 260
    sim = sim_of(W, H, D)
    for seed in (1, 2, 3):
        plane = check_case(sim, H, D, seed, 1, 1.0, 0.3, 17, None, None, None, ("one eddy", seed))
        assert np.count_nonzero(plane[1]) <= 4 and np.count_nonzero(plane[0] != float(SPEED)) <= 4
    plane = check_case(sim, H, D, 5, 64, 2.5, 0.3, 17, None, None, None, "64 eddies")
    blocks = plane[1, :256, :32].reshape(16, 16, 2, 16).transpose(0, 2, 1, 3).reshape(32, 256)
    assert np.any(np.all(blocks == 0.0, axis=1)) and np.count_nonzero(plane[1]) > 100   # a patch no eddy touches
    sim.close()


# ---- 2. in the step -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("precision,solver,acc", [("fp32", "jacobi", 6), ("fp64", "jacobi", 6), ("fp32", "gs_lex", 6), ("fp32", "jacobi", 0),
                                                  ("fp64", "gs_lex", 3)])
def test_a_step_writes_the_plane_of_its_step_number(precision, solver, acc):
    """the x = 1 face of the pre-diffusion snapshot v_*_prev, which every one of these modes keeps readable after the step"""
    import fluid_simulation_amd as F
    W, H, D = 8, 65, 19
    rng = np.random.default_rng(65019)
    U = SPEED * (1.0 + 0.2 * rng.standard_normal((D, H)))
    r = 0.1 * SPEED * rng.uniform(0.5, 1.5, size=(D, H))
    gust = [(0, 1.0), (2, 1.5), (5, 0.75)]
    sim = sim_of(W, H, D, precision, solver=solver, acc=acc)
    sim.set_mask(ball_mask(W, H, D, 2, 30, 9, 3))                             # a body that covers inlet cells: they are written too
    sim.set_inflow(profile=U, rms=r, gust=gust, eddies=257, sigma=2.5, u_rms=1.0, seed=12345)
    c = M.auto_convect(sim.dt, W, SPEED)
    assert sim._getf("inflow_convect") == np.float32(c) and c > 0
    p = M.Params(12345, 257, H, D, 2.5, c, 1.0)
    dtype = np.float64 if precision == "fp64" else np.float32
    for t in range(4):
        sim.step()
        want = M.cast(M.plane(p, U, r, gust, t, speed=SPEED), dtype)
        for j, f in enumerate((F.VX_PREV, F.VY_PREV, F.VZ_PREV)):
            got = sim.get(f)[1:D + 1, 1:H + 1, 1]
            assert got.dtype == dtype and bits_equal(np.ascontiguousarray(got), want[j]), (t, j)
        assert sim._geti("inflow_passes") == t + 1
    assert np.isfinite(sim.get(F.VX)).all()
    sim.close()


def test_neutral_setting_is_the_uniform_inlet():
    W, H, D = 24, 20, 12
    mask = ball_mask(W, H, D, 8, 10, 6, 3)
    for precision, solver in (("fp32", "jacobi"), ("fp64", "gs_lex")):
        a, b = sim_of(W, H, D, precision, solver=solver, acc=6, inflow="on"), sim_of(W, H, D, precision, solver=solver, acc=6)
        assert a._geti("inflow") == 1 and b._geti("inflow") == 0
        for h in (a, b):
            h.set_mask(mask)
        for step in range(3):
            a.run_one()
            b.run_one()
            for f in range(11):
                assert bits_equal(a.get(f), b.get(f)), (precision, step, f)
        assert a._geti("inflow_passes") == 3 and b._geti("inflow_passes") == 0
        a.close()
        b.close()


def test_off_means_off():
    W, H, D = 24, 20, 12
    mask = ball_mask(W, H, D, 8, 10, 6, 3)
    rng = np.random.default_rng(3)
    counts, fields = {}, {}
    for how in ("untouched", "off", "on"):
        sim = sim_of(W, H, D, acc=6, profile=1)
        if how != "untouched":
            sim.set_inflow(profile=SPEED * rng.uniform(0.5, 1.0, size=(D, H)), eddies=65, sigma=2.5, u_rms=3.0)
        if how == "off":
            sim.set_option("inflow", "off")
        sim.set_mask(mask)
        for _ in range(3):
            sim.run_one()
        counts[how] = {f: sim.timing(f)[1] for f in FAMILIES + ["inflow"]}
        counts[how]["passes"] = sim._geti("inflow_passes")
        fields[how] = [sim.get(f) for f in range(11)]
        sim.close()
    assert counts["untouched"] == counts["off"], counts
    assert counts["off"]["inflow"] == 0 and counts["off"]["passes"] == 0 and counts["on"]["inflow"] == 3 and counts["on"]["passes"] == 3
    assert counts["on"]["misc"] == counts["off"]["misc"] - 3                   # the uniform inlet's launch went
    for f in FAMILIES:
        if f != "misc":
            assert counts["on"][f] == counts["off"][f], (f, counts)
    for a, b in zip(fields["untouched"], fields["off"]):
        assert bits_equal(a, b)
    assert not bits_equal(fields["on"][1], fields["off"][1])


def test_the_query_changes_nothing_else():
    W, H, D = 12, 20, 18
    sim = sim_of(W, H, D, acc=6, profile=1)
    sim.set_mask(ball_mask(W, H, D, 5, 10, 9, 3))
    sim.run_one()
    sim.set_option("inflow_eddies", 65)
    sim.set_option("inflow_rms", 2.0)
    before = [sim.get(f) for f in range(11)]
    counts = {f: sim.timing(f)[1] for f in FAMILIES + ["inflow"]}
    assert sim._geti("inflow") == 0                                           # the query works with the option off
    plane = sim.inflow_plane(5)
    sim.inflow_eddies(5)
    assert same(plane, M.plane(M.Params(1, 65, H, D, 4.0, M.auto_convect(sim.dt, W, SPEED), 2.0), None, None, None, 5, speed=SPEED))
    after = {f: sim.timing(f)[1] for f in FAMILIES + ["inflow"]}
    assert after["inflow"] == counts["inflow"] + 2 and all(after[f] == counts[f] for f in FAMILIES), (counts, after)
    for f in range(11):
        assert bits_equal(sim.get(f), before[f]), f
    assert sim._geti("inflow_passes") == 0
    sim.close()


# ---- 3. the gust and the flow monitor -----------------------------------------------------------------------------------------

def test_the_inlet_mass_flux_follows_the_gust():
    """No eddies: the face a step writes is g(t) * U.  The monitor's profile row of x = 1 sums u over the fluid cells there; U in
    quarters and g in halves make every partial sum exact, so the sum's order does not matter and the flux must be g(t) times
    the sum of U over the fluid inlet cells exactly.  The monitor reads v_x, so the face is taken from the snapshot a step
    keeps and put into a second handle with the same body."""
    import fluid_simulation_amd as F
    W, H, D = 6, 9, 7
    rng = np.random.default_rng(97)
    U = rng.integers(40, 160, size=(D, H)) * 0.25
    gust = [(0, 0.5), (2, 1.5), (4, 1.0)]
    mask = np.zeros((D + 2, H + 2, W + 2), dtype=bool)
    mask[2:4, 3:6, 1:3] = True                                                # a block on the inlet face
    a, b = sim_of(W, H, D, "fp64", acc=4), sim_of(W, H, D, "fp64", acc=4)
    for h in (a, b):
        h.set_mask(mask)
    a.set_inflow(profile=U, gust=gust)
    fluid = ~mask[1:D + 1, 1:H + 1, 1]
    assert fluid.sum() == D * H - 6
    for t, g in enumerate((0.5, 1.0, 1.5, 1.25, 1.0, 1.0)):
        a.step()
        vx = b.get(F.VX)
        vx[:, :, 1] = a.get(F.VX_PREV)[:, :, 1]
        b.set(F.VX, vx)
        row = b.flow_monitor(x_profile=True)["x_profile"][0]
        assert row[0] == fluid.sum() and row[1] == g * U[fluid].sum(), (t, row)
    a.close()
    b.close()


# ---- 4. refusals --------------------------------------------------------------------------------------------------------------

def test_refusals_change_nothing():
    import fluid_simulation_amd as F
    EINVAL = F._lib.EINVAL
    W, H, D = 5, 7, 5
    sim = sim_of(W, H, D)
    rng = np.random.default_rng(11)
    U, r = rng.uniform(1, 2, size=(D, H)), rng.uniform(0, 1, size=(D, H))
    gust = [(0, 1.0), (5, 2.0)]
    sim.set_inflow(profile=U, rms=r, gust=gust, eddies=63, sigma=2.5, u_rms=1.5, convect=0.3, seed=5)
    p = M.Params(5, 63, H, D, 2.5, 0.3, 1.5)
    want = M.plane(p, U, r, gust, 3)
    L, h = sim._L, sim._h
    ptr = lambda a: a.ctypes.data
    bad_u = U.copy()
    bad_u[2, 3] = np.nan
    bad_r = r.copy()
    bad_r[0, 0] = np.inf
    out = np.empty(3 * H * D)
    refused = [
        lambda: L.fs_inflow_profile(h, ptr(U), ptr(r), H * D - 1),
        lambda: L.fs_inflow_profile(h, ptr(U), None, H * D + 1),
        lambda: L.fs_inflow_profile(h, ptr(bad_u), ptr(r), H * D),
        lambda: L.fs_inflow_profile(h, None, ptr(bad_r), H * D),
        lambda: L.fs_inflow_gust(h, ptr(np.array([0.0, 5.0, 5.0])), ptr(np.ones(3)), 3),
        lambda: L.fs_inflow_gust(h, ptr(np.array([0.0, 7.0, 5.0])), ptr(np.ones(3)), 3),
        lambda: L.fs_inflow_gust(h, ptr(np.array([0.0, np.nan])), ptr(np.ones(2)), 2),
        lambda: L.fs_inflow_gust(h, ptr(np.arange(2.0)), ptr(np.array([1.0, np.inf])), 2),
        lambda: L.fs_inflow_gust(h, ptr(np.arange(4097.0)), ptr(np.ones(4097)), 4097),
        lambda: L.fs_inflow_gust(h, ptr(np.arange(2.0)), ptr(np.ones(2)), -1),
        lambda: L.fs_inflow_plane(h, 3, ptr(out), out.size - 1),
        lambda: L.fs_inflow_plane(h, -1, ptr(out), out.size),
        lambda: L.fs_inflow_eddies(h, 3, ptr(out), 6 * 62),
    ]
    for k, call in enumerate(refused):
        assert call() == EINVAL and L.fs_last_error(), k
    options = [("inflow_sigma", "0.999"), ("inflow_sigma", "-2"), ("inflow_sigma", "nan"), ("inflow_sigma", "inf"), ("inflow_eddies", "65537"),
               ("inflow_eddies", "-1"), ("inflow_eddies", "1.5"), ("inflow_rms", "-0.5"), ("inflow_rms", "nan"), ("inflow_rms", "1e999"),
               ("inflow_convect", "-1"), ("inflow_convect", "inf"), ("inflow_convect", "fast"), ("inflow_seed", "-3"), ("inflow_seed", "x"),
               ("inflow_seed", "18446744073709551616"), ("inflow", "yes"), ("inflow_sigma", "")]
    for key, value in options:
        with pytest.raises(F.FluidsimError) as e:
            sim.set_option(key, value)
        assert e.value.code == EINVAL, (key, value)
    assert sim._geti("inflow") == 1 and sim._geti("inflow_eddies") == 63 and sim._getf("inflow_sigma") == 2.5
    assert sim._getf("inflow_rms") == 1.5 and sim._getf("inflow_convect") == np.float32(0.3)
    assert same(sim.inflow_plane(3), want)                                    # maps, knots, parameters: all as they were
    assert sim._L.fs_inflow_gust(h, None, None, 0) == 0                       # n = 0 clears the schedule
    assert same(sim.inflow_plane(3), M.plane(p, U, r, None, 3))
    sim.set_option("inflow_seed", "18446744073709551615")
    sim.set_option("inflow_eddies", 65536)                                    # the most there may be
    assert sim.inflow_eddies(0).shape == (65536, 6)
    sim.set_option("inflow_eddies", 0)
    assert sim.inflow_eddies(0).shape == (0, 6) and same(sim.inflow_plane(9)[1:], np.zeros((2, D, H)))
    sim.close()


def test_slab_handles_refuse():
    import fluid_simulation_amd as F
    sim = sim_of(8, 8, 8)
    sim.comm_init(0, 2, b"FSNULL:".ljust(128, b"\0"))
    for call in (lambda: sim.inflow_plane(0), lambda: sim.set_inflow(profile=np.ones((8, 8)))):
        with pytest.raises(F.FluidsimError) as e:
            call()
        assert e.value.code == F._lib.EINVAL and "single-GPU" in str(e.value)
    sim.set_option("inflow", "on")
    with pytest.raises(F.FluidsimError) as e:
        sim.step()
    assert e.value.code == F._lib.EINVAL and "single-GPU" in str(e.value) and sim._geti("inflow_passes") == 0
    sim.close()


# ---- 5. simulation.out and the stream's statelessness -----------------------------------------------------------------------

def test_cli_inflow_writes_the_same_frames(tmp_path):
    import fluid_simulation_amd as F
    exe = os.path.join(ROOT, "simulation.out")
    assert os.path.exists(exe), "simulation.out is built by __graft_entry__.build()"
    W, H, D = 16, 9, 8
    rng = np.random.default_rng(1698)
    U, r = SPEED * rng.uniform(0.4, 1.0, size=(D, H)), rng.uniform(0.5, 2.0, size=(D, H))
    gust = [(0, 0.5), (1, 1.25), (3, 1.0)]
    prof, gfile = tmp_path / "profile.txt", tmp_path / "gust.txt"
    prof.write_text("# the mean map, then the scale\n" + "\n".join(" ".join(repr(float(v)) for v in row) for row in U) + "\n\n" +
                    "\n".join(" ".join(repr(float(v)) for v in row) for row in r) + "\n")
    gfile.write_text("".join("%d %r   # a knot\n" % (t, f) for t, f in gust))
    cli, py = tmp_path / "cli", tmp_path / "py"
    cli.mkdir()
    py.mkdir()
    env = {k: v for k, v in os.environ.items() if not k.startswith("FS_")}
    base = [exe, "--grid", "%dx%dx%d" % (W, H, D), "--stl", "none", "--quiet"]
    subprocess.run(base + ["--steps", "3", "--dump-every", "1", "--dump-dir", str(cli), "--inflow-profile", str(prof), "--inflow-gust",
                           str(gfile), "--inflow-eddies", "65", "--inflow-sigma", "2.5", "--inflow-rms", "3", "--inflow-convect", "1.75",
                           "--inflow-seed", "99"], check=True, cwd=str(tmp_path), env=env, timeout=600)
    sim = F.Simulation(W, H, D, 3, quiet=1, dump_every=1, dump_dir=str(py))
    sim.set_inflow(profile=U, rms=r, gust=gust, eddies=65, sigma=2.5, u_rms=3.0, convect=1.75, seed=99)
    sim.run()
    sim.sync()
    assert sim._geti("inflow_passes") == 3
    # the stream is stateless: a handle that never stepped gives the plane the stepped one is about to write.  simulation.out
    # --resume restores the fields and not the count of completed steps (src/main.cpp says so), so a resumed run takes its
    # eddies from step 0 again; a caller who keeps the count continues the stream, which is what this checks
    fresh = sim_of(W, H, D)
    fresh.set_inflow(profile=U, rms=r, gust=gust, eddies=65, sigma=2.5, u_rms=3.0, convect=1.75, seed=99)
    assert same(fresh.inflow_plane(3), sim.inflow_plane(3)) and not same(fresh.inflow_plane(3), fresh.inflow_plane(0))
    fresh.close()
    sim.close()
    names = sorted(os.listdir(str(py)))
    assert names and names == sorted(os.listdir(str(cli)))
    for name in names:
        a, b = (py / name).read_bytes(), (cli / name).read_bytes()
        assert len(a) >= (W + 2) * (H + 2) * (D + 2) * 4 and a == b, name
    plain = tmp_path / "plain"
    plain.mkdir()
    subprocess.run(base + ["--steps", "3", "--dump-every", "1", "--dump-dir", str(plain)], check=True, cwd=str(tmp_path), env=env, timeout=600)
    assert (plain / "v_y.bin").read_bytes() != (cli / "v_y.bin").read_bytes()      # the flags did something
    # bad files and values are clean errors
    short, junk = tmp_path / "short.txt", tmp_path / "junk.txt"
    short.write_text("1 2 3\n")
    junk.write_text("0 1\n1 fast\n")
    for extra, word in ((["--inflow-profile", str(short)], "height * depth"), (["--inflow-profile", str(tmp_path / "none.txt")], "cannot open"),
                        (["--inflow-gust", str(junk)], "not a number"), (["--inflow-gust", str(short)], "pairs"),
                        (["--inflow-sigma", "0.5"], "inflow_sigma"), (["--inflow-eddies", "70000"], "inflow_eddies")):
        res = subprocess.run(base + ["--steps", "1", "--dump-every", "0"] + extra, cwd=str(tmp_path), env=env, timeout=600,
                             capture_output=True, text=True)
        assert res.returncode in (1, 2) and word in res.stderr, (extra, res.returncode, res.stderr)
