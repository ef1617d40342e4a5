"""Heat and buoyancy on the MI355X (fs_heat_*), through the C ABI via the Python mirror: pass A and pass C against the numpy
restatement of include/fluidsim.h (tests/heat_model.py) on grids where a 4-cells-per-lane, 64-lanes-wide, z-chunked row
kernel can go wrong, pass B against fs_linear_solver + fs_advect on a heat-off handle, a step in mode 2 against the same
calls made by hand, "off means off", the physics of a hot block, the refusals and the temperature as a source.  Every
comparison of numbers is bit for bit."""
import numpy as np
import pytest

import heat_model as M
from conftest import ball_mask, bits_equal

pytestmark = pytest.mark.gpu
# narrower than a lane's four cells and shorter than a chunk; an exact tile of 64 cells x 16 rows x 8 planes; a ragged x quad,
# a third band of rows and a chunk seam (chunks are 8 planes); a row of 130 cells with odd numbers of rows and planes
GRIDS = [(5, 4, 3), (64, 16, 8), (67, 18, 9), (130, 7, 11)]


def sim_of(W, H, D, precision="fp32", **kw):
    import fluid_simulation_amd as F
    kw.setdefault("quiet", 1)
    kw.setdefault("dump_every", 0)
    return F.Simulation(W, H, D, 1, precision=precision, **kw)


def zero_edges(a):
    """the twelve edges of the padded box (ghost in two or three directions) hold 0"""
    g = np.zeros(a.shape, dtype=np.int8)
    g[0] += 1
    g[-1] += 1
    g[:, 0] += 1
    g[:, -1] += 1
    g[:, :, 0] += 1
    g[:, :, -1] += 1
    a = a.copy()
    a[g >= 2] = 0
    return a


def masks(W, H, D):
    """name -> (padded boolean mask, the box of the wall heating or None = the whole domain)"""
    cx, cy, cz = (W + 1) // 2, (H + 1) // 2, (D + 1) // 2
    none = np.zeros((D + 2, H + 2, W + 2), dtype=bool)
    out = {"empty": (none, None)}
    m = none.copy()
    m[cz, cy, min(3, W)] = True
    out["one voxel"] = (m, None)
    m = none.copy()
    m[1:min(2, D) + 1, 1:min(2, H) + 1, 2:min(4, W) + 1] = True
    out["block on the y = 1 wall"] = (m, None)
    m = none.copy()
    m[1:min(2, D) + 1, 2:min(3, H) + 1, 2:min(3, W) + 1] = True
    m[D, H, W] = True
    out["two blocks, the box takes one"] = (m, (1, max(1, min(4, W - 2)), 1, min(4, H), 1, min(3, D)))
    m = none.copy()
    m[cz, cy, 1] = True
    out["a solid cell on the inlet plane"] = (m, None)
    return out


def random_field(rng, shape, dtype):
    a = (rng.standard_normal(shape) * 10.0 ** rng.integers(-2, 2)).astype(dtype)
    a[rng.random(shape) < 0.03] = dtype(-0.0)
    return zero_edges(a)


def load(sim, rng, mask):
    """seeded random theta, velocities and density into `sim`; -> (theta, [u, v, w], dens, obs)"""
    import fluid_simulation_amd as F
    sim.set_mask(mask)
    shape = mask.shape
    theta, u, v, w, dens = (random_field(rng, shape, sim.dtype) for _ in range(5))
    sim.set_temperature(theta)
    for f, a in ((F.VX, u), (F.VY, v), (F.VZ, w), (F.DENS, dens)):
        sim.set(f, a)
    return theta, [u, v, w], dens, sim.get(F.OBS)


# ---- 1. pass A against the model -------------------------------------------------------------------------------------------

@pytest.mark.parametrize("precision", ["fp32", "fp64"])
@pytest.mark.parametrize("grid", GRIDS)
def test_pass_a_matches_the_model(grid, precision):
    import fluid_simulation_amd as F
    W, H, D = grid
    sim = sim_of(W, H, D, precision)
    rng = np.random.default_rng([W, H, D, 1])
    moved = held = 0
    for i, (name, (mask, box)) in enumerate(masks(W, H, D).items()):
        for up in list(range(6)) + [None]:
            if up is None:                                   # no buoyancy: the velocities and the density must keep their bits
                par = M.params(mode=1, beta=0.0, alpha=0.0, up=2, inlet=1.5, wall=0.75, box=box, shape=grid)
            else:
                par = M.params(mode=1, beta=0.7, alpha=(0.3 if up != 4 else 0.0), up=up, inlet=(0.0 if up % 3 == 0 else 1.25),
                               wall=(2.5 if (up + i) % 2 == 0 else None), box=box, shape=grid)
            sim.set_heat_params(par)
            theta, vel, dens, obs = load(sim, rng, mask)
            want_t, want_v = M.apply(theta, vel, dens, obs, par, sim.dt)
            before = sim._geti("heat_applies")
            sim.heat_apply()
            assert sim._geti("heat_applies") == before + 1
            got_t = sim.temperature()
            assert bits_equal(got_t, want_t), (grid, precision, name, up, np.argwhere(got_t != want_t)[:4])
            for f, want in zip((F.VX, F.VY, F.VZ), want_v):
                got = sim.get(f)
                assert bits_equal(got, want), (grid, precision, name, up, F.FIELD_NAMES[f], np.argwhere(got != want)[:4])
            assert bits_equal(sim.get(F.DENS), dens), (name, up)
            if up is None:
                for f, a in zip((F.VX, F.VY, F.VZ), vel):
                    assert bits_equal(sim.get(f), a), (name, F.FIELD_NAMES[f])
            else:
                moved += int((want_v[up >> 1] != vel[up >> 1]).sum())
            held += int(M.held_cells(obs, par).sum())
    assert moved > 0 and (held > 0 or W * H * D < 100), "the force should move something, the wall hold something"
    sim.close()


# ---- 2. pass B is the existing arithmetic ----------------------------------------------------------------------------------

# dt = 2^-4 and kappa = 2^-10 make a = dt * kappa * w * h * d and c = 1 + 6 a exact in fp32, so the float arguments of
# fs_linear_solver carry the very numbers fs_heat_transport computes in either precision
@pytest.mark.parametrize("precision", ["fp32", "fp64"])
@pytest.mark.parametrize("solver", ["jacobi", "gs_lex", "rbsor"])
@pytest.mark.parametrize("grid", [(5, 4, 3), (67, 18, 9)])
def test_pass_b_is_solver_plus_advection(grid, solver, precision):
    import fluid_simulation_amd as F
    W, H, D = grid
    kappa, dt = 2.0 ** -10, 0.0625
    a = dt * kappa * W * H * D
    c = 1.0 + 6.0 * a
    assert float(np.float32(a)) == a and float(np.float32(c)) == c
    mask = masks(W, H, D)["block on the y = 1 wall"][0]
    rng = np.random.default_rng([W, H, D, 2])
    for acc in (1, 4, 7):
        sim = sim_of(W, H, D, precision, solver=solver, acc=acc, dt=dt)
        ref = sim_of(W, H, D, precision, solver=solver, acc=acc, dt=dt)
        sim.set_heat_params(M.params(mode=1, kappa=kappa, shape=grid))
        theta, vel, dens, _ = load(sim, rng, mask)
        vel = [0.2 * v for v in vel]                         # back-traces of a few cells
        ref.set_mask(mask)
        for f, arr in zip((F.VX, F.VY, F.VZ), vel):
            sim.set(f, arr)
            ref.set(f, arr)
        ref.set(F.DENS, theta)
        ref.set(F.BUFFER, theta)
        ref.linear_solver(0, F.DENS, F.BUFFER, a, c)
        ref.advect(0, F.BUFFER, F.DENS)
        sim.heat_transport()
        assert sim._geti("heat_transports") == 1
        got, want = sim.temperature(), ref.get(F.BUFFER)
        assert bits_equal(got, want), (grid, solver, precision, acc, np.argwhere(got != want)[:4])
        assert not bits_equal(got, theta)
        for f, arr in zip((F.VX, F.VY, F.VZ), vel):
            assert bits_equal(sim.get(f), arr.astype(sim.dtype))
        sim.close()
        ref.close()


# ---- 3. a step in mode 2 = the same calls by hand in mode 1 -------------------------------------------------------------------

@pytest.mark.parametrize("confinement", [0.0, 0.5])
@pytest.mark.parametrize("precision,solver", [("fp32", "jacobi"), ("fp64", "jacobi"), ("fp32", "gs_lex"), ("fp32", "rbsor"), ("fp32", "mg")])
def test_step_in_mode_2_is_the_calls_by_hand(precision, solver, confinement):
    import fluid_simulation_amd as F
    W, H, D = 24, 20, 12
    mask = ball_mask(W, H, D, 8, 10, 6, 3)
    a = sim_of(W, H, D, precision, solver=solver, acc=6, vorticity_confinement=confinement)
    b = sim_of(W, H, D, precision, solver=solver, acc=6)
    kw = dict(kappa=0.01, beta=0.8, alpha=0.2, up="+y", inlet=0.5, wall=1.0)
    a.set_heat(in_step=True, **kw)
    b.set_heat(in_step=False, **kw)
    rng = np.random.default_rng(3)
    dens = zero_edges(np.abs(rng.standard_normal(mask.shape)).astype(a.dtype))
    for h in (a, b):
        h.set_mask(mask)
        h.set(F.DENS, dens)
        h.set(F.BUFFER, dens)
    for step in range(3):
        a.step()
        if confinement:
            b.confine_vorticity(confinement)
        b.heat_apply()
        b.step()
        b.heat_transport()
        assert bits_equal(a.temperature(), b.temperature()), (step, "theta")
        for f in (F.VX, F.VY, F.VZ, F.DENS, F.PRESSURE):
            assert bits_equal(a.get(f), b.get(f)), (step, F.FIELD_NAMES[f])
    assert a._geti("heat_applies") == 3 and a._geti("heat_transports") == 3
    t = a.temperature()
    assert t.max() > 0 and np.count_nonzero(t) > 500, "the wall and the inlet should have heated something"
    a.close()
    b.close()


# ---- 4. off means off ----------------------------------------------------------------------------------------------------

def test_off_means_off():
    import fluid_simulation_amd as F
    W, H, D = 24, 20, 12
    mask = ball_mask(W, H, D, 8, 10, 6, 3)
    fields = {}
    for how in ("untouched", "neutral"):
        sim = sim_of(W, H, D, acc=6, profile=1)
        if how == "neutral":                                 # theta = 0 stays 0 and moves nothing
            sim.set_heat(kappa=0.01, beta=0.0, alpha=0.0, inlet=0.0, wall=None, in_step=True)
        sim.set_mask(mask)
        for _ in range(3):
            sim.run_one()
        fields[how] = [sim.get(f) for f in range(11)]
        launches = sim.timing("heat")[1]
        assert launches == (3 if how == "neutral" else 0), (how, launches)
        if how == "neutral":
            assert not sim.temperature().any()
            sim.sample_points([[2.0, 2.0, 2.0]])
            assert sim.sample(F.SOURCE_HEAT, "nearest")[0] == 0.0
            sim.heat_off()
            assert sim._geti("heat_mode") == 0
            for call in (lambda: sim.sample(F.SOURCE_HEAT, "nearest"), lambda: sim.image_values(F.SOURCE_HEAT, "slice", 2, 1),
                         lambda: sim.isosurface(F.SOURCE_HEAT, 0.5), sim.temperature, sim.heat_apply):
                with pytest.raises(F.FluidsimError) as e:
                    call()
                assert e.value.code == F._lib.EINVAL and "heat is off" in str(e.value)
            sim.run_one()                                    # and the handle goes on as one that never heard of heat
        sim.close()
    for f, (x, y) in enumerate(zip(fields["untouched"], fields["neutral"])):
        assert bits_equal(x, y), F.FIELD_NAMES[f]


# ---- 5. pass C against the model ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("precision", ["fp32", "fp64"])
@pytest.mark.parametrize("grid", GRIDS)
def test_pass_c_matches_the_model(grid, precision):
    W, H, D = grid
    sim = sim_of(W, H, D, precision)
    rng = np.random.default_rng([W, H, D, 5])
    for name, (mask, box) in masks(W, H, D).items():
        par = M.params(mode=1, kappa=0.01, wall=(None if name == "one voxel" else 1.0), box=box, shape=grid)
        sim.set_heat_params(par)
        theta, vel, _, obs = load(sim, rng, mask)
        want, want_planes = M.budget(theta, vel[0], obs, par)
        got = sim.heat_budget(per_plane=True)
        assert bits_equal(got["per_plane"], want_planes), (grid, precision, name, np.argwhere(got["per_plane"] != want_planes)[:4])
        assert bits_equal(got["values"], want), (grid, precision, name, got["values"], want)
        assert bits_equal(sim.temperature(), theta)          # a query changes nothing
    sim.close()


@pytest.mark.parametrize("precision", ["fp32", "fp64"])
def test_logged_records_match_the_model(precision):
    import fluid_simulation_amd as F
    W, H, D = 67, 18, 9
    mask, box = masks(W, H, D)["two blocks, the box takes one"]
    sim = sim_of(W, H, D, precision, acc=4)
    sim.set_mask(mask)
    sim.set_heat(kappa=0.01, beta=0.5, inlet=0.25, wall=1.0, box=box, log=8, in_step=True)
    par = sim.heat_params()
    rows = []
    for step in range(3):
        sim.step()
        whole, _ = M.budget(sim.temperature(), sim.get(F.VX), sim.get(F.OBS), par)
        rows.append(M.log_row(step + 1, whole))
    got, dropped = sim.heat_log(with_dropped=True)
    assert dropped == 0 and got.shape == (3, F.HEAT_LOG_COLS)
    assert bits_equal(got, np.array(rows)), (got, rows)
    assert got[2][1 + M.C_HELD] > 0 and got[2][1 + M.C_LOSS] != 0 and got[2][1 + M.C_IN] != 0
    assert sim.heat_log().shape == (0, F.HEAT_LOG_COLS)      # drained
    sim.close()


# ---- 6. physics ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("precision", ["fp32", "fp64"])
def test_a_hot_block_drives_a_plume(precision):
    """speed = 0, a 6 x 2 x 6 block whose walls are held at theta_w = 1, up = +y, 5 steps.
    The bound on max theta: theta_w is stored exactly; the exact update of a Jacobi sweep, (rhs + a * S) / (1 + 6 a) with S the
    sum of six neighbours, and the exact trilinear interpolation are means of non-negative values with weights that add up to
    at most 1, so neither can exceed the largest value it reads, and every rounded operation multiplies that bound by at most
    (1 + eps), eps the unit roundoff.  Roundings on the longest path of one sweep: 5 additions in S, the product with a, the
    addition of rhs, the product with 1 / c = 8, and 1 / c itself is off by 3 more (6 * a, 1 + ., the division): 11.  Of one
    advection: three levels of c * (1 - s) + c' * s, each (1 - s), a product and the sum = 9.  Pass A writes theta_w and 0
    exactly.  So N = steps * (11 * acc + 9)."""
    import fluid_simulation_amd as F
    W, H, D, acc, steps, theta_w = 24, 24, 12, 4, 5, 1.0
    mask = np.zeros((D + 2, H + 2, W + 2), dtype=bool)
    mask[4:10, 8:10, 10:16] = True
    above = np.zeros(mask.shape, dtype=bool)
    above[4:10, 11:21, 10:16] = True

    def run(beta, alpha, blob):
        sim = sim_of(W, H, D, precision, acc=acc)
        sim.speed = 0
        sim.set_mask(mask)
        sim.set_heat(kappa=2e-3, beta=beta, alpha=alpha, up="+y", wall=(theta_w if beta else None), in_step=True)
        if blob:
            q = np.zeros(mask.shape, dtype=sim.dtype)
            q[4:10, 12:17, 10:16] = 1.0
            sim.set(F.DENS, q)
            sim.set(F.BUFFER, q)
        for _ in range(steps):
            sim.step()
        out = sim.temperature(), sim.get(F.VY), sim.get(F.DENS)
        sim.close()
        return out

    theta, vy, _ = run(4.0, 0.0, False)
    rise = float(vy[above].astype(np.float64).sum())
    print("sum of v_y above the block %.6e, max theta %.17g" % (rise, float(theta.max())))
    assert rise > 0
    assert theta.min() >= 0                                  # sums and products of non-negatives never round below zero
    eps = 2.0 ** -24 if precision == "fp32" else 2.0 ** -53
    assert float(theta.max()) <= theta_w * (1.0 + eps) ** (steps * (11 * acc + 9))
    theta0, vy0, _ = run(0.0, 0.0, False)
    assert not vy0.any() and float(vy0[above].astype(np.float64).sum()) == 0.0
    # smoke that weighs: the blob above the block sinks
    _, vy_q, q = run(0.0, 3.0, True)
    assert q.max() > 0
    sink = float(vy_q[above].astype(np.float64).sum())
    print("sum of v_y through the heavy blob %.6e" % sink)
    assert sink < 0


# ---- 7. refusals ----------------------------------------------------------------------------------------------------------------

def test_refusals_leave_the_state_alone():
    import ctypes as C
    import fluid_simulation_amd as F
    EINVAL = F._lib.EINVAL
    W, H, D = 8, 6, 5
    sim = sim_of(W, H, D)
    L, h = sim._L, sim._h

    def refused(rc, word):
        assert rc == EINVAL, rc
        assert word.encode() in L.fs_last_error(), (word, L.fs_last_error())

    # the passes and the accessors in mode 0
    buf = np.zeros(sim.shape, dtype=np.float32)
    out = np.zeros(F.HEAT_COLS)
    refused(L.fs_heat_apply(h), "heat is off")
    refused(L.fs_heat_transport(h), "heat is off")
    refused(L.fs_heat_budget(h, out.ctypes.data, None), "heat is off")
    refused(L.fs_heat_get(h, buf.ctypes.data, buf.size, 4), "heat is off")
    refused(L.fs_heat_set(h, buf.ctypes.data, buf.size, 4), "heat is off")
    assert sim._geti("heat_applies") == 0 and sim._geti("heat_transports") == 0

    sim.set_heat(kappa=0.01, beta=0.5, alpha=0.25, up="-z", inlet=0.5, wall=2.0, box=(2, 7, 1, 6, 2, 4), log=4, in_step=False)
    good = sim.heat_params()
    assert good[0] == 1 and good[4] == 5 and tuple(good[8:14]) == (2, 7, 1, 6, 2, 4) and good[14] == 4
    rng = np.random.default_rng(7)
    theta = rng.standard_normal(sim.shape).astype(np.float32)
    sim.set_temperature(theta)

    def bad(k, v):
        p = good.copy()
        p[k] = v
        return p

    cases = [(bad(0, 3), "mode"), (bad(0, 0.5), "mode"), (bad(1, -1e-9), "kappa"), (bad(2, -1.0), "beta"), (bad(3, -0.5), "alpha"),
             (bad(4, 6), "up"), (bad(4, -1), "up"), (bad(6, 2), "wall mode"), (bad(8, 0), "box x0"), (bad(9, W + 1), "box x1"),
             (bad(10, 7), "box y0"), (bad(12, 4.5), "box z0"), (bad(13, 1), "box z0"), (bad(14, -1), "log"), (bad(14, 2 ** 20 + 1), "log")]
    for k in range(F.HEAT_PARAMS):
        for v in (float("nan"), float("inf"), float("-inf")):
            cases.append((bad(k, v), "par[%d]" % k))
    for p, word in cases:
        refused(L.fs_heat_params(h, p.ctypes.data, p.size), word)
        assert np.array_equal(sim.heat_params(), good), word
    refused(L.fs_heat_params(h, good.ctypes.data, 14), "FS_HEAT_PARAMS")
    refused(L.fs_heat_params(h, good.ctypes.data, 16), "FS_HEAT_PARAMS")
    refused(L.fs_heat_params_get(h, out.ctypes.data, 9), "FS_HEAT_PARAMS")
    refused(L.fs_heat_get(h, buf.ctypes.data, buf.size - 1, 4), "expected")
    refused(L.fs_heat_get(h, buf.ctypes.data, buf.size, 2), "elem_size")
    refused(L.fs_heat_set(h, buf.ctypes.data, buf.size + 1, 4), "expected")
    n, dropped = C.c_long(), C.c_long()
    assert np.array_equal(sim.heat_params(), good) and bits_equal(sim.temperature(), theta)
    # modes 1 and 2 keep theta, the log count too
    sim.set_heat_params(bad(0, 2))
    assert bits_equal(sim.temperature(), theta) and sim._geti("heat_mode") == 2
    assert L.fs_heat_log(h, None, 0, C.byref(n), C.byref(dropped)) == 0 and n.value == 0
    sim.close()


def test_slab_handles_refuse():
    """The FSNULL communicator makes a handle a z-slab handle in one process, as in tests/test_gpu_confine.py."""
    import fluid_simulation_amd as F
    sim = sim_of(8, 8, 8)
    sim.comm_init(0, 2, b"FSNULL:".ljust(128, b"\0"))
    for mode in (1, 2):
        with pytest.raises(F.FluidsimError) as e:
            sim.set_heat(kappa=0.01, in_step=(mode == 2))
        assert e.value.code == F._lib.EINVAL and "single GPU" in str(e.value)
    assert sim._geti("heat_mode") == 0
    for call in (sim.heat_apply, sim.heat_transport, sim.heat_budget, sim.temperature, sim.heat_log):
        with pytest.raises(F.FluidsimError) as e:
            call()
        assert e.value.code == F._lib.EINVAL and "single GPU" in str(e.value), call
    sim.heat_off()                                           # mode 0 is what a slab handle has
    assert sim._geti("heat_applies") == 0
    sim.close()


# ---- 8. the temperature as a source ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("precision", ["fp32", "fp64"])
def test_theta_is_a_source(precision):
    import fluid_simulation_amd as F
    W, H, D = 13, 7, 9
    sim = sim_of(W, H, D, precision)
    sim.set_heat(kappa=0.01, in_step=False)
    rng = np.random.default_rng(8)
    theta = rng.standard_normal(sim.shape).astype(sim.dtype)
    sim.set_temperature(theta)
    z, y, x = (a.ravel() for a in np.mgrid[0:D + 2, 0:H + 2, 0:W + 2])
    sim.sample_points(np.stack([x, y, z], axis=1).astype(np.float64))
    got = sim.sample(F.SOURCE_HEAT, "nearest")
    assert bits_equal(got, theta.astype(np.float64).ravel())
    sim.set(F.BUFFER, theta)
    for axis, index in ((2, 4), (1, 3), (0, 13)):
        img = sim.image_values(F.SOURCE_HEAT, "slice", axis, index)
        assert bits_equal(img, sim.image_values(F.BUFFER, "slice", axis, index)), axis
        want = theta[index] if axis == 2 else theta[:, index, :] if axis == 1 else theta[:, :, index]
        assert img.shape == want.shape and bits_equal(img, want.astype(np.float64)), axis
    verts, faces = sim.isosurface(F.SOURCE_HEAT, 0.25)
    ref_verts, ref_faces = sim.isosurface(F.BUFFER, 0.25)
    assert len(faces) > 0 and np.array_equal(verts, ref_verts) and np.array_equal(faces, ref_faces)
    sim.close()


# ---- 9. simulation.out --heat -----------------------------------------------------------------------------------------------------

def test_cli_heat_writes_the_same_log_and_frames(tmp_path):
    import os
    import subprocess
    import fluid_simulation_amd as F
    from conftest import GOLDEN, ROOT
    exe = os.path.join(ROOT, "simulation.out")
    assert os.path.exists(exe), "simulation.out is built by __graft_entry__.build()"
    stl = os.path.join(GOLDEN, "sphere_24x12.stl")
    env = {k: v for k, v in os.environ.items() if not k.startswith("FS_")}
    log, dump = tmp_path / "heat.csv", tmp_path / "theta.bin"
    subprocess.run([exe, "--grid", "16x8x8", "--steps", "3", "--stl", stl + ",0.25,0,0,0,-2,0,0", "--dump-every", "1", "--dump-dir",
                    str(tmp_path / "cli"), "--quiet", "--heat", "0.01,0.5,0.1", "--heat-up", "+z", "--heat-inlet", "0.25", "--heat-wall",
                    "1.5,1,12,1,8,1,8", "--heat-log", str(log), "--heat-dump", str(dump)], check=True, cwd=str(tmp_path), env=env,
                   timeout=600)
    sim = F.Simulation(16, 8, 8, 3, quiet=1, dump_every=0)
    assert F.loadSTLIntoObstacles(stl, sim, 0.25, 0.0, 0.0, 0.0, -2.0, 0.0, 0.0) > 0
    sim.set_heat(kappa=0.01, beta=0.5, alpha=0.1, up="+z", inlet=0.25, wall=1.5, box=(1, 12, 1, 8, 1, 8), log=3)
    frames = []
    for _ in range(3):
        sim.run_one()
        frames.append(sim.temperature(np.float32).tobytes())
    rows = sim.heat_log()
    sim.close()
    assert dump.read_bytes() == b"".join(frames) and any(np.frombuffer(frames[-1], dtype=np.float32) != 0)
    got = np.loadtxt(str(log), delimiter=",", skiprows=1, ndmin=2)
    assert open(str(log)).readline().strip() == "step," + ",".join(F.HEAT_NAMES)
    assert bits_equal(got, rows)
    # a flag without --heat, and a value fs_heat_params refuses
    r = subprocess.run([exe, "--grid", "16x8x8", "--steps", "1", "--stl", "none", "--dump-every", "0", "--quiet", "--heat-inlet", "1"],
                       cwd=str(tmp_path), env=env, timeout=600, capture_output=True, text=True)
    assert r.returncode != 0 and "--heat" in r.stderr
    r = subprocess.run([exe, "--grid", "16x8x8", "--steps", "1", "--stl", "none", "--dump-every", "0", "--quiet", "--heat", "-1,0,0"],
                       cwd=str(tmp_path), env=env, timeout=600, capture_output=True, text=True)
    assert r.returncode != 0 and "kappa" in r.stderr
