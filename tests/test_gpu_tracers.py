"""Tracer particles on the MI355X (fs_tracer_seed, fs_tracer_emitters, fs_tracer_advance, the move inside fs_step, the snapshot
log), through the C ABI via the Python mirror: every position and meta word is compared bit for bit with
tests/tracers_model.py, the numpy fp64 restatement of the definition in include/fluidsim.h -- hand-set rough fields on fp32
and fp64 handles, real runs with emitters, the pool's slot rule and the ring, fs_tracer_sample against the sampler, the
error cases, simulation.out --tracers and the viewer's streaklines and pathlines.  Two tests do not use the model: a uniform
flow whose every operation is exact, and a rigid rotation that tells the midpoint rule from Euler's.  The pools hold 1000
slots and 777 particles: more than one workgroup, not a multiple of 256."""
import os
import subprocess

import numpy as np
import pytest

import tracers_model as M
from conftest import GOLDEN, ROOT, ball_mask, bits_equal

pytestmark = pytest.mark.gpu
PRECISIONS = ["fp32", "fp64"]
precisions = pytest.mark.parametrize("precision", PRECISIONS)
FAMILIES = ["sweep", "sweep_pair", "sweep_triple", "divergence", "gradient", "advect", "bounds", "misc", "comm", "multigrid",
            "forces", "residual", "flow_stats", "vortex", "probes", "body_forces", "images"]
C, NP = 1000, 777


def sim_of(W, H, D, precision="fp32", **kw):
    import fluid_simulation_amd as F
    kw.setdefault("quiet", 1)
    kw.setdefault("dump_every", 0)
    return F.Simulation(W, H, D, 1, precision=precision, **kw)


def tunnel(precision="fp32", **kw):
    """the 24 x 16 x 12 ball tunnel of test_gpu_probes.py"""
    import fluid_simulation_amd as F
    W, H, D = 24, 16, 12
    kw.setdefault("quiet", 1)
    kw.setdefault("dump_every", 0)
    # one launch plan whatever the clock says, so that launch counts compare between handles (the bits never depend on it)
    kw.update(sweep_fuse=2, two_sweep_kernel="pair", pair_shape=1)
    sim = F.Simulation(W, H, D, 8, acc=6, precision=precision, **kw)
    sim.set_mask(ball_mask(W, H, D, 8, 8, 6, 3))
    return sim


def fields(sim):
    import fluid_simulation_amd as F
    return sim.get(F.VX), sim.get(F.VY), sim.get(F.VZ), sim.get(F.OBS)


def assert_pool(sim, pool, context):
    t = sim.tracers()
    n = pool.count
    assert sim.tracer_count == n and t["xyz"].shape == (n, 3) and t["xyz"].dtype == np.float64
    want = pool.xyz[:n]
    assert M.same_bits(t["xyz"], want), (context, np.flatnonzero(~((t["xyz"] == want) | (np.isnan(t["xyz"]) & np.isnan(want))).all(axis=1))[:8])
    for k, name in enumerate(("status", "source", "born", "moves")):
        assert t[name].dtype == np.int32 and np.array_equal(t[name], pool.meta[:n, k]), (context, name, np.flatnonzero(t[name] != pool.meta[:n, k])[:8])
    return t


def box_points(rng, shape, n):
    lo, hi = np.full(3, 0.5), np.array(shape, dtype=np.float64) + 0.5
    p = lo + rng.random((n, 3)) * (hi - lo)
    pick = rng.integers(0, 12, size=(n, 3))                    # some on the faces, edges and corners of B
    return np.ascontiguousarray(np.where(pick == 0, lo, np.where(pick == 1, hi, p)))


# ---- 1. hand-set rough fields ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("grid", [(9, 7, 5), (16, 16, 4)], ids=lambda g: "x".join(map(str, g)))
@precisions
def test_rough_fields_match_model(grid, precision):
    import fluid_simulation_amd as F
    W, H, D = grid
    rng = np.random.default_rng(W * 100 + D + (precision == "fp64"))
    sim = sim_of(W, H, D, precision, tracers=C)
    assert sim.tracer_capacity == C and sim.tracer_count == 0
    full = (D + 2, H + 2, W + 2)
    k = M.displacement(sim.dt, grid)
    for a, which in enumerate((F.VX, F.VY, F.VZ)):
        f = (rng.standard_normal(full) * 0.6 / k[a]).astype(sim.dtype)
        f[rng.random(full) < 0.1] = 0.0
        f[rng.random(full) < 0.002] = np.nan
        f[rng.random(full) < 0.001] = np.inf
        sim.set(which, f)
    obs = (rng.random(full) < 0.1).astype(sim.dtype)
    obs[rng.random(full) < 0.02] = 0.5                         # neither 0 nor 1: not solid
    sim.set(F.OBS, obs)
    vx, vy, vz, obs = fields(sim)
    pool = M.Pool(C)
    pts = box_points(rng, grid, NP - 12 if W == 16 else NP)
    sim.tracer_seed(pts)
    pool.seed(pts, 0)
    if W == 16:                                                # an explicit advance releases the emitters: 4 x 3 particles
        emit = box_points(rng, grid, 3)
        sim.tracer_emitters(emit, every=5)
        pool.emitters(emit, every=5)
    assert_pool(sim, pool, "seeded")
    for n in range(5):
        if n == 4 and W == 16:
            sim.tracer_emitters([])
            pool.emitters([])
        sim.tracer_advance()
        pool.advance(vx, vy, vz, obs, sim.dt, 0)
        t = assert_pool(sim, pool, (grid, precision, n))
    assert pool.count == NP
    for status in (M.ALIVE, M.OUT, M.HIT):
        assert (t["status"] == status).sum() >= 20, status
    assert np.isnan(t["xyz"]).any() and 0 < t["moves"].min() < t["moves"].max() == 5
    for which, before in ((F.VX, vx), (F.VY, vy), (F.VZ, vz), (F.OBS, obs)):
        assert bits_equal(sim.get(which), before)
    sim.close()


# ---- 2. exact uniform flow (independent of the model) -------------------------------------------------------------------------------

@precisions
def test_uniform_flow_is_exact(precision):
    import fluid_simulation_amd as F
    W, H, D = 16, 16, 4
    sim = sim_of(W, H, D, precision, dt=0.0625, tracers=C)     # k = (1, 1, 0.25)
    full = (D + 2, H + 2, W + 2)
    for which, v in ((F.VX, 0.25), (F.VY, -0.125), (F.VZ, 0.5)):
        sim.set(which, np.full(full, v, dtype=sim.dtype))
    sim.tracer_seed([[2.0, 8.0, 1.5]])
    for _ in range(8):
        sim.tracer_advance()
    t = sim.tracers()
    assert t["xyz"].tolist() == [[4.0, 7.0, 2.5]]
    assert (t["status"][0], t["source"][0], t["born"][0], t["moves"][0]) == (F.TRACER_ALIVE, -1, 0, 8)
    # the same in numpy: every product and sum is exact
    p = np.array([2.0, 8.0, 1.5])
    for _ in range(8):
        p = p + np.array([1.0, 1.0, 0.25]) * np.array([0.25, -0.125, 0.5])
    assert p.tolist() == [4.0, 7.0, 2.5]
    sim.close()


# ---- 3. the midpoint rule, not Euler ----------------------------------------------------------------------------------------------

def test_rotation_is_the_midpoint_rule():
    import fluid_simulation_amd as F
    W, H, D = 16, 16, 4
    theta, n = 0.1, 50
    sim = sim_of(W, H, D, "fp64", dt=0.0625, tracers=C)
    z, y, x = np.mgrid[0:D + 2, 0:H + 2, 0:W + 2].astype(np.float64)
    sim.set(F.VX, -theta * (y - 8.5))
    sim.set(F.VY, theta * (x - 8.5))
    sim.set(F.VZ, np.zeros_like(x))
    sim.tracer_seed([[12.5, 8.5, 2.25]])
    for _ in range(n):
        sim.tracer_advance()
    t = sim.tracers()
    assert t["status"][0] == F.TRACER_ALIVE and t["moves"][0] == n and t["xyz"][0, 2] == 2.25
    ratio = np.hypot(t["xyz"][0, 0] - 8.5, t["xyz"][0, 1] - 8.5) / 4.0
    want = (1.0 + theta ** 4 / 4.0) ** (n / 2.0)
    euler = (1.0 + theta ** 2) ** (n / 2.0)
    print("r / r0 = %.17g, midpoint %.17g (rel %.3g), Euler %.6g" % (ratio, want, abs(ratio / want - 1.0), euler))
    assert abs(ratio / want - 1.0) <= 1e-12
    assert euler > 1.28
    # the angle: n steps of atan2(theta, 1 - theta^2 / 2)
    angle = np.arctan2(t["xyz"][0, 1] - 8.5, t["xyz"][0, 0] - 8.5)
    turn = angle - n * np.arctan2(theta, 1.0 - theta * theta / 2.0)
    assert abs((turn + np.pi) % (2.0 * np.pi) - np.pi) <= 1e-12
    sim.close()


# ---- 4. deaths ---------------------------------------------------------------------------------------------------------------------

@precisions
def test_deaths(precision):
    import fluid_simulation_amd as F
    W, H, D = 24, 16, 12
    sim = tunnel(precision, tracers=C)
    solid = ball_mask(W, H, D, 8, 8, 6, 3)
    vx = np.where(solid, 0.0, 1.0).astype(sim.dtype)           # k_x = 1.2: 1.2 cells per advance
    vy = np.zeros_like(vx)
    vy[9, 12, 20] = np.nan
    sim.set(F.VX, vx)
    sim.set(F.VY, vy)
    sim.set(F.VZ, np.zeros_like(vx))
    pts = np.array([[3.0, 8.0, 6.0],      # driven into the ball
                    [24.0, 3.0, 3.0],     # through the outlet: already the midpoint is outside
                    [23.5, 3.0, 3.0],     # through the outlet: the midpoint is inside, the end point is not
                    [20.0, 12.0, 9.0],    # on a NaN velocity
                    [8.0, 8.0, 6.0],      # seeded inside the ball
                    [3.0, 2.0, 2.0]])     # free stream
    sim.tracer_seed(pts)
    pool = M.Pool(C)
    pool.seed(pts, 0)
    obs = sim.get(F.OBS)
    history = []
    for n in range(6):
        sim.tracer_advance()
        pool.advance(sim.get(F.VX), sim.get(F.VY), sim.get(F.VZ), obs, sim.dt, 0)
        history.append(assert_pool(sim, pool, n))
    first, last = history[0], history[-1]
    assert last["status"].tolist() == [F.TRACER_HIT, F.TRACER_OUT, F.TRACER_OUT, F.TRACER_OUT, F.TRACER_HIT, F.TRACER_ALIVE]
    # into the ball: HIT at the move that ended in a solid cell; the position of that move stays
    hit = [h["status"][0] for h in history].index(F.TRACER_HIT)
    assert hit >= 1 and history[hit]["moves"][0] == hit + 1 == last["moves"][0]
    cell = np.floor(history[hit]["xyz"][0] + 0.5).astype(int)
    assert solid[cell[2], cell[1], cell[0]] and history[hit]["xyz"][0, 0] > history[hit - 1]["xyz"][0, 0]
    assert bits_equal(last["xyz"][0], history[hit]["xyz"][0])
    # the outlet: OUT at the first move, the stored position is outside B, and it stays
    k = M.displacement(sim.dt, (W, H, D))
    assert first["status"][1] == F.TRACER_OUT and first["xyz"][1].tolist() == [24.0 + 0.5 * k[0], 3.0, 3.0]
    assert first["status"][2] == F.TRACER_OUT and first["xyz"][2].tolist() == [23.5 + k[0], 3.0, 3.0]
    assert first["xyz"][1, 0] > W + 0.5 and first["xyz"][2, 0] > W + 0.5
    assert last["moves"][1] == last["moves"][2] == 1 and bits_equal(last["xyz"][1:3], first["xyz"][1:3])
    # NaN: OUT, the NaN is stored
    assert first["status"][3] == F.TRACER_OUT and np.isnan(first["xyz"][3, 1]) and last["moves"][3] == 1
    # inside the ball: HIT after one advance without having moved
    assert first["status"][4] == F.TRACER_HIT and first["xyz"][4].tolist() == [8.0, 8.0, 6.0] and last["moves"][4] == 1
    assert last["moves"][5] == 6 and last["xyz"][5].tolist()[1:] == [2.0, 2.0] and last["xyz"][5, 0] > 10.0
    sim.close()


# ---- 5. real run -------------------------------------------------------------------------------------------------------------------

@precisions
def test_real_run_matches_model_and_changes_nothing(precision):
    import fluid_simulation_amd as F
    from fluid_simulation_amd import viewer
    W, H, D = 24, 16, 12
    sim = tunnel(precision, tracers=C, profile=1)
    ref = tunnel(precision, profile=1)
    emit = viewer.rake((1.0, 3.0, 6.0), (1.0, 13.0, 6.5), 8)
    seeds = np.concatenate([viewer.rake((2.0, 1.0, 1.0), (6.0, 16.0, 12.0), 400), viewer.rake((0.5, 8.0, 0.5), (24.5, 8.5, 12.5), NP - 32 - 400)])
    sim.tracer_emitters(emit, every=2)
    sim.tracer_seed(seeds)
    pool = M.Pool(C)
    pool.emitters(emit, every=2)
    pool.seed(seeds, 0)
    sim.reset_timing()
    ref.reset_timing()
    for step in range(1, 9):
        sim.run_one()
        ref.run_one()
        vx, vy, vz, obs = fields(sim)
        pool.step(vx, vy, vz, obs, sim.dt, step)
        t = assert_pool(sim, pool, (precision, step))
    assert pool.count == NP and sim._geti("tracer_seeded") == NP and sim._geti("tracer_emitters") == 8
    released = t["source"] >= 0
    assert released.sum() == 32 and np.array_equal(t["source"][released], np.tile(np.arange(8), 4))
    assert np.array_equal(t["born"][released], np.repeat([1, 3, 5, 7], 8)) and (t["born"][~released] == 0).all()
    assert np.array_equal(t["moves"][released & (t["status"] == F.TRACER_ALIVE)], 8 - t["born"][released & (t["status"] == F.TRACER_ALIVE)])
    assert (t["status"] == F.TRACER_ALIVE).sum() > 100 and (t["status"] != F.TRACER_ALIVE).sum() > 10
    for f in (F.DENS, F.VX, F.VY, F.VZ, F.PRESSURE):
        assert bits_equal(sim.get(f), ref.get(f)), F.FIELD_NAMES[f]
    for fam in FAMILIES:
        assert sim.timing(fam)[1] == ref.timing(fam)[1], fam
    assert sim.timing("tracers")[1] == 8 and sim.timing("tracers")[0] > 0.0
    assert ref.timing("tracers") == (0.0, 0)                 # the feature off: nothing launched for it
    ref.close()
    sim.close()


# ---- 6. pool and ring --------------------------------------------------------------------------------------------------------------

def test_pool_slots_and_clear():
    import fluid_simulation_amd as F
    sim = sim_of(8, 6, 5, tracers=10)
    pool = M.Pool(10)
    rng = np.random.default_rng(3)
    for n in (7, 6, 0, 25, 10, 1):                             # past the end, more than the pool at once, exactly the pool
        pts = box_points(rng, (8, 6, 5), n).reshape(n, 3)
        sim.tracer_seed(pts)
        pool.seed(pts, 0)
        assert_pool(sim, pool, n)
        assert sim._geti("tracer_seeded") == pool.seeded
    assert sim.tracer_count == 10 and pool.seeded == 49
    sim.tracer_clear()
    pool.clear()
    assert sim.tracer_count == 0 and sim._geti("tracer_seeded") == 0 and sim.tracers()["xyz"].shape == (0, 3)
    sim.tracer_seed([[1.0, 1.0, 1.0]])                         # slot 0 again; the other slots are FREE
    sim.tracer_emitters([[2.0, 2.0, 2.0]] * 9)
    sim.tracer_advance()
    t = sim.tracers()
    assert t["status"].tolist() == [F.TRACER_ALIVE] * 10 and t["source"].tolist() == [-1] + list(range(9))
    sim.tracer_clear()
    sim.set_option("tracer_log", 2)
    sim.tracer_emitters([])
    sim.tracer_advance()
    log = sim.tracer_log()
    assert log["status"].shape == (1, 10) and (log["status"] == F.TRACER_FREE).all() and (log["xyz"] == 0).all()
    sim.close()


def test_log_ring():
    import ctypes as Ct
    import fluid_simulation_amd as F
    W, H, D = 12, 6, 5
    sim = sim_of(W, H, D, acc=2, tracers=40, tracer_log=3)
    emit = np.array([[1.0, 2.0, 2.0], [1.0, 4.5, 3.0], [6.0, 3.0, 3.0]])
    sim.tracer_emitters(emit)
    pools = {}
    for step in range(1, 6):
        sim.run_one()
        pools[step] = sim.tracers()
    n, dropped = Ct.c_long(), Ct.c_long()
    assert sim._L.fs_tracer_log(sim._h, None, None, None, 0, Ct.byref(n), Ct.byref(dropped)) == 0
    assert (n.value, dropped.value) == (3, 2)                # both arrays NULL: the counts only, nothing drained
    xyz = np.zeros((3, 40, 3))
    status = np.zeros((3, 40), dtype=np.int32)
    assert sim._L.fs_tracer_log(sim._h, xyz.ctypes.data, status.ctypes.data, None, 2, Ct.byref(n), None) == F._lib.EINVAL and n.value == 3
    log, dropped = sim.tracer_log(with_dropped=True)
    assert log["step"].tolist() == [3, 4, 5] and dropped == 2 and log["xyz"].shape == (3, 40, 3) and log["status"].shape == (3, 40)
    for i, step in enumerate((3, 4, 5)):                       # a frame is the pool as it was fetched at that step
        count = 3 * step
        assert M.same_bits(log["xyz"][i, :count], pools[step]["xyz"]) and np.array_equal(log["status"][i, :count], pools[step]["status"])
        assert (log["status"][i, count:] == F.TRACER_FREE).all() and (log["xyz"][i, count:] == 0).all()
    assert sim.tracer_log()["step"].shape == (0,)             # draining empties the ring
    # a status only drain; an advance on demand takes a frame with the current step number
    sim.tracer_advance()
    assert sim._L.fs_tracer_log(sim._h, None, status.ctypes.data, None, 3, Ct.byref(n), None) == 0 and n.value == 1
    assert np.array_equal(status[0, :18], sim.tracers()["status"])
    # tracer_every can change at any time; setting tracer_log clears the log but not the pool
    sim.run_one()                                              # step 6
    sim.set_option("tracer_log", 4)
    assert sim.tracer_log()["step"].size == 0 and sim.tracer_count == 21
    sim.set_option("tracer_every", 3)
    for _ in range(5):                                         # steps 7 .. 11: (step - 1) % 3 == 0 at 7 and 10
        sim.run_one()
    assert sim.tracer_log()["step"].tolist() == [7, 10]
    # setting tracers clears the pool and the log
    sim.set_option("tracer_every", 1)
    sim.run_one()
    sim.set_option("tracers", 40)
    assert sim.tracer_log()["step"].size == 0 and sim.tracer_count == 0
    sim.run_one()                                              # step 13: emitters are the handle's, the pool starts again
    log = sim.tracer_log()
    assert log["step"].tolist() == [13] and sim.tracer_count == 3 and (log["status"][0, :3] == F.TRACER_ALIVE).all()
    sim.set_option("tracers", 0)                               # off
    sim.run_one()
    with pytest.raises(F.FluidsimError):
        sim.tracers()
    assert sim.tracer_capacity == 0 and sim.tracer_count == 0
    sim.close()


# ---- 7. tracer_sample ------------------------------------------------------------------------------------------------------------------

@precisions
def test_tracer_sample_is_the_sampler(precision):
    import fluid_simulation_amd as F
    from fluid_simulation_amd import viewer
    sim = tunnel(precision, tracers=C, flow_stats="mean")
    sim.tracer_seed(np.concatenate([viewer.rake((0.5, 0.5, 0.5), (24.5, 16.5, 12.5), 500), viewer.rake((3.0, 8.0, 6.0), (24.0, 9.0, 6.0), NP - 500)]))
    for _ in range(4):
        sim.run_one()
    t = sim.tracers()
    assert (t["status"] == F.TRACER_HIT).sum() > 20 and (t["status"] == F.TRACER_ALIVE).sum() > 100
    sim.sample_points(t["xyz"])
    for source in (F.VX, F.ISO_VORTEX | F.VORTEX_Q, F.SAMPLE_STAT | F.STAT_MEAN_VX):
        for mode in ("linear", "nearest", "fluid"):
            got, want = sim.tracer_sample(source, mode), sim.sample(source, mode)
            assert got.shape == (NP,) and M.same_bits(got, want), (source, mode)
        assert np.abs(got[np.isfinite(got)]).max() > 0
    assert M.same_bits(sim.tracers()["xyz"], t["xyz"])        # sampling moves nothing
    # dead particles are evaluated where they stopped: blown out of the padded box, they give NaN
    sim.set(F.VX, np.full(sim.shape, 100.0, dtype=sim.dtype))
    sim.tracer_advance()
    t2 = sim.tracers()
    gone = t2["xyz"][:, 0] > 25.0
    assert gone.sum() > 100 and (t2["status"][gone] == F.TRACER_OUT).all()
    with np.errstate(invalid="ignore"):
        outside = ~((t2["xyz"] >= 0.0) & (t2["xyz"] <= np.array([25.0, 17.0, 13.0]))).all(axis=1)
    got = sim.tracer_sample(F.VY)
    assert np.isnan(got[outside]).all() and np.isfinite(got[~outside]).all() and (~outside).sum() > 20
    sim.sample_points(t2["xyz"])
    assert M.same_bits(got, sim.sample(F.VY))
    sim.close()


# ---- 8. errors ---------------------------------------------------------------------------------------------------------------------

def test_errors():
    import ctypes as Ct
    import fluid_simulation_amd as F
    EINVAL = F._lib.EINVAL
    W, H, D = 8, 6, 5
    sim = sim_of(W, H, D)
    L, h = sim._L, sim._h
    good = np.array([[1.0, 1.0, 1.0], [8.5, 6.5, 5.5], [0.5, 0.5, 0.5]])
    n = Ct.c_long()
    # option off
    assert L.fs_tracer_advance(h) == EINVAL and "tracers" in (L.fs_last_error() or b"").decode()
    assert L.fs_tracer_seed(h, good.ctypes.data, 3) == EINVAL and L.fs_tracer_clear(h) == EINVAL
    assert L.fs_tracer_fetch(h, None, None, 0, Ct.byref(n)) == EINVAL
    assert L.fs_tracer_sample(h, F.VX, 1, None, 0) == EINVAL
    assert L.fs_tracer_log(h, None, None, None, 0, Ct.byref(n), None) == 0 and n.value == 0
    assert L.fs_tracer_emitters(h, good.ctypes.data, 3, 1) == 0 and sim._geti("tracer_emitters") == 3   # the list is the handle's
    sim.set_option("tracers", 16)
    # points outside B, or NaN: nothing is seeded, the emitters stay
    assert L.fs_tracer_seed(h, good.ctypes.data, 3) == 0 and sim.tracer_count == 3
    for k, bad in enumerate((0.25, np.nextafter(0.5, 0.0), np.nan, np.inf, -1.0)):
        for axis, hi in enumerate((W, H, D)):
            for value in (bad, hi + 0.5 + abs(bad) if np.isfinite(bad) else bad):
                pts = good.copy()
                pts[k % 3, axis] = value
                assert L.fs_tracer_seed(h, pts.ctypes.data, 3) == EINVAL, (axis, value)
                assert L.fs_tracer_emitters(h, pts.ctypes.data, 3, 1) == EINVAL, (axis, value)
    assert sim.tracer_count == 3 and sim._geti("tracer_seeded") == 3 and sim._geti("tracer_emitters") == 3
    # limits
    many = np.ones((F.TRACER_EMITTERS_MAX + 1, 3))
    assert L.fs_tracer_emitters(h, many.ctypes.data, F.TRACER_EMITTERS_MAX + 1, 1) == EINVAL
    assert L.fs_tracer_emitters(h, many.ctypes.data, -1, 1) == EINVAL and L.fs_tracer_emitters(h, None, 2, 1) == EINVAL
    for every in (0, -3):
        assert L.fs_tracer_emitters(h, good.ctypes.data, 3, every) == EINVAL, every
    assert sim._geti("tracer_emitters") == 3
    assert L.fs_tracer_emitters(h, many.ctypes.data, F.TRACER_EMITTERS_MAX, 7) == 0 and L.fs_tracer_emitters(h, None, 0, 1) == 0
    assert L.fs_tracer_seed(h, good.ctypes.data, -1) == EINVAL and L.fs_tracer_seed(h, None, 2) == EINVAL
    assert L.fs_tracer_seed(h, good.ctypes.data, (1 << 24) + 1) == EINVAL and L.fs_tracer_seed(h, None, 0) == 0
    # a fetch with too little room; sample sizes, modes and sources
    xyz = np.zeros((3, 3))
    meta = np.zeros((3, 4), dtype=np.int32)
    assert L.fs_tracer_fetch(h, xyz.ctypes.data, None, 2, Ct.byref(n)) == EINVAL and n.value == 3
    assert L.fs_tracer_fetch(h, None, meta.ctypes.data, 2, None) == EINVAL
    assert L.fs_tracer_fetch(h, xyz.ctypes.data, meta.ctypes.data, 3, None) == 0 and bits_equal(xyz, good)
    out = np.zeros(4)
    assert L.fs_tracer_sample(h, F.VX, 1, out.ctypes.data, 3) == 0
    assert L.fs_tracer_sample(h, F.VX, 1, out.ctypes.data, 4) == EINVAL and L.fs_tracer_sample(h, F.VX, 1, out.ctypes.data, 2) == EINVAL
    assert L.fs_tracer_sample(h, F.VX, 3, out.ctypes.data, 3) == EINVAL and L.fs_tracer_sample(h, 11, 1, out.ctypes.data, 3) == EINVAL
    assert L.fs_tracer_sample(h, F.VX, 1, None, 3) == EINVAL
    assert L.fs_tracer_sample(h, F.SAMPLE_STAT | F.STAT_MEAN_VX, 1, out.ctypes.data, 3) == EINVAL     # flow_stats is off
    # the options
    for key, bads in ((b"tracers", ("-1", "4194305", "x", "")), (b"tracer_log", ("-1", "65537", "x", "")), (b"tracer_every", ("0", "-3", "x"))):
        for bad in bads:
            assert L.fs_set_option(h, key, bad.encode()) == EINVAL, (key, bad)
    assert sim.tracer_capacity == 16 and sim.tracer_count == 3
    for fn in (L.fs_tracer_clear, L.fs_tracer_advance):
        assert fn(None) == EINVAL
    assert L.fs_tracer_seed(None, None, 0) == EINVAL and L.fs_tracer_emitters(None, None, 0, 1) == EINVAL
    assert L.fs_tracer_fetch(None, None, None, 0, None) == EINVAL and L.fs_tracer_sample(None, 0, 0, None, 0) == EINVAL
    assert L.fs_tracer_log(None, None, None, None, 0, None, None) == EINVAL
    sim.close()
    # the ring's size limit: N x C x 28 bytes over 1 GiB, from either side (a handle not yet in use allocates nothing)
    big = sim_of(8, 8, 8)
    assert big._L.fs_set_option(big._h, b"tracers", b"4194304") == 0
    assert big._L.fs_set_option(big._h, b"tracer_log", b"10") == EINVAL           # 10 x 4194304 x 28 = 1.09 GiB
    assert big._L.fs_set_option(big._h, b"tracer_log", b"9") == 0
    assert big._L.fs_set_option(big._h, b"tracers", b"4260881") == EINVAL and big.tracer_capacity == 4194304
    assert big._L.fs_set_option(big._h, b"tracers", b"1000") == 0
    assert big._L.fs_set_option(big._h, b"tracer_log", b"38348") == EINVAL        # 38347 x 1000 x 28 <= 2^30 < 38348 x 1000 x 28
    assert big._L.fs_set_option(big._h, b"tracer_log", b"38347") == 0
    assert big._L.fs_set_option(big._h, b"tracers", b"1001") == EINVAL
    big.close()
    # slab handles: every entry and option is refused; a handle with tracers on cannot become one
    sim = sim_of(8, 8, 8)
    sim.comm_init(0, 2, b"FSNULL:".ljust(128, b"\0"))
    L, h = sim._L, sim._h
    calls = [lambda: L.fs_tracer_seed(h, good.ctypes.data, 1), lambda: L.fs_tracer_emitters(h, good.ctypes.data, 1, 1),
             lambda: L.fs_tracer_emitters(h, None, 0, 1), lambda: L.fs_tracer_clear(h), lambda: L.fs_tracer_advance(h),
             lambda: L.fs_tracer_fetch(h, None, None, 0, Ct.byref(n)), lambda: L.fs_tracer_sample(h, F.VX, 1, out.ctypes.data, 0),
             lambda: L.fs_tracer_log(h, None, None, None, 0, Ct.byref(n), None), lambda: L.fs_set_option(h, b"tracers", b"16"),
             lambda: L.fs_set_option(h, b"tracer_log", b"2"), lambda: L.fs_set_option(h, b"tracer_every", b"2")]
    for k, call in enumerate(calls):
        assert call() == EINVAL, k
        assert "single-GPU" in (L.fs_last_error() or b"").decode(), k
    with pytest.raises(F.FluidsimError):
        sim.tracers()
    sim.close()
    sim = sim_of(8, 8, 8, tracers=16)
    with pytest.raises(F.FluidsimError):
        sim.comm_init(0, 2, b"FSNULL:".ljust(128, b"\0"))
    sim.set_option("tracers", 0)
    sim.comm_init(0, 2, b"FSNULL:".ljust(128, b"\0"))
    sim.close()


# ---- 9. simulation.out --tracers --------------------------------------------------------------------------------------------------

def test_cli_tracer_csv_matches_python(tmp_path):
    import fluid_simulation_amd as F
    exe = os.path.join(ROOT, "simulation.out")
    assert os.path.exists(exe), "simulation.out is built by __graft_entry__.build()"
    stl = os.path.join(GOLDEN, "sphere_24x12.stl")
    emit = [(1.0, 8.5, 8.5), (1.0, 4.0, 8.0), (0.5, 12.25, 3.0), (30.0, 8.0, 8.0), (10.0, 8.0, 8.0)]
    pts = tmp_path / "emitters.txt"
    pts.write_text("# a rake upstream\n1 8.5 8.5\n1.0 4 8   # below\n\n  0.5 12.25 3\n30\t8 8\n1e1 8 8\n")
    csv = tmp_path / "t.csv"
    env = {k: v for k, v in os.environ.items() if not k.startswith("FS_")}
    common = ["--grid", "32x16x16", "--steps", "6", "--stl", stl + ",0.5,0,0,0,-4,0,0", "--dump-every", "0", "--dump-dir", str(tmp_path), "--quiet"]
    subprocess.run([exe] + common + ["--tracers", "64", "--tracer-emitters", str(pts), "--tracer-every", "2", "--tracer-out", str(csv)],
                   check=True, cwd=str(tmp_path), env=env, timeout=600)
    lines = csv.read_text().splitlines()
    assert lines[0] == "slot,source,born,moves,status,x,y,z" and len(lines) == 1 + 15
    sim = F.Simulation(32, 16, 16, 6, quiet=1, dump_every=0, tracers=64)
    assert F.loadSTLIntoObstacles(stl, sim, 0.5, 0.0, 0.0, 0.0, -4.0, 0.0, 0.0) > 0
    sim.tracer_emitters(emit, every=2)
    sim.run()
    t = sim.tracers()
    rows = [ln.split(",") for ln in lines[1:]]
    assert [int(r[0]) for r in rows] == list(range(15))
    for col, name in ((1, "source"), (2, "born"), (3, "moves"), (4, "status")):
        assert [int(r[col]) for r in rows] == t[name].tolist(), name
    assert M.same_bits(np.array([[float(v) for v in r[5:]] for r in rows]), t["xyz"])
    assert t["born"].tolist() == [1] * 5 + [3] * 5 + [5] * 5 and (t["moves"] > 0).sum() >= 10
    # the same through the environment, and a malformed file is refused
    csv2 = tmp_path / "t2.csv"
    subprocess.run([exe] + common, check=True, cwd=str(tmp_path), timeout=600,
                   env=dict(env, FS_TRACERS="64", FS_TRACER_EMITTERS=str(pts), FS_TRACER_EVERY="2", FS_TRACER_OUT=str(csv2)))
    assert csv2.read_text() == csv.read_text()
    pts.write_text("1 2\n")
    r = subprocess.run([exe, "--grid", "32x16x16", "--steps", "1", "--tracers", "8", "--tracer-emitters", str(pts), "--stl", "none",
                        "--dump-every", "0", "--quiet"], cwd=str(tmp_path), env=env, timeout=600, capture_output=True, text=True)
    assert r.returncode != 0 and "x y z" in r.stderr
    # flags that would do nothing are refused
    pts.write_text("1 8 8\n")
    for flags, word in ((["--tracer-emitters", str(pts)], "--tracers"), (["--tracer-out", str(csv2)], "--tracers"),
                        (["--tracers", "8", "--tracer-every", "2"], "--tracer-emitters")):
        r = subprocess.run([exe, "--grid", "32x16x16", "--steps", "1", "--stl", "none", "--dump-every", "0", "--quiet"] + flags,
                           cwd=str(tmp_path), env=env, timeout=600, capture_output=True, text=True)
        assert r.returncode == 2 and word in r.stderr, flags
    sim.close()


# ---- 10. the viewer ----------------------------------------------------------------------------------------------------------------

def test_viewer_streaklines_and_pathlines():
    import fluid_simulation_amd as F
    from fluid_simulation_amd import viewer
    sim = tunnel(speed=1, tracers=64, tracer_log=8)
    emit = np.array([[1.0, 5.0, 6.0], [1.0, 8.0, 6.0], [7.0, 8.0, 6.0]])     # the last one sits inside the ball
    sim.tracer_emitters(emit, every=2)
    for _ in range(5):                                         # releases at steps 1, 3, 5
        sim.run_one()
    t = sim.tracers()
    assert t["status"].tolist() == [F.TRACER_ALIVE, F.TRACER_ALIVE, F.TRACER_HIT] * 2 + [F.TRACER_ALIVE] * 3
    lines = viewer.streaklines(sim)
    assert len(lines) == 3 and [ln.shape for ln in lines] == [(3, 3), (3, 3), (1, 3)]
    for e in (0, 1):                                           # newest first: born 5, 3, 1 = slots 6 + e, 3 + e, e
        assert M.same_bits(lines[e], t["xyz"][[6 + e, 3 + e, e]])
        assert (np.diff(lines[e][:, 0]) > 0).all()             # the older a particle, the further downstream
    for e in (0, 1, 2):
        assert lines[e][0].tolist() == emit[e].tolist()        # released in the last step: not yet moved
    log = sim.tracer_log()
    assert log["step"].tolist() == [1, 2, 3, 4, 5]
    paths = viewer.pathlines(log)
    assert len(paths) == 64
    assert len(paths[0]) == 1 and paths[0][0].shape == (5, 3) and M.same_bits(paths[0][0], log["xyz"][:, 0])
    assert len(paths[3]) == 1 and paths[3][0].shape == (3, 3) and M.same_bits(paths[3][0], log["xyz"][2:, 3])
    for slot in (2, 5, 8):                                     # ALIVE in the frame of its release, HIT from the next one on
        assert len(paths[slot]) == 1 and paths[slot][0].tolist() == [emit[2].tolist()]
    assert paths[9:] == [[] for _ in range(55)]
    sim.close()
