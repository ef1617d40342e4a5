"""Momentum zones on the MI355X (fs_zones, fs_zone_*), through the C ABI via the Python mirror: the mask, the pass and the
budget against the numpy restatement of include/fluidsim.h (tests/zones_model.py) on grids that take every path of the march
tiling, hand numbers, edge values, a step in mode 2 against the same calls made by hand, "off means off", the refusals,
simulation.out --zone and the direction of a fan and of a porous slab.  Every comparison of numbers is bit for bit."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import zones_model as M
from conftest import ROOT, ball_mask, bits_equal

pytestmark = pytest.mark.gpu
# two x-waves with a ragged 4-group; a full and a ragged 4-group of one row; several row groups; chunks of 8, 8 and 1 planes
GRIDS = [(5, 1, 1), (4, 1, 1), (13, 7, 9), (516, 4, 3), (8, 37, 4), (6, 5, 17)]


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
    """name -> padded boolean mask; every kind is clipped to the box, so each exists on every grid"""
    out = {"none": np.zeros((D + 2, H + 2, W + 2), dtype=bool)}
    out["ball"] = ball_mask(W, H, D, W / 2.0, H / 2.0, D / 2.0, max(1.0, min(W, H, D) / 3.0))
    m = out["none"].copy()
    m[1:min(2, D) + 1, 1:min(2, H) + 1, 1:min(3, W) + 1] = True
    out["block on a wall"] = m
    return out


def block_box(W, H, D):
    """the cells of masks()["block on a wall"]"""
    return (1, min(3, W), 1, min(2, H), 1, min(2, D))


def random_fields(rng, shape, dtype):
    """eleven padded arrays of mixed magnitude, a few -0.0, the box edges zero"""
    out = []
    for _ in range(11):
        a = (rng.standard_normal(shape) * 10.0 ** rng.integers(-2, 2, size=shape)).astype(dtype)
        a[rng.random(shape) < 0.03] = dtype(-0.0)
        out.append(zero_edges(a))
    return out


def zone_sets(W, H, D):
    """name -> rows"""
    whole = M.whole_box((W, H, D))
    cx, cy, cz = (W + 1) // 2, (H + 1) // 2, (D + 1) // 2
    out = {}
    out["the whole domain"] = [M.row(box=whole, g=(0.5, -0.25, 0.125), D=(1.0, 0.0, 2.5), F=(0.0, 3.0, 0.75))]
    out["the whole domain, a fan"] = [M.row(box=whole, axis=1, g=(0.0, 2.0, -1.0))]
    out["two corner cells"] = [M.row(box=(1, 1, 1, 1, 1, 1), D=(4.0, 4.0, 4.0)), M.row(box=(W, W, H, H, D, D), axis=1, g=(1.0, 1.0, 1.0), F=(0.0, 9.0, 0.0))]
    for axis, centre in ((0, (cy, cz)), (1, (cx, cz)), (2, (cx, cy))):
        out["cylinder along %d, integral centre, radius 2" % axis] = [M.row(M.CYLINDER, axis, whole, centre, 2.0, g=(0.1, 0.2, 0.3), F=(1.0, 1.0, 1.0))]
    out["cylinder, fractional centre"] = [M.row(M.CYLINDER, 2, whole, (cx + 0.5, cy - 0.25), 1.25, D=(0.5, 0.5, 0.5))]
    out["cylinder, radius 0"] = [M.row(M.CYLINDER, 1, whole, (cx, cz), 0.0, g=(1.0, 0.0, 0.0), D=(0.0, 7.0, 0.0))]
    out["inside the block"] = [M.row(box=block_box(W, H, D), g=(1.0, 1.0, 1.0), D=(1.0, 1.0, 1.0))]
    out["eight zones"] = [M.row(M.CYLINDER if k % 4 == 3 else M.BOX, k % 3, (1 + k % min(W, 3), W, 1, H, 1 + (k // 4) * (D // 2), D), (cx, cy), 2.5,
                                g=(0.01 * k, 0.0, -0.02 * k), D=(0.1 * (k % 2), 0.0, 0.0), F=(0.0, 0.2 * (k % 3), 0.0)) for k in range(8)]
    a = M.row(box=(1, max(1, W - 1), 1, H, 1, D), g=(0.5, 0.0, 0.0), D=(2.0, 0.0, 0.0))
    b = M.row(box=(min(2, W), W, 1, H, 1, D), axis=1, F=(3.0, 3.0, 3.0))
    out["two overlapping zones"] = [a, b]
    out["the same, the other way round"] = [b, a]
    return out


def load(sim, fields, mask):
    import fluid_simulation_amd as F
    sim.set_mask(mask)
    for f in range(11):
        if f != F.OBS:
            sim.set(f, fields[f])


def expect_pass(sim, ref, fields, mask, zones, context, nan_ok=False):
    """`sim` holds `fields` (11 padded arrays, OBS = the mask) and runs one pass; `ref` receives the model's values through
    fs_set_field, then fs_set_bounds (1, 2, 3).  All eleven fields of the two handles must hold the same bits, and the
    non-velocity fields their old ones.  -> the three velocity arrays after the pass"""
    import fluid_simulation_amd as F
    load(sim, fields, mask)
    obs = sim.get(F.OBS)
    new = M.apply_unbounded([fields[F.VX], fields[F.VY], fields[F.VZ]], obs, zones, sim.dt)
    ref.set_mask(mask)
    for f in range(11):
        if f != F.OBS:
            ref.set(f, new[f - F.VX] if f in (F.VX, F.VY, F.VZ) else fields[f])
    for b, f in ((1, F.VX), (2, F.VY), (3, F.VZ)):
        ref.set_bounds(b, f)
    sim.set_zones(zones, mode="manual")
    before = sim._geti("zone_applies")
    sim.apply_zones()
    assert sim._geti("zone_applies") == before + 1
    same = M.same if nan_ok else bits_equal
    out = []
    for f in range(11):
        got, want = sim.get(f), ref.get(f)
        assert same(got, want), (context, F.FIELD_NAMES[f], np.argwhere(got.view(np.uint8) != want.view(np.uint8))[:4])
        if f not in (F.VX, F.VY, F.VZ, F.OBS):
            assert same(got, fields[f]), (context, F.FIELD_NAMES[f], "changed")
        if f in (F.VX, F.VY, F.VZ):
            out.append(got)
    # and the model's own setBounds says the same
    for got, want in zip(out, M.apply([fields[F.VX], fields[F.VY], fields[F.VZ]], obs, zones, sim.dt)):
        assert same(got, want), (context, "model set_bounds")
    return out


# ---- 1. the mask against the model ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("precision", ["fp32", "fp64"])
@pytest.mark.parametrize("grid", GRIDS)
def test_mask_matches_the_model(grid, precision):
    import fluid_simulation_amd as F
    W, H, D = grid
    sim = sim_of(W, H, D, precision)
    marked = 0
    for mname, mask in masks(W, H, D).items():
        sim.set_mask(mask)
        obs = sim.get(F.OBS)
        for zname, zones in zone_sets(W, H, D).items():
            sim.set_zones(zones, mode="manual")
            got, want = sim.zone_mask(), M.mask(obs, zones)
            assert got.dtype == np.uint8 and np.array_equal(got, want), (grid, mname, zname, np.argwhere(got != want)[:4])
            marked += int(np.count_nonzero(want))
            if zname == "inside the block" and mname == "block on a wall":
                assert not want.any()
    assert marked > 0
    sim.close()


# ---- 2. the pass against the model ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("precision", ["fp32", "fp64"])
@pytest.mark.parametrize("grid", GRIDS)
def test_pass_matches_the_model(grid, precision):
    W, H, D = grid
    sim, ref = sim_of(W, H, D, precision), sim_of(W, H, D, precision)
    rng = np.random.default_rng([W, H, D, 2])
    orders_differ = 0
    for mname, mask in masks(W, H, D).items():
        sets = zone_sets(W, H, D)
        results = {}
        for zname, zones in sets.items():
            fields = random_fields(rng, mask.shape, sim.dtype) if zname != "the same, the other way round" else fields
            results[zname] = expect_pass(sim, ref, fields, mask, zones, (grid, precision, mname, zname))
        ab, ba = results["two overlapping zones"], results["the same, the other way round"]
        orders_differ += sum(not bits_equal(p, q) for p, q in zip(ab, ba))
    assert orders_differ > 0 or W < 3, "the order of two overlapping zones should show"
    sim.close()
    ref.close()


# ---- 3. hand numbers in fp64 ---------------------------------------------------------------------------------------------------

def test_hand_numbers():
    """DT is the handle's float dt widened, so with dt = 0.05 the denominator is 1 + DT, and 3 / (1 + DT) is 3 / 1.05 but for
    DT - 0.05: |3 / (1 + DT) - 3 / 1.05| <= 3 * |DT - 0.05| / 1.05^2 (the derivative of 3 / (1 + t) falls with t), plus one
    rounding of each quotient."""
    import fluid_simulation_amd as F
    W, H, D = 6, 5, 4
    sim = sim_of(W, H, D, "fp64", dt=0.05)
    DT = float(np.float32(0.05))
    assert float(sim.dt) == DT
    inner = (slice(1, -1),) * 3
    vx = np.zeros(sim.shape)
    vx[inner] = 3.0
    sim.set(F.VX, vx)
    sim.set_zones([M.row(box=M.whole_box((W, H, D)), D=(1.0, 0.0, 0.0))], mode="manual")
    sim.apply_zones()
    got = sim.get(F.VX)[inner]
    assert (got == 3.0 / (1.0 + DT)).all(), got.ravel()[:3]
    assert abs(float(got[0, 0, 0]) - 3.0 / 1.05) <= 3.0 * abs(DT - 0.05) / 1.05 ** 2 + 2 * np.spacing(3.0 / 1.05)
    assert not sim.get(F.VY).any() and not sim.get(F.VZ).any()
    # g only: v + DT * g, two roundings
    rng = np.random.default_rng(3)
    vel = [zero_edges(rng.standard_normal(sim.shape)) for _ in range(3)]
    g = (0.3, -1.7, 2.9)
    for f, a in zip((F.VX, F.VY, F.VZ), vel):
        sim.set(f, a)
    sim.set_zones([M.row(box=M.whole_box((W, H, D)), g=g)], mode="manual")
    sim.apply_zones()
    for f, a, ga in zip((F.VX, F.VY, F.VZ), vel, g):
        assert bits_equal(sim.get(f)[inner], a[inner] + DT * ga), F.FIELD_NAMES[f]
    sim.close()


# ---- 4. edge values --------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("precision", ["fp32", "fp64"])
def test_edge_values(precision):
    import fluid_simulation_amd as F
    W, H, D = 13, 7, 9
    sim, ref = sim_of(W, H, D, precision), sim_of(W, H, D, precision)
    mask = masks(W, H, D)["ball"]
    # -0.0 everywhere, a fan with g = 0 over half the box: outside it the sign stays, inside (T)(-0.0 + 0.0) is +0.0
    fields = [zero_edges(np.full(sim.shape, -0.0, dtype=sim.dtype)) for _ in range(11)]
    zones = [M.row(box=(1, 6, 1, H, 1, D))]
    vel = expect_pass(sim, ref, fields, mask, zones, "minus zero")
    tgt = M.target_cells(sim.get(F.OBS))
    inside = tgt & M.in_zone(zones[0], tgt.shape)
    outside = tgt & ~inside
    assert inside.any() and outside.any()
    for a in vel:
        assert np.signbit(a[outside]).all() and not np.signbit(a[inside]).any()
    # NaN and Inf in a fan (whose short cut must not hide 0 * Inf), a resistive zone and both
    rng = np.random.default_rng(4)
    for zname in ("the whole domain, a fan", "the whole domain", "two overlapping zones"):
        fields = random_fields(rng, mask.shape, sim.dtype)
        for f, bad in zip((F.VX, F.VY, F.VZ), (np.inf, np.nan, -np.inf)):
            fields[f][rng.random(mask.shape) < 0.05] = bad
            fields[f] = zero_edges(fields[f])                # the box edges are not the pass's business
        fields[F.VX][2, 3, 4] = np.finfo(sim.dtype).max      # finite; in fp64 its square is not
        vel = expect_pass(sim, ref, fields, mask, zone_sets(W, H, D)[zname], ("non-finite", zname), nan_ok=True)
        assert np.isnan(vel[2][tgt]).any() and np.isfinite(vel[2][tgt]).any()
    sim.close()
    ref.close()


# ---- 5. the budget -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("precision", ["fp32", "fp64"])
@pytest.mark.parametrize("grid", GRIDS)
def test_budget_matches_the_model(grid, precision):
    import fluid_simulation_amd as F
    W, H, D = grid
    sim = sim_of(W, H, D, precision)
    rng = np.random.default_rng([W, H, D, 5])
    empty = 0
    for mname, mask in masks(W, H, D).items():
        for zname, zones in zone_sets(W, H, D).items():
            fields = random_fields(rng, mask.shape, sim.dtype)
            load(sim, fields, mask)
            sim.set_zones(zones, mode="manual")
            obs = sim.get(F.OBS)
            want, want_planes = M.budget([fields[F.VX], fields[F.VY], fields[F.VZ]], obs, zones, sim.dt)
            got, got_planes = sim.zone_budget(per_plane=True)
            assert bits_equal(got_planes, want_planes), (grid, precision, mname, zname, np.argwhere(got_planes != want_planes)[:4])
            assert bits_equal(got, want), (grid, precision, mname, zname, got, want)
            assert bits_equal(sim.zone_budget(), want)
            for k in range(len(zones)):
                if want[k, M.C_CELLS] == 0:                  # a zone without cells: zeros and -Inf
                    empty += 1
                    assert got[k].tolist() == [0.0] * 6 + [-np.inf] and not np.signbit(got[k][:6]).any()
            for f in range(11):                              # a query changes nothing
                if f != F.OBS:
                    assert bits_equal(sim.get(f), fields[f]), (zname, F.FIELD_NAMES[f])
    assert empty > 0, "the zone inside the block holds no target cell"
    sim.close()


# ---- 6. a step in mode 2 = the pass, then the step -------------------------------------------------------------------------------

@pytest.mark.parametrize("others", [False, True])
@pytest.mark.parametrize("precision", ["fp32", "fp64"])
def test_step_in_mode_2_is_the_calls_by_hand(precision, others):
    import fluid_simulation_amd as F
    W, H, D = 24, 20, 12
    mask = ball_mask(W, H, D, 8, 10, 6, 3)
    zones = [M.row(box=(12, 14, 1, H, 1, D), D=(3.0, 0.5, 0.5), F=(2.0, 0.0, 0.0)),
             M.row(M.CYLINDER, 0, (17, 18, 1, H, 1, D), (10.0, 6.5), 4.0, g=(4.0, 0.0, 0.0)),
             M.row(box=(14, 17, 5, 15, 1, D), axis=1, g=(0.0, -1.0, 0.0), F=(0.0, 1.0, 1.0))]
    a = sim_of(W, H, D, precision, acc=6, vorticity_confinement=(0.5 if others else 0.0))
    b = sim_of(W, H, D, precision, acc=6)
    heat = dict(kappa=0.01, beta=0.8, alpha=0.2, up="+y", inlet=0.5, wall=1.0)
    for h in (a, b):
        h.set_mask(mask)
        if others:
            h.set_heat(in_step=(h is a), **heat)
    a.set_zones(zones, mode="step", log=8)
    b.set_zones(zones, mode="manual")
    rows = []
    for step in range(3):
        a.step()
        if others:                                           # the order: confinement, heat's pass A, the record, the zone pass
            b.confine_vorticity(0.5)
            b.heat_apply()
        before = [b.get(f) for f in (F.VX, F.VY, F.VZ)]
        whole = b.zone_budget()
        rows.append(M.log_row(step + 1, whole))
        assert bits_equal(whole, M.budget(before, b.get(F.OBS), zones, b.dt)[0]), step
        b.apply_zones()
        b.step()
        if others:
            b.heat_transport()
            assert bits_equal(a.temperature(), b.temperature()), (step, "theta")
        for f in (F.VX, F.VY, F.VZ, F.DENS, F.PRESSURE):
            assert bits_equal(a.get(f), b.get(f)), (step, F.FIELD_NAMES[f])
    assert a._geti("zone_applies") == 3 and a._geti("zone_mode") == 2 and b._geti("zone_mode") == 1
    got, dropped = a.zone_log(with_dropped=True)
    assert dropped == 0 and got.shape == (3, 1 + 3 * F.ZONE_COLS)
    assert bits_equal(got, np.array(rows)), (got, rows)
    assert got[2][1 + M.C_CELLS] > 0 and got[2][1 + M.C_DX] != 0
    assert a.zone_log().shape == (0, 1 + 3 * F.ZONE_COLS)    # drained
    assert b.zone_log().shape[0] == 0                        # no log was asked for
    a.close()
    b.close()


def test_a_short_log_drops_the_oldest():
    W, H, D = 16, 8, 8
    sim = sim_of(W, H, D, acc=4)
    zones = [M.row(box=(6, 8, 1, H, 1, D), g=(1.0, 0.0, 0.0))]
    sim.set_zones(zones, mode="step", log=2)
    want = []
    for step in range(5):
        want.append(M.log_row(step + 1, sim.zone_budget()))
        sim.step()
    got, dropped = sim.zone_log(with_dropped=True)
    assert dropped == 3 and got.shape[0] == 2
    assert bits_equal(got, np.array(want[3:]))
    sim.close()


# ---- 7. off means off ----------------------------------------------------------------------------------------------------------

def test_off_means_off():
    import fluid_simulation_amd as F
    W, H, D = 24, 20, 12
    mask = ball_mask(W, H, D, 8, 10, 6, 3)
    fields = {}
    for how in ("untouched", "never", "switched off", "no rows"):
        sim = sim_of(W, H, D, acc=6, profile=(0 if how == "untouched" else 1))
        if how == "switched off":
            sim.set_zones([M.row(box=(3, 9, 1, H, 1, D), g=(1.0, 0.0, 0.0), D=(1.0, 1.0, 1.0))], mode="step", log=4)
            sim.set_zones(None, mode="off")
        elif how == "no rows":
            sim.set_zones([], mode="step")
        sim.set_mask(mask)
        for _ in range(2):
            sim.run_one()
        fields[how] = [sim.get(f) for f in range(11)]
        if how != "untouched":
            assert sim.timing("zones")[1] == 0 and sim.timing("advect")[1] > 0, how
        assert sim._geti("zone_applies") == 0 and sim._geti("zone_mode") == 0, how
        rows, mode, log = sim.zones()
        assert rows.shape == (0, F.ZONE_PARAMS) and mode == 0 and log == 0
        with pytest.raises(F.FluidsimError) as e:
            sim.apply_zones()
        assert e.value.code == F._lib.EINVAL and "zones are off" in str(e.value)
        sim.close()
    for how in ("never", "switched off", "no rows"):
        for f, (x, y) in enumerate(zip(fields["untouched"], fields[how])):
            assert bits_equal(x, y), (how, F.FIELD_NAMES[f])


# ---- 8. refusals -----------------------------------------------------------------------------------------------------------------

def test_refusals_leave_the_zones_alone():
    import fluid_simulation_amd as F
    EINVAL = F._lib.EINVAL
    W, H, D = 8, 6, 5
    sim = sim_of(W, H, D)
    L, h = sim._L, sim._h
    good = np.array([M.row(box=(2, 7, 1, 6, 2, 4), g=(1.0, -2.0, 0.5), D=(0.0, 1.0, 2.0), F=(3.0, 0.0, 0.0)),
                     M.row(M.CYLINDER, 1, (1, 8, 2, 5, 1, 5), (4.5, 3.0), 2.5, F=(0.0, 1.0, 0.0))])
    sim.set_zones(good, mode="manual", log=4)

    def in_force():
        rows, mode, log = sim.zones()
        return bits_equal(rows, good) and mode == 1 and log == 4

    def refused(rc, *words):
        assert rc == EINVAL, rc
        for word in words:
            assert word.encode() in L.fs_last_error(), (word, L.fs_last_error())
        assert in_force(), words

    assert in_force()
    cases = []
    for k in range(F.ZONE_PARAMS):
        for v in (float("nan"), float("inf"), float("-inf")):
            cases.append((k, v))
    cases += [(0, 2), (0, -1), (0, 0.5), (1, 3), (1, -1), (1, 1.5), (2, 0), (3, W + 1), (2, 7.5), (4, 0), (5, H + 1), (4, 7), (6, 4.5),
              (7, D + 1), (6, D + 1), (10, -1e-9)] + [(k, -0.5) for k in range(14, 20)]
    for z in (0, 1):
        for k, v in cases:
            p = good.copy()
            p[z, k] = v
            refused(L.fs_zones(h, p.ctypes.data, 2, 1, 4), "zone %d" % z, "par[%d" % k)
    nine = np.array([good[0]] * 9)
    refused(L.fs_zones(h, nine.ctypes.data, 9, 1, 4), "FS_ZONE_MAX")
    refused(L.fs_zones(h, good.ctypes.data, -1, 1, 4), "n_zones")
    for mode in (3, -1):
        refused(L.fs_zones(h, good.ctypes.data, 2, mode, 4), "mode")
    for log in (-1, 2 ** 20 + 1):
        refused(L.fs_zones(h, good.ctypes.data, 2, 1, log), "log")
    refused(L.fs_zones(h, None, 2, 1, 4), "null")
    out = np.zeros(2 * F.ZONE_COLS)
    refused(L.fs_zone_budget(h, None, None), "null")
    refused(L.fs_zone_mask(h, out.ctypes.data, 7), "expected")
    n, dropped = C.c_long(), C.c_long()
    assert L.fs_zone_log(h, None, 0, C.byref(n), C.byref(dropped)) == 0 and n.value == 0
    # the same rows in the other mode keep the log's size
    sim.set_zones(good, mode="step", log=4)
    assert sim._geti("zone_mode") == 2
    sim.close()


def test_slab_handles_refuse():
    """The FSNULL communicator makes a handle a z-slab handle in one process, as in tests/test_gpu_confine.py."""
    import fluid_simulation_amd as F
    sim = sim_of(8, 8, 8)
    sim.comm_init(0, 2, b"FSNULL:".ljust(128, b"\0"))
    zones = [M.row(box=(2, 4, 1, 8, 1, 8), g=(1.0, 0.0, 0.0))]
    for mode in ("manual", "step"):
        with pytest.raises(F.FluidsimError) as e:
            sim.set_zones(zones, mode=mode)
        assert e.value.code == F._lib.EINVAL and "single GPU" in str(e.value)
    assert sim._geti("zone_mode") == 0 and sim.zones()[0].shape[0] == 0
    for call in (sim.apply_zones, sim.zone_budget, sim.zone_log, sim.zone_mask):
        with pytest.raises(F.FluidsimError) as e:
            call()
        assert e.value.code == F._lib.EINVAL and "single GPU" in str(e.value), call
    sim.set_zones(None, mode="off")                          # off is what a slab handle has
    assert sim._geti("zone_applies") == 0
    sim.close()


# ---- 9. simulation.out --zone ------------------------------------------------------------------------------------------------------

def test_cli_zones_write_the_same_log(tmp_path):
    import fluid_simulation_amd as F
    exe = os.path.join(ROOT, "simulation.out")
    assert os.path.exists(exe), "simulation.out is built by __graft_entry__.build()"
    env = {k: v for k, v in os.environ.items() if not k.startswith("FS_")}
    zones = [M.row(box=(5, 7, 1, 8, 1, 8), D=(2.0, 0.25, 0.25), F=(1.5, 0.0, 0.0)),
             M.row(M.CYLINDER, 0, (10, 11, 1, 8, 1, 8), (4.5, 4.5), 3.0, g=(2.5, 0.0, 0.0))]
    log = tmp_path / "zones.csv"
    args = [exe, "--grid", "16x8x8", "--steps", "3", "--stl", "none", "--dump-every", "0", "--quiet"]
    for r in zones:
        args += ["--zone", ",".join("%.17g" % v for v in r)]
    subprocess.run(args + ["--zone-log", str(log)], check=True, cwd=str(tmp_path), env=env, timeout=600)
    sim = F.Simulation(16, 8, 8, 3, quiet=1, dump_every=0)
    sim.set_zones(zones, mode="step", log=3)
    for _ in range(3):
        sim.run_one()
    rows = sim.zone_log()
    sim.close()
    assert rows.shape == (3, 1 + 2 * F.ZONE_COLS) and rows[2][1 + F.ZONE_COLS + M.C_CELLS] > 0 and rows[2][1 + M.C_DX] != 0
    got = np.loadtxt(str(log), delimiter=",", skiprows=1, ndmin=2)
    assert open(str(log)).readline().strip() == "step," + ",".join("z%d_%s" % (z, n) for z in range(2) for n in F.ZONE_NAMES)
    assert bits_equal(got, rows)
    # --zone-log without --zone, a malformed SPEC, and a value fs_zones refuses
    base = [exe, "--grid", "16x8x8", "--steps", "1", "--stl", "none", "--dump-every", "0", "--quiet"]
    r = subprocess.run(base + ["--zone-log", str(log)], cwd=str(tmp_path), env=env, timeout=600, capture_output=True, text=True)
    assert r.returncode != 0 and "--zone" in r.stderr
    r = subprocess.run(base + ["--zone", "0,0,1,2,3"], cwd=str(tmp_path), env=env, timeout=600, capture_output=True, text=True)
    assert r.returncode != 0
    bad = zones[0].copy()
    bad[14] = -1.0
    r = subprocess.run(base + ["--zone", ",".join("%.17g" % v for v in bad)], cwd=str(tmp_path), env=env, timeout=600, capture_output=True,
                       text=True)
    assert r.returncode != 0 and "par[14]" in r.stderr


# ---- 10. the physical direction: signs and orders only ------------------------------------------------------------------------------

@pytest.mark.parametrize("precision", ["fp32", "fp64"])
def test_a_fan_pushes_and_a_porous_slab_brakes(precision):
    import fluid_simulation_amd as F
    W, H, D = 24, 12, 12
    fan = [M.row(box=(11, 13, 4, 9, 4, 9), g=(5.0, 0.0, 0.0))]
    sim = sim_of(W, H, D, precision, acc=6)
    sim.speed = 0
    sim.set_zones(fan, mode="step")
    for _ in range(5):
        sim.step()
    zone = M.in_zone(fan[0], sim.shape)
    budget = sim.zone_budget()
    through = float(sim.get(F.VX)[zone].astype(np.float64).sum())
    print("fan: budget %r, sum of v_x over the zone %.6e" % (budget[0].tolist(), through))
    assert budget[0, M.C_CELLS] == 3 * 6 * 6 and budget[0, M.C_DX] > 0 and through > 0
    sim.close()
    slab = [M.row(box=(11, 13, 1, H, 1, D), D=(40.0, 0.0, 0.0), F=(10.0, 0.0, 0.0))]
    zone = M.in_zone(slab[0], (D + 2, H + 2, W + 2))
    mean = {}
    for how in ("open", "slab"):
        sim = sim_of(W, H, D, precision, acc=6)
        sim.speed = 1
        if how == "slab":
            sim.set_zones(slab, mode="step")
        for _ in range(10):
            sim.step()
        mean[how] = float(np.abs(sim.get(F.VX)[zone].astype(np.float64)).mean())
        sim.close()
    print("porous slab: mean |v_x| in the zone %.6e, without it %.6e" % (mean["slab"], mean["open"]))
    assert mean["slab"] < mean["open"]
