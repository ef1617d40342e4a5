"""Per-body pressure forces and moments (fs_label_bodies, fs_body_labels, fs_body_info, fs_body_force, option
"body_force_log" / fs_body_force_log) on the MI355X, through the Python mirror: labels and body info against the numpy
restatement in tests/bodies_model.py (exactly), analytic cases with dyadic numbers (exactly), random masks within the
worst-case bound of an fp64 sum, determinism, the per-step log inside real runs, errors, and the CSV of simulation.out."""
import os
import subprocess

import numpy as np
import pytest

import bodies_model as M
from conftest import GOLDEN, ROOT, bits_equal, load_golden, unpack_mask

pytestmark = pytest.mark.gpu
PRECISIONS = ["fp32", "fp64"]
GRIDS = [(37, 21, 18), (64, 48, 20), (5, 3, 4)]       # row pitch with and without padding, and a tiny one
EPS = 2.0 ** -52


def sim_of(W, H, D, precision="fp32", **kw):
    import fluid_simulation_amd as F
    kw.setdefault("quiet", 1)
    kw.setdefault("dump_every", 0)
    return F.Simulation(W, H, D, 1, precision=precision, **kw)


def zeros(W, H, D):
    return np.zeros((D + 2, H + 2, W + 2))


def put_box(obs, x0, x1, y0, y1, z0, z1, v=1.0):
    obs[z0:z1 + 1, y0:y1 + 1, x0:x1 + 1] = v
    return obs


# ---- 1. labels and info ------------------------------------------------------------------------------------------------

def golden(name):
    meta, arr = load_golden(name)
    return unpack_mask(arr["mask"], meta["W"], meta["H"], meta["D"]).astype(np.float64)


def serpentine():
    """One cell thick, winding through every second row of planes 1 and 3 of a 12 x 10 x 3 grid, joined through plane 2."""
    obs = zeros(12, 10, 3)
    for z in (1, 3):
        for y in range(1, 10, 2):
            obs[z, y, 1:13] = 1.0
        for k, y in enumerate(range(2, 10, 2)):
            obs[z, y, 12 if k % 2 == 0 else 1] = 1.0
    obs[2, 9, 1] = 1.0                                   # the far ends of the two planes' snakes
    return obs


def u_shape():
    obs = zeros(37, 21, 18)
    obs[9, 5, 3:34] = 1.0
    obs[9, 9, 3:34] = 1.0
    obs[9, 5:10, 33] = 1.0                               # the arms meet only at the far end
    return obs


def boxes_and_specks():
    """2 boxes and 40 isolated cells: 42 components, 16 bodies, 26 cells in the REST."""
    obs = zeros(64, 48, 20)
    put_box(obs, 5, 12, 5, 9, 3, 8)
    put_box(obs, 30, 34, 20, 30, 10, 15)
    k = 0
    for z in (2, 18):
        for y in range(36, 46, 2):
            for x in range(40, 48, 2):
                obs[z, y, x] = 1.0
                k += 1
    assert k == 40
    return obs


def odd_values():
    obs = zeros(37, 21, 18)
    put_box(obs, 4, 8, 4, 8, 4, 8, 0.5)                  # body cells that are not solid
    put_box(obs, 9, 10, 4, 8, 4, 8, 2.0)                 # joined to the first through faces
    put_box(obs, 20, 22, 10, 12, 10, 12, -1.0)
    obs[15, 18, 30] = 1.0
    return obs


LABEL_CASES = {
    "two_boxes_and_a_stray_cell": lambda: put_box(put_box(put_box(zeros(37, 21, 18), 4, 9, 3, 8, 2, 7), 20, 30, 10, 15, 9, 16),
                                                  34, 34, 19, 19, 3, 3),
    "golden_sphere_plus_plate": lambda: golden("g3_sphere_plus_plate_40x24x24"),
    "golden_plate_rot": lambda: golden("g3_plate_rot_32x24x20"),
    "golden_sphere": lambda: golden("g3_sphere_32x24x20"),
    "edge_touch": lambda: put_box(put_box(zeros(5, 3, 4), 1, 2, 1, 1, 2, 2), 3, 4, 2, 2, 2, 2),
    "corner_touch": lambda: put_box(put_box(zeros(5, 3, 4), 2, 2, 1, 1, 1, 2), 3, 3, 2, 2, 3, 3),
    "edge_touch_boxes": lambda: put_box(put_box(zeros(37, 21, 18), 4, 9, 3, 8, 2, 7), 10, 15, 9, 12, 2, 7),
    "body_on_a_wall": lambda: put_box(zeros(64, 48, 20), 1, 6, 1, 4, 14, 20),
    "serpentine": serpentine,
    "u_shape": u_shape,
    "two_equal_boxes": lambda: put_box(put_box(zeros(37, 21, 18), 20, 23, 10, 12, 9, 11), 4, 7, 3, 5, 2, 4),
    "boxes_and_40_specks": boxes_and_specks,
    "odd_obs_values": odd_values,
    "empty": lambda: zeros(37, 21, 18),
    "empty_tiny": lambda: zeros(5, 3, 4),
    "all_solid": lambda: put_box(zeros(64, 48, 20), 1, 64, 1, 48, 1, 20),
    "all_solid_tiny": lambda: put_box(zeros(5, 3, 4), 1, 5, 1, 3, 1, 4),
}
_MODEL = {}


def model_of(name):
    if name not in _MODEL:
        obs = LABEL_CASES[name]()
        _MODEL[name] = (obs,) + M.label_bodies(obs)
    return _MODEL[name]


def info_raw(rows):
    return np.stack([rows[n].astype(np.float64) for n in rows.dtype.names[1:13]], axis=1)


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("name", sorted(LABEL_CASES))
def test_labels_and_info_equal_the_model(name, precision):
    import fluid_simulation_amd as F
    obs, labels, info, ncomp = model_of(name)
    D, H, W = (n - 2 for n in obs.shape)
    sim = sim_of(W, H, D, precision)
    sim.set(F.OBS, obs.astype(sim.dtype))
    rows = sim.label_bodies()
    B = min(ncomp, M.BODY_MAX)
    assert (sim.body_count, sim.body_components) == (B, ncomp)
    got = sim.body_labels()
    assert got.dtype == np.int32 and np.array_equal(got, labels)
    assert len(rows) == B + 1 and list(rows["body"]) == list(range(B + 1))
    assert np.array_equal(info_raw(rows), info), (info_raw(rows), info)
    if B:
        assert np.array_equal(rows["cx"][1:], info[1:, 8] / info[1:, 0])
    # what the case is about
    if name == "two_boxes_and_a_stray_cell":
        assert list(info[:, 0]) == [0, 11 * 6 * 8, 6 * 6 * 6, 1]
    elif name in ("edge_touch", "corner_touch", "edge_touch_boxes"):
        assert ncomp == 2
    elif name == "serpentine":
        assert ncomp == 1 and info[1, 0] == 2 * (5 * 12 + 4) + 1
    elif name == "u_shape":
        assert ncomp == 1
    elif name == "two_equal_boxes":
        assert list(info[1:, 0]) == [36, 36] and info[1, 1] < info[2, 1] and got[2, 3, 4] == 1 and got[9, 10, 20] == 2
    elif name == "boxes_and_40_specks":
        assert (ncomp, B) == (42, 16) and info[0, 0] == 26 and (got == -1).sum() == 26
    elif name == "odd_obs_values":
        assert list(info[:, 0]) == [0, 175, 27, 1] and list(info[:, 11]) == [0, 0, 0, 1]
    elif name.startswith("empty"):
        assert B == 0 and list(info[0]) == [0, -1] + [0] * 10
    elif name.startswith("all_solid"):
        assert ncomp == 1 and info[1, 0] == W * H * D and info[1, 11] == H * D


def test_labels_follow_the_mask_lazily():
    """Without fs_label_bodies: every entry labels anew when obs changed, through fs_set_field and through addObstacle."""
    import fluid_simulation_amd as F
    sim = sim_of(37, 21, 18)
    assert sim.body_count == 0
    sim.addObstacle(5, 6, 7)
    assert sim.body_count == 1 and sim.body_labels()[7, 6, 5] == 1
    obs, labels, info, ncomp = model_of("two_boxes_and_a_stray_cell")
    sim.set(F.OBS, obs.astype(np.float32))
    assert np.array_equal(info_raw(sim.body_info()), info)
    assert np.array_equal(sim.body_labels(), labels)


# ---- 2. exact analytic cases -------------------------------------------------------------------------------------------

def two_boxes(W, H, D):
    obs = zeros(W, H, D)
    a = (4, 9, 3, 8, 2, 7)          # 6 x 6 x 6
    b = (20, 30, 10, 15, 9, 16)     # 11 x 6 x 8, the larger: body 1
    put_box(obs, *a)
    put_box(obs, *b)
    return obs, b, a


def query(sim, obs, p, origin=None):
    import fluid_simulation_amd as F
    sim.set(F.OBS, obs.astype(sim.dtype))
    sim.set(F.PRESSURE, np.asarray(p).astype(sim.dtype))
    if origin is not None:
        sim.set_option("moment_origin", origin)
    return sim.body_force(per_plane=True)


@pytest.mark.parametrize("precision", PRECISIONS)
def test_constant_pressure_on_closed_bodies_gives_no_force_and_no_moment(precision):
    obs, labels, info, ncomp = model_of("two_boxes_and_a_stray_cell")
    D, H, W = (n - 2 for n in obs.shape)
    tot, pp = query(sim_of(W, H, D, precision), obs, np.full(obs.shape, 0.75), origin=(3.5, -2.25, 10.0))
    assert tot.shape == (4, 8) and pp.shape == (D, 4, 8)
    assert np.array_equal(tot[:, :6], np.zeros((4, 6))), tot
    assert list(tot[:, 6]) == [0, 2 * (11 * 6 + 6 * 8 + 8 * 11), 6 * 6 * 6, 6] and list(tot[:, 7]) == [0, 48, 36, 1]


@pytest.mark.parametrize("precision", PRECISIONS)
def test_linear_pressure_around_two_boxes(precision):
    """p = a + g . (x, y, z) with dyadic a, g and a dyadic origin: every sum is exact in any order.  Per body S is the
    closed form of an Lx x Ly x Lz box, Sx = -gx (Lx + 1) Ly Lz (likewise y, z), and M equals the model exactly; M about
    another origin equals shift_moment of the first."""
    import fluid_simulation_amd as F
    W, H, D = 37, 21, 18
    obs, big, small = two_boxes(W, H, D)
    a, g = 0.5, (0.25, -0.125, 0.0625)
    z, y, x = np.mgrid[0:D + 2, 0:H + 2, 0:W + 2]
    p = a + g[0] * x + g[1] * y + g[2] * z
    r0, r1 = (2.5, 7.25, -1.0), (18.0, 0.5, 9.75)
    sim = sim_of(W, H, D, precision)
    tot, pp = query(sim, obs, p, origin=r0)
    labels, info, ncomp = M.label_bodies(obs)
    rec, mag = M.body_records(obs, p, labels, 2, origin=r0)
    for k, (x0, x1, y0, y1, z0, z1) in ((1, big), (2, small)):
        L = (x1 - x0 + 1, y1 - y0 + 1, z1 - z0 + 1)
        want = [-g[0] * (L[0] + 1) * L[1] * L[2], -g[1] * (L[1] + 1) * L[0] * L[2], -g[2] * (L[2] + 1) * L[0] * L[1]]
        assert np.array_equal(tot[k, :3], want), (k, tot[k], want)
        assert tot[k, 6] == 2 * (L[0] * L[1] + L[1] * L[2] + L[2] * L[0]) and tot[k, 7] == L[1] * L[2]
    assert np.array_equal(pp, rec) and np.array_equal(tot, M.totals(rec))
    assert np.abs(tot[1:, 3:6]).min() > 0
    assert not tot[0].any()
    tot1 = query(sim, obs, p, origin=r1)[0]
    assert np.array_equal(tot1[:, :3], tot[:, :3])
    assert np.array_equal(tot1[:, 3:6], F.shift_moment(tot[:, 3:6], tot[:, :3], r0, r1))
    assert not np.array_equal(tot1[:, 3:6], tot[:, 3:6])


# ---- 3. random masks -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("shape", GRIDS)
def test_random_mask_matches_the_model(precision, shape):
    """Every S and M entry lies within (faces + 8) * 2^-52 * sum |term| of the model: the first-order worst case of an
    fp64 sum of `faces` terms in any order, for the kernel and for the model, plus one rounding per product."""
    import fluid_simulation_amd as F
    W, H, D = shape
    rng = np.random.default_rng(W * 1000 + H * 10 + D)
    obs = zeros(W, H, D)
    obs[1:-1, 1:-1, 1:-1] = rng.choice([0.0, 1.0, 0.5, 2.0, -1.0], size=(D, H, W), p=[0.6, 0.25, 0.05, 0.05, 0.05])
    p = (rng.standard_normal(obs.shape) * 3.0).astype(np.float32 if precision == "fp32" else np.float64)
    origin = (W / 3.0, 0.1, -2.7)
    sim = sim_of(W, H, D, precision)
    tot, pp = query(sim, obs, p, origin=origin)
    labels, info, ncomp = M.label_bodies(obs)
    B = min(ncomp, M.BODY_MAX)
    assert np.array_equal(sim.body_labels(), labels) and np.array_equal(info_raw(sim.body_info()), info)
    origin64 = [float(repr(float(v))) for v in origin]
    rec, mag = M.body_records(obs, p, labels, B, origin=origin64)
    assert pp.shape == rec.shape == (D, B + 1, 8)
    assert np.array_equal(pp[:, :, 6:], rec[:, :, 6:])                              # faces and frontal rows: exact
    err = np.abs(pp[:, :, :6] - rec[:, :, :6])
    bound = (rec[:, :, 6:7] + 8) * EPS * mag
    print("largest error / bound, planes:", np.max(err / np.maximum(bound, 1e-300)))
    assert np.all(err <= bound)
    mtot = M.totals(rec)
    err = np.abs(tot[:, :6] - mtot[:, :6])
    bound = (mtot[:, 6:7] + 8) * EPS * mag.sum(axis=0)
    print("largest error / bound, totals:", np.max(err / np.maximum(bound, 1e-300)))
    assert np.all(err <= bound) and np.array_equal(tot[:, 6:], mtot[:, 6:])
    assert np.array_equal(tot[:, 7], info[:, 11])
    # the whole-grid record is the plane records added in increasing z, bit for bit
    assert bits_equal(tot, M.totals(pp))
    # against the total force of fs_obstacle_force
    q = sim.obstacle_force()
    assert tot[:, 6].sum() == q["faces"]
    err = np.abs(tot[:, :3].sum(axis=0) - q["S"])
    bound = (q["faces"] + 8) * EPS * mag[:, :, :3].sum(axis=(0, 1))
    print("largest error / bound, against fs_obstacle_force:", np.max(err / np.maximum(bound, 1e-300)))
    assert np.all(err <= bound)


# ---- 4. determinism --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("precision", PRECISIONS)
def test_same_bits_twice_and_under_other_tuning_keys(precision):
    W, H, D = 64, 48, 20
    rng = np.random.default_rng(5)
    obs = boxes_and_specks()
    p = rng.standard_normal(obs.shape) * 3.0
    sim = sim_of(W, H, D, precision)
    tot, pp = query(sim, obs, p, origin=(1.1, 2.2, 3.3))
    tot2, pp2 = sim.body_force(per_plane=True)
    assert bits_equal(tot, tot2) and bits_equal(pp, pp2)
    for key, val in (("vortex_ry", 1), ("sweep_ry", 4), ("sweep_blocks", 64), ("sweep_zc", 3), ("project_kernels", "cell"),
                     ("sweep_fuse", 1)):
        sim.set_option(key, val)
    tot3, pp3 = sim.body_force(per_plane=True)
    assert bits_equal(tot, tot3) and bits_equal(pp, pp3)
    other = sim_of(W, H, D, precision, vortex_ry=1, sweep_ry=4)
    tot4, pp4 = query(other, obs, p, origin=(1.1, 2.2, 3.3))
    assert bits_equal(tot, tot4) and bits_equal(pp, pp4)


# ---- 5. the per-step log ---------------------------------------------------------------------------------------------------

def tunnel(solver="jacobi", **kw):
    import fluid_simulation_amd as F
    kw.setdefault("dump_every", 0)
    sim = F.Simulation(24, 16, 12, 1, acc=8, solver=solver, quiet=1, **kw)
    obs = zeros(24, 16, 12)
    put_box(obs, 6, 9, 5, 10, 4, 8)          # 4 x 6 x 5: body 1
    put_box(obs, 15, 17, 7, 9, 3, 5)         # 3 x 3 x 3: body 2
    sim.set(F.OBS, obs.astype(np.float32))
    return sim


def raw_of(rows):
    return np.stack([rows[n].astype(np.float64) for n in rows.dtype.names[:16]], axis=1)


@pytest.mark.parametrize("solver", ["jacobi", "mg"])
def test_log_matches_query_and_per_pass_replay(solver):
    """The second-projection columns of a step's rows = fs_body_force right after that step; the first-projection
    columns = the query on a second handle that replays the step's first half through the per-pass entry points."""
    import fluid_simulation_amd as F
    origin = (12.5, 8.0, 6.25)
    sim = tunnel(solver, body_force_log=8, moment_origin=origin)
    for _ in range(2):
        sim.run_one()
    state = {f: sim.get(f) for f in (F.VX, F.VY, F.VZ, F.OBS)}
    sim.run_one()
    after = sim.body_force()
    rows = sim.body_force_log()
    assert list(rows["step"]) == [1, 1, 1, 2, 2, 2, 3, 3, 3] and list(rows["body"]) == [0, 1, 2] * 3
    last = raw_of(rows[-3:])
    assert bits_equal(last[:, 8:14], after[:, :6]) and bits_equal(last[:, 14:], after[:, 6:])
    assert list(after[:, 6]) == [0, 2 * (4 * 6 + 6 * 5 + 5 * 4), 54] and list(after[:, 7]) == [0, 30, 9]
    assert np.abs(after[1:, :6]).min() > 0

    rep = tunnel(solver, moment_origin=origin)
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
    first = rep.body_force()
    assert bits_equal(last[:, 2:8], first[:, :6])
    # the derived columns: both impulses of the step
    dims = (sim.dt, sim.speed, 24, 16, 12)
    force, coeff = F.pressure_force(first[:, :3] + after[:, :3], after[:, 7], *dims)
    torque, cm = F.pressure_moment(first[:, 3:6] + after[:, 3:6], after[:, 7], 1.0, *dims)
    for k, a in enumerate("xyz"):
        assert bits_equal(rows["f" + a][-3:], force[:, k]) and bits_equal(rows["t" + a][-3:], torque[:, k])
        assert np.array_equal(rows["c" + a][-3:], coeff[:, k], equal_nan=True)
        assert np.array_equal(rows["cm" + a][-3:], cm[:, k], equal_nan=True)


def test_log_leaves_the_run_unchanged():
    import fluid_simulation_amd as F
    out = {}
    for on in (0, 4):
        sim = tunnel(body_force_log=on)
        for _ in range(3):
            sim.run_one()
        out[on] = [sim.get(f) for f in range(11)]
        if on:
            assert len(sim.body_force_log()) == 9
        sim.close()
    for f in range(11):
        assert bits_equal(out[0][f], out[4][f]), F.FIELD_NAMES[f]


def test_log_wraps_and_reports_the_overwritten_steps():
    sim = tunnel(body_force_log=2)
    for _ in range(5):
        sim.step()
    rows, dropped = sim.body_force_log(with_dropped=True)
    assert list(rows["step"]) == [4, 4, 4, 5, 5, 5] and dropped == 3
    rows, dropped = sim.body_force_log(with_dropped=True)       # drained
    assert len(rows) == 0 and dropped == 0
    sim.step()
    rows, dropped = sim.body_force_log(with_dropped=True)
    assert list(rows["step"]) == [6, 6, 6] and dropped == 0
    sim.step()
    sim.set_option("body_force_log", 3)                          # re-setting clears
    assert len(sim.body_force_log()) == 0


def test_log_off_launches_nothing_and_on_two_per_step():
    for n, want in ((0, 0), (4, 6)):
        sim = tunnel(body_force_log=n, profile=1)
        for _ in range(3):
            sim.step()
        sim.sync()
        assert sim.timing("body_forces")[1] == want
        assert sim.timing("forces")[1] == 0
        if n:
            sim.body_force()
            sim.sync()
            assert sim.timing("body_forces")[1] == want + 1
        sim.close()


def test_changing_obs_or_the_origin_clears_the_log():
    import fluid_simulation_amd as F
    sim = tunnel(body_force_log=8)
    sim.step()
    sim.step()
    obs = sim.get(F.OBS)
    put_box(obs, 20, 21, 2, 3, 9, 10)                            # a third body, mid-run
    sim.set(F.OBS, obs)
    sim.step()                                                   # relabels at the top of the step: steps 1, 2 are gone
    rows = sim.body_force_log()
    assert list(rows["step"]) == [3] * 4 and list(rows["body"]) == [0, 1, 2, 3]
    assert list(rows["faces"]) == [0, 148, 54, 24]
    assert sim.body_count == 3
    sim.step()
    sim.set_option("moment_origin", "1,2,3")
    assert len(sim.body_force_log()) == 0
    sim.step()
    rows = sim.body_force_log()
    assert list(rows["step"]) == [5] * 4
    sim.step()
    sim.label_bodies()                                           # a forced relabelling clears it as well
    assert len(sim.body_force_log()) == 0
    # the moments of the log are taken about the origin in force
    sim.step()
    rows = raw_of(sim.body_force_log())
    assert bits_equal(rows[:, 8:14], sim.body_force()[:, :6])


# ---- 6. errors ---------------------------------------------------------------------------------------------------------------

def test_fsnull_slab_handle_refuses():
    import fluid_simulation_amd as F
    sim = F.Simulation(16, 16, 16, 1, quiet=1)
    sim.comm_init(0, 2, b"FSNULL:".ljust(128, b"\0"))
    for call in (sim.label_bodies, sim.body_labels, sim.body_info, sim.body_force, sim.body_force_log,
                 lambda: sim.set_option("body_force_log", 4)):
        with pytest.raises(F.FluidsimError) as e:
            call()
        assert e.value.code == -1 and "single-GPU" in str(e.value)
    # the other order: a handle with the log on cannot become a slab
    sim = F.Simulation(16, 16, 16, 1, quiet=1, body_force_log=4)
    with pytest.raises(F.FluidsimError) as e:
        sim.comm_init(0, 2, b"FSNULL:".ljust(128, b"\0"))
    assert e.value.code == -1 and "body_force_log" in str(e.value)
    sim.set_option("body_force_log", 0)
    sim.comm_init(0, 2, b"FSNULL:".ljust(128, b"\0"))


def test_too_few_rows_and_bad_origin():
    import ctypes as C

    import fluid_simulation_amd as F
    sim = tunnel(body_force_log=4)
    sim.step()
    n = C.c_long()
    buf = np.zeros((3, 16))
    for fn, args in ((sim._L.fs_body_info, (buf.ctypes.data, 2, C.byref(n))),
                     (sim._L.fs_body_force, (buf.ctypes.data, 2, C.byref(n), None)),
                     (sim._L.fs_body_force_log, (buf.ctypes.data, 2, C.byref(n), None))):
        assert fn(sim._h, *args) == F._lib.EINVAL
        assert n.value == 3
    assert sim._L.fs_body_labels(sim._h, buf.ctypes.data, 7) == F._lib.EINVAL
    assert len(sim.body_force_log()) == 3                        # the refused drain took nothing
    for bad in ("", "1,2", "1,2,3,4", "1;2;3", "a,b,c", "1,2,nan", "1,2,inf", "1,2,3x"):
        with pytest.raises(F.FluidsimError) as e:
            sim.set_option("moment_origin", bad)
        assert e.value.code == -1, bad
    with pytest.raises(F.FluidsimError):
        sim.set_option("body_force_log", -1)
    with pytest.raises(F.FluidsimError):
        sim.set_option("body_force_log", (1 << 20) + 1)
    sim.set_option("moment_origin", " 1.5,-2e0,+3")
    sim.set_option("moment_origin", (0.5, 1, 2))


# ---- 7. simulation.out --body-forces ---------------------------------------------------------------------------------------

def test_cli_body_forces_csv_matches_python(tmp_path):
    import fluid_simulation_amd as F
    exe = os.path.join(ROOT, "simulation.out")
    assert os.path.exists(exe), "simulation.out is built by __graft_entry__.build()"
    meta, arr = load_golden("g3_sphere_plus_plate_40x24x24")
    W, H, D = meta["W"], meta["H"], meta["D"]
    sphere, plate = os.path.join(GOLDEN, "sphere_24x12.stl"), os.path.join(GOLDEN, "plate_ascii.stl")
    csv = tmp_path / "b.csv"
    env = {k: v for k, v in os.environ.items() if not k.startswith("FS_")}
    subprocess.run([exe, "--grid", "%dx%dx%d" % (W, H, D), "--steps", "3", "--body-forces", str(csv), "--moment-origin", "20.5,12.5,12.5",
                    "--seed", str(meta["seed"]), "--stl", sphere + ",0.4,0,0,0,-8,0,0", "--stl", plate + ",0.7,0,0,0,6,0,0",
                    "--dump-every", "0", "--dump-dir", str(tmp_path), "--quiet"], check=True, cwd=str(tmp_path), env=env, timeout=600)
    lines = csv.read_text().splitlines()
    head = [ln for ln in lines if ln.startswith("#")]
    body = [ln for ln in lines if not ln.startswith("#")]
    assert body[0].split(",")[:16] == list(F.BODY_LOG_DTYPE.names[:16]) and body[0].split(",") == list(F.BODY_LOG_DTYPE.names)
    got = np.array([[float(v) for v in ln.split(",")] for ln in body[1:]])
    sim = F.Simulation(W, H, D, 3, quiet=1, dump_every=0, body_force_log=3, voxel_seed=meta["seed"], moment_origin=(20.5, 12.5, 12.5))
    F.loadSTLIntoObstacles(sphere, sim, 0.4, 0.0, 0.0, 0.0, -8.0, 0.0, 0.0)
    F.loadSTLIntoObstacles(plate, sim, 0.7, 0.0, 0.0, 0.0, 6.0, 0.0, 0.0)
    sim.run()
    rows = sim.body_force_log()
    want = np.stack([rows[k].astype(np.float64) for k in rows.dtype.names], axis=1)
    assert want.shape == (9, 28) and list(want[:3, 15]) == [0, meta_frontal(sim, 1), meta_frontal(sim, 2)]
    assert np.array_equal(got[:, :16], want[:, :16])
    assert np.allclose(got[:, 16:], want[:, 16:], rtol=1e-12, atol=0, equal_nan=True)
    info = sim.body_info()
    assert list(info["cells"]) == [0, 442, 280]
    table = np.array([[int(v) for v in ln[1:].split(",")] for ln in head[1:]])
    assert np.array_equal(table[:, 1:], info_raw(info).astype(np.int64)) and list(table[:, 0]) == [0, 1, 2]


def meta_frontal(sim, k):
    return int(sim.body_info()["frontal"][k])
