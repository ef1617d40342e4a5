"""What crosses the library's boundary, against tests/boundary_model.py: fs_get_field / fs_set_field as bit patterns at the
edges of the number formats and of the 64x4 pack / unpack block; frame dumps against what fs_get_field returns after each
step, under every solver and both precisions, strided, synchronous, by hand and across runs; the staging ring with the writer
behind; write errors on a full device; and the run statistics, printed numbers included."""
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest

import boundary_model as M

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
PRECISIONS = ("fp32", "fp64")
EINVAL, EIO = -1, -2      # FS_EINVAL, FS_EIO (include/fluidsim.h)
# the smallest grids that reach each edge: a frame that stays in stdio's buffer; W + 2 = 64 and 65 with H + 2 = 4 and 5, one
# lane each side of the 64x4 block of pack / unpack; a 257-cell row, wider than the statistics kernel's 256 threads;
# 32 * 33 = 1056 rows, more than its 1024 blocks; a frame of several stdio buffers
G_TINY, G_64, G_65, G_ROW, G_ROWS, G_BUFS = (5, 3, 2), (62, 2, 3), (63, 3, 2), (255, 2, 1), (4, 30, 31), (30, 20, 10)
GRIDS = (G_TINY, G_64, G_65, G_ROW, G_ROWS, G_BUFS)
TRANSFER_GRIDS = (G_64, G_65, G_ROW)
FRAME_FIELDS = None          # set by F(): DENS, OBS, VX, VY, VZ in file order
NAMES = tuple(n + ".bin" for n in M.FILES)


@pytest.fixture(scope="module")
def F():
    import fluid_simulation_amd as F
    global FRAME_FIELDS
    FRAME_FIELDS = (F.DENS, F.OBS, F.VX, F.VY, F.VZ)
    return F


def shape_of(grid):
    W, H, D = grid
    return (D + 2, H + 2, W + 2)


def handle(F, grid, precision, iter=1, **kw):
    kw.setdefault("quiet", 1)
    return F.Simulation(grid[0], grid[1], grid[2], iter, precision=precision, **kw)


def np_dtype(precision):
    return np.float64 if precision == "fp64" else np.float32


def convert(a, dtype):
    """the model's conversion between float formats (identity where the format stays)"""
    dtype = np.dtype(dtype)
    if a.dtype == dtype:
        return a
    return M.narrow(a) if dtype == np.float32 else M.widen(a)


def same_bits(got, want, exact):
    assert got.dtype == want.dtype and got.shape == want.shape
    if not exact:
        got, want = M.canon(got), M.canon(want)
    return np.array_equal(M.bits(got), M.bits(want))


def seeded_with_edges(grid, dtype, seed):
    """a standard-normal field with the whole edge table scattered over it, ghosts and the corners of the padded box included"""
    rng = np.random.default_rng(seed)
    shape = shape_of(grid)
    a = rng.standard_normal(shape).astype(dtype).reshape(-1)
    e = M.edge_values(dtype)
    assert a.size > 2 * e.size
    where = rng.choice(a.size, size=2 * e.size, replace=False)
    a[where] = np.concatenate([e, e[::-1]])
    a = a.reshape(shape)
    a[0, 0, 0], a[-1, -1, -1], a[0, -1, -1], a[-1, 0, 0], a[1, 1, -1], a[1, -1, 1] = e[:6]
    return a


# ---------------------------------------------------------------------------------------------------- transfers
@pytest.mark.parametrize("grid", TRANSFER_GRIDS)
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("precision", PRECISIONS)
def test_float_transfers_are_the_model_bit_for_bit(F, precision, dtype, grid):
    """set in `dtype`, get in both float dtypes: stored = the array in the handle's format, fetched = that in the host's.
    A path on which the format never changes keeps every bit, NaN payloads included; a converting one yields the model's
    bits once every NaN is mapped to the canonical one."""
    sim = handle(F, grid, precision)
    a = seeded_with_edges(grid, dtype, 3)
    sim.set(F.VY, a)
    stored = convert(a, np_dtype(precision))
    for out in (np.float32, np.float64):
        got = sim.get(F.VY, dtype=out)
        exact = np.dtype(dtype) == np_dtype(precision) == np.dtype(out)
        assert same_bits(got, convert(stored, out), exact), (precision, dtype, out, grid)
        if exact:
            assert np.isnan(got).sum() >= 8
    sim.close()


@pytest.mark.parametrize("grid", TRANSFER_GRIDS)
@pytest.mark.parametrize("precision", PRECISIONS)
def test_uint8_transfers(F, precision, grid):
    """set: every byte value becomes that number; get: truncation toward zero of values in [0, 256)"""
    sim = handle(F, grid, precision)
    rng = np.random.default_rng(4)
    shape = shape_of(grid)
    b = rng.integers(0, 256, size=shape, dtype=np.uint8)
    b.reshape(-1)[:256] = np.arange(256, dtype=np.uint8)
    b[-1, -1, -1], b[0, 0, -1] = 255, 254
    sim.set(F.DENS, b)
    assert same_bits(sim.get(F.DENS), b.astype(np_dtype(precision)), True)
    assert np.array_equal(sim.get(F.DENS, dtype=np.uint8), b)
    vals = np.array([0, 1, 2, 255, 0.5, 1.9, 254.999], dtype=np_dtype(precision))
    assert vals[-1] < 255
    a = vals[rng.integers(0, len(vals), size=shape)]
    a.reshape(-1)[:len(vals)] = vals
    a[-1, -1, -1], a[0, 0, -1] = vals[6], vals[5]
    sim.set(F.VX, a)
    got = sim.get(F.VX, dtype=np.uint8)
    assert got.dtype == np.uint8 and np.array_equal(got, M.to_u8(a))
    assert sorted(set(got.reshape(-1).tolist())) == [0, 1, 2, 254, 255]
    sim.close()


@pytest.mark.parametrize("grid", GRIDS)
@pytest.mark.parametrize("precision", PRECISIONS)
def test_a_field_of_indices_comes_back_as_indices(F, precision, grid):
    """every cell holds its own linear index (exact in float32 below 2^24): a pitch or stride error cannot cancel"""
    sim = handle(F, grid, precision)
    shape = shape_of(grid)
    n = int(np.prod(shape))
    assert n < 2 ** 24
    for src in (np.float32, np.float64):
        idx = np.arange(n, dtype=src).reshape(shape)
        sim.set(F.VZ, idx)
        for out in (np.float32, np.float64):
            assert np.array_equal(sim.get(F.VZ, dtype=out), idx.astype(out)), (src, out)
        sim.set(F.VZ, np.zeros(shape, dtype=src))
    sim.close()


def test_transfer_errors(F):
    sim = handle(F, G_64, "fp32")
    L, h = sim._L, sim._h
    n = int(np.prod(shape_of(G_64)))
    buf = np.zeros(n + 1, dtype=np.float64)
    assert L.fs_padded_size(h) == n
    for call in (L.fs_get_field, L.fs_set_field):
        assert call(h, F.VX, buf.ctypes.data, n, 4) == 0
        assert call(h, F.VX, buf.ctypes.data, n - 1, 4) == EINVAL and b"expected" in L.fs_last_error()
        assert call(h, F.VX, buf.ctypes.data, n + 1, 8) == EINVAL
        assert call(h, F.VX, buf.ctypes.data, n, 2) == EINVAL and b"elem_size" in L.fs_last_error()
        assert call(h, F.VX, buf.ctypes.data, n, 0) == EINVAL
        assert call(h, F.VX, None, n, 4) == EINVAL and b"null" in L.fs_last_error()
        assert call(h, 11, buf.ctypes.data, n, 4) == EINVAL
    sim.close()


# ---------------------------------------------------------------------------------------------------- frames
STEPS = 5
OBSTACLES = {G_TINY: [(3, 2, 1)],
             G_BUFS: [(x, y, z) for x in (10, 11, 12) for y in (8, 9) for z in (4, 5)],
             (32, 16, 8): [(x, y, z) for x in (10, 11) for y in (6, 7, 8) for z in (3, 4)]}
_twins = {}


def tunnel(F, grid, precision, solver, iter, **kw):
    sim = handle(F, grid, precision, iter=iter, solver=solver, acc=4, **kw)
    for c in OBSTACLES[grid]:
        sim.addObstacle(*c)
    return sim


def twin_frames(F, grid, precision, solver, steps=2 * STEPS):
    """frame_bytes of the state after each of `steps` run_one calls of a handle built like the dumping one (made once)"""
    key = (grid, precision, solver)
    if key not in _twins:
        sim = tunnel(F, grid, precision, solver, 1, dump_every=0)
        rec = []
        for _ in range(steps):
            sim.run_one()
            rec.append(M.frame_bytes([sim.get(f) for f in FRAME_FIELDS]))
        sim.close()
        assert len(set(r[0] for r in rec)) == steps and len(set(r[2] for r in rec)) == steps       # the state moves
        _twins[key] = rec
    return _twins[key]


def files_of(d):
    return [open(os.path.join(str(d), n), "rb").read() for n in NAMES]


def joined(rec, steps):
    """the five files that hold the frames of the 1-based `steps`"""
    return [b"".join(rec[s - 1][k] for s in steps) for k in range(5)]


def differing(got, want):
    return [(NAMES[k], len(got[k]), len(want[k])) for k in range(5) if got[k] != want[k]]


FRAME_CASES = [(s, p, g) for s in ("jacobi", "gs_lex", "rbsor", "mg") for p in PRECISIONS
               for g in ((G_TINY, G_BUFS) + (((32, 16, 8),) if s == "mg" else ()))]


@pytest.mark.parametrize("solver,precision,grid", FRAME_CASES)
def test_frames_of_a_run_hold_the_state_after_each_step(F, tmp_path, solver, precision, grid):
    rec = twin_frames(F, grid, precision, solver)
    sim = tunnel(F, grid, precision, solver, STEPS, dump_every=1, dump_dir=str(tmp_path))
    sim.run()
    sim.close()
    assert not differing(files_of(tmp_path), joined(rec, range(1, STEPS + 1)))
    if solver == "mg" and grid == (32, 16, 8):
        probe = tunnel(F, grid, precision, solver, 1, dump_every=0)
        probe.run_one()
        assert probe._geti("mg_levels") >= 2
        probe.close()


@pytest.mark.parametrize("grid", [G_TINY, G_BUFS])
@pytest.mark.parametrize("precision", PRECISIONS)
def test_dump_stride_last_frame_never_and_synchronous(F, tmp_path, precision, grid):
    rec = twin_frames(F, grid, precision, "jacobi")

    def run(name, **kw):
        d = tmp_path / name
        d.mkdir()
        sim = tunnel(F, grid, precision, "jacobi", STEPS, dump_dir=str(d), **kw)
        sim.run()
        sim.close()
        return d

    assert not differing(files_of(run("every2", dump_every=2)), joined(rec, (2, 4)))
    assert not differing(files_of(run("last", dump_every=-1)), joined(rec, (STEPS,)))
    never = run("never", dump_every=0)
    assert all(not (never / n).exists() or (never / n).stat().st_size == 0 for n in NAMES)
    sync, asyn = files_of(run("sync", dump_every=1, dump_async=0)), files_of(run("async", dump_every=1, dump_async=1))
    assert sync == asyn and not differing(sync, joined(rec, range(1, STEPS + 1)))


@pytest.mark.parametrize("grid", [G_TINY, G_BUFS])
@pytest.mark.parametrize("precision", PRECISIONS)
def test_dump_by_hand_and_second_run(F, tmp_path, precision, grid):
    # fs_dump_frame after each run_one, outside fs_run: the frames are what the same handle's get() returns
    a, b = tmp_path / "hand", tmp_path / "again"
    a.mkdir()
    b.mkdir()
    sim = tunnel(F, grid, precision, "jacobi", 1, dump_dir=str(a))
    own = []
    for _ in range(3):
        sim.run_one()
        sim.dump_frame()
        own.append(M.frame_bytes([sim.get(f) for f in FRAME_FIELDS]))
    sim.sync()
    sim.close()
    assert not differing(files_of(a), joined(own, (1, 2, 3)))
    assert own == twin_frames(F, grid, precision, "jacobi")[:3]
    # a second fs_run into the same directory: the files hold the second run only, continuing from the first run's state
    rec = twin_frames(F, grid, precision, "jacobi")
    sim = tunnel(F, grid, precision, "jacobi", STEPS, dump_every=1, dump_dir=str(b))
    sim.run()
    sim.run()
    sim.close()
    assert not differing(files_of(b), joined(rec, range(STEPS + 1, 2 * STEPS + 1)))


@pytest.mark.parametrize("grid", [G_TINY, G_65])
def test_fp64_frames_are_narrowed_as_the_model_narrows(F, tmp_path, grid):
    """fields seeded with the edge table are dumped without a step: ties, overflow, float32 subnormals and NaNs in a frame"""
    sim = handle(F, grid, "fp64", dump_dir=str(tmp_path))
    shape = shape_of(grid)
    fields = [seeded_with_edges(grid, np.float64, 20 + k) if k else np.arange(np.prod(shape), dtype=np.float64).reshape(shape)
              for k in range(5)]
    for f, a in zip(FRAME_FIELDS, fields):
        sim.set(f, a)
    sim.dump_frame()
    sim.sync()
    sim.close()
    for name, got, want in zip(NAMES, files_of(tmp_path), M.frame_bytes(fields)):
        got, want = np.frombuffer(got, dtype=np.float32), np.frombuffer(want, dtype=np.float32)
        assert same_bits(got, want, False), name
        assert name == NAMES[0] or (np.isinf(want).sum() >= 4 and ((np.abs(want) < 2.0 ** -126) & (want != 0)).sum() >= 4)


RING_GRID = (96, 64, 48)


def test_staging_ring_with_the_writer_behind(F, tmp_path):
    """Eight steps of one sweep each, a 6.5 MB frame after every one, asynchronously: the steps outrun the writer, so a dump
    finds its staging slot still on its way to disk and has to wait (dump_slot_waits counts that), and all eight frames must
    still be the state after their step.  Measured on an MI355X machine: on this grid, 96x64x48, dump_slot_waits was 6 after
    the eight frames, in each of four runs, so the grid did not have to grow."""
    grid, steps = RING_GRID, 8

    def make(**kw):
        sim = handle(F, grid, "fp32", iter=steps, acc=1, **kw)
        sim.addObstacle(10, 10, 10)
        return sim

    twin = make(dump_every=0)
    rec = []
    for _ in range(steps):
        twin.run_one()
        rec.append(M.frame_bytes([twin.get(f) for f in FRAME_FIELDS]))
    twin.close()
    sim = make(dump_every=1, dump_async=1, dump_dir=str(tmp_path))
    assert sim._geti("dump_slot_waits") == 0
    sim.run()
    waits = sim._geti("dump_slot_waits")
    sim.close()
    print("dump_slot_waits = %d over %d frames of %dx%dx%d" % ((waits, steps) + grid))
    assert not differing(files_of(tmp_path), joined(rec, range(1, steps + 1)))
    assert waits > 0


# ---------------------------------------------------------------------------------------------------- write errors
def dev_full_or_skip():
    try:
        with open("/dev/full", "wb"):
            pass
    except OSError:
        pytest.skip("/dev/full cannot be opened for writing")


@pytest.mark.parametrize("asynchronous", [0, 1])
@pytest.mark.parametrize("grid", [G_TINY, G_BUFS])
def test_a_full_device_reaches_the_caller_and_the_handle_recovers(tmp_path, grid, asynchronous):
    """five symlinks to /dev/full as the dump files: run() raises FS_EIO without hanging (a child process under a time limit,
    tests/dump_error_worker.py); with dump_dir set to a good directory the same handle runs again and writes its frames"""
    dev_full_or_skip()
    full, good = tmp_path / "full", tmp_path / "good"
    full.mkdir()
    good.mkdir()
    for n in NAMES:
        os.symlink("/dev/full", str(full / n))
    r = subprocess.run([sys.executable, os.path.join(HERE, "dump_error_worker.py"), str(grid[0]), str(grid[1]), str(grid[2]),
                        str(asynchronous), str(full), str(good), str(tmp_path / "result.json")],
                       capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    res = json.load(open(str(tmp_path / "result.json")))
    print(res)
    assert res["first_run"] == "FluidsimError" and res["code"] == EIO, res
    assert res["second_run"] == "ok" and res["frames_equal"] and res["bytes"] == 3 * 4 * int(np.prod(shape_of(grid))), res


# ---------------------------------------------------------------------------------------------------- statistics
def exact(v):
    return (float(v[0]), float(v[1]), float(v[2]))


@pytest.mark.parametrize("grid", GRIDS)
@pytest.mark.parametrize("precision", PRECISIONS)
def test_statistics_exact_on_integer_fields(F, precision, grid):
    sim = handle(F, grid, precision)
    shape = shape_of(grid)
    n = int(np.prod(shape))
    dt = np_dtype(precision)
    sim.set(F.VX, np.ones(shape, dtype=dt))
    assert sim.stats(F.VX) == (float(n), 1.0, 1.0)                 # pitch padding is not counted, ghosts are
    rng = np.random.default_rng(6)
    base = rng.integers(-1000, 1001, size=shape).astype(dt)
    top = float(2 ** 20 - 1)
    last = n - 1
    places = [(0, last), (last, 0), (n // 2, n // 3)]
    if grid == G_ROW:
        places += [(256, 2 * 257 + 256), (3 * 257 + 256, 257 + 255)]          # the last lane of a 257-cell row
    if grid == G_ROWS:
        places += [(1055 * 6 + 2, 1024 * 6 + 1), (1023 * 6, 1055 * 6)]          # row 1055 of 1056, and the rows around 1024
    for lo, hi in places:
        a = base.copy().reshape(-1)
        a[lo], a[hi] = -top, top
        sim.set(F.DENS, a.reshape(shape))
        want = M.stats(a)
        assert want[1:] == (-top, top) and want[0] == float(np.sum(a.astype(np.int64)))
        assert exact(sim.stats(F.DENS)) == want, (lo, hi)
    sim.close()


@pytest.mark.parametrize("precision", PRECISIONS)
def test_statistics_of_special_fields(F, precision):
    sim = handle(F, G_65, precision)
    shape, dt = shape_of(G_65), np_dtype(precision)
    sim.set(F.VY, np.full(shape, np.inf, dtype=dt))
    assert sim.stats(F.VY) == (math.inf, math.inf, math.inf)
    sim.set(F.VY, np.full(shape, -np.inf, dtype=dt))
    assert sim.stats(F.VY) == (-math.inf, -math.inf, -math.inf)
    if precision == "fp64":
        sim.set(F.VY, np.full(shape, 1e305))
        assert sim.stats(F.VY)[1:] == (1e305, 1e305)
        sim.set(F.VY, np.full(shape, -1e305))
        assert sim.stats(F.VY)[1:] == (-1e305, -1e305)
    rng = np.random.default_rng(8)
    a = rng.integers(-50, 51, size=shape).astype(dt)
    for cell in ((0, 0, 1), (1, 2, 3), (shape[0] - 1, shape[1] - 1, shape[2] - 1)):     # a NaN anywhere but in cell (0, 0, 0)
        b = a.copy()
        b[cell] = np.nan
        sim.set(F.VY, b)
        s, lo, hi = sim.stats(F.VY)
        want = M.stats(b)
        assert math.isnan(s) and math.isnan(want[0]) and (lo, hi) == want[1:], cell
    sim.close()


@pytest.mark.parametrize("grid", [G_ROW, G_ROWS])
@pytest.mark.parametrize("precision", PRECISIONS)
def test_statistics_sum_within_the_bound_of_any_order(F, precision, grid):
    """a sum of n float64 numbers in any order is within (n - 1) 2^-53 sum|v| of the exact one; min and max are exact"""
    sim = handle(F, grid, precision)
    a = np.random.default_rng(9).standard_normal(shape_of(grid)).astype(np_dtype(precision))
    sim.set(F.VZ, a)
    s, lo, hi = sim.stats(F.VZ)
    want = M.stats(a)
    bound = (a.size - 1) * 2.0 ** -53 * float(np.abs(a.astype(np.float64)).sum())
    print("sum %r model %r difference %g bound %g" % (s, want[0], abs(s - want[0]), bound))
    assert abs(s - want[0]) <= bound and (lo, hi) == want[1:]
    sim.close()
