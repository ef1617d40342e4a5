"""fs_streamlines on the MI355X against oracle/streamlines_ref.py, bit for bit, on the cases of tests/streamlines_cases.py:
analytic fields loaded with Simulation.set, ghost layer included, so the expected answer needs no GPU and
tests/test_streamlines_cases_cpu.py has shown that every case reaches what it is there for and that no decision in it hangs on
a rounding.  The restatement runs with the kernel's norm, sqrt((u*u + v*v) + w*w); everything else in it is the chain of IEEE
double operations the kernel and the host bookkeeping perform (the library is built with -ffp-contract=off), so the lines, in
order, every coordinate and every colour argument are compared as bit patterns; a NaN colour (a NaN cell in a velocity array)
must be NaN on both sides.  No tolerance anywhere in this file.

Then the two entry points (Simulation.streamlines, viewer.generate_streamlines with and without a colour map), the lifetime
of the result in the handle, the bounding box after the body moved or vanished, slab handles, and no effect on the fields."""
import ctypes

import numpy as np
import pytest

import streamlines_cases as C
from conftest import ball_mask, bits_equal

pytestmark = pytest.mark.gpu
cases = pytest.mark.parametrize("name", C.NAMES + [C.EXACT["name"]])
VIEWER_CASES = ["ball-20-gap", "long-row", "wall-z-fp32", "stagnant", "soft-mask", "ghosts", "inf-cell", "nan-cell", "unit-1x1x1",
                "step-negative", "proximity-0"]
_handles = {}


@pytest.fixture(scope="module")
def F():
    import fluid_simulation_amd as F
    return F


def loaded(F, name):
    """the handle of the case's grid and precision (one per pair, reused) holding the case's four arrays"""
    case = C.BY_NAME[name]
    key = (case["shape"], case["precision"])
    if key not in _handles:
        W, H, D = case["shape"]
        _handles[key] = [F.Simulation(W, H, D, 1, precision=case["precision"], quiet=1, dump_every=0), None]
    sim, holds = _handles[key]
    if holds != name:
        for which, a in zip((F.VX, F.VY, F.VZ, F.OBS), C.fields(name)):
            sim.set(which, C.as_stored(a))
        _handles[key][1] = name
    return sim


def call_args(par):
    par = dict(par)
    par["vel_change_threshold"] = par.pop("threshold")
    return par


def same_colours(got, want):
    got = np.asarray(got, dtype=np.float64)
    want = np.array([float(v) for v in want], dtype=np.float64)
    if got.shape != want.shape or not np.array_equal(np.isnan(got), np.isnan(want)):
        return False
    ok = ~np.isnan(want)
    return bits_equal(got[ok], want[ok])


def assert_same(name, got, gnorm, want, wnorm):
    equal = len(got) == len(want) and all(bits_equal(a, np.asarray(b, dtype=np.float64)) for a, b in zip(got, want))
    print("%s: %d lines, %d points (expected %d, %d), coordinates bit-equal: %s, colours bit-equal: %s"
          % (name, len(got), sum(len(l) for l in got), len(want), sum(len(l) for l in want), equal, same_colours(gnorm, wnorm)))
    assert len(got) == len(want), (len(got), len(want))
    assert [a.shape for a in got] == [b.shape for b in want]
    for i, (a, b) in enumerate(zip(got, want)):
        assert bits_equal(a, np.asarray(b, dtype=np.float64)), (name, i, float(np.abs(a - b).max()))
    assert same_colours(gnorm, wnorm), (name, gnorm, wnorm)


@cases
def test_lines_and_colours_bit_for_bit(F, name):
    sim = loaded(F, name)
    want, wnorm, _ = C.expected(name)
    got, gnorm = sim.streamlines(**call_args(C.BY_NAME[name]["par"]))
    assert gnorm.dtype == np.float64 and all(l.dtype == np.float64 for l in got)
    assert_same(name, got, gnorm, want, wnorm)
    if name == "nan-cell":
        assert len(gnorm) > 0 and np.all(np.isnan(gnorm))
    if name == "inf-cell":
        assert len(gnorm) > 0 and np.all(gnorm == 0.0)


@pytest.mark.parametrize("name", VIEWER_CASES)
def test_viewer_entry_point(F, name):
    """viewer.generate_streamlines on the arrays the GUI holds: the same lines; without a colour map the same colour
    arguments, with one its values.  The soft mask goes through here as the array it is, not as a 0/1 mask of it."""
    from fluid_simulation_amd import viewer
    case = C.BY_NAME[name]
    assert case["precision"] == "fp32"
    want, wnorm, _ = C.expected(name)
    vx, vy, vz, obs = C.fields(name)
    par = call_args(case["par"])
    lines, colours = viewer.generate_streamlines(vx, vy, vz, obs, **par)
    assert isinstance(colours, list)
    assert_same(name + " (viewer)", lines, colours, want, wnorm)
    seen = []

    def cmap(v):
        seen.append(v)
        return (0.25, 0.5, 0.75, 1.0)
    lines2, rgba = viewer.generate_streamlines(vx, vy, vz, obs, cmap=cmap, **par)
    assert len(lines2) == len(want) and all(bits_equal(a, b) for a, b in zip(lines2, lines))
    assert all(type(v) is float for v in seen) and same_colours(seen, wnorm)
    assert len(rgba) == len(want) and all(c.shape == (4,) and c.tolist() == [0.25, 0.5, 0.75, 1.0] for c in rgba)


def raw_fetch(sim, n_lines, n_points, which=(True, True, True)):
    off = np.full(n_lines + 1, -7, dtype=np.int64)
    pts = np.full((n_points, 3), -7.0)
    norm = np.full(n_lines, -7.0)
    rc = sim._L.fs_streamlines_fetch(sim._h, off.ctypes.data if which[0] else None, pts.ctypes.data if which[1] else None,
                                     norm.ctypes.data if which[2] else None)
    return rc, off, pts, norm


def test_result_lifetime_in_the_handle(F):
    big, small = "ball-20", "ball-20-gap"
    sim = loaded(F, big)
    first = sim.streamlines(**call_args(C.BY_NAME[big]["par"]))
    again = sim.streamlines(**call_args(C.BY_NAME[big]["par"]))
    assert len(first[0]) == len(again[0]) > 0 and all(bits_equal(a, b) for a, b in zip(first[0], again[0]))
    assert bits_equal(first[1], again[1])
    # a second call replaces the first result
    want, wnorm, _ = C.expected(small)
    second = sim.streamlines(**call_args(C.BY_NAME[small]["par"]))
    assert 0 < len(second[0]) < len(first[0])
    assert_same(small, second[0], second[1], want, wnorm)
    # the counts are optional, and so is each array of the fetch
    L = sim._L
    par = C.BY_NAME[small]["par"]
    args = (sim._h, par["density"], float(par["proximity"]), par["max_length"], float(par["step_size"]), float(par["threshold"]))
    assert L.fs_streamlines(*args, None, None) == 0
    nl, npts = ctypes.c_long(-1), ctypes.c_long(-1)
    assert L.fs_streamlines(*args, ctypes.byref(nl), None) == 0 and nl.value == len(want)
    assert L.fs_streamlines(*args, None, ctypes.byref(npts)) == 0 and npts.value == sum(len(l) for l in want)
    rc, off, pts, norm = raw_fetch(sim, nl.value, npts.value)
    assert rc == 0 and off[0] == 0 and off[-1] == npts.value and np.array_equal(np.diff(off), [len(l) for l in want])
    assert bits_equal(pts, np.concatenate(want)) and same_colours(norm, wnorm)
    for k in range(3):
        which = tuple(i == k for i in range(3))
        rc, o, p, n = raw_fetch(sim, nl.value, npts.value, which)
        assert rc == 0
        for filled, got, ref in zip(which, (o, p, n), (off, pts, norm)):
            assert np.array_equal(got, ref) if filled else np.all(got == -7)
    assert L.fs_streamlines_fetch(sim._h, None, None, None) == 0
    # a refused call leaves an empty result: the counts are not written, and a fetch returns the single offset 0
    for bad in (dict(density=-1), dict(max_length=-2), dict(density=5000), dict(max_length=1000001), dict(step_size=float("nan")),
                dict(proximity=float("nan")), dict(vel_change_threshold=float("nan"))):
        sim.streamlines(**call_args(par))
        with pytest.raises(F.FluidsimError):
            sim.streamlines(**dict(call_args(par), **bad))
        rc, off, pts, norm = raw_fetch(sim, nl.value, npts.value)
        assert rc == 0 and off[0] == 0 and np.all(off[1:] == -7) and np.all(pts == -7) and np.all(norm == -7)
    nl.value = -5
    assert L.fs_streamlines(sim._h, -1, 2.0, 100, 0.2, 0.1, ctypes.byref(nl), None) != 0 and nl.value == -5
    # a handle that was never asked has nothing to fetch and says so
    fresh = F.Simulation(6, 5, 4, 1, quiet=1, dump_every=0)
    assert fresh._L.fs_streamlines_fetch(fresh._h, None, None, None) != 0
    fresh.close()
    _handles[(C.BY_NAME[big]["shape"], "fp32")][1] = None


def test_the_bounding_box_follows_the_body(F):
    name = "ball-20"
    shape, par = C.BY_NAME[name]["shape"], C.BY_NAME[name]["par"]
    sim = loaded(F, name)
    vx, vy, vz, _ = C.fields(name)
    before, _ = sim.streamlines(**call_args(par))
    moved = np.ascontiguousarray(np.transpose(ball_mask(*shape, 27, 9, 8, 3.3), (2, 1, 0))).astype(np.float32)
    sim.set_mask(ball_mask(*shape, 27, 9, 8, 3.3))
    _handles[(shape, "fp32")][1] = None
    with np.errstate(all="ignore"):
        want, wnorm = C.R.generate_streamlines(vx, vy, vz, moved, norm=C.R.kernel_norm, **par)
    got, gnorm = sim.streamlines(**call_args(par))
    assert len(want) > 0 and len(before) > 0
    assert_same("moved ball", got, gnorm, want, wnorm)
    assert {tuple(l[0]) for l in got} != {tuple(l[0]) for l in before}
    # no solid left: no box, no lines, and a fetch of nothing succeeds
    sim.set_mask(np.zeros((shape[2] + 2, shape[1] + 2, shape[0] + 2), dtype=bool))
    lines, norm = sim.streamlines(**call_args(par))
    assert lines == [] and norm.shape == (0,)
    rc, off, _, _ = raw_fetch(sim, 0, 0)
    assert rc == 0 and off.tolist() == [0]


def test_slab_handles_refuse(F):
    sim = F.Simulation(8, 8, 8, 1, quiet=1)
    sim.comm_init(0, 2, b"FSNULL:".ljust(128, b"\0"))
    with pytest.raises(F.FluidsimError):
        sim.streamlines()
    assert sim._L.fs_streamlines_fetch(sim._h, None, None, None) == 0      # the refused call left the empty result


@pytest.mark.parametrize("name", ["ragged-fp64", "long-row", "nan-cell"])
def test_no_field_changes(F, name):
    sim = loaded(F, name)
    rng = np.random.default_rng(11)
    for which in (F.DENS, F.PRESSURE, F.DIVERGENCE, F.VX_PREV, F.VY_PREV, F.VZ_PREV, F.BUFFER):
        sim.set(which, rng.standard_normal(sim.shape).astype(sim.dtype))
    before = [sim.get(which) for which in range(11)]
    got, _ = sim.streamlines(**call_args(C.BY_NAME[name]["par"]))
    assert len(got) > 0
    after = [sim.get(which) for which in range(11)]
    for which, (a, b) in enumerate(zip(before, after)):
        assert a.dtype == sim.dtype and bits_equal(a, b), F.FIELD_NAMES[which]
    for which, a in zip((F.VX, F.VY, F.VZ, F.OBS), C.fields(name)):
        assert bits_equal(after[which], C.as_stored(a))
