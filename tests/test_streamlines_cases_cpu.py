"""CPU checks of the case table tests/streamlines_cases.py, run with oracle/streamlines_ref.py alone: what
tests/test_gpu_streamlines.py compares the device with must itself be worth comparing with.

* every case yields lines, except the ones that cannot (YIELD_NONE, each with its reason);
* every case reaches what its entry claims -- parts ended by the wall test, by the wall test after points in the clip zone of
  the interpolation, by the speed test, by the solid test, by non-finite coordinates; seeds inside solids; joined lines too
  short to keep, of exactly 5 (dropped) and 6 (kept) points; lines dropped and kept by the threshold;
* NO SEED of any case takes a decision closer than 1e-9 to its threshold (the trace hook of the restatement; the units are
  those of the quantity compared: cells, cells per step, mask value), so a last-bit difference could not flip one;
* numpy's own norm and the kernel's sqrt((u*u + v*v) + w*w) give the same lines and point counts everywhere.  Measured here
  (numpy 2.2.6): 15 of the 36 cases differ in some coordinate; the largest difference is 4.4e-15 (inf-cell and nan-cell;
  ball-30: 3.6e-15), and the colour arguments differ by at most 1.1e-16.  Asserted under 1e-9, the gate of
  test_gpu_edge.py.

The module takes about 20 s: each case is integrated twice, once per norm."""
import math

import numpy as np
import pytest

import streamlines_cases as C
from oracle import streamlines_ref as R

cases = pytest.mark.parametrize("name", C.NAMES)
MARGIN = 1e-9


def test_the_table_has_the_rows_it_should():
    assert len(set(C.NAMES)) == len(C.NAMES)
    shapes = {(c["shape"], c["precision"]) for c in C.CASES}
    for row in (((40, 20, 18), "fp32"), ((17, 11, 9), "fp64"), ((300, 7, 6), "fp32"), ((24, 12, 10), "fp32"),
                ((24, 12, 10), "fp64"), ((16, 10, 8), "fp32"), ((1, 1, 1), "fp32"), ((2, 1, 1), "fp64")):
        assert row in shapes, row
    par = lambda key: {c["par"][key] for c in C.CASES}
    assert {0, 1, 2, 3, 7, 20, 30} <= par("density") and {0, 1, 2, 3, 11, 100} <= par("max_length")
    assert {-0.2, 0.0, 1e3, 0.2} <= par("step_size") and {-50, 0, 1e4, 2} <= par("proximity")
    assert set(C.YIELD_NONE) <= set(C.NAMES)
    # between them the cases end parts in every way there is and give seeds every fate there is
    union = set().union(*(C.reached(C.expected(n)[2]) for n in C.NAMES))
    assert union >= {"wall", "clip", "speed", "solid", "nonfinite", "steps", "culled", "seed_in_solid", "short", "len5", "len6",
                     "thr_dropped", "kept"}, union


@cases
def test_case_reaches_what_its_row_claims(name):
    case = C.BY_NAME[name]
    lines, norms, records = C.expected(name)
    assert len(lines) == len(norms)
    if name in C.YIELD_NONE:
        assert lines == []
    else:
        assert len(lines) > 0
    tags = C.reached(records)
    assert set(case["reaches"]) <= tags, (set(case["reaches"]) - tags, tags)
    # the cap is zero: every seed's smallest margin counts
    nx, nyz = case["par"]["density"], case["par"]["density"] // 2
    assert len(records) == nx * nyz * nyz
    worst = min(records, key=lambda r: r[1], default=None)
    assert worst is None or worst[1] >= MARGIN, worst
    for line in lines:
        assert line.dtype == np.float64 and line.shape[0] > 5 and np.all(np.isfinite(line))


@cases
def test_numpy_norm_changes_no_count(name):
    lines, norms, _ = C.expected(name)
    lines_np, norms_np, _ = C.expected(name, kernel_order=False)
    assert [l.shape for l in lines] == [l.shape for l in lines_np]
    worst = max([float(np.abs(a - b).max()) for a, b in zip(lines, lines_np)], default=0.0)
    colour = max([abs(float(a) - float(b)) for a, b in zip(norms, norms_np) if not (math.isnan(a) and math.isnan(b))], default=0.0)
    print("%s: %d lines, %d points, numpy norm moves a coordinate by at most %.3g, a colour by %.3g"
          % (name, len(lines), sum(len(l) for l in lines), worst, colour))
    assert worst < 1e-9 and colour < 1e-9


def test_hooks_change_nothing():
    """norm=None, trace=None is the restatement as it was; a trace only listens"""
    vx, vy, vz, obs = C.fields("ragged-fp64")
    par = C.BY_NAME["ragged-fp64"]["par"]
    plain = R.generate_streamlines(vx, vy, vz, obs, **par)
    seen = []
    traced = R.generate_streamlines(vx, vy, vz, obs, trace=lambda *a: seen.append(a), **par)
    assert len(plain[0]) == len(traced[0]) > 0 and all(np.array_equal(a, b) for a, b in zip(plain[0], traced[0]))
    assert plain[1] == traced[1] and len(seen) == 16 * 8 * 8
    unhooked = C.expected("ragged-fp64", kernel_order=False)
    assert all(np.array_equal(a, b) for a, b in zip(plain[0], unhooked[0])) and plain[1] == unhooked[1]
    # the kernel's norm is numpy's up to the last bit, and exact where the answer is
    rng = np.random.default_rng(5)
    v = rng.standard_normal((200, 3))
    assert max(abs(R.kernel_norm(a) - np.linalg.norm(a)) / np.linalg.norm(a) for a in v) < 4e-16
    assert R.kernel_norm(np.array([3.0, 4.0, 12.0])) == 13.0 and R.kernel_norm(np.zeros(3)) == 0.0


def test_non_finite_cells_decide_the_colour():
    """np.max is NaN as soon as one cell is, and Python's min(NaN, 1.0) keeps it; an infinite cell makes every colour 0"""
    for name, check in (("nan-cell", math.isnan), ("inf-cell", lambda v: v == 0.0)):
        lines, norms, records = C.expected(name)
        assert len(lines) > 0 and all(check(float(v)) for v in norms)
        ends = [i["ends"] for _, _, i in records if "ends" in i]
        assert any("nonfinite" in e for e in ends) and any("nonfinite" not in e for e in ends)


def test_soft_mask_is_not_its_binarisation():
    """the viewer's code interpolates the obstacle array it was given: with the array turned into a 0/1 mask the lines
    stop elsewhere (what fluid_simulation_amd.viewer.generate_streamlines once did), and a cell of exactly 0.5 is no solid"""
    vx, vy, vz, obs = C.fields("soft-mask")
    par = C.BY_NAME["soft-mask"]["par"]
    want = C.expected("soft-mask")[0]
    with np.errstate(all="ignore"):
        binary = R.generate_streamlines(vx, vy, vz, (obs > 0.5).astype(np.float32), norm=R.kernel_norm, **par)[0]
        widened = R.generate_streamlines(vx, vy, vz, np.where(obs == 0.5, np.float32(0.6), obs), norm=R.kernel_norm, **par)[0]
    assert [l.shape for l in binary] != [l.shape for l in want]
    assert len(widened) != len(want)
    assert set(np.unique(obs).tolist()) == {0.0, float(np.float32(0.4)), 0.5, float(np.float32(0.6)), 1.0}


def test_ghost_cells_decide_the_maximum():
    vx, vy, vz, _ = C.fields("ghosts")
    stack = np.array([vx, vy, vz])
    assert np.unravel_index(np.argmax(stack), stack.shape) == (1, 0, 0, 0)
    assert stack[:, 1:-1, 1:-1, 1:-1].max() < 2.0 < stack[:, 0].min()
    _, norms, _ = C.expected("ghosts")
    assert 0.05 < min(norms) < max(norms) < 1.0          # speeds from 1 over a maximum of 11.5: nothing is cut at 1


def test_exact_landings_on_the_walls():
    """the case outside the table: coordinates are exact multiples of 0.25, x = 1 is kept and x = W + 1 is not"""
    lines, norms, records = C.expected(C.EXACT["name"])
    assert len(lines) == 8 * 4 * 4 - 1 and C.smallest_margin(records) == 0.0
    for line in lines:
        assert np.array_equal(line[:, 0], 1.0 + 0.25 * np.arange(32))          # 1.0 .. 8.75
        assert np.all(line[:, 1:] == line[0, 1:])
    assert set(norms) == {1.0 / float(np.float32(1.0) + np.float32(1e-6))}
