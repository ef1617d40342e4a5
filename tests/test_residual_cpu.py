"""CPU checks of the solve-residual surface: the Python helper that turns logged sums into reduction factors (against
values worked out by hand), the columns of the structured log, and the C ABI / ctypes entries they rest on."""
import os
import re

import numpy as np

from conftest import ROOT


def raw_row(step, solves):
    """One raw fs_residual_log row from six (r0_sq, r_sq, r_max, rhs_sq, cells) tuples."""
    row = [float(step)]
    for s in solves:
        row += list(s)
    return row


def test_solve_reduction_hand_values():
    from fluid_simulation_amd import solve_reduction
    nan = float("nan")
    rows = np.array([
        # sqrt(4/16) = 1/2, sqrt(1/64) = 1/8, sqrt(9/9) = 1 (a solve of zero sweeps), sqrt(0/4) = 0, 0/0: nothing to reduce,
        # a solve the step did not run
        raw_row(1, [(16.0, 4.0, 1.5, 7.0, 10), (64.0, 1.0, 0.5, 3.0, 10), (9.0, 9.0, 2.0, 9.0, 10), (4.0, 0.0, 0.0, 4.0, 10),
                    (0.0, 0.0, 0.0, 0.0, 10), (nan, nan, nan, nan, 0)]),
        raw_row(2, [(1.0, 0.25, 0.5, 1.0, 3)] * 6),
    ])
    assert rows.shape == (2, 31)
    red = solve_reduction(rows)
    assert red.shape == (2, 6) and red.dtype == np.float64
    assert np.array_equal(red[0, :4], [0.5, 0.125, 1.0, 0.0])
    assert np.isnan(red[0, 4]) and np.isnan(red[0, 5])
    assert np.array_equal(red[1], [0.5] * 6)
    assert np.array_equal(solve_reduction(rows[1]), [0.5] * 6)       # a single row


def test_solve_reduction_of_a_structured_log():
    from fluid_simulation_amd import RESIDUAL_LOG_DTYPE, solve_reduction
    rows = np.zeros(2, dtype=RESIDUAL_LOG_DTYPE)
    for k in range(6):
        rows["r0_sq_%d" % k] = [4.0 ** (k + 1), 1.0]
        rows["r_sq_%d" % k] = [1.0, 0.0625]
    rows["r0_sq_5"][1] = rows["r_sq_5"][1] = np.nan
    red = solve_reduction(rows)
    assert np.array_equal(red[0], [0.5 ** (k + 1) for k in range(6)])
    assert np.array_equal(red[1, :5], [0.25] * 5) and np.isnan(red[1, 5])


def test_residual_log_dtype_columns():
    from fluid_simulation_amd import RESIDUAL_LOG_DTYPE, _lib
    want = ["step"]
    for k in range(6):
        want += ["r0_sq_%d" % k, "r_sq_%d" % k, "r_max_%d" % k, "rhs_sq_%d" % k, "cells_%d" % k]
    want += ["reduction_%d" % k for k in range(6)]
    assert list(RESIDUAL_LOG_DTYPE.names) == want
    assert _lib.RESIDUAL_LOG_COLS == 31 == 1 + 5 * _lib.RESIDUAL_LOG_SOLVES and _lib.RESIDUAL_COLS == 4
    assert RESIDUAL_LOG_DTYPE["step"] == np.int64 and RESIDUAL_LOG_DTYPE["cells_3"] == np.int64
    assert RESIDUAL_LOG_DTYPE["r0_sq_0"] == np.float64 and RESIDUAL_LOG_DTYPE["reduction_5"] == np.float64


def test_header_documents_the_residual_entry_points():
    text = open(os.path.join(ROOT, "include", "fluidsim.h")).read()
    assert re.search(r"int fs_solve_residual\(fs_sim\* s, int b, int field, int prev, double a, double c, double out\[4\], "
                     r"double\* per_plane\);", text)
    assert re.search(r"int fs_diffuse_residual\(fs_sim\* s, int b, int field, int prev, double out\[4\], double\* per_plane\);", text)
    assert re.search(r"int fs_residual_log\(fs_sim\* s, double\* rows, long max_rows, long\* n_rows, long\* n_dropped\);", text)
    for line in ("#define FS_RESIDUAL_COLS 4", "#define FS_RESIDUAL_LOG_SOLVES 6", "#define FS_RESIDUAL_LOG_COLS 31"):
        assert line in text
    assert '"residual_log"' in text and '"residual"' in text
    # the definition: the order of the neighbours and the widening
    assert "(((((x[i+1] + x[i-1]) + x[j+1]) + x[j-1]) + x[l+1]) + x[l-1])" in text and "fp64" in text
    from fluid_simulation_amd import _lib
    for name in ("fs_solve_residual", "fs_diffuse_residual", "fs_residual_log"):
        assert name in _lib.exported_symbols()


def test_simulation_has_the_residual_methods():
    from fluid_simulation_amd import Simulation
    for name in ("solve_residual", "diffuse_residual", "pressure_residual", "residual_log"):
        assert callable(getattr(Simulation, name))


def test_kernel_takes_its_addresses_from_the_plan_header():
    """The kernel's translation unit uses residual_plan.h's items and loads, and holds no atomics."""
    src = open(os.path.join(ROOT, "fluid_simulation_amd", "csrc", "residual.hip")).read()
    for word in ("residual_plan(", "residual_item(", "residual_iters(", "residual_load("):
        assert word in src
    assert "atomic" not in src
    plan = open(os.path.join(ROOT, "fluid_simulation_amd", "csrc", "residual_plan.h")).read()
    assert "#include" not in plan and "__device__" not in plan and "__global__" not in plan
