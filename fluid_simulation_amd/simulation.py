"""Host-side mirror of the reference's solver interface, on top of the C ABI.

`Simulation` has the constructor, public data members and methods of the reference's
`class Simulation` (simulation.h:42-91) under the same names, and `loadSTLIntoObstacles`
has the signature of the reference's free function (object_loader.h:7-17), so code and
tests written against the reference read the same here.  Everything numeric happens in
libfluidsim.so on the MI355X.
"""
import ctypes as C
import os

import numpy as np

from . import _lib
from ._lib import FluidsimError, check  # noqa: F401

# Columns of Simulation.force_log(): fs_force_log's raw columns, then F and C of the step (S = S1 + S2)
FORCE_LOG_DTYPE = np.dtype([("step", np.int64), ("s1x", np.float64), ("s1y", np.float64), ("s1z", np.float64),
                            ("s2x", np.float64), ("s2y", np.float64), ("s2z", np.float64), ("faces", np.int64),
                            ("frontal", np.int64), ("fx", np.float64), ("fy", np.float64), ("fz", np.float64),
                            ("cx", np.float64), ("cy", np.float64), ("cz", np.float64)])

# Rows of Simulation.label_bodies(): fs_body_info's columns for record `body` (0 = the REST), then the centroid sum / cells
BODY_INFO_DTYPE = np.dtype([("body", np.int64)] +
                           [(n, np.int64) for n in ("cells", "anchor", "xmin", "xmax", "ymin", "ymax", "zmin", "zmax",
                                                    "sum_x", "sum_y", "sum_z", "frontal")] +
                           [("cx", np.float64), ("cy", np.float64), ("cz", np.float64)])

# Columns of Simulation.body_force_log(): fs_body_force_log's raw columns, then force F, torque T and the coefficients C
# (force) and CM (moment, for the l_ref of the call) of the step (S = S1 + S2, M = M1 + M2)
BODY_LOG_DTYPE = np.dtype([("step", np.int64), ("body", np.int64)] +
                          [(n + a, np.float64) for n in ("s1", "m1", "s2", "m2") for a in "xyz"] +
                          [("faces", np.int64), ("frontal", np.int64)] +
                          [(n + a, np.float64) for n in ("f", "t", "c", "cm") for a in "xyz"])

# Columns of Simulation.residual_log(): fs_residual_log's raw columns (step, then r0_sq_k, r_sq_k, r_max_k, rhs_sq_k,
# cells_k for the step's six solves k = 0..5: diffuse v_x, v_y, v_z, projection 1, projection 2, diffuse density), then
# reduction_k = sqrt(r_sq_k / r0_sq_k)
RESIDUAL_LOG_DTYPE = np.dtype(
    [("step", np.int64)] +
    [(name % k, np.int64 if name.startswith("cells") else np.float64) for k in range(_lib.RESIDUAL_LOG_SOLVES)
     for name in ("r0_sq_%d", "r_sq_%d", "r_max_%d", "rhs_sq_%d", "cells_%d")] +
    [("reduction_%d" % k, np.float64) for k in range(_lib.RESIDUAL_LOG_SOLVES)])


def solve_reduction(rows):
    """Reduction factor of each solve of each step, sqrt(r_sq / r0_sq): `rows` is a RESIDUAL_LOG_DTYPE array or raw
    fs_residual_log rows (..., 31); returns (..., 6) in fp64.  NaN for a solve that did not run (its columns are NaN)
    and where r0_sq is 0 (nothing to reduce)."""
    if getattr(rows, "dtype", None) is not None and rows.dtype.names:
        r0 = np.stack([rows["r0_sq_%d" % k] for k in range(_lib.RESIDUAL_LOG_SOLVES)], axis=-1).astype(np.float64)
        r1 = np.stack([rows["r_sq_%d" % k] for k in range(_lib.RESIDUAL_LOG_SOLVES)], axis=-1).astype(np.float64)
    else:
        raw = np.asarray(rows, dtype=np.float64)
        r0, r1 = raw[..., 1::5], raw[..., 2::5]
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(r0 != 0.0, np.sqrt(r1 / np.where(r0 != 0.0, r0, 1.0)), np.nan)


def _residual_dict(out, pp):
    with np.errstate(divide="ignore", invalid="ignore"):
        rel = float(np.sqrt(np.float64(out[0]) / np.float64(out[1])))
    r = {"r_sq": float(out[0]), "rhs_sq": float(out[1]), "r_max": float(out[2]), "cells": int(out[3]), "relative": rel}
    if pp is not None:
        r["per_plane"] = pp
    return r


# The 16 numbers of a flow-monitor record (include/fluidsim.h, "flow monitor"), the 5 of an x-profile row, and the 57
# columns of Simulation.monitor_log(): step, the whole record, then the profile row of each of the 8 stations.
MONITOR_NAMES = ("cells", "nonfinite", "sum_q", "sum_u", "sum_v", "sum_w", "sum_e", "sum_p", "max_abs_u", "max_abs_v",
                 "max_abs_w", "max_e", "min_q", "max_q", "min_p", "max_p")
MONITOR_PROFILE_NAMES = ("cells", "sum_u", "sum_uu", "sum_p", "sum_qu")
MONITOR_LOG_NAMES = (("step",) + MONITOR_NAMES +
                     tuple("s%d_%s" % (k, n) for k in range(_lib.MONITOR_STATIONS_MAX) for n in MONITOR_PROFILE_NAMES))


def monitor_cfl(dt, width, height, depth, max_abs_u, max_abs_v, max_abs_w):
    """The Courant numbers of a flow-monitor record: ((double)dt * N) * max |.| per axis, the length of the advection
    back-trace in cells; `dt` as the handle stores it (fp32)."""
    dt = float(np.float32(dt))
    return ((dt * int(width)) * float(max_abs_u), (dt * int(height)) * float(max_abs_v), (dt * int(depth)) * float(max_abs_w))


def pressure_force(s, frontal, dt, speed, width, height, depth):
    """Force and force coefficients of raw pressure sums (include/fluidsim.h, "pressure force on the obstacles"):
    F = S * h^2 / dt with h = 1 / cbrt(width * height * depth), and C = 2 * S / (dt * speed^2 * N_front), N_front =
    `frontal` (NaN where dt * speed^2 * N_front is 0).  `s` has shape (..., 3), `frontal` the leading shape; returns
    (F, C), both (..., 3), in fp64.  For a row of the force log, S = S1 + S2 (a step applies both projections)."""
    s = np.asarray(s, dtype=np.float64)
    n = np.asarray(frontal, dtype=np.float64)[..., None]
    h = 1.0 / np.cbrt(float(int(width) * int(height) * int(depth)))
    dt = float(dt)
    force = s * (h * h) / dt
    denom = dt * (float(speed) * float(speed)) * n
    with np.errstate(divide="ignore", invalid="ignore"):
        coeff = np.where(denom != 0.0, 2.0 * s / np.where(denom != 0.0, denom, 1.0), np.nan)
    return force, coeff


def pressure_moment(m, frontal, l_ref, dt, speed, width, height, depth):
    """Torque and moment coefficients of raw pressure moments (include/fluidsim.h, "per-body pressure forces and
    moments"): T = M * h^3 / dt with h = 1 / cbrt(width * height * depth), and C_M = 2 * M / (dt * speed^2 * N_front *
    L_ref), N_front = `frontal`, L_ref = `l_ref` in cells (NaN where the denominator is 0).  `m` has shape (..., 3),
    `frontal` the leading shape; returns (T, C_M), both (..., 3), in fp64."""
    m = np.asarray(m, dtype=np.float64)
    n = np.asarray(frontal, dtype=np.float64)[..., None]
    h = 1.0 / np.cbrt(float(int(width) * int(height) * int(depth)))
    dt = float(dt)
    torque = m * (h * h * h) / dt
    denom = dt * (float(speed) * float(speed)) * n * float(l_ref)
    with np.errstate(divide="ignore", invalid="ignore"):
        coeff = np.where(denom != 0.0, 2.0 * m / np.where(denom != 0.0, denom, 1.0), np.nan)
    return torque, coeff


def shift_moment(m, s, origin_from, origin_to):
    """The moment about `origin_to` of a record whose moment about `origin_from` is `m` and whose sum is `s`:
    M - (to - from) x S, in fp64.  `m` and `s` have shape (..., 3)."""
    m = np.asarray(m, dtype=np.float64)
    s = np.asarray(s, dtype=np.float64)
    d = np.asarray(origin_to, dtype=np.float64) - np.asarray(origin_from, dtype=np.float64)
    return m - np.cross(np.broadcast_to(d, s.shape), s)


class Simulation:
    """Simulation(w, h, d, iter, speed=30, dt=0.05, diff=2.0e-5, visc=1.5e-5, acc=15)
    -- simulation.h:59-64.  Extra keyword options map to fs_set_option."""

    def __init__(self, w, h, d, iter, speed=30, dt=0.05, diff=2.0e-5, visc=1.5e-5, acc=15,
                 precision="fp32", solver="jacobi", **options):
        L = _lib.lib()
        self._L = L
        self._h = L.fs_create(int(w), int(h), int(d), int(iter), int(speed), float(dt), float(diff), float(visc),
                              int(acc))
        if not self._h:
            raise FluidsimError(_lib.EHIP, (L.fs_last_error() or b"").decode(errors="replace"))
        self._h = C.c_void_p(self._h)
        self.precision = precision
        self._volume_size = {}                               # camera slot -> (rows, cols) of its ray set
        self.dtype = np.float64 if precision == "fp64" else np.float32
        self.set_option("precision", precision)
        self.set_option("solver", solver)
        for k, v in options.items():
            self.set_option(k, v)

    # -- lifetime -------------------------------------------------------------------
    def close(self):
        if getattr(self, "_h", None):
            self._L.fs_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def set_option(self, key, value):
        if isinstance(value, bool):
            value = "1" if value else "0"
        elif key == "moment_origin" and not isinstance(value, str):
            value = ",".join(repr(float(v)) for v in value)
        elif key == "monitor_stations" and not isinstance(value, str):
            value = ",".join(str(int(v)) for v in value)
        check(self._L.fs_set_option(self._h, key.encode(), str(value).encode()))

    # -- public data members of the reference class (simulation.h:44-54) ---------------
    def _geti(self, name):
        v = C.c_int()
        check(self._L.fs_get_int(self._h, name.encode(), C.byref(v)))
        return v.value

    def _getf(self, name):
        v = C.c_float()
        check(self._L.fs_get_float(self._h, name.encode(), C.byref(v)))
        return v.value

    width = property(lambda s: s._geti("width"))
    height = property(lambda s: s._geti("height"))
    depth = property(lambda s: s._geti("depth"))
    speed = property(lambda s: s._geti("speed"), lambda s, v: check(s._L.fs_set_int(s._h, b"speed", int(v))))
    acc = property(lambda s: s._geti("acc"), lambda s, v: check(s._L.fs_set_int(s._h, b"acc", int(v))))
    iter = property(lambda s: s._geti("iter"), lambda s, v: check(s._L.fs_set_int(s._h, b"iter", int(v))))
    dt = property(lambda s: s._getf("dt"), lambda s, v: check(s._L.fs_set_float(s._h, b"dt", float(v))))
    diff = property(lambda s: s._getf("diff"), lambda s, v: check(s._L.fs_set_float(s._h, b"diff", float(v))))
    visc = property(lambda s: s._getf("visc"), lambda s, v: check(s._L.fs_set_float(s._h, b"visc", float(v))))
    z_alternate = property(lambda s: s._geti("z_alternate"), lambda s, v: check(s._L.fs_set_int(s._h, b"z_alternate", int(v))))
    local_depth = property(lambda s: s._geti("local_depth"))
    z_offset = property(lambda s: s._geti("z_offset"))

    # -- methods of the reference class ------------------------------------------------
    def run(self):
        """Simulation::run(), simulation.cpp:49-91."""
        check(self._L.fs_run(self._h))

    def step(self):
        """Simulation::step(), simulation.cpp:96-150."""
        check(self._L.fs_step(self._h))

    def addObstacle(self, x, y, z):
        check(self._L.fs_add_obstacle(self._h, x, y, z))

    def addDensity(self, x, y, z, amount):
        check(self._L.fs_add_density(self._h, x, y, z, amount))

    def setVelocity(self, x, y, z, amount_x, amount_y, amount_z):
        check(self._L.fs_set_velocity(self._h, x, y, z, amount_x, amount_y, amount_z))

    # -- the rest of the C ABI ---------------------------------------------------------
    def run_one(self):
        """One iteration of run()'s time loop: inlet density, buffer = dens, step()."""
        check(self._L.fs_run_one(self._h))

    def sync(self):
        check(self._L.fs_sync(self._h))

    @property
    def shape(self):
        """C-order shape of a field as the viewers reshape it (gui.py:228-231): (D+2, H+2, W+2);
        under z-slabs D is this rank's local depth."""
        return (self.local_depth + 2, self.height + 2, self.width + 2)

    def get(self, which, dtype=None):
        dtype = np.dtype(dtype or self.dtype)
        n = self._L.fs_padded_size(self._h)
        out = np.empty(n, dtype=dtype)
        check(self._L.fs_get_field(self._h, which, out.ctypes.data_as(C.c_void_p), n, dtype.itemsize))
        return out.reshape(self.shape)

    def set(self, which, arr):
        a = np.ascontiguousarray(arr)
        if a.dtype not in (np.float32, np.float64, np.uint8):
            a = a.astype(self.dtype)
        a = a.reshape(-1)
        check(self._L.fs_set_field(self._h, which, a.ctypes.data_as(C.c_void_p), a.size, a.dtype.itemsize))

    def set_mask(self, mask):
        m = np.ascontiguousarray(np.asarray(mask) != 0, dtype=np.uint8).reshape(-1)
        check(self._L.fs_set_obstacle_mask(self._h, m.ctypes.data_as(C.c_void_p), m.size))

    def set_bounds(self, b, field):
        check(self._L.fs_set_bounds(self._h, b, field))

    def linear_solver(self, b, field, prev, a, c):
        check(self._L.fs_linear_solver(self._h, b, field, prev, a, c))

    def diffuse(self, b, field, prev):
        check(self._L.fs_diffuse(self._h, b, field, prev))

    def project(self):
        check(self._L.fs_project(self._h))

    def advect(self, b, field, prev):
        check(self._L.fs_advect(self._h, b, field, prev))

    def dump_frame(self):
        check(self._L.fs_dump_frame(self._h))

    def stats(self, which):
        s, lo, hi = C.c_double(), C.c_double(), C.c_double()
        check(self._L.fs_field_stats(self._h, which, C.byref(s), C.byref(lo), C.byref(hi)))
        return s.value, lo.value, hi.value

    def timing(self, family):
        ms, n = C.c_double(), C.c_long()
        check(self._L.fs_get_timing(self._h, family.encode(), C.byref(ms), C.byref(n)))
        return ms.value, n.value

    def reset_timing(self):
        check(self._L.fs_reset_timing(self._h))

    def streamlines(self, density=30, proximity=2, max_length=100, step_size=0.2, vel_change_threshold=0.1):
        """generate_streamlines of the reference's viewer (GUI/utils.py:118-213, defaults from
        GUI/config.py:18-23) from the fields on the device.  Returns (lines, norm_speeds): a list
        of (n_i, 3) float64 arrays in the viewer's (x, y, z) padded index space, in the reference's
        order, and for each line the value the viewer passes to `config.density_cmap`."""
        nl, npts = C.c_long(), C.c_long()
        check(self._L.fs_streamlines(self._h, int(density), float(proximity), int(max_length), float(step_size),
                                     float(vel_change_threshold), C.byref(nl), C.byref(npts)))
        off = np.zeros(nl.value + 1, dtype=np.int64)
        pts = np.zeros((npts.value, 3), dtype=np.float64)
        norm = np.zeros(nl.value, dtype=np.float64)
        check(self._L.fs_streamlines_fetch(self._h, off.ctypes.data, pts.ctypes.data, norm.ctypes.data))
        return [pts[off[i]:off[i + 1]].copy() for i in range(nl.value)], norm

    def obstacle_surface(self):
        """generate_obstacle_mesh of the reference's viewer (GUI/utils.py:10-38) from `obs` on the device:
        (vertices (n, 3) float32 in the viewer's padded (x, y, z) index space, faces (m, 3) int32)."""
        nv, nt = C.c_long(), C.c_long()
        check(self._L.fs_obstacle_surface(self._h, C.byref(nv), C.byref(nt)))
        verts = np.zeros((nv.value, 3), dtype=np.float32)
        faces = np.zeros((nt.value, 3), dtype=np.int32)
        check(self._L.fs_obstacle_surface_fetch(self._h, verts.ctypes.data, faces.ctypes.data))
        return verts, faces

    def obstacle_force(self, per_plane=False):
        """Pressure force on the obstacles from FS_PRESSURE as it is now (fs_obstacle_force; collective on z-slabs):
        a dict with the raw sums "S" (3,), the counts "faces" and "frontal" (N_front), "force" and "coeff" (see
        pressure_force), and with per_plane=True "per_plane", (depth, 5) records {Sx, Sy, Sz, faces, frontal} of the
        global planes 1..depth."""
        out = np.zeros(5, dtype=np.float64)
        pp = np.zeros((self.depth, 5), dtype=np.float64) if per_plane else None
        check(self._L.fs_obstacle_force(self._h, out.ctypes.data, None if pp is None else pp.ctypes.data))
        force, coeff = pressure_force(out[:3], out[4], self.dt, self.speed, self.width, self.height, self.depth)
        r = {"S": out[:3].copy(), "faces": int(out[3]), "frontal": int(out[4]), "force": force, "coeff": coeff}
        if per_plane:
            r["per_plane"] = pp
        return r

    def force_log(self, with_dropped=False):
        """Drains the per-step force log (option force_log=N; fs_force_log, collective on z-slabs): one row per
        retained step, oldest first, as a FORCE_LOG_DTYPE structured array.  with_dropped=True returns
        (rows, number of logged steps the ring overwrote since the last drain)."""
        n, dropped = C.c_long(), C.c_long()
        check(self._L.fs_force_log(self._h, None, 0, C.byref(n), C.byref(dropped)))
        raw = np.zeros((n.value, _lib.FORCE_LOG_COLS), dtype=np.float64)
        check(self._L.fs_force_log(self._h, raw.ctypes.data, n.value, C.byref(n), C.byref(dropped)))
        rows = np.zeros(n.value, dtype=FORCE_LOG_DTYPE)
        for k, name in enumerate(FORCE_LOG_DTYPE.names[:_lib.FORCE_LOG_COLS]):
            rows[name] = raw[:, k]
        force, coeff = pressure_force(raw[:, 1:4] + raw[:, 4:7], raw[:, 8], self.dt, self.speed, self.width,
                                      self.height, self.depth)
        for k, a in enumerate("xyz"):
            rows["f" + a] = force[:, k]
            rows["c" + a] = coeff[:, k]
        return (rows, dropped.value) if with_dropped else rows

    # -- per-body forces and moments (single GPU) --------------------------------------------
    def _body_info(self):
        n = C.c_long()
        check(self._L.fs_body_info(self._h, None, 0, C.byref(n)))
        raw = np.zeros((n.value, _lib.BODY_INFO_COLS), dtype=np.float64)
        check(self._L.fs_body_info(self._h, raw.ctypes.data, n.value, C.byref(n)))
        rows = np.zeros(n.value, dtype=BODY_INFO_DTYPE)
        rows["body"] = np.arange(n.value)
        for k, name in enumerate(BODY_INFO_DTYPE.names[1:1 + _lib.BODY_INFO_COLS]):
            rows[name] = raw[:, k]
        with np.errstate(divide="ignore", invalid="ignore"):
            for a in "xyz":
                rows["c" + a] = raw[:, 8 + "xyz".index(a)] / raw[:, 0]
        return rows

    def label_bodies(self):
        """Labels the solid cells into bodies now (fs_label_bodies) and returns the body table (fs_body_info) as a
        BODY_INFO_DTYPE structured array: row 0 is the REST, rows 1..B the bodies by decreasing size; cx, cy, cz is
        the centroid sum / cells (NaN for an empty REST)."""
        check(self._L.fs_label_bodies(self._h, None, None))
        return self._body_info()

    def body_info(self):
        """The body table of the current mask (labelled anew only if obs changed); see label_bodies."""
        return self._body_info()

    body_count = property(lambda s: s._geti("body_count"))
    body_components = property(lambda s: s._geti("body_components"))

    def body_labels(self):
        """The label array (fs_body_labels), int32 of `shape`: k on the cells of body k, -1 on REST cells, 0 elsewhere."""
        n = self._L.fs_padded_size(self._h)
        out = np.zeros(n, dtype=np.int32)
        check(self._L.fs_body_labels(self._h, out.ctypes.data, n))
        return out.reshape(self.shape)

    def body_force(self, per_plane=False):
        """Per-body pressure force and moment from FS_PRESSURE as it is now (fs_body_force): (B + 1, 8) records
        {Sx, Sy, Sz, Mx, My, Mz, faces, frontal rows}, row 0 the REST; with per_plane=True also the plane records,
        (depth, B + 1, 8), as a pair."""
        n = C.c_long()
        check(self._L.fs_body_force(self._h, None, 0, C.byref(n), None))
        out = np.zeros((n.value, _lib.BODY_COLS), dtype=np.float64)
        pp = np.zeros((self.depth, n.value, _lib.BODY_COLS), dtype=np.float64) if per_plane else None
        check(self._L.fs_body_force(self._h, out.ctypes.data, n.value, C.byref(n), None if pp is None else pp.ctypes.data))
        return (out, pp) if per_plane else out

    def body_force_log(self, with_dropped=False, l_ref=1.0):
        """Drains the per-step body-force log (option body_force_log=N; fs_body_force_log): B + 1 rows per retained
        step, oldest first, as a BODY_LOG_DTYPE structured array.  with_dropped=True returns (rows, number of logged
        steps the ring overwrote since the last drain)."""
        n, dropped = C.c_long(), C.c_long()
        check(self._L.fs_body_force_log(self._h, None, 0, C.byref(n), C.byref(dropped)))
        raw = np.zeros((n.value, _lib.BODY_LOG_COLS), dtype=np.float64)
        check(self._L.fs_body_force_log(self._h, raw.ctypes.data, n.value, C.byref(n), C.byref(dropped)))
        rows = np.zeros(n.value, dtype=BODY_LOG_DTYPE)
        for k, name in enumerate(BODY_LOG_DTYPE.names[:_lib.BODY_LOG_COLS]):
            rows[name] = raw[:, k]
        dims = (self.dt, self.speed, self.width, self.height, self.depth)
        force, coeff = pressure_force(raw[:, 2:5] + raw[:, 8:11], raw[:, 15], *dims)
        torque, cm = pressure_moment(raw[:, 5:8] + raw[:, 11:14], raw[:, 15], l_ref, *dims)
        for k, a in enumerate("xyz"):
            rows["f" + a] = force[:, k]
            rows["t" + a] = torque[:, k]
            rows["c" + a] = coeff[:, k]
            rows["cm" + a] = cm[:, k]
        return (rows, dropped.value) if with_dropped else rows

    def solve_residual(self, b, field, prev, a, c, per_plane=False):
        """Residual of the linearSolver system (b, field, prev, a, c) for the state as it is now (fs_solve_residual;
        collective on z-slabs; changes nothing): a dict with "r_sq" (sum of r^2 over the free cells), "rhs_sq" (sum of
        prev^2), "r_max", "cells", "relative" = sqrt(r_sq / rhs_sq), and with per_plane=True "per_plane", (depth, 4)
        records {r_sq, rhs_sq, r_max, cells} of the global planes 1..depth."""
        out = np.zeros(_lib.RESIDUAL_COLS, dtype=np.float64)
        pp = np.zeros((self.depth, _lib.RESIDUAL_COLS), dtype=np.float64) if per_plane else None
        check(self._L.fs_solve_residual(self._h, b, field, prev, float(a), float(c), out.ctypes.data,
                                        None if pp is None else pp.ctypes.data))
        return _residual_dict(out, pp)

    def diffuse_residual(self, b, field, prev, per_plane=False):
        """The same for the diffusion system of this handle, a = dt * diff * w * h * d and c = 1 + 6 a in its own
        precision (fs_diffuse_residual)."""
        out = np.zeros(_lib.RESIDUAL_COLS, dtype=np.float64)
        pp = np.zeros((self.depth, _lib.RESIDUAL_COLS), dtype=np.float64) if per_plane else None
        check(self._L.fs_diffuse_residual(self._h, b, field, prev, out.ctypes.data, None if pp is None else pp.ctypes.data))
        return _residual_dict(out, pp)

    def pressure_residual(self, per_plane=False):
        """The same for the pressure equation, (0, PRESSURE, DIVERGENCE, 1, 6): how far the last projection's solve got."""
        return self.solve_residual(0, _lib.PRESSURE, _lib.DIVERGENCE, 1.0, 6.0, per_plane=per_plane)

    def residual_log(self, with_dropped=False):
        """Drains the per-step residual log (option residual_log=N; fs_residual_log, collective on z-slabs): one row per
        retained step, oldest first, as a RESIDUAL_LOG_DTYPE structured array.  with_dropped=True returns
        (rows, number of logged steps the ring overwrote since the last drain)."""
        n, dropped = C.c_long(), C.c_long()
        check(self._L.fs_residual_log(self._h, None, 0, C.byref(n), C.byref(dropped)))
        raw = np.zeros((n.value, _lib.RESIDUAL_LOG_COLS), dtype=np.float64)
        check(self._L.fs_residual_log(self._h, raw.ctypes.data, n.value, C.byref(n), C.byref(dropped)))
        rows = np.zeros(n.value, dtype=RESIDUAL_LOG_DTYPE)
        for k, name in enumerate(RESIDUAL_LOG_DTYPE.names[:_lib.RESIDUAL_LOG_COLS]):
            rows[name] = raw[:, k]
        red = solve_reduction(raw)
        for k in range(_lib.RESIDUAL_LOG_SOLVES):
            rows["reduction_%d" % k] = red[:, k]
        return (rows, dropped.value) if with_dropped else rows

    def flow_monitor(self, per_plane=False, x_profile=False):
        """The flow monitor's record of the state as it is now (fs_flow_monitor; single-GPU handles; changes nothing): a
        dict of MONITOR_NAMES -> float over the target cells (interior, not solid), "values" the same 16 numbers as an
        array, "cfl" = (cfl_x, cfl_y, cfl_z) = ((double)dt * N) * max |.|, "kinetic_energy" = 0.5 * sum_e * h^3 with
        h = 1 / cbrt(w*h*d); per_plane=True adds "per_plane" (depth, 16), x_profile=True "x_profile" (width, 5:
        MONITOR_PROFILE_NAMES).  Every sum has one written order (include/fluidsim.h)."""
        out = np.zeros(_lib.MONITOR_COLS, dtype=np.float64)
        pp = np.zeros((self.depth, _lib.MONITOR_COLS), dtype=np.float64) if per_plane else None
        xp = np.zeros((self.width, _lib.MONITOR_PROFILE_COLS), dtype=np.float64) if x_profile else None
        check(self._L.fs_flow_monitor(self._h, out.ctypes.data, None if pp is None else pp.ctypes.data,
                                      None if xp is None else xp.ctypes.data))
        r = {name: float(out[k]) for k, name in enumerate(MONITOR_NAMES)}
        r["values"] = out
        w, h, d = self.width, self.height, self.depth
        r["cfl"] = monitor_cfl(self.dt, w, h, d, out[8], out[9], out[10])
        cell = 1.0 / float(np.cbrt(float(w * h * d)))
        r["kinetic_energy"] = 0.5 * float(out[6]) * (cell * cell * cell)
        if pp is not None:
            r["per_plane"] = pp
        if xp is not None:
            r["x_profile"] = xp
        return r

    def monitor_sample(self):
        """Appends a flow-monitor record of the state as it is now to the log (fs_step does so by itself with
        monitor_log=N, every monitor_every-th step)."""
        check(self._L.fs_monitor_sample(self._h))

    def monitor_log(self, with_dropped=False):
        """Drains the flow-monitor log (options monitor_log=N, monitor_every=K, monitor_stations="x1,x2,.."; fs_monitor_log):
        one row per retained record, oldest first, (n, 57) float64 with the columns MONITOR_LOG_NAMES -- step, the whole
        record, the x-profile row of each station (NaN for an unused one).  with_dropped=True returns (rows, number of
        records the ring overwrote since the last drain)."""
        n, dropped = C.c_long(), C.c_long()
        check(self._L.fs_monitor_log(self._h, None, 0, C.byref(n), C.byref(dropped)))
        rows = np.zeros((n.value, _lib.MONITOR_LOG_COLS), dtype=np.float64)
        check(self._L.fs_monitor_log(self._h, rows.ctypes.data, n.value, C.byref(n), C.byref(dropped)))
        return (rows, dropped.value) if with_dropped else rows

    def flow_stats(self, which, raw=False, dtype=None):
        """One field of the time-averaged flow statistics (options flow_stats="mean" | "moments", flow_stats_every,
        flow_stats_start; fs_flow_stats_field): `which` is STAT_MEAN_DENS .. STAT_MEAN_P, STAT_UU .. STAT_PP (covariances)
        or STAT_TKE; raw=True returns the raw fp64 sum instead.  Shaped like get(); float64 unless dtype says float32.  On
        z-slab handles the local slab, inter-slab halo planes 0."""
        dtype = np.dtype(dtype or np.float64)
        n = self._L.fs_padded_size(self._h)
        out = np.empty(n, dtype=dtype)
        check(self._L.fs_flow_stats_field(self._h, int(which) | (_lib.STAT_RAW if raw else 0), out.ctypes.data_as(C.c_void_p),
                                          n, dtype.itemsize))
        return out.reshape(self.shape)

    def flow_stats_sample(self):
        """Takes one sample of the state as it is now (fs_step does so by itself under the flow_stats options)."""
        check(self._L.fs_flow_stats_sample(self._h))

    def flow_stats_reset(self):
        """Forgets the samples taken so far; the next one starts the sums anew."""
        check(self._L.fs_flow_stats_reset(self._h))

    flow_stats_samples = property(lambda s: s._geti("flow_stats_samples"))

    def flow_stats_dump(self, dir):
        """Writes the mean flow as one float32 frame per file under `dir`, in the frame-dump layout the reference's
        viewers read: data, obs, v_x, v_y, v_z, p and (mode "moments") tke .bin (fs_flow_stats_dump; collective on z-slabs)."""
        check(self._L.fs_flow_stats_dump(self._h, os.fsencode(dir)))

    def vortex(self, which, dtype=None):
        """One vortex-identification field of the velocities as they are now (fs_vortex_field; collective on z-slabs):
        `which` is VORTEX_WX, VORTEX_WY, VORTEX_WZ (vorticity components), VORTEX_W2 (|omega|^2) or VORTEX_Q (the
        Q-criterion), per cell; 0 in solid and ghost cells.  Shaped like get(); float64 unless dtype says float32."""
        dtype = np.dtype(dtype or np.float64)
        n = self._L.fs_padded_size(self._h)
        out = np.empty(n, dtype=dtype)
        check(self._L.fs_vortex_field(self._h, int(which), out.ctypes.data_as(C.c_void_p), n, dtype.itemsize))
        return out.reshape(self.shape)

    def vortex_dump(self, dir):
        """Writes the five vortex fields as one float32 frame per file under `dir`, in the frame-dump layout:
        vort_x, vort_y, vort_z, vort_sq and q .bin (fs_vortex_dump; collective on z-slabs)."""
        check(self._L.fs_vortex_dump(self._h, os.fsencode(dir)))

    def confine_vorticity(self, eps):
        """One vorticity-confinement pass over the velocities now, of strength `eps` >= 0 (fs_confine_vorticity; single-GPU
        handles): v += dt * eps * (N x omega) in every fluid cell, N the unit vector up the gradient of |omega|, then the
        boundary handling of set_bounds.  The option vorticity_confinement=eps makes every step begin with such a pass."""
        check(self._L.fs_confine_vorticity(self._h, float(eps)))

    # -- heat and buoyancy (include/fluidsim.h, "heat and buoyancy"; single-GPU handles) --------------------------------------
    def set_heat(self, kappa=0.0, beta=0.0, alpha=0.0, up="+y", inlet=0.0, wall=None, box=None, log=0, in_step=True):
        """Switches heat on (fs_heat_params): a temperature theta, the excess over ambient, with thermal diffusivity `kappa`,
        buoyancy `beta` per unit theta and weight `alpha` per unit smoke density along `up` ("+x" .. "-z" or 0..5), `inlet`
        forced on the plane x = 1, and -- with `wall` a temperature -- the fluid cells beside a solid inside `box` =
        (x0, x1, y0, y1, z0, z1) in cells (default: the whole domain) held at it.  in_step=True makes every step apply and
        transport it (mode 2), False leaves that to heat_apply() / heat_transport() (mode 1).  log=N keeps the heat budget of
        the last N steps (heat_log()).  theta starts at 0 and survives a change of the parameters."""
        par = np.zeros(_lib.HEAT_PARAMS, dtype=np.float64)
        par[0] = 2 if in_step else 1
        par[1:4] = float(kappa), float(beta), float(alpha)
        par[4] = _lib.HEAT_UP[up] if isinstance(up, str) else int(up)
        par[5] = float(inlet)
        par[6] = 0 if wall is None else 1
        par[7] = 0.0 if wall is None else float(wall)
        par[8:14] = (1, self.width, 1, self.height, 1, self.depth) if box is None else tuple(box)
        par[14] = int(log)
        check(self._L.fs_heat_params(self._h, par.ctypes.data, par.size))

    def set_heat_params(self, par):
        """fs_heat_params with the HEAT_PARAMS numbers as they are (heat_params() returns them in this form)."""
        par = np.ascontiguousarray(par, dtype=np.float64).reshape(-1)
        check(self._L.fs_heat_params(self._h, par.ctypes.data, par.size))

    def heat_off(self):
        """Switches heat off and frees theta; the other parameters stay as they were."""
        par = self.heat_params()
        par[0] = 0
        check(self._L.fs_heat_params(self._h, par.ctypes.data, par.size))

    def heat_params(self):
        """The HEAT_PARAMS numbers in force (fs_heat_params_get)."""
        par = np.zeros(_lib.HEAT_PARAMS, dtype=np.float64)
        check(self._L.fs_heat_params_get(self._h, par.ctypes.data, par.size))
        return par

    def temperature(self, dtype=None):
        """theta, shaped like get() (fs_heat_get)."""
        dtype = np.dtype(dtype or self.dtype)
        n = self._L.fs_padded_size(self._h)
        out = np.empty(n, dtype=dtype)
        check(self._L.fs_heat_get(self._h, out.ctypes.data_as(C.c_void_p), n, dtype.itemsize))
        return out.reshape(self.shape)

    def set_temperature(self, arr):
        """Overwrites theta with a padded array, ghosts included; no bounds are applied (fs_heat_set)."""
        a = np.ascontiguousarray(arr)
        if a.dtype not in (np.float32, np.float64):
            a = a.astype(self.dtype)
        a = a.reshape(-1)
        check(self._L.fs_heat_set(self._h, a.ctypes.data_as(C.c_void_p), a.size, a.dtype.itemsize))

    def heat_apply(self):
        """Pass A now: inlet and wall temperatures, then the buoyancy force on the velocity component along `up`."""
        check(self._L.fs_heat_apply(self._h))

    def heat_transport(self):
        """Pass B now: theta is diffused with `kappa` and carried by the velocities as they are."""
        check(self._L.fs_heat_transport(self._h))

    def heat_budget(self, per_plane=False):
        """The heat budget of the state as it is now (fs_heat_budget; changes nothing): a dict of HEAT_NAMES -> float over the
        cells that are not solid, "values" the same HEAT_COLS numbers as an array; per_plane=True adds "per_plane"
        (depth, HEAT_COLS).  Every sum has one written order (include/fluidsim.h)."""
        out = np.zeros(_lib.HEAT_COLS, dtype=np.float64)
        pp = np.zeros((self.depth, _lib.HEAT_COLS), dtype=np.float64) if per_plane else None
        check(self._L.fs_heat_budget(self._h, out.ctypes.data, None if pp is None else pp.ctypes.data))
        r = {name: float(out[k]) for k, name in enumerate(_lib.HEAT_NAMES)}
        r["values"] = out
        if pp is not None:
            r["per_plane"] = pp
        return r

    def heat_log(self, with_dropped=False):
        """Drains the heat log (set_heat(log=N); fs_heat_log): one row per retained record, oldest first, (n, HEAT_LOG_COLS)
        float64 -- step, then the budget.  with_dropped=True returns (rows, records the ring overwrote since the last drain)."""
        n, dropped = C.c_long(), C.c_long()
        check(self._L.fs_heat_log(self._h, None, 0, C.byref(n), C.byref(dropped)))
        rows = np.zeros((n.value, _lib.HEAT_LOG_COLS), dtype=np.float64)
        check(self._L.fs_heat_log(self._h, rows.ctypes.data, n.value, C.byref(n), C.byref(dropped)))
        return (rows, dropped.value) if with_dropped else rows

    # -- momentum zones (include/fluidsim.h, "momentum zones"; single-GPU handles) ----------------------------------------------
    def set_zones(self, zones, mode="step", log=0):
        """Sets the momentum zones (fs_zones): `zones` is a sequence of rows of ZONE_PARAMS numbers, as the constructors of
        fluid_simulation_amd.zones return them (a list of rows, or rows and lists of rows mixed: sponge() returns several).
        mode "step" applies the pass in every step, "manual" leaves it to apply_zones(), "off" (or no rows) frees everything.
        log=N keeps the zone budgets of the last N steps (zone_log())."""
        rows = [np.asarray(z, dtype=np.float64).reshape(-1, _lib.ZONE_PARAMS) for z in ([] if zones is None else zones)]
        par = np.ascontiguousarray(np.concatenate(rows)) if rows else np.zeros((0, _lib.ZONE_PARAMS))
        m = _lib.ZONE_MODES[mode] if isinstance(mode, str) else int(mode)
        check(self._L.fs_zones(self._h, par.ctypes.data if par.size else None, par.shape[0], m, int(log)))

    def zones(self):
        """The zones in force (fs_zones_get): (rows (n, ZONE_PARAMS), mode, log)."""
        par = np.zeros((_lib.ZONE_MAX, _lib.ZONE_PARAMS), dtype=np.float64)
        n, mode, log = C.c_int(), C.c_int(), C.c_int()
        check(self._L.fs_zones_get(self._h, par.ctypes.data, C.byref(n), C.byref(mode), C.byref(log)))
        return par[:n.value].copy(), mode.value, log.value

    def apply_zones(self):
        """The zone pass now (fs_zone_apply)."""
        check(self._L.fs_zone_apply(self._h))

    def zone_budget(self, per_plane=False):
        """What a zone pass now would do (fs_zone_budget; changes nothing): (n_zones, ZONE_COLS) float64 -- the columns are
        ZONE_NAMES; per_plane=True returns (that, the same per plane: (depth, n_zones, ZONE_COLS))."""
        n = self.zones()[0].shape[0]
        out = np.zeros((n, _lib.ZONE_COLS), dtype=np.float64)
        pp = np.zeros((self.depth, n, _lib.ZONE_COLS), dtype=np.float64) if per_plane else None
        check(self._L.fs_zone_budget(self._h, out.ctypes.data, None if pp is None else pp.ctypes.data))
        return (out, pp) if per_plane else out

    def zone_log(self, with_dropped=False):
        """Drains the zone log (set_zones(log=N); fs_zone_log): one row per retained record, oldest first, (n, 1 + n_zones *
        ZONE_COLS) float64 -- the step, then the budget taken before that step's pass.  with_dropped=True returns (rows,
        records the ring overwrote since the last drain)."""
        cols = 1 + self.zones()[0].shape[0] * _lib.ZONE_COLS
        n, dropped = C.c_long(), C.c_long()
        check(self._L.fs_zone_log(self._h, None, 0, C.byref(n), C.byref(dropped)))
        rows = np.zeros((n.value, cols), dtype=np.float64)
        check(self._L.fs_zone_log(self._h, rows.ctypes.data, n.value, C.byref(n), C.byref(dropped)))
        return (rows, dropped.value) if with_dropped else rows

    def zone_mask(self):
        """Which target cells lie in which zone (fs_zone_mask): uint8, shaped like get(); bit k = zone k."""
        out = np.zeros(self.shape, dtype=np.uint8)
        check(self._L.fs_zone_mask(self._h, out.ctypes.data, out.size))
        return out

    def set_inflow(self, profile=None, rms=None, gust=None, eddies=0, sigma=4.0, u_rms=0.0, convect="auto", seed=1):
        """Configures the inflow generator and turns it on (include/fluidsim.h, "turbulent inflow"; single-GPU handles): every
        step then writes the x = 1 face as v_x = g(t) * U + r * u'_x, v_y = r * u'_y, v_z = r * u'_z.  `profile` (U) and
        `rms` (r) are maps of shape (depth, height) or None (speed everywhere / 1 everywhere; fluid_simulation_amd.inflow
        has power_law, log_law and intensity_profile); `gust` a sequence of (step, factor) knots or None; `eddies`, `sigma`,
        `u_rms`, `convect` (cells per step or "auto") and `seed` the synthetic eddies.  The same options are constructor
        keywords (inflow="on", inflow_eddies=N, inflow_sigma=S, inflow_rms=R, inflow_convect=C, inflow_seed=K).
        set_option("inflow", "off") restores the uniform inlet."""
        n = self.height * self.depth
        maps = []
        for m in (profile, rms):
            maps.append(None if m is None else np.ascontiguousarray(m, dtype=np.float64).reshape(-1))
            if maps[-1] is not None and maps[-1].size != n:
                raise ValueError("an inflow map has height * depth = %d values, not %d" % (n, maps[-1].size))
        check(self._L.fs_inflow_profile(self._h, *[None if m is None else m.ctypes.data for m in maps], n))
        knots = np.zeros((0, 2)) if gust is None else np.ascontiguousarray(gust, dtype=np.float64).reshape(-1, 2)
        ts, fs = np.ascontiguousarray(knots[:, 0]), np.ascontiguousarray(knots[:, 1])
        check(self._L.fs_inflow_gust(self._h, ts.ctypes.data, fs.ctypes.data, len(ts)))
        self.set_option("inflow_eddies", int(eddies))
        self.set_option("inflow_sigma", repr(float(sigma)))
        self.set_option("inflow_rms", repr(float(u_rms)))
        self.set_option("inflow_convect", convect if isinstance(convect, str) else repr(float(convect)))
        self.set_option("inflow_seed", int(seed))
        self.set_option("inflow", "on")

    def inflow_plane(self, step):
        """The three fp64 components of the inlet plane at step number `step`, before the rounding to the field type, as an
        array (3, depth, height) (fs_inflow_plane); works whether the inflow generator is on or off and changes no field."""
        out = np.empty((3, self.depth, self.height), dtype=np.float64)
        check(self._L.fs_inflow_plane(self._h, int(step), out.ctypes.data, out.size))
        return out

    def inflow_eddies(self, step):
        """The synthetic eddies at step number `step` (fs_inflow_eddies): an array (N, 6) of ex, ey, ez and the three signs."""
        out = np.empty((self._geti("inflow_eddies"), 6), dtype=np.float64)
        check(self._L.fs_inflow_eddies(self._h, int(step), out.ctypes.data, out.size))
        return out

    def isosurface(self, source, level):
        """The triangle mesh of {source > level} over the padded box (fs_isosurface; single-GPU handles): `source` is a
        field selector (DENS .. BUFFER) or ISO_VORTEX | VORTEX_*.  Returns (vertices (n, 3) float32 in the viewer's
        padded (x, y, z) index space, faces (m, 3) int32), normals pointing from inside to outside."""
        nv, nt = C.c_long(), C.c_long()
        check(self._L.fs_isosurface(self._h, int(source), float(level), C.byref(nv), C.byref(nt)))
        verts = np.zeros((nv.value, 3), dtype=np.float32)
        faces = np.zeros((nt.value, 3), dtype=np.int32)
        check(self._L.fs_isosurface_fetch(self._h, verts.ctypes.data, faces.ctypes.data))
        return verts, faces

    def sample_points(self, points):
        """Keeps the points at which sample() evaluates (fs_sample_points; single-GPU handles): `points` is (n, 3), x, y, z
        in the viewer's padded index space, a cell's value sitting at its integer coordinates.  Replaces the earlier set."""
        p = np.ascontiguousarray(points, dtype=np.float64).reshape(-1, 3)
        check(self._L.fs_sample_points(self._h, p.ctypes.data_as(C.c_void_p), p.shape[0]))
        self._sample_n = p.shape[0]

    def sample(self, source, mode="linear"):
        """The value of `source` at the kept points (fs_sample), (n,) float64; NaN outside the padded box.  `source` is a
        field selector (DENS .. BUFFER), ISO_VORTEX | VORTEX_*, or SAMPLE_STAT | STAT_* (| STAT_RAW); `mode` is "nearest"
        (the stored value of the nearest cell), "linear" (the reference's trilinear form) or "fluid" (the weighted mean of
        the corners that are not solid: the mode for points on an obstacle's surface), or a SAMPLE_* constant."""
        m = _lib.SAMPLE_MODES[mode] if isinstance(mode, str) else int(mode)
        n = getattr(self, "_sample_n", 0)
        out = np.empty(n, dtype=np.float64)
        check(self._L.fs_sample(self._h, int(source), m, out.ctypes.data_as(C.c_void_p), n))
        return out

    def set_probes(self, cells):
        """Sets the probe cells of the per-step probe log (fs_set_probes): `cells` is (n, 3) integers x, y, z in padded
        global coordinates (ghost cells allowed), n up to PROBE_MAX; an empty list turns the probes off.  Clears the log."""
        c = np.ascontiguousarray(cells, dtype=np.intc).reshape(-1, 3)
        check(self._L.fs_set_probes(self._h, c.ctypes.data_as(C.c_void_p), c.shape[0]))

    probe_count = property(lambda s: s._geti("probe_count"))

    def probe_sample(self):
        """Takes one record of the probes from the state as it is now (fs_step does so by itself with probe_log=N)."""
        check(self._L.fs_probe_sample(self._h))

    def probe_log(self, with_dropped=False):
        """Drains the per-step probe log (option probe_log=N; fs_probe_log, collective on z-slabs): {"step": (R,) int64,
        "values": (R, n, 5) float64 -- dens, v_x, v_y, v_z, pressure of each probe}, oldest record first.
        with_dropped=True returns (that, number of records the ring overwrote since the last drain)."""
        n, dropped = C.c_long(), C.c_long()
        count = self.probe_count
        cols = 1 + _lib.PROBE_VALUES * count
        check(self._L.fs_probe_log(self._h, None, 0, C.byref(n), C.byref(dropped)))
        raw = np.zeros((n.value, cols), dtype=np.float64)
        check(self._L.fs_probe_log(self._h, raw.ctypes.data_as(C.c_void_p), n.value, C.byref(n), C.byref(dropped)))
        log = {"step": raw[:, 0].astype(np.int64), "values": raw[:, 1:].reshape(n.value, count, _lib.PROBE_VALUES).copy()}
        return (log, dropped.value) if with_dropped else log

    # -- slice and projection images (single GPU) ----------------------------------------------
    def _image_shape(self, kind, axis, index):
        cols, rows = C.c_int(), C.c_int()
        check(self._L.fs_image_values(self._h, _lib.DENS, kind, int(axis), int(index), None, 0, C.byref(cols), C.byref(rows)))
        return rows.value, cols.value

    def image_values(self, source, kind, axis, index=0):
        """One value image of the state as it is now (fs_image_values): (rows, cols) float64.  `kind` is "slice" (the
        stored values at padded index `index` of `axis`), "sum", "max" or "min" (over the interior cells of the axis,
        in increasing order), or an IMG_* constant; `axis` is 0 (x), 1 (y) or 2 (z); `source` as for sample()."""
        k = _lib.IMG_KINDS[kind] if isinstance(kind, str) else int(kind)
        rows, cols = self._image_shape(k, axis, index)
        out = np.empty((rows, cols), dtype=np.float64)
        check(self._L.fs_image_values(self._h, int(source), k, int(axis), int(index), out.ctypes.data_as(C.c_void_p), out.size,
                                      None, None))
        return out

    def image_rgb(self, source, kind, axis, index=0, vmin=0.0, vmax=1.0, obstacle_alpha=0.0):
        """The same image through the handle's colour table (fs_image_rgb): (rows, cols, 3) uint8.  Values are clamped
        to vmin .. vmax, NaN is black, obstacle pixels are darkened by the factor 1 - obstacle_alpha."""
        k = _lib.IMG_KINDS[kind] if isinstance(kind, str) else int(kind)
        rows, cols = self._image_shape(k, axis, index)
        out = np.empty((rows, cols, 3), dtype=np.uint8)
        check(self._L.fs_image_rgb(self._h, int(source), k, int(axis), int(index), float(vmin), float(vmax),
                                   float(obstacle_alpha), out.ctypes.data_as(C.c_void_p), out.size, None, None))
        return out

    def set_colormap(self, table=None):
        """Sets the colour table (fs_image_colormap): (n, 3) uint8, n = 2 .. 4096; None restores the built-in one, the
        256 entries of the reference's 2-D viewer."""
        if table is None:
            check(self._L.fs_image_colormap(self._h, None, 0))
            return
        t = np.ascontiguousarray(table, dtype=np.uint8).reshape(-1, 3)
        check(self._L.fs_image_colormap(self._h, t.ctypes.data_as(C.c_void_p), t.shape[0]))

    def set_image_views(self, views):
        """Sets the views of the per-step image log (fs_image_views): a list of up to IMAGE_VIEWS_MAX tuples (source,
        kind, axis, index, vmin, vmax[, obstacle_alpha]); an empty list turns the log off.  Clears the log."""
        spec = np.zeros((len(views), 4), dtype=np.intc)
        rng = np.zeros((len(views), 3), dtype=np.float64)
        for i, v in enumerate(views):
            spec[i] = (int(v[0]), _lib.IMG_KINDS[v[1]] if isinstance(v[1], str) else int(v[1]), int(v[2]), int(v[3]))
            rng[i] = (float(v[4]), float(v[5]), float(v[6]) if len(v) > 6 else 0.0)
        check(self._L.fs_image_views(self._h, spec.ctypes.data_as(C.c_void_p), rng.ctypes.data_as(C.c_void_p), len(views)))
        self._image_views = [tuple(int(x) for x in row) for row in spec]

    image_view_count = property(lambda s: s._geti("image_views"))
    image_frame_bytes = property(lambda s: s._geti("image_frame_bytes"))

    def image_sample(self):
        """Takes one frame of the image views from the state as it is now (fs_step does so by itself with image_log=N)."""
        check(self._L.fs_image_sample(self._h))

    def image_log(self, with_dropped=False):
        """Drains the per-step image log (option image_log=N; fs_image_log): (steps, images) -- steps (F,) int64, and
        for each view an (F, rows, cols, 3) uint8 array, oldest frame first.  with_dropped=True returns (steps, images,
        number of frames the ring overwrote since the last drain)."""
        n, dropped = C.c_long(), C.c_long()
        check(self._L.fs_image_log(self._h, None, None, 0, C.byref(n), C.byref(dropped)))
        per = self.image_frame_bytes
        raw = np.zeros((n.value, per), dtype=np.uint8)
        steps = np.zeros(n.value, dtype=np.int64)
        check(self._L.fs_image_log(self._h, raw.ctypes.data_as(C.c_void_p), steps.ctypes.data_as(C.c_void_p), n.value,
                                   C.byref(n), C.byref(dropped)))
        images, at = [], 0
        for (_, kind, axis, index) in getattr(self, "_image_views", []):
            rows, cols = self._image_shape(kind, axis, index)
            images.append(raw[:, at:at + 3 * rows * cols].reshape(n.value, rows, cols, 3).copy())
            at += 3 * rows * cols
        return (steps, images, dropped.value) if with_dropped else (steps, images)

    # -- volume rendering (single GPU) -------------------------------------------------------------
    @staticmethod
    def _volume_par(vmin=0.0, vmax=1.0, opacity=1.0, step=0.5, t_min=0.01, obstacle=(128, 128, 128), background=(26, 26, 26)):
        return np.array([vmin, vmax, opacity, step, t_min] + [float(c) for c in obstacle] + [float(c) for c in background],
                        dtype=np.float64)

    def volume_rays(self, slot, rays):
        """Stores a ray set in camera slot `slot` (fs_volume_rays): (rows, cols, 6) float64, {ox, oy, oz, dx, dy, dz} per
        pixel in the viewer's padded coordinates, row 0 the top of the image.  None frees the slot."""
        if rays is None:
            check(self._L.fs_volume_rays(self._h, int(slot), None, 0, 0))
            self._volume_size.pop(int(slot), None)
            return
        r = np.ascontiguousarray(rays, dtype=np.float64)
        if r.ndim != 3 or r.shape[2] != 6:
            raise ValueError("expected (rows, cols, 6) rays")
        check(self._L.fs_volume_rays(self._h, int(slot), r.ctypes.data_as(C.c_void_p), r.shape[1], r.shape[0]))
        self._volume_size[int(slot)] = (r.shape[0], r.shape[1])

    def volume_camera(self, slot, eye, target, up=(0.0, 1.0, 0.0), fov_deg=45.0, ortho_height=None, size=(512, 512)):
        """Builds the rays of a pinhole camera (vertical field of view `fov_deg`) or, with `ortho_height` (the height of the
        image plane in cells), of an orthographic one, on the host in fp64, into camera slot `slot` (fs_volume_camera).
        `size` is (cols, rows).  The tangent is taken here; the library holds no trigonometry."""
        half = 0.5 * float(ortho_height) if ortho_height is not None else float(np.tan(np.deg2rad(np.float64(fov_deg)) / 2.0))
        cam = np.array(list(eye) + list(target) + list(up) + [half, 1.0 if ortho_height is not None else 0.0], dtype=np.float64)
        if cam.size != _lib.VOLUME_CAMERA:
            raise ValueError("eye, target and up are three numbers each")
        cols, rows = int(size[0]), int(size[1])
        check(self._L.fs_volume_camera(self._h, int(slot), cam.ctypes.data_as(C.c_void_p), cols, rows))
        self._volume_size[int(slot)] = (rows, cols)

    def volume_render(self, source, slot, with_acc=False, **par):
        """One ray-marched image of `source` (as for sample()) through the rays of camera slot `slot` (fs_volume_render):
        (rows, cols, 3) uint8; with_acc=True returns (rgb, acc), acc (rows, cols, 4) float64 = the composited colour and the
        remaining transparency before the background is added.  Keywords: vmin, vmax, opacity, step, t_min, obstacle,
        background (the two colours as three numbers in 0 .. 255)."""
        if int(slot) not in self._volume_size:
            raise ValueError("camera slot %d holds no rays (volume_camera, volume_rays)" % int(slot))
        rows, cols = self._volume_size[int(slot)]
        p = self._volume_par(**par)
        rgb = np.empty((rows, cols, 3), dtype=np.uint8)
        acc = np.empty((rows, cols, 4), dtype=np.float64) if with_acc else None
        check(self._L.fs_volume_render(self._h, int(source), int(slot), p.ctypes.data_as(C.c_void_p),
                                       rgb.ctypes.data_as(C.c_void_p), rgb.size,
                                       acc.ctypes.data_as(C.c_void_p) if with_acc else None, acc.size if with_acc else 0))
        return (rgb, acc) if with_acc else rgb

    def set_volume_views(self, views):
        """Sets the views of the per-step volume log (fs_volume_views): a list of up to VOLUME_VIEWS_MAX tuples (source,
        slot[, dict of volume_render's keywords]); an empty list turns the log off.  Clears the log."""
        spec = np.zeros((len(views), 2), dtype=np.intc)
        par = np.zeros((len(views), _lib.VOLUME_PARAMS), dtype=np.float64)
        for i, v in enumerate(views):
            spec[i] = (int(v[0]), int(v[1]))
            par[i] = self._volume_par(**(v[2] if len(v) > 2 else {}))
        check(self._L.fs_volume_views(self._h, spec.ctypes.data_as(C.c_void_p), par.ctypes.data_as(C.c_void_p), len(views)))
        self._volume_views = [int(row[1]) for row in spec]

    volume_view_count = property(lambda s: s._geti("volume_views"))
    volume_frame_bytes = property(lambda s: s._geti("volume_frame_bytes"))

    def volume_sample(self):
        """Takes one frame of the volume views from the state as it is now (fs_step does so by itself with volume_log=N)."""
        check(self._L.fs_volume_sample(self._h))

    def volume_log(self, with_dropped=False):
        """Drains the per-step volume log (option volume_log=N; fs_volume_log): (steps, images) -- steps (F,) int64, and
        for each view an (F, rows, cols, 3) uint8 array, oldest frame first.  with_dropped=True returns (steps, images,
        number of frames the ring overwrote since the last drain)."""
        n, dropped = C.c_long(), C.c_long()
        check(self._L.fs_volume_log(self._h, None, None, 0, C.byref(n), C.byref(dropped)))
        per = self.volume_frame_bytes
        raw = np.zeros((n.value, per), dtype=np.uint8)
        steps = np.zeros(n.value, dtype=np.int64)
        check(self._L.fs_volume_log(self._h, raw.ctypes.data_as(C.c_void_p), steps.ctypes.data_as(C.c_void_p), n.value,
                                    C.byref(n), C.byref(dropped)))
        images, at = [], 0
        for slot in getattr(self, "_volume_views", []):
            rows, cols = self._volume_size[slot]
            images.append(raw[:, at:at + 3 * rows * cols].reshape(n.value, rows, cols, 3).copy())
            at += 3 * rows * cols
        return (steps, images, dropped.value) if with_dropped else (steps, images)

    # -- tracer particles (single GPU) -----------------------------------------------------------
    tracer_count = property(lambda s: s._geti("tracer_count"))
    tracer_capacity = property(lambda s: s._geti("tracer_capacity"))

    def tracer_seed(self, points):
        """Appends particles to the tracer pool (option tracers=C; fs_tracer_seed): `points` is (n, 3), x, y, z in the
        viewer's padded index space, every one inside 0.5 .. N + 0.5 on each axis.  The j-th particle ever seeded goes
        into slot j % C: a full pool overwrites its oldest particles."""
        p = np.ascontiguousarray(points, dtype=np.float64).reshape(-1, 3)
        check(self._L.fs_tracer_seed(self._h, p.ctypes.data_as(C.c_void_p), p.shape[0]))

    def tracer_emitters(self, points, every=1):
        """Sets the emitters (fs_tracer_emitters): up to TRACER_EMITTERS_MAX points; every `every`-th step releases one
        particle per emitter, `source` = the emitter's index.  An empty list turns them off.  Replaces the list."""
        p = np.ascontiguousarray(points, dtype=np.float64).reshape(-1, 3)
        check(self._L.fs_tracer_emitters(self._h, p.ctypes.data_as(C.c_void_p), p.shape[0], int(every)))

    def tracer_advance(self):
        """Moves the particles through the velocity field as it is now, releases one particle per emitter and takes a
        snapshot (fs_tracer_advance; fs_step does all this by itself with tracers=C)."""
        check(self._L.fs_tracer_advance(self._h))

    def tracer_clear(self):
        """Frees every slot, resets the seed counter and clears the snapshot log (fs_tracer_clear)."""
        check(self._L.fs_tracer_clear(self._h))

    def tracers(self):
        """The pool's slots 0 .. tracer_count - 1 (fs_tracer_fetch): {"xyz": (n, 3) float64, "status", "source", "born",
        "moves": (n,) int32}; status is TRACER_FREE, TRACER_ALIVE, TRACER_OUT (left the box; xyz is where) or TRACER_HIT
        (ended in a solid cell)."""
        n = C.c_long()
        check(self._L.fs_tracer_fetch(self._h, None, None, 0, C.byref(n)))
        xyz = np.zeros((n.value, 3), dtype=np.float64)
        meta = np.zeros((n.value, 4), dtype=np.int32)
        check(self._L.fs_tracer_fetch(self._h, xyz.ctypes.data_as(C.c_void_p), meta.ctypes.data_as(C.c_void_p), n.value, C.byref(n)))
        return {"xyz": xyz, "status": meta[:, 0].copy(), "source": meta[:, 1].copy(), "born": meta[:, 2].copy(),
                "moves": meta[:, 3].copy()}

    def tracer_sample(self, source, mode="linear"):
        """The value of `source` at the particles' current positions (fs_tracer_sample), (tracer_count,) float64: the
        sampler on the pool's own position array.  `source` and `mode` as for sample()."""
        m = _lib.SAMPLE_MODES[mode] if isinstance(mode, str) else int(mode)
        n = self.tracer_count
        out = np.empty(n, dtype=np.float64)
        check(self._L.fs_tracer_sample(self._h, int(source), m, out.ctypes.data_as(C.c_void_p), n))
        return out

    def tracer_log(self, with_dropped=False):
        """Drains the snapshot log of the pool (option tracer_log=N; fs_tracer_log): {"step": (F,) int64, "xyz": (F, C, 3)
        float64, "status": (F, C) int32}, oldest frame first.  with_dropped=True returns (that, number of frames the ring
        overwrote since the last drain)."""
        n, dropped = C.c_long(), C.c_long()
        cap = self.tracer_capacity
        check(self._L.fs_tracer_log(self._h, None, None, None, 0, C.byref(n), C.byref(dropped)))
        xyz = np.zeros((n.value, cap, 3), dtype=np.float64)
        status = np.zeros((n.value, cap), dtype=np.int32)
        steps = np.zeros(n.value, dtype=np.int64)
        check(self._L.fs_tracer_log(self._h, xyz.ctypes.data_as(C.c_void_p), status.ctypes.data_as(C.c_void_p),
                                    steps.ctypes.data_as(C.c_void_p), n.value, C.byref(n), C.byref(dropped)))
        log = {"step": steps, "xyz": xyz, "status": status}
        return (log, dropped.value) if with_dropped else log

    def time_sweeps(self, b, field, prev, a, c, reps):
        ms = C.c_double()
        check(self._L.fs_time_sweeps(self._h, b, field, prev, a, c, reps, C.byref(ms)))
        return ms.value

    def comm_transport(self):
        return (self._L.fs_comm_transport(self._h) or b"").decode(errors="replace")

    def comm_init(self, rank, nranks, unique_id):
        buf = C.create_string_buffer(bytes(unique_id), _lib.COMM_ID_BYTES)
        check(self._L.fs_comm_init(self._h, rank, nranks, buf))


def comm_unique_id(transport="rccl"):
    """128-byte id for fs_comm_init.  "rccl": an ncclUniqueId (RCCL over xGMI, one GPU per rank).
    "shm": a host-staged development transport through POSIX shared memory, for ranks that
    are processes on one host and may share a GPU (tests on a 1-GPU box).
    "ipc": a stream-ordered device-to-device transport between rank processes of one host (hipIpc-mapped
    arrays, copy engines, device-side handshakes; ranks may share a GPU) -- csrc/ipc.h."""
    if transport in ("shm", "ipc"):
        name = "%s:/fs_slab_%d_%s" % ("FSSHM" if transport == "shm" else "FSIPC", os.getpid(), os.urandom(4).hex())
        return name.encode().ljust(_lib.COMM_ID_BYTES, b"\0")
    buf = C.create_string_buffer(_lib.COMM_ID_BYTES)
    check(_lib.lib().fs_comm_unique_id(buf))
    return buf.raw


def loadSTLIntoObstacles(stlFile, sim, scale=0.8, rot_x=0.0, rot_y=0.0, rot_z=0.0,
                         translate_x=0.0, translate_y=0.0, translate_z=0.0):
    """loadSTLIntoObstacles -- object_loader.h:7-17.  Like the reference, a file that cannot
    be read leaves the tunnel empty and is not an exception; returns the number of accepted
    sample points ("Added N obstacle points"), or None when the file could not be loaded."""
    added = C.c_long(0)
    rc = sim._L.fs_load_stl(sim._h, os.fsencode(stlFile), scale, rot_x, rot_y, rot_z,
                            translate_x, translate_y, translate_z, C.byref(added))
    if rc == _lib.EIO:
        return None
    check(rc)
    return added.value
