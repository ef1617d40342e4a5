"""numpy fp64 restatement of the tracer particles, written from the definition in include/fluidsim.h ("tracer particles"),
not from csrc/tracers.h: the move, the seeding and slot rule, the emitters' and the snapshots' schedule.  LIN is
sample_model.sample in mode LINEAR.  numpy's elementwise fp64 operations are IEEE and are never contracted, so every line of
the move is one rounding, in the order the definition writes them; the tests compare bit patterns, with no tolerance.

Fields are dense padded arrays shaped (D+2, H+2, W+2) as Simulation.get returns them (float32 or float64); positions are
(n, 3) float64, x, y, z."""
import numpy as np

import sample_model as SM

FREE, ALIVE, OUT, HIT = 0, 1, 2, 3
EMITTERS_MAX = 4096
FRAME_BYTES = 28


def extents(field):
    d, h, w = (k - 2 for k in np.asarray(field).shape)
    return w, h, d


def in_box(p, whd):
    """0.5 <= c <= N + 0.5 on each axis; NaN is outside"""
    hi = np.asarray(whd, dtype=np.float64) + 0.5
    with np.errstate(invalid="ignore"):
        return ((p >= 0.5) & (p <= hi)).all(axis=1)


def displacement(dt, whd):
    """k = ((double)dt * w, (double)dt * h, (double)dt * d) of a float dt"""
    return np.float64(np.float32(dt)) * np.asarray(whd, dtype=np.float64)


def _velocity(vx, vy, vz, p):
    return np.stack([SM.sample(f, None, p, SM.LINEAR) for f in (vx, vy, vz)], axis=1)


def move(vx, vy, vz, obs, dt, p):
    """The move of ALIVE particles at p: -> (p', status'), and whether the midpoint lay in B."""
    whd = extents(vx)
    p = np.asarray(p, dtype=np.float64).reshape(-1, 3)
    k = displacement(dt, whd)
    h = 0.5 * k
    with np.errstate(invalid="ignore", over="ignore"):
        u1 = _velocity(vx, vy, vz, p)
        d1 = h * u1
        m = p + d1
        mid_in = in_box(m, whd)
        u2 = _velocity(vx, vy, vz, np.where(mid_in[:, None], m, 1.0))
        d2 = k * u2
        full = p + d2
    q = np.where(mid_in[:, None], full, m)
    q_in = in_box(q, whd)
    with np.errstate(invalid="ignore"):
        cell = np.floor(np.where(q_in[:, None], q, 1.0) + 0.5).astype(np.int64)
    solid = np.asarray(obs)[cell[:, 2], cell[:, 1], cell[:, 0]] == 1
    status = np.where(~q_in, OUT, np.where(solid, HIT, ALIVE)).astype(np.int32)
    return q, status, mid_in


class Pool:
    """The pool of C slots with its host-side cursor, the emitters and the snapshot ring of `log` frames."""

    def __init__(self, capacity, log=0, every=1):
        self.C = int(capacity)
        self.log, self.every = int(log), int(every)
        self.emit, self.emit_every = np.zeros((0, 3)), 1
        self.clear()

    def clear(self):
        self.xyz = np.zeros((self.C, 3), dtype=np.float64)
        self.meta = np.zeros((self.C, 4), dtype=np.int32)     # status, source, born, moves
        self.seeded = 0
        self.frames = []                                       # (step, xyz, status), oldest first
        self.dropped = 0

    @property
    def count(self):
        return min(self.seeded, self.C)

    def _append(self, points, source, born):
        for j, p in enumerate(np.asarray(points, dtype=np.float64).reshape(-1, 3)):
            s = self.seeded % self.C
            self.xyz[s] = p
            self.meta[s] = (ALIVE, -1 if source is None else j, born, 0)
            self.seeded += 1

    def seed(self, points, steps_total):
        self._append(points, None, steps_total)

    def emitters(self, points, every=1):
        self.emit, self.emit_every = np.asarray(points, dtype=np.float64).reshape(-1, 3).copy(), int(every)

    def advance(self, vx, vy, vz, obs, dt, steps_total, release=True, snapshot=True):
        """1. every ALIVE particle moves, 2. the release, 3. the snapshot"""
        alive = np.flatnonzero(self.meta[:, 0] == ALIVE)
        if alive.size:
            q, status, _ = move(vx, vy, vz, obs, dt, self.xyz[alive])
            self.xyz[alive] = q
            self.meta[alive, 0] = status
            self.meta[alive, 3] += 1
        if release and len(self.emit):
            self._append(self.emit, "emitter", steps_total)
        if snapshot and self.log > 0:
            self.frames.append((steps_total, self.xyz.copy(), self.meta[:, 0].copy()))
            if len(self.frames) > self.log:
                self.frames.pop(0)
                self.dropped += 1

    def step(self, vx, vy, vz, obs, dt, steps_total):
        """what fs_step does at its sample point; steps_total counts the step that is ending"""
        self.advance(vx, vy, vz, obs, dt, steps_total, (steps_total - 1) % self.emit_every == 0,
                     (steps_total - 1) % self.every == 0)

    def drain(self):
        frames, dropped = self.frames, self.dropped
        self.frames, self.dropped = [], 0
        return frames, dropped


def same_bits(got, want):
    return SM.same_bits(got, want)
