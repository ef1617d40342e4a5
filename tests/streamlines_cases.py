"""The streamline cases shared by tests/test_streamlines_cases_cpu.py and tests/test_gpu_streamlines.py.

Every case is four analytic arrays -- v_x, v_y, v_z, obs, indexed [x, y, z] with the ghost layer, as the viewer holds them
(GUI/main_window.py:227-230), rounded to the handle's precision before anybody sees them -- and one parameter set.  The GPU
test loads them with Simulation.set (ghost layer included) and compares fs_streamlines bit for bit with
oracle/streamlines_ref.py run with the kernel's norm; the CPU test runs the restatement alone and shows that every case
reaches what its "reaches" entry claims and that no decision in it comes closer than 1e-9 to its threshold, so the
expected answer can be produced, and judged, on a machine without a GPU.

The base flow is v_x = 1 + 0.25 sin(y/3), v_y = 0.5 sin(x/3), v_z = 0.3 cos(y/2): no component is exactly zero on an
interior line, so a seed on the plane c = 1 leaves it instead of sliding along the wall test's threshold."""
import functools
import math

import numpy as np

from oracle import streamlines_ref as R

DEFAULTS = dict(density=30, proximity=2, max_length=100, step_size=0.2, threshold=0.1)      # GUI/config.py:18-23


def base_flow(shape):
    """float64, padded (W+2, H+2, D+2), ghost layer included"""
    x, y, z = np.meshgrid(*(np.arange(n + 2, dtype=np.float64) for n in shape), indexing="ij")
    return 1.0 + 0.25 * np.sin(y / 3.0), 0.5 * np.sin(x / 3.0), 0.3 * np.cos(y / 2.0) + 0.0 * z


def ball(shape, cx, cy, cz, r):
    x, y, z = np.meshgrid(*(np.arange(n + 2, dtype=np.float64) for n in shape), indexing="ij")
    m = ((x - cx) ** 2 + (y - cy) ** 2 + (z - cz) ** 2 <= r * r).astype(np.float64)
    m[0] = m[-1] = 0.0
    m[:, 0] = m[:, -1] = 0.0
    m[:, :, 0] = m[:, :, -1] = 0.0
    return m


def _ball_case(shape):
    return base_flow(shape) + (ball(shape, 14, 10, 9, 4.2),)


def _ragged(shape):
    return base_flow(shape) + (ball(shape, 8, 6, 5, 2.3),)


def _long_row(shape):
    obs = np.zeros(tuple(n + 2 for n in shape))
    obs[276:284, 3:5, 3:5] = 1.0                         # past x = 256
    return base_flow(shape) + (obs,)


def _wall(axis):
    """The flow runs into the high wall of `axis`: its normal component is a (c* - c) with c* = N + 0.9995, inside the
    clip zone N + 0.999 .. N + 1 of the interpolation, the other two components are constant.  A line closes in on c*
    from below; once above N + 0.999 it sees the velocity AT N + 0.999 (the clip), creeps on by about 4e-4 a step and
    leaves through the wall.  Bodies sit on the walls x = 1, y = H, z = D and in the far corner."""
    def make(shape):
        dims = tuple(n + 2 for n in shape)
        c = np.meshgrid(*(np.arange(n, dtype=np.float64) for n in dims), indexing="ij")
        v = [np.full(dims, 0.5), np.full(dims, 0.4), np.full(dims, 0.3)]
        v[axis] = 2.0 * ((shape[axis] + 0.9995) - c[axis])
        W, H, D = shape
        obs = np.zeros(dims)
        obs[1, 3:5, 3:5] = 1.0
        obs[10:12, H, 4:6] = 1.0
        obs[15:17, 5:7, D] = 1.0
        obs[W, H, D] = 1.0
        return v[0], v[1], v[2], obs
    return make


def _stagnant(shape):
    vx, vy, vz = base_flow(shape)
    for v in (vx, vy, vz):
        v[8:15, 4:10, 3:9] = 0.0                         # cells 8..14 x 4..9 x 3..8: exactly at rest
    obs = np.zeros_like(vx)
    obs[18:20, 5:7, 4:6] = 1.0
    return vx, vy, vz, obs


def _soft(shape):
    obs = np.zeros(tuple(n + 2 for n in shape))
    obs[12:15, 4:9, 3:8] = 0.4                           # downstream, a halo below the level: 0.4 -> 0.6 passes 0.5 half way
    obs[10:13, 5:8, 4:7] = 0.6                           # a shell above the level that is not 1: upstream, 0 -> 0.6 passes
    obs[11, 6, 5] = 1.0                                  # 0.5 after 5/6 of a cell, where a 0/1 mask would after 1/2
    obs[20, 10, 8] = 0.5                                 # exactly the level, far from the body: must not widen the box
    obs[7, 6, 5] = 0.5                                   # and one in the path of the lines that reach the body
    obs[14, 8, 7] = 0.5                                  # a corner of the halo
    return base_flow(shape) + (obs,)


def _ghosts(shape):
    """ghost faces, edges and corners hold values above every interior one; the largest sits in the corner (0, 0, 0),
    which no interpolation reads (a point has c >= 1): only np.max sees it"""
    out = []
    for k, v in enumerate(base_flow(shape)):
        x, y, z = np.meshgrid(*(np.arange(n) for n in v.shape), indexing="ij")
        edge = sum(((c == 0) | (c == n - 1)).astype(int) for c, n in zip((x, y, z), v.shape))
        big = np.array([0.0, 3.0, 5.0, 7.0])[edge] * (1.0 + 0.125 * k) + 0.01 * (x + 2 * y + 3 * z)
        out.append(np.where(edge > 0, big, v))
    out[1][0, 0, 0] = 11.5
    return tuple(out) + (ball(shape, 8, 5, 4, 1.6),)


def _param_grid(shape):
    return base_flow(shape) + (ball(shape, 9.0, 6.0, 5.0, 2.2),)


def _nonfinite(value):
    def make(shape):
        vx, vy, vz, obs = _param_grid(shape)
        vx[14, 7, 6] = value                             # downstream of the ball, inside the widened box's reach
        return vx, vy, vz, obs
    return make


def _unit(shape):
    obs = np.zeros(tuple(n + 2 for n in shape))
    obs[-1, -1, -1] = 1.0                                # the only "solid" is a ghost corner
    return base_flow(shape) + (obs,)


def _exact(shape):
    """v = (1, 0, 0) everywhere and a step of 0.25: every coordinate a line visits is a multiple of 0.25 computed without
    a rounding (u / speed = 1 / 1, x +- 0.25; y and z get +-0.0), so lines land EXACTLY on x = 1 (kept: 1 <= x) and on
    x = W + 1 (dropped: x < W + 1).  That is the one thing the margin rule of the table forbids, and the only thing that
    tells `<` from `<=` in the wall test; here there is no rounding for a margin to guard against."""
    dims = tuple(n + 2 for n in shape)
    obs = np.zeros(dims)
    obs[5, 5, 5] = 1.0
    return np.ones(dims), np.zeros(dims), np.zeros(dims), obs


def _case(name, shape, precision, make, reaches=(), **par):
    return dict(name=name, shape=shape, precision=precision, make=make, reaches=tuple(reaches), par=dict(DEFAULTS, **par))


P = (24, 12, 10)                                         # the grid of the parameter cases
WIDE = dict(proximity=1e4, threshold=0.0)                # every seed is a candidate, no line is dropped for its smoothness
CASES = [
    # the geometry of tests/test_gpu_edge.py: density 30 and 20, threshold 0 and one in a gap of the max_change values
    _case("ball-30", (40, 20, 18), "fp32", _ball_case, ("culled", "seed_in_solid", "solid", "steps", "kept"), threshold=0.0),
    _case("ball-30-gap", (40, 20, 18), "fp32", _ball_case, ("thr_dropped", "kept"), threshold=0.02),
    _case("ball-20", (40, 20, 18), "fp32", _ball_case, ("culled", "seed_in_solid", "solid", "kept"), density=20, threshold=0.0),
    _case("ball-20-gap", (40, 20, 18), "fp32", _ball_case, ("thr_dropped", "kept"), density=20, threshold=0.03275),
    _case("ragged-fp64", (17, 11, 9), "fp64", _ragged, ("culled", "seed_in_solid", "solid", "wall", "kept"),
          density=16, proximity=15, threshold=0.0),
    _case("long-row", (300, 7, 6), "fp32", _long_row, ("culled", "seed_in_solid", "solid", "wall", "kept"),
          density=16, proximity=33, threshold=0.0),
    _case("wall-x-fp32", P, "fp32", _wall(0), ("clip", "wall", "solid", "seed_in_solid", "kept"), density=6, **WIDE),
    _case("wall-y-fp32", P, "fp32", _wall(1), ("clip", "wall", "solid", "seed_in_solid", "kept"), density=6, **WIDE),
    _case("wall-z-fp32", P, "fp32", _wall(2), ("clip", "wall", "solid", "seed_in_solid", "kept"), density=6, **WIDE),
    _case("wall-x-fp64", P, "fp64", _wall(0), ("clip", "wall", "solid", "seed_in_solid", "kept"), density=6, **WIDE),
    _case("wall-y-fp64", P, "fp64", _wall(1), ("clip", "wall", "solid", "seed_in_solid", "kept"), density=6, **WIDE),
    _case("wall-z-fp64", P, "fp64", _wall(2), ("clip", "wall", "solid", "seed_in_solid", "kept"), density=6, **WIDE),
    _case("stagnant", P, "fp32", _stagnant, ("speed", "short", "len5", "len6", "kept"), density=22, max_length=7, proximity=45,
          threshold=0.0),
    _case("stagnant-long", P, "fp32", _stagnant, ("speed", "short", "kept"), density=8, **WIDE),
    _case("soft-mask", P, "fp32", _soft, ("culled", "seed_in_solid", "solid", "kept"), density=20, proximity=12, threshold=0.0),
    _case("ghosts", (16, 10, 8), "fp32", _ghosts, ("wall", "solid", "kept"), density=10, proximity=33, threshold=0.0),
    _case("inf-cell", P, "fp32", _nonfinite(np.inf), ("nonfinite", "kept"), density=10, proximity=43, threshold=0.0),
    _case("nan-cell", P, "fp32", _nonfinite(np.nan), ("nonfinite", "kept"), density=10, proximity=43, threshold=0.0),
    _case("unit-1x1x1", (1, 1, 1), "fp32", _unit, ("wall", "kept"), density=3, proximity=15, step_size=0.07, threshold=0.0),
    _case("unit-2x1x1", (2, 1, 1), "fp64", _unit, ("wall", "kept"), density=5, proximity=25, step_size=0.07, threshold=0.0),
    _case("density-0", P, "fp32", _param_grid, (), density=0, **WIDE),
    _case("density-1", P, "fp32", _param_grid, (), density=1, **WIDE),
    _case("density-2", P, "fp32", _param_grid, ("kept",), density=2, **WIDE),
    _case("density-3", P, "fp32", _param_grid, ("kept",), density=3, **WIDE),
    _case("density-7", P, "fp32", _param_grid, ("kept", "solid"), density=7, **WIDE),
    _case("max-length-0", P, "fp32", _param_grid, ("short",), density=7, max_length=0, **WIDE),
    _case("max-length-1", P, "fp32", _param_grid, ("short",), density=7, max_length=1, **WIDE),
    _case("max-length-2", P, "fp32", _param_grid, ("short",), density=7, max_length=2, **WIDE),
    _case("max-length-3", P, "fp32", _param_grid, ("short",), density=7, max_length=3, **WIDE),
    _case("max-length-11", P, "fp32", _param_grid, ("kept", "steps"), density=7, max_length=11, **WIDE),
    _case("step-negative", P, "fp32", _param_grid, ("kept", "solid"), density=14, step_size=-0.2, proximity=13, threshold=0.0),
    # every point is the seed, max_change is exactly 0: a threshold of 0 would sit on it
    _case("step-zero", P, "fp32", _param_grid, ("kept", "steps"), density=14, step_size=0.0, proximity=13, threshold=-1.0),
    _case("step-huge", P, "fp32", _param_grid, ("wall", "short"), density=14, step_size=1e3, proximity=13, threshold=0.0),
    _case("proximity-inverted", P, "fp32", _param_grid, ("culled",), density=14, proximity=-50, threshold=0.0),
    _case("proximity-0", P, "fp32", _param_grid, ("culled", "kept"), density=23, proximity=0, threshold=0.0),
    _case("proximity-all", P, "fp32", _param_grid, ("kept",), density=8, proximity=1e4, threshold=0.0),
]
# outside the table and its margin rule, see _exact
EXACT = _case("exact-walls", (8, 8, 8), "fp32", _exact, ("wall", "kept"), density=8, proximity=1e4, step_size=0.25, threshold=-1.0)
BY_NAME = {c["name"]: c for c in CASES + [EXACT]}
NAMES = [c["name"] for c in CASES]

# The cases that must yield no line, and why no input could make them: no seeds (density 0: no x seed; density 1: 1 // 2 = 0
# y and z seeds), a joined line of at most 2 * (max_length // 2) + 1 <= 3 points where more than 5 are asked for, a first
# step of 1000 cells that leaves any grid, and a box whose faces have changed sides.
YIELD_NONE = ("density-0", "density-1", "max-length-0", "max-length-1", "max-length-2", "max-length-3", "step-huge",
              "proximity-inverted")


@functools.lru_cache(maxsize=None)
def fields(name):
    """(vx, vy, vz, obs) of the case, indexed [x, y, z], in the handle's precision; read-only"""
    case = BY_NAME[name]
    dtype = np.float64 if case["precision"] == "fp64" else np.float32
    out = tuple(np.ascontiguousarray(a, dtype=dtype) for a in case["make"](case["shape"]))
    for a in out:
        assert a.shape == tuple(n + 2 for n in case["shape"])
        a.setflags(write=False)
    return out


def as_stored(a):
    """[x, y, z] -> the (D+2, H+2, W+2) C-order array Simulation.set takes"""
    return np.ascontiguousarray(np.transpose(a, (2, 1, 0)))


@functools.lru_cache(maxsize=None)
def expected(name, kernel_order=True):
    """The restatement's answer: (lines, colour arguments, records), records = one (seed, margin, info) per seed.
    kernel_order=False runs it with numpy's own norm."""
    case = BY_NAME[name]
    records = []
    with np.errstate(all="ignore"):
        lines, norms = R.generate_streamlines(*fields(name), norm=R.kernel_norm if kernel_order else None,
                                              trace=lambda seed, margin, info: records.append((seed, margin, info)),
                                              **case["par"])
    return lines, norms, records


def reached(records):
    """the tags (the vocabulary of the "reaches" entries) that the records of one case show"""
    tags = set()
    for _, _, info in records:
        fate = info["fate"]
        tags.add({"solid": "seed_in_solid", "threshold": "thr_dropped"}.get(fate, fate))
        for why in info.get("ends", ()):
            tags.add(why)
        # two accepted points in the clip zone before the wall: the velocity read through the clip placed the second
        if any(n >= 2 and why == "wall" for n, why in zip(info.get("clipped", ()), info.get("ends", ()))):
            tags.add("clip")
        if info.get("points") in (5, 6):
            tags.add("len%d" % info["points"])
    return tags


def smallest_margin(records):
    return min([m for _, m, _ in records], default=math.inf)
