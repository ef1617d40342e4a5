"""The iso-surface cases shared by tests/test_surface_cases_cpu.py and tests/test_gpu_surface_cases.py.

A case is a padded (z, y, x) array already rounded to the handle's precision, a level given as a Python float (the
library rounds it to the handle's precision), the source it is loaded into (a field such as "DENS", or "OBS") and what
it is there for ("reaches").  The GPU test loads the array with Simulation.set, ghost layer included, and compares
fs_isosurface (for OBS also fs_obstacle_surface) byte for byte, order included, with tests/surface_model.py; the CPU
test runs the model alone and counts what every "reaches" entry claims, so that the expected answer can be produced,
and judged, on a machine without a GPU.  Every array is seeded; the largest has 602 x 5 x 4 points.

The "reaches" entries (tests/test_surface_cases_cpu.py holds one counting function for each):
  closed / open / empty   the mesh closes up; has edges on the padded box's faces; has no vertex and no triangle
  x-chunks                crossings and triangles in each of the three 256-point chunks of a row, and on the edges
                          255-256, 256-257, 511-512, W-(W+1) with the y and z edges at those x (the running offset the
                          vertex and triangle kernels carry from chunk to chunk)
  row-chunks              vertices and triangles in rows of each of the three 256-row chunks of the row scan, in the
                          first and in the last row
  ties                    end points equal to the level (outside: t = 0) and vertices sharing a position
  level-rounding          cells equal to float32(level) that a comparison in double would call inside
  nonfinite               every pairing NaN|inside, -Inf|inside, +Inf|outside, +Inf|-Inf, +Inf|NaN on crossing edges
  overflow                edges on which L - v0 and v1 - v0 both overflow, and edges with t = 0 from one overflow
  subnormal               crossing edges with a subnormal end point or a subnormal difference
  signed-zero             crossing edges with a +0.0 and with a -0.0 end point
  mask                    a 0/1 array: every t is 0.5
  x-chunks-mask           vertices and triangles in each of the three 256-point chunks of a row and in the cubes at
                          x = 255, 256, 511, 512"""
import collections
import functools

import numpy as np

Case = collections.namedtuple("Case", "name shape precision array level source reaches")

DTYPES = {"fp32": np.float32, "fp64": np.float64}
SUB32 = float(np.float32(1.0e-45))                        # the smallest fp32 subnormal, 2^-149


def _padded(shape):
    W, H, D = shape
    return (D + 2, H + 2, W + 2)


def _noise(shape, seed):
    return np.random.default_rng(seed).random(_padded(shape))


def _clear_ghost(a, value=0.0):
    a[0] = a[-1] = value
    a[:, 0] = a[:, -1] = value
    a[:, :, 0] = a[:, :, -1] = value
    return a


def _long_row(shape, seed):
    """Noise to the boundary; at x = 255, 256, 257, 511, 512, W, W + 1 a checkerboard in (x + y + z) of values below
    and above 0.5, so that every x, y and z edge at those x crosses."""
    W = shape[0]
    a = _noise(shape, seed)
    z, y, x = np.indices(a.shape)
    for xs in (255, 256, 257, 511, 512, W, W + 1):
        high = ((xs + y[:, :, xs] + z[:, :, xs]) & 1) == 1
        a[:, :, xs] = 0.4 * a[:, :, xs] + np.where(high, 0.55, 0.05)
    return a


def _ties(shape, seed):
    return np.floor(5.0 * _noise(shape, seed)) / 4.0      # 0, 1/4, 1/2, 3/4, 1


def _level_rounding(shape, seed):
    rng = np.random.default_rng(seed)
    a = (0.2 * rng.random(_padded(shape))).astype(np.float32)
    a[rng.random(a.shape) < 0.3] = np.float32(0.1)        # > 0.1 as a double, == L once L is rounded to fp32
    return a


def _nonfinite(shape, seed):
    rng = np.random.default_rng(seed)
    a = _clear_ghost(rng.random(_padded(shape)))
    kind = rng.random(a.shape)
    interior = _clear_ghost(np.ones(a.shape, dtype=bool), False)
    for lo, value in ((0.0, np.nan), (0.027, np.inf), (0.054, -np.inf)):
        a[interior & (kind >= lo) & (kind < lo + 0.027)] = value
    return a


def _overflow(shape, seed):
    rng = np.random.default_rng(seed)
    values = np.array([-3.0e38, -1.0e38, 1.0e38, 2.5e38, 3.0e38])
    return values[rng.integers(0, len(values), _padded(shape))]


def _subnormal(shape, seed):
    rng = np.random.default_rng(seed)
    values = np.array([0.0, SUB32, 2 * SUB32, 3 * SUB32, -SUB32, -2 * SUB32, 1.2e-38, 2.4e-38, -1.2e-38], dtype=np.float32)
    return values[rng.integers(0, len(values), _padded(shape))]


def _signed_zero(shape, seed):
    rng = np.random.default_rng(seed)
    values = np.array([0.0, -0.0, 1.0e-3, -1.0e-3, 0.75, -0.5])
    return values[rng.integers(0, len(values), _padded(shape))]


def _random_mask(shape, seed):
    return (_noise(shape, seed) < 0.3).astype(np.float64)


def _bodies_mask(shape, seed):
    """the mask of tests/test_surface.py::test_touching_and_separate_bodies_and_cells_on_the_walls"""
    W, H, D = shape
    m = np.zeros(_padded(shape))
    m[2:5, 3:6, 4:9] = 1.0                                # a box
    m[7, 7, 7] = m[8, 8, 7] = 1.0                         # edge contact
    m[7, 10, 12] = m[8, 11, 13] = 1.0                     # corner contact
    m[1, 1, 1] = m[D, H, W] = 1.0                         # domain corners
    m[5:8, 1, 14:17] = 1.0                                # slab on the y = 1 wall
    return m


def _long_row_mask(shape, seed):
    """bodies before x = 256, across 256, between, across 512 and up to the last interior cell"""
    W, H, D = shape
    m = np.zeros(_padded(shape))
    m[1, 1, 100:104] = 1.0
    m[1:D + 1, 2:H + 1, 250:262] = 1.0
    m[1:D + 1, 1:3, 300:310] = 1.0
    m[1:D + 1, 1:3, 508:516] = 1.0
    m[D, H, 511:513] = 1.0
    m[1:D + 1, 1:H + 1, W - 3:W + 1] = 1.0
    return m


@functools.lru_cache(maxsize=None)
def cases():
    out = []

    def add(name, shape, make, seed, level, reaches, source="DENS", precisions=("fp32", "fp64")):
        for p in precisions:
            a = np.ascontiguousarray(make(shape, seed).astype(DTYPES[p]))
            a.setflags(write=False)
            out.append(Case("%s %s" % (name, p), shape, p, a, level, source, tuple(reaches)))

    add("noise interior", (16, 12, 10), lambda s, seed: _clear_ghost(_noise(s, seed)), 11, 0.5, ["closed"])
    add("noise to the boundary", (16, 12, 10), _noise, 12, 0.5, ["open"])
    add("noise to the boundary, second seed", (16, 12, 10), _noise, 13, 0.5, ["open"], precisions=("fp32",))
    add("long row", (600, 3, 2), _long_row, 14, 0.5, ["open", "x-chunks"])
    add("many rows", (5, 30, 20), _noise, 53, 0.5, ["open", "row-chunks"])
    add("smallest grid", (1, 1, 1), _noise, 16, 0.5, ["open"])
    add("ties", (12, 9, 7), _ties, 17, 0.5, ["open", "ties"])
    add("level rounding", (12, 9, 7), _level_rounding, 18, 0.1, ["open", "level-rounding"], precisions=("fp32",))
    add("non-finite", (16, 12, 10), _nonfinite, 19, 0.5, ["closed", "nonfinite"])
    add("overflow at 2e38", (12, 9, 7), _overflow, 20, 2.0e38, ["open", "overflow"], precisions=("fp32",))
    add("overflow at 0", (12, 9, 7), _overflow, 20, 0.0, ["open", "overflow"], precisions=("fp32",))
    add("subnormal at 0", (12, 9, 7), _subnormal, 21, 0.0, ["open", "subnormal"], precisions=("fp32",))
    add("subnormal at the smallest subnormal", (12, 9, 7), _subnormal, 21, SUB32, ["open", "subnormal"], precisions=("fp32",))
    for name, level in (("above everything", 2.0), ("below everything", -1.0), ("+Inf", float("inf")),
                        ("-Inf", float("-inf")), ("NaN", float("nan"))):
        add("empty: level " + name, (6, 5, 4), _noise, 22, level, ["empty"])
    add("signed zero at +0.0", (12, 9, 7), _signed_zero, 23, 0.0, ["open", "signed-zero"])
    add("signed zero at -0.0", (12, 9, 7), _signed_zero, 23, -0.0, ["open", "signed-zero"])
    add("random mask", (16, 12, 10), _random_mask, 24, 0.5, ["open", "mask"], source="OBS")
    add("touching bodies mask", (20, 16, 12), _bodies_mask, 0, 0.5, ["closed", "mask"], source="OBS")
    add("long row mask", (600, 3, 2), _long_row_mask, 0, 0.5, ["closed", "mask", "x-chunks-mask"], source="OBS")
    return tuple(out)


def by_name(name):
    for c in cases():
        if c.name == name:
            return c
    raise KeyError(name)


def ids():
    return [c.name for c in cases()]
