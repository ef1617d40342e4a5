"""Test infrastructure (only tests/ may import this): CPU restatement of the streamline code of
the reference's viewer, GUI/utils.py:40-213, with the parameters of GUI/config.py:18-23 passed in.

PARITY UNPINNED: the reference module itself cannot be imported in this image -- it imports
scikit-image at module level (utils.py:6) and PyQt6 further up, neither of which is installed --
and the reference holds no fixtures for it.  The functions below follow the source statement by
statement (cited per function) with numpy scalars exactly where the reference has them, so that
float32 grid values meet float64 coordinates the same way; colours are left as the number the
reference feeds its colour map (utils.py:202-205), because that map lives in GUI/config.py.

Two optional hooks, both off by default (None leaves every result as it was):

`norm` replaces np.linalg.norm in the three places the source calls it (the speed of a step, the
velocity change of the threshold filter, the speeds of the colour).  numpy's norm of a 3-vector is
sqrt(dot(x, x)), and how dot associates and whether it fuses its three products is the business of
the BLAS numpy was built with; the device computes sqrt((u*u + v*v) + w*w) with every operation
rounded once.  The two differ in the last bit for some vectors, which moves a coordinate by a few
1e-15 and nothing else (measured in tests/test_streamlines_cases_cpu.py).  `kernel_norm` below is
the device's form; with it every operation of the restatement is the IEEE double operation the
kernel performs, in the same order, and the GPU tests compare bit patterns.

`trace` reports how far the decisions were from their thresholds, so that a test can show that no
comparison it relies on hangs on a rounding.  integrate_part calls trace(margin, reason, clipped)
once: the smallest of |speed - 1e-6|, the distances of pos[k] from 1 and from dims[k] - 1 and
|interp(obs) - 0.5| over its steps; why it ended ("steps", "speed", "nonfinite", "wall", "solid");
and how many of its accepted points lay in the clip zone of interpolate_scalar (a coordinate above
shape - 1.001).  generate_streamlines calls trace(seed, margin, info) once per seed: the smallest
margin of any decision taken for it -- the seed's distance from the faces of the widened box in
the cull, the two parts' margins, |max_change - threshold|, the distance of every tested point
from the faces of the box -- and info = {"fate": "culled" | "solid" | "short" | "threshold" | "far"
| "kept", "ends": (backward reason, forward reason), "clipped": (backward, forward) points in the clip zone,
"points": len(full), "max_change": ...} as far as the seed got.  Comparisons of a stored value
with 0.5 (the bounding box, the seed's cell) and of integers involve no arithmetic and have no
margin."""
import math

import numpy as np


def kernel_norm(v):
    """the device's norm of a 3-vector (csrc/streamlines.hip): every operation rounded once"""
    u, v, w = np.float64(v[0]), np.float64(v[1]), np.float64(v[2])
    with np.errstate(over="ignore", invalid="ignore"):
        return np.sqrt((u * u + v * v) + w * w)


def interpolate_scalar(grid, x, y, z):
    """utils.py:40-76"""
    x = np.clip(x, 0, grid.shape[0] - 1.001)
    y = np.clip(y, 0, grid.shape[1] - 1.001)
    z = np.clip(z, 0, grid.shape[2] - 1.001)
    x0, y0, z0 = int(x), int(y), int(z)
    x1, y1, z1 = x0 + 1, y0 + 1, z0 + 1
    xd, yd, zd = x - x0, y - y0, z - z0
    c000 = grid[x0, y0, z0]
    c100 = grid[x1, y0, z0]
    c010 = grid[x0, y1, z0]
    c110 = grid[x1, y1, z0]
    c001 = grid[x0, y0, z1]
    c101 = grid[x1, y0, z1]
    c011 = grid[x0, y1, z1]
    c111 = grid[x1, y1, z1]
    c00 = c000 * (1 - xd) + c100 * xd
    c01 = c001 * (1 - xd) + c101 * xd
    c10 = c010 * (1 - xd) + c110 * xd
    c11 = c011 * (1 - xd) + c111 * xd
    c0 = c00 * (1 - yd) + c10 * yd
    c1 = c01 * (1 - yd) + c11 * yd
    return c0 * (1 - zd) + c1 * zd


def interpolate_vector(vx, vy, vz, x, y, z):
    """utils.py:78-83"""
    return np.array([interpolate_scalar(vx, x, y, z), interpolate_scalar(vy, x, y, z), interpolate_scalar(vz, x, y, z)])


def _gap(a, b):
    """|a - b| as a margin: infinite where either side is not a number"""
    d = abs(float(a) - float(b))
    return math.inf if math.isnan(d) else d


def integrate_part(start_pos, vx, vy, vz, obs, max_steps, direction, step_size, dims, norm=None, trace=None):
    """utils.py:85-115 (_integrate_streamline_part); dims = (config.width, height, depth)"""
    norm = np.linalg.norm if norm is None else norm
    points = [start_pos]
    velocities = [interpolate_vector(vx, vy, vz, *start_pos)]
    pos = start_pos.copy()
    margin, reason, clipped = math.inf, "steps", 0
    for _ in range(max_steps):
        vec = interpolate_vector(vx, vy, vz, pos[0], pos[1], pos[2])
        speed = norm(vec)
        if trace is not None:
            margin = min(margin, _gap(speed, 1e-6))
        if speed < 1e-6:
            reason = "speed"
            break
        step = direction * (vec / speed) * step_size
        pos = pos + step
        if np.any(np.isnan(pos)) or np.any(np.isinf(pos)):
            reason = "nonfinite"
            break
        if trace is not None:
            margin = min([margin] + [_gap(pos[k], 1) for k in range(3)] + [_gap(pos[k], dims[k] - 1) for k in range(3)])
        if not (1 <= pos[0] < dims[0] - 1 and 1 <= pos[1] < dims[1] - 1 and 1 <= pos[2] < dims[2] - 1):
            reason = "wall"
            break
        solid = interpolate_scalar(obs, pos[0], pos[1], pos[2])
        if trace is not None:
            margin = min(margin, _gap(solid, 0.5))
        if solid > 0.5:
            reason = "solid"
            break
        if trace is not None and any(pos[k] > obs.shape[k] - 1.001 for k in range(3)):
            clipped += 1
        points.append(pos.copy())
        velocities.append(vec)
    if trace is not None:
        trace(margin, reason, clipped)
    return points, velocities


def _box_gap(pt, omin, omax):
    return min([_gap(pt[k], omin[k]) for k in range(3)] + [_gap(pt[k], omax[k]) for k in range(3)])


def generate_streamlines(vx, vy, vz, obs, density=30, proximity=2, max_length=100, step_size=0.2, threshold=0.1,
                         norm=None, trace=None):
    """utils.py:118-213.  Arrays are indexed [x, y, z] and include the padding, as main_window.py:227-231
    hands them over.  Returns (list of (n, 3) arrays, list of the colour-map arguments)."""
    norm_of = np.linalg.norm if norm is None else norm
    dims = vx.shape
    lines, norms = [], []
    idx = np.where(obs > 0.5)
    if len(idx[0]) == 0:
        return lines, norms
    omin = np.array([np.min(idx[0]), np.min(idx[1]), np.min(idx[2])]) - (proximity / 10)
    omax = np.array([np.max(idx[0]), np.max(idx[1]), np.max(idx[2])]) + (proximity / 10)
    x_seeds = np.linspace(1, dims[0] - 2, density)
    y_seeds = np.linspace(1, dims[1] - 2, density // 2)
    z_seeds = np.linspace(1, dims[2] - 2, density // 2)
    denom = np.max([vx, vy, vz]) + 1e-6
    for zs in z_seeds:
        for ys in y_seeds:
            for xs in x_seeds:
                start = np.array([xs, ys, zs])
                margin, info, parts = math.inf, {}, []
                if trace is not None:
                    margin = _box_gap(start, omin, omax)
                if (start[0] < omin[0] or start[0] > omax[0] or start[1] < omin[1] or start[1] > omax[1] or
                        start[2] < omin[2] or start[2] > omax[2]):
                    if trace is not None:
                        trace(start, margin, dict(fate="culled"))
                    continue
                if obs[int(xs), int(ys), int(zs)] > 0.5:
                    if trace is not None:
                        trace(start, margin, dict(fate="solid"))
                    continue
                part_trace = None if trace is None else (lambda m, why, clipped: parts.append((m, why, clipped)))
                bp, bv = integrate_part(start, vx, vy, vz, obs, max_length // 2, -1.0, step_size, dims, norm, part_trace)
                fp, fv = integrate_part(start, vx, vy, vz, obs, max_length // 2, 1.0, step_size, dims, norm, part_trace)
                full = bp[::-1][:-1] + fp
                fvel = bv[::-1][:-1] + fv
                if trace is not None:
                    margin = min(margin, parts[0][0], parts[1][0])
                    info = dict(ends=(parts[0][1], parts[1][1]), clipped=(parts[0][2], parts[1][2]), points=len(full))
                if len(full) <= 5:
                    if trace is not None:
                        trace(start, margin, dict(info, fate="short"))
                    continue
                max_change = 0.0
                for i in range(1, len(fvel)):
                    change = norm_of(fvel[i] - fvel[i - 1])
                    if change > max_change:
                        max_change = change
                if trace is not None:
                    margin = min(margin, _gap(max_change, threshold))
                    info["max_change"] = float(max_change)
                if max_change < threshold:
                    if trace is not None:
                        trace(start, margin, dict(info, fate="threshold"))
                    continue
                near = False
                for i in range(0, len(full), 3):
                    pt = full[i]
                    if trace is not None:
                        margin = min(margin, _box_gap(pt, omin, omax))
                    if omin[0] <= pt[0] <= omax[0] and omin[1] <= pt[1] <= omax[1] and omin[2] <= pt[2] <= omax[2]:
                        near = True
                        break
                if not near:
                    if trace is not None:
                        trace(start, margin, dict(info, fate="far"))
                    continue
                speeds = [norm_of(v) for v in fvel]
                max_speed = max(speeds) if speeds else 0.0
                norms.append(min(max_speed / denom, 1.0))
                lines.append(np.array(full))
                if trace is not None:
                    trace(start, margin, dict(info, fate="kept"))
    return lines, norms
