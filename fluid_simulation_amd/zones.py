"""Rows for Simulation.set_zones (include/fluidsim.h, "momentum zones"): every constructor returns one row of ZONE_PARAMS = 20
numbers -- shape, axis, the box x0 x1 y0 y1 z0 z1, the cylinder's centre (two numbers) and radius, g (3), D (3), F (3) -- as a
float64 array; sponge() returns several rows.  Host-side arithmetic only: nothing here touches the library.

A cell in a zone is updated per pass as u' = (u + dt * g) / (1 + dt * (D + F * |u|)), per axis: g is an acceleration, D a rate
(per unit time) and F a resistance per unit length, in the units of INTEGRATION.md section 6, where a cell is h = 1 / cbrt(w *
h * d) long.  Boxes, centres and radii are in cells; the constructors that turn a coefficient into F take the grid for h."""
import numpy as np

from ._lib import ZONE_PARAMS

BOX, CYLINDER = 0, 1


def _three(v):
    a = np.asarray(v, dtype=np.float64)
    return np.full(3, float(a)) if a.ndim == 0 else a.reshape(3)


def cell_size(grid):
    """h = 1 / cbrt(w * h * d), the cell size of the force and heat conversions."""
    w, h, d = grid
    return 1.0 / np.cbrt(float(w) * float(h) * float(d))


def zone(shape, axis, box, centre=(0.0, 0.0), radius=0.0, g=0.0, D=0.0, F=0.0):
    """One row from its parts; g, D and F are a number (all three axes) or three."""
    row = np.zeros(ZONE_PARAMS, dtype=np.float64)
    row[0], row[1] = shape, axis
    row[2:8] = box
    row[8:10] = centre
    row[10] = radius
    row[11:14], row[14:17], row[17:20] = _three(g), _three(D), _three(F)
    return row


def porous_box(box, D=0.0, F=0.0):
    """A porous block (a radiator, a grille, a screen): linear resistance D and quadratic resistance F inside `box` = (x0, x1,
    y0, y1, z0, z1); each a number or one per axis."""
    return zone(BOX, 0, box, D=D, F=F)


def fan(box, g, axis=None):
    """A fan: the acceleration `g` (three numbers, or one along `axis`) inside `box`.  The flux column of its budget is taken
    along `axis`, by default the axis of g's largest component."""
    a = np.asarray(g, dtype=np.float64)
    if a.ndim == 0:
        axis = 0 if axis is None else axis
        vec = np.zeros(3)
        vec[axis] = float(a)
    else:
        vec = a.reshape(3)
        axis = int(np.argmax(np.abs(vec))) if axis is None else axis
    return zone(BOX, axis, box, g=vec)


def actuator_disk(axis, centre, radius, cells_thick, ct_local, *, grid):
    """A rotor as an actuator disk: a cylinder along `axis` around `centre` = (cx, cy, cz) in cell coordinates, `cells_thick`
    cells long starting at the cell round(centre[axis]), that takes the thrust 0.5 * ct_local * u_d^2 per unit area and density
    out of the flow, u_d the velocity at the disk (ct_local is C_T' = C_T / (1 - a)^2 of momentum theory).  Spread over the
    disk's length L = cells_thick * h that is the quadratic resistance F = 0.5 * ct_local / L on the axis.  `grid` = (w, h, d)
    gives h and clips the bounding box."""
    ext = [int(n) for n in grid]
    c = [float(v) for v in centre]
    box = [0] * 6
    for a in range(3):
        if a == axis:
            lo = int(round(c[a]))
            hi = lo + int(cells_thick) - 1
        else:
            lo, hi = int(np.floor(c[a] - radius)), int(np.ceil(c[a] + radius))
        box[2 * a], box[2 * a + 1] = max(1, lo), min(ext[a], hi)
    others = [a for a in range(3) if a != axis]
    F = np.zeros(3)
    F[axis] = 0.5 * float(ct_local) / (float(cells_thick) * cell_size(grid))
    return zone(CYLINDER, axis, box, centre=(c[others[0]], c[others[1]]), radius=radius, F=F)


def straightener(box, axis, strength):
    """A flow straightener (a honeycomb): the linear resistance `strength` on the two axes across `axis`, none along it."""
    D = np.full(3, float(strength))
    D[axis] = 0.0
    return zone(BOX, axis, box, D=D)


def sponge(x0, x1, strength, layers, *, grid):
    """A sponge in front of the outlet: `layers` slabs across the whole section that split the planes x0..x1 evenly, the linear
    resistance on all three axes ramped quadratically from strength / layers^2 in the first to `strength` in the last, so that
    a wake fades out instead of reflecting off the outlet's copied ghost face.  Returns the rows, (layers, ZONE_PARAMS)."""
    w, h, d = (int(n) for n in grid)
    n = x1 - x0 + 1
    if layers < 1 or layers > n:
        raise ValueError("a sponge of %d planes takes 1 .. %d layers" % (n, n))
    edges = [x0 + (n * k) // layers for k in range(layers + 1)]
    rows = [zone(BOX, 0, (edges[k], edges[k + 1] - 1, 1, h, 1, d), D=float(strength) * ((k + 1) / layers) ** 2) for k in range(layers)]
    return np.array(rows)
