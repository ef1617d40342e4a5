"""Viewer-side helper: the streamlines of the reference's GUI, computed on the GPU.

`generate_streamlines` takes what GUI/utils.py:118 `generate_streamlines` takes -- the last frame's
`v_x, v_y, v_z, obs` arrays including padding, transposed to (x, y, z) as GUI/main_window.py:227-230
does -- and returns the same `(streamlines, streamline_colors)` pair, so a maintainer of the viewer
swaps one call:

    # streamlines, colors = utils.generate_streamlines(vx=vx, vy=vy, vz=vz, obs_data=obs)
    from fluid_simulation_amd.viewer import generate_streamlines
    streamlines, colors = generate_streamlines(vx, vy, vz, obs, cmap=config.density_cmap)

The parameters default to GUI/config.py:18-23.  Without `cmap` the second value is the list of
numbers the reference passes to its colour map (utils.py:202-205)."""
import numpy as np

from . import _lib
from .simulation import Simulation

_handles = {}


def generate_streamlines(vx, vy, vz, obs_data, max_length=100, density=30, proximity=2, step_size=0.2,
                         vel_change_threshold=0.1, cmap=None):
    shape = tuple(int(n) - 2 for n in vx.shape)          # (W, H, D): the arrays carry the padding
    if min(shape) < 1 or vy.shape != vx.shape or vz.shape != vx.shape or obs_data.shape != vx.shape:
        raise ValueError("expected four padded arrays of one shape (W+2, H+2, D+2)")
    sim = _handles.get(shape)
    if sim is None:
        sim = _handles[shape] = Simulation(shape[0], shape[1], shape[2], 1, quiet=1, dump_every=0)
    back = (2, 1, 0)                                     # the library's arrays are (z, y, x), like the dump files
    sim.set(_lib.VX, np.ascontiguousarray(np.transpose(vx, back), dtype=np.float32))
    sim.set(_lib.VY, np.ascontiguousarray(np.transpose(vy, back), dtype=np.float32))
    sim.set(_lib.VZ, np.ascontiguousarray(np.transpose(vz, back), dtype=np.float32))
    # the array itself, not a mask of it: the reference interpolates what it was given (utils.py:110)
    sim.set(_lib.OBS, np.ascontiguousarray(np.transpose(obs_data, back), dtype=np.float32))
    lines, norm = sim.streamlines(density=density, proximity=proximity, max_length=max_length, step_size=step_size,
                                  vel_change_threshold=vel_change_threshold)
    if cmap is None:
        return lines, list(norm)
    return lines, [np.array(cmap(float(v))) for v in norm]


def generate_obstacle_mesh(obs_data):
    """GUI/utils.py:10 `generate_obstacle_mesh` on the GPU: takes the padded obstacle array transposed to
    (x, y, z) as GUI/main_window.py:204 passes it and returns the same dictionary ('vertexes', 'faces',
    'vertex_colors' -- solid gray, utils.py:19-24; three empty arrays when there is no obstacle).  The mesh is
    the 0.5 iso-surface like scikit-image's, but vertex / face order and the cut of ambiguous cubes are this
    library's (parity unpinned: scikit-image is not available to compare with)."""
    shape = tuple(int(n) - 2 for n in obs_data.shape)
    if len(shape) != 3 or min(shape) < 1:
        raise ValueError("expected the padded obstacle array (W+2, H+2, D+2)")
    sim = _handles.get(shape)
    if sim is None:
        sim = _handles[shape] = Simulation(shape[0], shape[1], shape[2], 1, quiet=1, dump_every=0)
    sim.set(_lib.OBS, np.ascontiguousarray(np.transpose(obs_data, (2, 1, 0)), dtype=np.float32))
    return _mesh_dict(*sim.obstacle_surface())


def _mesh_dict(verts, faces):
    if verts.shape[0] == 0:
        return {"vertexes": np.array([]), "faces": np.array([]), "vertex_colors": np.array([])}
    colors = np.ones((verts.shape[0], 4))
    colors[:, :3] = 0.5
    return {"vertexes": verts.astype(np.float64), "faces": faces, "vertex_colors": colors}


def generate_isosurface_mesh(sim, source, level):
    """The iso-surface {source > level} of a live `Simulation` as the dictionary generate_obstacle_mesh returns
    ('vertexes', 'faces', 'vertex_colors'): `source` is a field selector or ISO_VORTEX | VORTEX_* (for example
    ISO_VORTEX | VORTEX_Q at a positive level: the vortex cores).  The mesh never leaves the device's index space:
    padded (x, y, z) coordinates, as the obstacle mesh."""
    return _mesh_dict(*sim.isosurface(source, level))


def rake(p0, p1, n):
    """`n` points on the segment from p0 to p1, end points included, as an (n, 3) float64 array for
    `Simulation.sample_points`: a wake rake, or one row of a cut plane."""
    p0 = np.asarray(p0, dtype=np.float64).reshape(3)
    p1 = np.asarray(p1, dtype=np.float64).reshape(3)
    t = np.linspace(0.0, 1.0, int(n)).reshape(-1, 1) if int(n) > 1 else np.zeros((int(n), 1))
    return p0 + t * (p1 - p0)


def surface_pressure(sim, source=_lib.PRESSURE, p_ref=0.0):
    """The pressure distribution on the body of a live `Simulation`: the obstacle mesh (generate_obstacle_mesh's
    dictionary) plus 'p', `source` at every vertex in mode "fluid" -- a vertex sits on the edge between a solid and a
    fluid cell, and the solid cell holds 0 -- and 'cp' = 2 (p - p_ref) / (dt * speed^2), the scaling of the force
    coefficients (include/fluidsim.h, "pressure force on the obstacles").  Replaces the handle's sample points."""
    verts, faces = sim.obstacle_surface()
    mesh = _mesh_dict(verts, faces)
    sim.sample_points(verts.astype(np.float64))
    p = sim.sample(source, "fluid")
    denom = float(sim.dt) * (float(sim.speed) * float(sim.speed))
    with np.errstate(divide="ignore", invalid="ignore"):
        mesh["p"] = p
        mesh["cp"] = 2.0 * (p - float(p_ref)) / denom
    return mesh


def streaklines(sim):
    """The streaklines of a live `Simulation` with emitters (tracer_emitters): one (m, 3) float64 polyline per emitter,
    that emitter's ALIVE particles ordered by `born`, newest first -- the curve smoke from a nozzle draws, starting at the
    nozzle.  Particles released in the same step keep their slot order.  Host-side grouping of Simulation.tracers()."""
    t = sim.tracers()
    n = sim._geti("tracer_emitters")
    alive = t["status"] == _lib.TRACER_ALIVE
    lines = []
    for e in range(n):
        idx = np.flatnonzero(alive & (t["source"] == e))
        idx = idx[np.argsort(-t["born"][idx].astype(np.int64), kind="stable")]
        lines.append(t["xyz"][idx].copy())
    return lines


def pathlines(log):
    """The pathlines in a snapshot log (Simulation.tracer_log()): for each slot the list of (m, 3) float64 polylines it
    drew, cut wherever the slot was not ALIVE in a frame -- a slot that was overwritten while ALIVE in consecutive frames
    is not told apart here; keep the pool larger than the particles of a run.  Host-side grouping."""
    alive = log["status"] == _lib.TRACER_ALIVE           # (F, C)
    frames, slots = alive.shape if alive.ndim == 2 else (0, 0)
    out = []
    for s in range(slots):
        runs, start = [], None
        for f in range(frames + 1):
            on = f < frames and alive[f, s]
            if on and start is None:
                start = f
            elif not on and start is not None:
                runs.append(log["xyz"][start:f, s].copy())
                start = None
        out.append(runs)
    return out


# the 2-D viewer's colour ranges (gui.py:271-289) and the strength of its obstacle overlay (gui.py:295)
SLICE_RANGES = {"density": (_lib.DENS, 0.0, 0.01), "v_x": (_lib.VX, -10.0, 10.0), "v_y": (_lib.VY, -1.0, 1.0),
                "v_z": (_lib.VZ, -1.0, 1.0)}
SLICE_ALPHA = 0.2


def slice_image(sim, field="density", z=None):
    """The frame the reference's 2-D viewer shows (gui.py:257-295) of a live `Simulation`, rendered on the device: one
    z-slice of `field` ("density", "v_x", "v_y" or "v_z") through the viewer's colour map and ranges, obstacle cells
    darkened; (H+2, W+2, 3) uint8.  The default slice is the middle one, (D+2)//2."""
    source, vmin, vmax = SLICE_RANGES[field]
    if z is None:
        z = (sim.depth + 2) // 2
    return sim.image_rgb(source, "slice", 2, int(z), vmin=vmin, vmax=vmax, obstacle_alpha=SLICE_ALPHA)


# the 3-D viewer's camera (GUI/gl_widget.py:26-28: distance, azimuth, elevation; :64: a 45 degree field of view), its clear
# colour (:58, 0.1) and the gray of its obstacle mesh (GUI/utils.py:19-24, 0.5) as bytes
VOLUME_CAMERA = {"azimuth": 45.0, "elevation": 30.0, "distance": 200.0, "fov_deg": 45.0}
VOLUME_BACKGROUND = (26, 26, 26)
VOLUME_OBSTACLE = (128, 128, 128)


def orbit_eye(centre, azimuth, elevation, distance):
    """Where the 3-D viewer's camera stands (GUI/gl_widget.py:71-74: a translation by -distance along z, then rotations by
    the elevation about x and the azimuth about y, angles in degrees), orbiting `centre` instead of the origin; y is up."""
    az, el = np.deg2rad(np.float64(azimuth)), np.deg2rad(np.float64(elevation))
    d = np.float64(distance)
    off = np.array([-d * np.cos(el) * np.sin(az), d * np.sin(el), d * np.cos(el) * np.cos(az)], dtype=np.float64)
    return np.asarray(centre, dtype=np.float64).reshape(3) + off


def volume_image(sim, field="density", azimuth=45.0, elevation=30.0, distance=200.0, size=(512, 512), slot=0, fov_deg=45.0,
                 source=None, vmin=None, vmax=None, opacity=0.05, step=0.5, t_min=0.01, obstacle=VOLUME_OBSTACLE,
                 background=VOLUME_BACKGROUND):
    """A ray-marched 3-D view of a live `Simulation`, rendered on the device: `field` ("density", "v_x", "v_y", "v_z": the
    2-D viewer's colour ranges) or any `source` of sample() with vmin / vmax, seen by the reference GUI's camera (its
    orbit and defaults, GUI/gl_widget.py:26-28 and 64-76) looking at the centre of the box; obstacles are shaded gray
    surfaces.  `size` is (cols, rows); returns (rows, cols, 3) uint8.  Replaces the rays of camera slot `slot`."""
    src, lo, hi = SLICE_RANGES[field] if source is None else (int(source), 0.0, 1.0)
    lo = lo if vmin is None else vmin
    hi = hi if vmax is None else vmax
    centre = np.array([sim.width + 1, sim.height + 1, sim.depth + 1], dtype=np.float64) * 0.5
    sim.volume_camera(slot, orbit_eye(centre, azimuth, elevation, distance), centre, (0.0, 1.0, 0.0), fov_deg=fov_deg, size=size)
    return sim.volume_render(src, slot, vmin=lo, vmax=hi, opacity=opacity, step=step, t_min=t_min, obstacle=obstacle,
                             background=background)


def write_png(path, rgb):
    """Writes an (rows, cols, 3) uint8 image as an uncompressed 8-bit RGB PNG (fs_image_png; needs no GPU)."""
    import ctypes as C
    import os
    a = np.ascontiguousarray(rgb, dtype=np.uint8)
    if a.ndim != 3 or a.shape[2] != 3:
        raise ValueError("expected an (rows, cols, 3) image")
    _lib.check(_lib.lib().fs_image_png(a.ctypes.data_as(C.c_void_p), a.shape[1], a.shape[0], os.fsencode(path)))
