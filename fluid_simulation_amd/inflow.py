"""Host-side helpers for the inflow generator (Simulation.set_inflow; include/fluidsim.h, "turbulent inflow"): mean-velocity
and fluctuation-scale maps of the inlet plane as numpy arrays of shape (depth, height), the layout set_inflow takes.  The
device only reads such tables, so no power or logarithm enters the library's arithmetic.

The wall is the face below cell 1 of `axis` ("y": the floor, "z": the side wall), and the centre of cell i lies i - 1/2
cells above it."""
import numpy as np


def _heights(h, d, axis):
    if axis not in ("y", "z"):
        raise ValueError("axis: 'y' or 'z'")
    y = np.arange(1, int(h) + 1, dtype=np.float64) - 0.5
    z = np.arange(1, int(d) + 1, dtype=np.float64) - 0.5
    return np.broadcast_to(y[None, :] if axis == "y" else z[:, None], (int(d), int(h)))


def power_law(h, d, speed, alpha, ref_height, axis="y"):
    """U = speed * (height / ref_height) ** alpha: the power-law boundary layer (alpha about 1/7 over open terrain), `speed`
    the velocity at `ref_height` cells above the wall."""
    if not ref_height > 0:
        raise ValueError("ref_height must be positive")
    return np.ascontiguousarray(float(speed) * (_heights(h, d, axis) / float(ref_height)) ** float(alpha))


def log_law(h, d, speed, roughness, ref_height, axis="y"):
    """U = speed * ln(height / z0) / ln(ref_height / z0), 0 below the roughness length z0 = `roughness` (cells): the
    logarithmic boundary layer with `speed` at `ref_height` cells above the wall."""
    if not (roughness > 0 and ref_height > roughness):
        raise ValueError("need 0 < roughness < ref_height")
    y = _heights(h, d, axis)
    u = float(speed) * np.log(np.maximum(y, float(roughness)) / float(roughness)) / np.log(float(ref_height) / float(roughness))
    return np.ascontiguousarray(u)


def intensity_profile(h, d, intensity, ref_height, decay=0.0, axis="y", mean=None):
    """The fluctuation scale r for a turbulence intensity that falls off with height: r = intensity * (height / ref_height)
    ** (-decay), times the mean map `mean` where one is given (so that u_rms = 1 makes `intensity` the ratio of the
    fluctuation's standard deviation to the local mean), else times 1."""
    if not ref_height > 0:
        raise ValueError("ref_height must be positive")
    r = float(intensity) * (_heights(h, d, axis) / float(ref_height)) ** (-float(decay))
    if mean is not None:
        r = r * np.asarray(mean, dtype=np.float64).reshape(int(d), int(h))
    return np.ascontiguousarray(r)
