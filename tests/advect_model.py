"""Rough inputs for the semi-Lagrangian advection and a numpy classifier of its back-traces (numpy only).

The advection kernels of csrc/advect.hip come in several forms (option advect_kernels) that are claimed bit-identical;
which branch of a form a trace takes depends on where it ends: clamped to the inlet side (px == 0.5: the clamp tables, and
in the tile form the LDS window or the fallback to the global table), clamped to the outlet side (px == W + 0.5: side 1 of
the tables), not clamped in x (the gather from the big array), clamped in y or z (table rows 0 / H + 1, planes 0 / D + 1).
rough_fields() draws velocities under which every one of these classes holds a good share of the cells, classify() counts
them, and tile_window() restates the host function of the same name (the LDS cap on the window radius).  Nothing here
comes from the kernels' output: the tests compare fields with the CPU oracle and use this module only to prove that a
passing run has been through each branch.
"""
import numpy as np

DT = 0.05                # the default time step of Simulation / Oracle
TILE = 8                 # advect_tile_kernel: a workgroup owns TILE x TILE (y, z) rows
LDS_BYTES = 64 * 1024    # what tile_window() lets the staged windows take
FLOOR = 100              # cells every class must hold at every (grid, R) pair of FLOOR_R
SEED = 7

# (W, H, D) -> the window radii at which every class is held to FLOOR (the radii the tile form really runs at on that grid:
# advect_window = 1, 4, 24, 128 through tile_window() for one and for three staged tables, as far as traces still leave the
# window; beyond that the window covers the whole table and "lo_out" is empty by construction)
FLOOR_R = {(70, 33, 21): (1, 4, 24), (12, 80, 11): (1, 21, 24), (256, 9, 70): (1, 24, 32)}
TINY = (5, 3, 2)         # the tile is larger than the grid: exempt from the floor
WINDOWS = (1, 4, 24, 128)

CLASSES = ("lo_in", "lo_out", "hi", "mid", "mid_int", "ylo", "yhi", "zlo", "zhi", "lo_ylo", "hi_yhi", "lo_zhi", "hi_zlo")


def rough_fields(W, H, D, seed=SEED, dtype=np.float32, dt=DT):
    """ux, uy, uz, src: full padded (D+2, H+2, W+2) arrays in `dtype`.  Drawn in fp64 and rounded, so both precisions get
    the same flow.  ux per cell, equal odds: +2/dt (the trace clamps low), -2/dt (clamps high), normal * 3 / (dt W) (a few
    cells of travel), exactly 0 (px integral, tx == 0).  uy, equal odds: normal * 1.5 / (dt H) (stays near) or normal /
    (2 dt) (about H / 2 rows: clamps at both y walls and leaves windows); uz the same with D.  src is standard normal.
    The ghost faces are random too (a trace that clamps reads them).  The twelve edges of the padded box (cells that are
    ghosts in two or three directions) are 0: the reference's setBounds never writes them, so they are 0 in every state a
    run reaches, and the build relies on that (a solver pass leaves its result in another array, the row forms store
    whole 16-byte groups across the row end); corner traces read them, so here they must be what a run would hold."""
    rng = np.random.default_rng(seed)
    shape = (D + 2, H + 2, W + 2)
    kind = rng.integers(0, 4, shape)
    ux = np.select([kind == 0, kind == 1, kind == 2], [2.0 / dt, -2.0 / dt, rng.standard_normal(shape) * 3.0 / (dt * W)], 0.0)
    out = [ux]
    for n in (H, D):
        far = rng.integers(0, 2, shape) == 1
        near_v, far_v = rng.standard_normal(shape) * 1.5 / (dt * n), rng.standard_normal(shape) / (2.0 * dt)
        out.append(np.where(far, far_v, near_v))
    out.append(rng.standard_normal(shape))
    edges = box_edges(W, H, D)
    for a in out:
        a[edges] = 0.0
    return tuple(np.ascontiguousarray(a, dtype=dtype) for a in out)


def box_edges(W, H, D):
    """bool (D+2, H+2, W+2): the cells that are ghosts in at least two directions"""
    gz, gy, gx = (np.isin(np.arange(n + 2), (0, n + 1)) for n in (D, H, W))
    return (gz[:, None, None].astype(int) + gy[None, :, None] + gx[None, None, :]) >= 2


def rough_mask(W, H, D, seed=SEED):
    """3 % random interior solids: solids in the first and last columns, on the walls, and many near-solid cells."""
    rng = np.random.default_rng(seed + 1000)
    m = np.zeros((D + 2, H + 2, W + 2), dtype=bool)
    m[1:-1, 1:-1, 1:-1] = rng.random((D, H, W)) < 0.03
    return m


def tile_window(want, nf, itemsize):
    """tile_window<T>(want, nf) of advect.hip: the largest r <= want (at least 1) whose nf windows of (9 + 2r)^2 values
    fit LDS_BYTES."""
    r = max(1, int(want))
    while r > 1 and nf * (TILE + 2 * r + 1) ** 2 * itemsize > LDS_BYTES:
        r -= 1
    return r


def traces(W, H, D, ux, uy, uz, dtype=np.float32, dt=DT):
    """The clamped back-trace coordinates px, py, pz of every interior cell, (D, H, W) arrays computed in `dtype` as the
    kernels do (simulation.cpp:384-390): k = dtype(dt) dtype(N) with dt the fp32 member, p = clip(i - k u, 0.5, N + 0.5).
    ux, uy, uz are the CARRYING components: for b = 1..3 the caller passes `prev` for the advected one (:380-382)."""
    T = np.dtype(dtype).type
    half = T(0.5)
    out = []
    for axis, (n, u) in enumerate(((D, uz), (H, uy), (W, ux))):
        k = T(np.float32(dt)) * T(n)
        idx_shape = [1, 1, 1]
        idx_shape[axis] = n
        i = np.arange(1, n + 1).astype(dtype).reshape(idx_shape)
        p = i - k * np.asarray(u, dtype=dtype)[1:-1, 1:-1, 1:-1]
        out.append(np.clip(p, half, T(n) + half))
    pz, py, px = out
    assert px.dtype == py.dtype == pz.dtype == np.dtype(dtype)
    return px, py, pz


def _in_window(p, n, R, axis):
    """floor(p) and floor(p) + 1 inside [max(0, t0 - R), min(n + 1, t0 + TILE + R)], t0 the first row of the cell's tile"""
    idx_shape = [1, 1, 1]
    idx_shape[axis] = n
    i = np.arange(1, n + 1).reshape(idx_shape)
    t0 = 1 + TILE * ((i - 1) // TILE)
    w0, w1 = np.maximum(0, t0 - R), np.minimum(n + 1, t0 + TILE + R)
    p0 = np.floor(p).astype(np.int64)
    return (p0 >= w0) & (p0 + 1 <= w1)


def classify(W, H, D, ux, uy, uz, mask, R, dtype=np.float32, dt=DT):
    """Counts over the fluid cells, a dict: "fluid", and per class of CLASSES the cells whose trace (carried by ux, uy, uz,
    see traces()) is
      lo_in / lo_out   px == 0.5 with floor(py), floor(pz) and their + 1 inside / not inside the window of radius R of the
                       cell's 8 x 8 tile, clipped to the table
      hi               px == W + 0.5
      mid / mid_int    neither / neither and px integral (tx == 0)
      ylo yhi zlo zhi  py == 0.5, py == H + 0.5, pz == 0.5, pz == D + 0.5
      lo_ylo hi_yhi lo_zhi hi_zlo   an x clamp together with a y or z clamp (table rows 0 / H + 1, planes 0 / D + 1)."""
    T = np.dtype(dtype).type
    px, py, pz = traces(W, H, D, ux, uy, uz, dtype, dt)
    fluid = ~np.asarray(mask, dtype=bool)[1:-1, 1:-1, 1:-1]
    half = T(0.5)
    lo, hi = px == half, px == T(W) + half
    mid = ~lo & ~hi
    inside = _in_window(py, H, R, 1) & _in_window(pz, D, R, 0)
    ylo, yhi, zlo, zhi = py == half, py == T(H) + half, pz == half, pz == T(D) + half
    sets = {"lo_in": lo & inside, "lo_out": lo & ~inside, "hi": hi, "mid": mid, "mid_int": mid & (px == np.floor(px)),
            "ylo": ylo, "yhi": yhi, "zlo": zlo, "zhi": zhi, "lo_ylo": lo & ylo, "hi_yhi": hi & yhi, "lo_zhi": lo & zhi,
            "hi_zlo": hi & zlo}
    counts = {k: int(np.count_nonzero(v & fluid)) for k, v in sets.items()}
    counts["fluid"] = int(np.count_nonzero(fluid))
    return counts


def step_carriers(rep, ux, uy, uz, mask, speed=30):
    """The velocities that carry the three traces of a step's velocity advection (simulation.cpp:125-127, :380-382) when
    the step starts from ux, uy, uz, as three (ux, uy, uz) triples: v_x is carried by v_x_prev (the pre-diffusion snapshot,
    inlet applied) and the projected v_y, v_z; v_y by the advected v_x, v_y_prev and the projected v_z; v_z by the advected
    v_x, v_y and v_z_prev.  `rep` is a fresh oracle handle; the step's first half is replayed on it through its per-pass
    entry points (inlet, prev copies, three diffusions, projection, as tests/test_gpu_forces.py does), then the first two
    advections."""
    VX, VY, VZ, OBS, VX0, VY0, VZ0 = 1, 2, 3, 4, 7, 8, 9
    vx, vy, vz = (np.array(a, dtype=rep.dtype) for a in (ux, uy, uz))
    vx[1:-1, 1:-1, 1] = speed                                  # the inlet, simulation.cpp:103-105
    vy[1:-1, 1:-1, 1] = 0.0
    vz[1:-1, 1:-1, 1] = 0.0
    rep.set(OBS, np.asarray(mask, dtype=rep.dtype))
    for f, f0, a in ((VX, VX0, vx), (VY, VY0, vy), (VZ, VZ0, vz)):
        rep.set(f, a)
        rep.set(f0, a)
    for b, f, f0 in ((1, VX, VX0), (2, VY, VY0), (3, VZ, VZ0)):
        rep.diffuse(b, f, f0)
    rep.project()
    out = [(vx, rep.get(VY), rep.get(VZ))]
    rep.advect(1, VX, VX0)
    out.append((rep.get(VX), vy, rep.get(VZ)))
    rep.advect(2, VY, VY0)
    out.append((rep.get(VX), rep.get(VY), vz))
    return out


def classify_step(W, H, D, carriers, mask, R, dtype=np.float32, dt=DT):
    """classify() of each of the three traces of a fused velocity advection, summed: the traces of a class, all sources"""
    parts = [classify(W, H, D, cx, cy, cz, mask, R, dtype, dt) for cx, cy, cz in carriers]
    total = {k: sum(p[k] for p in parts) for k in CLASSES}
    total["fluid"] = parts[0]["fluid"]
    return total, parts


def assert_floors(counts, what=""):
    for k in CLASSES:
        assert counts[k] >= FLOOR, "%s: class %s has %d cells, the floor is %d" % (what, k, counts[k], FLOOR)


def assert_tiny(counts, what=""):
    """5 x 3 x 2: one tile whose window is the whole table, so no inlet-clamped trace can leave it"""
    assert counts["hi"] > 0 and counts["lo_in"] > 0 and counts["lo_out"] == 0, (what, counts)
