"""The point sampler on the MI355X (fs_sample_points, fs_sample), through the C ABI via the Python mirror: every value
is compared bit for bit with tests/sample_model.py, the numpy fp64 restatement of the definition in include/fluidsim.h --
random fields and points, a dyadic linear field, the nearest cell, FLUID mode on an obstacle's surface (and
viewer.surface_pressure on top of it), vortex and flow-statistics sources, no effect on the fields, and the error cases.
No tolerance anywhere.  The grids: 37 x 21 x 18 and 64 x 48 x 20 (row pitch with and without padding), 5 x 3 x 4 (tiny rows)."""
import numpy as np
import pytest

import sample_model as M
from conftest import ball_mask, bits_equal

pytestmark = pytest.mark.gpu
GRIDS = [(37, 21, 18), (64, 48, 20), (5, 3, 4)]
PRECISIONS = ["fp32", "fp64"]
grids = pytest.mark.parametrize("grid", GRIDS, ids=lambda g: "x".join(map(str, g)))
precisions = pytest.mark.parametrize("precision", PRECISIONS)


def sim_of(W, H, D, precision="fp32", **kw):
    import fluid_simulation_amd as F
    kw.setdefault("quiet", 1)
    kw.setdefault("dump_every", 0)
    return F.Simulation(W, H, D, 1, precision=precision, **kw)


def body_mask(W, H, D):
    """a ball in the tunnel plus a box that touches three walls (interior cells 1..2 on every axis)"""
    m = ball_mask(W, H, D, 0.6 * W, 0.5 * H + 0.5, 0.5 * D + 0.5, max(1.0, min(H, D) / 4.0))
    m[1:3, 1:3, 1:3] = True
    return m


def random_field(rng, shape, dtype):
    a = (rng.standard_normal(shape) * 10.0 ** rng.integers(-3, 4, size=shape)).astype(dtype)
    a[rng.random(shape) < 0.05] = 0.0
    return a


def check_modes(sim, source, field, obs, pts, context):
    """the kept points are `pts`: all three modes of `source` against the model applied to `field`"""
    for mode in M.MODES:
        got = sim.sample(source, M.MODE_NAMES[mode])
        want = M.sample(field, obs, pts, mode)
        assert got.dtype == np.float64 and got.shape == (pts.shape[0],)
        assert M.same_bits(got, want), (context, M.MODE_NAMES[mode], np.flatnonzero(
            ~((got == want) | (np.isnan(got) & np.isnan(want))))[:8])


# ---- 1. random fields ---------------------------------------------------------------------------------------------------

@grids
@precisions
def test_random_fields_match_model(grid, precision):
    import fluid_simulation_amd as F
    W, H, D = grid
    rng = np.random.default_rng(W * 1000 + H)
    sim = sim_of(W, H, D, precision)
    full = (D + 2, H + 2, W + 2)
    solid = np.zeros(full, dtype=bool)
    solid[1:-1, 1:-1, 1:-1] = rng.random((D, H, W)) < 0.35
    sim.set_mask(solid)
    pts = M.special_points(W, H, D, rng, n_random=300)
    sim.sample_points(pts)
    obs = sim.get(F.OBS)
    assert np.array_equal(obs != 0, solid)
    for which in (F.PRESSURE, F.VY, F.BUFFER):
        a = random_field(rng, full, sim.dtype)
        sim.set(which, a)
        stored = sim.get(which)
        assert bits_equal(stored, a)
        check_modes(sim, which, stored, obs, pts, (grid, precision, which))
    check_modes(sim, F.OBS, obs, obs, pts, (grid, precision, "obs"))
    outside = np.isnan(pts).any(axis=1) | (pts < 0).any(axis=1) | (pts > np.array(grid) + 1.0).any(axis=1)
    assert outside.sum() >= 19 and np.isnan(sim.sample(F.BUFFER, "nearest")[outside]).all()
    # a smaller and an empty point set replace the kept one
    sim.sample_points(pts[:7])
    assert M.same_bits(sim.sample(F.BUFFER, "linear"), M.sample(sim.get(F.BUFFER), obs, pts[:7], M.LINEAR))
    sim.sample_points(np.zeros((0, 3)))
    assert sim.sample(F.BUFFER).shape == (0,)
    sim.close()


# ---- 2. a dyadic linear field, and the nearest cell -----------------------------------------------------------------------

@grids
@precisions
def test_linear_field_and_nearest(grid, precision):
    import fluid_simulation_amd as F
    W, H, D = grid
    rng = np.random.default_rng(7 * W + D)
    sim = sim_of(W, H, D, precision)
    z, y, x = (a.astype(np.float64) for a in np.mgrid[0:D + 2, 0:H + 2, 0:W + 2])
    a0, gx, gy, gz = 3.5, 0.25, -1.5, 2.0                # every value and every product below is exact in fp32 and fp64
    sim.set(F.DENS, (a0 + gx * x + gy * y + gz * z).astype(sim.dtype))
    n = 400
    pts = np.stack([rng.integers(0, 8 * (W + 1) + 1, n), rng.integers(0, 8 * (H + 1) + 1, n),
                    rng.integers(0, 8 * (D + 1) + 1, n)], axis=1).astype(np.float64) / 8.0
    pts[0] = (0.0, 0.0, 0.0)
    pts[1] = (W + 1.0, H + 1.0, D + 1.0)
    sim.sample_points(pts)
    want = a0 + gx * pts[:, 0] + gy * pts[:, 1] + gz * pts[:, 2]
    assert M.same_bits(sim.sample(F.DENS, "linear"), want)
    # NEAREST is the stored value of the nearest cell, ties upwards
    field = random_field(rng, x.shape, sim.dtype)
    sim.set(F.VZ, field)
    pts = np.concatenate([pts, M.special_points(W, H, D, rng, n_random=200)])
    pts = pts[~(np.isnan(pts).any(axis=1) | (pts < 0).any(axis=1) | (pts > np.array(grid) + 1.0).any(axis=1))]
    sim.sample_points(pts)
    cell = []
    for k, N in enumerate(grid):
        i0 = np.minimum(np.floor(pts[:, k]).astype(np.int64), N)
        cell.append(i0 + (pts[:, k] - i0 >= 0.5))
    i, j, l = cell
    assert M.same_bits(sim.sample(F.VZ, "nearest"), sim.get(F.VZ)[l, j, i].astype(np.float64))
    sim.close()


# ---- 3. FLUID mode on the obstacle's surface ------------------------------------------------------------------------------

@grids
@precisions
def test_fluid_mode_on_the_surface(grid, precision):
    import fluid_simulation_amd as F
    from fluid_simulation_amd import viewer
    W, H, D = grid
    rng = np.random.default_rng(W + 31 * D)
    sim = sim_of(W, H, D, precision, speed=7, dt=0.125)
    solid = body_mask(W, H, D)
    sim.set_mask(solid)
    sim.set(F.PRESSURE, random_field(rng, solid.shape, sim.dtype) + sim.dtype(1.0))   # solid cells hold garbage: it must not leak
    p = sim.get(F.PRESSURE).astype(np.float64)
    verts, faces = sim.obstacle_surface()
    assert verts.shape[0] > 20
    v = verts.astype(np.float64)
    lo = np.floor(v).astype(np.int64)
    half = (v - lo) == 0.5
    assert np.array_equal(half.sum(axis=1), np.ones(v.shape[0]))          # a vertex is the midpoint of one grid edge
    hi = lo + half
    solid_lo, solid_hi = solid[lo[:, 2], lo[:, 1], lo[:, 0]], solid[hi[:, 2], hi[:, 1], hi[:, 0]]
    assert np.all(solid_lo != solid_hi)
    fluid_end = np.where(solid_lo[:, None], hi, lo)
    want = p[fluid_end[:, 2], fluid_end[:, 1], fluid_end[:, 0]]
    sim.sample_points(v)
    got = sim.sample(F.PRESSURE, "fluid")
    assert M.same_bits(got, want)
    assert (v.min(axis=0) == 0.5).all(), "the box touches three walls: vertices on edges to ghost cells"
    assert not M.same_bits(sim.sample(F.PRESSURE, "linear"), want), "plain interpolation mixes the solid cell's value in"
    # surface_pressure: the mesh, p and cp
    p_ref = 0.75
    mesh = viewer.surface_pressure(sim, p_ref=p_ref)
    assert np.array_equal(mesh["vertexes"], v) and np.array_equal(mesh["faces"], faces)
    assert M.same_bits(mesh["p"], want)
    assert sim.speed == 7 and sim.dt == 0.125
    assert M.same_bits(mesh["cp"], 2.0 * (want - p_ref) / (0.125 * 49.0))
    # another source through the same call
    sim.set(F.DENS, random_field(rng, solid.shape, sim.dtype))
    q = sim.get(F.DENS).astype(np.float64)
    assert M.same_bits(viewer.surface_pressure(sim, source=F.DENS)["p"], q[fluid_end[:, 2], fluid_end[:, 1], fluid_end[:, 0]])
    # all eight corners solid: NaN in FLUID mode only; weight on solid corners only: NaN as well
    sim.sample_points(np.array([[1.5, 1.5, 1.5], [1.25, 1.75, 1.5], [1.0, 1.0, 1.0], [2.0, 1.5, 2.0]]))
    assert np.isnan(sim.sample(F.PRESSURE, "fluid")).all()
    assert not np.isnan(sim.sample(F.PRESSURE, "linear")).any() and not np.isnan(sim.sample(F.PRESSURE, "nearest")).any()
    sim.close()


# ---- 4. real steps: vortex and flow-statistics sources, no side effects ------------------------------------------------------

@grids
@precisions
def test_derived_sources_and_no_side_effects(grid, precision):
    import fluid_simulation_amd as F
    W, H, D = grid
    rng = np.random.default_rng(D * 100 + W)
    sim = sim_of(W, H, D, precision, acc=4, flow_stats="moments")
    sim.set_mask(body_mask(W, H, D))
    for _ in range(4):
        sim.run_one()
    assert sim.flow_stats_samples == 4
    pts = M.special_points(W, H, D, rng, n_random=200)
    sim.sample_points(pts)
    before = [sim.get(f) for f in range(11)]
    obs = before[F.OBS]
    for which in (F.VORTEX_Q, F.VORTEX_WY):
        check_modes(sim, F.ISO_VORTEX | which, sim.vortex(which), obs, pts, (grid, precision, "vortex", which))
    assert np.abs(sim.vortex(F.VORTEX_Q)).max() > 0
    mean = sim.flow_stats(F.STAT_MEAN_VX)
    assert mean.dtype == np.float64 and np.abs(mean).max() > 0
    check_modes(sim, F.SAMPLE_STAT | F.STAT_MEAN_VX, mean, obs, pts, (grid, precision, "mean v_x"))
    check_modes(sim, F.SAMPLE_STAT | F.STAT_RAW | F.STAT_UU, sim.flow_stats(F.STAT_UU, raw=True), obs, pts, (grid, precision, "raw uu"))
    check_modes(sim, F.SAMPLE_STAT | F.STAT_TKE, sim.flow_stats(F.STAT_TKE), obs, pts, (grid, precision, "tke"))
    for f in (F.VX, F.PRESSURE, F.DIVERGENCE, F.VX_PREV):
        check_modes(sim, f, before[f], obs, pts, (grid, precision, "field", f))
    after = [sim.get(f) for f in range(11)]
    for f in range(11):
        assert bits_equal(before[f], after[f]), (F.FIELD_NAMES[f], "changed by fs_sample")
    assert sim.flow_stats_samples == 4
    # and the run goes on as if nothing had been sampled
    ref = sim_of(W, H, D, precision, acc=4)
    ref.set_mask(body_mask(W, H, D))
    for _ in range(5):
        ref.run_one()
    sim.run_one()
    for f in (F.DENS, F.VX, F.VY, F.VZ, F.PRESSURE):
        assert bits_equal(sim.get(f), ref.get(f)), F.FIELD_NAMES[f]
    ref.close()
    sim.close()


# ---- 5. errors --------------------------------------------------------------------------------------------------------------

def test_errors():
    import fluid_simulation_amd as F
    EINVAL = F._lib.EINVAL
    sim = sim_of(8, 6, 5)
    L, h = sim._L, sim._h
    pts = np.ascontiguousarray(np.ones((4, 3)))
    out = np.zeros(8)
    assert L.fs_sample(h, F.DENS, 1, out.ctypes.data, 0) == 0                     # no points kept: nothing to do
    assert L.fs_sample_points(h, pts.ctypes.data, 4) == 0
    assert L.fs_sample(h, F.DENS, 1, out.ctypes.data, 4) == 0
    for n in (3, 5, 0):                                                          # count mismatch
        assert L.fs_sample(h, F.DENS, 1, out.ctypes.data, n) == EINVAL
    assert L.fs_sample(h, F.DENS, 1, None, 4) == EINVAL
    for source in (-1, 11, 100, F.ISO_VORTEX | 5, F.ISO_VORTEX | 255, F.SAMPLE_STAT | 13, F.SAMPLE_STAT | F.ISO_VORTEX, 2048, 4096 | F.DENS):
        assert L.fs_sample(h, source, 1, out.ctypes.data, 4) == EINVAL, source
    for mode in (-1, 3, 17):
        assert L.fs_sample(h, F.DENS, mode, out.ctypes.data, 4) == EINVAL, mode
    # a stat source follows fs_flow_stats_field's errors: feature off, second moment in mode "mean", no samples yet, raw tke
    assert L.fs_sample(h, F.SAMPLE_STAT | F.STAT_MEAN_VX, 1, out.ctypes.data, 4) == EINVAL
    assert "flow_stats" in (L.fs_last_error() or b"").decode()
    sim.set_option("flow_stats", "mean")
    assert L.fs_sample(h, F.SAMPLE_STAT | F.STAT_UU, 1, out.ctypes.data, 4) == EINVAL
    assert L.fs_sample(h, F.SAMPLE_STAT | F.STAT_MEAN_VX, 1, out.ctypes.data, 4) == EINVAL
    assert L.fs_sample(h, F.SAMPLE_STAT | F.STAT_RAW | F.STAT_MEAN_VX, 1, out.ctypes.data, 4) == 0
    assert bits_equal(out[:4], np.zeros(4))
    sim.flow_stats_sample()
    assert L.fs_sample(h, F.SAMPLE_STAT | F.STAT_MEAN_VX, 1, out.ctypes.data, 4) == 0
    assert L.fs_sample(h, F.SAMPLE_STAT | F.STAT_RAW | F.STAT_TKE, 1, out.ctypes.data, 4) == EINVAL
    # the point count
    assert L.fs_sample_points(h, pts.ctypes.data, (1 << 24) + 1) == EINVAL
    assert L.fs_sample_points(h, pts.ctypes.data, -1) == EINVAL
    assert L.fs_sample_points(h, None, 4) == EINVAL
    assert L.fs_sample(h, F.DENS, 1, out.ctypes.data, 4) == 0                     # the kept set survived the refusals
    assert L.fs_sample_points(None, pts.ctypes.data, 4) == EINVAL and L.fs_sample(None, 0, 0, out.ctypes.data, 4) == EINVAL
    sim.close()
    # slab handles
    sim = sim_of(8, 8, 8)
    sim.comm_init(0, 2, b"FSNULL:".ljust(128, b"\0"))
    assert sim._L.fs_sample_points(sim._h, pts.ctypes.data, 4) == EINVAL
    assert "single-GPU" in (sim._L.fs_last_error() or b"").decode()
    assert sim._L.fs_sample(sim._h, F.DENS, 1, out.ctypes.data, 0) == EINVAL
    with pytest.raises(F.FluidsimError):
        sim.sample_points(pts)
    sim.close()


def test_rake():
    from fluid_simulation_amd import viewer
    r = viewer.rake((1.0, 2.0, 3.0), (5.0, 2.0, 1.0), 5)
    assert r.dtype == np.float64 and np.array_equal(r, [[1, 2, 3], [2, 2, 2.5], [3, 2, 2], [4, 2, 1.5], [5, 2, 1]])
    assert viewer.rake((1, 1, 1), (2, 2, 2), 1).tolist() == [[1.0, 1.0, 1.0]] and viewer.rake((1, 1, 1), (2, 2, 2), 0).shape == (0, 3)
    sim = sim_of(8, 6, 5)
    import fluid_simulation_amd as F
    z, y, x = (a.astype(np.float32) for a in np.mgrid[0:7, 0:8, 0:10])
    sim.set(F.VX, x + 2 * y + 4 * z)
    sim.sample_points(r)
    assert sim.sample(F.VX).tolist() == [17.0, 16.0, 15.0, 14.0, 13.0]
    sim.close()
