"""Slice and projection images on the MI355X (fs_image_values, fs_image_rgb, the image log), through the C ABI via the Python
mirror: every value is compared bit for bit and every byte for byte with tests/image_model.py, the numpy fp64 restatement of
the definition in include/fluidsim.h -- every kind on every axis, slices at both ghost planes and both interior ends, with
and without the obstacle darkening, the built-in and a custom colour table, vortex and flow-statistics sources, no effect on
the fields, the per-step log with its ring, and the error cases.  No tolerance anywhere.  The grids: 37 x 21 x 18 (odd
extents, padded pitch), 64 x 48 x 20 (unpadded pitch), 5 x 3 x 4 (tiny rows), 130 x 6 x 5 (three x tiles of the x-axis
kernel with a ragged tail, fewer rows than a wave), 9 x 70 x 3 (more than 64 rows for the x-axis kernel)."""
import os

import numpy as np
import pytest

import image_model as M
from conftest import GOLDEN, ball_mask, bits_equal

pytestmark = pytest.mark.gpu
GRIDS = [(37, 21, 18), (64, 48, 20), (5, 3, 4), (130, 6, 5), (9, 70, 3)]
PRECISIONS = ["fp32", "fp64"]
grids = pytest.mark.parametrize("grid", GRIDS, ids=lambda g: "x".join(map(str, g)))
precisions = pytest.mark.parametrize("precision", PRECISIONS)
TABLE = np.load(os.path.join(GOLDEN, "gui_density_cmap_256.npy"), allow_pickle=False)


def sim_of(W, H, D, precision="fp32", **kw):
    import fluid_simulation_amd as F
    kw.setdefault("quiet", 1)
    kw.setdefault("dump_every", 0)
    return F.Simulation(W, H, D, 1, precision=precision, **kw)


def body_mask(W, H, D):
    """a ball in the tunnel plus a box that touches three walls"""
    m = ball_mask(W, H, D, 0.6 * W, 0.5 * H + 0.5, 0.5 * D + 0.5, max(1.0, min(H, D) / 4.0))
    m[1:3, 1:3, 1:3] = True
    return m


def random_field(rng, shape, dtype, nan=True):
    """magnitudes spread over seven decades, so that the order of a sum matters; some NaN cells"""
    a = (rng.standard_normal(shape) * 10.0 ** rng.integers(-3, 4, size=shape)).astype(dtype)
    a[rng.random(shape) < 0.05] = 0.0
    if nan:
        a[rng.random(shape) < 0.003] = np.nan
        a[rng.random(shape) < 0.001] = np.inf
        a[rng.random(shape) < 0.001] = -np.inf
    return a


def random_mask(rng, W, H, D, p=0.02):
    solid = np.zeros((D + 2, H + 2, W + 2), dtype=bool)
    solid[1:-1, 1:-1, 1:-1] = rng.random((D, H, W)) < p
    solid[2, 2, 2] = True
    return solid


def slice_indices(N):
    return sorted({0, 1, N, N + 1})


def all_views(grid):
    """(kind, axis, index) of every kind on every axis; slices at index 0, 1, N, N+1"""
    out = []
    for axis in (0, 1, 2):
        out += [(M.SLICE, axis, i) for i in slice_indices(grid[axis])]
        out += [(kind, axis, 0) for kind in (M.SUM, M.MAX, M.MIN)]
    return out


def check_values(sim, source, field, grid, context):
    for kind, axis, index in all_views(grid):
        got = sim.image_values(source, kind, axis, index)
        want = M.values(field, kind, axis, index)
        assert got.dtype == np.float64 and got.shape == M.dims(axis, *grid)
        assert M.same_bits(got, want), (context, M.KIND_NAMES[kind], axis, index, np.argwhere(
            ~((got == want) | (np.isnan(got) & np.isnan(want))))[:6])


# ---- 1. random fields: values ---------------------------------------------------------------------------------------------

@grids
@precisions
def test_values_match_model(grid, precision):
    import fluid_simulation_amd as F
    W, H, D = grid
    rng = np.random.default_rng(W * 1000 + H)
    sim = sim_of(W, H, D, precision)
    full = (D + 2, H + 2, W + 2)
    for which in (F.PRESSURE, F.VY):
        a = random_field(rng, full, sim.dtype)
        sim.set(which, a)
        stored = sim.get(which)
        assert bits_equal(stored, a)
        check_values(sim, which, stored, grid, (grid, precision, which))
    # string kinds, and a kind given by name equals the constant
    assert M.same_bits(sim.image_values(F.VY, "sum", 0), sim.image_values(F.VY, F.IMG_SUM, 0))
    # the order matters for fp64 fields: the sum taken in decreasing x differs from the sequential one somewhere (fp32 values
    # over seven decades mostly add exactly in fp64: 24 + 23 + 7 bits)
    f = sim.get(F.VY).astype(np.float64)
    seq = M.values(f, M.SUM, 0)
    with np.errstate(invalid="ignore"):
        other = M.values(f[:, :, ::-1], M.SUM, 0)
    ok = np.isfinite(seq)
    if W > 8 and precision == "fp64":
        assert (seq[ok] != other[ok]).any()
    sim.close()


# ---- 2. random fields: bytes ---------------------------------------------------------------------------------------------------

@grids
@precisions
def test_rgb_matches_model(grid, precision):
    import fluid_simulation_amd as F
    W, H, D = grid
    rng = np.random.default_rng(W + 31 * D)
    sim = sim_of(W, H, D, precision)
    full = (D + 2, H + 2, W + 2)
    solid = random_mask(rng, W, H, D)
    sim.set_mask(solid)
    obs = sim.get(F.OBS)
    assert np.array_equal(obs != 0, solid)
    sim.set(F.DENS, random_field(rng, full, sim.dtype))
    field = sim.get(F.DENS)
    custom = rng.integers(0, 256, size=(7, 3)).astype(np.uint8)
    for table, name in ((TABLE, "built-in"), (custom, "custom")):
        sim.set_colormap(None if table is TABLE else table)
        for kind, axis, index in all_views(grid):
            for vmin, vmax, alpha in ((-10.0, 10.0, 0.2), (0.0, 0.01, 0.0), (-3.0, 500.0, 1.0)):
                got = sim.image_rgb(F.DENS, kind, axis, index, vmin=vmin, vmax=vmax, obstacle_alpha=alpha)
                want = M.image(field, obs, kind, axis, index, vmin, vmax, alpha, table)
                assert got.dtype == np.uint8 and got.shape == M.dims(axis, *grid) + (3,)
                assert np.array_equal(got, want), (grid, precision, name, M.KIND_NAMES[kind], axis, index, vmin, vmax, alpha,
                                                   np.argwhere((got != want).any(axis=2))[:6])
    # the silhouette darkens something on every axis, and a fractional obs counts from above one half only
    for axis in (0, 1, 2):
        assert M.flags(obs, M.SUM, axis).any()
    o2 = obs.copy()
    o2[1, 1, 1], o2[1, 1, 2], o2[2, 2, 2] = 0.5, 0.75, 0.25
    sim.set(F.OBS, o2)
    sim.set_colormap(None)
    for kind, axis, index in ((M.SLICE, 2, 1), (M.SLICE, 1, 1), (M.SLICE, 0, 1), (M.MAX, 2, 0), (M.MIN, 1, 0), (M.SUM, 0, 0)):
        got = sim.image_rgb(F.DENS, kind, axis, index, vmin=-1.0, vmax=1.0, obstacle_alpha=0.5)
        assert np.array_equal(got, M.image(field, sim.get(F.OBS), kind, axis, index, -1.0, 1.0, 0.5, TABLE)), (kind, axis)
    sim.close()


def test_viewer_slice_image():
    import fluid_simulation_amd as F
    from fluid_simulation_amd import viewer
    W, H, D = 24, 12, 10
    sim = sim_of(W, H, D, acc=3)
    sim.set_mask(body_mask(W, H, D))
    for _ in range(3):
        sim.run_one()
    obs = sim.get(F.OBS)
    for name, (source, vmin, vmax) in viewer.SLICE_RANGES.items():
        for z in (None, 1, D + 1):
            got = viewer.slice_image(sim, name, z)
            want = M.image(sim.get(source), obs, M.SLICE, 2, (D + 2) // 2 if z is None else z, vmin, vmax, 0.2, TABLE)
            assert np.array_equal(got, want), (name, z)
    assert len(np.unique(viewer.slice_image(sim, "v_x").reshape(-1, 3), axis=0)) > 4
    sim.close()


# ---- 3. real steps: vortex and flow-statistics sources, no side effects -------------------------------------------------------

@pytest.mark.parametrize("grid", [(37, 21, 18), (5, 3, 4)], ids=lambda g: "x".join(map(str, g)))
@precisions
def test_derived_sources_and_no_side_effects(grid, precision):
    import fluid_simulation_amd as F
    W, H, D = grid
    sim = sim_of(W, H, D, precision, acc=4, flow_stats="moments")
    sim.set_mask(body_mask(W, H, D))
    for _ in range(3):
        sim.run_one()
    before = [sim.get(f) for f in range(11)]
    obs = before[F.OBS]
    for which in (F.VORTEX_Q, F.VORTEX_WY):
        check_values(sim, F.ISO_VORTEX | which, sim.vortex(which, dtype=sim.dtype), grid, (grid, precision, "vortex", which))
    assert np.abs(sim.vortex(F.VORTEX_Q)).max() > 0
    mean = sim.flow_stats(F.STAT_MEAN_VX)
    assert mean.dtype == np.float64 and np.abs(mean).max() > 0
    check_values(sim, F.SAMPLE_STAT | F.STAT_MEAN_VX, mean, grid, (grid, precision, "mean v_x"))
    check_values(sim, F.SAMPLE_STAT | F.STAT_RAW | F.STAT_UU, sim.flow_stats(F.STAT_UU, raw=True), grid, (grid, precision, "raw uu"))
    check_values(sim, F.SAMPLE_STAT | F.STAT_TKE, sim.flow_stats(F.STAT_TKE), grid, (grid, precision, "tke"))
    got = sim.image_rgb(F.SAMPLE_STAT | F.STAT_MEAN_VX, "max", 1, vmin=-5.0, vmax=35.0, obstacle_alpha=0.2)
    assert np.array_equal(got, M.image(mean, obs, M.MAX, 1, 0, -5.0, 35.0, 0.2, TABLE))
    for f in (F.VX, F.PRESSURE, F.DIVERGENCE, F.VX_PREV):
        check_values(sim, f, before[f], grid, (grid, precision, "field", f))
    after = [sim.get(f) for f in range(11)]
    for f in range(11):
        assert bits_equal(before[f], after[f]), (F.FIELD_NAMES[f], "changed by an image")
    assert sim.flow_stats_samples == 3
    sim.close()


# ---- 4. the log ---------------------------------------------------------------------------------------------------------------------

def views_of(F, D):
    return [(F.DENS, "slice", 2, (D + 2) // 2, 0.0, 0.01, 0.2), (F.VX, "sum", 0, 0, -100.0, 700.0, 0.2)]


@precisions
def test_log_frames_are_the_images_of_their_steps(precision):
    import fluid_simulation_amd as F
    W, H, D = 37, 21, 18
    views = views_of(F, D)
    sim = sim_of(W, H, D, precision, acc=3, image_log=8, image_every=2, profile=1)
    sim.set_mask(body_mask(W, H, D))
    sim.set_image_views(views)
    assert sim.image_view_count == 2
    assert sim.image_frame_bytes == 3 * ((H + 2) * (W + 2) + (D + 2) * (H + 2))
    sim.reset_timing()
    for _ in range(5):
        sim.run_one()
    assert sim.timing("images")[1] == 2 * 3                  # views x frames
    steps, images, dropped = sim.image_log(with_dropped=True)
    assert steps.tolist() == [1, 3, 5] and dropped == 0 and len(images) == 2
    assert images[0].shape == (3, H + 2, W + 2, 3) and images[1].shape == (3, D + 2, H + 2, 3)
    assert sim.image_log()[0].shape == (0,)                  # draining empties the ring
    # a second identical run, with the log off: image_rgb at those steps, and identical fields
    ref = sim_of(W, H, D, precision, acc=3, profile=1)
    ref.set_mask(body_mask(W, H, D))
    ref.reset_timing()
    for step in range(1, 6):
        ref.run_one()
        if step in (1, 3, 5):
            i = (step - 1) // 2
            for v, (source, kind, axis, index, vmin, vmax, alpha) in enumerate(views):
                want = ref.image_rgb(source, kind, axis, index, vmin=vmin, vmax=vmax, obstacle_alpha=alpha)
                assert np.array_equal(images[v][i], want), (step, v)
                model = M.image(ref.get(source), ref.get(F.OBS), F._lib.IMG_KINDS[kind], axis, index, vmin, vmax, alpha, TABLE)
                assert np.array_equal(want, model), (step, v)
    assert ref.timing("images") == (0.0, 0)                  # the feature off: nothing launched for it
    for f in (F.DENS, F.VX, F.VY, F.VZ, F.PRESSURE):
        assert bits_equal(sim.get(f), ref.get(f)), F.FIELD_NAMES[f]
    assert len(np.unique(images[0][2].reshape(-1, 3), axis=0)) > 3, "the density frame shows the plume"
    ref.close()
    sim.close()


def test_log_ring_overwrite_sample_and_clearing():
    import fluid_simulation_amd as F
    W, H, D = 12, 6, 5
    views = views_of(F, D)
    sim = sim_of(W, H, D, acc=2, image_log=3)
    sim.set_image_views(views)
    for _ in range(5):
        sim.run_one()
    n, dropped = F._lib.C.c_long(), F._lib.C.c_long()
    assert sim._L.fs_image_log(sim._h, None, None, 0, F._lib.C.byref(n), F._lib.C.byref(dropped)) == 0
    assert (n.value, dropped.value) == (3, 2)                # frames = NULL: the counts only, nothing drained
    steps, images, dropped = sim.image_log(with_dropped=True)
    assert steps.tolist() == [3, 4, 5] and dropped == 2
    last = sim.image_rgb(*views[0][:4], vmin=0.0, vmax=0.01, obstacle_alpha=0.2)
    assert np.array_equal(images[0][2], last)
    # fs_image_sample: a frame of the state as it is now, with the current step number
    sim.image_sample()
    sim.image_sample()
    steps, images = sim.image_log()
    assert steps.tolist() == [5, 5] and np.array_equal(images[0][0], last) and np.array_equal(images[0][1], last)
    # setting the views, or the option, clears the log; image_every can change at any time
    sim.run_one()
    sim.set_image_views(views[:1])
    assert sim.image_log()[0].size == 0 and sim.image_frame_bytes == 3 * (H + 2) * (W + 2)
    sim.run_one()
    sim.set_option("image_log", 4)
    assert sim.image_log()[0].size == 0
    sim.set_option("image_every", 3)
    for _ in range(4):                                       # steps 8 .. 11: (step - 1) % 3 == 0 at step 10
        sim.run_one()
    steps, images = sim.image_log()
    assert steps.tolist() == [10] and len(images) == 1
    # a custom table takes effect in the log
    table = np.array([[1, 2, 3], [250, 128, 7]], dtype=np.uint8)
    sim.set_colormap(table)
    sim.set_option("image_every", 1)
    sim.run_one()
    steps, images = sim.image_log()
    want = M.image(sim.get(F.DENS), sim.get(F.OBS), M.SLICE, 2, (D + 2) // 2, 0.0, 0.01, 0.2, table)
    assert steps.tolist() == [12] and np.array_equal(images[0][0], want)
    # no views, or no ring: off
    sim.set_image_views([])
    sim.run_one()
    assert sim.image_log()[0].size == 0 and sim.image_view_count == 0
    with pytest.raises(F.FluidsimError):
        sim.image_sample()
    sim.close()


# ---- 5. errors ---------------------------------------------------------------------------------------------------------------------

def test_errors():
    import ctypes as C
    import fluid_simulation_amd as F
    EINVAL = F._lib.EINVAL
    W, H, D = 8, 6, 5
    sim = sim_of(W, H, D)
    L, h = sim._L, sim._h
    out = np.zeros((D + 2) * (H + 2) * (W + 2))
    rgb = np.zeros(3 * out.size, dtype=np.uint8)
    cols, rows = C.c_int(), C.c_int()
    # out = NULL reports the geometry
    for axis, want in ((0, (H + 2, D + 2)), (1, (W + 2, D + 2)), (2, (W + 2, H + 2))):
        assert L.fs_image_values(h, F.DENS, 0, axis, 0, None, 0, C.byref(cols), C.byref(rows)) == 0
        assert (cols.value, rows.value) == want
        assert L.fs_image_rgb(h, F.DENS, 1, axis, 0, 0.0, 1.0, 0.0, None, 0, C.byref(cols), C.byref(rows)) == 0
        assert (cols.value, rows.value) == want
    npix = (W + 2) * (H + 2)
    assert L.fs_image_values(h, F.DENS, 0, 2, 0, out.ctypes.data, npix, None, None) == 0
    assert L.fs_image_rgb(h, F.DENS, 0, 2, 0, 0.0, 1.0, 0.2, rgb.ctypes.data, 3 * npix, None, None) == 0
    for n in (npix - 1, npix + 1, 0):                                            # a wrong size
        assert L.fs_image_values(h, F.DENS, 0, 2, 0, out.ctypes.data, n, None, None) == EINVAL
        assert L.fs_image_rgb(h, F.DENS, 0, 2, 0, 0.0, 1.0, 0.2, rgb.ctypes.data, 3 * n, None, None) == EINVAL
    assert L.fs_image_rgb(h, F.DENS, 0, 2, 0, 0.0, 1.0, 0.2, rgb.ctypes.data, npix, None, None) == EINVAL
    for kind in (-1, 4, 17):
        assert L.fs_image_values(h, F.DENS, kind, 2, 0, out.ctypes.data, npix, None, None) == EINVAL, kind
    for axis in (-1, 3):
        assert L.fs_image_values(h, F.DENS, 0, axis, 0, out.ctypes.data, npix, None, None) == EINVAL, axis
    for axis, N in ((0, W), (1, H), (2, D)):
        for index in (-1, N + 2):
            assert L.fs_image_values(h, F.DENS, 0, axis, index, None, 0, None, None) == EINVAL, (axis, index)
        assert L.fs_image_values(h, F.DENS, 0, axis, N + 1, None, 0, None, None) == 0
        for kind in (1, 2, 3):                                                   # a projection takes index 0 only
            assert L.fs_image_values(h, F.DENS, kind, axis, 1, None, 0, None, None) == EINVAL
            assert L.fs_image_rgb(h, F.DENS, kind, axis, 1, 0.0, 1.0, 0.0, None, 0, None, None) == EINVAL
    for source in (-1, 11, 100, F.ISO_VORTEX | 5, F.ISO_VORTEX | 255, F.SAMPLE_STAT | 13, F.SAMPLE_STAT | F.ISO_VORTEX, 2048, 4096 | F.DENS):
        assert L.fs_image_values(h, source, 0, 2, 0, out.ctypes.data, npix, None, None) == EINVAL, source
        assert L.fs_image_rgb(h, source, 0, 2, 0, 0.0, 1.0, 0.0, rgb.ctypes.data, 3 * npix, None, None) == EINVAL, source
    for vmin, vmax, alpha in ((1.0, 1.0, 0.0), (2.0, 1.0, 0.0), (np.nan, 1.0, 0.0), (0.0, np.inf, 0.0), (-np.inf, 0.0, 0.0),
                             (0.0, 1.0, -0.1), (0.0, 1.0, 1.5), (0.0, 1.0, np.nan)):
        assert L.fs_image_rgb(h, F.DENS, 0, 2, 0, vmin, vmax, alpha, rgb.ctypes.data, 3 * npix, None, None) == EINVAL, (vmin, vmax, alpha)
    # a stat source follows fs_flow_stats_field's errors
    stat = F.SAMPLE_STAT | F.STAT_MEAN_VX
    assert L.fs_image_values(h, stat, 1, 2, 0, out.ctypes.data, npix, None, None) == EINVAL
    assert "flow_stats" in (L.fs_last_error() or b"").decode()
    sim.set_option("flow_stats", "mean")
    assert L.fs_image_values(h, F.SAMPLE_STAT | F.STAT_UU, 1, 2, 0, out.ctypes.data, npix, None, None) == EINVAL
    assert L.fs_image_values(h, stat, 1, 2, 0, out.ctypes.data, npix, None, None) == EINVAL          # no samples yet
    assert L.fs_image_values(h, stat | F.STAT_RAW, 1, 2, 0, out.ctypes.data, npix, None, None) == 0
    assert bits_equal(out[:npix], np.zeros(npix))
    sim.flow_stats_sample()
    assert L.fs_image_values(h, stat, 1, 2, 0, out.ctypes.data, npix, None, None) == 0
    assert L.fs_image_values(h, F.SAMPLE_STAT | F.STAT_RAW | F.STAT_TKE, 1, 2, 0, out.ctypes.data, npix, None, None) == EINVAL
    # the colour table
    t = np.zeros((4097, 3), dtype=np.uint8)
    for n in (1, -1, 4097):
        assert L.fs_image_colormap(h, t.ctypes.data, n) == EINVAL, n
    assert L.fs_image_colormap(h, None, 2) == EINVAL
    assert L.fs_image_colormap(h, t.ctypes.data, 2) == 0 and L.fs_image_colormap(h, t.ctypes.data, 4096) == 0
    assert L.fs_image_colormap(h, None, 0) == 0
    # the views: everything is validated at the call, and a refused call leaves the list as it was
    good = np.array([[F.DENS, 0, 2, 1], [F.VX, 1, 0, 0]], dtype=np.intc)
    rng = np.array([[0.0, 1.0, 0.2], [-1.0, 1.0, 0.0]])
    assert L.fs_image_views(h, good.ctypes.data, rng.ctypes.data, 2) == 0 and sim.image_view_count == 2
    for bad in ([11, 0, 2, 1], [F.DENS, 4, 2, 1], [F.DENS, 0, 3, 1], [F.DENS, 0, 2, D + 2], [F.DENS, 2, 2, 1], [F.SAMPLE_STAT | 13, 0, 2, 1]):
        spec = good.copy()
        spec[1] = bad
        assert L.fs_image_views(h, spec.ctypes.data, rng.ctypes.data, 2) == EINVAL, bad
    for bad in ([1.0, 1.0, 0.0], [0.0, np.nan, 0.0], [0.0, 1.0, 2.0]):
        r2 = rng.copy()
        r2[0] = bad
        assert L.fs_image_views(h, good.ctypes.data, r2.ctypes.data, 2) == EINVAL, bad
    many = np.tile(good[:1], (9, 1))
    assert L.fs_image_views(h, many.ctypes.data, np.tile(rng[:1], (9, 1)).ctypes.data, 9) == EINVAL
    assert L.fs_image_views(h, many.ctypes.data, np.tile(rng[:1], (9, 1)).ctypes.data, -1) == EINVAL
    assert L.fs_image_views(h, None, None, 2) == EINVAL
    assert sim.image_view_count == 2
    assert L.fs_image_views(h, many.ctypes.data, np.tile(rng[:1], (9, 1)).ctypes.data, 8) == 0 and sim.image_view_count == 8
    assert L.fs_image_views(h, good.ctypes.data, rng.ctypes.data, 2) == 0
    # the options
    for bad in ("-1", "65537", "x", ""):
        assert L.fs_set_option(h, b"image_log", bad.encode()) == EINVAL, bad
    for bad in ("0", "-3", "x"):
        assert L.fs_set_option(h, b"image_every", bad.encode()) == EINVAL, bad
    assert L.fs_set_option(h, b"image_log", b"65536") == 0                       # 65536 frames of 408 bytes
    # the drain
    assert L.fs_set_option(h, b"image_log", b"4") == 0
    for _ in range(3):
        sim.run_one()
    n = C.c_long()
    frames = np.zeros(3 * sim.image_frame_bytes, dtype=np.uint8)
    assert L.fs_image_log(h, frames.ctypes.data, None, 2, C.byref(n), None) == EINVAL and n.value == 3     # max_frames < n_frames
    assert L.fs_image_log(h, frames.ctypes.data, None, 3, C.byref(n), None) == 0
    assert L.fs_image_log(h, None, None, 0, C.byref(n), None) == 0 and n.value == 0
    for fn in (L.fs_image_sample,):
        assert fn(None) == EINVAL
    assert L.fs_image_values(None, 0, 0, 0, 0, None, 0, None, None) == EINVAL and L.fs_image_views(None, None, None, 0) == EINVAL
    assert L.fs_image_log(None, None, None, 0, None, None) == EINVAL and L.fs_image_colormap(None, None, 0) == EINVAL
    sim.close()
    # the ring's size limit: N x frame bytes over 1 GiB, from either side
    big = sim_of(600, 600, 4)
    spec = np.array([[F.DENS, 0, 2, 1]], dtype=np.intc)          # 602 x 602 x 3 = 1087212 bytes a frame: 987 fit 1 GiB
    assert big._L.fs_image_views(big._h, spec.ctypes.data, rng.ctypes.data, 1) == 0
    assert big._L.fs_set_option(big._h, b"image_log", b"988") == EINVAL
    assert big._L.fs_set_option(big._h, b"image_log", b"987") == 0
    two = np.tile(spec, (2, 1))
    assert big._L.fs_image_views(big._h, two.ctypes.data, np.tile(rng[:1], (2, 1)).ctypes.data, 2) == EINVAL
    assert big.image_view_count == 1
    big.close()
    # slab handles
    sim = sim_of(8, 8, 8)
    sim.comm_init(0, 2, b"FSNULL:".ljust(128, b"\0"))
    assert sim._L.fs_image_values(sim._h, F.DENS, 0, 2, 0, None, 0, None, None) == EINVAL
    assert "single-GPU" in (sim._L.fs_last_error() or b"").decode()
    assert sim._L.fs_image_rgb(sim._h, F.DENS, 0, 2, 0, 0.0, 1.0, 0.0, None, 0, None, None) == EINVAL
    assert sim._L.fs_image_views(sim._h, good.ctypes.data, rng.ctypes.data, 2) == EINVAL
    with pytest.raises(F.FluidsimError):
        sim.image_values(F.DENS, "slice", 2, 1)
    sim.close()
