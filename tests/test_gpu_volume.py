"""Volume rendering on the MI355X (fs_volume_rays, fs_volume_camera, fs_volume_render, the volume log), through the C ABI via
the Python mirror: every byte of rgb and every bit of acc is compared with tests/volume_model.py, the Python fp64 restatement
of the definition in include/fluidsim.h -- random fields spread over decades with NaN and infinite cells, a ball plus a
wall-touching box as obstacles, cameras outside and inside the box, a hand-made ray set with the special rays of the CPU test,
low opacity and high opacity with early termination, vortex and flow-statistics sources, no effect on the fields, the per-step
log with its ring, the launch counts, the error cases.  No tolerance anywhere.  The grids: 37 x 21 x 18 (odd extents, padded
pitch), 64 x 48 x 20 (unpadded pitch), 5 x 3 x 4 (tiny).  The images: 1 x 1, 7 x 5 (smaller than a wave's tile), 19 x 13
(ragged tiles), 70 x 9 (wider than a workgroup's 16 x 16 pixels; five of them).

A case must not pass by never exercising a path: each random case first asserts, on the model alone, that its rays include a
miss, a ray through fluid to the exit, an obstacle hit, an early termination and a skipped NaN sample."""
import functools
import math
import os
import subprocess

import numpy as np
import pytest

import image_model
import volume_model as M
from conftest import GOLDEN, ROOT, ball_mask, bits_equal

pytestmark = pytest.mark.gpu
GRIDS = [(37, 21, 18), (64, 48, 20), (5, 3, 4)]
PRECISIONS = ["fp32", "fp64"]
SIZES = [(1, 1), (7, 5), (19, 13), (70, 9)]              # (cols, rows)
grids = pytest.mark.parametrize("grid", GRIDS, ids=lambda g: "x".join(map(str, g)))
precisions = pytest.mark.parametrize("precision", PRECISIONS)
TABLE = np.load(os.path.join(GOLDEN, "gui_density_cmap_256.npy"), allow_pickle=False)
FAMILIES = ["sweep", "sweep_pair", "sweep_triple", "divergence", "gradient", "advect", "bounds", "misc", "comm", "multigrid", "forces",
            "residual", "flow_stats", "vortex", "probes", "body_forces", "images", "tracers"]
NEEDED = (M.MISS, M.EXIT, M.SOLID, M.EARLY, M.NAN_SKIPPED)
# low opacity, no early termination; high opacity, rays end at T < 0.05.  Steps of one cell and of half a cell.
LOW = dict(vmin=0.0, vmax=0.5, opacity=0.02, step=1.0, t_min=0.0, obstacle=(128, 128, 128), background=(26, 26, 26))
HIGH = dict(vmin=-0.1, vmax=0.3, opacity=3.0, step=0.5, t_min=0.05, obstacle=(200, 90, 10), background=(3, 250, 77))


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


def random_field(rng, shape, dtype):
    """magnitudes spread over decades around the colour ranges; some NaN and infinite cells"""
    a = (np.abs(rng.standard_normal(shape)) * 10.0 ** rng.integers(-4, 1, size=shape)).astype(dtype)
    a[rng.random(shape) < 0.1] = 0.0
    a[rng.random(shape) < 0.05] *= -1
    a[rng.random(shape) < 0.004] = np.nan
    a[rng.random(shape) < 0.001] = np.inf
    a[rng.random(shape) < 0.001] = -np.inf
    a[-2, -2, -2] = np.nan                               # cell (W, H, D): one NaN on the tiny grid too
    return a


def outside_camera(grid, size=(1, 1), ortho=False):
    """looks at the box centre from beyond the corner (W+1, H+1, D+1); the image plane is sized to the image's aspect so that
    the box fills most of a cols x rows image and the pixels towards its corners miss it"""
    W, H, D = grid
    centre = [0.5 * (W + 1), 0.5 * (H + 1), 0.5 * (D + 1)]
    eye = [centre[0] + 1.1 * (W + 1), centre[1] + 0.9 * (H + 1), centre[2] + 1.7 * (D + 1)]
    wide = max(1.0, size[0] / size[1])
    return eye + centre + [0.0, 1.0, 0.0] + ([0.7 * max(grid) / wide, 1.0] if ortho else [0.5 / wide, 0.0])


def inside_camera(grid):
    """stands in the far upper corner region of the box and looks at the wall-touching block"""
    W, H, D = grid
    return [W - 0.3, H - 0.2, D - 0.4] + [1.5, 1.5, 1.5] + [0.0, 0.0, 1.0] + [0.9, 0.0]


@functools.lru_cache(maxsize=None)
def case(grid, precision):
    """field (D+2, H+2, W+2) in the handle's precision, the solid mask, and the ray sets {name: (rows, cols, 6)}"""
    W, H, D = grid
    rng = np.random.default_rng(1000 * W + 10 * D + (precision == "fp64"))
    field = random_field(rng, (D + 2, H + 2, W + 2), np.float64 if precision == "fp64" else np.float32)
    solid = body_mask(W, H, D)
    solid[-2, -2, -2] = False
    rays = {}
    for cols, rows in SIZES:
        rays["outside %dx%d" % (cols, rows)] = M.camera_rays(outside_camera(grid, (cols, rows)), cols, rows)
    rays["ortho 19x13"] = M.camera_rays(outside_camera(grid, (19, 13), True), 19, 13)
    rays["inside 7x5"] = M.camera_rays(inside_camera(grid), 7, 5)
    rays["special"] = M.special_rays(W, H, D).reshape(1, -1, 6)
    for a in (field, solid):
        a.setflags(write=False)
    return field, solid, rays


@functools.lru_cache(maxsize=None)
def reference(grid, precision, name, high):
    field, solid, rays = case(grid, precision)
    return M.render(rays[name], field, solid.astype(np.float32), M.params(**(HIGH if high else LOW)), TABLE)


def classes_of(grid, precision):
    seen = 0
    for name in case(grid, precision)[2]:
        for high in (False, True):
            seen |= int(np.bitwise_or.reduce(reference(grid, precision, name, high)[2].reshape(-1)))
    return seen


def set_rays(sim, slot, rays):
    sim.volume_rays(slot, rays)


# ---- 1. random fields against the model -----------------------------------------------------------------------------------

@grids
@precisions
def test_render_matches_model(grid, precision):
    import fluid_simulation_amd as F
    W, H, D = grid
    seen = classes_of(grid, precision)                       # the model alone: every path is exercised
    for bit in NEEDED:
        assert seen & bit, ("the case's rays never take path", bit)
    field, solid, rays = case(grid, precision)
    sim = sim_of(W, H, D, precision)
    sim.set_mask(solid)
    sim.set(F.PRESSURE, field)
    assert bits_equal(sim.get(F.PRESSURE), field) and np.array_equal(sim.get(F.OBS) != 0, solid)
    before = [sim.get(f) for f in range(11)]
    for slot, (name, r) in enumerate(rays.items()):
        slot %= F._lib.VOLUME_CAMERAS_MAX
        if name.startswith("outside") or name.startswith("ortho") or name.startswith("inside"):
            cols, rows = r.shape[1], r.shape[0]
            cam = outside_camera(grid, (cols, rows), name.startswith("ortho")) if not name.startswith("inside") else inside_camera(grid)
            if cam[10]:
                sim.volume_camera(slot, cam[0:3], cam[3:6], cam[6:9], ortho_height=2.0 * cam[9], size=(cols, rows))
            else:                                            # the tangent is taken in Python: hand the library the half height itself
                c = np.array(cam, dtype=np.float64)
                F._lib.check(sim._L.fs_volume_camera(sim._h, slot, c.ctypes.data, cols, rows))
                sim._volume_size[slot] = (rows, cols)
        else:
            set_rays(sim, slot, r)
        for high in (False, True):
            want_rgb, want_acc, _ = reference(grid, precision, name, high)
            rgb, acc = sim.volume_render(F.PRESSURE, slot, with_acc=True, **(HIGH if high else LOW))
            assert rgb.dtype == np.uint8 and rgb.shape == r.shape[:2] + (3,) and acc.shape == r.shape[:2] + (4,)
            assert M.same_bits(acc, want_acc), (grid, precision, name, high, np.argwhere(
                (acc.view(np.uint64) != want_acc.view(np.uint64)).any(axis=2))[:6])
            assert np.array_equal(rgb, want_rgb), (grid, precision, name, high, np.argwhere((rgb != want_rgb).any(axis=2))[:6])
            assert np.array_equal(sim.volume_render(F.PRESSURE, slot, **(HIGH if high else LOW)), want_rgb)   # acc = NULL
    after = [sim.get(f) for f in range(11)]
    for f in range(11):
        assert bits_equal(before[f], after[f]), (F.FIELD_NAMES[f], "changed by a rendering")
    sim.close()


def test_camera_rays_are_the_models():
    """fs_volume_camera's rays, seen through a field that encodes nothing: a ray set given by hand renders the same bytes"""
    import fluid_simulation_amd as F
    grid = (37, 21, 18)
    field, solid, rays = case(grid, "fp32")
    sim = sim_of(*grid)
    sim.set_mask(solid)
    sim.set(F.DENS, field)
    for ortho in (False, True):
        cam = outside_camera(grid, (19, 13), ortho)
        c = np.array(cam, dtype=np.float64)
        F._lib.check(sim._L.fs_volume_camera(sim._h, 0, c.ctypes.data, 19, 13))
        sim._volume_size[0] = (13, 19)
        sim.volume_rays(1, M.camera_rays(cam, 19, 13))
        a, b = sim.volume_render(F.DENS, 0, with_acc=True, **HIGH), sim.volume_render(F.DENS, 1, with_acc=True, **HIGH)
        assert np.array_equal(a[0], b[0]) and M.same_bits(a[1], b[1])
    sim.close()


# ---- 2. derived sources after real steps, a custom table ----------------------------------------------------------------------

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
    rays = M.camera_rays(outside_camera(grid, (19, 13)), 19, 13)
    sim.volume_rays(2, rays)
    custom = np.array([[0, 0, 0], [255, 255, 255], [10, 200, 30], [250, 128, 7], [1, 2, 3]], dtype=np.uint8)
    for table in (TABLE, custom):
        sim.set_colormap(None if table is TABLE else table)
        q = sim.vortex(F.VORTEX_Q, dtype=sim.dtype)
        par = dict(vmin=-50.0, vmax=50.0, opacity=0.5, step=0.5, t_min=0.02)
        rgb, acc = sim.volume_render(F.ISO_VORTEX | F.VORTEX_Q, 2, with_acc=True, **par)
        want = M.render(rays, q, obs, M.params(**par), table)
        assert M.same_bits(acc, want[1]) and np.array_equal(rgb, want[0]), (grid, precision, "vortex Q")
        mean = sim.flow_stats(F.STAT_MEAN_VX)
        assert mean.dtype == np.float64 and np.abs(mean).max() > 0
        par = dict(vmin=0.0, vmax=35.0, opacity=0.05, step=0.25, t_min=0.1)
        rgb, acc = sim.volume_render(F.SAMPLE_STAT | F.STAT_MEAN_VX, 2, with_acc=True, **par)
        want = M.render(rays, mean, obs, M.params(**par), table)
        assert M.same_bits(acc, want[1]) and np.array_equal(rgb, want[0]), (grid, precision, "mean v_x")
        assert len(np.unique(rgb.reshape(-1, 3), axis=0)) > 3
    after = [sim.get(f) for f in range(11)]
    for f in range(11):
        assert bits_equal(before[f], after[f]), (F.FIELD_NAMES[f], "changed by a rendering")
    assert sim.flow_stats_samples == 3
    sim.close()


def test_viewer_volume_image():
    import fluid_simulation_amd as F
    from fluid_simulation_amd import viewer
    W, H, D = 24, 12, 10
    sim = sim_of(W, H, D, acc=3)
    sim.set_mask(body_mask(W, H, D))
    for _ in range(3):
        sim.run_one()
    centre = np.array([W + 1, H + 1, D + 1], dtype=np.float64) * 0.5
    for az, el, dist, size in ((45.0, 30.0, 200.0, (19, 13)), (-70.0, 10.0, 40.0, (7, 5))):
        got = viewer.volume_image(sim, "density", azimuth=az, elevation=el, distance=dist, size=size, slot=1)
        a, e = np.deg2rad(np.float64(az)), np.deg2rad(np.float64(el))
        eye = centre + np.array([-dist * np.cos(e) * np.sin(a), dist * np.sin(e), dist * np.cos(e) * np.cos(a)])
        sim.volume_camera(3, eye, centre, (0.0, 1.0, 0.0), fov_deg=45.0, size=size)
        par = dict(vmin=0.0, vmax=0.01, opacity=0.05, step=0.5, t_min=0.01, obstacle=(128, 128, 128), background=(26, 26, 26))
        assert got.shape == (size[1], size[0], 3) and np.array_equal(got, sim.volume_render(F.DENS, 3, **par)), (az, el)
        half = float(np.tan(np.deg2rad(np.float64(45.0)) / 2.0))
        rays = M.camera_rays(list(viewer.orbit_eye(centre, az, el, dist)) + list(centre) + [0.0, 1.0, 0.0, half, 0.0], *size)
        assert np.array_equal(got, M.render(rays, sim.get(F.DENS), sim.get(F.OBS), M.params(**par), TABLE)[0]), (az, el)
    # the default view of the reference GUI sees the whole box of this size: more than the background
    assert len(np.unique(viewer.volume_image(sim, "v_x", size=(19, 13), distance=60.0).reshape(-1, 3), axis=0)) > 3
    sim.close()


# ---- 3. the log -------------------------------------------------------------------------------------------------------------------

def log_setup(sim, F, grid):
    sim.volume_camera(0, outside_camera(grid)[0:3], outside_camera(grid)[3:6], (0.0, 1.0, 0.0), fov_deg=50.0, size=(19, 13))
    sim.volume_rays(2, M.camera_rays(outside_camera(grid, (7, 5), True), 7, 5))
    views = [(F.DENS, 0, dict(vmin=0.0, vmax=0.01, opacity=0.3, step=0.5, t_min=0.02)),
             (F.VX, 2, dict(vmin=-5.0, vmax=35.0, opacity=0.01, step=1.0, t_min=0.0, background=(0, 0, 0)))]
    sim.set_volume_views(views)
    return views


@precisions
def test_log_frames_are_the_renderings_of_their_steps(precision):
    import fluid_simulation_amd as F
    grid = W, H, D = 37, 21, 18
    sim = sim_of(W, H, D, precision, acc=3, volume_log=8, volume_every=2, profile=1)
    sim.set_mask(body_mask(W, H, D))
    views = log_setup(sim, F, grid)
    assert sim.volume_view_count == 2 and sim.volume_frame_bytes == 3 * (19 * 13 + 7 * 5)
    sim.reset_timing()
    for _ in range(5):
        sim.run_one()
    assert sim.timing("volume")[1] == 2 * 3 and sim.timing("volume")[0] > 0.0     # views x frames
    steps, images, dropped = sim.volume_log(with_dropped=True)
    assert steps.tolist() == [1, 3, 5] and dropped == 0 and len(images) == 2
    assert images[0].shape == (3, 13, 19, 3) and images[1].shape == (3, 5, 7, 3)
    assert sim.volume_log()[0].shape == (0,)                 # draining empties the ring
    # a second identical run, with the log off: volume_render at those steps, the model, identical fields and launch counts
    ref = sim_of(W, H, D, precision, acc=3, profile=1)
    ref.set_mask(body_mask(W, H, D))
    log_setup(ref, F, grid)
    ref.reset_timing()
    counts = dict.fromkeys(FAMILIES + ["volume"], 0)
    for step in range(1, 6):
        ref.run_one()
        for fam in counts:                                   # the step's own launches: volume_render below counts as "misc"
            counts[fam] += ref.timing(fam)[1]
        if step in (1, 3, 5):
            for v, (source, slot, par) in enumerate(views):
                want = ref.volume_render(source, slot, **par)
                assert np.array_equal(images[v][(step - 1) // 2], want), (step, v)
                if step == 5 and slot == 2:
                    rays = M.camera_rays(outside_camera(grid, (7, 5), True), 7, 5)
                    assert np.array_equal(want, M.render(rays, ref.get(source), ref.get(F.OBS), M.params(**par), TABLE)[0])
        ref.reset_timing()
    assert counts["volume"] == 0                        # the feature off: nothing launched for it
    for fam in FAMILIES:
        assert sim.timing(fam)[1] == counts[fam], fam   # the other families' counts are unchanged by the log
    for f in (F.DENS, F.VX, F.VY, F.VZ, F.PRESSURE):
        assert bits_equal(sim.get(f), ref.get(f)), F.FIELD_NAMES[f]
    assert len(np.unique(images[0][2].reshape(-1, 3), axis=0)) > 3, "the density frame shows the plume"
    ref.close()
    sim.close()


def test_log_ring_overwrite_sample_and_clearing():
    import fluid_simulation_amd as F
    C = F._lib.C
    grid = W, H, D = 12, 6, 5
    sim = sim_of(W, H, D, acc=2, volume_log=3)
    views = log_setup(sim, F, grid)
    for _ in range(5):
        sim.run_one()
    n, dropped = C.c_long(), C.c_long()
    assert sim._L.fs_volume_log(sim._h, None, None, 0, C.byref(n), C.byref(dropped)) == 0
    assert (n.value, dropped.value) == (3, 2)                # frames = NULL: the counts only, nothing drained
    steps, images, dropped = sim.volume_log(with_dropped=True)
    assert steps.tolist() == [3, 4, 5] and dropped == 2
    last = sim.volume_render(views[0][0], views[0][1], **views[0][2])
    assert np.array_equal(images[0][2], last)
    # fs_volume_sample: a frame of the state as it is now, with the current step number
    sim.volume_sample()
    sim.volume_sample()
    steps, images = sim.volume_log()
    assert steps.tolist() == [5, 5] and np.array_equal(images[0][0], last) and np.array_equal(images[0][1], last)
    # setting the views, the rays of a slot in use, or the option clears the log; volume_every can change at any time
    sim.run_one()
    sim.set_volume_views(views[:1])
    assert sim.volume_log()[0].size == 0 and sim.volume_frame_bytes == 3 * 19 * 13
    sim.run_one()
    sim.volume_rays(2, M.camera_rays(outside_camera(grid), 3, 2))        # slot 2 is used by no view any more: the log stays
    assert sim._L.fs_volume_log(sim._h, None, None, 0, C.byref(n), None) == 0 and n.value == 1
    sim.volume_camera(0, outside_camera(grid)[0:3], outside_camera(grid)[3:6], size=(7, 5))   # in use: cleared, a new frame size
    assert sim.volume_log()[0].size == 0 and sim.volume_frame_bytes == 3 * 7 * 5
    sim.run_one()
    steps, images = sim.volume_log()
    assert steps.tolist() == [8] and np.array_equal(images[0][0], sim.volume_render(views[0][0], 0, **views[0][2]))
    sim.run_one()
    sim.set_option("volume_log", 4)
    assert sim.volume_log()[0].size == 0
    sim.set_option("volume_every", 3)
    for _ in range(4):                                       # steps 10 .. 13: (step - 1) % 3 == 0 at steps 10 and 13
        sim.run_one()
    steps, images = sim.volume_log()
    assert steps.tolist() == [10, 13] and len(images) == 1
    # a custom table takes effect in the log
    table = np.array([[1, 2, 3], [250, 128, 7]], dtype=np.uint8)
    sim.set_colormap(table)
    sim.set_option("volume_every", 1)
    sim.run_one()
    steps, images = sim.volume_log()
    rays = M.camera_rays(outside_camera(grid)[:9] + [float(np.tan(np.deg2rad(np.float64(45.0)) / 2.0)), 0.0], 7, 5)
    want = M.render(rays, sim.get(F.DENS), sim.get(F.OBS), M.params(**views[0][2]), table)[0]
    assert steps.tolist() == [14] and np.array_equal(images[0][0], want)
    # a slot in use cannot be freed; no views, or no ring: off
    with pytest.raises(F.FluidsimError):
        sim.volume_rays(0, None)
    sim.set_volume_views([])
    sim.volume_rays(0, None)
    sim.run_one()
    assert sim.volume_log()[0].size == 0 and sim.volume_view_count == 0
    with pytest.raises(F.FluidsimError):
        sim.volume_sample()
    sim.close()


# ---- 4. simulation.out --volume -------------------------------------------------------------------------------------------------

def test_cli_volume_pngs_match_python(tmp_path):
    import fluid_simulation_amd as F
    exe = os.path.join(ROOT, "simulation.out")
    assert os.path.exists(exe), "simulation.out is built by __graft_entry__.build()"
    stl = os.path.join(GOLDEN, "sphere_24x12.stl")
    out = tmp_path / "vol"
    env = {k: v for k, v in os.environ.items() if not k.startswith("FS_")}
    subprocess.run([exe, "--grid", "32x16x16", "--steps", "5", "--stl", stl + ",0.5,0,0,0,-4,0,0", "--dump-every", "0", "--dump-dir",
                    str(tmp_path), "--quiet", "--volume", str(out), "--volume-view", "30,20,60", "--volume-size", "19x13",
                    "--volume-range", "0,0.005", "--volume-opacity", "0.5", "--volume-every", "2"],
                   check=True, cwd=str(tmp_path), env=env, timeout=600)
    assert sorted(os.listdir(out)) == ["1.png", "3.png", "5.png"]
    sim = F.Simulation(32, 16, 16, 5, quiet=1, dump_every=0)
    assert F.loadSTLIntoObstacles(stl, sim, 0.5, 0.0, 0.0, 0.0, -4.0, 0.0, 0.0) > 0
    rad = 3.14159265358979323846 / 180.0                     # the program's own arithmetic, through the same libm
    az, el, dist = 30.0 * rad, 20.0 * rad, 60.0
    centre = [0.5 * 33, 0.5 * 17, 0.5 * 17]
    cam = [centre[0] - dist * math.cos(el) * math.sin(az), centre[1] + dist * math.sin(el), centre[2] + dist * math.cos(el) * math.cos(az)] + \
        centre + [0.0, 1.0, 0.0, math.tan(22.5 * rad), 0.0]
    F._lib.check(sim._L.fs_volume_camera(sim._h, 0, np.array(cam, dtype=np.float64).ctypes.data, 19, 13))
    sim._volume_size[0] = (13, 19)
    seen = set()
    for step in range(1, 6):
        sim.run_one()
        if step % 2 == 1:
            want = sim.volume_render(F.DENS, 0, vmin=0.0, vmax=0.005, opacity=0.5, step=0.5, t_min=0.01)
            got, _ = image_model.parse_png((out / ("%d.png" % step)).read_bytes())
            assert np.array_equal(got, want), step
            seen |= {tuple(c) for c in got.reshape(-1, 3)}
    assert (26, 26, 26) in seen and len(seen) > 3            # the background, the sphere, the plume
    sim.close()


# ---- 5. errors -------------------------------------------------------------------------------------------------------------------

def test_errors():
    import ctypes as C
    import fluid_simulation_amd as F
    EINVAL = F._lib.EINVAL
    W, H, D = 8, 6, 5
    sim = sim_of(W, H, D)
    L, h = sim._L, sim._h
    rays = M.camera_rays(outside_camera((W, H, D)), 4, 3)
    par = np.array(M.params(), dtype=np.float64)
    rgb, acc = np.zeros(36, dtype=np.uint8), np.zeros(48)

    def render(source=F.DENS, slot=0, p=par, nb=36, na=48, with_rgb=True, with_acc=True):
        return L.fs_volume_render(h, source, slot, p.ctypes.data if p is not None else None, rgb.ctypes.data if with_rgb else None, nb,
                                  acc.ctypes.data if with_acc else None, na)

    assert render() == EINVAL and "holds no rays" in (L.fs_last_error() or b"").decode()          # an empty slot
    # the ray sets
    for slot in (-1, 4):
        assert L.fs_volume_rays(h, slot, rays.ctypes.data, 4, 3) == EINVAL
        assert L.fs_volume_camera(h, slot, np.array(outside_camera((W, H, D))).ctypes.data, 4, 3) == EINVAL
    for cols, rows in ((0, 3), (4, 0), (-1, 3), (2049, 1), (1, 2049)):
        assert L.fs_volume_rays(h, 0, rays.ctypes.data, cols, rows) == EINVAL, (cols, rows)
        assert L.fs_volume_camera(h, 0, np.array(outside_camera((W, H, D))).ctypes.data, cols, rows) == EINVAL, (cols, rows)
    assert L.fs_volume_camera(h, 0, np.array(outside_camera((W, H, D))).ctypes.data, 0, 0) == EINVAL
    assert L.fs_volume_rays(h, 0, None, 4, 3) == EINVAL and L.fs_volume_camera(h, 0, None, 4, 3) == EINVAL
    assert L.fs_volume_rays(h, 0, None, 0, 0) == 0                                  # freeing a free slot
    eye, target, up = [1.0, 2.0, 3.0], [4.0, 5.0, 6.0], [0.0, 1.0, 0.0]
    for cam in (eye + eye + up + [0.5, 0.0], eye + target + [3.0, 3.0, 3.0] + [0.5, 0.0], eye + target + up + [0.0, 0.0],
                eye + target + up + [float("nan"), 0.0], [float("inf")] + eye[1:] + target + up + [0.5, 0.0]):
        assert L.fs_volume_camera(h, 0, np.array(cam).ctypes.data, 4, 3) == EINVAL, cam
    assert L.fs_volume_rays(h, 0, rays.ctypes.data, 4, 3) == 0
    assert render() == 0 and render(with_rgb=False) == 0 and render(with_acc=False) == 0 and render(with_rgb=False, with_acc=False) == 0
    assert L.fs_volume_rays(h, 0, None, 0, 0) == 0 and render() == EINVAL            # freed
    assert L.fs_volume_rays(h, 0, rays.ctypes.data, 4, 3) == 0
    # sizes, slots, sources, parameters
    for nb, na in ((35, 48), (37, 48), (0, 48), (36, 47), (36, 0), (12, 48)):
        assert render(nb=nb, na=na) == EINVAL, (nb, na)
    assert render(nb=0, with_rgb=False) == 0 and render(na=0, with_acc=False) == 0   # the size of a NULL array is not looked at
    for slot in (-1, 1, 4):
        assert render(slot=slot) == EINVAL, slot
    assert render(p=None) == EINVAL
    for source in (-1, 11, 100, F.ISO_VORTEX | 5, F.ISO_VORTEX | 255, F.SAMPLE_STAT | 13, F.SAMPLE_STAT | F.ISO_VORTEX, 2048, 4096 | F.DENS):
        assert render(source=source) == EINVAL, source
    bad_pars = []
    for k, v in ((0, 1.0), (0, 2.0), (1, np.inf), (0, np.nan), (2, -0.1), (2, np.inf), (3, 0.0), (3, -1.0), (3, np.nan), (3, 7.0e-4),
                 (4, 1.0), (4, -0.01), (4, np.nan), (5, 255.5), (7, -1.0), (10, 256.0), (8, np.nan)):
        p = par.copy()
        p[k] = v
        bad_pars.append(p)
        assert render(p=p) == EINVAL, (k, v)
    p = par.copy()
    p[3] = 1.0e-3                                            # diag / step = 12.2 / 0.001 < 16384: legal
    assert render(p=p) == 0
    # a stat source follows fs_flow_stats_field's errors
    stat = F.SAMPLE_STAT | F.STAT_MEAN_VX
    assert render(source=stat) == EINVAL and "flow_stats" in (L.fs_last_error() or b"").decode()
    sim.set_option("flow_stats", "mean")
    assert render(source=F.SAMPLE_STAT | F.STAT_UU) == EINVAL and render(source=stat) == EINVAL     # no samples yet
    assert render(source=stat | F.STAT_RAW) == 0
    sim.flow_stats_sample()
    assert render(source=stat) == 0
    # the views: everything is validated at the call, and a refused call leaves the list as it was
    good = np.array([[F.DENS, 0], [F.VX, 0]], dtype=np.intc)
    pars = np.tile(par, (5, 1))
    assert L.fs_volume_views(h, good.ctypes.data, pars.ctypes.data, 2) == 0 and sim.volume_view_count == 2
    for bad in ([11, 0], [F.DENS, 4], [F.DENS, -1], [F.DENS, 1], [F.SAMPLE_STAT | 13, 0]):        # slot 1 holds no rays
        spec = good.copy()
        spec[1] = bad
        assert L.fs_volume_views(h, spec.ctypes.data, pars.ctypes.data, 2) == EINVAL, bad
    for p in bad_pars:
        p2 = pars.copy()
        p2[1] = p
        assert L.fs_volume_views(h, good.ctypes.data, p2.ctypes.data, 2) == EINVAL, p
    many = np.tile(good[:1], (5, 1))
    assert L.fs_volume_views(h, many.ctypes.data, pars.ctypes.data, 5) == EINVAL
    assert L.fs_volume_views(h, many.ctypes.data, pars.ctypes.data, -1) == EINVAL
    assert L.fs_volume_views(h, None, None, 2) == EINVAL
    assert sim.volume_view_count == 2
    assert L.fs_volume_views(h, many.ctypes.data, pars.ctypes.data, 4) == 0 and sim.volume_view_count == 4
    assert L.fs_volume_rays(h, 0, None, 0, 0) == EINVAL and "used by a view" in (L.fs_last_error() or b"").decode()
    assert L.fs_volume_views(h, good.ctypes.data, pars.ctypes.data, 2) == 0
    # the options
    for bad in ("-1", "65537", "x", ""):
        assert L.fs_set_option(h, b"volume_log", bad.encode()) == EINVAL, bad
    for bad in ("0", "-3", "x"):
        assert L.fs_set_option(h, b"volume_every", bad.encode()) == EINVAL, bad
    assert L.fs_set_option(h, b"volume_log", b"65536") == 0                      # 65536 frames of 72 bytes
    # the drain
    assert L.fs_set_option(h, b"volume_log", b"4") == 0
    for _ in range(3):
        sim.run_one()
    n = C.c_long()
    frames = np.zeros(3 * sim.volume_frame_bytes, dtype=np.uint8)
    assert L.fs_volume_log(h, frames.ctypes.data, None, 2, C.byref(n), None) == EINVAL and n.value == 3    # max_frames < n_frames
    assert L.fs_volume_log(h, frames.ctypes.data, None, 3, C.byref(n), None) == 0
    assert L.fs_volume_log(h, None, None, 0, C.byref(n), None) == 0 and n.value == 0
    assert L.fs_volume_sample(None) == EINVAL and L.fs_volume_rays(None, 0, None, 0, 0) == EINVAL
    assert L.fs_volume_camera(None, 0, None, 1, 1) == EINVAL and L.fs_volume_render(None, 0, 0, None, None, 0, None, 0) == EINVAL
    assert L.fs_volume_views(None, None, None, 0) == EINVAL and L.fs_volume_log(None, None, None, 0, None, None) == EINVAL
    sim.close()
    # the ring's size limit: N x frame bytes over 1 GiB, from every side
    big = sim_of(8, 8, 4)
    wide = np.zeros((600, 600, 6))                           # 600 x 600 x 3 = 1080000 bytes a frame: 994 fit 1 GiB
    big.volume_rays(0, wide)
    spec = np.array([[F.DENS, 0]], dtype=np.intc)
    assert big._L.fs_volume_views(big._h, spec.ctypes.data, pars.ctypes.data, 1) == 0
    assert big._L.fs_set_option(big._h, b"volume_log", b"995") == EINVAL
    assert big._L.fs_set_option(big._h, b"volume_log", b"994") == 0
    two = np.tile(spec, (2, 1))
    assert big._L.fs_volume_views(big._h, two.ctypes.data, pars.ctypes.data, 2) == EINVAL and big.volume_view_count == 1
    wider = np.zeros((601, 600, 6))
    assert big._L.fs_volume_rays(big._h, 0, wider.ctypes.data, 600, 601) == EINVAL      # the slot in use would outgrow the ring
    assert big.volume_frame_bytes == 1080000
    assert big._L.fs_volume_rays(big._h, 1, wider.ctypes.data, 600, 601) == 0           # a slot no view uses
    big.close()
    # slab handles
    sim = sim_of(8, 8, 8)
    sim.comm_init(0, 2, b"FSNULL:".ljust(128, b"\0"))
    for rc in (sim._L.fs_volume_rays(sim._h, 0, rays.ctypes.data, 4, 3),
               sim._L.fs_volume_camera(sim._h, 0, np.array(outside_camera((8, 8, 8))).ctypes.data, 4, 3),
               sim._L.fs_volume_render(sim._h, F.DENS, 0, par.ctypes.data, rgb.ctypes.data, 36, None, 0),
               sim._L.fs_volume_views(sim._h, good.ctypes.data, pars.ctypes.data, 2),
               sim._L.fs_set_option(sim._h, b"volume_log", b"4")):
        assert rc == EINVAL and "single-GPU" in (sim._L.fs_last_error() or b"").decode()
    with pytest.raises(F.FluidsimError):
        sim.volume_sample()
    sim.close()
    sim = sim_of(8, 8, 8, volume_log=2)
    with pytest.raises(F.FluidsimError):
        sim.comm_init(0, 2, b"FSNULL:".ljust(128, b"\0"))
    sim.close()
