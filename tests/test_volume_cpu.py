"""The arithmetic of the volume renderer (csrc/volume.h), on the host: a driver compiled with the host C++ compiler and
-ffp-contract=off (the library's own setting) runs exactly the inline functions the ray-march kernel and fs_volume_camera call
-- the camera's rays, the parameter check with its loop limit, and whole rays through small volumes -- and every result is
compared bit for bit with the Python fp64 restatement in tests/volume_model.py, which is written from the definition in
include/fluidsim.h.  Also closed forms that need no model, and the constants of the ctypes layer against the header.  No
tolerance anywhere."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import volume_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "fluid_simulation_amd", "csrc")
HEADER = os.path.join(ROOT, "include", "fluidsim.h")
GOLDEN = os.path.join(ROOT, "tests", "golden")
TABLE = np.load(os.path.join(GOLDEN, "gui_density_cmap_256.npy"), allow_pickle=False)

# stdin, one job after the other, numbers as hex bit patterns unless noted:
#   "cam <cols> <rows>" (decimal), 11 camera entries -> "0", or "1" and then one line of 6 numbers per ray
#   "par <W> <H> <D>" (decimal), 11 parameters -> "<ok 0|1> <kmax decimal>"
#   "ray <elem 4|8|84> <W> <H> <D> <n> <rays>" (decimal; 84: an fp64 source over fp32 obs), 11 parameters, 3 n table bytes
#       (decimal), the source and then obs, (D+2)(H+2)(W+2) values each, then 6 numbers per ray
#       -> per ray: acc[4], then r g b (decimal)
DRIVER = r'''
#include "volume.h"
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
using namespace fs;
template <class T> static T rd()
{
    unsigned long long b;
    if (std::scanf("%llx", &b) != 1) std::exit(3);
    T v;
    if (sizeof(T) == 4) { uint32_t bb = (uint32_t)b; std::memcpy(&v, &bb, 4); } else { uint64_t bb = b; std::memcpy(&v, &bb, 8); }
    return v;
}
static void put(double v) { uint64_t b; std::memcpy(&b, &v, 8); std::printf(" %016llx", (unsigned long long)b); }
template <class E, class O> static int rays(int W, int H, int D, int n, int count)
{
    VolumeView vw = {};
    for (int k = 0; k < VOLUME_PARAMS; ++k) vw.par[k] = rd<double>();
    if (!volume_params_ok(vw.par, W, H, D, &vw.kmax)) return 2;
    vw.W = W; vw.H = H; vw.D = D; vw.py = W + 2; vw.pz = (long)(W + 2) * (H + 2); vw.n = n;
    std::vector<uint8_t> table(3 * (size_t)n);
    for (uint8_t& b : table) { int t; if (std::scanf("%d", &t) != 1) return 2; b = (uint8_t)t; }
    const size_t cells = (size_t)(W + 2) * (H + 2) * (D + 2);
    std::vector<E> src(cells);
    std::vector<O> obs(cells);
    for (E& x : src) x = rd<E>();
    for (O& x : obs) x = rd<O>();
    for (int k = 0; k < count; ++k) {
        double ray[6], acc[4];
        uint8_t rgb[3];
        for (double& x : ray) x = rd<double>();
        volume_ray<E, O>(ray, src.data(), obs.data(), vw, table.data(), acc, rgb);
        for (double a : acc) put(a);
        std::printf(" %d %d %d\n", rgb[0], rgb[1], rgb[2]);
    }
    return 0;
}
int main()
{
    char job[16];
    while (std::scanf("%15s", job) == 1) {
        if (!std::strcmp(job, "cam")) {
            int cols, rows;
            if (std::scanf("%d %d", &cols, &rows) != 2) return 2;
            double cam[11];
            for (double& x : cam) x = rd<double>();
            VolumeCamera c;
            if (!volume_camera_basis(cam, c)) { std::printf("0\n"); continue; }
            std::printf("1\n");
            for (int i = 0; i < rows; ++i)
                for (int j = 0; j < cols; ++j) {
                    double ray[6];
                    volume_camera_ray(c, cols, rows, i, j, ray);
                    for (double x : ray) put(x);
                    std::printf("\n");
                }
        } else if (!std::strcmp(job, "par")) {
            int W, H, D;
            if (std::scanf("%d %d %d", &W, &H, &D) != 3) return 2;
            double par[VOLUME_PARAMS];
            for (double& x : par) x = rd<double>();
            long kmax = -1;
            const bool ok = volume_params_ok(par, W, H, D, &kmax);
            std::printf("%d %ld\n", ok ? 1 : 0, ok ? kmax : -1L);
        } else if (!std::strcmp(job, "ray")) {
            int elem, W, H, D, n, count;
            if (std::scanf("%d %d %d %d %d %d", &elem, &W, &H, &D, &n, &count) != 6 || n < 2 || n > IMG_TABLE_MAX) return 2;
            const int rc = elem == 4 ? rays<float, float>(W, H, D, n, count)
                         : elem == 8 ? rays<double, double>(W, H, D, n, count) : rays<double, float>(W, H, D, n, count);
            if (rc) return rc;
        } else if (!std::strcmp(job, "consts")) {
            std::printf("%d %d %d %d\n", VOLUME_PARAMS, VOLUME_CAMERAS_MAX, VOLUME_VIEWS_MAX, VOLUME_SAMPLES_MAX);
        } else {
            return 2;
        }
    }
    return 0;
}
'''


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.dtype.itemsize == 4 else np.uint64).reshape(-1)


def hexes(a):
    return " ".join("%x" % int(b) for b in bits(a))


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++")
    if cxx is None:
        pytest.fail("no C++ compiler")
    d = tmp_path_factory.mktemp("volume_cpu")
    src = d / "driver.cpp"
    src.write_text(DRIVER)
    exe = d / "driver"
    subprocess.run([cxx, "-std=c++17", "-O2", "-Wall", "-Werror", "-ffp-contract=off", "-I", CSRC, str(src), "-o", str(exe)],
                   check=True)

    def run(text):
        return subprocess.run([str(exe)], input=text, capture_output=True, text=True, check=True).stdout

    return run


def driver_camera(driver, cam, cols, rows):
    out = driver("cam %d %d\n%s\n" % (cols, rows, hexes(np.array(cam, dtype=np.float64)))).splitlines()
    if out[0] == "0":
        return None
    vals = np.array([[int(t, 16) for t in line.split()] for line in out[1:]], dtype=np.uint64)
    return vals.view(np.float64).reshape(rows, cols, 6)


def driver_rays(driver, rays, field, obs, par, table):
    """-> (rgb (n, 3) uint8, acc (n, 4) float64) of the rays (n, 6)"""
    field, obs = np.ascontiguousarray(field), np.ascontiguousarray(obs)
    D, H, W = (n - 2 for n in field.shape)
    elem = 4 if field.dtype == np.float32 else (8 if obs.dtype == np.float64 else 84)
    rays = np.ascontiguousarray(rays, dtype=np.float64).reshape(-1, 6)
    text = "ray %d %d %d %d %d %d\n%s\n%s\n%s\n%s\n%s\n" % (
        elem, W, H, D, table.shape[0], rays.shape[0], hexes(np.array(par, dtype=np.float64)),
        " ".join(str(int(b)) for b in table.reshape(-1)), hexes(field), hexes(obs), hexes(rays))
    lines = [line.split() for line in driver(text).splitlines()]
    acc = np.array([[int(t, 16) for t in line[:4]] for line in lines], dtype=np.uint64).view(np.float64).reshape(-1, 4)
    rgb = np.array([[int(t) for t in line[4:]] for line in lines], dtype=np.uint8).reshape(-1, 3)
    return rgb, acc


def random_field(rng, shape, dtype, nan=True):
    """magnitudes spread over decades around the colour range; some NaN and infinite cells"""
    a = (np.abs(rng.standard_normal(shape)) * 10.0 ** rng.integers(-3, 1, size=shape)).astype(dtype)
    a[rng.random(shape) < 0.1] = 0.0
    a[rng.random(shape) < 0.05] *= -1
    if nan:
        a[rng.random(shape) < 0.01] = np.nan
        a[rng.random(shape) < 0.003] = np.inf
        a[rng.random(shape) < 0.003] = -np.inf
    return a


def random_obs(rng, W, H, D, dtype, p=0.03):
    o = np.zeros((D + 2, H + 2, W + 2), dtype=dtype)
    o[1:-1, 1:-1, 1:-1] = (rng.random((D, H, W)) < p).astype(dtype)
    o[1:3, 1:3, 1:3] = 1                                 # a block against three walls: normals of every n2
    o[2, 2, 3] = 0.5                                     # not solid
    o[2, 3, 3] = 0.75                                    # solid
    o[D, H, W] = 0                                       # fluid: the cell random_field's caller makes NaN
    return o


CAMERAS = [
    # eye, target, up, half_height, ortho
    ([60.0, 40.0, 70.0], [19.0, 11.0, 9.5], [0.0, 1.0, 0.0], 0.41421356237309503, 0.0),
    ([-30.0, 5.0, 4.0], [10.0, 6.0, 5.0], [0.0, 0.0, 1.0], 0.2, 0.0),
    ([7.0, 5.0, 3.0], [20.0, 9.0, 8.0], [0.1, 1.0, -0.2], 1.0, 0.0),                    # from inside a box
    ([60.0, 40.0, 70.0], [19.0, 11.0, 9.5], [0.0, 1.0, 0.0], 14.0, 1.0),                # orthographic
    ([10.0, 80.0, 9.0], [10.0, 0.0, 9.0], [1.0, 0.0, 0.0], 9.5, 1.0),                   # straight down
]


# ---- 1. camera rays ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("size", [(1, 1), (7, 5), (19, 13), (2, 9)], ids=lambda s: "%dx%d" % s)
def test_camera_rays_match_model(driver, size):
    cols, rows = size
    for eye, target, up, half, ortho in CAMERAS:
        cam = eye + target + up + [half, ortho]
        got, want = driver_camera(driver, cam, cols, rows), M.camera_rays(cam, cols, rows)
        assert got is not None and M.same_bits(got, want), (cam, size)
        # the direction has unit length up to rounding, the central pixel of an odd image looks at the target
        assert np.abs(np.sqrt((got[..., 3:] ** 2).sum(axis=2)) - 1.0).max() < 1e-15
    got = driver_camera(driver, CAMERAS[0][0] + CAMERAS[0][1] + CAMERAS[0][2] + [0.5, 0.0], 5, 3)
    f = np.array(CAMERAS[0][1]) - np.array(CAMERAS[0][0])
    assert np.abs(got[1, 2, 3:] - f / np.sqrt((f * f).sum())).max() < 1e-15
    assert got[0, 2, 4] > got[2, 2, 4] and np.array_equal(got[..., :3], np.broadcast_to(CAMERAS[0][0], (3, 5, 3)))   # row 0 is the top


def test_camera_errors(driver):
    eye, target, up = [1.0, 2.0, 3.0], [4.0, 5.0, 6.0], [0.0, 1.0, 0.0]
    bad = [eye + eye + up + [0.5, 0.0],                                 # target == eye
           eye + target + [3.0, 3.0, 3.0] + [0.5, 0.0],                 # up along the view direction
           eye + target + [0.0, 0.0, 0.0] + [0.5, 0.0],
           eye + target + up + [0.0, 0.0], eye + target + up + [-1.0, 1.0],
           [float("nan")] + eye[1:] + target + up + [0.5, 0.0], eye + target + up + [float("inf"), 0.0],
           eye + target + up + [0.5, float("nan")], eye + [1e200, 5.0, 6.0] + up + [0.5, 0.0]]   # F.F overflows
    for cam in bad:
        assert driver_camera(driver, cam, 3, 2) is None and M.camera_rays(cam, 3, 2) is None, cam


# ---- 2. parameters -----------------------------------------------------------------------------------------------------------------

def test_params_and_loop_limit(driver):
    good = M.params(vmin=-1.0, vmax=2.0, opacity=0.3, step=0.25, t_min=0.05)
    cases = [good, M.params(step=1.0e-2), M.params(opacity=0.0, t_min=0.0), M.params(step=300.0)]
    for k, v in ((0, 2.0), (1, float("inf")), (0, float("nan")), (2, -0.1), (2, float("inf")), (3, 0.0), (3, -1.0), (3, float("nan")),
                 (4, 1.0), (4, -0.01), (5, 255.5), (7, -1.0), (10, 256.0), (8, float("nan")), (3, 1.0e-3)):
        p = list(good)
        p[k] = v
        cases.append(p)
    for W, H, D in ((37, 21, 18), (5, 3, 4), (512, 512, 512)):
        for p in cases:
            ok, kmax = (int(t) for t in driver("par %d %d %d\n%s\n" % (W, H, D, hexes(np.array(p)))).split())
            want = M.kmax_of(p, W, H, D)
            assert (ok, kmax) == ((1, want) if want is not None else (0, -1)), (W, H, D, p)
    assert M.kmax_of(good, 37, 21, 18) is not None and M.kmax_of(M.params(step=1.0e-3), 37, 21, 18) is None
    # the largest legal sample count: diag / step == 16384 exactly
    assert M.kmax_of(M.params(step=3.0 / 16384.0), 1, 1, 0) == 16386 and M.kmax_of(M.params(step=2.9999 / 16384.0), 1, 1, 0) is None


# ---- 3. ray against box, whole marches ---------------------------------------------------------------------------------------

def test_special_rays_cover_the_box_classes():
    W, H, D = 9, 6, 5
    rays = M.special_rays(W, H, D)
    got = [M.box(r[:3], r[3:], (W, H, D)) if all(M.finite(x) for x in r) and any(x != 0 for x in r[3:]) else "invalid"
           for r in rays.tolist()]
    assert sum(1 for g in got if g == "invalid") == 6 and sum(1 for g in got if g is None) >= 6
    assert got[-1] is None                                   # exact grazing: t0 == t1 is a miss
    t = M.box([-1.0, 1.0, 3.0], [1.0, -1.0, 0.0], (W, H, D))
    assert t is None
    hits = [g for g in got if g not in (None, "invalid")]
    assert any(g[0] == 0.0 for g in hits) and any(g[0] > 0.0 for g in hits) and any(g[1] == M.INF for g in hits)


@pytest.mark.parametrize("dtypes", [(np.float32, np.float32), (np.float64, np.float64), (np.float64, np.float32)],
                         ids=["fp32", "fp64", "fp64-over-fp32"])
@pytest.mark.parametrize("grid", [(9, 6, 5), (3, 2, 1)], ids=lambda g: "x".join(map(str, g)))
def test_marches_match_model(driver, grid, dtypes):
    W, H, D = grid
    rng = np.random.default_rng(W * 100 + D + dtypes[0]().itemsize)
    field = random_field(rng, (D + 2, H + 2, W + 2), dtypes[0])
    obs = random_obs(rng, W, H, D, dtypes[1])
    field[D, H, W] = np.nan                              # at least one NaN sample on the tiny grid too
    custom = rng.integers(0, 256, size=(7, 3)).astype(np.uint8)
    cam = M.camera_rays([2.6 * W, 1.9 * H, 3.1 * D] + [0.5 * W, 0.5 * H, 0.5 * D] + [0.0, 1.0, 0.0] + [0.45, 0.0], 9, 7).reshape(-1, 6)
    inside = M.camera_rays([0.7 * W, 0.6 * H, 0.5 * D] + [0.0, 0.0, 0.0] + [0.0, 0.0, 1.0] + [0.8, 0.0], 5, 4).reshape(-1, 6)
    rand = np.concatenate([rng.uniform(-3.0, max(grid) + 4.0, size=(40, 3)), rng.standard_normal((40, 3))], axis=1)
    rays = np.concatenate([M.special_rays(W, H, D), cam, inside, rand])
    seen = 0
    for par, table in ((M.params(0.0, 0.5, 0.4, 0.5, 0.0), TABLE), (M.params(-0.1, 0.3, 6.0, 0.25, 0.2, (200, 90, 10), (3, 250, 77)), custom),
                       (M.params(0.0, 1.0, 0.0, 0.7, 0.5), TABLE)):
        got_rgb, got_acc = driver_rays(driver, rays, field, obs, par, table)
        rgb, acc, cls = M.render(rays.reshape(1, -1, 6), field, obs, par, table)
        bad = np.argwhere(~(got_acc.view(np.uint64) == acc[0].view(np.uint64)).all(axis=1))[:6]
        assert M.same_bits(got_acc, acc[0]), (grid, par[:5], bad, got_acc[bad[:2, 0]], acc[0][bad[:2, 0]])
        assert np.array_equal(got_rgb, rgb[0]), (grid, par[:5])
        seen |= int(np.bitwise_or.reduce(cls.reshape(-1)))
        miss = (cls[0] & (M.MISS | M.INVALID)) != 0
        assert np.array_equal(acc[0][miss], np.tile([0.0, 0.0, 0.0, 1.0], (miss.sum(), 1)))
    # the rays exercised every path
    for bit in (M.INVALID, M.MISS, M.EXIT, M.SOLID, M.EARLY, M.NAN_SKIPPED, M.CUT):
        assert seen & bit, bit


# ---- 4. closed forms ----------------------------------------------------------------------------------------------------------

def test_closed_forms(driver):
    W, H, D = 8, 5, 4
    shape = (D + 2, H + 2, W + 2)
    zero = np.zeros(shape, dtype=np.float32)
    rays = np.concatenate([M.special_rays(W, H, D), M.camera_rays([30.0, 20.0, 25.0, 4.0, 3.0, 2.0, 0.0, 1.0, 0.0, 0.3, 0.0], 6, 5).reshape(-1, 6)])
    # a field equal to vmin everywhere: exactly the background, T = 1
    par = M.params(0.25, 1.0, 5.0, 0.5, 0.1, (1, 2, 3), (17, 200, 255))
    rgb, acc = driver_rays(driver, rays, np.full(shape, 0.25, dtype=np.float32), zero, par, TABLE)
    assert np.array_equal(rgb, np.tile(np.array([17, 200, 255], dtype=np.uint8), (len(rays), 1)))
    assert np.array_equal(acc, np.tile([0.0, 0.0, 0.0, 1.0], (len(rays), 1)))
    # a uniform field along an axis-parallel ray: T is the sequential product (1 - a)^n, n = the samples with tk < t1
    v, vmin, vmax, opacity, step = 0.75, 0.0, 1.0, 0.125, 0.5
    par = M.params(vmin, vmax, opacity, step, 0.0)
    ray = np.array([[-2.0, 2.5, 2.5, 1.0, 0.0, 0.0]])
    rgb, acc = driver_rays(driver, ray, np.full(shape, v, dtype=np.float64), zero.astype(np.float64), par, TABLE)
    a = (opacity * ((v - vmin) / (vmax - vmin))) * step
    n = 2 * (W + 1)                                          # t0 = 2, t1 = W + 3, samples at 2.25, 2.75, ..
    T = 1.0
    col = TABLE[min(255, int(((v - vmin) / (vmax - vmin)) * 256.0))].astype(np.float64)
    C = np.zeros(3)
    for _ in range(n):
        C = C + (T * a) * col
        T = T * (1.0 - a)
    assert acc[0, 3] == T and np.array_equal(acc[0, :3], C) and 0.0 < T < 1.0
    # an axis-aligned wall hit head-on: shade = 1, the obstacle colour exactly
    wall = zero.copy()
    wall[:, :, 5:] = 1.0
    par = M.params(0.0, 1.0, 1.0, 0.5, 0.0, (201, 102, 53), (9, 9, 9))
    ray = np.array([[-1.0, 2.5, 2.5, 1.0, 0.0, 0.0], [-1.0, 2.5, 2.5, 2.0, 0.0, 0.0], [-1.0, 2.5, 0.5, 0.96, 0.0, 0.28]])
    rgb, acc = driver_rays(driver, ray, zero, wall, par, TABLE)
    assert np.array_equal(rgb[0], [201, 102, 53]) and np.array_equal(acc[0], [201.0, 102.0, 53.0, 0.0])
    assert np.array_equal(rgb[1], [201, 102, 53])            # |d| = 2: the shade is capped at 1
    s = 0.3 + 0.7 * (abs(0.96) * 1.0)                        # oblique: 0.3 + 0.7 |n.d|
    assert np.array_equal(acc[2], [201.0 * s, 102.0 * s, 53.0 * s, 0.0])


# ---- 5. constants --------------------------------------------------------------------------------------------------------------

def test_constants_match_header(driver):
    from fluid_simulation_amd import _lib
    text = open(HEADER).read()

    def define(name):
        return int(re.search(r"#define\s+%s\s+(\d+)" % name, text).group(1))

    for name, model, mirror in (("FS_VOLUME_PARAMS", M.PARAMS, _lib.VOLUME_PARAMS), ("FS_VOLUME_CAMERAS_MAX", M.CAMERAS_MAX, _lib.VOLUME_CAMERAS_MAX),
                                ("FS_VOLUME_VIEWS_MAX", M.VIEWS_MAX, _lib.VOLUME_VIEWS_MAX), ("FS_VOLUME_CAMERA", M.CAMERA, _lib.VOLUME_CAMERA),
                                ("FS_VOLUME_SAMPLES_MAX", M.SAMPLES_MAX, _lib.VOLUME_SAMPLES_MAX)):
        assert define(name) == model == mirror, name
    assert [int(t) for t in driver("consts\n").split()] == [M.PARAMS, M.CAMERAS_MAX, M.VIEWS_MAX, M.SAMPLES_MAX]
    for name in ("fs_volume_rays", "fs_volume_camera", "fs_volume_render", "fs_volume_views", "fs_volume_sample", "fs_volume_log"):
        assert name in _lib.exported_symbols() and re.search(r"\bint %s\(fs_sim\* s" % name, text), name
    assert len(M.params()) == M.PARAMS
