"""The arithmetic of the slice and projection images (csrc/image.h), on the host: a driver compiled with the host C++ compiler
and -ffp-contract=off (the library's own setting) runs exactly the inline functions the image kernels call -- the sequential
sum / max / min / silhouette step and the colouring -- over seeded random columns and values, float and double, and every
result is compared bit for bit with the numpy fp64 restatement in tests/image_model.py, which is written from the definition
in include/fluidsim.h.  Also: the built-in colour table and the model against bytes recorded from matplotlib
(tools/make_image_goldens.py), live against matplotlib where it is installed, fs_image_png through ctypes (it needs no GPU),
and the constants of the ctypes layer against the header.  No tolerance anywhere."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import image_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "fluid_simulation_amd", "csrc")
HEADER = os.path.join(ROOT, "include", "fluidsim.h")
GOLDEN = os.path.join(ROOT, "tests", "golden")

# stdin, one job after the other, numbers as hex bit patterns unless noted:
#   "col <elem 4|8> <columns> <cells>", then columns x cells values -> per column: sum max min any
#   "rgb <n> <count>" (decimal), vmin vmax alpha, then 3 n table bytes (decimal), then count x (value, flag 0|1) -> r g b
#   "table" -> the built-in table, 768 decimal bytes
DRIVER = r'''
#include "image.h"
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
template <int KIND, class E> static double reduce(const E* v, int n)
{
    double a = image_start<KIND>();
    for (int k = 0; k < n; ++k) a = image_step<KIND, E>(a, v[k]);
    return a;
}
template <class E> static void columns(int ncol, int n)
{
    std::vector<E> v((size_t)n);
    for (int c = 0; c < ncol; ++c) {
        for (E& x : v) x = rd<E>();
        put(reduce<IMG_SUM>(v.data(), n));
        put(reduce<IMG_MAX>(v.data(), n));
        put(reduce<IMG_MIN>(v.data(), n));
        put(reduce<IMG_ANY>(v.data(), n));
        std::printf("\n");
    }
}
int main()
{
    char job[16];
    while (std::scanf("%15s", job) == 1) {
        if (!std::strcmp(job, "col")) {
            int elem, ncol, n;
            if (std::scanf("%d %d %d", &elem, &ncol, &n) != 3) return 2;
            if (elem == 4) columns<float>(ncol, n); else columns<double>(ncol, n);
        } else if (!std::strcmp(job, "rgb")) {
            int n, count;
            if (std::scanf("%d %d", &n, &count) != 2 || n < 2 || n > IMG_TABLE_MAX) return 2;
            const double vmin = rd<double>(), vmax = rd<double>(), alpha = rd<double>();
            std::vector<uint8_t> table(3 * (size_t)n);
            for (uint8_t& b : table) { int t; if (std::scanf("%d", &t) != 1) return 2; b = (uint8_t)t; }
            for (int k = 0; k < count; ++k) {
                const double v = rd<double>();
                int flag;
                if (std::scanf("%d", &flag) != 1) return 2;
                uint8_t c[3];
                image_colour(v, flag != 0, vmin, vmax, alpha, table.data(), n, c);
                std::printf("%d %d %d\n", c[0], c[1], c[2]);
            }
        } else if (!std::strcmp(job, "table")) {
            for (int k = 0; k < 3 * IMG_DEFAULT_N; ++k) std::printf("%d ", IMG_DEFAULT_TABLE[k]);
            std::printf("\n");
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
    d = tmp_path_factory.mktemp("image_cpu")
    src = d / "driver.cpp"
    src.write_text(DRIVER)
    exe = d / "driver"
    subprocess.run([cxx, "-std=c++17", "-O2", "-Wall", "-Werror", "-ffp-contract=off", "-I", CSRC, str(src), "-o", str(exe)],
                   check=True)

    def run(text):
        return subprocess.run([str(exe)], input=text, capture_output=True, text=True, check=True).stdout

    return run


def driver_columns(driver, cols):
    """cols: (columns, cells) -> (columns, 4) float64: sum, max, min, any"""
    out = driver("col %d %d %d\n%s\n" % (cols.dtype.itemsize, cols.shape[0], cols.shape[1], hexes(cols)))
    rows = np.array([[int(t, 16) for t in line.split()] for line in out.splitlines()], dtype=np.uint64)
    return rows.view(np.float64).reshape(cols.shape[0], 4)


def driver_colour(driver, val, flag, vmin, vmax, alpha, table):
    val = np.ascontiguousarray(val, dtype=np.float64).reshape(-1)
    flag = np.asarray(flag, dtype=bool).reshape(-1)
    head = "rgb %d %d\n%s\n%s\n" % (table.shape[0], val.size, hexes(np.array([vmin, vmax, alpha], dtype=np.float64)),
                                  " ".join(str(int(b)) for b in table.reshape(-1)))
    body = "\n".join("%x %d" % (int(b), int(f)) for b, f in zip(bits(val), flag))
    out = driver(head + body + "\n")
    return np.array([[int(t) for t in line.split()] for line in out.splitlines()], dtype=np.uint8).reshape(val.size, 3)


def random_field(rng, shape, dtype):
    """magnitudes spread over seven decades, so that the order of a sum matters; some zeros of both signs, NaN and infinities"""
    a = (rng.standard_normal(shape) * 10.0 ** rng.integers(-3, 4, size=shape)).astype(dtype)
    a[rng.random(shape) < 0.05] = 0.0
    a[rng.random(shape) < 0.03] = -0.0
    a[rng.random(shape) < 0.01] = np.nan
    a[rng.random(shape) < 0.004] = np.inf
    a[rng.random(shape) < 0.004] = -np.inf
    return a


# ---- 1. the column reductions ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("shape", [(7, 5, 4), (1, 1, 1), (33, 3, 9)], ids=lambda s: "x".join(map(str, s)))
def test_reductions_match_model(driver, dtype, shape):
    W, H, D = shape
    rng = np.random.default_rng(515 + W)
    field = random_field(rng, (D + 2, H + 2, W + 2), dtype)
    obs = (rng.random(field.shape) < 0.1).astype(dtype)
    obs[rng.random(field.shape) < 0.05] = dtype(0.5)         # exactly one half: not an obstacle
    obs[rng.random(field.shape) < 0.05] = dtype(0.75)
    for axis in (0, 1, 2):
        col = np.moveaxis(field, 2 - axis, 0)[1:-1]          # the interior cells of the axis, first
        ocol = np.moveaxis(obs, 2 - axis, 0)[1:-1]
        rows, cols = col.shape[1:]
        assert (rows, cols) == M.dims(axis, W, H, D)
        got = driver_columns(driver, np.ascontiguousarray(col.reshape(col.shape[0], -1).T))
        for kind, k in ((M.SUM, 0), (M.MAX, 1), (M.MIN, 2)):
            want = M.values(field, kind, axis)
            assert M.same_bits(got[:, k].reshape(rows, cols), want), (axis, M.KIND_NAMES[kind])
        silhouette = driver_columns(driver, np.ascontiguousarray(ocol.reshape(ocol.shape[0], -1).T))[:, 3].reshape(rows, cols)
        assert np.array_equal(silhouette != 0.0, M.flags(obs, M.SUM, axis))
        assert set(np.unique(silhouette)) <= {0.0, 1.0}


def test_reduction_edge_cases(driver):
    """+-0.0 ties keep the first, NaN is never taken, an all-NaN column keeps the start value, the sum starts from +0.0"""
    nan, inf = np.nan, np.inf
    cols = np.array([[-0.0, 0.0, -0.0, 0.0], [0.0, -0.0, 0.0, -0.0], [nan, nan, nan, nan], [nan, 2.0, nan, 1.0],
                     [-0.0, -0.0, -0.0, -0.0], [inf, -inf, 1.0, 2.0], [1e30, 1.0, -1e30, 1.0], [3.0, 3.0, 3.0, 3.0]])
    for dtype in (np.float32, np.float64):
        got = driver_columns(driver, cols.astype(dtype))
        field = np.zeros((3, 3, 6), dtype=dtype)             # W = 4, H = D = 1: the columns of axis x at y = z = 1
        for c, column in enumerate(cols):
            field[1, 1, 1:5] = column.astype(dtype)
            for kind, k in ((M.SUM, 0), (M.MAX, 1), (M.MIN, 2)):
                assert M.same_bits(got[c, k], M.values(field, kind, 0)[1, 1]), (dtype, c, kind)
        assert M.same_bits(got[0, 1:3], [-0.0, -0.0]) and M.same_bits(got[1, 1:3], [0.0, 0.0])     # the first of equal values stays
        assert M.same_bits(got[2, :3], [nan, -inf, inf])
        assert got[3, 1] == 2.0 and got[3, 2] == 1.0
        assert M.same_bits(got[4, 0], 0.0)                   # +0.0 + -0.0 ... = +0.0
        assert np.isnan(got[5, 0]) and got[5, 1] == inf and got[5, 2] == -inf
        assert got[6, 0] == 1.0                              # ((1e30 + 1) - 1e30) + 1: sequential, not pairwise


# ---- 2. the colouring -----------------------------------------------------------------------------------------------------------

def colour_values(rng, vmin, vmax, n):
    span = vmax - vmin
    edges = vmin + span * np.arange(0, n + 1, max(1, n // 64)) / n          # on bin edges
    v = np.concatenate([edges, np.nextafter(edges, -np.inf), np.nextafter(edges, np.inf),
                        vmin - 0.3 * span + 1.6 * span * rng.random(300),
                        [vmin, vmax, np.nan, np.inf, -np.inf, 0.0, -0.0, np.nextafter(vmax, np.inf), np.nextafter(vmin, -np.inf)]])
    return v.astype(np.float64)


@pytest.mark.parametrize("n", [2, 256, 4096])
def test_colouring_matches_model(driver, n):
    rng = np.random.default_rng(n)
    table = rng.integers(0, 256, size=(n, 3)).astype(np.uint8)
    table[0], table[-1] = (255, 255, 255), (1, 254, 3)
    for vmin, vmax in ((0.0, 0.01), (-10.0, 10.0), (-1.0, 1.0), (-3.7e-5, 1.3e7)):
        v = colour_values(rng, vmin, vmax, n)
        flag = rng.random(v.size) < 0.5
        for alpha in (0.0, 0.2, 1.0, 0.3333):
            got = driver_colour(driver, v, flag, vmin, vmax, alpha, table)
            want = M.colour(v, flag, vmin, vmax, alpha, table)
            assert np.array_equal(got, want), (n, vmin, vmax, alpha, np.flatnonzero((got != want).any(axis=1))[:8])
        top = driver_colour(driver, np.array([vmax, np.inf, vmin, -np.inf, np.nan]), np.zeros(5, bool), vmin, vmax, 0.0, table)
        assert np.array_equal(top, [table[-1], table[-1], table[0], table[0], (0, 0, 0)])


# ---- 3. the built-in table and the recorded matplotlib bytes ---------------------------------------------------------------------

def builtin_table(driver):
    return np.array([int(t) for t in driver("table\n").split()], dtype=np.uint8).reshape(256, 3)


def test_builtin_table_is_the_recorded_one(driver):
    t = builtin_table(driver)
    want = np.load(os.path.join(GOLDEN, "gui_density_cmap_256.npy"), allow_pickle=False)
    assert want.dtype == np.uint8 and want.shape == (256, 3)
    assert np.array_equal(t, want)
    assert tuple(t[0]) == (255, 255, 255) and tuple(t[127]) == (0, 190, 252) and tuple(t[255]) == (255, 0, 0)


def test_model_and_driver_give_the_recorded_bytes(driver):
    z = np.load(os.path.join(GOLDEN, "gui_slice_image.npz"), allow_pickle=False)
    table = np.load(os.path.join(GOLDEN, "gui_density_cmap_256.npy"), allow_pickle=False)
    data, obs, alpha = z["data"], z["obs"], float(z["alpha"])
    assert data.dtype == np.float32 and np.isnan(data).any() and np.isinf(data).any() and alpha == 0.2
    for k, (vmin, vmax) in enumerate(z["ranges"]):
        want = z["rgb_%d" % k]
        val = data.astype(np.float64)
        assert np.array_equal(M.colour(val, obs > 0.5, vmin, vmax, alpha, table), want), (vmin, vmax)
        got = driver_colour(driver, val, obs > 0.5, vmin, vmax, alpha, table).reshape(want.shape)
        assert np.array_equal(got, want), (vmin, vmax)


def test_live_against_matplotlib(driver):
    pytest.importorskip("matplotlib")
    from matplotlib.colors import LinearSegmentedColormap, Normalize
    cmap = LinearSegmentedColormap.from_list("density_cmap", ["white", "lightgreen", "green", "deepskyblue", "blue", "darkred", "red"])
    table = builtin_table(driver)
    assert np.array_equal((cmap(np.arange(256))[:, :3] * 255).astype(np.uint8), table)
    rng = np.random.default_rng(99)
    for vmin, vmax in ((0.0, 0.01), (-10.0, 10.0), (-1.0, 1.0), (0.37, 11.3)):
        v = colour_values(rng, vmin, vmax, 256).astype(np.float32).reshape(1, -1)       # the viewer's input is float32
        solid = rng.random(v.shape) < 0.4
        rgb = (cmap(Normalize(vmin=vmin, vmax=vmax, clip=True)(v))[..., :3] * 255).astype(np.uint8)
        rgb[solid] = (rgb[solid].astype(np.float32) * (1 - 0.2)).astype(np.uint8)
        assert np.array_equal(M.colour(v.astype(np.float64), solid, vmin, vmax, 0.2, table), rgb), (vmin, vmax)


# ---- 4. the PNG writer -------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def libpath():
    from fluid_simulation_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        subprocess.check_call(["make", "-C", CSRC, "-j4"])
    return _lib.LIB_PATH


@pytest.mark.parametrize("cols,rows", [(1, 1), (3, 2), (514, 66), (300, 80)], ids=lambda v: str(v))
def test_png_round_trip(libpath, tmp_path, cols, rows):
    lib = ctypes.CDLL(libpath)
    lib.fs_image_png.restype = ctypes.c_int
    lib.fs_image_png.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_char_p]
    rng = np.random.default_rng(cols * 1000 + rows)
    rgb = rng.integers(0, 256, size=(rows, cols, 3)).astype(np.uint8)
    path = tmp_path / "image.png"
    assert lib.fs_image_png(rgb.ctypes.data, cols, rows, os.fsencode(str(path))) == 0
    data = path.read_bytes()
    pixels, blocks = M.parse_png(data)
    assert np.array_equal(pixels, rgb)
    scan = rows * (1 + 3 * cols)
    assert blocks == (scan + 65534) // 65535
    if (cols, rows) in ((514, 66), (300, 80)):
        assert scan > 65535 and blocks > 1                   # more than one stored block
    # the bytes are a pure function of the pixels
    assert lib.fs_image_png(rgb.ctypes.data, cols, rows, os.fsencode(str(path))) == 0 and path.read_bytes() == data
    assert len(data) == 8 + 25 + 12 + (2 + 5 * blocks + scan + 4) + 12


def test_png_errors(libpath, tmp_path):
    lib = ctypes.CDLL(libpath)
    lib.fs_image_png.restype = ctypes.c_int
    lib.fs_image_png.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_char_p]
    rgb = np.zeros((2, 2, 3), dtype=np.uint8)
    ok = os.fsencode(str(tmp_path / "a.png"))
    assert lib.fs_image_png(None, 2, 2, ok) == -1 and lib.fs_image_png(rgb.ctypes.data, 2, 2, None) == -1
    assert lib.fs_image_png(rgb.ctypes.data, 0, 2, ok) == -1 and lib.fs_image_png(rgb.ctypes.data, 2, -1, ok) == -1
    assert lib.fs_image_png(rgb.ctypes.data, 2, 2, os.fsencode(str(tmp_path / "no" / "such" / "dir.png"))) == -2


def test_write_png_through_the_viewer_module(libpath, tmp_path):
    from fluid_simulation_amd import viewer
    rgb = np.arange(5 * 7 * 3, dtype=np.uint8).reshape(5, 7, 3)
    viewer.write_png(str(tmp_path / "v.png"), rgb)
    assert np.array_equal(M.parse_png((tmp_path / "v.png").read_bytes())[0], rgb)
    with pytest.raises(ValueError):
        viewer.write_png(str(tmp_path / "w.png"), rgb[:, :, 0])


# ---- 5. constants ---------------------------------------------------------------------------------------------------------------------

def test_python_constants_match_header():
    from fluid_simulation_amd import _lib, viewer
    import fluid_simulation_amd as F
    text = open(HEADER).read()
    enum = dict((k, int(v)) for k, v in re.findall(r"\b(FS_IMG_[A-Z]+)\s*=\s*(\d+)", text))
    assert enum == {"FS_IMG_SLICE": _lib.IMG_SLICE, "FS_IMG_SUM": _lib.IMG_SUM, "FS_IMG_MAX": _lib.IMG_MAX, "FS_IMG_MIN": _lib.IMG_MIN}
    assert (_lib.IMG_SLICE, _lib.IMG_SUM, _lib.IMG_MAX, _lib.IMG_MIN) == (0, 1, 2, 3) == (M.SLICE, M.SUM, M.MAX, M.MIN)
    assert int(re.search(r"#define\s+FS_IMAGE_VIEWS_MAX\s+(\d+)", text).group(1)) == _lib.IMAGE_VIEWS_MAX == 8
    assert _lib.IMG_KINDS == {"slice": 0, "sum": 1, "max": 2, "min": 3}
    for name in ("IMG_SLICE", "IMG_SUM", "IMG_MAX", "IMG_MIN", "IMAGE_VIEWS_MAX"):
        assert getattr(F, name) == getattr(_lib, name)
    # the 2-D viewer's defaults
    assert viewer.SLICE_RANGES == {"density": (_lib.DENS, 0.0, 0.01), "v_x": (_lib.VX, -10.0, 10.0), "v_y": (_lib.VY, -1.0, 1.0),
                                   "v_z": (_lib.VZ, -1.0, 1.0)} and viewer.SLICE_ALPHA == 0.2
    image_h = open(os.path.join(CSRC, "image.h")).read()
    assert "IMG_SLICE = 0, IMG_SUM = 1, IMG_MAX = 2, IMG_MIN = 3" in image_h
