"""The arithmetic of the point sampler (csrc/sample.h), on the host: a driver compiled with the host C++ compiler and
-ffp-contract=off (the library's own setting) runs exactly the inline functions the sampler kernel calls -- the same corner
gather, the same three modes -- over seeded random fields, obstacle patterns and points, and every value is compared bit
for bit with the numpy fp64 restatement in tests/sample_model.py, which is written from the definition in
include/fluidsim.h.  float and double sources, float and double obs.  Also: the constants of the ctypes layer against the
header."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import sample_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "fluid_simulation_amd", "csrc")
HEADER = os.path.join(ROOT, "include", "fluidsim.h")

# stdin: "<source elem 4|8> <obs elem 4|8> <W> <H> <D> <n>", then the dense padded source, the dense padded obs and the
# n x 3 point coordinates, all as hex bit patterns.  stdout: per point one line, the three modes' values as hex bit patterns.
DRIVER = r'''
#include "sample.h"
#include <cstdint>
#include <cstdlib>
#include <cstdio>
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
template <int MODE, class E, class O>
static double at(const std::vector<E>& src, const std::vector<O>& obs, int W, int H, int D, double x, double y, double z)
{
    const long py = W + 2, pz = (long)(W + 2) * (H + 2);
    int i0, j0, l0;
    double sx, sy, sz;
    const bool okx = sample_axis(x, W, i0, sx), oky = sample_axis(y, H, j0, sy), okz = sample_axis(z, D, l0, sz);
    const long base = (long)i0 + (long)j0 * py + (long)l0 * pz;
    E v[8];
    O o[8];
    for (int c = 0; c < 8; ++c) {
        const long at = base + (c & 1) + ((c >> 1) & 1) * py + (c >> 2) * pz;
        if (at < 0 || at >= (long)src.size()) std::exit(4);
        v[c] = src[at];
        o[c] = obs[at];
    }
    return sample_value<MODE, E, O>(okx && oky && okz, v, o, sx, sy, sz);
}
template <class E, class O> static int run(int W, int H, int D, int n)
{
    const size_t cells = (size_t)(W + 2) * (H + 2) * (D + 2);
    std::vector<E> src(cells);
    std::vector<O> obs(cells);
    for (E& v : src) v = rd<E>();
    for (O& v : obs) v = rd<O>();
    for (int k = 0; k < n; ++k) {
        const double x = rd<double>(), y = rd<double>(), z = rd<double>();
        put(at<SAMPLE_NEAREST>(src, obs, W, H, D, x, y, z));
        put(at<SAMPLE_LINEAR>(src, obs, W, H, D, x, y, z));
        put(at<SAMPLE_FLUID>(src, obs, W, H, D, x, y, z));
        std::printf("\n");
    }
    return 0;
}
int main()
{
    int elem, oelem, W, H, D, n;
    if (std::scanf("%d %d %d %d %d %d", &elem, &oelem, &W, &H, &D, &n) != 6) return 2;
    if (elem == 4 && oelem == 4) return run<float, float>(W, H, D, n);
    if (elem == 8 && oelem == 4) return run<double, float>(W, H, D, n);
    if (elem == 8 && oelem == 8) return run<double, double>(W, H, D, n);
    return 2;
}
'''


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++")
    if cxx is None:
        pytest.fail("no C++ compiler")
    d = tmp_path_factory.mktemp("sample_cpu")
    src = d / "driver.cpp"
    src.write_text(DRIVER)
    exe = d / "driver"
    subprocess.run([cxx, "-std=c++17", "-O2", "-Wall", "-Werror", "-Wno-maybe-uninitialized", "-ffp-contract=off", "-I", CSRC,
                    str(src), "-o", str(exe)], check=True)

    def bits(a):
        a = np.ascontiguousarray(a)
        return a.view(np.uint32 if a.dtype.itemsize == 4 else np.uint64).reshape(-1)

    def run(field, obs, points):
        """-> (n, 3) float64: the three modes' values"""
        d2, h2, w2 = field.shape
        text = "%d %d %d %d %d %d\n" % (field.dtype.itemsize, obs.dtype.itemsize, w2 - 2, h2 - 2, d2 - 2, points.shape[0])
        for a in (field, obs, points):
            text += " ".join("%x" % int(b) for b in bits(a)) + "\n"
        out = subprocess.run([str(exe)], input=text, capture_output=True, text=True, check=True).stdout
        rows = np.array([[int(t, 16) for t in line.split()] for line in out.splitlines()], dtype=np.uint64)
        return rows.view(np.float64).reshape(points.shape[0], 3)

    return run


def random_case(dtype, odtype, shape, seed):
    w, h, d = shape
    rng = np.random.default_rng(seed)
    full = (d + 2, h + 2, w + 2)
    field = (rng.standard_normal(full) * 10.0 ** rng.integers(-3, 4, size=full)).astype(dtype)
    field[rng.random(full) < 0.05] = 0.0
    obs = (rng.random(full) < 0.35).astype(odtype)
    obs[rng.random(full) < 0.03] = odtype(0.5)                 # neither 0 nor 1: counts as not solid
    return field, obs, M.special_points(w, h, d, rng, n_random=96)


@pytest.mark.parametrize("dtype,odtype", [(np.float32, np.float32), (np.float64, np.float32), (np.float64, np.float64)],
                         ids=["f32", "f64_obs32", "f64"])
@pytest.mark.parametrize("shape", [(7, 5, 4), (1, 1, 1), (5, 3, 4)], ids=lambda s: "x".join(map(str, s)))
def test_driver_matches_model(driver, dtype, odtype, shape):
    field, obs, pts = random_case(dtype, odtype, shape, seed=20260 + shape[0])
    got = driver(field, obs, pts)
    for mode in M.MODES:
        want = M.sample(field, obs, pts, mode)
        assert M.same_bits(got[:, mode], want), (M.MODE_NAMES[mode], np.flatnonzero(
            ~((got[:, mode] == want) | (np.isnan(got[:, mode]) & np.isnan(want))))[:8])
    outside = np.isnan(pts).any(axis=1) | (pts < 0).any(axis=1) | (pts > np.array(shape) + 1.0).any(axis=1)
    assert outside.sum() >= 19
    assert np.isnan(got[outside]).all()
    assert not np.isnan(got[~outside][:, :2]).any()


def test_nonfinite_corners(driver):
    """LINEAR multiplies every corner: a NaN or infinite corner of weight 0 gives NaN; NEAREST returns the stored value
    itself; FLUID skips corners of weight 0."""
    field = np.zeros((4, 4, 4), dtype=np.float32)
    obs = np.zeros_like(field)
    field[1, 1, 1] = 3.0
    field[1, 1, 2] = np.inf
    field[2, 1, 1] = np.nan
    pts = np.array([[1.0, 1.0, 1.0]])
    got = driver(field, obs, pts)
    assert got[0, M.NEAREST] == 3.0 and np.isnan(got[0, M.LINEAR]) and got[0, M.FLUID] == 3.0
    for mode in M.MODES:
        assert M.same_bits(got[:, mode], M.sample(field, obs, pts, mode))


def test_fluid_edge_midpoint_and_all_solid(driver):
    """At the midpoint of an edge between a solid and a fluid cell FLUID returns exactly the fluid cell's value; with all
    eight corners solid it returns NaN."""
    rng = np.random.default_rng(5)
    field = rng.standard_normal((5, 5, 5)).astype(np.float32)
    obs = np.zeros_like(field)
    obs[2, 2, 2] = 1.0
    pts = np.array([[2.5, 2.0, 2.0], [1.5, 2.0, 2.0], [2.0, 2.5, 2.0], [2.0, 1.5, 2.0], [2.0, 2.0, 2.5], [2.0, 2.0, 1.5]])
    want = np.array([field[2, 2, 3], field[2, 2, 1], field[2, 3, 2], field[2, 1, 2], field[3, 2, 2], field[1, 2, 2]], dtype=np.float64)
    got = driver(field, obs, pts)
    assert M.same_bits(got[:, M.FLUID], want)
    obs[:] = 1.0
    got = driver(field, obs, np.array([[2.25, 2.5, 2.75], [2.0, 2.0, 2.0]]))
    assert np.isnan(got[:, M.FLUID]).all() and not np.isnan(got[:, M.LINEAR]).any()


def test_python_constants_match_header():
    from fluid_simulation_amd import _lib
    import fluid_simulation_amd as F
    text = open(HEADER).read()
    enum = dict((k, int(v)) for k, v in re.findall(r"\b(FS_SAMPLE_[A-Z]+)\s*=\s*(\d+)", text))
    defs = dict((k, int(v)) for k, v in re.findall(r"#define\s+(FS_(?:SAMPLE|PROBE)_[A-Z]+)\s+(\d+)", text))
    assert enum == {"FS_SAMPLE_NEAREST": _lib.SAMPLE_NEAREST, "FS_SAMPLE_LINEAR": _lib.SAMPLE_LINEAR, "FS_SAMPLE_FLUID": _lib.SAMPLE_FLUID}
    assert defs == {"FS_SAMPLE_STAT": _lib.SAMPLE_STAT, "FS_PROBE_MAX": _lib.PROBE_MAX, "FS_PROBE_VALUES": _lib.PROBE_VALUES}
    assert (enum["FS_SAMPLE_NEAREST"], enum["FS_SAMPLE_LINEAR"], enum["FS_SAMPLE_FLUID"]) == (0, 1, 2)
    assert (defs["FS_SAMPLE_STAT"], defs["FS_PROBE_MAX"], defs["FS_PROBE_VALUES"]) == (1024, 4096, 5)
    assert (M.NEAREST, M.LINEAR, M.FLUID) == (_lib.SAMPLE_NEAREST, _lib.SAMPLE_LINEAR, _lib.SAMPLE_FLUID)
    assert _lib.SAMPLE_MODES == {"nearest": 0, "linear": 1, "fluid": 2}
    assert len(_lib.PROBE_NAMES) == _lib.PROBE_VALUES
    for name in ("SAMPLE_NEAREST", "SAMPLE_LINEAR", "SAMPLE_FLUID", "SAMPLE_STAT", "PROBE_MAX", "PROBE_VALUES"):
        assert getattr(F, name) == getattr(_lib, name)
    # the stat, vortex and raw bits of a source never collide
    assert _lib.SAMPLE_STAT > (_lib.ISO_VORTEX | _lib.VORTEX_Q) and _lib.SAMPLE_STAT > (_lib.STAT_RAW | _lib.STAT_TKE)
