"""Momentum zones on the host: the numpy restatement of include/fluidsim.h (tests/zones_model.py) against a plain triple-loop
restatement on tiny grids, and the arithmetic of csrc/zones.h itself -- a driver compiled with the host C++ compiler and the
library's -ffp-contract=off runs exactly the inline functions the kernels call, cell by cell, and every output is compared
bit for bit with the model.  The driver is also built with -fsanitize=address,undefined and run as a program.  Also: the
constructors of fluid_simulation_amd.zones against hand-written rows, and the prototypes."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import zones_model as M
from conftest import bits_equal

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "fluid_simulation_amd", "csrc")
HEADER = os.path.join(ROOT, "include", "fluidsim.h")
DT = 0.05
GRIDS = [(1, 1, 1), (2, 1, 3), (4, 3, 2), (6, 5, 4)]

# stdin: "<elem 4|8> <W> <H> <D> <n_zones>", the zones' rows (fp64 bit patterns), dt (fp64 bit pattern of the widened float),
# then per padded cell in [z][y][x] order v_x, v_y, v_z (bit patterns of the element type) and the flag byte
# stdout: per interior cell in the same order "mask v_x' v_y' v_z'" (the pass without its setBounds), then per plane and zone
# "P" and the seven budget values, then per zone "W" and the seven values of the whole (fp64 bit patterns)
DRIVER = r'''
#include "zones.h"
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
using namespace fs;
template <class T, class B> static T rd() { unsigned long long b; if (std::scanf("%llx", &b) != 1) std::exit(3); B bb = (B)b; T v; std::memcpy(&v, &bb, sizeof v); return v; }
template <class T, class B> static void put(T v) { B b; std::memcpy(&b, &v, sizeof v); std::printf(" %llx", (unsigned long long)b); }
template <class T, class B> static int run(int W, int H, int D, int nz)
{
    ZoneTable zt;
    std::memset(&zt, 0, sizeof zt);
    std::vector<double> par((size_t)nz * ZONE_PARAMS);
    for (double& p : par) p = rd<double, uint64_t>();
    zt.dt = rd<double, uint64_t>();
    zt.n = nz;
    for (int k = 0; k < nz; ++k) zt.z[k] = zone_make(&par[(size_t)k * ZONE_PARAMS], zt.dt);
    const long sy = W + 2, sz = sy * (H + 2), n = sz * (D + 2);
    std::vector<T> v[3] = { std::vector<T>((size_t)n), std::vector<T>((size_t)n), std::vector<T>((size_t)n) };
    std::vector<unsigned> fl((size_t)n);
    for (long c = 0; c < n; ++c) {
        for (int a = 0; a < 3; ++a) v[a][(size_t)c] = rd<T, B>();
        if (std::scanf("%u", &fl[(size_t)c]) != 1) return 3;
    }
    // the pass and the mask
    for (int z = 1; z <= D; ++z)
        for (int y = 1; y <= H; ++y)
            for (int x = 1; x <= W; ++x) {
                const long c = x + y * sy + z * sz;
                T out[3] = { v[0][(size_t)c], v[1][(size_t)c], v[2][(size_t)c] };
                unsigned bits = 0;
                if (zone_target(fl[(size_t)c])) {
                    double u[3] = { (double)out[0], (double)out[1], (double)out[2] };
                    for (int k = 0; k < nz; ++k)
                        if (zone_in(zt.z[k], x, y, z)) {
                            if (!zone_meets(zt.z[k], x, x, y, y, z, z)) return 4;
                            zone_stage_apply(zt.z[k], zt.dt, u);
                            bits |= 1u << k;
                        }
                    if (bits)
                        for (int a = 0; a < 3; ++a) out[a] = (T)u[a];
                }
                std::printf("%u", bits);
                for (int a = 0; a < 3; ++a) put<T, B>(out[a]);
                std::printf("\n");
            }
    // the budget: columns in increasing y, planes in increasing x, the whole in increasing z
    std::vector<ZoneSums> whole((size_t)nz, zone_sums_start());
    for (int z = 1; z <= D; ++z) {
        std::vector<ZoneSums> plane((size_t)nz, zone_sums_start());
        for (int x = 1; x <= W; ++x)
            for (int k = 0; k < nz; ++k) {
                ZoneSums col = zone_sums_start();
                for (int y = 1; y <= H; ++y) {
                    const long c = x + y * sy + z * sz;
                    if (!zone_in(zt.z[k], x, y, z) || !zone_target(fl[(size_t)c])) continue;
                    double u[3] = { (double)v[0][(size_t)c], (double)v[1][(size_t)c], (double)v[2][(size_t)c] };
                    for (int j = 0; j < k; ++j)
                        if (zone_in(zt.z[j], x, y, z)) zone_stage_apply(zt.z[j], zt.dt, u);
                    const double u0[3] = { u[0], u[1], u[2] };
                    const ZoneStage st = zone_stage(zt.z[k], zt.dt, u);
                    zone_sums_add(col, zt.z[k], u0, u, st);
                }
                for (int j = 0; j < ZONE_COLS; ++j) plane[(size_t)k].v[j] = zone_combine(j, plane[(size_t)k].v[j], col.v[j]);
            }
        for (int k = 0; k < nz; ++k) {
            std::printf("P");
            for (int j = 0; j < ZONE_COLS; ++j) {
                put<double, uint64_t>(plane[(size_t)k].v[j]);
                whole[(size_t)k].v[j] = zone_combine(j, whole[(size_t)k].v[j], plane[(size_t)k].v[j]);
            }
            std::printf("\n");
        }
    }
    for (int k = 0; k < nz; ++k) {
        std::printf("W");
        for (int j = 0; j < ZONE_COLS; ++j) {
            if (zone_start(j) != zone_sums_start().v[j]) return 5;
            put<double, uint64_t>(whole[(size_t)k].v[j]);
        }
        std::printf("\n");
    }
    return 0;
}
int main()
{
    static_assert(ZONE_PARAMS == 20 && ZONE_COLS == 7 && ZONE_MAX == 8 && ZONE_SOLID == 1u && ZONE_NEAR == 2u, "the header's numbers");
    int elem, W, H, D, nz;
    if (std::scanf("%d %d %d %d %d", &elem, &W, &H, &D, &nz) != 5 || nz < 0 || nz > ZONE_MAX) return 2;
    return elem == 4 ? run<float, uint32_t>(W, H, D, nz) : run<double, uint64_t>(W, H, D, nz);
}
'''


def build_driver(d, sanitize):
    cxx = shutil.which("g++") or shutil.which("c++")
    if cxx is None:
        pytest.fail("no C++ compiler")
    src = d / "driver.cpp"
    src.write_text(DRIVER)
    exe = d / ("driver_san" if sanitize else "driver")
    flags = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if sanitize else ["-O2"]
    subprocess.run([cxx, "-std=c++17", "-Wall", "-Werror", "-ffp-contract=off"] + flags + ["-I", CSRC, str(src), "-o", str(exe)],
                   check=True)
    return exe


@pytest.fixture(scope="module")
def drivers(tmp_path_factory):
    d = tmp_path_factory.mktemp("zones_driver")
    return build_driver(d, False), build_driver(d, True)


def run_driver(exe, vel, obs, zones, dt):
    T = vel[0].dtype
    U = np.uint32 if T == np.float32 else np.uint64
    D, H, W = (n - 2 for n in vel[0].shape)
    words = ["%d %d %d %d %d" % (T.itemsize, W, H, D, len(zones))]
    words += ["%x" % int(b) for r in zones for b in np.asarray(r, dtype=np.float64).view(np.uint64)]
    words.append("%x" % int(np.float64(np.float32(dt)).view(np.uint64)))
    flags = M.flag_bytes(obs)
    for a, b, c, f in zip(vel[0].ravel().view(U), vel[1].ravel().view(U), vel[2].ravel().view(U), flags.ravel()):
        words.append("%x %x %x %d" % (int(a), int(b), int(c), int(f)))
    out = subprocess.run([str(exe)], input="\n".join(words) + "\n", capture_output=True, text=True)
    assert out.returncode == 0, (out.returncode, out.stderr[-2000:])
    tok = [line.split() for line in out.stdout.splitlines()]
    cells, rest = tok[:W * H * D], tok[W * H * D:]
    assert len(rest) == (D + 1) * len(zones)
    shape = (D, H, W)
    bits = np.array([int(r[0]) for r in cells], dtype=np.uint8).reshape(shape)
    new = [np.array([int(r[1 + a], 16) for r in cells], dtype=U).view(T).reshape(shape) for a in range(3)]
    planes = np.array([[int(w, 16) for w in r[1:]] for r in rest if r[0] == "P"], dtype=np.uint64).view(np.float64).reshape(D, len(zones), M.COLS)
    whole = np.array([[int(w, 16) for w in r[1:]] for r in rest if r[0] == "W"], dtype=np.uint64).view(np.float64).reshape(len(zones), M.COLS)
    return bits, new, whole, planes


def masks(W, H, D):
    shape = (D + 2, H + 2, W + 2)
    out = {"none": np.zeros(shape, dtype=bool)}
    m = out["none"].copy()
    m[(D + 1) // 2, (H + 1) // 2, min(3, W)] = True
    out["one voxel"] = m
    m = out["none"].copy()
    m[1:min(2, D) + 1, 1, 1:min(3, W) + 1] = True
    out["block on the y = 1 wall"] = m
    return out


def fields(rng, shape, dtype):
    """u, v, w: seeded, mixed magnitudes, a few -0.0, the twelve box edges zero"""
    out = []
    for _ in range(3):
        a = (rng.standard_normal(shape) * 10.0 ** rng.integers(-2, 2, size=shape)).astype(dtype)
        a[rng.random(shape) < 0.05] = dtype(-0.0)
        g = np.zeros(shape, dtype=np.int8)
        g[0] += 1
        g[-1] += 1
        g[:, 0] += 1
        g[:, -1] += 1
        g[:, :, 0] += 1
        g[:, :, -1] += 1
        a[g >= 2] = 0
        out.append(a)
    return out


def zone_sets(W, H, D):
    """name -> rows: every shape and axis, rim cells decided by <=, a fractional centre, radius 0, overlaps, plain zones"""
    whole = M.whole_box((W, H, D))
    cx, cy, cz = (W + 1) // 2, (H + 1) // 2, (D + 1) // 2
    out = {"no zone": []}
    out["the whole domain, all terms"] = [M.row(box=whole, g=(0.5, -0.25, 0.125), D=(1.0, 0.0, 2.5), F=(0.0, 3.0, 0.75))]
    out["a fan (D = F = 0)"] = [M.row(box=whole, axis=2, g=(0.0, 0.0, 1.5))]
    out["two corner cells"] = [M.row(box=(1, 1, 1, 1, 1, 1), D=(4.0, 4.0, 4.0)), M.row(box=(W, W, H, H, D, D), axis=1, F=(0.0, 9.0, 0.0))]
    for axis, centre in ((0, (cy, cz)), (1, (cx, cz)), (2, (cx, cy))):
        out["cylinder along %d, radius 2" % axis] = [M.row(M.CYLINDER, axis, whole, centre, 2.0, g=(0.1, 0.2, 0.3), F=(1.0, 1.0, 1.0))]
    out["cylinder, fractional centre"] = [M.row(M.CYLINDER, 0, whole, (cy + 0.5, cz - 0.25), 1.25, D=(0.5, 0.5, 0.5))]
    out["cylinder, radius 0"] = [M.row(M.CYLINDER, 2, whole, (cx, cy), 0.0, g=(1.0, 0.0, 0.0))]
    a = M.row(box=(1, max(1, W - 1), 1, H, 1, D), g=(0.5, 0.0, 0.0), D=(2.0, 0.0, 0.0))
    b = M.row(box=(min(2, W), W, 1, H, 1, D), axis=1, F=(3.0, 3.0, 3.0))
    out["two overlapping zones"] = [a, b]
    out["the same, the other way round"] = [b, a]
    out["eight zones"] = [M.row(box=whole, axis=k % 3, g=(0.01 * k, 0.0, -0.02 * k), D=(0.1 * (k % 2), 0.0, 0.0), F=(0.0, 0.2 * (k % 3), 0.0))
                          for k in range(8)]
    return out


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("grid", GRIDS)
def test_model_matches_the_triple_loop(grid, dtype):
    W, H, D = grid
    rng = np.random.default_rng([W, H, D, 1])
    for mname, mask in masks(W, H, D).items():
        obs = mask.astype(dtype)
        for zname, zones in zone_sets(W, H, D).items():
            vel = fields(rng, mask.shape, dtype)
            bits, new, whole, planes = M.naive(vel, obs, zones, DT)
            assert np.array_equal(M.mask(obs, zones), bits), (mname, zname)
            for a, b in zip(M.apply(vel, obs, zones, DT), new):
                assert bits_equal(a, b), (mname, zname)
            got_whole, got_planes = M.budget(vel, obs, zones, DT)
            assert bits_equal(got_planes, planes), (mname, zname)
            assert bits_equal(got_whole, whole), (mname, zname)


def test_model_edge_values():
    """-0.0 outside every zone keeps its sign, inside a fan it does not; a zone in the wrong order gives other bits."""
    W, H, D = 6, 5, 4
    shape = (D + 2, H + 2, W + 2)
    negz = [np.full(shape, -0.0, dtype=np.float32) for _ in range(3)]
    obs = np.zeros(shape, dtype=np.float32)
    fan = [M.row(box=(2, 3, 1, H, 1, D), g=(0.0, 0.0, 0.0))]
    out = M.apply_unbounded(negz, obs, fan, DT)
    assert np.signbit(out[0][1:-1, 1:-1, 4:-1]).all() and not np.signbit(out[0][1:-1, 1:-1, 2:4]).any()
    rng = np.random.default_rng(5)
    vel = fields(rng, shape, np.float32)
    sets = zone_sets(W, H, D)
    ab = M.apply(vel, obs, sets["two overlapping zones"], DT)
    ba = M.apply(vel, obs, sets["the same, the other way round"], DT)
    assert any(not bits_equal(p, q) for p, q in zip(ab, ba))


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("grid", GRIDS)
def test_zones_h_matches_the_model(drivers, grid, dtype):
    """csrc/zones.h, compiled for the host, cell by cell -- and once more under AddressSanitizer and UBSan."""
    W, H, D = grid
    rng = np.random.default_rng([W, H, D, 2])
    c = slice(1, -1)
    for mname, mask in masks(W, H, D).items():
        obs = mask.astype(dtype)
        for k, (zname, zones) in enumerate(zone_sets(W, H, D).items()):
            vel = fields(rng, mask.shape, dtype)
            if k % 4 == 1:                                   # non-finite speeds: the plain zones must take the full text there
                for a, bad in zip(vel, (np.inf, np.nan, -np.inf)):
                    a[rng.random(a.shape) < 0.1] = bad
            for exe in (drivers if k in (1, 2, 9) else drivers[:1]):
                bits, new, whole, planes = run_driver(exe, vel, obs, zones, DT)
                assert np.array_equal(bits, M.mask(obs, zones)[c, c, c]), (mname, zname)
                for a, b in zip(new, M.apply_unbounded(vel, obs, zones, DT)):
                    assert M.same(a, b[c, c, c]), (mname, zname)
                want_whole, want_planes = M.budget(vel, obs, zones, DT)
                assert M.same(planes, want_planes), (mname, zname)
                assert M.same(whole, want_whole), (mname, zname)


def test_zones_header_includes_nothing():
    """csrc/zones.h must stay compilable by the host compiler alone."""
    inc = re.findall(r"^\s*#\s*include\s+(\S+)", open(os.path.join(CSRC, "zones.h")).read(), flags=re.M)
    assert inc == [], inc


def test_constructors_against_hand_written_rows():
    from fluid_simulation_amd import zones as Z
    box = (3, 5, 1, 8, 2, 7)
    assert Z.porous_box(box, D=2.0, F=(1.0, 0.5, 0.25)).tolist() == [0, 0, 3, 5, 1, 8, 2, 7, 0, 0, 0, 0, 0, 0, 2, 2, 2, 1, 0.5, 0.25]
    assert Z.fan(box, (0.0, -3.0, 1.0)).tolist() == [0, 1, 3, 5, 1, 8, 2, 7, 0, 0, 0, 0, -3, 1, 0, 0, 0, 0, 0, 0]
    assert Z.fan(box, 2.5, axis=2).tolist() == [0, 2, 3, 5, 1, 8, 2, 7, 0, 0, 0, 0, 0, 2.5, 0, 0, 0, 0, 0, 0]
    assert Z.straightener(box, 0, 50.0).tolist() == [0, 0, 3, 5, 1, 8, 2, 7, 0, 0, 0, 0, 0, 0, 0, 50, 50, 0, 0, 0]
    # a 16 x 8 x 8 grid has 1024 cells: h = 1 / cbrt(1024), F = 0.5 * ct' / (2 h) = 0.5 * 2 / 2 * cbrt(1024)
    disk = Z.actuator_disk(0, (6.0, 4.5, 4.5), 3.0, 2, 2.0, grid=(16, 8, 8))
    assert disk[:11].tolist() == [1, 0, 6, 7, 1, 8, 1, 8, 4.5, 4.5, 3.0] and disk[11:17].tolist() == [0] * 6
    assert disk[18:].tolist() == [0, 0] and disk[17] == 0.5 * 2.0 / (2.0 * (1.0 / np.cbrt(1024.0)))
    disk = Z.actuator_disk(2, (20.0, 10.0, 3.0), 2.5, 1, 1.0, grid=(64, 32, 16))
    assert disk[:11].tolist() == [1, 2, 17, 23, 7, 13, 3, 3, 20.0, 10.0, 2.5] and disk[19] > 0 and disk[17] == disk[18] == 0
    rows = Z.sponge(25, 32, 8.0, 4, grid=(32, 6, 5))
    assert rows.shape == (4, 20)
    assert [r[2:8].tolist() for r in rows] == [[25, 26, 1, 6, 1, 5], [27, 28, 1, 6, 1, 5], [29, 30, 1, 6, 1, 5], [31, 32, 1, 6, 1, 5]]
    assert [r[14:17].tolist() for r in rows] == [[0.5] * 3, [2.0] * 3, [4.5] * 3, [8.0] * 3]
    assert all(r[0] == 0 and not r[8:14].any() and not r[17:].any() for r in rows)
    rows = Z.sponge(10, 14, 1.0, 2, grid=(14, 3, 3))         # five planes in two layers: 2 + 3
    assert [r[2:4].tolist() for r in rows] == [[10, 11], [12, 14]]
    with pytest.raises(ValueError):
        Z.sponge(10, 11, 1.0, 3, grid=(14, 3, 3))


def test_header_declares_the_prototypes():
    text = re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S))
    from fluid_simulation_amd import _lib
    for proto in ("int fs_zones(fs_sim* s, const double* par, int n_zones, int mode, int log);",
                  "int fs_zones_get(fs_sim* s, double* par, int* n_zones, int* mode, int* log);",
                  "int fs_zone_apply(fs_sim* s);", "int fs_zone_budget(fs_sim* s, double* out, double* per_plane);",
                  "int fs_zone_log(fs_sim* s, double* rows, long max_rows, long* n_rows, long* n_dropped);",
                  "int fs_zone_mask(fs_sim* s, uint8_t* dst, size_t n);"):
        assert proto in text, proto
        name = proto.split("(")[0].split()[-1]
        assert name in _lib.exported_symbols() and name in _lib._SIGNATURES
        assert len(_lib._SIGNATURES[name][1]) == proto.count(",") + 1, name
    for define, value in (("FS_ZONE_MAX", _lib.ZONE_MAX), ("FS_ZONE_PARAMS", _lib.ZONE_PARAMS), ("FS_ZONE_COLS", _lib.ZONE_COLS)):
        assert "#define %s %d" % (define, value) in text, define
    assert _lib.ZONE_PARAMS == M.PARAMS and _lib.ZONE_COLS == M.COLS and _lib.ZONE_MAX == M.MAX and len(_lib.ZONE_NAMES) == M.COLS
