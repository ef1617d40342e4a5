"""Heat and buoyancy on the host: the numpy restatement of include/fluidsim.h (tests/heat_model.py) against a plain
triple-loop restatement on tiny grids, its stores against the CPU oracle's set_bounds, the -0.0 case, and the arithmetic of
csrc/heat.h itself -- a driver compiled with the host C++ compiler and the library's -ffp-contract=off runs exactly the inline
functions the kernels call, cell by cell, and every output is compared bit for bit with the model.  The driver is also built
with -fsanitize=address,undefined and run as a program.  Also: the prototypes."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import heat_model as M
from conftest import bits_equal

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "fluid_simulation_amd", "csrc")
HEADER = os.path.join(ROOT, "include", "fluidsim.h")
DT = 0.05
GRIDS = [(1, 1, 1), (2, 1, 3), (4, 3, 2), (5, 4, 3), (6, 5, 4)]

# stdin: "<elem 4|8> <W> <H> <D>", the 15 parameters (fp64 bit patterns), dt (fp64 bit pattern of the widened float), then per
# padded cell in [z][y][x] order theta, v_up, dens (bit patterns of the element type) and the flag byte
# stdout: per interior cell in the same order the working value, the new v_up (bit patterns), held 0|1, the cell's conductive
# loss (fp64 bit pattern; 0 where the cell is not held)
DRIVER = r'''
#include "heat.h"
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
using namespace fs;
template <class T, class B> static T rd() { unsigned long long b; if (std::scanf("%llx", &b) != 1) std::exit(3); B bb = (B)b; T v; std::memcpy(&v, &bb, sizeof v); return v; }
template <class T, class B> static void put(T v) { B b; std::memcpy(&b, &v, sizeof v); std::printf(" %llx", (unsigned long long)b); }
template <class T, class B> static int run(int W, int H, int D)
{
    double par[HEAT_PARAMS];
    for (int k = 0; k < HEAT_PARAMS; ++k) par[k] = rd<double, uint64_t>();
    HeatPass p;
    p.beta = par[HP_BETA]; p.alpha = par[HP_ALPHA]; p.dt = rd<double, uint64_t>();
    p.inlet = par[HP_INLET]; p.wall_t = par[HP_WALL_T]; p.up = (int)par[HP_UP]; p.wall = (int)par[HP_WALL];
    for (int k = 0; k < 6; ++k) p.box[k] = (int)par[HP_X0 + k];
    const long sy = W + 2, sz = sy * (H + 2), n = sz * (D + 2);
    std::vector<T> th((size_t)n), v((size_t)n), q((size_t)n);
    std::vector<unsigned> fl((size_t)n);
    for (long c = 0; c < n; ++c) {
        th[(size_t)c] = rd<T, B>(); v[(size_t)c] = rd<T, B>(); q[(size_t)c] = rd<T, B>();
        if (std::scanf("%u", &fl[(size_t)c]) != 1) return 3;
    }
    const long step[6] = { -1, 1, -sy, sy, -sz, sz };
    const unsigned bit[6] = { 8u, 4u, 32u, 16u, 128u, 64u };
    for (int z = 1; z <= D; ++z)
        for (int y = 1; y <= H; ++y)
            for (int x = 1; x <= W; ++x) {
                const long c = x + y * sy + z * sz;
                const unsigned f = fl[(size_t)c];
                const T t = heat_working<T>(p, th[(size_t)c], f, x, y, z);
                put<T, B>(t);
                put<T, B>(heat_buoyancy<T>(p, v[(size_t)c], t, q[(size_t)c]));
                const bool held = heat_held(p, f, x, y, z);
                double nb[6] = { 0, 0, 0, 0, 0, 0 }, loss = 0.0;
                bool count[6] = { false, false, false, false, false, false };
                if (held) {
                    for (int j = 0; j < 6; ++j) {
                        if (!(f & bit[j])) continue;
                        const int nx = x + (j == 0 ? -1 : j == 1 ? 1 : 0), ny = y + (j == 2 ? -1 : j == 3 ? 1 : 0), nz = z + (j == 4 ? -1 : j == 5 ? 1 : 0);
                        if (heat_held(p, fl[(size_t)(c + step[j])], nx, ny, nz)) continue;
                        count[j] = true;
                        nb[j] = (double)th[(size_t)(c + step[j])];
                    }
                    loss = heat_cell_loss((double)th[(size_t)c], nb, count);
                }
                std::printf(" %d", held ? 1 : 0);
                put<double, uint64_t>(loss);
                std::printf("\n");
            }
    return 0;
}
int main()
{
    static_assert(HEAT_PARAMS == 15 && HEAT_COLS == 9 && HEAT_SOLID == 1u && HEAT_NEAR == 2u, "the header's numbers");
    int elem, W, H, D;
    if (std::scanf("%d %d %d %d", &elem, &W, &H, &D) != 4) return 2;
    return elem == 4 ? run<float, uint32_t>(W, H, D) : run<double, uint64_t>(W, H, D);
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
    d = tmp_path_factory.mktemp("heat_driver")
    return build_driver(d, False), build_driver(d, True)


def run_driver(exe, theta, v, dens, obs, par, dt):
    U = np.uint32 if theta.dtype == np.float32 else np.uint64
    D, H, W = (n - 2 for n in theta.shape)
    words = ["%d %d %d %d" % (theta.dtype.itemsize, W, H, D)]
    words += ["%x" % int(b) for b in np.asarray(par, dtype=np.float64).view(np.uint64)]
    words.append("%x" % int(np.float64(np.float32(dt)).view(np.uint64)))
    flags = M.flag_bytes(obs)
    for t, a, q, f in zip(theta.ravel().view(U), v.ravel().view(U), dens.ravel().view(U), flags.ravel()):
        words.append("%x %x %x %d" % (int(t), int(a), int(q), int(f)))
    out = subprocess.run([str(exe)], input="\n".join(words) + "\n", capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-2000:]
    tok = [line.split() for line in out.stdout.splitlines()]
    assert len(tok) == W * H * D
    shape = (D, H, W)
    t = np.array([int(r[0], 16) for r in tok], dtype=U).view(theta.dtype).reshape(shape)
    vn = np.array([int(r[1], 16) for r in tok], dtype=U).view(theta.dtype).reshape(shape)
    held = np.array([int(r[2]) for r in tok], dtype=bool).reshape(shape)
    loss = np.array([int(r[3], 16) for r in tok], dtype=np.uint64).view(np.float64).reshape(shape)
    return t, vn, held, loss


def masks(W, H, D):
    shape = (D + 2, H + 2, W + 2)
    out = {"none": np.zeros(shape, dtype=bool)}
    m = out["none"].copy()
    m[(D + 1) // 2, (H + 1) // 2, min(3, W)] = True
    out["one voxel"] = m
    m = out["none"].copy()
    m[1:min(2, D) + 1, 1, 1:min(3, W) + 1] = True
    out["block on the y = 1 wall"] = m
    m = out["none"].copy()
    m[1, 1, 1] = True
    m[D, H, W] = True
    out["two bodies, one on the inlet"] = m
    return out


def fields(rng, shape, dtype):
    """theta, u, v, w, dens: seeded, mixed magnitudes, a few -0.0, the twelve box edges zero"""
    out = []
    for _ in range(5):
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


def cases(W, H, D):
    """parameter sets: every up code, the wall on (whole box and a box of one corner) and off, inlet zero and not"""
    for up in range(6):
        yield M.params(beta=0.7, alpha=0.3, up=up, inlet=0.0 if up % 2 else 1.25, wall=(2.5 if up < 4 else None), shape=(W, H, D))
    yield M.params(beta=0.0, alpha=0.9, up=2, inlet=-0.5, wall=1.0, box=(1, max(1, W // 2), 1, H, 1, max(1, D // 2)))
    yield M.params(beta=1.1, alpha=0.0, up=5, inlet=0.0, wall=None, shape=(W, H, D))
    yield M.params(beta=0.0, alpha=0.0, up=2, inlet=3.0, wall=0.5, shape=(W, H, D))


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("grid", GRIDS)
def test_model_matches_the_triple_loop(grid, dtype):
    W, H, D = grid
    rng = np.random.default_rng([W, H, D, 1])
    for name, mask in masks(W, H, D).items():
        obs = mask.astype(dtype)
        for par in cases(W, H, D):
            theta, u, v, w, dens = fields(rng, mask.shape, dtype)
            t, vel = M.apply(theta, [u, v, w], dens, obs, par, DT)
            nt, nvel = M.naive_apply(theta, [u, v, w], dens, obs, par, DT)
            assert bits_equal(t, nt), (name, par)
            for a, b in zip(vel, nvel):
                assert bits_equal(a, b), (name, par)
            whole, planes = M.budget(theta, u, obs, par)
            nwhole, nplanes = M.naive_budget(theta, u, obs, par)
            assert bits_equal(planes, nplanes), (name, par)
            assert bits_equal(whole, nwhole), (name, par)


@pytest.mark.parametrize("fp64", [False, True])
def test_stores_are_the_oracles_set_bounds(oracle_mod, fp64):
    """Step 3: theta and the up component come out as the CPU oracle's setBounds leaves the un-bounded arrays."""
    O = oracle_mod
    W, H, D = 6, 5, 4
    dtype = np.float64 if fp64 else np.float32
    ora = O.Oracle(W, H, D, solver=O.JACOBI, fp64=fp64)
    rng = np.random.default_rng(11)
    for name, mask in masks(W, H, D).items():
        obs = mask.astype(dtype)
        ora.set_mask(mask)
        for par in cases(W, H, D):
            theta, u, v, w, dens = fields(rng, mask.shape, dtype)
            t, vel = M.apply(theta, [u, v, w], dens, obs, par, DT)
            t0, vel0 = M.apply_unbounded(theta, [u, v, w], dens, obs, par, DT)
            ora.set(O.DENS, t0)
            ora.set_bounds(0, O.DENS)
            assert bits_equal(ora.get(O.DENS), t), (name, par)
            if par[2] != 0 or par[3] != 0:
                a = int(par[4]) >> 1
                ora.set(O.VX + a, vel0[a])
                ora.set_bounds(a + 1, O.VX + a)
                assert bits_equal(ora.get(O.VX + a), vel[a]), (name, par)
    ora.close()


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_without_buoyancy_the_velocities_are_untouched(dtype):
    """(T)((double)v + 0.0) would turn -0.0 into +0.0: with alpha = beta = 0 the pass must not go near the velocities."""
    W, H, D = 5, 4, 3
    shape = (D + 2, H + 2, W + 2)
    negz = np.full(shape, -0.0, dtype=dtype)
    theta = np.ones(shape, dtype=dtype)
    obs = np.zeros(shape, dtype=dtype)
    par = M.params(beta=0.0, alpha=0.0, inlet=2.0, wall=1.0, shape=(W, H, D))
    vel = [negz.copy(), negz.copy(), negz.copy()]
    t, out = M.apply(theta, vel, negz, obs, par, DT)
    for a, b in zip(out, vel):
        assert a is b and np.signbit(a).all()
    assert (t[1:-1, 1:-1, 1] == 2.0).all()
    # and the force that is exactly zero does: the reason for the rule
    with_force = M.buoyancy(negz, np.zeros(shape, dtype=dtype), np.zeros(shape, dtype=dtype), M.params(beta=1.0, shape=(W, H, D)), DT)
    assert not np.signbit(with_force).any()


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("grid", GRIDS)
def test_heat_h_matches_the_model(drivers, grid, dtype):
    """csrc/heat.h, compiled for the host, cell by cell -- and once more under AddressSanitizer and UBSan."""
    W, H, D = grid
    rng = np.random.default_rng([W, H, D, 2])
    c = slice(1, -1)
    for name, mask in masks(W, H, D).items():
        obs = mask.astype(dtype)
        for k, par in enumerate(cases(W, H, D)):
            theta, u, v, w, dens = fields(rng, mask.shape, dtype)
            a = int(par[4]) >> 1
            vup = [u, v, w][a]
            for exe in (drivers if k == 0 else drivers[:1]):
                t, vn, held, loss = run_driver(exe, theta, vup, dens, obs, par, DT)
                assert bits_equal(t, M.working(theta, obs, par)[c, c, c]), (name, par)
                assert bits_equal(vn, M.buoyancy(vup, M.working(theta, obs, par), dens, par, DT)[c, c, c]), (name, par)
                want_held = M.held_cells(obs, par)[c, c, c]
                assert np.array_equal(held, want_held), (name, par)
                want_loss = np.where(want_held, M.cell_losses(theta, obs, par)[c, c, c], 0.0)
                assert bits_equal(loss, want_loss), (name, par)


def test_heat_header_includes_nothing():
    """csrc/heat.h must stay compilable by the host compiler alone."""
    inc = re.findall(r"^\s*#\s*include\s+(\S+)", open(os.path.join(CSRC, "heat.h")).read(), flags=re.M)
    assert inc == [], inc


def test_header_declares_the_prototypes():
    text = re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S))
    from fluid_simulation_amd import _lib
    for proto in ("int fs_heat_params(fs_sim* s, const double* par, int n);", "int fs_heat_params_get(fs_sim* s, double* par, int n);",
                  "int fs_heat_apply(fs_sim* s);", "int fs_heat_transport(fs_sim* s);",
                  "int fs_heat_budget(fs_sim* s, double out[FS_HEAT_COLS], double* per_plane);",
                  "int fs_heat_log(fs_sim* s, double* rows, long max_rows, long* n_rows, long* n_dropped);",
                  "int fs_heat_get(fs_sim* s, void* dst, size_t n_elems, int elem_size);",
                  "int fs_heat_set(fs_sim* s, const void* src, size_t n_elems, int elem_size);"):
        assert proto in text, proto
        name = proto.split("(")[0].split()[-1]
        assert name in _lib.exported_symbols() and name in _lib._SIGNATURES
    for define, value in (("FS_HEAT_PARAMS", _lib.HEAT_PARAMS), ("FS_HEAT_COLS", _lib.HEAT_COLS), ("FS_HEAT_LOG_COLS", _lib.HEAT_LOG_COLS),
                          ("FS_SOURCE_HEAT", _lib.SOURCE_HEAT)):
        assert "#define %s %d" % (define, value) in text, define
    assert _lib.HEAT_PARAMS == M.PARAMS and _lib.HEAT_COLS == M.COLS and _lib.SOURCE_HEAT == 8192


def test_set_option_has_no_heat_key():
    """The heat parameters are one atomic call of their own, not keys of fs_set_option."""
    src = open(os.path.join(CSRC, "fluidsim.cpp")).read()
    body = src[src.index("int fs_set_option("):src.index("int fs_get_int(")]
    assert "heat" not in body
