"""The arithmetic of the tracer particles (csrc/tracers.h), on the host: a driver compiled with the host C++ compiler and
-ffp-contract=off (the library's own setting) runs exactly the inline move the kernel calls -- the same corner gather, the
same two stages, the same status rule -- over seeded random velocity fields and obstacle patterns, and every position and
status is compared bit for bit with the numpy fp64 restatement in tests/tracers_model.py, which is written from the
definition in include/fluidsim.h.  float and double fields.  Also: the slot rule of a release, and the constants of the
ctypes layer against the header."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import tracers_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "fluid_simulation_amd", "csrc")
HEADER = os.path.join(ROOT, "include", "fluidsim.h")

# stdin: "move <elem 4|8> <W> <H> <D> <n> <dt bits>", then the dense padded v_x, v_y, v_z and obs and the n x 3 positions, all
# as hex bit patterns; stdout: per particle "x y z" as hex bit patterns and the status.
# stdin: "slots <first> <n> <C>"; stdout: tracer_released of every slot.
DRIVER = r'''
#include "tracers.h"
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
template <class E> static int run(int W, int H, int D, int n, float dt)
{
    const size_t cells = (size_t)(W + 2) * (H + 2) * (D + 2);
    std::vector<E> f[4];
    for (auto& a : f) {
        a.resize(cells);
        for (E& v : a) v = rd<E>();
    }
    const double k[3] = { (double)dt * (double)W, (double)dt * (double)H, (double)dt * (double)D };
    for (int i = 0; i < n; ++i) {
        double P[3] = { rd<double>(), rd<double>(), rd<double>() };
        const int status = tracer_move<E>(f[0].data(), f[1].data(), f[2].data(), f[3].data(), W, H, D, W + 2,
                                          (long)(W + 2) * (H + 2), k, P);
        for (int a = 0; a < 3; ++a) {
            uint64_t b;
            std::memcpy(&b, &P[a], 8);
            std::printf("%016llx ", (unsigned long long)b);
        }
        std::printf("%d\n", status);
    }
    return 0;
}
int main()
{
    char what[16];
    if (std::scanf("%15s", what) != 1) return 2;
    if (!std::strcmp(what, "slots")) {
        int first, n, C;
        if (std::scanf("%d %d %d", &first, &n, &C) != 3) return 2;
        for (int s = 0; s < C; ++s) std::printf("%d\n", tracer_released(s, first, n, C));
        return 0;
    }
    int elem, W, H, D, n;
    if (std::scanf("%d %d %d %d %d", &elem, &W, &H, &D, &n) != 5) return 2;
    const float dt = rd<float>();
    return elem == 4 ? run<float>(W, H, D, n, dt) : run<double>(W, H, D, n, dt);
}
'''


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.dtype.itemsize == 4 else np.uint64).reshape(-1)


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++")
    if cxx is None:
        pytest.fail("no C++ compiler")
    d = tmp_path_factory.mktemp("tracers_cpu")
    src = d / "driver.cpp"
    src.write_text(DRIVER)
    exe = d / "driver"
    subprocess.run([cxx, "-std=c++17", "-O2", "-Wall", "-Werror", "-Wno-maybe-uninitialized", "-ffp-contract=off", "-I", CSRC,
                    str(src), "-o", str(exe)], check=True)

    def text(cmd):
        return subprocess.run([str(exe)], input=cmd, capture_output=True, text=True, check=True).stdout

    def move(vx, vy, vz, obs, dt, points):
        """-> (n, 3) float64 positions, (n,) int status"""
        d2, h2, w2 = vx.shape
        cmd = "move %d %d %d %d %d %x\n" % (vx.dtype.itemsize, w2 - 2, h2 - 2, d2 - 2, points.shape[0], int(bits(np.float32(dt))[0]))
        for a in (vx, vy, vz, obs, points):
            cmd += " ".join("%x" % int(b) for b in bits(a)) + "\n"
        rows = [line.split() for line in text(cmd).splitlines()]
        xyz = np.array([[int(t, 16) for t in r[:3]] for r in rows], dtype=np.uint64).view(np.float64).reshape(-1, 3)
        return xyz, np.array([int(r[3]) for r in rows], dtype=np.int32)

    move.slots = lambda first, n, C: [int(t) for t in text("slots %d %d %d\n" % (first, n, C)).split()]
    return move


def random_case(dtype, shape, seed, n_random=200):
    """rough velocities of a few cells per step, a few NaN and infinite cells, one cell in five solid; points spread
    over B, on its faces and corners, and next to the faces with the velocity pointing out"""
    w, h, d = shape
    rng = np.random.default_rng(seed)
    full = (d + 2, h + 2, w + 2)
    dt = 0.05
    k = M.displacement(dt, shape)
    vel = [(rng.standard_normal(full) * 1.5 / k[a]).astype(dtype) for a in range(3)]
    for f in vel:
        f[rng.random(full) < 0.1] = 0.0
        f[rng.random(full) < 0.004] = np.nan
        f[rng.random(full) < 0.002] = np.inf
        f[rng.random(full) < 0.002] = -np.inf
    obs = (rng.random(full) < 0.2).astype(dtype)
    obs[rng.random(full) < 0.03] = dtype(0.5)                  # neither 0 nor 1: not solid
    for f in vel:                                              # most solid cells hold no velocity, as in a run
        f[(obs == 1) & (rng.random(full) < 0.7)] = 0.0
    lo, hi = np.full(3, 0.5), np.array(shape, dtype=np.float64) + 0.5
    pts = [lo + rng.random((n_random, 3)) * (hi - lo)]
    face = lo + rng.random((48, 3)) * (hi - lo)                # on the faces, edges and corners of B
    pick = rng.integers(0, 3, size=(48, 3))
    face = np.where(pick == 0, lo, np.where(pick == 1, hi, face))
    pts.append(face)
    pts.append(np.array([lo, hi, [lo[0], hi[1], lo[2]], [hi[0], lo[1], hi[2]]]))
    pts.append(np.nextafter(face[:16], 0.5 * (lo + hi)))       # one ulp inside them
    cells = np.stack([rng.integers(1, w + 1, 24), rng.integers(1, h + 1, 24), rng.integers(1, d + 1, 24)], axis=1).astype(np.float64)
    pts.append(cells)                                          # cell centres
    pts.append(np.clip(cells + rng.choice([-0.5, 0.5], size=cells.shape), lo, hi))   # and cell faces: floor(c + 0.5) ties
    return vel, obs, dt, np.ascontiguousarray(np.concatenate(pts, axis=0))


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("shape", [(9, 7, 5), (5, 4, 3)], ids=lambda s: "x".join(map(str, s)))
def test_driver_matches_model(driver, dtype, shape):
    vel, obs, dt, pts = random_case(dtype, shape, seed=777 + shape[0])
    assert M.in_box(pts, shape).all() and pts.shape[0] >= 300
    got_xyz, got_status = driver(vel[0], vel[1], vel[2], obs, dt, pts)
    want_xyz, want_status, mid_in = M.move(vel[0], vel[1], vel[2], obs, dt, pts)
    assert M.same_bits(got_xyz, want_xyz), np.flatnonzero(~((got_xyz == want_xyz) | (np.isnan(got_xyz) & np.isnan(want_xyz))).all(axis=1))[:8]
    assert np.array_equal(got_status, want_status), np.flatnonzero(got_status != want_status)[:8]
    # every class is there: alive, out through the midpoint, out at the end point, out by NaN, hit
    nan = np.isnan(want_xyz).any(axis=1)
    assert (want_status == M.ALIVE).sum() >= 20 and (want_status == M.HIT).sum() >= 10
    assert (~mid_in & ~nan).sum() >= 10 and (mid_in & (want_status == M.OUT) & ~nan).sum() >= 5 and nan.sum() >= 3
    assert (want_status[nan] == M.OUT).all()
    moved = (want_xyz != pts).any(axis=1)
    assert moved.sum() > 0.8 * len(pts)


def test_hand_cases(driver):
    """A uniform flow moves exactly; a particle inside a solid cell does not move and is HIT; the midpoint leaving B ends
    the move there; a NaN velocity gives NaN and OUT."""
    w, h, d = 16, 16, 4
    full = (d + 2, h + 2, w + 2)
    vx, vy, vz = (np.full(full, v, dtype=np.float32) for v in (0.25, -0.125, 0.5))
    obs = np.zeros(full, dtype=np.float32)
    dt = 0.0625                                               # k = (1, 1, 0.25)
    pts = np.array([[2.0, 8.0, 1.5], [16.25, 8.0, 1.5], [5.0, 5.0, 4.5]])
    xyz, status = driver(vx, vy, vz, obs, dt, pts)
    assert xyz[0].tolist() == [2.25, 7.875, 1.625] and status[0] == M.ALIVE
    assert xyz[1].tolist() == [16.5, 7.875, 1.625] and status[1] == M.ALIVE      # x = N + 0.5 is still in B
    assert xyz[2].tolist() == [5.125, 4.9375, 4.5625] and status[2] == M.OUT     # the midpoint left B: P' is the midpoint
    obs[2, 8, 2] = 1.0
    for f in (vx, vy, vz):
        f[1:4, 7:10, 1:4] = 0.0
    xyz, status = driver(vx, vy, vz, obs, dt, np.array([[2.25, 7.75, 2.0]]))
    assert xyz[0].tolist() == [2.25, 7.75, 2.0] and status[0] == M.HIT
    vy[3, 3, 3] = np.nan
    xyz, status = driver(vx, vy, vz, obs, dt, np.array([[3.0, 3.0, 3.0], [2.0, 3.0, 3.0]]))
    assert np.isnan(xyz[0, 1]) and status[0] == M.OUT and not np.isnan(xyz[0, 0])
    assert np.isnan(xyz[1, 1]) and status[1] == M.OUT        # a NaN corner of weight 0 still counts
    for case in (pts, np.array([[2.25, 7.75, 2.0], [3.0, 3.0, 3.0]])):
        want_xyz, want_status, _ = M.move(vx, vy, vz, obs, dt, case)
        got_xyz, got_status = driver(vx, vy, vz, obs, dt, case)
        assert M.same_bits(got_xyz, want_xyz) and np.array_equal(got_status, want_status)


@pytest.mark.parametrize("first,n,C", [(0, 0, 5), (3, 4, 10), (8, 4, 10), (2, 10, 10), (7, 23, 10), (0, 4096, 64), (5, 1, 1)])
def test_release_slots(driver, first, n, C):
    """the slot rule of a release: particle e goes into slot (first + e) % C, the later ones overwrite the earlier"""
    want = [-1] * C
    for e in range(n):
        want[(first + e) % C] = e
    assert driver.slots(first, n, C) == want


def test_python_constants_match_header():
    from fluid_simulation_amd import _lib
    import fluid_simulation_amd as F
    text = open(HEADER).read()
    enum = dict((k, int(v)) for k, v in re.findall(r"\b(FS_TRACER_[A-Z]+)\s*=\s*(\d+)", text))
    defs = dict((k, int(v)) for k, v in re.findall(r"#define\s+(FS_TRACER_[A-Z_]+)\s+(\d+)", text))
    assert enum == {"FS_TRACER_FREE": _lib.TRACER_FREE, "FS_TRACER_ALIVE": _lib.TRACER_ALIVE, "FS_TRACER_OUT": _lib.TRACER_OUT,
                    "FS_TRACER_HIT": _lib.TRACER_HIT}
    assert defs == {"FS_TRACER_EMITTERS_MAX": _lib.TRACER_EMITTERS_MAX, "FS_TRACER_FRAME_BYTES": _lib.TRACER_FRAME_BYTES}
    assert (_lib.TRACER_FREE, _lib.TRACER_ALIVE, _lib.TRACER_OUT, _lib.TRACER_HIT) == (0, 1, 2, 3) == (M.FREE, M.ALIVE, M.OUT, M.HIT)
    assert (_lib.TRACER_EMITTERS_MAX, _lib.TRACER_FRAME_BYTES) == (4096, 28) == (M.EMITTERS_MAX, M.FRAME_BYTES)
    assert len(_lib.TRACER_STATUS_NAMES) == 4
    for name in ("TRACER_FREE", "TRACER_ALIVE", "TRACER_OUT", "TRACER_HIT", "TRACER_EMITTERS_MAX", "TRACER_FRAME_BYTES"):
        assert getattr(F, name) == getattr(_lib, name)
    src = open(os.path.join(CSRC, "tracers.h")).read()
    assert "TRACER_FRAME_BYTES = %d" % _lib.TRACER_FRAME_BYTES in src


def test_viewer_pathlines_cut_where_not_alive():
    """host-side grouping of a snapshot log: one list of polylines per slot, cut where the slot was not ALIVE"""
    from fluid_simulation_amd import viewer
    status = np.array([[1, 0, 1], [1, 1, 3], [2, 1, 1], [1, 1, 1]], dtype=np.int32)       # (frames, slots)
    xyz = np.arange(4 * 3 * 3, dtype=np.float64).reshape(4, 3, 3)
    paths = viewer.pathlines({"step": np.arange(1, 5), "xyz": xyz, "status": status})
    assert [len(p) for p in paths] == [2, 1, 2]
    assert np.array_equal(paths[0][0], xyz[0:2, 0]) and np.array_equal(paths[0][1], xyz[3:4, 0])
    assert np.array_equal(paths[1][0], xyz[1:4, 1])
    assert np.array_equal(paths[2][0], xyz[0:1, 2]) and np.array_equal(paths[2][1], xyz[2:4, 2])
    assert viewer.pathlines({"step": np.zeros(0), "xyz": np.zeros((0, 5, 3)), "status": np.zeros((0, 5), dtype=np.int32)}) == [[]] * 5
