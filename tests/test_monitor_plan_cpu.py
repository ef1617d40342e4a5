"""The address plan of the flow monitor (csrc/monitor_plan.h), on the host: every load of every lane of every workgroup
of the streaming pass and every workspace slot of the three launches are walked for a wide range of grids, halo depths and
both element sizes -- every interior cell is visited exactly once, nothing outside the interior is read, every load lies
inside its allocation and is aligned to its width, and every slot of the workspace is written exactly once.  The kernels
(csrc/monitor.hip) take their indices from this header.  The driver is also built with AddressSanitizer and UBSan."""
import os
import shutil
import subprocess

import pytest

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "fluid_simulation_amd", "csrc")

# Without arguments: the whole enumeration, one count of violations per invariant (and the first few violating cases).
# With arguments W H D: the plan of that grid.
DRIVER = r'''
#include "monitor_plan.h"
#include <cstdio>
#include <cstdlib>
#include <map>
#include <string>
#include <vector>

static std::map<std::string, long> bad;

static void fail(const char* what, int W, int H, int D, int zh, int es)
{
    if (bad[what]++ < 4) std::printf("# %s: %dx%dx%d zh %d elem %d\n", what, W, H, D, zh, es);
}

int main(int argc, char** argv)
{
    if (argc == 4) {
        const fs::MonitorPlan p = fs::monitor_plan(atoi(argv[1]), atoi(argv[2]), atoi(argv[3]));
        std::printf("%d %ld %d %ld %ld %ld %ld\n", p.nxg, fs::monitor_groups(p), fs::monitor_iters(p), p.planes_off, p.profile_off,
                    p.result_off, p.doubles);
        return 0;
    }
    std::vector<int> Ws;
    for (int w = 1; w <= 70; ++w) Ws.push_back(w);
    for (int w : {255, 256, 257, 511, 512, 513, 1024}) Ws.push_back(w);
    const int Hs[] = {1, 2, 7, 16, 33}, Ds[] = {1, 2, 5};
    long cases = 0, loads = 0, idle_lanes = 0, tails = 0, slots = 0;
    for (int W : Ws)
        for (int H : Hs)
            for (int D : Ds)
                for (int zh = 1; zh <= 3; ++zh)
                    for (int es : {4, 8}) {
                        ++cases;
                        // GridDesc as Engine::init lays a field out (restated): row pitch, plane pitch, the elements in front
                        // of the pointer the kernels receive, the elements of the allocation; the flag bytes have the same
                        // count and the same shift, one byte each
                        const long sy = ((long)(W + 5) + 3) / 4 * 4;
                        const long sz = sy * (H + 2);
                        const long lead = 3 + (long)(zh - 1) * sz;
                        const long n = (sz * (D + 2 * zh) + 8 + 3) / 4 * 4;
                        const fs::MonitorPlan p = fs::monitor_plan(W, H, D);
                        if (p.nxg != (W + fs::MON_FT - 1) / fs::MON_FT || p.planes_off != (long)D * fs::MON_COL * W ||
                            p.profile_off != p.planes_off + (long)D * fs::MON_PLANE ||
                            p.result_off != p.profile_off + (long)W * fs::MON_PROFILE || p.doubles != p.result_off + fs::MON_RESULT ||
                            fs::monitor_iters(p) * fs::MON_U < H || (fs::monitor_iters(p) - 1) * fs::MON_U >= H)
                            fail("plan shape", W, H, D, zh, es);
                        std::vector<int> seen((size_t)(W + 2) * (H + 2) * (D + 2), 0);
                        std::vector<int> written((size_t)p.doubles, 0);
                        auto write = [&](long slot) {
                            ++slots;
                            if (slot < 0 || slot >= p.doubles) fail("slot outside the workspace", W, H, D, zh, es);
                            else ++written[(size_t)slot];
                        };
                        // the streaming pass: one workgroup beyond the launch must own nothing
                        const long groups = fs::monitor_groups(p);
                        for (long grp = 0; grp <= groups; ++grp)
                            for (int lane = 0; lane < fs::MON_FT; ++lane) {
                                const fs::MonitorColumn c = fs::monitor_column(p, grp, lane);
                                if (grp == groups) {
                                    if (c.valid && c.z <= D) fail("column beyond the launch", W, H, D, zh, es);
                                    continue;
                                }
                                if (!c.valid) { ++idle_lanes; continue; }
                                if (c.x < 1 || c.x > W || c.z < 1 || c.z > D) { fail("column outside the interior", W, H, D, zh, es); continue; }
                                int last = 0;
                                // the kernel looks one iteration ahead: that one must find no row
                                for (int it = 0; it <= fs::monitor_iters(p); ++it)
                                    for (int u = 0; u < fs::MON_U; ++u) {
                                        const int y = fs::monitor_row(p, it, u);
                                        if (!y) { ++tails; continue; }
                                        if (it == fs::monitor_iters(p)) { fail("row beyond the loop", W, H, D, zh, es); continue; }
                                        if (y != last + 1 || y > H) fail("rows not in increasing y", W, H, D, zh, es);
                                        last = y;
                                        const long cell = fs::monitor_cell(c.x, y, c.z, sy, sz);
                                        if (cell != c.x + y * sy + c.z * sz) fail("cell index", W, H, D, zh, es);
                                        for (int k = 0; k < fs::MON_NLOADS; ++k) {
                                            const fs::MonitorLoad l = fs::monitor_load(k);
                                            const long e = cell + l.off;
                                            const long width = k == fs::ML_FLAGS ? 1 : es;
                                            ++loads;
                                            if (e < -lead || e + l.elems > n - lead) fail("load outside its allocation", W, H, D, zh, es);
                                            // allocations start 256-byte aligned and arrays of a pool lie a multiple of 64 elements apart
                                            long bytes = l.elems * width;
                                            if (bytes > 16) bytes = 16;
                                            if (((e + lead) * width) % bytes != 0) fail("misaligned load", W, H, D, zh, es);
                                            if (l.off != 0 || l.elems != 1) fail("a load reads beside its cell", W, H, D, zh, es);
                                        }
                                        ++seen[(size_t)((c.z * (H + 2) + y) * (long)(W + 2) + c.x)];
                                    }
                                if (last != H) fail("column not walked to its end", W, H, D, zh, es);
                                for (int k = 0; k < fs::MON_COL; ++k) {
                                    const long s = fs::monitor_column_slot(p, c.z, c.x, k);
                                    if (s >= p.planes_off) fail("column slot outside its section", W, H, D, zh, es);
                                    write(s);
                                }
                            }
                        for (int z = 0; z <= D + 1; ++z)
                            for (int y = 0; y <= H + 1; ++y)
                                for (int x = 0; x <= W + 1; ++x) {
                                    const bool interior = x >= 1 && x <= W && y >= 1 && y <= H && z >= 1 && z <= D;
                                    const int s = seen[(size_t)((z * (H + 2) + y) * (long)(W + 2) + x)];
                                    if (interior && s != 1) fail("interior cell not visited exactly once", W, H, D, zh, es);
                                    if (!interior && s != 0) fail("ghost cell read for a value", W, H, D, zh, es);
                                }
                        // the second launch, lane by lane as the kernel decodes it (one lane beyond it must own nothing); what a
                        // lane reads must have been written; the lanes of a kind lie together
                        const long lanes = fs::monitor_reduce_lanes(p);
                        if (lanes != (long)D * fs::MON_PLANE + (long)W * fs::MON_PROFILE) fail("reduce lanes", W, H, D, zh, es);
                        if (fs::monitor_reduce_lane(p, lanes).role != fs::MR_NONE) fail("lane beyond the second launch", W, H, D, zh, es);
                        int last_kind = 0, kind_changes = 0;
                        for (long i = 0; i < lanes; ++i) {
                            const fs::MonitorLane ln = fs::monitor_reduce_lane(p, i);
                            if (ln.role == fs::MR_PLANE) {
                                const int z = ln.a, k = ln.k;
                                if (z < 1 || z > D || k < 0 || k >= fs::MON_PLANE) { fail("plane lane", W, H, D, zh, es); continue; }
                                const int src = fs::monitor_plane_source(k), kind = fs::monitor_plane_kind(k);
                                if (src < 0 || src >= fs::MON_COL || (kind == 0) != (src < fs::MC_MAXU))
                                    fail("plane source", W, H, D, zh, es);
                                if (i > 0 && kind != last_kind) ++kind_changes;
                                last_kind = kind;
                                for (int x = 1; x <= W; ++x) {
                                    const long s = fs::monitor_column_slot(p, z, x, src);
                                    if (s < 0 || s >= p.planes_off || written[(size_t)s] != 1) fail("plane reads an unwritten slot", W, H, D, zh, es);
                                }
                                const long s = fs::monitor_plane_slot(p, z, k);
                                if (s < p.planes_off || s >= p.profile_off) fail("plane slot outside its section", W, H, D, zh, es);
                                write(s);
                            } else if (ln.role == fs::MR_PROFILE) {
                                const int x = ln.a, j = ln.k;
                                if (x < 1 || x > W || j < 0 || j >= fs::MON_PROFILE) { fail("profile lane", W, H, D, zh, es); continue; }
                                const int src = fs::monitor_profile_source(j);
                                if (src < 0 || src >= fs::MC_MAXU) fail("profile source", W, H, D, zh, es);
                                for (int z = 1; z <= D; ++z) {
                                    const long s = fs::monitor_column_slot(p, z, x, src);
                                    if (s < 0 || s >= p.planes_off || written[(size_t)s] != 1) fail("profile reads an unwritten slot", W, H, D, zh, es);
                                }
                                const long s = fs::monitor_profile_slot(p, x, j);
                                if (s < p.profile_off || s >= p.result_off) fail("profile slot outside its section", W, H, D, zh, es);
                                write(s);
                            } else {
                                fail("idle lane inside the second launch", W, H, D, zh, es);
                            }
                        }
                        if (kind_changes != 2) fail("plane lanes not dealt by kind", W, H, D, zh, es);
                        // the third launch writes the result (here the slot of a query): every element once, from planes and
                        // profile rows that were written, each wave of one kind
                        for (int t = 0; t <= fs::MON_WHOLE_FT; ++t) {
                            const fs::MonitorLane ln = fs::monitor_whole_lane(t);
                            if (t == fs::MON_WHOLE_FT) {
                                if (ln.role != fs::MR_NONE) fail("lane beyond the third launch", W, H, D, zh, es);
                            } else if (ln.role == fs::MR_PLANE) {
                                if (ln.k < 0 || ln.k >= fs::MON_PLANE) { fail("whole lane", W, H, D, zh, es); continue; }
                                const int want = t / 64 == 0 ? 0 : t / 64 == 1 ? 1 : -1;
                                if (fs::monitor_plane_kind(ln.k) != want || t / 64 > 2) fail("a wave of the third launch mixes kinds", W, H, D, zh, es);
                                for (int z = 1; z <= D; ++z)
                                    if (written[(size_t)fs::monitor_plane_slot(p, z, ln.k)] != 1) fail("whole reads an unwritten slot", W, H, D, zh, es);
                                write(p.result_off + fs::monitor_result_whole(ln.k));
                            } else if (ln.role == fs::MR_PROFILE) {
                                if (ln.a < 0 || ln.a >= fs::MON_STATIONS || ln.k < 0 || ln.k >= fs::MON_PROFILE) { fail("station lane", W, H, D, zh, es); continue; }
                                for (int x : {1, W})
                                    if (written[(size_t)fs::monitor_profile_slot(p, x, ln.k)] != 1) fail("station reads an unwritten slot", W, H, D, zh, es);
                                write(p.result_off + fs::monitor_result_station(ln.a, ln.k));
                            }
                        }
                        for (long s = 0; s < p.doubles; ++s)
                            if (written[(size_t)s] != 1) { fail("slot not written exactly once", W, H, D, zh, es); break; }
                    }
    long total = 0;
    for (const auto& kv : bad) {
        std::printf("# %s: %ld\n", kv.first.c_str(), kv.second);
        total += kv.second;
    }
    std::printf("%ld %ld %ld %ld %ld %ld\n", cases, loads, idle_lanes, tails, slots, total);
    return 0;
}
'''


def build(tmp_path_factory, name, flags):
    cxx = shutil.which("g++") or shutil.which("c++")
    if cxx is None:
        pytest.fail("no C++ compiler")
    d = tmp_path_factory.mktemp(name)
    src = d / "driver.cpp"
    src.write_text(DRIVER)
    exe = d / "driver"
    subprocess.run([cxx, "-std=c++17", "-I", CSRC, str(src), "-o", str(exe)] + flags, check=True)
    return str(exe)


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    return build(tmp_path_factory, "monitor_plan", ["-O2"])


def check_enumeration(out):
    cases, loads, idle_lanes, tails, slots, bad = map(int, out.splitlines()[-1].split())
    assert bad == 0, out
    assert cases == 77 * 5 * 3 * 3 * 2 and loads > 10 ** 7 and idle_lanes > 0 and tails > 0 and slots > 10 ** 6, out


def test_every_load_and_every_slot(driver):
    """W 1..70, 255..257, 511..513, 1024 x H {1, 2, 7, 16, 33} x D {1, 2, 5} x halo depth 1..3 x fp32 / fp64: no violation of
    any invariant, and the enumeration reaches partly filled workgroups and partly filled iterations."""
    check_enumeration(subprocess.run([driver], check=True, capture_output=True, text=True).stdout)


def test_the_same_under_asan_and_ubsan(tmp_path_factory):
    exe = build(tmp_path_factory, "monitor_plan_san", ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    check_enumeration(r.stdout)


@pytest.mark.parametrize("W,H,D,want", [
    (512, 512, 512, (2, 1024, 128, 512 * 18 * 512, 512 * 18 * 512 + 512 * 16, 512 * 18 * 512 + 512 * 16 + 512 * 5,
                     512 * 18 * 512 + 512 * 16 + 512 * 5 + 56)),   # the benchmark grid: 37.7 MB of column records
    (1, 1, 1, (1, 1, 1, 18, 34, 39, 95)),
    (257, 3, 2, (2, 4, 1, 257 * 18 * 2, 257 * 36 + 32, 257 * 36 + 32 + 257 * 5, 257 * 36 + 32 + 257 * 5 + 56)),
    (13, 7, 5, (1, 5, 2, 13 * 18 * 5, 13 * 90 + 80, 13 * 90 + 80 + 65, 13 * 90 + 80 + 65 + 56)),
])
def test_plan_of_a_grid(driver, W, H, D, want):
    out = subprocess.run([driver, str(W), str(H), str(D)], check=True, capture_output=True, text=True).stdout.split()
    assert tuple(int(v) for v in out) == want
