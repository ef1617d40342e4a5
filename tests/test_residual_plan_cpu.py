"""The address plan of the residual kernel (csrc/residual_plan.h), on the host: every load of every lane of every
workgroup is walked for a wide range of grids, halo depths and both element sizes -- each lies inside its allocation,
each vector load is aligned to its width, every interior cell is visited exactly once and nothing outside the interior
contributes.  The kernel (csrc/residual.hip) takes its rows, columns and offsets from this header."""
import os
import shutil
import subprocess

import pytest

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "fluid_simulation_amd", "csrc")

# Without arguments: the whole enumeration, one count of violations per invariant (and the first few violating cases).
# With arguments W H: the plan of that grid.
DRIVER = r'''
#include "residual_plan.h"
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
    if (argc == 3) {
        const fs::ResidualPlan p = fs::residual_plan(atoi(argv[1]), atoi(argv[2]));
        std::printf("%d %d %d\n", p.G, p.rc, p.nchunk);
        return 0;
    }
    std::vector<int> Ws;
    for (int w = 1; w <= 70; ++w) Ws.push_back(w);
    for (int w : {255, 256, 257, 511, 512, 513, 514, 1023, 1024}) Ws.push_back(w);
    const int Hs[] = {1, 2, 7, 16, 33}, Ds[] = {1, 2, 5};
    long cases = 0, loads = 0, multi_chunk = 0, tails = 0;
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
                        const fs::ResidualPlan p = fs::residual_plan(W, H);
                        if (p.G != (W + 3) / 4 || p.rc < 1 || p.nchunk < 1 || (long)p.rc * p.nchunk < H || (long)p.rc * (p.nchunk - 1) >= H)
                            fail("plan shape", W, H, D, zh, es);
                        if (p.nchunk > 1) ++multi_chunk;
                        std::vector<int> seen((size_t)(W + 2) * (H + 2) * (D + 2), 0);
                        for (int z = 1; z <= D; ++z)
                            for (int chunk = 0; chunk < p.nchunk; ++chunk) {
                                const int iters = fs::residual_iters(p, chunk);
                                long items = 0;
                                // one iteration beyond the kernel's loop: nothing may be left for it
                                for (int it = 0; it <= iters; ++it)
                                    for (int u = 0; u < fs::RES_U; ++u)
                                        for (int lane = 0; lane < fs::RES_FT; ++lane) {
                                            const fs::ResidualItem i = fs::residual_item(p, chunk, lane, it, u);
                                            if (!i.valid) { ++tails; continue; }
                                            if (it == iters) { fail("item beyond the loop", W, H, D, zh, es); continue; }
                                            ++items;
                                            if (i.y < 1 || i.y > H || i.x0 < 1 || i.x0 > W || (i.x0 - 1) % 4 != 0) {
                                                fail("group outside the interior", W, H, D, zh, es);
                                                continue;
                                            }
                                            const long c = i.x0 + i.y * sy + z * sz;
                                            for (int k = 0; k < fs::RES_NLOADS; ++k) {
                                                const fs::ResidualLoad l = fs::residual_load(k, sy, sz);
                                                const long e = c + l.off;
                                                const long width = l.array == fs::RES_FLAGS ? 1 : es;
                                                ++loads;
                                                if (e < -lead || e + l.elems > n - lead) fail("load outside its allocation", W, H, D, zh, es);
                                                // allocations start 256-byte aligned and arrays of a pool lie a multiple of 64 elements apart
                                                long bytes = l.elems * width;
                                                if (bytes > 16) bytes = 16;      // a 32-byte group of doubles moves as two 16-byte loads
                                                if (((e + lead) * width) % bytes != 0) fail("misaligned load", W, H, D, zh, es);
                                            }
                                            for (int j = 0; j < 4; ++j)
                                                if (i.x0 + j <= W) ++seen[(size_t)((z * (H + 2) + i.y) * (long)(W + 2) + i.x0 + j)];
                                        }
                                if (items != fs::residual_chunk_items(p, chunk)) fail("items of a chunk", W, H, D, zh, es);
                            }
                        for (int z = 0; z <= D + 1; ++z)
                            for (int y = 0; y <= H + 1; ++y)
                                for (int x = 0; x <= W + 1; ++x) {
                                    const bool interior = x >= 1 && x <= W && y >= 1 && y <= H && z >= 1 && z <= D;
                                    const int s = seen[(size_t)((z * (H + 2) + y) * (long)(W + 2) + x)];
                                    if (interior && s != 1) fail("interior cell not visited exactly once", W, H, D, zh, es);
                                    if (!interior && s != 0) fail("ghost cell contributes", W, H, D, zh, es);
                                }
                    }
    long total = 0;
    for (const auto& kv : bad) {
        std::printf("# %s: %ld\n", kv.first.c_str(), kv.second);
        total += kv.second;
    }
    std::printf("%ld %ld %ld %ld %ld\n", cases, loads, multi_chunk, tails, total);
    return 0;
}
'''


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    cxx = shutil.which("c++") or shutil.which("g++")
    if cxx is None:
        pytest.fail("no C++ compiler")
    d = tmp_path_factory.mktemp("residual_plan")
    src = d / "driver.cpp"
    src.write_text(DRIVER)
    exe = d / "driver"
    subprocess.run([cxx, "-std=c++17", "-O2", "-I", CSRC, str(src), "-o", str(exe)], check=True)
    return str(exe)


def test_every_load_of_every_lane(driver):
    """W 1..70, 255..257, 511..514, 1023, 1024 x H {1, 2, 7, 16, 33} x D {1, 2, 5} x halo depth 1..3 x fp32 / fp64: no
    violation of any invariant, and the enumeration reaches planes of several chunks and partly filled iterations."""
    out = subprocess.run([driver], check=True, capture_output=True, text=True).stdout
    cases, loads, multi_chunk, tails, bad = map(int, out.splitlines()[-1].split())
    assert bad == 0, out
    assert cases == 79 * 5 * 3 * 3 * 2 and loads > 10 ** 7 and multi_chunk > 0 and tails > 0, out


@pytest.mark.parametrize("W,H,want", [
    (512, 512, (128, 32, 16)),        # the benchmark grid: 16 workgroups of 4096 groups per plane
    (13, 7, (4, 7, 1)),
    (1024, 33, (256, 16, 3)),
    (64, 48, (16, 48, 1)),
    (4, 9000, (1, 4096, 3)),
    (20000, 3, (5000, 1, 3)),         # a row longer than a workgroup's share: one row per chunk
])
def test_plan_depends_on_the_plane_shape_only(driver, W, H, want):
    out = subprocess.run([driver, str(W), str(H)], check=True, capture_output=True, text=True).stdout.split()
    assert tuple(int(v) for v in out) == want
