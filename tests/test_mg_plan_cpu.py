"""The level plan of solver=mg (csrc/mg_plan.h), on the host: for every slab split of a wide range of grids, the coarse levels
coarsen like one GPU, the distributed levels are a prefix that keeps the eight children of every coarse cell on one rank, the
prefix is as long as the rules allow, and the plan refuses or exports only where it must."""
import os
import shutil
import subprocess

import pytest

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "fluid_simulation_amd", "csrc")

# Without arguments: every invariant over the enumeration, one count of violations each (and the first few violating cases).
# With arguments W H Dg nranks min_planes: that plan, one line per level.
DRIVER = r'''
#include "mg_plan.h"
#include <cstdio>
#include <cstdlib>
#include <map>
#include <string>

static bool halves(int W, int H, int D)    // restated: all extents even, every half at least 4 cells
{
    return W % 2 == 0 && H % 2 == 0 && D % 2 == 0 && W >= 8 && H >= 8 && D >= 8;
}

static std::map<std::string, long> bad;

static void fail(const char* what, int W, int H, int Dg, int n, int mp, int l)
{
    if (bad[what]++ < 4)
        std::printf("# %s: %dx%dx%d nranks %d min_planes %d level %d\n", what, W, H, Dg, n, mp, l);
}

int main(int argc, char** argv)
{
    if (argc == 6) {
        const fs::MgPlan p = fs::mg_plan(atoi(argv[1]), atoi(argv[2]), atoi(argv[3]), atoi(argv[4]), atoi(argv[5]));
        std::printf("status %d first_repl %d export %d\n", p.status, p.first_repl, (int)p.export_pool);
        for (const fs::MgPlanLevel& l : p.lv) std::printf("%d %d %d %d %d\n", l.W, l.H, l.D, (int)l.dist, l.Dl);
        return 0;
    }
    const int WH[][2] = {{32, 16}, {64, 64}, {1024, 512}, {48, 40}, {24, 16}, {33, 16}, {16, 7}, {6, 16}, {8, 8}, {12, 20}};
    const int MP[] = {1, 2, 3, 4, 8, 16, 32, 64};
    long plans = 0, seams = 0, odd_coarsest = 0, refused = 0;
    for (const auto& wh : WH)
        for (int Dg = 1; Dg <= 1100; ++Dg)
            for (int n = 1; n <= 8; ++n) {
                if (Dg % n) continue;
                const int W = wh[0], H = wh[1];
                const fs::MgPlan one = fs::mg_plan(W, H, Dg, 1, 32);
                for (int mp : MP) {
                    const fs::MgPlan p = fs::mg_plan(W, H, Dg, n, mp);
                    ++plans;
                    const int nl = (int)p.lv.size();
                    // refused exactly when a rank holds an odd number of level-0 planes and a coarse level exists
                    const bool refuse = n > 1 && (Dg / n) % 2 != 0 && halves(W, H, Dg);
                    if ((p.status == fs::MgPlan::ODD_SLAB) != refuse || (p.status != fs::MgPlan::OK && !refuse)) fail("refusal", W, H, Dg, n, mp, 0);
                    if (refuse) { ++refused; continue; }
                    // an export only of something to allocate: a slab run with at least one coarse level
                    if (p.export_pool != (n > 1 && nl > 1)) fail("export", W, H, Dg, n, mp, 0);
                    // the global hierarchy does not depend on the split: halve while all extents halve
                    if (nl != (int)one.lv.size()) fail("levels vs one GPU", W, H, Dg, n, mp, 0);
                    for (int l = 0; l < nl && l < (int)one.lv.size(); ++l)
                        if (p.lv[l].W != one.lv[l].W || p.lv[l].H != one.lv[l].H || p.lv[l].D != one.lv[l].D) fail("shape vs one GPU", W, H, Dg, n, mp, l);
                    if (p.lv[0].W != W || p.lv[0].H != H || p.lv[0].D != Dg) fail("level 0", W, H, Dg, n, mp, 0);
                    for (int l = 1; l < nl; ++l) {
                        const fs::MgPlanLevel &c = p.lv[l], &f = p.lv[l - 1];
                        if (!halves(f.W, f.H, f.D) || c.W * 2 != f.W || c.H * 2 != f.H || c.D * 2 != f.D) fail("halving", W, H, Dg, n, mp, l);
                    }
                    if (halves(p.lv[nl - 1].W, p.lv[nl - 1].H, p.lv[nl - 1].D)) fail("stops early", W, H, Dg, n, mp, nl - 1);
                    // distributed levels: level 0 iff slabs, then a prefix 1 .. first_repl-1
                    if (p.lv[0].dist != (n > 1) || p.lv[0].Dl != Dg / n) fail("level 0 split", W, H, Dg, n, mp, 0);
                    if (p.first_repl < 1 || p.first_repl > nl || (n == 1 && p.first_repl != 1)) fail("first_repl range", W, H, Dg, n, mp, 0);
                    for (int l = 1; l < nl; ++l) {
                        const fs::MgPlanLevel& c = p.lv[l];
                        if (c.dist != (l < p.first_repl)) fail("prefix", W, H, Dg, n, mp, l);
                        if (c.dist && (c.D % n != 0 || c.Dl * n != c.D || c.Dl < mp)) fail("distributed level split", W, H, Dg, n, mp, l);
                        if (!c.dist && (c.Dl != c.D || c.zoff(n - 1) != 0)) fail("held-whole level", W, H, Dg, n, mp, l);
                        // a distributed level with a level below it: even planes per rank (odd only on the coarsest)
                        if (c.dist && l < nl - 1 && c.Dl % 2 != 0) fail("odd distributed parent", W, H, Dg, n, mp, l);
                        if (c.dist && l == nl - 1 && c.Dl % 2 != 0) ++odd_coarsest;
                    }
                    // the prefix is as long as the rules allow: the first level held whole could not have been distributed
                    if (n > 1 && p.first_repl < nl) {
                        const int l = p.first_repl;
                        const fs::MgPlanLevel& c = p.lv[l];
                        if (c.D % n == 0 && c.D / n >= mp && ((c.D / n) % 2 == 0 || l == nl - 1)) fail("prefix too short", W, H, Dg, n, mp, l);
                    }
                    // children of every coarse cell on one rank: coarse plane Z (global, 1-based) has fine planes 2Z-1 and 2Z;
                    // the owner of a plane of a distributed level follows from the zoff / Dl of each rank
                    for (int l = 1; l < nl && n > 1; ++l) {
                        const fs::MgPlanLevel &c = p.lv[l], &f = p.lv[l - 1];
                        if (!f.dist) break;
                        auto owner = [&](const fs::MgPlanLevel& v, int z) {
                            for (int r = 0; r < n; ++r)
                                if (z > v.zoff(r) && z <= v.zoff(r) + v.Dl) return r;
                            return -1;
                        };
                        if (!c.dist) ++seams;
                        for (int Z = 1; Z <= c.D; ++Z) {
                            const int r = owner(f, 2 * Z - 1);
                            if (r < 0 || owner(f, 2 * Z) != r) { fail("children straddle ranks", W, H, Dg, n, mp, l); break; }
                            if (c.dist && owner(c, Z) != r) { fail("coarse plane off its children's rank", W, H, Dg, n, mp, l); break; }
                        }
                        // the seam: each rank writes the planes (zoff / 2, Dl / 2) of its parent planes, which must be
                        // exactly the coarse planes whose children it holds, and all ranks together the whole level
                        if (!c.dist) {
                            int covered = 0;
                            for (int r = 0; r < n; ++r) {
                                const int z0 = f.zoff(r) / 2, dl = f.Dl / 2;
                                if (2 * z0 != f.zoff(r) || 2 * dl != f.Dl || z0 != covered) fail("seam view", W, H, Dg, n, mp, l);
                                covered = z0 + dl;
                            }
                            if (covered != c.D) fail("seam view", W, H, Dg, n, mp, l);
                        }
                    }
                }
            }
    long total = 0;
    for (const auto& kv : bad) {
        std::printf("# %s: %ld\n", kv.first.c_str(), kv.second);
        total += kv.second;
    }
    std::printf("%ld %ld %ld %ld %ld\n", plans, seams, odd_coarsest, refused, total);
    return 0;
}
'''


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    cxx = shutil.which("c++") or shutil.which("g++")
    if cxx is None:
        pytest.fail("no C++ compiler")
    d = tmp_path_factory.mktemp("mg_plan")
    src = d / "driver.cpp"
    src.write_text(DRIVER)
    exe = d / "driver"
    subprocess.run([cxx, "-std=c++17", "-O1", "-I", CSRC, str(src), "-o", str(exe)], check=True)
    return str(exe)


def plan(driver, W, H, Dg, nranks, min_planes):
    out = subprocess.run([driver, str(W), str(H), str(Dg), str(nranks), str(min_planes)], check=True, capture_output=True,
                         text=True).stdout.splitlines()
    head = out[0].split()
    levels = [tuple(int(v) for v in line.split()) for line in out[1:]]
    return dict(status=int(head[1]), first_repl=int(head[3]), export=int(head[5]), levels=levels)


def test_mg_plan_invariants_over_every_slab_split(driver):
    """Dg 1..1100, every nranks 1..8 that divides it, ten W x H pairs (odd and below 8 among them), mg_min_planes 1 .. 64:
    every invariant holds in every plan, and the enumeration reaches seams, odd coarsest levels and refusals."""
    out = subprocess.run([driver], check=True, capture_output=True, text=True).stdout
    plans, seams, odd_coarsest, refused, bad = map(int, out.splitlines()[-1].split())
    assert bad == 0, out
    assert plans > 200000 and seams > 10000 and odd_coarsest > 100 and refused > 1000, out


# level: (W, H, D, distributed, planes per rank or whole D)
@pytest.mark.parametrize("W,H,Dg,nranks,min_planes,first_repl,levels", [
    # the profiled slab shapes at the default mg_min_planes: the distribution they run with today
    (512, 512, 512, 4, 32, 3, [(512, 512, 512, 1, 128), (256, 256, 256, 1, 64), (128, 128, 128, 1, 32), (64, 64, 64, 0, 64),
                               (32, 32, 32, 0, 32), (16, 16, 16, 0, 16), (8, 8, 8, 0, 8), (4, 4, 4, 0, 4)]),
    (1024, 512, 512, 8, 32, 2, [(1024, 512, 512, 1, 64), (512, 256, 256, 1, 32), (256, 128, 128, 0, 128), (128, 64, 64, 0, 64),
                                (64, 32, 32, 0, 32), (32, 16, 16, 0, 16), (16, 8, 8, 0, 8), (8, 4, 4, 0, 4)]),
    (256, 256, 256, 4, 32, 2, [(256, 256, 256, 1, 64), (128, 128, 128, 1, 32), (64, 64, 64, 0, 64), (32, 32, 32, 0, 32),
                               (16, 16, 16, 0, 16), (8, 8, 8, 0, 8), (4, 4, 4, 0, 4)]),
    # odd seams: a distributed level with an odd number of planes per rank and a level below it is held whole instead
    (32, 16, 132, 2, 32, 1, [(32, 16, 132, 1, 66), (16, 8, 66, 0, 66), (8, 4, 33, 0, 33)]),
    (32, 16, 264, 4, 32, 1, [(32, 16, 264, 1, 66), (16, 8, 132, 0, 132), (8, 4, 66, 0, 66)]),
    (32, 32, 264, 2, 8, 2, [(32, 32, 264, 1, 132), (16, 16, 132, 1, 66), (8, 8, 66, 0, 66), (4, 4, 33, 0, 33)]),
    # an odd number of planes per rank on the coarsest level is fine: every level distributed
    (64, 64, 96, 2, 3, 5, [(64, 64, 96, 1, 48), (32, 32, 48, 1, 24), (16, 16, 24, 1, 12), (8, 8, 12, 1, 6), (4, 4, 6, 1, 3)]),
])
def test_mg_plan_pinned_shapes(driver, W, H, Dg, nranks, min_planes, first_repl, levels):
    p = plan(driver, W, H, Dg, nranks, min_planes)
    assert (p["status"], p["first_repl"], p["export"]) == (0, first_repl, 1)
    assert p["levels"] == levels


@pytest.mark.parametrize("W,H,Dg,nranks,status,export,nlevels", [
    (32, 16, 18, 2, 2, 0, 2),       # 9 planes per rank and a coarse level: refused
    (33, 16, 18, 2, 0, 0, 1),       # 9 planes per rank, but W is odd: no coarse level, nothing to refuse
    (33, 16, 32, 2, 0, 0, 1),       # no coarse level on slabs: nothing to allocate, nothing to export
    (32, 16, 6, 2, 0, 0, 1),
    (32, 16, 32, 1, 0, 0, 3),       # one GPU: never an export
    (32, 16, 32, 2, 0, 1, 3),
])
def test_mg_plan_refuses_and_exports_only_where_it_must(driver, W, H, Dg, nranks, status, export, nlevels):
    p = plan(driver, W, H, Dg, nranks, 32)
    assert (p["status"], p["export"], len(p["levels"])) == (status, export, nlevels)
