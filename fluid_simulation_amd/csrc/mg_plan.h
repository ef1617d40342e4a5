// mg_plan.h -- host-side level plan of the multigrid solve (multigrid.hip): the coarse levels of a grid and, on z-slabs,
// which of them are distributed like level 0 and which are held whole by every rank.  Plain C++ (no HIP), so that a CPU test
// can drive it (tests/test_mg_plan_cpu.py).
#pragma once
#include <vector>

namespace fs {

constexpr int MG_MIN_DIM = 4;

// A level is halved while all three extents are even and every half keeps at least MG_MIN_DIM cells.
inline bool mg_halvable(int W, int H, int D)
{
    return W % 2 == 0 && H % 2 == 0 && D % 2 == 0 && W / 2 >= MG_MIN_DIM && H / 2 >= MG_MIN_DIM && D / 2 >= MG_MIN_DIM;
}

struct MgPlanLevel {
    int W, H, D;       // the global level (a slab run coarsens exactly like the same run on one GPU)
    bool dist;         // distributed: rank r holds planes zoff(r)+1 .. zoff(r)+Dl (+ one halo plane per side)
    int Dl;            // planes a rank holds: D / nranks if distributed, else D (the whole level)
    int zoff(int rank) const { return dist ? rank * Dl : 0; }
};

struct MgPlan {
    static constexpr int OK = 0, ODD_SLAB = 2;      // ODD_SLAB: a rank holds an odd number of level-0 planes (refused)
    int status = OK;
    int first_repl = 1;                             // levels 1 .. first_repl-1 distributed, first_repl .. held whole
    bool export_pool = false;                       // a slab run with coarse levels: their arrays are exported to the peers
                                                    // (a grid that cannot be halved allocates nothing, so exports nothing)
    std::vector<MgPlanLevel> lv;                    // lv[0] is level 0 (the simulation grid), lv[1..] the coarse levels
};

// The hierarchy of a W x H x Dg grid split into nranks z-slabs of Dg / nranks planes (nranks = 1: one GPU, every coarse
// level held whole).  A coarse level stays distributed while every rank keeps at least min_planes planes of it.
inline MgPlan mg_plan(int W, int H, int Dg, int nranks, int min_planes)
{
    MgPlan p;
    p.lv.push_back({W, H, Dg, nranks > 1, Dg / nranks});
    bool dist = nranks > 1;
    int D = Dg;
    while (mg_halvable(W, H, D)) {
        W /= 2; H /= 2; D /= 2;
        dist = dist && D % nranks == 0 && D / nranks >= (min_planes > 1 ? min_planes : 1);
        // ... and, unless it is the coarsest level, holds an even number of them: the level below is then held whole, and
        // the planes each rank restricts into it (slab_view: half its own) must be the coarse cells whose children it holds
        if (dist && (D / nranks) % 2 != 0 && mg_halvable(W, H, D)) dist = false;
        p.lv.push_back({W, H, D, dist, dist ? D / nranks : D});
        if (dist) p.first_repl = (int)p.lv.size();
    }
    if (nranks > 1 && p.lv.size() > 1 && p.lv[0].Dl % 2 != 0) p.status = MgPlan::ODD_SLAB;  // children of a coarse cell must be one rank's
    p.export_pool = nranks > 1 && p.status == MgPlan::OK && p.lv.size() > 1;
    return p;
}

}  // namespace fs
