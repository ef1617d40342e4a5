// residual_plan.h -- the address plan of residual_kernel (residual.hip): which workgroup, lane and loop iteration takes
// which four cells, and which elements of x, x0 and the flag bytes it loads for them, with which width.  Plain C++
// without HIP (constexpr functions, usable on the host and in the kernel), so that tests/test_residual_plan_cpu.py
// can walk every load of every lane on the CPU: the kernel takes its rows, columns and offsets from here and from
// nowhere else.  Internal to libfluidsim.so.
#pragma once

namespace fs {

constexpr int RES_FT = 256;        // threads per workgroup; the summation order is defined for this size, do not tune it
constexpr int RES_U = 2;           // groups of four cells a lane has in flight (independent loads per loop iteration)
constexpr int RES_ITEMS = 4096;    // groups a workgroup takes, about: whole rows, at least one

// A plane is cut into chunks of `rc` consecutive rows, one workgroup each; rc and nchunk depend on (W, H) only, so
// a plane's partial records and the order they are added in do not depend on the launch, the slab split or timing.
struct ResidualPlan {
    int W, H;
    int G;         // groups of four x-consecutive cells per row: cells 1 + 4 k .. 4 + 4 k, k = 0 .. G - 1
    int rc;        // rows per chunk
    int nchunk;    // chunks per plane
};

constexpr ResidualPlan residual_plan(int W, int H)
{
    ResidualPlan p{W, H, (W + 3) / 4, 1, 1};
    p.rc = RES_ITEMS / p.G;
    if (p.rc > H) p.rc = H;
    if (p.rc < 1) p.rc = 1;
    p.nchunk = (H + p.rc - 1) / p.rc;
    return p;
}

// groups of chunk k (its last chunk may hold fewer rows)
constexpr int residual_chunk_items(const ResidualPlan& p, int chunk)
{
    const int left = p.H - chunk * p.rc;
    return (left < p.rc ? left : p.rc) * p.G;
}
// loop iterations of a workgroup: every lane runs them all (RES_U groups each, the tail ones empty)
constexpr int residual_iters(const ResidualPlan& p, int chunk)
{
    return (residual_chunk_items(p, chunk) + RES_FT * RES_U - 1) / (RES_FT * RES_U);
}

struct ResidualItem {
    bool valid;
    int y, x0;     // row, first of the four cells (x0 = 1 mod 4); cells with x > W do not count
};
// what lane `lane` holds as its group `u` (0 .. RES_U - 1) in iteration `iter` of chunk `chunk`
constexpr ResidualItem residual_item(const ResidualPlan& p, int chunk, int lane, int iter, int u)
{
    const int i = (iter * RES_U + u) * RES_FT + lane;
    if (i >= residual_chunk_items(p, chunk)) return ResidualItem{false, 0, 0};
    const int r = i / p.G;
    return ResidualItem{true, 1 + chunk * p.rc + r, 1 + 4 * (i - r * p.G)};
}

// The loads of one group, as offsets from its first cell c = x0 + y * sy + z * sz (elements; the flag bytes use the
// same index).  `elems` is the width of the load in elements of its array.
enum { RES_X = 0, RES_RHS = 1, RES_FLAGS = 2 };
enum { RL_C = 0, RL_YM, RL_YP, RL_ZM, RL_ZP, RL_XM, RL_XP, RL_RHS, RL_FLAGS, RES_NLOADS };
struct ResidualLoad {
    int array;     // RES_X, RES_RHS or RES_FLAGS
    long off;
    int elems;
};
constexpr ResidualLoad residual_load(int k, long sy, long sz)
{
    switch (k) {
    case RL_C: return ResidualLoad{RES_X, 0, 4};
    case RL_YM: return ResidualLoad{RES_X, -sy, 4};
    case RL_YP: return ResidualLoad{RES_X, sy, 4};
    case RL_ZM: return ResidualLoad{RES_X, -sz, 4};
    case RL_ZP: return ResidualLoad{RES_X, sz, 4};
    case RL_XM: return ResidualLoad{RES_X, -1, 1};      // left neighbour of the group's first cell
    case RL_XP: return ResidualLoad{RES_X, 4, 1};       // right neighbour of its last cell
    case RL_RHS: return ResidualLoad{RES_RHS, 0, 4};
    default: return ResidualLoad{RES_FLAGS, 0, 4};
    }
}

}  // namespace fs
