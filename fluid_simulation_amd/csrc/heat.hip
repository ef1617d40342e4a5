// heat.hip -- heat and buoyancy (include/fluidsim.h, "heat and buoyancy"): the streaming pass of fs_heat_apply and the three
// launches of the heat budget.  The arithmetic is heat.h's; this file only moves the data.
//
// The pass is HBM-bound: per cell it reads theta, one velocity component, the density and a flag byte, and writes theta and
// the component (21 bytes in fp32); without buoyancy (beta = alpha = 0) only theta and the flag byte move.  It marches like the
// two projection passes (kernels_dev.h): a wave owns 256 x-consecutive cells of RY rows, a lane four x-consecutive cells of
// each (one 16-byte access per array and row), and walks a chunk of planes; the tiles are dealt XCD-contiguously.  Every cell
// depends on its own values alone, so the pass works in place and needs no LDS.
#include "heat.h"
#include "kernels_dev.h"
#include "monitor_plan.h"

namespace fs {

namespace {

static_assert(HEAT_SOLID == F_SOLID && HEAT_NEAR == F_NEAR, "heat.h restates two bits of the flag byte");

constexpr int HEAT_RY = 2;

// FORCE = false (beta = alpha = 0): the velocity and the density are neither read nor written.
// Reads and writes rows 1..H of planes zbeg..zend at the 16-byte groups that start at cells x0 <= W (inside the padded row:
// x0 + 3 <= W + 3 < sy), and the ghost cells beside them (store_row_bounds, kernels_dev.h:
// cells x0-1 .. x0+4 <= W+3 < sy of rows y-1 .. y+1 of planes z-1 .. z+1); the flag bytes as one word at the same index.
template <class T, bool FORCE>
__global__ __launch_bounds__(256) void heat_apply_kernel(GridDesc g, HeatPass hp, T* __restrict__ theta, T* __restrict__ vup,
                                                          const T* __restrict__ dens, const uint8_t* __restrict__ flags,
                                                          int zc_len, int nxw, int nybg, int nblk)
{
    constexpr int RY = HEAT_RY;
    const MarchTile<T> t = march_tile<T, RY>(g, zc_len, nxw, nybg, nblk);
    if (!t.live) return;                                 // wave-uniform
    const int bv = 1 + (hp.up >> 1);                     // the boundary code of the component along `up`
    const SlabCtx whole = { 0, g.D, 1, 1 };              // both z walls are physical: single GPU
    for (int z = t.zbeg; z <= t.zend; ++z) {
        const long off = t.row0 + (long)z * g.sz;
        T th[RY][4], v[RY][4], q[RY][4];
        unsigned fl[RY];
#pragma unroll
        for (int r = 0; r < RY; ++r) {
            const bool on = t.lane_on && (t.y0 + r <= g.H);
            ld_row(theta + off + r * g.sy, on, th[r]);
            fl[r] = on ? *reinterpret_cast<const unsigned*>(flags + off + r * g.sy) : 0u;
            if constexpr (FORCE) {
                ld_row(vup + off + r * g.sy, on, v[r]);
                ld_row(dens + off + r * g.sy, on, q[r]);
            }
        }
#pragma unroll
        for (int r = 0; r < RY; ++r) {
            const int y = t.y0 + r;
            if (!(t.lane_on && y <= g.H)) continue;
            const long base = off + r * g.sy;
            T tn[4], vn[4];
            unsigned kill_t = 0, kill_v = 0;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const unsigned f = (fl[r] >> (8 * e)) & 0xffu;
                if (f & F_SOLID) kill_t |= 1u << e;
                if (f & (F_SOLID | F_NEAR)) kill_v |= 1u << e;
                tn[e] = heat_working<T>(hp, th[r][e], f, t.x0 + e, y, z);
                if constexpr (FORCE) vn[e] = heat_buoyancy<T>(hp, v[r][e], tn[e], q[r][e]);
            }
            store_row_bounds<T>(g, whole, theta, base, t.x0, y, z, tn, kill_t, 0);
            if constexpr (FORCE) store_row_bounds<T>(g, whole, vup, base, t.x0, y, z, vn, kill_v, bv);
        }
    }
}

// ---- the heat budget ------------------------------------------------------------------------------------------------------
// The COLUMN record of the column (z, x): the first seven values of a PLANE record over the column's cells, and sum u * theta.
enum { HQ_CELLS = 0, HQ_SUM, HQ_SUM2, HQ_MAX, HQ_MIN, HQ_HELD, HQ_LOSS, HQ_FLUX, HEAT_COLQ };

struct HeatPlan {
    int W, H, D;
    long planes_off, result_off, doubles;
};
__host__ __device__ inline HeatPlan heat_plan(int W, int H, int D)
{
    HeatPlan p{W, H, D, 0, 0, 0};
    p.planes_off = (long)D * HEAT_COLQ * W;
    p.result_off = p.planes_off + (long)D * HEAT_COLS;
    p.doubles = p.result_off + HEAT_COLS;
    return p;
}
__device__ __forceinline__ long heat_column_slot(const HeatPlan& p, int z, int x, int k) { return ((long)(z - 1) * HEAT_COLQ + k) * p.W + (x - 1); }
__device__ __forceinline__ long heat_plane_slot(const HeatPlan& p, int z, int k) { return p.planes_off + (long)(z - 1) * HEAT_COLS + k; }

// how value k of a PLANE record combines: 0 a sum, 1 "if (a > m) m = a" from -Inf, -1 "if (a < m) m = a" from +Inf
__device__ __forceinline__ int heat_kind(int k) { return k == HC_MAX ? 1 : k == HC_MIN ? -1 : 0; }
__device__ __forceinline__ double heat_start(int k) { return k == HC_MAX ? -__builtin_huge_val() : k == HC_MIN ? __builtin_huge_val() : 0.0; }
__device__ __forceinline__ double heat_combine(int kind, double m, double a)
{
    if (kind == 0) return m + a;
    if (kind > 0) return a > m ? a : m;
    return a < m ? a : m;
}

// The streaming pass, dealt as the flow monitor's (monitor_plan.h): a lane owns a column (z, x) -- the lanes of a wave lie
// along x -- and walks its rows in increasing y, MON_U rows loaded ahead of their sums.  The held cells (few: a body's
// surface) read their six neighbours' flag bytes and, where those count, temperatures.
template <class T>
__global__ __launch_bounds__(MON_FT) void heat_columns_kernel(MonitorPlan pl, HeatPlan hpl, HeatPass hp, long sy, long sz,
                                                              const T* __restrict__ theta, const T* __restrict__ u,
                                                              const uint8_t* __restrict__ flags, double* __restrict__ ws)
{
    const MonitorColumn col = monitor_column(pl, (long)blockIdx.x, (int)threadIdx.x);
    if (!col.valid) return;
    const int x = col.x, z = col.z;
    const bool edge = (x == 1 || x == pl.W);
    const double inf = __builtin_huge_val();
    int cells = 0, nheld = 0;
    double s1 = 0.0, s2 = 0.0, hi = -inf, lo = inf, loss = 0.0, flux = 0.0;
    const long step[6] = { -1, 1, -sy, sy, -sz, sz };
    const unsigned bit[6] = { F_XM, F_XP, F_YM, F_YP, F_ZM, F_ZP };
    const int iters = monitor_iters(pl);
    for (int it = 0; it < iters; ++it) {
        T tv[MON_U], uv[MON_U];
        unsigned fv[MON_U];
#pragma unroll
        for (int k = 0; k < MON_U; ++k) {
            const int y = monitor_row(pl, it, k);
            const long c = monitor_cell(x, y ? y : 1, z, sy, sz);
            fv[k] = y ? flags[c] : (unsigned)F_SOLID;
            tv[k] = theta[c];
            uv[k] = edge ? u[c] : (T)0;
        }
#pragma unroll
        for (int k = 0; k < MON_U; ++k) {
            if (fv[k] & F_SOLID) continue;
            const int y = monitor_row(pl, it, k);
            const long c = monitor_cell(x, y, z, sy, sz);
            const double th = (double)tv[k];
            ++cells;
            s1 += th;
            s2 += th * th;
            if (th > hi) hi = th;
            if (th < lo) lo = th;
            if (edge) flux += (double)uv[k] * th;
            if (heat_held(hp, fv[k], x, y, z)) {
                ++nheld;
                double nb[6];
                bool count[6];
#pragma unroll
                for (int j = 0; j < 6; ++j) {
                    count[j] = false;
                    nb[j] = 0.0;
                    if (fv[k] & bit[j]) {                // in range and fluid
                        const int nx = x + (j == 0 ? -1 : j == 1 ? 1 : 0), ny = y + (j == 2 ? -1 : j == 3 ? 1 : 0),
                                  nz = z + (j == 4 ? -1 : j == 5 ? 1 : 0);
                        if (!heat_held(hp, flags[c + step[j]], nx, ny, nz)) {
                            count[j] = true;
                            nb[j] = (double)theta[c + step[j]];
                        }
                    }
                }
                loss += heat_cell_loss(th, nb, count);
            }
        }
    }
    const double rec[HEAT_COLQ] = { (double)cells, s1, s2, hi, lo, (double)nheld, loss, flux };
#pragma unroll
    for (int k = 0; k < HEAT_COLQ; ++k) ws[heat_column_slot(hpl, z, x, k)] = rec[k];
}

// The second launch: one lane per (plane, value) combines the plane's columns in increasing x; the outflow and the inflow are
// the flux of the columns x = W and x = 1.
__global__ __launch_bounds__(256) void heat_planes_kernel(HeatPlan pl, double* __restrict__ ws)
{
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (long)pl.D * HEAT_COLS) return;
    const int z = 1 + (int)(i / HEAT_COLS), k = (int)(i % HEAT_COLS);
    double m;
    if (k == HC_OUT) m = ws[heat_column_slot(pl, z, pl.W, HQ_FLUX)];
    else if (k == HC_IN) m = ws[heat_column_slot(pl, z, 1, HQ_FLUX)];
    else {
        const int kind = heat_kind(k);
        m = heat_start(k);
        for (int x = 1; x <= pl.W; ++x) m = heat_combine(kind, m, ws[heat_column_slot(pl, z, x, k)]);
    }
    ws[heat_plane_slot(pl, z, k)] = m;
}

// The third launch, one wave: a lane per value of the WHOLE record combines the planes in increasing z.
__global__ __launch_bounds__(64) void heat_whole_kernel(HeatPlan pl, const double* ws, double* result)
{
    const int k = (int)threadIdx.x;
    if (k >= HEAT_COLS) return;
    const int kind = heat_kind(k);
    double m = heat_start(k);
    for (int z = 1; z <= pl.D; ++z) m = heat_combine(kind, m, ws[heat_plane_slot(pl, z, k)]);
    result[k] = m;
}

}  // namespace

template <class T>
void launch_heat_apply(hipStream_t st, const GridDesc& g, const HeatPass& p, T* theta, T* vup, const T* dens, const uint8_t* flags)
{
    const MarchLaunch m = march_launch(g, HEAT_RY);
    if (p.beta != 0.0 || p.alpha != 0.0)
        hipLaunchKernelGGL((heat_apply_kernel<T, true>), dim3(m.nblk), dim3(256), 0, st, g, p, theta, vup, dens, flags, m.zc_len, m.nxw,
                           m.nybg, m.nblk);
    else
        hipLaunchKernelGGL((heat_apply_kernel<T, false>), dim3(m.nblk), dim3(256), 0, st, g, p, theta, vup, dens, flags, m.zc_len, m.nxw,
                           m.nybg, m.nblk);
}
template void launch_heat_apply<float>(hipStream_t, const GridDesc&, const HeatPass&, float*, float*, const float*, const uint8_t*);
template void launch_heat_apply<double>(hipStream_t, const GridDesc&, const HeatPass&, double*, double*, const double*, const uint8_t*);

size_t heat_workspace_doubles(const GridDesc& g) { return (size_t)heat_plan(g.W, g.H, g.D).doubles; }
size_t heat_planes_offset(const GridDesc& g) { return (size_t)heat_plan(g.W, g.H, g.D).planes_off; }

template <class T>
void launch_heat_budget(hipStream_t st, const GridDesc& g, const HeatPass& p, const T* theta, const T* u, const uint8_t* flags,
                        double* ws, double* result)
{
    const MonitorPlan pl = monitor_plan(g.W, g.H, g.D);
    const HeatPlan hpl = heat_plan(g.W, g.H, g.D);
    hipLaunchKernelGGL((heat_columns_kernel<T>), dim3((unsigned)monitor_groups(pl)), dim3(MON_FT), 0, st, pl, hpl, p, g.sy, g.sz, theta, u,
                       flags, ws);
    hipLaunchKernelGGL(heat_planes_kernel, dim3((unsigned)(((long)g.D * HEAT_COLS + 255) / 256)), dim3(256), 0, st, hpl, ws);
    hipLaunchKernelGGL(heat_whole_kernel, dim3(1), dim3(64), 0, st, hpl, ws, result);
}
template void launch_heat_budget<float>(hipStream_t, const GridDesc&, const HeatPass&, const float*, const float*, const uint8_t*,
                                        double*, double*);
template void launch_heat_budget<double>(hipStream_t, const GridDesc&, const HeatPass&, const double*, const double*, const uint8_t*,
                                         double*, double*);

}  // namespace fs
