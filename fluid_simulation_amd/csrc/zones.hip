// zones.hip -- momentum zones (include/fluidsim.h, "momentum zones"): the streaming pass of fs_zone_apply, the three launches of
// the zone budget and the mask of fs_zone_mask.  The arithmetic is zones.h's; this file only moves the data.
//
// The pass is HBM-bound: per cell it reads the three velocity components and a flag byte and writes the components (25 bytes
// in fp32).  It marches like the heat pass (heat.hip, kernels_dev.h): a wave owns 256 x-consecutive cells of RY rows, a lane
// four x-consecutive cells of each (one 16-byte access per array and row), and walks a chunk of planes; the tiles are dealt
// XCD-contiguously.  Every cell depends on its own values alone, so the pass works in place and needs no LDS.  The zone table
// is a kernel argument (about 1 KB), read with wave-uniform indices; a wave first drops the zones whose box misses its
// footprint, so the fp64 square root and divisions are paid inside zones only -- everywhere else the pass copies with bounds.
#include "zones.h"
#include "kernels_dev.h"
#include "monitor_plan.h"

namespace fs {

namespace {

static_assert(ZONE_SOLID == F_SOLID && ZONE_NEAR == F_NEAR, "zones.h restates two bits of the flag byte");
static_assert(ZONE_MAX * ZONE_COLS <= 64, "the third launch of the budget is one wave");

constexpr int ZONE_RY = 2;

// Reads and writes rows 1..H of planes zbeg..zend at the 16-byte groups that start at cells x0 <= W (inside the padded row:
// x0 + 3 <= W + 3 < sy), and the ghost cells beside them (store_row_bounds, kernels_dev.h: cells x0-1 .. x0+4 <= W+3 < sy of
// rows y-1 .. y+1 of planes z-1 .. z+1); the flag bytes as one word at the same index.  Exactly heat_apply_kernel's accesses.
template <class T>
__global__ __launch_bounds__(256) void zone_apply_kernel(GridDesc g, ZoneTable zt, T* __restrict__ vx, T* __restrict__ vy,
                                                          T* __restrict__ vz, const uint8_t* __restrict__ flags, int zc_len, int nxw,
                                                          int nybg, int nblk)
{
    constexpr int RY = ZONE_RY;
    const MarchTile<T> t = march_tile<T, RY>(g, zc_len, nxw, nybg, nblk);
    if (!t.live) return;                                 // wave-uniform
    const SlabCtx whole = { 0, g.D, 1, 1 };              // both z walls are physical: single GPU
    // the zones whose box meets this wave's footprint (wave-uniform: lane 0's first cell, the wave's rows and planes)
    const int fx0 = __builtin_amdgcn_readfirstlane(t.x0);
    unsigned live = 0;
    for (int k = 0; k < zt.n; ++k)
        if (zone_meets(zt.z[k], fx0, fx0 + 255, t.y0, t.y0 + RY - 1, t.zbeg, t.zend)) live |= 1u << k;
    for (int z = t.zbeg; z <= t.zend; ++z) {
        const long off = t.row0 + (long)z * g.sz;
        unsigned lz = 0;                                 // ... and this plane
        for (unsigned m = live; m; m &= m - 1) {
            const int k = __builtin_ctz(m);
            if (z >= zt.z[k].box[4] && z <= zt.z[k].box[5]) lz |= 1u << k;
        }
        T ax[RY][4], ay[RY][4], az[RY][4];
        unsigned fl[RY];
#pragma unroll
        for (int r = 0; r < RY; ++r) {
            const bool on = t.lane_on && (t.y0 + r <= g.H);
            ld_row(vx + off + r * g.sy, on, ax[r]);
            ld_row(vy + off + r * g.sy, on, ay[r]);
            ld_row(vz + off + r * g.sy, on, az[r]);
            fl[r] = on ? *reinterpret_cast<const unsigned*>(flags + off + r * g.sy) : 0u;
        }
#pragma unroll
        for (int r = 0; r < RY; ++r) {
            const int y = t.y0 + r;
            if (!(t.lane_on && y <= g.H)) continue;
            const long base = off + r * g.sy;
            unsigned kill = 0;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const unsigned f = (fl[r] >> (8 * e)) & 0xffu;
                if (!zone_target(f)) kill |= 1u << e;
            }
            if (lz) {
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const int x = t.x0 + e;
                    if (((kill >> e) & 1u) || x > g.W) continue;
                    double u[3] = { (double)ax[r][e], (double)ay[r][e], (double)az[r][e] };
                    bool hit = false;
                    for (unsigned m = lz; m; m &= m - 1) {
                        const int k = __builtin_ctz(m);      // wave-uniform: the zone is read with scalar loads
                        if (zone_in(zt.z[k], x, y, z)) {
                            zone_stage_apply(zt.z[k], zt.dt, u);
                            hit = true;
                        }
                    }
                    if (hit) {                               // a cell in no zone keeps its bits, -0.0 included
                        ax[r][e] = (T)u[0];
                        ay[r][e] = (T)u[1];
                        az[r][e] = (T)u[2];
                    }
                }
            }
            store_row_bounds<T>(g, whole, vx, base, t.x0, y, z, ax[r], kill, 1);
            store_row_bounds<T>(g, whole, vy, base, t.x0, y, z, ay[r], kill, 2);
            store_row_bounds<T>(g, whole, vz, base, t.x0, y, z, az[r], kill, 3);
        }
    }
}

// ---- the zone budget -------------------------------------------------------------------------------------------------------
// The workspace, in doubles: the COLUMN records value by value (so that lanes along x store side by side), then the PLANE
// records in the order of fs_zone_budget's per_plane -- [z][zone][value] -- then the result of an on-demand query.
struct ZonePlan {
    int W, H, D, n;
    long planes_off, result_off, doubles;
};
__host__ __device__ inline ZonePlan zone_plan(int W, int H, int D, int n)
{
    ZonePlan p{W, H, D, n, 0, 0, 0};
    p.planes_off = (long)D * n * ZONE_COLS * W;
    p.result_off = p.planes_off + (long)D * n * ZONE_COLS;
    p.doubles = p.result_off + (long)n * ZONE_COLS;
    return p;
}
__device__ __forceinline__ long zone_column_slot(const ZonePlan& p, int z, int x, int k, int c)
{
    return (((long)(z - 1) * p.n + k) * ZONE_COLS + c) * p.W + (x - 1);
}
__device__ __forceinline__ long zone_plane_slot(const ZonePlan& p, int z, int k, int c)
{
    return p.planes_off + ((long)(z - 1) * p.n + k) * ZONE_COLS + c;
}

// The first launch, dealt as the flow monitor's streaming pass (monitor_plan.h), once per zone (blockIdx.y): a lane owns a
// column (z, x) -- the lanes of a wave lie along x -- and walks the rows of the zone's box in increasing y; the rows outside
// hold no cell of the zone, and a skipped cell adds nothing.  A cell's value goes through the earlier zones' stages first.
// Reads the interior cells (x, y, z) of the box alone; writes the column's ZONE_COLS slots.
template <class T>
__global__ __launch_bounds__(MON_FT) void zone_columns_kernel(MonitorPlan pl, ZonePlan zpl, ZoneTable zt, long sy, long sz,
                                                              const T* __restrict__ vx, const T* __restrict__ vy,
                                                              const T* __restrict__ vz, const uint8_t* __restrict__ flags,
                                                              double* __restrict__ ws)
{
    const MonitorColumn col = monitor_column(pl, (long)blockIdx.x, (int)threadIdx.x);
    if (!col.valid) return;
    const int x = col.x, z = col.z, k = (int)blockIdx.y;
    const Zone& q = zt.z[k];
    ZoneSums s = zone_sums_start();
    if (x >= q.box[0] && x <= q.box[1] && z >= q.box[4] && z <= q.box[5]) {
        for (int y = q.box[2]; y <= q.box[3]; ++y) {
            if (!zone_in(q, x, y, z)) continue;
            const long c = monitor_cell(x, y, z, sy, sz);
            if (!zone_target(flags[c])) continue;
            double u[3] = { (double)vx[c], (double)vy[c], (double)vz[c] };
            for (int j = 0; j < k; ++j)
                if (zone_in(zt.z[j], x, y, z)) zone_stage_apply(zt.z[j], zt.dt, u);
            const double u0[3] = { u[0], u[1], u[2] };
            const ZoneStage st = zone_stage(q, zt.dt, u);
            zone_sums_add(s, q, u0, u, st);
        }
    }
#pragma unroll
    for (int c = 0; c < ZONE_COLS; ++c) ws[zone_column_slot(zpl, z, x, k, c)] = s.v[c];
}

// The second launch: one lane per (plane, zone, value) combines the plane's columns in increasing x.
__global__ __launch_bounds__(256) void zone_planes_kernel(ZonePlan pl, double* __restrict__ ws)
{
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    const int per = pl.n * ZONE_COLS;
    if (i >= (long)pl.D * per) return;
    const int z = 1 + (int)(i / per), k = (int)(i % per) / ZONE_COLS, c = (int)(i % per) % ZONE_COLS;
    double m = zone_start(c);
    for (int x = 1; x <= pl.W; ++x) m = zone_combine(c, m, ws[zone_column_slot(pl, z, x, k, c)]);
    ws[zone_plane_slot(pl, z, k, c)] = m;
}

// The third launch, one wave: a lane per (zone, value) combines the planes in increasing z.
__global__ __launch_bounds__(64) void zone_whole_kernel(ZonePlan pl, const double* ws, double* result)
{
    const int i = (int)threadIdx.x;
    if (i >= pl.n * ZONE_COLS) return;
    const int k = i / ZONE_COLS, c = i % ZONE_COLS;
    double m = zone_start(c);
    for (int z = 1; z <= pl.D; ++z) m = zone_combine(c, m, ws[zone_plane_slot(pl, z, k, c)]);
    result[i] = m;
}

// fs_zone_mask: a thread per byte of the dense padded array; the ghost cells take 0.  Reads the flag bytes of interior cells.
__global__ __launch_bounds__(256) void zone_mask_kernel(GridDesc g, ZoneTable zt, const uint8_t* __restrict__ flags,
                                                        uint8_t* __restrict__ dst, long total)
{
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    const int x = (int)(i % (g.W + 2)), y = (int)((i / (g.W + 2)) % (g.H + 2)), z = (int)(i / ((long)(g.W + 2) * (g.H + 2)));
    unsigned bits = 0;
    if (x >= 1 && x <= g.W && y >= 1 && y <= g.H && z >= 1 && z <= g.D && zone_target(flags[cell(g, x, y, z)]))
        for (int k = 0; k < zt.n; ++k)
            if (zone_in(zt.z[k], x, y, z)) bits |= 1u << k;
    dst[i] = (uint8_t)bits;
}

}  // namespace

template <class T>
void launch_zone_apply(hipStream_t st, const GridDesc& g, const ZoneTable& zt, T* vx, T* vy, T* vz, const uint8_t* flags)
{
    const MarchLaunch m = march_launch(g, ZONE_RY);
    hipLaunchKernelGGL((zone_apply_kernel<T>), dim3(m.nblk), dim3(256), 0, st, g, zt, vx, vy, vz, flags, m.zc_len, m.nxw, m.nybg, m.nblk);
}
template void launch_zone_apply<float>(hipStream_t, const GridDesc&, const ZoneTable&, float*, float*, float*, const uint8_t*);
template void launch_zone_apply<double>(hipStream_t, const GridDesc&, const ZoneTable&, double*, double*, double*, const uint8_t*);

size_t zone_workspace_doubles(const GridDesc& g, int n_zones) { return (size_t)zone_plan(g.W, g.H, g.D, n_zones).doubles; }
size_t zone_planes_offset(const GridDesc& g, int n_zones) { return (size_t)zone_plan(g.W, g.H, g.D, n_zones).planes_off; }

template <class T>
void launch_zone_budget(hipStream_t st, const GridDesc& g, const ZoneTable& zt, const T* vx, const T* vy, const T* vz,
                        const uint8_t* flags, double* ws, double* result)
{
    const MonitorPlan pl = monitor_plan(g.W, g.H, g.D);
    const ZonePlan zpl = zone_plan(g.W, g.H, g.D, zt.n);
    hipLaunchKernelGGL((zone_columns_kernel<T>), dim3((unsigned)monitor_groups(pl), (unsigned)zt.n), dim3(MON_FT), 0, st, pl, zpl, zt,
                       g.sy, g.sz, vx, vy, vz, flags, ws);
    hipLaunchKernelGGL(zone_planes_kernel, dim3((unsigned)(((long)g.D * zt.n * ZONE_COLS + 255) / 256)), dim3(256), 0, st, zpl, ws);
    hipLaunchKernelGGL(zone_whole_kernel, dim3(1), dim3(64), 0, st, zpl, ws, result);
}
template void launch_zone_budget<float>(hipStream_t, const GridDesc&, const ZoneTable&, const float*, const float*, const float*,
                                        const uint8_t*, double*, double*);
template void launch_zone_budget<double>(hipStream_t, const GridDesc&, const ZoneTable&, const double*, const double*, const double*,
                                         const uint8_t*, double*, double*);

void launch_zone_mask(hipStream_t st, const GridDesc& g, const ZoneTable& zt, const uint8_t* flags, uint8_t* dst)
{
    const long total = (long)(g.W + 2) * (g.H + 2) * (g.D + 2);
    hipLaunchKernelGGL(zone_mask_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, g, zt, flags, dst, total);
}

}  // namespace fs
