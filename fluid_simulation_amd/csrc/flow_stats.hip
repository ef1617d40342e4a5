// flow_stats.hip -- time-averaged flow statistics: the accumulation kernel (one streaming pass per sample) and the
// finalize kernel (one derived field per fetch).  The arithmetic is flow_stats.h's; this file only moves the data.
#include "flow_stats.h"
#include "kernels_dev.h"

namespace fs {

namespace {

constexpr int ST_THREADS = 256;

// Lane m of the launch owns group m of the flat layout (flow_stats.h): four consecutive cells of every array.  It loads
// the five fields' groups (one 16-byte load each for fp32, 32 bytes for fp64) and, unless FIRST, every accumulator's group
// (2 x 16 bytes) before it stores anything, adds cell by cell, and stores every accumulator's group (2 x 16 bytes).  No
// lane touches another lane's cells: no atomics, no LDS, no masks; a cell's sums depend on its own values and the order
// of the samples only.  The fields are read through their allocation-relative bases (pointer - LEAD), which the pool
// keeps 16 / 32-byte aligned; the group past the last ghost cell is inside every field's tail pad (GridDesc::n).
template <class T, int NACC, bool FIRST>
__global__ __launch_bounds__(ST_THREADS) void flow_stats_kernel(long groups, const V4<T>* __restrict__ q,
                                                                const V4<T>* __restrict__ u, const V4<T>* __restrict__ v,
                                                                const V4<T>* __restrict__ w, const V4<T>* __restrict__ p,
                                                                FlowStatsAcc acc)
{
    const long m = (long)blockIdx.x * ST_THREADS + threadIdx.x;
    if (m >= groups) return;                              // whole tail lanes of the last workgroup
    const V4<T> fq = q[m], fu = u[m], fv = v[m], fw = w[m], fp = p[m];
    V4<double> s[NACC];
    if (!FIRST) {
#pragma unroll
        for (int k = 0; k < NACC; ++k) s[k] = reinterpret_cast<const V4<double>*>(acc.a[k])[m];
    }
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        double t[NACC];
        flow_stats_terms<NACC, T>(fq.e[c], fu.e[c], fv.e[c], fw.e[c], fp.e[c], t);
#pragma unroll
        for (int k = 0; k < NACC; ++k) s[k].e[c] = flow_stats_add<FIRST>(FIRST ? 0.0 : s[k].e[c], t[k]);
    }
#pragma unroll
    for (int k = 0; k < NACC; ++k) reinterpret_cast<V4<double>*>(acc.a[k])[m] = s[k];
}

// One derived field, same lane-to-group assignment; `out` has the accumulators' layout.  Reads only the accumulators the
// selector needs.  zlo0 / zhi0: the local plane (0 / D + 1) that is an inter-slab halo and is written as 0, or -1.
template <int KIND>   // 0 raw sum, 1 mean, 2 covariance, 3 tke
__global__ __launch_bounds__(ST_THREADS) void flow_stats_finalize_kernel(long groups, long sz, FlowStatsAcc acc, int which,
                                                                         double n, int zlo0, int zhi0, double* __restrict__ out)
{
    const long m = (long)blockIdx.x * ST_THREADS + threadIdx.x;
    if (m >= groups) return;
    auto ld = [&](int k) { return reinterpret_cast<const V4<double>*>(acc.a[k])[m]; };
    V4<double> r;
    if (KIND == 0) {
        r = ld(which);
    } else if (KIND == 1) {
        const V4<double> s = ld(which);
#pragma unroll
        for (int c = 0; c < 4; ++c) r.e[c] = flow_stats_mean(s.e[c], n);
    } else if (KIND == 2) {
        const V4<double> sab = ld(which), sa = ld(flow_stats_factor_a(which)), sb = ld(flow_stats_factor_b(which));
#pragma unroll
        for (int c = 0; c < 4; ++c) r.e[c] = flow_stats_cov(sab.e[c], sa.e[c], sb.e[c], n);
    } else {
        const V4<double> su = ld(ST_U), sv = ld(ST_V), sw = ld(ST_W), suu = ld(ST_UU), svv = ld(ST_VV), sww = ld(ST_WW);
#pragma unroll
        for (int c = 0; c < 4; ++c)
            r.e[c] = flow_stats_tke(flow_stats_cov(suu.e[c], su.e[c], su.e[c], n), flow_stats_cov(svv.e[c], sv.e[c], sv.e[c], n),
                                    flow_stats_cov(sww.e[c], sw.e[c], sw.e[c], n));
    }
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        const long j = 4 * m - LEAD + c;                  // cell index: local plane z starts at z * sz
        const int z = j < 0 ? -1 : (int)(j / sz);
        if (z == zlo0 || z == zhi0) r.e[c] = 0.0;
    }
    reinterpret_cast<V4<double>*>(out)[m] = r;
}

}  // namespace

template <class T>
void launch_flow_stats(hipStream_t st, const GridDesc& g, int nacc, bool first, const T* q, const T* u, const T* v, const T* w,
                       const T* p, const FlowStatsAcc& acc)
{
    const long groups = flow_stats_groups(g.sz, g.D);
    const dim3 grid((unsigned)((groups + ST_THREADS - 1) / ST_THREADS)), block(ST_THREADS);
    auto b = [](const T* f) { return reinterpret_cast<const V4<T>*>(f - LEAD); };
#define FS_ST_LAUNCH(NACC, FIRST) \
    hipLaunchKernelGGL((flow_stats_kernel<T, NACC, FIRST>), grid, block, 0, st, groups, b(q), b(u), b(v), b(w), b(p), acc)
    if (nacc == ST_NMEAN) {
        if (first) FS_ST_LAUNCH(ST_NMEAN, true); else FS_ST_LAUNCH(ST_NMEAN, false);
    } else {
        if (first) FS_ST_LAUNCH(ST_NMOMENTS, true); else FS_ST_LAUNCH(ST_NMOMENTS, false);
    }
#undef FS_ST_LAUNCH
}
template void launch_flow_stats<float>(hipStream_t, const GridDesc&, int, bool, const float*, const float*, const float*,
                                       const float*, const float*, const FlowStatsAcc&);
template void launch_flow_stats<double>(hipStream_t, const GridDesc&, int, bool, const double*, const double*, const double*,
                                        const double*, const double*, const FlowStatsAcc&);

void launch_flow_stats_finalize(hipStream_t st, const GridDesc& g, const FlowStatsAcc& acc, int which, bool raw, long n,
                                bool zero_lo, bool zero_hi, double* out)
{
    const long groups = flow_stats_groups(g.sz, g.D);
    const dim3 grid((unsigned)((groups + ST_THREADS - 1) / ST_THREADS)), block(ST_THREADS);
    const int zlo0 = zero_lo ? 0 : -2, zhi0 = zero_hi ? g.D + 1 : -2;
    const double dn = (double)n;
#define FS_ST_FIN(KIND) \
    hipLaunchKernelGGL((flow_stats_finalize_kernel<KIND>), grid, block, 0, st, groups, g.sz, acc, which, dn, zlo0, zhi0, out)
    if (raw) FS_ST_FIN(0);
    else if (which < ST_NMEAN) FS_ST_FIN(1);
    else if (which < ST_TKE) FS_ST_FIN(2);
    else FS_ST_FIN(3);
#undef FS_ST_FIN
}

}  // namespace fs
