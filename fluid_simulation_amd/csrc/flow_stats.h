// flow_stats.h -- time-averaged flow statistics (include/fluidsim.h, "time-averaged flow statistics"): the per-cell
// arithmetic of the accumulation and finalize kernels (flow_stats.hip) and their array layout; kernels.h has the launchers.
// The arithmetic is plain C++ without HIP (inline functions, usable on the host and in the kernels), so that
// tests/test_flow_stats_cpu.py compiles exactly what the kernels run.  Beyond the reference: it has no averaging.
// Internal to libfluidsim.so.
#pragma once

#if defined(__HIPCC__)
#define FS_STATS_HD __host__ __device__
#else
#define FS_STATS_HD
#endif

namespace fs {

// accumulator order: the five sums, then the seven product sums (the order of the FS_STAT_* selectors)
enum {
    ST_Q = 0, ST_U, ST_V, ST_W, ST_P,
    ST_UU, ST_VV, ST_WW, ST_UV, ST_UW, ST_VW, ST_PP,
    ST_NMEAN = 5, ST_NMOMENTS = 12, ST_TKE = 12
};

// the two factors of product sum k (ST_UU .. ST_PP), as sum indices
FS_STATS_HD inline int flow_stats_factor_a(int k) { return k == ST_UU || k == ST_UV || k == ST_UW ? ST_U : k == ST_VV || k == ST_VW ? ST_V : k == ST_WW ? ST_W : ST_P; }
FS_STATS_HD inline int flow_stats_factor_b(int k) { return k == ST_UU ? ST_U : k == ST_VV || k == ST_UV ? ST_V : k == ST_WW || k == ST_UW || k == ST_VW ? ST_W : ST_P; }

// What one sample adds to a cell's accumulators: t[0 .. NACC - 1].  A product is (double)a * (double)b, rounded once (exact
// for fp32 fields: 24 + 24 bits), and is taken before the add.
template <int NACC, class T>
FS_STATS_HD inline void flow_stats_terms(T q, T u, T v, T w, T p, double* t)
{
    const double dq = (double)q, du = (double)u, dv = (double)v, dw = (double)w, dp = (double)p;
    t[ST_Q] = dq; t[ST_U] = du; t[ST_V] = dv; t[ST_W] = dw; t[ST_P] = dp;
    if (NACC > ST_NMEAN) {
        t[ST_UU] = du * du; t[ST_VV] = dv * dv; t[ST_WW] = dw * dw;
        t[ST_UV] = du * dv; t[ST_UW] = du * dw; t[ST_VW] = dv * dw;
        t[ST_PP] = dp * dp;
    }
}

// One accumulator, one sample: one rounding.  FIRST (the first sample after a reset) adds to +0.0 without reading the
// accumulator, so that a reset costs no pass over memory; -0.0 becomes +0.0 either way.
template <bool FIRST>
FS_STATS_HD inline double flow_stats_add(double s, double x)
{
    return FIRST ? 0.0 + x : s + x;
}

// derived fields, every operation rounded (the library and the test driver are built without contraction)
FS_STATS_HD inline double flow_stats_mean(double s, double n) { return s / n; }
FS_STATS_HD inline double flow_stats_cov(double s_ab, double s_a, double s_b, double n)
{
    const double m2 = s_ab / n;
    const double ma = s_a / n, mb = s_b / n;
    const double mm = ma * mb;
    return m2 - mm;
}
FS_STATS_HD inline double flow_stats_tke(double cuu, double cvv, double cww) { return ((cuu + cvv) + cww) * 0.5; }

// ---- array layout ----------------------------------------------------------------------------------------------------
// An accumulator array uses the fields' own pitched indexing (kernels.h, GridDesc) over the local planes 0 .. D + 1: cell
// (x, y, z) at a[x + y * sy + z * sz], a = allocation base + LEAD.  sy and sz are multiples of four and the base is an
// aligned allocation, so the cell at x = 1 of every row is 32-byte aligned in fp64 (16-byte in an fp32 field) and the whole
// range is a flat run of aligned groups of four cells: group m = cells 4 m - 3 .. 4 m, m = 0 .. groups - 1.  Row padding and
// edge groups hold no cell of the padded array and are never read back.
inline long flow_stats_groups(long sz, int D) { return sz * (long)(D + 2) / 4 + 1; }

}  // namespace fs
