// monitor.hip -- the three launches of one flow-monitor record (monitor.h).  Reads only the five fields and the flag bytes;
// writes only its workspace and the record.  Every index comes from monitor_plan.h.
#include "monitor.h"
#include <hip/hip_runtime.h>

namespace fs {

namespace {

// the six loads of one cell; f = F_SOLID where the column has no such row
template <class T>
struct MonCell {
    T q, u, v, w, p;
    unsigned f;
};

template <class T>
__device__ __forceinline__ MonCell<T> monitor_fetch(const MonitorPlan& pl, int iter, int k, int x, int z, long sy, long sz,
                                                    const T* __restrict__ q, const T* __restrict__ u, const T* __restrict__ v,
                                                    const T* __restrict__ w, const T* __restrict__ p,
                                                    const uint8_t* __restrict__ flags)
{
    MonCell<T> r{(T)0, (T)0, (T)0, (T)0, (T)0, F_SOLID};
    const int y = monitor_row(pl, iter, k);   // the same in every lane; 0 behind the column's end (the last look-ahead)
    if (y) {
        const long c = monitor_cell(x, y, z, sy, sz);
        r.f = flags[c + monitor_load(ML_FLAGS).off];
        r.q = q[c + monitor_load(ML_Q).off];
        r.u = u[c + monitor_load(ML_U).off];
        r.v = v[c + monitor_load(ML_V).off];
        r.w = w[c + monitor_load(ML_W).off];
        r.p = p[c + monitor_load(ML_P).off];
    }
    return r;
}

// The streaming pass.  A lane owns the column (z, x) monitor_plan.h deals it -- the lanes of a wave lie along x, so each of
// the six loads of a row is one run of consecutive elements -- and walks its rows in increasing y with the running values
// of the COLUMN record in registers.  The MON_U rows of the next iteration are loaded before this iteration's are added.
template <class T>
__global__ __launch_bounds__(MON_FT) void monitor_columns_kernel(MonitorPlan pl, long sy, long sz, const T* __restrict__ q,
                                                                 const T* __restrict__ u, const T* __restrict__ v,
                                                                 const T* __restrict__ w, const T* __restrict__ p,
                                                                 const uint8_t* __restrict__ flags, double* __restrict__ ws)
{
    const MonitorColumn col = monitor_column(pl, (long)blockIdx.x, (int)threadIdx.x);
    if (!col.valid) return;
    const double inf = __builtin_huge_val();
    int cells = 0, bad = 0;
    double sq = 0.0, su = 0.0, sv = 0.0, sw = 0.0, se = 0.0, sp = 0.0, suu = 0.0, squ = 0.0;
    double mu = 0.0, mv = 0.0, mw = 0.0, me = 0.0;
    double qlo = inf, qhi = -inf, plo = inf, phi = -inf;
    const int iters = monitor_iters(pl);
    MonCell<T> cur[MON_U], nxt[MON_U];
#pragma unroll
    for (int k = 0; k < MON_U; ++k) cur[k] = monitor_fetch<T>(pl, 0, k, col.x, col.z, sy, sz, q, u, v, w, p, flags);
    for (int it = 0; it < iters; ++it) {
#pragma unroll
        for (int k = 0; k < MON_U; ++k) nxt[k] = monitor_fetch<T>(pl, it + 1, k, col.x, col.z, sy, sz, q, u, v, w, p, flags);
#pragma unroll
        for (int k = 0; k < MON_U; ++k) {
            if (cur[k].f & F_SOLID) continue;
            const double dq = (double)cur[k].q, du = (double)cur[k].u, dv = (double)cur[k].v, dw = (double)cur[k].w,
                         dp = (double)cur[k].p;
            ++cells;
            if (!(__builtin_isfinite(dq) && __builtin_isfinite(du) && __builtin_isfinite(dv) && __builtin_isfinite(dw) &&
                  __builtin_isfinite(dp)))
                ++bad;
            const double uu = du * du;
            const double e = (uu + dv * dv) + dw * dw;
            sq += dq;
            su += du;
            sv += dv;
            sw += dw;
            se += e;
            sp += dp;
            suu += uu;
            squ += dq * du;
            const double au = __builtin_fabs(du), av = __builtin_fabs(dv), aw = __builtin_fabs(dw);
            if (au > mu) mu = au;
            if (av > mv) mv = av;
            if (aw > mw) mw = aw;
            if (e > me) me = e;
            if (dq < qlo) qlo = dq;
            if (dq > qhi) qhi = dq;
            if (dp < plo) plo = dp;
            if (dp > phi) phi = dp;
        }
#pragma unroll
        for (int k = 0; k < MON_U; ++k) cur[k] = nxt[k];
    }
    const double rec[MON_COL] = { (double)cells, (double)bad, sq, su, sv, sw, se, sp, suu, squ, mu, mv, mw, me, qlo, qhi, plo, phi };
#pragma unroll
    for (int k = 0; k < MON_COL; ++k) ws[monitor_column_slot(pl, col.z, col.x, k)] = rec[k];
}

// A sequential combination of n values v(0) .. v(n - 1) from `start`, in this order: kind 0 adds, 1 / -1 take the maximum /
// minimum.  The chain of a lane is serial by definition; its loads are not, so MON_B of them are in flight before the first
// is used (one lane walks hundreds of values that no other lane of its wave shares a cache line with).
constexpr int MON_B = 32;
template <int KIND>
__device__ __forceinline__ double monitor_combine(double m, double a)
{
    if (KIND == 0) return m + a;
    if (KIND > 0) return a > m ? a : m;
    return a < m ? a : m;
}
template <int KIND, class F>
__device__ __forceinline__ double monitor_fold_as(double start, int n, F&& value)
{
    double m = start;
    int i = 0;
    for (; i + MON_B <= n; i += MON_B) {
        double a[MON_B];
#pragma unroll
        for (int j = 0; j < MON_B; ++j) a[j] = value(i + j);
#pragma unroll
        for (int j = 0; j < MON_B; ++j) m = monitor_combine<KIND>(m, a[j]);
    }
    for (; i < n; ++i) m = monitor_combine<KIND>(m, value(i));
    return m;
}
// the lanes are dealt by kind (monitor_plan.h), so in all but the few waves that straddle two kinds one branch runs
template <class F>
__device__ __forceinline__ double monitor_fold(int kind, double start, int n, F&& value)
{
    if (kind == 0) return monitor_fold_as<0>(start, n, value);
    if (kind > 0) return monitor_fold_as<1>(start, n, value);
    return monitor_fold_as<-1>(start, n, value);
}

// where quantity k of a PLANE (and the WHOLE) record starts: sums and the four maxima at 0, a minimum at +Inf, a maximum at -Inf
__device__ __forceinline__ double monitor_plane_start(int k)
{
    const double inf = __builtin_huge_val();
    return k < 12 ? 0.0 : monitor_plane_kind(k) < 0 ? inf : -inf;
}

// The second launch: one lane per (plane, quantity) combines the plane's columns in increasing x, one lane per (x, quantity)
// adds the columns of that x in increasing z.
__global__ __launch_bounds__(256) void monitor_reduce_kernel(MonitorPlan pl, double* __restrict__ ws)
{
    const MonitorLane ln = monitor_reduce_lane(pl, (long)blockIdx.x * blockDim.x + threadIdx.x);
    if (ln.role == MR_PLANE) {
        const int z = ln.a, k = ln.k, src = monitor_plane_source(k);
        ws[monitor_plane_slot(pl, z, k)] = monitor_fold(monitor_plane_kind(k), monitor_plane_start(k), pl.W, [&](int xi) {
            return ws[monitor_column_slot(pl, z, 1 + xi, src)];
        });
    } else if (ln.role == MR_PROFILE) {
        const int x = ln.a, j = ln.k, src = monitor_profile_source(j);
        ws[monitor_profile_slot(pl, x, j)] = monitor_fold_as<0>(0.0, pl.D, [&](int zi) {
            return ws[monitor_column_slot(pl, 1 + zi, x, src)];
        });
    }
}

// The third launch, one workgroup: a lane per quantity of the WHOLE record combines the planes in increasing z -- a wave for
// the sums, one for the maxima, one for the minima -- and the lanes of the fourth wave copy the stations' X-PROFILE rows (an
// unused station: NaN).
__global__ __launch_bounds__(MON_WHOLE_FT) void monitor_whole_kernel(MonitorPlan pl, MonitorStations st, const double* ws,
                                                                     double* result)
{
    const MonitorLane ln = monitor_whole_lane((int)threadIdx.x);
    if (ln.role == MR_PLANE) {
        const int k = ln.k;
        result[monitor_result_whole(k)] = monitor_fold(monitor_plane_kind(k), monitor_plane_start(k), pl.D, [&](int zi) {
            return ws[monitor_plane_slot(pl, 1 + zi, k)];
        });
    } else if (ln.role == MR_PROFILE) {
        int x = 0;
#pragma unroll
        for (int s = 0; s < MON_STATIONS; ++s)
            if (s == ln.a) x = st.x[s];
        result[monitor_result_station(ln.a, ln.k)] = (x >= 1 && x <= pl.W) ? ws[monitor_profile_slot(pl, x, ln.k)] : __builtin_nan("");
    }
}

}  // namespace

size_t monitor_workspace_doubles(const GridDesc& g) { return (size_t)monitor_plan(g.W, g.H, g.D).doubles; }

template <class T>
void launch_monitor(hipStream_t st, const GridDesc& g, const T* q, const T* u, const T* v, const T* w, const T* p,
                    const uint8_t* flags, const MonitorStations& stations, double* ws, double* result)
{
    const MonitorPlan pl = monitor_plan(g.W, g.H, g.D);
    hipLaunchKernelGGL((monitor_columns_kernel<T>), dim3((unsigned)monitor_groups(pl)), dim3(MON_FT), 0, st, pl, g.sy, g.sz, q, u, v, w,
                       p, flags, ws);
    hipLaunchKernelGGL(monitor_reduce_kernel, dim3((unsigned)((monitor_reduce_lanes(pl) + 255) / 256)), dim3(256), 0, st, pl, ws);
    hipLaunchKernelGGL(monitor_whole_kernel, dim3(1), dim3(MON_WHOLE_FT), 0, st, pl, stations, ws, result);
}
template void launch_monitor<float>(hipStream_t, const GridDesc&, const float*, const float*, const float*, const float*, const float*,
                                    const uint8_t*, const MonitorStations&, double*, double*);
template void launch_monitor<double>(hipStream_t, const GridDesc&, const double*, const double*, const double*, const double*,
                                     const double*, const uint8_t*, const MonitorStations&, double*, double*);

}  // namespace fs
