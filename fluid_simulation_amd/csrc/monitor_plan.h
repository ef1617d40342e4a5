// monitor_plan.h -- the address plan of the flow monitor (monitor.hip): which workgroup and lane of the streaming pass owns
// which column (z, x), which rows a loop iteration takes, which elements of the five fields and the flag bytes it loads for
// them and with which width, and where every record lies in the workspace.  Plain C++ without HIP (constexpr functions,
// usable on the host and in the kernels), so that tests/test_monitor_plan_cpu.py can walk every load and every workspace
// slot on the CPU: the kernels take their indices from here and from nowhere else.  Internal to libfluidsim.so.
#pragma once

namespace fs {

constexpr int MON_FT = 256;        // lanes per workgroup of the streaming pass: 256 x-consecutive columns of one plane
constexpr int MON_U = 4;           // rows a lane loads per loop iteration; the next iteration's loads are issued before this one's sums

// the COLUMN record (include/fluidsim.h, "Flow monitor"): ten sums, four maxima that start at 0, q and p extrema
enum {
    MC_CELLS = 0, MC_NONFINITE, MC_Q, MC_U, MC_V, MC_W, MC_E, MC_P, MC_UU, MC_QU,
    MC_MAXU, MC_MAXV, MC_MAXW, MC_MAXE, MC_MINQ, MC_MAXQ, MC_MINP, MC_MAXP, MON_COL
};
constexpr int MON_PLANE = 16;      // FS_MONITOR_COLS: the PLANE and the WHOLE record
constexpr int MON_PROFILE = 5;     // FS_MONITOR_PROFILE_COLS: one X-PROFILE row
constexpr int MON_STATIONS = 8;    // FS_MONITOR_STATIONS_MAX
constexpr int MON_RESULT = MON_PLANE + MON_STATIONS * MON_PROFILE;   // what the third launch writes: a log row without its step

// which value of a COLUMN record quantity k of a PLANE record / quantity j of an X-PROFILE row is made of
constexpr int monitor_plane_source(int k) { return k < 8 ? k : k + 2; }
constexpr int monitor_profile_source(int j) { return j == 0 ? MC_CELLS : j == 1 ? MC_U : j == 2 ? MC_UU : j == 3 ? MC_P : MC_QU; }
// how quantity k of a PLANE record combines: 0 a sum, 1 a maximum (if (a > m) m = a), -1 a minimum (if (a < m) m = a)
constexpr int monitor_plane_kind(int k) { return k < 8 ? 0 : k < 12 ? 1 : (k == 12 || k == 14) ? -1 : 1; }

// The workspace, in doubles: the COLUMN records quantity by quantity, so that the lanes of the streaming pass (along x) store
// side by side and the lanes of the x-profile (along x too) load side by side; then the PLANE records, the X-PROFILE rows and
// the result of an on-demand query.
struct MonitorPlan {
    int W, H, D;
    int nxg;                 // workgroups per plane
    long planes_off;         // first double of the PLANE records = doubles of the COLUMN records
    long profile_off;
    long result_off;
    long doubles;            // the whole workspace
};

constexpr MonitorPlan monitor_plan(int W, int H, int D)
{
    MonitorPlan p{W, H, D, (W + MON_FT - 1) / MON_FT, 0, 0, 0, 0};
    p.planes_off = (long)D * MON_COL * W;
    p.profile_off = p.planes_off + (long)D * MON_PLANE;
    p.result_off = p.profile_off + (long)W * MON_PROFILE;
    p.doubles = p.result_off + MON_RESULT;
    return p;
}

constexpr long monitor_groups(const MonitorPlan& p) { return (long)p.nxg * p.D; }

struct MonitorColumn {
    bool valid;
    int z, x;
};
// the column lane `lane` of workgroup `group` owns
constexpr MonitorColumn monitor_column(const MonitorPlan& p, long group, int lane)
{
    const int x = 1 + (int)(group % p.nxg) * MON_FT + lane;
    return MonitorColumn{x <= p.W, 1 + (int)(group / p.nxg), x};
}

// loop iterations of a lane, and the row it takes as its u-th (0 .. MON_U - 1) in iteration `iter`: 0 = none, the column ended
constexpr int monitor_iters(const MonitorPlan& p) { return (p.H + MON_U - 1) / MON_U; }
constexpr int monitor_row(const MonitorPlan& p, int iter, int u)
{
    const int y = 1 + iter * MON_U + u;
    return y <= p.H ? y : 0;
}

// The loads of one cell: one element of each of the five fields and one flag byte, all at the cell's own index
// c = x + y * sy + z * sz (elements; the flag bytes use the same index).  A load one element wide is aligned wherever it lies.
enum { ML_Q = 0, ML_U, ML_V, ML_W, ML_P, ML_FLAGS, MON_NLOADS };
struct MonitorLoad {
    long off;
    int elems;
};
constexpr MonitorLoad monitor_load(int /*k*/) { return MonitorLoad{0, 1}; }
constexpr long monitor_cell(int x, int y, int z, long sy, long sz) { return (long)x + (long)y * sy + (long)z * sz; }

// where the records lie
constexpr long monitor_column_slot(const MonitorPlan& p, int z, int x, int k) { return ((long)(z - 1) * MON_COL + k) * p.W + (x - 1); }
constexpr long monitor_plane_slot(const MonitorPlan& p, int z, int k) { return p.planes_off + (long)(z - 1) * MON_PLANE + k; }
constexpr long monitor_profile_slot(const MonitorPlan& p, int x, int j) { return p.profile_off + (long)(x - 1) * MON_PROFILE + j; }

// The lanes of the second and third launch are dealt by kind, the eight sums first, then the six maxima, then the two minima:
// a lane's chain is serial, and in a wave whose lanes all combine the same way it is one addition (or one comparison) per
// value instead of all three and a selection.
constexpr int MON_NSUM = 8, MON_NMAX = 6, MON_NMIN = 2;
constexpr int monitor_max_quantity(int j) { return j < 4 ? 8 + j : j == 4 ? 13 : 15; }
constexpr int monitor_min_quantity(int j) { return j == 0 ? 12 : 14; }
enum { MR_NONE = 0, MR_PLANE, MR_PROFILE };
struct MonitorLane {
    int role;      // MR_PLANE: quantity k of plane a (second launch) or of the WHOLE record (third); MR_PROFILE: see below
    int a, k;
};
// The second launch: 8 D lanes make the sums of the planes (quantity fastest), 6 D lanes the maxima, 2 D lanes the minima; the
// lanes behind them make the X-PROFILE, quantity k of row x = a (x fastest: side-by-side loads).
constexpr long monitor_reduce_lanes(const MonitorPlan& p) { return (long)p.D * MON_PLANE + (long)p.W * MON_PROFILE; }
constexpr MonitorLane monitor_reduce_lane(const MonitorPlan& p, long i)
{
    const long D = p.D;
    if (i < 0) return MonitorLane{MR_NONE, 0, 0};
    if (i < MON_NSUM * D) return MonitorLane{MR_PLANE, 1 + (int)(i / MON_NSUM), (int)(i % MON_NSUM)};
    i -= MON_NSUM * D;
    if (i < MON_NMAX * D) return MonitorLane{MR_PLANE, 1 + (int)(i / MON_NMAX), monitor_max_quantity((int)(i % MON_NMAX))};
    i -= MON_NMAX * D;
    if (i < MON_NMIN * D) return MonitorLane{MR_PLANE, 1 + (int)(i / MON_NMIN), monitor_min_quantity((int)(i % MON_NMIN))};
    i -= MON_NMIN * D;
    if (i < (long)p.W * MON_PROFILE) return MonitorLane{MR_PROFILE, 1 + (int)(i % p.W), (int)(i / p.W)};
    return MonitorLane{MR_NONE, 0, 0};
}
// The third launch, one workgroup of four waves: wave 0 the sums of the WHOLE record, wave 1 its maxima, wave 2 its minima;
// wave 3 copies the stations' rows, MR_PROFILE: quantity k of station a.
constexpr int MON_WHOLE_FT = 256;
constexpr MonitorLane monitor_whole_lane(int t)
{
    const int w = t / 64, l = t % 64;
    if (w == 0 && l < MON_NSUM) return MonitorLane{MR_PLANE, 0, l};
    if (w == 1 && l < MON_NMAX) return MonitorLane{MR_PLANE, 0, monitor_max_quantity(l)};
    if (w == 2 && l < MON_NMIN) return MonitorLane{MR_PLANE, 0, monitor_min_quantity(l)};
    if (w == 3 && l < MON_STATIONS * MON_PROFILE) return MonitorLane{MR_PROFILE, l / MON_PROFILE, l % MON_PROFILE};
    return MonitorLane{MR_NONE, 0, 0};
}
// where the third launch puts quantity k of the WHOLE record / quantity k of station a, in its MON_RESULT doubles
constexpr int monitor_result_whole(int k) { return k; }
constexpr int monitor_result_station(int a, int k) { return MON_PLANE + a * MON_PROFILE + k; }

}  // namespace fs
