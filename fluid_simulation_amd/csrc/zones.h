// zones.h -- momentum zones (include/fluidsim.h, "momentum zones"): which cells a zone holds, the arithmetic of one stage of
// the pass in zones.hip (fs_zone_apply) and what a stage adds to the zone budget (fs_zone_budget).  Plain C++ without HIP
// (inline functions, usable on the host and in the kernels), so that tests/test_zones_cpu.py compiles exactly what the
// kernels run.  Beyond the reference: it can put nothing into the flow that is not a solid voxel.  Internal to libfluidsim.so.
#pragma once

#if defined(__HIPCC__)
#define FS_ZONE_HD __host__ __device__
#else
#define FS_ZONE_HD
#endif

namespace fs {

// the entries of one zone's row (FS_ZONE_PARAMS of them)
enum {
    ZP_SHAPE = 0, ZP_AXIS, ZP_X0, ZP_X1, ZP_Y0, ZP_Y1, ZP_Z0, ZP_Z1, ZP_C1, ZP_C2, ZP_RADIUS, ZP_GX, ZP_GY, ZP_GZ, ZP_DX, ZP_DY,
    ZP_DZ, ZP_FX, ZP_FY, ZP_FZ, ZONE_PARAMS
};
// the columns of one zone's budget (FS_ZONE_COLS of them)
enum { ZC_CELLS = 0, ZC_DX, ZC_DY, ZC_DZ, ZC_DK, ZC_FLUX, ZC_MAXM, ZONE_COLS };
constexpr int ZONE_MAX = 8;        // FS_ZONE_MAX

// the two bits of a cell's flag byte the passes look at (kernels.h: F_SOLID, F_NEAR; zones.hip asserts that they agree)
constexpr unsigned ZONE_SOLID = 1u, ZONE_NEAR = 2u;

// One zone as the passes take it: G = DT * g and R2 = radius * radius are computed once, on the host (zone_make).
struct Zone {
    double c1, c2, r2;             // cylinder: centre on the two axes other than `axis` (lower axis first), radius squared
    double G[3], D[3], F[3];
    int box[6];                    // x0, x1, y0, y1, z0, z1, in cells
    int shape, axis;
    int plain;                     // D = F = 0: every denominator is 1 wherever the speed is finite
    int pad_;
};
struct ZoneTable {
    double dt;                     // DT: the handle's float member, widened
    int n, pad_;
    Zone z[ZONE_MAX];
};

// row `par` of fs_zones -> the zone; dt = DT
FS_ZONE_HD inline Zone zone_make(const double* par, double dt)
{
    Zone q;
    q.shape = (int)par[ZP_SHAPE];
    q.axis = (int)par[ZP_AXIS];
    for (int k = 0; k < 6; ++k) q.box[k] = (int)par[ZP_X0 + k];
    q.c1 = par[ZP_C1];
    q.c2 = par[ZP_C2];
    q.r2 = par[ZP_RADIUS] * par[ZP_RADIUS];
    bool plain = true;
    for (int a = 0; a < 3; ++a) {
        q.G[a] = dt * par[ZP_GX + a];
        q.D[a] = par[ZP_DX + a];
        q.F[a] = par[ZP_FX + a];
        if (q.D[a] != 0.0 || q.F[a] != 0.0) plain = false;
    }
    q.plain = plain ? 1 : 0;
    q.pad_ = 0;
    return q;
}

// does the zone's box meet the box [x0, x1] x [y0, y1] x [z0, z1]?  (what a wave asks about its footprint)
FS_ZONE_HD inline bool zone_meets(const Zone& q, int x0, int x1, int y0, int y1, int z0, int z1)
{
    return q.box[0] <= x1 && q.box[1] >= x0 && q.box[2] <= y1 && q.box[3] >= y0 && q.box[4] <= z1 && q.box[5] >= z0;
}

// is the cell IN the zone?  (whether it is a TARGET cell is the flag byte's business: zone_target)
FS_ZONE_HD inline bool zone_in(const Zone& q, int x, int y, int z)
{
    if (x < q.box[0] || x > q.box[1] || y < q.box[2] || y > q.box[3] || z < q.box[4] || z > q.box[5]) return false;
    if (q.shape == 0) return true;
    const int i = q.axis == 0 ? y : x, j = q.axis == 2 ? y : z;
    const double p = (double)i - q.c1;
    const double s = (double)j - q.c2;
    const double pp = p * p;
    const double ss = s * s;
    const double d2 = pp + ss;
    return d2 <= q.r2;
}
FS_ZONE_HD inline bool zone_target(unsigned flag) { return (flag & (ZONE_SOLID | ZONE_NEAR)) == 0; }

// the correctly rounded fp64 square root: __builtin_sqrt is sqrt() without a header, on the host and in the kernel
FS_ZONE_HD inline double zone_sqrt(double x) { return __builtin_sqrt(x); }

FS_ZONE_HD inline double zone_k(const double (&u)[3])
{
    const double xx = u[0] * u[0];
    const double yy = u[1] * u[1];
    const double zz = u[2] * u[2];
    const double xy = xx + yy;
    return xy + zz;
}

// what a stage hands to the budget
struct ZoneStage {
    double k0, m, k1;
};

// One stage, in place on u; every operation is rounded once, in this order (the library and the test driver are built
// without contraction).  The full text, which the budget always runs.
FS_ZONE_HD inline ZoneStage zone_stage(const Zone& q, double dt, double (&u)[3])
{
    ZoneStage st;
    st.k0 = zone_k(u);
    st.m = zone_sqrt(st.k0);
    for (int a = 0; a < 3; ++a) {
        const double n = u[a] + q.G[a];
        const double r = q.F[a] * st.m;
        const double s = q.D[a] + r;
        const double t = dt * s;
        const double d = 1.0 + t;
        u[a] = n / d;
    }
    st.k1 = zone_k(u);
    return st;
}

// The same values of u, for the pass, which needs nothing else.  A zone with D = F = 0 has r = 0 * m = 0, s = 0, t = 0 and
// d = 1 wherever m is finite, and n / 1.0 is n: the square root and the divisions are skipped there.  m is finite exactly
// where k0 is (a finite k0 is >= 0), and k0 - k0 is 0 for a finite k0 and NaN for Inf and NaN.
FS_ZONE_HD inline void zone_stage_apply(const Zone& q, double dt, double (&u)[3])
{
    if (q.plain) {
        const double k0 = zone_k(u);
        if (k0 - k0 == 0.0) {
            for (int a = 0; a < 3; ++a) u[a] = u[a] + q.G[a];
            return;
        }
    }
    zone_stage(q, dt, u);
}

// what the stage of zone `q` on the input `u0` (its result `u1`, its `st`) adds to the zone's seven budget values
struct ZoneSums {
    double v[ZONE_COLS];
};
FS_ZONE_HD inline ZoneSums zone_sums_start()
{
    ZoneSums s;
    for (int k = 0; k < ZONE_COLS; ++k) s.v[k] = 0.0;
    s.v[ZC_MAXM] = -__builtin_huge_val();
    return s;
}
FS_ZONE_HD inline void zone_sums_add(ZoneSums& s, const Zone& q, const double (&u0)[3], const double (&u1)[3], const ZoneStage& st)
{
    s.v[ZC_CELLS] = s.v[ZC_CELLS] + 1.0;
    for (int a = 0; a < 3; ++a) {
        const double d = u1[a] - u0[a];
        s.v[ZC_DX + a] = s.v[ZC_DX + a] + d;
    }
    const double dk = st.k1 - st.k0;
    const double e = 0.5 * dk;
    s.v[ZC_DK] = s.v[ZC_DK] + e;
    s.v[ZC_FLUX] = s.v[ZC_FLUX] + (q.axis == 0 ? u0[0] : q.axis == 1 ? u0[1] : u0[2]);
    if (st.m > s.v[ZC_MAXM]) s.v[ZC_MAXM] = st.m;
}
// how value k of two records combines: a sum, or "if (a > m) m = a"
FS_ZONE_HD inline double zone_combine(int k, double m, double a)
{
    if (k == ZC_MAXM) return a > m ? a : m;
    return m + a;
}
FS_ZONE_HD inline double zone_start(int k) { return k == ZC_MAXM ? -__builtin_huge_val() : 0.0; }

}  // namespace fs
