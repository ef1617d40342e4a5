// confine.h -- vorticity confinement (include/fluidsim.h, "vorticity confinement"): the per-cell arithmetic of the
// z-marching kernel in confine.hip; kernels.h has the launcher.  Plain C++ without HIP (inline functions, usable on the
// host and in the kernel), so that tests/test_confine_cpu.py compiles exactly what the kernel runs.  Beyond the
// reference: it has no body force of this kind.  Internal to libfluidsim.so.
#pragma once
#include "vortex.h"

namespace fs {

// bit k of the "neighbour is a target cell" mask, in the order of the flag byte's F_XP .. F_ZM
enum { CONFINE_XP = 0, CONFINE_XM, CONFINE_YP, CONFINE_YM, CONFINE_ZP, CONFINE_ZM };

// the correctly rounded fp64 square root: __builtin_sqrt is sqrt() without a header, on the host and in the kernel
FS_VORTEX_HD inline double confine_sqrt(double x) { return __builtin_sqrt(x); }

struct ConfineCurl {
    double wx, wy, wz, m;
};
struct ConfineForce {
    double fx, fy, fz;
    bool on;             // false: the degenerate case, the cell keeps its stored values
};

// every operation below is rounded once, in this order (the library and the test driver are built without contraction)

// omega = vortex.h's curl and m = |omega| of a target cell from its 18 neighbour values
template <class T>
FS_VORTEX_HD inline ConfineCurl confine_magnitude(const VortexNb<T>& n)
{
    ConfineCurl c;
    c.wx = vortex_wx(n);
    c.wy = vortex_wy(n);
    c.wz = vortex_wz(n);
    const double xx = c.wx * c.wx, yy = c.wy * c.wy, zz = c.wz * c.wz;
    c.m = confine_sqrt((xx + yy) + zz);
    return c;
}

// f = N x omega, N = eta / |eta|, eta = the central-difference gradient of m.  mn[k] = m of neighbour k (CONFINE_XP ..),
// read only where bit k of `bits` says that neighbour is a target cell; elsewhere the cell's own m stands in.
FS_VORTEX_HD inline ConfineForce confine_force(const ConfineCurl& c, const double (&mn)[6], unsigned bits)
{
    const double xp = ((bits >> CONFINE_XP) & 1u) ? mn[CONFINE_XP] : c.m, xm = ((bits >> CONFINE_XM) & 1u) ? mn[CONFINE_XM] : c.m;
    const double yp = ((bits >> CONFINE_YP) & 1u) ? mn[CONFINE_YP] : c.m, ym = ((bits >> CONFINE_YM) & 1u) ? mn[CONFINE_YM] : c.m;
    const double zp = ((bits >> CONFINE_ZP) & 1u) ? mn[CONFINE_ZP] : c.m, zm = ((bits >> CONFINE_ZM) & 1u) ? mn[CONFINE_ZM] : c.m;
    const double ex = 0.5 * (xp - xm);
    const double ey = 0.5 * (yp - ym);
    const double ez = 0.5 * (zp - zm);
    const double xx = ex * ex, yy = ey * ey, zz = ez * ez;
    const double e2 = (xx + yy) + zz;
    ConfineForce f = { 0.0, 0.0, 0.0, false };
    if (!(e2 > 0.0)) return f;                           // zero, underflow, NaN
    const double len = confine_sqrt(e2);
    const double nx = ex / len, ny = ey / len, nz = ez / len;
    const double a0 = ny * c.wz, a1 = nz * c.wy;
    const double b0 = nz * c.wx, b1 = nx * c.wz;
    const double c0 = nx * c.wy, c1 = ny * c.wx;
    f.fx = a0 - a1;
    f.fy = b0 - b1;
    f.fz = c0 - c1;
    f.on = true;
    return f;
}

// v' = (T)((double)v + k * f)
template <class T>
FS_VORTEX_HD inline T confine_apply(T v, double k, double f)
{
    const double kf = k * f;
    return (T)((double)v + kf);
}

}  // namespace fs
