// vortex.h -- vortex identification (include/fluidsim.h, "vortex identification"): the per-cell arithmetic of the
// z-marching kernel in vortex.hip; kernels.h has the launcher.  Plain C++ without HIP (inline functions, usable on the
// host and in the kernel), so that tests/test_vortex_cpu.py compiles exactly what the kernel runs.  Beyond the
// reference: it has no vorticity and no Q-criterion.  Internal to libfluidsim.so.
#pragma once

#if defined(__HIPCC__)
#define FS_VORTEX_HD __host__ __device__
#else
#define FS_VORTEX_HD
#endif

namespace fs {

// selector order of FS_VORTEX_*
enum { VORTEX_WX = 0, VORTEX_WY, VORTEX_WZ, VORTEX_W2, VORTEX_Q, VORTEX_NFIELDS };

// The 18 neighbour values of a cell: a_bp / a_bm = component a (u = v_x, v = v_y, w = v_z) one cell towards +b / -b.
// A function reads only the members its formula names; the kernel fills only those.
template <class T>
struct VortexNb {
    T u_xp, u_xm, u_yp, u_ym, u_zp, u_zm;
    T v_xp, v_xm, v_yp, v_ym, v_zp, v_zm;
    T w_xp, w_xm, w_yp, w_ym, w_zp, w_zm;
};

// Which of its x / y / z neighbours selector `sel` reads of component `comp` (0 u, 1 v, 2 w): what the kernel loads.
FS_VORTEX_HD constexpr bool vortex_needs(int sel, int comp, int axis)
{
    return sel == VORTEX_Q ? true
         : comp == axis    ? false                                   // the diagonal g_aa enters Q only
         : sel == VORTEX_W2 ? true
         : sel != comp && sel != axis;                               // W_s = 0.5 * (D_a c - D_c a) over the two others
}

// D_b f = f[+1 along b] - f[-1 along b] in fp64 on the widened stored values: one rounding (none for fp32 fields)
template <class T>
FS_VORTEX_HD inline double vortex_diff(T plus, T minus) { return (double)plus - (double)minus; }

// every operation below is rounded once, in this order (the library and the test driver are built without contraction)
template <class T>
FS_VORTEX_HD inline double vortex_wx(const VortexNb<T>& n)
{
    const double a = vortex_diff(n.w_yp, n.w_ym), b = vortex_diff(n.v_zp, n.v_zm);
    return 0.5 * (a - b);
}
template <class T>
FS_VORTEX_HD inline double vortex_wy(const VortexNb<T>& n)
{
    const double a = vortex_diff(n.u_zp, n.u_zm), b = vortex_diff(n.w_xp, n.w_xm);
    return 0.5 * (a - b);
}
template <class T>
FS_VORTEX_HD inline double vortex_wz(const VortexNb<T>& n)
{
    const double a = vortex_diff(n.v_xp, n.v_xm), b = vortex_diff(n.u_yp, n.u_ym);
    return 0.5 * (a - b);
}
// |omega|^2 (no square root: callers take it)
template <class T>
FS_VORTEX_HD inline double vortex_w2(const VortexNb<T>& n)
{
    const double wx = vortex_wx(n), wy = vortex_wy(n), wz = vortex_wz(n);
    const double xx = wx * wx, yy = wy * wy, zz = wz * wz;
    return (xx + yy) + zz;
}
// Q = -1/2 g_ij g_ji with g_ab = 0.5 * D_b a (the factor is exact)
template <class T>
FS_VORTEX_HD inline double vortex_q(const VortexNb<T>& n)
{
    const double gxx = 0.5 * vortex_diff(n.u_xp, n.u_xm), gxy = 0.5 * vortex_diff(n.u_yp, n.u_ym), gxz = 0.5 * vortex_diff(n.u_zp, n.u_zm);
    const double gyx = 0.5 * vortex_diff(n.v_xp, n.v_xm), gyy = 0.5 * vortex_diff(n.v_yp, n.v_ym), gyz = 0.5 * vortex_diff(n.v_zp, n.v_zm);
    const double gzx = 0.5 * vortex_diff(n.w_xp, n.w_xm), gzy = 0.5 * vortex_diff(n.w_yp, n.w_ym), gzz = 0.5 * vortex_diff(n.w_zp, n.w_zm);
    const double dxx = gxx * gxx, dyy = gyy * gyy, dzz = gzz * gzz;
    const double diag = (dxx + dyy) + dzz;
    const double oxy = gxy * gyx, oxz = gxz * gzx, oyz = gyz * gzy;
    const double off = (oxy + oxz) + oyz;
    return -0.5 * diag - off;
}

template <int SEL, class T>
FS_VORTEX_HD inline double vortex_value(const VortexNb<T>& n)
{
    return SEL == VORTEX_WX ? vortex_wx(n) : SEL == VORTEX_WY ? vortex_wy(n) : SEL == VORTEX_WZ ? vortex_wz(n)
         : SEL == VORTEX_W2 ? vortex_w2(n) : vortex_q(n);
}

}  // namespace fs
