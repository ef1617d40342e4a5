// heat.h -- heat and buoyancy (include/fluidsim.h, "heat and buoyancy"): the per-cell arithmetic of the streaming pass in
// heat.hip (fs_heat_apply) and of the heat budget's conductive loss (fs_heat_budget).  Plain C++ without HIP (inline
// functions, usable on the host and in the kernels), so that tests/test_heat_cpu.py compiles exactly what the kernels run.
// Beyond the reference: it transports one passive scalar and has no body force.  Internal to libfluidsim.so.
#pragma once

#if defined(__HIPCC__)
#define FS_HEAT_HD __host__ __device__
#else
#define FS_HEAT_HD
#endif

namespace fs {

// the entries of fs_heat_params' array (FS_HEAT_PARAMS of them)
enum {
    HP_MODE = 0, HP_KAPPA, HP_BETA, HP_ALPHA, HP_UP, HP_INLET, HP_WALL, HP_WALL_T, HP_X0, HP_X1, HP_Y0, HP_Y1, HP_Z0, HP_Z1,
    HP_LOG, HEAT_PARAMS
};
// the columns of a PLANE and of the WHOLE record of the heat budget (FS_HEAT_COLS of them)
enum { HC_CELLS = 0, HC_SUM, HC_SUM2, HC_MAX, HC_MIN, HC_HELD, HC_LOSS, HC_OUT, HC_IN, HEAT_COLS };

// the two bits of a cell's flag byte the passes look at (kernels.h: F_SOLID, F_NEAR; heat.hip asserts that they agree)
constexpr unsigned HEAT_SOLID = 1u, HEAT_NEAR = 2u;

// what one pass needs of the parameters
struct HeatPass {
    double beta, alpha, dt;      // dt: the handle's float member, widened
    double inlet, wall_t;
    int up;                      // 0..5 = +x, -x, +y, -y, +z, -z
    int wall;                    // 1: near-wall fluid cells inside the box are held at wall_t
    int box[6];                  // x0, x1, y0, y1, z0, z1, in cells
};

// is the cell one whose temperature the wall holds?
FS_HEAT_HD inline bool heat_held(const HeatPass& p, unsigned flag, int x, int y, int z)
{
    return p.wall != 0 && !(flag & HEAT_SOLID) && (flag & HEAT_NEAR) != 0 && x >= p.box[0] && x <= p.box[1] && y >= p.box[2] &&
           y <= p.box[3] && z >= p.box[4] && z <= p.box[5];
}

// step 1: the working value of an interior cell -- its own, the inlet's on the plane x = 1, the wall's where it is held
template <class T>
FS_HEAT_HD inline T heat_working(const HeatPass& p, T theta, unsigned flag, int x, int y, int z)
{
    T t = theta;
    if (x == 1) t = (T)p.inlet;
    if (heat_held(p, flag, x, y, z)) t = (T)p.wall_t;
    return t;
}

// step 2: v_up' = (T)((double)v_up +- dt * (beta * theta' - alpha * q)); every operation is rounded once, in this order
// (the library and the test driver are built without contraction)
template <class T>
FS_HEAT_HD inline T heat_buoyancy(const HeatPass& p, T v, T theta_new, T q)
{
    const double b = p.beta * (double)theta_new;
    const double w = p.alpha * (double)q;
    const double d = b - w;
    const double f = p.dt * d;
    return (p.up & 1) ? (T)((double)v - f) : (T)((double)v + f);
}

// The conductive loss of a held cell: the sum over its in-range, fluid, not-held neighbours, in the order x-, x+, y-, y+, z-,
// z+, of (theta_c - theta_nb).  count[k] says whether neighbour k counts, nb[k] is its temperature (read only where it counts).
FS_HEAT_HD inline double heat_cell_loss(double theta_c, const double (&nb)[6], const bool (&count)[6])
{
    double s = 0.0;
    for (int k = 0; k < 6; ++k)
        if (count[k]) {
            const double d = theta_c - nb[k];
            s = s + d;
        }
    return s;
}

}  // namespace fs
