// residual.h -- residual of a linearSolver system on the device (fs_solve_residual, fs_diffuse_residual, option
// "residual_log").  Internal to libfluidsim.so.  Beyond the reference: it never evaluates a residual (include/fluidsim.h).
#pragma once
#include "kernels.h"
#include "residual_plan.h"

namespace fs {

// A cell is FREE where setBounds leaves it to the sweep: interior, not F_SOLID and, for b = 1, 2, 3, not F_NEAR.  There
//     r = (x0 + a * (((((x[i+1] + x[i-1]) + x[j+1]) + x[j-1]) + x[l+1]) + x[l-1])) - c * x
// in fp64 from the stored values, in this order.  Per z-plane the record is
//     { sum r^2, sum x0^2, max |r|, free cells }   (fp64)
// over the plane's free cells.  A plane's record is a pure function of that plane, its two z neighbours and (W, H):
// the plane is cut into the row chunks of residual_plan.h, a workgroup of a fixed size reduces one chunk with a fixed
// assignment of cells to lanes, a fixed shuffle butterfly and a fixed wave order, and a second kernel adds a plane's
// partial records in chunk order.  No atomics -- launch shape, slab split and timing cannot change a record.
constexpr int RESIDUAL_REC = 4;

// doubles of `partial` the two kernels need for this grid
size_t residual_partial_doubles(const GridDesc& g);

// out[(z - 1) * RESIDUAL_REC + k] for the local planes z = 1 .. g.D; reads planes 0 .. g.D + 1 of x (on a z-slab the
// halo planes must be current), x0 and the flag bytes at the cells themselves.  Two launches, nothing else is written.
template <class T>
void launch_residual(hipStream_t st, const GridDesc& g, int b, const T* x, const T* x0, const uint8_t* flags, double a, double c,
                     double* partial, double* out);

}  // namespace fs
