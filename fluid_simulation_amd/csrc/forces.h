// forces.h -- pressure force of the stream on the obstacles (fs_obstacle_force, option "force_log").
// Internal to libfluidsim.so.  Beyond the reference: it has no force output (include/fluidsim.h).
#pragma once
#include "kernels.h"

namespace fs {

// A face is BLOCKED where the projection's gradient (simulation.cpp:328-356) takes its one-sided form across it:
// between a cell c with obs(c) != 1 and a 6-neighbour n inside the interior range with obs(n) != 0 -- in flag bytes,
// c is not F_SOLID, n is in range, and the matching F_XP..F_ZM bit of c is clear.  Per z-plane the kernel writes
//     { Sx, Sy, Sz, blocked faces, frontal rows }   (fp64)
// S = sum over the plane's blocked faces of p(c) * e, e the unit vector from c toward n; frontal rows = rows (y, z)
// of the plane that hold an F_SOLID cell.  A plane's record is a pure function of that plane's p and flag bytes:
// one workgroup of a fixed size per plane, a fixed assignment of the plane's cells to its lanes and a fixed
// shuffle / LDS tree, no atomics on floating-point values -- launch shape, slab split and timing cannot change it.
constexpr int FORCE_REC = 5;

// out[(z - 1) * FORCE_REC + k] for the local planes z = 1 .. g.D
template <class T>
void launch_forces(hipStream_t st, const GridDesc& g, const SlabCtx& sc, const T* p, const uint8_t* flags, double* out);

}  // namespace fs
