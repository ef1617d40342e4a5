// tracers.h -- tracer particles (include/fluidsim.h, "tracer particles"): the per-particle arithmetic of the move kernel in
// tracers.hip, and its launcher.  The arithmetic is plain C++ without HIP (inline functions, usable on the host and in the
// kernel), templated on the element type of the fields, so that tests/test_tracers_cpu.py compiles exactly what the kernel
// runs: the corner gather included, which is sample.h's (sample_axis, sample_linear) and is not restated here.  Beyond the
// reference: it follows no parcel; the displacement per step is the one its advect traces back (simulation.cpp:384-390).
// Internal to libfluidsim.so.
#pragma once

#include "sample.h"

namespace fs {

// status order of a slot (the first of its four meta words {status, source, born, moves})
enum { TRACER_FREE = 0, TRACER_ALIVE = 1, TRACER_OUT = 2, TRACER_HIT = 3 };
constexpr int TRACER_META = 4;
constexpr int TRACER_FRAME_BYTES = 28;  // per slot and snapshot frame: three fp64 coordinates and the status word

// THE BOX B: 0.5 <= c <= N + 0.5 on each axis, the range advect clamps its back-traces to.  NaN is outside.
FS_SAMPLE_HD inline bool tracer_in_box(const double* P, int W, int H, int D)
{
    return P[0] >= 0.5 && P[0] <= (double)W + 0.5 && P[1] >= 0.5 && P[1] <= (double)H + 0.5 && P[2] >= 0.5 &&
           P[2] <= (double)D + 0.5;
}

// vel = (LIN(u, P), LIN(v, P), LIN(w, P)): FS_SAMPLE_LINEAR of the three fields at one point.  u, v, w are arrays indexed
// x + y * py + z * pz.  All 24 corner loads are issued before any arithmetic; a point outside [0, N + 1] loads the corners
// of cell 0 of its bad axes (always inside the arrays) and gives NaN, as the sampler does.
template <class E>
FS_SAMPLE_HD inline void tracer_velocity(const E* u, const E* v, const E* w, int W, int H, int D, long py, long pz,
                                         const double* P, double* vel)
{
    int i0, j0, l0;
    double sx, sy, sz;
    const bool okx = sample_axis(P[0], W, i0, sx), oky = sample_axis(P[1], H, j0, sy), okz = sample_axis(P[2], D, l0, sz);
    const bool inside = okx && oky && okz;
    const long base = (long)i0 + (long)j0 * py + (long)l0 * pz;
    E cu[8], cv[8], cw[8];
    for (int c = 0; c < 8; ++c) {
        const long at = base + (c & 1) + ((c >> 1) & 1) * py + (c >> 2) * pz;
        cu[c] = u[at];
        cv[c] = v[at];
        cw[c] = w[at];
    }
    vel[0] = sample_value<SAMPLE_LINEAR, E, E>(inside, cu, cu, sx, sy, sz);
    vel[1] = sample_value<SAMPLE_LINEAR, E, E>(inside, cv, cv, sx, sy, sz);
    vel[2] = sample_value<SAMPLE_LINEAR, E, E>(inside, cw, cw, sx, sy, sz);
}

// The move of an ALIVE particle at P (explicit midpoint rule on the frozen velocity field): P becomes P', the new status is
// returned.  k = ((double)dt * W, (double)dt * H, (double)dt * D).  Every operation is rounded once, in the order written
// (the library and the test driver are built without contraction).
template <class E>
FS_SAMPLE_HD inline int tracer_move(const E* u, const E* v, const E* w, const E* obs, int W, int H, int D, long py, long pz,
                                    const double* k, double* P)
{
    double u1[3], M[3], Q[3];
    tracer_velocity(u, v, w, W, H, D, py, pz, P, u1);
    for (int a = 0; a < 3; ++a) {
        const double h = 0.5 * k[a];                     // exact
        const double d = h * u1[a];
        M[a] = P[a] + d;
    }
    if (tracer_in_box(M, W, H, D)) {
        double u2[3];
        tracer_velocity(u, v, w, W, H, D, py, pz, M, u2);
        for (int a = 0; a < 3; ++a) {
            const double d = k[a] * u2[a];
            Q[a] = P[a] + d;
        }
    } else {
        for (int a = 0; a < 3; ++a) Q[a] = M[a];
    }
    for (int a = 0; a < 3; ++a) P[a] = Q[a];
    if (!tracer_in_box(Q, W, H, D)) return TRACER_OUT;
    // the cell of P': 1 .. N + 1 on each axis, inside the arrays
    const long cell = (long)__builtin_floor(Q[0] + 0.5) + (long)__builtin_floor(Q[1] + 0.5) * py +
                      (long)__builtin_floor(Q[2] + 0.5) * pz;
    return (double)obs[cell] == 1.0 ? TRACER_HIT : TRACER_ALIVE;
}

// The slot a release of n particles starting at slot `first` of a pool of C leaves in slot s: the last e < n with
// (first + e) % C == s, or -1 (n may exceed C: the later particles overwrite the earlier ones).
FS_SAMPLE_HD inline int tracer_released(int s, int first, int n, int C)
{
    int d = s - first;
    if (d < 0) d += C;
    if (d >= n) return -1;
    return d + ((n - 1 - d) / C) * C;
}

}  // namespace fs

#if defined(__HIPCC__)

namespace fs {

// One advance of the pool: what the kernel needs besides the fields.
struct TracerPass {
    int C;                      // slots
    double* xyz;                // 3 C
    int* meta;                  // 4 C
    double k[3];
    const double* emit;         // the emitters' points; released into slots (first + e) % C with source e, born `born`
    int n_emit, first, born;    // n_emit = 0: no release in this advance
    double* frame_xyz;          // the snapshot frame to fill (3 C, C), nullptr = none is due
    int* frame_status;
};

// 1. every ALIVE particle moves, 2. the release, 3. the snapshot: one launch, one thread per slot.  u, v, w, obs are
// LEAD-shifted arrays of the fields' pitched layout.
template <class E>
void launch_tracer_advance(hipStream_t st, const GridDesc& g, const TracerPass& pass, const E* u, const E* v, const E* w,
                           const E* obs);

}  // namespace fs
#endif
