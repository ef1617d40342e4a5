// sample.h -- point probes and field sampling (include/fluidsim.h, "point probes and field sampling"): the per-point
// arithmetic of the sampler and probe kernels in sample.hip, and their launchers.  The arithmetic is plain C++ without HIP
// (inline functions, usable on the host and in the kernels), templated on the element type of the source, so that
// tests/test_sample_cpu.py compiles exactly what the kernels run.  Beyond the reference: it evaluates its fields nowhere but
// in advect's back-trace (simulation.cpp:412-420), whose lerp form FS_SAMPLE_LINEAR keeps.  Internal to libfluidsim.so.
#pragma once

#if defined(__HIPCC__)
#define FS_SAMPLE_HD __host__ __device__
#else
#define FS_SAMPLE_HD
#endif

namespace fs {

// mode order of FS_SAMPLE_*
enum { SAMPLE_NEAREST = 0, SAMPLE_LINEAR = 1, SAMPLE_FLUID = 2, SAMPLE_NMODES = 3 };
constexpr int PROBE_VALUES = 5;         // FS_PROBE_VALUES: q, u, v, w, p

// One coordinate x of a point against an axis of N interior cells (the box is [0, N + 1]): the lower corner i0 =
// min(floor(x), N) and the offset s = x - i0 (exact: both are below 2^31 and x - i0 lies in [0, 1]).  Returns false, with
// the corner of cell 0 so that a caller can still load, when x is NaN, below 0 or above N + 1.
FS_SAMPLE_HD inline bool sample_axis(double x, int N, int& i0, double& s)
{
    if (!(x >= 0.0 && x <= (double)(N + 1))) {
        i0 = 0;
        s = 0.0;
        return false;
    }
    const int i = (int)__builtin_floor(x);
    i0 = i < N ? i : N;
    s = x - (double)i0;
    return true;
}

// The corner values of a point: v[a + 2 * b + 4 * c] is the stored value at (i0 + a, j0 + b, l0 + c), memory order.
// Every operation below is rounded once, in the order written (the library and the test driver are built without
// contraction).

// the nearest corner's stored value, ties towards the upper corner
template <class E>
FS_SAMPLE_HD inline double sample_nearest(const E* v, double sx, double sy, double sz)
{
    const int a = sx >= 0.5 ? 1 : 0, b = sy >= 0.5 ? 1 : 0, c = sz >= 0.5 ? 1 : 0;
    return (double)v[a + 2 * b + 4 * c];
}

// the reference's lerp form (simulation.cpp:412-420): x, then y, then z.  Every corner is multiplied, so that a NaN or
// infinite corner gives NaN even where its weight is 0.
template <class E>
FS_SAMPLE_HD inline double sample_linear(const E* v, double sx, double sy, double sz)
{
    const double tx = 1.0 - sx, ty = 1.0 - sy, tz = 1.0 - sz;
    double c[4];
    for (int k = 0; k < 4; ++k) {
        const double lo = (double)v[2 * k] * tx, hi = (double)v[2 * k + 1] * sx;
        c[k] = lo + hi;
    }
    double d[2];
    for (int k = 0; k < 2; ++k) {
        const double lo = c[2 * k] * ty, hi = c[2 * k + 1] * sy;
        d[k] = lo + hi;
    }
    const double lo = d[0] * tz, hi = d[1] * sz;
    return lo + hi;
}

// The weighted mean over the corners that carry weight and are not solid (o = the corners' obs values, same order): the
// value for points on an obstacle's surface, where half of the trilinear weight sits in solid cells that hold 0.
template <class E, class O>
FS_SAMPLE_HD inline double sample_fluid(const E* v, const O* o, double sx, double sy, double sz)
{
    const double tx = 1.0 - sx, ty = 1.0 - sy, tz = 1.0 - sz;
    double num = 0.0, den = 0.0;
    bool any = false;
    for (int k = 0; k < 8; ++k) {                         // memory order: c outer, b, a inner
        const double wxy = ((k & 1) ? sx : tx) * ((k & 2) ? sy : ty);
        const double w = wxy * ((k & 4) ? sz : tz);
        if (w > 0.0 && !((double)o[k] == 1.0)) {
            const double wv = w * (double)v[k];
            num = num + wv;
            den = den + w;
            any = true;
        }
    }
    return any ? num / den : __builtin_nan("");
}

template <int MODE, class E, class O>
FS_SAMPLE_HD inline double sample_value(bool inside, const E* v, const O* o, double sx, double sy, double sz)
{
    if (!inside) return __builtin_nan("");
    return MODE == SAMPLE_NEAREST ? sample_nearest(v, sx, sy, sz)
         : MODE == SAMPLE_LINEAR  ? sample_linear(v, sx, sy, sz)
                                  : sample_fluid(v, o, sx, sy, sz);
}

}  // namespace fs

#if defined(__HIPCC__)
#include "kernels.h"

namespace fs {

// The sampler: out[k] = the value of `src` at point (pts[3 k], pts[3 k + 1], pts[3 k + 2]), k < n.  `src` and `obs` are
// LEAD-shifted arrays of the fields' pitched layout (E / O: their element types); obs is read in mode SAMPLE_FLUID only.
// pts and out are device arrays.
template <class E, class O>
void launch_sample(hipStream_t st, const GridDesc& g, int mode, long n, const double* pts, const E* src, const O* obs,
                   double* out);

// One probe record: rec[5 k + ..] = {q, u, v, w, p}[idx[k]] widened, k < n; idx[k] < 0 (a cell of another slab): +0.0.
template <class T>
void launch_probe_record(hipStream_t st, int n, const long* idx, const T* q, const T* u, const T* v, const T* w, const T* p,
                         double* rec);

}  // namespace fs
#endif
