// sample.hip -- point probes and field sampling: the sampler kernel (one thread per point) and the probe kernel (one
// thread per probe).  The arithmetic is sample.h's; this file only moves the data.
//
// Both are latency-bound gathers, not bandwidth problems: a point reads 8 (mode FLUID: 16) scattered values out of four
// rows of two planes and writes 8 bytes, so what a launch costs is the depth of its dependent-load chain (the point, then
// the corners), not bytes.  All corner loads of a thread are therefore issued before any arithmetic, and a wave's
// neighbouring points (a rake, a cut plane) share their rows' cache lines.  No LDS, no atomics, no scratch.
// -Rpass-analysis (gfx950), VGPRs of sample_kernel for fp32 / fp64 sources: NEAREST 24 / 28, LINEAR 30 / 30, FLUID 39 / 52
// (46 for an fp64 statistics field over fp32 obs); probe_kernel 14; scratch 0 and 8 waves per SIMD for every one of them.
#include "sample.h"
#include <hip/hip_runtime.h>

namespace fs {

namespace {

constexpr int SM_THREADS = 256;

template <class E, class O, int MODE>
__global__ __launch_bounds__(SM_THREADS) void sample_kernel(long n, const double* __restrict__ pts, const E* __restrict__ src,
                                                            const O* __restrict__ obs, int W, int H, int D, long py, long pz,
                                                            double* __restrict__ out)
{
    const long k = (long)blockIdx.x * SM_THREADS + threadIdx.x;
    if (k >= n) return;
    const double x = pts[3 * k], y = pts[3 * k + 1], z = pts[3 * k + 2];
    int i0, j0, l0;
    double sx, sy, sz;
    const bool okx = sample_axis(x, W, i0, sx), oky = sample_axis(y, H, j0, sy), okz = sample_axis(z, D, l0, sz);
    const bool inside = okx && oky && okz;
    // a point outside the box loads the corners of cell (0, 0, 0) of its bad axes: always inside the arrays
    const long base = (long)i0 + (long)j0 * py + (long)l0 * pz;
    E v[8];
    O o[8];
#pragma unroll
    for (int c = 0; c < 8; ++c) v[c] = src[base + (c & 1) + ((c >> 1) & 1) * py + (c >> 2) * pz];
    if (MODE == SAMPLE_FLUID) {
#pragma unroll
        for (int c = 0; c < 8; ++c) o[c] = obs[base + (c & 1) + ((c >> 1) & 1) * py + (c >> 2) * pz];
    }
    out[k] = sample_value<MODE, E, O>(inside, v, o, sx, sy, sz);
}

template <class T>
__global__ __launch_bounds__(SM_THREADS) void probe_kernel(int n, const long* __restrict__ idx, const T* __restrict__ q,
                                                           const T* __restrict__ u, const T* __restrict__ v,
                                                           const T* __restrict__ w, const T* __restrict__ p,
                                                           double* __restrict__ rec)
{
    const int k = blockIdx.x * SM_THREADS + threadIdx.x;
    if (k >= n) return;
    const long c = idx[k];
    double r[PROBE_VALUES] = {0.0, 0.0, 0.0, 0.0, 0.0};
    if (c >= 0) {
        const T fq = q[c], fu = u[c], fv = v[c], fw = w[c], fp = p[c];
        r[0] = (double)fq; r[1] = (double)fu; r[2] = (double)fv; r[3] = (double)fw; r[4] = (double)fp;
    }
#pragma unroll
    for (int j = 0; j < PROBE_VALUES; ++j) rec[(long)PROBE_VALUES * k + j] = r[j];
}

}  // namespace

template <class E, class O>
void launch_sample(hipStream_t st, const GridDesc& g, int mode, long n, const double* pts, const E* src, const O* obs,
                   double* out)
{
    if (n <= 0) return;
    const dim3 grid((unsigned)((n + SM_THREADS - 1) / SM_THREADS)), block(SM_THREADS);
#define FS_SM_LAUNCH(MODE) \
    hipLaunchKernelGGL((sample_kernel<E, O, MODE>), grid, block, 0, st, n, pts, src, obs, g.W, g.H, g.D, g.sy, g.sz, out)
    if (mode == SAMPLE_NEAREST) FS_SM_LAUNCH(SAMPLE_NEAREST);
    else if (mode == SAMPLE_LINEAR) FS_SM_LAUNCH(SAMPLE_LINEAR);
    else FS_SM_LAUNCH(SAMPLE_FLUID);
#undef FS_SM_LAUNCH
}
template void launch_sample<float, float>(hipStream_t, const GridDesc&, int, long, const double*, const float*, const float*, double*);
template void launch_sample<double, float>(hipStream_t, const GridDesc&, int, long, const double*, const double*, const float*, double*);
template void launch_sample<double, double>(hipStream_t, const GridDesc&, int, long, const double*, const double*, const double*, double*);

template <class T>
void launch_probe_record(hipStream_t st, int n, const long* idx, const T* q, const T* u, const T* v, const T* w, const T* p,
                         double* rec)
{
    if (n <= 0) return;
    const dim3 grid((unsigned)((n + SM_THREADS - 1) / SM_THREADS)), block(SM_THREADS);
    hipLaunchKernelGGL((probe_kernel<T>), grid, block, 0, st, n, idx, q, u, v, w, p, rec);
}
template void launch_probe_record<float>(hipStream_t, int, const long*, const float*, const float*, const float*, const float*,
                                         const float*, double*);
template void launch_probe_record<double>(hipStream_t, int, const long*, const double*, const double*, const double*,
                                          const double*, const double*, double*);

}  // namespace fs
