// tracers.hip -- tracer particles: the move kernel, one thread per slot of the pool.  The arithmetic is tracers.h's; this
// file only moves the data.
//
// A latency-bound gather like the sampler: a move is two dependent stages of 24 scattered loads (eight corners of three
// fields, all issued before the stage's arithmetic) plus one obs load, so what a launch costs is the depth of that chain and
// the cache lines a wave touches, not bytes.  A slot that is FREE or dead costs one 4-byte load (and, when a snapshot frame is
// due, its copy into the frame); the release of the emitters and the snapshot are slot ranges / stores of the same launch, so
// the pool is passed over once per advance.  No LDS, no atomics, no reductions, no scratch.
// -Rpass-analysis (gfx950), tracer_kernel for fp32 / fp64 fields: 74 / 74 VGPRs, scratch 0, 6 waves per SIMD.
#include "tracers.h"
#include <hip/hip_runtime.h>

namespace fs {

namespace {

constexpr int TR_THREADS = 256;

template <class E>
__global__ __launch_bounds__(TR_THREADS) void tracer_kernel(TracerPass a, const E* __restrict__ u, const E* __restrict__ v,
                                                            const E* __restrict__ w, const E* __restrict__ obs, int W, int H,
                                                            int D, long py, long pz)
{
    const int s = blockIdx.x * TR_THREADS + threadIdx.x;
    if (s >= a.C) return;
    int status = a.meta[TRACER_META * s];
    const int e = a.n_emit > 0 ? tracer_released(s, a.first, a.n_emit, a.C) : -1;
    const bool frame = a.frame_xyz != nullptr;
    if (e < 0 && status != TRACER_ALIVE && !frame) return;
    double P[3];
    if (e >= 0) {                                        // released into this slot: not moved in this advance
        for (int c = 0; c < 3; ++c) P[c] = a.emit[3 * e + c];
        status = TRACER_ALIVE;
        *reinterpret_cast<int4*>(a.meta + TRACER_META * s) = make_int4(TRACER_ALIVE, e, a.born, 0);
        for (int c = 0; c < 3; ++c) a.xyz[3 * (long)s + c] = P[c];
    } else {
        for (int c = 0; c < 3; ++c) P[c] = a.xyz[3 * (long)s + c];
        if (status == TRACER_ALIVE) {
            const int moves = a.meta[TRACER_META * s + 3];
            status = tracer_move<E>(u, v, w, obs, W, H, D, py, pz, a.k, P);
            for (int c = 0; c < 3; ++c) a.xyz[3 * (long)s + c] = P[c];
            a.meta[TRACER_META * s] = status;
            a.meta[TRACER_META * s + 3] = moves + 1;
        }
    }
    if (frame) {
        for (int c = 0; c < 3; ++c) a.frame_xyz[3 * (long)s + c] = P[c];
        a.frame_status[s] = status;
    }
}

}  // namespace

template <class E>
void launch_tracer_advance(hipStream_t st, const GridDesc& g, const TracerPass& pass, const E* u, const E* v, const E* w,
                           const E* obs)
{
    if (pass.C <= 0) return;
    const dim3 grid((unsigned)((pass.C + TR_THREADS - 1) / TR_THREADS)), block(TR_THREADS);
    hipLaunchKernelGGL((tracer_kernel<E>), grid, block, 0, st, pass, u, v, w, obs, g.W, g.H, g.D, g.sy, g.sz);
}
template void launch_tracer_advance<float>(hipStream_t, const GridDesc&, const TracerPass&, const float*, const float*,
                                           const float*, const float*);
template void launch_tracer_advance<double>(hipStream_t, const GridDesc&, const TracerPass&, const double*, const double*,
                                            const double*, const double*);

}  // namespace fs
