// volume.hip -- direct volume rendering: the ray-march kernel, one thread per ray.  The arithmetic is volume.h's; this file
// only maps rays to lanes and moves the data.
//
// A latency-bound gather like the sampler's (sample.hip), but with a dependent chain per ray: every sample needs the nearest
// cell's obs value and the eight corners of the source (nine independent loads, issued together), and the next sample's
// addresses do not depend on them, only whether the march goes on.  What pays is (a) many waves in flight -- no LDS, a
// register budget that keeps 8 waves per SIMD -- and (b) neighbouring rays that gather from the same cache lines: a wave of
// 64 covers an 8 x 8 pixel tile (lane l is pixel (l / 8, l % 8) of it), not a 64 x 1 strip, so that its rays stay within a
// few rows and planes of each other along the whole march, and a workgroup of four waves covers 16 x 16 pixels.  Rays that
// end early (a miss, an obstacle, T < t_min) leave their lanes idle until the tile's longest ray is done; the square tile
// keeps those lengths close.  Ragged image edges are guarded.  Read-only on the fields; plain vector stores of three bytes and
// four doubles per pixel; no atomics, no inline assembly.
// The tile shape is a starting point, not a measured optimum ("volume rendering").
#include "volume.h"
#include <hip/hip_runtime.h>

namespace fs {

namespace {

constexpr int VOL_TILE = 8;             // a wave's tile: 8 x 8 pixels
constexpr int VOL_BLOCK = 16;           // a workgroup's: 16 x 16 pixels, four waves
constexpr int VOL_THREADS = VOL_BLOCK * VOL_BLOCK;

template <class E, class O>
__global__ __launch_bounds__(VOL_THREADS) void volume_kernel(VolumeView vw, int cols, int rows, const double* __restrict__ rays,
                                                             const E* __restrict__ src, const O* __restrict__ obs,
                                                             const uint8_t* __restrict__ table, uint8_t* __restrict__ rgb,
                                                             double* __restrict__ acc)
{
    const int t = threadIdx.x, wave = t >> 6, lane = t & 63;
    const int c = blockIdx.x * VOL_BLOCK + (wave & 1) * VOL_TILE + (lane & (VOL_TILE - 1));
    const int r = blockIdx.y * VOL_BLOCK + (wave >> 1) * VOL_TILE + (lane >> 3);
    if (c >= cols || r >= rows) return;
    const long k = (long)r * cols + c;
    double ray[6];
#pragma unroll
    for (int a = 0; a < 6; ++a) ray[a] = rays[6 * k + a];
    double out[4];
    uint8_t b[3];
    volume_ray<E, O>(ray, src, obs, vw, table, out, b);
    if (rgb) {
        rgb[3 * k] = b[0];
        rgb[3 * k + 1] = b[1];
        rgb[3 * k + 2] = b[2];
    }
    if (acc) {
#pragma unroll
        for (int a = 0; a < 4; ++a) acc[4 * k + a] = out[a];
    }
}

}  // namespace

template <class E, class O>
void launch_volume(hipStream_t st, const GridDesc& g, VolumeView vw, int cols, int rows, const double* rays, const E* src,
                   const O* obs, const uint8_t* table, uint8_t* rgb, double* acc)
{
    if (cols <= 0 || rows <= 0) return;
    vw.W = g.W; vw.H = g.H; vw.D = g.D;
    vw.py = g.sy; vw.pz = g.sz;
    const dim3 grid((unsigned)((cols + VOL_BLOCK - 1) / VOL_BLOCK), (unsigned)((rows + VOL_BLOCK - 1) / VOL_BLOCK));
    hipLaunchKernelGGL((volume_kernel<E, O>), grid, dim3(VOL_THREADS), 0, st, vw, cols, rows, rays, src, obs, table, rgb, acc);
}
template void launch_volume<float, float>(hipStream_t, const GridDesc&, VolumeView, int, int, const double*, const float*,
                                          const float*, const uint8_t*, uint8_t*, double*);
template void launch_volume<double, float>(hipStream_t, const GridDesc&, VolumeView, int, int, const double*, const double*,
                                           const float*, const uint8_t*, uint8_t*, double*);
template void launch_volume<double, double>(hipStream_t, const GridDesc&, VolumeView, int, int, const double*, const double*,
                                            const double*, const uint8_t*, uint8_t*, double*);

}  // namespace fs
