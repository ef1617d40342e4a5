// forces.hip -- per-plane pressure-force records over the obstacles' blocked faces (forces.h).
#include "forces.h"
#include "kernels_dev.h"

#include <algorithm>

namespace fs {

namespace {

constexpr int FT = 512;           // threads per plane; the summation order is defined for this size, do not tune it
constexpr int U = 4;              // groups of cells a lane has in flight (independent loads per loop iteration)
constexpr int ROWCHUNK = 8192;    // rows per pass of the LDS row bitmask (frontal rows)

// Lane t of the plane's workgroup takes the groups of four x-consecutive cells i = t, t + FT, t + 2 FT, ... of each
// chunk of `rc` rows, group i = (row i / G, cells 1 + 4 (i % G) .. 4 + 4 (i % G)), G = ceil(W / 4): one 4-byte load of
// flag bytes and, where one of the four cells has a blocked face, one 16-byte (fp32) / 32-byte (fp64) load of p -- the
// first interior cell of a row is 16-byte aligned (kernels.h).  U groups are loaded before any is used.  Each lane adds
// p(c) * e_k cell by cell in group order in fp64, then the 64 lanes of a wave combine by a butterfly of shuffles and
// thread 0 adds the wave sums in wave order.  rc depends on W only (items of a chunk fit 32 bits).
template <class T>
__global__ __launch_bounds__(FT) void forces_kernel(GridDesc g, SlabCtx sc, const T* __restrict__ p,
                                                    const uint8_t* __restrict__ flags, double* __restrict__ out, int rc)
{
    __shared__ unsigned rowbits[ROWCHUNK / 32];
    __shared__ double wsum[FT / 64][3];
    __shared__ int wcnt[FT / 64];
    const int t = threadIdx.x;
    const int z = 1 + blockIdx.x;
    const int zg = z + sc.zoff;
    const bool rzp = zg + 1 <= sc.Dglobal, rzm = zg - 1 >= 1;
    const unsigned G = (unsigned)(g.W + 3) >> 2;
    double sx = 0.0, sy = 0.0, sz = 0.0;
    int faces = 0, frontal = 0;
    for (int y0 = 1; y0 <= g.H; y0 += rc) {
        const int nrow = min(rc, g.H - y0 + 1);
        for (int i = t; i < ROWCHUNK / 32; i += FT) rowbits[i] = 0u;
        __syncthreads();
        const unsigned items = (unsigned)nrow * G;
        for (unsigned base = t; base < items; base += FT * U) {
            unsigned f4[U], blk[U];
            long c[U];
            int ry[U], x0[U];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const unsigned i = base + (unsigned)(u * FT);
                f4[u] = 0u;
                ry[u] = -1;
                x0[u] = 0;
                c[u] = 0;
                if (i < items) {
                    const unsigned r = i / G;
                    ry[u] = (int)r;
                    x0[u] = 1 + 4 * (int)(i - r * G);
                    c[u] = cell(g, x0[u], y0 + (int)r, z);
                    f4[u] = *reinterpret_cast<const unsigned*>(flags + c[u]);
                }
            }
            // blocked faces, 6 bits per cell (+x -x +y -y +z -z), and the row's solid bit
#pragma unroll
            for (int u = 0; u < U; ++u) {
                blk[u] = 0u;
                if (ry[u] < 0) continue;
                const int y = y0 + ry[u];
                bool solid = false;
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const int x = x0[u] + j;
                    const unsigned f = (f4[u] >> (8 * j)) & 0xffu;
                    if (x > g.W) continue;
                    if (f & F_SOLID) { solid = true; continue; }
                    const unsigned b = (unsigned)(x + 1 <= g.W && !(f & F_XP)) | (unsigned)(x - 1 >= 1 && !(f & F_XM)) << 1 |
                                       (unsigned)(y + 1 <= g.H && !(f & F_YP)) << 2 | (unsigned)(y - 1 >= 1 && !(f & F_YM)) << 3 |
                                       (unsigned)(rzp && !(f & F_ZP)) << 4 | (unsigned)(rzm && !(f & F_ZM)) << 5;
                    blk[u] |= b << (6 * j);
                }
                if (solid) atomicOr(&rowbits[ry[u] >> 5], 1u << (ry[u] & 31));
                faces += __popc(blk[u]);
            }
            V4<T> pv[U];
#pragma unroll
            for (int u = 0; u < U; ++u)
                if (blk[u]) pv[u] = *reinterpret_cast<const V4<T>*>(p + c[u]);
#pragma unroll
            for (int u = 0; u < U; ++u) {
                if (!blk[u]) continue;
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const unsigned b = (blk[u] >> (6 * j)) & 63u;
                    if (!b) continue;
                    const double pc = (double)pv[u].e[j];
                    if ((b & 3u) == 1u) sx += pc; else if ((b & 3u) == 2u) sx -= pc;
                    if ((b & 12u) == 4u) sy += pc; else if ((b & 12u) == 8u) sy -= pc;
                    if ((b & 48u) == 16u) sz += pc; else if ((b & 48u) == 32u) sz -= pc;
                }
            }
        }
        __syncthreads();
        for (int i = t; i < (nrow + 31) / 32; i += FT) frontal += __popc(rowbits[i]);
        __syncthreads();
    }
    double v[3] = { sx, sy, sz };
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
#pragma unroll
        for (int k = 0; k < 3; ++k) v[k] += __shfl_xor(v[k], m, 64);
        faces += __shfl_xor(faces, m, 64);
        frontal += __shfl_xor(frontal, m, 64);
    }
    const int w = t >> 6;
    if ((t & 63) == 0) {
        wsum[w][0] = v[0];
        wsum[w][1] = v[1];
        wsum[w][2] = v[2];
        wcnt[w] = faces;
        rowbits[w] = (unsigned)frontal;   // free again after the last chunk's barrier
    }
    __syncthreads();
    if (t == 0) {
        double s[3] = { wsum[0][0], wsum[0][1], wsum[0][2] };
        long nf = wcnt[0], nr = (long)rowbits[0];
        for (int k = 1; k < FT / 64; ++k) {
            s[0] += wsum[k][0];
            s[1] += wsum[k][1];
            s[2] += wsum[k][2];
            nf += wcnt[k];
            nr += (long)rowbits[k];
        }
        double* o = out + (long)(z - 1) * FORCE_REC;
        o[0] = s[0];
        o[1] = s[1];
        o[2] = s[2];
        o[3] = (double)nf;
        o[4] = (double)nr;
    }
}

}  // namespace

template <class T>
void launch_forces(hipStream_t st, const GridDesc& g, const SlabCtx& sc, const T* p, const uint8_t* flags, double* out)
{
    const long G = (g.W + 3) / 4;
    const int rc = (int)std::max(1L, std::min((long)ROWCHUNK, (1L << 31) / G));   // a chunk's groups fit 32 bits
    hipLaunchKernelGGL((forces_kernel<T>), dim3(g.D), dim3(FT), 0, st, g, sc, p, flags, out, rc);
}
template void launch_forces<float>(hipStream_t, const GridDesc&, const SlabCtx&, const float*, const uint8_t*, double*);
template void launch_forces<double>(hipStream_t, const GridDesc&, const SlabCtx&, const double*, const uint8_t*, double*);

}  // namespace fs
