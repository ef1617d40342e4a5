// residual.hip -- per-plane residual records of a linearSolver system (residual.h).  Reads only; writes only its own
// record buffers.
#include "residual.h"
#include "kernels_dev.h"

namespace fs {

namespace {

constexpr int NW = RES_FT / 64;

// Workgroup (chunk, plane) takes the groups of four x-consecutive cells that residual_plan.h deals to its lanes: per
// group five 16-byte (fp32) / 32-byte (fp64) loads of x (the cells, their y and their z neighbours), two single
// elements of x (the x neighbours of the group's ends), one such load of x0 and one 4-byte load of flag bytes -- the
// first interior cell of a row is 16-byte aligned (kernels.h).  RES_U groups are loaded before any is used.  Each lane
// adds r^2 and x0^2 cell by cell in group order in fp64, the 64 lanes of a wave combine by a butterfly of shuffles and
// thread 0 adds the wave sums in wave order.
template <class T>
__global__ __launch_bounds__(RES_FT) void residual_kernel(GridDesc g, const T* __restrict__ x, const T* __restrict__ x0,
                                                          const uint8_t* __restrict__ flags, unsigned zero_bits, double a, double c,
                                                          double* __restrict__ partial)
{
    __shared__ double wsum[NW][3];
    __shared__ int wcnt[NW];
    const ResidualPlan p = residual_plan(g.W, g.H);
    const int t = threadIdx.x;
    const int chunk = (int)(blockIdx.x % (unsigned)p.nchunk);
    const int z = 1 + (int)(blockIdx.x / (unsigned)p.nchunk);
    const long oym = residual_load(RL_YM, g.sy, g.sz).off, oyp = residual_load(RL_YP, g.sy, g.sz).off;
    const long ozm = residual_load(RL_ZM, g.sy, g.sz).off, ozp = residual_load(RL_ZP, g.sy, g.sz).off;
    const long oxm = residual_load(RL_XM, g.sy, g.sz).off, oxp = residual_load(RL_XP, g.sy, g.sz).off;
    double sr = 0.0, sb = 0.0, mr = 0.0;
    int cells = 0;
    const int iters = residual_iters(p, chunk);
    for (int it = 0; it < iters; ++it) {
        V4<T> qc[RES_U], qym[RES_U], qyp[RES_U], qzm[RES_U], qzp[RES_U], rh[RES_U];
        T qxm[RES_U], qxp[RES_U];
        unsigned f4[RES_U];
        int xf[RES_U];
#pragma unroll
        for (int u = 0; u < RES_U; ++u) {
            const ResidualItem i = residual_item(p, chunk, t, it, u);
            xf[u] = 0;
            if (i.valid) {
                xf[u] = i.x0;
                const long k = cell(g, i.x0, i.y, z);
                f4[u] = *reinterpret_cast<const unsigned*>(flags + k);
                qc[u] = *reinterpret_cast<const V4<T>*>(x + k);
                qym[u] = *reinterpret_cast<const V4<T>*>(x + k + oym);
                qyp[u] = *reinterpret_cast<const V4<T>*>(x + k + oyp);
                qzm[u] = *reinterpret_cast<const V4<T>*>(x + k + ozm);
                qzp[u] = *reinterpret_cast<const V4<T>*>(x + k + ozp);
                qxm[u] = x[k + oxm];
                qxp[u] = x[k + oxp];
                rh[u] = *reinterpret_cast<const V4<T>*>(x0 + k);
            }
        }
#pragma unroll
        for (int u = 0; u < RES_U; ++u) {
            if (!xf[u]) continue;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const unsigned f = (f4[u] >> (8 * j)) & 0xffu;
                if (xf[u] + j > g.W || (f & zero_bits)) continue;
                const double xp = (double)(j < 3 ? qc[u].e[(j + 1) & 3] : qxp[u]);
                const double xm = (double)(j > 0 ? qc[u].e[(j + 3) & 3] : qxm[u]);
                const double rhs = (double)rh[u].e[j];
                const double nb = ((((xp + xm) + (double)qyp[u].e[j]) + (double)qym[u].e[j]) + (double)qzp[u].e[j]) + (double)qzm[u].e[j];
                const double r = (rhs + a * nb) - c * (double)qc[u].e[j];
                sr += r * r;
                sb += rhs * rhs;
                mr = fmax(mr, fabs(r));
                ++cells;
            }
        }
    }
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
        sr += __shfl_xor(sr, m, 64);
        sb += __shfl_xor(sb, m, 64);
        mr = fmax(mr, __shfl_xor(mr, m, 64));
        cells += __shfl_xor(cells, m, 64);
    }
    const int w = t >> 6;
    if ((t & 63) == 0) {
        wsum[w][0] = sr;
        wsum[w][1] = sb;
        wsum[w][2] = mr;
        wcnt[w] = cells;
    }
    __syncthreads();
    if (t == 0) {
        double s0 = wsum[0][0], s1 = wsum[0][1], s2 = wsum[0][2];
        int n = wcnt[0];
        for (int k = 1; k < NW; ++k) {
            s0 += wsum[k][0];
            s1 += wsum[k][1];
            s2 = fmax(s2, wsum[k][2]);
            n += wcnt[k];
        }
        double* o = partial + ((long)(z - 1) * p.nchunk + chunk) * RESIDUAL_REC;
        o[0] = s0;
        o[1] = s1;
        o[2] = s2;
        o[3] = (double)n;
    }
}

// one thread per plane: its partial records in chunk order
__global__ void residual_combine_kernel(int D, int nchunk, const double* __restrict__ partial, double* __restrict__ out)
{
    const int zi = blockIdx.x * blockDim.x + threadIdx.x;
    if (zi >= D) return;
    const double* q = partial + (long)zi * nchunk * RESIDUAL_REC;
    double s0 = q[0], s1 = q[1], s2 = q[2], s3 = q[3];
    for (int k = 1; k < nchunk; ++k) {
        q += RESIDUAL_REC;
        s0 += q[0];
        s1 += q[1];
        s2 = fmax(s2, q[2]);
        s3 += q[3];
    }
    double* o = out + (long)zi * RESIDUAL_REC;
    o[0] = s0;
    o[1] = s1;
    o[2] = s2;
    o[3] = s3;
}

}  // namespace

size_t residual_partial_doubles(const GridDesc& g)
{
    return (size_t)residual_plan(g.W, g.H).nchunk * (size_t)g.D * RESIDUAL_REC;
}

template <class T>
void launch_residual(hipStream_t st, const GridDesc& g, int b, const T* x, const T* x0, const uint8_t* flags, double a, double c,
                     double* partial, double* out)
{
    const ResidualPlan p = residual_plan(g.W, g.H);
    const unsigned zero_bits = (b == 0) ? F_SOLID : (F_SOLID | F_NEAR);
    hipLaunchKernelGGL((residual_kernel<T>), dim3((unsigned)p.nchunk * (unsigned)g.D), dim3(RES_FT), 0, st, g, x, x0, flags, zero_bits, a, c, partial);
    hipLaunchKernelGGL(residual_combine_kernel, dim3((g.D + 63) / 64), dim3(64), 0, st, g.D, p.nchunk, partial, out);
}
template void launch_residual<float>(hipStream_t, const GridDesc&, int, const float*, const float*, const uint8_t*, double, double,
                                     double*, double*);
template void launch_residual<double>(hipStream_t, const GridDesc&, int, const double*, const double*, const uint8_t*, double, double,
                                      double*, double*);

}  // namespace fs
