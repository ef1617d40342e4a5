// image.hip -- slice and projection images: the slice gather, the two projection kernels (a march along z or y, and the
// LDS-transposed reduction along x), and the colour kernel.  The arithmetic is image.h's; this file only moves the data.
//
// The order along the axis is strictly sequential on all three axes (include/fluidsim.h): a pixel is a pure function of its
// column of cells.  So no kernel splits a column between lanes; parallelism comes from the pixels alone, and what is left to
// the kernels is to keep the loads wide, coalesced and many in flight.
//
// Projection along z or y (project_march_kernel): a lane owns the pixels of one aligned 16-byte group of a row (four fp32 or
// two fp64 cells adjacent in x; group m = cells VEC m - (VEC - 1) .. VEC m, the grouping of flow_stats.h) and marches the
// axis with MARCH_DEPTH independent 16-byte loads in flight, then adds them in order.  A wave reads 1 KiB runs of a row.
// Every field element is read once.  Group 0 starts VEC - 1 cells before its row: inside the allocation, because the march
// starts at cell 1 of the axis, which is at least one row past the array's first one; what it reads there is not stored.
// The last group ends at most VEC - 1 cells past x = W + 1, inside the row's pitch (sy >= W + 5).
//
// Projection along x (project_x_kernel): a lane owns one (y, z) row -- rows are contiguous, sy apart, because sz = sy (H + 2)
// -- and a wave owns 64 rows.  Per tile of TX = 16 VEC cells of x, 16 lanes load one row's segment with one 16-byte load each
// (256 contiguous bytes per row, four rows per wave instruction, 16 instructions in flight per lane), the wave stores the
// tile into LDS with a row stride of TX + 1 elements, and each lane then adds its own row's segment in increasing x: lane l
// reads element l (TX + 1) + x, which is bank (l + x) mod 32 for fp32 and the bank pair 2 (l + x) mod 64 for fp64 --
// conflict-free in both of a wave's 32-lane halves.  The stores are ds_write_b32 at (row + 4 m + e) mod 32: two-way.  Groups
// start at x = 1 (16-byte aligned) and are loaded only where their first cell is <= W, so a load ends at most at x = W + 3.
//
// -Rpass-analysis (gfx950), fp32 / fp64 sources: project_march_kernel 52 .. 56 / 44 VGPRs, 8 waves per SIMD; project_x_kernel
// 106 VGPRs and 16640 / 16896 bytes of LDS (nine one-wave workgroups per CU); slice_kernel 13, colour_kernel 16; scratch 0
// for every kernel of this file.
#include "image.h"
#include <hip/hip_runtime.h>

namespace fs {

namespace {

constexpr int IM_THREADS = 256;
constexpr int MARCH_DEPTH = 8;          // independent 16-byte loads a lane of the march keeps in flight

template <class E>
struct alignas(16) Group {
    static constexpr int N = 16 / (int)sizeof(E);
    E v[N];
};

template <class E, class O>
__global__ __launch_bounds__(IM_THREADS) void slice_kernel(const E* __restrict__ src, const O* __restrict__ obs, int cols, long npix,
                                                           long base, long col_stride, long row_stride, double* __restrict__ val,
                                                           uint8_t* __restrict__ flag)
{
    const long k = (long)blockIdx.x * IM_THREADS + threadIdx.x;
    if (k >= npix) return;
    const long r = k / cols, c = k - r * cols;
    const long at = base + c * col_stride + r * row_stride;
    val[k] = (double)src[at];
    flag[k] = image_solid(obs[at]) ? 1 : 0;
}

// rows of the image are `row_stride` elements apart in the source, the cells of a column `step` apart; G groups per row
template <class E, int KIND>
__global__ __launch_bounds__(IM_THREADS) void project_march_kernel(const E* __restrict__ src, int W, int rows, int G, int N,
                                                                   long row_stride, long step, double* __restrict__ val,
                                                                   uint8_t* __restrict__ flag)
{
    constexpr int VEC = Group<E>::N;
    const long t = (long)blockIdx.x * IM_THREADS + threadIdx.x;
    if (t >= (long)rows * G) return;
    const int r = (int)(t / G), m = (int)(t - (long)r * G);
    const int x0 = VEC * m - (VEC - 1);
    const E* p = src + (long)r * row_stride + x0;
    double a[VEC];
#pragma unroll
    for (int e = 0; e < VEC; ++e) a[e] = image_start<KIND>();
    int k = 1;
    for (; k + MARCH_DEPTH - 1 <= N; k += MARCH_DEPTH) {
        Group<E> q[MARCH_DEPTH];
#pragma unroll
        for (int j = 0; j < MARCH_DEPTH; ++j) q[j] = *reinterpret_cast<const Group<E>*>(p + (long)(k + j) * step);
#pragma unroll
        for (int j = 0; j < MARCH_DEPTH; ++j)
#pragma unroll
            for (int e = 0; e < VEC; ++e) a[e] = image_step<KIND, E>(a[e], q[j].v[e]);
    }
    for (; k <= N; ++k) {
        const Group<E> q = *reinterpret_cast<const Group<E>*>(p + (long)k * step);
#pragma unroll
        for (int e = 0; e < VEC; ++e) a[e] = image_step<KIND, E>(a[e], q.v[e]);
    }
    const long out = (long)r * (W + 2);
#pragma unroll
    for (int e = 0; e < VEC; ++e) {
        const int x = x0 + e;
        if (x >= 0 && x <= W + 1) {
            if (KIND == IMG_ANY) flag[out + x] = a[e] != 0.0 ? 1 : 0;
            else val[out + x] = a[e];
        }
    }
}

template <class E, int KIND>
__global__ __launch_bounds__(64) void project_x_kernel(const E* __restrict__ src, int W, long sy, long nrows, double* __restrict__ val,
                                                       uint8_t* __restrict__ flag)
{
    constexpr int VEC = Group<E>::N, TX = 16 * VEC, LDW = TX + 1;
    __shared__ E tile[64 * LDW];
    const int lane = threadIdx.x, sub = lane >> 4, m = lane & 15;
    const long row0 = (long)blockIdx.x * 64;
    double a = image_start<KIND>();
    for (int x0 = 1; x0 <= W; x0 += TX) {
        const int xg = x0 + VEC * m;                     // the first cell of this lane's group
        Group<E> q[16];
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const long row = row0 + 4 * i + sub;
#pragma unroll
            for (int e = 0; e < VEC; ++e) q[i].v[e] = (E)0;
            if (row < nrows && xg <= W) q[i] = *reinterpret_cast<const Group<E>*>(src + row * sy + xg);
        }
#pragma unroll
        for (int i = 0; i < 16; ++i)
#pragma unroll
            for (int e = 0; e < VEC; ++e) tile[(4 * i + sub) * LDW + VEC * m + e] = q[i].v[e];
        __syncthreads();
        const int nx = W - x0 + 1 < TX ? W - x0 + 1 : TX;
        for (int x = 0; x < nx; ++x) a = image_step<KIND, E>(a, tile[lane * LDW + x]);
        __syncthreads();
    }
    const long row = row0 + lane;
    if (row < nrows) {
        if (KIND == IMG_ANY) flag[row] = a != 0.0 ? 1 : 0;
        else val[row] = a;
    }
}

__global__ __launch_bounds__(IM_THREADS) void colour_kernel(long npix, const double* __restrict__ val, const uint8_t* __restrict__ flag,
                                                            double vmin, double vmax, double alpha, const uint8_t* __restrict__ table,
                                                            int n, uint8_t* __restrict__ rgb)
{
    const long k = (long)blockIdx.x * IM_THREADS + threadIdx.x;
    if (k >= npix) return;
    uint8_t c[3];
    image_colour(val[k], flag[k] != 0, vmin, vmax, alpha, table, n, c);
    rgb[3 * k] = c[0];
    rgb[3 * k + 1] = c[1];
    rgb[3 * k + 2] = c[2];
}

template <class E, int KIND>
void project_kind(hipStream_t st, const GridDesc& g, int axis, const E* src, double* val, uint8_t* flag)
{
    if (axis == 0) {
        const long nrows = (long)(g.H + 2) * (g.D + 2);
        hipLaunchKernelGGL((project_x_kernel<E, KIND>), dim3((unsigned)((nrows + 63) / 64)), dim3(64), 0, st, src, g.W, g.sy, nrows,
                           val, flag);
        return;
    }
    constexpr int VEC = Group<E>::N;
    const int G = (g.W + 1 + VEC - 1) / VEC + 1;         // groups 0 .. ceil((W + 1) / VEC) cover x = 0 .. W + 1
    const int rows = axis == 2 ? g.H + 2 : g.D + 2, N = axis == 2 ? g.D : g.H;
    const long row_stride = axis == 2 ? g.sy : g.sz, step = axis == 2 ? g.sz : g.sy;
    const long threads = (long)rows * G;
    hipLaunchKernelGGL((project_march_kernel<E, KIND>), dim3((unsigned)((threads + IM_THREADS - 1) / IM_THREADS)), dim3(IM_THREADS), 0,
                       st, src, g.W, rows, G, N, row_stride, step, val, flag);
}

}  // namespace

template <class E, class O>
void launch_image_slice(hipStream_t st, const GridDesc& g, int axis, int index, const E* src, const O* obs, double* val,
                        uint8_t* flag)
{
    int cols, rows;
    image_dims(axis, g.W, g.H, g.D, &cols, &rows);
    const long npix = (long)cols * rows;
    const long base = (long)index * (axis == 0 ? 1 : axis == 1 ? g.sy : g.sz);
    const long col_stride = axis == 0 ? g.sy : 1, row_stride = axis == 2 ? g.sy : g.sz;
    hipLaunchKernelGGL((slice_kernel<E, O>), dim3((unsigned)((npix + IM_THREADS - 1) / IM_THREADS)), dim3(IM_THREADS), 0, st, src, obs,
                       cols, npix, base, col_stride, row_stride, val, flag);
}
template void launch_image_slice<float, float>(hipStream_t, const GridDesc&, int, int, const float*, const float*, double*, uint8_t*);
template void launch_image_slice<double, float>(hipStream_t, const GridDesc&, int, int, const double*, const float*, double*, uint8_t*);
template void launch_image_slice<double, double>(hipStream_t, const GridDesc&, int, int, const double*, const double*, double*, uint8_t*);

template <class E>
void launch_image_project(hipStream_t st, const GridDesc& g, int kind, int axis, const E* src, double* val, uint8_t* flag)
{
    if (kind == IMG_SUM) project_kind<E, IMG_SUM>(st, g, axis, src, val, flag);
    else if (kind == IMG_MAX) project_kind<E, IMG_MAX>(st, g, axis, src, val, flag);
    else if (kind == IMG_MIN) project_kind<E, IMG_MIN>(st, g, axis, src, val, flag);
    else project_kind<E, IMG_ANY>(st, g, axis, src, val, flag);
}
template void launch_image_project<float>(hipStream_t, const GridDesc&, int, int, const float*, double*, uint8_t*);
template void launch_image_project<double>(hipStream_t, const GridDesc&, int, int, const double*, double*, uint8_t*);

void launch_image_colour(hipStream_t st, long npix, const double* val, const uint8_t* flag, double vmin, double vmax, double alpha,
                         const uint8_t* table, int n, uint8_t* rgb)
{
    if (npix <= 0) return;
    hipLaunchKernelGGL(colour_kernel, dim3((unsigned)((npix + IM_THREADS - 1) / IM_THREADS)), dim3(IM_THREADS), 0, st, npix, val, flag,
                       vmin, vmax, alpha, table, n, rgb);
}

}  // namespace fs
