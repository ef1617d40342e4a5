// advect.hip -- semi-Lagrangian advection in its four forms (per cell, per cell with clamp tables, row,
// tile), the clamp-table kernel and the gradient + velocity-advection pass.  Moved out of kernels.hip unchanged.
#include <hip/hip_runtime.h>
#include "kernels.h"
#include "kernels_dev.h"

namespace fs {

// =====================================================================================
// Semi-Lagrangian advection + setBounds(b, field)   simulation.cpp:367-424
// The back-trace is clamped in GLOBAL coordinates; `prev` may be the all-gathered global
// array under z-slab partitioning (prev_zshift = zoff planes), see fluidsim.cpp.
// =====================================================================================
template <class T>
__device__ __forceinline__ T clamp_ref(T v, T lo, T hi) { return (v < lo) ? lo : ((hi < v) ? hi : v); }   // std::clamp

// The two x-neighbours of a trace's corner as ONE load: an element-aligned 2-vector (global memory takes 8- / 16-byte
// loads at 4- / 8-byte alignment on this part).  A gather is paid per load instruction and distinct cache line, so four
// loads per trace instead of eight is what matters here, not the bytes.
typedef float pair_f __attribute__((ext_vector_type(2), aligned(4)));
typedef double pair_d __attribute__((ext_vector_type(2), aligned(8)));
template <class T> struct PairOf;
template <> struct PairOf<float> { using type = pair_f; };
template <> struct PairOf<double> { using type = pair_d; };
template <class T>
__device__ __forceinline__ typename PairOf<T>::type ld_pair(const T* p) { return *reinterpret_cast<const typename PairOf<T>::type*>(p); }

template <class T>
__device__ __forceinline__ T back_trace_tab(const GridDesc& g, const SlabCtx& sc, const T* __restrict__ src, long zshift,
                                            const T* __restrict__ tab, int x, int y, int z, T ux, T uy, T uz, T kx, T ky, T kz);

// TAB: traces whose x coordinate clamps read the pre-interpolated inlet / outlet column tables (see
// advect_columns_kernel below) instead of the eight scattered values of the big array.
template <class T, bool TAB>
__global__ __launch_bounds__(256) void advect_kernel(GridDesc g, SlabCtx sc, int b, T* __restrict__ field,
                                                      const T* __restrict__ prev, const T* vx, const T* vy,
                                                      const T* vz, const uint8_t* __restrict__ flags, T kx, T ky, T kz,
                                                      long prev_zshift, const T* __restrict__ tab)
{
    const int x = 1 + blockIdx.x * blockDim.x + threadIdx.x;
    const int y = 1 + blockIdx.y * blockDim.y + __builtin_amdgcn_readfirstlane(threadIdx.y);   // cell_block(): a wave is one row
    const int z = 1 + blockIdx.z;
    if (x > g.W || y > g.H) return;
    const long c = cell(g, x, y, z);
    const unsigned f = flags[c];
    const T one = (T)1, half = (T)0.5;
    T u = (T)0;
    if (!(f & F_SOLID)) {
        // :380-382: the component being advected is carried by its own pre-advection value; the density (b = 0) by the
        // current velocity alone -- its own value is not read at all (4 of 24 streamed bytes per cell)
        T ux, uy, uz;
        if (b == 0) {                                    // uniform
            ux = vx[c]; uy = vy[c]; uz = vz[c];
        } else {                                         // (the array being written is never read: `field` is restrict)
            const T own = prev[c + prev_zshift];
            ux = (b == 1) ? own : vx[c];
            uy = (b == 2) ? own : vy[c];
            uz = (b == 3) ? own : vz[c];
        }
        if constexpr (TAB) {
            u = back_trace_tab<T>(g, sc, prev, prev_zshift, tab, x, y, z, ux, uy, uz, kx, ky, kz);
        } else {
        const int zg = z + sc.zoff;                      // global plane index
        T px = clamp_ref<T>((T)x - kx * ux, half, (T)g.W + half);          // :384-390
        T py = clamp_ref<T>((T)y - ky * uy, half, (T)g.H + half);
        T pz = clamp_ref<T>((T)zg - kz * uz, half, (T)sc.Dglobal + half);
        const int x0 = (int)floor(px), y0 = (int)floor(py), z0 = (int)floor(pz);
        const T tx = px - (T)x0, ty = py - (T)y0, tz = pz - (T)z0;
        const T* s = prev + prev_zshift + cell(g, x0, y0, z0 - sc.zoff);
        const auto q00 = ld_pair(s), q01 = ld_pair(s + g.sz), q10 = ld_pair(s + g.sy), q11 = ld_pair(s + g.sy + g.sz);
        const T a00 = q00.x * (one - tx) + q00.y * tx;                        // :412-415
        const T a01 = q01.x * (one - tx) + q01.y * tx;
        const T a10 = q10.x * (one - tx) + q10.y * tx;
        const T a11 = q11.x * (one - tx) + q11.y * tx;
        const T b0 = a00 * (one - ty) + a10 * ty;                             // :417-418
        const T b1 = a01 * (one - ty) + a11 * ty;
        u = b0 * (one - tz) + b1 * tz;                                        // :420
        }
    }
    const bool kill = (b != 0) && (f & F_NEAR);
    field[c] = kill ? (T)0 : u;
    write_face_ghosts(g, sc, field, c, x, y, z, u, b);
}

// The three velocity advections of a step (simulation.cpp:125-127) in one pass.  advect(2)
// and advect(3) read the already advected v_x / v_y only at their own cell (:380-382), so one
// thread can chain them: trace v_x, then v_y with the new (stored) v_x, then v_z with the new
// v_x and v_y.  Eight array streams instead of fifteen; results are bit-identical.
template <class T>
__device__ __forceinline__ T back_trace(const GridDesc& g, const SlabCtx& sc, const T* __restrict__ src, long zshift,
                                        int x, int y, int z, T ux, T uy, T uz, T kx, T ky, T kz)
{
    // z is the local plane; the trace is clamped in global coordinates and `src + zshift` is indexed
    // with local planes (zshift = zoff planes when src is the gathered global array of a slab)
    const T one = (T)1, half = (T)0.5;
    T px = clamp_ref<T>((T)x - kx * ux, half, (T)g.W + half);          // :384-390
    T py = clamp_ref<T>((T)y - ky * uy, half, (T)g.H + half);
    T pz = clamp_ref<T>((T)(z + sc.zoff) - kz * uz, half, (T)sc.Dglobal + half);
    const int x0 = (int)floor(px), y0 = (int)floor(py), z0 = (int)floor(pz);
    const T tx = px - (T)x0, ty = py - (T)y0, tz = pz - (T)z0;
    const T* s = src + zshift + cell(g, x0, y0, z0 - sc.zoff);
    const auto q00 = ld_pair(s), q01 = ld_pair(s + g.sz), q10 = ld_pair(s + g.sy), q11 = ld_pair(s + g.sy + g.sz);
    const T a00 = q00.x * (one - tx) + q00.y * tx;                        // :412-415
    const T a01 = q01.x * (one - tx) + q01.y * tx;
    const T a10 = q10.x * (one - tx) + q10.y * tx;
    const T a11 = q11.x * (one - tx) + q11.y * tx;
    const T b0 = a00 * (one - ty) + a10 * ty;                             // :417-418
    const T b1 = a01 * (one - ty) + a11 * ty;
    return b0 * (one - tz) + b1 * tz;                                     // :420
}

template <class T, bool TAB>
__global__ __launch_bounds__(256) void advect_velocity_kernel(GridDesc g, SlabCtx sc, T* __restrict__ vx,
                                                               T* __restrict__ vy, T* __restrict__ vz,
                                                               const T* __restrict__ px, const T* __restrict__ py,
                                                               const T* __restrict__ pz,
                                                               const uint8_t* __restrict__ flags, T kx, T ky, T kz,
                                                               long zshift, const T* __restrict__ tab)
{
    const int x = 1 + blockIdx.x * blockDim.x + threadIdx.x;
    const int y = 1 + blockIdx.y * blockDim.y + __builtin_amdgcn_readfirstlane(threadIdx.y);   // cell_block(): a wave is one row
    const int z = 1 + blockIdx.z;
    if (x > g.W || y > g.H) return;
    const long c = cell(g, x, y, z);
    const unsigned f = flags[c];
    const bool near = (f & F_NEAR) != 0;
    T nx = (T)0, ny = (T)0, nz = (T)0;                   // un-zeroed results (0 inside solids, :375-377)
    T sx = (T)0, sy = (T)0;                              // what setBounds leaves in v_x, v_y
    if (!(f & F_SOLID)) {
        const T oy = vy[c], oz = vz[c];
        if constexpr (TAB) {
            const long plane2 = 2 * (long)(g.H + 2) * (g.D + 2);
            nx = back_trace_tab<T>(g, sc, px, zshift, tab, x, y, z, px[c + zshift], oy, oz, kx, ky, kz);
            sx = near ? (T)0 : nx;
            ny = back_trace_tab<T>(g, sc, py, zshift, tab + plane2, x, y, z, sx, py[c + zshift], oz, kx, ky, kz);
            sy = near ? (T)0 : ny;
            nz = back_trace_tab<T>(g, sc, pz, zshift, tab + 2 * plane2, x, y, z, sx, sy, pz[c + zshift], kx, ky, kz);
        } else {
            nx = back_trace<T>(g, sc, px, zshift, x, y, z, px[c + zshift], oy, oz, kx, ky, kz);
            sx = near ? (T)0 : nx;
            ny = back_trace<T>(g, sc, py, zshift, x, y, z, sx, py[c + zshift], oz, kx, ky, kz);
            sy = near ? (T)0 : ny;
            nz = back_trace<T>(g, sc, pz, zshift, x, y, z, sx, sy, pz[c + zshift], kx, ky, kz);
        }
    }
    vx[c] = near ? (T)0 : nx;
    vy[c] = near ? (T)0 : ny;
    vz[c] = near ? (T)0 : nz;
    write_face_ghosts(g, sc, vx, c, x, y, z, nx, 1);
    write_face_ghosts(g, sc, vy, c, x, y, z, ny, 2);
    write_face_ghosts(g, sc, vz, c, x, y, z, nz, 3);
}

// The gradient pass of the step's first projection (simulation.cpp:322-361) and the three velocity advections that follow
// it (:125-127) in one pass.  The advection overwrites all three velocities and reads the projected ones only at its own cell,
// and of those only v_y and v_z (v_x is carried by the pre-diffusion snapshot px, :380): a thread forms what the gradient pass
// would have stored there -- v - grad p, zeroed next to a solid (store_row_bounds) -- in registers and traces with it.  The
// projected v_x is never formed, the projected v_y, v_z and all three ghost-face sets never reach memory: the advection's own
// setBounds writes every one of those cells again, and no trace reads them (the traces read px, py, pz).  p's y and z
// neighbours come from L1 / L2 as in gradient_kernel.  In place: a thread reads vy, vz at its own cell before it writes it.
template <class T>
__global__ __launch_bounds__(256) void gradient_advect_velocity_kernel(GridDesc g, SlabCtx sc, const T* __restrict__ p,
                                                                        T* __restrict__ vx, T* __restrict__ vy,
                                                                        T* __restrict__ vz, const T* __restrict__ px,
                                                                        const T* __restrict__ py, const T* __restrict__ pz,
                                                                        const uint8_t* __restrict__ flags, T h, T two_h, T kx,
                                                                        T ky, T kz)
{
    const int x = 1 + blockIdx.x * blockDim.x + threadIdx.x;
    const int y = 1 + blockIdx.y * blockDim.y + __builtin_amdgcn_readfirstlane(threadIdx.y);   // cell_block(): a wave is one row
    const int z = 1 + blockIdx.z;
    if (x > g.W || y > g.H) return;
    const long c = cell(g, x, y, z);
    const unsigned f = flags[c];
    const bool near = (f & F_NEAR) != 0;
    T nx = (T)0, ny = (T)0, nz = (T)0;                   // un-zeroed results (0 inside solids, :375-377)
    T sx = (T)0, sy = (T)0;                              // what setBounds leaves in v_x, v_y
    if (!(f & F_SOLID)) {
        T oy = vy[c], oz = vz[c];
        const T pc = p[c];
        oy -= one_sided_grad<T>(f & F_YP, f & F_YM, p[c + g.sy], pc, p[c - g.sy], h, two_h);   // :326-334
        oz -= one_sided_grad<T>(f & F_ZP, f & F_ZM, p[c + g.sz], pc, p[c - g.sz], h, two_h);
        if (near) oy = oz = (T)0;                        // setBounds(2, v_y), (3, v_z) of the projection
        nx = back_trace<T>(g, sc, px, 0, x, y, z, px[c], oy, oz, kx, ky, kz);
        sx = near ? (T)0 : nx;
        ny = back_trace<T>(g, sc, py, 0, x, y, z, sx, py[c], oz, kx, ky, kz);
        sy = near ? (T)0 : ny;
        nz = back_trace<T>(g, sc, pz, 0, x, y, z, sx, sy, pz[c], kx, ky, kz);
    }
    vx[c] = near ? (T)0 : nx;
    vy[c] = near ? (T)0 : ny;
    vz[c] = near ? (T)0 : nz;
    write_face_ghosts(g, sc, vx, c, x, y, z, nx, 1);
    write_face_ghosts(g, sc, vy, c, x, y, z, ny, 2);
    write_face_ghosts(g, sc, vz, c, x, y, z, nz, 3);
}

// ---- row forms of the two advection kernels (option advect_kernels=row; NOT the default) ------------
// Measured slower than the per-cell kernels above on MI355X (512^3: 2.8 against 2.4 ms per step fp32, 5.0
// against 3.5 fp64, profiles/r02g_advect_row_vs_cell_*.json): the per-cell form already gets what this form
// was built for -- a wave's 64 clamped traces land on the same two or three cache lines of the inlet column,
// so its gathers coalesce by themselves -- and it keeps four times as many waves in flight to hide the
// latency of the dependent gather.  Kept because it is exercised by the tests (bit-identical) and documents
// the experiment.
// Same arithmetic, restructured around what the memory system sees:
//  * a lane owns four x-consecutive cells: the velocities, the cell's own source values and the result move as
//    one dwordx4 each (a wave = 1 KiB of a row per stream), the solid / near-solid tests come from the kill byte
//    (one byte per four cells) instead of four flag bytes;
//  * the back-trace is data-dependent, but in a wind tunnel most of it is not: dt*W*u_x is hundreds of cells
//    (SURVEY 7.3-3), so the x coordinate of almost every trace clamps to 0.5 -- x0 = 0, weight exactly 0.5
//    (:388, :392-401) -- and the x interpolation (:412-415) only ever combines the ghost column x = 0 with
//    x = 1 (or x = W with W+1 at the other clamp).  advect_columns_kernel does that interpolation once per
//    (y, z) into two small tables (2 x (H+2)(D+2) values per source field, L2-resident); a clamped trace then
//    reads 4 table values as two 8-byte loads instead of 8 scattered values of the big array.  Same
//    expression, same operands, same rounding: bit-identical with the per-cell kernels (tests).
// Traces that do not clamp gather as before.  Wave shuffles do not apply here: which lanes share source rows
// depends on the velocities.
template <class T>
__global__ __launch_bounds__(256) void advect_columns_kernel(GridDesc g, const T* __restrict__ p0, const T* __restrict__ p1,
                                                              const T* __restrict__ p2, int nsrc, T* __restrict__ tab)
{
    // tab[(2*k + side) * (H+2)(D+2) + y + z*(H+2)]: source k, side 0 = columns (0, 1), side 1 = columns (W, W+1)
    const long plane = (long)(g.H + 2) * (g.D + 2);
    const long i = blockIdx.x * (long)blockDim.x + threadIdx.x;
    if (i >= plane) return;
    const int y = (int)(i % (g.H + 2)), z = (int)(i / (g.H + 2));
    const T one = (T)1, half = (T)0.5;
    for (int k = 0; k < nsrc; ++k) {
        const T* s = (k == 0 ? p0 : k == 1 ? p1 : p2) + cell(g, 0, y, z);
        tab[(2 * k + 0) * plane + i] = s[0] * (one - half) + s[1] * half;                 // :412-415 with tx = 0.5
        tab[(2 * k + 1) * plane + i] = s[g.W] * (one - half) + s[g.W + 1] * half;
    }
}

template <class T>
__device__ __forceinline__ T back_trace_tab(const GridDesc& g, const SlabCtx& sc, const T* __restrict__ src, long zshift,
                                            const T* __restrict__ tab, int x, int y, int z, T ux, T uy, T uz, T kx, T ky, T kz)
{
    const T one = (T)1, half = (T)0.5;
    const T px = clamp_ref<T>((T)x - kx * ux, half, (T)g.W + half);          // :384-390
    const T py = clamp_ref<T>((T)y - ky * uy, half, (T)g.H + half);
    const T pz = clamp_ref<T>((T)(z + sc.zoff) - kz * uz, half, (T)sc.Dglobal + half);
    const int y0 = (int)floor(py), z0 = (int)floor(pz);
    const T ty = py - (T)y0, tz = pz - (T)z0;
    T a00, a01, a10, a11;
    const bool lo = (px == half), hi = (px == (T)g.W + half);
    if (tab != nullptr && (lo || hi)) {
        // x0 = 0 (or W) and tx = 0.5 exactly: the x interpolation was done by advect_columns_kernel
        const long plane = (long)(g.H + 2) * (g.D + 2);
        const T* t = tab + (hi ? plane : 0) + y0 + (long)z0 * (g.H + 2);
        a00 = t[0];
        a10 = t[1];
        a01 = t[g.H + 2];
        a11 = t[g.H + 3];
    } else {
        const int x0 = (int)floor(px);
        const T tx = px - (T)x0;
        const T* s = src + zshift + cell(g, x0, y0, z0 - sc.zoff);
        const auto q00 = ld_pair(s), q01 = ld_pair(s + g.sz), q10 = ld_pair(s + g.sy), q11 = ld_pair(s + g.sy + g.sz);
        a00 = q00.x * (one - tx) + q00.y * tx;                                // :412-415
        a01 = q01.x * (one - tx) + q01.y * tx;
        a10 = q10.x * (one - tx) + q10.y * tx;
        a11 = q11.x * (one - tx) + q11.y * tx;
    }
    const T b0 = a00 * (one - ty) + a10 * ty;                                 // :417-418
    const T b1 = a01 * (one - ty) + a11 * ty;
    return b0 * (one - tz) + b1 * tz;                                         // :420
}

// advect(b, field, prev) + setBounds(b, field): four cells per lane
template <class T>
__global__ __launch_bounds__(256) void advect_row_kernel(GridDesc g, SlabCtx sc, int b, T* __restrict__ field,
                                                          const T* __restrict__ prev, const T* vx, const T* vy, const T* vz,
                                                          const uint8_t* __restrict__ kill, const T* __restrict__ tab, T kx,
                                                          T ky, T kz, long zshift)
{
    const int x0 = 1 + (blockIdx.x * 64 + (threadIdx.x & 63)) * 4;
    const int y = 1 + blockIdx.y * 4 + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);   // a wave is one row
    const int z = 1 + blockIdx.z;
    if (x0 > g.W || y > g.H) return;
    const long c = cell(g, x0, y, z);
    const unsigned kb = kill[(c + 3) >> 2];              // bits 0-3 solid, bits 4-7 solid or next to a solid
    T own[4], ax[4], ay[4], az[4], u[4];
    ld_row(prev + c + zshift, b != 0, own);
    ld_row(vx + c, b != 1, ax);
    ld_row(vy + c, b != 2, ay);
    ld_row(vz + c, b != 3, az);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        u[e] = (T)0;                                     // solid cells: 0 (:375-377)
        if (x0 + e <= g.W && !((kb >> e) & 1u)) {
            const T ux = (b == 1) ? own[e] : ax[e];      // :380-382
            const T uy = (b == 2) ? own[e] : ay[e];
            const T uz = (b == 3) ? own[e] : az[e];
            u[e] = back_trace_tab<T>(g, sc, prev, zshift, tab, x0 + e, y, z, ux, uy, uz, kx, ky, kz);
        }
    }
    store_row_bounds<T>(g, sc, field, c, x0, y, z, u, (b == 0) ? (kb & 15u) : (kb >> 4), b);
}

// the three velocity advections of a step in one pass (see advect_velocity_kernel): four cells per lane
template <class T>
__global__ __launch_bounds__(256) void advect_velocity_row_kernel(GridDesc g, SlabCtx sc, T* __restrict__ vx, T* __restrict__ vy,
                                                                   T* __restrict__ vz, const T* __restrict__ px,
                                                                   const T* __restrict__ py, const T* __restrict__ pz,
                                                                   const uint8_t* __restrict__ kill, const T* __restrict__ tab,
                                                                   T kx, T ky, T kz, long zshift)
{
    const int x0 = 1 + (blockIdx.x * 64 + (threadIdx.x & 63)) * 4;
    const int y = 1 + blockIdx.y * 4 + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int z = 1 + blockIdx.z;
    if (x0 > g.W || y > g.H) return;
    const long c = cell(g, x0, y, z);
    const unsigned kb = kill[(c + 3) >> 2];
    const unsigned near4 = kb >> 4;
    const long plane2 = 2 * (long)(g.H + 2) * (g.D + 2);
    const T* tx_ = tab, *ty_ = tab ? tab + plane2 : nullptr, *tz_ = tab ? tab + 2 * plane2 : nullptr;
    T ox[4], oy[4], oz[4], qy[4], qz[4], nx[4], ny[4], nz[4];
    ld_row(px + c + zshift, true, ox);
    ld_row(py + c + zshift, true, qy);
    ld_row(pz + c + zshift, true, qz);
    ld_row(vy + c, true, oy);
    ld_row(vz + c, true, oz);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        nx[e] = ny[e] = nz[e] = (T)0;                    // un-zeroed results (0 inside solids, :375-377)
        if (x0 + e <= g.W && !((kb >> e) & 1u)) {
            const bool near = ((near4 >> e) & 1u) != 0;
            nx[e] = back_trace_tab<T>(g, sc, px, zshift, tx_, x0 + e, y, z, ox[e], oy[e], oz[e], kx, ky, kz);
            const T sx = near ? (T)0 : nx[e];            // what setBounds leaves in v_x
            ny[e] = back_trace_tab<T>(g, sc, py, zshift, ty_, x0 + e, y, z, sx, qy[e], oz[e], kx, ky, kz);
            const T sy = near ? (T)0 : ny[e];
            nz[e] = back_trace_tab<T>(g, sc, pz, zshift, tz_, x0 + e, y, z, sx, sy, qz[e], kx, ky, kz);
        }
    }
    store_row_bounds<T>(g, sc, vx, c, x0, y, z, nx, near4, 1);
    store_row_bounds<T>(g, sc, vy, c, x0, y, z, ny, near4, 2);
    store_row_bounds<T>(g, sc, vz, c, x0, y, z, nz, near4, 3);
}

// ---- tile form (option advect_kernels=tile; round 3) ---------------------------------------------------------------
// Where the flow is rough (the properly projected flow of solver=mg: |u_y|, |u_z| of order one, i.e. traces that leave
// their cell by tens of rows and planes) the 64 traces of a wave end in up to 64 different cache lines per load and the
// per-cell kernels spend their time in the L2 -> L1 path.  The x coordinate still clamps to the
// inlet for almost every trace, so what is gathered is the x-interpolated inlet column table (advect_columns_kernel):
// a workgroup owns TY x TZ (y, z) rows of cells over the whole row length, stages the window of that table that
// traces of at most R rows / planes can reach in LDS -- coalesced, once per 32 K cells -- and gathers from there; a
// trace that leaves the window, or does not clamp, takes the per-cell path (global table or array).  Same table values,
// same expressions: bit-identical with the other forms.
template <class T, int NF>
__global__ __launch_bounds__(1024) void advect_tile_kernel(GridDesc g, SlabCtx sc, int b, T* __restrict__ f0, T* __restrict__ f1,
                                                            T* __restrict__ f2, const T* __restrict__ p0, const T* __restrict__ p1,
                                                            const T* __restrict__ p2, const T* vx, const T* vy, const T* vz,
                                                            const uint8_t* __restrict__ flags, T kx, T ky, T kz,
                                                            const T* __restrict__ tab, int R)
{
    constexpr int TY = 8, TZ = 8;
    extern __shared__ unsigned char win_raw[];
    T* win = reinterpret_cast<T*>(win_raw);
    const int ty0 = 1 + blockIdx.x * TY, tz0 = 1 + blockIdx.y * TZ;
    // window of table rows (y) and planes (z) this tile's traces can reach, clipped to the table
    const int wy0 = max(0, ty0 - R), wy1 = min(g.H + 1, ty0 + TY + R), wz0 = max(0, tz0 - R), wz1 = min(g.D + 1, tz0 + TZ + R);
    const int WY = wy1 - wy0 + 1, WZ = wz1 - wz0 + 1;
    const long tplane = (long)(g.H + 2) * (g.D + 2);
    for (int k = 0; k < NF; ++k) {
        const T* t = tab + 2 * k * tplane;                   // the inlet side of source k
        for (int i = threadIdx.x; i < WY * WZ; i += 1024) {
            const int yy = i % WY, zz = i / WY;
            win[(long)k * WY * WZ + i] = t[(wy0 + yy) + (long)(wz0 + zz) * (g.H + 2)];
        }
    }
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const T one = (T)1, half = (T)0.5;
    // one trace of source k (arguments as back_trace_tab)
    auto trace = [&](int k, const T* src, int x, int y, int z, T ux, T uy, T uz) -> T {
        const T px = clamp_ref<T>((T)x - kx * ux, half, (T)g.W + half);          // :384-390
        const T py = clamp_ref<T>((T)y - ky * uy, half, (T)g.H + half);
        const T pz = clamp_ref<T>((T)z - kz * uz, half, (T)g.D + half);
        const int y0 = (int)floor(py), z0 = (int)floor(pz);
        if (px == half && y0 >= wy0 && y0 + 1 <= wy1 && z0 >= wz0 && z0 + 1 <= wz1) {
            const T ty = py - (T)y0, tz = pz - (T)z0;
            const T* w = win + (long)k * WY * WZ + (y0 - wy0) + (long)(z0 - wz0) * WY;
            const T a00 = w[0], a10 = w[1], a01 = w[WY], a11 = w[WY + 1];
            const T b0 = a00 * (one - ty) + a10 * ty;                         // :417-418
            const T b1 = a01 * (one - ty) + a11 * ty;
            return b0 * (one - tz) + b1 * tz;                                 // :420
        }
        return back_trace_tab<T>(g, sc, src, 0, tab + 2 * k * tplane, x, y, z, ux, uy, uz, kx, ky, kz);
    };
    // 16 waves share the TY x TZ rows of the tile; a wave walks its rows 64 cells at a time
    for (int row = wave; row < TY * TZ; row += 16) {
        const int y = ty0 + row % TY, z = tz0 + row / TY;
        if (y > g.H || z > g.D) continue;                    // wave-uniform
        for (int x = 1 + lane; x <= g.W; x += 64) {
            const long c = cell(g, x, y, z);
            const unsigned f = flags[c];
            const bool near = (f & F_NEAR) != 0;
            if constexpr (NF == 1) {
                T u = (T)0;
                if (!(f & F_SOLID)) {
                    T ux, uy, uz;
                    if (b == 0) {                            // uniform
                        ux = vx[c]; uy = vy[c]; uz = vz[c];
                    } else {
                        const T own = p0[c];
                        ux = (b == 1) ? own : vx[c];         // :380-382
                        uy = (b == 2) ? own : vy[c];
                        uz = (b == 3) ? own : vz[c];
                    }
                    u = trace(0, p0, x, y, z, ux, uy, uz);
                }
                f0[c] = ((b != 0) && near) ? (T)0 : u;
                write_face_ghosts(g, sc, f0, c, x, y, z, u, b);
            } else {
                T nx = (T)0, ny = (T)0, nz = (T)0;           // un-zeroed results (0 inside solids, :375-377)
                if (!(f & F_SOLID)) {
                    const T oy = f1[c], oz = f2[c];          // f0, f1, f2 = v_x, v_y, v_z: read at the own cell, then overwritten
                    nx = trace(0, p0, x, y, z, p0[c], oy, oz);
                    const T sx = near ? (T)0 : nx;           // what setBounds leaves in v_x
                    ny = trace(1, p1, x, y, z, sx, p1[c], oz);
                    const T sy = near ? (T)0 : ny;
                    nz = trace(2, p2, x, y, z, sx, sy, p2[c]);
                }
                f0[c] = near ? (T)0 : nx;
                f1[c] = near ? (T)0 : ny;
                f2[c] = near ? (T)0 : nz;
                write_face_ghosts(g, sc, f0, c, x, y, z, nx, 1);
                write_face_ghosts(g, sc, f1, c, x, y, z, ny, 2);
                write_face_ghosts(g, sc, f2, c, x, y, z, nz, 3);
            }
        }
    }
}

// window radius that fits 64 KB of LDS for NF staged tables (the tile is 8 x 8 rows)
template <class T>
static int tile_window(int want, int nf)
{
    int r = want < 1 ? 1 : want;
    while (r > 1 && (long)nf * (8 + 2 * r + 1) * (8 + 2 * r + 1) * (long)sizeof(T) > 64 * 1024) --r;
    return r;
}

// the clamp tables only describe a source array that is this GPU's whole domain (a slab traces into the gathered array)
template <class T>
static const T* build_columns(hipStream_t st, const GridDesc& g, const SlabCtx& sc, const T* p0, const T* p1, const T* p2,
                              int nsrc, T* coltab, long zshift)
{
    if (!coltab || zshift != 0 || !(sc.lo_wall && sc.hi_wall)) return nullptr;
    const long plane = (long)(g.H + 2) * (g.D + 2);
    hipLaunchKernelGGL((advect_columns_kernel<T>), dim3((unsigned)((plane + 255) / 256)), dim3(256), 0, st, g, p0, p1, p2, nsrc,
                       coltab);
    return coltab;
}

template <class T>
void launch_advect_velocity(hipStream_t st, const SweepTune& tune, const GridDesc& g, const SlabCtx& sc, T* vx, T* vy, T* vz,
                            const T* px, const T* py, const T* pz, const uint8_t* flags, const uint8_t* kill, T* coltab, T kx,
                            T ky, T kz, long zshift)
{
    const T* tab = (tune.advect_cell == 1) ? nullptr : build_columns<T>(st, g, sc, px, py, pz, 3, coltab, zshift);
    if (tune.advect_cell == 3 && tab) {
        const int R = tile_window<T>(tune.advect_window, 3);
        const size_t lds = (size_t)3 * (8 + 2 * R + 1) * (8 + 2 * R + 1) * sizeof(T);
        hipLaunchKernelGGL((advect_tile_kernel<T, 3>), dim3((g.H + 7) / 8, (g.D + 7) / 8), dim3(1024), lds, st, g, sc, 0, vx, vy, vz, px,
                           py, pz, vx, vy, vz, flags, kx, ky, kz, tab, R);
        return;
    }
    if (tune.advect_cell) {
        if (tab)
            hipLaunchKernelGGL((advect_velocity_kernel<T, true>), cell_grid(g), cell_block(), 0, st, g, sc, vx, vy, vz, px, py,
                               pz, flags, kx, ky, kz, zshift, tab);
        else
            hipLaunchKernelGGL((advect_velocity_kernel<T, false>), cell_grid(g), cell_block(), 0, st, g, sc, vx, vy, vz, px, py,
                               pz, flags, kx, ky, kz, zshift, tab);
        return;
    }
    hipLaunchKernelGGL((advect_velocity_row_kernel<T>), row_grid(g), dim3(256), 0, st, g, sc, vx, vy, vz, px, py, pz, kill, tab,
                       kx, ky, kz, zshift);
}
template void launch_advect_velocity<float>(hipStream_t, const SweepTune&, const GridDesc&, const SlabCtx&, float*, float*,
                                            float*, const float*, const float*, const float*, const uint8_t*, const uint8_t*,
                                            float*, float, float, float, long);
template void launch_advect_velocity<double>(hipStream_t, const SweepTune&, const GridDesc&, const SlabCtx&, double*, double*,
                                             double*, const double*, const double*, const double*, const uint8_t*,
                                             const uint8_t*, double*, double, double, double, long);

template <class T>
void launch_gradient_advect_velocity(hipStream_t st, const GridDesc& g, const SlabCtx& sc, const T* p, T* vx, T* vy, T* vz,
                                     const T* px, const T* py, const T* pz, const uint8_t* flags, T h, T two_h, T kx, T ky, T kz)
{
    hipLaunchKernelGGL((gradient_advect_velocity_kernel<T>), cell_grid(g), cell_block(), 0, st, g, sc, p, vx, vy, vz, px, py, pz,
                       flags, h, two_h, kx, ky, kz);
}
template void launch_gradient_advect_velocity<float>(hipStream_t, const GridDesc&, const SlabCtx&, const float*, float*, float*,
                                                     float*, const float*, const float*, const float*, const uint8_t*, float,
                                                     float, float, float, float);
template void launch_gradient_advect_velocity<double>(hipStream_t, const GridDesc&, const SlabCtx&, const double*, double*, double*,
                                                      double*, const double*, const double*, const double*, const uint8_t*,
                                                      double, double, double, double, double);

template <class T>
void launch_advect(hipStream_t st, const SweepTune& tune, const GridDesc& g, const SlabCtx& sc, int b, T* field, const T* prev,
                   const T* vx, const T* vy, const T* vz, const uint8_t* flags, const uint8_t* kill, T* coltab, T kx, T ky, T kz,
                   long prev_zshift)
{
    const T* tab = (tune.advect_cell == 1) ? nullptr : build_columns<T>(st, g, sc, prev, prev, prev, 1, coltab, prev_zshift);
    if (tune.advect_cell == 3 && tab) {
        const int R = tile_window<T>(tune.advect_window, 1);
        const size_t lds = (size_t)(8 + 2 * R + 1) * (8 + 2 * R + 1) * sizeof(T);
        hipLaunchKernelGGL((advect_tile_kernel<T, 1>), dim3((g.H + 7) / 8, (g.D + 7) / 8), dim3(1024), lds, st, g, sc, b, field, field,
                           field, prev, prev, prev, vx, vy, vz, flags, kx, ky, kz, tab, R);
        return;
    }
    if (tune.advect_cell) {
        if (tab)
            hipLaunchKernelGGL((advect_kernel<T, true>), cell_grid(g), cell_block(), 0, st, g, sc, b, field, prev, vx, vy, vz,
                               flags, kx, ky, kz, prev_zshift, tab);
        else
            hipLaunchKernelGGL((advect_kernel<T, false>), cell_grid(g), cell_block(), 0, st, g, sc, b, field, prev, vx, vy, vz,
                               flags, kx, ky, kz, prev_zshift, tab);
        return;
    }
    hipLaunchKernelGGL((advect_row_kernel<T>), row_grid(g), dim3(256), 0, st, g, sc, b, field, prev, vx, vy, vz, kill, tab, kx,
                       ky, kz, prev_zshift);
}
template void launch_advect<float>(hipStream_t, const SweepTune&, const GridDesc&, const SlabCtx&, int, float*, const float*,
                                   const float*, const float*, const float*, const uint8_t*, const uint8_t*, float*, float, float,
                                   float, long);
template void launch_advect<double>(hipStream_t, const SweepTune&, const GridDesc&, const SlabCtx&, int, double*, const double*,
                                    const double*, const double*, const double*, const uint8_t*, const uint8_t*, double*, double,
                                    double, double, long);

}  // namespace fs
