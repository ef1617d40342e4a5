// project.hip -- the two projection passes around the pressure solve (divergence, gradient), each in
// its z-marching form and in the per-cell form that states it plainly.  Moved out of kernels.hip unchanged.
#include <hip/hip_runtime.h>
#include "kernels.h"
#include "kernels_dev.h"

namespace fs {

// =====================================================================================
// z-marching forms of the two projection passes.  Same wave decomposition as the sweep
// (256 x-consecutive cells x RY rows per wave, 16 B per lane, XCD-contiguous tiles): the
// planes z-1 / z+1 a cell needs stay in registers while the wave walks along z, rows y-1 /
// y+1 are L1/L2 hits, x neighbours cross lanes by shuffle, so every input array is read from
// HBM once.  Arithmetic and pass order are those of the per-cell kernels below, which remain
// as the plain statement (and serve fs_set_option "project_kernels"="cell").
// =====================================================================================
// (MarchTile, march_tile, ld_row and store_row_bounds live in kernels_dev.h: vortex.hip and heat.hip march the same way)

// divergence + pressure reset + setBounds(0,div) + setBounds(0,p)   simulation.cpp:295-319
// STORE_P = false leaves `p` alone: the caller starts the pressure solve with a pass that takes level 0 as all zeros
// instead of reading it (sweep_fused.hip, zero start), so the reset would be written to HBM for nobody.
template <class T, int RY, bool STORE_P>
__global__ __launch_bounds__(256) void divergence_march_kernel(GridDesc g, SlabCtx sc, const T* __restrict__ vx,
                                                                const T* __restrict__ vy, const T* __restrict__ vz,
                                                                T* __restrict__ dv, T* __restrict__ p,
                                                                const uint8_t* __restrict__ flags, T mhalf_h, int zc_len,
                                                                int nxw, int nybg, int nblk)
{
    const MarchTile<T> t = march_tile<T, RY>(g, zc_len, nxw, nybg, nblk);
    if (!t.live) return;                                 // wave-uniform
    const int H = g.H;
    const T zero = (T)0;
    T zm[RY][4], zc[RY][4], zp[RY][4];                   // v_z at planes z-1, z, z+1
#pragma unroll
    for (int r = 0; r < RY; ++r) {
        const bool on = t.lane_on && (t.y0 + r <= H);
        ld_row(vz + t.row0 + (long)(t.zbeg - 1) * g.sz + r * g.sy, on, zm[r]);
        ld_row(vz + t.row0 + (long)t.zbeg * g.sz + r * g.sy, on, zc[r]);
    }
    for (int z = t.zbeg; z <= t.zend; ++z) {
        const long off = t.row0 + (long)z * g.sz;
        T xr[RY][4], yr[RY + 2][4];
        unsigned fl[RY];
#pragma unroll
        for (int r = 0; r < RY; ++r) {
            const bool on = t.lane_on && (t.y0 + r <= H);
            ld_row(vz + off + g.sz + r * g.sy, on, zp[r]);
            ld_row(vx + off + r * g.sy, on, xr[r]);
            fl[r] = on ? *reinterpret_cast<const unsigned*>(flags + off + r * g.sy) : 0u;
        }
#pragma unroll
        for (int r = 0; r < RY + 2; ++r) ld_row(vy + off + (r - 1) * g.sy, t.lane_on && (t.y0 + r - 1 <= H + 1), yr[r]);
#pragma unroll
        for (int r = 0; r < RY; ++r) {
            const int y = t.y0 + r;
            T left = __shfl_up(xr[r][3], 1);
            T right = __shfl_down(xr[r][0], 1);
            if (!(t.lane_on && y <= H)) continue;        // y <= H is wave-uniform; shuffles are above
            const long base = off + r * g.sy;
            if (t.edge_l) left = vx[base - 1];
            if (t.edge_r) right = vx[base + 4];
            T d[4], zeros[4] = {zero, zero, zero, zero};
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const unsigned f = (fl[r] >> (8 * e)) & 0xffu;
                T acc = zero;                            // :306-312 in this order
                if (f & F_XP) acc += (e < 3) ? xr[r][e + 1] : right;
                if (f & F_XM) acc -= (e > 0) ? xr[r][e - 1] : left;
                if (f & F_YP) acc += yr[r + 2][e];
                if (f & F_YM) acc -= yr[r][e];
                if (f & F_ZP) acc += zp[r][e];
                if (f & F_ZM) acc -= zm[r][e];
                d[e] = (f & F_SOLID) ? zero : mhalf_h * acc;
            }
            store_row_bounds<T>(g, sc, dv, base, t.x0, y, z, d, 0u, 0);
            if constexpr (STORE_P) store_row_bounds<T>(g, sc, p, base, t.x0, y, z, zeros, 0u, 0);
        }
#pragma unroll
        for (int r = 0; r < RY; ++r)
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                zm[r][e] = zc[r][e];
                zc[r][e] = zp[r][e];
            }
    }
}

// v -= grad p, then setBounds(1,vx), (2,vy), (3,vz)   simulation.cpp:322-361
template <class T, int RY>
__global__ __launch_bounds__(256) void gradient_march_kernel(GridDesc g, SlabCtx sc, const T* __restrict__ p,
                                                              T* __restrict__ vx, T* __restrict__ vy, T* __restrict__ vz,
                                                              const uint8_t* __restrict__ flags, T h, T two_h, int zc_len,
                                                              int nxw, int nybg, int nblk)
{
    const MarchTile<T> t = march_tile<T, RY>(g, zc_len, nxw, nybg, nblk);
    if (!t.live) return;
    const int H = g.H;
    T pm[RY][4], pc[RY][4], pp[RY][4];
#pragma unroll
    for (int r = 0; r < RY; ++r) {
        const bool on = t.lane_on && (t.y0 + r <= H);
        ld_row(p + t.row0 + (long)(t.zbeg - 1) * g.sz + r * g.sy, on, pm[r]);
        ld_row(p + t.row0 + (long)t.zbeg * g.sz + r * g.sy, on, pc[r]);
    }
    for (int z = t.zbeg; z <= t.zend; ++z) {
        const long off = t.row0 + (long)z * g.sz;
        T hb[4], ht[4];
        ld_row(p + off - g.sy, t.lane_on, hb);
        ld_row(p + off + RY * g.sy, t.lane_on && (t.y0 + RY <= H + 1), ht);
        unsigned fl[RY];
#pragma unroll
        for (int r = 0; r < RY; ++r) {
            const bool on = t.lane_on && (t.y0 + r <= H);
            ld_row(p + off + g.sz + r * g.sy, on, pp[r]);
            fl[r] = on ? *reinterpret_cast<const unsigned*>(flags + off + r * g.sy) : 0u;
        }
        // in a partial band the row above the last live row is the ghost row H+1, not loaded above
#pragma unroll
        for (int r = 1; r < RY; ++r)
            if (t.y0 + r == H + 1) ld_row(p + off + r * g.sy, t.lane_on, pc[r]);
#pragma unroll
        for (int r = 0; r < RY; ++r) {
            const int y = t.y0 + r;
            T left = __shfl_up(pc[r][3], 1);
            T right = __shfl_down(pc[r][0], 1);
            if (!(t.lane_on && y <= H)) continue;
            const long base = off + r * g.sy;
            if (t.edge_l) left = p[base - 1];
            if (t.edge_r) right = p[base + 4];
            T ux[4], uy[4], uz[4];
            ld_row(vx + base, true, ux);
            ld_row(vy + base, true, uy);
            ld_row(vz + base, true, uz);
            unsigned killmask = 0;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const unsigned f = (fl[r] >> (8 * e)) & 0xffu;
                if (f & (F_SOLID | F_NEAR)) killmask |= 1u << e;
                if (!(f & F_SOLID)) {                    // :326
                    const T c0 = pc[r][e];
                    const T xp1 = (e < 3) ? pc[r][e + 1] : right, xm1 = (e > 0) ? pc[r][e - 1] : left;
                    const T yp1 = (r < RY - 1) ? pc[r < RY - 1 ? r + 1 : r][e] : ht[e];
                    const T ym1 = (r > 0) ? pc[r > 0 ? r - 1 : 0][e] : hb[e];
                    ux[e] -= one_sided_grad<T>(f & F_XP, f & F_XM, xp1, c0, xm1, h, two_h);
                    uy[e] -= one_sided_grad<T>(f & F_YP, f & F_YM, yp1, c0, ym1, h, two_h);
                    uz[e] -= one_sided_grad<T>(f & F_ZP, f & F_ZM, pp[r][e], c0, pm[r][e], h, two_h);
                }
            }
            store_row_bounds<T>(g, sc, vx, base, t.x0, y, z, ux, killmask, 1);
            store_row_bounds<T>(g, sc, vy, base, t.x0, y, z, uy, killmask, 2);
            store_row_bounds<T>(g, sc, vz, base, t.x0, y, z, uz, killmask, 3);
        }
#pragma unroll
        for (int r = 0; r < RY; ++r)
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                pm[r][e] = pc[r][e];
                pc[r][e] = pp[r][e];
            }
    }
}

// (MarchLaunch / march_launch: kernels_dev.h)

// (write_face_ghosts, the ghost-face writes of the per-cell kernels, lives in kernels_dev.h)

// =====================================================================================
// project, part 1: divergence + pressure reset + setBounds(0,div) + setBounds(0,p)
//   simulation.cpp:295-319
// =====================================================================================
template <class T, bool STORE_P>
__global__ __launch_bounds__(256) void divergence_kernel(GridDesc g, SlabCtx sc, const T* __restrict__ vx,
                                                          const T* __restrict__ vy, const T* __restrict__ vz,
                                                          T* __restrict__ dv, T* __restrict__ p,
                                                          const uint8_t* __restrict__ flags, T mhalf_h)
{
    const int x = 1 + blockIdx.x * blockDim.x + threadIdx.x;
    const int y = 1 + blockIdx.y * blockDim.y + threadIdx.y;
    const int z = 1 + blockIdx.z;
    if (x > g.W || y > g.H) return;
    const long c = cell(g, x, y, z);
    const unsigned f = flags[c];
    T d = (T)0;
    if (!(f & F_SOLID)) {
        T acc = (T)0;                                    // :306-312
        if (f & F_XP) acc += vx[c + 1];
        if (f & F_XM) acc -= vx[c - 1];
        if (f & F_YP) acc += vy[c + g.sy];
        if (f & F_YM) acc -= vy[c - g.sy];
        if (f & F_ZP) acc += vz[c + g.sz];
        if (f & F_ZM) acc -= vz[c - g.sz];
        d = mhalf_h * acc;                               // (-0.5f*h)*div_val, :314
    }
    dv[c] = d;
    write_face_ghosts(g, sc, dv, c, x, y, z, d, 0);      // setBounds(0,div): solid cells already hold 0
    if constexpr (STORE_P) {
        p[c] = (T)0;
        write_face_ghosts(g, sc, p, c, x, y, z, (T)0, 0);    // setBounds(0,p)
    }
}

template <class T>
void launch_divergence(hipStream_t st, const SweepTune& tune, const GridDesc& g, const SlabCtx& sc, const T* vx, const T* vy,
                       const T* vz, T* div, T* p, const uint8_t* flags, T mhalf_h, bool store_p)
{
    if (tune.project_cell) {
        if (store_p)
            hipLaunchKernelGGL((divergence_kernel<T, true>), cell_grid(g), cell_block(), 0, st, g, sc, vx, vy, vz, div, p, flags,
                               mhalf_h);
        else
            hipLaunchKernelGGL((divergence_kernel<T, false>), cell_grid(g), cell_block(), 0, st, g, sc, vx, vy, vz, div, p, flags,
                               mhalf_h);
        return;
    }
    constexpr int RY = 2;
    const MarchLaunch m = march_launch(g, RY);
    if (store_p)
        hipLaunchKernelGGL((divergence_march_kernel<T, RY, true>), dim3(m.nblk), dim3(256), 0, st, g, sc, vx, vy, vz, div, p, flags,
                           mhalf_h, m.zc_len, m.nxw, m.nybg, m.nblk);
    else
        hipLaunchKernelGGL((divergence_march_kernel<T, RY, false>), dim3(m.nblk), dim3(256), 0, st, g, sc, vx, vy, vz, div, p, flags,
                           mhalf_h, m.zc_len, m.nxw, m.nybg, m.nblk);
}
template void launch_divergence<float>(hipStream_t, const SweepTune&, const GridDesc&, const SlabCtx&, const float*,
                                       const float*, const float*, float*, float*, const uint8_t*, float, bool);
template void launch_divergence<double>(hipStream_t, const SweepTune&, const GridDesc&, const SlabCtx&, const double*,
                                        const double*, const double*, double*, double*, const uint8_t*, double, bool);

// =====================================================================================
// project, part 2: v -= grad p, then setBounds(1,vx), (2,vy), (3,vz)
//   simulation.cpp:322-361
// =====================================================================================

template <class T>
__global__ __launch_bounds__(256) void gradient_kernel(GridDesc g, SlabCtx sc, const T* __restrict__ p,
                                                        T* __restrict__ vx, T* __restrict__ vy, T* __restrict__ vz,
                                                        const uint8_t* __restrict__ flags, T h, T two_h)
{
    const int x = 1 + blockIdx.x * blockDim.x + threadIdx.x;
    const int y = 1 + blockIdx.y * blockDim.y + threadIdx.y;
    const int z = 1 + blockIdx.z;
    if (x > g.W || y > g.H) return;
    const long c = cell(g, x, y, z);
    const unsigned f = flags[c];
    T ux = vx[c], uy = vy[c], uz = vz[c];
    if (!(f & F_SOLID)) {
        const T pc = p[c];
        ux -= one_sided_grad<T>(f & F_XP, f & F_XM, p[c + 1], pc, p[c - 1], h, two_h);
        uy -= one_sided_grad<T>(f & F_YP, f & F_YM, p[c + g.sy], pc, p[c - g.sy], h, two_h);
        uz -= one_sided_grad<T>(f & F_ZP, f & F_ZM, p[c + g.sz], pc, p[c - g.sz], h, two_h);
    }
    const bool kill = (f & (F_SOLID | F_NEAR)) != 0;
    vx[c] = kill ? (T)0 : ux;
    vy[c] = kill ? (T)0 : uy;
    vz[c] = kill ? (T)0 : uz;
    write_face_ghosts(g, sc, vx, c, x, y, z, ux, 1);
    write_face_ghosts(g, sc, vy, c, x, y, z, uy, 2);
    write_face_ghosts(g, sc, vz, c, x, y, z, uz, 3);
}

template <class T>
void launch_gradient(hipStream_t st, const SweepTune& tune, const GridDesc& g, const SlabCtx& sc, const T* p, T* vx, T* vy,
                     T* vz, const uint8_t* flags, T h, T two_h)
{
    if (tune.project_cell) {
        hipLaunchKernelGGL((gradient_kernel<T>), cell_grid(g), cell_block(), 0, st, g, sc, p, vx, vy, vz, flags, h, two_h);
        return;
    }
    constexpr int RY = 2;
    const MarchLaunch m = march_launch(g, RY);
    hipLaunchKernelGGL((gradient_march_kernel<T, RY>), dim3(m.nblk), dim3(256), 0, st, g, sc, p, vx, vy, vz, flags, h, two_h,
                       m.zc_len, m.nxw, m.nybg, m.nblk);
}
template void launch_gradient<float>(hipStream_t, const SweepTune&, const GridDesc&, const SlabCtx&, const float*, float*,
                                     float*, float*, const uint8_t*, float, float);
template void launch_gradient<double>(hipStream_t, const SweepTune&, const GridDesc&, const SlabCtx&, const double*,
                                      double*, double*, double*, const uint8_t*, double, double);

}  // namespace fs
