// kernels_dev.h -- device-side helpers shared by the kernel translation units.  Internal to libfluidsim.so.
//
// Which file holds which kernels of the step:
//   kernels.hip      the solver passes outside sweep_fused.hip: single-sweep and pair Jacobi, Gauss-Seidel
//   sweep_fused.hip  the fused two- and three-sweep Jacobi kernel (compiled in slices, see the Makefile)
//   project.hip      divergence and gradient, z-marching and per-cell
//   advect.hip       the advection forms, the clamp tables, gradient + velocity advection
//   fields.hip       stand-alone setBounds, flag / kill / clean tables, inlet, pack / unpack, copy, stats, point
// Here: what more than one of them (and heat.hip, confine.hip, multigrid.hip, vortex.hip) needs -- the cell index, the ghost
// writes of the per-cell kernels, the row store with setBounds fused in (store_row_bounds), the one-sided pressure gradient,
// the peer-push store, the XCD remap, the z-march tile and the launch grids.
#pragma once
#include <hip/hip_runtime.h>
#include "kernels.h"

namespace fs {

template <class T>
struct alignas(16) V4 {
    T e[4];
};

__device__ __forceinline__ long cell(const GridDesc& g, int x, int y, int z)
{
    return (long)x + (long)y * g.sy + (long)z * g.sz;
}

// Ghost-face writes shared by the per-cell kernels: `u` is the un-zeroed new value of
// interior cell (x,y,z) of a field with boundary code b (simulation.cpp:187-215).
template <class T>
__device__ __forceinline__ void write_face_ghosts(const GridDesc& g, const SlabCtx& sc, T* q, long c, int x, int y,
                                                  int z, T u, int b)
{
    if (x == 1) q[c - 1] = (b == 1) ? -u : u;
    if (x == g.W) q[c + 1] = u;
    if (y == 1) q[c - g.sy] = (b == 2) ? -u : u;
    if (y == g.H) q[c + g.sy] = (b == 2) ? -u : u;
    if (z == 1 && sc.lo_wall) q[c - g.sz] = (b == 3) ? -u : u;
    if (z == g.D && sc.hi_wall) q[c + g.sz] = (b == 3) ? -u : u;
}

// Store the lane's four cells of an interior row of a field with boundary code b, the way
// setBounds leaves them (simulation.cpp:183-246): `u` un-zeroed values, `killmask` bit e set =>
// cell e is zeroed; ghost faces determined by this row are written from the un-zeroed values.
// The projection, advection and heat passes call it.  The Jacobi kernels keep their own stores, which carry the peer push and
// the nontemporal variants; confine_kernel and mg_prolong0_kernel restate it, because the call made them longer.
template <class T>
__device__ __forceinline__ void store_row_bounds(const GridDesc& g, const SlabCtx& sc, T* dst, long base, int x0, int y, int z,
                                                 const T (&u)[4], unsigned killmask, int b)
{
    const T zero = (T)0;
    V4<T> st;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const int x = x0 + e;
        T ghost_src = (e > 0) ? u[e - 1] : zero;
        st.e[e] = (x <= g.W) ? (((killmask >> e) & 1u) ? zero : u[e]) : ((x == g.W + 1) ? ghost_src : zero);
    }
    *reinterpret_cast<V4<T>*>(dst + base) = st;
    if (x0 == 1) dst[base - 1] = (b == 1) ? -u[0] : u[0];
    if (x0 + 3 == g.W) dst[base + 4] = u[3];
    const bool zlo = (z == 1) && sc.lo_wall, zhi = (z == g.D) && sc.hi_wall;
    if (y == 1 || y == g.H || zlo || zhi) {
        V4<T> gy, gz;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const bool in = (x0 + e <= g.W);
            gy.e[e] = in ? ((b == 2) ? -u[e] : u[e]) : zero;
            gz.e[e] = in ? ((b == 3) ? -u[e] : u[e]) : zero;
        }
        if (y == 1) *reinterpret_cast<V4<T>*>(dst + base - g.sy) = gy;
        if (y == g.H) *reinterpret_cast<V4<T>*>(dst + base + g.sy) = gy;
        if (zlo) *reinterpret_cast<V4<T>*>(dst + base - g.sz) = gz;
        if (zhi) *reinterpret_cast<V4<T>*>(dst + base + g.sz) = gz;
    }
}

// d p / d x at a fluid cell from the neighbours that are fluid (fp, fm): centred, one-sided or none (simulation.cpp:326-334)
template <class T>
__device__ __forceinline__ T one_sided_grad(bool fp, bool fm, T pp, T pc, T pm, T h, T two_h)
{
    if (fp && fm) return (pp - pm) / two_h;              // :329-330
    if (fp) return (pp - pc) / h;                        // :331-332
    if (fm) return (pc - pm) / h;                        // :333-334
    return (T)0;
}

// launch grids: a thread per cell in blocks of 64 x 4 (a wave is one row), and a lane per four cells of a row
inline dim3 cell_grid(const GridDesc& g) { return dim3((g.W + 63) / 64, (g.H + 3) / 4, g.D); }
inline dim3 cell_block() { return dim3(64, 4, 1); }
inline dim3 row_grid(const GridDesc& g) { return dim3((g.W + 255) / 256, (g.H + 3) / 4, g.D); }

// A store of a solver pass, and (PUSH) its copies into the neighbours' halo planes: dl / dh = PeerPush::lo / hi where the
// plane being written is one the lower / upper neighbour needs, else 0 (wave-uniform).
template <bool PUSH, class V>
__device__ __forceinline__ void put(V* p, const V& v, long dl, long dh)
{
    *p = v;
    if constexpr (PUSH) {
        if (dl) *reinterpret_cast<V*>(reinterpret_cast<char*>(p) + dl) = v;
        if (dh) *reinterpret_cast<V*>(reinterpret_cast<char*>(p) + dh) = v;
    }
}

// Blocks are dealt round-robin over the 8 XCDs (block b lands on XCD b % 8, each with its
// own 4 MiB L2).  Remap so that every XCD owns one contiguous range of work items and
// y-adjacent tiles, which share halo rows, hit the same L2.  Affects speed only.
__device__ __forceinline__ int xcd_contiguous(int b, int nblk)
{
    int q = nblk >> 3, r = nblk & 7, k = b & 7;
    return k * q + (k < r ? k : r) + (b >> 3);
}

// The tile of a z-marching kernel (the two projection passes in project.hip, the vortex fields in vortex.hip): a wave owns
// 256 x-consecutive cells x RY rows, a lane four x-consecutive cells of each (one 16-byte access per row), and walks planes
// zbeg..zend; workgroup = four waves = 4 * RY rows.
template <class T>
struct MarchTile {
    int lane, x0, y0, zbeg, zend;
    bool lane_on, full_group, edge_l, edge_r, live;
    long row0;
};
template <class T, int RY>
__device__ __forceinline__ MarchTile<T> march_tile(const GridDesc& g, int zc_len, int nxw, int nybg, int nblk)
{
    MarchTile<T> t;
    const int v = xcd_contiguous(blockIdx.x, nblk);
    const int xw = v % nxw, ybg = (v / nxw) % nybg, zc = v / (nxw * nybg);
    t.lane = threadIdx.x & 63;
    t.y0 = 1 + (ybg * 4 + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6)) * RY;   // wave-uniform row: scalar tests and row pointers
    t.x0 = 1 + xw * 256 + t.lane * 4;
    t.lane_on = t.x0 <= g.W;
    t.zbeg = 1 + zc * zc_len;
    t.zend = min(g.D, t.zbeg + zc_len - 1);
    t.full_group = (t.x0 + 3 <= g.W);
    t.edge_l = t.lane_on && (t.lane == 0);
    t.edge_r = t.lane_on && t.full_group && ((t.lane == 63) || (t.x0 + 4 > g.W));
    t.live = (t.y0 <= g.H) && (t.zbeg <= t.zend);
    t.row0 = cell(g, t.x0, t.y0, 0);
    return t;
}
template <class T>
__device__ __forceinline__ void ld_row(const T* ptr, bool on, T (&out)[4])
{
    V4<T> q = {{(T)0, (T)0, (T)0, (T)0}};
    if (on) q = *reinterpret_cast<const V4<T>*>(ptr);
#pragma unroll
    for (int e = 0; e < 4; ++e) out[e] = q.e[e];
}

// the launch shape of those kernels: about 2048 workgroups, z chunks of at least 8 planes
struct MarchLaunch {
    int zc_len, nxw, nybg, nblk;
};
inline MarchLaunch march_launch(const GridDesc& g, int RY)
{
    MarchLaunch m;
    m.nxw = (g.W + 255) / 256;
    const int nyb = (g.H + RY - 1) / RY;
    m.nybg = (nyb + 3) / 4;
    const long per_layer = (long)m.nxw * m.nybg;
    long want = (2048 + per_layer - 1) / per_layer;
    if (want < 1) want = 1;
    m.zc_len = (int)((g.D + want - 1) / want);
    if (m.zc_len < 8) m.zc_len = g.D < 8 ? g.D : 8;
    const int nzc = (g.D + m.zc_len - 1) / m.zc_len;
    m.nblk = (int)(per_layer * nzc);
    return m;
}

}  // namespace fs
