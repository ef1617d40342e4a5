// kernels.hip -- hand-written gfx950 (CDNA4) kernels of the wind-tunnel step: the solver passes that are not in
// sweep_fused.hip (single-sweep and pair Jacobi, Gauss-Seidel).  The projection passes are in project.hip, advection in
// advect.hip, setBounds and the small whole-field passes in fields.hip; kernels_dev.h lists them.
//
// Everything here is HBM-bound stencil / gather work (0.67 flop per byte for the sweep), so
// there is no MFMA anywhere: the design points are 16-byte-per-lane coalesced streams,
// register/LDS reuse of the six stencil neighbours, wave shuffles for the x neighbours,
// XCD-aware block order, and boundary handling fused into the producing kernel.
//
// Arithmetic follows the reference expression by expression (cited per kernel) and the
// file is compiled with -ffp-contract=off, so fp32 results are bit-identical with the
// reference's `c++ -O2` build for the same iteration order.
#include <hip/hip_runtime.h>
#include "kernels.h"
#include "kernels_dev.h"
#include <type_traits>

namespace fs {

// =====================================================================================
// Jacobi sweep with fused setBounds.
//   linearSolver  simulation.cpp:251-273 (one iteration of the k loop, neighbours read
//                 from the previous iterate `src`), followed by
//   setBounds     simulation.cpp:183-246 applied to the new iterate `dst`.
//
// Work decomposition: a wave owns 256 x-consecutive cells (4 per lane, one dwordx4) by RY
// rows and marches along z keeping planes z-1, z, z+1 of its patch in registers, so each
// value of `src` is fetched from memory once per sweep (plus halo rows/columns, which are
// L1/L2 hits).  x neighbours cross lanes with a wave shuffle; only the wave's edge lanes
// touch memory for them.  A block is four waves stacked in y.
// =====================================================================================
// Everything a wave needs of one z plane when that plane is the stencil centre: its own
// RY x 4 patch, the rows above and below the patch, and the two columns beside it.
template <class T, int RY>
struct PlaneIn {
    T core[RY][4];
    T hb[4], ht[4];      // rows y0-1 and y0+RY
    T eL[RY], eR[RY];    // columns x0-1 and x0+4 (only the wave's edge lanes load them)
};
template <class T, int RY>
struct AuxIn {
    T rhs[RY][4];
    unsigned fl[RY];     // kill byte of the lane's four cells: bits 0-3 solid, bits 4-7 solid-or-near
};

template <class T, int RY, int ABL, bool PUSH>
__global__ __launch_bounds__(256) void jacobi_sweep_kernel(GridDesc g, SlabCtx sc, const T* __restrict__ src,
                                                            const T* __restrict__ rhs, T* __restrict__ dst,
                                                            const uint8_t* __restrict__ flags, int b, T a, T inv_c,
                                                            int z_first, int z_last, int zc_len, int z_stride, int nxw,
                                                            int nybg, int nblk, PeerPush pp)
{
    const int v = xcd_contiguous(blockIdx.x, nblk);
    const int xw = v % nxw;
    const int ybg = (v / nxw) % nybg;
    const int zc = v / (nxw * nybg);

    const int lane = threadIdx.x & 63, wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);   // uniform, and the compiler may know
    const int W = g.W, H = g.H, D = g.D;
    const int y0 = 1 + (ybg * 4 + wv) * RY;
    if (y0 > H) return;                                  // wave-uniform
    const int x0 = 1 + xw * 256 + lane * 4;
    const bool lane_on = x0 <= W;
    const int zbeg = z_first + zc * z_stride;            // z_stride == zc_len except for the two-range launch
    const int zend = min(z_last, zbeg + zc_len - 1);
    if (zbeg > zend) return;

    const bool full_group = (x0 + 3 <= W);
    const bool edge_l = lane_on && (lane == 0);                                   // x0-1 comes from memory
    const bool edge_r = lane_on && full_group && ((lane == 63) || (x0 + 4 > W));  // x0+4 comes from memory
    const int kill_shift = (b == 0) ? 0 : 4;             // which nibble of the kill byte applies (simulation.cpp:222 vs :240)
    const T zero = (T)0;
    const long row0 = cell(g, x0, y0, 0);                // lane's first cell in plane 0

    auto ld4 = [&](const T* ptr, bool on, T (&out)[4]) {
        V4<T> q = {{zero, zero, zero, zero}};
        if (on) q = *reinterpret_cast<const V4<T>*>(ptr);
#pragma unroll
        for (int e = 0; e < 4; ++e) out[e] = q.e[e];
    };
    // rows up to the ghost row H+1 are fetched: in a partial band it is some row's y+1 neighbour
    auto fetch_core = [&](int z, T (&out)[RY][4]) {
        const T* pz = src + row0 + (long)z * g.sz;
#pragma unroll
        for (int r = 0; r < RY; ++r) ld4(pz + r * g.sy, lane_on && (y0 + r <= H + 1), out[r]);
    };
    auto fetch_plane = [&](int z, PlaneIn<T, RY>& P, bool as_centre) {
        fetch_core(z, P.core);
        const T* pz = src + row0 + (long)z * g.sz;
        const bool halo = as_centre && !(ABL & 2);
        ld4(pz - g.sy, lane_on && halo, P.hb);
        ld4(pz + RY * g.sy, lane_on && halo && (y0 + RY <= H + 1), P.ht);
#pragma unroll
        for (int r = 0; r < RY; ++r) {
            const bool row_on = as_centre && (y0 + r <= H);
            P.eL[r] = (edge_l && row_on) ? pz[r * g.sy - 1] : zero;
            P.eR[r] = (edge_r && row_on) ? pz[r * g.sy + 4] : zero;
        }
    };
    auto fetch_aux = [&](int z, AuxIn<T, RY>& X) {
        const long off = row0 + (long)z * g.sz;
#pragma unroll
        for (int r = 0; r < RY; ++r) {
            const bool on = lane_on && (y0 + r <= H);
            ld4(rhs + off + r * g.sy, on && !(ABL & 4), X.rhs[r]);
            X.fl[r] = (on && !(ABL & 1)) ? (unsigned)flags[(off + r * g.sy + 3) >> 2] : 0u;
        }
    };

    // Software pipeline: while plane z is computed, the loads of plane z+2 (and of the rhs /
    // flags of plane z+1) are in flight, so a wave waits for memory once per plane instead of
    // once per dependent load.
    T m[RY][4];
    PlaneIn<T, RY> A, B, N;
    AuxIn<T, RY> xa, xn;
    fetch_core(zbeg - 1, m);
    fetch_plane(zbeg, A, true);
    fetch_aux(zbeg, xa);
    fetch_plane(zbeg + 1, B, zbeg + 1 <= zend);

    for (int z = zbeg; z <= zend; ++z) {
        if (z + 1 <= zend) {                              // wave-uniform
            fetch_plane(z + 2, N, z + 2 <= zend);
            fetch_aux(z + 1, xn);
        }

#pragma unroll
        for (int r = 0; r < RY; ++r) {
            const int y = y0 + r;
            // x neighbours across lanes (all lanes execute the shuffles)
            T left = __shfl_up(A.core[r][3], 1);
            T right = __shfl_down(A.core[r][0], 1);
            if (edge_l) left = A.eL[r];
            if (edge_r) right = A.eR[r];
            if (y <= H && lane_on) {                      // y <= H is wave-uniform
                const long base = row0 + (long)z * g.sz + r * g.sy;
                const unsigned fl = xa.fl[r];
                T u[4];
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    T xp1 = (e < 3) ? A.core[r][e + 1] : right;
                    T xm1 = (e > 0) ? A.core[r][e - 1] : left;
                    T yp1 = (r < RY - 1) ? A.core[r + 1][e] : A.ht[e];
                    T ym1 = (r > 0) ? A.core[r - 1][e] : A.hb[e];
                    // simulation.cpp:264-269: order x+1, x-1, y+1, y-1, z+1, z-1
                    T nb = xp1 + xm1 + yp1 + ym1 + B.core[r][e] + m[r][e];
                    u[e] = (xa.rhs[r][e] + a * nb) * inv_c;
                }

                // ---- fused setBounds on the new iterate (faces read un-zeroed values) ----
                V4<T> st;
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const int x = x0 + e;
                    const bool kill = ((fl >> (e + kill_shift)) & 1u) != 0;
                    T ghost_src = (e > 0) ? u[e - 1] : zero;
                    // cells past W: the outflow ghost copies u(W) (:191); row padding stays 0
                    st.e[e] = (x <= W) ? (kill ? zero : u[e]) : ((x == W + 1) ? ghost_src : zero);
                }
                const long dl = (PUSH && z <= pp.planes) ? pp.lo : 0, dh = (PUSH && z > D - pp.planes) ? pp.hi : 0;   // wave-uniform
                if (!(ABL & 8) || st.e[0] == (T)123456789) put<PUSH>(reinterpret_cast<V4<T>*>(dst + base), st, dl, dh);
                if (x0 == 1) put<PUSH>(dst + base - 1, (b == 1) ? -u[0] : u[0], dl, dh);        // :189-190
                if (full_group && x0 + 3 == W) put<PUSH>(dst + base + 4, u[3], dl, dh);         // :191
                const bool yface = (y == 1) || (y == H);                                        // wave-uniform
                const bool zface = (z == 1 && sc.lo_wall) || (z == D && sc.hi_wall);            // wave-uniform
                if (yface || zface) {
                    V4<T> gy, gz;
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        const bool in = (x0 + e <= W);
                        gy.e[e] = in ? ((b == 2) ? -u[e] : u[e]) : zero;                        // :198-201
                        gz.e[e] = in ? ((b == 3) ? -u[e] : u[e]) : zero;                        // :208-214
                    }
                    if (y == 1) put<PUSH>(reinterpret_cast<V4<T>*>(dst + base - g.sy), gy, dl, dh);
                    if (y == H) put<PUSH>(reinterpret_cast<V4<T>*>(dst + base + g.sy), gy, dl, dh);
                    if (z == 1 && sc.lo_wall) *reinterpret_cast<V4<T>*>(dst + base - g.sz) = gz;
                    if (z == D && sc.hi_wall) *reinterpret_cast<V4<T>*>(dst + base + g.sz) = gz;
                }
            }
        }

#pragma unroll
        for (int r = 0; r < RY; ++r)
#pragma unroll
            for (int e = 0; e < 4; ++e) m[r][e] = A.core[r][e];
        A = B;
        B = N;
        xa = xn;
    }
}

template <class T, int RY, int ABL>
static void launch_jacobi_v(hipStream_t st, const SweepTune& tune, const GridDesc& g, const SlabCtx& sc, const T* src,
                            const T* rhs, T* dst, const uint8_t* flags, int b, T a, T inv_c, int z_first, int z_last,
                            int second_first, const PeerPush* push)
{
    const int nxw = (g.W + 255) / 256;
    const int nyb = (g.H + RY - 1) / RY;
    const int nybg = (nyb + 3) / 4;
    const int planes = z_last - z_first + 1;
    const long per_layer = (long)nxw * nybg;
    if (second_first >= 0) {
        // two equally long ranges (the slab's two boundary regions) as two chunks of one launch
        const int last2 = second_first + planes - 1;
        hipLaunchKernelGGL((jacobi_sweep_kernel<T, RY, ABL, false>), dim3((unsigned)(per_layer * 2)), dim3(256), 0, st, g, sc, src,
                           rhs, dst, flags, b, a, inv_c, z_first, last2, planes, second_first - z_first, nxw, nybg,
                           (int)(per_layer * 2), PeerPush());
        return;
    }
    // enough z chunks for ~target_blocks blocks, but chunks of at least 8 planes (each chunk
    // re-reads 2 warm-up planes)
    long want = (tune.target_blocks + per_layer - 1) / per_layer;
    if (want < 1) want = 1;
    int zc_len = (int)((planes + want - 1) / want);
    if (zc_len < 8) zc_len = planes < 8 ? planes : 8;
    if (tune.zc_len > 0) zc_len = tune.zc_len < planes ? tune.zc_len : planes;
    const int nzc = (planes + zc_len - 1) / zc_len;
    const int nblk = (int)(per_layer * nzc);
    if (ABL == 0 && push && (push->lo || push->hi))
        hipLaunchKernelGGL((jacobi_sweep_kernel<T, RY, 0, true>), dim3(nblk), dim3(256), 0, st, g, sc, src, rhs, dst, flags, b,
                           a, inv_c, z_first, z_last, zc_len, zc_len, nxw, nybg, nblk, *push);
    else
        hipLaunchKernelGGL((jacobi_sweep_kernel<T, RY, ABL, false>), dim3(nblk), dim3(256), 0, st, g, sc, src, rhs, dst, flags, b,
                           a, inv_c, z_first, z_last, zc_len, zc_len, nxw, nybg, nblk, PeerPush());
}

template <class T>
void launch_jacobi(hipStream_t st, const SweepTune& tune, const GridDesc& g, const SlabCtx& sc, const T* src, const T* rhs,
                   T* dst, const uint8_t* flags, int b, T a, T inv_c, int z_first, int z_last, int second_first, const PeerPush* push)
{
    if (z_last < z_first) return;
#define FS_GO(RY, ABL) launch_jacobi_v<T, RY, ABL>(st, tune, g, sc, src, rhs, dst, flags, b, a, inv_c, z_first, z_last, second_first, push)
    if (tune.abl == 0) {
        if (tune.ry == 4) FS_GO(4, 0);
        else FS_GO(2, 0);
    } else {   // timing-only ablations (wrong results by design), RY = 4
        switch (tune.abl) {
            case 1: FS_GO(4, 1); break;
            case 2: FS_GO(4, 2); break;
            case 4: FS_GO(4, 4); break;
            case 8: FS_GO(4, 8); break;
            case 3: FS_GO(4, 3); break;
            default: FS_GO(4, 0); break;
        }
    }
#undef FS_GO
}
template void launch_jacobi<float>(hipStream_t, const SweepTune&, const GridDesc&, const SlabCtx&, const float*, const float*,
                                   float*, const uint8_t*, int, float, float, int, int, int, const PeerPush*);
template void launch_jacobi<double>(hipStream_t, const SweepTune&, const GridDesc&, const SlabCtx&, const double*,
                                    const double*, double*, const uint8_t*, int, double, double, int, int, int, const PeerPush*);

// =====================================================================================
// Two Jacobi sweeps per pass over memory (temporal blocking), bit-identical with two
// launches of jacobi_sweep_kernel.
//
// One sweep moves 12 B per cell for 8 flops; the only way past the HBM roof is to apply
// several sweeps while the data is on chip.  Level 0 = `src`, level 1 = the iterate after
// one sweep + setBounds (never written to memory), level 2 = `dst`.
//
// A workgroup owns the full row width (NXW waves of 256 cells) times a band of BY = NYW*2
// rows and marches along z.  Per plane zl it (1) computes level 1 of plane zl for its band
// from level-0 planes zl-1..zl+1 held in registers, exactly as the single sweep does,
// including the zeroing of solids and the ghost faces of setBounds; (2) publishes that
// level-1 plane tile (interior rows + the ghost rows/columns setBounds would have written)
// in LDS; (3) after one barrier computes level 2 of plane zl-1 from level-1 planes
// zl-2, zl-1, zl of its own cells (registers) and the in-plane neighbours out of the LDS
// tile, and stores it with the fused setBounds.  Three LDS plane buffers rotate, so one
// barrier per plane suffices.  Bands overlap by two rows and z chunks by two planes: the
// first and last level-1 row of a band have no level-2 output there (their level-1
// neighbour row belongs to the next band); rows next to the walls use the ghost rows.
// =====================================================================================
// MODE: 0 = two Jacobi sweeps; 1 = one red-black iteration (solver=rbsor; coarse-level-style smoothing); 2 = two damped
// Jacobi sweeps, q + omega*(r - q) in every cell (the level-0 smoother of solver=mg)
template <class T, int NXW, int NYW, int MODE, bool PUSH>
__global__ __launch_bounds__(NXW* NYW * 64) void jacobi_pair_kernel(GridDesc g, SlabCtx sc, const T* __restrict__ src,
                                                                     const T* __restrict__ rhs, T* __restrict__ dst,
                                                                     const uint8_t* __restrict__ flags, int b, T a,
                                                                     T inv_c, int z_first, int z_last, int zc_len,
                                                                     int z_stride, int nbands, int nblk, T omega, PeerPush pp)
{
    constexpr int RY = 2, BY = NYW * RY, TW = NXW * 256 + 8;
    // ring of four level-1 plane tiles (plane z lives in slot z & 3); column index = x + 3
    __shared__ T tile[4][BY][TW];

    const int v = xcd_contiguous(blockIdx.x, nblk);
    const int band = v % nbands, zc = v / nbands;
    // readfirstlane: the wave index is the same in all 64 lanes, but only this tells the compiler so -- rows,
    // row pointers and every row test then live in scalar registers and branch as scalars
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
    const int wx = wave % NXW, wy = wave / NXW;
    const int W = g.W, H = g.H, D = g.D;
    const int s = band * (BY - 2);                       // tile row t <-> grid row s + t
    const int ty0 = wy * RY, y0 = s + ty0;
    const int x0 = 1 + wx * 256 + lane * 4;
    const bool lane_on = x0 <= W;
    const int zbeg = z_first + zc * z_stride, zend = min(z_last, zbeg + zc_len - 1);  // level-2 output planes
    if (zbeg > zend) return;                             // block-uniform
    // level-1 planes: one beyond the output chunk on each side; beyond a physical wall there is
    // no such plane (its level-1 ghost is derived below), beyond a slab boundary it is the
    // neighbour's plane, recomputed here from the two-deep halo
    const int zl_first = max(sc.lo_wall ? 1 : 0, zbeg - 1), zl_last = min(sc.hi_wall ? D : D + 1, zend + 1);
    const int out_lo = max(1, s + 1), out_hi = min(H, s + BY - 2);        // level-2 output rows

    const bool full_group = (x0 + 3 <= W);
    const bool edge_l = lane_on && (lane == 0);
    const bool edge_r = lane_on && full_group && ((lane == 63) || (x0 + 4 > W));
    const int kill_shift = (b == 0) ? 0 : 4;
    const T zero = (T)0;
    const long row0 = cell(g, x0, y0, 0);

    auto ld4 = [&](const T* ptr, bool on, T (&out)[4]) {
        V4<T> q = {{zero, zero, zero, zero}};
        if (on) q = *reinterpret_cast<const V4<T>*>(ptr);
#pragma unroll
        for (int e = 0; e < 4; ++e) out[e] = q.e[e];
    };
    auto row_in_mem = [&](int y) { return y >= 0 && y <= H + 1; };
    auto fetch_core = [&](int z, T (&out)[RY][4]) {
        const T* pz = src + row0 + (long)z * g.sz;
#pragma unroll
        for (int r = 0; r < RY; ++r) ld4(pz + r * g.sy, lane_on && row_in_mem(y0 + r), out[r]);
    };
    // the rows above/below the patch and the columns beside it are only needed of the plane that is
    // the stencil centre: they are fetched one plane behind the cores (P.core is not used here)
    auto fetch_side = [&](int z, PlaneIn<T, RY>& P) {
        const T* pz = src + row0 + (long)z * g.sz;
        ld4(pz - g.sy, lane_on && row_in_mem(y0 - 1), P.hb);
        ld4(pz + RY * g.sy, lane_on && row_in_mem(y0 + RY), P.ht);
#pragma unroll
        for (int r = 0; r < RY; ++r) {
            const bool row_on = (y0 + r >= 1) && (y0 + r <= H);
            P.eL[r] = (edge_l && row_on) ? pz[r * g.sy - 1] : zero;
            P.eR[r] = (edge_r && row_on) ? pz[r * g.sy + 4] : zero;
        }
    };
    auto fetch_aux = [&](int z, AuxIn<T, RY>& X) {
        const long off = row0 + (long)z * g.sz;
#pragma unroll
        for (int r = 0; r < RY; ++r) {
            const bool on = lane_on && (y0 + r >= 1) && (y0 + r <= H);
            ld4(rhs + off + r * g.sy, on, X.rhs[r]);
            X.fl[r] = on ? (unsigned)flags[(off + r * g.sy + 3) >> 2] : 0u;
        }
    };

    // one stencil application; simulation.cpp:264-269 order x+1, x-1, y+1, y-1, z+1, z-1
    auto relax4 = [&](const T (&cc)[4], T left, T right, const T (&ym)[4], const T (&yp)[4], const T (&zm)[4],
                      const T (&zp)[4], const T (&rh)[4], T (&u)[4]) {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            T xp1 = (e < 3) ? cc[e + 1] : right;
            T xm1 = (e > 0) ? cc[e - 1] : left;
            T nb = xp1 + xm1 + yp[e] + ym[e] + zp[e] + zm[e];
            u[e] = (rh[e] + a * nb) * inv_c;
        }
    };
    // what setBounds leaves in memory for the lane's four cells of an interior row
    auto settle4 = [&](const T (&u)[4], unsigned fl, T (&st)[4]) {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int x = x0 + e;
            const bool kill = ((fl >> (e + kill_shift)) & 1u) != 0;
            T ghost_src = (e > 0) ? u[e - 1] : zero;
            st[e] = (x <= W) ? (kill ? zero : u[e]) : ((x == W + 1) ? ghost_src : zero);
        }
    };
    auto face4 = [&](const T (&u)[4], bool negate, T (&out)[4]) {
#pragma unroll
        for (int e = 0; e < 4; ++e) out[e] = (x0 + e <= W) ? (negate ? -u[e] : u[e]) : zero;
    };
    // RB (solver=rbsor, not in the reference): the two levels of a pass are the two colours of one
    // red-black SOR iteration -- level 1 moves the cells with even x+y+z (global z), level 2 the odd
    // ones, each from its value q towards the Jacobi update r by q + omega*(r - q); the other colour
    // keeps its value.  setBounds between the halves is what the levels do anyway.
    auto blend4 = [&](T (&u)[4], const T (&old)[4], int y, int z, int colour) {
        const int par = (x0 + y + z + sc.zoff + colour) & 1;          // parity of cell e = 0 relative to the colour
#pragma unroll
        for (int e = 0; e < 4; ++e) u[e] = (((par + e) & 1) == 0) ? old[e] + omega * (u[e] - old[e]) : old[e];
    };
    auto damp4 = [&](T (&u)[4], const T (&old)[4]) {
#pragma unroll
        for (int e = 0; e < 4; ++e) u[e] = old[e] + omega * (u[e] - old[e]);
    };
    auto lds_row = [&](int z, int t, T (&out)[4]) {
        V4<T> q = *reinterpret_cast<const V4<T>*>(&tile[z & 3][t][x0 + 3]);
#pragma unroll
        for (int e = 0; e < 4; ++e) out[e] = q.e[e];
    };
    auto lds_put = [&](int z, int t, const T (&in)[4]) {
        V4<T> q;
#pragma unroll
        for (int e = 0; e < 4; ++e) q.e[e] = in[e];
        *reinterpret_cast<V4<T>*>(&tile[z & 3][t][x0 + 3]) = q;
    };

    // level 2 of plane zo: every level-1 operand comes out of the LDS ring (planes zo-1, zo,
    // zo+1), x neighbours of the lane's own group by wave shuffle
    auto level2 = [&](int zo, const AuxIn<T, RY>& X) {
#pragma unroll
        for (int r = 0; r < RY; ++r) {
            const int y = y0 + r, t = ty0 + r;
            const bool row_out = (y >= out_lo) && (y <= out_hi);     // wave-uniform
            T cc[4] = {zero, zero, zero, zero};
            if (row_out && lane_on) lds_row(zo, t, cc);
            T left = __shfl_up(cc[3], 1);
            T right = __shfl_down(cc[0], 1);
            if (!(row_out && lane_on)) continue;
            if (edge_l) left = tile[zo & 3][t][x0 + 2];
            if (edge_r) right = tile[zo & 3][t][x0 + 7];
            T ym[4], yp[4], zm[4], zp[4];
            lds_row(zo, t - 1, ym);
            lds_row(zo, t + 1, yp);
            lds_row(zo - 1, t, zm);
            lds_row(zo + 1, t, zp);
            T u[4], st[4];
            relax4(cc, left, right, ym, yp, zm, zp, X.rhs[r], u);
            if (MODE == 1) blend4(u, cc, y, zo, 1);
            if (MODE == 2) damp4(u, cc);
            settle4(u, X.fl[r], st);
            const long base = row0 + (long)zo * g.sz + r * g.sy;
            V4<T> q;
#pragma unroll
            for (int e = 0; e < 4; ++e) q.e[e] = st[e];
            const long dl = (PUSH && zo <= pp.planes) ? pp.lo : 0, dh = (PUSH && zo > D - pp.planes) ? pp.hi : 0;   // wave-uniform
            put<PUSH>(reinterpret_cast<V4<T>*>(dst + base), q, dl, dh);
            if (x0 == 1) put<PUSH>(dst + base - 1, (b == 1) ? -u[0] : u[0], dl, dh);            // :189-190
            if (full_group && x0 + 3 == W) put<PUSH>(dst + base + 4, u[3], dl, dh);             // :191
            const bool zlo_face = (zo == 1) && sc.lo_wall, zhi_face = (zo == D) && sc.hi_wall;
            if (y == 1 || y == H || zlo_face || zhi_face) {
                T f[4];
                V4<T> qq;
                face4(u, b == 2, f);
#pragma unroll
                for (int e = 0; e < 4; ++e) qq.e[e] = f[e];
                if (y == 1) put<PUSH>(reinterpret_cast<V4<T>*>(dst + base - g.sy), qq, dl, dh);  // :198-201
                if (y == H) put<PUSH>(reinterpret_cast<V4<T>*>(dst + base + g.sy), qq, dl, dh);
                face4(u, b == 3, f);
#pragma unroll
                for (int e = 0; e < 4; ++e) qq.e[e] = f[e];
                if (zlo_face) *reinterpret_cast<V4<T>*>(dst + base - g.sz) = qq;                // :208-214
                if (zhi_face) *reinterpret_cast<V4<T>*>(dst + base + g.sz) = qq;
            }
        }
    };

    // level-0 stream, software-pipelined one plane ahead of its use (see jacobi_sweep_kernel)
    T m[RY][4], Bc[RY][4], Nc[RY][4];
    PlaneIn<T, RY> A, SN;                                // A: centre plane (core + sides); SN: sides of the next centre
    AuxIn<T, RY> xc, xn, xm;
    fetch_core(zl_first - 1, m);
    fetch_core(zl_first, A.core);
    fetch_side(zl_first, A);
    fetch_aux(zl_first, xc);
    fetch_core(zl_first + 1, Bc);
    xm = xc;

    for (int zl = zl_first; zl <= zl_last; ++zl) {
        if (zl + 1 <= zl_last) {                         // block-uniform
            fetch_core(zl + 2, Nc);                      // zl+2 <= D+1
            fetch_side(zl + 1, SN);
            fetch_aux(zl + 1, xn);
        }

        // ---- level 1 of plane zl for this wave's rows, published with its setBounds ghosts
        T gz[RY][4];
#pragma unroll
        for (int r = 0; r < RY; ++r) {
            const int y = y0 + r, t = ty0 + r;
            T left = __shfl_up(A.core[r][3], 1);
            T right = __shfl_down(A.core[r][0], 1);
            if (edge_l) left = A.eL[r];
            if (edge_r) right = A.eR[r];
            T u[4] = {zero, zero, zero, zero};
            const bool row_on = (y >= 1) && (y <= H);    // wave-uniform
            if (row_on && lane_on) {
                T ym[4], yp[4], st[4];
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    ym[e] = (r > 0) ? A.core[r > 0 ? r - 1 : 0][e] : A.hb[e];
                    yp[e] = (r < RY - 1) ? A.core[r < RY - 1 ? r + 1 : r][e] : A.ht[e];
                }
                relax4(A.core[r], left, right, ym, yp, m[r], Bc[r], xc.rhs[r], u);
                if (MODE == 1) blend4(u, A.core[r], y, zl, 0);
                if (MODE == 2) damp4(u, A.core[r]);
                settle4(u, xc.fl[r], st);
                lds_put(zl, t, st);
                if (x0 == 1) tile[zl & 3][t][3] = (b == 1) ? -u[0] : u[0];                      // ghost column x = 0
                if (full_group && x0 + 3 == W) tile[zl & 3][t][W + 4] = u[3];                  // ghost column x = W+1
                T f[4];
                if (y == 1 && t >= 1) { face4(u, b == 2, f); lds_put(zl, t - 1, f); }           // ghost row y = 0
                if (y == H && t + 1 < BY) { face4(u, b == 2, f); lds_put(zl, t + 1, f); }       // ghost row y = H+1
            }
            face4(u, b == 3, gz[r]);
        }
        if (zl == 1 && sc.lo_wall) {                     // level-1 ghost plane z = 0 (:208-210)
#pragma unroll
            for (int r = 0; r < RY; ++r)
                if (lane_on && y0 + r >= 1 && y0 + r <= H) lds_put(0, ty0 + r, gz[r]);
        }
        __syncthreads();

        // ---- level 2 of plane zl-1
        if (zl - 1 >= zbeg) level2(zl - 1, xm);
        if (zl == D && zend == D && sc.hi_wall) {
            // top wall: level-1 ghost plane z = D+1 is +-u1(D) (:212-214).  Its ring slot still
            // holds plane D-3, which slower waves may be reading: fence both sides.
            __syncthreads();
#pragma unroll
            for (int r = 0; r < RY; ++r)
                if (lane_on && y0 + r >= 1 && y0 + r <= H) lds_put(D + 1, ty0 + r, gz[r]);
            __syncthreads();
            level2(D, xc);
        }

#pragma unroll
        for (int r = 0; r < RY; ++r)
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                m[r][e] = A.core[r][e];
                SN.core[r][e] = Bc[r][e];
                Bc[r][e] = Nc[r][e];
            }
        A = SN;
        xm = xc;
        xc = xn;
    }
}

template <class T, int NXW, int NYW>
static void launch_pair_v(hipStream_t st, const SweepTune& tune, const GridDesc& g, const SlabCtx& sc, const T* src,
                          const T* rhs, T* dst, const uint8_t* flags, int b, T a, T inv_c, int z_first, int z_last,
                          const SweepShape& shape, int alt, int second_first, T omega, bool damped, const PeerPush* push)
{
    // omega == 0: two Jacobi sweeps; otherwise one red-black SOR iteration with that relaxation factor, or (damped)
    // two Jacobi sweeps damped by it
    const bool pushing = push && (push->lo || push->hi) && omega == (T)0 && second_first < 0;
    const PeerPush pp = pushing ? *push : PeerPush();
    auto kernel = pushing ? jacobi_pair_kernel<T, NXW, NYW, 0, true>
                  : (omega == (T)0) ? jacobi_pair_kernel<T, NXW, NYW, 0, false>
                  : damped ? jacobi_pair_kernel<T, NXW, NYW, 2, false> : jacobi_pair_kernel<T, NXW, NYW, 1, false>;
    const int planes = z_last - z_first + 1;
    if (planes <= 0) return;
    const int nbands = plan_bands(g.H, shape);
    if (second_first >= 0) {
        // two equally long ranges (the slab's two boundary regions) as two chunks of one launch
        hipLaunchKernelGGL(kernel, dim3(nbands * 2), dim3(NXW * NYW * 64), 0, st, g, sc, src,
                           rhs, dst, flags, b, a, inv_c, z_first, second_first + planes - 1, planes,
                           second_first - z_first, nbands, nbands * 2, omega, pp);
        return;
    }
    // z chunks: each re-reads 4 level-0 planes and recomputes 2 level-1 planes (launch_plan.h: chunk_len)
    const int slots = tune.cu_slots > 0 ? tune.cu_slots : 256;
    int zc_len = chunk_len(planes, nbands, alt, chunk_min_len(SweepKernel::Pair), chunk_overlap(SweepKernel::Pair, 2), slots);
    if (tune.pair_zc > 0) zc_len = tune.pair_zc < planes ? tune.pair_zc : planes;
    const int nzc = (planes + zc_len - 1) / zc_len;
    const int nblk = nbands * nzc;
    hipLaunchKernelGGL(kernel, dim3(nblk), dim3(NXW * NYW * 64), 0, st, g, sc, src, rhs,
                       dst, flags, b, a, inv_c, z_first, z_last, zc_len, zc_len, nbands, nblk, omega, pp);
}

// The builds of jacobi_pair_kernel (launch_plan.h: SHAPE_TABLE says which row widths and shape ids reach them).
using PairBuildsF32 = Builds<Build<2, 1, 12, 2>, Build<2, 1, 8, 2>, Build<2, 1, 10, 2>, Build<2, 1, 16, 2>, Build<2, 2, 6, 2>,
                             Build<2, 2, 4, 2>, Build<2, 2, 5, 2>, Build<2, 2, 8, 2>, Build<2, 3, 4, 2>, Build<2, 4, 3, 2>>;
using PairBuildsF64 = Builds<Build<2, 1, 8, 2>, Build<2, 2, 4, 2>, Build<2, 3, 3, 2>, Build<2, 4, 2, 2>>;
static_assert(PairBuildsF32::covers(4, SweepKernel::Pair) && PairBuildsF64::covers(8, SweepKernel::Pair),
              "a pair-kernel shape of SHAPE_TABLE has no build here");

// plan = two-sweep id of the pair kernel (< 0: plan 0).  All plans give identical results; the host driver times them once
// per grid and keeps the fastest.
template <class T>
void launch_jacobi_pair(hipStream_t st, const SweepTune& tune, const GridDesc& g, const SlabCtx& sc, const T* src, const T* rhs,
                        T* dst, const uint8_t* flags, int b, T a, T inv_c, int z_first, int z_last, int plan, int second_first,
                        T omega, bool damped, const PeerPush* push)
{
    PlanId p = decode_plan(false, plan);
    if (sizeof(T) == 4 && tune.pair_shape > 0) p.shape = tune.pair_shape;   // forced shape: fp32 builds only
    const SweepShape* shape = launch_shape(sizeof(T), SweepKernel::Pair, g.W, p.shape);
    if (!shape) return;                                  // rows above 1024 cells: plan_supported is false
    using List = std::conditional_t<sizeof(T) == 4, PairBuildsF32, PairBuildsF64>;
    List::run(*shape, [&](auto build) {
        using B = decltype(build);
        launch_pair_v<T, B::NXW, B::NYW>(st, tune, g, sc, src, rhs, dst, flags, b, a, inv_c, z_first, z_last, *shape, p.alt,
                                         second_first, omega, damped, push);
    });
}
template void launch_jacobi_pair<float>(hipStream_t, const SweepTune&, const GridDesc&, const SlabCtx&, const float*, const float*,
                                        float*, const uint8_t*, int, float, float, int, int, int, int, float, bool,
                                        const PeerPush*);
template void launch_jacobi_pair<double>(hipStream_t, const SweepTune&, const GridDesc&, const SlabCtx&, const double*,
                                         const double*, double*, const uint8_t*, int, double, double, int, int, int, int, double,
                                         bool, const PeerPush*);

// =====================================================================================
// Reference-order in-place sweep (verification mode, single GPU).
//   linearSolver  simulation.cpp:251-273 at one thread: x outermost, z innermost, in place.
// Cells on a hyperplane x+y+z = s only depend on hyperplanes s-1 (already updated) and s+1
// (not yet updated), exactly like the lexicographic sweep, so walking s upward with a
// barrier between hyperplanes reproduces the reference bit for bit.  One workgroup does
// the whole solve (all `sweeps` iterations and their setBounds) so that a workgroup
// barrier is the only synchronisation needed; this mode is for parity, not speed.
// =====================================================================================
template <class T>
__device__ void bounds_in_block(const GridDesc& g, T* q, const uint8_t* flags, int b)
{
    const int W = g.W, H = g.H, D = g.D;
    const int tid = threadIdx.x, nt = blockDim.x;
    for (int t = tid; t < H * D; t += nt) {
        int y = 1 + t % H, z = 1 + t / H;
        T in = q[cell(g, 1, y, z)];
        q[cell(g, 0, y, z)] = (b == 1) ? -in : in;
        q[cell(g, W + 1, y, z)] = q[cell(g, W, y, z)];
    }
    for (int t = tid; t < W * D; t += nt) {
        int x = 1 + t % W, z = 1 + t / W;
        T lo = q[cell(g, x, 1, z)], hi = q[cell(g, x, H, z)];
        q[cell(g, x, 0, z)] = (b == 2) ? -lo : lo;
        q[cell(g, x, H + 1, z)] = (b == 2) ? -hi : hi;
    }
    for (int t = tid; t < W * H; t += nt) {
        int x = 1 + t % W, y = 1 + t / W;
        T lo = q[cell(g, x, y, 1)], hi = q[cell(g, x, y, D)];
        q[cell(g, x, y, 0)] = (b == 3) ? -lo : lo;
        q[cell(g, x, y, D + 1)] = (b == 3) ? -hi : hi;
    }
    __syncthreads();
    const unsigned zero_bits = (b == 0) ? F_SOLID : (F_SOLID | F_NEAR);
    for (long t = tid; t < (long)W * H * D; t += nt) {
        int x = 1 + (int)(t % W), y = 1 + (int)((t / W) % H), z = 1 + (int)(t / ((long)W * H));
        long c = cell(g, x, y, z);
        if (flags[c] & zero_bits) q[c] = (T)0;
    }
    __syncthreads();
}

template <class T>
__global__ __launch_bounds__(1024) void gs_lex_kernel(GridDesc g, T* q, const T* rhs, const uint8_t* flags, int b, T a,
                                                       T inv_c, int sweeps)
{
    const int W = g.W, H = g.H, D = g.D;
    const int tid = threadIdx.x, nt = blockDim.x;
    for (int it = 0; it < sweeps; ++it) {
        for (int s = 3; s <= W + H + D; ++s) {
            // y in [max(1, s-W-D) .. min(H, s-2)]
            for (int t = tid; t < H * D; t += nt) {
                int y = 1 + t % H, z = 1 + t / H;
                int x = s - y - z;
                if (x >= 1 && x <= W) {
                    long c = cell(g, x, y, z);
                    T nb = q[c + 1] + q[c - 1] + q[c + g.sy] + q[c - g.sy] + q[c + g.sz] + q[c - g.sz];
                    q[c] = (rhs[c] + a * nb) * inv_c;
                }
            }
            __syncthreads();
        }
        bounds_in_block(g, q, flags, b);
    }
}

// Larger grids: the same order, tile by tile.  Cubic tiles of TS^3 cells are themselves swept in
// hyperplane order I+J+L = k, one launch per k (tiles on one tile-hyperplane only touch tiles on
// k-1, already done, and k+1, not yet started); inside a tile one workgroup walks the cell
// hyperplanes with a barrier in between, as gs_lex_kernel does for the whole grid -- on a copy of
// the tile in LDS, so that a step costs an LDS round trip rather than one through L2.
template <class T, int TS>
__global__ __launch_bounds__(TS* TS) void gs_tile_kernel(GridDesc g, T* q, const T* __restrict__ rhs, T a, T inv_c, int k,
                                                          int nL)
{
    constexpr int E = TS + 2;
    __shared__ T t[E][E][E];                             // the tile with one cell of its surroundings on every side
    const int I = blockIdx.x, J = blockIdx.y, L = k - I - J;
    if (L < 0 || L >= nL) return;                        // block-uniform
    const int bx = I * TS, by = J * TS, bz = L * TS;     // tile index e <-> grid coordinate b + e
    // Surroundings as they are in memory now: the -1 faces belong to tiles of hyperplane k-1 (already
    // swept), the +1 faces to tiles of k+1 (not yet), exactly what the lexicographic order sees.
    for (int i = threadIdx.x; i < E * E * E; i += TS * TS) {
        const int ex = i % E, ey = (i / E) % E, ez = i / (E * E);
        const int gx = bx + ex, gy = by + ey, gz = bz + ez;
        t[ez][ey][ex] = (gx <= g.W + 1 && gy <= g.H + 1 && gz <= g.D + 1) ? q[cell(g, gx, gy, gz)] : (T)0;
    }
    const int ly = threadIdx.x % TS, lz = threadIdx.x / TS;
    const int y = by + 1 + ly, z = bz + 1 + lz;
    const bool yz_on = (y <= g.H) && (z <= g.D);
    T r[TS];
#pragma unroll
    for (int lx = 0; lx < TS; ++lx) r[lx] = (yz_on && bx + 1 + lx <= g.W) ? rhs[cell(g, bx + 1 + lx, y, z)] : (T)0;
    __syncthreads();
    for (int s = 0; s < 3 * TS - 2; ++s) {
        const int lx = s - ly - lz;
        if (yz_on && lx >= 0 && lx < TS && bx + 1 + lx <= g.W) {
            T(*c)[E][E] = t;
            const int ex = lx + 1, ey = ly + 1, ez = lz + 1;
            T nb = c[ez][ey][ex + 1] + c[ez][ey][ex - 1] + c[ez][ey + 1][ex] + c[ez][ey - 1][ex] + c[ez + 1][ey][ex] +
                   c[ez - 1][ey][ex];
            T rv = (T)0;
#pragma unroll
            for (int j = 0; j < TS; ++j) rv = (j == lx) ? r[j] : rv;
            c[ez][ey][ex] = (rv + a * nb) * inv_c;
        }
        __syncthreads();
    }
    if (yz_on) {
#pragma unroll
        for (int lx = 0; lx < TS; ++lx)
            if (bx + 1 + lx <= g.W) q[cell(g, bx + 1 + lx, y, z)] = t[lz + 1][ly + 1][lx + 1];
    }
}

template <class T>
void launch_gs_lex(hipStream_t st, const GridDesc& g, T* q, const T* rhs, const uint8_t* flags, int b, T a, T inv_c,
                   int sweeps)
{
    if ((long)g.W * g.H * g.D <= 32768) {                // small: one workgroup does the whole solve in one launch
        hipLaunchKernelGGL((gs_lex_kernel<T>), dim3(1), dim3(1024), 0, st, g, q, rhs, flags, b, a, inv_c, sweeps);
        return;
    }
    constexpr int TS = 16;
    const int nI = (g.W + TS - 1) / TS, nJ = (g.H + TS - 1) / TS, nL = (g.D + TS - 1) / TS;
    SlabCtx whole = { 0, g.D, 1, 1 };                    // gs_lex is single-GPU only
    for (int it = 0; it < sweeps; ++it) {
        for (int k = 0; k <= nI + nJ + nL - 3; ++k)
            hipLaunchKernelGGL((gs_tile_kernel<T, TS>), dim3(nI, nJ), dim3(TS * TS), 0, st, g, q, rhs, a, inv_c, k, nL);
        launch_set_bounds<T>(st, g, whole, q, flags, b);
    }
}
template void launch_gs_lex<float>(hipStream_t, const GridDesc&, float*, const float*, const uint8_t*, int, float, float,
                                   int);
template void launch_gs_lex<double>(hipStream_t, const GridDesc&, double*, const double*, const uint8_t*, int, double,
                                    double, int);

}  // namespace fs
