// vortex.hip -- vortex identification: one z-marching kernel that writes one of the five fields of vortex.h (vorticity
// components, |omega|^2, Q) for every target cell.  The arithmetic is vortex.h's; this file only moves the data, the way
// the two projection passes do (kernels_dev.h, march_tile): a lane owns four x-consecutive cells of RY rows, keeps planes
// z-1, z, z+1 of a component in registers where the selector differences it along z, takes rows y-1 / y+1 from the rows
// of the same wave plus two halo rows, and x-1 / x+1 from the neighbouring lanes.
#include "vortex.h"
#include "kernels_dev.h"

namespace fs {

namespace {

// One velocity component as the kernel holds it.  NX / NY / NZ: the selector reads its x / y / z neighbours.
//   NZ:  m, c, p = planes z-1, z, z+1 of the wave's rows, rotated as the wave walks along z (every plane read once);
//   else c = plane z, loaded per step, and only where NX or NY asks for it.
//   NY:  hb / ht = the rows below and above the wave's rows in plane z.
// Rows up to the ghost row H + 1 are loaded, so that the row above the last live row of a partial band is in c.
template <class T, int RY, bool NX, bool NY, bool NZ>
struct Component {
    static constexpr bool ANY = NX || NY || NZ;
    T m[RY][4], c[RY][4], p[RY][4], hb[4], ht[4];

    __device__ __forceinline__ bool row_on(const MarchTile<T>& t, const GridDesc& g, int r) const { return t.lane_on && (t.y0 + r <= g.H + 1); }

    __device__ __forceinline__ void prime(const T* __restrict__ f, const MarchTile<T>& t, const GridDesc& g)
    {
        if (!NZ) return;
#pragma unroll
        for (int r = 0; r < RY; ++r) {
            ld_row(f + t.row0 + (long)(t.zbeg - 1) * g.sz + r * g.sy, row_on(t, g, r), m[r]);
            ld_row(f + t.row0 + (long)t.zbeg * g.sz + r * g.sy, row_on(t, g, r), c[r]);
        }
    }
    // off = the lane's first cell of row y0 in plane z
    __device__ __forceinline__ void load(const T* __restrict__ f, const MarchTile<T>& t, const GridDesc& g, long off)
    {
        if (!ANY) return;
#pragma unroll
        for (int r = 0; r < RY; ++r) {
            if (NZ) ld_row(f + off + g.sz + r * g.sy, row_on(t, g, r), p[r]);
            else ld_row(f + off + r * g.sy, row_on(t, g, r), c[r]);
        }
        if (NY) {
            ld_row(f + off - g.sy, t.lane_on, hb);
            ld_row(f + off + RY * g.sy, row_on(t, g, RY), ht);
        }
    }
    __device__ __forceinline__ void rotate()
    {
        if (!NZ) return;
#pragma unroll
        for (int r = 0; r < RY; ++r)
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                m[r][e] = c[r][e];
                c[r][e] = p[r][e];
            }
    }
    // the six neighbours of cell e of row r; left / right = the cells before / after the lane's four (all lanes call
    // edges() for them before any lane leaves)
    __device__ __forceinline__ void edges(int r, T& left, T& right) const
    {
        if (!NX) return;
        left = __shfl_up(c[r][3], 1);
        right = __shfl_down(c[r][0], 1);
    }
    __device__ __forceinline__ void edge_loads(const T* __restrict__ f, const MarchTile<T>& t, long base, T& left, T& right) const
    {
        if (!NX) return;
        if (t.edge_l) left = f[base - 1];
        if (t.edge_r) right = f[base + 4];
    }
    __device__ __forceinline__ void nb(int r, int e, T left, T right, T& xp, T& xm, T& yp, T& ym, T& zp, T& zm) const
    {
        if (NX) {
            xp = (e < 3) ? c[r][e < 3 ? e + 1 : e] : right;
            xm = (e > 0) ? c[r][e > 0 ? e - 1 : e] : left;
        }
        if (NY) {
            yp = (r < RY - 1) ? c[r < RY - 1 ? r + 1 : r][e] : ht[e];
            ym = (r > 0) ? c[r > 0 ? r - 1 : r][e] : hb[e];
        }
        if (NZ) {
            zp = p[r][e];
            zm = m[r][e];
        }
    }
};

// Writes rows 1..H of planes zbeg..zend of `out` (the fields' pitched layout): a target cell (interior, obs != 1) takes
// the selector's value rounded once to T, every other cell of the lane's four +0.0.  The cells no lane owns -- the ghost
// column x = 0, the ghost rows and the planes 0 and D + 1 -- are never written: the caller's array holds +0.0 there.
// Reads planes zbeg-1..zend+1, rows y0-1..min(y0+RY, H+1) and cells x0-1..x0+4 <= W+4 < sy of a row: inside the padded
// box but for the row pad, which every 16-byte row access of the project touches.
template <class T, int RY, int SEL>
__global__ __launch_bounds__(256) void vortex_march_kernel(GridDesc g, const T* __restrict__ vx, const T* __restrict__ vy,
                                                            const T* __restrict__ vz, const uint8_t* __restrict__ flags,
                                                            T* __restrict__ out, int zc_len, int nxw, int nybg, int nblk)
{
    const MarchTile<T> t = march_tile<T, RY>(g, zc_len, nxw, nybg, nblk);
    if (!t.live) return;                                 // wave-uniform
    Component<T, RY, vortex_needs(SEL, 0, 0), vortex_needs(SEL, 0, 1), vortex_needs(SEL, 0, 2)> U;
    Component<T, RY, vortex_needs(SEL, 1, 0), vortex_needs(SEL, 1, 1), vortex_needs(SEL, 1, 2)> V;
    Component<T, RY, vortex_needs(SEL, 2, 0), vortex_needs(SEL, 2, 1), vortex_needs(SEL, 2, 2)> Wc;
    U.prime(vx, t, g);
    V.prime(vy, t, g);
    Wc.prime(vz, t, g);
    for (int z = t.zbeg; z <= t.zend; ++z) {
        const long off = t.row0 + (long)z * g.sz;
        U.load(vx, t, g, off);
        V.load(vy, t, g, off);
        Wc.load(vz, t, g, off);
        unsigned fl[RY];
#pragma unroll
        for (int r = 0; r < RY; ++r)
            fl[r] = (t.lane_on && t.y0 + r <= g.H) ? *reinterpret_cast<const unsigned*>(flags + off + r * g.sy) : 0u;
#pragma unroll
        for (int r = 0; r < RY; ++r) {
            const T zero = (T)0;
            T ul = zero, ur = zero, vl = zero, vr = zero, wl = zero, wr = zero;
            U.edges(r, ul, ur);
            V.edges(r, vl, vr);
            Wc.edges(r, wl, wr);
            if (!(t.lane_on && t.y0 + r <= g.H)) continue;   // y <= H is wave-uniform; the shuffles are above
            const long base = off + r * g.sy;
            U.edge_loads(vx, t, base, ul, ur);
            V.edge_loads(vy, t, base, vl, vr);
            Wc.edge_loads(vz, t, base, wl, wr);
            V4<T> st;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                VortexNb<T> n = {};
                U.nb(r, e, ul, ur, n.u_xp, n.u_xm, n.u_yp, n.u_ym, n.u_zp, n.u_zm);
                V.nb(r, e, vl, vr, n.v_xp, n.v_xm, n.v_yp, n.v_ym, n.v_zp, n.v_zm);
                Wc.nb(r, e, wl, wr, n.w_xp, n.w_xm, n.w_yp, n.w_ym, n.w_zp, n.w_zm);
                const bool target = (t.x0 + e <= g.W) && !((fl[r] >> (8 * e)) & F_SOLID);
                st.e[e] = target ? (T)vortex_value<SEL, T>(n) : zero;
            }
            *reinterpret_cast<V4<T>*>(out + base) = st;
        }
        U.rotate();
        V.rotate();
        Wc.rotate();
    }
}

}  // namespace

template <class T>
void launch_vortex(hipStream_t st, const SweepTune& tune, const GridDesc& g, const SlabCtx& sc, int which, const T* vx,
                   const T* vy, const T* vz, const uint8_t* flags, T* out)
{
    (void)sc;                                            // planes 0 and D + 1 are never written, wall or halo
    const int ry = tune.vortex_ry == 1 ? 1 : 2;
    const MarchLaunch m = march_launch(g, ry);
#define FS_VORTEX_LAUNCH_RY(RY, SEL)                                                                                       \
    hipLaunchKernelGGL((vortex_march_kernel<T, RY, SEL>), dim3(m.nblk), dim3(256), 0, st, g, vx, vy, vz, flags, out, m.zc_len, \
                       m.nxw, m.nybg, m.nblk)
#define FS_VORTEX_LAUNCH(SEL)                    \
    do {                                         \
        if (ry == 1) FS_VORTEX_LAUNCH_RY(1, SEL); \
        else FS_VORTEX_LAUNCH_RY(2, SEL);        \
    } while (0)
    switch (which) {
    case VORTEX_WX: FS_VORTEX_LAUNCH(VORTEX_WX); break;
    case VORTEX_WY: FS_VORTEX_LAUNCH(VORTEX_WY); break;
    case VORTEX_WZ: FS_VORTEX_LAUNCH(VORTEX_WZ); break;
    case VORTEX_W2: FS_VORTEX_LAUNCH(VORTEX_W2); break;
    default: FS_VORTEX_LAUNCH(VORTEX_Q); break;
    }
#undef FS_VORTEX_LAUNCH
#undef FS_VORTEX_LAUNCH_RY
}
template void launch_vortex<float>(hipStream_t, const SweepTune&, const GridDesc&, const SlabCtx&, int, const float*, const float*,
                                   const float*, const uint8_t*, float*);
template void launch_vortex<double>(hipStream_t, const SweepTune&, const GridDesc&, const SlabCtx&, int, const double*,
                                    const double*, const double*, const uint8_t*, double*);

}  // namespace fs
