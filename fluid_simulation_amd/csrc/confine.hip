// confine.hip -- vorticity confinement: one fused z-marching kernel that reads the three velocity components once and
// writes the three confined components, ghost faces and zeroed cells included (include/fluidsim.h, "vorticity
// confinement").  The arithmetic is confine.h's; this file only moves the data.
//
// A workgroup owns a tile of TX x TY cells and walks a chunk of planes.  The stencil has radius 2 in two stages -- the curl
// of a cell reads its six neighbours, the force reads |curl| of the six neighbours -- so both stages live in LDS rings:
//   sv: planes p-1, p, p+1 of u, v, w for the tile and two cells of halo (x from 16-byte row accesses: the ring's rows start
//       four cells left of the tile, where a row is 16-byte aligned);
//   sm: |curl| on planes p-1 and p for the tile and one cell of halo, in fp64 (the planes below and above the one being
//       emitted are needed at a lane's own cells only: registers).
// Iteration p first requests plane p+2 (16-byte loads into registers) and the flag bytes of plane p+1, then computes |curl|
// on plane p (a lane: its own four x-consecutive cells of one row, whose curl, flag bytes and stored values it keeps in
// registers; the first lanes: a cell of the halo ring each), emits plane p-1 from the registers of the iteration before, and
// only then stores plane p+2 over plane p-1 in the ring: the loads travel behind the arithmetic (two workgroups of four waves
// per CU are too few to hide them otherwise; the unpipelined form measured 1.57x slower).  Two barriers per plane.  Every
// plane of a chunk is read once, plus two planes of lead-in and two of lead-out per chunk and the halo (1.33x for the 64 x 16
// tile of fp32, 1.69x for the 64 x 8 tile of fp64).
#include "confine.h"
#include "kernels_dev.h"

namespace fs {

namespace {

template <class T>
struct ConfineShape {
    static constexpr int TX = 64, TY = sizeof(T) == 4 ? 16 : 8;   // two workgroups per CU fit the 160 KB of LDS either way
    static constexpr int NT = TX * TY / 4;                       // a lane owns four x-consecutive cells
    static constexpr int NQ = TX / 4 + 2, RV = TY + 4;           // sv: quads per row (col = x - (tx0 - 4)), rows (row = y - (ty0 - 2))
    static constexpr int RM = TY + 2;                            // sm: the same columns, row = y - (ty0 - 1)
    // Both rings keep a row as four sub-rows: cell `col` lies at [col & 3][col >> 2], so that the 16 lanes of a row, which own
    // four consecutive cells each, read consecutive words for each of their cells and its x neighbours (as plain rows they would
    // read every fourth word: 4-way bank conflicts, 70 % of the LDS cycles when measured).  QP = 20 makes a row 80 elements: the
    // rows of a wave start 16 banks apart (fp32; 32 for 8-byte elements, which are served 32 lanes at a time) and tile the 64 banks.
    static constexpr int QP = 20;
    static constexpr int NB = 2 * TX + 2 * TY;                   // cells of the halo ring around the tile (face neighbours only)
};

// The launch shape: about 1024 workgroups (two per CU at a time), z chunks of at least 8 planes -- march_launch's rule
// (kernels_dev.h) with half the workgroups, because every chunk re-reads four planes.
struct ConfineLaunch {
    int zc_len, ntx, nty, nblk;
};
template <class T>
ConfineLaunch confine_launch(const GridDesc& g)
{
    using S = ConfineShape<T>;
    ConfineLaunch m;
    m.ntx = (g.W + S::TX - 1) / S::TX;
    m.nty = (g.H + S::TY - 1) / S::TY;
    const long per_layer = (long)m.ntx * m.nty;
    long want = (1024 + per_layer - 1) / per_layer;
    if (want < 1) want = 1;
    m.zc_len = (int)((g.D + want - 1) / want);
    if (m.zc_len < 8) m.zc_len = g.D < 8 ? g.D : 8;
    const int nzc = (g.D + m.zc_len - 1) / m.zc_len;
    m.nblk = (int)(per_layer * nzc);
    return m;
}

__device__ __forceinline__ int ring3(int p) { return (p + 3) % 3; }   // p >= -1

// Plane p of the three components on its way into its ring slot (p is uniform over the workgroup): fetch() issues the lane's
// 16-byte loads into registers, stash() stores them into the ring -- an iteration's arithmetic runs between the two.
template <class T>
struct ConfineStage {
    static constexpr int TOTAL = 3 * ConfineShape<T>::RV * ConfineShape<T>::NQ;
    static constexpr int NS = (TOTAL + ConfineShape<T>::NT - 1) / ConfineShape<T>::NT;
    T q[NS][4];
};
template <class T, bool STORE>
__device__ __forceinline__ void confine_move_plane(ConfineStage<T>& st, T (&sv)[3][3][ConfineShape<T>::RV][4][ConfineShape<T>::QP],
                                                   const GridDesc& g, const T* __restrict__ vx, const T* __restrict__ vy,
                                                   const T* __restrict__ vz, int tid, int tx0, int ty0, int p)
{
    using S = ConfineShape<T>;
    if (p < 0 || p > g.D + 1) return;
    const int s = ring3(p);
#pragma unroll
    for (int j = 0; j < ConfineStage<T>::NS; ++j) {
        const int i = tid + j * S::NT;
        const int comp = i / (S::RV * S::NQ), rem = i % (S::RV * S::NQ), row = rem / S::NQ, qd = rem % S::NQ;
        const int yy = ty0 - 2 + row, xs = tx0 - 4 + 4 * qd;
        const bool on = i < ConfineStage<T>::TOTAL && yy >= 0 && yy <= g.H + 1 && xs <= g.W + 1;
        if (STORE) {
            if (on) {
#pragma unroll
                for (int e = 0; e < 4; ++e) sv[s][comp][row][e][qd] = st.q[j][e];
            }
        } else {
            const T* f = comp == 0 ? vx : comp == 1 ? vy : vz;
            ld_row(f + (long)xs + (long)yy * g.sy + (long)p * g.sz, on, st.q[j]);
        }
    }
}
// curl and |curl| of the target cell at ring position (row, col) of plane p (slots sm1, s0, sp1 = planes p-1, p, p+1)
template <class T>
__device__ __forceinline__ ConfineCurl confine_curl_at(const T (&sv)[3][3][ConfineShape<T>::RV][4][ConfineShape<T>::QP], int sm1, int s0,
                                                       int sp1, int row, int col)
{
    const int e = col & 3, q = col >> 2, ep = (col + 1) & 3, qp = (col + 1) >> 2, em = (col - 1) & 3, qm = (col - 1) >> 2;
    VortexNb<T> n = {};
    n.u_yp = sv[s0][0][row + 1][e][q]; n.u_ym = sv[s0][0][row - 1][e][q];
    n.u_zp = sv[sp1][0][row][e][q];    n.u_zm = sv[sm1][0][row][e][q];
    n.v_xp = sv[s0][1][row][ep][qp];   n.v_xm = sv[s0][1][row][em][qm];
    n.v_zp = sv[sp1][1][row][e][q];    n.v_zm = sv[sm1][1][row][e][q];
    n.w_xp = sv[s0][2][row][ep][qp];   n.w_xm = sv[s0][2][row][em][qm];
    n.w_yp = sv[s0][2][row + 1][e][q]; n.w_ym = sv[s0][2][row - 1][e][q];
    return confine_magnitude(n);
}

template <int NBT>
__device__ __forceinline__ void confine_fetch_flags(const uint8_t* __restrict__ flags, const GridDesc& g, int p, bool own_on, long own0,
                                                    const long (&bcell)[NBT], unsigned& flq, unsigned (&bfq)[NBT])
{
    const bool plane = p >= 1 && p <= g.D;
    flq = (plane && own_on) ? *reinterpret_cast<const unsigned*>(flags + own0 + (long)p * g.sz) : 0x01010101u;
#pragma unroll
    for (int j = 0; j < NBT; ++j) bfq[j] = (plane && bcell[j] >= 0) ? flags[bcell[j] + (long)p * g.sz] : (unsigned)F_SOLID;
}

// Reads planes zbeg-2..zend+2 (inside 0..D+1), rows ty0-2..ty0+TY+1 (inside 0..H+1) and the 16-byte groups that start at
// cells tx0-4 >= -3 .. <= W+1 of a row: inside the allocation (LEAD cells lie before cell 0) and inside the padded box but for
// the row pad, which every 16-byte row access of the project touches.  Writes, of each result array, rows 0..H+1 of planes
// zbeg..zend (and the ghost planes 0 / D+1 beside them) at cells 0..W+3 < sy; the twelve box edges take +0.0 or stay.
template <class T>
__global__ __launch_bounds__(ConfineShape<T>::NT) __attribute__((flatten)) void confine_kernel(GridDesc g, const T* __restrict__ vx, const T* __restrict__ vy,
                                                                      const T* __restrict__ vz, const uint8_t* __restrict__ flags,
                                                                      T* __restrict__ ox, T* __restrict__ oy, T* __restrict__ oz,
                                                                      double k, int zc_len, int ntx, int nty, int nblk)
{
    using S = ConfineShape<T>;
    __shared__ alignas(16) T sv[3][3][S::RV][4][S::QP];
    __shared__ alignas(16) double sm[2][S::RM][4][S::QP];  // planes p-1 and p: a lane keeps |curl| of its own cells on the planes
                                                           // below and above the one it emits in registers

    const int blk = xcd_contiguous(blockIdx.x, nblk);
    const int tx0 = 1 + (blk % ntx) * S::TX, ty0 = 1 + ((blk / ntx) % nty) * S::TY, zc = blk / (ntx * nty);
    const int zbeg = 1 + zc * zc_len, zend = min(g.D, zbeg + zc_len - 1);
    const int tid = threadIdx.x, xq = tid % (S::TX / 4), yr = tid / (S::TX / 4);
    const int x0 = tx0 + 4 * xq, y = ty0 + yr;
    const bool own_on = x0 <= g.W && y <= g.H;
    const long own0 = (long)x0 + (long)y * g.sy;          // the lane's first cell in plane 0

    ConfineCurl wc[4] = {}, wn[4] = {};                   // the lane's four cells on the plane to emit / the plane just computed
    unsigned flc = 0, fln = 0;
    T vc[3][4] = {}, vn[3][4] = {};
    double mbelow[4] = {};                                // |curl| of the lane's cells one plane below the one to emit

    // the lane's cells of the halo ring (two rows of TX, two columns of TY), -1 = none or outside the interior
    constexpr int NBT = (S::NB + S::NT - 1) / S::NT;
    int bx[NBT], by[NBT];
    long bcell[NBT];
#pragma unroll
    for (int j = 0; j < NBT; ++j) {
        const int i = tid + j * S::NT;
        if (i < 2 * S::TX) {
            bx[j] = tx0 + i % S::TX;
            by[j] = i < S::TX ? ty0 - 1 : ty0 + S::TY;
        } else {
            const int r = i - 2 * S::TX;
            bx[j] = r < S::TY ? tx0 - 1 : tx0 + S::TX;
            by[j] = ty0 + r % S::TY;
        }
        const bool in = i < S::NB && bx[j] >= 1 && bx[j] <= g.W && by[j] >= 1 && by[j] <= g.H;
        bcell[j] = in ? (long)bx[j] + (long)by[j] * g.sy : -1;
    }
    // the flag bytes of the lane's cells on plane p: its own four (one word) and its halo-ring cells; solid where there is no cell
    unsigned flq = 0, bfq[NBT];

    ConfineStage<T> stage;
    for (int p = zbeg - 2; p <= zbeg; ++p) {
        confine_move_plane<T, false>(stage, sv, g, vx, vy, vz, tid, tx0, ty0, p);
        confine_move_plane<T, true>(stage, sv, g, vx, vy, vz, tid, tx0, ty0, p);
    }
    confine_fetch_flags<NBT>(flags, g, zbeg - 1, own_on, own0, bcell, flq, bfq);
    __syncthreads();
    // Iteration p: plane p + 2 and the flag bytes of plane p + 1 are requested first and arrive behind the arithmetic; the ring
    // holds planes p-1, p, p+1.  |curl| on plane p; barrier; emit plane p-1; plane p + 2 replaces plane p - 1; barrier.
    for (int p = zbeg - 1; p <= zend + 1; ++p) {
        if (p <= zend) confine_move_plane<T, false>(stage, sv, g, vx, vy, vz, tid, tx0, ty0, p + 2);
        fln = flq;
        unsigned bfn[NBT];
#pragma unroll
        for (int j = 0; j < NBT; ++j) bfn[j] = bfq[j];
        confine_fetch_flags<NBT>(flags, g, p + 1, own_on, own0, bcell, flq, bfq);
        if (p >= 1 && p <= g.D) {
            const int sm1 = ring3(p - 1), s0 = ring3(p), sp1 = ring3(p + 1);
            if (own_on) {
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const int row = yr + 2, col = 4 + 4 * xq + e;
#pragma unroll
                    for (int a = 0; a < 3; ++a) vn[a][e] = sv[s0][a][row][e][xq + 1];
                    const bool target = (x0 + e <= g.W) && !((fln >> (8 * e)) & F_SOLID);
                    ConfineCurl c = { 0.0, 0.0, 0.0, 0.0 };
                    if (target) c = confine_curl_at<T>(sv, sm1, s0, sp1, row, col);
                    wn[e] = c;
                    sm[p & 1][yr + 1][e][xq + 1] = c.m;
                }
            }
#pragma unroll
            for (int j = 0; j < NBT; ++j) {
                if (bcell[j] < 0 || (bfn[j] & F_SOLID)) continue;
                const int bc = bx[j] - (tx0 - 4);
                sm[p & 1][by[j] - (ty0 - 1)][bc & 3][bc >> 2] = confine_curl_at<T>(sv, sm1, s0, sp1, by[j] - (ty0 - 2), bc).m;
            }
        }
        __syncthreads();
        const int q = p - 1;                              // the plane to emit: its |curl| neighbours are all in sm now
        if (q >= zbeg && own_on) {
            const int mq = q & 1;
            T un[3][4];                                   // the new values before any zeroing: what the ghost faces copy
            V4<T> st[3];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const unsigned fb = (flc >> (8 * e)) & 0xffu;
                const int mr = yr + 1, mc = 4 + 4 * xq + e;
#pragma unroll
                for (int a = 0; a < 3; ++a) un[a][e] = vc[a][e];
                if (x0 + e <= g.W && !(fb & F_SOLID)) {
                    const double mn[6] = { sm[mq][mr][(mc + 1) & 3][(mc + 1) >> 2], sm[mq][mr][(mc - 1) & 3][(mc - 1) >> 2],
                                           sm[mq][mr + 1][e][xq + 1], sm[mq][mr - 1][e][xq + 1], wn[e].m, mbelow[e] };
                    const ConfineForce f = confine_force(wc[e], mn, (fb >> 2) & 63u);
                    if (f.on) {
                        un[0][e] = confine_apply(vc[0][e], k, f.fx);
                        un[1][e] = confine_apply(vc[1][e], k, f.fy);
                        un[2][e] = confine_apply(vc[2][e], k, f.fz);
                    }
                }
#pragma unroll
                for (int a = 0; a < 3; ++a) {
                    const int x = x0 + e;
                    st[a].e[e] = x <= g.W      ? ((fb & (F_SOLID | F_NEAR)) ? (T)0 : un[a][e])
                               : x == g.W + 1 ? un[a][e > 0 ? e - 1 : 0]      // the ghost face x = W + 1 (e > 0 here: x0 <= W)
                                              : (T)0;                         // the row pad
                }
            }
            // (store_row_bounds of kernels_dev.h with b = 1, 2, 3, restated: through three calls this kernel is 40 / 51 instructions longer)
            const long base = own0 + (long)q * g.sz;
            T* const out[3] = { ox, oy, oz };
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                T* o = out[a];
                *reinterpret_cast<V4<T>*>(o + base) = st[a];
                if (x0 == 1) o[base - 1] = (a == 0) ? -un[a][0] : un[a][0];
                if (x0 + 3 == g.W) o[base + 4] = un[a][3];
                // ghost rows and planes: the reflected or copied new values; the box edges beyond x = W take +0.0
                V4<T> gy, gz;
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const bool in = x0 + e <= g.W;
                    gy.e[e] = in ? ((a == 1) ? -un[a][e] : un[a][e]) : (T)0;
                    gz.e[e] = in ? ((a == 2) ? -un[a][e] : un[a][e]) : (T)0;
                }
                if (y == 1) *reinterpret_cast<V4<T>*>(o + base - g.sy) = gy;
                if (y == g.H) *reinterpret_cast<V4<T>*>(o + base + g.sy) = gy;
                if (q == 1) *reinterpret_cast<V4<T>*>(o + base - g.sz) = gz;
                if (q == g.D) *reinterpret_cast<V4<T>*>(o + base + g.sz) = gz;
            }
        }
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            mbelow[e] = wc[e].m;
            wc[e] = wn[e];
#pragma unroll
            for (int a = 0; a < 3; ++a) vc[a][e] = vn[a][e];
        }
        flc = fln;
        if (p <= zend) confine_move_plane<T, true>(stage, sv, g, vx, vy, vz, tid, tx0, ty0, p + 2);
        __syncthreads();
    }
}

}  // namespace

template <class T>
void launch_confine(hipStream_t st, const GridDesc& g, const T* vx, const T* vy, const T* vz, const uint8_t* flags, T* ox, T* oy,
                    T* oz, double k)
{
    const ConfineLaunch m = confine_launch<T>(g);
    hipLaunchKernelGGL((confine_kernel<T>), dim3(m.nblk), dim3(ConfineShape<T>::NT), 0, st, g, vx, vy, vz, flags, ox, oy, oz, k,
                       m.zc_len, m.ntx, m.nty, m.nblk);
}
template void launch_confine<float>(hipStream_t, const GridDesc&, const float*, const float*, const float*, const uint8_t*, float*,
                                    float*, float*, double);
template void launch_confine<double>(hipStream_t, const GridDesc&, const double*, const double*, const double*, const uint8_t*,
                                     double*, double*, double*, double);

}  // namespace fs
