// sweep_fused.hip -- NL Jacobi sweeps per pass over memory (temporal blocking), register-centred.
//
//   linearSolver  simulation.cpp:251-273 (NL iterations of the k loop, neighbours read from the
//                 previous iterate), each followed by
//   setBounds     simulation.cpp:183-246,
// bit-identical with NL launches of jacobi_sweep_kernel (kernels.hip).
//
// One sweep moves 12 B per cell (fp32) for 8 flops; the only way past the HBM roof is to apply
// several sweeps while the data is on chip.  Level 0 = `src`, level j = the iterate after j
// sweeps + setBounds (levels 1..NL-1 never reach memory), level NL = `dst`.
//
// A workgroup owns the full row width (NXW waves of 256 cells) times a band of BY = NYW*RY rows
// and marches along z.  A wave keeps its own cells of every level for three consecutive planes in
// registers (three slots per level, rotated by unrolling the march three times, so nothing is
// ever copied); LDS only carries what a wave needs from its neighbours -- the rows just above
// and below its patch and the two columns beside it -- in a two-slot ring per intermediate level.
// In iteration zl a wave computes level 1 of plane zl, level 2 of plane zl-1 (and level 3 of plane
// zl-2); level j+1 of plane P reads the level-j tile of plane P that was published one iteration
// earlier, so one barrier per iteration is enough and two slots per ring suffice.  The right-hand
// side of a plane is needed in NL consecutive iterations; each thread parks its own values in a
// private LDS ring instead of holding NL+1 planes of it in registers.
//
// setBounds between the levels, exactly as it would happen in memory: interior cells are zeroed
// (settle4); the ghost columns x = 0, W+1 and ghost rows y = 0, H+1 of a level are written into
// the LDS tile from the unzeroed values (simulation.cpp:186-201), the ghost planes z = 0, D+1
// into the register slot the missing plane would occupy (:208-214).
// Bands overlap by 2(NL-1) rows and z chunks by 2(NL-1) planes.
//
// Instantiations (LDS = (NL-1)*2*BY*TW + NL*(BY-2)*RW elements must stay under 160 KB):
//   fp32 NL=3  rows <= 512 cells   the solver kernel at 256^3 and 512^3: 0.37 ms per pass at 512^3
//                                  = 0.12 ms per sweep, 12 waves of two rows, 150 VGPRs, no scratch
//   fp32 NL=2  rows 513..1024      config 4: bands of 8 or 9 rows (6 or 7 productive) where the older
//                                  jacobi_pair_kernel (kernels.hip) only fits 6 (4 productive)
//   fp64 NL=2  rows <= 512         config 5: bands of 10 rows (8 productive) against 8 (6)
// The two NL=2 families are candidates of the host's one-off timing, which so far always prefers the pair
// kernel to them (0.83 vs 0.71 ms at 1024x512x512, 0.84 vs 0.77 fp64 at 512^3: both sit at the same memory
// ceiling, and per level this structure costs more instructions); three sweeps per pass is where it pays.
// SLAB = true adds what a z-slab of a multi-GPU run needs: an output plane range (the boundary
// regions are computed first), no physical wall on a side that borders another slab -- the levels
// are then computed NL-1 planes into the neighbour's planes from the NL-deep halo -- and an optional
// second range in the same launch.  SLAB = false compiles all of that away (whole domain on one GPU).
//
// What made the difference in speed is written up in DESIGN.md section 4 (uniform wave index through
// readfirstlane, scalar plane pointers + opaque 32-bit lane offsets, unpredicated loads).
#include <hip/hip_runtime.h>
#include "kernels.h"
#include "kernels_dev.h"
#include <type_traits>

namespace fs {

template <int N>
struct IC {
    static constexpr int value = N;
};

// Experiment switch (build with -DFS_EXP_NT=1|2|3): nontemporal loads of the right-hand side (1) and / or nontemporal
// stores of the result (2).  Measured at 512^3 on one box (profiles/r02k_nontemporal_ab_c3.json): 0 -> 0.1465, 1 -> 0.150,
// 2 -> 0.146, 3 -> 0.148 ms per sweep; the shipped library is built with 0.
// Nontemporal loads of level 0 (dead after the pass; tried with the reversed march so that the Infinity Cache might keep more of the two
// arrays that are read again) are not a switch here: 84.1 against 59.7-60.3 ms per step at 512^3 (profiles/r18a_z_alternate.json).
#ifndef FS_EXP_NT
#define FS_EXP_NT 0
#endif
template <class T>
using Vec4 = T __attribute__((ext_vector_type(4)));

// x neighbours across lanes (fp32): lane i takes lane i - 1's (wave_shr:1) or lane i + 1's (wave_shl:1) value; the one
// lane without a source (lane 0 / lane 63) keeps `edge`, the cell beyond the wave (bound_ctrl off).  Needs all 64 lanes on.
__device__ __forceinline__ float lane_from_left(float v, float edge)
{
    return __int_as_float(__builtin_amdgcn_update_dpp(__float_as_int(edge), __float_as_int(v), 0x138, 0xf, 0xf, false));
}
__device__ __forceinline__ float lane_from_right(float v, float edge)
{
    return __int_as_float(__builtin_amdgcn_update_dpp(__float_as_int(edge), __float_as_int(v), 0x130, 0xf, 0xf, false));
}
// a wave-uniform fp32 load through the scalar cache (s_load_dword)
__device__ __forceinline__ float load_uniform(const char* p)
{
    return *(const __attribute__((address_space(4))) float*)p;
}

// WALLSEL = 3 (mask-free build): {zbeg, zend, ga, gb} per workgroup, made on the host (chunk_plan.h: mask_free_plan)
struct CleanArgs {
    const int* plan = nullptr;
};

// Z0 (zero start): level 0 is all zeros and is not read -- no load_core, no hb / ht / eL / eR loads, L0 held as constants.  The
// level-1 expression stays (rh + a * nb) * inv_c on nb = 0 + 0 + ..., the operations a zeroed `src` would feed it (no
// fast-math, -ffp-contract=off), so the result is bit-identical with reading zeros; `src` is never dereferenced.
//
// ZREV (reversed march): the workgroup marches from plane D down to plane 1, so that a pass which follows an upward one starts
// on the planes that pass touched last (what the Infinity Cache still holds).  Everything below works on LOGICAL planes
// z' = D + 1 - z and is the upward march of the z-mirrored problem; only three things know the real plane: the plane addresses
// (plane_of, the kill bytes, the stores -- one mapping, `zorg_b` + z' * `zdir_b`), the sum of the two z neighbours in relax4 (the
// reference adds z+1 before z-1 in REAL coordinates, and fp32 sums do not commute in the last bit), and the host's mask-free
// table, which is made from the mirrored clean table (chunk_plan.h).  Both z walls are physical and treated alike (face4 on
// b == 3 at either), so nothing else changes.
template <class T, int NL, int NXW, int NYW, int RY, bool ALIGNED, bool SLAB, int WALLSEL, bool Z0 = false, bool ZREV = false>
__global__ __launch_bounds__(NXW* NYW * 64) void jacobi_fused_kernel(GridDesc g, SlabCtx sc, const T* __restrict__ src,
                                                                      const T* __restrict__ rhs, T* __restrict__ dst,
                                                                      const uint8_t* __restrict__ flags, int b, T a, T inv_c,
                                                                      int z_first, int z_last, int zc_len, int z_stride,
                                                                      int nbands, int nblk, PeerPush pp, CleanArgs ca)
{
    static_assert(NL == 2 || NL == 3, "two or three sweeps per pass");
    static_assert(!Z0 || (NL == 3 && ALIGNED && !SLAB && sizeof(T) == 4 && (WALLSEL == 1 || WALLSEL == 3)),
                  "the zero-start form exists for the whole-domain lane-aligned fp32 three-sweep builds");
    static_assert(!ZREV || (NL == 3 && ALIGNED && !SLAB && sizeof(T) == 4 && (WALLSEL == 1 || WALLSEL == 3) && !Z0),
                  "the reversed march exists for the whole-domain lane-aligned fp32 three-sweep builds that read level 0");
    constexpr int BY = NYW * RY, TW = NXW * 256 + 8, RW = NXW * 256;
    constexpr int OV = NL - 1;                           // rows / planes a band / chunk loses per side
    constexpr int ES = (int)sizeof(T);
    // WALLSEL = 2, the "lean interior" experiment (round-2 verdict, item 5): no right-hand-side ring -- the later levels re-read
    // the rhs rows from memory (L2 / MALL hits) -- which frees 61 KB of LDS for 16-row bands, and only the wall-free body
    // (workgroups that touch no wall).  See DESIGN.md section 4 for what it measured.
    constexpr bool RS = (WALLSEL != 2);
    // XS: three fp32 sweeps on lane-aligned rows take the x neighbours of a lane's four cells from the lanes beside it (DPP
    // wave shifts) and only the one value beyond either end of the wave from memory (level 1: a scalar load) or the LDS tile
    // (levels 2, 3: one read of the tile cell `publish` wrote).  Same values as the per-lane reads of the other builds.
    constexpr bool XS = ALIGNED && NL == 3 && sizeof(T) == 4;
    static_assert(((NL - 1) * 2 * BY * TW + (RS ? NL * (BY - 2) * RW : 0)) * ES <= 160 * 1024, "LDS budget");
    __shared__ T ring[NL - 1][2][BY][TW];                // [level-1][plane & 1][tile row][x + 3]
    __shared__ T rsave[RS ? NL : 1][RS ? BY - 2 : 1][RW];   // thread-private: rhs of the last NL planes

    const int v = xcd_contiguous(blockIdx.x, nblk);
    const int band = v % nbands, zc = v / nbands;
    // readfirstlane: the wave index is the same in all 64 lanes, but only this tells the compiler so -- rows,
    // row pointers and every row test then live in scalar registers and branch as scalars
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
    const int wx = wave % NXW, wy = wave / NXW;
    const int W = g.W, H = g.H, D = g.D;
    // tile row t <-> grid row s + t.  Band k outputs the BY - 2 OV rows k (BY - 2 OV) + 1 ..: every band the same number,
    // also the bands at the y walls (a wall costs no rows, so with s = k (BY - 2 OV) the first band would output NL - 2 more
    // than the others; round 3 shifts the origin instead, which makes the wall bands the lighter ones)
    const int s = band * (BY - 2 * OV) - (OV - 1);
    const int ty0 = wy * RY, y0 = s + ty0;
    const int xl = wx * 256 + lane * 4;
    const int x0 = 1 + xl;
    const bool lane_on = ALIGNED || (x0 <= W);
    const bool full_group = ALIGNED || (x0 + 3 <= W);
    // physical z walls: both on one GPU; on a slab only the first / last rank has one
    const bool lo_wall = SLAB ? (sc.lo_wall != 0) : true, hi_wall = SLAB ? (sc.hi_wall != 0) : true;
    const int* plan = WALLSEL == 3 ? ca.plan + 4 * v : nullptr;                          // (wave-uniform: scalar loads)
    const int zbeg = WALLSEL == 3 ? plan[0] : SLAB ? z_first + zc * z_stride : 1 + zc * zc_len;   // level-NL output planes
    const int zend = WALLSEL == 3 ? plan[1] : min(SLAB ? z_last : D, zbeg + zc_len - 1);
    if (zbeg > zend) return;                             // block-uniform
    // planes of level j: NL-j beyond the output chunk on each side; beyond a physical wall there is no
    // such plane (its ghost is derived below), beyond a slab boundary it is the neighbour's plane,
    // recomputed here from the NL-deep halo
    const int zlo_lim = lo_wall ? 1 : 1 - OV, zhi_lim = hi_wall ? D : D + OV;
    const int lo1 = max(zlo_lim, zbeg - OV), hi1 = min(zhi_lim, zend + OV);             // level-1 planes
    const int lo2 = max(zlo_lim, zbeg - (OV - 1)), hi2 = min(zhi_lim, zend + (OV - 1)); // level-2 planes
    const int zmax0 = hi_wall ? D + 1 : D + NL, zmax1 = hi_wall ? D : D + OV;           // last level-0 / level-1 plane that exists
    // Everything below can exist twice (WALLSEL = 1): the general body, and one for workgroups that touch no wall in y or z
    // (interior bands x interior z chunks), in which every wall test, ghost row / ghost plane and the registers that carry
    // them are compiled out -- 523 instead of 837 instructions per plane, 126 instead of 152 VGPRs on its own.  The two are
    // separate loops selected once per workgroup (two bodies inside ONE loop spill at their merge, round 1).
    // The march's state lives outside the bodies so that a workgroup can change body between plane iterations (round 3):
    T L0[3][RY][4], L1[3][RY][4] = {}, L2[3][RY][4] = {};
    T hb[4], ht[4], eL[RY], eR[RY], rcur[RY][4];
    T gz1[RY][4] = {}, gz2[RY][4] = {};                 // ghost plane D+1 of levels 1 and 2 while it waits for its register slot
    unsigned flc[RY], kl[3][RY] = {};                    // (not in idle load registers: a select on those would wait for the loads)
    if constexpr (Z0) {
#pragma unroll
        for (int r = 0; r < RY; ++r) {
            eL[r] = eR[r] = (T)0;
#pragma unroll
            for (int e = 0; e < 4; ++e) L0[0][r][e] = L0[1][r][e] = L0[2][r][e] = (T)0;
        }
#pragma unroll
        for (int e = 0; e < 4; ++e) hb[e] = ht[e] = (T)0;
    }
    // `ngroups` groups of three plane iterations from z_from on with one of the bodies (the register slots rotate with period
    // three: a group starts and ends with every plane in its home slot, so bodies can alternate between groups), then, with
    // tail_to >= 0, the march's last one or two iterations up to tail_to.  wallc: 1 general, 0 wall-free, 2 mask-free (wall-free,
    // and every kill byte its settle4s would read is 0: no kill-byte loads, settle4 is a copy)
    auto run = [&](auto wallc, int z_from, int ngroups, int tail_to) {
    constexpr bool WALLS = decltype(wallc)::value == 1, MF = decltype(wallc)::value == 2;
    const bool lo_wall_c = WALLS && lo_wall, hi_wall_c = WALLS && hi_wall;      // the ghost-plane code of the physical z walls
    // rows a level can be computed for: one fewer per level at a band edge, none lost at a wall
    const bool top_in_tile = WALLS && (s + BY - 1 >= H + 1), bottom_in_tile = WALLS && (s <= 0);
    const int r2lo = bottom_in_tile ? 1 : s + 1, r2hi = top_in_tile ? H : s + BY - 2;
    const int r3lo = bottom_in_tile ? 1 : s + 2, r3hi = top_in_tile ? H : s + BY - 3;
    const int kill_shift = (b == 0) ? 0 : 4;
    const T zero = (T)0;

    // Addressing: a plane pointer (wave-uniform, advanced by the march) plus a 32-bit byte offset per
    // row that never changes.  Loads are never predicated (a predicated load merges with a default
    // value, which makes the compiler wait for it on the spot instead of one iteration later): rows
    // outside the array are clamped to a row inside it and lanes beyond the row end read the row
    // start; what they fetch is never used for a cell that exists.
    // Per-row byte offsets inside a plane sit in vector registers, the plane pointers in scalar ones --
    // the scalar file is the scarce one here (every spilled scalar costs a v_readlane plus hazard nops).
    const unsigned col0 = lane_on ? (unsigned)x0 : 1u;
    // levels 2, 3 (XS): the tile column holding lane 0's left neighbour (lanes 0-31) or lane 63's right one (lanes 32-63) --
    // one ds_read_b32 with two addresses, one per half-wave, in place of a 4-way bank conflict per x neighbour
    const int xe = wx * 256 + (lane < 32 ? 3 : 260);
    auto clampy = [&](int y) { return (unsigned)min(max(y, 0), H + 1); };
    unsigned oc[RY];                                     // bytes into a plane of T; kill byte index = (element + 3) >> 2
#pragma unroll
    for (int r = 0; r < RY; ++r) oc[r] = (col0 + clampy(y0 + r) * (unsigned)g.sy) * (unsigned)ES;
    const long plane_b = (long)g.sz * ES, plane_f = (long)(g.sz >> 2), row_b = (long)g.sy * ES;
    // rows below / above the patch: the first / last own row's offset with a wave-uniform step (0 where clamped)
    const long step_b = (long)(clampy(y0) - clampy(y0 - 1)) * row_b, step_t = (long)(clampy(y0 + RY) - clampy(y0 + RY - 1)) * row_b;
    // logical plane z -> bytes from an array's plane 0 (ZREV: real plane D + 1 - z)
    const long zorg_b = ZREV ? (long)(D + 1) * plane_b : 0, zdir_b = ZREV ? -plane_b : plane_b;
    auto plane_of = [&](const T* base, int z) { return reinterpret_cast<const char*>(base) + zorg_b + (long)z * zdir_b; };   // wave-uniform
    auto ld4 = [&](const char* ptr, T (&out)[4]) {
        V4<T> q = *reinterpret_cast<const V4<T>*>(ptr);
#pragma unroll
        for (int e = 0; e < 4; ++e) out[e] = q.e[e];
    };

    auto load_core = [&](int z, T (&out)[RY][4]) {
        if constexpr (Z0) return;
        const char* sp = plane_of(src, z);
#pragma unroll
        for (int r = 0; r < RY; ++r) ld4(sp + oc[r], out[r]);
    };
    auto load_side = [&](int z) {                        // what level 1 of plane z needs beside the wave's own cells
        const char* sp = plane_of(src, z);
        const char* rp = plane_of(rhs, z);
        const uint8_t* fp = flags + (long)(ZREV ? D + 1 - z : z) * plane_f;
        if constexpr (!Z0) {
            ld4(sp - step_b + oc[0], hb);
            ld4(sp + step_t + oc[RY - 1], ht);
        }
#pragma unroll
        for (int r = 0; r < RY; ++r) {
            if constexpr (Z0) {                          // (level 0 is not read)
            } else if constexpr (XS) {                   // the cells x = 256 wx and 256 wx + 257 of the row (wave-uniform)
                const char* rowp = sp + (long)(wx * 256 + (int)clampy(y0 + r) * g.sy) * ES;
                eL[r] = load_uniform(rowp);
                eR[r] = load_uniform(rowp + 257 * ES);
            } else {
                eL[r] = *reinterpret_cast<const T*>(sp + oc[r] - ES);    // every lane fetches its own x neighbours:
                eR[r] = *reinterpret_cast<const T*>(sp + oc[r] + 4 * ES);    // no shuffles, no edge lanes
            }
            if (FS_EXP_NT & 1) {
                const Vec4<T> q = __builtin_nontemporal_load(reinterpret_cast<const Vec4<T>*>(rp + oc[r]));
#pragma unroll
                for (int e = 0; e < 4; ++e) rcur[r][e] = q[e];
            } else ld4(rp + oc[r], rcur[r]);
            if constexpr (!MF) flc[r] = (unsigned)fp[(oc[r] / (unsigned)ES + 3u) >> 2];
        }
    };

    // one stencil application; simulation.cpp:264-269 order x+1, x-1, y+1, y-1, z+1, z-1
    // (Writing the four cells as two interleaved packed chains removes 55 of the 73 hazard s_nops per plane iteration of
    // the wall-free body and gains nothing -- 0.1301 against 0.1282 ms per sweep, round 3: the other waves of the SIMD fill
    // those slots.)
    auto relax4 = [&](const T (&cc)[4], T left, T right, const T (&ym)[4], const T (&yp)[4], const T (&zm)[4],
                      const T (&zp)[4], const T (&rh)[4], T (&u)[4]) {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            T xp1 = (e < 3) ? cc[e + 1] : right;
            T xm1 = (e > 0) ? cc[e - 1] : left;
            T nb = xp1 + xm1 + yp[e] + ym[e] + (ZREV ? zm[e] : zp[e]) + (ZREV ? zp[e] : zm[e]);   // (real z+1 first)
            u[e] = (rh[e] + a * nb) * inv_c;
        }
    };
    // what setBounds leaves in memory for the lane's four cells of an interior row.  Most waves
    // have no solid cell anywhere near: they skip the zeroing logic on one wave-uniform test.
    auto settle4 = [&](const T (&u)[4], unsigned fl, T (&st)[4]) {
        if constexpr (MF) {
#pragma unroll
            for (int e = 0; e < 4; ++e) st[e] = u[e];
            return;
        }
        const unsigned kb = (fl >> kill_shift) & 15u;
        if (ALIGNED && __builtin_amdgcn_ballot_w64(kb != 0) == 0) {
#pragma unroll
            for (int e = 0; e < 4; ++e) st[e] = u[e];
            return;
        }
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const bool kill = ((kb >> e) & 1u) != 0;
            if (ALIGNED) st[e] = kill ? zero : u[e];
            else {
                const int x = x0 + e;
                T ghost_src = (e > 0) ? u[e - 1] : zero;
                st[e] = (x <= W) ? (kill ? zero : u[e]) : ((x == W + 1) ? ghost_src : zero);
            }
        }
    };
    auto lds_get = [&](const T* rowp, T (&out)[4]) {
        V4<T> q = *reinterpret_cast<const V4<T>*>(rowp);
#pragma unroll
        for (int e = 0; e < 4; ++e) out[e] = q.e[e];
    };
    auto lds_set = [&](T* rowp, const T (&in)[4]) {
        V4<T> q;
#pragma unroll
        for (int e = 0; e < 4; ++e) q.e[e] = in[e];
        *reinterpret_cast<V4<T>*>(rowp) = q;
    };
    auto face4 = [&](const T (&u)[4], bool negate, T (&out)[4]) {
#pragma unroll
        for (int e = 0; e < 4; ++e) out[e] = (ALIGNED || x0 + e <= W) ? (negate ? -u[e] : u[e]) : zero;
    };
    // publish a freshly computed row of level RG+1: the settled cells plus the ghosts its setBounds writes
    auto publish = [&](auto rgc, int P, int r, const T (&u)[4], const T (&st)[4]) {
        constexpr int RG = decltype(rgc)::value;
        const int y = y0 + r, t = ty0 + r;
        T(*tl)[TW] = ring[RG][P & 1];
        lds_set(&tl[t][x0 + 3], st);
        if (x0 == 1) tl[t][3] = (b == 1) ? -u[0] : u[0];                                          // :189-190
        if (full_group && x0 + 3 == W) tl[t][W + 4] = u[3];                                       // :191
        if (WALLS && (y == 1 || y == H)) {
            T f[4];
            face4(u, b == 2, f);
            if (y == 1 && t >= 1) lds_set(&tl[t - 1][x0 + 3], f);                                  // :198-199
            if (y == H && t + 1 < BY) lds_set(&tl[t + 1][x0 + 3], f);                              // :200-201
        }
    };

    // level j+1 of plane P, row r, from the wave's level-j registers (planes P-1, P, P+1) and the
    // level-j tile of plane P in LDS (x neighbours, and the y neighbours the wave does not own)
    auto next_row = [&](auto rgc, int P, int r, const T (&s0)[RY][4], const T (&s1)[RY][4], const T (&s2)[RY][4],
                        const T (&rh)[4], T (&u)[4]) {
        constexpr int RG = decltype(rgc)::value;
        const int y = y0 + r, t = ty0 + r;
        T(*tl)[TW] = ring[RG][P & 1];
        T left, right;
        if constexpr (XS) {                              // lane 0's left / lane 63's right: one address per half-wave
            const T edge = tl[t][xe];
            left = lane_from_left(s1[r][3], edge);
            right = lane_from_right(s1[r][0], edge);
        } else {
            left = tl[t][x0 + 2];                        // neighbour lane's / wave's cell, or the ghost column x = 0
            right = tl[t][x0 + 7];                       // ... or the ghost column x = W+1
        }
        T ym[4], yp[4];
        if (r > 0 && (!WALLS || y != 1)) {
#pragma unroll
            for (int e = 0; e < 4; ++e) ym[e] = s1[r > 0 ? r - 1 : 0][e];
        } else lds_get(&tl[t - 1][x0 + 3], ym);          // another wave's row, or the ghost row y = 0
        if (r < RY - 1 && (!WALLS || y != H)) {
#pragma unroll
            for (int e = 0; e < 4; ++e) yp[e] = s1[r < RY - 1 ? r + 1 : r][e];
        } else lds_get(&tl[t + 1][x0 + 3], yp);          // another wave's row, or the ghost row y = H+1
        relax4(s1[r], left, right, ym, yp, s0[r], s2[r], rh, u);
    };

    // final level: the stores of the sweep plus those of its setBounds
    auto store_final = [&](int zo, int r, const T (&u)[4], unsigned fl) {
        const int y = y0 + r;
        T st[4];
        settle4(u, fl, st);
        char* base = reinterpret_cast<char*>(dst) + zorg_b + (long)zo * zdir_b + oc[r];
        // z-slab push exchange: the planes the neighbours need next also go straight into their halo planes (wave-uniform)
        const long dl = (SLAB && zo <= pp.planes) ? pp.lo : 0, dh = (SLAB && zo > D - pp.planes) ? pp.hi : 0;
        if (FS_EXP_NT & 2) {
            Vec4<T> q;
#pragma unroll
            for (int e = 0; e < 4; ++e) q[e] = st[e];
            __builtin_nontemporal_store(q, reinterpret_cast<Vec4<T>*>(base));
        } else {
            V4<T> q;
#pragma unroll
            for (int e = 0; e < 4; ++e) q.e[e] = st[e];
            put<SLAB>(reinterpret_cast<V4<T>*>(base), q, dl, dh);
        }
        if (x0 == 1) put<SLAB>(reinterpret_cast<T*>(base - ES), (b == 1) ? -u[0] : u[0], dl, dh);   // :189-190
        if (full_group && x0 + 3 == W) put<SLAB>(reinterpret_cast<T*>(base + 4 * ES), u[3], dl, dh);   // :191
        if (WALLS && (y == 1 || y == H)) {
            T f[4];
            V4<T> qq;
            face4(u, b == 2, f);
#pragma unroll
            for (int e = 0; e < 4; ++e) qq.e[e] = f[e];
            if (y == 1) put<SLAB>(reinterpret_cast<V4<T>*>(base - row_b), qq, dl, dh);               // :198-201
            if (y == H) put<SLAB>(reinterpret_cast<V4<T>*>(base + row_b), qq, dl, dh);
        }
        const bool zlo_face = (zo == 1) && lo_wall_c, zhi_face = (zo == D) && hi_wall_c;
        if (zlo_face || zhi_face) {
            T f[4];
            V4<T> qq;
            face4(u, b == 3, f);
#pragma unroll
            for (int e = 0; e < 4; ++e) qq.e[e] = f[e];
            if (zlo_face) *reinterpret_cast<V4<T>*>(base - zdir_b) = qq;                            // :208-214
            if (zhi_face) *reinterpret_cast<V4<T>*>(base + zdir_b) = qq;
        }
    };

    // One step of the march.  PH: which register slot is which plane (rotates with period 3).
    auto iter = [&](auto phc, int zl) {
        constexpr int PH = decltype(phc)::value;
        constexpr int I0 = PH, I1 = (PH + 1) % 3, I2 = (PH + 2) % 3;
        // level-0 planes zl-1, zl, zl+1 sit in L0[I0], L0[I1], L0[I2]; level j planes
        // p-1, p (and the one computed now, p+1) in Lj[I0], Lj[I1], Lj[I2]
        // The row offsets are made opaque once per iteration: otherwise loop strength reduction folds
        // each (plane pointer + row offset) into its own 64-bit vector induction variable -- two VGPRs
        // per access kept across the loop -- instead of a scalar base plus this 32-bit offset.
#pragma unroll
        for (int r = 0; r < RY; ++r) asm volatile("" : "+v"(oc[r]));
        // the rhs ring: NL = 3 rotates with the register slots (compile-time slot), NL = 2 by plane parity
        T(*rs_put)[RW] = rsave[(NL == 3) ? PH : (zl & 1)];
        T(*rs_get2)[RW] = rsave[(NL == 3) ? I2 : ((zl - 1) & 1)];
        const bool wall_lo1 = (zl == 1) && lo_wall_c, wall_hi1 = (zl == D) && hi_wall_c;
        if (zl <= hi1) {                                 // ---- level 1 of plane zl
#pragma unroll
            for (int r = 0; r < RY; ++r) {
                const int y = y0 + r, t = ty0 + r;
                const bool row_on = (y >= 1) && (y <= H);     // wave-uniform
                if (row_on && lane_on) {
                    T ym[4], yp[4], u[4];
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        ym[e] = (r > 0) ? L0[I1][r > 0 ? r - 1 : 0][e] : hb[e];
                        yp[e] = (r < RY - 1) ? L0[I1][r < RY - 1 ? r + 1 : r][e] : ht[e];
                    }
                    T left = eL[r], right = eR[r];
                    if constexpr (XS && !Z0) {
                        left = lane_from_left(L0[I1][r][3], eL[r]);
                        right = lane_from_right(L0[I1][r][0], eR[r]);
                    }
                    relax4(L0[I1][r], left, right, ym, yp, L0[I0][r], L0[I2][r], rcur[r], u);
                    settle4(u, flc[r], L1[I2][r]);
                    publish(IC<0>{}, zl, r, u, L1[I2][r]);
                    if (RS && t >= 1 && t <= BY - 2) lds_set(&rs_put[t - 1][xl], rcur[r]);
                    if (wall_lo1) face4(u, b == 3, L1[I1][r]);      // ghost plane z = 0 takes plane 0's slot, :208-210
                    if (wall_hi1) face4(u, b == 3, gz1[r]);         // ghost plane z = D+1 waits for its slot, :212-214
                }
                if constexpr (!MF) kl[PH][r] = flc[r];
            }
        }
        // next plane's level-0 data, one iteration ahead.  Unconditional (a conditional load merges
        // with the old register contents, and the merge waits for the load); past the last plane the
        // same plane is fetched again and never used.
        // lean variant: the right-hand sides of the two older planes, issued BEFORE the prefetch (memory returns in order:
        // a wait for these must not wait for the next plane's loads as well)
        T rh2[RS ? 1 : RY][4], rh3[RS ? 1 : RY][4];
        if constexpr (!RS) {
            const char* rp2 = plane_of(rhs, max(zl - 1, lo1));
            const char* rp3 = plane_of(rhs, max(zl - 2, lo1));
#pragma unroll
            for (int r = 0; r < RY; ++r) { ld4(rp2 + oc[r], rh2[r]); ld4(rp3 + oc[r], rh3[r]); }
        }
        __builtin_amdgcn_sched_barrier(0);               // pin the loads here: left alone, the scheduler sinks them to the
        load_core(min(zl + 2, zmax0), L0[I0]);           // end of the iteration to shorten live ranges, and the next
        load_side(min(zl + 1, zmax1));                   // iteration then starts by waiting a full memory latency
        asm volatile("" ::: "memory");                   // (the IR-level sink pass does the same across blocks)
        __builtin_amdgcn_sched_barrier(0);
        const int P2 = zl - 1;
        const bool wall_lo2 = (P2 == 1) && lo_wall_c, wall_hi2 = (P2 == D) && hi_wall_c;
        if constexpr (NL == 3) {
            if (P2 >= lo2 && P2 <= hi2) {                // ---- level 2 of plane zl-1 (intermediate)
#pragma unroll
                for (int r = 0; r < RY; ++r) {
                    const int y = y0 + r, t = ty0 + r;
                    if (y >= r2lo && y <= r2hi) {        // wave-uniform
                        T rh[4], u[4];
                        if constexpr (RS) lds_get(&rs_get2[t - 1][xl], rh);
                        else {
#pragma unroll
                            for (int e = 0; e < 4; ++e) rh[e] = rh2[r][e];
                        }
                        next_row(IC<0>{}, P2, r, L1[I0], L1[I1], L1[I2], rh, u);
                        if (lane_on) {
                            settle4(u, kl[I2][r], L2[I2][r]);
                            publish(IC<NL - 2>{}, P2, r, u, L2[I2][r]);
                            if (wall_lo2) face4(u, b == 3, L2[I1][r]);
                            if (wall_hi2) face4(u, b == 3, gz2[r]);
                        }
                    }
                }
            }
        } else {
            if (P2 >= zbeg && P2 <= zend) {              // ---- level 2 of plane zl-1 (final)
#pragma unroll
                for (int r = 0; r < RY; ++r) {
                    const int y = y0 + r, t = ty0 + r;
                    if (y >= r2lo && y <= r2hi) {
                        T rh[4], u[4];
                        lds_get(&rs_get2[t - 1][xl], rh);
                        next_row(IC<0>{}, P2, r, L1[I0], L1[I1], L1[I2], rh, u);
                        if (lane_on) store_final(P2, r, u, kl[I2][r]);
                    }
                }
            }
        }
        if (wall_hi1) {                                  // level 1's oldest slot is free now: it becomes plane D+1
#pragma unroll
            for (int r = 0; r < RY; ++r)
#pragma unroll
                for (int e = 0; e < 4; ++e) L1[I0][r][e] = gz1[r][e];
        }
        if constexpr (NL == 3) {
            const int P3 = zl - 2;
            if (P3 >= zbeg && P3 <= zend) {              // ---- level 3 of plane zl-2
#pragma unroll
                for (int r = 0; r < RY; ++r) {
                    const int y = y0 + r, t = ty0 + r;
                    if (y >= r3lo && y <= r3hi) {
                        T rh[4], u[4];
                        if constexpr (RS) lds_get(&rsave[I1][t - 1][xl], rh);
                        else {
#pragma unroll
                            for (int e = 0; e < 4; ++e) rh[e] = rh3[r][e];
                        }
                        next_row(IC<NL - 2>{}, P3, r, L2[I0], L2[I1], L2[I2], rh, u);
                        if (lane_on) store_final(P3, r, u, kl[I1][r]);
                    }
                }
            }
            if (wall_hi2) {
#pragma unroll
                for (int r = 0; r < RY; ++r)
#pragma unroll
                    for (int e = 0; e < 4; ++e) L2[I0][r][e] = gz2[r][e];
            }
        }
        __syncthreads();
    };

    if (z_from == lo1) {                                 // the march starts here: first loads
        load_core(lo1 - 1, L0[0]);
        load_core(lo1, L0[1]);
        load_core(min(lo1 + 1, zmax0), L0[2]);
        load_side(lo1);
    }
    int zl = z_from;
    for (int k = 0; k < ngroups; ++k) {
        iter(IC<0>{}, zl);
        iter(IC<1>{}, zl + 1);
        iter(IC<2>{}, zl + 2);
        zl += 3;
    }
    if (zl <= tail_to) {
        iter(IC<0>{}, zl);
        if (zl + 1 <= tail_to) iter(IC<1>{}, zl + 1);
    }
    if (MF && ngroups > 0) {                             // what a masked body that follows reads of planes z_from + 3 ngroups - 2 ..
#pragma unroll                                           // + 3 ngroups: clean, so all 0
        for (int r = 0; r < RY; ++r) {
            flc[r] = 0u;
#pragma unroll
            for (int q = 0; q < 3; ++q) kl[q][r] = 0u;
        }
    }
    };
    const int zl_end = zend + OV;                        // the march: iterations lo1 .. zl_end
    const int total = zl_end - lo1 + 1, ngroups = total / 3;
    if constexpr (WALLSEL == 1 || WALLSEL == 3) {
        // Two bodies.  A band at a y wall runs the general one throughout (and is the lighter band, see `s`).  Any other band
        // needs it only where a level touches a physical z wall: the iterations up to NL (plane 1 as level 1 .. NL) and those
        // from D on; the groups of three iterations that contain none of those run the wall-free body.
        const bool ywall = (s <= 0) || (s + BY - 1 >= H + 1);
        // groups [0, g0) general, [g0, g1) wall-free, [g1, ngroups) + tail general
        int g0 = ngroups, g1 = ngroups;
        if (!ywall) {
            g0 = (lo_wall && lo1 <= NL) ? min(ngroups, (NL - lo1) / 3 + 1) : 0;
            g1 = hi_wall ? max(g0, min(ngroups, (D - lo1) / 3)) : ngroups;     // group k covers lo1 + 3k .. lo1 + 3k + 2 < D
        }
        run(IC<1>{}, lo1, g0, -1);
        if constexpr (WALLSEL == 1) run(IC<0>{}, lo1 + 3 * g0, g1 - g0, -1);
        else {
            // mask-free build: the wall-free groups run mask-free [g0, ga), wall-free [ga, gb), mask-free [gb, g1), the split the
            // host made from the clean table (chunk_plan.h).  (Bodies alternating inside a loop spill at the loop's merge: 168
            // VGPRs + 372 B of scratch, against 150 and none for these three straight-line runs.)
            const int ga = plan[2], gb = plan[3];
            run(IC<2>{}, lo1 + 3 * g0, ga - g0, -1);
            run(IC<0>{}, lo1 + 3 * ga, gb - ga, -1);
            run(IC<2>{}, lo1 + 3 * gb, g1 - gb, -1);
        }
        run(IC<1>{}, lo1 + 3 * g1, ngroups - g1, zl_end);
    } else {
        run(IC<WALLSEL == 2 ? 0 : 1>{}, lo1, ngroups, zl_end);
    }
}

// ---------------------------------------------------------------------------------------------
// launch plans
// ---------------------------------------------------------------------------------------------
// The mask-free build's per-workgroup table of one launch shape on the device: made and uploaded at its first launch after a mask
// change (host work and one upload, no wait on the device), then reused.  z chunks balanced per band by `cost`, or equal ones of
// zc_len planes when it is off.  (inline: a slice without a three-sweep build does not call it)
// zrev: the table of a reversed pass -- the same, in its logical planes, from the z-mirrored clean table.
inline const int* mask_free_plan(hipStream_t st, MaskPlan& mp, const ChunkCost& cost, const GridDesc& g, int BY, int nbands,
                                 int nzc, int zc_len, bool zrev)
{
    const bool bal = cost.general > 0;
    for (const MaskPlan::Chunks& c : mp.chunks)
        if (c.BY == BY && c.nbands == nbands && c.nzc == nzc && c.zc_len == (bal ? 0 : zc_len) && c.zrev == zrev &&
            c.cost.general == cost.general && c.cost.wall_free == cost.wall_free && c.cost.mask_free == cost.mask_free)
            return c.dev;
    if (zrev && mp.host_rev.empty()) mp.host_rev = mirrored_clean(mp.host, mp.words, g.D);
    const std::vector<uint32_t>& tab = zrev ? mp.host_rev : mp.host;
    std::vector<int> chunks;
    if (bal) chunks = balanced_chunks(tab, mp.words, g.H, g.D, BY, nbands, nzc, cost);
    else
        for (int zc = 0; zc < nzc; ++zc)
            for (int band = 0; band < nbands; ++band) {
                chunks.push_back(1 + zc * zc_len);
                chunks.push_back(std::min(g.D, zc * zc_len + zc_len));
            }
    MaskPlan::Chunks c{BY, nbands, nzc, bal ? 0 : zc_len, zrev, cost, mask_free_plan(tab, mp.words, g.H, g.D, BY, nbands, chunks), nullptr};
    if (hipMalloc((void**)&c.dev, c.plan.size() * sizeof(int)) != hipSuccess) return nullptr;
    mp.chunks.push_back(std::move(c));
    MaskPlan::Chunks& k = mp.chunks.back();
    if (hipMemcpyAsync(k.dev, k.plan.data(), k.plan.size() * sizeof(int), hipMemcpyHostToDevice, st) != hipSuccess) return nullptr;
    return k.dev;
}

// One build of the kernel: all the forms of it that a launch can pick.  Explicitly instantiated per build in the slice that
// the list below assigns it to; the dispatcher reaches the other slices' through `extern template`.
template <class T, int NL, int NXW, int NYW, int RY>
void launch_fused_v(hipStream_t st, const SweepTune& tune, const GridDesc& g, const SlabCtx& sc, const T* src,
                           const T* rhs, T* dst, const uint8_t* flags, int b, T a, T inv_c, int z_first, int z_last,
                           const SweepShape& shape, int alt, int second_first, const PeerPush* push, MaskPlan* mp, bool zero_src,
                           bool zrev)
{
    const PeerPush pp = (push && second_first < 0) ? *push : PeerPush();
    constexpr int BY = NYW * RY, THREADS = NXW * NYW * 64;
    const int planes = z_last - z_first + 1;
    if (planes <= 0) return;
    const int nbands = plan_bands(g.H, shape);
    const bool aligned = (g.W == NXW * 256);
    const bool whole = sc.lo_wall && sc.hi_wall && z_first == 1 && z_last == g.D && second_first < 0;
    int zc_len, z_stride, nblk;
    if (second_first >= 0) {
        // two equally long ranges (the slab's two boundary regions) as two chunks of one launch
        zc_len = planes;
        z_stride = second_first - z_first;
        z_last = second_first + planes - 1;
        nblk = nbands * 2;
    } else {
        // z chunks re-read 2 NL level-0 planes and recompute the levels below the last on 2(NL-1) + ... planes
        // (launch_plan.h: chunk_len)
        const SweepKernel kind = NL == 3 ? SweepKernel::Three : SweepKernel::Fused2;
        const int slots = tune.cu_slots > 0 ? tune.cu_slots : 256;
        zc_len = chunk_len(planes, nbands, alt, chunk_min_len(kind), chunk_overlap(kind, NL), slots);
        if (tune.pair_zc > 0) zc_len = tune.pair_zc < planes ? tune.pair_zc : planes;
        const int nzc = (planes + zc_len - 1) / zc_len;
        z_stride = zc_len;
        nblk = nbands * nzc;
    }
    // whole-domain, lane-aligned rows (the benchmark grids) get the build without any slab logic; everything
    // else the general one
    CleanArgs ca;
#define FS_LAUNCH(AL, SL, WS)                                                                                            \
    hipLaunchKernelGGL((jacobi_fused_kernel<T, NL, NXW, NYW, RY, AL, SL, WS>), dim3(nblk), dim3(THREADS), 0, st, g, sc, src, \
                       rhs, dst, flags, b, a, inv_c, z_first, z_last, zc_len, z_stride, nbands, nblk, pp, ca)
    // the same launch with the zero-start form of the kernel: same plan, same workgroups, `src` not read
#define FS_LAUNCH_Z0(WS)                                                                                                  \
    hipLaunchKernelGGL((jacobi_fused_kernel<T, NL, NXW, NYW, RY, true, false, WS, true>), dim3(nblk), dim3(THREADS), 0, st, g, sc, \
                       src, rhs, dst, flags, b, a, inv_c, z_first, z_last, zc_len, z_stride, nbands, nblk, pp, ca)
    // ... and with the reversed march: the same launch of the z-mirrored problem (chunks and plan in logical planes)
#define FS_LAUNCH_ZREV(WS)                                                                                                \
    hipLaunchKernelGGL((jacobi_fused_kernel<T, NL, NXW, NYW, RY, true, false, WS, false, true>), dim3(nblk), dim3(THREADS), 0, st, g, \
                       sc, src, rhs, dst, flags, b, a, inv_c, z_first, z_last, zc_len, z_stride, nbands, nblk, pp, ca)
    // the reversed builds: rows of two waves (512 cells), where the three arrays of a solve outgrow the Infinity Cache
    constexpr bool HAS_ZREV = (NL == 3 && NXW == 2 && sizeof(T) == 4);
    zrev = zrev && HAS_ZREV && !zero_src;
    // The wall-free second body exists for the three-sweep kernel on lane-aligned whole-domain grids (the benchmark grids).
    // Rounds 1-2 selected a body per WORKGROUP: 9 % (512^3) to 14 % (256^3) faster for the interior ones, but a pass ends with its
    // slowest workgroup, and at 512^3 (256 workgroups, one per CU) half of them touch a z wall.  Round 3 selects per GROUP OF
    // THREE PLANE ITERATIONS instead (only the first and last groups of a z-wall chunk run the general body) and shifts the band
    // origin so that the two y-wall bands, which run it throughout, carry one row less per level: 0.1448 -> 0.1371 ms per sweep
    // at 512^3 on one box, 0.1380 -> 0.1282 on another, 0.0172 -> 0.0166 at 256^3 (profiles/r3y_*); letting the y-wall bands
    // run the wall-free body too (timing only) changes nothing any more, so "auto" now means always.
    const bool two_bodies = tune.wall_free >= 1;
    if constexpr (NL == 3) {                             // (the two-body builds exist for three sweeps only)
        if (aligned && two_bodies) {
            // mask_free "auto": rows of two waves only -- on 256-cell rows (c2) this build measured slower (4.70 -> 4.81 ms per step)
            const bool mask_free = tune.mask_free >= 2 || (tune.mask_free == 1 && NXW >= 2);
            if (whole && mask_free && mp && !mp->host.empty() &&
                (ca.plan = mask_free_plan(st, *mp, tune.chunk_cost, g, BY, nbands, nblk / nbands, zc_len, zrev && whole))) {
                // the mask-free build, on z chunks balanced per band unless the cost model is off
                if constexpr (sizeof(T) == 4) {
                    if (zero_src) { FS_LAUNCH_Z0(3); return; }
                }
                if constexpr (HAS_ZREV) {
                    if (zrev) { FS_LAUNCH_ZREV(3); return; }
                }
                FS_LAUNCH(true, false, 3);
            } else if (whole) {
                if constexpr (sizeof(T) == 4) {
                    if (zero_src) { FS_LAUNCH_Z0(1); return; }
                }
                if constexpr (HAS_ZREV) {
                    if (zrev) { FS_LAUNCH_ZREV(1); return; }
                }
                FS_LAUNCH(true, false, 1);
            } else FS_LAUNCH(true, true, 1);             // z-slabs: an inner rank has no z wall at all
            return;
        }
    }
    if (aligned && whole) FS_LAUNCH(true, false, 0);
    else if (aligned) FS_LAUNCH(true, true, 0);
    else FS_LAUNCH(false, true, 0);
#undef FS_LAUNCH
#undef FS_LAUNCH_Z0
#undef FS_LAUNCH_ZREV
}

// ---------------------------------------------------------------------------------------------
// The builds of jacobi_fused_kernel (launch_plan.h: SHAPE_TABLE says which row widths and shape ids reach them), written once
// and grouped by the slice that compiles them.  The device compiler works through one translation unit on one thread, a
// three-sweep fp32 build (eight forms of the kernel, ten with the reversed march) costs it 22 to 35 s and a two-sweep or fp64
// build (three forms) 4 to 6 s, so the Makefile compiles this file once per slice (-DFS_FUSED_SLICE=<k> -> sweep_fused_<k>.o)
// and the slices build side by side.
// X(T, NL, NXW, NYW, RY); SEP() stands between two entries.  A slice holds one element type.  DESIGN.md section 6 has the
// measured compile time of each build and slice, from which this assignment comes.  A new slice also goes into FUSED_SLICES
// of the Makefile.
// ---------------------------------------------------------------------------------------------
#ifndef FS_FUSED_SLICE
#error "sweep_fused.hip is compiled in slices: -DFS_FUSED_SLICE=<k>, one object per slice (see the Makefile)"
#endif
#define FS_FUSED_SLICE_0(X, SEP) X(float, 3, 1, 10, 2) SEP() X(float, 2, 4, 3, 3)
#define FS_FUSED_SLICE_1(X, SEP) X(float, 3, 1, 8, 2) SEP() X(float, 2, 3, 4, 2)
#define FS_FUSED_SLICE_2(X, SEP) X(float, 3, 1, 6, 2) SEP() X(float, 2, 4, 4, 2)
#define FS_FUSED_SLICE_3(X, SEP) X(float, 3, 2, 6, 2)
#define FS_FUSED_SLICE_4(X, SEP) X(float, 3, 2, 5, 2)
#define FS_FUSED_SLICE_5(X, SEP) X(double, 2, 1, 10, 2) SEP() X(double, 2, 2, 5, 2) SEP() X(double, 2, 2, 4, 2)
#define FS_FUSED_BUILDS_F32(X, SEP) \
    FS_FUSED_SLICE_0(X, SEP) SEP() FS_FUSED_SLICE_1(X, SEP) SEP() FS_FUSED_SLICE_2(X, SEP) SEP() FS_FUSED_SLICE_3(X, SEP) SEP() FS_FUSED_SLICE_4(X, SEP)
#define FS_FUSED_BUILDS_F64(X, SEP) FS_FUSED_SLICE_5(X, SEP)
#define FS_COMMA() ,
#define FS_NOTHING()
#define FS_PASTE_(a, b) a##b
#define FS_PASTE(a, b) FS_PASTE_(a, b)

#define FS_AS_BUILD(T, NL, NXW, NYW, RY) Build<NL, NXW, NYW, RY>
using FusedBuildsF32 = Builds<FS_FUSED_BUILDS_F32(FS_AS_BUILD, FS_COMMA)>;
using FusedBuildsF64 = Builds<FS_FUSED_BUILDS_F64(FS_AS_BUILD, FS_COMMA)>;
static_assert(FusedBuildsF32::covers(4, SweepKernel::Three) && FusedBuildsF32::covers(4, SweepKernel::Fused2) &&
                  FusedBuildsF64::covers(8, SweepKernel::Fused2) && FusedBuildsF64::covers(8, SweepKernel::Three),
              "a fused-kernel shape of SHAPE_TABLE has no build here");

// every build is declared as instantiated elsewhere; then this slice's own are instantiated (a build that is in the lists but
// in no compiled slice fails to link)
#define FS_INSTANTIATE(T, NL, NXW, NYW, RY)                                                                                    \
    template void launch_fused_v<T, NL, NXW, NYW, RY>(hipStream_t, const SweepTune&, const GridDesc&, const SlabCtx&, const T*, \
                                                      const T*, T*, const uint8_t*, int, T, T, int, int, const SweepShape&, int, \
                                                      int, const PeerPush*, MaskPlan*, bool, bool);
#define FS_DECLARE(T, NL, NXW, NYW, RY) extern FS_INSTANTIATE(T, NL, NXW, NYW, RY)
FS_FUSED_BUILDS_F32(FS_DECLARE, FS_NOTHING)
FS_FUSED_BUILDS_F64(FS_DECLARE, FS_NOTHING)
FS_PASTE(FS_FUSED_SLICE_, FS_FUSED_SLICE)(FS_INSTANTIATE, FS_NOTHING)

// ---------------------------------------------------------------------------------------------
// What exists once, in slice 0: the MaskPlan members, the zero-start query and the dispatchers
// ---------------------------------------------------------------------------------------------
#if FS_FUSED_SLICE == 0
void MaskPlan::clear_chunks()
{
    for (Chunks& c : chunks) hipFree(c.dev);
    chunks.clear();
    host_rev.clear();
}
void MaskPlan::release()
{
    clear_chunks();
    if (tab) hipFree(tab);
    tab = nullptr;
    host.clear();
}

// Whether a whole-range launch of the three-sweep kernel with this plan reaches a build that has the zero-start form: the
// conditions launch_fused_v tests on its way to FS_LAUNCH_Z0 (fp32, lane-aligned rows of 256 or 512 cells, whole domain, the
// two-body builds), asked by the host before it decides not to zero the iterate in memory.
bool jacobi_fused_zero_start(const SweepTune& tune, const GridDesc& g, const SlabCtx& sc, int elem_size, int plan)
{
    if (elem_size != 4 || plan < 0 || tune.abl == 16 || tune.wall_free < 1 || !sc.lo_wall || !sc.hi_wall || g.D < 1) return false;
    const SweepShape* shape = launch_shape(4, SweepKernel::Three, g.W, decode_plan(true, plan).shape);
    return shape && shape->NL == 3 && g.W == shape->NXW * 256;
}

// The same question for the reversed march (launch_fused_v: HAS_ZREV and the way to FS_LAUNCH_ZREV): rows of 512 cells only.
bool jacobi_fused_reversed(const SweepTune& tune, const GridDesc& g, const SlabCtx& sc, int elem_size, int plan)
{
    if (!jacobi_fused_zero_start(tune, g, sc, elem_size, plan)) return false;
    const SweepShape* shape = launch_shape(4, SweepKernel::Three, g.W, decode_plan(true, plan).shape);
    return shape->NXW == 2;
}

// plan = the three-sweep id (levels == 3) or the two-sweep id of the fused kernel (levels == 2); < 0: plan 0.  All plans give
// the same bits, the host driver times them once per grid.
template <class T>
void launch_jacobi_fused(hipStream_t st, const SweepTune& tune, const GridDesc& g, const SlabCtx& sc, int levels, const T* src,
                         const T* rhs, T* dst, const uint8_t* flags, int b, T a, T inv_c, int z_first, int z_last, int plan,
                         int second_first, const PeerPush* push, MaskPlan* mp, bool zero_src, bool zrev)
{
    const PlanId p = decode_plan(levels == 3, plan);
    const SweepKernel kind = levels == 3 ? SweepKernel::Three : SweepKernel::Fused2;
    if constexpr (sizeof(T) == 4) {
        if (levels == 3 && tune.abl == 16 && g.W == 512 && sc.lo_wall && sc.hi_wall && z_first == 1 && z_last == g.D && second_first < 0) {
            // EXPERIMENT, timing only (wrong at the walls): every workgroup runs the lean interior body in 16-row bands
            const int nbands = plan_bands(g.H, SweepShape{3, 2, 8, 2});
            const int nzc = p.alt == 0 ? 5 : p.alt == 1 ? 6 : 4;
            const int zc_len = (g.D + nzc - 1) / nzc, nblk = nbands * nzc;
            hipLaunchKernelGGL((jacobi_fused_kernel<float, 3, 2, 8, 2, true, false, 2>), dim3(nblk), dim3(1024), 0, st, g, sc, src, rhs, dst, flags,
                               b, a, inv_c, z_first, z_last, zc_len, zc_len, nbands, nblk, PeerPush(), CleanArgs());
            return;
        }
    }
    const SweepShape* shape = launch_shape(sizeof(T), kind, g.W, p.shape);
    if (!shape) return;                                  // no such kernel for this row width: plan_supported is false
    using List = std::conditional_t<sizeof(T) == 4, FusedBuildsF32, FusedBuildsF64>;
    List::run(*shape, [&](auto build) {
        using B = decltype(build);
        launch_fused_v<T, B::NL, B::NXW, B::NYW, B::RY>(st, tune, g, sc, src, rhs, dst, flags, b, a, inv_c, z_first, z_last, *shape,
                                                        p.alt, second_first, push, sizeof(T) == 4 ? mp : nullptr, zero_src, zrev);
    });
}
template void launch_jacobi_fused<float>(hipStream_t, const SweepTune&, const GridDesc&, const SlabCtx&, int, const float*,
                                         const float*, float*, const uint8_t*, int, float, float, int, int, int, int,
                                         const PeerPush*, MaskPlan*, bool, bool);
template void launch_jacobi_fused<double>(hipStream_t, const SweepTune&, const GridDesc&, const SlabCtx&, int, const double*,
                                          const double*, double*, const uint8_t*, int, double, double, int, int, int, int,
                                          const PeerPush*, MaskPlan*, bool, bool);
#endif  // FS_FUSED_SLICE == 0

}  // namespace fs
