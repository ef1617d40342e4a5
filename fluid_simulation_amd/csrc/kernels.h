// kernels.h -- launch interface between the host driver (fluidsim.cpp) and the gfx950
// kernels (kernels.hip, sweep_fused.hip, project.hip, advect.hip, fields.hip, voxelize.hip).  Internal to libfluidsim.so.
#pragma once
#include "chunk_plan.h"
#include "launch_plan.h"
#include <hip/hip_runtime_api.h>
#include <cstddef>
#include <cstdint>

namespace fs {

// HBM layout of one field (DESIGN.md "Data layout").  Element (x,y,z), 0 <= x <= W+1 etc,
// lives at p[x + y*sy + z*sz] where p is the allocation base shifted by LEAD elements, so
// that the first interior cell of every row (x = 1) is 16-byte aligned and a lane can
// move its four x-consecutive cells with one dwordx4.  sy is a multiple of 4.
struct GridDesc {
    int W, H, D;   // interior extents of THIS slab (D = local planes under z-slab partitioning)
    long sy, sz;   // row and plane pitch in elements
    long n;        // elements per allocation (including `lead` and the tail pad)
    long lead;     // elements between the allocation base and p: LEAD + (zh-1) planes
    int zh;        // halo planes kept on each z side: 1 (single GPU), 2 or 3 (z-slabs: planes 1-zh..D+zh
                   // exist so that two / three fused sweeps can cross a slab boundary)
};
constexpr int LEAD = 3;

// per-cell flag byte, same indexing as a field
enum : unsigned {
    F_SOLID = 1u,        // obs == 1                              (simulation.cpp:222)
    F_NEAR = 2u,         // fluid cell with an in-range solid 6-neighbour (simulation.cpp:232-238)
    F_XP = 4u, F_XM = 8u, F_YP = 16u, F_YM = 32u, F_ZP = 64u, F_ZM = 128u   // neighbour in range and obs == 0 (simulation.cpp:307-312)
};

// z-slab context: global z of local plane 1 is zoff+1; the physical z walls exist only on
// the first / last slab.
struct SlabCtx {
    int zoff;       // global index offset of this slab's planes
    int Dglobal;    // global depth
    int lo_wall;    // 1 if local plane 0 is the physical z=0 ghost plane
    int hi_wall;    // 1 if local plane D+1 is the physical z=Dglobal+1 ghost plane
};

// Tunables of the sweep launch (set through fs_set_option "sweep_ry" / "sweep_zc" /
// "sweep_blocks"; "sweep_abl" selects timing-only ablation builds used by tools/tune_sweep.py).
// One instance per handle (fs_sim::tune): options never leak between handles or host threads.
struct SweepTune {
    int ry = 2;               // rows per wave patch of the single-sweep kernel: 2 or 4
    int zc_len = 0;           // planes per z chunk; 0 = derive from target_blocks
    int target_blocks = 2048; // aim for about this many workgroups per launch
    int abl = 0;
    int cu_slots = 256;       // CUs a launch of this handle can fill (fewer when the compute stream carries a CU mask, z-slabs with
                              // "comm_cus"): what the launchers' z-chunk models divide the workgroups over
    int fuse = 3;             // sweeps fused per pass over memory: 1 never, 2 two-sweep kernels only, 3 (default) also time the
                              // three-sweep kernel per grid and use it where a sweep costs less, 4 use it wherever it exists
    int pair_zc = 0;          // planes per z chunk of the pair kernel; 0 = automatic
    int project_cell = 0;     // 1 = per-cell divergence/gradient kernels instead of the z-marching ones
    int vortex_ry = 2;        // rows per wave of the vortex kernel (vortex.hip): 1 or 2; speed only, every bit is the same
    int pair_shape = 0;       // >0 forces a pair-kernel workgroup shape (1 = 8, 2 = 10, 3 = 16 waves); 0 = timed choice
    int advect_cell = 1;      // 1 (default) = per-cell advection kernels; 2 = the same with clamp tables; 3 = the tile kernels (clamp
                              // tables staged in LDS, for rough flows; single GPU, else as 2); 0 = the row kernels (four
                              // cells per lane + clamp tables); bit-identical, within 5 % of each other (profiles/r03e_*, r02g_*)
    int advect_window = 24;   // advect_cell == 3 (the tile kernels): rows / planes around a tile whose inlet-table values are staged in
                              // LDS; a trace that ends further away takes the per-cell path (capped by what 64 KB of LDS hold)
    int wall_free = 1;        // three-sweep kernel, whole-domain aligned grids: plane iterations that touch no y / z wall run a wall-free
                              // second body -- 0 never, 1 (default) and 2 always (round 3: selected per group of three iterations)
    int two_kind = 0;         // which two-sweep kernel: 0 = timed choice, 1 = jacobi_pair_kernel only, 2 = jacobi_fused_kernel<NL=2> only
    int mask_free = 1;        // three-sweep kernel where it runs the wall-free body (single GPU): groups of plane iterations whose rows
                              // hold no kill byte run a third, mask-free body -- 0 never, 1 (default) on rows of 512 cells (two waves; it
                              // is slower on 256-cell rows), 2 always
    ChunkCost chunk_cost;     // z chunks of that build balanced per band by this cost model (chunk_plan.h); 0,0,0 (default) = equal
                              // chunks, which measured faster
};

// Single GPU: the clean table of the mask-free three-sweep build (chunk_plan.h), rebuilt with the kill bytes, and the
// per-workgroup tables derived from it on the host (one per launch shape, made at its first launch after a mask change).
struct MaskPlan {
    uint32_t* tab = nullptr;             // device staging of `host`, (D + 2) planes x `words`
    int words = 0;                       // per plane: (H + 2 + 31) / 32 rows' words + one pad word
    std::vector<uint32_t> host;          // copy of `tab`
    std::vector<uint32_t> host_rev;      // chunk_plan.h: mirrored_clean(host), made when a reversed pass first asks for a plan
    struct Chunks {
        int BY, nbands, nzc, zc_len;     // zc_len: equal chunks of that length, 0 = balanced by `cost`
        bool zrev;                       // the plan of a reversed pass: logical planes, from host_rev
        ChunkCost cost;
        std::vector<int> plan;           // chunk_plan.h: mask_free_plan
        int* dev;
    };
    std::vector<Chunks> chunks;
    void clear_chunks();                 // the mask changed
    void release();
    ~MaskPlan() { release(); }
};
void launch_build_clean(hipStream_t st, const GridDesc& g, const uint8_t* kill, uint32_t* tab, int words);

// z-slab "push" exchange (FSIPC transport, csrc/ipc.h): a solver pass stores the planes its neighbours need next straight
// into THEIR halo planes (peer-mapped arrays) beside its own -- no boundary launch, no copy, no second stream.
// lo / hi = byte offset from a cell of `dst` to the same cell of the lower / upper neighbour's copy of that plane in the
// neighbour's halo (0 = no neighbour on that side), planes = how many of the slab's outermost planes per side go over.
struct PeerPush {
    long lo = 0, hi = 0;
    int planes = 0;
};

// NOTE: the sweep launchers take the KILL-byte array (launch_build_kill), not the flag bytes.
template <class T>
void launch_jacobi(hipStream_t st, const SweepTune& tune, const GridDesc& g, const SlabCtx& sc, const T* src, const T* rhs,
                   T* dst, const uint8_t* kill, int b, T a, T inv_c, int z_first, int z_last, int second_first = -1,
                   const PeerPush* push = nullptr);
// second_first >= 0: ALSO compute the equally long range starting there, in the same launch (a
// slab's two boundary regions); push: see PeerPush (plain Jacobi passes over one range only)

// Two sweeps in one pass (temporal blocking); same result as two launch_jacobi calls.  Which grids have the kernel, and the
// halo planes a z-slab needs for it: launch_plan.h, plan_supported (current in `src`; one plane less of `rhs` and `flags`).
// plan = a two-sweep id of the pair kernel (launch_plan.h).
template <class T>
void launch_jacobi_pair(hipStream_t st, const SweepTune& tune, const GridDesc& g, const SlabCtx& sc, const T* src, const T* rhs,
                        T* dst, const uint8_t* flags, int b, T a, T inv_c, int z_first, int z_last, int plan,
                        int second_first = -1, T omega = (T)0, bool damped = false, const PeerPush* push = nullptr);
// omega != 0: one red-black SOR iteration instead; with `damped`, two Jacobi sweeps damped by omega (q + omega*(r - q))
// NL = `levels` (2 or 3) sweeps per pass, register-centred (sweep_fused.hip).  On a z-slab `src` needs `levels` current halo
// planes per side, `rhs` and `flags` levels-1.  plan = the three-sweep id, or the two-sweep id of the fused kernel;
// second_first as above.
template <class T>
void launch_jacobi_fused(hipStream_t st, const SweepTune& tune, const GridDesc& g, const SlabCtx& sc, int levels, const T* src,
                         const T* rhs, T* dst, const uint8_t* flags, int b, T a, T inv_c, int z_first, int z_last, int plan,
                         int second_first = -1, const PeerPush* push = nullptr, MaskPlan* mp = nullptr, bool zero_src = false,
                         bool zrev = false);
// mp: the single-GPU clean table (fp32 three sweeps only; nullptr = no mask-free body)
// zero_src: level 0 is all zeros and `src` is not read (the first pass of a pressure solve, whose iterate the divergence pass
// would otherwise have to zero in memory first).  Only where jacobi_fused_zero_start says the launch has such a build: the
// same launch plan, workgroups and arithmetic as the reading build, bit-identical with it on a zeroed `src`.
bool jacobi_fused_zero_start(const SweepTune& tune, const GridDesc& g, const SlabCtx& sc, int elem_size, int plan);
// zrev: the pass marches from plane D down to plane 1 (same bits; a pass after an upward one then starts on the planes the
// Infinity Cache still holds).  Only where jacobi_fused_reversed says the launch has such a build (fp32 rows of 512 cells,
// whole domain, the two-body builds), and never together with zero_src.
bool jacobi_fused_reversed(const SweepTune& tune, const GridDesc& g, const SlabCtx& sc, int elem_size, int plan);

template <class T>
void launch_gs_lex(hipStream_t st, const GridDesc& g, T* q, const T* rhs, const uint8_t* flags, int b, T a, T inv_c,
                   int sweeps);

template <class T>
void launch_set_bounds(hipStream_t st, const GridDesc& g, const SlabCtx& sc, T* q, const uint8_t* flags, int b);

template <class T>
void launch_divergence(hipStream_t st, const SweepTune& tune, const GridDesc& g, const SlabCtx& sc, const T* vx, const T* vy,
                       const T* vz, T* div, T* p, const uint8_t* flags, T mhalf_h, bool store_p = true);
// store_p = false: `p` is left as it is (the solve that follows starts from zeros it does not read, launch_jacobi_fused)

template <class T>
void launch_gradient(hipStream_t st, const SweepTune& tune, const GridDesc& g, const SlabCtx& sc, const T* p, T* vx, T* vy,
                     T* vz, const uint8_t* flags, T h, T two_h);

// `prev_zshift` = element offset added to local indices of `prev` (0 normally; under
// z-slabs `prev` is the all-gathered global array and the shift is zoff planes).
// `kill` = the kill-byte array, `coltab` = scratch for the clamp tables of the row kernels: 6 * (H+2) * (D+2)
// elements, or nullptr (no tables; also ignored on slabs).  tune.advect_cell selects the per-cell kernels.
template <class T>
void launch_advect(hipStream_t st, const SweepTune& tune, const GridDesc& g, const SlabCtx& sc, int b, T* field, const T* prev,
                   const T* vx, const T* vy, const T* vz, const uint8_t* flags, const uint8_t* kill, T* coltab, T kx, T ky, T kz,
                   long prev_zshift);

// advect(1,vx,px); advect(2,vy,py); advect(3,vz,pz) in one pass.  On a slab px/py/pz are the
// gathered global arrays and zshift the element offset of this slab's plane 0 in them.
template <class T>
void launch_advect_velocity(hipStream_t st, const SweepTune& tune, const GridDesc& g, const SlabCtx& sc, T* vx, T* vy, T* vz,
                            const T* px, const T* py, const T* pz, const uint8_t* flags, const uint8_t* kill, T* coltab, T kx,
                            T ky, T kz, long zshift);

// launch_gradient of a projection and the launch_advect_velocity that follows it in one pass (single GPU, per-cell form):
// vy, vz hold the velocities before the gradient, p the solved pressure; all three come out advected, as the two launches
// leave them.  The projected velocities themselves are not stored.
template <class T>
void launch_gradient_advect_velocity(hipStream_t st, const GridDesc& g, const SlabCtx& sc, const T* p, T* vx, T* vy, T* vz,
                                     const T* px, const T* py, const T* pz, const uint8_t* flags, T h, T two_h, T kx, T ky, T kz);

template <class T>
void launch_build_flags(hipStream_t st, const GridDesc& g, const SlabCtx& sc, const T* obs, uint8_t* flags);

// one kill byte per four cells for the sweep kernels (see kernels.hip, sweep_fused.hip); `kill` is shifted so
// that byte (cell + 3) / 4 belongs to the lane group starting at `cell`
void launch_build_kill(hipStream_t st, const GridDesc& g, const SlabCtx& sc, const uint8_t* flags, uint8_t* kill);

template <class T>
void launch_inlet_velocity(hipStream_t st, const GridDesc& g, const SlabCtx& sc, T* vx, T* vy, T* vz, T speed);
template <class T>
void launch_inlet_density(hipStream_t st, const GridDesc& g, const SlabCtx& sc, T* dens, T amount);

// dense (reference layout, (W+2)(H+2)(D+2), x fastest) <-> pitched device layout, with
// element-type conversion.  zlo..zhi (inclusive, local planes) select the planes moved.
template <class T, class U>
void launch_pack(hipStream_t st, const GridDesc& g, const T* field, U* dense, int zlo, int zhi);
template <class T, class U>
void launch_unpack(hipStream_t st, const GridDesc& g, const U* dense, T* field, int zlo, int zhi);

template <class T>
void launch_copy(hipStream_t st, const GridDesc& g, const T* src, T* dst);

// sum / min / max over the padded box; out = 3 doubles on the device
template <class T>
void launch_stats(hipStream_t st, const GridDesc& g, const T* field, double* out3, double* scratch, int nscratch,
                  int zlo, int zhi);

template <class T>
void launch_point_add(hipStream_t st, T* p, long idx, T amount, int set_instead);

// Time-averaged flow statistics (flow_stats.h has the arithmetic and the array layout; flow_stats.hip the kernels).
struct FlowStatsAcc {
    double* a[12];                   // allocation bases (cell index -LEAD) of the mode's accumulators, in flow_stats.h's order
};
// One sample: every accumulator of the mode (nacc = 5 or 12) takes the five fields' values, cell by cell.  q, u, v, w, p are
// LEAD-shifted field pointers (local plane 0 at index 0); first = the first sample after a reset (nothing is read).
template <class T>
void launch_flow_stats(hipStream_t st, const GridDesc& g, int nacc, bool first, const T* q, const T* u, const T* v, const T* w,
                       const T* p, const FlowStatsAcc& acc);
// One derived field (`which` = flow_stats.h's ST_Q .. ST_TKE; raw: the sum itself) of `n` samples into `out`, an fp64 array
// of the accumulators' layout (allocation base).  zero_lo / zero_hi: local plane 0 / D + 1 is an inter-slab halo, written 0.
void launch_flow_stats_finalize(hipStream_t st, const GridDesc& g, const FlowStatsAcc& acc, int which, bool raw, long n,
                                bool zero_lo, bool zero_hi, double* out);

// Vortex identification (vortex.h has the arithmetic, vortex.hip the z-marching kernel).  One field, `which` = VORTEX_WX ..
// VORTEX_Q, of the velocities vx, vy, vz into `out`, an array of the fields' layout (LEAD-shifted like them): rows 1..H of
// planes 1..D are written whole -- target cells (flags without F_SOLID) the value, the others +0.0 -- and nothing else is,
// so `out` must hold +0.0 in its ghost column, rows and planes beforehand.  Reads planes 0..D+1 of the velocities.
template <class T>
void launch_vortex(hipStream_t st, const SweepTune& tune, const GridDesc& g, const SlabCtx& sc, int which, const T* vx,
                   const T* vy, const T* vz, const uint8_t* flags, T* out);

// Vorticity confinement (confine.h has the arithmetic, confine.hip the fused z-marching kernel).  One pass over the velocities
// vx, vy, vz (read only, planes 0..D+1) into ox, oy, oz, three other arrays of the fields' layout: every target cell takes
// v + k * (N x omega), the other interior cells their stored values, and the three arrays come out as set_bounds(1 / 2 / 3)
// would leave them -- ghost faces from the new values, solid cells and their fluid neighbours zeroed.  The twelve box edges
// of the results are not written or take +0.0.  Single GPU (g.zh == 1, both z walls physical).
template <class T>
void launch_confine(hipStream_t st, const GridDesc& g, const T* vx, const T* vy, const T* vz, const uint8_t* flags, T* ox, T* oy,
                    T* oz, double k);

// Turbulent inflow (inflow.h has the arithmetic, inflow.hip the two kernels).  launch_inflow_table: the entries of the p.n eddies
// at step t into tab (where not null) and their ex, ey, ez and three signs into eddies (p.n x 6, where not null); nothing where
// p.n == 0.  launch_inflow_plane: the x = 1 face, cells 1..H x 1..D, from tab's p.n entries, the gust factor and the two maps
// (H x D doubles, y fastest; null = `speed` everywhere / 1 everywhere) -- cast into vx, vy, vz where out is null, else as three
// planes of H x D doubles into out and the fields are not touched.  Single GPU (g.zh == 1).
struct InflowParams;
struct InflowEntry;
void launch_inflow_table(hipStream_t st, const InflowParams& p, long t, InflowEntry* tab, double* eddies);
template <class T>
void launch_inflow_plane(hipStream_t st, const GridDesc& g, const InflowParams& p, const InflowEntry* tab, double gust, double speed,
                         const double* mean, const double* scale, T* vx, T* vy, T* vz, double* out);

// Heat and buoyancy (heat.h has the arithmetic, heat.hip the kernels).  launch_heat_apply: one streaming pass, in place, over
// the temperature `theta` and -- only where p.beta != 0 or p.alpha != 0 -- the velocity component `vup` along p.up, which
// reads the density `dens`; otherwise vup and dens are not touched and may be null.  Both arrays come out as set_bounds(0, .)
// and set_bounds(1 + p.up / 2, .) would leave them: ghost faces from the un-zeroed new values, solid cells (for the velocity
// also their fluid neighbours) zeroed; the twelve box edges are not written or take +0.0.
// launch_heat_budget: the heat budget of `theta` and the x velocity `u` in three launches -- the COLUMN records, the PLANE
// records, the WHOLE record into `result` (HEAT_COLS doubles on the device) -- through the workspace `ws`
// (heat_workspace_doubles, whose PLANE records start at heat_planes_offset); no atomics, every sum in its written order.
// Single GPU (g.zh == 1, both z walls physical).
struct HeatPass;
template <class T>
void launch_heat_apply(hipStream_t st, const GridDesc& g, const HeatPass& p, T* theta, T* vup, const T* dens, const uint8_t* flags);
size_t heat_workspace_doubles(const GridDesc& g);
size_t heat_planes_offset(const GridDesc& g);
template <class T>
void launch_heat_budget(hipStream_t st, const GridDesc& g, const HeatPass& p, const T* theta, const T* u, const uint8_t* flags,
                        double* ws, double* result);

// Momentum zones (zones.h has the arithmetic, zones.hip the kernels).  launch_zone_apply: one streaming pass, in place, over the
// three velocity components; they come out as set_bounds(1, .), (2, .), (3, .) would leave them.
// launch_zone_budget: the budget of zt.n zones in three launches -- the COLUMN records, the PLANE records, the WHOLE records
// into `result` (zt.n * ZONE_COLS doubles on the device) -- through the workspace `ws` (zone_workspace_doubles for that many
// zones, whose PLANE records start at zone_planes_offset); no atomics, every sum in its written order; nothing else is written.
// launch_zone_mask: bit k of byte (x, y, z) of the dense padded array `dst` ((W+2)(H+2)(D+2) bytes on the device) is set where
// the cell is a target cell in zone k.  Single GPU (g.zh == 1, both z walls physical).
struct ZoneTable;
template <class T>
void launch_zone_apply(hipStream_t st, const GridDesc& g, const ZoneTable& zt, T* vx, T* vy, T* vz, const uint8_t* flags);
size_t zone_workspace_doubles(const GridDesc& g, int n_zones);
size_t zone_planes_offset(const GridDesc& g, int n_zones);
template <class T>
void launch_zone_budget(hipStream_t st, const GridDesc& g, const ZoneTable& zt, const T* vx, const T* vy, const T* vz,
                        const uint8_t* flags, double* ws, double* result);
void launch_zone_mask(hipStream_t st, const GridDesc& g, const ZoneTable& zt, const uint8_t* flags, uint8_t* dst);

}  // namespace fs
