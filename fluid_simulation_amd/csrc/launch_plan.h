// launch_plan.h -- the launch plans of the two- and three-sweep Jacobi kernels (jacobi_pair_kernel, kernels.hip;
// jacobi_fused_kernel, sweep_fused.hip): plan ids, workgroup shapes, band count, the z-chunk model, the candidates the host
// times and the check of a replayed id.  Plain C++ (no HIP), so that a CPU test can drive it (tests/test_launch_plan_cpu.py).
// A plan = kernel x workgroup shape x which of the model's three best z-chunk counts (alt).  All plans give the same bits.
#pragma once
#include <vector>

namespace fs {

enum class SweepKernel { Pair, Fused2, Three };          // two sweeps (kernels.hip), two and three sweeps (sweep_fused.hip)
constexpr int plan_levels(SweepKernel k) { return k == SweepKernel::Three ? 3 : 2; }

// ---- ids: public (fs_get_int "pair_shape" / "triple_plan", "launch_plans", the bench line, profiles/sweep_traffic.json) ----
// two-sweep id: pair kernel shape + 8 alt, fused kernel 64 + shape + 8 alt; three-sweep id: shape + 8 alt
struct PlanId {
    SweepKernel kind;
    int shape, alt;
};
constexpr int PLAN_ALTS = 3, PLAN_ALT_STEP = 8, PLAN_FUSED2 = 64;
constexpr int encode_plan(const PlanId& p) { return (p.kind == SweepKernel::Fused2) * PLAN_FUSED2 + p.shape + PLAN_ALT_STEP * p.alt; }
constexpr PlanId decode_plan(bool three_sweep_id, int id)
{
    if (id < 0) id = 0;                                  // "no plan yet" runs plan 0
    const bool fused2 = !three_sweep_id && id >= PLAN_FUSED2;
    if (fused2) id -= PLAN_FUSED2;
    return {three_sweep_id ? SweepKernel::Three : fused2 ? SweepKernel::Fused2 : SweepKernel::Pair, id % PLAN_ALT_STEP,
            id / PLAN_ALT_STEP};
}

// ---- workgroup shapes ------------------------------------------------------------------------------------------------------
// NXW x NYW waves; a wave covers 256 cells of RY rows (the pair kernel: two rows), a workgroup a band of BY rows, of which
// NL - 1 per side are recomputed overlap
struct SweepShape {
    int NL, NXW, NYW, RY;
    constexpr int BY() const { return NYW * RY; }
    constexpr bool is(int nl, int nxw, int nyw, int ry) const { return NL == nl && NXW == nxw && NYW == nyw && RY == ry; }
};
struct ShapeRow {                                        // shape ids 0 .. n-1 of rows of wmin .. wmax cells
    int elem;                                            // element size: 4 / 8
    SweepKernel kind;
    int wmin, wmax;
    int n, timed;                                        // ids 0 .. timed-1 are timed, the rest option "pair_shape" only
    SweepShape s[4];
};
// fp32 pair: 12, 8, 10 waves (<= 168 VGPRs) and 16 (spills; tuning tool only); band count vs CU count decides, e.g. 10 waves
// at 512^3, 12 at 256^3.  fp64 pair: LDS, 4 * BY * TW * 8 bytes, must stay under 160 KB.  Three sweeps: two rows per wave
// throughout (three rows and 8 waves were slower: the instruction stream of a wave is what limits this kernel); the smaller
// bands trade recomputed rows for longer z chunks and, at 12 rows of 256 cells, two workgroups per CU.  fp32 fused two
// sweeps: 16 waves x two rows (<= 128 VGPRs) or 12 waves x three rows.  fp64 fused: 10 waves, or 8 (256 VGPRs).
inline constexpr ShapeRow SHAPE_TABLE[] = {
    {4, SweepKernel::Pair, 1, 256, 4, 3, {{2, 1, 12, 2}, {2, 1, 8, 2}, {2, 1, 10, 2}, {2, 1, 16, 2}}},
    {4, SweepKernel::Pair, 257, 512, 4, 3, {{2, 2, 6, 2}, {2, 2, 4, 2}, {2, 2, 5, 2}, {2, 2, 8, 2}}},
    {4, SweepKernel::Pair, 513, 768, 1, 1, {{2, 3, 4, 2}}},
    {4, SweepKernel::Pair, 769, 1024, 1, 1, {{2, 4, 3, 2}}},
    {8, SweepKernel::Pair, 1, 256, 1, 1, {{2, 1, 8, 2}}},
    {8, SweepKernel::Pair, 257, 512, 1, 1, {{2, 2, 4, 2}}},
    {8, SweepKernel::Pair, 513, 768, 1, 1, {{2, 3, 3, 2}}},
    {8, SweepKernel::Pair, 769, 1024, 1, 1, {{2, 4, 2, 2}}},
    {4, SweepKernel::Three, 1, 256, 3, 3, {{3, 1, 10, 2}, {3, 1, 8, 2}, {3, 1, 6, 2}}},
    {4, SweepKernel::Three, 257, 512, 2, 2, {{3, 2, 6, 2}, {3, 2, 5, 2}}},
    {4, SweepKernel::Fused2, 513, 768, 1, 1, {{2, 3, 4, 2}}},
    {4, SweepKernel::Fused2, 769, 1024, 2, 2, {{2, 4, 4, 2}, {2, 4, 3, 3}}},
    {8, SweepKernel::Fused2, 1, 256, 1, 1, {{2, 1, 10, 2}}},
    {8, SweepKernel::Fused2, 257, 512, 2, 2, {{2, 2, 5, 2}, {2, 2, 4, 2}}},
};

constexpr const ShapeRow* shape_row(int elem, SweepKernel kind, int W)
{
    for (const ShapeRow& r : SHAPE_TABLE)
        if (r.elem == elem && r.kind == kind && r.wmin <= W && W <= r.wmax) return &r;
    return nullptr;
}
// the shape a launch runs: an id the row lacks (a forced "pair_shape" this width has no build for) runs shape 0
constexpr const SweepShape* launch_shape(int elem, SweepKernel kind, int W, int shape)
{
    const ShapeRow* r = shape_row(elem, kind, W);
    return !r ? nullptr : &r->s[shape >= 0 && shape < r->n ? shape : 0];
}

// What a .hip file instantiates, named once: Builds<Build<NL, NXW, NYW, RY>...>::run calls f(Build<...>{}) for the build of
// `s`; covers() is for a static_assert next to the list, so that a table entry without a build fails to compile.
template <int NL_, int NXW_, int NYW_, int RY_>
struct Build { static constexpr int NL = NL_, NXW = NXW_, NYW = NYW_, RY = RY_; };
template <class... B>
struct Builds {
    static constexpr bool has(const SweepShape& s) { return (s.is(B::NL, B::NXW, B::NYW, B::RY) || ...); }
    static constexpr bool covers(int elem, SweepKernel kind)
    {
        for (const ShapeRow& r : SHAPE_TABLE)
            for (int i = 0; i < r.n; ++i)
                if (r.elem == elem && r.kind == kind && !has(r.s[i])) return false;
        return true;
    }
    template <class F>
    static bool run(const SweepShape& s, F&& f)
    {
        return ((s.is(B::NL, B::NXW, B::NYW, B::RY) ? (f(B{}), true) : false) || ...);
    }
};

// ---- which kernels a grid has --------------------------------------------------------------------------------------------
struct PlanGrid {
    int elem, W;
    bool whole;                                          // whole domain; else a z-slab with zh halo planes per side
    int zh, fuse;                                        // fuse: option "sweep_fuse"
};
// NL sweeps cross a slab boundary on NL halo planes; three sweeps: fp32 rows up to 512 cells; fused two sweeps: fp32 rows of
// 513 .. 1024, fp64 up to 512; pair: rows up to 1024
constexpr bool plan_supported(const PlanGrid& G, SweepKernel k)
{
    return (G.whole || G.zh >= plan_levels(k)) && G.fuse >= plan_levels(k) && shape_row(G.elem, k, G.W) != nullptr;
}

// band k outputs rows k (BY - 2 (NL-1)) + 1 .. (k + 1)(BY - 2 (NL-1)), the last band up to row H
constexpr int plan_bands(int H, const SweepShape& s)
{
    const int step = s.BY() - 2 * (s.NL - 1);
    return (H + step - 1) / step;
}

// ---- z chunks ------------------------------------------------------------------------------------------------------------
// Planes per z chunk of a launch over `planes` planes in `nbands` bands.  A chunk re-reads and recomputes `overlap` planes
// beyond its own, so chunks should be long (at least min_len, at most 64 of them), and their count should fill the CUs
// evenly (one workgroup per slot).  Model: fraction of CU slots filled x useful fraction of a chunk's planes; `alt` picks
// the alt-th best count by it (the host driver times alt = 0, 1, 2 once per grid, because how the block count falls against
// the CUs matters more than the model knows).
inline int chunk_len(int planes, int nbands, int alt, int min_len, int overlap, int slots)
{
    int cand_nzc[PLAN_ALTS] = {1, 1, 1};
    double cand_eff[PLAN_ALTS] = {-1.0, -1.0, -1.0};
    for (int nzc = 1; nzc <= 64 && (nzc == 1 || planes / nzc >= min_len); ++nzc) {
        const long blocks = (long)nbands * nzc;
        const long rounds = (blocks + slots - 1) / slots;
        const int len = (planes + nzc - 1) / nzc;
        const double eff = (double)blocks / (double)(rounds * slots) * (double)len / (double)(len + overlap);
        for (int k = 0; k < PLAN_ALTS; ++k)
            if (eff > cand_eff[k] + 1e-9) {
                for (int j = PLAN_ALTS - 1; j > k; --j) { cand_eff[j] = cand_eff[j - 1]; cand_nzc[j] = cand_nzc[j - 1]; }
                cand_eff[k] = eff;
                cand_nzc[k] = nzc;
                break;
            }
    }
    int pick = alt < 0 ? 0 : (alt >= PLAN_ALTS ? PLAN_ALTS - 1 : alt);
    while (pick > 0 && cand_eff[pick] < 0.0) --pick;
    return (planes + cand_nzc[pick] - 1) / cand_nzc[pick];
}
// the two launchers' constants: minimum chunk length and overlap planes
constexpr int chunk_min_len(SweepKernel k) { return k == SweepKernel::Pair ? 12 : 16; }
constexpr int chunk_overlap(SweepKernel k, int NL) { return k == SweepKernel::Pair ? 3 : 2 * NL - 1; }

// ---- what the host times, and what it accepts for replay ---------------------------------------------------------------
// ids of kernel k in timing order (a later candidate has to beat an earlier one by a margin, so the order matters)
inline std::vector<int> kernel_candidates(const PlanGrid& G, SweepKernel k)
{
    std::vector<int> out;
    for (int shape = 0; plan_supported(G, k) && shape < shape_row(G.elem, k, G.W)->timed; ++shape)
        for (int alt = 0; alt < PLAN_ALTS; ++alt) out.push_back(encode_plan({k, shape, alt}));
    return out;
}
// options: pair_shape > 0 forces a workgroup shape of the pair kernel, two_kind ("two_sweep_kernel") one of the two kernels
inline std::vector<int> two_sweep_candidates(const PlanGrid& G, int pair_shape, int two_kind)
{
    const bool forced_pair = pair_shape > 0 || two_kind == 1 || !plan_supported(G, SweepKernel::Fused2);
    const bool forced_fused = !forced_pair && two_kind == 2;
    std::vector<int> out = forced_fused ? std::vector<int>() : kernel_candidates(G, SweepKernel::Pair);
    const std::vector<int> fused = forced_pair ? std::vector<int>() : kernel_candidates(G, SweepKernel::Fused2);
    out.insert(out.end(), fused.begin(), fused.end());
    return out;
}

// A replayed id ("launch_plans"): one that names a kernel, shape or alt this grid does not have is refused, not run --
// except a three-sweep id on a grid without that kernel, which is ignored (one setting can serve several grids).
enum class Replay { Use, Ignore, Refuse };
inline Replay check_replay(const PlanGrid& G, bool three_sweep_id, int id)
{
    if (id < 0) return Replay::Ignore;                   // -1: no such plan given
    const PlanId p = decode_plan(three_sweep_id, id);
    if (!plan_supported(G, p.kind)) return three_sweep_id ? Replay::Ignore : Replay::Refuse;
    return (p.shape < shape_row(G.elem, p.kind, G.W)->timed && p.alt < PLAN_ALTS) ? Replay::Use : Replay::Refuse;
}

}  // namespace fs
