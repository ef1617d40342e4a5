// chunk_plan.h -- host-side z-chunk plan of the three-sweep kernel's mask-free build (sweep_fused.hip): per band, chunk
// boundaries chosen so that every workgroup's estimated cost is about the same.  Plain C++ (no HIP), so that a CPU test can
// drive it (tests/chunk_plan_driver.cpp).
#pragma once
#include <algorithm>
#include <cstdint>
#include <vector>

namespace fs {

// Cost per plane iteration of the three bodies, in arbitrary units: general (a level touches a y / z wall), wall-free,
// mask-free (wall-free and no kill byte on the planes and rows the iteration's settle4s read).
struct ChunkCost {
    int general = 0, wall_free = 0, mask_free = 0;   // all 0 = no balancing: equal z chunks
};

// Clean table: bit y of word (z * words + y / 32) is set iff row y of plane z holds no kill bit in either nibble
// (planes 0 .. D+1, rows 0 .. H+1).  True iff rows s .. s+BY-1 of plane z are all clean.
inline bool band_clean(const std::vector<uint32_t>& tab, int words, int z, int s, int BY)
{
    for (int y = s; y < s + BY; ++y)
        if (!((tab[(size_t)z * words + (size_t)y / 32] >> (y % 32)) & 1u)) return false;
    return true;
}

// (zbeg, zend) of every workgroup v = band + nbands * zc of a launch with `nzc` chunks per band, output planes 1..D.  Each
// band's non-empty chunks cover 1..D exactly once, in order; a chunk with zbeg > zend is empty (its workgroup returns).
// The model: a chunk with output planes zb..ze runs the plane iterations max(1, zb-2) .. ze+2 (three levels, two planes of
// overlap per side) plus one iteration's worth of start-up loads; an iteration is general within three planes of a z wall
// and throughout in a band at a y wall; of the others, those from the band's first to its last iteration that is not clean on
// planes zl-2 .. zl+3 are wall-free (the kernel runs one wall-free stretch per chunk), the rest mask-free.
inline std::vector<int> balanced_chunks(const std::vector<uint32_t>& tab, int words, int H, int D, int BY, int nbands,
                                        int nzc, const ChunkCost& c)
{
    constexpr int OV = 2;
    std::vector<int> out((size_t)2 * nbands * nzc);
    std::vector<double> pre((size_t)D + 4, 0.0);         // pre[i] = cost of iterations 1..i, i <= D + 2
    for (int band = 0; band < nbands; ++band) {
        const int s = band * (BY - 2 * OV) - (OV - 1);
        const bool ywall = (s <= 0) || (s + BY - 1 >= H + 1);
        auto general = [&](int zl) { return ywall || zl <= 3 || zl >= D - 2; };
        int first = D + OV + 1, last = 0;
        for (int zl = 4; zl <= D - 3 && !ywall; ++zl) {
            bool clean = true;
            for (int p = zl - 2; p <= zl + 3 && clean; ++p) clean = band_clean(tab, words, p, s, BY);
            if (!clean) {
                first = std::min(first, zl);
                last = zl;
            }
        }
        for (int zl = 1; zl <= D + OV; ++zl) {
            const double k = general(zl) ? c.general : (zl >= first && zl <= last) ? c.wall_free : c.mask_free;
            pre[(size_t)zl] = pre[(size_t)zl - 1] + k;
        }
        auto cost = [&](int zb, int ze) { return pre[(size_t)ze + OV] - pre[(size_t)std::max(1, zb - OV) - 1] + c.wall_free; };
        // greedy cuts under a bound T: each chunk as long as it stays within T (at least one plane); feasible if <= nzc chunks
        auto cut = [&](double T, std::vector<int>* ends) {
            int zb = 1, n = 0;
            while (zb <= D) {
                int ze = zb;
                while (ze < D && cost(zb, ze + 1) <= T) ++ze;
                if (ends) ends->push_back(ze);
                ++n;
                zb = ze + 1;
            }
            return n;
        };
        double lo = 0.0, hi = cost(1, D);
        for (int it = 0; it < 60; ++it) {
            const double mid = 0.5 * (lo + hi);
            if (cut(mid, nullptr) <= nzc) hi = mid;
            else lo = mid;
        }
        std::vector<int> ends;
        cut(hi, &ends);
        int zb = 1;
        for (int zc = 0; zc < nzc; ++zc) {
            const size_t v = (size_t)band + (size_t)nbands * zc;
            const int ze = zc < (int)ends.size() ? ends[(size_t)zc] : zb - 1;
            out[2 * v] = zb;
            out[2 * v + 1] = ze;
            zb = std::max(zb, ze + 1);
        }
    }
    return out;
}

// The clean table of the z-mirrored problem: plane z of the result is plane D + 1 - z of `tab`.  A reversed march (sweep_fused.hip,
// ZREV) numbers its planes that way, so its chunks and its mask-free plan are the upward ones of this table.
inline std::vector<uint32_t> mirrored_clean(const std::vector<uint32_t>& tab, int words, int D)
{
    std::vector<uint32_t> out(tab.size());
    for (int z = 0; z <= D + 1; ++z)
        std::copy(tab.begin() + (size_t)(D + 1 - z) * words, tab.begin() + (size_t)(D + 2 - z) * words, out.begin() + (size_t)z * words);
    return out;
}

// What a workgroup of the mask-free build reads at its start: {zbeg, zend, ga, gb} per workgroup, from its (zbeg, zend).  Its
// wall-free groups [g0, g1) (as jacobi_fused_kernel numbers them) run mask-free [g0, ga), wall-free [ga, gb), mask-free
// [gb, g1): ga / gb - 1 are the first / last group that is not clean.  Group k (iterations Z = lo1 + 3k .. Z + 2) is clean when
// the band's rows s .. s + BY - 1 hold no kill byte on planes Z - 2 .. Z + 3: its settle4s read planes Z - 2 .. Z + 2 and it
// leaves the kill bytes of Z + 1 .. Z + 3 to the group after it.
inline std::vector<int> mask_free_plan(const std::vector<uint32_t>& tab, int words, int H, int D, int BY, int nbands,
                                       const std::vector<int>& chunks)
{
    constexpr int NL = 3, OV = 2;
    const size_t nblk = chunks.size() / 2;
    std::vector<int> out(4 * nblk);
    for (size_t v = 0; v < nblk; ++v) {
        const int zbeg = chunks[2 * v], zend = chunks[2 * v + 1];
        const int s = (int)(v % (size_t)nbands) * (BY - 2 * OV) - (OV - 1);
        const bool ywall = (s <= 0) || (s + BY - 1 >= H + 1);
        const int lo1 = std::max(1, zbeg - OV), ngroups = std::max(0, (zend + OV - lo1 + 1) / 3);
        int g0 = ngroups, g1 = ngroups;
        if (!ywall && zbeg <= zend) {
            g0 = lo1 <= NL ? std::min(ngroups, (NL - lo1) / 3 + 1) : 0;
            g1 = std::max(g0, std::min(ngroups, (D - lo1) / 3));
        }
        int ga = g1, gb = g1;
        for (int k = g0; k < g1; ++k) {
            const int Z = lo1 + 3 * k;
            bool clean = true;
            for (int p = Z - 2; p <= Z + 3 && clean; ++p) clean = band_clean(tab, words, std::min(std::max(p, 0), D + 1), s, BY);
            if (!clean) {
                if (ga == g1) ga = k;
                gb = k + 1;
            }
        }
        out[4 * v] = zbeg;
        out[4 * v + 1] = zend;
        out[4 * v + 2] = ga;
        out[4 * v + 3] = gb;
    }
    return out;
}

}  // namespace fs
