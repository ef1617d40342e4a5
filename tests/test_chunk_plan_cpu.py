"""The balanced z-chunk plan of the three-sweep kernel's mask-free build (csrc/chunk_plan.h), on the host: for random clean
tables and every launch shape, each band's chunks cover output planes 1..D exactly once and in order."""
import os
import shutil
import subprocess

import pytest

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "fluid_simulation_amd", "csrc")

DRIVER = r'''
#include "chunk_plan.h"
#include <cstdio>
#include <random>
int main()
{
    std::mt19937 rng(7);
    int bad = 0, plans = 0;
    for (int t = 0; t < 300; ++t) {
        const int H = 10 + (int)(rng() % 300), D = 3 + (int)(rng() % 300), BY = 10 + 2 * (int)(rng() % 6);
        const int nbands = (H + BY - 5) / (BY - 4), nzc = 1 + (int)(rng() % 12), words = (H + 2 + 31) / 32 + 1;
        std::vector<uint32_t> tab((size_t)(D + 2) * words, 0xffffffffu);
        const int dirty = (int)(rng() % 40);
        for (int k = 0; k < dirty; ++k) {
            const int z = (int)(rng() % (D + 2)), y = (int)(rng() % (H + 2));
            tab[(size_t)z * words + y / 32] &= ~(1u << (y % 32));
        }
        fs::ChunkCost c{1 + (int)(rng() % 30), 1 + (int)(rng() % 30), 1 + (int)(rng() % 30)};
        const std::vector<int> p = fs::balanced_chunks(tab, words, H, D, BY, nbands, nzc, c);
        for (int b = 0; b < nbands; ++b) {
            int next = 1;
            for (int zc = 0; zc < nzc; ++zc) {
                const int zb = p[2 * (b + nbands * zc)], ze = p[2 * (b + nbands * zc) + 1];
                if (zb > ze) continue;
                if (zb != next || ze > D) ++bad;
                next = ze + 1;
            }
            if (next != D + 1) ++bad;
            ++plans;
        }
    }
    std::printf("%d %d\n", plans, bad);
    return 0;
}
'''


def test_balanced_chunks_cover_every_plane_once(tmp_path):
    cxx = shutil.which("c++") or shutil.which("g++")
    if cxx is None:
        pytest.fail("no C++ compiler")
    src = tmp_path / "driver.cpp"
    src.write_text(DRIVER)
    exe = tmp_path / "driver"
    subprocess.run([cxx, "-std=c++17", "-O1", "-I", CSRC, str(src), "-o", str(exe)], check=True)
    plans, bad = map(int, subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split())
    assert plans > 1000 and bad == 0


# mask_free_plan's safety property.  The group numbering g0 / g1 is restated from jacobi_fused_kernel (sweep_fused.hip, the
# WALLSEL 1 / 3 split: whole domain, NL = 3); cleanliness is read straight from the table bits, not through band_clean.
SAFETY_DRIVER = r'''
#include "chunk_plan.h"
#include <cstdio>
#include <random>
static bool row_clean(const std::vector<uint32_t>& tab, int words, int z, int y)
{
    return (tab[(size_t)z * words + (size_t)(y >> 5)] >> (y & 31)) & 1u;
}
int main()
{
    std::mt19937 rng(11);
    const int BYS[4] = {10, 12, 16, 20};
    long groups = 0, mask_free = 0, unclean = 0, numbering = 0, order = 0, ywall_mf = 0, walls = 0, loose = 0;
    for (int t = 0; t < 400; ++t) {
        const int BY = BYS[t % 4], H = 8 + (int)(rng() % 120), D = 1 + (int)(rng() % 160);
        const int nbands = (H + BY - 5) / (BY - 4), words = (H + 2 + 31) / 32 + 1;
        std::vector<uint32_t> tab((size_t)(D + 2) * words, 0xffffffffu);
        const int kind = (int)(rng() % 4), dirty = kind == 0 ? 0 : kind == 1 ? 1 + (int)(rng() % 4) : (int)(rng() % 60);
        for (int k = 0; k < dirty; ++k) {
            const int z = (int)(rng() % (D + 2));
            // kind 3: rows two neighbouring bands share (band k + 1 starts BY - 4 rows after band k)
            const int y = kind == 3 ? (int)(((1 + rng() % 8) * (BY - 4) - 1 + rng() % 4) % (H + 2)) : (int)(rng() % (H + 2));
            tab[(size_t)z * words + y / 32] &= ~(1u << (y % 32));
        }
        // equal chunks as the launcher cuts them (nzc * zc_len may pass D: empty trailing chunks), or balanced ones
        const int nzc = 1 + (int)(rng() % 10);
        std::vector<int> chunks;
        if (rng() % 2) {
            const int zc_len = 1 + (D + nzc - 1) / nzc + (int)(rng() % 3) * (D / 4);
            for (int zc = 0; zc < nzc; ++zc)
                for (int band = 0; band < nbands; ++band) {
                    chunks.push_back(1 + zc * zc_len);
                    chunks.push_back(std::min(D, zc * zc_len + zc_len));
                }
        } else {
            fs::ChunkCost c{1 + (int)(rng() % 30), 1 + (int)(rng() % 30), 1 + (int)(rng() % 30)};
            chunks = fs::balanced_chunks(tab, words, H, D, BY, nbands, nzc + (int)(rng() % 2) * D, c);
        }
        const std::vector<int> p = fs::mask_free_plan(tab, words, H, D, BY, nbands, chunks);
        const int nblk = (int)chunks.size() / 2;
        for (int v = 0; v < nblk; ++v) {
            const int zbeg = p[4 * v], zend = p[4 * v + 1], ga = p[4 * v + 2], gb = p[4 * v + 3];
            if (zbeg != chunks[2 * v] || zend != chunks[2 * v + 1]) ++numbering;
            if (zbeg > zend) continue;                   // the workgroup returns at once
            // jacobi_fused_kernel: lo1, zl_end, ngroups and the wall-free groups [g0, g1)
            const int s = (v % nbands) * (BY - 4) - 1;
            const int lo1 = std::max(1, zbeg - 2), zl_end = zend + 2, ngroups = (zl_end - lo1 + 1) / 3;
            const bool ywall = (s <= 0) || (s + BY - 1 >= H + 1);
            int g0 = ngroups, g1 = ngroups;
            if (!ywall) {
                g0 = (lo1 <= 3) ? std::min(ngroups, (3 - lo1) / 3 + 1) : 0;
                g1 = std::max(g0, std::min(ngroups, (D - lo1) / 3));
            }
            if (!(g0 <= ga && ga <= gb && gb <= g1)) { ++order; continue; }
            if (ywall && g0 != g1) ++ywall_mf;
            for (int k = g0; k < g1; ++k) {
                const int Z = lo1 + 3 * k;
                ++groups;
                // a wall-free group: no level of iterations Z .. Z+2 is plane 1 or plane D
                if (Z - 2 < 2 || Z + 2 > D - 1) ++walls;
                bool clean = true;
                for (int z = Z - 2; z <= Z + 3; ++z)
                    for (int y = s; y <= s + BY - 1; ++y)
                        if (z < 0 || z > D + 1 || y < 0 || y > H + 1 || !row_clean(tab, words, z, y)) clean = false;
                const bool mf = k < ga || k >= gb;
                if (mf) ++mask_free;
                if (mf && !clean) ++unclean;
                if (ga < gb && (k == ga || k == gb - 1) && clean) ++loose;   // ga / gb - 1: the first / last group that is not clean
            }
        }
    }
    std::printf("%ld %ld %ld %ld %ld %ld %ld %ld\n", groups, mask_free, unclean, numbering, order, ywall_mf, walls, loose);
    return 0;
}
'''


def test_mask_free_plan_hands_only_clean_groups_to_the_mask_free_body(tmp_path):
    """For random clean tables, band heights 10, 12, 16 and 20, equal and balanced chunks (empty ones included): every group
    a workgroup runs mask-free ([g0, ga) and [gb, g1)) holds no kill byte on rows s .. s+BY-1 of planes Z-2 .. Z+3, the
    wall-free groups [g0, g1) touch no z wall and exist in no y-wall band, g0 <= ga <= gb <= g1, and the wall-free stretch
    [ga, gb) starts and ends on a group that is not clean."""
    cxx = shutil.which("c++") or shutil.which("g++")
    if cxx is None:
        pytest.fail("no C++ compiler")
    src = tmp_path / "safety.cpp"
    src.write_text(SAFETY_DRIVER)
    exe = tmp_path / "safety"
    subprocess.run([cxx, "-std=c++17", "-O1", "-I", CSRC, str(src), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()
    groups, mask_free, unclean, numbering, order, ywall_mf, walls, loose = map(int, out)
    assert groups > 10000 and 0 < mask_free < groups, out
    assert (unclean, numbering, order, ywall_mf, walls, loose) == (0, 0, 0, 0, 0, 0), out
