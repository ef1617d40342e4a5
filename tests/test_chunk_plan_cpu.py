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
