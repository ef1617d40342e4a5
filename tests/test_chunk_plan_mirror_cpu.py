"""The mask-free plan of a reversed three-sweep pass (csrc/chunk_plan.h: mirrored_clean + mask_free_plan), on the host.  A
reversed pass numbers its planes z' = D + 1 - z; its table {zbeg, zend, ga, gb} is the upward one of the z-mirrored clean table.
Here the header is compiled and its output compared with a restatement in Python that never mirrors anything: it reads
cleanliness of logical plane z' straight from REAL plane D + 1 - z' of the table."""
import os
import shutil
import subprocess

import numpy as np
import pytest

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "fluid_simulation_amd", "csrc")

# stdin: cases "H D BY nbands nzc zc_len words" followed by (D + 2) * words table words; stdout: the mirrored table's words,
# then the plan's 4 * nblk numbers, one line each per case
DRIVER = r'''
#include "chunk_plan.h"
#include <cstdio>
int main()
{
    int H, D, BY, nbands, nzc, zc_len, words;
    while (std::scanf("%d %d %d %d %d %d %d", &H, &D, &BY, &nbands, &nzc, &zc_len, &words) == 7) {
        std::vector<uint32_t> tab((size_t)(D + 2) * words);
        for (uint32_t& w : tab)
            if (std::scanf("%u", &w) != 1) return 1;
        const std::vector<uint32_t> rev = fs::mirrored_clean(tab, words, D);
        std::vector<int> chunks;
        for (int zc = 0; zc < nzc; ++zc)
            for (int band = 0; band < nbands; ++band) {
                chunks.push_back(1 + zc * zc_len);
                chunks.push_back(std::min(D, zc * zc_len + zc_len));
            }
        for (uint32_t w : rev) std::printf("%u ", w);
        std::printf("\n");
        for (int x : fs::mask_free_plan(rev, words, H, D, BY, nbands, chunks)) std::printf("%d ", x);
        std::printf("\n");
    }
    return 0;
}
'''


def _model_plan(clean_real, H, D, BY, nbands, nzc, zc_len):
    """clean_real[z, y]: row y of REAL plane z holds no kill bit.  The plan of the reversed pass, in its logical planes."""
    out = []
    for v in range(nbands * nzc):
        band, zc = v % nbands, v // nbands
        zbeg, zend = 1 + zc * zc_len, min(D, zc * zc_len + zc_len)
        s = band * (BY - 4) - 1
        ywall = s <= 0 or s + BY - 1 >= H + 1
        lo1 = max(1, zbeg - 2)
        ngroups = max(0, (zend + 2 - lo1 + 1) // 3)
        g0 = g1 = ngroups
        if not ywall and zbeg <= zend:
            g0 = min(ngroups, (3 - lo1) // 3 + 1) if lo1 <= 3 else 0
            g1 = max(g0, min(ngroups, (D - lo1) // 3))
        ga = gb = g1
        for k in range(g0, g1):
            Z = lo1 + 3 * k
            planes = [D + 1 - min(max(p, 0), D + 1) for p in range(Z - 2, Z + 4)]      # logical -> real
            if not all(clean_real[z, s:s + BY].all() for z in planes):
                if ga == g1:
                    ga = k
                gb = k + 1
        out += [zbeg, zend, ga, gb]
    return out


def test_mirrored_plan_matches_a_model_that_reads_real_planes(tmp_path):
    cxx = shutil.which("c++") or shutil.which("g++")
    if cxx is None:
        pytest.fail("no C++ compiler")
    src = tmp_path / "mirror.cpp"
    src.write_text(DRIVER)
    exe = tmp_path / "mirror"
    subprocess.run([cxx, "-std=c++17", "-O1", "-I", CSRC, str(src), "-o", str(exe)], check=True)
    rng = np.random.default_rng(23)
    cases, text = [], []
    for t in range(200):
        BY = (10, 12, 16, 20)[t % 4]
        H, D = int(rng.integers(8, 120)), int(rng.integers(1, 120))
        nbands, words = (H + BY - 5) // (BY - 4), (H + 2 + 31) // 32 + 1
        nzc = int(rng.integers(1, 8))
        zc_len = 1 + (D + nzc - 1) // nzc + int(rng.integers(0, 3)) * (D // 4)
        clean = np.ones((D + 2, 32 * words), dtype=bool)
        kind = t % 3                                   # none / a few rows / many rows dirty, more of them at the low z end
        for _ in range(0 if kind == 0 else int(rng.integers(1, 5)) if kind == 1 else int(rng.integers(5, 60))):
            z = int(rng.integers(0, D + 2))
            clean[z if rng.integers(0, 3) else z // 3, int(rng.integers(0, H + 2))] = False
        tab = (clean.reshape(D + 2, words, 32) * (1 << np.arange(32, dtype=np.uint64))).sum(axis=2).astype(np.uint32)
        cases.append((clean, H, D, BY, nbands, nzc, zc_len, words, tab))
        text.append("%d %d %d %d %d %d %d\n%s\n" % (H, D, BY, nbands, nzc, zc_len, words, " ".join(map(str, tab.reshape(-1)))))
    lines = subprocess.run([str(exe)], input="".join(text), check=True, capture_output=True, text=True).stdout.splitlines()
    assert len(lines) == 2 * len(cases)
    mask_free = wall_free = 0
    for i, (clean, H, D, BY, nbands, nzc, zc_len, words, tab) in enumerate(cases):
        rev = np.array(lines[2 * i].split(), dtype=np.uint32).reshape(D + 2, words)
        assert (rev == tab[::-1]).all(), i             # plane z of the mirrored table is plane D + 1 - z
        got = list(map(int, lines[2 * i + 1].split()))
        want = _model_plan(clean, H, D, BY, nbands, nzc, zc_len)
        assert got == want, (i, H, D, BY, nzc, zc_len)
        for v in range(nbands * nzc):
            zbeg, zend, ga, gb = got[4 * v:4 * v + 4]
            wall_free += gb - ga
            mask_free += zbeg <= zend
    assert wall_free > 100 and mask_free > 1000        # the cases do exercise both kinds of group
