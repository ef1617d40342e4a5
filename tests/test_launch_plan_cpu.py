"""The launch plans of the two- and three-sweep Jacobi kernels (csrc/launch_plan.h), on the host: the header's ids, shape
table, band counts, z-chunk model, candidate order and replay check, line by line against the independent restatement in
launch_plan_model.py (which the GPU plan tests build their cases and obstacle masks from) and against values worked out
beforehand.  A driver compiled with the host C++ compiler answers queries on its standard input."""
import os
import random
import shutil
import subprocess

import pytest

from launch_plan_model import FUSED2, GRIDS, MG_GRID, RB_GRIDS, chunk_len, model_chunk_len, nbands, plan_list

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "fluid_simulation_amd", "csrc")

# queries, one per line:
#   grid W H D elem whole zh fuse pair_shape two_kind  ->  "two <ids>", "three <ids>", then per candidate
#                                                          "plan <two|three> id NL NXW NYW RY BY nbands chunk_len chunks"
#   chunk planes nbands alt min_len overlap slots      ->  "chunk <len>"
#   replay W elem whole zh fuse two three              ->  "replay <two> <three>"   (0 use, 1 ignore, 2 refuse)
#   ids                                                ->  "id <three?> id kind shape alt encode(decode(id))" for every id
DRIVER = r'''
#include "launch_plan.h"
#include <cstdio>
#include <cstring>
using namespace fs;
static void plans(const PlanGrid& G, int H, int D, bool three, const std::vector<int>& ids)
{
    std::printf(three ? "three" : "two");
    for (int id : ids) std::printf(" %d", id);
    std::printf("\n");
    for (int id : ids) {
        const PlanId p = decode_plan(three, id);
        const SweepShape* s = launch_shape(G.elem, p.kind, G.W, p.shape);
        const int nb = plan_bands(H, *s);
        const int len = chunk_len(D, nb, p.alt, chunk_min_len(p.kind), chunk_overlap(p.kind, s->NL), 256);
        std::printf("plan %s %d %d %d %d %d %d %d %d %d\n", three ? "three" : "two", id, s->NL, s->NXW, s->NYW, s->RY, s->BY(), nb,
                    len, (D + len - 1) / len);
    }
}
int main()
{
    char cmd[16];
    while (std::scanf("%15s", cmd) == 1) {
        if (!std::strcmp(cmd, "grid")) {
            int W, H, D, elem, whole, zh, fuse, pair_shape, two_kind;
            if (std::scanf("%d %d %d %d %d %d %d %d %d", &W, &H, &D, &elem, &whole, &zh, &fuse, &pair_shape, &two_kind) != 9) return 1;
            const PlanGrid G{elem, W, whole != 0, zh, fuse};
            plans(G, H, D, false, two_sweep_candidates(G, pair_shape, two_kind));
            plans(G, H, D, true, kernel_candidates(G, SweepKernel::Three));
        } else if (!std::strcmp(cmd, "chunk")) {
            int planes, nb, alt, min_len, overlap, slots;
            if (std::scanf("%d %d %d %d %d %d", &planes, &nb, &alt, &min_len, &overlap, &slots) != 6) return 1;
            std::printf("chunk %d\n", chunk_len(planes, nb, alt, min_len, overlap, slots));
        } else if (!std::strcmp(cmd, "replay")) {
            int W, elem, whole, zh, fuse, two, three;
            if (std::scanf("%d %d %d %d %d %d %d", &W, &elem, &whole, &zh, &fuse, &two, &three) != 7) return 1;
            const PlanGrid G{elem, W, whole != 0, zh, fuse};
            std::printf("replay %d %d\n", (int)check_replay(G, false, two), (int)check_replay(G, true, three));
        } else if (!std::strcmp(cmd, "ids")) {
            for (int three = 0; three < 2; ++three)
                for (int id = 0; id < (three ? 32 : 128); ++id) {
                    const PlanId p = decode_plan(three != 0, id);
                    std::printf("id %d %d %d %d %d %d\n", three, id, (int)p.kind, p.shape, p.alt, encode_plan(p));
                }
        } else {
            return 2;
        }
    }
    return 0;
}
'''

BENCH_GRIDS = [(256, 256, 256, False), (512, 512, 512, False), (1024, 512, 512, False), (512, 512, 512, True),
               (128, 64, 64, False)]
SLAB_GRID = (1024, 512, 128, False)      # 1024x512x512 as four z-slabs
USE, IGNORE, REFUSE = 0, 1, 2


@pytest.fixture(scope="module")
def ask(tmp_path_factory):
    cxx = shutil.which("c++") or shutil.which("g++")
    if cxx is None:
        pytest.fail("no C++ compiler")
    d = tmp_path_factory.mktemp("launch_plan")
    src = d / "driver.cpp"
    src.write_text(DRIVER)
    exe = d / "driver"
    subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-Werror", "-I", CSRC, str(src), "-o", str(exe)], check=True)

    def ask(lines):
        r = subprocess.run([str(exe)], input="\n".join(lines) + "\n", check=True, capture_output=True, text=True)
        return r.stdout.splitlines()
    return ask


def ask_grid(ask, W, H, D, fp64, whole=True, zh=1, fuse=3, pair_shape=0, two_kind=0):
    """(two-sweep ids, three-sweep ids, {(which, id): (NL, NXW, NYW, RY, BY, nbands, chunk_len, chunks)}) from the header."""
    out = ask(["grid %d %d %d %d %d %d %d %d %d" % (W, H, D, 8 if fp64 else 4, whole, zh, fuse, pair_shape, two_kind)])
    ids = {"two": None, "three": None}
    plans = {}
    for line in out:
        f = line.split()
        if f[0] in ids:
            assert ids[f[0]] is None, out
            ids[f[0]] = [int(x) for x in f[1:]]
        else:
            assert f[0] == "plan" and (f[1], int(f[2])) not in plans, out
            plans[(f[1], int(f[2]))] = tuple(int(x) for x in f[3:])
    assert set(plans) == {("two", i) for i in ids["two"]} | {("three", i) for i in ids["three"]}, out
    return ids["two"], ids["three"], plans


def expected_ids(W, fp64, whole=True, zh=1, fuse=3, pair_shape=0, two_kind=0):
    """The candidates in timing order, from the options' documented meaning: a kernel of NL sweeps needs sweep_fuse >= NL and,
    on a z-slab, NL halo planes; pair_shape > 0 and two_sweep_kernel = pair leave the pair kernel only, two_sweep_kernel =
    fused the fused one where the grid has it."""
    plans = plan_list(W, fp64)
    can = lambda nl: fuse >= nl and (whole or zh >= nl)
    pair = [p[2] for p in plans if p[0] == "pair"] if can(2) else []
    fused = [p[2] for p in plans if p[0] == "fused"] if can(2) else []
    three = [p[3] for p in plans if p[0] == "three"] if can(3) else []
    if pair_shape > 0 or two_kind == 1 or not fused:
        return pair, three
    return (fused if two_kind == 2 else pair + fused), three


def expected_plans(W, H, D, fp64):
    want = {}
    for kind, _, pid, tid, _, NL, BY, alt in plan_list(W, fp64):
        ln = model_chunk_len(kind, H, D, NL, BY, alt)
        want[("three", tid) if kind == "three" else ("two", pid)] = (NL, BY, nbands(H, BY, NL), ln, (D + ln - 1) // ln)
    return want


ALL_GRIDS = GRIDS + RB_GRIDS + [MG_GRID] + BENCH_GRIDS + [SLAB_GRID]


@pytest.mark.parametrize("W,H,D,fp64", ALL_GRIDS, ids=["%dx%dx%d-%s" % (g[0], g[1], g[2], "fp64" if g[3] else "fp32") for g in ALL_GRIDS])
def test_header_equals_the_restatement(ask, W, H, D, fp64):
    """Whole domain, default options: the same ids in the same order, and per id the same NL, band height, band count, chunk
    length and chunk count; NXW waves cover the row and NYW x RY rows make the band."""
    two, three, plans = ask_grid(ask, W, H, D, fp64)
    assert (two, three) == expected_ids(W, fp64)
    assert two == [p[2] for p in plan_list(W, fp64) if p[0] != "three"]
    want = expected_plans(W, H, D, fp64)
    assert set(plans) == set(want)
    for key, (NL, NXW, NYW, RY, BY, nb, ln, cnt) in plans.items():
        assert (NL, BY, nb, ln, cnt) == want[key], (key, plans[key], want[key])
        assert NXW == (W + 255) // 256 and NYW * RY == BY and nb * (BY - 2 * (NL - 1)) >= H, (key, plans[key])


def test_shape_table_literals(ask):
    """(NL, NXW, NYW, RY) of every shape id, as the docstring of test_gpu_launch_plans.py lists the instantiations."""
    def shapes(W, fp64, which, base=0):
        plans = ask_grid(ask, W, 40, 48, fp64)[2]
        return [plans[(which, base + s)][:4] for s in range(8) if (which, base + s) in plans]

    for W, want in ((200, [(2, 1, 12, 2), (2, 1, 8, 2), (2, 1, 10, 2)]), (512, [(2, 2, 6, 2), (2, 2, 4, 2), (2, 2, 5, 2)]),
                    (600, [(2, 3, 4, 2)]), (1024, [(2, 4, 3, 2)])):
        assert shapes(W, False, "two") == want
    for W, want in ((256, [(2, 1, 8, 2)]), (300, [(2, 2, 4, 2)]), (768, [(2, 3, 3, 2)]), (769, [(2, 4, 2, 2)])):
        assert shapes(W, True, "two") == want
    assert shapes(256, False, "three") == [(3, 1, 10, 2), (3, 1, 8, 2), (3, 1, 6, 2)]
    assert shapes(257, False, "three") == [(3, 2, 6, 2), (3, 2, 5, 2)]
    assert shapes(513, False, "three") == [] and shapes(200, True, "three") == []
    assert shapes(512, False, "two", FUSED2) == [] and shapes(768, False, "two", FUSED2) == [(2, 3, 4, 2)]
    assert shapes(1024, False, "two", FUSED2) == [(2, 4, 4, 2), (2, 4, 3, 3)]
    assert shapes(256, True, "two", FUSED2) == [(2, 1, 10, 2)] and shapes(512, True, "two", FUSED2) == [(2, 2, 5, 2), (2, 2, 4, 2)]
    assert shapes(513, True, "two", FUSED2) == []


def test_pinned_plans(ask):
    """id -> (bands, chunks, chunk length) the restatement gave before the header existed."""
    pinned = [
        ((512, 512, 512, False), "three", {0: (64, 4, 128), 8: (64, 8, 64), 16: (64, 12, 43), 1: (86, 11, 47)}),
        ((512, 512, 512, False), "two", {2: (64, 4, 128), 0: (52, 14, 37)}),
        ((256, 256, 256, False), "three", {0: (16, 16, 16), 2: (32, 8, 32), 18: (32, 16, 16)}),
        ((1024, 512, 512, False), "two", {0: (128, 2, 256), 64: (86, 14, 37), 65: (74, 10, 52)}),
        ((512, 512, 512, True), "two", {0: (86, 14, 37), 64: (64, 4, 128)}),
    ]
    for (W, H, D, fp64), which, want in pinned:
        plans = ask_grid(ask, W, H, D, fp64)[2]
        for pid, (nb, cnt, ln) in want.items():
            assert plans[(which, pid)][5:] == (nb, ln, cnt), ((W, H, D, fp64), which, pid, plans[(which, pid)])
    assert 64 * 4 == 256    # 512^3, three-sweep plan 0: one workgroup per CU


OPTION_SETS = [dict(fuse=4), dict(fuse=2), dict(fuse=1), dict(two_kind=1), dict(two_kind=2), dict(pair_shape=2), dict(pair_shape=3),
               dict(pair_shape=1, two_kind=2), dict(fuse=2, two_kind=2)]
SLAB_SETS = [dict(whole=False, zh=zh, **o) for zh in (1, 2, 3) for o in (dict(), dict(fuse=2), dict(two_kind=2))]


def test_candidates_under_options_and_on_slabs(ask):
    """sweep_fuse, pair_shape, two_sweep_kernel and the halo depth of a z-slab select among the same plans, in the same order;
    they never change a plan's geometry.  The config-4 slab (rows of 1024 cells, two halo planes) has no three-sweep kernel."""
    seen = set()
    for W, H, D, fp64 in GRIDS + BENCH_GRIDS + [SLAB_GRID]:
        base = ask_grid(ask, W, H, D, fp64)[2]
        for o in OPTION_SETS + SLAB_SETS:
            two, three, plans = ask_grid(ask, W, H, D, fp64, **o)
            assert (two, three) == expected_ids(W, fp64, **o), ((W, H, D, fp64), o)
            assert all(plans[k] == base[k] for k in plans), ((W, H, D, fp64), o)
            seen.add((bool(two), bool(three)))
    assert seen == {(True, True), (True, False), (False, False)}
    assert ask_grid(ask, *SLAB_GRID, whole=False, zh=2)[:2] == ([0, 8, 16, 64, 72, 80, 65, 73, 81], [])
    assert ask_grid(ask, 512, 512, 128, False, whole=False, zh=2)[:2] == ([0, 8, 16, 1, 9, 17, 2, 10, 18], [])
    assert ask_grid(ask, 512, 512, 128, False, whole=False, zh=3)[1] == [0, 8, 16, 1, 9, 17]
    assert ask_grid(ask, 2000, 8, 8, False)[:2] == ([], [])      # rows above 1024 cells: the single-sweep kernel only


def test_chunk_model_random_sweep(ask):
    rng = random.Random(5)
    cases = []
    for _ in range(6000):
        planes = rng.choice([rng.randint(1, 40), rng.randint(1, 300), rng.randint(1, 1100), 48, 128, 256, 512])
        nb = rng.choice([1, rng.randint(1, 20), rng.randint(1, 140), rng.randint(1, 600)])
        min_len, overlap = rng.choice([(12, 3), (16, 3), (16, 5)])
        slots = rng.choice([256, 256, 248, 240, 128, 64, 304, 7, 1])
        cases.append((planes, nb, rng.randint(0, 2), min_len, overlap, slots))
    got = ask(["chunk %d %d %d %d %d %d" % c for c in cases])
    assert len(got) == len(cases)
    bad = [(c, g) for c, g in zip(cases, got) if g != "chunk %d" % chunk_len(*c)]
    assert not bad, bad[:5]
    assert len({c[5] for c in cases}) >= 7 and sum(c[5] != 256 for c in cases) > 2000


def test_ids_round_trip(ask):
    lines = ask(["ids"])
    assert len(lines) == 128 + 32
    for line in lines:
        _, three, pid, kind, shape, alt, enc = (int(x) if i else x for i, x in enumerate(line.split()))
        assert enc == pid, line
        low = pid - FUSED2 if (not three and pid >= FUSED2) else pid
        assert (kind, shape, alt) == (2 if three else 1 if pid >= FUSED2 else 0, low % 8, low // 8), line


def _replay(ask, W, fp64, value, whole=True, zh=1, fuse=3):
    two, three = value.split(",")
    out = ask(["replay %d %d %d %d %d %s %s" % (W, 8 if fp64 else 4, whole, zh, fuse, two, three)])
    return tuple(int(x) for x in out[0].split()[1:])


def test_replay_check(ask):
    """The refusal matrix of test_gpu_launch_plans.py (test_plans_the_grid_does_not_have_are_refused), the ignored
    three-sweep id of its test_three_sweep_id_ignored_where_the_kernel_is_missing, and every plan a grid has."""
    refused = [(512, False, "0,2"), (256, False, "0,24"), (256, False, "24,-1"), (1024, False, "88,-1"), (300, False, "64,-1"),
               (600, False, "1,-1"), (200, True, "65,-1"), (200, True, "40,-1")]
    for W, fp64, value in refused:
        got = _replay(ask, W, fp64, value)
        assert REFUSE in got, (W, fp64, value, got)
        assert got[1] == (IGNORE if value.endswith(",-1") else REFUSE) and got[0] == (REFUSE if value.endswith(",-1") else USE)
    for W, fp64 in ((200, True), (600, False)):
        assert _replay(ask, W, fp64, "0,5") == (USE, IGNORE)
    assert _replay(ask, 256, False, "-1,-1") == (IGNORE, IGNORE)
    assert _replay(ask, 256, False, "3,-1") == (REFUSE, IGNORE)      # the 16-wave shape is no plan id: option pair_shape = 3
    assert _replay(ask, 512, False, "0,0", fuse=2) == (USE, IGNORE) and _replay(ask, 512, False, "0,-1", fuse=1) == (REFUSE, IGNORE)
    assert _replay(ask, 512, False, "0,0", whole=False, zh=2) == (USE, IGNORE)
    assert _replay(ask, 512, False, "0,0", whole=False, zh=1) == (REFUSE, IGNORE)
    for W, H, D, fp64 in ALL_GRIDS:
        for p in plan_list(W, fp64):
            assert _replay(ask, W, fp64, p[1]) == (USE, USE if p[0] == "three" else IGNORE), (W, fp64, p)


def test_plan_table_and_chunk_models():
    """The grids of test_gpu_launch_plans.py reach every instantiation of the table in its docstring, and on every grid 48 planes
    deep each kernel's three alts give at least two (here: three) different chunk counts, so that alt 1 and 2 are not alt 0
    again."""
    reached = set()
    for W, H, D, fp64 in GRIDS:
        for kind, _, _, _, _, NL, BY, alt in plan_list(W, fp64):
            reached.add((kind, fp64, (W + 255) // 256 if kind == "pair" else W <= 256 if kind != "fused" or fp64 else W <= 768, BY))
        if D >= 48:
            for kind, _, _, _, _, NL, BY, _ in plan_list(W, fp64):
                counts = {(D + model_chunk_len(kind, H, D, NL, BY, a) - 1) // model_chunk_len(kind, H, D, NL, BY, a) for a in range(3)}
                assert len(counts) >= 2, (W, H, D, kind, BY, counts)
    pair32 = {(n, by) for k, f, n, by in reached if k == "pair" and not f}
    assert pair32 == {(1, 24), (1, 16), (1, 20), (2, 12), (2, 8), (2, 10), (3, 8), (4, 6)}
    assert {(n, by) for k, f, n, by in reached if k == "pair" and f} == {(1, 16), (2, 8), (3, 6), (4, 4)}
    assert {(s, by) for k, f, s, by in reached if k == "three"} == {(True, 20), (True, 16), (True, 12), (False, 12), (False, 10)}
    assert {(s, by) for k, f, s, by in reached if k == "fused" and not f} == {(True, 8), (False, 8), (False, 9)}
    assert {(s, by) for k, f, s, by in reached if k == "fused" and f} == {(True, 20), (False, 10), (False, 8)}
    # a few values of the models, worked by hand: 48 planes, one band, 256 slots -> as many chunks as allowed, then fewer
    assert [chunk_len(48, 1, a, 16, 5) for a in range(3)] == [16, 24, 48]
    assert [chunk_len(48, 1, a, 12, 3) for a in range(3)] == [12, 16, 24]
    assert [chunk_len(10, 3, a, 16, 5) for a in range(3)] == [10, 10, 10]
