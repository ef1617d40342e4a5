"""The rough advection inputs of tests/advect_model.py on the CPU: every class of back-trace that a kernel form of
csrc/advect.hip treats differently holds at least FLOOR cells at every (grid, window radius) pair the GPU test
(tests/test_gpu_advect_rough.py) leans on, the oracle stays finite and non-trivial under them, and the restated
tile_window() gives the radii the LDS cap leaves.  The counts recorded here are the ones the GPU module's coverage table
quotes; they come from the numpy model alone."""
import numpy as np
import pytest

import advect_model as M

ORDER = ("fluid",) + M.CLASSES
# classify() of the recipe (seed M.SEED) per (grid, R), columns as ORDER: the per-pass advections, prev = the velocity itself
PASS_COUNTS = {
    ((70, 33, 21), 1): [47068, 6060, 5884, 11936, 23188, 11846, 5110, 5001, 5347, 5179, 1289, 1262, 1267, 1382],
    ((70, 33, 21), 4): [47068, 7638, 4306, 11936, 23188, 11846, 5110, 5001, 5347, 5179, 1289, 1262, 1267, 1382],
    ((70, 33, 21), 24): [47068, 11784, 160, 11936, 23188, 11846, 5110, 5001, 5347, 5179, 1289, 1262, 1267, 1382],
    ((12, 80, 11), 1): [10259, 1357, 1495, 2825, 4582, 2545, 1078, 1030, 1265, 1275, 305, 277, 339, 336],
    ((12, 80, 11), 21): [10259, 2331, 521, 2825, 4582, 2545, 1078, 1030, 1265, 1275, 305, 277, 339, 336],
    ((12, 80, 11), 24): [10259, 2401, 451, 2825, 4582, 2545, 1078, 1030, 1265, 1275, 305, 277, 339, 336],
    ((256, 9, 70), 1): [156513, 21667, 17662, 39194, 77990, 39054, 20271, 20511, 15988, 16014, 5029, 5138, 4032, 4010],
    ((256, 9, 70), 24): [156513, 34125, 5204, 39194, 77990, 39054, 20271, 20511, 15988, 16014, 5029, 5138, 4032, 4010],
    ((256, 9, 70), 32): [156513, 36321, 3008, 39194, 77990, 39054, 20271, 20511, 15988, 16014, 5029, 5138, 4032, 4010],
}
# classify_step() of the first step from the same state (oracle acc = 4): the traces of all three sources of the velocity
# advection, and the lo_out traces of each source (v_x, v_y, v_z)
STEP_COUNTS = {
    ((70, 33, 21), 1): ([47068, 22142, 16722, 27490, 74850, 27684, 11276, 10762, 13147, 12822, 2923, 2003, 3005, 2711], [5400, 6299, 5023]),
    ((70, 33, 21), 4): ([47068, 28779, 10085, 27490, 74850, 27684, 11276, 10762, 13147, 12822, 2923, 2003, 3005, 2711], [3251, 4178, 2656]),
    ((70, 33, 21), 24): ([47068, 38648, 216, 27490, 74850, 27684, 11276, 10762, 13147, 12822, 2923, 2003, 3005, 2711], [42, 174, 0]),
    ((12, 80, 11), 1): ([10259, 4947, 4845, 5823, 15162, 5502, 2384, 2330, 3335, 3203, 631, 490, 876, 787], [2014, 1343, 1488]),
    ((12, 80, 11), 21): ([10259, 8916, 876, 5823, 15162, 5502, 2384, 2330, 3335, 3203, 631, 490, 876, 787], [352, 474, 50]),
    ((12, 80, 11), 24): ([10259, 9063, 729, 5823, 15162, 5502, 2384, 2330, 3335, 3203, 631, 490, 876, 787], [285, 413, 31]),
    ((256, 9, 70), 1): ([156513, 65139, 64895, 90752, 248753, 91093, 38559, 38685, 34554, 34310, 9925, 7215, 9122, 6684], [19143, 26225, 19527]),
    ((256, 9, 70), 24): ([156513, 121033, 9001, 90752, 248753, 91093, 38559, 38685, 34554, 34310, 9925, 7215, 9122, 6684], [1275, 1692, 6034]),
    ((256, 9, 70), 32): ([156513, 125467, 4567, 90752, 248753, 91093, 38559, 38685, 34554, 34310, 9925, 7215, 9122, 6684], [412, 577, 3578]),
}
TABLE_DTYPE = {(70, 33, 21): np.float32, (12, 80, 11): np.float64, (256, 9, 70): np.float32}
CASES = [((70, 33, 21), np.float32), ((70, 33, 21), np.float64), ((12, 80, 11), np.float64), ((12, 80, 11), np.float32),
         ((256, 9, 70), np.float32)]


def test_tile_window_model():
    """the table of the LDS cap: 64 KB / (nf * itemsize) >= (9 + 2 r)^2"""
    assert [M.tile_window(128, nf, size) for size in (4, 8) for nf in (1, 3)] == [59, 32, 40, 21]
    for nf, size, r in ((1, 4, 59), (3, 4, 32), (1, 8, 40), (3, 8, 21)):
        assert nf * (9 + 2 * r) ** 2 * size <= 65536 < nf * (9 + 2 * (r + 1)) ** 2 * size
    # below the cap the radius is what was asked for, and never below 1
    assert [M.tile_window(w, 3, 8) for w in (0, 1, 4, 21, 22, 24)] == [1, 1, 4, 21, 21, 21]
    assert [M.tile_window(w, 1, 8) for w in (24, 40, 41)] == [24, 40, 40]
    assert [M.tile_window(w, 3, 4) for w in (24, 32, 33)] == [24, 32, 32]


def test_recipe_is_what_it_says():
    W, H, D = 70, 33, 21
    ux, uy, uz, src = M.rough_fields(W, H, D, M.SEED, np.float64)
    assert ux.shape == uy.shape == uz.shape == src.shape == (D + 2, H + 2, W + 2)
    for value in (2 / M.DT, -2 / M.DT, 0.0):
        assert abs(np.mean(ux[1:-1, 1:-1, 1:-1] == value) - 0.25) < 0.01
    edges = M.box_edges(W, H, D)
    assert edges.sum() == 4 * (W + H + D) + 8 and edges[0, 0, 5] and edges[3, H + 1, W + 1] and not edges[0, 4, 5]
    for a in (ux, uy, uz, src):
        assert not a[edges].any() and np.count_nonzero(a[0, 1:-1, 1:-1]) > 0.7 * W * H      # faces random, edges 0
    assert np.abs(ux).max() == 2 / M.DT
    for a32, a64 in zip(M.rough_fields(W, H, D, M.SEED, np.float32), (ux, uy, uz, src)):
        assert a32.dtype == np.float32 and np.array_equal(a32, a64.astype(np.float32))
    m = M.rough_mask(W, H, D, M.SEED)
    assert not m[0].any() and not m[-1].any() and not m[:, 0].any() and not m[:, -1].any()
    assert not m[:, :, 0].any() and not m[:, :, -1].any()
    assert m[:, :, 1].any() and m[:, :, W].any() and m[:, 1].any() and m[:, H].any() and m[1].any() and m[D].any()
    assert abs(m[1:-1, 1:-1, 1:-1].mean() - 0.03) < 0.005


@pytest.mark.parametrize("shape,dtype", CASES)
def test_every_class_reaches_the_floor(shape, dtype):
    W, H, D = shape
    ux, uy, uz, _ = M.rough_fields(W, H, D, M.SEED, dtype)
    mask = M.rough_mask(W, H, D, M.SEED)
    for R in M.FLOOR_R[shape]:
        c = M.classify(W, H, D, ux, uy, uz, mask, R, dtype)
        print(shape, np.dtype(dtype).name, "R", R, c)
        M.assert_floors(c, "%s R %d" % (shape, R))
        assert c["lo_in"] + c["lo_out"] + c["hi"] + c["mid"] == c["fluid"]
        if dtype == TABLE_DTYPE[shape]:
            assert [c[k] for k in ORDER] == PASS_COUNTS[(shape, R)]


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_tiny_grid(dtype):
    W, H, D = M.TINY
    ux, uy, uz, _ = M.rough_fields(W, H, D, M.SEED, dtype)
    c = M.classify(W, H, D, ux, uy, uz, M.rough_mask(W, H, D, M.SEED), 1, dtype)
    print(M.TINY, c)
    M.assert_tiny(c)


def test_outlet_only_flow_reads_side_one_everywhere():
    W, H, D = 70, 33, 21
    ux, uy, uz, _ = M.rough_fields(W, H, D, M.SEED, np.float32)
    ux[~M.box_edges(W, H, D)] = -2 / M.DT                  # (the edges of the box stay 0, see rough_fields)
    c = M.classify(W, H, D, ux, uy, uz, M.rough_mask(W, H, D, M.SEED), 1, np.float32)
    assert c["hi"] == c["fluid"] > 0 and c["lo_in"] == c["lo_out"] == c["mid"] == 0
    assert c["hi_yhi"] >= M.FLOOR and c["hi_zlo"] >= M.FLOOR


def test_classifier_on_hand_traces():
    """one cell per class on a 16 x 16 x 16 grid, R = 1: the tile of cell (y, z) = (12, 12) is rows 9..16, its window 8..17"""
    W = H = D = 16
    dt = 1.0 / 16                                           # k = dt N = 1: a velocity is a distance in cells, exactly
    z = np.zeros((D + 2, H + 2, W + 2), dtype=np.float32)
    mask = np.ones(z.shape, dtype=bool)                     # everything solid but the cells under test
    want = {}

    def put(x, y, zc, dx, dy, dz, *classes):
        mask[zc, y, x] = False
        ux[zc, y, x], uy[zc, y, x], uz[zc, y, x] = dx, dy, dz
        for c in classes:
            want[c] = want.get(c, 0) + 1

    ux, uy, uz = z.copy(), z.copy(), z.copy()
    put(3, 12, 12, 40, 0, 0, "lo_in")                       # clamps low, stays in its row and plane
    put(4, 12, 12, 40, 4, 0, "lo_in")                       # y0 = 8 = the window's first row
    put(5, 12, 12, 40, 4.5, 0, "lo_out")                    # y0 = 7: one row below the window
    put(6, 12, 12, 40, -4.5, 0, "lo_in", "yhi")             # py = 16.5: y0 + 1 = 17, the last row of window and table
    put(7, 12, 12, 40, 0, 5, "lo_out")                      # z0 = 7
    put(8, 12, 12, -40, 0, 0, "hi")
    put(9, 12, 12, 2, 0, 0, "mid", "mid_int")
    put(10, 12, 12, 2.25, 0, 0, "mid")
    put(11, 12, 12, 40, 40, 0, "lo_out", "ylo", "lo_ylo")
    put(12, 12, 12, -40, -40, 0, "hi", "yhi", "hi_yhi")
    put(13, 12, 12, 40, 0, -40, "lo_in", "zhi", "lo_zhi")
    put(14, 12, 12, -40, 0, 40, "hi", "zlo", "hi_zlo")
    got = M.classify(W, H, D, ux, uy, uz, mask, 1, np.float32, dt)
    assert got["fluid"] == 12
    assert {c: got[c] for c in M.CLASSES} == {c: want.get(c, 0) for c in M.CLASSES}


@pytest.mark.parametrize("shape,dtype", CASES + [(M.TINY, np.float32), (M.TINY, np.float64)])
def test_oracle_under_the_rough_flow(oracle_mod, shape, dtype):
    """The four per-pass advections and three whole steps on the oracle: finite, non-trivial, |v| <= 2 / dt (an advected
    value is a convex combination of source values, the inlet's 30 is below the recipe's 40).  On the floor grids the first
    step's velocity advection also holds every class, counted over the traces of its three sources."""
    O = oracle_mod
    W, H, D = shape
    fp64 = dtype == np.float64
    ux, uy, uz, src = M.rough_fields(W, H, D, M.SEED, dtype)
    mask = M.rough_mask(W, H, D, M.SEED)
    ora = O.Oracle(W, H, D, solver=O.JACOBI, fp64=fp64, acc=4)
    ora.set_mask(mask)
    for b, field, prev in ((0, O.DENS, O.BUF), (1, O.VX, O.VX0), (2, O.VY, O.VY0), (3, O.VZ, O.VZ0)):
        for f, a in ((O.VX, ux), (O.VY, uy), (O.VZ, uz)):
            ora.set(f, a)
        source = src if b == 0 else (ux, uy, uz)[b - 1]
        ora.set(prev, source)
        ora.advect(b, field, prev)
        got = ora.get(field)
        assert np.isfinite(got).all() and np.abs(got).max() > 0.5
        assert np.abs(got).max() <= np.abs(source).max()
    for f, a in ((O.VX, ux), (O.VY, uy), (O.VZ, uz), (O.DENS, np.abs(src))):
        ora.set(f, a)
    for step in range(3):
        ora.run_one()
        for f in range(11):
            assert np.isfinite(ora.get(f)).all(), (step, O.FIELD_NAMES[f])
            assert not ora.get(f)[M.box_edges(W, H, D)].any(), (step, O.FIELD_NAMES[f])    # nobody writes the edges
        vmax = max(np.abs(ora.get(f)).max() for f in (O.VX, O.VY, O.VZ))
        print(shape, np.dtype(dtype).name, "step", step + 1, "max |v|", vmax, "max dens", ora.get(O.DENS).max())
        assert 1.0 < vmax <= 2 / M.DT
        assert ora.get(O.DENS).max() > 0.1
    ora.close()
    if shape == M.TINY:
        return
    rep = O.Oracle(W, H, D, solver=O.JACOBI, fp64=fp64, acc=4)
    carriers = M.step_carriers(rep, ux, uy, uz, mask)
    rep.close()
    for R in M.FLOOR_R[shape]:
        total, parts = M.classify_step(W, H, D, carriers, mask, R, dtype)
        print(shape, np.dtype(dtype).name, "step 1, R", R, total, "lo_out per source", [p["lo_out"] for p in parts])
        M.assert_floors(total, "step 1 of %s R %d" % (shape, R))
        if dtype == TABLE_DTYPE[shape]:
            assert ([total[k] for k in ORDER], [p["lo_out"] for p in parts]) == STEP_COUNTS[(shape, R)]
