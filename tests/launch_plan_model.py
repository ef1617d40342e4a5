"""The launch plans of the two- and three-sweep Jacobi kernels, restated independently of the library: the id table, the
band heights, the launchers' z-chunk model and the grids the plan tests run.  tests/test_launch_plan_cpu.py holds
csrc/launch_plan.h to this restatement line by line; tests/test_gpu_launch_plans.py builds its cases and masks from it."""

FUSED2 = 64


# ---- the plan table ------------------------------------------------------------------------------------------------------
# (shape id, band height BY) per kernel, by precision and row width: the pair kernel (kernels.hip, BY = 2 NY) and the fused
# kernel (sweep_fused.hip, BY = NY RY)
def pair_shapes(W, fp64):
    nxw = (W + 255) // 256
    if fp64:
        return [(0, {1: 16, 2: 8, 3: 6, 4: 4}[nxw])]
    return {1: [(0, 24), (1, 16), (2, 20)], 2: [(0, 12), (1, 8), (2, 10)], 3: [(0, 8)], 4: [(0, 6)]}[nxw]


def fused2_shapes(W, fp64):
    if fp64:
        return [(0, 20)] if W <= 256 else [(0, 10), (1, 8)] if W <= 512 else []
    return [] if W <= 512 else [(0, 8)] if W <= 768 else [(0, 8), (1, 9)]


def three_shapes(W, fp64):
    if fp64 or W > 512:
        return []
    return [(0, 20), (1, 16), (2, 12)] if W <= 256 else [(0, 12), (1, 10)]


def plan_list(W, fp64):
    """(kind, launch_plans value, expected pair_shape, triple_plan, two_sweep_fused, NL, BY, alt) of every plan of a grid."""
    out = []
    for shape, by in pair_shapes(W, fp64):
        for alt in range(3):
            pid = shape + 8 * alt
            out.append(("pair", "%d,-1" % pid, pid, -1, 0, 2, by, alt))
    for shape, by in fused2_shapes(W, fp64):
        for alt in range(3):
            pid = FUSED2 + shape + 8 * alt
            out.append(("fused", "%d,-1" % pid, pid, -1, 1, 2, by, alt))
    for shape, by in three_shapes(W, fp64):
        for alt in range(3):
            tid = shape + 8 * alt
            out.append(("three", "0,%d" % tid, 0, tid, 0, 3, by, alt))
    return out


# ---- the launchers' z-chunk model (kernels.hip launch_pair_v, sweep_fused.hip launch_fused_v) ---------------------------------
def chunk_len(planes, nbands, alt, min_len, extra, slots=256):
    """Planes per z chunk the launcher picks for `alt`: the alt-th best chunk count by filled CU slots x useful planes."""
    eff, cnt = [-1.0] * 3, [1] * 3
    nzc = 1
    while nzc <= 64 and (nzc == 1 or planes // nzc >= min_len):
        blocks = nbands * nzc
        rounds = (blocks + slots - 1) // slots
        ln = (planes + nzc - 1) // nzc
        e = blocks / (rounds * slots) * ln / (ln + extra)
        for k in range(3):
            if e > eff[k] + 1e-9:
                eff[k + 1:], cnt[k + 1:] = eff[k:2], cnt[k:2]
                eff[k], cnt[k] = e, nzc
                break
        nzc += 1
    pick = alt
    while pick > 0 and eff[pick] < 0.0:
        pick -= 1
    return (planes + cnt[pick] - 1) // cnt[pick]


def nbands(H, BY, NL):
    step = BY - 2 * (NL - 1)
    return (H + step - 1) // step


def model_chunk_len(kind, H, D, NL, BY, alt):
    if kind == "pair":
        return chunk_len(D, nbands(H, BY, 2), alt, 12, 3)
    return chunk_len(D, nbands(H, BY, NL), alt, 16, 2 * NL - 1)


# ---- the grids of tests/test_gpu_launch_plans.py ---------------------------------------------------------------------------
GRIDS = [
    # three-sweep fp32: ragged <= 256, exactly 256, ragged 257..511, exactly 512 (and the pair kernel's nxw = 1, 2)
    (200, 40, 48, False), (256, 40, 48, False), (300, 40, 48, False), (512, 40, 48, False),
    # two-sweep fused fp32: 513..768, 769..1024 (pair nxw = 3, 4)
    (600, 20, 48, False), (768, 20, 48, False), (800, 20, 48, False), (1024, 20, 48, False),
    # fp64: fused <= 256, 257..512 (ragged and aligned); pair nxw = 1..4
    (200, 40, 48, True), (300, 30, 48, True), (512, 30, 48, True), (700, 16, 48, True), (1024, 16, 48, True),
    # degenerate: H = 1..3, D shorter than one chunk
    (256, 1, 5, False), (300, 2, 9, False), (1000, 3, 7, False), (100, 3, 6, True), (600, 1, 10, True),
]

RB_GRIDS = [(100, 30, 48, False), (300, 20, 48, False), (700, 12, 36, False), (1000, 9, 36, False), (100, 30, 48, True),
            (300, 20, 36, True)]

MG_GRID = (128, 64, 64, False)   # test_multigrid_under_every_pair_plan
