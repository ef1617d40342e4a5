"""Every launch plan of the Jacobi sweep kernels, forced through "launch_plans", against the CPU oracle bit for bit.

On each grid the host times the workgroup shapes of the two-sweep kernels (jacobi_pair_kernel, kernels.hip, and
jacobi_fused_kernel<NL = 2>, sweep_fused.hip) and of the three-sweep kernel (jacobi_fused_kernel<NL = 3>), each with the
three best z-chunk counts of its launcher's model, and keeps the fastest (fluidsim.cpp, choose_launch_plans).  Every plan
must compute the same bits, but the suite's other tests only ever run the plan that won on the test box's clock.  Here
each plan is replayed with launch_plans = "<two-sweep id>,<three-sweep id>":

    pair kernel               id = shape + 8 alt
    two-sweep fused kernel    id = 64 + shape + 8 alt
    three-sweep kernel        id = shape + 8 alt            (alt = 0, 1, 2: which of the three best chunk counts)

The id table is written out in launch_plan_model.py, not read back from the library (test_launch_plan_cpu.py holds the
library's table, csrc/launch_plan.h, to it).  Which instantiation each id reaches, and the case that runs it (test ids are
test_jacobi_plan[<grid>-<kernel><id>-acc<acc>]; a grid id is W x H x D and precision):

  instantiation (SHAPE_TABLE entry)                 rows          shape ids    grids that run it
  kernels.hip launch_jacobi_pair<float>
    Build<2, 1, 12, 2>                           <= 256        0            200x40x48, 256x40x48, 256x1x5 (fp32)
    Build<2, 1, 8, 2>                            <= 256        1            same
    Build<2, 1, 10, 2>                           <= 256        2            same
    Build<2, 1, 16, 2> (pair_shape = 3 only)     <= 256        0, 8, 16     test_pair_shape_16_waves[200]   
    Build<2, 2, 6, 2>                            257..512      0            300x40x48, 512x40x48, 300x2x9 (fp32)
    Build<2, 2, 4, 2>                            257..512      1            same
    Build<2, 2, 5, 2>                            257..512      2            same
    Build<2, 2, 8, 2>  (pair_shape = 3 only)     257..512      0, 8, 16     test_pair_shape_16_waves[300]   
    Build<2, 3, 4, 2>                            513..768      0            600x20x48, 768x20x48 (fp32)
    Build<2, 4, 3, 2>                            769..1024     0            800x20x48, 1024x20x48, 1000x3x7 (fp32)
  kernels.hip launch_jacobi_pair<double>
    Build<2, 1, 8, 2>                            <= 256        0            200x40x48, 100x3x6 (fp64)
    Build<2, 2, 4, 2>                            257..512      0            300x30x48, 512x30x48 (fp64)
    Build<2, 3, 3, 2>                            513..768      0            700x16x48, 600x1x10 (fp64)
    Build<2, 4, 2, 2>                            769..1024     0            1024x16x48 (fp64)
  sweep_fused.hip launch_jacobi_fused<float>, three sweeps (the three-sweep id)
    Build<3, 1, 10, 2>  20-row bands           <= 256        0            200x40x48, 256x40x48, 256x1x5 (fp32)
    Build<3, 1, 8, 2>   16-row bands           <= 256        1            same
    Build<3, 1, 6, 2>   12-row bands           <= 256        2            same
    Build<3, 2, 6, 2>   12-row bands           257..512      0            300x40x48, 512x40x48, 300x2x9 (fp32)
    Build<3, 2, 5, 2>   10-row bands           257..512      1            same
  sweep_fused.hip launch_jacobi_fused<float>, two sweeps (the two-sweep id, 64 + ...)
    Build<2, 3, 4, 2>   8-row bands            513..768      0            600x20x48, 768x20x48 (fp32)
    Build<2, 4, 4, 2>   8-row bands            769..1024     0            800x20x48, 1024x20x48, 1000x3x7 (fp32)
    Build<2, 4, 3, 3>   9-row bands            769..1024     1            same
  sweep_fused.hip launch_jacobi_fused<double> (two sweeps, 64 + ...)
    Build<2, 1, 10, 2>  20-row bands           <= 256        0            200x40x48, 100x3x6 (fp64)
    Build<2, 2, 5, 2>   10-row bands           257..512      0            300x30x48, 512x30x48 (fp64)
    Build<2, 2, 4, 2>   8-row bands            257..512      1            same

(The timing-only ablation build of launch_jacobi_fused<float>, sweep_abl = 16, is wrong at the walls by design and left
out.)  Each plan runs with acc 7 and 8: passes [3, 3, 1] and [3, 3, 2] of the three-sweep kernel, [2, 2, 2, 1] and
[2, 2, 2, 2] of a two-sweep kernel.  The grids are 48 planes deep, so that the three alts give three different chunk counts
(checked against a restatement of the launchers' chunk models), and the masks are made from each plan's band and chunk
geometry (_geometry_mask).  The mask-free and wall-free bodies of the three-sweep kernel get their own cases, so do the
red-black and damped passes of solver = rbsor / mg (they reuse the pair plan), the single-sweep kernel's options, the
per-cell projection kernels and the host's refusal of plans a grid does not have.
"""
import hashlib

import numpy as np
import pytest

from conftest import bits_equal
from launch_plan_model import FUSED2, GRIDS, RB_GRIDS, model_chunk_len, nbands, plan_list, three_shapes

pytestmark = pytest.mark.gpu

JACOBI_ACCS = (7, 8)


@pytest.fixture(scope="module")
def F():
    import fluid_simulation_amd as F
    return F


# ---- masks from the plans' geometry ----------------------------------------------------------------------------------------
def _geometry_mask(W, H, D, plans):
    """Solids where a plan's bands and chunks meet: on the rows two neighbouring bands share, one row beyond either band edge
    (a near-solid ring reaching into the other band), on the planes either side of each chunk boundary (the chunk count
    each alt gives), in all eight corners (next to all six walls), and a plate one cell thick."""
    m = np.zeros((D + 2, H + 2, W + 2), dtype=bool)
    xs = sorted({1, max(1, W // 3), max(1, W // 2), max(1, 2 * W // 3 + 1), W})

    def put(z, y, x):
        if 1 <= z <= D and 1 <= y <= H and 1 <= x <= W:
            m[z, y, x] = True

    seen = set()
    i = 0
    for kind, _, _, _, _, NL, BY, alt in plans:
        OV = NL - 1
        step = BY - 2 * OV
        if (NL, BY) not in seen:
            seen.add((NL, BY))
            for k in range(min(3, nbands(H, BY, NL) - 1)):
                s0, s1 = k * step - (OV - 1), (k + 1) * step - (OV - 1)
                z = 1 + (5 * i + 7 * k) % D
                x = xs[(i + k) % len(xs)]
                for y in range(s1, s0 + BY):                     # rows bands k and k + 1 share
                    put(z, y, x)
                    put(z, y, min(W, x + 1))
                put(1 + (z + 11) % D, s0 + BY, xs[(i + k + 1) % len(xs)])     # ring into band k from above
                put(1 + (z + 17) % D, s1 - 1, xs[(i + k + 2) % len(xs)])      # ring into band k + 1 from below
            i += 1
        zc = model_chunk_len(kind, H, D, NL, BY, alt)
        for c in range(1, (D + zc - 1) // zc):                  # last plane of chunk c - 1, first of chunk c
            y = 1 + (3 * c + BY) % H
            put(c * zc, y, xs[c % len(xs)])
            put(c * zc + 1, y, xs[(c + 1) % len(xs)])
    for z in (1, D):
        for y in (1, H):
            for x in (1, W):
                m[z, y, x] = True
    if W >= 3 and H >= 3 and D >= 3:
        m[D // 4 + 1:3 * D // 4 + 1, H // 4 + 1:3 * H // 4 + 1, 2 * W // 3 + 1] = True
    return m


def _masks(W, H, D, plans):
    return {"geometry": _geometry_mask(W, H, D, plans), "tunnel": np.zeros((D + 2, H + 2, W + 2), dtype=bool)}


# ---- oracle runs, shared by every plan of a grid ------------------------------------------------------------------------------
_ORACLE = {}


def oracle_fields(O, W, H, D, fp64, mask_name, mask, acc, solver="jacobi", omega=None, mg=None):
    key = (W, H, D, fp64, mask_name, hashlib.sha256(np.packbits(mask).tobytes()).hexdigest(), acc, solver, omega, mg)
    if key not in _ORACLE:
        sol = {"jacobi": O.JACOBI, "rbsor": O.RBSOR, "mg": O.MG}[solver]
        kw = {}
        if omega is not None:
            kw["omega"] = omega
        if mg is not None:
            kw["mg"] = mg
        ora = O.Oracle(W, H, D, solver=sol, fp64=fp64, threads=4, acc=acc, **kw)
        ora.set_mask(mask)
        for _ in range(2):
            ora.run_one()
        _ORACLE[key] = [ora.get(f) for f in range(11)]
        ora.close()
    return _ORACLE[key]


def run_sim(F, W, H, D, fp64, mask, acc, opts, solver="jacobi"):
    sim = F.Simulation(W, H, D, 1, acc=acc, quiet=1, solver=solver, precision="fp64" if fp64 else "fp32")
    for k, v in opts.items():
        sim.set_option(k, v)
    sim.set_mask(mask)
    for _ in range(2):
        sim.run_one()
    out = [sim.get(f) for f in range(11)]
    got = (sim._geti("pair_shape"), sim._geti("triple_plan"), sim._geti("two_sweep_fused"))
    sim.close()
    return out, got


def assert_same(F, got, want, what):
    for f in range(11):
        assert bits_equal(got[f], want[f]), "%s: %s differs from the oracle" % (what, F.FIELD_NAMES[f])


# ---- part 1: every plan of every kernel -----------------------------------------------------------------------------------
def _grid_id(W, H, D, fp64):
    return "%dx%dx%d-%s" % (W, H, D, "fp64" if fp64 else "fp32")


def _jacobi_cases():
    cases = []
    for W, H, D, fp64 in GRIDS:
        for p in plan_list(W, fp64):
            for acc in JACOBI_ACCS:
                cases.append(pytest.param(W, H, D, fp64, p, acc, id="%s-%s%s-acc%d" % (
                    _grid_id(W, H, D, fp64), p[0], p[1].split(",")[0 if p[0] != "three" else 1], acc)))
    return cases


@pytest.mark.parametrize("W,H,D,fp64,plan,acc", _jacobi_cases())
def test_jacobi_plan(F, oracle_mod, W, H, D, fp64, plan, acc):
    """One forced plan, two steps, all 11 fields against the oracle; the library reports the plan it replayed.  The
    three-sweep plans also run in an empty tunnel (the mask-free body throughout, where it is on)."""
    kind, value, want_pair, want_triple, want_fused = plan[:5]
    plans = plan_list(W, fp64)
    masks = _masks(W, H, D, plans)
    for name in (("geometry", "tunnel") if kind == "three" else ("geometry",)):
        ref = oracle_fields(oracle_mod, W, H, D, fp64, name, masks[name], acc)
        got, rep = run_sim(F, W, H, D, fp64, masks[name], acc, {"launch_plans": value})
        assert rep == (want_pair, want_triple, want_fused), "%s: reported %s" % (value, rep)
        assert_same(F, got, ref, "%s %s launch_plans=%s acc=%d mask=%s" % (_grid_id(W, H, D, fp64), kind, value, acc, name))


# ---- part 2: mask-free and wall-free builds of every three-sweep shape ------------------------------------------------------------
def _mask_free_cases():
    cases = []
    for W, mf in ((512, "auto"), (256, "1")):
        for shape, by in three_shapes(W, False):
            for alt in range(3):
                for wf in ("0", "1"):
                    for cost in ("0", "14,10,9"):
                        cases.append(pytest.param(W, mf, shape + 8 * alt, wf, cost, id="W%d-BY%d-three%d-wall_free%s-cost%s" % (
                            W, by, shape + 8 * alt, wf, cost.replace(",", "_"))))
    return cases


@pytest.mark.parametrize("W,mask_free,tid,wall_free,cost", _mask_free_cases())
def test_three_sweep_mask_free_builds(F, oracle_mod, W, mask_free, tid, wall_free, cost):
    H, D, acc = 40, 48, 8
    masks = _masks(W, H, D, plan_list(W, False))
    opts = {"launch_plans": "0,%d" % tid, "mask_free": mask_free, "wall_free": wall_free, "chunk_cost": cost}
    for name in ("geometry", "tunnel"):
        ref = oracle_fields(oracle_mod, W, H, D, False, name, masks[name], acc)
        got, rep = run_sim(F, W, H, D, False, masks[name], acc, opts)
        assert rep == (0, tid, 0), rep
        assert_same(F, got, ref, "%dx%dx%d %s mask=%s" % (W, H, D, opts, name))


@pytest.mark.parametrize("W,mask_free", [(256, "1"), (512, "auto")])
def test_three_sweep_plans_switched_on_one_handle(F, W, mask_free):
    """launch_plans changed between steps of one handle, with mask changes in between: the mask-free build's per-launch-shape
    chunk tables (MaskPlan::chunks) are made per shape, reused when a shape comes back and dropped when the mask changes.
    Against the single-sweep kernel on the same sequence."""
    H, D = 40, 48
    geo = _geometry_mask(W, H, D, plan_list(W, False))
    geo2 = geo.copy()
    geo2[D // 2:D // 2 + 2, 5:H - 5, W // 2] = True
    tunnel = np.zeros_like(geo)
    n = len(three_shapes(W, False))
    seq = [(0, geo), (1, geo), (n - 1 + 8, geo), (0, geo), (17, tunnel), (1, tunnel), (0, tunnel), (9, geo2), (0, geo2), (16, geo)]

    def run(opts, forced):
        sim = F.Simulation(W, H, D, 1, acc=8, quiet=1, **opts)
        last = None
        seen = []
        for tid, m in seq:
            if forced:
                sim.set_option("launch_plans", "0,%d" % tid)
            if m is not last:
                sim.set_mask(m)
                last = m
            sim.run_one()
            if forced:
                seen.append(sim._geti("triple_plan"))
        out = [sim.get(f) for f in range(11)]
        sim.close()
        return out, seen

    ref, _ = run({"sweep_fuse": "1"}, False)
    for cost in ("0", "14,10,9"):
        got, seen = run({"mask_free": mask_free, "chunk_cost": cost}, True)
        assert seen == [t for t, _ in seq]
        assert_same(F, got, ref, "%dx%dx%d switched plans, chunk_cost %s" % (W, H, D, cost))


# ---- part 3: rbsor and multigrid under every pair plan ---------------------------------------------------------------------------
@pytest.mark.parametrize("W,H,D,fp64", RB_GRIDS, ids=[_grid_id(*g) for g in RB_GRIDS])
def test_rbsor_under_every_pair_plan(F, oracle_mod, W, H, D, fp64):
    acc, omega = 5, 1.6
    plans = [p for p in plan_list(W, fp64) if p[0] == "pair"]
    m = _geometry_mask(W, H, D, plans)
    ref = oracle_fields(oracle_mod, W, H, D, fp64, "geometry", m, acc, solver="rbsor", omega=omega)
    for p in plans:
        got, rep = run_sim(F, W, H, D, fp64, m, acc, {"launch_plans": p[1], "sor_omega": omega}, solver="rbsor")
        assert rep[0] == p[2], rep
        assert_same(F, got, ref, "%s rbsor launch_plans=%s" % (_grid_id(W, H, D, fp64), p[1]))


def test_multigrid_under_every_pair_plan(F, oracle_mod):
    """solver=mg: the damped level-0 passes run the pair plan (plan_two_pair); 128x64x64 has four levels."""
    W, H, D, acc, mg = 128, 64, 64, 5, (2, 1, 1, 30)
    plans = [p for p in plan_list(W, False) if p[0] == "pair"]
    m = _geometry_mask(W, H, D, plans)
    ref = oracle_fields(oracle_mod, W, H, D, False, "geometry", m, acc, solver="mg", mg=mg)
    for p in plans:
        opts = {"launch_plans": p[1], "mg_cycles": mg[0], "mg_pre": mg[1], "mg_post": mg[2], "mg_coarse_iters": mg[3]}
        got, rep = run_sim(F, W, H, D, False, m, acc, opts, solver="mg")
        assert rep[0] == p[2], rep
        assert_same(F, got, ref, "mg launch_plans=%s" % p[1])


# ---- part 5: options that claim identical bits -----------------------------------------------------------------------------------
SWEEP_GRIDS = [(1, 3, 7), (255, 17, 7), (257, 1, 9), (513, 5, 7), (1024, 3, 6), (256, 5, 8), (1, 17, 5)]


@pytest.mark.parametrize("fp64", [False, True], ids=["fp32", "fp64"])
@pytest.mark.parametrize("W,H,D", SWEEP_GRIDS)
def test_single_sweep_kernel_options(F, oracle_mod, W, H, D, fp64):
    """sweep_fuse = 1: every pass is the single-sweep kernel, with 2 or 4 rows per wave, z chunks of 1, 3 and more than D
    planes or derived from the block target (one block, the default 2048, a million)."""
    acc = 5
    m = _geometry_mask(W, H, D, [])
    ref = oracle_fields(oracle_mod, W, H, D, fp64, "geometry", m, acc)
    for ry in ("2", "4"):
        for zc in ("0", "1", "3", str(D + 40)):
            for blocks in (None, "1", "1000000"):
                opts = {"sweep_fuse": "1", "sweep_ry": ry, "sweep_zc": zc}
                if blocks:
                    opts["sweep_blocks"] = blocks
                got, _ = run_sim(F, W, H, D, fp64, m, acc, opts)
                assert_same(F, got, ref, "%s %s" % (_grid_id(W, H, D, fp64), opts))


PROJECT_GRIDS = [(37, 13, 5), (256, 9, 13), (300, 7, 16), (64, 8, 3), (512, 6, 7)]


@pytest.mark.parametrize("fp64", [False, True], ids=["fp32", "fp64"])
@pytest.mark.parametrize("W,H,D", PROJECT_GRIDS)
def test_project_kernels_march_and_cell(F, oracle_mod, W, H, D, fp64):
    """The z-marching and the per-cell divergence / gradient kernels, D < 8 and D not a multiple of 8 included."""
    acc = 6
    m = _geometry_mask(W, H, D, [])
    ref = oracle_fields(oracle_mod, W, H, D, fp64, "geometry", m, acc)
    for pk in ("march", "cell"):
        got, _ = run_sim(F, W, H, D, fp64, m, acc, {"project_kernels": pk})
        assert_same(F, got, ref, "%s project_kernels=%s" % (_grid_id(W, H, D, fp64), pk))


@pytest.mark.parametrize("W", [200, 300])
def test_pair_shape_16_waves(F, oracle_mod, W):
    """pair_shape = 3, the 16-wave pair build (Build<2, 1, 16, 2> / <2, 2, 8, 2>), with each of its chunk counts."""
    H, D, acc = 40, 48, 8
    plans = plan_list(W, False)
    m = _masks(W, H, D, plans)["geometry"]
    ref = oracle_fields(oracle_mod, W, H, D, False, "geometry", m, acc)
    for pid in (0, 8, 16):
        got, rep = run_sim(F, W, H, D, False, m, acc, {"pair_shape": "3", "launch_plans": "%d,-1" % pid})
        assert rep == (pid, -1, 0), rep
        assert_same(F, got, ref, "%dx%dx%d pair_shape=3 launch_plans=%d,-1" % (W, H, D, pid))


# ---- part 6: replay validation (host side) -------------------------------------------------------------------------------------
@pytest.mark.parametrize("W,fp64,value", [
    (512, False, "0,2"),        # three-sweep shape 2: rows of 512 cells have two
    (256, False, "0,24"),       # three-sweep alt 3
    (256, False, "24,-1"),      # pair alt 3
    (1024, False, "88,-1"),     # fused alt 3
    (300, False, "64,-1"),      # a fused id on fp32 rows <= 512
    (600, False, "1,-1"),       # pair shape 1 on rows > 512
    (200, True, "65,-1"),       # fused shape 1 on fp64 rows <= 256
    (200, True, "40,-1"),       # an id between the pair and the fused range
])
def test_plans_the_grid_does_not_have_are_refused(F, W, fp64, value):
    sim = F.Simulation(W, 8, 8, 1, acc=4, quiet=1, precision="fp64" if fp64 else "fp32")
    sim.set_option("launch_plans", value)
    with pytest.raises(F.FluidsimError) as e:
        sim.run_one()
    assert "launch_plans" in str(e.value), str(e.value)
    sim.close()


def test_malformed_launch_plans_are_refused(F):
    sim = F.Simulation(64, 8, 8, 1, quiet=1)
    for v in ("3", "a,b", "128,0", "0,32", "-2,0", "0,-2", ""):
        with pytest.raises(F.FluidsimError):
            sim.set_option("launch_plans", v)
    for v in ("-1,-1", "0,-1", "127,31"):
        sim.set_option("launch_plans", v)
    sim.close()


@pytest.mark.parametrize("W,fp64", [(200, True), (600, False)])
def test_three_sweep_id_ignored_where_the_kernel_is_missing(F, oracle_mod, W, fp64):
    H, D, acc = 9, 12, 7
    m = _geometry_mask(W, H, D, [])
    ref = oracle_fields(oracle_mod, W, H, D, fp64, "geometry", m, acc)
    got, rep = run_sim(F, W, H, D, fp64, m, acc, {"launch_plans": "0,5"})
    assert rep == (0, -1, 0), rep
    assert_same(F, got, ref, "%s launch_plans=0,5" % _grid_id(W, H, D, fp64))


@pytest.mark.parametrize("W", [256, 1024])
def test_minus_one_minus_one_times_as_usual(F, oracle_mod, W):
    """"-1,-1" is no replay: the plans are timed again (also after a replay on the same handle) and the chosen ids are ids the
    grid has."""
    H, D, acc = 40 if W == 256 else 20, 48, 8
    plans = plan_list(W, False)
    m = _geometry_mask(W, H, D, plans)
    ref = oracle_fields(oracle_mod, W, H, D, False, "geometry", m, acc)
    two_ids = {p[2] for p in plans if p[0] != "three"}
    three_ids = {p[3] for p in plans if p[0] == "three"} | {-1}
    got, rep = run_sim(F, W, H, D, False, m, acc, {"launch_plans": "-1,-1"})
    assert rep[0] in two_ids and rep[1] in three_ids and rep[2] == (rep[0] >= FUSED2), rep
    assert_same(F, got, ref, "W=%d launch_plans=-1,-1" % W)
    sim = F.Simulation(W, H, D, 1, acc=acc, quiet=1)
    sim.set_option("launch_plans", "%d,-1" % max(two_ids))
    sim.set_mask(m)
    sim.run_one()
    assert sim._geti("pair_shape") == max(two_ids)
    sim.set_option("launch_plans", "-1,-1")
    sim.run_one()
    assert sim._geti("pair_shape") in two_ids and sim._geti("triple_plan") in three_ids
    out = [sim.get(f) for f in range(11)]
    sim.close()
    assert_same(F, out, ref, "W=%d replay, then -1,-1 on one handle" % W)
