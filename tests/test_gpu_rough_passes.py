"""The step's own kernels on rough and special-valued inputs, without a tolerance: every comparison is rough_cases.same(),
bit equality after every NaN is mapped to one canonical NaN (a NaN's sign and payload depend on operand order and are no part
of the contract).  The inputs are the seeded recipe of tests/rough_cases.py: five value classes per cell (plain, subnormal,
+-0, values at the normal / subnormal border, values whose sums overflow), a non-finite variant with +Inf, -Inf and NaN at
named cells, rough back-trace velocities of every clamp class, and obstacle arrays with 15 % / 60 % scattered solids, solids on
all six faces, clean planes, and "odd" values that are neither 0 nor 1 (0.5, 2, -0, -1, NaN, nextafter(1, 2); ghosts included).

Part a: the GPU under solver = gs_lex against what the compiled reference computed from the same inputs
(tests/golden/g8_rough_digests.json, arrays where stored), with no oracle in between.

Part b: the kernel forms against the oracle (JACOBI, RBSOR, MG; fp32 and fp64) on the same recipe, the non-finite variant
with three more cells in mid-domain (rows 16 | 17, planes 5 | 6, beside the seam of a row's first two waves).  Where the
library has a counter for a form, the case asserts through it that the form ran (triple_plan, two_sweep_fused, pair_shape,
reversed_passes, zero_start_projections, project_advect_steps): a form that was silently replaced is a failure, not a pass.
There is no counter for which body of the three-sweep kernel a workgroup runs, nor for the advection (cell / celltab / tile /
row) and projection (march / cell) kernel families.  The bodies are pinned by geometry instead: the case forces the launch plan
(launch_plans = "0,0": shape 0, so the band height is known), and two_body_groups() / group_state() restate from H, D, BY and the
obstacle array which bands and which groups of three plane iterations run which body (sweep_fused.hip, the end of
jacobi_fused_kernel; chunk_plan.h, mask_free_plan), and the case asserts what it needs of that.  The advection and projection
families are only requested by option; that the option selects the family is the subject of test_gpu_advect_rough.py and
test_gpu_launch_plans.py.

Coverage: form x obstacle kind -> test id.  Every special field holds all five finite classes
(test_oracle_rough_cpu.py counts them), so "finite" stands for those five and "nonfinite" for those five plus Inf / NaN.
A row runs both variants unless it says otherwise; "odd" obstacles run on 37x21x9, 256x6x5 and 256x40x12.

  form (how it is forced; what proves it ran)                     obstacles         test id
  gs_lex against the recorded reference                           s15 s60 faces odd test_gs_lex_against_recorded_reference[<grid>-<obs>-<variant>]
  single-sweep kernel (sweep_fuse=1; pair_shape = triple_plan     s60 odd           test_solves[single-37x21x9-fp32|fp64], [single-260x6x5-*],
    = -1: no other kernel was planned)                                                [single-256x6x5-fp32]
  pair kernel (sweep_fuse=2 two_sweep_kernel=pair;                faces odd         test_solves[pair-37x21x9-*], [pair-260x6x5-fp32],
    two_sweep_fused = 0, pair_shape >= 0, triple_plan = -1)                           [pair-256x6x5-fp32], [pair-1000x3x7-fp32]
  fused two-sweep kernel (two_sweep_kernel=fused;                 s15 odd           test_solves[fused2-1000x3x7-fp32], [fused2-260x6x5-fp64],
    two_sweep_fused = 1)                                                              [fused2-37x21x9-fp64]
  three-sweep kernel, general body, general build                 faces odd         test_solves[three-37x21x9-fp32], [three-260x6x5-fp32]
    (sweep_fuse=4; triple_plan >= 0), ragged rows, two z chunks
  three-sweep kernel, general body of the aligned builds          s15 clean none    test_solves[three_wf0|three_wf1|three_mf-256x6x5|512x4x5-fp32]
    (one band at both y walls, no wall-free group: stated)          odd
  three-sweep, wall-free body (wall_free=1 mask_free=0;           s15 odd           test_solves[wall_free-256x40x12-fp32], [wall_free-512x30x12-fp32]
    triple_plan = 0; interior bands with g1 > g0: stated)
  three-sweep, mask-free body (mask_free=1; empty tunnel: every   none deep s15     test_solves[mask_free-256x40x12-fp32], [mask_free-512x30x12-fp32]
    wall-free group clean; deep: the first clean, the last not;     odd
    s15: none clean, the wall-free body of that build)
  three-sweep, wall_free=0 on the same grids (one body)           s15               test_solves[one_body-256x40x12-fp32], [one_body-512x30x12-fp32]
  three-sweep, downward march (z_alternate=1; reversed_passes     s15 clean / deep  test_solves[three_zalt-512x4x5-fp32] (general body),
    = one per solve of >= 6 sweeps)                                 none              [zalt-512x30x12-fp32] (wall-free and mask-free groups)
  rbsor omega 1.5 on 32x16x8 (pair_shape >= 0; non-finite         s15 odd           test_rbsor_and_multigrid[rbsor-fp32|fp64]
    cells in the high corner only)
  multigrid on 32x16x8 (mg_levels = 2), finite variant only       s15 odd           test_rbsor_and_multigrid[mg-fp32]
  projection, z-march / per-cell kernels (by option)              s60 faces odd     test_projection[march|cell-<grid>-<prec>]
  projection, zero start 0 / 1 (zero_start_projections            s15 clean odd /   test_projection_zero_start[256x6x5-mask_free0|1] (general body),
    = 0 / one per projection with acc >= 3)                         none deep s15     [256x40x12-mask_free0|1] (wall-free / mask-free groups)
  advection cell / celltab / tile / row (by option), b = 0..3,    s15 s60 odd       test_advection[<kernels>-<grid>-<prec>]
    and b = 1..3 with a special-valued source (finite variant)
  whole steps, gradient inside the advection or apart             s15 faces odd     test_whole_steps[<grid>-<prec>]  (finite variant only: a step
    (project_advect_steps = 4 / 0), from rough and from                               must not trace with NaN velocities)
    special-valued velocities
  stand-alone setBounds, b = 0..3                                 s60 faces odd     test_set_bounds[<grid>-<prec>]

Grids: 37x21x9 (W % 4 = 1, padded pitch, a partial last band), 260x6x5 (a second x-wave with four live cells), 256x6x5
(lane-aligned: the aligned three-sweep builds and the zero start, general body only), 512x4x5 (two waves: the downward
march, general body only), 1000x3x7 (the wide rows' two-sweep kernels), 5x3x2.  256x40x12 and 512x30x12 are the smallest
aligned grids on which shape 0 (20- / 12-row bands) has a band clear of both y walls and, in one z chunk, two groups of three
plane iterations clear of both z walls (iterations 4 .. 9): the wall-free and mask-free bodies need them.  The three-sweep
kernel has no fp64 build, the fused two-sweep kernel no fp32 build for rows up to 512 cells and no fp64 build beyond: those
forms run where they exist.  The solves run 7 and 8 sweeps (passes [3, 3, 1] and [3, 3, 2], [2, 2, 2, 1] and [2, 2, 2, 2]) with
the pressure equation's coefficients and a diffusion's, and the four diffusions (b = 0..3: the in-kernel setBounds of every
sign).
"""
import json
import os

import numpy as np
import pytest

import rough_cases as R
from conftest import GOLDEN
from launch_plan_model import model_chunk_len, nbands, three_shapes

pytestmark = pytest.mark.gpu

ODD_GRIDS = [(37, 21, 9), (256, 6, 5), (256, 40, 12)]
ACCS = (7, 8)


def _diff(shape):
    """a = dt diff W H D is about 0.5 on every grid: the neighbour sum carries weight in a diffusion, and a times a sum of huge
    values overflows now and then, not everywhere"""
    return 10.0 / (shape[0] * shape[1] * shape[2])

# Part b, non-finite variant: the conditions of the recorded fixtures hold for the oracle's outputs too (NaN share of the
# interior at most 10 %, at least 5 non-finite cells): the mid-domain cells form one cluster, and 8 Jacobi sweeps carry a
# value 8 cells.


@pytest.fixture(scope="module")
def F():
    import fluid_simulation_amd as F
    assert list(F.FIELD_NAMES) == R.NAMES
    return F


def _gid(shape):
    return "%dx%dx%d" % tuple(shape)


def _dtype(prec):
    return np.float64 if prec == "fp64" else np.float32


def _obs_kinds(shape, binary):
    return tuple(binary) + (("odd",) if tuple(shape) in ODD_GRIDS else ())


_INPUTS, _WANT = {}, {}


def inputs(shape, obs, variant, prec, mid=True):
    key = (tuple(shape), obs, variant, prec, mid)
    if key not in _INPUTS:
        _INPUTS[key] = R.case_inputs(*shape, obs, variant, _dtype(prec), mid=mid)
    return _INPUTS[key]


def select(inp, variant, prefixes, accs=ACCS):
    return [ps for ps in R.pass_list(inp, variant, acc=accs[0], lin_accs=accs) if ps["name"].startswith(tuple(prefixes))]


def oracle_outputs(O, shape, obs, variant, prec, prefixes, solver="jacobi", mid=True, accs=ACCS, **kw):
    """{output name: array} of the selected passes on the oracle, computed once and shared (never modified)"""
    key = (tuple(shape), obs, variant, prec, tuple(prefixes), solver, mid, accs, tuple(sorted(kw.items())))
    if key not in _WANT:
        inp = inputs(shape, obs, variant, prec, mid)
        sol = {"jacobi": O.JACOBI, "rbsor": O.RBSOR, "mg": O.MG}[solver]
        handles, out = {}, {}
        for ps in select(inp, variant, prefixes, accs):
            if ps["acc"] not in handles:
                handles[ps["acc"]] = O.Oracle(*shape, solver=sol, fp64=prec == "fp64", threads=4, iter=1, acc=ps["acc"], diff=_diff(shape), **kw)
            out.update(R.run_pass(handles[ps["acc"]], inp, ps, _dtype(prec)))
        for h in handles.values():
            h.close()
        for k, a in out.items():
            a.setflags(write=False)
            if variant == "nonfinite" and k not in R.ALL_ZERO:
                assert R.nonfinite_cells(a) >= R.NONFINITE_MIN, (key, k)
                assert R.nan_share(a) <= R.NAN_SHARE_MAX, (key, k, R.nan_share(a))
            if variant == "finite" and k.startswith(("step", "sstep")):
                assert np.isfinite(a).all(), (key, k)
        _WANT[key] = out
    return _WANT[key]


def gpu_outputs(sim, shape, obs, variant, prec, prefixes, mid=True, accs=ACCS):
    inp = inputs(shape, obs, variant, prec, mid)
    out = {}
    for ps in select(inp, variant, prefixes, accs):
        sim.acc = ps["acc"]
        out.update(R.run_pass(sim, inp, ps, _dtype(prec)))
    return out


def assert_same(got, want, what):
    assert sorted(got) == sorted(want) and got, what
    for k in want:
        print("%s %s: NaN share %.4f, non-finite cells %d" % (what, k, R.nan_share(want[k]), R.nonfinite_cells(want[k])))
        assert R.same(got[k], want[k]), "%s %s: first difference (cell, GPU, expected, cells) %s" % (
            what, k, R.first_difference(got[k], want[k]))


def simulation(F, shape, prec, solver="jacobi", **opts):
    return F.Simulation(*shape, 1, acc=ACCS[0], diff=_diff(shape), quiet=1, precision=prec, solver=solver, **opts)


# ---- part a: gs_lex on the GPU against the recorded reference ---------------------------------------------------------------------
with open(os.path.join(GOLDEN, "g8_rough_digests.json")) as _f:
    _G8 = {c["id"]: c for c in json.load(_f)["cases"]}
_A_CASES = [c for c in R.recorded_cases() if c[:3] in R.REF_GPU_GRIDS]


@pytest.mark.parametrize("W,H,D,obs,variant", _A_CASES, ids=[R.case_id(*c) for c in _A_CASES])
def test_gs_lex_against_recorded_reference(F, W, H, D, obs, variant):
    """Every recorded pass and the finite variants' two steps, from the recorded inputs, under solver = gs_lex: the digests
    the reference left, and the arrays where they are stored."""
    rec = _G8[R.case_id(W, H, D, obs, variant)]
    inp = R.case_inputs(W, H, D, obs, variant)
    for k, a in inp.items():
        assert R.digest(a) == rec["inputs"][k], "recipe changed: input %s" % k
    stored = np.load(os.path.join(GOLDEN, "g8_rough_37x21x9.npz"), allow_pickle=False)
    sim = F.Simulation(W, H, D, 1, acc=R.ACC, quiet=1, solver="gs_lex")
    seen = 0
    for ps in R.pass_list(inp, variant):
        sim.acc = ps["acc"]
        for k, a in R.run_pass(sim, inp, ps).items():
            key = rec["id"] + "__" + k
            if key in stored.files:
                assert R.same(a, stored[key]), "%s: first difference (cell, GPU, reference, cells) %s" % (key, R.first_difference(a, stored[key]))
            assert R.digest(a) == rec["outputs"][k], "%s %s differs from the reference" % (rec["id"], k)
            seen += 1
    sim.close()
    assert seen == len(rec["outputs"])


# ---- part b: the solves ----------------------------------------------------------------------------------------------------------
def _no_fused_kernel(sim, solves):
    assert (sim._geti("pair_shape"), sim._geti("triple_plan")) == (-1, -1)


def _pair(sim, solves):
    assert sim._geti("two_sweep_fused") == 0 and sim._geti("pair_shape") >= 0 and sim._geti("triple_plan") == -1


def _fused2(sim, solves):
    assert sim._geti("two_sweep_fused") == 1 and sim._geti("triple_plan") == -1


def _three(sim, solves):
    assert sim._geti("triple_plan") >= 0 and sim._geti("reversed_passes") == 0


def _three_down(sim, solves):
    # [3, 3, 1] and [3, 3, 2]: the second pass of every solve marches downward
    assert sim._geti("triple_plan") >= 0 and sim._geti("reversed_passes") == solves


# ---- which body of the aligned three-sweep builds runs where (one z chunk over planes 1 .. D, whole domain) ----------------------
def two_body_groups(H, D, BY):
    """-> ([first row s of every band clear of both y walls], g0, g1): sweep_fused.hip runs groups [0, g0) and [g1, ngroups)
    plus the tail in the general body and [g0, g1) in the wall-free one (mask-free where clean), in those bands only."""
    NL, OV, lo1 = 3, 2, 1
    ngroups = (D + OV - lo1 + 1) // 3
    g0 = min(ngroups, (NL - lo1) // 3 + 1)
    g1 = max(g0, min(ngroups, (D - lo1) // 3))
    starts = [k * (BY - 2 * OV) - (OV - 1) for k in range(nbands(H, BY, NL))]
    return [s for s in starts if not (s <= 0 or s + BY - 1 >= H + 1)], g0, g1


def group_state(obs, s, BY, k):
    """Group k (plane iterations Z = 1 + 3 k .. Z + 2) of the band at row s is clean when rows s .. s + BY - 1 hold no kill byte
    on planes Z - 2 .. Z + 3 (chunk_plan.h).  -> "clean" if no solid lies in or next to those rows and planes (so none can
    hold a solid or near-solid cell), "masked" if a solid lies in them, else "unknown"."""
    solid = np.asarray(obs) == 1
    D, H = solid.shape[0] - 2, solid.shape[1] - 2
    Z = 1 + 3 * k
    if solid[max(Z - 2, 0):min(Z + 3, D + 1) + 1, max(s, 0):min(s + BY - 1, H + 1) + 1].any():
        return "masked"
    if not solid[max(Z - 3, 0):min(Z + 4, D + 1) + 1, max(s - 1, 0):min(s + BY, H + 1) + 1].any():
        return "clean"
    return "unknown"


def body_claims(shape, obs_kind, obs, want):
    """What a case says about the bodies, asserted from the restated geometry.  want: "general" (no wall-free group anywhere),
    "wall_free" (interior bands with wall-free groups), "mask_free" (and what the obstacle kind promises about clean groups)."""
    W, H, D = shape
    BY = three_shapes(W, False)[0][1]
    assert model_chunk_len("three", H, D, 3, BY, 0) == D           # one z chunk: the groups below are the launch's
    interior, g0, g1 = two_body_groups(H, D, BY)
    if want == "general":
        assert not interior or g1 == g0, (shape, interior, g0, g1)
        return
    assert interior and g1 - g0 >= 2, (shape, interior, g0, g1)
    if want == "mask_free":
        states = [[group_state(obs, s, BY, k) for k in range(g0, g1)] for s in interior]
        if obs_kind == "none":
            assert all(st == "clean" for row in states for st in row), states
        elif obs_kind == "deep":                                    # mask-free first, then the wall-free body with kill bytes
            assert all(row[0] == "clean" and row[-1] == "masked" for row in states), states
        elif obs_kind == "s15":
            assert all(st == "masked" for row in states for st in row), states
    for (z, y, x) in R.mid_cells(W, H, D):                          # the mid-domain non-finite cells sit in a wall-free group
        assert any(s <= y <= s + BY - 1 for s in interior) and 1 + 3 * g0 <= z <= 3 * g1, (shape, z, y, x)


def _three0(sim, solves):
    assert sim._geti("triple_plan") == 0 and sim._geti("reversed_passes") == 0


def _three0_down(sim, solves):
    assert sim._geti("triple_plan") == 0 and sim._geti("reversed_passes") == solves


G37, G260, G256, G512, G1000 = (37, 21, 9), (260, 6, 5), (256, 6, 5), (512, 4, 5), (1000, 3, 7)
G256B, G512B = (256, 40, 12), (512, 30, 12)
THREE = {"sweep_fuse": "4", "pair_zc": str(R.ZC)}
BODIES = {"sweep_fuse": "4", "launch_plans": "0,0"}        # shape 0 and the model's first chunk count: one chunk at D = 12
# form -> (options, z_alternate, binary obstacle kinds, counter check, [(grid, precision)], body claim)
SOLVE_FORMS = {
    "single": ({"sweep_fuse": "1", "sweep_zc": str(R.ZC)}, None, ("s60",), _no_fused_kernel,
               [(G37, "fp32"), (G37, "fp64"), (G260, "fp32"), (G260, "fp64"), (G256, "fp32")], None),
    "pair": ({"sweep_fuse": "2", "two_sweep_kernel": "pair", "pair_zc": str(R.ZC)}, None, ("faces",), _pair,
             [(G37, "fp32"), (G37, "fp64"), (G260, "fp32"), (G256, "fp32"), (G1000, "fp32")], None),
    "fused2": ({"sweep_fuse": "2", "two_sweep_kernel": "fused", "pair_zc": str(R.ZC)}, None, ("s15",), _fused2,
               [(G1000, "fp32"), (G260, "fp64"), (G37, "fp64")], None),
    "three": (THREE, None, ("faces",), _three, [(G37, "fp32"), (G260, "fp32")], None),
    # the aligned builds on grids too small for a second body: the general body of each build
    "three_wf0": (dict(THREE, wall_free="0"), None, ("s15",), _three, [(G256, "fp32"), (G512, "fp32")], "general"),
    "three_wf1": (dict(THREE, wall_free="1", mask_free="0"), None, ("s15",), _three, [(G256, "fp32"), (G512, "fp32")], "general"),
    "three_mf": (dict(THREE, wall_free="1", mask_free="1"), None, ("clean", "none"), _three, [(G256, "fp32"), (G512, "fp32")], "general"),
    "three_zalt": (dict(THREE, mask_free="1"), 1, ("s15", "clean"), _three_down, [(G512, "fp32")], "general"),
    # the wall-free and mask-free bodies
    "one_body": (dict(BODIES, wall_free="0"), None, ("s15",), _three0, [(G256B, "fp32"), (G512B, "fp32")], "wall_free"),
    "wall_free": (dict(BODIES, wall_free="1", mask_free="0"), None, ("s15",), _three0, [(G256B, "fp32"), (G512B, "fp32")], "wall_free"),
    "mask_free": (dict(BODIES, wall_free="1", mask_free="1"), None, ("none", "deep", "s15"), _three0, [(G256B, "fp32"), (G512B, "fp32")],
                  "mask_free"),
    "zalt": (dict(BODIES, wall_free="1", mask_free="1"), 1, ("deep", "none"), _three0_down, [(G512B, "fp32")], "mask_free"),
}
_SOLVE_CASES = [pytest.param(form, g, p, id="%s-%s-%s" % (form, _gid(g), p)) for form, v in SOLVE_FORMS.items() for g, p in v[4]]
SOLVE_PASSES = ("lin_", "diffuse_")


@pytest.mark.parametrize("form,shape,prec", _SOLVE_CASES)
def test_solves(F, oracle_mod, form, shape, prec):
    """linear_solver with the pressure and a diffusion's coefficients at 7 and 8 sweeps, and diffuse for b = 0..3, under one
    forced kernel form, against the Jacobi oracle."""
    opts, zalt, binary, check, _, claim = SOLVE_FORMS[form]
    for obs in _obs_kinds(shape, binary):
        if claim:
            body_claims(shape, obs, inputs(shape, obs, "finite", prec)["obs"], claim)
        for variant in R.VARIANTS:
            want = oracle_outputs(oracle_mod, shape, obs, variant, prec, SOLVE_PASSES)
            # the expected fields are no fixed point of the inputs: one sweep more is another field
            assert not R.same(want["lin_a1_acc7"], want["lin_a1_acc8"]) and not R.same(want["lin_a03_acc7"], want["lin_a03_acc8"])
            sim = simulation(F, shape, prec, **opts)
            if zalt is not None:
                sim.z_alternate = zalt
            got = gpu_outputs(sim, shape, obs, variant, prec, SOLVE_PASSES)
            check(sim, len(want))
            sim.close()
            assert_same(got, want, "%s %s %s %s %s" % (form, _gid(shape), prec, obs, variant))


@pytest.mark.parametrize("solver,prec", [("rbsor", "fp32"), ("rbsor", "fp64"), ("mg", "fp32")])
def test_rbsor_and_multigrid(F, oracle_mod, solver, prec):
    """32x16x8: red-black SOR (omega 1.5) on both coefficient sets, and the multigrid pressure solve (two V-cycles), each
    against its own oracle; both run the pair kernel's plan.  A red-black iteration carries a value two cells, so the
    non-finite variant keeps to the high-corner cells here and runs 3 and 4 iterations (as far as 6 and 8 Jacobi sweeps reach;
    the finite variant runs 7 and 8); a V-cycle carries a NaN to every cell (the 30 iterations on the
    coarsest level cover it, the prolongation brings it back), so multigrid runs the finite variant only."""
    shape = (32, 16, 8)
    kw = {"omega": 1.5} if solver == "rbsor" else {"mg": (2, 1, 1, 30)}
    opts = {"sor_omega": 1.5} if solver == "rbsor" else {"mg_cycles": 2, "mg_pre": 1, "mg_post": 1, "mg_coarse_iters": 30}
    prefixes = ("lin_",) if solver == "rbsor" else ("lin_a1_", "project")
    for obs in ("s15", "odd"):
        for variant in R.VARIANTS[:2 if solver == "rbsor" else 1]:
            accs = ACCS if variant == "finite" else (3, 4)
            want = oracle_outputs(oracle_mod, shape, obs, variant, prec, prefixes, solver=solver, mid=False, accs=accs, **kw)
            sim = simulation(F, shape, prec, solver=solver, **opts)
            got = gpu_outputs(sim, shape, obs, variant, prec, prefixes, mid=False, accs=accs)
            assert sim._geti("pair_shape") >= 0
            if solver == "mg":
                assert sim._geti("mg_levels") == 2
            sim.close()
            assert_same(got, want, "%s %s %s %s" % (solver, prec, obs, variant))


# ---- part b: projection -----------------------------------------------------------------------------------------------------------
_PROJECT_CASES = [(k, g, p) for k in ("march", "cell") for g, p in
                  [(G37, "fp32"), (G37, "fp64"), (G260, "fp32"), (G256, "fp32"), (G256, "fp64"), (R.TINY, "fp32")]]


@pytest.mark.parametrize("kernels,shape,prec", _PROJECT_CASES, ids=["%s-%s-%s" % (k, _gid(g), p) for k, g, p in _PROJECT_CASES])
def test_projection(F, oracle_mod, kernels, shape, prec):
    """project with 7 sweeps and with none (divergence and gradient alone) under the z-marching and the per-cell kernels:
    special velocities, junk in p."""
    for obs in _obs_kinds(shape, ("s60", "faces")):
        for variant in R.VARIANTS[:1 if shape == R.TINY else 2]:
            want = oracle_outputs(oracle_mod, shape, obs, variant, prec, ("project",))
            sim = simulation(F, shape, prec, project_kernels=kernels)
            got = gpu_outputs(sim, shape, obs, variant, prec, ("project",))
            sim.close()
            assert_same(got, want, "project_kernels=%s %s %s %s %s" % (kernels, _gid(shape), prec, obs, variant))


@pytest.mark.parametrize("mask_free", ["0", "1"], ids=["mask_free0", "mask_free1"])
@pytest.mark.parametrize("shape", [G256, G256B], ids=_gid)
def test_projection_zero_start(F, oracle_mod, shape, mask_free):
    """The pressure solve's first pass takes level 0 as constants (zero_start = 1) or reads the zeroed p; the counter says
    which.  The launch plans are chosen in a first projection: the zero start needs them chosen.  On 256x6x5 only the general
    body of the zero-start builds runs; on 256x40x12 the wall-free body and, with mask_free = 1, the mask-free one."""
    prec, big = "fp32", shape == G256B
    opts = dict(BODIES) if big else {"sweep_fuse": "4"}
    for obs in (("none", "deep", "s15", "odd") if big else ("s15", "clean", "odd")):
        body_claims(shape, obs, inputs(shape, obs, "finite", prec)["obs"], ("mask_free" if mask_free == "1" else "wall_free") if big else "general")
        for variant in R.VARIANTS:
            want = oracle_outputs(oracle_mod, shape, obs, variant, prec, ("project",))
            for zs in ("0", "1"):
                sim = simulation(F, shape, prec, zero_start=zs, mask_free=mask_free, **opts)
                sim.project()
                assert sim._geti("zero_start_projections") == 0 and sim._geti("triple_plan") >= 0
                got = gpu_outputs(sim, shape, obs, variant, prec, ("project",))
                # "project" runs 7 sweeps (acc >= 3: the zero start where it is on), "project0" none (never)
                assert sim._geti("zero_start_projections") == (1 if zs == "1" else 0)
                sim.close()
                assert_same(got, want, "zero_start=%s mask_free=%s %s %s %s" % (zs, mask_free, _gid(shape), obs, variant))


# ---- part b: advection ------------------------------------------------------------------------------------------------------------
_ADVECT_CASES = [(k, g, p) for k in ("cell", "celltab", "tile", "row") for g, p in
                 [(G37, "fp32"), (G37, "fp64"), (G260, "fp32"), (G256, "fp32"), (G256, "fp64"), (R.TINY, "fp32")]]


@pytest.mark.parametrize("kernels,shape,prec", _ADVECT_CASES, ids=["%s-%s-%s" % (k, _gid(g), p) for k, g, p in _ADVECT_CASES])
def test_advection(F, oracle_mod, kernels, shape, prec):
    """advect for b = 0..3 with rough velocities: a special-valued (and, in the non-finite variant, Inf / NaN carrying) scalar for
    b = 0; for b = 1..3 the rough velocities themselves, and special-valued ones capped at 1e30 (finite variant only: see
    rough_cases)."""
    for obs in _obs_kinds(shape, ("s15", "s60")):
        for variant in R.VARIANTS[:1 if shape == R.TINY else 2]:
            want = oracle_outputs(oracle_mod, shape, obs, variant, prec, ("advect_",))
            assert len(want) == (7 if variant == "finite" else 1)
            sim = simulation(F, shape, prec, advect_kernels=kernels)
            got = gpu_outputs(sim, shape, obs, variant, prec, ("advect_",))
            sim.close()
            assert_same(got, want, "advect_kernels=%s %s %s %s %s" % (kernels, _gid(shape), prec, obs, variant))


_STEP_CASES = [(G37, "fp32"), (G37, "fp64"), (G256, "fp32"), (G512, "fp32")]


@pytest.mark.parametrize("shape,prec", _STEP_CASES, ids=["%s-%s" % (_gid(g), p) for g, p in _STEP_CASES])
def test_whole_steps(F, oracle_mod, shape, prec):
    """Two steps from rough velocities and two from special-valued ones (capped at the inlet speed), each with a special-valued
    density, with the first projection's gradient inside the velocity advection and apart: all fields after each step."""
    for obs in _obs_kinds(shape, ("s15", "faces")):
        want = oracle_outputs(oracle_mod, shape, obs, "finite", prec, ("step", "sstep"))
        assert len(want) == 40
        for fpa in ("0", "1"):
            sim = simulation(F, shape, prec, advect_kernels="cell", fuse_project_advect=fpa, sweep_fuse="4")
            got = gpu_outputs(sim, shape, obs, "finite", prec, ("step", "sstep"))
            assert sim._geti("project_advect_steps") == (4 if fpa == "1" else 0)
            sim.close()
            assert_same(got, want, "fuse_project_advect=%s %s %s %s" % (fpa, _gid(shape), prec, obs))


# ---- part b: setBounds ------------------------------------------------------------------------------------------------------------
_BOUNDS_CASES = [(g, p) for g in R.GRIDS for p in ("fp32", "fp64")]


@pytest.mark.parametrize("shape,prec", _BOUNDS_CASES, ids=["%s-%s" % (_gid(g), p) for g, p in _BOUNDS_CASES])
def test_set_bounds(F, oracle_mod, shape, prec):
    for obs in _obs_kinds(shape, ("s60", "faces")):
        for variant in R.VARIANTS[:1 if tuple(shape) == R.TINY else 2]:
            want = oracle_outputs(oracle_mod, shape, obs, variant, prec, ("set_bounds_",))
            sim = simulation(F, shape, prec)
            got = gpu_outputs(sim, shape, obs, variant, prec, ("set_bounds_",))
            sim.close()
            assert_same(got, want, "set_bounds %s %s %s %s" % (_gid(shape), prec, obs, variant))
