"""Rough and special-valued inputs for the step's passes, from a seed (numpy only).

One recipe serves three users: oracle/make_golden.py g8 (records what the compiled reference computes from these inputs),
tests/test_oracle_rough_cpu.py (holds oracle/cpu_ref.c to that) and tests/test_gpu_rough_passes.py (holds the HIP kernels
to the reference and to the oracle).  Nothing here computes an expected result.

Value classes of special(), per cell with equal odds:

  plain   standard normal
  sub     an integer in -50 .. 50 times finfo.smallest_subnormal
  zero    +0 or -0
  edge    normal x finfo.tiny: straddles the border between normal and subnormal numbers, so products underflow
  huge    normal x finfo.max / 10: a sum of six neighbours can overflow

The non-finite variant writes +Inf, -Inf and NaN into named cells: three in the high corner (corner_cells), and for the
Jacobi cases three more in mid-domain (mid_cells) on a band edge (rows 16 | 17 of the three-sweep kernel's 20-row bands) and
a z-chunk edge (planes 5 | 6 under pair_zc = sweep_zc = ZC where the grid is deeper than that).  Gauss-Seidel in the reference's order carries a NaN to every
cell after it, so only the high corner is used where the reference is involved.  The obstacle arrays are kept clear of solids
at the named cells and their six neighbours: a solid there would zero the very values the case is about.

The twelve edges of the padded box are 0 in every array (advect_model.rough_fields says why the build relies on that).

Back-trace velocities are advect_model.rough_fields: finite, every clamp class.  A NaN velocity makes the reference
convert NaN to int, which is undefined there, so it is no case: the velocity advections (b = 1..3) and the whole steps run
in the finite variant only, and in the non-finite variant only the advected scalar (b = 0) carries non-finite values.
Because the source of a velocity advection is also what carries its trace, the finite variant has a second set of velocity
advections ("advect_special_b1..3") and of whole steps ("sstep1", "sstep2") whose velocities are special fields capped at
CAP_ADVECT and CAP_STEP: subnormals, signed zeros and border values as they are, the huge class at the cap, so that
dt N v stays finite and the trace is defined in the reference.
"""
import hashlib

import numpy as np

from advect_model import box_edges, rough_fields

# (W, H, D): the smallest shapes that still reach each instantiation of the sweep kernels (compare launch_plan_model.GRIDS)
GRIDS = [
    (37, 21, 9),      # W % 4 = 1, padded pitch, partial last band
    (260, 6, 5),      # a second x-wave holding four live cells
    (256, 6, 5),      # lane-aligned rows: three-sweep kernel, zero start
    (512, 4, 5),      # two full waves per row: the downward march
    (1000, 3, 7),     # the two-sweep kernels of wide rows
    (5, 3, 2),        # tiny
]
TINY = (5, 3, 2)
REF_GPU_GRIDS = [(5, 3, 2), (37, 21, 9), (260, 6, 5)]      # the grids the GPU runs gs_lex on against the recorded reference
BINARY = ("s15", "s60", "faces")
OBS_KINDS = BINARY + ("odd",)
VARIANTS = ("finite", "nonfinite")
SEED = 20
ZC = 5                        # planes per z chunk the GPU cases ask for (pair_zc, sweep_zc)
ACC = 4                       # sweeps of the recorded diffuse / project / steps; linear_solver is recorded at LIN_ACCS
LIN_ACCS = (2, 4)
COEFFS = (("a1", 1.0, 6.0), ("a03", 0.3, 2.8))     # the pressure equation's coefficients, and a diffusion's
NAN_SHARE_MAX = 0.10          # non-finite variants: NaN share of the interior of every compared output
NONFINITE_MIN = 5             # ... and its non-finite cells, ghosts included
CAP_ADVECT = 1.0e30           # advect_special_b*: |source| of a velocity advection; dt N v <= 0.05 x 1000 x 1e30 is finite in fp32
CAP_STEP = 30.0               # sstep*: |v| at the start of a step with special velocities: the inlet speed
ALL_ZERO = ("project0_pressure",)      # a projection zeroes p and acc = 0 runs no sweep: nothing non-finite can be asked of it

DENS, VX, VY, VZ, OBS, P, DIV, VX0, VY0, VZ0, BUF = range(11)
NAMES = ["dens", "v_x", "v_y", "v_z", "obs", "pressure", "divergence", "v_x_prev", "v_y_prev", "v_z_prev", "buffer"]
ODD_VALUES = ("0", "0", "0", "0", "1", "1", "0.5", "2", "-0", "-1", "nan", "next")


# ---- helpers ---------------------------------------------------------------------------------------------------------------
def canon(a):
    """every NaN -> the one quiet NaN numpy writes for float('nan'): the reference's NaN sign and payload depend on its
    compiler's operand order and are no part of the contract"""
    a = np.array(a, copy=True)
    a[np.isnan(a)] = np.nan
    return a


def same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and canon(a).tobytes() == canon(b).tobytes()


def digest(a):
    return hashlib.sha256(np.ascontiguousarray(canon(a)).tobytes()).hexdigest()


def nan_share(a):
    """NaN share of the interior cells"""
    return float(np.isnan(a[1:-1, 1:-1, 1:-1]).mean())


def nonfinite_cells(a):
    return int(np.count_nonzero(~np.isfinite(a)))


def first_difference(a, b):
    """(z, y, x), got, want of the first cell where canon(a) and canon(b) differ, for messages"""
    u = np.uint32 if a.dtype == np.float32 else np.uint64
    d = np.argwhere(canon(a).view(u) != canon(b).view(u))
    if not len(d):
        return None
    i = tuple(int(v) for v in d[0])
    return i, float(a[i]), float(b[i]), len(d)


# ---- the named non-finite cells, (z, y, x) -> value ----------------------------------------------------------------------------
def corner_cells(W, H, D):
    """x >= W - 2, y >= H - 1, z >= D - 1"""
    return {(D, H, W): np.inf, (D, H, W - 1): -np.inf, (D, H - 1, W): np.nan}


def mid_cells(W, H, D):
    yb = min(16, H - 1)
    xs = min(256, W - 2)                                     # the seam between a row's first two waves where there is one; else
                                                             # beside the corner cells, so that the two clusters overlap
    zc = ZC if D > ZC else 3                                 # the last plane of the first z chunk where there are two
    # one cluster: what 8 Jacobi sweeps carry away from it stays within x = xs - 9 .. xs + 9
    return {(zc, yb, xs - 1): np.nan, (zc + 1, yb + 1, xs): np.inf, (zc, yb, xs + 1): -np.inf}


def named_cells(W, H, D, where):
    cells = {}
    if where in ("corner", "corner+mid"):
        cells.update(corner_cells(W, H, D))
    if where == "corner+mid":
        cells.update(mid_cells(W, H, D))
    for (z, y, x) in cells:
        assert 1 <= z <= D and 1 <= y <= H and 1 <= x <= W, (W, H, D, z, y, x)
    return cells


# ---- value fields ----------------------------------------------------------------------------------------------------------
def special(W, H, D, seed, dtype=np.float32, nonfinite=None):
    """A padded (D+2, H+2, W+2) array of the five value classes; nonfinite = None | "corner" | "corner+mid"."""
    fi = np.finfo(dtype)
    rng = np.random.default_rng(seed)
    shape = (D + 2, H + 2, W + 2)
    kind = rng.integers(0, 5, shape)
    plain = rng.standard_normal(shape)
    sub = rng.integers(-50, 51, shape).astype(np.float64)
    neg = rng.integers(0, 2, shape) == 1
    edge = rng.standard_normal(shape)
    huge = rng.standard_normal(shape)
    T = np.dtype(dtype).type
    a = plain.astype(dtype)
    a = np.where(kind == 1, (sub.astype(dtype) * T(fi.smallest_subnormal)).astype(dtype), a)
    a = np.where(kind == 2, np.where(neg, T(-0.0), T(0.0)), a)
    a = np.where(kind == 3, (edge.astype(dtype) * T(fi.tiny)).astype(dtype), a)
    a = np.where(kind == 4, (huge.astype(dtype) * (T(fi.max) / T(10))).astype(dtype), a)
    a = np.ascontiguousarray(a, dtype=dtype)
    a[box_edges(W, H, D)] = 0.0
    if nonfinite:
        for cell, v in named_cells(W, H, D, nonfinite).items():
            a[cell] = v
    return a


# ---- obstacle arrays -------------------------------------------------------------------------------------------------------
def _keep_clear(W, H, D):
    """bool: the named cells (corner and mid) and their six neighbours"""
    m = np.zeros((D + 2, H + 2, W + 2), dtype=bool)
    if (W, H, D) == TINY:
        return m
    for (z, y, x) in named_cells(W, H, D, "corner+mid"):
        m[z, y, x] = True
        for dz, dy, dx in ((1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1)):
            m[z + dz, y + dy, x + dx] = True
    return m


def obstacles(kind, W, H, D, seed=SEED, dtype=np.float32):
    """The padded obstacle array in `dtype`.
      s15 / s60   15 % / 60 % scattered interior solids (60 % encloses fluid cells: all six neighbours solid)
      faces       solids in columns 1 and W, rows 1 and H, planes 1 and D (a third of each face's cells) and 2 % elsewhere
      clean       a few solids in plane 1 only: every other plane is free of kill bytes (the mask-free body runs)
      deep        a few solids in planes D - 2 and D - 1, rows 16 and 17: the planes below D - 3 are free of kill bytes
      none        no solid
      odd         every cell of the padded array, ghosts included, drawn from ODD_VALUES: 0.5, 2, -1, NaN and
                  nextafter(1, 2) are neither `== 1` (solid) nor `== 0` (a fluid neighbour)"""
    rng = np.random.default_rng(seed + 500)
    shape = (D + 2, H + 2, W + 2)
    o = np.zeros(shape, dtype=dtype)
    inner = (slice(1, -1),) * 3
    if kind in ("s15", "s60"):
        o[inner] = rng.random((D, H, W)) < (0.15 if kind == "s15" else 0.60)
    elif kind == "faces":
        face = np.zeros((D, H, W), dtype=bool)
        face[0] = face[-1] = True
        face[:, 0] = face[:, -1] = True
        face[:, :, 0] = face[:, :, -1] = True
        r = rng.random((D, H, W))
        o[inner] = np.where(face, r < 1.0 / 3.0, r < 0.02)
    elif kind == "clean":
        o[1, 1:1 + max(1, H // 2), W // 3:W // 3 + 3] = 1.0
    elif kind == "deep":
        yb = min(16, H - 1)
        o[D - 2:D, yb:yb + 2, W // 3:W // 3 + 3] = 1.0
    elif kind == "odd":
        T = np.dtype(dtype).type
        table = np.array([0, 0, 0, 0, 1, 1, 0.5, 2, -0.0, -1, np.nan, np.nextafter(T(1), T(2))], dtype=dtype)
        assert len(table) == len(ODD_VALUES)
        o = np.ascontiguousarray(table[rng.integers(0, len(table), shape)])
    elif kind != "none":
        raise ValueError(kind)
    o[_keep_clear(W, H, D)] = 0.0
    return o


def enclosed_cells(o):
    """fluid interior cells whose six neighbours are all solid"""
    s = o == 1
    c = ~s[1:-1, 1:-1, 1:-1]
    return int(np.count_nonzero(c & s[1:-1, 1:-1, 2:] & s[1:-1, 1:-1, :-2] & s[1:-1, 2:, 1:-1] & s[1:-1, :-2, 1:-1] &
                                s[2:, 1:-1, 1:-1] & s[:-2, 1:-1, 1:-1]))


# ---- a case: its inputs and its passes -----------------------------------------------------------------------------------------
def case_id(W, H, D, obs_kind, variant):
    return "%dx%dx%d-%s-%s" % (W, H, D, obs_kind, variant)


def case_inputs(W, H, D, obs_kind, variant, dtype=np.float32, seed=SEED, mid=False):
    """name -> array: the rough velocities ux, uy, uz, four special fields A .. D and the obstacle array.  `mid`: the
    non-finite variant also writes the mid-domain cells (Jacobi cases)."""
    if variant == "nonfinite":
        assert (W, H, D) != TINY, "5x3x2 is left out of the non-finite variant: a NaN reaches most of its 30 cells"
    nf = None if variant == "finite" else ("corner+mid" if mid else "corner")
    ux, uy, uz, _ = rough_fields(W, H, D, seed, dtype)
    inp = {"ux": ux, "uy": uy, "uz": uz, "obs": obstacles(obs_kind, W, H, D, seed, dtype)}
    for k, name in enumerate("ABCD"):
        inp[name] = special(W, H, D, seed + 1 + k, dtype, nf)
    for name in ("ux", "uy", "uz"):
        assert np.isfinite(inp[name]).all()
    return inp


def pass_list(inp, variant, acc=ACC, lin_accs=LIN_ACCS, steps=2):
    """The passes of a case in the order they are recorded.  A pass is a dict: name, acc, fields (selector -> array; every
    other field but the obstacles is zero before the call), calls [(method, args)] and outs [(output name, selector)] read
    after the last call; keep = True runs on from the state the pass before it left."""
    A, B, C, Dd = inp["A"], inp["B"], inp["C"], inp["D"]
    rough = {VX: inp["ux"], VY: inp["uy"], VZ: inp["uz"]}
    out = []

    def add(name, a, fields, calls, outs, keep=False):
        out.append(dict(name=name, acc=a, fields=fields, calls=calls, outs=outs, keep=keep))

    for b in range(4):
        add("set_bounds_b%d" % b, acc, {VX: A}, [("set_bounds", (b, VX))], [("set_bounds_b%d" % b, VX)])
    pairs = ((0, DENS, BUF), (1, VX, VX0), (2, VY, VY0), (3, VZ, VZ0))
    for b, f, p in pairs:
        add("diffuse_b%d" % b, acc, {f: A, p: B}, [("diffuse", (b, f, p))], [("diffuse_b%d" % b, f)])
    for tag, a, c in COEFFS:
        for n in lin_accs:
            name = "lin_%s_acc%d" % (tag, n)
            add(name, n, {P: A, DIV: B}, [("linear_solver", (0, P, DIV, a, c))], [(name, P)])
    for b, f, p in pairs:
        if b and variant != "finite":
            continue                   # the source of a velocity advection carries its trace: finite only (module docstring)
        fields = dict(rough)
        fields[p] = A if b == 0 else rough[f]
        add("advect_b%d" % b, acc, fields, [("advect", (b, f, p))], [("advect_b%d" % b, f)])
    if variant == "finite":
        for b, f, p in pairs[1:]:
            fields = dict(rough)
            fields[p] = np.clip((B, C, Dd)[b - 1], -CAP_ADVECT, CAP_ADVECT)
            add("advect_special_b%d" % b, acc, fields, [("advect", (b, f, p))], [("advect_special_b%d" % b, f)])
    for tag, n in (("project", acc), ("project0", 0)):      # acc = 0: divergence and gradient alone, whatever the solver
        add(tag, n, {VX: A, VY: B, VZ: C, P: Dd}, [("project", ())], [(tag + "_" + NAMES[f], f) for f in (VX, VY, VZ, P, DIV)])
    if variant == "finite":
        for k in range(steps):
            fields = dict(rough)
            fields[DENS] = A
            add("step%d" % (k + 1), acc, fields, [("run_one", ())],
                [("step%d_%s" % (k + 1, NAMES[f]), f) for f in range(11) if f != OBS], keep=k > 0)
        for k in range(steps):
            fields = {VX: np.clip(B, -CAP_STEP, CAP_STEP), VY: np.clip(C, -CAP_STEP, CAP_STEP), VZ: np.clip(Dd, -CAP_STEP, CAP_STEP), DENS: A}
            add("sstep%d" % (k + 1), acc, fields, [("run_one", ())],
                [("sstep%d_%s" % (k + 1, NAMES[f]), f) for f in range(11) if f != OBS], keep=k > 0)
    return out


def run_pass(h, inp, ps, dtype=np.float32):
    """Run one pass of pass_list() on a handle (the reference shim, an oracle or a GPU Simulation: they share method names
    and field selectors) -> {output name: array}."""
    if not ps["keep"]:
        zero = np.zeros(inp["obs"].shape, dtype=dtype)
        h.set(OBS, inp["obs"])
        for f in range(11):
            if f != OBS:
                h.set(f, ps["fields"].get(f, zero))
    for method, args in ps["calls"]:
        getattr(h, method)(*args)
    return {name: h.get(f) for name, f in ps["outs"]}


def check_conditions(name, variant, arrays):
    """The conditions of a recorded case on {output name: array}: whole steps of a finite variant are finite; every
    output of a non-finite variant keeps its NaN share within NAN_SHARE_MAX and holds at least NONFINITE_MIN non-finite
    cells.  -> (largest NaN share, fewest non-finite cells) for the record."""
    worst, fewest = 0.0, None
    for k, a in arrays.items():
        if variant == "finite":
            if k.startswith(("step", "sstep")):
                assert np.isfinite(a).all(), "%s: %s is not finite" % (name, k)
            continue
        if k in ALL_ZERO:
            assert not a.any(), "%s: %s is not zero" % (name, k)
            continue
        share, n = nan_share(a), nonfinite_cells(a)
        assert share <= NAN_SHARE_MAX, "%s: %s is %.1f %% NaN" % (name, k, 100 * share)
        assert n >= NONFINITE_MIN, "%s: %s holds %d non-finite cells" % (name, k, n)
        worst = max(worst, share)
        fewest = n if fewest is None else min(fewest, n)
    return worst, fewest


def recorded_cases():
    """(W, H, D, obstacle kind, variant) of every case make_golden.py g8 records"""
    return [(W, H, D, o, v) for (W, H, D) in GRIDS for o in OBS_KINDS for v in VARIANTS
            if not ((W, H, D) == TINY and v == "nonfinite")]


# arrays (not only digests) are stored for these outputs of these cases, so that a failure can be located
STORED_CASES = [(5, 3, 2, o, "finite") for o in BINARY] + [(37, 21, 9, "s15", "finite"), (37, 21, 9, "s15", "nonfinite"),
                                                          (37, 21, 9, "faces", "finite")]
STORED_37 = {"finite": ("diffuse_b1", "lin_a1_acc4", "advect_b0", "advect_special_b1", "project_v_x", "project_pressure",
                        "project_divergence", "step2_v_x", "sstep2_dens"),
             "nonfinite": ("lin_a03_acc4", "advect_b0", "project_v_x", "project_pressure")}


def stored_outputs(W, H, D, variant, names):
    return list(names) if (W, H, D) == TINY else [n for n in names if n in STORED_37[variant]]
