"""The oracle (oracle/cpu_ref.c) against the compiled, unmodified reference on rough and special-valued inputs: every pass
of the step and two whole steps on the cases of tests/rough_cases.py (back-traces that clamp at every wall, 15 % and 60 %
scattered solids with enclosed cells, solids in the first and last columns, rows and planes, obstacle values that are
neither 0 nor 1, subnormals, signed zeros, values at the normal / subnormal border, values whose sums overflow, and in the
non-finite variant +Inf, -Inf and NaN in the high corner).

Live wherever the reference shim exists (oracle/_ref/libref.so), array by array; elsewhere against the SHA-256 digests
oracle/make_golden.py g8 recorded from it (tests/golden/g8_rough_digests.json).  Every comparison is rough_cases.same():
bit equality after every NaN is mapped to one canonical NaN, because the reference's NaN sign and payload depend on its
compiler's operand order.  The reference is deterministic only at one thread, so each part runs in a child at
OMP_NUM_THREADS=1 (this file, run as a script).

  part      what is held to the reference
  gs_lex    the GS_LEX oracle on every recorded output of every case
  solvers   the JACOBI and RBSOR oracles on the passes that do not depend on the solver: set_bounds, advect, project at acc = 0
  fp64      the fp64 oracle on set_bounds (inputs widened exactly, outputs narrowed exactly: both only move and negate values)
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
DIGESTS = os.path.join(HERE, "golden", "g8_rough_digests.json")
ARRAYS = os.path.join(HERE, "golden", "g8_rough_37x21x9.npz")
SOLVER_FREE = ("set_bounds_", "advect_", "project0")


def _recorded():
    with open(DIGESTS) as f:
        return json.load(f)


# ---- in this process: the fixture itself -----------------------------------------------------------------------------------------
def test_recipe_reproduces_the_recorded_inputs():
    """A drift of numpy's generator (or an edit of the recipe without `make_golden.py g8`) fails here as "recipe changed"."""
    import rough_cases as R
    g = _recorded()
    assert [c["id"] for c in g["cases"]] == [R.case_id(*c) for c in R.recorded_cases()]
    for c in g["cases"]:
        inp = R.case_inputs(c["W"], c["H"], c["D"], c["obs"], c["variant"])
        assert sorted(inp) == sorted(c["inputs"])
        for k, a in inp.items():
            assert R.digest(a) == c["inputs"][k], "recipe changed: %s input %s" % (c["id"], k)
        assert not any(np.isnan(inp[k]).any() for k in ("ux", "uy", "uz"))
        names = [n for ps in R.pass_list(inp, c["variant"]) for n, _ in ps["outs"]]
        assert sorted(names) == sorted(c["outputs"])


def test_recorded_cases_hold_what_they_are_for():
    """The conditions asserted while recording, on the recorded numbers; and that the inputs are as rough as claimed."""
    import rough_cases as R
    g = _recorded()
    assert g["nan_share_max"] == R.NAN_SHARE_MAX == 0.10 and g["nonfinite_min"] == R.NONFINITE_MIN == 5
    for c in g["cases"]:
        shape = (c["W"], c["H"], c["D"])
        if c["variant"] == "nonfinite":
            assert shape != R.TINY
            for k, share in c["nan_share"].items():
                if k in R.ALL_ZERO:
                    continue
                assert share <= R.NAN_SHARE_MAX, (c["id"], k, share)
                assert c["nonfinite"][k] >= R.NONFINITE_MIN, (c["id"], k)
        else:
            assert "nan_share" not in c and any(k.startswith("step2_") for k in c["outputs"])
        if c["obs"] == "s60" and shape != R.TINY:
            assert c["enclosed"] > 0, c["id"]
        if c["obs"] == "faces" and shape != R.TINY:
            o = R.obstacles("faces", *shape)
            for face in (o[1:-1, 1:-1, 1], o[1:-1, 1:-1, -2], o[1:-1, 1, 1:-1], o[1:-1, -2, 1:-1], o[1, 1:-1, 1:-1], o[-2, 1:-1, 1:-1]):
                assert (face == 1).any(), c["id"]
        if c["obs"] == "odd" and shape != R.TINY:
            o = R.obstacles("odd", *shape)
            ghosts = np.ones(o.shape, dtype=bool)
            ghosts[1:-1, 1:-1, 1:-1] = False
            for region in (o[1:-1, 1:-1, 1:-1], o[ghosts]):
                assert np.isnan(region).any() and (region == 0.5).any() and (region == 2).any() and (region == -1).any()
                assert ((region > 1) & (region < 1.001)).any() and (region == 1).any()
    # the stored arrays are the recorded ones
    z = np.load(ARRAYS, allow_pickle=False)
    by_id = {c["id"]: c for c in g["cases"]}
    keys = [k for k in z.files if k != "meta"]
    assert len(keys) >= 40
    for k in keys:
        cid, out = k.split("__")
        assert R.digest(z[k]) == by_id[cid]["outputs"][out], k


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_every_special_field_holds_every_value_class(dtype):
    """Each of the four special fields of each grid but 5x3x2 holds subnormals, both zeros, both sides of the normal /
    subnormal border, huge values and plain ones, in the interior and on the ghost faces; the box edges are 0; the
    non-finite variant adds exactly the named cells."""
    import rough_cases as R
    from advect_model import box_edges
    fi = np.finfo(dtype)
    for W, H, D in R.GRIDS:
        if (W, H, D) == R.TINY:
            continue
        inp = R.case_inputs(W, H, D, "s15", "finite", dtype, mid=True)
        nf = R.case_inputs(W, H, D, "s15", "nonfinite", dtype, mid=True)
        named = R.named_cells(W, H, D, "corner+mid")
        assert len(named) == 6
        edges = box_edges(W, H, D)
        faces = ~edges
        faces[1:-1, 1:-1, 1:-1] = False
        for k in "ABCD":
            a = inp[k]
            assert a.dtype == dtype and not a[edges].any() and np.isfinite(a).all()
            for region in (a[1:-1, 1:-1, 1:-1], a[faces]):
                mag = np.abs(region)
                assert ((mag > 0) & (mag < fi.tiny / 64)).any()                      # subnormal integers
                assert ((region == 0) & np.signbit(region)).any() and ((region == 0) & ~np.signbit(region)).any()
                assert ((mag >= fi.tiny / 64) & (mag < fi.tiny)).any() and ((mag >= fi.tiny) & (mag < 8 * fi.tiny)).any()
                assert (mag > fi.max / 1000).any() and ((mag > 1e-3) & (mag < 10)).any()
            bad = ~np.isfinite(nf[k])
            assert int(bad.sum()) == 6 and all(bad[c] for c in named)
            same = nf[k].copy()
            for c in named:
                same[c] = a[c]
            assert same.tobytes() == a.tobytes()
        for kind in R.OBS_KINDS + ("clean", "none"):
            o = R.obstacles(kind, W, H, D, dtype=dtype)
            for (z, y, x) in named:
                assert o[z, y, x] == 0 and o[z, y, x + 1] == 0 and o[z, y, x - 1] == 0 and o[z + 1, y, x] == 0


def test_canonical_nan_helpers():
    import rough_cases as R
    a = np.array([1.0, np.nan, -0.0, np.inf], dtype=np.float32)
    b = a.copy()
    b.view(np.uint32)[1] = 0xFFC00123                      # another NaN: sign and payload differ
    assert a.tobytes() != b.tobytes() and R.same(a, b) and R.digest(a) == R.digest(b)
    c = a.copy()
    c[2] = 0.0                                             # +0 for -0 is a difference
    assert not R.same(a, c) and R.digest(a) != R.digest(c)
    assert not R.same(a, a.astype(np.float64))
    assert R.first_difference(a, c)[0] == (2,)


# ---- in a child at one thread: the oracle against the reference ------------------------------------------------------------------
@pytest.mark.parametrize("part", ["gs_lex", "solvers", "fp64"])
def test_oracle_matches_reference_on_rough_cases(oracle_mod, part):
    env = dict(os.environ, OMP_NUM_THREADS="1")
    out = subprocess.run([sys.executable, os.path.abspath(__file__), part], env=env, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, (out.stdout + out.stderr)[-4000:]
    assert "ok %s" % part in out.stdout, out.stdout[-2000:]


def _child(part):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, HERE)
    import rough_cases as R
    from oracle import cpu_ref as O
    live = O.have_reference()
    g = _recorded()
    stored = np.load(ARRAYS, allow_pickle=False)
    compared = 0
    for c in g["cases"]:
        W, H, D, variant = c["W"], c["H"], c["D"], c["variant"]
        inp = R.case_inputs(W, H, D, c["obs"], variant)
        passes = R.pass_list(inp, variant)
        if part != "gs_lex":
            passes = [ps for ps in passes if ps["name"].startswith(SOLVER_FREE)]
        if part == "fp64":
            passes = [ps for ps in passes if ps["name"].startswith("set_bounds_")]
            inp64 = {k: v.astype(np.float64) for k, v in inp.items()}
            passes64 = [ps for ps in R.pass_list(inp64, variant) if ps["name"].startswith("set_bounds_")]
        solvers = {"gs_lex": [O.GS_LEX], "solvers": [O.JACOBI, O.RBSOR], "fp64": [O.GS_LEX]}[part]
        refs, oras = {}, {}
        for i, ps in enumerate(passes):
            acc = ps["acc"]
            want = None
            if live:
                if acc not in refs:
                    refs[acc] = O.Reference(W, H, D, iter=1, acc=acc)
                want = R.run_pass(refs[acc], inp, ps)
                R.check_conditions(c["id"], variant, want)
                for k, a in want.items():                  # the live reference is the recorded one
                    assert R.digest(a) == c["outputs"][k], "reference differs from its record: %s %s" % (c["id"], k)
            for sol in solvers:
                if (sol, acc) not in oras:
                    oras[(sol, acc)] = O.Oracle(W, H, D, solver=sol, fp64=part == "fp64", threads=1, iter=1, acc=acc, omega=1.5)
                if part == "fp64":
                    got = {k: a.astype(np.float32) for k, a in R.run_pass(oras[(sol, acc)], inp64, passes64[i], np.float64).items()}
                else:
                    got = R.run_pass(oras[(sol, acc)], inp, ps)
                for k, a in got.items():
                    what = "%s %s (oracle solver %d, %s)" % (c["id"], k, sol, part)
                    key = c["id"] + "__" + k
                    ref = want[k] if live else (stored[key] if key in stored.files else None)
                    if ref is not None:
                        assert R.same(a, ref), "%s: first difference (cell, oracle, reference, cells) %s" % (what, R.first_difference(a, ref))
                    assert R.digest(a) == c["outputs"][k], what
                    compared += 1
                if not live:
                    R.check_conditions(c["id"], variant, got)
        for h in list(refs.values()) + list(oras.values()):
            h.close()
    print("ok %s: %d arrays, %s" % (part, compared, "live reference" if live else "recorded digests"))


if __name__ == "__main__":
    _child(sys.argv[1])
