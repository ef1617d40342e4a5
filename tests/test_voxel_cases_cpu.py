"""The voxelizer case table (tests/voxel_cases.py) on the oracle alone: every case reaches what it claims, so that the
expected masks of tests/test_gpu_voxelizer.py can be produced, and judged, on a machine without a GPU.

The conditions are fixed, not measured:
  * a case marked sensitive differs from itself at seed + 1 in at least 20 % of the cells of the two masks' union;
  * a clip case has odd-parity samples that the range test accepts on the face it names, and ones it rejects beyond it;
  * a case not marked degenerate has a non-empty mask;
  * the sample count per axis, the triangle count and the seed folding are what the table says.
Where the compiled reference exists, the oracle is also held to it on every clean file, in a child at one thread with the
seed the reference derives from its thread id, as tests/test_oracle_vs_ref.py does: that ties the oracle's restatement of
libstdc++'s generate_canonical and of the jitter to the real thing on meshes where they decide the answer."""
import os
import subprocess
import sys

import numpy as np
import pytest

import voxel_cases as V
from conftest import ROOT

FLOOR = 0.20


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    return V.write_all(tmp_path_factory.mktemp("voxel_cases"))


@pytest.fixture(scope="module")
def answers(oracle_mod, files):
    """the oracle's answer per (case name, seed), computed once"""
    memo = {}

    def get(c, seed=None):
        key = (c["name"], c["seed"] if seed is None else seed)
        if key not in memo:
            memo[key] = V.oracle_load(oracle_mod, c, files[c["name"]], seed=seed, trace=1 << 20 if c["clip"] else 0)
        return memo[key]
    return get


@pytest.mark.parametrize("c", V.CASES, ids=V.ids(V.CASES))
def test_case_is_what_the_table_says(oracle_mod, files, answers, c):
    tris = oracle_mod.Oracle(4, 4, 4).stl_triangles(files[c["name"]])
    a = answers(c)
    if c["ntri"] is None:
        assert len(tris) == 0 and a["added"] is None and not a["mask"].any()
        return
    assert len(tris) == c["ntri"]
    assert a["added"] is not None and a["ns"] == c["ns"]
    assert a["added"] >= int(a["mask"].sum())                    # several samples may mark one cell
    m = a["mask"]
    assert not (m[0].any() or m[-1].any() or m[:, 0].any() or m[:, -1].any() or m[:, :, 0].any() or m[:, :, -1].any())
    if not c["degenerate"]:
        assert a["added"] > 0 and m.any()
    if c["ns"] == 0:
        assert a["added"] == 0 and a["kept"] == 0
    if c["name"] == "ns_3":
        assert 0 < a["kept"] < 256
    if c["name"] == "outside":
        assert a["added"] == 0 and a["kept"] > 0


@pytest.mark.parametrize("c", V.SENSITIVE, ids=V.ids(V.SENSITIVE))
def test_sensitive_case_meets_the_floor(answers, c):
    share = V.differing_share(answers(c)["mask"], answers(c, c["seed"] + 1)["mask"])
    print("%s: seeds %d and %d differ in %.1f %% of the union" % (c["name"], c["seed"], c["seed"] + 1, 100 * share))
    assert share >= FLOOR


@pytest.mark.parametrize("c", V.CLIP, ids=V.ids(V.CLIP))
def test_clip_case_reaches_its_face(answers, c):
    a = answers(c)
    rec = a["records"]
    assert len(rec) == a["kept"]                                 # the whole stream was recorded
    odd = rec[(rec["crossings"] & 1) == 1]
    axis, side = c["clip"]
    n = c["grid"][axis]
    g = odd["xyz"][:, axis]
    inside = odd["cell"] >= 0
    on_face = inside & (g == (n if side else 1))
    beyond = ~inside & ((g > n) if side else (g < 1))
    assert on_face.any() and beyond.any()
    assert int(inside.sum()) == a["added"]
    # and nothing is dropped that lies inside on all three axes
    lo = (odd["xyz"] >= 1).all(axis=1) & (odd["xyz"] <= np.array(c["grid"])).all(axis=1)
    assert np.array_equal(lo, inside)


def test_seed_folding(answers):
    bowl = V.BY_NAME["bowl"]
    one = answers(bowl)["mask"]
    for s in V.FOLD_TO_ONE:
        assert np.array_equal(answers(V.BY_NAME["bowl_seed_%d" % s])["mask"], one), s
    assert V.differing_share(answers(V.BY_NAME["bowl_seed_%d" % (V.M31 - 1)])["mask"], one) >= FLOOR


def test_tile_cases_around_256_are_distinct(answers):
    """255, 256 and 257 triangles give three different masks: the 256th and the 257th triangle count"""
    m = [answers(V.BY_NAME["tris_%d" % n])["mask"] for n in (255, 256, 257)]
    assert (m[0] ^ m[1]).any() and (m[1] ^ m[2]).any()


CHILD = r'''
import os, sys, tempfile
sys.path.insert(0, %(root)r)
sys.path.insert(0, %(tests)r)
import numpy as np
from oracle import cpu_ref as O
import voxel_cases as V

with tempfile.TemporaryDirectory() as d:
    files = V.write_all(d)
    for c in V.CASES:
        if not c["clean"] or c["name"].startswith("bowl_seed_"):   # the seed is the reference's own: those are "bowl" again
            continue
        W, H, D = c["grid"]
        r = O.Reference(W, H, D)
        seed = r.thread_seed()
        kw = V.kwargs(c, seed)
        kw.pop("seed")
        r.load_stl(files[c["name"]], **kw)
        got = V.oracle_load(O, c, files[c["name"]], seed=seed)
        assert np.array_equal(r.get(O.OBS) > 0.5, got["mask"]), c["name"]
        assert set(np.unique(r.get(O.OBS))) <= {0.0, 1.0}, c["name"]
        assert c["degenerate"] or got["mask"].any(), c["name"]
        r.close()
print("\nok")   # may land inside a line of the reference's own block-buffered console output
'''


def test_oracle_matches_live_reference_on_clean_cases(oracle_mod):
    if not oracle_mod.have_reference():
        pytest.skip("the compiled reference is not on this machine")
    code = CHILD % {"root": ROOT, "tests": os.path.join(ROOT, "tests")}
    env = dict(os.environ, OMP_NUM_THREADS="1")
    out = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, timeout=600)
    assert out.returncode == 0, (out.stdout + out.stderr)[-3000:].decode(errors="replace")
    assert b"ok" in out.stdout.split()   # the reference's own buffered console lines may follow
