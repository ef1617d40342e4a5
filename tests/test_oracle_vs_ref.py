"""Comparison of the oracle with the compiled, unmodified reference (oracle/_ref/libref.so) on cases that are
not among the array goldens: six random tunnels and two voxelizer calls (tests/golden/g7_live_ref_digests.json).
Live wherever the reference shim exists (the build container; the GPU box when the prebuilt .so travelled);
elsewhere against the SHA-256 digests of every field the reference computed for the same inputs, recorded by
oracle/make_golden.py.  The reference is deterministic only at OMP_NUM_THREADS=1, which this file arranges by
running the comparison in a child."""
import os
import subprocess
import sys

from conftest import GOLDEN, ROOT

CHILD = r'''
import hashlib, json, os, sys
sys.path.insert(0, %(root)r)
import numpy as np
from oracle import cpu_ref as O

live = O.have_reference()
g = json.load(open(%(golden)r))

def digest(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()

def ball(W, H, D, cx, cy, cz, r):
    z, y, x = np.mgrid[0:D + 2, 0:H + 2, 0:W + 2]
    m = ((x - cx) ** 2 + (y - cy) ** 2 + (z - cz) ** 2) <= r * r
    m[0] = m[-1] = False; m[:, 0] = m[:, -1] = False; m[:, :, 0] = m[:, :, -1] = False
    return m

for c in g["cases"]:
    W, H, D = c["W"], c["H"], c["D"]
    kw = dict(iter=c["iter"], acc=c["acc"], speed=c["speed"], dt=c["dt"], diff=c["diff"])
    o = O.Oracle(W, H, D, solver=O.GS_LEX, threads=1, **kw)
    r = O.Reference(W, H, D, **kw) if live else None
    m = ball(W, H, D, *c["ball"])
    for s in (o, r) if live else (o,):
        s.set_mask(m)
        s.add_density(1 + W // 2, 1 + H // 2, 1 + D // 2, 0.7)
        s.set_velocity(1, 1, 1, 0.5, -0.25, 2.0)
    for step in range(c["iter"]):
        if live:
            r.run_one()
        o.run_one()
        for f in range(11):
            b = o.get(f)
            what = (W, H, D, c["acc"], step, O.FIELD_NAMES[f])
            if live:
                assert np.array_equal(r.get(f).view(np.uint32), b.view(np.uint32)), what
            else:
                assert digest(b) == c["sha256"][step][f], what

# voxelizer with fresh arguments; live, the seed is whatever the reference's thread-id hash is today
for v in g["voxelizer"]:
    stl = os.path.join(%(golden_dir)r, v["stl"])
    kw = dict(scale=v["scale"], rot=tuple(v["rot"]), translate=tuple(v["translate"]))
    o = O.Oracle(v["W"], v["H"], v["D"])
    if live:
        r = O.Reference(v["W"], v["H"], v["D"])
        seed = r.thread_seed()
        r.load_stl(stl, **kw)
        o.load_stl(stl, seed=seed, **kw)
        assert np.array_equal(r.get(O.OBS), o.get(O.OBS)), stl
        assert r.get(O.OBS).sum() > 0
    else:
        o.load_stl(stl, seed=v["seed"], **kw)
        assert digest(o.get(O.OBS)) == v["obs_sha256"], stl
        assert o.get(O.OBS).sum() == v["obs_cells"] > 0
print("ok")
'''


def test_oracle_matches_live_reference(oracle_mod):
    code = CHILD % {"root": ROOT, "golden": os.path.join(GOLDEN, "g7_live_ref_digests.json"), "golden_dir": GOLDEN}
    env = dict(os.environ, OMP_NUM_THREADS="1")
    out = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, (out.stdout + out.stderr)[-3000:]
    assert "ok" in out.stdout.split()   # the reference's own buffered console lines may follow
