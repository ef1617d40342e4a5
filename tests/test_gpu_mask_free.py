"""The three-sweep kernel's mask-free build (lane-aligned fp32 rows, one GPU): groups of plane iterations whose band rows hold
no kill byte run a body without kill bytes, and the z chunks are balanced per band by a cost model.  Neither may change a
bit: mask_free = 0, auto and 1 and the balanced / equal chunks must give the same fields as the oracle or the single-sweep
kernels, wherever the obstacles sit relative to bands, groups and chunk boundaries, and after the mask changes."""
import hashlib

import numpy as np
import pytest

from conftest import bits_equal

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def F():
    import fluid_simulation_amd as F
    return F


def _ball(W, H, D, cx, cy, cz, r):
    z, y, x = np.ogrid[0:D + 2, 0:H + 2, 0:W + 2]
    m = ((x - cx) ** 2 + (y - cy) ** 2 + (z - cz) ** 2) <= r * r
    m[0] = m[-1] = False
    m[:, 0] = m[:, -1] = False
    m[:, :, 0] = m[:, :, -1] = False
    return m


def _mask(kind, W, H, D):
    m = np.zeros((D + 2, H + 2, W + 2), dtype=bool)
    if kind == "band_overlap":                   # kill rows exactly on the rows bands 0/1 and 1/2 of 12-row bands share
        m[D // 3:D // 3 + 4, 7:11, W // 3:W // 3 + 30] = True
        m[D // 2, 15:19, 5] = True
    elif kind == "near_only":                    # solids whose near-solid ring reaches into a band the solid is not in
        m[D // 2, 6, 40] = m[D // 2 + 7, 11, W - 3] = m[D // 3, 19, W // 2] = True
    elif kind == "one_cell":
        m[D // 2, H // 2, W // 2] = True
        m[9, 9, 9] = True
    elif kind == "z_wall_group":                 # inside the general body's first / last groups
        m[2, H // 2, W // 4] = m[3, 9:12, 100:104] = m[D - 1, H // 2 - 1, W // 2] = True
    elif kind == "single_plane":                 # one plane: only the levels of some groups see it
        m[D // 2 + 1, 8:H - 8, W // 4:W // 2] = True
    elif kind == "ball_plate":
        m = _ball(W, H, D, W / 3.0, H / 2.0, D / 2.0, min(H, D) / 4.0)
        m[D // 3:2 * D // 3, H // 4:3 * H // 4, 2 * W // 3:2 * W // 3 + 3] = True
    return m


def _run(F, W, H, D, masks, opts, steps=2, acc=9, digest=False):
    sim = F.Simulation(W, H, D, 1, acc=acc, quiet=1)
    for k, v in opts.items():
        sim.set_option(k, v)
    for m in masks:                              # each mask for `steps` steps: a change between solves rebuilds the tables
        sim.set_mask(m)
        for _ in range(steps):
            sim.run_one()
    out = [hashlib.sha256(sim.get(f).tobytes()).hexdigest() if digest else sim.get(f) for f in range(11)]
    sim.close()
    return out


VARIANTS = [{"mask_free": "0"}, {"mask_free": "auto"}, {"mask_free": "1"}, {"mask_free": "1", "chunk_cost": "14,10,9"},
            {"mask_free": "1", "chunk_cost": "30,10,1"}]
KINDS = ["band_overlap", "near_only", "one_cell", "z_wall_group", "single_plane", "ball_plate"]


@pytest.mark.parametrize("W,H,D", [(512, 30, 60), (256, 46, 50)])
@pytest.mark.parametrize("kind", KINDS)
def test_mask_free_options_match_oracle(F, oracle_mod, W, H, D, kind):
    O = oracle_mod
    m = _mask(kind, W, H, D)
    ora = O.Oracle(W, H, D, solver=O.JACOBI, threads=4, acc=9)
    ora.set_mask(m)
    for _ in range(2):
        ora.run_one()
    ref = [ora.get(f) for f in range(11)]
    for opts in VARIANTS:
        got = _run(F, W, H, D, [m], dict(opts, sweep_fuse="4"))
        for f in range(11):
            assert bits_equal(got[f], ref[f]), "%s %dx%dx%d %s: %s" % (kind, W, H, D, opts, F.FIELD_NAMES[f])


@pytest.mark.parametrize("W,H,D", [(512, 60, 120), (256, 256, 256)])
def test_mask_free_with_mask_changes_and_short_chunks(F, W, H, D):
    """Mask A, then B, then an empty tunnel, each for two steps (the clean and chunk tables must follow every change), with
    obstacles straddling chunk boundaries (pair_zc forces many chunks), against the single-sweep kernels."""
    a = _mask("ball_plate", W, H, D)
    b = _mask("band_overlap", W, H, D)
    b[D // 4:D // 4 + 3, 1:H + 1, W // 2] = True
    masks = [a, b, np.zeros_like(a)]
    ref = _run(F, W, H, D, masks, {"sweep_fuse": "1"})
    for opts in VARIANTS[:4] + [{"mask_free": "1", "pair_zc": "13"}]:
        got = _run(F, W, H, D, masks, dict(opts, sweep_fuse="4"))
        for f in range(11):
            assert bits_equal(got[f], ref[f]), "%dx%dx%d %s: %s" % (W, H, D, opts, F.FIELD_NAMES[f])


def test_mask_free_bench_shape(F):
    """512^3 with a sphere and a plate (the benchmark's kind of obstacle) for one step: mask_free 0 and 1 give the same bits."""
    W = H = D = 512
    m = _ball(W, H, D, W / 4.0, H / 2.0, D / 2.0, 57.0)
    m[200:330, 150:360, 300:308] = True
    out = [_run(F, W, H, D, [m], {"mask_free": v}, steps=1, acc=6, digest=True) for v in ("0", "1")]
    for f in range(11):
        assert out[0][f] == out[1][f], F.FIELD_NAMES[f]


def test_mask_free_option_values(F):
    sim = F.Simulation(64, 16, 16, 1, quiet=1)
    for v in ("0", "auto", "1"):
        sim.set_option("mask_free", v)
    for v in ("0", "14,10,9"):
        sim.set_option("chunk_cost", v)
    for k, v in (("mask_free", "2"), ("chunk_cost", "1,0,1"), ("chunk_cost", "3,4"), ("chunk_cost", "-1,2,3")):
        with pytest.raises(Exception):
            sim.set_option(k, v)
    sim.close()
