"""Vorticity confinement on the MI355X (fs_confine_vorticity, option "vorticity_confinement"), through the C ABI via the
Python mirror: the fused kernel against the numpy restatement of include/fluidsim.h (tests/confine_model.py) on grids that
take every path of its tiling, hand fields, degenerate inputs, a step with the option against pass + step without it, the
CPU oracle driven with the model, "off means off", the error cases and simulation.out --confinement.  Every comparison is
bit for bit."""
import os
import subprocess

import numpy as np
import pytest

import confine_model as M
from conftest import ROOT, GOLDEN, ball_mask, bits_equal

pytestmark = pytest.mark.gpu
FAMILIES = ["sweep", "sweep_pair", "sweep_triple", "divergence", "gradient", "advect", "bounds", "misc", "comm", "multigrid",
            "forces", "residual", "flow_stats", "vortex", "probes", "body_forces", "images", "tracers", "volume"]
EPS = 0.37                                               # eps * dt is no power of two


def sim_of(W, H, D, precision="fp32", **kw):
    import fluid_simulation_amd as F
    kw.setdefault("quiet", 1)
    kw.setdefault("dump_every", 0)
    return F.Simulation(W, H, D, 1, precision=precision, **kw)


def zero_edges(a):
    """the twelve edges of the padded box (ghost in two or three directions) hold 0, as include/fluidsim.h demands"""
    g = np.zeros(a.shape, dtype=np.int8)
    g[0] += 1
    g[-1] += 1
    g[:, 0] += 1
    g[:, -1] += 1
    g[:, :, 0] += 1
    g[:, :, -1] += 1
    a = a.copy()
    a[g >= 2] = 0
    return a


def masks(W, H, D):
    """name -> padded boolean mask; every kind is clipped to the box, so each exists on every grid"""
    cx, cy, cz = (W + 1) // 2, (H + 1) // 2, (D + 1) // 2
    out = {"none": np.zeros((D + 2, H + 2, W + 2), dtype=bool)}
    m = out["none"].copy()
    m[cz, cy, min(3, W)] = True
    out["one voxel"] = m
    out["ball"] = ball_mask(W, H, D, W / 2.0, H / 2.0, D / 2.0, max(1.0, min(W, H, D) / 3.0))
    m = out["none"].copy()
    m[1:min(2, D) + 1, 1:min(2, H) + 1, 1:min(3, W) + 1] = True
    out["block on a wall"] = m
    m = out["none"].copy()
    m[cz, cy, 2] = m[cz, cy, 4] = True
    out["one-cell gap"] = m
    m = out["none"].copy()
    for dz, dy, dx in ((0, 0, 1), (0, 0, -1), (0, 1, 0), (0, -1, 0), (1, 0, 0), (-1, 0, 0)):
        z, y, x = cz + dz, cy + dy, cx + dx
        if 1 <= z <= D and 1 <= y <= H and 1 <= x <= W:
            m[z, y, x] = True
    out["enclosed cell"] = m
    return out


def same(a, b, nan_ok):
    """bit for bit; with nan_ok a NaN matches a NaN of any sign and payload (host and device propagate them differently)"""
    if not nan_ok:
        return bits_equal(a, b)
    na, nb = np.isnan(a), np.isnan(b)
    return bool(np.array_equal(na, nb)) and bits_equal(np.where(na, 0, a), np.where(nb, 0, b))


def expect_pass(sim, ref, fields, mask, eps, context, nan_ok=False):
    """`sim` holds `fields` (11 padded arrays, OBS = the mask) and runs one pass; `ref` receives the model's result through
    fs_set_field, then fs_set_bounds (1, 2, 3).  All eleven fields of the two handles must hold the same bits."""
    import fluid_simulation_amd as F
    for h in (sim, ref):
        h.set_mask(mask)
    for f in range(11):
        if f != F.OBS:
            sim.set(f, fields[f])
    obs = sim.get(F.OBS)
    k = float(sim.dt) * float(eps)                           # (double)dt * eps, rounded once
    new = M.confine(fields[F.VX], fields[F.VY], fields[F.VZ], obs, k)
    for f in range(11):
        if f != F.OBS:
            ref.set(f, new[f - F.VX] if f in (F.VX, F.VY, F.VZ) else fields[f])
    for b, f in ((1, F.VX), (2, F.VY), (3, F.VZ)):
        ref.set_bounds(b, f)
    before = sim._geti("confinement_passes")
    sim.confine_vorticity(eps)
    assert sim._geti("confinement_passes") == before + 1
    for f in range(11):
        got, want = sim.get(f), ref.get(f)
        assert same(got, want, nan_ok), (context, F.FIELD_NAMES[f], np.argwhere(got.view(np.uint8) != want.view(np.uint8))[:4])
        if f not in (F.VX, F.VY, F.VZ, F.OBS):
            assert same(got, fields[f], nan_ok), (context, F.FIELD_NAMES[f], "changed")
    return new


# ---- 1. the pass against the model -----------------------------------------------------------------------------------------

# (6, 5, 17): the kernel chunks z by march_launch's rule with its own workgroup target (confine_launch in confine.hip: chunks of
# at least 8 planes), which on a one-tile layer gives chunks of 8, 8 and 1 planes
@pytest.mark.parametrize("precision", ["fp32", "fp64"])
@pytest.mark.parametrize("grid", [(5, 1, 1), (4, 1, 1), (13, 7, 9), (516, 4, 3), (8, 37, 4), (6, 5, 17)])
def test_pass_matches_the_model(grid, precision):
    W, H, D = grid
    sim, ref = sim_of(W, H, D, precision), sim_of(W, H, D, precision)
    rng = np.random.default_rng([W, H, D])
    shape = (D + 2, H + 2, W + 2)
    changed = 0
    for name, mask in masks(W, H, D).items():
        fields = [zero_edges((rng.standard_normal(shape) * 10.0 ** rng.integers(-2, 2)).astype(sim.dtype)) for _ in range(11)]
        new = expect_pass(sim, ref, fields, mask, EPS, (grid, precision, name))
        changed += sum(int((a != b).sum()) for a, b in zip(new, fields[1:4]))
    assert changed > 0, "the force should move something"
    sim.close()
    ref.close()


# ---- 2. hand fields -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("precision", ["fp32", "fp64"])
@pytest.mark.parametrize("which", [0, 1, 2])
def test_hand_fields(which, precision):
    """u = a y^2 (v = a z^2, w = a x^2) written with its analytic ghosts: every interior cell comes back as a s^2 - 2 a k s,
    the other two components stay zero.  dt = 1/16 and eps = 4 make k = dt * eps = 0.25 exactly."""
    import fluid_simulation_amd as F
    W, H, D, a = 7, 6, 5, 3.0
    sim = sim_of(W, H, D, precision, dt=0.0625)
    eps = 4.0
    k = float(sim.dt) * eps
    assert k == 0.25
    u, v, w, comp, s = M.hand_field(which, sim.dtype, W, H, D, a)
    for f, arr in zip((F.VX, F.VY, F.VZ), (u, v, w)):
        sim.set(f, zero_edges(arr))
    sim.confine_vorticity(eps)
    c = slice(1, -1)
    for j, f in enumerate((F.VX, F.VY, F.VZ)):
        want = (a * s * s - 2 * a * k * s) if j == comp else np.zeros(s.shape)
        got = sim.get(f)
        assert np.array_equal(got[c, c, c], want[c, c, c].astype(sim.dtype)), (which, j)
    sim.close()


@pytest.mark.parametrize("precision", ["fp32", "fp64"])
def test_lamb_oseen_vortex_is_spun_up(precision):
    import fluid_simulation_amd as F
    sim = sim_of(32, 32, 5, precision, dt=0.0625)
    eps = 4.0
    u, v, w, rx, ry, r2 = M.lamb_oseen(sim.dtype)
    u, v, w = zero_edges(u), zero_edges(v), zero_edges(w)
    for f, arr in zip((F.VX, F.VY, F.VZ), (u, v, w)):
        sim.set(f, arr)
    sim.confine_vorticity(eps)
    out = [sim.get(f) for f in (F.VX, F.VY, F.VZ)]
    c = slice(1, -1)
    w_in = w.copy()
    out[2][0], out[2][-1] = w_in[0], w_in[-1]                # w's z ghosts are reflected zeros: -0.0; the interior is what counts
    tmin, ratio = M.check_co_rotation(u, v, w, out, rx, ry, r2)
    print("smallest tangential increment %.3e, largest radial/tangential %.3f" % (tmin, ratio))
    want = M.confine(u, v, w, np.zeros(u.shape, dtype=sim.dtype), float(sim.dt) * eps)
    for a, b in zip(out, want):
        assert bits_equal(a[c, c, c], b[c, c, c])
    sim.close()


# ---- 3. degenerate inputs -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("precision", ["fp32", "fp64"])
def test_degenerate_inputs(precision):
    import fluid_simulation_amd as F
    W, H, D = 13, 7, 9
    sim, ref = sim_of(W, H, D, precision), sim_of(W, H, D, precision)
    x, y, z = M.grid(W, H, D)
    zero = np.zeros(x.shape, dtype=sim.dtype)
    negz = zero_edges(-zero)                                 # -0.0 in every cell but the box edges, which hold +0.0
    shear = zero_edges((3.0 * y).astype(sim.dtype))
    c = slice(1, -1)
    for name, (u, v, w) in {"zero": (zero, zero, zero), "shear": (shear, zero, zero), "minus zero": (negz, zero, negz),
                            "shear and minus zero": (shear, negz, negz)}.items():
        for f, arr in zip((F.VX, F.VY, F.VZ), (u, v, w)):
            sim.set(f, arr)
        sim.confine_vorticity(EPS)
        for f, arr in zip((F.VX, F.VY, F.VZ), (u, v, w)):
            assert bits_equal(sim.get(f)[c, c, c], arr[c, c, c]), (name, f)
    # a NaN in one cell changes only what the model changes
    rng = np.random.default_rng(5)
    fields = [zero_edges(rng.standard_normal(x.shape).astype(sim.dtype)) for _ in range(11)]
    fields[F.VY][4, 3, 6] = np.nan
    mask = masks(W, H, D)["one voxel"]
    new = expect_pass(sim, ref, fields, mask, EPS, "NaN", nan_ok=True)
    nan_cells = sum(int(np.isnan(a[c, c, c]).sum()) for a in new)
    assert 1 <= nan_cells < 60, nan_cells                    # the cell itself, and the few cells whose stencil holds it
    sim.close()
    ref.close()


# ---- 4. a step with the option = a pass, then the step without it ---------------------------------------------------------------

@pytest.mark.parametrize("precision,solver", [("fp32", "jacobi"), ("fp64", "jacobi"), ("fp32", "gs_lex")])
def test_step_with_the_option_is_pass_then_step(precision, solver):
    W, H, D = 24, 20, 12
    mask = ball_mask(W, H, D, 8, 10, 6, 3)
    a = sim_of(W, H, D, precision, solver=solver, acc=6, vorticity_confinement=0.5)
    b = sim_of(W, H, D, precision, solver=solver, acc=6)
    assert a._getf("vorticity_confinement") == 0.5 and b._getf("vorticity_confinement") == 0.0
    for h in (a, b):
        h.set_mask(mask)
    for step in range(6):
        a.run_one()
        b.confine_vorticity(0.5)
        b.run_one()
        for f in range(11):
            assert bits_equal(a.get(f), b.get(f)), (step, f)
    assert a._geti("confinement_passes") == 6 and b._geti("confinement_passes") == 6
    a.close()
    b.close()


# ---- 5. against the oracle ------------------------------------------------------------------------------------------------

def test_steps_match_the_oracle_driven_with_the_model(oracle_mod):
    import fluid_simulation_amd as F
    O = oracle_mod
    W, H, D, acc, eps = 24, 20, 12, 6, 0.5
    mask = ball_mask(W, H, D, 8, 10, 6, 3)
    sim = sim_of(W, H, D, "fp32", acc=acc, vorticity_confinement=eps)
    ora = O.Oracle(W, H, D, solver=O.JACOBI, iter=4, acc=acc)
    sim.set_mask(mask)
    ora.set_mask(mask)
    k = float(sim.dt) * eps
    moved = 0
    for step in range(4):
        u, v, w, obs = (ora.get(f) for f in (F.VX, F.VY, F.VZ, F.OBS))
        new = M.confine(u, v, w, obs, k)
        moved += int((new[0] != u).sum())
        for f, arr, b in ((F.VX, new[0], 1), (F.VY, new[1], 2), (F.VZ, new[2], 3)):
            ora.set(f, arr)
            ora.set_bounds(b, f)
        ora.run_one()
        sim.run_one()
        for f in (F.VX, F.VY, F.VZ, F.DENS):
            assert bits_equal(sim.get(f), ora.get(f)), (step, F.FIELD_NAMES[f])
    assert moved > 0, "the ball's wake should give the force something to do"
    sim.close()
    ora.close()


# ---- 6. off means off -----------------------------------------------------------------------------------------------------

def test_off_means_off():
    W, H, D = 24, 20, 12
    mask = ball_mask(W, H, D, 8, 10, 6, 3)
    counts, fields = {}, {}
    for how in ("untouched", "zero", "on"):
        sim = sim_of(W, H, D, acc=6, profile=1, sweep_fuse=2, two_sweep_kernel="pair", pair_shape=1)
        if how == "zero":
            sim.set_option("vorticity_confinement", "0")
        elif how == "on":
            sim.set_option("vorticity_confinement", 0.5)
        sim.set_mask(mask)
        for _ in range(5):
            sim.run_one()
        counts[how] = {f: sim.timing(f)[1] for f in FAMILIES + ["confinement"]}
        fields[how] = [sim.get(f) for f in range(11)]
        sim.close()
    assert counts["untouched"] == counts["zero"], counts
    assert counts["zero"]["confinement"] == 0 and counts["on"]["confinement"] == 5
    for f in FAMILIES:
        assert counts["on"][f] == counts["zero"][f], (f, counts)
    assert counts["zero"]["advect"] > 0 and counts["zero"]["gradient"] > 0, counts
    for a, b in zip(fields["untouched"], fields["zero"]):
        assert bits_equal(a, b)
    assert not bits_equal(fields["on"][1], fields["zero"][1])


# ---- 7. errors ------------------------------------------------------------------------------------------------------------

def test_errors():
    import fluid_simulation_amd as F
    EINVAL = F._lib.EINVAL
    sim = sim_of(8, 6, 5)
    sim.set_option("vorticity_confinement", 0.25)
    for bad in (-1.0, -1e-300, float("nan"), float("inf"), float("-inf")):
        assert sim._L.fs_confine_vorticity(sim._h, bad) == EINVAL, bad
        assert b"epsilon" in sim._L.fs_last_error()
        with pytest.raises(F.FluidsimError) as e:
            sim.set_option("vorticity_confinement", bad)
        assert e.value.code == EINVAL, bad
        assert sim._getf("vorticity_confinement") == 0.25
    for bad in ("", "abc", "0.5x", "1,0"):
        with pytest.raises(F.FluidsimError) as e:
            sim.set_option("vorticity_confinement", bad)
        assert e.value.code == EINVAL and sim._getf("vorticity_confinement") == 0.25, bad
    assert sim._geti("confinement_passes") == 0
    sim.confine_vorticity(0.0)                               # a no-op
    assert sim._geti("confinement_passes") == 0
    sim.confine_vorticity(0.5)
    sim.step()
    assert sim._geti("confinement_passes") == 2
    sim.close()


def test_slab_handles_refuse():
    import fluid_simulation_amd as F
    sim = sim_of(8, 8, 8)
    sim.comm_init(0, 2, b"FSNULL:".ljust(128, b"\0"))
    with pytest.raises(F.FluidsimError) as e:
        sim.confine_vorticity(0.5)
    assert e.value.code == F._lib.EINVAL and "single GPU" in str(e.value)
    sim.set_option("vorticity_confinement", 0.5)
    with pytest.raises(F.FluidsimError) as e:
        sim.step()
    assert e.value.code == F._lib.EINVAL and "single GPU" in str(e.value)
    assert sim._geti("confinement_passes") == 0
    sim.close()


# ---- 8. simulation.out --confinement ------------------------------------------------------------------------------------------

def test_cli_confinement_writes_the_same_frames(tmp_path):
    import fluid_simulation_amd as F
    exe = os.path.join(ROOT, "simulation.out")
    assert os.path.exists(exe), "simulation.out is built by __graft_entry__.build()"
    stl = os.path.join(GOLDEN, "sphere_24x12.stl")
    cli, py = tmp_path / "cli", tmp_path / "py"
    cli.mkdir()
    py.mkdir()
    env = {k: v for k, v in os.environ.items() if not k.startswith("FS_")}
    subprocess.run([exe, "--grid", "16x8x8", "--steps", "3", "--stl", stl + ",0.25,0,0,0,-2,0,0", "--dump-every", "1", "--dump-dir",
                    str(cli), "--quiet", "--confinement", "0.5"], check=True, cwd=str(tmp_path), env=env, timeout=600)
    sim = F.Simulation(16, 8, 8, 3, quiet=1, dump_every=1, dump_dir=str(py), vorticity_confinement=0.5)
    assert F.loadSTLIntoObstacles(stl, sim, 0.25, 0.0, 0.0, 0.0, -2.0, 0.0, 0.0) > 0
    sim.run()
    sim.sync()
    assert sim.get(F.OBS).sum() > 0, "the sphere should give the tunnel a body"
    assert sim._geti("confinement_passes") == 3
    sim.close()
    names = sorted(os.listdir(str(py)))
    assert names and names == sorted(os.listdir(str(cli)))
    for name in names:
        a, b = (py / name).read_bytes(), (cli / name).read_bytes()
        assert len(a) >= 18 * 10 * 10 * 4 and a == b, name
    # a value the option refuses is refused here too
    r = subprocess.run([exe, "--grid", "16x8x8", "--steps", "1", "--stl", "none", "--dump-every", "0", "--quiet", "--confinement", "-1"],
                       cwd=str(tmp_path), env=env, timeout=600, capture_output=True, text=True)
    assert r.returncode != 0 and "vorticity_confinement" in r.stderr
