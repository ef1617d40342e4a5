"""Vortex identification on the MI355X (fs_vortex_field, fs_vortex_dump), through the C ABI via the Python mirror: hand
fields that fix the definition of include/fluidsim.h, real steps against the numpy restatement of tests/vortex_model.py,
no effect on the simulation and no cost without a call, the error cases, the dump, simulation.out --vortex, and z-slab
runs bit-identical with one GPU.  Every comparison is bit for bit: a cell's value is a pure function of its 18 neighbour
values and its obs."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import vortex_model as M
from conftest import ROOT, ball_mask, bits_equal

pytestmark = pytest.mark.gpu
WORKER = os.path.join(ROOT, "tests", "vortex_slab_worker.py")
FAMILIES = ["sweep", "sweep_pair", "sweep_triple", "divergence", "gradient", "advect", "bounds", "misc", "comm", "multigrid",
            "forces", "residual", "flow_stats"]
DUMP_FILES = ["vort_x.bin", "vort_y.bin", "vort_z.bin", "vort_sq.bin", "q.bin"]


def sim_of(W, H, D, precision="fp32", **kw):
    import fluid_simulation_amd as F
    kw.setdefault("quiet", 1)
    kw.setdefault("dump_every", 0)
    return F.Simulation(W, H, D, 1, precision=precision, **kw)


def check_all(sim, want, context=""):
    """all five selectors, fetched as fp64 and as fp32: the fp64 result rounded once to the handle's precision, then
    converted as fs_get_field converts"""
    import fluid_simulation_amd as F
    with np.errstate(all="ignore"):
        for which in range(5):
            stored = want[which].astype(sim.dtype)
            got = sim.vortex(which)
            assert got.dtype == np.float64 and bits_equal(got, stored.astype(np.float64)), (context, F.VORTEX_NAMES[which], "fp64")
            got4 = sim.vortex(which, dtype=np.float32)
            assert got4.dtype == np.float32 and bits_equal(got4, stored.astype(np.float32)), (context, F.VORTEX_NAMES[which], "fp32")


# ---- 1. hand fields ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("precision", ["fp32", "fp64"])
@pytest.mark.parametrize("grid", [(8, 6, 5), (13, 7, 9)])
def test_hand_fields(grid, precision):
    """Rigid rotation, pure shear and plane strain written with fs_set_field, ghosts included: every target cell holds
    exactly the hand value, every other cell (ghosts, two solid cells) +0.0, sign bit included."""
    import fluid_simulation_amd as F
    W, H, D = grid
    k = 3.0
    z, y, x = (a.astype(np.float64) for a in np.mgrid[0:D + 2, 0:H + 2, 0:W + 2])
    zero = np.zeros_like(x)
    cases = {
        "rotation about z": ((-k * (y - 3), k * (x - 4), zero), (0, 0, 2 * k, 4 * k * k, k * k)),
        "rotation about x": ((zero, -k * (z - 2), k * (y - 3)), (2 * k, 0, 0, 4 * k * k, k * k)),
        "rotation about y": ((k * (z - 2), zero, -k * (x - 4)), (0, 2 * k, 0, 4 * k * k, k * k)),
        "shear": ((k * y, zero, zero), (0, 0, -k, k * k, 0)),
        "strain": ((k * x, -k * y, zero), (0, 0, 0, 0, -k * k)),
    }
    solid = np.zeros(x.shape, dtype=bool)
    solid[2, 3, 4] = solid[D, H, W] = True
    target = np.zeros(x.shape, dtype=bool)
    target[1:-1, 1:-1, 1:-1] = True
    target &= ~solid
    sim = sim_of(W, H, D, precision)
    sim.set_mask(solid)
    for name, (uvw, hand) in cases.items():
        for f, a in zip((F.VX, F.VY, F.VZ), uvw):
            sim.set(f, a.astype(sim.dtype))
        for which, value in enumerate(hand):
            for dtype in (np.float64, np.float32):
                got = sim.vortex(which, dtype=dtype)
                assert got.shape == x.shape and got.dtype == dtype
                assert np.all(got[target] == value), (name, which, dtype, got[target][:4], value)
                assert bits_equal(got[~target], np.zeros(int((~target).sum()), dtype=dtype)), (name, which, dtype)
    sim.close()


# ---- 2. real steps against numpy ----------------------------------------------------------------------------------------

@pytest.mark.parametrize("grid,precision,solver", [
    ((32, 16, 16), "fp32", "jacobi"),
    ((24, 20, 12), "fp64", "jacobi"),
    ((37, 11, 6), "fp32", "jacobi"),                     # odd extents, W not a multiple of four
    ((37, 11, 6), "fp64", "jacobi"),
    ((64, 32, 32), "fp32", "mg"),
    ((512, 8, 8), "fp32", "jacobi"),                     # rows of two waves
    ((512, 8, 8), "fp64", "jacobi"),
    ((5, 1, 1), "fp32", "jacobi"),                       # one row, one plane
])
def test_real_steps_match_numpy(grid, precision, solver):
    import fluid_simulation_amd as F
    W, H, D = grid
    sim = sim_of(W, H, D, precision, solver=solver, acc=6)
    r = max(1.0, min(H, D) / 4.0)
    if min(grid) > 1:
        sim.set_mask(ball_mask(W, H, D, W / 3.0, H / 2.0, D / 2.0, r))
    for _ in range(8):
        sim.run_one()
    u, v, w, obs = (sim.get(f) for f in (F.VX, F.VY, F.VZ, F.OBS))
    want = M.fields(u, v, w, obs)
    if min(grid) > 1:
        assert obs.sum() > 0 and np.abs(want[M.WZ]).max() > 0, "the ball should have shed some vorticity"
        assert np.abs(want[M.Q]).max() > 0
    check_all(sim, want, context=(grid, precision, solver))
    # the other launch shape gives the same bits
    sim.set_option("vortex_ry", 1)
    check_all(sim, want, context=(grid, precision, solver, "vortex_ry=1"))
    sim.close()


# ---- 3. no side effects -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("precision", ["fp32", "fp64"])
def test_changes_no_field(precision):
    import fluid_simulation_amd as F
    W, H, D = 24, 20, 12
    sim = sim_of(W, H, D, precision, acc=6)
    sim.set_mask(ball_mask(W, H, D, 8, 10, 6, 3))
    for _ in range(5):
        sim.run_one()
    before = [sim.get(f) for f in range(11)]
    for which in range(5):
        sim.vortex(which)
        sim.vortex(which, dtype=np.float32)
    sim.isosurface(F.ISO_VORTEX | F.VORTEX_Q, 0.0)
    after = [sim.get(f) for f in range(11)]
    for f, (a, b) in enumerate(zip(before, after)):
        assert bits_equal(a, b), F.FIELD_NAMES[f]
    sim.close()


def test_calls_every_step_change_nothing_and_count_one_launch_each():
    """Two profiled runs with fixed launch plans, one fetching Q and WX after every step: the same eleven fields, the
    "vortex" family counts one launch per call (0 without a call), every other family counts the same."""
    W, H, D = 24, 20, 16
    fields, counts = {}, {}
    for calls in (False, True):
        sim = sim_of(W, H, D, acc=6, profile=1, sweep_fuse=2, two_sweep_kernel="pair", pair_shape=1)
        sim.set_mask(ball_mask(W, H, D, 8, 10, 8, 4))
        for _ in range(2):
            sim.run_one()
        sim.reset_timing()
        for _ in range(5):
            sim.run_one()
            if calls:
                sim.vortex(M.Q)
                sim.vortex(M.WX, dtype=np.float32)
        counts[calls] = {f: sim.timing(f)[1] for f in FAMILIES + ["vortex"]}
        fields[calls] = [sim.get(f) for f in range(11)]
        sim.close()
    assert counts[False]["vortex"] == 0
    assert counts[True]["vortex"] == 10
    for f in FAMILIES:
        assert counts[False][f] == counts[True][f], (f, counts)
    assert counts[False]["advect"] > 0 and counts[False]["gradient"] > 0, counts
    for a, b in zip(fields[False], fields[True]):
        assert bits_equal(a, b)


# ---- 4. errors --------------------------------------------------------------------------------------------------------------

def test_errors():
    import fluid_simulation_amd as F
    EINVAL = F._lib.EINVAL
    sim = sim_of(8, 6, 5)
    n = sim._L.fs_padded_size(sim._h)
    out = np.zeros(n)
    for which in (5, -1, 512):
        assert sim._L.fs_vortex_field(sim._h, which, out.ctypes.data, n, 8) == EINVAL, which
        assert len(sim._L.fs_last_error()) > 20
    assert sim._L.fs_vortex_field(sim._h, 4, out.ctypes.data, n - 1, 8) == EINVAL           # wrong element count
    assert b"elements" in sim._L.fs_last_error()
    assert sim._L.fs_vortex_field(sim._h, 4, out.ctypes.data, n, 2) == EINVAL               # wrong element size
    assert b"elem_size" in sim._L.fs_last_error()
    assert sim._L.fs_vortex_field(sim._h, 4, None, n, 8) == EINVAL
    assert sim._L.fs_vortex_dump(sim._h, None) == EINVAL
    for source in (F.ISO_VORTEX | 7, F.ISO_VORTEX | 5, 11, -1, 1024):
        with pytest.raises(F.FluidsimError) as e:
            sim.isosurface(source, 0.0)
        assert e.value.code == EINVAL, source
    assert sim._L.fs_isosurface_fetch(sim._h, None, None) == EINVAL                           # nothing computed yet
    assert sim._L.fs_vortex_field(sim._h, 4, out.ctypes.data, n, 8) == 0
    sim.close()


def test_null_transport_refuses():
    import fluid_simulation_amd as F
    sim = sim_of(8, 8, 8)
    sim.comm_init(0, 2, b"FSNULL:".ljust(128, b"\0"))
    for call in (lambda: sim.vortex(F.VORTEX_Q), lambda: sim.vortex_dump("/tmp")):
        with pytest.raises(F.FluidsimError) as e:
            call()
        assert e.value.code == F._lib.EINVAL and "FSNULL" in str(e.value)
    sim.close()


# ---- 5. dump ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("precision", ["fp32", "fp64"])
def test_dump_is_one_float32_frame_per_file(tmp_path, precision):
    W, H, D = 24, 20, 16
    sim = sim_of(W, H, D, precision, acc=6)
    sim.set_mask(ball_mask(W, H, D, 8, 10, 8, 4))
    for _ in range(6):
        sim.run_one()
    d = str(tmp_path)
    for name in DUMP_FILES:                              # stale, longer files: the dump truncates
        open(os.path.join(d, name), "wb").write(b"x" * ((W + 2) * (H + 2) * (D + 2) * 4 + 100))
    sim.vortex_dump(d)
    sim.vortex_dump(d)                                   # and does not append
    for which, name in enumerate(DUMP_FILES):
        data = open(os.path.join(d, name), "rb").read()
        assert len(data) == (W + 2) * (H + 2) * (D + 2) * 4, name
        assert data == sim.vortex(which, dtype=np.float32).tobytes(), name
    assert np.abs(np.frombuffer(open(os.path.join(d, "q.bin"), "rb").read(), dtype=np.float32)).max() > 0
    with pytest.raises(Exception):
        sim.vortex_dump(os.path.join(d, "no", "such", "directory"))
    sim.close()


def test_cli_vortex(tmp_path):
    import fluid_simulation_amd as F
    exe = os.path.join(ROOT, "simulation.out")
    assert os.path.exists(exe), "simulation.out is built by __graft_entry__.build()"
    stl = os.path.join(ROOT, "tests", "golden", "sphere_24x12.stl")   # an empty tunnel stays uniform: no vorticity at all
    d = tmp_path / "d"
    d.mkdir()
    env = {k: v for k, v in os.environ.items() if not k.startswith("FS_")}
    r = subprocess.run([exe, "--vortex", str(d), "--steps", "9", "--grid", "32x16x16", "--stl", stl + ",0.5,0,0,0,-4,0,0",
                        "--dump-every", "0", "--quiet", "--json"], check=True, cwd=str(tmp_path), env=env, timeout=600,
                       capture_output=True, text=True)
    line = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
    assert line["steps"] == 9 and line["grid"] == [32, 16, 16]
    assert sorted(os.listdir(str(d))) == sorted(DUMP_FILES)
    sim = F.Simulation(32, 16, 16, 9, quiet=1, dump_every=0)
    assert F.loadSTLIntoObstacles(stl, sim, 0.5, 0.0, 0.0, 0.0, -4.0, 0.0, 0.0) > 0
    sim.run()
    assert sim.get(F.OBS).sum() > 0, "the sphere should give the tunnel a body"
    assert np.abs(sim.vortex(F.VORTEX_WZ)).max() > 0 and np.abs(sim.vortex(F.VORTEX_Q)).max() > 0
    for which, name in enumerate(DUMP_FILES):
        assert (d / name).read_bytes() == sim.vortex(which, dtype=np.float32).tobytes(), name
    sim.close()


# ---- 6. z-slabs -------------------------------------------------------------------------------------------------------------

def ipc_usable():
    exe = os.path.join(ROOT, "tools", "ipc_probe")
    if not os.path.exists(exe):
        return False, "tools/ipc_probe was not built"
    r = subprocess.run([exe, "2", "8", "1"], capture_output=True, text=True, timeout=120,
                       env=dict(os.environ, FS_IPC_TIMEOUT_S="20"))
    return r.returncode == 0, (r.stdout + r.stderr)[-400:]


_SINGLE = {}


def run_ranks(tmp, nranks, transport, W, H, D, steps):
    import fluid_simulation_amd as F
    out = os.path.join(tmp, "%s_n%d" % (transport, nranks))
    os.makedirs(out)
    idfile = os.path.join(out, "id.bin")
    if nranks > 1:
        open(idfile, "wb").write(F.comm_unique_id(transport))
    procs = [subprocess.Popen([sys.executable, WORKER, str(r), str(nranks), idfile, out, str(W), str(H), str(D), str(steps)],
                              env=dict(os.environ, FS_IPC_TIMEOUT_S="60")) for r in range(nranks)]
    for p in procs:
        assert p.wait(timeout=600) == 0
    ranks = [dict(np.load(os.path.join(out, "rank%d.npz" % r))) for r in range(nranks)]
    files = {name: open(os.path.join(out, "vortex", name), "rb").read() for name in DUMP_FILES}
    return ranks, files


@pytest.mark.parametrize("nranks,transport", [(2, "shm"), (3, "shm"), (4, "shm"), (2, "ipc"), (3, "ipc"), (4, "ipc")])
def test_slabs_bit_identical_with_one_gpu(tmp_path, nranks, transport):
    import fluid_simulation_amd as F
    if transport == "ipc":
        ok, why = ipc_usable()
        if not ok:
            pytest.skip("FSIPC transport not usable on this box: " + why)
    W, H, D, steps = 32, 16, 24, 8
    if "ref" not in _SINGLE:
        _SINGLE["ref"] = run_ranks(str(tmp_path), 1, "single", W, H, D, steps)
    (ref,), ref_files = _SINGLE["ref"]
    # the one-GPU run itself is what the definition says
    want = M.fields(ref["vx"], ref["vy"], ref["vz"], ref["obs"])
    for which, name in enumerate(F.VORTEX_NAMES):
        assert bits_equal(ref[name], want[which].astype(np.float32).astype(np.float64)), name
    assert np.abs(ref["q"]).max() > 0 and np.abs(ref["mid_q"]).max() > 0
    ranks, files = run_ranks(str(tmp_path), nranks, transport, W, H, D, steps)
    Dl = D // nranks
    names = list(F.VORTEX_NAMES) + ["q_f32", "mid_q"]
    for r, z in enumerate(ranks):
        zoff = int(z["zoff"])
        assert zoff == r * Dl
        for k in names:
            assert z[k].shape == (Dl + 2, H + 2, W + 2)
            lo = 0 if r == 0 else 1                       # the planes a rank owns, and the physical ghost planes it holds
            hi = Dl + 1 if r == nranks - 1 else Dl
            assert bits_equal(z[k][lo:hi + 1], ref[k][zoff + lo:zoff + hi + 1]), (r, k)
            zero = np.zeros((H + 2, W + 2), dtype=z[k].dtype)
            if r > 0:
                assert bits_equal(z[k][0], zero), (r, k, "lower halo plane")
            if r < nranks - 1:
                assert bits_equal(z[k][Dl + 1], zero), (r, k, "upper halo plane")
        for k in ("vx", "vy", "vz"):                     # and the run itself is the one-GPU run
            assert bits_equal(z[k][1:Dl + 1], ref[k][zoff + 1:zoff + Dl + 1]), (r, k)
    for which, name in enumerate(DUMP_FILES):
        assert len(ref_files[name]) == (W + 2) * (H + 2) * (D + 2) * 4, name
        assert files[name] == ref_files[name], name
        assert ref_files[name] == ref[F.VORTEX_NAMES[which]].astype(np.float32).tobytes(), name
