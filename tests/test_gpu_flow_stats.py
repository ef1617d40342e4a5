"""Time-averaged flow statistics (options "flow_stats" / "flow_stats_every" / "flow_stats_start", fs_flow_stats_*) on the
MI355X, through the C ABI via the Python mirror: a hand case that fixes the definition of include/fluidsim.h, real steps
against a numpy fp64 restatement, sampling windows and resets, the error cases, no effect on the simulation, no cost
when off, z-slab runs bit-identical with one GPU, the mean-flow dump, and simulation.out --mean-flow.  Every comparison
is bit for bit: a cell's sums are a pure function of its sampled values and their order."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT, ball_mask, bits_equal

pytestmark = pytest.mark.gpu
WORKER = os.path.join(ROOT, "tests", "flow_stats_slab_worker.py")
PAIRS = [(1, 1), (2, 2), (3, 3), (1, 2), (1, 3), (2, 3), (4, 4)]      # uu vv ww uv uw vw pp, as indices into q u v w p
FAMILIES = ["sweep", "sweep_pair", "sweep_triple", "divergence", "gradient", "advect", "bounds", "misc", "comm", "multigrid",
            "forces", "residual"]


def sim_of(W, H, D, precision="fp32", **kw):
    import fluid_simulation_amd as F
    kw.setdefault("quiet", 1)
    kw.setdefault("dump_every", 0)
    return F.Simulation(W, H, D, 1, precision=precision, **kw)


def five(sim):
    import fluid_simulation_amd as F
    return [sim.get(f) for f in (F.DENS, F.VX, F.VY, F.VZ, F.PRESSURE)]


class Restated:
    """The definition of include/fluidsim.h in numpy fp64, one rounded operation per numpy call."""

    def __init__(self):
        self.S, self.n = None, 0

    def add(self, fields):
        d = [np.asarray(f).astype(np.float64) for f in fields]
        terms = d + [d[a] * d[b] for a, b in PAIRS]
        self.S = [np.float64(0.0) + t for t in terms] if self.n == 0 else [s + t for s, t in zip(self.S, terms)]
        self.n += 1

    def field(self, which, raw=False):
        if raw:
            return self.S[which]
        n = np.float64(self.n)
        if which < 5:
            return self.S[which] / n
        if which < 12:
            a, b = PAIRS[which - 5]
            m2 = self.S[which] / n
            mm = (self.S[a] / n) * (self.S[b] / n)
            return m2 - mm
        return ((self.field(5) + self.field(6)) + self.field(7)) * np.float64(0.5)


def check_all(sim, want, nsel=13, context=""):
    """every selector, raw and derived, fetched as fp64 and as fp32 (= the fp64 result cast to float32)"""
    import fluid_simulation_amd as F
    with np.errstate(all="ignore"):
        for which in range(nsel):
            for raw in ((False, True) if which != F.STAT_TKE else (False,)):
                w = want.field(which, raw)
                got = sim.flow_stats(which, raw=raw)
                assert got.dtype == np.float64 and bits_equal(got, w), (context, F.STAT_NAMES[which], raw, "fp64")
                got4 = sim.flow_stats(which, raw=raw, dtype=np.float32)
                assert got4.dtype == np.float32 and bits_equal(got4, w.astype(np.float32)), (context, F.STAT_NAMES[which], raw, "fp32")


# ---- 1. hand case -----------------------------------------------------------------------------------------------------

def test_hand_case_small_integers():
    """8x6x5, three samples of integer-valued fields base + offset: every sum, mean and covariance is an integer that
    fp64 holds exactly -- offsets q (1, 2, 3), u (-3, 0, 3), v (3, 0, -3), w (-6, 0, 6), p (3, 0, -3) give
    mean q = Q + 2, the others their base; var u = var v = var p = 6, var w = 24, cov uv = -6, uw = 12, vw = -12, tke = 18."""
    import fluid_simulation_amd as F
    W, H, D = 8, 6, 5
    rng = np.random.default_rng(11)
    shape = (D + 2, H + 2, W + 2)
    base = [rng.integers(-5, 6, size=shape).astype(np.float64) for _ in range(5)]
    offs = [(1, 2, 3), (-3, 0, 3), (3, 0, -3), (-6, 0, 6), (3, 0, -3)]
    sim = sim_of(W, H, D, flow_stats="moments")
    for i in range(3):
        for f, b, o in zip((F.DENS, F.VX, F.VY, F.VZ, F.PRESSURE), base, offs):
            sim.set(f, (b + o[i]).astype(np.float32))
        sim.flow_stats_sample()
    assert sim.flow_stats_samples == 3
    Q, U, V, Wz, P = base
    for which, b, o in zip(range(5), base, offs):
        assert bits_equal(sim.flow_stats(which, raw=True), 3 * b + sum(o)), which
        assert bits_equal(sim.flow_stats(which), b + sum(o) / 3.0), which
    sq = lambda b, o: sum((b + k) ** 2 for k in o)      # noqa: E731
    pr = lambda a, oa, b, ob: sum((a + i) * (b + j) for i, j in zip(oa, ob))      # noqa: E731
    raw2 = [sq(U, offs[1]), sq(V, offs[2]), sq(Wz, offs[3]), pr(U, offs[1], V, offs[2]), pr(U, offs[1], Wz, offs[3]),
            pr(V, offs[2], Wz, offs[3]), sq(P, offs[4])]
    for k, w in enumerate(raw2):
        assert bits_equal(sim.flow_stats(5 + k, raw=True), w), k
    for which, c in zip(range(5, 12), (6.0, 6.0, 24.0, -6.0, 12.0, -12.0, 6.0)):
        assert bits_equal(sim.flow_stats(which), np.full(shape, c)), which
    assert bits_equal(sim.flow_stats(F.STAT_TKE), np.full(shape, 18.0))
    assert bits_equal(sim.flow_stats(F.STAT_TKE, dtype=np.float32), np.full(shape, 18.0, dtype=np.float32))
    sim.close()


# ---- 2. real steps against numpy ----------------------------------------------------------------------------------------

def run_against_numpy(W, H, D, precision, solver, mask, steps=12):
    sim = sim_of(W, H, D, precision, solver=solver, acc=6, flow_stats="moments")
    if mask is not None:
        sim.set_mask(mask)
    want = Restated()
    for _ in range(steps):
        sim.run_one()
        want.add(five(sim))
    assert sim.flow_stats_samples == steps
    assert np.abs(want.field(1)).max() > 1.0, "the inlet should have given the tunnel a flow"
    check_all(sim, want, context=(W, H, D, precision, solver))
    sim.close()


@pytest.mark.parametrize("solver", ["jacobi", "mg"])
@pytest.mark.parametrize("precision", ["fp32", "fp64"])
@pytest.mark.parametrize("grid", [(24, 20, 16), (30, 17, 9), (300, 8, 6)])
def test_real_steps_match_numpy(grid, precision, solver):
    """12 run_one steps with "moments": a ball in 24x20x16, W not a multiple of four, a row of more than one wave."""
    W, H, D = grid
    mask = ball_mask(W, H, D, 8, 10, 8, 4) if grid == (24, 20, 16) else None
    run_against_numpy(W, H, D, precision, solver, mask)


def test_real_steps_match_numpy_bench_row_width():
    run_against_numpy(512, 64, 32, "fp32", "jacobi", ball_mask(512, 64, 32, 100, 32, 16, 10))


# ---- 3. windows -----------------------------------------------------------------------------------------------------------

def test_sampling_window_reset_and_clear():
    import fluid_simulation_amd as F
    W, H, D = 24, 20, 16
    sim = sim_of(W, H, D, acc=6, flow_stats="moments", flow_stats_start=5, flow_stats_every=3)
    sim.set_mask(ball_mask(W, H, D, 8, 10, 8, 4))
    want = Restated()
    for step in range(1, 21):
        sim.run_one()
        if step in (6, 9, 12, 15, 18):
            want.add(five(sim))
    assert sim.flow_stats_samples == 5
    check_all(sim, want, context="window")
    # a reset restarts the sums; the first sample after it overwrites what the arrays held
    sim.flow_stats_reset()
    assert sim.flow_stats_samples == 0
    sim.set_option("flow_stats_start", 0)
    sim.set_option("flow_stats_every", 1)
    want = Restated()
    sim.run_one()
    want.add(five(sim))
    assert sim.flow_stats_samples == 1
    check_all(sim, want, context="first sample after a reset")
    for _ in range(2):
        sim.run_one()
        want.add(five(sim))
    check_all(sim, want, context="after a reset")
    # setting the option again clears
    sim.set_option("flow_stats", "moments")
    assert sim.flow_stats_samples == 0
    with pytest.raises(F.FluidsimError):
        sim.flow_stats(F.STAT_MEAN_VX)
    assert bits_equal(sim.flow_stats(F.STAT_UU, raw=True), np.zeros(sim.shape))
    want = Restated()
    sim.flow_stats_sample()
    want.add(five(sim))
    check_all(sim, want, context="after setting the option again")
    # "mean" keeps the five sums only
    sim.set_option("flow_stats", "mean")
    want = Restated()
    for _ in range(3):
        sim.run_one()
        want.add(five(sim))
    assert sim.flow_stats_samples == 3
    check_all(sim, want, nsel=5, context="mean")
    sim.close()


# ---- 4. errors ------------------------------------------------------------------------------------------------------------

def test_errors():
    import fluid_simulation_amd as F

    def refused(call, *words):
        with pytest.raises(F.FluidsimError) as e:
            call()
        assert e.value.code == F._lib.EINVAL, e.value
        text = str(e.value)
        assert len(text) > 25 and all(w in text for w in words), text

    sim = sim_of(8, 6, 5)
    refused(lambda: sim.flow_stats(F.STAT_MEAN_VX), "off")                 # the feature is off
    refused(lambda: sim.flow_stats(F.STAT_MEAN_VX, raw=True), "off")
    refused(sim.flow_stats_sample, "off")
    refused(lambda: sim.flow_stats_dump("/tmp"), "off")
    assert sim.flow_stats_samples == 0
    refused(lambda: sim.set_option("flow_stats", "variance"), "mean")
    refused(lambda: sim.set_option("flow_stats_every", 0))
    refused(lambda: sim.set_option("flow_stats_start", -1))
    sim.set_option("flow_stats", "mean")
    refused(lambda: sim.flow_stats(F.STAT_MEAN_VX), "n = 0")               # no samples yet
    refused(lambda: sim.flow_stats_dump("/tmp"), "n = 0")
    sim.flow_stats_sample()
    sim.flow_stats(F.STAT_MEAN_VX)
    for which in (F.STAT_UU, F.STAT_PP, F.STAT_TKE):
        refused(lambda: sim.flow_stats(which), "moments")                  # second moments in mode "mean"
        if which != F.STAT_TKE:
            refused(lambda: sim.flow_stats(which, raw=True), "moments")
    sim.set_option("flow_stats", "moments")
    sim.flow_stats_sample()
    refused(lambda: sim.flow_stats(F.STAT_TKE, raw=True), "raw")           # tke has no raw sum
    refused(lambda: sim.flow_stats(13))
    refused(lambda: sim.flow_stats(-1))
    out = np.zeros(7)
    assert sim._L.fs_flow_stats_field(sim._h, 0, out.ctypes.data, out.size, 8) == F._lib.EINVAL      # wrong element count
    n = sim._L.fs_padded_size(sim._h)
    out = np.zeros(n)
    assert sim._L.fs_flow_stats_field(sim._h, 0, out.ctypes.data, n, 2) == F._lib.EINVAL             # wrong element size
    sim.set_option("flow_stats", "off")
    refused(lambda: sim.flow_stats(F.STAT_MEAN_VX), "off")
    sim.close()


# ---- 5. / 6. no effect on the simulation, no cost when off ------------------------------------------------------------------

@pytest.mark.parametrize("precision", ["fp32", "fp64"])
def test_no_effect_on_the_simulation(precision):
    W, H, D = 24, 20, 16
    runs = []
    for mode in ("off", "moments"):
        sim = sim_of(W, H, D, precision, acc=6, flow_stats=mode)
        sim.set_mask(ball_mask(W, H, D, 8, 10, 8, 4))
        for _ in range(10):
            sim.run_one()
        runs.append(five(sim))
        sim.close()
    for a, b in zip(*runs):
        assert bits_equal(a, b)


def test_off_launches_nothing():
    """Five profiled steps: with the feature off the "flow_stats" family counts no launch, and every other family counts
    what it counts with the feature on (one launch per sample there).  Fixed launch plans, so that no timed choice can
    make the two runs differ."""
    W, H, D = 24, 20, 16
    counts = {}
    for mode in ("off", "moments"):
        sim = sim_of(W, H, D, acc=6, flow_stats=mode, profile=1, sweep_fuse=2, two_sweep_kernel="pair", pair_shape=1)
        sim.set_mask(ball_mask(W, H, D, 8, 10, 8, 4))
        for _ in range(2):
            sim.run_one()
        sim.reset_timing()
        for _ in range(5):
            sim.run_one()
        counts[mode] = {f: sim.timing(f)[1] for f in FAMILIES + ["flow_stats"]}
        sim.close()
    assert counts["off"]["flow_stats"] == 0
    assert counts["moments"]["flow_stats"] == 5
    for f in FAMILIES:
        assert counts["off"][f] == counts["moments"][f], (f, counts)
    assert counts["off"]["advect"] > 0 and counts["off"]["sweep_pair"] > 0, counts


# ---- 7. z-slabs -------------------------------------------------------------------------------------------------------------

def ipc_usable():
    exe = os.path.join(ROOT, "tools", "ipc_probe")
    if not os.path.exists(exe):
        return False, "tools/ipc_probe was not built"
    r = subprocess.run([exe, "2", "8", "1"], capture_output=True, text=True, timeout=120,
                       env=dict(os.environ, FS_IPC_TIMEOUT_S="20"))
    return r.returncode == 0, (r.stdout + r.stderr)[-400:]


_SINGLE = {}
DUMP_FILES = ["data.bin", "obs.bin", "v_x.bin", "v_y.bin", "v_z.bin", "p.bin", "tke.bin"]


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
    files = {name: open(os.path.join(out, "mean", name), "rb").read() for name in DUMP_FILES}
    return ranks, files


@pytest.mark.parametrize("nranks,transport", [(2, "shm"), (4, "shm"), (2, "ipc"), (4, "ipc")])
def test_slabs_bit_identical_with_one_gpu(tmp_path, nranks, transport):
    import fluid_simulation_amd as F
    if transport == "ipc":
        ok, why = ipc_usable()
        if not ok:
            pytest.skip("FSIPC transport not usable on this box: " + why)
    W, H, D, steps = 32, 16, 32, 8
    if "ref" not in _SINGLE:
        _SINGLE["ref"] = run_ranks(str(tmp_path), 1, "single", W, H, D, steps)
    (ref,), ref_files = _SINGLE["ref"]
    assert int(ref["samples"]) == steps and np.abs(ref["tke"]).max() > 0
    ranks, files = run_ranks(str(tmp_path), nranks, transport, W, H, D, steps)
    Dl = D // nranks
    names = [k for k in ref if k not in ("samples", "zoff", "stream_syncs")]
    assert len(names) == 13 + 12 + 1
    for r, z in enumerate(ranks):
        assert int(z["samples"]) == steps and int(z["stream_syncs"]) == 0, (r, z["samples"], z["stream_syncs"])
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
    for name in DUMP_FILES:
        assert len(ref_files[name]) == (W + 2) * (H + 2) * (D + 2) * 4, name
        assert files[name] == ref_files[name], name
    assert ref_files["tke.bin"] == np.ascontiguousarray(ref["tke_f32"]).tobytes()
    assert ref_files["v_x.bin"] == ref["mean_vx"].astype(np.float32).tobytes()
    assert F.STAT_NAMES[F.STAT_TKE] == "tke"


# ---- 8. dump ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("precision,mode", [("fp32", "moments"), ("fp64", "moments"), ("fp32", "mean")])
def test_dump_is_one_float32_frame_per_file(tmp_path, precision, mode):
    import fluid_simulation_amd as F
    W, H, D = 24, 20, 16
    sim = sim_of(W, H, D, precision, acc=6, flow_stats=mode)
    sim.set_mask(ball_mask(W, H, D, 8, 10, 8, 4))
    for _ in range(6):
        sim.run_one()
    d = str(tmp_path)
    for name in DUMP_FILES:                              # stale, longer files: the dump truncates
        open(os.path.join(d, name), "wb").write(b"x" * ((W + 2) * (H + 2) * (D + 2) * 4 + 100))
    os.remove(os.path.join(d, "tke.bin"))
    sim.flow_stats_dump(d)
    sim.flow_stats_dump(d)                               # and does not append
    want = {"data.bin": F.STAT_MEAN_DENS, "v_x.bin": F.STAT_MEAN_VX, "v_y.bin": F.STAT_MEAN_VY, "v_z.bin": F.STAT_MEAN_VZ,
            "p.bin": F.STAT_MEAN_P}
    if mode == "moments":
        want["tke.bin"] = F.STAT_TKE
    else:
        assert not os.path.exists(os.path.join(d, "tke.bin"))
    for name, which in want.items():
        assert open(os.path.join(d, name), "rb").read() == sim.flow_stats(which, dtype=np.float32).tobytes(), name
    assert open(os.path.join(d, "obs.bin"), "rb").read() == sim.get(F.OBS, dtype=np.float32).tobytes()
    assert np.frombuffer(open(os.path.join(d, "obs.bin"), "rb").read(), dtype=np.float32).sum() > 0
    sim.close()


# ---- 9. simulation.out --mean-flow -------------------------------------------------------------------------------------------

def test_cli_mean_flow(tmp_path):
    import fluid_simulation_amd as F
    exe = os.path.join(ROOT, "simulation.out")
    assert os.path.exists(exe), "simulation.out is built by __graft_entry__.build()"
    d = tmp_path / "d"
    d.mkdir()
    env = {k: v for k, v in os.environ.items() if not k.startswith("FS_")}
    r = subprocess.run([exe, "--mean-flow", str(d), "--mean-from", "10", "--steps", "20", "--stl", "none", "--dump-every", "0",
                        "--quiet", "--json"], check=True, cwd=str(tmp_path), env=env, timeout=600, capture_output=True, text=True)
    line = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
    assert line["mean_flow_samples"] == 10 and line["steps"] == 20
    W, H, D = line["grid"]
    assert sorted(os.listdir(str(d))) == sorted(DUMP_FILES[:6])            # mode "mean": no tke.bin
    sim = F.Simulation(W, H, D, 20, quiet=1, dump_every=0, flow_stats="mean", flow_stats_start=10)
    sim.run()
    assert sim.flow_stats_samples == 10
    for name, which in (("data.bin", F.STAT_MEAN_DENS), ("v_x.bin", F.STAT_MEAN_VX), ("v_y.bin", F.STAT_MEAN_VY),
                        ("v_z.bin", F.STAT_MEAN_VZ), ("p.bin", F.STAT_MEAN_P)):
        assert (d / name).read_bytes() == sim.flow_stats(which, dtype=np.float32).tobytes(), name
    sim.close()
    # --mean-moments adds tke.bin; --mean-every thins the samples
    r = subprocess.run([exe, "--mean-flow", str(d), "--mean-moments", "--mean-every", "4", "--steps", "9", "--grid", "32x16x16",
                        "--stl", "none", "--dump-every", "0", "--quiet", "--json"], check=True, cwd=str(tmp_path), env=env,
                       timeout=600, capture_output=True, text=True)
    line = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
    assert line["mean_flow_samples"] == 3                                   # steps 1, 5, 9
    assert (d / "tke.bin").stat().st_size == 34 * 18 * 18 * 4 == (d / "v_x.bin").stat().st_size
