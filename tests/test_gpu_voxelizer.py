"""fs_load_stl on the GPU against the oracle (oracle/cpu_ref.c, cr_load_stl) on the case table of tests/voxel_cases.py: mask
and count cell for cell, in both precisions, on meshes where the random stream decides the answer (an open shell at one
sample per cell), at the triangle counts around the LDS tile, at sample counts of 0, 1 and 3, on every face of the grid, on
every file format, on malformed files, and on z-slabs.  tests/test_voxel_cases_cpu.py proves on the oracle that each case
reaches what it claims.  No tolerance anywhere."""
import ctypes

import numpy as np
import pytest

import voxel_cases as V
from conftest import bits_equal

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def F():
    import fluid_simulation_amd as F
    return F


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    return V.write_all(tmp_path_factory.mktemp("voxel_cases"))


@pytest.fixture(scope="module")
def answers(oracle_mod, files):
    """the oracle's answer per (case name, grid, seed), computed once and shared by both precisions and the slabs"""
    memo = {}

    def get(c, seed=None):
        key = (c["name"], c["grid"], c["translate"], c["seed"] if seed is None else seed)
        if key not in memo:
            memo[key] = V.oracle_load(oracle_mod, c, files[c["name"]], seed=seed)
        return memo[key]
    return get


def gpu_load(F, c, path, precision="fp32", seed=None, sim=None):
    """-> (sim, what loadSTLIntoObstacles returned)"""
    W, H, D = c["grid"]
    if sim is None:
        sim = F.Simulation(W, H, D, 1, acc=2, quiet=1, precision=precision, voxel_seed=c["seed"] if seed is None else seed)
    return sim, F.loadSTLIntoObstacles(path, sim, c["scale"], *c["rot"], *c["translate"])


def exact_mask(F, sim):
    """OBS as a mask, after checking that it holds nothing but 0 and 1"""
    obs = sim.get(F.OBS)
    assert obs.dtype == sim.dtype
    assert np.array_equal(obs, (obs != 0).astype(obs.dtype))                 # exactly 1.0 where set
    return obs > 0.5


# ---- 1. mask and count, every case, both precisions -----------------------------------------------------------------------

@pytest.mark.parametrize("precision", ["fp32", "fp64"])
@pytest.mark.parametrize("c", V.CASES, ids=V.ids(V.CASES))
def test_mask_and_count_match_the_oracle(F, files, answers, c, precision):
    want = answers(c)
    sim, added = gpu_load(F, c, files[c["name"]], precision)
    got = exact_mask(F, sim)
    sim.close()
    assert added == want["added"]                                            # None where the file holds no triangle
    assert np.array_equal(got, want["mask"])
    if c["sensitive"]:
        # the seed reaches the kernel: the neighbouring seed gives another mask, the oracle's for that seed
        other = answers(c, c["seed"] + 1)
        sim, added = gpu_load(F, c, files[c["name"]], precision, seed=c["seed"] + 1)
        got2 = exact_mask(F, sim)
        sim.close()
        assert (got2 ^ got).any()
        assert added == other["added"] and np.array_equal(got2, other["mask"])


# ---- 2. accumulation --------------------------------------------------------------------------------------------------------

SMALL = (24, 16, 12)


def small(name, **kw):
    return dict(V.BY_NAME[name], grid=SMALL, **kw)


@pytest.mark.parametrize("precision", ["fp32", "fp64"])
def test_two_loads_accumulate_and_the_flags_are_rebuilt(F, oracle_mod, files, precision):
    """Two loads into one handle add up; a load after a step changes the next step exactly as it does on the oracle."""
    O = oracle_mod
    W, H, D = SMALL
    a = small("tris_12", scale=0.5, translate=(-5.0, 0.0, 0.0))
    b = small("bowl", scale=0.6, translate=(5.0, 1.0, -1.0))
    fp64 = precision == "fp64"
    sim = F.Simulation(W, H, D, 2, acc=6, quiet=1, precision=precision, voxel_seed=9)
    ora = O.Oracle(W, H, D, solver=O.JACOBI, fp64=fp64, iter=2, acc=6)
    _, n = gpu_load(F, a, files[a["name"]], sim=sim)
    assert n == ora.load_stl(files[a["name"]], **V.kwargs(a, 9)) > 0
    first = exact_mask(F, sim)
    assert np.array_equal(first, ora.get(O.OBS) > 0.5)
    sim.run_one()
    ora.run_one()
    _, n = gpu_load(F, b, files[b["name"]], sim=sim)
    assert n == ora.load_stl(files[b["name"]], **V.kwargs(b, 9)) > 0
    both = exact_mask(F, sim)
    assert np.array_equal(both, ora.get(O.OBS) > 0.5)
    assert (both & ~first).any() and not (first & ~both).any()               # the second mesh came on top of the first
    sim.run_one()
    ora.run_one()
    for f in range(11):
        assert bits_equal(sim.get(f), ora.get(f)), F.FIELD_NAMES[f]
    sim.close()


# ---- 3. degenerate and malformed files ----------------------------------------------------------------------------------------

def bad_paths(tmp_path, files):
    out = {}
    for name, (data, _) in V.bad_files().items():
        p = tmp_path / (name + ".stl")
        p.write_bytes(data)
        out[name] = str(p)
    out["missing"] = str(tmp_path / "none.stl")
    for name in ("solid_header_binary", "ns_0", "outside"):
        out[name] = files[name]
    return out


def test_degenerate_and_malformed_files_leave_the_handle_whole(F, oracle_mod, files, tmp_path):
    """Every such file gives what the oracle gives -- None where no triangle could be read, else a count, 0 included -- and
    leaves the obstacles that were there alone; the handle then steps."""
    O = oracle_mod
    c = small("bowl", scale=1.0)
    W, H, D = SMALL
    expect_none = {"empty", "83_bytes", "84_bytes_count_0", "missing", "solid_header_binary"}
    expect_zero = {"ns_0", "outside", "text_not_stl"}
    for name, path in sorted(bad_paths(tmp_path, files).items()):
        case = V.BY_NAME[name] if name in ("ns_0", "outside") else c
        case = dict(case, grid=SMALL)
        sim = F.Simulation(W, H, D, 1, acc=2, quiet=1, voxel_seed=c["seed"])
        ora = O.Oracle(W, H, D)
        sim.addObstacle(2, 3, 4)
        ora.add_obstacle(2, 3, 4)
        _, added = gpu_load(F, case, path, sim=sim)
        n = ora.load_stl(path, **V.kwargs(case))
        assert added == (None if n < 0 else n), name
        if name in expect_none:
            assert added is None, name
        if name in expect_zero:
            assert added == 0, name
        if name in ("truncated_in_record_3", "count_ffffffff_3_records", "count_2_of_5_records"):
            assert added is not None, name
        got = exact_mask(F, sim)
        assert np.array_equal(got, ora.get(O.OBS) > 0.5), name
        assert got[4, 3, 2]
        if name in expect_none | expect_zero:
            assert int(got.sum()) == 1, name
        sim.run_one()
        sim.close()


# ---- 4. device memory -----------------------------------------------------------------------------------------------------------

def test_loads_do_not_leak_device_memory(F, files, tmp_path):
    """30 loads into one handle, a third of them failing ones: free device memory moves by less than 64 MiB (the bound and
    the method of test_create_destroy_does_not_leak_device_memory)."""
    hip = ctypes.CDLL("libamdhip64.so.7")
    total = ctypes.c_size_t()
    bad = bad_paths(tmp_path, files)
    c = V.BY_NAME["bowl"]
    sim = F.Simulation(*c["grid"], 1, acc=2, quiet=1, voxel_seed=1)

    def cycle(n):
        for i in range(n):
            if i % 3 == 2:
                name = ("missing", "empty", "solid_header_binary", "84_bytes_count_0")[(i // 3) % 4]
                assert gpu_load(F, c, bad[name], sim=sim)[1] is None
            else:
                k = V.BY_NAME["tris_1020" if i % 3 else "bowl"]
                assert gpu_load(F, dict(k, grid=c["grid"]), files[k["name"]], sim=sim)[1] > 0

    cycle(3)                               # warm up allocator pools / code objects
    free0, free1 = ctypes.c_size_t(), ctypes.c_size_t()
    assert hip.hipMemGetInfo(ctypes.byref(free0), ctypes.byref(total)) == 0
    cycle(30)
    assert hip.hipMemGetInfo(ctypes.byref(free1), ctypes.byref(total)) == 0
    leaked = int(free0.value) - int(free1.value)
    assert leaked < 64 << 20, "device memory shrank by %d MB over 30 loads" % (leaked >> 20)
    sim.run_one()
    sim.close()


# ---- 5. z-slabs -------------------------------------------------------------------------------------------------------------------

SLAB_CASES = [
    dict(V.BY_NAME["rot_25_40_70"], grid=(64, 48, 36)),                               # the bowl, tilted across all slabs
    dict(V.BY_NAME["clip_z+"], grid=(24, 20, 18), translate=(0.0, 0.0, 18 / 2.0 - 1.5)),
    dict(V.BY_NAME["clip_z-"], grid=(24, 20, 18), translate=(0.0, 0.0, -(18 / 2.0 - 1.5))),
]


@pytest.mark.parametrize("precision", ["fp32", "fp64"])
@pytest.mark.parametrize("ranks,rank", [(2, 0), (2, 1), (3, 1)])
@pytest.mark.parametrize("c", SLAB_CASES, ids=V.ids(SLAB_CASES))
def test_slab_marks_its_planes_and_its_halo_planes(F, files, answers, c, ranks, rank, precision):
    """A slab rank holds planes z_offset .. z_offset + local_depth + 1 of the single-GPU mask: its own and one halo plane on
    either side (deeper halo planes are not visible through get).  No step is run, so the FSNULL transport, which moves
    nothing, is enough."""
    want = answers(c)
    W, H, D = c["grid"]
    sim = F.Simulation(W, H, D, 1, acc=2, quiet=1, precision=precision, voxel_seed=c["seed"])
    sim.comm_init(rank, ranks, b"FSNULL:".ljust(128, b"\0"))
    _, added = gpu_load(F, c, files[c["name"]], sim=sim)
    assert added == want["added"]                                            # the count is the whole mesh's on every rank
    got = exact_mask(F, sim)
    z0, dl = sim.z_offset, sim.local_depth
    assert dl == D // ranks and z0 == rank * dl
    part = want["mask"][z0:z0 + dl + 2]
    assert got.shape == part.shape and np.array_equal(got, part)
    if not c["clip"]:                                                        # the bowl lies in every slab and in its halo planes
        assert part[1:-1].any() and (part[0].any() or part[-1].any())
    sim.close()
