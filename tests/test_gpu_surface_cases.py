"""The four kernels of csrc/surface.hip against tests/surface_model.py on the cases of tests/surface_cases.py: vertices
and triangles byte for byte, order included (the ORDER and DEGENERATE clauses of include/fluidsim.h).  No tolerance
anywhere.  What each case is there for, and that it gets there, is shown without a GPU by
tests/test_surface_cases_cpu.py."""
import numpy as np
import pytest

import surface_cases as SC
import surface_model as M
from conftest import ball_mask

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def F():
    import fluid_simulation_amd as F
    return F


def handle(F, c):
    W, H, D = c.shape
    return F.Simulation(W, H, D, 1, quiet=1, dump_every=0, precision=c.precision)


def load(F, sim, c):
    """the case's array into its source, ghost layer included; what comes back is what was sent, bit for bit"""
    source = getattr(F, c.source)
    sim.set(source, c.array)
    back = sim.get(source)
    assert back.dtype == c.array.dtype and back.tobytes() == c.array.tobytes()
    return source


def first_difference(field, level, got, want):
    """where the device's mesh first leaves the model's: the vertex with its grid point and axis, the triangle with its
    cube and configuration"""
    (gv, gf), (wv, wf) = got, want
    lines = ["vertices %d (model %d), triangles %d (model %d)" % (len(gv), len(wv), len(gf), len(wf))]
    n = min(len(gv), len(wv))
    bad = np.flatnonzero((gv[:n].view(np.uint32) != wv[:n].view(np.uint32)).any(axis=1))
    if len(bad):
        i = int(bad[0])
        x, y, z, axis = (int(v) for v in M.vertex_owners(field, level)[i])
        hi = [z, y, x]
        hi[2 - axis] += 1
        lines.append("%d vertices differ; the first is %d, on the %s edge of grid point (%d, %d, %d), v0 = %r, v1 = %r: got %r, model %r"
                     % (len(bad), i, "xyz"[axis], x, y, z, field[z, y, x], field[tuple(hi)], gv[i].tolist(), wv[i].tolist()))
    m = min(len(gf), len(wf))
    bad = np.flatnonzero((gf[:m] != wf[:m]).any(axis=1))
    if len(bad):
        i = int(bad[0])
        x, y, z, cfg = (int(v) for v in M.triangle_cubes(field, level)[i])
        lines.append("%d triangles differ; the first is %d, of the cube at (%d, %d, %d) in configuration %d: got %r, model %r"
                     % (len(bad), i, x, y, z, cfg, gf[i].tolist(), wf[i].tolist()))
    return "\n".join(lines)


def assert_same(field, level, got, want):
    gv, gf = got
    wv, wf = want
    assert gv.dtype == np.float32 and gf.dtype == np.int32 and gv.shape[1:] == (3,) and gf.shape[1:] == (3,)
    if gv.tobytes() != wv.tobytes() or gf.tobytes() != wf.tobytes() or gv.shape != wv.shape or gf.shape != wf.shape:
        pytest.fail(first_difference(field, level, got, want))


@pytest.mark.parametrize("name", SC.ids())
def test_the_device_gives_the_models_mesh(F, name):
    c = SC.by_name(name)
    want = M.mesh(c.array, c.level)
    sim = handle(F, c)
    try:
        source = load(F, sim, c)
        assert_same(c.array, c.level, sim.isosurface(source, c.level), want)
        if c.source == "OBS":
            assert_same(c.array, c.level, sim.obstacle_surface(), want)
        if "empty" in c.reaches:
            assert want[0].shape == (0, 3) and want[1].shape == (0, 3)
        else:
            assert np.all(np.isfinite(want[0])) and len(want[1]) > 0
    finally:
        sim.close()


def test_the_same_bytes_again_and_between_other_meshes(F):
    """One long-row case twice on one handle, on a fresh handle, and interleaved with another case on the same handle (a
    stale vbase array, row offset or table would show)."""
    c, other = SC.by_name("long row fp32"), SC.by_name("long row mask fp32")
    assert c.shape == other.shape
    want, want_other = M.mesh(c.array, c.level), M.mesh(other.array, other.level)
    assert len(want[0]) != len(want_other[0])
    sim = handle(F, c)
    try:
        load(F, sim, c)
        first = sim.isosurface(F.DENS, c.level)
        second = sim.isosurface(F.DENS, c.level)
        assert_same(c.array, c.level, first, want)
        assert first[0].tobytes() == second[0].tobytes() and first[1].tobytes() == second[1].tobytes()
        load(F, sim, other)
        assert_same(other.array, other.level, sim.isosurface(F.OBS, other.level), want_other)
        assert_same(c.array, c.level, sim.isosurface(F.DENS, c.level), want)
        assert_same(other.array, other.level, sim.obstacle_surface(), want_other)
        assert_same(c.array, c.level, sim.isosurface(F.DENS, c.level), want)
        assert_same(c.array, 0.25, sim.isosurface(F.DENS, 0.25), M.mesh(c.array, 0.25))      # another level, then back
        assert_same(c.array, c.level, sim.isosurface(F.DENS, c.level), want)
    finally:
        sim.close()
    fresh = handle(F, c)
    try:
        load(F, fresh, c)
        assert_same(c.array, c.level, fresh.isosurface(F.DENS, c.level), want)
    finally:
        fresh.close()


@pytest.mark.parametrize("precision", ["fp32", "fp64"])
def test_a_vortex_source_in_the_models_order(F, precision):
    """The Q-criterion behind a ball after a few steps: the field the handle computes itself, exactly, order included."""
    W, H, D = 48, 24, 24
    sim = F.Simulation(W, H, D, 1, quiet=1, dump_every=0, precision=precision, acc=8)
    try:
        sim.set_mask(ball_mask(W, H, D, 14, 12, 12, 4))
        for _ in range(8):
            sim.run_one()
        q = sim.vortex(F.VORTEX_Q, dtype=sim.dtype)                       # exactly what the handle holds
        assert q.dtype == sim.dtype and q.max() > 0
        level = 0.25 * float(q.max())
        got = sim.isosurface(F.ISO_VORTEX | F.VORTEX_Q, level)
        want = M.mesh(q, level)
        assert len(want[0]) > 50 and len(want[1]) > 50
        assert_same(q, level, got, want)
    finally:
        sim.close()


def test_the_viewer_passes_the_meshes_through(F):
    from fluid_simulation_amd import viewer
    c = SC.by_name("non-finite fp32")
    want = M.mesh(c.array, c.level)
    sim = handle(F, c)
    try:
        load(F, sim, c)
        mesh = viewer.generate_isosurface_mesh(sim, F.DENS, c.level)
    finally:
        sim.close()
    assert set(mesh) == {"vertexes", "faces", "vertex_colors"}
    assert_same(c.array, c.level, (mesh["vertexes"].astype(np.float32), mesh["faces"]), want)
    assert np.array_equal(mesh["vertexes"], want[0].astype(np.float64))
    assert mesh["vertex_colors"].shape == (len(want[0]), 4)
    c = SC.by_name("random mask fp32")
    want = M.mesh(c.array, c.level)
    mesh = viewer.generate_obstacle_mesh(np.transpose(c.array, (2, 1, 0)))   # (x, y, z), as GUI/main_window.py:204 passes it
    assert set(mesh) == {"vertexes", "faces", "vertex_colors"}
    assert_same(c.array, c.level, (mesh["vertexes"].astype(np.float32), mesh["faces"]), want)
    assert np.array_equal(mesh["vertexes"], want[0].astype(np.float64))
    assert mesh["vertex_colors"].shape == (len(want[0]), 4)
