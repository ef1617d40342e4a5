"""fs_isosurface on the MI355X: the marching-cubes extractor of fs_obstacle_surface freed from `obs` at 0.5.  A smooth
scalar field at two levels and the Q-criterion behind a ball are checked against the vertex formula of
include/fluidsim.h restated in numpy (tests/vortex_model.py) bit for bit, and for what any correct iso-surface must
satisfy (closed, consistently oriented, normals from inside to outside); the obstacle mesh is byte-identical through
either entry point, and the two result slots are independent."""
import ctypes as C

import numpy as np
import pytest

import vortex_model as M
from conftest import ball_mask, bits_equal

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def F():
    import fluid_simulation_amd as F
    return F


def check_mesh(field, level, verts, faces, normals=True):
    """field: the padded (z, y, x) array in the handle's precision.  normals: also check every single triangle's normal
    (for a smooth, well resolved field; the whole mesh's orientation is checked either way).  Returns (V, E, F)."""
    want, outward = M.iso_vertices(field, level)
    nv = len(verts)
    assert verts.dtype == np.float32 and faces.dtype == np.int32
    assert nv == len(want)                                                # one vertex per crossing edge of the padded box
    assert len(np.unique(want, axis=0)) == nv, "the test's levels are chosen so that no two edges share a vertex position"
    order = np.lexsort((verts[:, 2], verts[:, 1], verts[:, 0]))
    assert bits_equal(verts[order], want)                                 # the vertex set, order-free, bit for bit
    assert faces.min() >= 0 and faces.max() < nv and len(np.unique(faces)) == nv
    # closed and consistently oriented: each directed edge once, its reverse once
    e = np.concatenate([faces[:, [0, 1]], faces[:, [1, 2]], faces[:, [2, 0]]]).astype(np.int64)
    key = e[:, 0] * nv + e[:, 1]
    rev = e[:, 1] * nv + e[:, 0]
    assert len(np.unique(key)) == len(key)
    assert np.array_equal(np.sort(key), np.sort(rev))
    # normals: from the inside end to the outside end of the edges the triangle's vertices lie on
    out_of = np.empty_like(outward)
    out_of[order] = outward
    p0, p1, p2 = (verts[faces[:, k]].astype(np.float64) for k in range(3))
    normal = np.cross(p1 - p0, p2 - p0)
    toward = out_of[faces[:, 0]] + out_of[faces[:, 1]] + out_of[faces[:, 2]]
    dots = np.einsum("ij,ij->i", normal, toward)
    if normals:
        assert np.all(dots > 0), (int((dots <= 0).sum()), len(dots))
    assert dots.sum() > 0
    vol = float(np.einsum("ij,ij->i", p0, np.cross(p1, p2)).sum() / 6.0)
    assert vol > 0
    return nv, len(key) // 2, len(faces)


def bump(W, H, D):
    z, y, x = (a.astype(np.float64) for a in np.mgrid[0:D + 2, 0:H + 2, 0:W + 2])
    r2 = (x - 9.3) ** 2 / 30.0 + (y - 6.7) ** 2 / 14.0 + (z - 5.1) ** 2 / 8.0
    return np.exp(-r2) + 0.04 * np.sin(0.7 * x + 0.3 * y - 0.5 * z)


@pytest.mark.parametrize("level", [0.35, 0.6180339887])
@pytest.mark.parametrize("precision", ["fp32", "fp64"])
def test_smooth_scalar_field(F, precision, level):
    W, H, D = 20, 14, 10
    sim = F.Simulation(W, H, D, 1, quiet=1, precision=precision)
    sim.set(F.DENS, bump(W, H, D).astype(sim.dtype))
    a = sim.get(F.DENS)
    assert a.dtype == sim.dtype and len(np.unique(a)) > 1000              # not a 0/1 field
    inside = a > a.dtype.type(level)
    assert inside.sum() > 20 and not inside[0].any() and not inside[-1].any() and not inside[:, 0].any() \
        and not inside[:, -1].any() and not inside[:, :, 0].any() and not inside[:, :, -1].any()
    verts, faces = sim.isosurface(F.DENS, level)
    V, E, Fc = check_mesh(a, level, verts, faces)
    assert V - E + Fc == 2                                                # one closed surface of genus 0
    v2, f2 = sim.isosurface(F.DENS, level)                                # deterministic
    assert np.array_equal(verts, v2) and np.array_equal(faces, f2)
    sim.close()


def test_nan_is_outside_and_an_empty_mesh(F):
    W, H, D = 20, 14, 10
    sim = F.Simulation(W, H, D, 1, quiet=1)
    a = bump(W, H, D).astype(np.float32)
    a[5, 7, 9] = np.nan                                                   # a cell deep inside the 0.35 surface
    sim.set(F.DENS, a)
    verts, faces = sim.isosurface(F.DENS, 0.35)
    with np.errstate(invalid="ignore"):
        inside = sim.get(F.DENS) > np.float32(0.35)
    m = inside.astype(bool)
    crossing = int((m[:, :, 1:] != m[:, :, :-1]).sum() + (m[:, 1:, :] != m[:, :-1, :]).sum() + (m[1:, :, :] != m[:-1, :, :]).sum())
    assert not m[5, 7, 9] and len(verts) == crossing
    # DEGENERATE (include/fluidsim.h): every vertex is finite, and the six around the NaN cell are their edges' midpoints
    assert np.all(np.isfinite(verts))
    assert m[5, 7, 8] and m[5, 7, 10] and m[5, 6, 9] and m[5, 8, 9] and m[4, 7, 9] and m[6, 7, 9]
    rows = {tuple(v) for v in verts.tolist()}
    for mid in ((8.5, 7, 5), (9.5, 7, 5), (9, 6.5, 5), (9, 7.5, 5), (9, 7, 4.5), (9, 7, 5.5)):
        assert mid in rows, mid
    assert faces.min() >= 0 and faces.max() < len(verts) and len(np.unique(faces)) == len(verts)
    verts, faces = sim.isosurface(F.DENS, 5.0)                           # nothing is above 5
    assert verts.shape == (0, 3) and faces.shape == (0, 3)
    sim.close()


@pytest.mark.parametrize("precision", ["fp32", "fp64"])
def test_q_criterion_behind_a_ball(F, precision):
    from fluid_simulation_amd import viewer
    W, H, D = 48, 24, 24
    sim = F.Simulation(W, H, D, 1, quiet=1, dump_every=0, precision=precision, acc=8)
    sim.set_mask(ball_mask(W, H, D, 14, 12, 12, 4))
    for _ in range(20):
        sim.run_one()
    q = sim.vortex(F.VORTEX_Q, dtype=sim.dtype)                           # exactly what the handle holds
    assert q.max() > 0
    level = 0.25 * float(q.max())                                         # a fixed fraction of the run's own maximum
    verts, faces = sim.isosurface(F.ISO_VORTEX | F.VORTEX_Q, level)
    assert len(verts) > 0 and len(faces) > 0
    V, E, Fc = check_mesh(q, level, verts, faces, normals=False)
    assert (V - E + Fc) % 2 == 0                                          # closed surfaces only
    mesh = viewer.generate_isosurface_mesh(sim, F.ISO_VORTEX | F.VORTEX_Q, level)
    assert set(mesh) == {"vertexes", "faces", "vertex_colors"}
    assert np.array_equal(mesh["vertexes"].astype(np.float32), verts) and np.array_equal(mesh["faces"], faces)
    assert mesh["vertex_colors"].shape == (len(verts), 4)
    # the other vortex sources run too: |omega|^2 at a fraction of its maximum
    w2 = sim.vortex(F.VORTEX_W2, dtype=sim.dtype)
    lv = 0.5 * float(w2.max())
    v2, f2 = sim.isosurface(F.ISO_VORTEX | F.VORTEX_W2, lv)
    check_mesh(w2, lv, v2, f2, normals=False)
    sim.close()


def stl_mask_sim(F, tmp_path):
    from fluid_simulation_amd import shapes
    W = H = D = 128
    sim = F.Simulation(W, H, D, 1, quiet=1)
    sphere = shapes.write_binary_stl(str(tmp_path / "sphere.stl"), shapes.sphere_triangles(2.0, 48, 24))
    plate = shapes.write_binary_stl(str(tmp_path / "plate.stl"), shapes.box_triangles(0.2, 2.4, 1.6))
    F.loadSTLIntoObstacles(sphere, sim, 0.3, 0.0, 0.0, 0.0, -W / 4.0, 0.0, 0.0)
    F.loadSTLIntoObstacles(plate, sim, 0.45, 0.0, 0.0, 0.0, W / 8.0, 0.0, 0.0)
    return sim


@pytest.mark.parametrize("case", ["ball fp32", "ball fp64", "long row", "stl"])
def test_obstacle_mesh_is_byte_identical_through_either_entry_point(F, tmp_path, case):
    if case == "stl":
        sim = stl_mask_sim(F, tmp_path)
    else:
        W, H, D, r = (300, 20, 18, 7.5) if case == "long row" else (33, 31, 29, 12.3) if case == "ball fp64" else (40, 30, 24, 8.0)
        sim = F.Simulation(W, H, D, 1, quiet=1, precision="fp64" if case == "ball fp64" else "fp32")
        sim.set_mask(ball_mask(W, H, D, W / 3.0, H / 2.0, D / 2.0, r))
    assert sim.get(F.OBS).sum() > 0
    verts, faces = sim.obstacle_surface()
    iv, it = sim.isosurface(F.OBS, 0.5)
    assert len(verts) > 0 and verts.tobytes() == iv.tobytes() and faces.tobytes() == it.tobytes()
    frac = verts - np.floor(verts)
    assert np.all((frac == 0.0) | (frac == 0.5))                          # the midpoints, as before
    sim.close()


def test_the_two_result_slots_are_independent(F):
    W, H, D = 20, 14, 10
    sim = F.Simulation(W, H, D, 1, quiet=1)
    sim.set(F.DENS, bump(W, H, D).astype(np.float32))
    sim.set_mask(ball_mask(W, H, D, 6, 7, 5, 2.5))
    iv, it = sim.isosurface(F.DENS, 0.35)
    ov, ot = sim.obstacle_surface()                                       # computed after: must not replace the iso slot
    assert len(iv) != len(ov)
    iv2, it2 = np.zeros_like(iv), np.zeros_like(it)
    assert sim._L.fs_isosurface_fetch(sim._h, iv2.ctypes.data, it2.ctypes.data) == 0
    assert np.array_equal(iv, iv2) and np.array_equal(it, it2)
    sim.isosurface(F.DENS, 0.6)                                           # and the reverse
    ov2, ot2 = np.zeros_like(ov), np.zeros_like(ot)
    assert sim._L.fs_obstacle_surface_fetch(sim._h, ov2.ctypes.data, ot2.ctypes.data) == 0
    assert np.array_equal(ov, ov2) and np.array_equal(ot, ot2)
    nv, nt = C.c_long(), C.c_long()
    assert sim._L.fs_isosurface(sim._h, F.DENS, 0.35, C.byref(nv), C.byref(nt)) == 0
    assert (nv.value, nt.value) == (len(iv), len(it))
    sim.close()


def test_slab_handles_refuse(F):
    sim = F.Simulation(8, 8, 8, 1, quiet=1)
    sim.comm_init(0, 2, b"FSNULL:".ljust(128, b"\0"))
    for source in (F.OBS, F.DENS, F.ISO_VORTEX | F.VORTEX_Q):
        with pytest.raises(F.FluidsimError) as e:
            sim.isosurface(source, 0.5)
        assert e.value.code == F._lib.EINVAL
    sim.close()
