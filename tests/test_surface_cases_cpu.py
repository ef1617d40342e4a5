"""The iso-surface cases of tests/surface_cases.py judged on the model alone (tests/surface_model.py): no GPU.  Every
case must give a well-formed mesh (one finite vertex per crossing edge, on its edge; every vertex used; closed, or open
only along the padded box's faces), every "reaches" entry is counted and must occur at least FLOOR times, the cases
together must meet all 256 cube configurations, the DEGENERATE rule of include/fluidsim.h must matter where it is claimed
to (NaN vertices without it, the same faces either way), and the vectorised model must equal a plain triple loop written
from the header's text, byte for byte."""
import functools

import numpy as np
import pytest

import surface_cases as SC
import surface_model as M

FLOOR = 4
CASES = SC.cases()


@functools.lru_cache(maxsize=None)
def model(name):
    c = SC.by_name(name)
    verts, faces = M.mesh(c.array, c.level)
    verts.setflags(write=False)
    faces.setflags(write=False)
    return verts, faces


def crossing_edges(c):
    """per axis: (xx, yy, zz, v0, v1) of the crossing edges, v0 at the owning point"""
    cross = M.crossings(M.inside_of(c.array, c.level))
    out = []
    for axis in range(3):
        zz, yy, xx = np.nonzero(cross[axis])
        hi = [zz, yy, xx]
        hi[2 - axis] = hi[2 - axis] + 1
        out.append((xx, yy, zz, c.array[zz, yy, xx], c.array[tuple(hi)]))
    return out


def all_edge_values(c):
    e = crossing_edges(c)
    return np.concatenate([a[3] for a in e]), np.concatenate([a[4] for a in e])


def on_box_face(c, own):
    """for vertices given by their owners (x, y, z, axis): (n, 6) bools, vertex lies in the box face (axis k, low / high)"""
    W, H, D = c.shape
    hi = (W + 1, H + 1, D + 1)
    cols = []
    for k in range(3):
        for side in (0, hi[k]):
            cols.append((own[:, k] == side) & (own[:, 3] != k))
    return np.stack(cols, axis=1)


@pytest.mark.parametrize("name", SC.ids())
def test_every_case_gives_a_well_formed_mesh(name):
    c = SC.by_name(name)
    verts, faces = model(name)
    assert verts.dtype == np.float32 and faces.dtype == np.int32 and verts.shape[1:] == (3,) and faces.shape[1:] == (3,)
    assert c.array.dtype == SC.DTYPES[c.precision] and c.array.shape == SC._padded(c.shape)
    inside = M.inside_of(c.array, c.level)
    n_cross = int(sum(x.sum() for x in M.crossings(inside)))
    kinds = [r for r in c.reaches if r in ("closed", "open", "empty")]
    assert len(kinds) == 1
    if kinds[0] == "empty":
        assert n_cross == 0 and verts.shape == (0, 3) and faces.shape == (0, 3)
        return
    nv = len(verts)
    assert nv == n_cross and nv > 0
    assert np.all(np.isfinite(verts))
    own = M.vertex_owners(c.array, c.level)
    assert len(own) == nv
    lo = own[:, :3].astype(np.float32)
    along = np.zeros((nv, 3), dtype=bool)
    along[np.arange(nv), own[:, 3]] = True
    assert np.all(np.where(along, (verts >= lo) & (verts <= lo + np.float32(1.0)), verts == lo))   # on its own edge
    assert faces.min() >= 0 and faces.max() < nv
    assert len(np.unique(faces)) == nv                                    # every vertex is used
    assert np.all(faces[:, 0] != faces[:, 1]) and np.all(faces[:, 1] != faces[:, 2]) and np.all(faces[:, 2] != faces[:, 0])
    if kinds[0] == "closed":
        assert M.is_closed(faces, nv)
        assert M.euler_number(nv, faces) % 2 == 0
    else:
        b = M.boundary_edges(faces, nv)                                   # asserts: no directed edge twice
        assert len(b) >= (FLOOR if min(c.shape) > 1 else 1) and not M.is_closed(faces, nv)
        face_a, face_b = on_box_face(c, own[b[:, 0]]), on_box_face(c, own[b[:, 1]])
        assert np.all((face_a & face_b).any(axis=1))                      # both ends in one face of the padded box


def test_the_cases_together_meet_all_256_cube_configurations():
    seen = np.zeros(256, dtype=np.int64)
    for c in CASES:
        seen += np.bincount(M.cube_configs(M.inside_of(c.array, c.level)).ravel(), minlength=256)
    assert np.all(seen > 0), np.flatnonzero(seen == 0)


def test_the_case_table_is_the_recorded_one():
    """The model reads the table through fs_surface_case_table, so a change of the host table that still triangulates
    every cube would move the device and the model together.  "Table order" is part of the contract: the 256 cases as
    the library built them when the order was pinned (tests/golden/surface_case_table.npz; tests/test_surface_table.py
    judges their geometry)."""
    from conftest import load_golden
    _, g = load_golden("surface_case_table")
    ntri, edges = M.table()
    assert np.array_equal(g["ntri"], ntri) and np.array_equal(g["edges"], edges)
    assert int(ntri.sum()) > 256 and ntri.max() <= 5 and edges.max() == 11
    for cfg in range(256):
        assert np.all(edges[cfg, ntri[cfg]:] == 0)


# ---- one counting function per "reaches" entry: each returns {what: count}, every count must reach FLOOR -------------

def reach_x_chunks(c):
    W = c.shape[0]
    own = M.vertex_owners(c.array, c.level)
    cubes = M.triangle_cubes(c.array, c.level)
    n = {}
    for k in range(3):
        n["vertices in x-chunk %d" % k] = int((own[:, 0] // 256 == k).sum())
        n["triangles in x-chunk %d" % k] = int((cubes[:, 0] // 256 == k).sum())
    for x in (255, 256, 511, W):
        n["x edge %d-%d" % (x, x + 1)] = int(((own[:, 0] == x) & (own[:, 3] == 0)).sum())
        n["triangles of the cubes at x = %d" % x] = int((cubes[:, 0] == x).sum())
    for x in (255, 256, 257, 511, 512, W, W + 1):
        for axis in (1, 2):
            n["%s edges at x = %d" % ("xyz"[axis], x)] = int(((own[:, 0] == x) & (own[:, 3] == axis)).sum())
    # rows that have something in all three chunks: the carry is per row
    ny = c.shape[1] + 2
    for what, rows, xs in (("vertices", own[:, 2] * ny + own[:, 1], own[:, 0]), ("triangles", cubes[:, 2] * ny + cubes[:, 1], cubes[:, 0])):
        full = 0
        for r in np.unique(rows):
            full += len(np.unique(xs[rows == r] // 256)) == 3
        n["rows with %s in all three chunks" % what] = full
    return n


def reach_x_chunks_mask(c):
    own = M.vertex_owners(c.array, c.level)
    cubes = M.triangle_cubes(c.array, c.level)
    n = {}
    for k in range(3):
        n["vertices in x-chunk %d" % k] = int((own[:, 0] // 256 == k).sum())
        n["triangles in x-chunk %d" % k] = int((cubes[:, 0] // 256 == k).sum())
    for x in (255, 256, 511, 512):
        n["triangles of the cubes at x = %d" % x] = int((cubes[:, 0] == x).sum())
    return n


def reach_row_chunks(c):
    W, H, D = c.shape
    nrows = (H + 2) * (D + 2)
    assert nrows > 2 * 256
    own = M.vertex_owners(c.array, c.level)
    cubes = M.triangle_cubes(c.array, c.level)
    vrow, trow = own[:, 2] * (H + 2) + own[:, 1], cubes[:, 2] * (H + 2) + cubes[:, 1]
    n = {}
    for k in range(3):
        n["vertices in row-chunk %d" % k] = int((vrow // 256 == k).sum())
        n["triangles in row-chunk %d" % k] = int((trow // 256 == k).sum())
    n["vertices in the first row"] = int((vrow == 0).sum())
    n["vertices in the last row"] = int((vrow == nrows - 1).sum())
    n["triangles in the first row of cubes"] = int((trow == 0).sum())
    n["triangles in the last row of cubes"] = int((trow == D * (H + 2) + H).sum())
    return n


def reach_ties(c):
    L = c.array.dtype.type(c.level)
    v0, v1 = all_edge_values(c)
    verts, faces = model(c.name)
    _, inverse, counts = np.unique(verts, axis=0, return_inverse=True, return_counts=True)
    shared = counts[inverse.ravel()] > 1
    p = verts[faces]
    flat = (p[:, 0] == p[:, 1]).all(axis=1) | (p[:, 1] == p[:, 2]).all(axis=1) | (p[:, 2] == p[:, 0]).all(axis=1)
    frac = verts - np.floor(verts)
    return {"edges whose owning end equals the level (t = 0)": int((v0 == L).sum()),
            "edges whose far end equals the level (t = 1)": int((v1 == L).sum()),
            "vertices on a grid point": int((frac == 0).all(axis=1).sum()),
            "vertices sharing a position": int(shared.sum()),
            "zero-area triangles": int(flat.sum())}


def reach_level_rounding(c):
    assert c.array.dtype == np.float32
    L = np.float32(c.level)
    assert float(L) != c.level
    inside = M.inside_of(c.array, c.level)
    in_double = c.array.astype(np.float64) > c.level
    v0, v1 = all_edge_values(c)
    assert not inside[c.array == L].any()
    differs = int(sum(x.sum() for x in M.crossings(in_double))) - int(sum(x.sum() for x in M.crossings(inside)))
    return {"cells equal to float32(level), inside for a comparison in double": int((in_double & ~inside).sum()),
            "crossing edges with such an end point": int(((v0 == L) | (v1 == L)).sum()),
            "difference in the number of crossing edges": abs(differs)}


def reach_nonfinite(c):
    L = c.array.dtype.type(c.level)
    v0, v1 = all_edge_values(c)
    with np.errstate(invalid="ignore"):
        def pairs(p, q):
            return int(((p(v0) & q(v1)) | (p(v1) & q(v0))).sum())
        inside = lambda v: v > L                                          # noqa: E731
        finite_in = lambda v: np.isfinite(v) & (v > L)                    # noqa: E731
        finite_out = lambda v: np.isfinite(v) & ~(v > L)                  # noqa: E731
        assert inside(np.array([np.inf]))[0]
        return {"NaN beside inside": pairs(np.isnan, finite_in),
                "-Inf beside inside": pairs(np.isneginf, finite_in),
                "+Inf beside outside": pairs(np.isposinf, finite_out),
                "+Inf beside -Inf": pairs(np.isposinf, np.isneginf),
                "+Inf beside NaN": pairs(np.isposinf, np.isnan)}


def reach_overflow(c):
    L = c.array.dtype.type(c.level)
    v0, v1 = all_edge_values(c)
    with np.errstate(all="ignore"):
        num, den = L - v0, v1 - v0
        t = num / den
    assert np.all(np.isfinite(v0)) and np.all(np.isfinite(v1))
    n = {"edges whose v1 - v0 alone overflows: t = 0": int((np.isfinite(num) & np.isinf(den) & (t == 0)).sum())}
    if c.level != 0.0:
        n["edges whose L - v0 and v1 - v0 both overflow: t = NaN"] = int((np.isinf(num) & np.isinf(den) & np.isnan(t)).sum())
    return n


def reach_subnormal(c):
    tiny = np.finfo(c.array.dtype).tiny
    v0, v1 = all_edge_values(c)
    sub = lambda v: (v != 0) & (np.abs(v) < tiny)                         # noqa: E731
    verts, _ = model(c.name)
    frac = verts - np.floor(verts)
    return {"crossing edges with a subnormal end point": int((sub(v0) | sub(v1)).sum()),
            "crossing edges with a subnormal v1 - v0": int(sub(v1 - v0).sum()),
            "vertices strictly inside their edge": int(((frac > 0) & (frac < 1)).any(axis=1).sum())}


def reach_signed_zero(c):
    v0, v1 = all_edge_values(c)
    pos = lambda v: (v == 0) & ~np.signbit(v)                             # noqa: E731
    neg = lambda v: (v == 0) & np.signbit(v)                              # noqa: E731
    inside = M.inside_of(c.array, c.level)
    assert not inside[c.array == 0].any()                                 # +-0.0 > +-0.0 is false
    return {"crossing edges with a +0.0 end point": int((pos(v0) | pos(v1)).sum()),
            "crossing edges with a -0.0 end point": int((neg(v0) | neg(v1)).sum())}


def reach_mask(c):
    assert np.all((c.array == 0) | (c.array == 1)) and c.level == 0.5
    verts, _ = model(c.name)
    frac = verts - np.floor(verts)
    assert np.all((frac == 0.0) | (frac == 0.5)) and np.all((frac == 0.5).sum(axis=1) == 1)
    return {"midpoint vertices": len(verts)}


REACH = {"x-chunks": reach_x_chunks, "x-chunks-mask": reach_x_chunks_mask, "row-chunks": reach_row_chunks, "ties": reach_ties,
         "level-rounding": reach_level_rounding, "nonfinite": reach_nonfinite, "overflow": reach_overflow,
         "subnormal": reach_subnormal, "signed-zero": reach_signed_zero, "mask": reach_mask}


@pytest.mark.parametrize("name", SC.ids())
def test_every_case_reaches_what_it_claims(name):
    c = SC.by_name(name)
    for r in c.reaches:
        if r in ("closed", "open", "empty"):
            continue                                                      # judged with the mesh above
        counts = REACH[r](c)
        assert counts and min(counts.values()) >= FLOOR, (r, counts)


def test_every_reaches_entry_is_claimed_by_some_case():
    claimed = {r for c in CASES for r in c.reaches}
    assert claimed == set(REACH) | {"closed", "open", "empty"}
    assert {c.source for c in CASES} == {"DENS", "OBS"} and {c.precision for c in CASES} == {"fp32", "fp64"}


@pytest.mark.parametrize("name", [n for n in SC.ids() if n.startswith(("non-finite", "overflow at 2e38"))])
def test_the_degenerate_rule_matters_and_leaves_the_faces_alone(name):
    c = SC.by_name(name)
    verts, faces = model(name)
    raw_verts, raw_faces = M.mesh(c.array, c.level, degenerate=False)
    assert np.all(np.isfinite(verts))
    bad = ~np.isfinite(raw_verts).all(axis=1)
    assert bad.sum() >= FLOOR                                             # what the kernel wrote before the rule
    assert np.isnan(raw_verts[bad]).any()
    assert raw_faces.tobytes() == faces.tobytes()
    ok = ~bad
    in_range = ok & (raw_verts >= np.floor(raw_verts)).all(axis=1)
    assert raw_verts[in_range & (raw_verts == verts).all(axis=1)].shape[0] >= FLOOR   # sound edges are left as they were
    frac = verts[bad] - np.floor(verts[bad])
    assert np.all((frac == 0.5).sum(axis=1) == 1)                         # the rule puts them at the midpoint


# ---- the model against a plain loop, written from the ORDER and DEGENERATE text of include/fluidsim.h ----------------

def loop_mesh(a, level):
    T = a.dtype.type
    L = T(level)
    nz, ny, nx = a.shape
    ntri, edges = M.table()

    def inside(x, y, z):
        with np.errstate(invalid="ignore"):
            return bool(a[z, y, x] > L)

    verts, index = [], {}
    for z in range(nz):
        for y in range(ny):
            for x in range(nx):
                for axis in range(3):
                    q = [x, y, z]
                    q[axis] += 1
                    if q[0] >= nx or q[1] >= ny or q[2] >= nz or inside(x, y, z) == inside(*q):
                        continue
                    v0, v1 = a[z, y, x], a[q[2], q[1], q[0]]
                    with np.errstate(all="ignore"):
                        t = (L - v0) / (v1 - v0)
                    assert type(t) is T
                    if not (np.isfinite(v0) and np.isfinite(v1)) or not (t >= 0 and t <= 1):
                        t = T(0.5)
                    p = [np.float32(x), np.float32(y), np.float32(z)]
                    p[axis] = p[axis] + np.float32(t)
                    index[(x, y, z, axis)] = len(verts)
                    verts.append(p)
    faces = []
    for z in range(nz - 1):
        for y in range(ny - 1):
            for x in range(nx - 1):
                cfg = 0
                for i in range(8):
                    cfg |= int(inside(x + (i & 1), y + ((i >> 1) & 1), z + ((i >> 2) & 1))) << i
                for k in range(int(ntri[cfg])):
                    tri = []
                    for e in edges[cfg, k]:
                        axis, ov, ou = int(e) >> 2, (int(e) >> 1) & 1, int(e) & 1
                        lower, higher = [j for j in range(3) if j != axis]
                        p = [x, y, z]
                        p[lower] += ou
                        p[higher] += ov
                        tri.append(index[(p[0], p[1], p[2], axis)])
                    faces.append(tri)
    return np.array(verts, dtype=np.float32).reshape(-1, 3), np.array(faces, dtype=np.int32).reshape(-1, 3)


@pytest.mark.parametrize("which", ["noise fp32", "non-finite fp64", "ties fp32"])
def test_the_model_equals_a_plain_triple_loop(which):
    if which == "noise fp32":
        a, level = SC._noise((7, 6, 5), 31).astype(np.float32), 0.5
    elif which == "non-finite fp64":
        a, level = SC._nonfinite((8, 7, 6), 32), 0.5
        assert np.isnan(a).sum() >= FLOOR and np.isinf(a).sum() >= FLOOR
    else:
        a, level = SC._ties((6, 5, 4), 33).astype(np.float32), 0.5
    verts, faces = M.mesh(a, level)
    lv, lf = loop_mesh(a, level)
    assert len(verts) > 100 and len(faces) > 100
    assert verts.tobytes() == lv.tobytes() and faces.tobytes() == lf.tobytes()


def test_vortex_model_iso_vertices_is_the_same_definition():
    import vortex_model as V
    c = SC.by_name("non-finite fp32")
    verts, _ = model(c.name)
    rows, outward = V.iso_vertices(c.array, c.level)
    assert np.all(np.isfinite(rows))
    order = np.lexsort((verts[:, 2], verts[:, 1], verts[:, 0]))
    assert rows.tobytes() == verts[order].tobytes()
    assert outward.shape == (len(verts), 3) and np.all(np.abs(outward).sum(axis=1) == 1)
