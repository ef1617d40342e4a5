"""The vortex-identification fields and the iso-surface vertices of include/fluidsim.h ("vortex identification") restated
in numpy, one rounded operation per numpy call, written from the header's formulas (not from the kernels).  Shared by
tests/test_vortex_cpu.py, tests/test_gpu_vortex.py and tests/test_gpu_isosurface.py."""
import numpy as np

WX, WY, WZ, W2, Q = range(5)
HALF = np.float64(0.5)


def from_differences(d):
    """d[a][b] = D_b a in fp64 (a: u, v, w; b: x, y, z) -> [WX, WY, WZ, W2, Q] in fp64."""
    (uxx, uxy, uxz), (vyx, vyy, vyz), (wzx, wzy, wzz) = d      # named g-wise below: g_ab = 0.5 * D_b a
    wx = HALF * (wzy - vyz)
    wy = HALF * (uxz - wzx)
    wz = HALF * (vyx - uxy)
    w2 = (wx * wx + wy * wy) + wz * wz
    gxx, gxy, gxz = HALF * uxx, HALF * uxy, HALF * uxz
    gyx, gyy, gyz = HALF * vyx, HALF * vyy, HALF * vyz
    gzx, gzy, gzz = HALF * wzx, HALF * wzy, HALF * wzz
    diag = (gxx * gxx + gyy * gyy) + gzz * gzz
    off = (gxy * gyx + gxz * gzx) + gyz * gzy
    q = np.float64(-0.5) * diag - off
    return [wx, wy, wz, w2, q]


def from_stencils(nb):
    """nb: (..., 18) values in the order u_xp u_xm u_yp u_ym u_zp u_zm, then v, then w -> five fp64 arrays."""
    n = np.asarray(nb).astype(np.float64)
    d = [[n[..., 6 * a + 2 * b] - n[..., 6 * a + 2 * b + 1] for b in range(3)] for a in range(3)]
    return from_differences(d)


def fields(u, v, w, obs):
    """Padded (z, y, x) arrays as fs_get_field returns them -> the five padded fp64 fields: the formula in target cells
    (interior, obs != 1), +0.0 everywhere else."""
    f = [np.asarray(a).astype(np.float64) for a in (u, v, w)]
    c = slice(1, -1)
    d = [[a[c, c, 2:] - a[c, c, :-2], a[c, 2:, c] - a[c, :-2, c], a[2:, c, c] - a[:-2, c, c]] for a in f]
    target = np.asarray(obs)[c, c, c] != 1
    out = []
    with np.errstate(all="ignore"):
        for val in from_differences(d):
            full = np.zeros(f[0].shape, dtype=np.float64)
            full[c, c, c] = np.where(target, val, np.float64(0.0))
            out.append(full)
    return out


def iso_vertices(field, level):
    """The vertices of the iso-surface {field > level} of a padded (z, y, x) array in the handle's precision (the array's
    dtype): one per grid edge whose end points lie on different sides, at (float32)coord + (float32)t along the edge's
    axis, t = (L - v0) / (v1 - v0) in that precision, 0.5 where the DEGENERATE rule of include/fluidsim.h says so -- the
    definition of tests/surface_model.py, which this calls.  Returns (n, 3) float32 rows (x, y, z), sorted, and for each
    the unit step from the inside end to the outside end."""
    import surface_model as S
    a = np.asarray(field)
    rows, _ = S.mesh(a, level)
    own = S.vertex_owners(a, level)
    assert len(own) == len(rows)
    outward = np.zeros((len(rows), 3))
    outward[np.arange(len(rows)), own[:, 3]] = np.where(S.inside_of(a, level)[own[:, 2], own[:, 1], own[:, 0]], 1.0, -1.0)
    order = np.lexsort((rows[:, 2], rows[:, 1], rows[:, 0]))
    return rows[order], outward[order]


def sorted_rows(verts):
    v = np.asarray(verts, dtype=np.float32)
    return v[np.lexsort((v[:, 2], v[:, 1], v[:, 0]))]
