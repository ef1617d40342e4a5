"""Vorticity confinement as include/fluidsim.h defines it ("vorticity confinement"), restated in numpy with one rounded
operation per numpy call, written from the header's text (not from the kernel).  Shared by tests/test_confine_cpu.py and
tests/test_gpu_confine.py."""
import numpy as np

HALF = np.float64(0.5)


def curl(u, v, w):
    """Padded (z, y, x) arrays -> (WX, WY, WZ) of every interior cell in fp64, cell units."""
    u, v, w = (np.asarray(a).astype(np.float64) for a in (u, v, w))
    c = slice(1, -1)

    def dx(a):
        return a[c, c, 2:] - a[c, c, :-2]

    def dy(a):
        return a[c, 2:, c] - a[c, :-2, c]

    def dz(a):
        return a[2:, c, c] - a[:-2, c, c]

    wx = HALF * (dy(w) - dz(v))
    wy = HALF * (dz(u) - dx(w))
    wz = HALF * (dx(v) - dy(u))
    return wx, wy, wz


def magnitude(wx, wy, wz):
    return np.sqrt((wx * wx + wy * wy) + wz * wz)


def force(wx, wy, wz, m, mn, bits):
    """omega and m of cells, mn = their six neighbour magnitudes (xp, xm, yp, ym, zp, zm), bits = six booleans "that
    neighbour is a target cell" -> (fx, fy, fz, on); f is meaningless where on is False."""
    val = [np.where(b, n, m) for n, b in zip(mn, bits)]
    ex = HALF * (val[0] - val[1])
    ey = HALF * (val[2] - val[3])
    ez = HALF * (val[4] - val[5])
    e2 = (ex * ex + ey * ey) + ez * ez
    on = e2 > 0
    length = np.sqrt(e2)
    nx, ny, nz = ex / length, ey / length, ez / length
    fx = ny * wz - nz * wy
    fy = nz * wx - nx * wz
    fz = nx * wy - ny * wx
    return fx, fy, fz, on


def apply(v, k, f):
    """v' = (T)((double)v + k * f), T = v's dtype"""
    v = np.asarray(v)
    return (v.astype(np.float64) + np.float64(k) * f).astype(v.dtype)


def confine(u, v, w, obs, k):
    """One pass WITHOUT the boundary enforcement: padded (z, y, x) arrays of one dtype -> the three new padded arrays, in
    which every target cell that is not degenerate holds its updated value and every other cell what it held.  k = the
    fp64 product (double)dt * eps."""
    u, v, w = (np.asarray(a) for a in (u, v, w))
    obs = np.asarray(obs)
    c = slice(1, -1)
    interior = np.zeros(u.shape, dtype=bool)
    interior[c, c, c] = True
    target = interior & (obs != 1)
    fluid = interior & (obs == 0)                            # what a cell's flag byte says of its neighbours
    with np.errstate(all="ignore"):
        wx, wy, wz = curl(u, v, w)
        m = np.full(u.shape, np.nan)
        m[c, c, c] = np.where(target[c, c, c], magnitude(wx, wy, wz), np.nan)
        sh = [(c, c, slice(2, None)), (c, c, slice(0, -2)), (c, slice(2, None), c), (c, slice(0, -2), c),
              (slice(2, None), c, c), (slice(0, -2), c, c)]
        fx, fy, fz, on = force(wx, wy, wz, m[c, c, c], [m[s] for s in sh], [fluid[s] for s in sh])
        do = target[c, c, c] & on
        out = []
        for a, f in ((u, fx), (v, fy), (w, fz)):
            r = a.copy()
            r[c, c, c] = np.where(do, apply(a[c, c, c], k, f), a[c, c, c])
            out.append(r)
    return out



# ---- fields whose result is known, shared by the host and the device tests ---------------------------------------------

def grid(W, H, D):
    z, y, x = np.mgrid[0:D + 2, 0:H + 2, 0:W + 2]
    return x.astype(np.float64), y.astype(np.float64), z.astype(np.float64)


def hand_field(which, dtype, W=7, H=6, D=5, a=3.0):
    """u = a y^2, v = a z^2 or w = a x^2, analytic in the ghosts too; -> (u, v, w, component index, coordinate)"""
    x, y, z = grid(W, H, D)
    f = [np.zeros(x.shape, dtype=dtype) for _ in range(3)]
    coord = (y, z, x)[which]
    f[which] = (a * coord * coord).astype(dtype)
    return f[0], f[1], f[2], which, coord


def lamb_oseen(dtype, W=32, H=32, D=5):
    x, y, z = grid(W, H, D)
    rx, ry = x - 16.5, y - 16.5
    r2 = rx * rx + ry * ry
    q = 8.0 * (1.0 - np.exp(-r2 / 25.0)) / r2
    return (-ry * q).astype(dtype), (rx * q).astype(dtype), np.zeros(x.shape, dtype=dtype), rx, ry, r2


def check_co_rotation(u, v, w, out, rx, ry, r2):
    """The increment spins the vortex up: tangential part > 0, radial part at most a quarter of it, w untouched."""
    c = slice(1, -1)
    du = out[0].astype(np.float64) - u.astype(np.float64)
    dv = out[1].astype(np.float64) - v.astype(np.float64)
    r = np.sqrt(r2)
    tang = (-ry * du + rx * dv) / r
    rad = (rx * du + ry * dv) / r
    ring = np.zeros(r2.shape, dtype=bool)
    ring[c, c, c] = ((r2 > 2) & (r2 < 144))[c, c, c]
    assert ring.sum() > 1000
    assert (tang[ring] > 0).all(), float(tang[ring].min())
    assert (np.abs(rad[ring]) <= 0.25 * tang[ring]).all(), float((np.abs(rad[ring]) / tang[ring]).max())
    assert np.array_equal(out[2].view(np.uint8), w.view(np.uint8))
    return float(tang[ring].min()), float((np.abs(rad[ring]) / tang[ring]).max())
