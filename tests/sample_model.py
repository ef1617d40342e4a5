"""numpy fp64 restatement of the point sampler, written from the definition in include/fluidsim.h ("point probes and
field sampling"), not from csrc/sample.h.  numpy's elementwise fp64 operations are IEEE and are never contracted, so every
line below is one rounding, in the order the definition writes them; the tests compare bit patterns, with no tolerance.

`field` and `obs` are dense padded arrays shaped (D+2, H+2, W+2) as Simulation.get returns them (float32 or float64);
`points` is (n, 3) float64, x, y, z."""
import numpy as np

NEAREST, LINEAR, FLUID = 0, 1, 2
MODES = (NEAREST, LINEAR, FLUID)
MODE_NAMES = {NEAREST: "nearest", LINEAR: "linear", FLUID: "fluid"}


def _axis(x, n):
    """i0 = min(floor(x), N), s = x - i0, and whether x lies in [0, N + 1] (NaN: no)."""
    with np.errstate(invalid="ignore"):
        ok = (x >= 0.0) & (x <= np.float64(n + 1))
    xs = np.where(ok, x, 0.0)
    i0 = np.minimum(np.floor(xs).astype(np.int64), n)
    return i0, xs - i0.astype(np.float64), ok


def sample(field, obs, points, mode):
    field = np.asarray(field)
    d, h, w = (k - 2 for k in field.shape)
    p = np.asarray(points, dtype=np.float64).reshape(-1, 3)
    i0, sx, okx = _axis(p[:, 0], w)
    j0, sy, oky = _axis(p[:, 1], h)
    l0, sz, okz = _axis(p[:, 2], d)
    ok = okx & oky & okz
    tx, ty, tz = 1.0 - sx, 1.0 - sy, 1.0 - sz

    def v(a, b, c):
        return field[l0 + c, j0 + b, i0 + a].astype(np.float64)

    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        if mode == NEAREST:
            a, b, c = (sx >= 0.5).astype(np.int64), (sy >= 0.5).astype(np.int64), (sz >= 0.5).astype(np.int64)
            r = field[l0 + c, j0 + b, i0 + a].astype(np.float64)
        elif mode == LINEAR:
            cbc = {}
            for c in (0, 1):
                for b in (0, 1):
                    lo = v(0, b, c) * tx
                    hi = v(1, b, c) * sx
                    cbc[b, c] = lo + hi
            dc = {}
            for c in (0, 1):
                lo = cbc[0, c] * ty
                hi = cbc[1, c] * sy
                dc[c] = lo + hi
            lo = dc[0] * tz
            hi = dc[1] * sz
            r = lo + hi
        elif mode == FLUID:
            obs = np.asarray(obs)
            num = np.zeros(p.shape[0], dtype=np.float64)
            den = np.zeros(p.shape[0], dtype=np.float64)
            counted = np.zeros(p.shape[0], dtype=bool)
            for c in (0, 1):                                  # memory order: c outer, b, a inner
                for b in (0, 1):
                    for a in (0, 1):
                        wxy = (sx if a else tx) * (sy if b else ty)
                        wgt = wxy * (sz if c else tz)
                        counts = (wgt > 0.0) & (obs[l0 + c, j0 + b, i0 + a] != 1)
                        wv = wgt * v(a, b, c)
                        num = np.where(counts, num + wv, num)
                        den = np.where(counts, den + wgt, den)
                        counted |= counts
            r = np.where(counted, num / np.where(counted, den, 1.0), np.nan)
        else:
            raise ValueError("unknown mode %r" % (mode,))
    return np.where(ok, r, np.nan)


def same_bits(got, want):
    """Bit-for-bit equality of two float64 arrays, any NaN equal to any NaN (the definition says "NaN", not which)."""
    got = np.ascontiguousarray(got, dtype=np.float64)
    want = np.ascontiguousarray(want, dtype=np.float64)
    if got.shape != want.shape:
        return False
    nan = np.isnan(want)
    return bool(np.array_equal(np.isnan(got), nan) and
                np.array_equal(got.view(np.uint64)[~nan], want.view(np.uint64)[~nan]))


def special_points(w, h, d, rng, n_random=64):
    """Random points in the box plus the edge cases: exact integers, half-integers, 0 and N + 1 on every axis, values just
    outside the box, and NaN."""
    hi = np.array([w + 1, h + 1, d + 1], dtype=np.float64)
    pts = [rng.uniform(0.0, 1.0, size=(n_random, 3)) * hi]
    ints = np.stack([rng.integers(0, w + 2, 24), rng.integers(0, h + 2, 24), rng.integers(0, d + 2, 24)], axis=1).astype(np.float64)
    pts.append(ints)
    pts.append(np.minimum(ints + 0.5, hi))                                    # half-integers (clipped to the far face)
    pts.append(np.where(rng.integers(0, 2, size=(24, 3)) == 1, ints, np.minimum(ints + 0.5, hi)))   # mixed
    pts.append(np.array([[0.0, 0.0, 0.0], hi, [0.0, hi[1], 0.0], [hi[0], 0.0, hi[2]], [-0.0, 1.0, 1.0],
                         [w, h, d], [w + 0.5, h + 0.5, d + 0.5], [w + 0.25, 0.75, d + 1.0]]))
    inside = np.array([1.25, 1.5, 1.75])
    for k in range(3):
        for bad in (np.nextafter(0.0, -1.0), -1.0, np.nextafter(hi[k], np.inf), hi[k] + 1.0, np.nan, np.inf, -np.inf):
            q = inside.copy()
            q[k] = bad
            pts.append(q.reshape(1, 3))
    pts.append(np.array([[np.nan, np.nan, np.nan]]))
    return np.ascontiguousarray(np.concatenate(pts, axis=0), dtype=np.float64)
