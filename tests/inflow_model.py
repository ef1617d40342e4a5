"""The turbulent inflow of include/fluidsim.h ("turbulent inflow") restated in numpy, from the header's text and not from the
kernels: the hash in uint64 (exact, wrapping), everything else in float64 with one rounded operation per numpy call, sums
in ascending k.  eddies(params, t), plane(params, U, r, gust, t) and cast() are what the tests compare the library with."""
import numpy as np

U64 = np.uint64
G = U64(0x9E3779B97F4A7C15)
M1 = U64(0xBF58476D1CE4E5B9)
M2 = U64(0x94D049BB133111EB)
TENT_K = np.float64(1.2247448713915890)      # sqrt(3/2), correctly rounded
assert TENT_K == np.sqrt(np.float64(1.5))


class Params:
    """seed, N eddies, the plane h x d, sigma, convection c (cells per step), u_rms"""

    def __init__(self, seed, n, h, d, sigma, convect, u_rms):
        self.seed, self.n, self.h, self.d = int(seed) & (2 ** 64 - 1), int(n), int(h), int(d)
        self.sigma, self.convect, self.u_rms = np.float64(sigma), np.float64(convect), np.float64(u_rms)

    def extent(self, cells):
        return np.float64(cells - 1) + np.float64(2.0) * self.sigma

    @property
    def amp(self):
        if self.n <= 0:
            return np.float64(0.0)
        vol = ((np.float64(2.0) * self.sigma) * self.extent(self.h)) * self.extent(self.d)
        den = np.float64(self.n) * ((self.sigma * self.sigma) * self.sigma)
        return self.u_rms * np.sqrt(vol / den)


def auto_convect(dt, width, speed):
    """the default convection: ((double)dt * (double)width) * (double)speed, dt the handle's float"""
    return (np.float64(np.float32(dt)) * np.float64(width)) * np.float64(speed)


def mix(z):
    with np.errstate(over="ignore"):
        z = (z ^ (z >> U64(30))) * M1
        z = (z ^ (z >> U64(27))) * M2
        return z ^ (z >> U64(31))


def hash64(seed, k, gen, draw):
    """HASH(seed, k, gen, draw) over arrays of uint64 (k, gen) and scalars (seed, draw)"""
    k = np.asarray(k, dtype=U64)
    gen = np.asarray(gen, dtype=U64)
    with np.errstate(over="ignore"):
        a = mix(U64(seed) + G * (k + U64(1)))
        b = mix(a + G * gen)
        return mix(b + G * U64(draw + 1))


def uniform(h):
    return (h >> U64(11)).astype(np.float64) * np.float64(2.0 ** -53)


def eddies(p, t):
    """dict of arrays over k = 0 .. N-1 at step t: ex, ey, ez, gen (float64 whole numbers), sign (N, 3) of -1.0 / +1.0; with
    an array of steps of shape (S,) every array gains a leading axis S"""
    k = np.arange(p.n, dtype=U64)
    two = np.float64(2.0) * p.sigma
    u0 = uniform(hash64(p.seed, k, np.zeros(p.n, dtype=U64), 0))
    start = u0 * two
    moved = np.asarray(t, dtype=np.float64)[..., None] * p.convect
    s = start + moved
    q = s / two
    gen = np.floor(q)
    base = gen * two
    rem = s - base
    rem = np.where(rem < 0.0, np.float64(0.0), rem)
    over = ~(rem < two)
    rem = np.where(over, np.float64(0.0), rem)
    gen = np.where(over, gen + np.float64(1.0), gen)
    gi = gen.astype(U64)
    low = np.float64(1.0) - p.sigma
    ex = low + rem
    ey = low + uniform(hash64(p.seed, k, gi, 1)) * p.extent(p.h)
    ez = low + uniform(hash64(p.seed, k, gi, 2)) * p.extent(p.d)
    sign = np.stack([np.where((hash64(p.seed, k, gi, 3 + j) >> U64(63)) != 0, -1.0, 1.0) for j in range(3)], axis=-1)
    return {"ex": ex, "ey": ey, "ez": ez, "gen": gen, "sign": sign}


def tent(rho):
    a = np.float64(1.0) - np.abs(rho)
    return TENT_K * np.where(a > 0.0, a, np.float64(0.0))


def fluctuation_at(p, t, ys, zs, chunk=1 << 21):
    """u' (3, m) float64 at the cells (ys[i], zs[i]) at step t: per cell the sum over the eddies in ascending k from +0.0
    (np.cumsum adds strictly one after the other)"""
    ys = np.asarray(ys, dtype=np.float64).reshape(-1)
    zs = np.asarray(zs, dtype=np.float64).reshape(-1)
    u = np.zeros((3, ys.size))
    if p.n <= 0:
        return u
    e = eddies(p, t)
    inv = np.float64(1.0) / p.sigma
    ax = p.amp * tent((np.float64(1.0) - e["ex"]) * inv)
    m = max(1, chunk // p.n)
    for lo in range(0, ys.size, m):
        y, z = ys[None, lo:lo + m], zs[None, lo:lo + m]
        fy = tent((y - e["ey"][:, None]) * inv)
        fz = tent((z - e["ez"][:, None]) * inv)
        w = (ax[:, None] * fy) * fz
        for j in range(3):
            terms = np.concatenate([np.zeros((1, w.shape[1])), e["sign"][:, j, None] * w], axis=0)
            u[j, lo:lo + m] = np.cumsum(terms, axis=0)[-1]
    return u


def fluctuation(p, t):
    """u' (3, d, h) float64 at every inlet cell"""
    z, y = np.mgrid[1:p.d + 1, 1:p.h + 1]
    return fluctuation_at(p, t, y, z).reshape(3, p.d, p.h)


def gust_factor(gust, t):
    """g(t) of a schedule [(step, factor), ...] or None"""
    if gust is None or len(gust) == 0:
        return np.float64(1.0)
    ts = np.array([g[0] for g in gust], dtype=np.float64)
    fs = np.array([g[1] for g in gust], dtype=np.float64)
    x = np.float64(t)
    if x <= ts[0]:
        return fs[0]
    if x >= ts[-1]:
        return fs[-1]
    i = int(np.searchsorted(ts, x, side="right")) - 1   # ts[i] <= x < ts[i + 1]
    frac = (x - ts[i]) / (ts[i + 1] - ts[i])
    return fs[i] + (fs[i + 1] - fs[i]) * frac


def plane(p, U, r, gust, t, speed=0):
    """the three fp64 components (3, d, h) of the inlet plane at step t before the rounding to the field type; U and r are
    (d, h) maps or None (speed everywhere / 1 everywhere)"""
    u = fluctuation(p, t)
    mean = np.full((p.d, p.h), np.float64(speed)) if U is None else np.asarray(U, dtype=np.float64).reshape(p.d, p.h)
    scale = np.ones((p.d, p.h)) if r is None else np.asarray(r, dtype=np.float64).reshape(p.d, p.h)
    g = gust_factor(gust, t)
    out = np.empty((3, p.d, p.h))
    out[0] = g * mean + scale * u[0]
    out[1] = scale * u[1]
    out[2] = scale * u[2]
    return out


def cast(pl, dtype):
    """the one rounding to the field type"""
    with np.errstate(over="ignore"):
        return np.asarray(pl, dtype=np.float64).astype(dtype)
