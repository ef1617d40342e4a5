"""The flow monitor of include/fluidsim.h ("flow monitor") restated in numpy: the COLUMN, PLANE and WHOLE records and the
X-PROFILE of five padded fields and an obstacle array, every sum by elementwise fp64 additions in the header's order (rows in
increasing y, then columns in increasing x, then planes in increasing z), so that the kernels must return these bits.
`naive` is the same text as scalar loops, for tiny grids."""
import numpy as np

COLS = 16
PROFILE_COLS = 5
STATIONS_MAX = 8
LOG_COLS = 1 + COLS + STATIONS_MAX * PROFILE_COLS
# the COLUMN record's values, in the order used here
(C_CELLS, C_NONFINITE, C_Q, C_U, C_V, C_W, C_E, C_P, C_UU, C_QU, C_MAXU, C_MAXV, C_MAXW, C_MAXE, C_MINQ, C_MAXQ, C_MINP,
 C_MAXP, C_N) = range(19)
PLANE_FROM = [0, 1, 2, 3, 4, 5, 6, 7, C_MAXU, C_MAXV, C_MAXW, C_MAXE, C_MINQ, C_MAXQ, C_MINP, C_MAXP]
PROFILE_FROM = [C_CELLS, C_U, C_UU, C_P, C_QU]
# how a PLANE value combines: 0 a sum, +1 "if (a > m) m = a", -1 "if (a < m) m = a"; and where it starts
KIND = [0] * 8 + [1, 1, 1, 1, -1, 1, -1, 1]
START = [0.0] * 12 + [np.inf, -np.inf, np.inf, -np.inf]


def _wide(a):
    return np.ascontiguousarray(a).astype(np.float64)


def columns(q, u, v, w, p, obs):
    """(C_N, D, W) fp64: the COLUMN record of every (z, x).  The fields are padded (D+2, H+2, W+2) arrays."""
    q, u, v, w, p = (_wide(a) for a in (q, u, v, w, p))
    target = np.asarray(obs)[1:-1, 1:-1, 1:-1] != 1
    D, H, W = target.shape
    c = np.zeros((C_N, D, W))
    c[C_MINQ] = c[C_MINP] = np.inf
    c[C_MAXQ] = c[C_MAXP] = -np.inf
    with np.errstate(all="ignore"):
        for y in range(1, H + 1):
            t = target[:, y - 1, :]
            cq, cu, cv, cw, cp = (a[1:-1, y, 1:-1] for a in (q, u, v, w, p))
            finite = np.isfinite(cq) & np.isfinite(cu) & np.isfinite(cv) & np.isfinite(cw) & np.isfinite(cp)
            uu = cu * cu
            e = (uu + cv * cv) + cw * cw
            for k, a in ((C_CELLS, 1.0), (C_NONFINITE, np.where(finite, 0.0, 1.0)), (C_Q, cq), (C_U, cu), (C_V, cv), (C_W, cw),
                         (C_E, e), (C_P, cp), (C_UU, uu), (C_QU, cq * cu)):
                c[k] = np.where(t, c[k] + a, c[k])
            for k, a in ((C_MAXU, np.abs(cu)), (C_MAXV, np.abs(cv)), (C_MAXW, np.abs(cw)), (C_MAXE, e), (C_MAXQ, cq), (C_MAXP, cp)):
                c[k] = np.where(t & (a > c[k]), a, c[k])
            for k, a in ((C_MINQ, cq), (C_MINP, cp)):
                c[k] = np.where(t & (a < c[k]), a, c[k])
    return c


def _fold(kind, start, seq):
    """Combines the arrays of `seq` one after the other, elementwise, from `start`."""
    m = None
    with np.errstate(all="ignore"):
        for a in seq:
            if m is None:
                m = np.full(np.shape(a), start, dtype=np.float64)
            m = m + a if kind == 0 else np.where(a > m, a, m) if kind > 0 else np.where(a < m, a, m)
    return m


def monitor(q, u, v, w, p, obs):
    """(whole (16,), planes (D, 16), profile (W, 5)) in fp64."""
    c = columns(q, u, v, w, p, obs)
    _, D, W = c.shape
    planes = np.zeros((D, COLS))
    whole = np.zeros(COLS)
    for k in range(COLS):
        planes[:, k] = _fold(KIND[k], START[k], (c[PLANE_FROM[k], :, x] for x in range(W)))
        whole[k] = _fold(KIND[k], START[k], (planes[z, k] for z in range(D)))
    profile = np.zeros((W, PROFILE_COLS))
    for j in range(PROFILE_COLS):
        profile[:, j] = _fold(0, 0.0, (c[PROFILE_FROM[j], z, :] for z in range(D)))
    return whole, planes, profile


def log_row(step, whole, profile, stations):
    """One row of fs_monitor_log: step, the whole record, the profile rows of the stations (x indices, 1-based), NaN behind."""
    row = np.full(LOG_COLS, np.nan)
    row[0] = step
    row[1:1 + COLS] = whole
    for k, x in enumerate(stations):
        row[1 + COLS + PROFILE_COLS * k:1 + COLS + PROFILE_COLS * (k + 1)] = profile[x - 1]
    return row


def cfl(dt, shape, whole):
    """(cfl_x, cfl_y, cfl_z) = ((double)dt * N) * max |.| with dt as an fp32 handle member; shape = (W, H, D)."""
    dt = float(np.float32(dt))
    return tuple((dt * int(n)) * float(whole[8 + a]) for a, n in enumerate(shape))


def naive(q, u, v, w, p, obs):
    """The header once more, cell by cell in Python floats: for tiny grids."""
    import math
    D, H, W = (n - 2 for n in np.shape(obs))
    f = [[[[float(np.float64(a[z][y][x])) for a in (q, u, v, w, p)] for x in range(W + 2)] for y in range(H + 2)] for z in range(D + 2)]
    inf = math.inf
    col = {}
    with np.errstate(all="ignore"):
        for z in range(1, D + 1):
            for x in range(1, W + 1):
                r = [0.0] * 14 + [inf, -inf, inf, -inf]
                for y in range(1, H + 1):
                    if obs[z][y][x] == 1:
                        continue
                    cq, cu, cv, cw, cp = f[z][y][x]
                    uu = np.float64(cu) * np.float64(cu)
                    e = (uu + np.float64(cv) * np.float64(cv)) + np.float64(cw) * np.float64(cw)
                    bad = not all(math.isfinite(a) for a in (cq, cu, cv, cw, cp))
                    for k, a in enumerate((1.0, 1.0 if bad else 0.0, cq, cu, cv, cw, e, cp, uu, np.float64(cq) * np.float64(cu))):
                        r[k] = float(np.float64(r[k]) + np.float64(a))
                    for k, a in ((10, abs(cu)), (11, abs(cv)), (12, abs(cw)), (13, float(e)), (15, cq), (17, cp)):
                        if a > r[k]:
                            r[k] = a
                    for k, a in ((14, cq), (16, cp)):
                        if a < r[k]:
                            r[k] = a
                col[z, x] = r
        planes = np.zeros((D, COLS))
        whole = np.array(START, dtype=np.float64)
        profile = np.zeros((W, PROFILE_COLS))
        for z in range(1, D + 1):
            m = list(START)
            for x in range(1, W + 1):
                for k in range(COLS):
                    a = col[z, x][PLANE_FROM[k]]
                    if KIND[k] == 0:
                        m[k] = float(np.float64(m[k]) + np.float64(a))
                    elif (KIND[k] > 0 and a > m[k]) or (KIND[k] < 0 and a < m[k]):
                        m[k] = a
            planes[z - 1] = m
            for k in range(COLS):
                a = m[k]
                if KIND[k] == 0:
                    whole[k] = whole[k] + np.float64(a)
                elif (KIND[k] > 0 and a > whole[k]) or (KIND[k] < 0 and a < whole[k]):
                    whole[k] = a
        for x in range(1, W + 1):
            for j in range(PROFILE_COLS):
                s = np.float64(0.0)
                for z in range(1, D + 1):
                    s = s + np.float64(col[z, x][PROFILE_FROM[j]])
                profile[x - 1, j] = s
    return whole, planes, profile
