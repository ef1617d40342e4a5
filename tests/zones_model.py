"""Momentum zones as include/fluidsim.h defines them ("momentum zones"), restated in numpy with one rounded operation per numpy
call and fp64 intermediates, written from the header's text (not from the kernels): the mask (fs_zone_mask), the pass
(fs_zone_apply) and the budget (fs_zone_budget) in its written order of summation.  `naive_*` are the same texts as scalar
loops, for tiny grids.  Shared by tests/test_zones_cpu.py and tests/test_gpu_zones.py.  Arrays are padded, indexed [z, y, x];
`zones` is a sequence of rows of 20 numbers."""
import numpy as np

from heat_model import NEIGHBOURS, cell_kinds, flag_bytes, interior, set_bounds  # noqa: F401  (what "solid", "near" and setBounds mean)

PARAMS = 20
COLS = 7
MAX = 8
(C_CELLS, C_DX, C_DY, C_DZ, C_DK, C_FLUX, C_MAXM) = range(COLS)
START = [0.0, 0.0, 0.0, 0.0, 0.0, 0.0, -np.inf]
BOX, CYLINDER = 0, 1


def row(shape=BOX, axis=0, box=(1, 1, 1, 1, 1, 1), centre=(0.0, 0.0), radius=0.0, g=(0.0, 0.0, 0.0), D=(0.0, 0.0, 0.0), F=(0.0, 0.0, 0.0)):
    r = np.zeros(PARAMS)
    r[0], r[1] = shape, axis
    r[2:8] = box
    r[8:10] = centre
    r[10] = radius
    r[11:14], r[14:17], r[17:20] = g, D, F
    return r


def whole_box(grid):
    W, H, D = grid
    return (1, W, 1, H, 1, D)


def target_cells(obs):
    """interior, obs != 1, no interior 6-neighbour with obs == 1"""
    solid, near, _ = cell_kinds(obs)
    return interior(np.shape(obs)) & ~solid & ~near


def in_zone(r, shape):
    """The cells IN the zone (padded boolean array)."""
    z, y, x = np.indices(shape)
    x0, x1, y0, y1, z0, z1 = (int(v) for v in r[2:8])
    inside = (x >= x0) & (x <= x1) & (y >= y0) & (y <= y1) & (z >= z0) & (z <= z1)
    if int(r[0]) == BOX:
        return inside
    axis = int(r[1])
    i, j = [a for k, a in enumerate((x, y, z)) if k != axis]
    p = i.astype(np.float64) - np.float64(r[8])
    q = j.astype(np.float64) - np.float64(r[9])
    r2 = np.float64(r[10]) * np.float64(r[10])
    return inside & (p * p + q * q <= r2)


def mask(obs, zones):
    """fs_zone_mask: bit k where the cell is a target cell in zone k."""
    tgt = target_cells(obs)
    out = np.zeros(np.shape(obs), dtype=np.uint8)
    for k, r in enumerate(zones):
        out |= ((tgt & in_zone(r, out.shape)).astype(np.uint8) << k).astype(np.uint8)
    return out


def stage(u, r, dt):
    """One stage on whole fp64 arrays: (u', k0, m, k1)."""
    DT = np.float64(np.float32(dt))
    with np.errstate(all="ignore"):
        k0 = (u[0] * u[0] + u[1] * u[1]) + u[2] * u[2]
        m = np.sqrt(k0)
        new = []
        for a in range(3):
            G = DT * np.float64(r[11 + a])
            n = u[a] + G
            rr = np.float64(r[17 + a]) * m
            s = np.float64(r[14 + a]) + rr
            t = DT * s
            d = 1.0 + t
            new.append(n / d)
        k1 = (new[0] * new[0] + new[1] * new[1]) + new[2] * new[2]
    return new, k0, m, k1


def apply_unbounded(vel, obs, zones, dt):
    """The pass WITHOUT its setBounds: [u, v, w] with the target cells' new values, everything else as stored."""
    vel = [np.asarray(v) for v in vel]
    tgt = target_cells(obs)
    u = [v.astype(np.float64) for v in vel]
    touched = np.zeros(vel[0].shape, dtype=bool)
    for r in zones:
        sel = tgt & in_zone(r, touched.shape)
        new = stage(u, r, dt)[0]
        u = [np.where(sel, n, o) for n, o in zip(new, u)]
        touched |= sel
    with np.errstate(all="ignore"):
        return [np.where(touched, a.astype(v.dtype), v) for a, v in zip(u, vel)]


def apply(vel, obs, zones, dt):
    """fs_zone_apply: [u', v', w'] as fs_set_bounds(1, .), (2, .), (3, .) leave the pass's values."""
    return [set_bounds(a, b + 1, obs) for b, a in enumerate(apply_unbounded(vel, obs, zones, dt))]


def _combine(k, m, a):
    return np.where(a > m, a, m) if k == C_MAXM else m + a


def budget(vel, obs, zones, dt):
    """fs_zone_budget: (whole (n, 7), planes (D, n, 7)) in fp64; columns in increasing y, planes in increasing x, the whole
    in increasing z."""
    tgt = target_cells(obs)
    u = [np.asarray(v).astype(np.float64) for v in vel]
    D, H, W = (n - 2 for n in np.shape(obs))
    c = slice(1, -1)
    planes = np.zeros((D, len(zones), COLS))
    whole = np.zeros((len(zones), COLS))
    for k, r in enumerate(zones):
        sel = tgt & in_zone(r, tgt.shape)
        new, k0, m, k1 = stage(u, r, dt)
        with np.errstate(all="ignore"):
            add = [np.ones(tgt.shape)] + [n - o for n, o in zip(new, u)] + [0.5 * (k1 - k0), u[int(r[1])], m]
            col = np.zeros((COLS, D, W))
            col[C_MAXM] = -np.inf
            for y in range(1, H + 1):
                s = sel[c, y, c]
                for j in range(COLS):
                    a = add[j][c, y, c]
                    col[j] = np.where(s & (a > col[j]), a, col[j]) if j == C_MAXM else np.where(s, col[j] + a, col[j])
            for j in range(COLS):
                p = np.full(D, START[j])
                for x in range(W):
                    p = _combine(j, p, col[j][:, x])
                planes[:, k, j] = p
                w = np.float64(START[j])
                for z in range(D):
                    w = _combine(j, w, p[z])
                whole[k, j] = w
        u = [np.where(sel, n, o) for n, o in zip(new, u)]
    return whole, planes


def same(a, b):
    """bit for bit; a NaN matches a NaN of any sign and payload (IEEE 754 leaves those of an arithmetic NaN open)"""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    na, nb = np.isnan(a), np.isnan(b)
    u = {4: np.uint32, 8: np.uint64}[a.dtype.itemsize]
    return bool(np.array_equal(na, nb) and np.array_equal(np.where(na, 0, a).view(u), np.where(nb, 0, b).view(u)))


def log_row(step, whole):
    return np.concatenate([[float(step)], np.asarray(whole).ravel()])


# ---- the header once more, cell by cell: for tiny grids --------------------------------------------------------------------

def _is_target(obs, z, y, x):
    D, H, W = (n - 2 for n in np.shape(obs))
    if obs[z, y, x] == 1:
        return False
    for dz, dy, dx in NEIGHBOURS:
        p = (z + dz, y + dy, x + dx)
        if 1 <= p[0] <= D and 1 <= p[1] <= H and 1 <= p[2] <= W and obs[p] == 1:
            return False
    return True


def _is_in(r, z, y, x):
    x0, x1, y0, y1, z0, z1 = (int(v) for v in r[2:8])
    if not (x0 <= x <= x1 and y0 <= y <= y1 and z0 <= z <= z1):
        return False
    if int(r[0]) == BOX:
        return True
    i, j = [(y, z), (x, z), (x, y)][int(r[1])]
    p = np.float64(i) - np.float64(r[8])
    q = np.float64(j) - np.float64(r[9])
    return bool(p * p + q * q <= np.float64(r[10]) * np.float64(r[10]))


def _naive_stage(u, r, DT):
    k0 = (u[0] * u[0] + u[1] * u[1]) + u[2] * u[2]
    m = np.sqrt(k0)
    new = []
    for a in range(3):
        n = u[a] + DT * np.float64(r[11 + a])
        d = np.float64(1.0) + DT * (np.float64(r[14 + a]) + np.float64(r[17 + a]) * m)
        new.append(n / d)
    k1 = (new[0] * new[0] + new[1] * new[1]) + new[2] * new[2]
    return new, k0, m, k1


def naive(vel, obs, zones, dt):
    """(mask, [u', v', w'] of the pass, whole, planes of the budget) by scalar loops in the header's order."""
    vel = [np.asarray(v) for v in vel]
    T = vel[0].dtype.type
    D, H, W = (n - 2 for n in np.shape(obs))
    DT = np.float64(np.float32(dt))
    bits = np.zeros(np.shape(obs), dtype=np.uint8)
    out = [v.copy() for v in vel]
    nz = len(zones)
    planes = np.zeros((D, nz, COLS))
    whole = np.array([START] * nz, dtype=np.float64).reshape(nz, COLS)
    with np.errstate(all="ignore"):
        for z in range(1, D + 1):
            plane = np.array([START] * nz, dtype=np.float64).reshape(nz, COLS)
            for x in range(1, W + 1):
                colm = np.array([START] * nz, dtype=np.float64).reshape(nz, COLS)
                for y in range(1, H + 1):
                    if not _is_target(obs, z, y, x):
                        continue
                    u = [np.float64(v[z, y, x]) for v in vel]
                    hit = False
                    for k, r in enumerate(zones):
                        if not _is_in(r, z, y, x):
                            continue
                        hit = True
                        bits[z, y, x] |= np.uint8(1 << k)
                        new, k0, m, k1 = _naive_stage(u, r, DT)
                        colm[k, C_CELLS] = colm[k, C_CELLS] + 1.0
                        for a in range(3):
                            colm[k, C_DX + a] = colm[k, C_DX + a] + (new[a] - u[a])
                        colm[k, C_DK] = colm[k, C_DK] + 0.5 * (k1 - k0)
                        colm[k, C_FLUX] = colm[k, C_FLUX] + u[int(r[1])]
                        if m > colm[k, C_MAXM]:
                            colm[k, C_MAXM] = m
                        u = new
                    if hit:
                        for a in range(3):
                            out[a][z, y, x] = T(u[a])
                for k in range(nz):
                    for j in range(COLS):
                        plane[k, j] = (colm[k, j] if colm[k, j] > plane[k, j] else plane[k, j]) if j == C_MAXM else plane[k, j] + colm[k, j]
            planes[z - 1] = plane
            for k in range(nz):
                for j in range(COLS):
                    whole[k, j] = (plane[k, j] if plane[k, j] > whole[k, j] else whole[k, j]) if j == C_MAXM else whole[k, j] + plane[k, j]
    return bits, [set_bounds(a, b + 1, obs) for b, a in enumerate(out)], whole, planes
