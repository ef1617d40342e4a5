"""Heat and buoyancy as include/fluidsim.h defines them ("heat and buoyancy"), restated in numpy with one rounded operation
per numpy call and fp64 intermediates, written from the header's text (not from the kernels): pass A (fs_heat_apply) and
pass C (fs_heat_budget) in its written order of summation.  `naive_*` are the same texts as scalar loops, for tiny grids.
Shared by tests/test_heat_cpu.py and tests/test_gpu_heat.py.  Arrays are padded, indexed [z, y, x]."""
import numpy as np

PARAMS = 15
COLS = 9
(C_CELLS, C_SUM, C_SUM2, C_MAX, C_MIN, C_HELD, C_LOSS, C_OUT, C_IN) = range(COLS)
KIND = [0, 0, 0, 1, -1, 0, 0, 0, 0]                        # 0 a sum, +1 "if (a > m) m = a", -1 "if (a < m) m = a"
START = [0.0, 0.0, 0.0, -np.inf, np.inf, 0.0, 0.0, 0.0, 0.0]
UP = {"+x": 0, "-x": 1, "+y": 2, "-y": 3, "+z": 4, "-z": 5}
# neighbours in the order of the conductive loss: x-, x+, y-, y+, z-, z+ as (dz, dy, dx)
NEIGHBOURS = [(0, 0, -1), (0, 0, 1), (0, -1, 0), (0, 1, 0), (-1, 0, 0), (1, 0, 0)]


def params(mode=1, kappa=0.0, beta=0.0, alpha=0.0, up=2, inlet=0.0, wall=None, box=None, log=0, shape=None):
    """The array fs_heat_params takes; shape = (W, H, D) gives the default box."""
    p = np.zeros(PARAMS)
    p[0:6] = mode, kappa, beta, alpha, (UP[up] if isinstance(up, str) else up), inlet
    p[6:8] = (0, 0.0) if wall is None else (1, wall)
    p[8:14] = box if box is not None else (1, shape[0], 1, shape[1], 1, shape[2])
    p[14] = log
    return p


def interior(shape):
    m = np.zeros(shape, dtype=bool)
    m[1:-1, 1:-1, 1:-1] = True
    return m


def cell_kinds(obs):
    """(solid, near, fluid) boolean padded arrays: interior with obs == 1; interior with obs != 1 and an interior
    6-neighbour with obs == 1; interior with obs == 0."""
    obs = np.asarray(obs)
    inner = interior(obs.shape)
    solid = inner & (obs == 1)
    fluid = inner & (obs == 0)
    beside = np.zeros(obs.shape, dtype=bool)
    for dz, dy, dx in NEIGHBOURS:
        beside |= np.roll(solid, (-dz, -dy, -dx), axis=(0, 1, 2))   # solid has no ghost cells, so nothing wraps into the interior
    near = inner & ~solid & beside
    return solid, near, fluid


def held_cells(obs, par):
    """The cells pass A holds at the wall temperature."""
    solid, near, _ = cell_kinds(obs)
    if int(par[6]) == 0:
        return np.zeros(np.shape(obs), dtype=bool)
    z, y, x = np.indices(np.shape(obs))
    x0, x1, y0, y1, z0, z1 = (int(v) for v in par[8:14])
    return near & (x >= x0) & (x <= x1) & (y >= y0) & (y <= y1) & (z >= z0) & (z <= z1)


def set_bounds(a, b, obs):
    """fs_set_bounds(b, .) on a padded array: ghost faces from the interior as it is, then the zeroing.  The twelve box
    edges stay."""
    a = np.array(a)
    c = slice(1, -1)
    a[c, c, 0] = -a[c, c, 1] if b == 1 else a[c, c, 1]
    a[c, c, -1] = a[c, c, -2]
    a[c, 0, c] = -a[c, 1, c] if b == 2 else a[c, 1, c]
    a[c, -1, c] = -a[c, -2, c] if b == 2 else a[c, -2, c]
    a[0, c, c] = -a[1, c, c] if b == 3 else a[1, c, c]
    a[-1, c, c] = -a[-2, c, c] if b == 3 else a[-2, c, c]
    solid, near, _ = cell_kinds(obs)
    a[solid] = 0
    if b in (1, 2, 3):
        a[near] = 0
    return a


def working(theta, obs, par):
    """Step 1: the working value of every interior cell (ghosts as stored)."""
    theta = np.asarray(theta)
    t = theta.copy()
    t[1:-1, 1:-1, 1] = theta.dtype.type(par[5])
    t[held_cells(obs, par)] = theta.dtype.type(par[7])
    return t


def buoyancy(v, t, q, par, dt):
    """Step 2 on whole arrays: (T)((double)v +- dt * (beta * t - alpha * q)), dt the handle's float member."""
    v = np.asarray(v)
    with np.errstate(all="ignore"):
        b = np.float64(par[2]) * np.asarray(t).astype(np.float64)
        w = np.float64(par[3]) * np.asarray(q).astype(np.float64)
        d = b - w
        f = np.float64(np.float32(dt)) * d
        wide = v.astype(np.float64)
        return (wide - f if int(par[4]) & 1 else wide + f).astype(v.dtype)


def apply_unbounded(theta, vel, dens, obs, par, dt):
    """Pass A WITHOUT step 3: (t, [u, v, w]) with the interior cells' new values, everything else as stored."""
    t = working(theta, obs, par)
    vel = [np.array(a) for a in vel]
    if par[2] != 0 or par[3] != 0:
        a = int(par[4]) >> 1
        new = buoyancy(vel[a], t, dens, par, dt)
        c = slice(1, -1)
        vel[a][c, c, c] = new[c, c, c]
    return t, vel


def apply(theta, vel, dens, obs, par, dt):
    """Pass A: (theta', [u', v', w']).  With beta = alpha = 0 the velocities are the very arrays passed in."""
    t, new = apply_unbounded(theta, vel, dens, obs, par, dt)
    t = set_bounds(t, 0, obs)
    if par[2] == 0 and par[3] == 0:
        return t, list(vel)
    a = int(par[4]) >> 1
    new[a] = set_bounds(new[a], a + 1, obs)
    return t, new


def _fold(kind, start, seq):
    m = None
    with np.errstate(all="ignore"):
        for a in seq:
            if m is None:
                m = np.full(np.shape(a), start, dtype=np.float64)
            m = m + a if kind == 0 else np.where(a > m, a, m) if kind > 0 else np.where(a < m, a, m)
    return m


def cell_losses(theta, obs, par):
    """The conductive loss of every cell as if it were held (fp64, padded): s = 0, then s = s + (theta_c - theta_n) over the
    neighbours that are interior, have obs == 0 and are not held, in the order x-, x+, y-, y+, z-, z+."""
    theta = np.ascontiguousarray(theta).astype(np.float64)
    _, _, fluid = cell_kinds(obs)
    counts = fluid & ~held_cells(obs, par)
    s = np.zeros(theta.shape)
    with np.errstate(all="ignore"):
        for dz, dy, dx in NEIGHBOURS:
            nb_t = np.roll(theta, (-dz, -dy, -dx), axis=(0, 1, 2))
            nb_ok = np.roll(counts, (-dz, -dy, -dx), axis=(0, 1, 2))
            s = np.where(nb_ok, s + (theta - nb_t), s)
    return s


def flag_bytes(obs):
    """The flag byte of every cell as the library builds it: 1 solid, 2 near, 4 / 8 x+ / x-, 16 / 32 y+ / y-, 64 / 128 z+ / z-
    "that neighbour is interior with obs == 0"."""
    solid, near, fluid = cell_kinds(obs)
    f = solid.astype(np.uint8) | (near.astype(np.uint8) << 1)
    for bit, (dz, dy, dx) in zip((8, 4, 32, 16, 128, 64), NEIGHBOURS):
        f |= np.where(interior(f.shape) & np.roll(fluid, (-dz, -dy, -dx), axis=(0, 1, 2)), bit, 0).astype(np.uint8)
    return f


def budget(theta, u, obs, par):
    """Pass C: (whole (9,), planes (D, 9)) in fp64, columns in increasing y, planes in increasing x, the whole in increasing z."""
    theta = np.ascontiguousarray(theta).astype(np.float64)
    u = np.ascontiguousarray(u).astype(np.float64)
    obs = np.asarray(obs)
    solid, near, fluid = cell_kinds(obs)
    target = interior(obs.shape) & ~solid
    held = held_cells(obs, par)
    D, H, W = (n - 2 for n in obs.shape)
    c = slice(1, -1)
    cell_loss = cell_losses(theta, obs, par)
    with np.errstate(all="ignore"):
        col = np.zeros((8, D, W))
        col[3], col[4] = -np.inf, np.inf
        for y in range(1, H + 1):
            tg, th, hd = target[c, y, c], theta[c, y, c], held[c, y, c]
            for k, a in ((0, 1.0), (1, th), (2, th * th)):
                col[k] = np.where(tg, col[k] + a, col[k])
            col[3] = np.where(tg & (th > col[3]), th, col[3])
            col[4] = np.where(tg & (th < col[4]), th, col[4])
            col[5] = np.where(tg & hd, col[5] + 1.0, col[5])
            col[6] = np.where(tg & hd, col[6] + cell_loss[c, y, c], col[6])
            col[7] = np.where(tg, col[7] + u[c, y, c] * th, col[7])
    planes = np.zeros((D, COLS))
    whole = np.zeros(COLS)
    for k in range(COLS):
        if k == C_OUT:
            planes[:, k] = col[7][:, W - 1]
        elif k == C_IN:
            planes[:, k] = col[7][:, 0]
        else:
            planes[:, k] = _fold(KIND[k], START[k], (col[k][:, x] for x in range(W)))
        whole[k] = _fold(KIND[k], START[k], (planes[z, k] for z in range(D)))
    return whole, planes


def log_row(step, whole):
    return np.concatenate([[float(step)], whole])


# ---- the header once more, cell by cell: for tiny grids --------------------------------------------------------------------

def _is_held(obs, par, z, y, x):
    D, H, W = (n - 2 for n in np.shape(obs))
    if int(par[6]) == 0 or obs[z, y, x] == 1:
        return False
    x0, x1, y0, y1, z0, z1 = (int(v) for v in par[8:14])
    if not (x0 <= x <= x1 and y0 <= y <= y1 and z0 <= z <= z1):
        return False
    for dz, dy, dx in NEIGHBOURS:
        p = (z + dz, y + dy, x + dx)
        if 1 <= p[0] <= D and 1 <= p[1] <= H and 1 <= p[2] <= W and obs[p] == 1:
            return True
    return False


def naive_apply(theta, vel, dens, obs, par, dt):
    theta = np.asarray(theta)
    T = theta.dtype.type
    D, H, W = (n - 2 for n in theta.shape)
    force = par[2] != 0 or par[3] != 0
    a = int(par[4]) >> 1
    t = theta.copy()
    out = [np.array(v) for v in vel] if force else list(vel)
    dt64 = np.float64(np.float32(dt))
    with np.errstate(all="ignore"):
        for z in range(1, D + 1):
            for y in range(1, H + 1):
                for x in range(1, W + 1):
                    w = theta[z, y, x]
                    if x == 1:
                        w = T(par[5])
                    if _is_held(obs, par, z, y, x):
                        w = T(par[7])
                    t[z, y, x] = w
                    if force:
                        b = np.float64(par[2]) * np.float64(w)
                        g = np.float64(par[3]) * np.float64(dens[z, y, x])
                        d = b - g
                        f = dt64 * d
                        v = np.float64(vel[a][z, y, x])
                        out[a][z, y, x] = T(v - f) if int(par[4]) & 1 else T(v + f)
    t = set_bounds(t, 0, obs)
    if force:
        out[a] = set_bounds(out[a], a + 1, obs)
    return t, out


def naive_budget(theta, u, obs, par):
    D, H, W = (n - 2 for n in np.shape(obs))
    planes = np.zeros((D, COLS))
    whole = np.array(START, dtype=np.float64)

    def comb(k, m, a):
        if KIND[k] == 0:
            return np.float64(m) + np.float64(a)
        if KIND[k] > 0:
            return a if a > m else m
        return a if a < m else m

    with np.errstate(all="ignore"):
        for z in range(1, D + 1):
            m = list(START)
            for x in range(1, W + 1):
                r = [0.0, 0.0, 0.0, -np.inf, np.inf, 0.0, 0.0, 0.0]
                for y in range(1, H + 1):
                    if obs[z, y, x] == 1:
                        continue
                    th = np.float64(theta[z, y, x])
                    r[0] = r[0] + 1.0
                    r[1] = np.float64(r[1]) + th
                    r[2] = np.float64(r[2]) + th * th
                    if th > r[3]:
                        r[3] = th
                    if th < r[4]:
                        r[4] = th
                    r[7] = np.float64(r[7]) + np.float64(u[z, y, x]) * th
                    if _is_held(obs, par, z, y, x):
                        r[5] = r[5] + 1.0
                        s = np.float64(0.0)
                        for dz, dy, dx in NEIGHBOURS:
                            p = (z + dz, y + dy, x + dx)
                            if not (1 <= p[0] <= D and 1 <= p[1] <= H and 1 <= p[2] <= W) or obs[p] != 0 or _is_held(obs, par, *p):
                                continue
                            s = s + (th - np.float64(theta[p]))
                        r[6] = np.float64(r[6]) + s
                for k in range(7):
                    m[k] = comb(k, m[k], r[k])
                if x == W:
                    m[C_OUT] = r[7]
                if x == 1:
                    m[C_IN] = r[7]
            planes[z - 1] = m
            for k in range(COLS):
                whole[k] = comb(k, whole[k], m[k])
    return whole, planes
