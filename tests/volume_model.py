"""The volume renderer restated in Python fp64, written from the definition in include/fluidsim.h ("volume rendering"), not
from csrc/volume.h: the rays of a camera, the box test, the march with its solid and fluid samples, the outputs.  Python floats
are IEEE doubles and every operation below is one rounding, in the header's order.  Fields are (D+2, H+2, W+2) arrays; their
values are widened exactly.  Besides acc and rgb, `render` reports each ray's class, so that a test can require that its rays
exercise every path."""
import math

import numpy as np

PARAMS = 11
CAMERAS_MAX = 4
VIEWS_MAX = 4
CAMERA = 11
SAMPLES_MAX = 16384
RN = (None, 1.0, 0.7071067811865476, 0.5773502691896257)
INF = float("inf")
# classes of a ray (bits)
INVALID, MISS, EXIT, SOLID, EARLY, NAN_SKIPPED, CUT = 1, 2, 4, 8, 16, 32, 64


def finite(x):
    return x - x == 0.0


def params(vmin=0.0, vmax=1.0, opacity=1.0, step=0.5, t_min=0.01, obstacle=(128, 128, 128), background=(26, 26, 26)):
    return [float(vmin), float(vmax), float(opacity), float(step), float(t_min)] + [float(c) for c in obstacle] + \
        [float(c) for c in background]


def kmax_of(par, W, H, D):
    """the loop limit, or None where the parameters are illegal"""
    if len(par) != PARAMS or not all(finite(p) for p in par):
        return None
    vmin, vmax, opacity, step, t_min = par[:5]
    if not (vmin < vmax and opacity >= 0.0 and step > 0.0 and 0.0 <= t_min < 1.0):
        return None
    if not all(0.0 <= c <= 255.0 for c in par[5:]):
        return None
    w, h, d = float(W + 1), float(H + 1), float(D + 1)
    q = math.sqrt((w * w + h * h) + d * d) / step
    if not q <= float(SAMPLES_MAX):
        return None
    return int(q) + 2


# ---- camera -----------------------------------------------------------------------------------------------------------------

def _dot(a, b):
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]


def _cross(a, b):
    return [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]


def _normalise(a):
    l2 = _dot(a, a)
    if not (l2 > 0.0 and finite(l2)):
        return None
    l = math.sqrt(l2)
    return [a[0] / l, a[1] / l, a[2] / l]


def camera_rays(cam, cols, rows):
    """cam = eye[3] + target[3] + up[3] + [half_height, ortho] -> (rows, cols, 6) float64, or None for an illegal camera"""
    cam = [float(c) for c in cam]
    if len(cam) != CAMERA or not all(finite(c) for c in cam) or not cam[9] > 0.0:
        return None
    eye, target, up, half, ortho = cam[0:3], cam[3:6], cam[6:9], cam[9], cam[10] != 0.0
    f = _normalise([target[a] - eye[a] for a in range(3)])
    if f is None:
        return None
    r = _normalise(_cross(f, up))
    if r is None:
        return None
    u = _cross(r, f)
    out = np.zeros((rows, cols, 6), dtype=np.float64)
    aspect = float(cols) / float(rows)
    for i in range(rows):
        sy = (1.0 - (2.0 * (float(i) + 0.5)) / float(rows)) * half
        for j in range(cols):
            sx = (((2.0 * (float(j) + 0.5)) / float(cols) - 1.0) * half) * aspect
            if ortho:
                out[i, j, :3] = [(eye[a] + sx * r[a]) + sy * u[a] for a in range(3)]
                out[i, j, 3:] = f
            else:
                out[i, j, :3] = eye
                d = _normalise([(f[a] + sx * r[a]) + sy * u[a] for a in range(3)])
                out[i, j, 3:] = d if d is not None else [0.0, 0.0, 0.0]
    return out


# ---- one ray ----------------------------------------------------------------------------------------------------------------

def box(o, d, N):
    """(t0, t1) of a valid ray against the box, or None for a miss; N = (W, H, D)"""
    t0, t1 = 0.0, INF
    for a in range(3):
        hi = float(N[a] + 1)
        if d[a] == 0.0:
            if not (0.0 <= o[a] <= hi):
                return None
            continue
        ta, tb = (0.0 - o[a]) / d[a], (hi - o[a]) / d[a]
        lo, up = (ta, tb) if ta < tb else (tb, ta)
        t0 = t0 if t0 > lo else lo
        t1 = t1 if t1 < up else up
    return (t0, t1) if t0 < t1 else None


def colour_index(v, vmin, vmax, n):
    c = vmin if v < vmin else (vmax if v > vmax else v)
    t = (c - vmin) / (vmax - vmin)
    k = int(t * float(n))
    return k if k < n - 1 else n - 1


def linear(F, p, N):
    """FS_SAMPLE_LINEAR at a point inside the box: the lerp along x, then y, then z, every corner multiplied"""
    i0, s = [], []
    for a in range(3):
        i = int(math.floor(p[a]))
        i = i if i < N[a] else N[a]
        i0.append(i)
        s.append(p[a] - float(i))
    (x, y, z), (sx, sy, sz) = i0, s
    tx, ty, tz = 1.0 - sx, 1.0 - sy, 1.0 - sz
    c = []
    for dz in (0, 1):
        for dy in (0, 1):
            row = F[z + dz][y + dy]
            c.append(row[x] * tx + row[x + 1] * sx)
    d0 = c[0] * ty + c[1] * sy
    d1 = c[2] * ty + c[3] * sy
    return d0 * tz + d1 * sz


def ray(o, d, F, S, N, par, kmax, table):
    """F: nested lists [z][y][x] of Python floats; S: the same of 0 / 1 solid flags; table: list of (r, g, b).
    -> (acc[4], rgb[3], class bits)"""
    vmin, vmax, opacity, step, t_min = par[:5]
    obst, back = par[5:8], par[8:11]
    C, T, cls = [0.0, 0.0, 0.0], 1.0, 0
    if not all(finite(x) for x in list(o) + list(d)) or (d[0] == 0.0 and d[1] == 0.0 and d[2] == 0.0):
        cls = INVALID
        tt = None
    else:
        tt = box(o, d, N)
        if tt is None:
            cls = MISS
    if tt is not None:
        t0, t1 = tt
        n = len(table)
        k = 0
        while True:
            if k >= kmax:
                cls |= CUT
                break
            tk = t0 + (float(k) + 0.5) * step
            if not tk < t1:
                cls |= EXIT
                break
            p = []
            for a in range(3):
                x = o[a] + tk * d[a]
                hi = float(N[a] + 1)
                p.append(0.0 if x < 0.0 else (hi if x > hi else x))
            i = [int(p[a] + 0.5) for a in range(3)]

            def solid(x, y, z):
                if x < 0 or x > N[0] + 1 or y < 0 or y > N[1] + 1 or z < 0 or z > N[2] + 1:
                    return 0
                return S[z][y][x]
            if solid(*i):
                g = [solid(i[0] + 1, i[1], i[2]) - solid(i[0] - 1, i[1], i[2]),
                     solid(i[0], i[1] + 1, i[2]) - solid(i[0], i[1] - 1, i[2]),
                     solid(i[0], i[1], i[2] + 1) - solid(i[0], i[1], i[2] - 1)]
                n2 = g[0] * g[0] + g[1] * g[1] + g[2] * g[2]
                shade = 1.0
                if n2 != 0:
                    s = 0.3 + 0.7 * (abs((float(g[0]) * d[0] + float(g[1]) * d[1]) + float(g[2]) * d[2]) * RN[n2])
                    shade = s if s < 1.0 else 1.0
                for c in range(3):
                    C[c] = C[c] + T * (obst[c] * shade)
                T = 0.0
                cls |= SOLID
                break
            v = linear(F, p, N)
            if v != v:
                cls |= NAN_SKIPPED
            else:
                cl = vmin if v < vmin else (vmax if v > vmax else v)
                tn = (cl - vmin) / (vmax - vmin)
                ao = (opacity * tn) * step
                a = ao if ao < 1.0 else 1.0
                if a > 0.0:
                    col = table[colour_index(v, vmin, vmax, n)]
                    w = T * a
                    for c in range(3):
                        C[c] = C[c] + w * float(col[c])
                    T = T * (1.0 - a)
            if T < t_min:
                cls |= EARLY
                break
            k += 1
    rgb = []
    for c in range(3):
        s = (C[c] + T * back[c]) + 0.5
        rgb.append(int(s if s < 255.0 else 255.0))
    return C + [T], rgb, cls


def render(rays, field, obs, par, table):
    """rays (rows, cols, 6); field, obs (D+2, H+2, W+2) -> (rgb (rows, cols, 3) uint8, acc (rows, cols, 4) float64,
    classes (rows, cols) int)"""
    field = np.asarray(field)
    D, H, W = (n - 2 for n in field.shape)
    N = (W, H, D)
    kmax = kmax_of(par, W, H, D)
    assert kmax is not None, "illegal parameters"
    with np.errstate(invalid="ignore"):
        F = field.astype(np.float64).tolist()
        S = (np.asarray(obs).astype(np.float64) > 0.5).astype(int).tolist()
    tab = [tuple(int(b) for b in t) for t in np.asarray(table).reshape(-1, 3)]
    rays = np.asarray(rays, dtype=np.float64)
    rows, cols = rays.shape[:2]
    rgb = np.zeros((rows, cols, 3), dtype=np.uint8)
    acc = np.zeros((rows, cols, 4), dtype=np.float64)
    cls = np.zeros((rows, cols), dtype=np.int64)
    for i in range(rows):
        for j in range(cols):
            r = [float(x) for x in rays[i, j]]
            a, b, c = ray(r[:3], r[3:], F, S, N, par, kmax, tab)
            acc[i, j], rgb[i, j], cls[i, j] = a, b, c
    return rgb, acc, cls


def special_rays(W, H, D):
    """the classes of the box test, by hand: entry through each face, axis-parallel rays with zero components inside and
    outside, an origin inside, exact grazing with t0 == t1, invalid rays"""
    cx, cy, cz = 0.5 * (W + 1), 0.5 * (H + 1), 0.5 * (D + 1)
    nan, inf = float("nan"), float("inf")
    r = [
        [-3.0, cy, cz, 1.0, 0.01, 0.02], [W + 4.0, cy, cz, -1.0, 0.03, -0.01],          # through x = 0 and x = W+1
        [cx, -2.0, cz, 0.02, 1.0, 0.01], [cx, H + 3.5, cz, 0.01, -1.0, 0.02],           # y faces
        [cx, cy, -5.0, 0.01, -0.02, 1.0], [cx, cy, D + 2.25, -0.02, 0.01, -1.0],        # z faces
        [-1.0, cy, cz, 1.0, 0.0, 0.0], [cx, H + 2.0, cz, 0.0, -2.0, 0.0], [cx, cy, -1.0, 0.0, 0.0, 0.5],   # axis-parallel, inside
        [-1.0, -0.5, cz, 1.0, 0.0, 0.0], [cx, -1.0, D + 1.5, 0.0, 1.0, 0.0], [W + 1.25, cy, -1.0, 0.0, 0.0, 1.0],  # ... outside
        [-1.0, 0.0, cz, 1.0, 0.0, 0.0], [-1.0, H + 1.0, D + 1.0, 1.0, 0.0, 0.0],         # along a face and an edge: inside
        [cx, cy, cz, 0.3, -0.2, 0.9], [cx, cy, cz, -1.0, 0.0, 0.0], [1.5, 1.5, 1.5, 1.0, 1.0, 1.0],        # origins inside
        [cx, cy, cz, -0.0, 0.0, 1.0],                                                   # a negative zero component
        [-1.0, -1.0, cz, 1.0, 1.0, 0.0], [-1.0, H + 2.0, cz, 1.0, -1.0, 0.0],           # in through an edge, then the interior
        [-2.0, cy, cz, -1.0, 0.0, 0.0], [cx, cy, D + 3.0, 0.0, 0.0, 1.0],                # pointing away: t1 < 0
        [nan, cy, cz, 1.0, 0.0, 0.0], [cx, cy, cz, 1.0, nan, 0.0], [cx, inf, cz, 0.0, -1.0, 0.0], [cx, cy, cz, 0.0, 0.0, -inf],
        [cx, cy, cz, 0.0, 0.0, 0.0], [cx, cy, cz, -0.0, 0.0, -0.0],                      # d = 0
        [W + 0.25, H + 0.25, D + 0.25, 1.0e-3, 0.0, 0.0], [W + 0.25, H + 0.25, D + 0.25, 0.0, 1.0e-320, 0.0],               # |d| << 1: cut at the loop limit (t1 = inf)
        [-1.0e300, cy, cz, 1.0e300, 0.0, 0.0], [cx, cy, -4.0, 1.0e-320, 0.0, 1.0],       # huge and denormal components
    ]
    # exact grazing: the ray x + y = 0 touches the box in the single point (0, 0): t0 == t1 == 1
    r.append([-1.0, 1.0, cz, 1.0, -1.0, 0.0])
    return np.array(r, dtype=np.float64)


def same_bits(a, b):
    a = np.ascontiguousarray(a, dtype=np.float64)
    b = np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))
