"""numpy restatement of "per-body pressure forces and moments" in include/fluidsim.h, written from the header text:
body cells, components (iterated minimum over face neighbours), the ordering rule and the REST bucket, body info, and
the per-plane force and moment records with the per-record sum of |term| that bounds the error of a sum in any order.
Arrays are the viewers' (D + 2, H + 2, W + 2), x fastest.  No scipy."""
import numpy as np

BODY_MAX = 16
BODY_COLS = 8
BODY_INFO_COLS = 12
AXES = ((0, 0, 1), (0, 1, 0), (1, 0, 0))     # (dz, dy, dx) of axis x, y, z


def body_cells(obs):
    o = np.asarray(obs, dtype=np.float64)
    m = np.zeros(o.shape, dtype=bool)
    m[1:-1, 1:-1, 1:-1] = o[1:-1, 1:-1, 1:-1] != 0.0
    return m


def component_anchors(obs):
    """Per cell the anchor (smallest padded linear index) of its component, -1 on cells that are no body cells: every
    body cell takes the minimum over itself and its face neighbours until nothing changes."""
    body = body_cells(obs)
    big = np.iinfo(np.int64).max
    idx = np.arange(body.size, dtype=np.int64).reshape(body.shape)
    L = np.where(body, idx, big)
    while True:
        M = L.copy()
        for ax in range(3):
            for sh in (1, -1):
                M = np.minimum(M, np.roll(L, sh, axis=ax))     # ghost cells hold `big`: a roll brings nothing in
        M = np.where(body, M, big)
        flat = M.reshape(-1)
        M = np.where(body, flat[np.where(body, M, 0)], big)    # one pointer jump: the anchor my anchor knows
        if np.array_equal(M, L):
            break
        L = M
    return np.where(body, L, -1)


def order_bodies(anchors, sizes, max_bodies=BODY_MAX):
    """Label of each component: 1..B by decreasing size, ties by increasing anchor; -1 for the others (the REST)."""
    order = sorted(range(len(anchors)), key=lambda i: (-int(sizes[i]), int(anchors[i])))
    lab = [-1] * len(anchors)
    for rank, i in enumerate(order[:max_bodies]):
        lab[i] = rank + 1
    return lab


def label_bodies(obs):
    """-> (labels int32 (k on body k, -1 REST, 0 elsewhere), info (B + 1, 12) float64, number of components)"""
    o = np.asarray(obs, dtype=np.float64)
    A = component_anchors(o)
    anchors, sizes = np.unique(A[A >= 0], return_counts=True)
    lab = order_bodies(anchors, sizes)
    B = min(len(anchors), BODY_MAX)
    labels = np.zeros(o.shape, dtype=np.int32)
    for a, k in zip(anchors, lab):
        labels[A == a] = k
    z, y, x = np.indices(o.shape)
    idx = np.arange(o.size, dtype=np.int64).reshape(o.shape)
    info = np.zeros((B + 1, BODY_INFO_COLS))
    for k in range(B + 1):
        sel = labels == (k if k else -1)
        n = int(sel.sum())
        if n == 0:
            info[k, 1] = -1.0
            continue
        frontal = int((sel & (o == 1.0)).any(axis=2).sum())
        info[k] = [n, idx[sel].min(), x[sel].min(), x[sel].max(), y[sel].min(), y[sel].max(), z[sel].min(), z[sel].max(),
                   x[sel].sum(), y[sel].sum(), z[sel].sum(), frontal]
    return labels, info, len(anchors)


def face_terms(axis, sign, p, rx, ry, rz):
    """The six additions (Sx, Sy, Sz, Mx, My, Mz) of one blocked face, each product rounded once; arrays broadcast."""
    q = np.where(sign > 0, p, -p).astype(np.float64)
    t = [np.zeros_like(q) for _ in range(6)]
    t[axis] = q
    if axis == 0:
        t[4], t[5] = q * rz, -(q * ry)
    elif axis == 1:
        t[3], t[5] = -(q * rz), q * rx
    else:
        t[3], t[4] = q * ry, -(q * rx)
    return t


def face_term(axis, sign, p, rx, ry, rz, acc):
    """face_term of csrc/bodies.h on six fp64 accumulators, add by add."""
    t = face_terms(axis, sign, np.float64(p), np.float64(rx), np.float64(ry), np.float64(rz))
    used = {0: (0, 4, 5), 1: (1, 3, 5), 2: (2, 3, 4)}[axis]
    for c in used:
        acc[c] = np.float64(acc[c]) + np.float64(t[c])
    return acc


def body_records(obs, p, labels, B, origin=(0.0, 0.0, 0.0)):
    """-> (rec (D, B + 1, 8): {Sx, Sy, Sz, Mx, My, Mz, faces, frontal rows} per plane and record,
           mag (D, B + 1, 6): the sum of |term| behind each of the six sums)"""
    o = np.asarray(obs, dtype=np.float64)
    D, H, W = (n - 2 for n in o.shape)
    inner = (slice(1, D + 1), slice(1, H + 1), slice(1, W + 1))
    upd = o[inner] != 1.0
    pc = np.asarray(p).astype(np.float64)[inner]
    z, y, x = np.meshgrid(np.arange(1, D + 1), np.arange(1, H + 1), np.arange(1, W + 1), indexing="ij")
    rx, ry, rz = x - np.float64(origin[0]), y - np.float64(origin[1]), z - np.float64(origin[2])
    recof = np.where(labels > 0, labels, 0)
    rec = np.zeros((D, B + 1, BODY_COLS))
    mag = np.zeros((D, B + 1, 6))
    for axis, (dz, dy, dx) in enumerate(AXES):
        for sgn in (1, -1):
            nsl = (slice(1 + sgn * dz, D + 1 + sgn * dz), slice(1 + sgn * dy, H + 1 + sgn * dy),
                   slice(1 + sgn * dx, W + 1 + sgn * dx))
            zz, yy, xx = z + sgn * dz, y + sgn * dy, x + sgn * dx
            inr = (xx >= 1) & (xx <= W) & (yy >= 1) & (yy <= H) & (zz >= 1) & (zz <= D)
            blocked = upd & inr & (o[nsl] != 0.0)
            terms = face_terms(axis, sgn, pc, rx, ry, rz)
            for k in range(B + 1):
                sel = blocked & (recof[nsl] == k)
                rec[:, k, 6] += sel.sum(axis=(1, 2))
                for c in range(6):
                    rec[:, k, c] += np.where(sel, terms[c], 0.0).sum(axis=(1, 2))
                    mag[:, k, c] += np.where(sel, np.abs(terms[c]), 0.0).sum(axis=(1, 2))
    for k in range(B + 1):
        sel = (labels[inner] == (k if k else -1)) & (o[inner] == 1.0)
        rec[:, k, 7] = sel.any(axis=2).sum(axis=1)
    return rec, mag


def totals(rec):
    """The whole-grid records: the planes added in increasing z in fp64, from +0.0."""
    tot = np.zeros(rec.shape[1:])
    for r in rec:
        tot = tot + r
    return tot
