"""numpy fp64 restatement of the slice and projection images, written from the definition in include/fluidsim.h ("slice and
projection images"): the geometry, the four kinds with their strictly sequential order along the axis, the obstacle flag, the
colouring, and the PNG layout as a parser.  Fields are dense padded arrays of shape (D+2, H+2, W+2), as Simulation.get()
returns them."""
import struct
import zlib

import numpy as np

SLICE, SUM, MAX, MIN = range(4)
KINDS = (SLICE, SUM, MAX, MIN)
KIND_NAMES = {SLICE: "slice", SUM: "sum", MAX: "max", MIN: "min"}


def dims(axis, W, H, D):
    """(rows, cols) of an image along `axis` (0 = x, 1 = y, 2 = z)"""
    cols = H + 2 if axis == 0 else W + 2
    rows = H + 2 if axis == 2 else D + 2
    return rows, cols


def _columns(a, axis):
    """(N+2, rows, cols): the cells along `axis` first; rows run along the higher remaining axis, columns along the lower"""
    return np.moveaxis(np.asarray(a), 2 - axis, 0)


def values(field, kind, axis, index=0):
    """the value image, (rows, cols) float64"""
    col = _columns(field, axis).astype(np.float64)          # exact widening
    n = col.shape[0] - 2
    if kind == SLICE:
        return col[index].copy()
    if kind == SUM:
        s = np.zeros(col.shape[1:], dtype=np.float64)        # +0.0
        with np.errstate(invalid="ignore"):                  # inf + -inf is NaN, by definition
            for k in range(1, n + 1):
                s = s + col[k]                               # one rounding per add
        return s
    m = np.full(col.shape[1:], -np.inf if kind == MAX else np.inf, dtype=np.float64)
    for k in range(1, n + 1):
        v = col[k]
        with np.errstate(invalid="ignore"):
            m = np.where(v > m, v, m) if kind == MAX else np.where(v < m, v, m)   # NaN compares false: never taken
    return m


def flags(obs, kind, axis, index=0):
    """the obstacle flag of every pixel, (rows, cols) bool"""
    col = _columns(obs, axis).astype(np.float64) > 0.5
    if kind == SLICE:
        return col[index].copy()
    return col[1:-1].any(axis=0)


def colour(val, flag, vmin, vmax, alpha, table):
    """value image + flag image -> (rows, cols, 3) uint8 through `table`, (n, 3) uint8"""
    table = np.asarray(table, dtype=np.uint8).reshape(-1, 3)
    n = table.shape[0]
    v = np.asarray(val, dtype=np.float64)
    vmin, vmax = np.float64(vmin), np.float64(vmax)
    nan = np.isnan(v)
    w = np.where(nan, vmin, v)
    c = np.where(w < vmin, vmin, np.where(w > vmax, vmax, w))
    t = (c - vmin) / (vmax - vmin)
    k = np.minimum(n - 1, (t * np.float64(n)).astype(np.int64))
    rgb = table[k].copy()
    rgb[nan] = 0
    if alpha > 0:
        f = np.float32(np.float64(1.0) - np.float64(alpha))
        m = np.asarray(flag, dtype=bool)
        rgb[m] = (rgb[m].astype(np.float32) * f).astype(np.uint8)     # truncation
    return rgb


def image(field, obs, kind, axis, index, vmin, vmax, alpha, table):
    return colour(values(field, kind, axis, index), flags(obs, kind, axis, index), vmin, vmax, alpha, table)


def same_bits(got, want):
    """Bit-for-bit equality of two float64 arrays, any NaN equal to any NaN: the definition says where a value is NaN, and
    IEEE 754 leaves the payload and sign of an arithmetic NaN to the implementation."""
    got = np.ascontiguousarray(got, dtype=np.float64)
    want = np.ascontiguousarray(want, dtype=np.float64)
    if got.shape != want.shape:
        return False
    nan = np.isnan(want)
    return bool(np.array_equal(np.isnan(got), nan) and
                np.array_equal(got.view(np.uint64)[~nan], want.view(np.uint64)[~nan]))


def parse_png(data):
    """The pixels of a PNG as fs_image_png writes it, (rows, cols, 3) uint8.  Asserts the layout the header promises: the
    signature, IHDR (8-bit RGB, non-interlaced), exactly one IDAT whose zlib stream is stored deflate blocks only, IEND,
    every chunk's CRC, the Adler-32, and filter type 0 on every scanline.  Returns (pixels, number of stored blocks)."""
    assert data[:8] == b"\x89PNG\r\n\x1a\n", "signature"
    at, chunks = 8, []
    while at < len(data):
        (length,) = struct.unpack(">I", data[at:at + 4])
        ctype = data[at + 4:at + 8]
        body = data[at + 8:at + 8 + length]
        (crc,) = struct.unpack(">I", data[at + 8 + length:at + 12 + length])
        assert len(body) == length and crc == (zlib.crc32(ctype + body) & 0xFFFFFFFF), ("crc", ctype)
        chunks.append((ctype, body))
        at += 12 + length
    assert at == len(data) and [c for c, _ in chunks] == [b"IHDR", b"IDAT", b"IEND"], [c for c, _ in chunks]
    assert len(chunks[0][1]) == 13 and len(chunks[2][1]) == 0
    cols, rows, depth, ctype, comp, filt, lace = struct.unpack(">IIBBBBB", chunks[0][1])
    assert (depth, ctype, comp, filt, lace) == (8, 2, 0, 0, 0)
    z = chunks[1][1]
    assert (z[0] & 0x0F) == 8 and ((z[0] << 8) | z[1]) % 31 == 0 and not (z[1] & 0x20), "zlib header"
    at, raw, blocks, final = 2, b"", 0, False
    while not final:
        head = z[at]
        assert head in (0, 1), "a stored block, on a byte boundary"
        final = head == 1
        n, nn = struct.unpack("<HH", z[at + 1:at + 5])
        assert n ^ nn == 0xFFFF
        raw += z[at + 5:at + 5 + n]
        assert len(z[at + 5:at + 5 + n]) == n
        at += 5 + n
        blocks += 1
    (adler,) = struct.unpack(">I", z[at:at + 4])
    assert at + 4 == len(z) and adler == (zlib.adler32(raw) & 0xFFFFFFFF), "adler-32"
    assert zlib.decompress(z) == raw
    lines = np.frombuffer(raw, dtype=np.uint8).reshape(rows, 1 + 3 * cols)
    assert not lines[:, 0].any(), "filter type 0"
    return lines[:, 1:].reshape(rows, cols, 3).copy(), blocks
