"""What crosses the library's boundary, in plain numpy: the conversions of fs_get_field / fs_set_field and of the frame dump
(csrc/fields.hip pack_kernel / unpack_kernel), the bytes of a frame (csrc/dump.h), the console's density sum
(Engine::reference_order_sum) and the run statistics (stats_partial_kernel / stats_final_kernel).  No GPU, no library.

Definitions:
  narrowing  float64 -> float32 is IEEE round-to-nearest-even, subnormal results kept, overflow to infinity;
  widening   float32 -> float64 is exact;
  uint8      truncation toward zero, defined only for 0 <= v < 256;
  a NaN      keeps every bit in a transfer that does not convert; one that converts yields some NaN (compare after canon()).
"""
import math

import numpy as np

FLT_MAX = float(np.finfo(np.float32).max)
FILES = ("data", "obs", "v_x", "v_y", "v_z")          # file order of a frame; the fields are DENS, OBS, VX, VY, VZ


def narrow(a64):
    a64 = np.asarray(a64, dtype=np.float64)
    with np.errstate(over="ignore", invalid="ignore"):
        return a64.astype(np.float32)


def widen(a32):
    with np.errstate(invalid="ignore"):                 # a signalling NaN is quieted, not an error
        return np.asarray(a32, dtype=np.float32).astype(np.float64)


def to_u8(a):
    a = np.asarray(a)
    if not bool(np.all((a >= 0) & (a < 256))):          # a NaN fails both comparisons
        raise ValueError("to_u8 is defined for 0 <= v < 256 only")
    return np.trunc(a).astype(np.uint8)


def canon(a):
    """every NaN -> the one quiet NaN numpy writes for float('nan') (rough_cases.canon's rule)"""
    a = np.array(a, copy=True)
    a[np.isnan(a)] = np.nan
    return a


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({1: np.uint8, 4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def _both_signs(v):
    return np.concatenate([v, -v])                      # negation flips the sign bit of a NaN too and keeps its payload


def narrowing_values():
    """float64 values at the edges of the float32 format, with both signs; NARROWED_BITS holds what they must become"""
    nan = np.array([0x7ff8000000000000, 0x7ff0000000000001, 0x7ff8000000abcdef, 0x7ff4000012345678], dtype=np.uint64).view(np.float64)
    v = np.array([1 + 2.0 ** -24,                         # tie -> even, down
                  1 + 3 * 2.0 ** -24,                     # tie -> even, up
                  1 + 2.0 ** -24 + 2.0 ** -50,            # just above the tie
                  FLT_MAX * (1 + 2.0 ** -25),             # below the overflow threshold: stays FLT_MAX
                  FLT_MAX * (1 + 2.0 ** -24),             # above it: infinity
                  2.0 ** -149,                            # the smallest float32 subnormal
                  2.0 ** -150,                            # tie between 0 and it -> even: 0
                  2.0 ** -150 * (1 + 2.0 ** -20),         # just above that tie
                  2.0 ** -126 * (1 - 2.0 ** -30),         # just below the smallest normal: rounds up to it
                  0.0, np.inf], dtype=np.float64)
    return _both_signs(np.concatenate([v, nan]))


# float32 bit patterns of narrow(narrowing_values()), written by hand; None = some NaN
NARROWED_BITS = [0x3f800000, 0x3f800002, 0x3f800001, 0x7f7fffff, 0x7f800000, 0x00000001, 0x00000000, 0x00000001, 0x00800000,
                 0x00000000, 0x7f800000, None, None, None, None]
NARROWED_BITS = NARROWED_BITS + [None if b is None else b | 0x80000000 for b in NARROWED_BITS]


def edge_values(dtype):
    """The value table of the transfer tests as an array of `dtype`: for float64 the narrowing table followed by what a
    same-width transfer must keep (float64 subnormals, NaNs with payloads); for float32 subnormals, signed zeros, the
    largest and smallest normals, infinities and NaNs with payloads, quiet and signalling."""
    dtype = np.dtype(dtype)
    if dtype == np.float64:
        own = np.array([0x0000000000000001, 0x000fffffffffffff, 0x0010000000000000, 0x7fefffffffffffff,
                        0x7ff8000000000001, 0x7ff00000deadbeef, 0x7fffffffffffffff], dtype=np.uint64).view(np.float64)
        return np.concatenate([narrowing_values(), _both_signs(own)])
    if dtype == np.float32:
        own = np.array([0x00000000, 0x00000001, 0x007fffff, 0x00800000, 0x7f7fffff, 0x7f800000,
                        0x7fc00000, 0x7fc12345, 0x7f800001, 0x7fa00000, 0x7fffffff], dtype=np.uint32).view(np.float32)
        return _both_signs(own)
    raise ValueError("edge_values: float32 or float64")


def frame_bytes(fields):
    """The bytes one frame adds to the five files, in file order: `fields` are the arrays DENS, OBS, VX, VY, VZ of the state
    (any float dtype, shape (D+2, H+2, W+2)); each is narrowed to float32 and laid out in C order."""
    fields = list(fields)
    assert len(fields) == len(FILES)
    return [np.ascontiguousarray(narrow(f)).tobytes() for f in fields]


def reduce_order_sum(a):
    """libstdc++'s std::reduce(first, last) over the array in C order, in the array's own dtype: groups of four as
    (a0 + a1) + (a2 + a3), each added to the running sum, then the tail one by one"""
    a = np.ascontiguousarray(a).reshape(-1)
    t = a.dtype.type
    n4 = a.size // 4 * 4
    with np.errstate(over="ignore", invalid="ignore"):
        g = a[:n4].reshape(-1, 4)
        v3 = (g[:, 0] + g[:, 1]) + (g[:, 2] + g[:, 3])
        assert v3.dtype == a.dtype
        init = t(0)
        for v in v3:
            init = t(init + v)
        for v in a[n4:]:
            init = t(init + v)
    return init


def stats(a):
    """(sum, min, max) of the whole array as fs_field_stats defines them: the sum of the values in float64 (here the exactly
    rounded one where every value is finite), min and max over the values that are not NaN (+inf / -inf if there is none)"""
    v = np.asarray(a).astype(np.float64).reshape(-1)
    if np.isfinite(v).all():
        s = math.fsum(v.tolist())
    else:
        with np.errstate(invalid="ignore"):
            s = float(np.sum(v))
    ok = v[~np.isnan(v)]
    return s, (float(ok.min()) if ok.size else math.inf), (float(ok.max()) if ok.size else -math.inf)
