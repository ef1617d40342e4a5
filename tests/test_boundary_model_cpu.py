"""The model the boundary tests measure with (tests/boundary_model.py), checked on its own: the reduction order against a
scalar loop, narrowing against bit patterns written by hand, and the bytes of a frame against the reference's own dump."""
import math

import numpy as np
import pytest

import boundary_model as M
from conftest import load_golden


def scalar_reduce(a):
    """<numeric>'s std::reduce, random-access branch, one scalar operation at a time"""
    t = a.dtype.type
    init, i, n = t(0), 0, len(a)
    with np.errstate(over="ignore", invalid="ignore"):
        while n - i >= 4:
            v1 = t(a[i] + a[i + 1])
            v2 = t(a[i + 2] + a[i + 3])
            v3 = t(v1 + v2)
            init = t(init + v3)
            i += 4
        while i < n:
            init = t(init + a[i])
            i += 1
    return init


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_reduce_order_sum_is_the_scalar_loop(dtype):
    rng = np.random.default_rng(11)
    differs = 0
    for n in list(range(10)) + [1001]:
        a = (rng.standard_normal(n) * 10.0 ** rng.integers(-3, 4, n)).astype(dtype)
        got, want = M.reduce_order_sum(a), scalar_reduce(a)
        assert type(got) is dtype and M.bits(np.array([got]))[0] == M.bits(np.array([want]))[0], n
        plain = dtype(0)
        for v in a:
            plain = dtype(plain + v)
        differs += int(plain != got)
    assert differs > 0                       # the order matters on these arrays: a plain left-to-right sum is another number
    assert M.reduce_order_sum(np.zeros((2, 3, 0), dtype=dtype)) == 0


def test_narrow_on_the_table():
    v = M.narrowing_values()
    assert len(v) == len(M.NARROWED_BITS) == 30
    got = M.narrow(v)
    assert got.dtype == np.float32
    for x, g, want in zip(v, M.bits(got), M.NARROWED_BITS):
        if want is None:
            assert math.isnan(x) and (int(g) & 0x7f800000) == 0x7f800000 and (int(g) & 0x007fffff) != 0, (x, hex(int(g)))
        else:
            assert int(g) == want, (x.hex(), hex(int(g)), hex(want))
    # the table's own claims: which side of which threshold each value lies on
    assert v[0] == 1 + 2.0 ** -24 and v[3] > M.FLT_MAX and v[4] > v[3] and v[6] * 2 == v[5] and v[8] < 2.0 ** -126
    assert np.signbit(v[15:]).all() and not np.signbit(v[:15]).any()


def test_edge_values_and_u8():
    for dt, u in ((np.float32, np.uint32), (np.float64, np.uint64)):
        e = M.edge_values(dt)
        assert e.dtype == dt and len(set(M.bits(e).tolist())) == len(e)          # distinct bit patterns, NaNs included
        assert np.isnan(e).sum() >= 8 and np.isinf(e).sum() >= 2
        tiny = np.finfo(dt).tiny
        assert ((np.abs(e) < tiny) & (e != 0)).sum() >= 4                        # subnormals of the format itself
        assert M.bits(M.canon(e)).dtype == u
    assert M.to_u8(np.array([0, 0.5, 1, 1.9, 2, 254.999, 255])).tolist() == [0, 0, 1, 1, 2, 254, 255]
    assert M.to_u8(np.array([255.99], dtype=np.float32)).tolist() == [255]
    for bad in (-0.5, 256.0, np.nan, np.inf, -1.0):
        with pytest.raises(ValueError):
            M.to_u8(np.array([1.0, bad]))


def test_frame_bytes_are_the_reference_dump():
    """the frames of the committed reference dump, widened and put through frame_bytes, are the dump again: file order,
    C order, and narrowing that undoes widening"""
    meta, arr = load_golden("g4_layout_8x6x4")
    shape = (meta["steps"], meta["D"] + 2, meta["H"] + 2, meta["W"] + 2)
    frames = {fn: arr[fn].view(np.float32).reshape(shape) for fn in M.FILES}
    out = {fn: b"" for fn in M.FILES}
    for s in range(meta["steps"]):
        for fn, b in zip(M.FILES, M.frame_bytes([M.widen(frames[fn][s]) for fn in M.FILES])):
            out[fn] += b
    for fn in M.FILES:
        assert out[fn] == arr[fn].tobytes(), fn
    # a transposed field or a swapped pair of files is another dump
    one = [frames[fn][-1] for fn in M.FILES]
    assert M.frame_bytes(one)[2] != M.frame_bytes([one[0], one[1], one[3], one[2], one[4]])[2]
    assert M.frame_bytes(one)[2] != np.ascontiguousarray(one[2].transpose(2, 1, 0)).tobytes()


def test_stats_model():
    a = np.array([[3.0, -7.0], [np.nan, 2.5]])
    s, lo, hi = M.stats(a)
    assert math.isnan(s) and (lo, hi) == (-7.0, 3.0)
    assert M.stats(np.full(5, np.inf, dtype=np.float32)) == (math.inf, math.inf, math.inf)
    assert M.stats(np.full(3, 1e305)) == (3 * 1e305, 1e305, 1e305)
    assert M.stats(np.arange(-4, 5, dtype=np.float32)) == (0.0, -4.0, 4.0)
