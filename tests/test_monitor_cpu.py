"""The numpy restatement of the flow monitor (tests/monitor_model.py) against the header's text as scalar loops, and the
properties the header promises: counts that agree between the three records, non-finite values that are counted and never
become an extremum, ghost and solid cells that contribute nothing.  No GPU."""
import numpy as np
import pytest

import monitor_model as M


def fields(rng, W, H, D, dtype=np.float32, solid=0.25):
    shape = (D + 2, H + 2, W + 2)
    f = [rng.standard_normal(shape).astype(dtype) for _ in range(5)]
    obs = np.zeros(shape, dtype=dtype)
    obs[1:-1, 1:-1, 1:-1] = rng.random((D, H, W)) < solid
    return f, obs


def same(a, b):
    return all(np.array_equal(x, y, equal_nan=True) for x, y in zip(a, b))


@pytest.mark.parametrize("W,H,D", [(1, 1, 1), (3, 2, 1), (5, 4, 3), (2, 7, 2)])
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_model_is_the_naive_triple_loop(W, H, D, dtype):
    rng = np.random.default_rng(W * 100 + H * 10 + D)
    f, obs = fields(rng, W, H, D, dtype)
    assert same(M.monitor(*f, obs), M.naive(*f, obs))
    # and with non-finite values about
    f[1][1, 1, 1] = np.nan
    f[4][D, H, W] = np.inf
    f[0][1, H, 1] = -np.inf
    assert same(M.monitor(*f, obs), M.naive(*f, obs))


def test_counts_agree_between_the_records():
    rng = np.random.default_rng(7)
    f, obs = fields(rng, 9, 5, 4)
    whole, planes, profile = M.monitor(*f, obs)
    fluid = int((obs[1:-1, 1:-1, 1:-1] != 1).sum())
    assert whole[0] == fluid == planes[:, 0].sum() == profile[:, 0].sum()
    assert whole[1] == 0
    # each sum is near the plain numpy sum over the target cells (the order differs, the value hardly)
    t = obs[1:-1, 1:-1, 1:-1] != 1
    for k, a in ((2, f[0]), (3, f[1]), (4, f[2]), (5, f[3]), (7, f[4])):
        assert whole[k] == pytest.approx(a[1:-1, 1:-1, 1:-1].astype(np.float64)[t].sum(), rel=1e-12, abs=1e-12)
    assert whole[8] == np.abs(f[1][1:-1, 1:-1, 1:-1].astype(np.float64)[t]).max()
    assert whole[12] == f[0][1:-1, 1:-1, 1:-1].astype(np.float64)[t].min()
    assert whole[15] == f[4][1:-1, 1:-1, 1:-1].astype(np.float64)[t].max()
    assert profile[:, 1].sum() == pytest.approx(whole[3], rel=1e-12, abs=1e-12)


@pytest.mark.parametrize("bad", [np.nan, np.inf, -np.inf])
@pytest.mark.parametrize("field", range(5))
def test_nonfinite_in_a_target_cell_is_counted_and_no_maximum(bad, field):
    rng = np.random.default_rng(11)
    f, obs = fields(rng, 6, 4, 3, solid=0.0)
    clean = M.monitor(*f, obs)
    f[field][2, 3, 4] = bad
    whole, planes, profile = M.monitor(*f, obs)
    assert whole[1] == 1 and planes[1, 1] == 1 and planes[0, 1] == 0 and whole[0] == clean[0][0]
    if np.isnan(bad):
        # a NaN never replaces a running value: every extremum is finite
        assert np.all(np.isfinite(whole[8:])) and np.all(np.isfinite(planes[:, 8:]))
    elif field in (0, 4):
        # an infinite q or p leaves the four maxima finite and is the extremum of its own field, as the comparisons order it
        assert np.all(np.isfinite(whole[8:12]))
        assert whole[(12 if field == 0 else 14) + (bad > 0)] == bad
    else:
        # an infinite velocity is ordered too: "if (a > m) m = a" takes |.| = +Inf, and e with it; nothing becomes NaN
        assert whole[8 + field - 1] == np.inf and whole[11] == np.inf and not np.any(np.isnan(whole[8:]))
    # the planes without the cell keep their bits
    assert np.array_equal(planes[[0, 2]], clean[1][[0, 2]])


def test_nan_in_solid_and_ghost_cells_changes_nothing():
    rng = np.random.default_rng(13)
    f, obs = fields(rng, 7, 5, 3)
    clean = M.monitor(*f, obs)
    solid = np.argwhere(obs == 1)
    assert len(solid) > 3
    for a in f:
        for z, y, x in solid:
            a[z, y, x] = np.nan
        a[0], a[-1], a[:, 0], a[:, -1], a[:, :, 0], a[:, :, -1] = np.nan, np.inf, np.nan, -np.inf, np.nan, np.nan
    assert same(M.monitor(*f, obs), clean)


def test_empty_set():
    rng = np.random.default_rng(17)
    f, obs = fields(rng, 4, 3, 2)
    obs[1, 1:-1, 1:-1] = 1                                   # plane 1 all solid
    whole, planes, profile = M.monitor(*f, obs)
    assert np.array_equal(planes[0], [0.0] * 12 + [np.inf, -np.inf, np.inf, -np.inf])
    obs[1:-1, 1:-1, 1:-1] = 1
    whole, planes, profile = M.monitor(*f, obs)
    assert np.array_equal(whole, [0.0] * 12 + [np.inf, -np.inf, np.inf, -np.inf]) and not profile.any()


def test_log_row_and_cfl():
    rng = np.random.default_rng(19)
    f, obs = fields(rng, 5, 3, 2)
    whole, planes, profile = M.monitor(*f, obs)
    row = M.log_row(3, whole, profile, [2, 5])
    assert row.shape == (57,) and row[0] == 3 and np.array_equal(row[1:17], whole)
    assert np.array_equal(row[17:22], profile[1]) and np.array_equal(row[22:27], profile[4]) and np.all(np.isnan(row[27:]))
    dt = 0.05
    assert M.cfl(dt, (5, 3, 2), whole) == ((float(np.float32(dt)) * 5) * whole[8], (float(np.float32(dt)) * 3) * whole[9],
                                           (float(np.float32(dt)) * 2) * whole[10])
