"""The six per-step logs (force_log, body_force_log, residual_log, probe_log, image_log, tracer_log) as rings: a handle
whose ring holds `cap` records must return, after k steps, exactly the last min(k, cap) records that a handle with a ring
too large to wrap returns for the same run -- rows, step numbers and the dropped count, bit for bit -- whatever k is:
0, 1, cap, cap + 1 and 2 cap + 2 between fetches are the points where the first retained slot, the length of the first
run and the presence of a second run change.  A size-only query reports the same counts and drains nothing; a second
fetch finds the ring empty.  16 x 8 x 8 with one block is the smallest grid on which every log has more than one plane
record and the obstacle touches fluid on all sides."""
import ctypes as Ct

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
W, H, D = 16, 8, 8
LOGS = ["force_log", "body_force_log", "residual_log", "probe_log", "image_log", "tracer_log"]
NEVER_WRAPS = 16


def handle(log, cap):
    """the seeded run with `log` at `cap` records"""
    import fluid_simulation_amd as F
    kw = {log: cap}
    if log == "tracer_log":
        kw["tracers"] = 8
    sim = F.Simulation(W, H, D, 1, speed=1, acc=4, quiet=1, dump_every=0, **kw)   # speed 1: under a cell per step
    rng = np.random.default_rng(2024)
    full = (D + 2, H + 2, W + 2)
    obs = np.zeros(full, dtype=np.float32)
    obs[3:6, 3:6, 6:10] = 1.0                                  # one block, fluid on all six sides
    sim.set(F.OBS, obs)
    sim.set(F.DENS, (rng.random(full) * 0.01).astype(np.float32))
    for which in (F.VX, F.VY, F.VZ):
        sim.set(which, (rng.standard_normal(full) * 0.5).astype(np.float32))
    if log == "probe_log":
        sim.set_probes([(3, 4, 4), (12, 5, 2)])
    if log == "image_log":
        sim.set_image_views([(F.DENS, "slice", 2, (D + 2) // 2, 0.0, 0.01, 0.2)])
    if log == "tracer_log":
        sim.tracer_seed([(1.0, 1.5, 1.5), (1.5, 7.0, 2.0), (2.0, 2.0, 7.0)])   # upstream, clear of the block
    return sim


def sizes(sim, log):
    """(records, dropped) of a size-only query; a record is what one ring slot holds"""
    n, dropped = Ct.c_long(-1), Ct.c_long(-1)
    L, h = sim._L, sim._h
    if log == "image_log":
        rc = L.fs_image_log(h, None, None, 0, Ct.byref(n), Ct.byref(dropped))
    elif log == "tracer_log":
        rc = L.fs_tracer_log(h, None, None, None, 0, Ct.byref(n), Ct.byref(dropped))
    else:
        rc = getattr(L, "fs_" + log)(h, None, 0, Ct.byref(n), Ct.byref(dropped))
    assert rc == 0
    if log == "body_force_log":                                # B + 1 rows per record
        per = sim.body_count + 1
        assert n.value % per == 0
        return n.value // per, dropped.value
    return n.value, dropped.value


def fetch(sim, log):
    """(step of each record, bytes of each record without its step, dropped), oldest first"""
    if log in ("force_log", "residual_log", "body_force_log"):
        rows, dropped = getattr(sim, log)(with_dropped=True)
        per = sim.body_count + 1 if log == "body_force_log" else 1
        rows = rows.reshape(-1, per)
        steps = [int(r["step"][0]) for r in rows]
        assert all((r["step"] == r["step"][0]).all() for r in rows)
        blank = rows.copy()
        blank["step"] = 0
        return steps, [r.tobytes() for r in blank], dropped
    if log == "probe_log":
        rec, dropped = sim.probe_log(with_dropped=True)
        return rec["step"].tolist(), [v.tobytes() for v in rec["values"]], dropped
    if log == "image_log":
        steps, images, dropped = sim.image_log(with_dropped=True)
        return steps.tolist(), [f.tobytes() for f in images[0]], dropped
    rec, dropped = sim.tracer_log(with_dropped=True)
    return rec["step"].tolist(), [x.tobytes() + s.tobytes() for x, s in zip(rec["xyz"], rec["status"])], dropped


@pytest.mark.parametrize("cap", [1, 3])
@pytest.mark.parametrize("log", LOGS)
def test_ring_returns_the_last_records_of_an_unwrapped_log(log, cap):
    a, b = handle(log, cap), handle(log, NEVER_WRAPS)
    seen = set()
    for k in (0, 1, cap, cap + 1, 2 * cap + 2):
        for _ in range(k):
            a.run_one()
            b.run_one()
        keep = min(k, cap)
        assert sizes(a, log) == (keep, k - keep), k
        assert sizes(a, log) == (keep, k - keep), k           # the query drained nothing
        steps_a, rows_a, dropped_a = fetch(a, log)
        assert sizes(b, log) == (k, 0), k
        steps_b, rows_b, dropped_b = fetch(b, log)
        assert len(rows_b) == k and dropped_b == 0, k
        assert steps_b == list(range(steps_b[0], steps_b[0] + k)) if k else steps_b == []
        assert dropped_a == k - keep, k
        assert steps_a == steps_b[k - keep:], k
        assert rows_a == rows_b[k - keep:], k
        assert fetch(a, log) == ([], [], 0), k                # drained
        assert sizes(a, log) == (0, 0), k
        seen.update(rows_b)
    # the records of different steps differ, so a record from the wrong slot would not have passed
    assert len(seen) == 4 * cap + 4
    a.close()
    b.close()
