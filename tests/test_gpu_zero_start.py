"""Option "zero_start": where the pressure solve of a projection starts with the three-sweep kernel in a lane-aligned fp32
whole-domain build, the divergence pass does not write p = 0 and that first pass takes level 0 as constants instead of
reading it.  Nothing may change: one handle runs with zero_start = 0 (the launches as they were), another with 1, on the
same inputs, and every field is compared bit for bit, ghost cells included.  fs_get_int "zero_start_projections" says
which path a projection took, so the fallbacks (ragged rows, acc < 3, the residual log) are seen to be fallbacks."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

# rows of one and two waves (lane-aligned), three or more bands with both y-wall bands, one z chunk whose first and last
# groups touch the z walls around at least one interior group; 70-cell rows are ragged: no zero-start build, must fall back
GRIDS = [(256, 20, 10), (512, 28, 13), (70, 18, 9)]
ACCS = (3, 5, 80, 2)                         # acc = 2 plans no three-sweep pass: must fall back


@pytest.fixture(scope="module")
def F():
    import fluid_simulation_amd as F
    return F


def _masks(W, H, D):
    out = {"none": np.zeros((D + 2, H + 2, W + 2), dtype=bool)}
    m = out["none"].copy()
    m[D // 2, H // 2, 1] = True                                  # one-cell solids in the first and the last column
    m[D // 2 + 1, H // 2 + 2, W] = True
    out["x_walls"] = m
    m = out["none"].copy()
    m[D // 2, 1:H // 2, W // 4:W // 2] = True                    # a plate one plane thick that touches the y = 1 wall
    out["plate_y1"] = m
    if W == 512:
        z, y, x = np.ogrid[0:D + 2, 0:H + 2, 0:W + 2]            # a ball across the seam between the row's two waves
        out["ball_seam"] = ((x - 256.5) ** 2 + (y - H / 2.0) ** 2 + (z - D / 2.0) ** 2) <= 16.0
    return out


def _inputs(W, H, D):
    rng = np.random.default_rng(W * 1000 + H)
    return [rng.standard_normal((D + 2, H + 2, W + 2)).astype(np.float32) for _ in range(4)]


def _handle(F, W, H, D, zero_start, mask_free, **opts):
    return F.Simulation(W, H, D, 1, acc=5, quiet=1, sweep_fuse="4", zero_start=zero_start, mask_free=mask_free, **opts)


@pytest.mark.parametrize("mask_free", ["0", "1"])
@pytest.mark.parametrize("W,H,D", GRIDS)
def test_project_is_bit_identical_with_and_without_zero_start(F, W, H, D, mask_free):
    vx, vy, vz, junk = _inputs(W, H, D)
    sims = [_handle(F, W, H, D, v, mask_free) for v in ("0", "1")]
    fields = (F.PRESSURE, F.DIVERGENCE, F.VX, F.VY, F.VZ)
    aligned = W in (256, 512)
    taken = 0
    for s in sims:
        s.project()                              # the launch plans are chosen in the first solve; zero start needs them chosen
        assert s._geti("zero_start_projections") == 0
    for name, m in _masks(W, H, D).items():
        for acc in ACCS:
            out = []
            for s in sims:
                s.set_mask(m)
                s.acc = acc
                for f, a in ((F.VX, vx), (F.VY, vy), (F.VZ, vz), (F.PRESSURE, junk)):   # p holds junk: it must not be read
                    s.set(f, a)
                s.project()
                out.append([s.get(f) for f in fields])
            for f, a, b in zip(fields, out[0], out[1]):
                assert a.tobytes() == b.tobytes(), "%dx%dx%d %s acc %d mask_free %s: %s" % (W, H, D, name, acc, mask_free,
                                                                                             F.FIELD_NAMES[f])
            taken += 1 if (aligned and acc >= 3) else 0
            assert sims[0]._geti("zero_start_projections") == 0
            assert sims[1]._geti("zero_start_projections") == taken, (name, acc)
    for s in sims:
        s.close()


@pytest.mark.parametrize("W,H,D", GRIDS[:2])
def test_residual_log_forces_the_fallback(F, W, H, D):
    """The log's "before" record of a pressure solve reads p ahead of the solve: with the log on, p is zeroed in memory as
    before and the records are those of zero_start = 0."""
    m = _masks(W, H, D)["plate_y1"]
    logs, fields, counts = [], [], []
    for v in ("0", "1"):
        s = _handle(F, W, H, D, v, "auto", residual_log=4)
        s.set_mask(m)
        for _ in range(2):
            s.run_one()
        logs.append(s.residual_log())
        fields.append([s.get(f) for f in range(11)])
        counts.append(s._geti("zero_start_projections"))
        s.set_option("residual_log", 0)          # log off: the same handle now takes the zero start, two projections per step
        s.run_one()
        counts.append(s._geti("zero_start_projections"))
        fields[-1] += [s.get(f) for f in range(11)]
        s.close()
    assert len(logs[0]) == 2 and logs[0].tobytes() == logs[1].tobytes()
    for f, (a, b) in enumerate(zip(fields[0], fields[1])):
        assert a.tobytes() == b.tobytes(), f
    assert counts == [0, 0, 0, 2]


def test_zero_start_option_values(F):
    sim = F.Simulation(64, 16, 16, 1, quiet=1)
    for k in ("zero_start", "fuse_project_advect"):
        for v in ("0", "auto", "1"):
            sim.set_option(k, v)
        with pytest.raises(Exception):
            sim.set_option(k, "2")
    sim.close()
