"""fs_set_int "z_alternate" (-1 auto, 0, 1): a three-sweep pass that follows an upward pass of the same solve marches from plane D down to plane 1
(jacobi_fused_kernel's ZREV form), so that it starts on the planes the Infinity Cache still holds.  Nothing may change: one
handle runs with z_alternate = 0 (the launches as they were), another with 1, on the same inputs, and every field is compared
byte for byte, ghost cells included.  fs_get_int "reversed_passes" says how many passes ran downward, so that a case which
silently ran upward is not taken for a pass.

What can go wrong in the reversed form and what here would show it: the order of the two z neighbours in the stencil sum (last-bit
differences on random fields, every case), the two ghost-plane stores and face4 on b = 3 (diffuse with b = 3, ghost planes are
compared), the kill bytes of a mirrored plane (masks that differ between the two z ends), the mask-free plan of the mirrored
clean table (mask_free = 1 with those masks, three z chunks with interior seams), the alternation itself (pass lists of one to
26 three-sweep passes with each kind of remainder)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

# rows of two waves have the reversed builds; rows of one wave (256 cells) and ragged rows have none and must run upward.
# pair_zc = 5 cuts D = 13 / 10 / 9 into three / two z chunks with interior seams.
GRIDS = [(512, 28, 13), (256, 20, 10)]
RAGGED = (70, 18, 9)
# sweeps per solve -> its passes: 3 / 3+1 / 3+2 / 3+3 / 3+3+3 / 26 x 3 + 2; a pass runs downward iff it has three sweeps and the
# pass before it in the solve ran upward: up, down, up, down, ...
REVERSED = {3: 0, 4: 0, 5: 0, 6: 1, 9: 1, 80: 13}


@pytest.fixture(scope="module")
def F():
    import fluid_simulation_amd as F
    return F


def _masks(W, H, D):
    """Obstacles that differ between the two z ends (a mirrored kill byte or plan shows), one per hazard."""
    none = np.zeros((D + 2, H + 2, W + 2), dtype=bool)
    out = {}
    m = none.copy()
    m[1, H // 2, W // 3] = True                                  # a solid cell at plane 1 only
    out["cell_z1"] = m
    m = none.copy()
    m[D, 3:H - 2, W // 4:W // 2] = True                          # a plate one plane thick at plane D
    out["plate_zD"] = m
    if W == 512:
        z, y, x = np.ogrid[0:D + 2, 0:H + 2, 0:W + 2]            # a ball across the seam between the row's two waves, low in z
        out["ball_seam_z3"] = ((x - 256.5) ** 2 + (y - H / 2.0) ** 2 + (z - 3.0) ** 2) <= 16.0
        out["ball_seam_z3"][0] = out["ball_seam_z3"][D + 1] = False
    m = none.copy()
    m[D // 2 - 1, 1:H // 2, W // 4:W // 2] = True                # a plate that touches the y = 1 wall, off the middle plane
    out["plate_y1"] = m
    return out


def _inputs(W, H, D):
    rng = np.random.default_rng(W * 1000 + H + 7)
    return [rng.standard_normal((D + 2, H + 2, W + 2)).astype(np.float32) for _ in range(5)]


def _handle(F, W, H, D, z_alternate, mask_free, **opts):
    # diff / visc large enough that the neighbour sum carries weight in a diffusion solve (a = dt * diff * W * H * D ~ 0.1 .. 1)
    s = F.Simulation(W, H, D, 1, acc=5, diff=1.0e-4, visc=1.0e-4, quiet=1, sweep_fuse="4", pair_zc=5, mask_free=mask_free, **opts)
    s.z_alternate = z_alternate
    return s


def _same(F, fields, a, b, what):
    for f, x, y in zip(fields, a, b):
        assert x.tobytes() == y.tobytes(), "%s: %s differs" % (what, F.FIELD_NAMES[f])


def _solves(F, sims, W, H, D, mask_free, has_build):
    vx, vy, vz, q, junk = _inputs(W, H, D)
    fields = (F.PRESSURE, F.DIVERGENCE, F.VX, F.VY, F.VZ, F.DENS)
    for s in sims:
        s.project()                                  # the launch plans are chosen in the first solve
        assert s._geti("reversed_passes") == 0       # acc = 5: one three-sweep pass
    taken = 0
    for name, m in _masks(W, H, D).items():          # (the mask changes between solves of one handle)
        for acc, n in REVERSED.items():
            out = []
            for s in sims:
                s.set_mask(m)
                s.acc = acc
                for f, a in ((F.VX, vx), (F.VY, vy), (F.VZ, vz), (F.DENS, q), (F.PRESSURE, junk)):
                    s.set(f, a)
                s.diffuse(1, F.VX, F.DENS)
                s.diffuse(2, F.VY, F.DENS)
                s.diffuse(3, F.VZ, F.DENS)
                s.project()
                out.append([s.get(f) for f in fields])
            _same(F, fields, out[0], out[1], "%dx%dx%d %s acc %d mask_free %s" % (W, H, D, name, acc, mask_free))
            taken += 4 * n if has_build else 0
            assert sims[0]._geti("reversed_passes") == 0
            assert sims[1]._geti("reversed_passes") == taken, (name, acc)


@pytest.mark.parametrize("mask_free", ["0", "1"])
@pytest.mark.parametrize("W,H,D", GRIDS)
def test_solves_are_byte_identical_with_and_without_z_alternate(F, W, H, D, mask_free):
    sims = [_handle(F, W, H, D, v, mask_free) for v in (0, 1)]
    _solves(F, sims, W, H, D, mask_free, has_build=(W == 512))
    for s in sims:
        s.close()


@pytest.mark.parametrize("mask_free", ["0", "1"])
@pytest.mark.parametrize("W,H,D", GRIDS)
def test_steps_are_byte_identical_with_and_without_z_alternate(F, W, H, D, mask_free):
    """Two whole steps at acc = 80 and at acc = 9: every field of the handle."""
    m = _masks(W, H, D)["plate_zD"] | _masks(W, H, D)["cell_z1"]
    for acc in (80, 9):
        out, counts = [], []
        for v in (0, 1):
            s = _handle(F, W, H, D, v, mask_free)
            s.set_mask(m)
            s.acc = acc
            s.run_one()
            s.run_one()
            out.append([s.get(f) for f in range(11)])
            counts.append(s._geti("reversed_passes"))
            s.close()
        _same(F, range(11), out[0], out[1], "%dx%dx%d two steps acc %d mask_free %s" % (W, H, D, acc, mask_free))
        assert counts[0] == 0
        if W == 512:
            assert counts[1] > 0 and counts[1] % REVERSED[acc] == 0, counts      # every solve of a step alternates alike
        else:
            assert counts[1] == 0


def test_ragged_rows_and_small_grids_run_upward(F):
    W, H, D = RAGGED
    sims = [_handle(F, W, H, D, v, "1") for v in (0, 1)]
    _solves(F, sims, W, H, D, "1", has_build=False)
    for s in sims:
        s.close()
    # auto: only where the three arrays of a pass outgrow the Infinity Cache
    W, H, D = GRIDS[0]
    s = _handle(F, W, H, D, -1, "1")
    s.acc = 80
    s.project()
    assert s._geti("reversed_passes") == 0
    s.close()


def test_z_alternate_values(F):
    sim = F.Simulation(64, 16, 16, 1, quiet=1)
    assert sim.z_alternate == -1
    for v in (0, 1, -1):
        sim.z_alternate = v
        assert sim.z_alternate == v
    for v in (2, -2):
        with pytest.raises(Exception):
            sim.z_alternate = v
    assert sim.z_alternate == -1
    assert sim._geti("reversed_passes") == 0
    sim.close()
