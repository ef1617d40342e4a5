"""The arithmetic of the inflow generator (csrc/inflow.h), on the host: a driver compiled with the host C++ compiler and the
library's -ffp-contract=off runs exactly the inline functions the two kernels call -- the plane the way the plane kernel
does it, 16 x 16 patches that keep the eddies inflow_touches lets through -- and every output is compared bit for bit
with the numpy restatement of include/fluidsim.h (tests/inflow_model.py).  Also: properties and statistics of the model,
the header's includes, the prototypes, and the Python helpers against closed forms."""
import itertools
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import inflow_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "fluid_simulation_amd", "csrc")
HEADER = os.path.join(ROOT, "include", "fluidsim.h")

# stdin, per case one line: "C seed n h d sigma c u_rms t speed gust plane hasU hasR" (reals as fp64 bit patterns, plane = 0:
# the eddies only) followed by the h*d values of U and of r where given; or "G t n" followed by n knots (step, factor).
# stdout per C case: a line "amp", n lines "ex ey ez gen neg", then where plane != 0 one line of 3*h*d values; per G case g(t).
DRIVER = r'''
#include "inflow.h"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
using namespace fs;
static double rd() { unsigned long long b; if (std::scanf("%llx", &b) != 1) std::exit(3); double v; std::memcpy(&v, &b, 8); return v; }
static void put(double v) { unsigned long long b; std::memcpy(&b, &v, 8); std::printf("%016llx ", b); }
int main()
{
    static_assert(sizeof(InflowEntry) == 32 && alignof(InflowEntry) == 16, "two 16-byte loads per entry");
    char cmd[4];
    while (std::scanf("%3s", cmd) == 1) {
        if (cmd[0] == 'G') {
            long t; int n;
            if (std::scanf("%ld %d", &t, &n) != 2) return 2;
            std::vector<double> ts(n), fs_(n);
            for (int i = 0; i < n; ++i) { ts[i] = rd(); fs_[i] = rd(); }
            put(inflow_gust(ts.data(), fs_.data(), n, t));
            std::printf("\n");
            continue;
        }
        InflowParams p;
        unsigned long long seed; long t; int plane, hasU, hasR;
        if (std::scanf("%llu %d %d %d", &seed, &p.n, &p.h, &p.d) != 4) return 2;
        p.seed = seed;
        p.sigma = rd(); p.convect = rd();
        const double urms = rd();
        if (std::scanf("%ld", &t) != 1) return 2;
        const double speed = rd(), gust = rd();
        if (std::scanf("%d %d %d", &plane, &hasU, &hasR) != 3) return 2;
        const size_t cells = (size_t)p.h * p.d;
        std::vector<double> U(hasU ? cells : 0), R(hasR ? cells : 0);
        for (double& v : U) v = rd();
        for (double& v : R) v = rd();
        p.amp = inflow_amplitude(p.n, p.h, p.d, p.sigma, urms);
        if (!inflow_step_ok(t, p.sigma, p.convect)) return 4;
        put(p.amp); std::printf("\n");
        const double inv = 1.0 / p.sigma;
        std::vector<InflowEntry> tab(p.n);
        for (int k = 0; k < p.n; ++k) {
            const InflowEddy e = inflow_eddy(p, k, t);
            tab[k] = inflow_entry(e, p.amp, inv);
            put(e.ex); put(e.ey); put(e.ez); put(e.gen); std::printf("%u\n", e.neg);
        }
        if (!plane) continue;
        std::vector<double> out(3 * cells);
        const int P = 16;
        for (int z0 = 1; z0 <= p.d; z0 += P)
            for (int y0 = 1; y0 <= p.h; y0 += P) {
                const int y1 = y0 + P - 1 < p.h ? y0 + P - 1 : p.h, z1 = z0 + P - 1 < p.d ? z0 + P - 1 : p.d;
                std::vector<InflowEntry> list;
                for (int k = 0; k < p.n; ++k)
                    if (inflow_touches(tab[k], p.sigma, (double)y0, (double)y1, (double)z0, (double)z1)) list.push_back(tab[k]);
                for (int z = z0; z <= z1; ++z)
                    for (int y = y0; y <= y1; ++y) {
                        double u[3] = { 0.0, 0.0, 0.0 }, o[3];
                        for (const InflowEntry& q : list) inflow_accumulate(u, q, inflow_pair(q, (double)y, (double)z, inv));
                        const size_t i = (size_t)(z - 1) * p.h + (y - 1);
                        inflow_compose(o, gust, hasU ? U[i] : speed, hasR ? R[i] : 1.0, u);
                        for (int j = 0; j < 3; ++j) out[j * cells + i] = o[j];
                    }
            }
        for (double v : out) put(v);
        std::printf("\n");
    }
    return 0;
}
'''

SIGMAS = [1.0, 2.5, 8.0, 40.0]                       # 40: larger than every plane
CONVECTS = [0.0, 0.3, 7.75, 1000.5]                  # frozen, slow, crossing a rebirth, many rebirths per step
STEPS = [0, 1, 17, 10 ** 6]
COUNTS = [1, 63, 64, 65, 257, 1000]
PLANES = [(1, 1), (3, 2), (7, 5), (65, 3)]


def bits(x):
    return "%016x" % int(np.float64(x).view(np.uint64))


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++")
    if cxx is None:
        pytest.fail("no C++ compiler")
    d = tmp_path_factory.mktemp("inflow_driver")
    src = d / "driver.cpp"
    src.write_text(DRIVER)
    exe = d / "driver"
    subprocess.run([cxx, "-std=c++17", "-O2", "-Wall", "-Werror", "-ffp-contract=off", "-I", CSRC, str(src), "-o", str(exe)], check=True)

    def run(cases, exe=exe):
        """cases: dicts with p (M.Params), t, and optionally speed, gust (a factor), plane, U, r -> per case a dict"""
        lines = []
        for c in cases:
            p = c["p"]
            U, r = c.get("U"), c.get("r")
            words = ["C", str(p.seed), str(p.n), str(p.h), str(p.d), bits(p.sigma), bits(p.convect), bits(p.u_rms), str(c["t"]),
                     bits(c.get("speed", 0.0)), bits(c.get("gust", 1.0)), "1" if c.get("plane") else "0", "01"[U is not None],
                     "01"[r is not None]]
            for m in (U, r):
                if m is not None:
                    words += [bits(v) for v in np.asarray(m, dtype=np.float64).reshape(-1)]
            lines.append(" ".join(words))
        out = subprocess.run([str(exe)], input="\n".join(lines) + "\n", capture_output=True, text=True, check=True).stdout.splitlines()
        res, at = [], 0
        for c in cases:
            p = c["p"]
            amp = np.array([int(out[at].split()[0], 16)], dtype=np.uint64).view(np.float64)[0]
            rows = [ln.split() for ln in out[at + 1:at + 1 + p.n]]
            at += 1 + p.n
            e = np.array([[int(w, 16) for w in r[:4]] for r in rows], dtype=np.uint64).reshape(p.n, 4).view(np.float64)
            neg = np.array([int(r[4]) for r in rows], dtype=np.int64)
            got = {"amp": amp, "ex": e[:, 0], "ey": e[:, 1], "ez": e[:, 2], "gen": e[:, 3],
                   "sign": np.stack([np.where((neg >> j) & 1, -1.0, 1.0) for j in range(3)], axis=-1).reshape(p.n, 3)}
            if c.get("plane"):
                got["plane"] = np.array([int(w, 16) for w in out[at].split()], dtype=np.uint64).view(np.float64).reshape(3, p.d, p.h)
                at += 1
            res.append(got)
        assert at == len(out)
        return res

    run.exe, run.cxx, run.source, run.dir = str(exe), cxx, src, d
    return run


def same(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def test_driver_eddies_match_the_model_on_the_whole_grid(driver):
    """hash, positions, generations and signs: sigma x c x t x N, the plane cycling"""
    cases = []
    for i, (sg, c, t, n) in enumerate(itertools.product(SIGMAS, CONVECTS, STEPS, COUNTS)):
        h, d = PLANES[i % 4]
        cases.append({"p": M.Params(0x9E3779B97F4A7C15 * (i + 1), n, h, d, sg, c, 0.75), "t": t})
    for c, got in zip(cases, driver(cases)):
        want = M.eddies(c["p"], c["t"])
        assert same(got["amp"], c["p"].amp)
        for key in ("ex", "ey", "ez", "gen", "sign"):
            assert same(got[key], want[key]), (key, vars(c["p"]), c["t"])


def test_driver_plane_matches_the_model(driver):
    """the plane through patch culling, with maps that hold +-0, huge and tiny values, a gust factor; every sigma x c x t, the
    counts and planes cycling so that each sigma meets each of them"""
    rng = np.random.default_rng(20061)
    cases = []
    for i, (sg, c, t) in enumerate(itertools.product(SIGMAS, CONVECTS, STEPS)):
        n = COUNTS[(i + i // 16) % 6]
        h, d = PLANES[(i + i // 4) % 4]
        U = rng.standard_normal((d, h)) * 10.0 ** rng.integers(-30, 30, size=(d, h))
        r = rng.standard_normal((d, h)) * 10.0 ** rng.integers(-30, 30, size=(d, h))
        U.flat[rng.integers(0, U.size)] = -0.0
        r.flat[rng.integers(0, r.size)] = 0.0 if i % 2 else -0.0
        kind = i % 3                                        # both maps, none, the mean only
        cases.append({"p": M.Params(1000 + i, n, h, d, sg, c, 1.5), "t": t, "plane": True, "speed": 30.0, "gust": 0.625 + 0.25 * (i % 5),
                      "U": U if kind != 1 else None, "r": r if kind == 0 else None})
    for c, got in zip(cases, driver(cases)):
        want = M.plane(c["p"], c["U"], c["r"], [(0, c["gust"])], c["t"], speed=30.0)
        assert same(got["plane"], want), (vars(c["p"]), c["t"])
        if c["p"].sigma == 40.0:                            # every eddy touches every cell
            assert np.all(got["plane"][1:] != 0.0) or c["r"] is not None


def test_driver_under_asan_and_ubsan(driver):
    """the same stand-alone host program with -fsanitize=address,undefined: planes of one and of several patches, sigma below
    and above the plane, one eddy and a thousand"""
    exe = driver.dir / "driver_san"
    subprocess.run([driver.cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-ffp-contract=off", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-I", CSRC, str(driver.source), "-o", str(exe)], check=True)
    rng = np.random.default_rng(5)
    cases = []
    for i, ((h, d), sg, n) in enumerate(itertools.product([(1, 1), (65, 3), (33, 40)], [1.0, 40.0], [1, 1000])):
        cases.append({"p": M.Params(i, n, h, d, sg, 7.75, 1.5), "t": 17 + i, "plane": True, "speed": 30.0, "gust": 1.25,
                      "U": rng.standard_normal((d, h)) if i % 2 else None, "r": rng.standard_normal((d, h)) if i % 3 else None})
    for c, got in zip(cases, driver(cases, exe=exe)):
        assert same(got["plane"], M.plane(c["p"], c["U"], c["r"], [(0, 1.25)], c["t"], speed=30.0)), vars(c["p"])


def test_gust_factor_at_between_and_outside_the_knots(driver):
    knots = [(3.0, 0.5), (4.0, 2.0), (10.0, -1.0), (1000.0, 1.0e-3)]
    assert M.gust_factor(None, 7) == 1.0 and M.gust_factor([], 7) == 1.0
    assert M.gust_factor(knots, 0) == 0.5 and M.gust_factor(knots, 3) == 0.5 and M.gust_factor(knots, 4) == 2.0
    assert M.gust_factor(knots, 7) == 0.5 and M.gust_factor(knots, 1000) == 1.0e-3 and M.gust_factor(knots, 10 ** 9) == 1.0e-3
    assert M.gust_factor(knots, 5) == np.float64(2.0) + np.float64(-3.0) * (np.float64(1.0) / np.float64(6.0))
    text = ""
    steps = [0, 3, 4, 5, 6, 7, 9, 10, 11, 500, 999, 1000, 1001, 10 ** 9]
    for t in steps:
        text += "G %d %d %s\n" % (t, len(knots), " ".join(bits(a) + " " + bits(b) for a, b in knots))
    text += "G 5 0\n"
    out = subprocess.run([driver.exe], input=text, capture_output=True, text=True, check=True).stdout.split()
    got = np.array([int(w, 16) for w in out], dtype=np.uint64).view(np.float64)
    assert same(got, [M.gust_factor(knots, t) for t in steps] + [1.0])


# ---- properties of the model ------------------------------------------------------------------------------------------

def test_every_eddy_lies_in_the_box():
    for sg, c, t in itertools.product(SIGMAS, CONVECTS, STEPS + [123456789]):
        p = M.Params(7, 1000, 7, 5, sg, c, 1.0)
        e = M.eddies(p, t)
        lo = 1.0 - sg
        assert np.all(e["ex"] >= lo) and np.all(e["ex"] <= 1.0 + sg)          # closed above: (1 - sigma) + rem may round up to it
        assert np.all(e["ey"] >= lo) and np.all(e["ey"] <= 7 + sg) and np.all(e["ez"] >= lo) and np.all(e["ez"] <= 5 + sg)
        assert np.all(e["gen"] == np.floor(e["gen"])) and np.all(e["gen"] >= 0) and np.all(np.abs(e["sign"]) == 1.0)
    e = M.eddies(M.Params(7, 1000, 7, 5, 8.0, 0.3, 1.0), 17)                  # all of the box is used
    assert e["ex"].min() < -6.0 and e["ex"].max() > 8.0 and e["ey"].min() < -6.0 and e["ey"].max() > 14.0


def test_ex_advances_by_c_between_rebirths_and_a_rebirth_moves_the_eddy():
    p = M.Params(11, 257, 7, 5, 8.0, 0.3, 1.0)
    a, b = M.eddies(p, 100), M.eddies(p, 101)
    stay = a["gen"] == b["gen"]
    assert stay.sum() > 200 and (~stay).sum() >= 1
    # s = start + t * c is rounded at a magnitude below 64: two roundings of at most 2^-48 each, and ex one more
    assert np.all(np.abs((b["ex"][stay] - a["ex"][stay]) - 0.3) <= 3 * 2.0 ** -48)
    assert same(a["ey"][stay], b["ey"][stay]) and same(a["ez"][stay], b["ez"][stay]) and same(a["sign"][stay], b["sign"][stay])
    assert np.all(b["gen"][~stay] == a["gen"][~stay] + 1) and np.all(b["ex"][~stay] < a["ex"][~stay])
    assert np.all(a["ey"][~stay] != b["ey"][~stay]) and np.all(a["ez"][~stay] != b["ez"][~stay])
    frozen = M.Params(11, 257, 7, 5, 8.0, 0.0, 1.0)
    for key in ("ex", "ey", "ez", "sign"):
        assert same(M.eddies(frozen, 0)[key], M.eddies(frozen, 10 ** 6)[key])


def test_seeds_and_call_order():
    p1, p2 = M.Params(1, 257, 7, 5, 2.5, 7.75, 1.0), M.Params(2, 257, 7, 5, 2.5, 7.75, 1.0)
    first = {t: M.eddies(p1, t) for t in (17, 0, 5)}
    again = {t: M.eddies(p1, t) for t in (5, 17, 0)}
    for t in first:
        for key in first[t]:
            assert same(first[t][key], again[t][key])
    other = M.eddies(p2, 17)
    assert np.mean(first[17]["ey"] == other["ey"]) < 0.01 and np.mean(first[17]["ex"] == other["ex"]) < 0.01
    many = M.eddies(p1, np.array([0, 5, 17]))                                 # an array of steps is the same stream
    for i, t in enumerate((0, 5, 17)):
        for key in many:
            assert same(many[key][i], first[t][key])
    # the hash: no two of 2^16 eddies share a start, the uniforms fill [0, 1)
    u = M.uniform(M.hash64(1, np.arange(65536), np.zeros(65536, dtype=np.uint64), 0))
    assert len(np.unique(u)) == 65536 and u.min() >= 0.0 and u.max() < 1.0 and abs(u.mean() - 0.5) < 5 * np.sqrt(1 / 12 / 65536)


# ---- statistics of the model ------------------------------------------------------------------------------------------

def moments(x):
    """x (3, n) samples of the three components -> per check (value, standard error estimated from the sample)"""
    n = x.shape[1]
    mean = x.mean(axis=1)
    dev = x - mean[:, None]
    var = (dev * dev).mean(axis=1)
    out = {"mean": (mean, np.sqrt(var / n)), "var": (var, (dev * dev).std(axis=1) / np.sqrt(n))}
    pairs = [(0, 1), (0, 2), (1, 2)]
    prod = np.stack([dev[a] * dev[b] for a, b in pairs])
    out["cov"] = (prod.mean(axis=1), prod.std(axis=1) / np.sqrt(n))
    return out


def check_moments(x, u_rms):
    m = moments(x)
    ratios = {}
    val, se = m["mean"]
    assert np.all(np.abs(val) < 5 * se), (val, se)
    ratios["mean/se"] = np.abs(val / se).max()
    val, se = m["var"]
    assert np.all(5 * se < 0.05 * u_rms ** 2), se                             # the sample is large enough for a 5 % statement
    assert np.all(np.abs(val - u_rms ** 2) < 5 * se), (val, se)
    ratios["var/u_rms^2"] = val / u_rms ** 2
    ratios["(var-u_rms^2)/se"] = np.abs((val - u_rms ** 2) / se).max()
    val, se = m["cov"]
    assert np.all(np.abs(val) < 5 * se), (val, se)
    ratios["cov/se"] = np.abs(val / se).max()
    return ratios


def test_statistics_of_the_fluctuations():
    """c > 2 sigma: every eddy is reborn every step, so steps are independent samples of (ey, ez, signs); c is no multiple
    of 2 sigma, so that an eddy's ex also moves through the box from step to step (at c = 2 sigma every eddy would keep its
    ex for ever and the variance would be that of 128 fixed x factors).  Cells 2 sigma apart share no eddy.  sigma = 1 on a
    7 x 7 plane with N = V / sigma^3 = 128 eddies, u_rms = 1.5, 4000 steps x the 16 cells (1|3|5|7, 1|3|5|7) = 64000 samples
    per component.  Observed: variance / u_rms^2 = 1.0010, 1.0036, 0.9968 with 5 standard errors = 3.3 % of u_rms^2,
    |variance - u_rms^2| at most 0.56 standard errors, |mean| at most 0.79 and |covariance| at most 0.72 of theirs."""
    p = M.Params(2006, 128, 7, 7, 1.0, 2.7654321, 1.5)
    z, y = np.meshgrid([1, 3, 5, 7], [1, 3, 5, 7], indexing="ij")
    x = np.concatenate([M.fluctuation_at(p, t, y, z) for t in range(4000)], axis=1)
    assert x.shape == (3, 64000)
    print(check_moments(x, 1.5))


def test_statistics_at_a_corner_cell():
    """The same at the corner cell (1, 1) alone, where only the box's padding by sigma keeps the variance: 64000 steps,
    evaluated for all steps at once (the sum over the eddies still in ascending k).  Observed: variance / u_rms^2 = 0.9867,
    0.9964, 1.0048, 5 standard errors = 3.3 %, |variance - u_rms^2| at most 2.06 standard errors, |mean| at most 2.34 and
    |covariance| at most 1.00 of theirs."""
    p = M.Params(1883, 128, 7, 7, 1.0, 2.7654321, 1.5)
    inv = np.float64(1.0) / p.sigma
    parts = []
    for lo in range(0, 64000, 8000):
        e = M.eddies(p, np.arange(lo, lo + 8000))
        w = (p.amp * M.tent((1.0 - e["ex"]) * inv)) * M.tent((1.0 - e["ey"]) * inv) * M.tent((1.0 - e["ez"]) * inv)
        zero = np.zeros((len(w), 1))                                          # the sum starts at +0.0
        parts.append(np.stack([np.cumsum(np.concatenate([zero, e["sign"][:, :, j] * w], axis=1), axis=1)[:, -1] for j in range(3)]))
    x = np.concatenate(parts, axis=1)
    assert same(x[:, 5], M.fluctuation_at(p, 5, [1], [1])[:, 0]) and same(x[:, 63999], M.fluctuation_at(p, 63999, [1], [1])[:, 0])
    print(check_moments(x, 1.5))


# ---- the sources ------------------------------------------------------------------------------------------------------

def test_inflow_h_needs_no_hip():
    text = open(os.path.join(CSRC, "inflow.h")).read()
    assert re.findall(r'#include\s+[<"]([^>"]+)[>"]', text) == ["cstdint"]
    assert "__device__" in text and "FS_INFLOW_HD" in text
    hip = open(os.path.join(CSRC, "inflow.hip")).read()
    for fn in ("inflow_eddy", "inflow_entry", "inflow_touches", "inflow_pair", "inflow_accumulate", "inflow_compose"):
        assert re.search(r"\b%s\(" % fn, hip), fn                              # the kernels call what the driver calls
    assert "atomic" not in hip


def test_the_entries_are_declared_exported_and_bound():
    from fluid_simulation_amd import _lib
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    want = {"fs_inflow_profile": r"int fs_inflow_profile\(fs_sim\* s, const double\* u, const double\* rms, size_t n\);",
            "fs_inflow_gust": r"int fs_inflow_gust\(fs_sim\* s, const double\* steps, const double\* factor, int n\);",
            "fs_inflow_plane": r"int fs_inflow_plane\(fs_sim\* s, long step, double\* out, size_t n\);",
            "fs_inflow_eddies": r"int fs_inflow_eddies\(fs_sim\* s, long step, double\* out, size_t n\);"}
    for name, proto in want.items():
        assert re.search(proto, text), name
        assert name in _lib.exported_symbols() and name in _lib._SIGNATURES
        assert len(_lib._SIGNATURES[name][1]) == 4
    assert "#define FS_INFLOW_EDDIES_MAX 65536" in text and _lib.INFLOW_EDDIES_MAX == 65536
    assert "#define FS_INFLOW_KNOTS_MAX 4096" in text and _lib.INFLOW_KNOTS_MAX == 4096
    src = open(os.path.join(CSRC, "fluidsim.cpp")).read()
    assert '"monitor", "inflow" }' in src                                      # the timing family
    main = open(os.path.join(ROOT, "src", "main.cpp")).read()
    for flag in ("inflow-profile", "inflow-gust", "inflow-eddies", "inflow-sigma", "inflow-rms", "inflow-convect", "inflow-seed"):
        assert main.count("--" + flag) >= 1 and '"%s"' % flag in main, flag


def test_python_helpers_against_closed_forms():
    from fluid_simulation_amd import inflow as I
    u = I.power_law(6, 4, 30.0, 0.25, 8.0)
    assert u.shape == (4, 6) and u.dtype == np.float64 and u.flags.c_contiguous
    assert np.all(u == u[0]) and u[0, 0] == 30.0 * (0.5 / 8.0) ** 0.25 and u[2, 5] == 30.0 * (5.5 / 8.0) ** 0.25
    assert I.power_law(17, 3, 30.0, 0.25, 8.5)[1, 8] == 30.0                   # the reference height itself
    uz = I.power_law(6, 4, 30.0, 1.0, 2.0, axis="z")
    assert np.all(uz[:, 0:1] == uz) and uz[:, 0].tolist() == [7.5, 22.5, 37.5, 52.5]
    lg = I.log_law(9, 2, 20.0, 0.5, 8.5)
    assert lg.shape == (2, 9) and lg[0, 8] == 20.0 and lg[0, 0] == 0.0 and np.all(np.diff(lg[0]) > 0)
    assert lg[1, 3] == 20.0 * np.log(3.5 / 0.5) / np.log(8.5 / 0.5)
    assert I.log_law(4, 1, 20.0, 2.0, 8.0)[0].tolist()[:2] == [0.0, 0.0]        # below the roughness length
    ti = I.intensity_profile(6, 4, 0.1, 2.5)
    assert ti.shape == (4, 6) and np.all(ti == 0.1)
    ti = I.intensity_profile(6, 4, 0.1, 2.5, decay=1.0, mean=u)
    assert ti[3, 2] == 0.1 * (2.5 / 2.5) ** -1.0 * u[3, 2] and ti[0, 0] == 0.1 * (0.5 / 2.5) ** -1.0 * u[0, 0]
    for bad in (lambda: I.power_law(4, 4, 1.0, 0.2, 0.0), lambda: I.log_law(4, 4, 1.0, 2.0, 1.0), lambda: I.power_law(4, 4, 1.0, 0.2, 1.0, axis="x")):
        with pytest.raises(ValueError):
            bad()
