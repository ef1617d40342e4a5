// inflow.h -- turbulent inflow (include/fluidsim.h, "turbulent inflow"): the counter-based hash, the eddy of a step, the tent,
// the cell-eddy product and the composition of an inlet cell's three components.  inflow.hip's two kernels call exactly these
// inline functions; kernels.h has the launcher.  Plain C++ without HIP (usable on the host and in the kernels), so that
// tests/test_inflow_cpu.py compiles exactly what the kernels run.  Beyond the reference: its only inflow is (speed, 0, 0).
// Internal to libfluidsim.so.
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define FS_INFLOW_HD __host__ __device__
#else
#define FS_INFLOW_HD
#endif

namespace fs {

constexpr int INFLOW_EDDIES_MAX = 65536;
constexpr int INFLOW_KNOTS_MAX = 4096;
constexpr double INFLOW_TENT_K = 1.2247448713915890;    // sqrt(3/2), correctly rounded
constexpr double INFLOW_GEN_MAX = 9007199254740992.0;   // generations stay below 2^53: they are whole numbers in fp64

// what one synthetic-eddy field is made from; everything the kernels need beside the step number
struct InflowParams {
    uint64_t seed;
    int n;              // eddies, 0 .. INFLOW_EDDIES_MAX
    int h, d;           // the inlet plane: cells 1..h times 1..d
    double sigma;       // eddy radius in cells, >= 1
    double convect;     // cells an eddy moves in x per step, >= 0
    double amp;         // A = u_rms * sqrt(V / (N * sigma^3)), 0 where n == 0 (inflow_amplitude)
};

// one eddy at one step
struct InflowEddy {
    double ex, ey, ez;
    double gen;         // the generation, a whole number
    unsigned neg;       // bit j set: the sign of component j (x, y, z) is -1
};

// an entry of the eddy table the plane kernel reads: 32 bytes, two 16-byte loads
struct alignas(16) InflowEntry {
    double ey, ez;
    double ax;          // A * f((1 - ex) * inv)
    uint64_t neg;       // the sign bits
};

// every operation below is rounded once, in this order (the library and the test driver are built without contraction)

// MIX: the finaliser of splitmix64
FS_INFLOW_HD inline uint64_t inflow_mix(uint64_t z)
{
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
// HASH(seed, k, gen, draw)
FS_INFLOW_HD inline uint64_t inflow_hash(uint64_t seed, uint64_t k, uint64_t gen, uint64_t draw)
{
    const uint64_t G = 0x9E3779B97F4A7C15ull;
    const uint64_t a = inflow_mix(seed + G * (k + 1));
    const uint64_t b = inflow_mix(a + G * gen);
    return inflow_mix(b + G * (draw + 1));
}
// UNI: [0, 1) from the upper 53 bits
FS_INFLOW_HD inline double inflow_uniform(uint64_t hash) { return (double)(hash >> 11) * 0x1p-53; }

// the box's extent along y or z for a plane of n cells: (n - 1) + 2 sigma
FS_INFLOW_HD inline double inflow_extent(int n, double sigma) { return (double)(n - 1) + 2.0 * sigma; }

// A; 0 where there are no eddies
inline double inflow_amplitude(int n, int h, int d, double sigma, double u_rms)
{
    if (n <= 0) return 0.0;
    const double vol = ((2.0 * sigma) * inflow_extent(h, sigma)) * inflow_extent(d, sigma);
    const double den = (double)n * ((sigma * sigma) * sigma);
    return u_rms * __builtin_sqrt(vol / den);
}

// the largest travel in generations a step number may ask for: (double)t * c / (2 sigma) + 2 must stay below 2^53
inline bool inflow_step_ok(long t, double sigma, double convect)
{
    if (t < 0) return false;
    const double q = ((double)t * convect) / (2.0 * sigma);
    return q + 2.0 < INFLOW_GEN_MAX;
}

// eddy k at step t
FS_INFLOW_HD inline InflowEddy inflow_eddy(const InflowParams& p, int k, long t)
{
    const double two = 2.0 * p.sigma;
    const double u0 = inflow_uniform(inflow_hash(p.seed, (uint64_t)k, 0, 0));
    const double start = u0 * two;
    const double moved = (double)t * p.convect;
    const double s = start + moved;
    const double q = s / two;
    double gen = __builtin_floor(q);
    const double base = gen * two;
    double rem = s - base;
    if (rem < 0.0) rem = 0.0;                            // the quotient rounded up to a whole number: the eddy is newly born
    if (!(rem < two)) { rem = 0.0; gen = gen + 1.0; }    // the product rounded down: likewise, one generation on
    const uint64_t gi = (uint64_t)gen;
    InflowEddy e;
    e.gen = gen;
    e.ex = (1.0 - p.sigma) + rem;
    e.ey = (1.0 - p.sigma) + inflow_uniform(inflow_hash(p.seed, (uint64_t)k, gi, 1)) * inflow_extent(p.h, p.sigma);
    e.ez = (1.0 - p.sigma) + inflow_uniform(inflow_hash(p.seed, (uint64_t)k, gi, 2)) * inflow_extent(p.d, p.sigma);
    e.neg = 0;
    for (int j = 0; j < 3; ++j) e.neg |= (unsigned)(inflow_hash(p.seed, (uint64_t)k, gi, 3 + (uint64_t)j) >> 63) << j;
    return e;
}

// f(rho) = sqrt(3/2) * max(0, 1 - |rho|)
FS_INFLOW_HD inline double inflow_tent(double rho)
{
    const double a = 1.0 - __builtin_fabs(rho);
    return INFLOW_TENT_K * (a > 0.0 ? a : 0.0);
}

// the table's entry of an eddy: its x factor carries A
FS_INFLOW_HD inline InflowEntry inflow_entry(const InflowEddy& e, double amp, double inv)
{
    InflowEntry t;
    t.ey = e.ey;
    t.ez = e.ez;
    t.ax = amp * inflow_tent((1.0 - e.ex) * inv);
    t.neg = e.neg;
    return t;
}

// w of one (cell, eddy) pair: (ax * f_y) * f_z
FS_INFLOW_HD inline double inflow_pair(const InflowEntry& t, double y, double z, double inv)
{
    const double fy = inflow_tent((y - t.ey) * inv);
    const double fz = inflow_tent((z - t.ez) * inv);
    return (t.ax * fy) * fz;
}

// can eddy t give a cell of rows ylo..yhi, planes zlo..zhi a non-zero w?  Conservative by a whole cell, so that no rounding of
// (y - ey) * inv matters: a cell further than sigma + 1 from the centre along one axis has a tent of exactly 0 there
FS_INFLOW_HD inline bool inflow_touches(const InflowEntry& t, double sigma, double ylo, double yhi, double zlo, double zhi)
{
    const double reach = sigma + 1.0;
    return t.ax != 0.0 && t.ey + reach > ylo && t.ey - reach < yhi && t.ez + reach > zlo && t.ez - reach < zhi;
}

// u'_j += eps_j * w for the three components (eps_j * w is exact: a sign)
FS_INFLOW_HD inline void inflow_accumulate(double (&u)[3], const InflowEntry& t, double w)
{
    u[0] = u[0] + ((t.neg & 1u) ? -w : w);
    u[1] = u[1] + ((t.neg & 2u) ? -w : w);
    u[2] = u[2] + ((t.neg & 4u) ? -w : w);
}

// the three components of an inlet cell before the rounding to the field type
FS_INFLOW_HD inline void inflow_compose(double (&out)[3], double gust, double mean, double scale, const double (&u)[3])
{
    const double gm = gust * mean;
    const double fx = scale * u[0];
    out[0] = gm + fx;
    out[1] = scale * u[1];
    out[2] = scale * u[2];
}

// g(t): knots (ts[i], fs[i]), ts strictly increasing; constant outside them; 1 without a schedule
inline double inflow_gust(const double* ts, const double* fs_, int n, long t)
{
    if (n <= 0) return 1.0;
    const double x = (double)t;
    if (x <= ts[0]) return fs_[0];
    if (x >= ts[n - 1]) return fs_[n - 1];
    int i = 0;
    while (!(x < ts[i + 1])) ++i;                        // ts[i] <= x < ts[i + 1]
    const double frac = (x - ts[i]) / (ts[i + 1] - ts[i]);
    return fs_[i] + (fs_[i + 1] - fs_[i]) * frac;
}

}  // namespace fs
