// volume.h -- direct volume rendering (include/fluidsim.h, "volume rendering"): the construction of a camera's rays, the
// per-ray arithmetic of the ray-march kernel in volume.hip, and its launcher.  The arithmetic is plain C++ without HIP
// (inline functions, usable on the host and in the kernel), templated on the element types of the source and of obs, so that
// tests/test_volume_cpu.py compiles exactly what the kernel runs.  The sampler is sample.h's FS_SAMPLE_LINEAR and the colour
// index image.h's, both unchanged.  The reference's counterpart is the camera of its 3-D viewer (GUI/gl_widget.py:26-28,
// 64-76), which draws streamlines and the obstacle mesh; it renders no volume.  Internal to libfluidsim.so.
//
// Everything is fp64; every written operation is rounded once, in the order written (the library and the test driver are
// built without contraction).  The march uses + - * / and comparisons only: no sqrt, no transcendental function.
#pragma once
#include <stdint.h>

#include "image.h"
#include "sample.h"

#if defined(__HIPCC__)
#define FS_VOLUME_HD __host__ __device__
#else
#define FS_VOLUME_HD
#endif

namespace fs {

constexpr int VOLUME_PARAMS = 11;           // FS_VOLUME_PARAMS
constexpr int VOLUME_CAMERAS_MAX = 4;       // FS_VOLUME_CAMERAS_MAX
constexpr int VOLUME_VIEWS_MAX = 4;         // FS_VOLUME_VIEWS_MAX
constexpr int VOLUME_SAMPLES_MAX = 16384;   // FS_VOLUME_SAMPLES_MAX
constexpr int VOLUME_SIZE_MAX = 2048;       // columns or rows of a ray set
// order of par[]
enum { VP_VMIN = 0, VP_VMAX, VP_OPACITY, VP_STEP, VP_TMIN, VP_OBST_R, VP_OBST_G, VP_OBST_B, VP_BACK_R, VP_BACK_G, VP_BACK_B };

FS_VOLUME_HD inline bool volume_finite(double x) { return x - x == 0.0; }   // false for NaN and both infinities

// ---- rays of a camera (host only: the one place with a sqrt) ----------------------------------------------------------
// cam[11] = {eye[3], target[3], up[3], half_height, ortho}.  The basis, in this order:
//     F = target - eye;            f = F / sqrt((F.x F.x + F.y F.y) + F.z F.z)            (each component divided)
//     R = f x up = (f.y up.z - f.z up.y, f.z up.x - f.x up.z, f.x up.y - f.y up.x);        r = R / sqrt((R.R)), as above
//     u = r x f, the same component pattern
// Returns false (the camera is FS_EINVAL) if an entry of cam is not finite, half_height <= 0, or F.F or R.R is 0 or not finite.
struct VolumeCamera {
    double eye[3], f[3], r[3], u[3], half_height;
    bool ortho;
};
inline double volume_dot(const double* a, const double* b)
{
    const double xx = a[0] * b[0], yy = a[1] * b[1], zz = a[2] * b[2];
    return (xx + yy) + zz;
}
inline void volume_cross(const double* a, const double* b, double* c)
{
    const double x0 = a[1] * b[2], x1 = a[2] * b[1], y0 = a[2] * b[0], y1 = a[0] * b[2], z0 = a[0] * b[1], z1 = a[1] * b[0];
    c[0] = x0 - x1;
    c[1] = y0 - y1;
    c[2] = z0 - z1;
}
inline bool volume_normalise(const double* a, double* n)
{
    const double l2 = volume_dot(a, a);
    if (!(l2 > 0.0) || !volume_finite(l2)) return false;
    const double l = __builtin_sqrt(l2);
    for (int k = 0; k < 3; ++k) n[k] = a[k] / l;
    return true;
}
inline bool volume_camera_basis(const double* cam, VolumeCamera& c)
{
    for (int k = 0; k < 11; ++k)
        if (!volume_finite(cam[k])) return false;
    if (!(cam[9] > 0.0)) return false;
    double F[3], R[3];
    for (int k = 0; k < 3; ++k) { c.eye[k] = cam[k]; F[k] = cam[3 + k] - cam[k]; }
    if (!volume_normalise(F, c.f)) return false;
    volume_cross(c.f, cam + 6, R);
    if (!volume_normalise(R, c.r)) return false;
    volume_cross(c.r, c.f, c.u);
    c.half_height = cam[9];
    c.ortho = cam[10] != 0.0;
    return true;
}
// The ray of pixel (i, j) -- row i (0 at the top), column j -- of a cols x rows image: ray[6] = {o, d}.
//     sx = (((2 (j + 0.5)) / cols - 1) * half_height) * (cols / rows)        cols / rows: the fp64 quotient
//     sy = (1 - (2 (i + 0.5)) / rows) * half_height
//     V_a = (f_a + sx r_a) + sy u_a          P_a = (eye_a + sx r_a) + sy u_a
//     perspective:  o = eye, d = V / sqrt((V.V))          orthographic:  o = P, d = f
inline void volume_camera_ray(const VolumeCamera& c, int cols, int rows, int i, int j, double* ray)
{
    const double aspect = (double)cols / (double)rows;
    const double jx = 2.0 * ((double)j + 0.5), iy = 2.0 * ((double)i + 0.5);
    const double sx = ((jx / (double)cols - 1.0) * c.half_height) * aspect;
    const double sy = (1.0 - iy / (double)rows) * c.half_height;
    if (c.ortho) {
        for (int a = 0; a < 3; ++a) {
            const double xr = sx * c.r[a], yu = sy * c.u[a];
            ray[a] = (c.eye[a] + xr) + yu;
            ray[3 + a] = c.f[a];
        }
        return;
    }
    double V[3];
    for (int a = 0; a < 3; ++a) {
        const double xr = sx * c.r[a], yu = sy * c.u[a];
        V[a] = (c.f[a] + xr) + yu;
        ray[a] = c.eye[a];
    }
    if (!volume_normalise(V, ray + 3))                   // cannot happen for a finite camera: |V| >= |f| up to rounding
        for (int a = 0; a < 3; ++a) ray[3 + a] = 0.0;    // (an invalid ray: the pixel is background)
}

// ---- one view's parameters --------------------------------------------------------------------------------------------
// par[VOLUME_PARAMS] as fs_volume_render takes them; true if they are legal for a W x H x D grid.  *kmax receives the loop
// limit of the march: with diag = sqrt((((W+1)^2 + (H+1)^2) + (D+1)^2)) (exact integers below 2^53) and q = diag / step,
// legal means q <= VOLUME_SAMPLES_MAX, and kmax = (long)q + 2 -- more samples than a ray of |d| >= 1 can take through the box.
inline bool volume_params_ok(const double* par, int W, int H, int D, long* kmax)
{
    for (int k = 0; k < VOLUME_PARAMS; ++k)
        if (!volume_finite(par[k])) return false;
    if (!(par[VP_VMIN] < par[VP_VMAX]) || !(par[VP_OPACITY] >= 0.0) || !(par[VP_STEP] > 0.0)) return false;
    if (!(par[VP_TMIN] >= 0.0 && par[VP_TMIN] < 1.0)) return false;
    for (int k = VP_OBST_R; k <= VP_BACK_B; ++k)
        if (!(par[k] >= 0.0 && par[k] <= 255.0)) return false;
    const double w = (double)(W + 1), h = (double)(H + 1), d = (double)(D + 1);
    const double diag = __builtin_sqrt((w * w + h * h) + d * d), q = diag / par[VP_STEP];
    if (!(q <= (double)VOLUME_SAMPLES_MAX)) return false;
    if (kmax) *kmax = (long)q + 2;
    return true;
}

// ---- one ray ------------------------------------------------------------------------------------------------------------
struct VolumeView {                         // what the kernel gets by value
    double par[VOLUME_PARAMS];
    long kmax;
    int W, H, D;
    long py, pz;                            // pitches of the source's and obs's layout, elements
    int n;                                  // entries of the colour table
};

// One axis of the slab test: false = the ray misses.
FS_VOLUME_HD inline bool volume_slab(double o, double d, int N, double& t0, double& t1)
{
    const double hi = (double)(N + 1);
    if (d == 0.0) return o >= 0.0 && o <= hi;
    const double ta = (0.0 - o) / d, tb = (hi - o) / d;
    const double lo = ta < tb ? ta : tb, up = ta < tb ? tb : ta;
    t0 = t0 > lo ? t0 : lo;
    t1 = t1 < up ? t1 : up;
    return true;
}
FS_VOLUME_HD inline double volume_clamp(double p, int N)
{
    const double hi = (double)(N + 1);
    return p < 0.0 ? 0.0 : (p > hi ? hi : p);
}
template <class O>
FS_VOLUME_HD inline int volume_solid_at(const O* obs, const VolumeView& vw, int i, int j, int l)
{
    if (i < 0 || i > vw.W + 1 || j < 0 || j > vw.H + 1 || l < 0 || l > vw.D + 1) return 0;
    return image_solid(obs[(long)i + (long)j * vw.py + (long)l * vw.pz]) ? 1 : 0;
}
FS_VOLUME_HD inline uint8_t volume_byte(double C, double T, double back)
{
    const double tb = T * back;
    const double s = (C + tb) + 0.5;
    return (uint8_t)(s < 255.0 ? s : 255.0);
}

// ray[6] = {o, d}; src / obs: LEAD-shifted arrays of the pitched layout vw describes (E / O: their element types); table: vw.n
// RGB triples.  acc[4] = {C_r, C_g, C_b, T} before the background is added, rgb[3] the bytes.
// Every index loaded is in range by construction: p is clamped to [0, N + 1], sample_axis gives i0 <= N, the nearest cell
// (int)(p + 0.5) lies in 0 .. N + 1, and volume_solid_at checks its neighbours.
template <class E, class O>
FS_VOLUME_HD inline void volume_ray(const double* ray, const E* src, const O* obs, const VolumeView& vw, const uint8_t* table,
                                    double* acc, uint8_t* rgb)
{
    const double* par = vw.par;
    const double vmin = par[VP_VMIN], vmax = par[VP_VMAX], opacity = par[VP_OPACITY], step = par[VP_STEP], t_min = par[VP_TMIN];
    const double ox = ray[0], oy = ray[1], oz = ray[2], dx = ray[3], dy = ray[4], dz = ray[5];
    double C[3] = {0.0, 0.0, 0.0}, T = 1.0;
    bool hit = volume_finite(ox) && volume_finite(oy) && volume_finite(oz) && volume_finite(dx) && volume_finite(dy) &&
               volume_finite(dz) && !(dx == 0.0 && dy == 0.0 && dz == 0.0);
    double t0 = 0.0, t1 = __builtin_inf();
    hit = hit && volume_slab(ox, dx, vw.W, t0, t1);
    hit = hit && volume_slab(oy, dy, vw.H, t0, t1);
    hit = hit && volume_slab(oz, dz, vw.D, t0, t1);
    hit = hit && t0 < t1;
    if (hit) {
        const double den = vmax - vmin;
        for (long k = 0; k < vw.kmax; ++k) {
            const double tk = t0 + ((double)k + 0.5) * step;
            if (!(tk < t1)) break;
            const double px = volume_clamp(ox + tk * dx, vw.W), py = volume_clamp(oy + tk * dy, vw.H),
                         pz = volume_clamp(oz + tk * dz, vw.D);
            // the nearest cell's obs and the eight corners: nine independent loads, issued before any of them is used
            const int ci = (int)(px + 0.5), cj = (int)(py + 0.5), cl = (int)(pz + 0.5);
            int i0, j0, l0;
            double sx, sy, sz;
            sample_axis(px, vw.W, i0, sx);
            sample_axis(py, vw.H, j0, sy);
            sample_axis(pz, vw.D, l0, sz);
            const O oc = obs[(long)ci + (long)cj * vw.py + (long)cl * vw.pz];
            const long base = (long)i0 + (long)j0 * vw.py + (long)l0 * vw.pz;
            E v8[8];
            for (int c = 0; c < 8; ++c) v8[c] = src[base + (c & 1) + ((c >> 1) & 1) * vw.py + (c >> 2) * vw.pz];
            if (image_solid(oc)) {
                const int gx = volume_solid_at(obs, vw, ci + 1, cj, cl) - volume_solid_at(obs, vw, ci - 1, cj, cl);
                const int gy = volume_solid_at(obs, vw, ci, cj + 1, cl) - volume_solid_at(obs, vw, ci, cj - 1, cl);
                const int gz = volume_solid_at(obs, vw, ci, cj, cl + 1) - volume_solid_at(obs, vw, ci, cj, cl - 1);
                const int n2 = gx * gx + gy * gy + gz * gz;
                double shade = 1.0;
                if (n2 != 0) {
                    const double rn = n2 == 1 ? 1.0 : n2 == 2 ? 0.7071067811865476 : 0.5773502691896257;
                    const double xx = (double)gx * dx, yy = (double)gy * dy, zz = (double)gz * dz;
                    const double dot = (xx + yy) + zz;
                    const double ad = dot < 0.0 ? -dot : dot;
                    const double s = 0.3 + 0.7 * (ad * rn);
                    shade = s < 1.0 ? s : 1.0;           // a NaN (infinite d) shades fully
                }
                for (int c = 0; c < 3; ++c) C[c] = C[c] + T * (par[VP_OBST_R + c] * shade);
                T = 0.0;
                break;
            }
            const double v = sample_linear(v8, sx, sy, sz);
            if (v == v) {
                const double cv = v < vmin ? vmin : (v > vmax ? vmax : v);
                const double tn = (cv - vmin) / den;
                const double ao = (opacity * tn) * step;
                const double a = ao < 1.0 ? ao : 1.0;
                if (a > 0.0) {
                    const int idx = image_colour_index(v, vmin, vmax, vw.n);
                    const double w = T * a;
                    for (int c = 0; c < 3; ++c) C[c] = C[c] + w * (double)table[3 * idx + c];
                    T = T * (1.0 - a);
                }
            }
            if (T < t_min) break;
        }
    }
    if (acc) { acc[0] = C[0]; acc[1] = C[1]; acc[2] = C[2]; acc[3] = T; }
    if (rgb)
        for (int c = 0; c < 3; ++c) rgb[c] = volume_byte(C[c], T, par[VP_BACK_R + c]);
}

}  // namespace fs

#if defined(__HIPCC__)
#include "kernels.h"

namespace fs {

// One image: rays[6 * (r * cols + c) + ..] on the device, one thread per ray; rgb (3 bytes per pixel) and acc (4 doubles per
// pixel) are device arrays, either may be null.  src / obs as for launch_sample.  vw.W .. vw.pz are filled in from g here.
template <class E, class O>
void launch_volume(hipStream_t st, const GridDesc& g, VolumeView vw, int cols, int rows, const double* rays, const E* src,
                   const O* obs, const uint8_t* table, uint8_t* rgb, double* acc);

}  // namespace fs
#endif
