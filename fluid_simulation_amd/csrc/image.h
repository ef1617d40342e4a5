// image.h -- slice and projection images (include/fluidsim.h, "slice and projection images"): the per-pixel arithmetic of
// the image kernels in image.hip, the built-in colour table, and the launchers.  The arithmetic is plain C++ without HIP
// (inline functions, usable on the host and in the kernels), so that tests/test_image_cpu.py compiles exactly what the kernels
// run.  The reference's counterpart is its 2-D viewer (gui.py:61-79, 257-295), which does the same on the host from dumped
// volumes, one z-slice at a time; projections are beyond it.  Internal to libfluidsim.so.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define FS_IMAGE_HD __host__ __device__
#else
#define FS_IMAGE_HD
#endif

namespace fs {

// kind order of FS_IMG_*; IMG_ANY is internal: the obstacle flag of a projection's pixel (obs > 0.5 anywhere in the column)
enum { IMG_SLICE = 0, IMG_SUM = 1, IMG_MAX = 2, IMG_MIN = 3, IMG_NKINDS = 4, IMG_ANY = 4 };
constexpr int IMG_TABLE_MAX = 4096;     // entries a colour table may have
constexpr int IMG_DEFAULT_N = 256;

// ---- a column's reduction: `a` is the accumulator, v the next cell's stored value, cells in increasing order ----------
template <int KIND>
FS_IMAGE_HD inline double image_start()
{
    return KIND == IMG_MAX ? -__builtin_inf() : KIND == IMG_MIN ? __builtin_inf() : 0.0;
}
// SUM: one rounding per add.  MAX / MIN: NaN is never taken, of equal values the first stays.  ANY: 1.0 once obs > 0.5.
template <int KIND, class E>
FS_IMAGE_HD inline double image_step(double a, E v)
{
    const double d = (double)v;
    if (KIND == IMG_SUM) return a + d;
    if (KIND == IMG_MAX) return d > a ? d : a;
    if (KIND == IMG_MIN) return d < a ? d : a;
    return d > 0.5 ? 1.0 : a;
}
template <class O>
FS_IMAGE_HD inline bool image_solid(O o) { return (double)o > 0.5; }

// ---- colouring: fp64, every operation rounded once, in this order ------------------------------------------------------
// the table entry of a value, -1 for NaN; vmin < vmax, both finite, 2 <= n <= IMG_TABLE_MAX
FS_IMAGE_HD inline int image_colour_index(double v, double vmin, double vmax, int n)
{
    if (v != v) return -1;
    const double c = v < vmin ? vmin : (v > vmax ? vmax : v);
    const double num = c - vmin, den = vmax - vmin;
    const double t = num / den;
    const double tn = t * (double)n;
    const int k = (int)tn;
    return k < n - 1 ? k : n - 1;
}
// a byte of an obstacle pixel, f = (float)(1.0 - alpha): truncation
FS_IMAGE_HD inline uint8_t image_shade(uint8_t b, float f)
{
    const float p = (float)b * f;
    return (uint8_t)p;
}
// one pixel: value and obstacle flag to rgb[3]
FS_IMAGE_HD inline void image_colour(double v, bool solid, double vmin, double vmax, double alpha, const uint8_t* table, int n,
                                     uint8_t* rgb)
{
    const int k = image_colour_index(v, vmin, vmax, n);
    uint8_t r = 0, g = 0, b = 0;
    if (k >= 0) { r = table[3 * k]; g = table[3 * k + 1]; b = table[3 * k + 2]; }
    if (solid && alpha > 0.0) {
        const float f = (float)(1.0 - alpha);
        r = image_shade(r, f); g = image_shade(g, f); b = image_shade(b, f);
    }
    rgb[0] = r; rgb[1] = g; rgb[2] = b;
}

// image geometry: columns run along the lower remaining axis, rows along the higher one
inline void image_dims(int axis, int W, int H, int D, int* cols, int* rows)
{
    *cols = axis == 0 ? H + 2 : W + 2;
    *rows = axis == 2 ? H + 2 : D + 2;
}

// The default table: the 256 triples matplotlib builds for the 2-D viewer's seven colour stops (gui.py:38-41), written out
// (the piecewise-linear formula recomputed in C++ differs from matplotlib by one count in some entries); recorded by
// tools/make_image_goldens.py, pinned by tests/golden/gui_density_cmap_256.npy.
static const uint8_t IMG_DEFAULT_TABLE[3 * IMG_DEFAULT_N] = {
    255,255,255, 252,254,252, 249,254,249, 247,253,247, 244,253,244, 241,253,241, 239,252,239, 236,252,236,
    234,251,234, 231,251,231, 228,251,228, 226,250,226, 223,250,223, 221,249,221, 218,249,218, 215,249,215,
    213,248,213, 210,248,210, 207,247,207, 205,247,205, 202,247,202, 200,246,200, 197,246,197, 194,245,194,
    192,245,192, 189,245,189, 187,244,187, 184,244,184, 181,243,181, 179,243,179, 176,243,176, 174,242,174,
    171,242,171, 168,241,168, 166,241,166, 163,241,163, 160,240,160, 158,240,158, 155,239,155, 153,239,153,
    150,239,150, 147,238,147, 145,238,145, 142,236,142, 138,234,138, 135,231,135, 132,228,132, 128,226,128,
    125,223,125, 121,221,121, 118,218,118, 115,216,115, 111,213,111, 108,210,108, 105,208,105, 101,205,101,
    98,203,98, 94,200,94, 91,197,91, 88,195,88, 84,192,84, 81,190,81, 77,187,77, 74,184,74,
    71,182,71, 67,179,67, 64,177,64, 60,174,60, 57,172,57, 54,169,54, 50,166,50, 47,164,47,
    44,161,44, 40,159,40, 37,156,37, 33,153,33, 30,151,30, 27,148,27, 23,146,23, 20,143,20,
    16,140,16, 13,138,13, 10,135,10, 6,133,6, 3,130,3, 0,128,0, 0,129,6, 0,130,12,
    0,132,18, 0,133,24, 0,135,29, 0,136,36, 0,138,42, 0,139,48, 0,141,54, 0,142,60,
    0,144,66, 0,145,72, 0,147,77, 0,148,84, 0,150,90, 0,151,96, 0,153,102, 0,154,108,
    0,156,114, 0,157,120, 0,159,125, 0,160,132, 0,162,138, 0,163,144, 0,165,150, 0,166,156,
    0,168,162, 0,169,168, 0,170,173, 0,172,180, 0,173,186, 0,175,192, 0,176,198, 0,178,204,
    0,179,210, 0,181,216, 0,182,221, 0,184,228, 0,185,234, 0,187,240, 0,188,246, 0,190,252,
    0,188,255, 0,184,255, 0,179,255, 0,175,255, 0,170,255, 0,166,255, 0,161,255, 0,157,255,
    0,152,255, 0,148,255, 0,143,255, 0,139,255, 0,134,255, 0,130,255, 0,125,255, 0,121,255,
    0,116,255, 0,112,255, 0,107,255, 0,103,255, 0,98,255, 0,94,255, 0,89,255, 0,85,255,
    0,80,255, 0,76,255, 0,71,255, 0,67,255, 0,62,255, 0,58,255, 0,53,255, 0,49,255,
    0,44,255, 0,40,255, 0,35,255, 0,31,255, 0,26,255, 0,22,255, 0,17,255, 0,13,255,
    0,8,255, 0,4,255, 0,0,255, 3,0,249, 6,0,243, 9,0,236, 13,0,230, 16,0,225,
    19,0,219, 22,0,212, 26,0,206, 29,0,200, 32,0,195, 35,0,188, 39,0,182, 42,0,176,
    45,0,170, 49,0,164, 52,0,158, 55,0,152, 58,0,146, 62,0,140, 65,0,134, 68,0,128,
    71,0,122, 75,0,116, 78,0,110, 81,0,104, 85,0,99, 88,0,92, 91,0,86, 94,0,80,
    98,0,74, 101,0,68, 104,0,62, 107,0,56, 111,0,50, 114,0,44, 117,0,38, 121,0,32,
    124,0,26, 127,0,20, 130,0,14, 134,0,8, 137,0,2, 140,0,0, 143,0,0, 145,0,0,
    148,0,0, 151,0,0, 154,0,0, 156,0,0, 159,0,0, 162,0,0, 164,0,0, 167,0,0,
    170,0,0, 173,0,0, 175,0,0, 178,0,0, 181,0,0, 184,0,0, 186,0,0, 189,0,0,
    192,0,0, 194,0,0, 197,0,0, 200,0,0, 203,0,0, 205,0,0, 208,0,0, 211,0,0,
    214,0,0, 216,0,0, 219,0,0, 222,0,0, 224,0,0, 227,0,0, 230,0,0, 233,0,0,
    235,0,0, 238,0,0, 241,0,0, 244,0,0, 246,0,0, 249,0,0, 252,0,0, 255,0,0,
};

}  // namespace fs

#if defined(__HIPCC__)
#include "kernels.h"

namespace fs {

// All sources are LEAD-shifted arrays of the fields' pitched layout (E: the source's element type, O: that of obs).
// val: rows * cols doubles, flag: rows * cols bytes (1 = obstacle pixel), row 0 first.

// FS_IMG_SLICE at padded index `index` of `axis`: the stored values widened, and obs > 0.5 at the same cells.
template <class E, class O>
void launch_image_slice(hipStream_t st, const GridDesc& g, int axis, int index, const E* src, const O* obs, double* val,
                        uint8_t* flag);
// A projection along `axis`, kind IMG_SUM | IMG_MAX | IMG_MIN into val (flag = nullptr), or IMG_ANY into flag (val = nullptr):
// cells 1 .. N of each column in increasing order, strictly sequential.
template <class E>
void launch_image_project(hipStream_t st, const GridDesc& g, int kind, int axis, const E* src, double* val, uint8_t* flag);
// value image + flag image -> RGB bytes; table: n triples on the device
void launch_image_colour(hipStream_t st, long npix, const double* val, const uint8_t* flag, double vmin, double vmax, double alpha,
                         const uint8_t* table, int n, uint8_t* rgb);

}  // namespace fs
#endif
