// bodies.h -- per-body pressure forces and moments (include/fluidsim.h, "per-body pressure forces and moments"): the
// per-face arithmetic of the kernel in bodies.hip and the host's ordering of the components, and their launchers.
// The arithmetic and the ordering are plain C++ without HIP (inline functions, usable on the host and in the kernels), so
// that tests/test_bodies_cpu.py compiles exactly what runs.  Beyond the reference: it has no force output.
// Internal to libfluidsim.so.
#pragma once

#include <algorithm>
#include <vector>

#if defined(__HIPCC__)
#define FS_BODIES_HD __host__ __device__
#else
#define FS_BODIES_HD
#endif

namespace fs {

constexpr int BODY_MAX = 16;            // FS_BODY_MAX
constexpr int BODY_REC = 8;             // FS_BODY_COLS: Sx, Sy, Sz, Mx, My, Mz, faces, frontal rows
constexpr int BODY_INFO = 12;           // FS_BODY_INFO_COLS

// One blocked face of cell c: the neighbour lies on the `sign` (+1 / -1) side of c along `axis` (0, 1, 2), p = p(c)
// widened, (rx, ry, rz) = c's padded index coordinates minus the moment origin.  q = sign * p goes to acc[axis] (S) and
// r x (q e_axis) to acc[3..5] (M).  The face centre is half a cell from c along e_axis, which the cross product with
// e_axis removes: the arm of a face is its cell's.  Every product and every add is rounded once, in the order written
// (the library and the test driver are built without contraction).
FS_BODIES_HD inline void face_term(int axis, int sign, double p, double rx, double ry, double rz, double* acc)
{
    const double q = sign > 0 ? p : -p;
    acc[axis] = acc[axis] + q;
    if (axis == 0) {
        const double a = q * rz, b = q * ry;
        acc[4] = acc[4] + a;
        acc[5] = acc[5] - b;
    } else if (axis == 1) {
        const double a = q * rz, b = q * rx;
        acc[3] = acc[3] - a;
        acc[5] = acc[5] + b;
    } else {
        const double a = q * ry, b = q * rx;
        acc[3] = acc[3] + a;
        acc[4] = acc[4] - b;
    }
}

// A component: its anchor (smallest padded linear index of its cells) and its size in cells.
struct BodyPair {
    long anchor, size;
};

// The label of each component of `pairs` (any order): 1 .. B = min(components, max) by decreasing size, ties by
// increasing anchor; -1 (the REST) for the others.
inline std::vector<int> order_bodies(const std::vector<BodyPair>& pairs, int max)
{
    std::vector<size_t> idx(pairs.size());
    for (size_t i = 0; i < idx.size(); ++i) idx[i] = i;
    std::sort(idx.begin(), idx.end(), [&](size_t a, size_t b) {
        return pairs[a].size != pairs[b].size ? pairs[a].size > pairs[b].size : pairs[a].anchor < pairs[b].anchor;
    });
    std::vector<int> remap(pairs.size(), -1);
    for (size_t r = 0; r < idx.size() && r < (size_t)(max > 0 ? max : 0); ++r) remap[idx[r]] = (int)r + 1;
    return remap;
}

}  // namespace fs

#if defined(__HIPCC__)
#include "kernels.h"

namespace fs {

// The labels live in a dense padded int32 array, cell (x, y, z) at x + (W + 2) * (y + (H + 2) * z) -- the index that is
// a component's anchor.  All launchers run on `st`; none synchronises.

// L[i] = i on body cells (interior, obs != 0), -1 elsewhere; *n_cells (device, zeroed by the caller) += body cells
template <class T>
void launch_body_init(hipStream_t st, const GridDesc& g, const T* obs, int* L, unsigned long long* n_cells);
// One round of label equivalence with pointer jumping: every body cell takes the root of the smallest label among
// itself and its face neighbours and hands it to its old label's cell (integer atomicMin only).  *changed (device) is
// set to 1 if a label fell.  At the fixed point every cell holds its component's anchor, whatever the order.
void launch_body_merge(hipStream_t st, const GridDesc& g, int* L, int* changed);
// cnt[a] (zeroed by the caller, dense like L) += cells whose label is a; *n_roots (zeroed) += components
void launch_body_count(hipStream_t st, const GridDesc& g, const int* L, int* cnt, unsigned long long* n_roots);
// pairs[2 k], pairs[2 k + 1] = anchor, size of the components, k < *n_roots in no particular order; *cursor zeroed
void launch_body_compact(hipStream_t st, const GridDesc& g, const int* L, const int* cnt, long* pairs,
                         unsigned long long* cursor);
// cnt[pairs[2 k]] = lab[k], then L[i] = cnt[L[i]] on body cells and 0 elsewhere
void launch_body_relabel(hipStream_t st, const GridDesc& g, long n_pairs, const long* pairs, const int* lab, int* L, int* cnt);
// info[k * BODY_INFO + ..], k = 0 .. BODY_MAX (record of label k, 0 = REST): integer atomics only.  The caller sets
// cells, maxima, sums and frontal rows to 0 and anchor and minima to ~0 beforehand.  `flags`: the flag bytes (F_SOLID).
void launch_body_info(hipStream_t st, const GridDesc& g, const int* L, const uint8_t* flags, unsigned long long* info);

// Plane records: out[((z - 1) * nrec + k) * BODY_REC + ..] for planes z = 1 .. g.D and records k < nrec, and their sums
// in increasing z from +0.0: total[k * BODY_REC + ..].  bbox[6 k + ..] = the cells {x0, x1, y0, y1, z0, z1} workgroup
// (z, k) scans: record k's bounding box grown by one cell and clipped to the interior, x0 > x1 for an empty record.
// One launch of each of two kernels.
template <class T>
void launch_body_forces(hipStream_t st, const GridDesc& g, const T* p, const uint8_t* flags, const int* L, const int* bbox,
                        int nrec, const double* origin, double* out, double* total);

}  // namespace fs
#endif
