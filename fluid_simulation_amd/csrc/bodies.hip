// bodies.hip -- body labels of the solid cells and per-body force and moment records (bodies.h).
// Labelling: label equivalence with pointer jumping over a dense int32 array, integer atomics only.  Records: one
// workgroup of BT lanes per (plane, record) over the record's bounding box, a fixed assignment of its cells to the lanes
// and a fixed shuffle / LDS tree, no atomics on floating-point values.
// -Rpass-analysis (gfx950): body_forces_kernel 60 (fp32) / 52 (fp64) VGPRs and 1248 bytes of LDS, the labelling kernels
// 4 .. 20 VGPRs (body_info_kernel: 968 bytes of LDS); scratch 0 and 8 waves per SIMD for every one of them.
#include "bodies.h"
#include "kernels_dev.h"

namespace fs {

namespace {

constexpr int LT = 256;           // threads per workgroup of the labelling kernels
constexpr int BT = 256;           // threads per (plane, record); the summation order is defined for this size, do not tune it
constexpr int ROWCHUNK = 8192;    // rows per pass of the LDS row bitmask (frontal rows)

struct Dense {
    int X, Y, Z;
    long N;
};
inline Dense dense_of(const GridDesc& g)
{
    Dense d = { g.W + 2, g.H + 2, g.D + 2, 0 };
    d.N = (long)d.X * d.Y * d.Z;
    return d;
}
inline unsigned blocks_for(long n, int per) { return (unsigned)((n + per - 1) / per); }

template <class T>
__global__ __launch_bounds__(LT) void body_init_kernel(GridDesc g, Dense dn, const T* __restrict__ obs, int* __restrict__ L,
                                                       unsigned long long* __restrict__ n_cells)
{
    const long i = (long)blockIdx.x * LT + threadIdx.x;
    bool body = false;
    if (i < dn.N) {
        const int x = (int)(i % dn.X), y = (int)((i / dn.X) % dn.Y), z = (int)(i / ((long)dn.X * dn.Y));
        if (x >= 1 && x <= g.W && y >= 1 && y <= g.H && z >= 1 && z <= g.D) body = obs[cell(g, x, y, z)] != (T)0;
        L[i] = body ? (int)i : -1;
    }
    const unsigned long long m = __ballot(body);
    if ((threadIdx.x & 63) == 0 && m) atomicAdd(n_cells, (unsigned long long)__popcll(m));
}

__global__ __launch_bounds__(LT) void body_merge_kernel(Dense dn, int* L, int* changed)
{
    const long i = (long)blockIdx.x * LT + threadIdx.x;
    if (i >= dn.N) return;
    const int l = __hip_atomic_load(&L[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (l < 0) return;
    // a body cell is interior, so its six neighbours exist; cells that are no body cells hold -1
    const long sy = dn.X, sz = (long)dn.X * dn.Y;
    const long nb[6] = { i + 1, i - 1, i + sy, i - sy, i + sz, i - sz };
    int m = l;
#pragma unroll
    for (int k = 0; k < 6; ++k) {
        const int v = __hip_atomic_load(&L[nb[k]], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (v >= 0 && v < m) m = v;
    }
    // labels only fall, and a cell's label is never above its own index: the chase ends at a cell that holds itself
    int r = m;
    for (;;) {
        const int t = __hip_atomic_load(&L[r], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (t >= r || t < 0) break;
        r = t;
    }
    if (r < l) {
        atomicMin(&L[i], r);
        atomicMin(&L[l], r);
        *changed = 1;
    }
}

__global__ __launch_bounds__(LT) void body_count_kernel(Dense dn, const int* __restrict__ L, int* __restrict__ cnt,
                                                        unsigned long long* __restrict__ n_roots)
{
    const long i = (long)blockIdx.x * LT + threadIdx.x;
    bool root = false;
    if (i < dn.N) {
        const int l = L[i];
        if (l >= 0) {
            atomicAdd(&cnt[l], 1);
            root = (l == (int)i);
        }
    }
    const unsigned long long m = __ballot(root);
    if ((threadIdx.x & 63) == 0 && m) atomicAdd(n_roots, (unsigned long long)__popcll(m));
}

__global__ __launch_bounds__(LT) void body_compact_kernel(Dense dn, const int* __restrict__ L, const int* __restrict__ cnt,
                                                          long* __restrict__ pairs, unsigned long long* __restrict__ cursor)
{
    const long i = (long)blockIdx.x * LT + threadIdx.x;
    if (i >= dn.N || L[i] != (int)i) return;
    const unsigned long long k = atomicAdd(cursor, 1ull);
    pairs[2 * k] = i;
    pairs[2 * k + 1] = (long)cnt[i];
}

__global__ __launch_bounds__(LT) void body_scatter_kernel(long n, const long* __restrict__ pairs, const int* __restrict__ lab,
                                                          int* __restrict__ cnt)
{
    const long k = (long)blockIdx.x * LT + threadIdx.x;
    if (k < n) cnt[pairs[2 * k]] = lab[k];
}

__global__ __launch_bounds__(LT) void body_relabel_kernel(Dense dn, int* __restrict__ L, const int* __restrict__ cnt)
{
    const long i = (long)blockIdx.x * LT + threadIdx.x;
    if (i >= dn.N) return;
    const int a = L[i];
    L[i] = a >= 0 ? cnt[a] : 0;
}

// record of a label: 1..BODY_MAX the bodies, 0 the REST (-1)
__device__ __forceinline__ int record_of(int lab) { return lab > 0 ? lab : 0; }

constexpr int NREC = BODY_MAX + 1;

__global__ __launch_bounds__(LT) void body_info_kernel(Dense dn, const int* __restrict__ L, unsigned long long* __restrict__ info)
{
    // per workgroup in LDS first, then one global atomic per touched entry
    __shared__ unsigned cells[NREC], lo[NREC][4], hi[NREC][3];    // lo: anchor, xmin, ymin, zmin
    __shared__ unsigned long long sum[NREC][3];
    for (int k = threadIdx.x; k < NREC; k += LT) {
        cells[k] = 0u;
        for (int a = 0; a < 4; ++a) lo[k][a] = ~0u;
        for (int a = 0; a < 3; ++a) { hi[k][a] = 0u; sum[k][a] = 0ull; }
    }
    __syncthreads();
    const long i = (long)blockIdx.x * LT + threadIdx.x;
    if (i < dn.N) {
        const int lab = L[i];
        if (lab != 0) {
            const int k = record_of(lab);
            const unsigned x = (unsigned)(i % dn.X), y = (unsigned)((i / dn.X) % dn.Y), z = (unsigned)(i / ((long)dn.X * dn.Y));
            atomicAdd(&cells[k], 1u);
            atomicMin(&lo[k][0], (unsigned)i);
            atomicMin(&lo[k][1], x);
            atomicMin(&lo[k][2], y);
            atomicMin(&lo[k][3], z);
            atomicMax(&hi[k][0], x);
            atomicMax(&hi[k][1], y);
            atomicMax(&hi[k][2], z);
            atomicAdd(&sum[k][0], (unsigned long long)x);
            atomicAdd(&sum[k][1], (unsigned long long)y);
            atomicAdd(&sum[k][2], (unsigned long long)z);
        }
    }
    __syncthreads();
    for (int k = threadIdx.x; k < NREC; k += LT) {
        if (!cells[k]) continue;
        unsigned long long* o = info + (long)k * BODY_INFO;
        atomicAdd(&o[0], (unsigned long long)cells[k]);
        atomicMin(&o[1], (unsigned long long)lo[k][0]);
        for (int a = 0; a < 3; ++a) {
            atomicMin(&o[2 + 2 * a], (unsigned long long)lo[k][1 + a]);
            atomicMax(&o[3 + 2 * a], (unsigned long long)hi[k][a]);
            atomicAdd(&o[8 + a], sum[k][a]);
        }
    }
}

// one wave per interior row (y, z): which records hold an F_SOLID cell in it
__global__ __launch_bounds__(LT) void body_frontal_kernel(GridDesc g, Dense dn, const int* __restrict__ L,
                                                          const uint8_t* __restrict__ flags, unsigned long long* __restrict__ info)
{
    const long row = (long)blockIdx.x * (LT / 64) + (threadIdx.x >> 6);
    if (row >= (long)g.H * g.D) return;                  // whole waves leave together
    const int y = 1 + (int)(row % g.H), z = 1 + (int)(row / g.H);
    const int* Lr = L + (long)dn.X * (y + (long)dn.Y * z);
    const uint8_t* fr = flags + cell(g, 0, y, z);
    unsigned mask = 0u;
    for (int x = 1 + (threadIdx.x & 63); x <= g.W; x += 64) {
        const int lab = Lr[x];
        if (lab != 0 && (fr[x] & F_SOLID)) mask |= 1u << record_of(lab);
    }
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) mask |= (unsigned)__shfl_xor((int)mask, m, 64);
    if ((threadIdx.x & 63) == 0)
        for (int k = 0; k < NREC; ++k)
            if (mask >> k & 1u) atomicAdd(&info[(long)k * BODY_INFO + 11], 1ull);
}

// Lane t of workgroup (z, k) takes the groups of four x-consecutive cells i = t, t + BT, ... of each chunk of `rc` rows
// of the record's box: group i = (row i / G, group g0 + i % G), G = the groups the box's x range touches; group n holds
// cells 1 + 4 n .. 4 + 4 n.  One 4-byte load of flag bytes and, where one of the four cells has a blocked face towards
// the record, one 16-byte (fp32) / 32-byte (fp64) load of p -- as in forces_kernel -- plus a label read at the neighbour
// of every blocked face.  Each lane adds its faces cell by cell, +x -x +y -y +z -z within a cell, in fp64 (face_term);
// the 64 lanes of a wave combine by a butterfly of shuffles and thread 0 adds the wave sums in wave order.
template <class T>
__global__ __launch_bounds__(BT) void body_forces_kernel(GridDesc g, Dense dn, const T* __restrict__ p,
                                                         const uint8_t* __restrict__ flags, const int* __restrict__ L,
                                                         const int* __restrict__ bbox, int nrec, double r0x, double r0y,
                                                         double r0z, double* __restrict__ out, int rc)
{
    __shared__ unsigned rowbits[ROWCHUNK / 32];
    __shared__ double wsum[BT / 64][6];
    __shared__ int wcnt[BT / 64][2];
    const int t = threadIdx.x;
    const int z = 1 + blockIdx.x, k = blockIdx.y;
    const int want = k == 0 ? -1 : k;
    const int bx0 = bbox[6 * k], bx1 = bbox[6 * k + 1], by0 = bbox[6 * k + 2], by1 = bbox[6 * k + 3], bz0 = bbox[6 * k + 4],
              bz1 = bbox[6 * k + 5];
    double* o = out + ((long)(z - 1) * nrec + k) * BODY_REC;
    if (bx0 > bx1 || z < bz0 || z > bz1) {               // the whole workgroup: nothing of this record near this plane
        if (t < BODY_REC) o[t] = 0.0;
        return;
    }
    const bool rzp = z + 1 <= g.D, rzm = z - 1 >= 1;
    const unsigned g0 = (unsigned)(bx0 - 1) >> 2, G = ((unsigned)(bx1 - 1) >> 2) - g0 + 1u;
    const long dsy = dn.X, dsz = (long)dn.X * dn.Y;
    const double rz = (double)z - r0z;
    double acc[6] = { 0.0, 0.0, 0.0, 0.0, 0.0, 0.0 };
    int faces = 0, frontal = 0;
    for (int y0 = by0; y0 <= by1; y0 += rc) {
        const int nrow = min(rc, by1 - y0 + 1);
        for (int i = t; i < ROWCHUNK / 32; i += BT) rowbits[i] = 0u;
        __syncthreads();
        const unsigned items = (unsigned)nrow * G;
        for (unsigned i = t; i < items; i += BT) {
            const unsigned r = i / G;
            const int x0 = 1 + 4 * (int)(g0 + (i - r * G));
            const int y = y0 + (int)r;
            const long c = cell(g, x0, y, z);
            const long dl = (long)x0 + dsy * y + dsz * z;
            const unsigned f4 = *reinterpret_cast<const unsigned*>(flags + c);
            unsigned blk = 0u;
            bool solid = false;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int x = x0 + j;
                const unsigned f = (f4 >> (8 * j)) & 0xffu;
                if (x > g.W) continue;
                if (f & F_SOLID) {
                    if (L[dl + j] == want) solid = true;
                    continue;
                }
                unsigned b = (unsigned)(x + 1 <= g.W && !(f & F_XP)) | (unsigned)(x - 1 >= 1 && !(f & F_XM)) << 1 |
                             (unsigned)(y + 1 <= g.H && !(f & F_YP)) << 2 | (unsigned)(y - 1 >= 1 && !(f & F_YM)) << 3 |
                             (unsigned)(rzp && !(f & F_ZP)) << 4 | (unsigned)(rzm && !(f & F_ZM)) << 5;
                if (!b) continue;
                // the face belongs to the record of its neighbour's label
                if ((b & 1u) && L[dl + j + 1] != want) b &= ~1u;
                if ((b & 2u) && L[dl + j - 1] != want) b &= ~2u;
                if ((b & 4u) && L[dl + j + dsy] != want) b &= ~4u;
                if ((b & 8u) && L[dl + j - dsy] != want) b &= ~8u;
                if ((b & 16u) && L[dl + j + dsz] != want) b &= ~16u;
                if ((b & 32u) && L[dl + j - dsz] != want) b &= ~32u;
                blk |= b << (6 * j);
            }
            if (solid) atomicOr(&rowbits[r >> 5], 1u << (r & 31));
            if (!blk) continue;
            faces += __popc(blk);
            const V4<T> pv = *reinterpret_cast<const V4<T>*>(p + c);
            const double ry = (double)y - r0y;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const unsigned b = (blk >> (6 * j)) & 63u;
                if (!b) continue;
                const double pc = (double)pv.e[j];
                const double rx = (double)(x0 + j) - r0x;
                if (b & 1u) face_term(0, +1, pc, rx, ry, rz, acc);
                if (b & 2u) face_term(0, -1, pc, rx, ry, rz, acc);
                if (b & 4u) face_term(1, +1, pc, rx, ry, rz, acc);
                if (b & 8u) face_term(1, -1, pc, rx, ry, rz, acc);
                if (b & 16u) face_term(2, +1, pc, rx, ry, rz, acc);
                if (b & 32u) face_term(2, -1, pc, rx, ry, rz, acc);
            }
        }
        __syncthreads();
        for (int i = t; i < (nrow + 31) / 32; i += BT) frontal += __popc(rowbits[i]);
        __syncthreads();
    }
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
#pragma unroll
        for (int a = 0; a < 6; ++a) acc[a] += __shfl_xor(acc[a], m, 64);
        faces += __shfl_xor(faces, m, 64);
        frontal += __shfl_xor(frontal, m, 64);
    }
    const int w = t >> 6;
    if ((t & 63) == 0) {
#pragma unroll
        for (int a = 0; a < 6; ++a) wsum[w][a] = acc[a];
        wcnt[w][0] = faces;
        wcnt[w][1] = frontal;
    }
    __syncthreads();
    if (t == 0) {
        double s[6];
        for (int a = 0; a < 6; ++a) s[a] = wsum[0][a];
        long nf = wcnt[0][0], nr = wcnt[0][1];
        for (int q = 1; q < BT / 64; ++q) {
            for (int a = 0; a < 6; ++a) s[a] += wsum[q][a];
            nf += wcnt[q][0];
            nr += wcnt[q][1];
        }
        for (int a = 0; a < 6; ++a) o[a] = s[a];
        o[6] = (double)nf;
        o[7] = (double)nr;
    }
}

// thread (k, col): the plane records of record k added in increasing z, from +0.0
__global__ void body_total_kernel(int D, int nrec, const double* __restrict__ planes, double* __restrict__ total)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nrec * BODY_REC) return;
    double s = 0.0;
    for (int z = 0; z < D; ++z) s += planes[(long)z * nrec * BODY_REC + i];
    total[i] = s;
}

}  // namespace

template <class T>
void launch_body_init(hipStream_t st, const GridDesc& g, const T* obs, int* L, unsigned long long* n_cells)
{
    const Dense dn = dense_of(g);
    hipLaunchKernelGGL((body_init_kernel<T>), dim3(blocks_for(dn.N, LT)), dim3(LT), 0, st, g, dn, obs, L, n_cells);
}
template void launch_body_init<float>(hipStream_t, const GridDesc&, const float*, int*, unsigned long long*);
template void launch_body_init<double>(hipStream_t, const GridDesc&, const double*, int*, unsigned long long*);

void launch_body_merge(hipStream_t st, const GridDesc& g, int* L, int* changed)
{
    const Dense dn = dense_of(g);
    hipLaunchKernelGGL(body_merge_kernel, dim3(blocks_for(dn.N, LT)), dim3(LT), 0, st, dn, L, changed);
}

void launch_body_count(hipStream_t st, const GridDesc& g, const int* L, int* cnt, unsigned long long* n_roots)
{
    const Dense dn = dense_of(g);
    hipLaunchKernelGGL(body_count_kernel, dim3(blocks_for(dn.N, LT)), dim3(LT), 0, st, dn, L, cnt, n_roots);
}

void launch_body_compact(hipStream_t st, const GridDesc& g, const int* L, const int* cnt, long* pairs, unsigned long long* cursor)
{
    const Dense dn = dense_of(g);
    hipLaunchKernelGGL(body_compact_kernel, dim3(blocks_for(dn.N, LT)), dim3(LT), 0, st, dn, L, cnt, pairs, cursor);
}

void launch_body_relabel(hipStream_t st, const GridDesc& g, long n_pairs, const long* pairs, const int* lab, int* L, int* cnt)
{
    const Dense dn = dense_of(g);
    if (n_pairs > 0)
        hipLaunchKernelGGL(body_scatter_kernel, dim3(blocks_for(n_pairs, LT)), dim3(LT), 0, st, n_pairs, pairs, lab, cnt);
    hipLaunchKernelGGL(body_relabel_kernel, dim3(blocks_for(dn.N, LT)), dim3(LT), 0, st, dn, L, cnt);
}

void launch_body_info(hipStream_t st, const GridDesc& g, const int* L, const uint8_t* flags, unsigned long long* info)
{
    const Dense dn = dense_of(g);
    hipLaunchKernelGGL(body_info_kernel, dim3(blocks_for(dn.N, LT)), dim3(LT), 0, st, dn, L, info);
    hipLaunchKernelGGL(body_frontal_kernel, dim3(blocks_for((long)g.H * g.D, LT / 64)), dim3(LT), 0, st, g, dn, L, flags, info);
}

template <class T>
void launch_body_forces(hipStream_t st, const GridDesc& g, const T* p, const uint8_t* flags, const int* L, const int* bbox,
                        int nrec, const double* origin, double* out, double* total)
{
    const Dense dn = dense_of(g);
    const long G = (g.W + 3) / 4;
    const int rc = (int)std::max(1L, std::min((long)ROWCHUNK, (1L << 31) / G));   // a chunk's groups fit 32 bits
    hipLaunchKernelGGL((body_forces_kernel<T>), dim3(g.D, nrec), dim3(BT), 0, st, g, dn, p, flags, L, bbox, nrec, origin[0],
                       origin[1], origin[2], out, rc);
    hipLaunchKernelGGL(body_total_kernel, dim3((nrec * BODY_REC + 63) / 64), dim3(64), 0, st, g.D, nrec, out, total);
}
template void launch_body_forces<float>(hipStream_t, const GridDesc&, const float*, const uint8_t*, const int*, const int*, int,
                                        const double*, double*, double*);
template void launch_body_forces<double>(hipStream_t, const GridDesc&, const double*, const uint8_t*, const int*, const int*, int,
                                         const double*, double*, double*);

}  // namespace fs
