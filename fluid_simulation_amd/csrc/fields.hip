// fields.hip -- the small passes over whole fields: stand-alone setBounds, the flag, kill and clean tables,
// inlet, pack / unpack, copy, stats and the point poke.  Moved out of kernels.hip unchanged.
#include <hip/hip_runtime.h>
#include "kernels.h"
#include "kernels_dev.h"

namespace fs {

// =====================================================================================
// Stand-alone setBounds (simulation.cpp:183-246): faces first, then the zeroing passes.
// The hot kernels fuse this; the stand-alone form serves fs_set_bounds and odd callers.
// =====================================================================================
template <class T>
__global__ void bounds_faces_kernel(GridDesc g, SlabCtx sc, T* q, int b)
{
    const int W = g.W, H = g.H, D = g.D;
    const long nx = (long)H * D, ny = (long)W * D, nz = (long)W * H;
    for (long t = blockIdx.x * (long)blockDim.x + threadIdx.x; t < nx + ny + nz; t += (long)gridDim.x * blockDim.x) {
        if (t < nx) {
            int y = 1 + (int)(t % H), z = 1 + (int)(t / H);
            T in = q[cell(g, 1, y, z)];
            q[cell(g, 0, y, z)] = (b == 1) ? -in : in;
            q[cell(g, W + 1, y, z)] = q[cell(g, W, y, z)];
        } else if (t < nx + ny) {
            long u = t - nx;
            int x = 1 + (int)(u % W), z = 1 + (int)(u / W);
            T lo = q[cell(g, x, 1, z)], hi = q[cell(g, x, H, z)];
            q[cell(g, x, 0, z)] = (b == 2) ? -lo : lo;
            q[cell(g, x, H + 1, z)] = (b == 2) ? -hi : hi;
        } else {
            long u = t - nx - ny;
            int x = 1 + (int)(u % W), y = 1 + (int)(u / W);
            if (sc.lo_wall) {
                T lo = q[cell(g, x, y, 1)];
                q[cell(g, x, y, 0)] = (b == 3) ? -lo : lo;
            }
            if (sc.hi_wall) {
                T hi = q[cell(g, x, y, D)];
                q[cell(g, x, y, D + 1)] = (b == 3) ? -hi : hi;
            }
        }
    }
}

template <class T>
__global__ void bounds_zero_kernel(GridDesc g, T* q, const uint8_t* flags, int b)
{
    const int x = 1 + blockIdx.x * blockDim.x + threadIdx.x;
    const int y = 1 + blockIdx.y * blockDim.y + threadIdx.y;
    const int z = 1 + blockIdx.z;
    if (x > g.W || y > g.H) return;
    const unsigned zero_bits = (b == 0) ? F_SOLID : (F_SOLID | F_NEAR);
    long c = cell(g, x, y, z);
    if (flags[c] & zero_bits) q[c] = (T)0;
}


template <class T>
void launch_set_bounds(hipStream_t st, const GridDesc& g, const SlabCtx& sc, T* q, const uint8_t* flags, int b)
{
    long faces = (long)g.H * g.D + (long)g.W * g.D + (long)g.W * g.H;
    int nb = (int)((faces + 255) / 256);
    if (nb > 4096) nb = 4096;
    hipLaunchKernelGGL((bounds_faces_kernel<T>), dim3(nb), dim3(256), 0, st, g, sc, q, b);
    hipLaunchKernelGGL((bounds_zero_kernel<T>), cell_grid(g), cell_block(), 0, st, g, q, flags, b);
}
template void launch_set_bounds<float>(hipStream_t, const GridDesc&, const SlabCtx&, float*, const uint8_t*, int);
template void launch_set_bounds<double>(hipStream_t, const GridDesc&, const SlabCtx&, double*, const uint8_t*, int);

// =====================================================================================
// Flag bytes from the obstacle array.  Tests follow the reference literally:
// solid <=> obs == 1 (simulation.cpp:222), fluid neighbour <=> in range && obs == 0 (:307).
// Under z-slabs "in range" refers to the global depth; the halo planes of `obs` hold the
// neighbouring slabs' cells.
// =====================================================================================
template <class T>
__global__ void build_flags_kernel(GridDesc g, SlabCtx sc, const T* __restrict__ obs, uint8_t* __restrict__ flags,
                                   int zlo)
{
    const int x = 1 + blockIdx.x * blockDim.x + threadIdx.x;
    const int y = 1 + blockIdx.y * blockDim.y + threadIdx.y;
    const int z = zlo + blockIdx.z;
    if (x > g.W || y > g.H) return;
    const long c = cell(g, x, y, z);
    const int zg = z + sc.zoff;
    const bool rxp = x + 1 <= g.W, rxm = x - 1 >= 1, ryp = y + 1 <= g.H, rym = y - 1 >= 1;
    const bool rzp = zg + 1 <= sc.Dglobal, rzm = zg - 1 >= 1;
    const T one = (T)1, zero = (T)0;
    unsigned f = 0;
    if (obs[c] == one) {
        f = F_SOLID;
    } else {
        bool near = (rxp && obs[c + 1] == one) || (rxm && obs[c - 1] == one) || (ryp && obs[c + g.sy] == one) ||
                    (rym && obs[c - g.sy] == one) || (rzp && obs[c + g.sz] == one) || (rzm && obs[c - g.sz] == one);
        if (near) f |= F_NEAR;
    }
    if (rxp && obs[c + 1] == zero) f |= F_XP;
    if (rxm && obs[c - 1] == zero) f |= F_XM;
    if (ryp && obs[c + g.sy] == zero) f |= F_YP;
    if (rym && obs[c - g.sy] == zero) f |= F_YM;
    if (rzp && obs[c + g.sz] == zero) f |= F_ZP;
    if (rzm && obs[c - g.sz] == zero) f |= F_ZM;
    flags[c] = (uint8_t)f;
}

template <class T>
void launch_build_flags(hipStream_t st, const GridDesc& g, const SlabCtx& sc, const T* obs, uint8_t* flags)
{
    // with zh-deep halos the flags of the first zh-1 halo planes on a slab side are needed too (a fused
    // pass recomputes the lower levels of those planes); the outermost halo plane only serves as their z neighbour
    const int zlo = (g.zh >= 2 && !sc.lo_wall) ? 2 - g.zh : 1, zhi = (g.zh >= 2 && !sc.hi_wall) ? g.D + g.zh - 1 : g.D;
    dim3 grid = cell_grid(g);
    grid.z = zhi - zlo + 1;
    hipLaunchKernelGGL((build_flags_kernel<T>), grid, cell_block(), 0, st, g, sc, obs, flags, zlo);
}
template void launch_build_flags<float>(hipStream_t, const GridDesc&, const SlabCtx&, const float*, uint8_t*);
template void launch_build_flags<double>(hipStream_t, const GridDesc&, const SlabCtx&, const double*, uint8_t*);

// Kill bytes for the sweep kernels: one byte per lane group (four x-consecutive cells starting at
// x = 1 mod 4), bits 0-3 = solid, bits 4-7 = solid or next to a solid; byte index = (cell + 3) / 4.
// A quarter of the flag traffic, and the sweeps need nothing else of the flags.
__global__ void build_kill_kernel(GridDesc g, const uint8_t* __restrict__ flags, uint8_t* __restrict__ kill, int zlo)
{
    const int gx = blockIdx.x * blockDim.x + threadIdx.x;            // group index along x
    const int y = 1 + blockIdx.y * blockDim.y + threadIdx.y;
    const int z = zlo + blockIdx.z;
    const int x0 = 1 + 4 * gx;
    if (x0 > g.W || y > g.H) return;
    const long c = cell(g, x0, y, z);
    const unsigned f = *reinterpret_cast<const unsigned*>(flags + c);
    unsigned out = 0;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const unsigned fe = (f >> (8 * e)) & 0xffu;
        if (fe & F_SOLID) out |= 1u << e;
        if (fe & (F_SOLID | F_NEAR)) out |= 16u << e;
    }
    kill[(c + 3) >> 2] = (uint8_t)out;
}
void launch_build_kill(hipStream_t st, const GridDesc& g, const SlabCtx& sc, const uint8_t* flags, uint8_t* kill)
{
    const int zlo = (g.zh >= 2 && !sc.lo_wall) ? 2 - g.zh : 1, zhi = (g.zh >= 2 && !sc.hi_wall) ? g.D + g.zh - 1 : g.D;
    const int ng = (g.W + 3) / 4;
    hipLaunchKernelGGL(build_kill_kernel, dim3((ng + 63) / 64, (g.H + 3) / 4, zhi - zlo + 1), dim3(64, 4, 1), 0, st, g,
                       flags, kill, zlo);
}

// Clean table of the mask-free three-sweep build (chunk_plan.h): one workgroup per plane 0..D+1, one wave per row at a time;
// bit y of the plane's words is set iff no kill byte of row y has a bit in either nibble.  Kill bytes outside rows 1..H,
// planes 1..D are the zeros the array was cleared to.
__global__ void build_clean_kernel(GridDesc g, const uint8_t* __restrict__ kill, uint32_t* __restrict__ tab, int words)
{
    __shared__ uint32_t w[64];
    const int z = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int i = threadIdx.x; i < words; i += blockDim.x) w[i] = 0u;
    __syncthreads();
    const int ng = (g.W + 3) / 4;
    for (int y = wave; y <= g.H + 1; y += blockDim.x / 64) {
        bool dirty = false;
        for (int gx = lane; gx < ng; gx += 64) dirty |= kill[(cell(g, 1 + 4 * gx, y, z) + 3) >> 2] != 0;
        if (__builtin_amdgcn_ballot_w64(dirty) == 0 && lane == 0) atomicOr(&w[y >> 5], 1u << (y & 31));
    }
    __syncthreads();
    for (int i = threadIdx.x; i < words; i += blockDim.x) tab[(long)z * words + i] = w[i];
}
void launch_build_clean(hipStream_t st, const GridDesc& g, const uint8_t* kill, uint32_t* tab, int words)
{
    hipLaunchKernelGGL(build_clean_kernel, dim3(g.D + 2), dim3(256), 0, st, g, kill, tab, words);
}

// =====================================================================================
// Inlet forcing: velocity (speed,0,0) on the x=1 face (simulation.cpp:103-105) and
// +amount density on the same face (simulation.cpp:65-67).
// =====================================================================================
template <class T>
__global__ void inlet_velocity_kernel(GridDesc g, T* vx, T* vy, T* vz, T speed, int zlo)
{
    const int y = 1 + blockIdx.x * blockDim.x + threadIdx.x;
    const int z = zlo + blockIdx.y;
    if (y > g.H) return;
    const long c = cell(g, 1, y, z);
    vx[c] = speed;
    vy[c] = (T)0;
    vz[c] = (T)0;
}
template <class T>
__global__ void inlet_density_kernel(GridDesc g, T* dens, T amount, int zlo)
{
    const int y = 1 + blockIdx.x * blockDim.x + threadIdx.x;
    const int z = zlo + blockIdx.y;
    if (y > g.H) return;
    dens[cell(g, 1, y, z)] += amount;
}
template <class T>
void launch_inlet_velocity(hipStream_t st, const GridDesc& g, const SlabCtx& sc, T* vx, T* vy, T* vz, T speed)
{
    // a slab also forces the inlet cells of its halo planes (they are interior planes of the
    // neighbouring slab), so the halos stay current without an exchange
    const int zlo = sc.lo_wall ? 1 : 1 - g.zh, zhi = sc.hi_wall ? g.D : g.D + g.zh;
    hipLaunchKernelGGL((inlet_velocity_kernel<T>), dim3((g.H + 63) / 64, zhi - zlo + 1), dim3(64), 0, st, g, vx, vy, vz,
                       speed, zlo);
}
template <class T>
void launch_inlet_density(hipStream_t st, const GridDesc& g, const SlabCtx& sc, T* dens, T amount)
{
    const int zlo = sc.lo_wall ? 1 : 1 - g.zh, zhi = sc.hi_wall ? g.D : g.D + g.zh;
    hipLaunchKernelGGL((inlet_density_kernel<T>), dim3((g.H + 63) / 64, zhi - zlo + 1), dim3(64), 0, st, g, dens, amount,
                       zlo);
}
template void launch_inlet_velocity<float>(hipStream_t, const GridDesc&, const SlabCtx&, float*, float*, float*, float);
template void launch_inlet_velocity<double>(hipStream_t, const GridDesc&, const SlabCtx&, double*, double*, double*, double);
template void launch_inlet_density<float>(hipStream_t, const GridDesc&, const SlabCtx&, float*, float);
template void launch_inlet_density<double>(hipStream_t, const GridDesc&, const SlabCtx&, double*, double);

// =====================================================================================
// Layout conversion: pitched device field <-> the reference's dense padded array
// (simulation.h:9, the frame-dump layout of simulation.cpp:143-147).
// =====================================================================================
template <class T, class U>
__global__ void pack_kernel(GridDesc g, const T* __restrict__ f, U* __restrict__ dense, int zlo)
{
    const int x = blockIdx.x * blockDim.x + threadIdx.x;
    const int y = blockIdx.y * blockDim.y + threadIdx.y;
    const int z = zlo + blockIdx.z;
    if (x > g.W + 1 || y > g.H + 1) return;
    dense[(long)x + (long)y * (g.W + 2) + (long)(z - zlo) * (g.W + 2) * (g.H + 2)] = (U)f[cell(g, x, y, z)];
}
template <class T, class U>
__global__ void unpack_kernel(GridDesc g, const U* __restrict__ dense, T* __restrict__ f, int zlo)
{
    const int x = blockIdx.x * blockDim.x + threadIdx.x;
    const int y = blockIdx.y * blockDim.y + threadIdx.y;
    const int z = zlo + blockIdx.z;
    if (x > g.W + 1 || y > g.H + 1) return;
    f[cell(g, x, y, z)] = (T)dense[(long)x + (long)y * (g.W + 2) + (long)(z - zlo) * (g.W + 2) * (g.H + 2)];
}
template <class T, class U>
void launch_pack(hipStream_t st, const GridDesc& g, const T* field, U* dense, int zlo, int zhi)
{
    if (zhi < zlo) return;
    hipLaunchKernelGGL((pack_kernel<T, U>), dim3((g.W + 2 + 63) / 64, (g.H + 2 + 3) / 4, zhi - zlo + 1), dim3(64, 4, 1),
                       0, st, g, field, dense, zlo);
}
template <class T, class U>
void launch_unpack(hipStream_t st, const GridDesc& g, const U* dense, T* field, int zlo, int zhi)
{
    if (zhi < zlo) return;
    hipLaunchKernelGGL((unpack_kernel<T, U>), dim3((g.W + 2 + 63) / 64, (g.H + 2 + 3) / 4, zhi - zlo + 1),
                       dim3(64, 4, 1), 0, st, g, dense, field, zlo);
}
#define FS_INST_PACK(T, U)                                                                     \
    template void launch_pack<T, U>(hipStream_t, const GridDesc&, const T*, U*, int, int);     \
    template void launch_unpack<T, U>(hipStream_t, const GridDesc&, const U*, T*, int, int);
FS_INST_PACK(float, float)
FS_INST_PACK(float, double)
FS_INST_PACK(double, float)
FS_INST_PACK(double, double)
FS_INST_PACK(float, uint8_t)
FS_INST_PACK(double, uint8_t)

template <class T>
__global__ void copy_kernel(const T* __restrict__ src, T* __restrict__ dst, long n4)
{
    // whole allocation, 16 B per lane (allocation length is a multiple of 4 elements)
    for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < n4; i += (long)gridDim.x * blockDim.x)
        reinterpret_cast<V4<T>*>(dst)[i] = reinterpret_cast<const V4<T>*>(src)[i];
}
template <class T>
void launch_copy(hipStream_t st, const GridDesc& g, const T* src, T* dst)
{
    // src/dst are the shifted pointers; copy the underlying allocations
    long n4 = g.n / 4;
    hipLaunchKernelGGL((copy_kernel<T>), dim3(2048), dim3(256), 0, st, src - g.lead, dst - g.lead, n4);
}
template void launch_copy<float>(hipStream_t, const GridDesc&, const float*, float*);
template void launch_copy<double>(hipStream_t, const GridDesc&, const double*, double*);

// =====================================================================================
// Diagnostics of Simulation::run(): sum / min / max of a whole padded array
// (simulation.cpp:73-90).  Two-stage reduction in double.
// =====================================================================================
template <class T>
__global__ __launch_bounds__(256) void stats_partial_kernel(GridDesc g, const T* __restrict__ f, double* part, int zlo,
                                                             int zhi)
{
    const long rows = (long)(g.H + 2) * (zhi - zlo + 1);
    // the extremes start from the infinities: a field that is +Inf everywhere, or above any finite start, has itself as minimum
    double s = 0.0, mn = (double)INFINITY, mx = -(double)INFINITY;
    for (long r = blockIdx.x; r < rows; r += gridDim.x) {
        int y = (int)(r % (g.H + 2)), z = zlo + (int)(r / (g.H + 2));
        for (int x = threadIdx.x; x <= g.W + 1; x += blockDim.x) {
            double v = (double)f[cell(g, x, y, z)];
            s += v;
            mn = v < mn ? v : mn;
            mx = v > mx ? v : mx;
        }
    }
    __shared__ double sh[3][256];
    sh[0][threadIdx.x] = s; sh[1][threadIdx.x] = mn; sh[2][threadIdx.x] = mx;
    __syncthreads();
    for (int k = 128; k > 0; k >>= 1) {
        if ((int)threadIdx.x < k) {
            sh[0][threadIdx.x] += sh[0][threadIdx.x + k];
            sh[1][threadIdx.x] = fmin(sh[1][threadIdx.x], sh[1][threadIdx.x + k]);
            sh[2][threadIdx.x] = fmax(sh[2][threadIdx.x], sh[2][threadIdx.x + k]);
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        part[3 * blockIdx.x + 0] = sh[0][0];
        part[3 * blockIdx.x + 1] = sh[1][0];
        part[3 * blockIdx.x + 2] = sh[2][0];
    }
}
__global__ void stats_final_kernel(const double* part, int n, double* out3)
{
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    double s = 0.0, mn = (double)INFINITY, mx = -(double)INFINITY;
    for (int i = 0; i < n; ++i) {
        s += part[3 * i];
        mn = fmin(mn, part[3 * i + 1]);
        mx = fmax(mx, part[3 * i + 2]);
    }
    out3[0] = s; out3[1] = mn; out3[2] = mx;
}
template <class T>
void launch_stats(hipStream_t st, const GridDesc& g, const T* field, double* out3, double* scratch, int nscratch,
                  int zlo, int zhi)
{
    int nb = nscratch / 3;
    if (nb > 1024) nb = 1024;
    hipLaunchKernelGGL((stats_partial_kernel<T>), dim3(nb), dim3(256), 0, st, g, field, scratch, zlo, zhi);
    hipLaunchKernelGGL(stats_final_kernel, dim3(1), dim3(64), 0, st, scratch, nb, out3);
}
template void launch_stats<float>(hipStream_t, const GridDesc&, const float*, double*, double*, int, int, int);
template void launch_stats<double>(hipStream_t, const GridDesc&, const double*, double*, double*, int, int, int);

template <class T>
__global__ void point_kernel(T* p, long idx, T amount, int set_instead)
{
    if (threadIdx.x == 0 && blockIdx.x == 0) p[idx] = set_instead ? amount : p[idx] + amount;
}
template <class T>
void launch_point_add(hipStream_t st, T* p, long idx, T amount, int set_instead)
{
    hipLaunchKernelGGL((point_kernel<T>), dim3(1), dim3(64), 0, st, p, idx, amount, set_instead);
}
template void launch_point_add<float>(hipStream_t, float*, long, float, int);
template void launch_point_add<double>(hipStream_t, double*, long, double, int);

}  // namespace fs
