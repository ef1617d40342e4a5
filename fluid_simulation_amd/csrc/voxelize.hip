// voxelize.hip -- STL -> solid voxels on the GPU.
//
// Restates loadSTLIntoObstacles (object_loader.cpp:270-452) at its one-thread semantics:
// the reference draws six numbers from one std::minstd_rand stream for every sample point
// that survives the coarse-grid rejection, in i,j,k order.  Here the rejection test runs
// for all samples in parallel, an exclusive scan gives every surviving sample its rank r
// in that order, and the sample jumps the generator ahead by 6r draws (x_n = x_0 * a^n mod
// m), so each sample sees exactly the numbers the sequential loop would have given it and
// the mask is reproducible bit for bit from (STL, arguments, seed).
//
// Mesh parsing, the Euler rotation (host cosf/sinf, like the reference) and the 64^3
// coarse occupancy grid are one-off host work on O(triangles) data; the
// O(samples x triangles) ray-parity test is the kernel.  Compiled with -ffp-contract=off.
// The host work and every per-sample function the kernels call live in voxelize_math.h, plain
// C++ that tests/test_voxelize_cpu.py compiles on the host; here are the kernels, the scan
// and the launches.
#include <hip/hip_runtime.h>
#include <rocprim/device/device_scan.hpp>

#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "kernels.h"
#include "voxelize.h"
#include "voxelize_math.h"

namespace fs {

namespace {

using namespace vox;

// ---------------------------------------------------------------------------- device

// VoxelGrid::contains, object_loader.cpp:79-87
__global__ void keep_kernel(VoxParams q, const uint8_t* __restrict__ occ, uint8_t* __restrict__ keep, long nsamp)
{
    long n = blockIdx.x * (long)blockDim.x + threadIdx.x;
    if (n >= nsamp) return;
    keep[n] = sample_kept(q, occ, n);
}

__global__ void compact_kernel(const uint8_t* __restrict__ keep, const unsigned* __restrict__ rank,
                               unsigned* __restrict__ list, long nsamp)
{
    long n = blockIdx.x * (long)blockDim.x + threadIdx.x;
    if (n >= nsamp) return;
    if (keep[n]) list[rank[n]] = (unsigned)n;
}

constexpr int TILE = 256;   // triangles staged in LDS per pass (9 KB)

// One lane per surviving sample; all triangles stream through LDS in tiles that the whole
// block tests against (object_loader.cpp:417-444).
__global__ __launch_bounds__(256) void parity_kernel(VoxParams q, const float* __restrict__ tri,
                                                      const unsigned* __restrict__ list, long nkept,
                                                      int* __restrict__ cells, unsigned long long* __restrict__ count)
{
    __shared__ float sh[TILE * 9];
    const long r = blockIdx.x * (long)blockDim.x + threadIdx.x;
    const bool on = r < nkept;
    float px = 0, py = 0, pz = 0, dx = 1, dy = 1, dz = 1;
    if (on) {
        sample_point(q, (long)list[r], px, py, pz);
        unsigned st = lcg_jump(q.seed, (unsigned long long)r);
        px += lcg_jitter(st);                                    // :417-419
        py += lcg_jitter(st);
        pz += lcg_jitter(st);
        dx = lcg_unit(st);                                       // :422
        dy = lcg_unit(st);
        dz = lcg_unit(st);
    }
    int crossings = 0;
    for (int base = 0; base < q.ntri; base += TILE) {
        const int cnt = min(TILE, q.ntri - base);
        __syncthreads();
        for (int i = threadIdx.x; i < cnt * 9; i += blockDim.x) sh[i] = tri[(long)base * 9 + i];
        __syncthreads();
        if (on)
            for (int t = 0; t < cnt; ++t) crossings += ray_hits(px, py, pz, dx, dy, dz, &sh[t * 9]) ? 1 : 0;
    }
    int id;
    if (on && (crossings & 1) && sample_cell(q, px, py, pz, id)) {   // :432-434
        unsigned long long at = atomicAdd(count, 1ull);
        cells[at] = id;
    }
}

template <class T>
__global__ void mark_cells_kernel(GridDesc g, SlabCtx sc, T* obs, const int* __restrict__ cells, long n)
{
    long i = blockIdx.x * (long)blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int id = cells[i];
    const int x = id % (g.W + 2), y = (id / (g.W + 2)) % (g.H + 2), z = id / ((g.W + 2) * (g.H + 2));
    const int zl = z - sc.zoff;
    // a slab also records the solids of its halo planes (the flag build reads them)
    if (zl < 1 - g.zh || zl > g.D + g.zh) return;
    obs[(long)x + (long)y * g.sy + (long)zl * g.sz] = (T)1;     // Simulation::addObstacle, simulation.cpp:157
}

#define VX_HIP(expr)                                                                     \
    do {                                                                                 \
        hipError_t e_ = (expr);                                                          \
        if (e_ != hipSuccess) { out->error = std::string(#expr ": ") + hipGetErrorString(e_); return -3; } \
    } while (0)

}  // namespace

template <class T>
void launch_mark_cells(hipStream_t st, const GridDesc& g, const SlabCtx& sc, T* obs, const int* cells, long n)
{
    if (n <= 0) return;
    hipLaunchKernelGGL((mark_cells_kernel<T>), dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, g, sc, obs, cells, n);
}
template void launch_mark_cells<float>(hipStream_t, const GridDesc&, const SlabCtx&, float*, const int*, long);
template void launch_mark_cells<double>(hipStream_t, const GridDesc&, const SlabCtx&, double*, const int*, long);

int voxelize_stl(hipStream_t st, const char* path, int W, int H, int D, float scale, float rot_x, float rot_y,
                 float rot_z, float tr_x, float tr_y, float tr_z, unsigned seed, bool quiet, VoxelResult* out)
{
    std::vector<Tri> raw;
    if (!read_stl(path, raw)) {
        fprintf(stderr, "Error: Cannot open STL file: %s\n", path);          // :101
        fprintf(stderr, "Failed to load STL: %s\n", path);                   // :283
        out->error = std::string("cannot open STL file: ") + path;
        return -2;
    }
    if (!quiet) printf("Loaded %zu triangles.\n", raw.size());               // :172
    if (raw.empty()) {
        fprintf(stderr, "Failed to load STL: %s\n", path);
        out->error = std::string("no triangles in STL file: ") + path;
        return -2;
    }

    VoxSetup su;
    setup(raw, W, H, D, scale, rot_x, rot_y, rot_z, tr_x, tr_y, tr_z, seed, su);
    const VoxParams& q = su.q;
    const std::vector<float>& rt = su.rt;
    const std::vector<uint8_t>& occ = su.occ;
    const int ns = q.ns;
    const float res = q.res;
    if (!quiet) {
        printf("Rotated object voxelization:\n  Grid: %d x %d x %d\n  Resolution: %g\n", ns, ns, ns, res);
        printf("  Rotations: X=%g\xC2\xB0 Y=%g\xC2\xB0 Z=%g\xC2\xB0\n", rot_x, rot_y, rot_z);
        printf("Built spatial grid for fast rejection.\n");          // :391
    }

    out->ntri = (long)raw.size();
    out->ns = ns;
    out->resolution = res;
    out->added = 0;
    const long nsamp = (long)ns * ns * ns;
    if (nsamp <= 0) {
        if (!quiet) printf("Added 0 obstacle points.\n");
        return 0;
    }

    // one device slab for everything: tri | occ | keep | rank | list | count
    auto up = [](size_t v) { return (v + 255) / 256 * 256; };
    const size_t o_tri = 0;
    const size_t o_occ = o_tri + up(rt.size() * sizeof(float));
    const size_t o_keep = o_occ + up(occ.size());
    const size_t o_rank = o_keep + up((size_t)nsamp);
    const size_t o_list = o_rank + up((size_t)nsamp * 4);
    const size_t o_cnt = o_list + up((size_t)nsamp * 4);
    size_t scan_bytes = 0;
    rocprim::exclusive_scan((void*)nullptr, scan_bytes, (uint8_t*)nullptr, (unsigned*)nullptr, 0u, (size_t)nsamp,
                            rocprim::plus<unsigned>(), st);
    const size_t o_scan = o_cnt + 256;
    const size_t total = o_scan + up(scan_bytes);
    char* w = nullptr;
    VX_HIP(hipMalloc((void**)&w, total));
    out->d_work = w;
    VX_HIP(hipMemcpyAsync(w + o_tri, rt.data(), rt.size() * sizeof(float), hipMemcpyHostToDevice, st));
    VX_HIP(hipMemcpyAsync(w + o_occ, occ.data(), occ.size(), hipMemcpyHostToDevice, st));
    VX_HIP(hipMemsetAsync(w + o_cnt, 0, 256, st));

    uint8_t* d_keep = (uint8_t*)(w + o_keep);
    unsigned* d_rank = (unsigned*)(w + o_rank);
    unsigned* d_list = (unsigned*)(w + o_list);
    unsigned long long* d_cnt = (unsigned long long*)(w + o_cnt);
    const unsigned nb = (unsigned)((nsamp + 255) / 256);
    hipLaunchKernelGGL(keep_kernel, dim3(nb), dim3(256), 0, st, q, (const uint8_t*)(w + o_occ), d_keep, nsamp);
    VX_HIP(rocprim::exclusive_scan((void*)(w + o_scan), scan_bytes, d_keep, d_rank, 0u, (size_t)nsamp,
                                   rocprim::plus<unsigned>(), st));
    hipLaunchKernelGGL(compact_kernel, dim3(nb), dim3(256), 0, st, (const uint8_t*)d_keep, (const unsigned*)d_rank,
                       d_list, nsamp);
    unsigned last_rank = 0;
    uint8_t last_keep = 0;
    VX_HIP(hipMemcpyAsync(&last_rank, d_rank + (nsamp - 1), 4, hipMemcpyDeviceToHost, st));
    VX_HIP(hipMemcpyAsync(&last_keep, d_keep + (nsamp - 1), 1, hipMemcpyDeviceToHost, st));
    VX_HIP(hipStreamSynchronize(st));
    const long nkept = (long)last_rank + (last_keep ? 1 : 0);

    if (nkept > 0) {
        VX_HIP(hipMalloc((void**)&out->d_cells, (size_t)nkept * sizeof(int)));
        hipLaunchKernelGGL(parity_kernel, dim3((unsigned)((nkept + 255) / 256)), dim3(256), 0, st, q,
                           (const float*)(w + o_tri), (const unsigned*)d_list, nkept, out->d_cells, d_cnt);
        unsigned long long cnt = 0;
        VX_HIP(hipMemcpyAsync(&cnt, d_cnt, 8, hipMemcpyDeviceToHost, st));
        VX_HIP(hipStreamSynchronize(st));
        out->added = (long)cnt;
    }
    if (!quiet) printf("Added %ld obstacle points.\n", out->added);          // :451
    return 0;
}

void voxelize_free(VoxelResult* r)
{
    if (r->d_cells) hipFree(r->d_cells);
    if (r->d_work) hipFree(r->d_work);
    r->d_cells = nullptr;
    r->d_work = nullptr;
}

}  // namespace fs
