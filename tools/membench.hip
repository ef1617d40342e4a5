// tools/membench.hip -- calibration of the achievable HBM / Infinity-Cache streaming rates for
// the access mixes of the solver (development tool).  hipcc --offload-arch=gfx950 -O3 membench.hip -o membench
// `membench [MB] [blocks]`: the streaming mixes; `membench zdir [planes] [rounds]`: march direction against the Infinity Cache
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdlib>
#include <vector>
#define CK(x) do { hipError_t e = (x); if (e != hipSuccess) { printf("%s: %s\n", #x, hipGetErrorString(e)); exit(1); } } while (0)

__global__ void k_read(const float4* __restrict__ a, float* out, long n4)
{
    float s = 0;
    for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < n4; i += (long)gridDim.x * blockDim.x) {
        float4 v = a[i];
        s += v.x + v.y + v.z + v.w;
    }
    if (s == 1.2345e-30f) out[0] = s;
}
__global__ void k_write(float4* __restrict__ a, long n4)
{
    for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < n4; i += (long)gridDim.x * blockDim.x)
        a[i] = make_float4(1.f, 2.f, 3.f, 4.f);
}
__global__ void k_copy(const float4* __restrict__ a, float4* __restrict__ b, long n4)
{
    for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < n4; i += (long)gridDim.x * blockDim.x) b[i] = a[i];
}
__global__ void k_triad(const float4* __restrict__ a, const float4* __restrict__ b, float4* __restrict__ c, long n4)
{
    for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < n4; i += (long)gridDim.x * blockDim.x) {
        float4 x = a[i], y = b[i];
        c[i] = make_float4(x.x + y.x, x.y + y.y, x.z + y.z, x.w + y.w);
    }
}
// contiguous chunk per block instead of grid-stride
__global__ void k_triad_chunk(const float4* __restrict__ a, const float4* __restrict__ b, float4* __restrict__ c, long n4)
{
    long per = (n4 + gridDim.x - 1) / gridDim.x;
    long beg = blockIdx.x * per, end = beg + per < n4 ? beg + per : n4;
    for (long i = beg + threadIdx.x; i < end; i += blockDim.x) {
        float4 x = a[i], y = b[i];
        c[i] = make_float4(x.x + y.x, x.y + y.y, x.z + y.z, x.w + y.w);
    }
}

// ---- mode "zdir": does a pass that starts where the previous pass ended find its first planes in the Infinity Cache? ----
// The arrays are stacks of planes (514 x 514 floats, as a 512^3 grid with its ghost cells).  The stack is cut into `nch` z chunks
// that are marched side by side, each by its own share of the workgroups, plane by plane: upward (dir = +1, every chunk from
// its first plane) or downward (dir = -1, every chunk from its last plane), as the z-marching solver kernels do.
typedef float v4f __attribute__((ext_vector_type(4)));
constexpr long PLANE4 = 514L * 514 / 4;                  // float4s per plane
template <int MIX>                                       // 0: write c;  1: read a;  2: read a, read b, write c;  3: 2 with a read nontemporal
__global__ __launch_bounds__(256) void k_march(const float4* __restrict__ a, const float4* __restrict__ b, float4* __restrict__ c,
                                               float* out, int planes, int nch, int dir)
{
    const int bpc = gridDim.x / nch, ch = blockIdx.x / bpc, bi = blockIdx.x % bpc;
    const int per = (planes + nch - 1) / nch, p0 = ch * per, p1 = min(planes, p0 + per);
    float s = 0;
    for (int k = 0; k < p1 - p0; ++k) {
        const long base = (long)(dir > 0 ? p0 + k : p1 - 1 - k) * PLANE4;
        for (long i = bi * 256L + threadIdx.x; i < PLANE4; i += bpc * 256L) {
            if (MIX == 0) c[base + i] = make_float4(1.f, 2.f, 3.f, 4.f);
            if (MIX == 1) { float4 v = a[base + i]; s += v.x + v.y + v.z + v.w; }
            if (MIX >= 2) {
                float4 x, y = b[base + i];
                if (MIX == 3) {
                    const v4f q = __builtin_nontemporal_load(reinterpret_cast<const v4f*>(a + base + i));
                    x = make_float4(q.x, q.y, q.z, q.w);
                } else x = a[base + i];
                c[base + i] = make_float4(x.x + y.x, x.y + y.y, x.z + y.z, x.w + y.w);
            }
        }
    }
    if (MIX == 1 && s == 1.2345e-30f) out[0] = s;
}

static int zdir_main(int argc, char** argv)
{
    const int planes = argc > 2 ? atoi(argv[2]) : 511;   // 511 planes of 1.057 MB = 540 MB per array
    const int rounds = argc > 3 ? atoi(argv[3]) : 5;
    const long n4 = planes * PLANE4;
    float4 *a, *b, *c; float* out;
    CK(hipMalloc(&a, n4 * 16)); CK(hipMalloc(&b, n4 * 16)); CK(hipMalloc(&c, n4 * 16)); CK(hipMalloc(&out, 64));
    CK(hipMemset(a, 0, n4 * 16)); CK(hipMemset(b, 0, n4 * 16)); CK(hipMemset(c, 0, n4 * 16));
    hipEvent_t e0, e1; CK(hipEventCreate(&e0)); CK(hipEventCreate(&e1));
    const double MB = (double)n4 * 16 / 1e6;
    auto timed = [&](auto launch) {
        CK(hipEventRecord(e0)); launch(); CK(hipEventRecord(e1)); CK(hipEventSynchronize(e1));
        float ms; CK(hipEventElapsedTime(&ms, e0, e1)); return ms * 1e3;
    };
    for (int nch : {1, 4}) {
        const int blocks = 1024;
        auto wr = [&](float4* p, int dir) { hipLaunchKernelGGL(k_march<0>, dim3(blocks), dim3(256), 0, 0, a, b, p, out, planes, nch, dir); };
        auto rd = [&](const float4* p, int dir) { hipLaunchKernelGGL(k_march<1>, dim3(blocks), dim3(256), 0, 0, p, b, c, out, planes, nch, dir); };
        auto mix = [&](const float4* s, float4* d, int dir) { hipLaunchKernelGGL(k_march<2>, dim3(blocks), dim3(256), 0, 0, s, b, d, out, planes, nch, dir); };
        auto mixnt = [&](const float4* s, float4* d, int dir) { hipLaunchKernelGGL(k_march<3>, dim3(blocks), dim3(256), 0, 0, s, b, d, out, planes, nch, dir); };
        for (int r = 0; r < rounds; ++r) {
            // 1. one array: written upward, then read once, upward or downward, each after a fresh write
            wr(a, +1); const double up = timed([&] { rd(a, +1); });
            wr(a, +1); const double dn = timed([&] { rd(a, -1); });
            printf("zdir read   nch %d round %d  %.0f MB  after upward write: read up %7.1f us  read down %7.1f us  down/up %.3f\n",
                   nch, r, MB, up, dn, dn / up);
        }
        for (int r = 0; r < rounds; ++r) {
            // 2. the sweep's mix (read iterate, read rhs, write new iterate): the pass after an upward pass
            mix(a, c, +1); const double up = timed([&] { mix(c, a, +1); });
            mix(a, c, +1); const double dn = timed([&] { mix(c, a, -1); });
            printf("zdir 2R+1W  nch %d round %d  %.0f MB/array  after upward pass: pass up %7.1f us  pass down %7.1f us  down/up %.3f\n",
                   nch, r, MB, up, dn, dn / up);
        }
        for (int r = 0; r < rounds; ++r) {
            // 3. 26 passes in a row, ping-pong between two arrays: all upward, or alternating
            mix(a, c, +1);
            const double up = timed([&] { for (int k = 0; k < 26; ++k) mix(k & 1 ? a : c, k & 1 ? c : a, +1); }) / 26;
            mix(a, c, +1);
            const double al = timed([&] { for (int k = 0; k < 26; ++k) mix(k & 1 ? a : c, k & 1 ? c : a, k & 1 ? +1 : -1); }) / 26;
            // ... and with the old iterate (dead after the pass) read nontemporal, so that it might not take up the cache
            mixnt(a, c, +1);
            const double nu = timed([&] { for (int k = 0; k < 26; ++k) mixnt(k & 1 ? a : c, k & 1 ? c : a, +1); }) / 26;
            mixnt(a, c, +1);
            const double na = timed([&] { for (int k = 0; k < 26; ++k) mixnt(k & 1 ? a : c, k & 1 ? c : a, k & 1 ? +1 : -1); }) / 26;
            printf("zdir 26pass nch %d round %d  %.0f MB/array  per pass: all up %7.1f us  alternating %7.1f us  alt/up %.3f;  nt iterate: all up %7.1f  alternating %7.1f\n",
                   nch, r, MB, up, al, al / up, nu, na);
        }
    }
    return 0;
}

int main(int argc, char** argv)
{
    if (argc > 1 && argv[1][0] == 'z') return zdir_main(argc, argv);
    long mb = argc > 1 ? atol(argv[1]) : 543;
    int blocks = argc > 2 ? atoi(argv[2]) : 2048;
    long n4 = mb * 1000000L / 16;
    float4 *a, *b, *c; float* out;
    CK(hipMalloc(&a, n4 * 16)); CK(hipMalloc(&b, n4 * 16)); CK(hipMalloc(&c, n4 * 16)); CK(hipMalloc(&out, 64));
    CK(hipMemset(a, 0, n4 * 16)); CK(hipMemset(b, 0, n4 * 16)); CK(hipMemset(c, 0, n4 * 16));
    hipEvent_t e0, e1; CK(hipEventCreate(&e0)); CK(hipEventCreate(&e1));
    const int reps = 20;
    auto timeit = [&](const char* name, double bytes, auto launch) {
        launch(); CK(hipDeviceSynchronize());
        CK(hipEventRecord(e0));
        for (int r = 0; r < reps; ++r) launch();
        CK(hipEventRecord(e1)); CK(hipEventSynchronize(e1));
        float ms; CK(hipEventElapsedTime(&ms, e0, e1)); ms /= reps;
        printf("%-16s %4ld MB/array  blocks %5d  %8.1f us  %7.0f GB/s\n", name, mb, blocks, ms * 1e3, bytes / ms / 1e6);
    };
    double B = (double)n4 * 16;
    timeit("read", B, [&] { hipLaunchKernelGGL(k_read, dim3(blocks), dim3(256), 0, 0, a, out, n4); });
    timeit("write", B, [&] { hipLaunchKernelGGL(k_write, dim3(blocks), dim3(256), 0, 0, c, n4); });
    timeit("copy", 2 * B, [&] { hipLaunchKernelGGL(k_copy, dim3(blocks), dim3(256), 0, 0, a, c, n4); });
    timeit("triad 2R+1W", 3 * B, [&] { hipLaunchKernelGGL(k_triad, dim3(blocks), dim3(256), 0, 0, a, b, c, n4); });
    timeit("triad chunked", 3 * B, [&] { hipLaunchKernelGGL(k_triad_chunk, dim3(blocks), dim3(256), 0, 0, a, b, c, n4); });
    return 0;
}
