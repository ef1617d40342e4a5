// inflow.hip -- turbulent inflow: the x = 1 face of the three velocities from a mean profile, a gust factor and a
// synthetic-eddy field (include/fluidsim.h, "turbulent inflow").  The arithmetic is inflow.h's; this file only moves the data.
//
// Two kernels.  inflow_table_kernel: one thread per eddy writes the step's table entry (ey, ez, A * f_x, signs; 32 bytes).
// inflow_plane_kernel: a workgroup of four waves owns a PY x PZ patch of the plane, one cell per lane.  It streams the table
// in tiles of one entry per lane (two 16-byte loads), keeps the entries whose support can reach the patch -- each wave's
// ballot and the lane's prefix count give the entry its place, the waves' counts chain the waves, so the kept entries stand
// in LDS in ascending k -- and, when the list could not take another tile or the table ends, every lane sums the list for its
// cell (all lanes read the same entry: an LDS broadcast).  Only about (2 sigma)^2 / (h d) of all pairs are non-zero; with the
// 16 x 16 patch a lane evaluates (16 + 2 sigma + 2)^2 / (2 sigma)^2 times the pairs that count instead of all of them
// (measured at 512 x 512, 8679 eddies, sigma = 8: 0.048 ms against 1.75 ms with every entry kept).  A
// lane adds for its own cell only; the order of every sum is the table's.  The patch's cells are strided stores whatever
// its shape (x is fixed), so the patch is square, which keeps the fewest entries.
#include "inflow.h"
#include "kernels_dev.h"

namespace fs {

namespace {

constexpr int INFLOW_PY = 16, INFLOW_PZ = 16;           // the patch
constexpr int INFLOW_NT = INFLOW_PY * INFLOW_PZ;        // lanes = cells of a patch = entries of a tile
constexpr int INFLOW_CAP = 2 * INFLOW_NT;               // entries the LDS list holds (16 KB)

__global__ __launch_bounds__(256) void inflow_table_kernel(InflowParams p, long t, double inv, InflowEntry* tab, double* eddies)
{
    const int k = blockIdx.x * 256 + threadIdx.x;
    if (k >= p.n) return;
    const InflowEddy e = inflow_eddy(p, k, t);
    if (tab) tab[k] = inflow_entry(e, p.amp, inv);
    if (eddies) {
        double* o = eddies + (size_t)k * 6;
        o[0] = e.ex;
        o[1] = e.ey;
        o[2] = e.ez;
        for (int j = 0; j < 3; ++j) o[3 + j] = ((e.neg >> j) & 1u) ? -1.0 : 1.0;
    }
}

template <class T>
__global__ __launch_bounds__(INFLOW_NT) void inflow_plane_kernel(GridDesc g, const InflowEntry* tab, int n, double sigma, double inv,
                                                                 double gust, double speed, const double* mean, const double* scale,
                                                                 T* vx, T* vy, T* vz, double* out)
{
    __shared__ InflowEntry list[INFLOW_CAP];
    __shared__ int wave_kept[INFLOW_NT / 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int y0 = 1 + blockIdx.x * INFLOW_PY, z0 = 1 + blockIdx.y * INFLOW_PZ;
    const int y = y0 + (tid % INFLOW_PY), z = z0 + (tid / INFLOW_PY);
    const double ylo = (double)y0, yhi = (double)min(y0 + INFLOW_PY - 1, g.H);
    const double zlo = (double)z0, zhi = (double)min(z0 + INFLOW_PZ - 1, g.D);
    const double yd = (double)y, zd = (double)z;
    double u[3] = { 0.0, 0.0, 0.0 };
    int count = 0;                                       // entries in the list (the same in every lane)
    for (int base = 0; base < n; base += INFLOW_NT) {
        const int k = base + tid;
        InflowEntry e = { 0.0, 0.0, 0.0, 0 };
        bool keep = false;
        if (k < n) {
            e = tab[k];
            keep = inflow_touches(e, sigma, ylo, yhi, zlo, zhi);
        }
        const unsigned long long kept = __ballot(keep);
        if (lane == 0) wave_kept[wave] = __popcll(kept);
        __syncthreads();
        int at = count, all = 0;
#pragma unroll
        for (int w = 0; w < INFLOW_NT / 64; ++w) {
            const int c = wave_kept[w];
            if (w < wave) at += c;
            all += c;
        }
        if (keep) list[at + __popcll(kept & ((1ull << lane) - 1ull))] = e;   // at most count + 256 <= INFLOW_CAP
        count += all;
        __syncthreads();
        if (count + INFLOW_NT > INFLOW_CAP || base + INFLOW_NT >= n) {
            for (int i = 0; i < count; ++i) {
                const InflowEntry q = list[i];
                inflow_accumulate(u, q, inflow_pair(q, yd, zd, inv));
            }
            count = 0;
            __syncthreads();
        }
    }
    if (y > g.H || z > g.D) return;
    const size_t plane = (size_t)g.H * (size_t)g.D, i = (size_t)(z - 1) * (size_t)g.H + (size_t)(y - 1);
    double o[3];
    inflow_compose(o, gust, mean ? mean[i] : speed, scale ? scale[i] : 1.0, u);
    if (out) {
        out[i] = o[0];
        out[plane + i] = o[1];
        out[2 * plane + i] = o[2];
    } else {
        const long c = cell(g, 1, y, z);
        vx[c] = (T)o[0];
        vy[c] = (T)o[1];
        vz[c] = (T)o[2];
    }
}

}  // namespace

void launch_inflow_table(hipStream_t st, const InflowParams& p, long t, InflowEntry* tab, double* eddies)
{
    if (p.n <= 0) return;
    hipLaunchKernelGGL(inflow_table_kernel, dim3((p.n + 255) / 256), dim3(256), 0, st, p, t, 1.0 / p.sigma, tab, eddies);
}

template <class T>
void launch_inflow_plane(hipStream_t st, const GridDesc& g, const InflowParams& p, const InflowEntry* tab, double gust, double speed,
                         const double* mean, const double* scale, T* vx, T* vy, T* vz, double* out)
{
    hipLaunchKernelGGL((inflow_plane_kernel<T>), dim3((g.H + INFLOW_PY - 1) / INFLOW_PY, (g.D + INFLOW_PZ - 1) / INFLOW_PZ),
                       dim3(INFLOW_NT), 0, st, g, tab, p.n, p.sigma, 1.0 / p.sigma, gust, speed, mean, scale, vx, vy, vz, out);
}
template void launch_inflow_plane<float>(hipStream_t, const GridDesc&, const InflowParams&, const InflowEntry*, double, double,
                                         const double*, const double*, float*, float*, float*, double*);
template void launch_inflow_plane<double>(hipStream_t, const GridDesc&, const InflowParams&, const InflowEntry*, double, double,
                                          const double*, const double*, double*, double*, double*, double*);

}  // namespace fs
