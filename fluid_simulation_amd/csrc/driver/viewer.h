// driver/viewer.h -- the viewer's streamlines and meshes (GUI/utils.py of the reference)
#pragma once
#include "common.h"
#include "../streamlines.h"
#include "../surface.h"

namespace {

template <class T>
struct Viewer {
    explicit Viewer(Engine<T>& e_) : eng(e_), S(e_.S), g(e_.g), arr(e_.arr), slot(e_.slot) {}

    // ---- the viewer's streamlines (GUI/utils.py:118-213) -------------------------------------
    // The device integrates every seed in both directions; what is left for the host is the
    // reference's bookkeeping per seed: joining the two parts and the three filters.
    int streamlines(int density, double proximity, int max_length, double step_size, double threshold)
    {
        S->sl_offsets.assign(1, 0);
        S->sl_points.clear();
        S->sl_norm.clear();
        if (S->comm.active()) return fail(FS_EINVAL, "streamlines are computed on a single-GPU handle");
        if (density < 0 || max_length < 0) return fail(FS_EINVAL, "density and max_length must be >= 0");
        if (density > 4096 || max_length > 1000000) return fail(FS_EINVAL, "density <= 4096 and max_length <= 1e6, please");
        if (!(step_size == step_size) || !(proximity == proximity) || !(threshold == threshold))
            return fail(FS_EINVAL, "streamline parameters must not be NaN");
        const T* obs = arr[slot[FS_OBS]];
        fs::StreamParams p;
        p.nx = density; p.ny = density / 2; p.nz = density / 2;          // utils.py:136-138
        p.half = max_length / 2;
        p.step_size = step_size;
        const int dims[3] = { g.W + 2, g.H + 2, g.D + 2 };               // config.width/height/depth
        for (int k = 0; k < 3; ++k) {
            p.clip_hi[k] = (double)dims[k] - 1.001;
            p.bound_hi[k] = (double)(dims[k] - 1);
        }
        int box[6];
        {
            DevBuf<int> d_box;
            HIP_TRY(d_box.alloc(6));
            fs::launch_obs_bbox<T>(S->stream, g, obs, d_box.get());
            HIP_TRY(hipMemcpyAsync(box, d_box.get(), sizeof box, hipMemcpyDeviceToHost, S->stream));
            HIP_TRY(hipStreamSynchronize(S->stream));
        }
        if (box[0] > box[3]) return FS_OK;                               // no obstacles: no streamlines (:134-135)
        for (int k = 0; k < 3; ++k) {
            p.lo[k] = (double)box[k] - proximity / 10;
            p.hi[k] = (double)box[3 + k] + proximity / 10;
        }
        const long nseed = (long)p.nx * p.ny * p.nz;
        if (nseed == 0) return FS_OK;
        // np.linspace(1, dim - 2, n): arange(n) * step + start, last element = stop
        std::vector<double> seeds((size_t)p.nx + p.ny + p.nz);
        {
            const int cnt[3] = { p.nx, p.ny, p.nz };
            size_t o = 0;
            for (int k = 0; k < 3; ++k) {
                const double start = 1.0, stop = (double)(dims[k] - 2);
                const int n = cnt[k];
                const double step = n > 1 ? (stop - start) / (double)(n - 1) : 0.0;
                for (int i = 0; i < n; ++i) seeds[o + i] = (double)i * step + start;
                if (n > 1) seeds[o + n - 1] = stop;
                o += n;
            }
        }
        // utils.py:147-150: seeds outside the widened bounding box are skipped before anything else
        std::vector<int> cand;
        for (int iz = 0; iz < p.nz; ++iz)
            for (int iy = 0; iy < p.ny; ++iy)
                for (int ix = 0; ix < p.nx; ++ix) {
                    const double sx = seeds[ix], sy = seeds[p.nx + iy], sz = seeds[(size_t)p.nx + p.ny + iz];
                    if (sx < p.lo[0] || sx > p.hi[0] || sy < p.lo[1] || sy > p.hi[1] || sz < p.lo[2] || sz > p.hi[2]) continue;
                    cand.push_back((iz * p.ny + iy) * p.nx + ix);
                }
        const long ncand = (long)cand.size();
        if (ncand == 0) return FS_OK;
        const size_t per = (size_t)(p.half + 1) * 3, npts = (size_t)ncand * 2 * per;
        if (npts > ((size_t)1 << 29))                    // 2 x 4 GiB of points and velocities: split the call instead
            return fail(FS_ENOMEM, "%ld seeds x %d steps is more than one call should integrate; lower density or max_length", ncand, max_length);
        int rc = FS_OK, any_nan = 0;
        std::vector<double> pts, vel;
        std::vector<int> count((size_t)ncand * 2);
        double mx[3][3];
        do {
            DevBuf<double> seeds_buf, pts_buf, vel_buf;  // the device buffers go where this block ends
            DevBuf<int> count_buf, cand_buf, nan_buf;
            if (seeds_buf.alloc(seeds.size()) != hipSuccess || pts_buf.alloc(npts) != hipSuccess || vel_buf.alloc(npts) != hipSuccess ||
                count_buf.alloc(count.size()) != hipSuccess || cand_buf.alloc(cand.size()) != hipSuccess || nan_buf.alloc(1) != hipSuccess) {
                rc = fail(FS_ENOMEM, "streamline buffers");
                break;
            }
            double *const d_seeds = seeds_buf.get(), *const d_pts = pts_buf.get(), *const d_vel = vel_buf.get();
            int *const d_count = count_buf.get(), *const d_cand = cand_buf.get(), *const d_nan = nan_buf.get();
            pts.resize(npts);
            vel.resize(npts);
            if (hipMemcpyAsync(d_seeds, seeds.data(), seeds.size() * 8, hipMemcpyHostToDevice, S->stream) != hipSuccess ||
                hipMemcpyAsync(d_cand, cand.data(), cand.size() * 4, hipMemcpyHostToDevice, S->stream) != hipSuccess) { rc = fail(FS_EHIP, "seed upload"); break; }
            fs::launch_streamlines<T>(S->stream, g, arr[slot[FS_VX]], arr[slot[FS_VY]], arr[slot[FS_VZ]], obs, p, d_seeds, d_cand,
                                      (int)ncand, d_count, d_pts, d_vel);
            if (hipMemsetAsync(d_nan, 0, 4, S->stream) != hipSuccess) { rc = fail(FS_EHIP, "streamline flag"); break; }
            fs::launch_any_nan<T>(S->stream, g, arr[slot[FS_VX]], arr[slot[FS_VY]], arr[slot[FS_VZ]], d_nan);
            if (hipMemcpyAsync(count.data(), d_count, count.size() * 4, hipMemcpyDeviceToHost, S->stream) != hipSuccess ||
                hipMemcpyAsync(&any_nan, d_nan, 4, hipMemcpyDeviceToHost, S->stream) != hipSuccess ||
                hipMemcpyAsync(pts.data(), d_pts, npts * 8, hipMemcpyDeviceToHost, S->stream) != hipSuccess ||
                hipMemcpyAsync(vel.data(), d_vel, npts * 8, hipMemcpyDeviceToHost, S->stream) != hipSuccess ||
                hipStreamSynchronize(S->stream) != hipSuccess) { rc = fail(FS_EHIP, "streamline kernel or copy failed"); break; }
            for (int k = 0; k < 3; ++k)
                if ((rc = eng.stats_of(arr[slot[FS_VX + k]], mx[k]))) break;
        } while (0);
        if (rc) return rc;
        // np.max([vx, vy, vz]) + 1e-6 in the arrays' own precision (float32 for the reference's dumps).  np.max is NaN
        // if any cell is; the maximum of the field statistics skips NaN (the reference's own loop), hence the flag.
        const T vmax = (T)std::fmax(std::fmax(mx[0][2], mx[1][2]), mx[2][2]);
        const double denom = any_nan ? std::numeric_limits<double>::quiet_NaN() : (double)(T)(vmax + (T)1e-6);
        auto norm3 = [](double a, double b, double c) { return std::sqrt((a * a + b * b) + c * c); };
        std::vector<double> line, lvel;
        for (long sd = 0; sd < ncand; ++sd) {
            const int nb = count[2 * sd], nf = count[2 * sd + 1];
            if (nb == 0) continue;                                       // seed inside an obstacle
            const double* B = &pts[(size_t)(2 * sd) * per], *F = &pts[(size_t)(2 * sd + 1) * per];
            const double* VB = &vel[(size_t)(2 * sd) * per], *VF = &vel[(size_t)(2 * sd + 1) * per];
            line.clear();
            lvel.clear();
            for (int i = nb - 1; i >= 1; --i)                            // backward[::-1][:-1]  (:167-168)
                for (int c = 0; c < 3; ++c) { line.push_back(B[3 * i + c]); lvel.push_back(VB[3 * i + c]); }
            for (int i = 0; i < nf; ++i)
                for (int c = 0; c < 3; ++c) { line.push_back(F[3 * i + c]); lvel.push_back(VF[3 * i + c]); }
            const int n = (int)(line.size() / 3);
            if (n <= 5) continue;                                        // :171-172
            double max_change = 0.0;                                     // :175-181
            for (int i = 1; i < n; ++i) {
                const double ch = norm3(lvel[3 * i] - lvel[3 * i - 3], lvel[3 * i + 1] - lvel[3 * i - 2], lvel[3 * i + 2] - lvel[3 * i - 1]);
                if (ch > max_change) max_change = ch;
            }
            if (max_change < threshold) continue;
            bool near = false;                                           // :184-195, every third point
            for (int i = 0; i < n && !near; i += 3)
                near = p.lo[0] <= line[3 * i] && line[3 * i] <= p.hi[0] && p.lo[1] <= line[3 * i + 1] && line[3 * i + 1] <= p.hi[1] &&
                       p.lo[2] <= line[3 * i + 2] && line[3 * i + 2] <= p.hi[2];
            if (!near) continue;
            // :198-205 with Python's max and min: max keeps its first element unless a later one compares greater,
            // min(r, 1.0) is r unless 1.0 < r -- a NaN ratio stays NaN
            double max_speed = norm3(lvel[0], lvel[1], lvel[2]);
            for (int i = 1; i < n; ++i) {
                const double sp = norm3(lvel[3 * i], lvel[3 * i + 1], lvel[3 * i + 2]);
                if (sp > max_speed) max_speed = sp;
            }
            const double ratio = max_speed / denom;
            S->sl_norm.push_back(1.0 < ratio ? 1.0 : ratio);
            S->sl_points.insert(S->sl_points.end(), line.begin(), line.end());
            S->sl_offsets.push_back((long)(S->sl_points.size() / 3));
        }
        return FS_OK;
    }

    // ---- the viewer's obstacle mesh (GUI/utils.py:10-38) ------------------------------------------
    // the mesh of `field` > `level` into one of the handle's two result slots
    int surface_into(const T* field, T level, std::vector<float>& verts, std::vector<int>& tris, bool& valid)
    {
        verts.clear();
        tris.clear();
        valid = false;
        fs::SurfaceResult r;
        const char* msg = "";
        int rc = fs::extract_surface<T>(S->stream, g, field, level, &r, &msg);
        if (rc) return fail(rc, "%s", msg);
        verts.resize((size_t)r.nverts * 3);
        tris.resize((size_t)r.ntris * 3);
        hipError_t e = hipSuccess;
        if (r.nverts > 0) {
            e = hipMemcpyAsync(verts.data(), r.d_verts, verts.size() * sizeof(float), hipMemcpyDeviceToHost, S->stream);
            if (e == hipSuccess) e = hipMemcpyAsync(tris.data(), r.d_tris, tris.size() * sizeof(int), hipMemcpyDeviceToHost, S->stream);
            if (e == hipSuccess) e = hipStreamSynchronize(S->stream);
        }
        fs::surface_free(&r);
        if (e != hipSuccess) return fail(FS_EHIP, "copying the surface: %s", hipGetErrorString(e));
        valid = true;
        return FS_OK;
    }

    int obstacle_surface()
    {
        S->surf_valid = false;
        if (S->comm.active()) return fail(FS_EINVAL, "the obstacle surface is extracted on a single-GPU handle");
        return surface_into(arr[slot[FS_OBS]], (T)0.5, S->surf_verts, S->surf_tris, S->surf_valid);
    }

private:
    Engine<T>& eng;
    fs_sim* const S;
    const fs::GridDesc& g;
    T* (&arr)[NPOOL_MAX];
    int (&slot)[NSLOT];
};

}  // namespace
