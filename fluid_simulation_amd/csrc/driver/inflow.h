// driver/inflow.h -- turbulent inflow (csrc/inflow.h; beyond the reference)
#pragma once
#include "common.h"
#include "../inflow.h"

namespace {

template <class T>
struct Inflow {
    explicit Inflow(Engine<T>& e_) : S(e_.S), g(e_.g), arr(e_.arr), slot(e_.slot) {}

    // the parameters as they stand; FS_EINVAL where they do not make a finite amplitude or step t is out of range
    int params(const char* who, long t, fs::InflowParams* p) const
    {
        p->seed = S->inflow_seed;
        p->n = S->inflow_n;
        p->h = g.H;
        p->d = g.D;
        p->sigma = S->inflow_sigma;
        p->convect = S->inflow_convect_now();
        p->amp = fs::inflow_amplitude(p->n, p->h, p->d, p->sigma, S->inflow_rms);
        if (!std::isfinite(p->amp)) return fail(FS_EINVAL, "%s: the eddies' amplitude u_rms * sqrt(V / (N sigma^3)) is not finite", who);
        if (!std::isfinite(p->convect) || !(p->convect >= 0.0)) return fail(FS_EINVAL, "%s: the convection dt * width * speed is negative or not finite", who);
        if (!fs::inflow_step_ok(t, p->sigma, p->convect)) return fail(FS_EINVAL, "%s: step %ld is negative or beyond 2^53 eddy generations", who, t);
        return FS_OK;
    }
    // the maps on the device as fs_inflow_profile last left them, and room in the table for the eddies
    int ensure()
    {
        if (up_gen != S->inflow_gen) {
            const size_t cells = (size_t)g.H * (size_t)g.D;
            const std::vector<double>* host[2] = { &S->inflow_mean, &S->inflow_scale };
            DevBuf<double>* dev[2] = { &dmean, &dscale };
            HIP_TRY(hipStreamSynchronize(S->stream));    // a queued plane may still read the old maps
            for (int k = 0; k < 2; ++k) {
                if (host[k]->empty()) {
                    HIP_TRY(dev[k]->release());
                    continue;
                }
                HIP_TRY(dev[k]->grow(cells));
                HIP_TRY(hipMemcpy(dev[k]->get(), host[k]->data(), cells * sizeof(double), hipMemcpyHostToDevice));
            }
            up_gen = S->inflow_gen;
        }
        HIP_TRY(tab.grow((size_t)S->inflow_n, S->stream));   // a queued plane may still read the old table
        return FS_OK;
    }
    // the plane of step t: into the three velocities' x = 1 face, or (out not null) as 3 x d x h doubles into out
    void launch(const fs::InflowParams& p, long t, double* out)
    {
        const double gust = fs::inflow_gust(S->gust_t.data(), S->gust_f.data(), (int)S->gust_t.size(), t);
        ScopedSpan sp(S, FAM_INFLOW);
        fs::launch_inflow_table(S->stream, p, t, tab.get(), nullptr);
        fs::launch_inflow_plane<T>(S->stream, g, p, tab.get(), gust, (double)S->speed, dmean.get(), dscale.get(), arr[slot[FS_VX]],
                                   arr[slot[FS_VY]], arr[slot[FS_VZ]], out);
    }
    int plane(long t, double* out)
    {
        if (S->comm.active()) return fail(FS_EINVAL, "fs_inflow_plane: the inflow generator needs a single-GPU handle");
        fs::InflowParams p;
        int rc = params("fs_inflow_plane", t, &p);
        if (rc) return rc;
        if ((rc = ensure())) return rc;
        const size_t bytes = (size_t)3 * g.H * g.D * sizeof(double);
        HIP_TRY(plane_out.grow((size_t)3 * g.H * g.D));
        launch(p, t, plane_out.get());
        HIP_TRY(hipMemcpyAsync(out, plane_out.get(), bytes, hipMemcpyDeviceToHost, S->stream));
        HIP_TRY(hipStreamSynchronize(S->stream));
        return FS_OK;
    }
    int eddies(long t, double* out)
    {
        if (S->comm.active()) return fail(FS_EINVAL, "fs_inflow_eddies: the inflow generator needs a single-GPU handle");
        fs::InflowParams p;
        int rc = params("fs_inflow_eddies", t, &p);
        if (rc) return rc;
        if (p.n <= 0) return FS_OK;
        HIP_TRY(dbg.grow((size_t)fs::INFLOW_EDDIES_MAX * 6));
        {
            ScopedSpan sp(S, FAM_INFLOW);
            fs::launch_inflow_table(S->stream, p, t, nullptr, dbg.get());
        }
        HIP_TRY(hipMemcpyAsync(out, dbg.get(), (size_t)p.n * 6 * sizeof(double), hipMemcpyDeviceToHost, S->stream));
        HIP_TRY(hipStreamSynchronize(S->stream));
        return FS_OK;
    }

private:
    fs_sim* const S;
    const fs::GridDesc& g;
    T* (&arr)[NPOOL_MAX];
    int (&slot)[NSLOT];
    // the two maps as uploaded for S->inflow_gen (null = not given), the eddy table of the step being written (grown to
    // "inflow_eddies" entries), the result of fs_inflow_plane / fs_inflow_eddies; all stream-ordered reuse
    DevBuf<double> dmean, dscale, plane_out, dbg;
    DevBuf<fs::InflowEntry> tab;
    long up_gen = -1;
};

}  // namespace
