// driver/zones.h -- momentum zones (csrc/zones.h; beyond the reference)
#pragma once
#include "common.h"
#include "../zones.h"

namespace {

template <class T>
struct Zones {
    explicit Zones(Engine<T>& e_) : eng(e_), S(e_.S), g(e_.g), arr(e_.arr), slot(e_.slot), flags(e_.flags) {}

    // fs_zones with rows the entry has checked: the workspace and the log first, then the values.  Off frees everything.
    int config(const double* par, int n, int mode, int log)
    {
        if (n == 0 || mode == 0) {
            HIP_TRY(ring.setup(S->stream, 0));           // synchronises where a queued record may still write to it
            if (ws.get()) HIP_TRY(hipStreamSynchronize(S->stream));
            HIP_TRY(ws.release());
            S->zone_n = S->zone_mode = S->zone_log = 0;
            return FS_OK;
        }
        if (S->comm.active()) return fail(FS_EINVAL, "fs_zones: zones need a single GPU handle (the pass is not exchanged between slabs)");
        HIP_TRY(ws.grow(fs::zone_workspace_doubles(g, n), S->stream));
        if (log != ring.at.cap || n != S->zone_n) HIP_TRY(ring.setup(S->stream, 0, log, (size_t)n * fs::ZONE_COLS * sizeof(double)));
        memcpy(S->zones, par, (size_t)n * fs::ZONE_PARAMS * sizeof(double));
        S->zone_n = n;
        S->zone_mode = mode;
        S->zone_log = log;
        return FS_OK;
    }
    // the zones as the kernels take them; dt is read now, so a changed dt holds from the next pass on
    fs::ZoneTable table() const
    {
        fs::ZoneTable zt;
        memset(&zt, 0, sizeof zt);
        zt.dt = (double)S->dt;
        zt.n = S->zone_n;
        for (int k = 0; k < zt.n; ++k) zt.z[k] = fs::zone_make(S->zones + (size_t)k * fs::ZONE_PARAMS, zt.dt);
        return zt;
    }
    int need(const char* who)
    {
        if (S->comm.active()) return fail(FS_EINVAL, "%s: zones need a single GPU handle (the pass is not exchanged between slabs)", who);
        if (S->zone_mode == 0) return fail(FS_EINVAL, "%s: zones are off (fs_zones, mode 1 or 2)", who);
        return FS_OK;
    }
    // the pass: the three velocity components, in place.  One launch.
    int apply_pass(const char* who)
    {
        int rc = need(who);
        if (rc) return rc;
        if ((rc = eng.ensure_flags())) return rc;
        if (!eng.in_step) eng.vzmax_prev = -1.0;
        for (int f : { FS_VX, FS_VY, FS_VZ })
            if ((rc = eng.unalias(f))) return rc;
        {
            ScopedSpan sp(S, FAM_ZONES);
            fs::launch_zone_apply<T>(S->stream, g, table(), arr[slot[FS_VX]], arr[slot[FS_VY]], arr[slot[FS_VZ]], flags);
        }
        ++S->n_zone_apply;
        return FS_OK;
    }
    int apply() { return apply_pass("fs_zone_apply"); }

    // the budget of the state as it is now into `result` (a ring slot or the workspace's result slots)
    void budget_launch(double* result)
    {
        ScopedSpan sp(S, FAM_ZONES, 3);
        fs::launch_zone_budget<T>(S->stream, g, table(), arr[slot[FS_VX]], arr[slot[FS_VY]], arr[slot[FS_VZ]], flags, ws.get(), result);
    }
    // fs_step, the zone log: the budget of the state the pass is about to change (three launches, no host synchronisation);
    // the record carries the number of the step that is running
    void record()
    {
        if (!ring.on()) return;
        budget_launch((double*)ring.slot(ring.at.next()));
        ring.at.commit(S->steps_total + 1);
    }
    int budget(double* out, double* per_plane)
    {
        int rc = need("fs_zone_budget");
        if (rc) return rc;
        if ((rc = eng.ensure_flags())) return rc;
        const size_t cols = (size_t)S->zone_n * fs::ZONE_COLS;
        const size_t total = fs::zone_workspace_doubles(g, S->zone_n), planes = fs::zone_planes_offset(g, S->zone_n);
        budget_launch(ws.get() + (total - cols));
        std::vector<double> host(total - planes);        // the plane records, then the result
        HIP_TRY(hipMemcpyAsync(host.data(), ws.get() + planes, host.size() * sizeof(double), hipMemcpyDeviceToHost, S->stream));
        HIP_TRY(hipStreamSynchronize(S->stream));
        memcpy(out, host.data() + (size_t)g.D * cols, cols * sizeof(double));
        if (per_plane) memcpy(per_plane, host.data(), (size_t)g.D * cols * sizeof(double));
        return FS_OK;
    }
    int log_fetch(double* rows, long max_rows, long* n_rows, long* n_dropped)
    {
        if (S->comm.active()) return fail(FS_EINVAL, "fs_zone_log: zones need a single GPU handle");
        const long n = ring.at.retained();
        int rc = ring.fetch_begin({"fs_zone_log", "rows", "rows = NULL"}, n, max_rows, rows != nullptr, n_rows, n_dropped);
        if (rc != LogRing::GO_ON) return rc;
        const size_t cols = (size_t)S->zone_n * fs::ZONE_COLS;
        std::vector<double> mine((size_t)n * cols);
        HIP_TRY(ring.fetch_copy(S->stream, mine.data()));
        for (long i = 0; i < n; ++i) {
            double* o = rows + (size_t)i * (1 + cols);
            o[0] = (double)ring.at.step_of(i);
            memcpy(o + 1, &mine[(size_t)i * cols], cols * sizeof(double));
        }
        ring.fetch_end();
        return FS_OK;
    }
    int mask(uint8_t* dst, size_t n)
    {
        int rc = need("fs_zone_mask");
        if (rc) return rc;
        if ((long)n != eng.dense_cells()) return fail(FS_EINVAL, "fs_zone_mask: expected %ld elements, got %zu", eng.dense_cells(), n);
        if ((rc = eng.ensure_flags())) return rc;
        if ((rc = eng.need_dense(n))) return rc;
        {
            ScopedSpan sp(S, FAM_ZONES);
            fs::launch_zone_mask(S->stream, g, table(), flags, (uint8_t*)eng.dense.get());
        }
        HIP_TRY(hipMemcpyAsync(dst, eng.dense.get(), n, hipMemcpyDeviceToHost, S->stream));
        HIP_TRY(hipStreamSynchronize(S->stream));
        return FS_OK;
    }

private:
    Engine<T>& eng;
    fs_sim* const S;
    const fs::GridDesc& g;
    T* (&arr)[NPOOL_MAX];
    int (&slot)[NSLOT];
    uint8_t*& flags;
    DevBuf<double> ws;                  // workspace of the budget's three launches, sized for the zones in force
    LogRing ring;                       // the per-step zone log: records of zone_n * ZONE_COLS doubles
};

}  // namespace
