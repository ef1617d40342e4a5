// driver/forces.h -- pressure force on the obstacles (csrc/forces.h; beyond the reference)
#pragma once
#include "common.h"
#include "../forces.h"
#include "plane_records.h"

namespace {

template <class T>
struct Forces {
    explicit Forces(Engine<T>& e_) : eng(e_), S(e_.S), g(e_.g), sc(e_.sc), arr(e_.arr), slot(e_.slot), flags(e_.flags) {}

    // ring slot k, projection j: g.D plane records
    double* ring_slot(long k, int j) const { return (double*)ring.slot(k) + (size_t)j * plane_doubles(); }
    size_t plane_doubles() const { return (size_t)fs::FORCE_REC * (size_t)g.D; }

    // (re)allocate and clear the ring after fs_set_option("force_log")
    int ensure_ring()
    {
        if (ring.gen == S->force_log_gen) return FS_OK;
        HIP_TRY(ring.setup(S->stream, S->force_log_gen, S->force_log, 2 * plane_doubles() * sizeof(double)));
        return FS_OK;
    }

    int obstacle_force(double* out5, double* per_plane)
    {
        if (S->comm.active() && S->comm.null_transport) return fail(FS_EINVAL, "obstacle forces need the other slabs' planes; the FSNULL transport carries none");
        int rc = eng.ensure_flags();
        if (rc) return rc;
        const size_t n = plane_doubles();
        HIP_TRY(scratch.grow(n));
        {
            ScopedSpan sp(S, FAM_FORCES);
            fs::launch_forces<T>(S->stream, g, sc, arr[slot[FS_PRESSURE]], flags, scratch.get());
        }
        std::vector<double> mine(n), all;
        HIP_TRY(hipMemcpyAsync(mine.data(), scratch.get(), n * sizeof(double), hipMemcpyDeviceToHost, S->stream));
        HIP_TRY(hipStreamSynchronize(S->stream));
        if ((rc = gather_plane_records(eng, mine, all, "obstacle forces"))) return rc;
        combine_planes(S, g, [&](int r, int zl) { return &all[(size_t)r * n + (size_t)zl * fs::FORCE_REC]; }, out5);
        if (per_plane) memcpy(per_plane, all.data(), all.size() * sizeof(double));
        return FS_OK;
    }

    int log_fetch(double* rows, long max_rows, long* n_rows, long* n_dropped)
    {
        int rc = ensure_ring();
        if (rc) return rc;
        const long n = ring.at.retained();
        rc = ring.fetch_begin({"fs_force_log", "rows", "rows = NULL"}, n, max_rows, rows != nullptr, n_rows, n_dropped);
        if (rc != LogRing::GO_ON) return rc;
        if (S->comm.active() && S->comm.null_transport) return fail(FS_EINVAL, "obstacle forces need the other slabs' planes; the FSNULL transport carries none");
        const size_t per = 2 * plane_doubles();   // one step: both projections
        std::vector<double> mine((size_t)n * per), all;
        HIP_TRY(ring.fetch_copy(S->stream, mine.data()));
        if ((rc = gather_plane_records(eng, mine, all, "obstacle forces"))) return rc;
        const size_t blob = mine.size();
        for (long i = 0; i < n; ++i) {
            double s[2][fs::FORCE_REC];
            for (int j = 0; j < 2; ++j)
                combine_planes(S, g, [&](int r, int zl) {
                    return &all[(size_t)r * blob + (size_t)i * per + (size_t)j * (per / 2) + (size_t)zl * fs::FORCE_REC]; }, s[j]);
            double* o = rows + (size_t)i * FS_FORCE_LOG_COLS;
            o[0] = (double)ring.at.step_of(i);
            for (int k = 0; k < 3; ++k) {
                o[1 + k] = s[0][k];
                o[4 + k] = s[1][k];
            }
            o[7] = s[1][3];
            o[8] = s[1][4];
        }
        ring.fetch_end();
        return FS_OK;
    }

    // "force_log": projection `proj` (0, 1) of the running step; its plane records go straight into the step's ring slot (no host sync)
    void record(int proj)
    {
        if (!ring.on()) return;
        ScopedSpan sp(S, FAM_FORCES);
        fs::launch_forces<T>(S->stream, g, sc, arr[slot[FS_PRESSURE]], flags, ring_slot(ring.at.next(), proj));
    }
    void commit() { if (ring.on()) ring.at.commit(S->steps_total); }   // the step is complete

private:
    Engine<T>& eng;
    fs_sim* const S;
    const fs::GridDesc& g;
    const fs::SlabCtx& sc;
    T* (&arr)[NPOOL_MAX];
    int (&slot)[NSLOT];
    uint8_t*& flags;
    // the per-step log is a device ring of steps x 2 projections x g.D plane records
    LogRing ring;                       // for S->force_log_gen
    DevBuf<double> scratch;             // fs_obstacle_force: one record per local plane
};

}  // namespace
