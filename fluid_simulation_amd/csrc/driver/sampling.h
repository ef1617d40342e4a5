// driver/sampling.h -- field sampling and point probes (csrc/sample.h; beyond the reference)
#pragma once
#include "common.h"
#include "../sample.h"
#include "plane_records.h"

namespace {

template <class T>
struct Sampling {
    explicit Sampling(Engine<T>& e_) : eng(e_), S(e_.S), g(e_.g), sc(e_.sc), arr(e_.arr), slot(e_.slot) {}

    int points(const double* xyz, long n)
    {
        if (S->comm.active()) return fail(FS_EINVAL, "fs_sample_points: fields are sampled on a single-GPU handle");
        hipError_t e = samp_pts.grow((size_t)n * 3, S->stream);   // a queued sample may still use what is freed here
        if (e == hipSuccess) e = samp_out.grow((size_t)n, S->stream);
        if (e != hipSuccess) {
            samp_pts.release();
            samp_out.release();
            samp_n = 0;
            return fail(FS_ENOMEM, "fs_sample_points: %ld points: %s", n, hipGetErrorString(e));
        }
        samp_n = n;
        if (n > 0) {
            HIP_TRY(hipMemcpyAsync(samp_pts.get(), xyz, (size_t)n * 3 * sizeof(double), hipMemcpyHostToDevice, S->stream));
            HIP_TRY(hipStreamSynchronize(S->stream));    // `xyz` may be freed by the caller
        }
        return FS_OK;
    }

    // The array behind a source of fs_sample and of the image entries: a field selector (-> field), FS_ISO_VORTEX |
    // FS_VORTEX_* (the field is computed first, -> field), or FS_SAMPLE_STAT | sel (the derived field goes into the staging
    // buffer in the accumulators' layout, which is the fields' pitched one, -> stat).  Both are LEAD-shifted.
    int resolve_source(const char* who, int source, const T*& field, const double*& stat)
    {
        int rc;
        field = nullptr;
        stat = nullptr;
        if (source >= 0 && source < FS_NFIELDS) {
            field = arr[slot[source]];
        } else if ((source & ~(FS_ISO_VORTEX - 1)) == FS_ISO_VORTEX && (source & (FS_ISO_VORTEX - 1)) < FS_VORTEX_NFIELDS) {
            if ((rc = eng.vortex.compute(who, source & (FS_ISO_VORTEX - 1)))) return rc;
            field = eng.vortex.array();
        } else if ((source & ~(FS_SAMPLE_STAT - 1)) == FS_SAMPLE_STAT) {
            if ((rc = eng.flow_stats.stage(who, source & (FS_SAMPLE_STAT - 1), stat))) return rc;
        } else if (source == FS_SOURCE_HEAT) {
            if (!eng.heat.on()) return fail(FS_EINVAL, "%s: FS_SOURCE_HEAT while heat is off (fs_heat_params, mode 1 or 2)", who);
            field = arr[slot[F_THETA]];
        } else {
            return fail(FS_EINVAL, "%s: unknown source %d (a field selector, FS_SOURCE_HEAT, FS_ISO_VORTEX | FS_VORTEX_* or FS_SAMPLE_STAT | FS_STAT_*)", who, source);
        }
        return FS_OK;
    }

    // `source` in `mode` at the n device points `pts` into the device array `vals`, copied to `out`: fs_sample on the kept
    // points, fs_tracer_sample on the pool's positions.  The caller has checked n against its point count.
    int sample_at(const char* who, int source, int mode, const double* pts, double* vals, double* out, long n)
    {
        if (mode < 0 || mode >= fs::SAMPLE_NMODES) return fail(FS_EINVAL, "%s: unknown mode %d (FS_SAMPLE_NEAREST | LINEAR | FLUID)", who, mode);
        const T* field = nullptr;
        const double* stat = nullptr;
        int rc = resolve_source(who, source, field, stat);
        if (rc) return rc;
        if (n == 0) return FS_OK;
        if (!out) return fail(FS_EINVAL, "%s: null output", who);
        const T* obs = arr[slot[FS_OBS]];
        {
            ScopedSpan sp(S, FAM_MISC);
            if (stat) fs::launch_sample<double, T>(S->stream, g, mode, n, pts, stat, obs, vals);
            else fs::launch_sample<T, T>(S->stream, g, mode, n, pts, field, obs, vals);
        }
        HIP_TRY(hipMemcpyAsync(out, vals, (size_t)n * sizeof(double), hipMemcpyDeviceToHost, S->stream));
        HIP_TRY(hipStreamSynchronize(S->stream));
        return FS_OK;
    }

    int sample(int source, int mode, double* out, long n)
    {
        if (S->comm.active()) return fail(FS_EINVAL, "fs_sample: fields are sampled on a single-GPU handle");
        if (n != samp_n) return fail(FS_EINVAL, "fs_sample: %ld points are kept (fs_sample_points), the call has room for %ld", samp_n, n);
        return sample_at("fs_sample", source, mode, samp_pts.get(), samp_out.get(), out, n);
    }

    double* probe_slot(long k) const { return (double*)probe_ring.slot(k); }

    // set up the probe list and (re)allocate and clear the ring after fs_set_probes / fs_set_option("probe_log")
    int ensure_probe_ring()
    {
        if (probe_ring.gen == S->probe_gen) return FS_OK;
        if (probe_idx.get()) {
            HIP_TRY(hipStreamSynchronize(S->stream));    // a queued record may still use what is freed here
            HIP_TRY(probe_idx.release());
        }
        probe_n = 0;
        HIP_TRY(probe_ring.setup(S->stream, S->probe_gen));   // off
        const int n = (int)(S->probes.size() / 3);
        if (n == 0 || S->probe_log <= 0) return FS_OK;
        // the owner of a probe is the rank that owns its global plane (z = 0: the first, z = D + 1: the last)
        std::vector<long> idx((size_t)n);
        for (int k = 0; k < n; ++k) {
            const int x = S->probes[3 * (size_t)k], y = S->probes[3 * (size_t)k + 1], z = S->probes[3 * (size_t)k + 2];
            const int zl = z - sc.zoff;
            const bool mine = (zl >= 1 && zl <= g.D) || (z == 0 && sc.lo_wall) || (z == sc.Dglobal + 1 && sc.hi_wall);
            idx[(size_t)k] = mine ? (long)x + (long)y * g.sy + (long)zl * g.sz : -1;
        }
        HIP_TRY(probe_idx.alloc(idx.size()));
        HIP_TRY(hipMemcpyAsync(probe_idx.get(), idx.data(), idx.size() * sizeof(long), hipMemcpyHostToDevice, S->stream));
        HIP_TRY(hipStreamSynchronize(S->stream));        // `idx` goes out of scope
        probe_n = n;
        HIP_TRY(probe_ring.setup(S->stream, S->probe_gen, S->probe_log, (size_t)n * fs::PROBE_VALUES * sizeof(double)));
        return FS_OK;
    }

    // one record of the state as it is now into the next ring slot
    void probe_record()
    {
        {
            ScopedSpan sp(S, FAM_PROBES);
            fs::launch_probe_record<T>(S->stream, probe_n, probe_idx.get(), arr[slot[FS_DENS]], arr[slot[FS_VX]], arr[slot[FS_VY]],
                                       arr[slot[FS_VZ]], arr[slot[FS_PRESSURE]], probe_slot(probe_ring.at.next()));
        }
        probe_ring.at.commit(S->steps_total);
    }

    int probe_sample()
    {
        int rc = ensure_probe_ring();
        if (rc) return rc;
        if (!probe_ring.on()) return fail(FS_EINVAL, "fs_probe_sample: no probes are set (fs_set_probes), or option \"probe_log\" is 0");
        probe_record();
        return FS_OK;
    }

    int probe_log_fetch(double* rows, long max_rows, long* n_rows, long* n_dropped)
    {
        int rc = ensure_probe_ring();
        if (rc) return rc;
        const long n = probe_ring.at.retained();
        rc = probe_ring.fetch_begin({"fs_probe_log", "rows", "rows = NULL"}, n, max_rows, rows != nullptr, n_rows, n_dropped);
        if (rc != LogRing::GO_ON) return rc;
        if (S->comm.active() && S->comm.null_transport) return fail(FS_EINVAL, "probe records need the other slabs' planes; the FSNULL transport carries none");
        const size_t per = (size_t)probe_n * fs::PROBE_VALUES;   // one record
        std::vector<double> mine((size_t)n * per), all;
        HIP_TRY(probe_ring.fetch_copy(S->stream, mine.data()));
        if ((rc = gather_plane_records(eng, mine, all, "probe records"))) return rc;
        const size_t blob = mine.size();
        const int nr = S->comm.active() ? S->comm.nranks : 1, ld = S->D / nr;
        std::vector<size_t> owner_off((size_t)probe_n);  // only the owner's value is used
        for (int k = 0; k < probe_n; ++k) {
            const int z = S->probes[3 * (size_t)k + 2];
            const int r = z <= 0 ? 0 : z > S->D ? nr - 1 : (z - 1) / ld;
            owner_off[(size_t)k] = (size_t)r * blob + (size_t)k * fs::PROBE_VALUES;
        }
        const size_t cols = 1 + per;
        for (long i = 0; i < n; ++i) {
            double* o = rows + (size_t)i * cols;
            o[0] = (double)probe_ring.at.step_of(i);
            for (int k = 0; k < probe_n; ++k)
                for (int j = 0; j < fs::PROBE_VALUES; ++j)
                    o[1 + (size_t)k * fs::PROBE_VALUES + j] = all[owner_off[(size_t)k] + (size_t)i * per + j];
        }
        probe_ring.fetch_end();
        return FS_OK;
    }

    // fs_step, "probe_log": the state the step left is a record of the probes
    void probe_step() { if (probe_ring.on()) probe_record(); }

private:
    Engine<T>& eng;
    fs_sim* const S;
    const fs::GridDesc& g;
    const fs::SlabCtx& sc;
    T* (&arr)[NPOOL_MAX];
    int (&slot)[NSLOT];
    // the point set of fs_sample_points and the values of the last fs_sample, on the device
    DevBuf<double> samp_pts, samp_out;  // grown on demand
    long samp_n = 0;                    // points kept
    // point probes: the per-step log is a device ring of records x probe_n probes x {q, u, v, w, p}
    DevBuf<long> probe_idx;             // each probe's cell index in this slab's arrays, -1 = a plane another rank owns
    LogRing probe_ring;                 // for S->probe_gen, as is the list; on only with probe_n > 0
    int probe_n = 0;
};

}  // namespace
