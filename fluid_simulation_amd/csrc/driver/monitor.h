// driver/monitor.h -- flow monitor (csrc/monitor.h; beyond the reference)
#pragma once
#include "common.h"
#include "../monitor.h"
#include "../monitor_plan.h"

namespace {

template <class T>
struct Monitor {
    explicit Monitor(Engine<T>& e_) : eng(e_), S(e_.S), g(e_.g), arr(e_.arr), slot(e_.slot), flags(e_.flags) {}

    int ensure_ws()
    {
        HIP_TRY(ws.grow(fs::monitor_workspace_doubles(g)));
        return FS_OK;
    }

    // (re)allocate and clear the ring after fs_set_option("monitor_log") / ("monitor_stations")
    int ensure_ring()
    {
        if (ring.gen == S->monitor_gen) return FS_OK;
        HIP_TRY(ring.setup(S->stream, S->monitor_gen));   // off, whatever fails below
        if (S->monitor_log <= 0) return FS_OK;
        if (S->comm.active()) return fail(FS_EINVAL, "monitor_log: the flow monitor needs a single-GPU handle");
        int rc = ensure_ws();
        if (rc) return rc;
        HIP_TRY(ring.setup(S->stream, S->monitor_gen, S->monitor_log, (size_t)fs::MON_RESULT * sizeof(double)));
        return FS_OK;
    }

    // one record of the state as it is now into `result` (a ring slot or the workspace's result slot)
    void launch(double* result)
    {
        ScopedSpan sp(S, FAM_MONITOR);
        fs::launch_monitor<T>(S->stream, g, arr[slot[FS_DENS]], arr[slot[FS_VX]], arr[slot[FS_VY]], arr[slot[FS_VZ]],
                              arr[slot[FS_PRESSURE]], flags, S->monitor_stations, ws.get(), result);
    }
    void record()
    {
        launch((double*)ring.slot(ring.at.next()));
        ring.at.commit(S->steps_total);
    }

    int sample()
    {
        if (S->comm.active()) return fail(FS_EINVAL, "fs_monitor_sample: the flow monitor needs a single-GPU handle");
        int rc = eng.ensure_flags();
        if (rc) return rc;
        if ((rc = ensure_ring())) return rc;
        if (!ring.on()) return fail(FS_EINVAL, "fs_monitor_sample: option \"monitor_log\" is 0");
        record();
        return FS_OK;
    }

    int query(double* out16, double* per_plane, double* x_profile)
    {
        if (S->comm.active()) return fail(FS_EINVAL, "fs_flow_monitor: the flow monitor needs a single-GPU handle");
        int rc = eng.ensure_flags();
        if (rc) return rc;
        if ((rc = ensure_ws())) return rc;
        const fs::MonitorPlan pl = fs::monitor_plan(g.W, g.H, g.D);
        launch(ws.get() + pl.result_off);
        // planes, profile and result lie one behind the other (monitor_plan.h)
        std::vector<double> host((size_t)(pl.doubles - pl.planes_off));
        HIP_TRY(hipMemcpyAsync(host.data(), ws.get() + pl.planes_off, host.size() * sizeof(double), hipMemcpyDeviceToHost, S->stream));
        HIP_TRY(hipStreamSynchronize(S->stream));
        if (out16) memcpy(out16, host.data() + (pl.result_off - pl.planes_off), fs::MON_PLANE * sizeof(double));
        if (per_plane) memcpy(per_plane, host.data(), (size_t)g.D * fs::MON_PLANE * sizeof(double));
        if (x_profile) memcpy(x_profile, host.data() + (pl.profile_off - pl.planes_off), (size_t)g.W * fs::MON_PROFILE * sizeof(double));
        return FS_OK;
    }

    int log_fetch(double* rows, long max_rows, long* n_rows, long* n_dropped)
    {
        if (S->comm.active()) return fail(FS_EINVAL, "fs_monitor_log: the flow monitor needs a single-GPU handle");
        int rc = ensure_ring();
        if (rc) return rc;
        const long n = ring.at.retained();
        rc = ring.fetch_begin({"fs_monitor_log", "rows", "rows = NULL"}, n, max_rows, rows != nullptr, n_rows, n_dropped);
        if (rc != LogRing::GO_ON) return rc;
        std::vector<double> mine((size_t)n * fs::MON_RESULT);
        HIP_TRY(ring.fetch_copy(S->stream, mine.data()));
        for (long i = 0; i < n; ++i) {
            double* o = rows + (size_t)i * FS_MONITOR_LOG_COLS;
            o[0] = (double)ring.at.step_of(i);
            memcpy(o + 1, &mine[(size_t)i * fs::MON_RESULT], fs::MON_RESULT * sizeof(double));
        }
        ring.fetch_end();
        return FS_OK;
    }

    bool on() const { return ring.on(); }

private:
    Engine<T>& eng;
    fs_sim* const S;
    const fs::GridDesc& g;
    T* (&arr)[NPOOL_MAX];
    int (&slot)[NSLOT];
    uint8_t*& flags;
    // the workspace of its three launches (allocated at the first record, stream-ordered reuse) and the per-step log, a device
    // ring of records of MON_RESULT doubles (the whole record, then the stations' profile rows)
    DevBuf<double> ws;
    LogRing ring;                       // for S->monitor_gen
};

}  // namespace
