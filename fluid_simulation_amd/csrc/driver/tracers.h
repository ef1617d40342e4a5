// driver/tracers.h -- tracer particles (csrc/tracers.h; beyond the reference)
#pragma once
#include "common.h"
#include "../tracers.h"

namespace {

template <class T>
struct Tracers {
    explicit Tracers(Engine<T>& e_) : eng(e_), S(e_.S), g(e_.g), arr(e_.arr), slot(e_.slot) {}

    // a ring slot is one frame's bytes, but the ring is laid out in two sections: every position frame, then every status frame
    double* tracer_frame_xyz(long f) const { return (double*)tr_ring.base.get() + (size_t)f * 3 * (size_t)tr_cap; }
    int* tracer_frame_status(long f) const { return (int*)tracer_frame_xyz(tr_ring.at.cap) + (size_t)f * (size_t)tr_cap; }

    int config() { return ensure(); }

    // (re)allocate and clear the pool after fs_set_option("tracers") and the ring after that or ("tracer_log"); upload the
    // emitters after fs_tracer_emitters, so that an advance in mid-step allocates and copies nothing
    int ensure()
    {
        if (tr_gen != S->tracer_gen) {
            if (tr_xyz.get()) {
                HIP_TRY(hipStreamSynchronize(S->stream));    // a queued advance may still use what is freed here
                HIP_TRY(tr_xyz.release());
                HIP_TRY(tr_meta.release());
                HIP_TRY(tr_emit.release());
                HIP_TRY(tr_out.release());
            }
            tr_cap = 0;
            tr_emit_gen = -1;
            tr_ring.gen = -1;                            // the frames are C slots wide: the ring goes with the pool
            S->tracer_seeded = 0;
            tr_gen = S->tracer_gen;
            if (S->tracers > 0) {
                if (S->comm.active()) return fail(FS_EINVAL, "tracers need a single-GPU handle");
                const size_t C = (size_t)S->tracers;
                hipError_t e = tr_xyz.alloc(C * 3);
                if (e == hipSuccess) e = tr_meta.alloc(C * fs::TRACER_META);
                if (e == hipSuccess) e = tr_emit.alloc((size_t)FS_TRACER_EMITTERS_MAX * 3);
                if (e != hipSuccess) {                   // the option goes back to off: capacity and entries agree, a later set tries again
                    tr_xyz.release();
                    tr_meta.release();
                    S->tracers = 0;
                    return fail(FS_ENOMEM, "tracers: %zu slots: %s (the option is 0 again)", C, hipGetErrorString(e));
                }
                HIP_TRY(hipMemsetAsync(tr_xyz.get(), 0, C * 3 * sizeof(double), S->stream));
                HIP_TRY(hipMemsetAsync(tr_meta.get(), 0, C * fs::TRACER_META * sizeof(int), S->stream));   // every slot FREE
                tr_cap = S->tracers;
            }
        }
        if (tr_ring.gen != S->tracer_log_gen || (tr_cap == 0 && tr_ring.base.get())) {
            const hipError_t e = tr_ring.setup(S->stream, S->tracer_log_gen, tr_cap > 0 ? S->tracer_log : 0, (size_t)tr_cap * fs::TRACER_FRAME_BYTES);
            if (e != hipSuccess && !tr_ring.base.get()) {      // no memory.  Likewise: the log is off until the option is set again
                const int frames = S->tracer_log;
                S->tracer_log = 0;
                return fail(FS_ENOMEM, "tracer_log: %d frames of %d slots: %s (the option is 0 again)", frames, tr_cap, hipGetErrorString(e));
            }
            HIP_TRY(e);
        }
        if (tr_cap > 0 && tr_emit_gen != S->tracer_emit_gen) {
            if (!S->tracer_emit.empty()) {
                HIP_TRY(hipMemcpyAsync(tr_emit.get(), S->tracer_emit.data(), S->tracer_emit.size() * sizeof(double), hipMemcpyHostToDevice, S->stream));
                HIP_TRY(hipStreamSynchronize(S->stream));    // the host list may change before the copy has run
            }
            tr_emit_gen = S->tracer_emit_gen;
        }
        return FS_OK;
    }

    // one advance: the move of every ALIVE particle, the emitters' release (if `release`), a snapshot frame (if `snapshot`
    // and the log is on).  One launch; the slot cursor is the host's.
    void advance_pass(bool release, bool snapshot)
    {
        fs::TracerPass pass;
        pass.C = tr_cap;
        pass.xyz = tr_xyz.get();
        pass.meta = tr_meta.get();
        pass.k[0] = (double)S->dt * (double)S->W;        // simulation.cpp:384-386, exact in fp64
        pass.k[1] = (double)S->dt * (double)S->H;
        pass.k[2] = (double)S->dt * (double)S->D;
        pass.emit = tr_emit.get();
        pass.n_emit = release ? (int)(S->tracer_emit.size() / 3) : 0;
        pass.first = (int)(S->tracer_seeded % tr_cap);
        pass.born = (int)S->steps_total;
        const bool frame = snapshot && tr_ring.on();
        pass.frame_xyz = frame ? tracer_frame_xyz(tr_ring.at.next()) : nullptr;
        pass.frame_status = frame ? tracer_frame_status(tr_ring.at.next()) : nullptr;
        {
            ScopedSpan sp(S, FAM_TRACERS);
            fs::launch_tracer_advance<T>(S->stream, g, pass, arr[slot[FS_VX]], arr[slot[FS_VY]], arr[slot[FS_VZ]], arr[slot[FS_OBS]]);
        }
        S->tracer_seeded += pass.n_emit;
        if (frame) tr_ring.at.commit(S->steps_total);
    }

    int need(const char* who)
    {
        if (S->comm.active()) return fail(FS_EINVAL, "%s: tracers need a single-GPU handle", who);
        int rc = ensure();
        if (rc) return rc;
        if (tr_cap == 0) return fail(FS_EINVAL, "%s: option \"tracers\" is 0", who);
        return FS_OK;
    }

    int advance()
    {
        int rc = need("fs_tracer_advance");
        if (rc) return rc;
        advance_pass(true, true);
        return FS_OK;
    }

    int seed(const double* xyz, long n)
    {
        int rc = need("fs_tracer_seed");
        if (rc) return rc;
        if (n == 0) return FS_OK;
        // the j-th particle ever seeded goes into slot j % C: of more than C only the last C remain
        const long C = tr_cap, skip = n > C ? n - C : 0, m = n - skip;
        const long first = (S->tracer_seeded + skip) % C, run = std::min<long>(m, C - first);
        std::vector<int32_t> meta((size_t)m * fs::TRACER_META);
        for (long j = 0; j < m; ++j) {
            int32_t* w = &meta[(size_t)j * fs::TRACER_META];
            w[0] = fs::TRACER_ALIVE; w[1] = -1; w[2] = (int32_t)S->steps_total; w[3] = 0;
        }
        const double* src = xyz + 3 * skip;
        HIP_TRY(hipMemcpyAsync(tr_xyz.get() + 3 * first, src, (size_t)run * 3 * sizeof(double), hipMemcpyHostToDevice, S->stream));
        HIP_TRY(hipMemcpyAsync(tr_meta.get() + fs::TRACER_META * first, meta.data(), (size_t)run * fs::TRACER_META * sizeof(int32_t), hipMemcpyHostToDevice, S->stream));
        if (m > run) {
            HIP_TRY(hipMemcpyAsync(tr_xyz.get(), src + 3 * run, (size_t)(m - run) * 3 * sizeof(double), hipMemcpyHostToDevice, S->stream));
            HIP_TRY(hipMemcpyAsync(tr_meta.get(), meta.data() + (size_t)run * fs::TRACER_META, (size_t)(m - run) * fs::TRACER_META * sizeof(int32_t),
                                   hipMemcpyHostToDevice, S->stream));
        }
        HIP_TRY(hipStreamSynchronize(S->stream));        // `xyz` may be freed by the caller
        S->tracer_seeded += n;
        return FS_OK;
    }

    int clear()
    {
        int rc = need("fs_tracer_clear");
        if (rc) return rc;
        HIP_TRY(hipMemsetAsync(tr_xyz.get(), 0, (size_t)tr_cap * 3 * sizeof(double), S->stream));
        HIP_TRY(hipMemsetAsync(tr_meta.get(), 0, (size_t)tr_cap * fs::TRACER_META * sizeof(int), S->stream));
        S->tracer_seeded = 0;
        tr_ring.at.drain();
        return FS_OK;
    }

    int fetch(double* xyz, int32_t* meta, long max, long* n)
    {
        int rc = need("fs_tracer_fetch");
        if (rc) return rc;
        const long count = std::min<long>(S->tracer_seeded, tr_cap);
        if (n) *n = count;
        if (!xyz && !meta) return FS_OK;
        if (max < count) return fail(FS_EINVAL, "fs_tracer_fetch: %ld particles, room for %ld (pass both arrays NULL to ask)", count, max);
        if (count == 0) return FS_OK;
        if (xyz) HIP_TRY(hipMemcpyAsync(xyz, tr_xyz.get(), (size_t)count * 3 * sizeof(double), hipMemcpyDeviceToHost, S->stream));
        if (meta) HIP_TRY(hipMemcpyAsync(meta, tr_meta.get(), (size_t)count * fs::TRACER_META * sizeof(int32_t), hipMemcpyDeviceToHost, S->stream));
        HIP_TRY(hipStreamSynchronize(S->stream));
        return FS_OK;
    }

    int sample(int source, int mode, double* out, long n)
    {
        int rc = need("fs_tracer_sample");
        if (rc) return rc;
        const long count = std::min<long>(S->tracer_seeded, tr_cap);
        if (n != count) return fail(FS_EINVAL, "fs_tracer_sample: the pool holds %ld particles, the call has room for %ld", count, n);
        if (n > 0 && out) {
            const hipError_t e = tr_out.grow((size_t)tr_cap);
            if (e != hipSuccess) return fail(FS_ENOMEM, "fs_tracer_sample: %d values: %s", tr_cap, hipGetErrorString(e));
        }
        return eng.sampling.sample_at("fs_tracer_sample", source, mode, tr_xyz.get(), tr_out.get(), out, n);
    }

    int log_fetch(double* xyz, int32_t* status, long* steps, long max_frames, long* n_frames, long* n_dropped)
    {
        if (S->comm.active()) return fail(FS_EINVAL, "fs_tracer_log: tracers need a single-GPU handle");
        int rc = ensure();
        if (rc) return rc;
        rc = tr_ring.fetch_begin({"fs_tracer_log", "frames", "both arrays NULL"}, tr_ring.at.retained(), max_frames,
                                 xyz || status, n_frames, n_dropped);
        if (rc != LogRing::GO_ON) return rc;
        HIP_TRY(tr_ring.fetch_copy(S->stream, xyz, tracer_frame_xyz(0), (size_t)tr_cap * 3 * sizeof(double),
                                   status, tracer_frame_status(0), (size_t)tr_cap * sizeof(int32_t)));
        tr_ring.fetch_end(steps);
        return FS_OK;
    }

    // fs_step, "tracers": the particles move through the state the step left, the emitters release, a snapshot is taken
    void step()
    {
        if (tr_cap > 0)
            advance_pass((S->steps_total - 1) % S->tracer_emit_every == 0, (S->steps_total - 1) % S->tracer_every == 0);
    }

private:
    Engine<T>& eng;
    fs_sim* const S;
    const fs::GridDesc& g;
    T* (&arr)[NPOOL_MAX];
    int (&slot)[NSLOT];
    // the pool (positions as the sampler's point list, four meta words per slot), the emitters' points, and the snapshot log,
    // a device ring of frames (all position frames, then all status frames)
    DevBuf<double> tr_xyz;
    DevBuf<int> tr_meta;
    int tr_cap = 0;                     // slots allocated: S->tracers once set up
    long tr_gen = -1;                   // S->tracer_gen the pool was set up for
    DevBuf<double> tr_emit;             // FS_TRACER_EMITTERS_MAX points, allocated with the pool
    long tr_emit_gen = -1;              // S->tracer_emit_gen the device list holds
    DevBuf<double> tr_out;              // fs_tracer_sample: one value per slot, allocated at the first call
    LogRing tr_ring;                    // for S->tracer_log_gen, -1 after a new pool
};

}  // namespace
