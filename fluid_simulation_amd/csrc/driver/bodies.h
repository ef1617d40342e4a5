// driver/bodies.h -- per-body forces and moments (csrc/bodies.h; beyond the reference)
#pragma once
#include "common.h"
#include "../bodies.h"

namespace {

template <class T>
struct Bodies {
    explicit Bodies(Engine<T>& e_) : eng(e_), S(e_.S), g(e_.g), arr(e_.arr), slot(e_.slot), flags(e_.flags) {}

    // Label the body cells if obs changed since the last labelling (or `force`).  Synchronises: a mask change is a set-up event.
    int ensure(bool force = false)
    {
        if (S->comm.active()) return fail(FS_EINVAL, "bodies are labelled on a single-GPU handle");
        int rc = eng.ensure_flags();
        if (rc) return rc;
        if (!bodies_dirty && !force && body_L.get()) return FS_OK;
        const long N = eng.dense_cells();
        if (N >= (1L << 31)) return fail(FS_EINVAL, "body labels are 32-bit: %ld padded cells are too many", N);
        DevBuf<int> cnt_buf, lab_buf;                    // the temporaries: freed on every path out
        DevBuf<unsigned long long> ctr_buf;
        DevBuf<long> pairs_buf;
        constexpr int NINFO = (fs::BODY_MAX + 1) * fs::BODY_INFO;
        HIP_TRY(body_L.grow((size_t)N));
        HIP_TRY(body_bbox.grow((fs::BODY_MAX + 1) * 6));
        HIP_TRY(body_planes.grow((size_t)g.D * (fs::BODY_MAX + 1) * fs::BODY_REC));
        HIP_TRY(body_total.grow((fs::BODY_MAX + 1) * fs::BODY_REC));
        HIP_TRY(cnt_buf.alloc(std::max<size_t>(1, (size_t)N)));
        HIP_TRY(ctr_buf.alloc(4 + NINFO));
        int* const cnt = cnt_buf.get();
        unsigned long long* const ctr = ctr_buf.get();   // body cells, components, cursor, changed; then the info table
        HIP_TRY(hipMemsetAsync(ctr, 0, 4 * sizeof(unsigned long long), S->stream));
        fs::launch_body_init<T>(S->stream, g, arr[slot[FS_OBS]], body_L.get(), ctr);
        unsigned long long n_cells = 0;
        HIP_TRY(hipMemcpyAsync(&n_cells, ctr, sizeof n_cells, hipMemcpyDeviceToHost, S->stream));
        HIP_TRY(hipStreamSynchronize(S->stream));
        for (unsigned long long round = 0;; ++round) {
            if (round > n_cells + 1) return fail(FS_EHIP, "body labels did not settle within %llu rounds", round);
            int changed = 0;
            HIP_TRY(hipMemsetAsync(ctr + 3, 0, sizeof(unsigned long long), S->stream));
            fs::launch_body_merge(S->stream, g, body_L.get(), (int*)(ctr + 3));
            HIP_TRY(hipMemcpyAsync(&changed, ctr + 3, sizeof changed, hipMemcpyDeviceToHost, S->stream));
            HIP_TRY(hipStreamSynchronize(S->stream));
            if (!changed) break;
        }
        HIP_TRY(hipMemsetAsync(cnt, 0, (size_t)N * sizeof(int), S->stream));
        fs::launch_body_count(S->stream, g, body_L.get(), cnt, ctr + 1);
        unsigned long long n_roots = 0;
        HIP_TRY(hipMemcpyAsync(&n_roots, ctr + 1, sizeof n_roots, hipMemcpyDeviceToHost, S->stream));
        HIP_TRY(hipStreamSynchronize(S->stream));
        HIP_TRY(pairs_buf.alloc(std::max<size_t>(1, (size_t)n_roots * 2)));
        HIP_TRY(lab_buf.alloc(std::max<size_t>(1, (size_t)n_roots)));
        long* const pairs = pairs_buf.get();
        int* const lab = lab_buf.get();
        fs::launch_body_compact(S->stream, g, body_L.get(), cnt, pairs, ctr + 2);
        std::vector<fs::BodyPair> hp((size_t)n_roots);
        static_assert(sizeof(fs::BodyPair) == 2 * sizeof(long), "pairs travel as two longs");
        if (n_roots) HIP_TRY(hipMemcpyAsync(hp.data(), pairs, (size_t)n_roots * 2 * sizeof(long), hipMemcpyDeviceToHost, S->stream));
        HIP_TRY(hipStreamSynchronize(S->stream));
        const std::vector<int> remap = fs::order_bodies(hp, fs::BODY_MAX);
        if (n_roots) HIP_TRY(hipMemcpyAsync(lab, remap.data(), (size_t)n_roots * sizeof(int), hipMemcpyHostToDevice, S->stream));
        fs::launch_body_relabel(S->stream, g, (long)n_roots, pairs, lab, body_L.get(), cnt);
        unsigned long long hinfo[NINFO];
        for (int k = 0; k <= fs::BODY_MAX; ++k)
            for (int c = 0; c < fs::BODY_INFO; ++c)
                hinfo[k * fs::BODY_INFO + c] = (c == 1 || c == 2 || c == 4 || c == 6) ? ~0ull : 0ull;
        HIP_TRY(hipMemcpyAsync(ctr + 4, hinfo, sizeof hinfo, hipMemcpyHostToDevice, S->stream));
        fs::launch_body_info(S->stream, g, body_L.get(), flags, ctr + 4);
        HIP_TRY(hipMemcpyAsync(hinfo, ctr + 4, sizeof hinfo, hipMemcpyDeviceToHost, S->stream));
        HIP_TRY(hipStreamSynchronize(S->stream));
        body_ncomp = (long)n_roots;
        body_B = (int)std::min<unsigned long long>(n_roots, fs::BODY_MAX);
        body_info_host.assign((size_t)(body_B + 1) * fs::BODY_INFO, 0.0);
        int bbox[(fs::BODY_MAX + 1) * 6];
        for (int k = 0; k <= fs::BODY_MAX; ++k) {
            int* b = bbox + 6 * k;
            b[0] = b[2] = b[4] = 1;
            b[1] = b[3] = b[5] = 0;                     // empty
            if (k > body_B) continue;
            const unsigned long long* q = hinfo + k * fs::BODY_INFO;
            double* o = &body_info_host[(size_t)k * fs::BODY_INFO];
            if (q[0] == 0) {                             // only the REST can be empty
                o[1] = -1.0;
                continue;
            }
            for (int c = 0; c < fs::BODY_INFO; ++c) o[c] = (double)q[c];
            if (k == 0) {                                // the REST scans whole planes
                b[1] = g.W; b[3] = g.H; b[5] = g.D;
            } else {
                b[0] = std::max(1, (int)q[2] - 1); b[1] = std::min(g.W, (int)q[3] + 1);
                b[2] = std::max(1, (int)q[4] - 1); b[3] = std::min(g.H, (int)q[5] + 1);
                b[4] = std::max(1, (int)q[6] - 1); b[5] = std::min(g.D, (int)q[7] + 1);
            }
        }
        HIP_TRY(hipMemcpyAsync(body_bbox.get(), bbox, sizeof bbox, hipMemcpyHostToDevice, S->stream));
        HIP_TRY(hipStreamSynchronize(S->stream));       // `bbox` and the temporaries leave scope
        bodies_dirty = false;
        body_ring.gen = -1;
        return FS_OK;
    }

    // ring slot k, projection j: body_B + 1 whole-grid records
    size_t body_slot_doubles() const { return (size_t)(body_B + 1) * fs::BODY_REC; }
    double* body_slot(long k, int j) const { return (double*)body_ring.slot(k) + (size_t)j * body_slot_doubles(); }

    // "body_force_log" on: label anew if obs changed; (re)allocate and clear the ring after a relabelling,
    // fs_set_option("body_force_log") and ("moment_origin").  Off: nothing is launched or allocated.
    int ensure_ring()
    {
        if (S->body_log > 0) {
            int rc = ensure();
            if (rc) return rc;
        }
        if (body_ring.gen == S->body_log_gen) return FS_OK;
        HIP_TRY(body_ring.setup(S->stream, S->body_log_gen, S->body_log, 2 * body_slot_doubles() * sizeof(double)));
        return FS_OK;
    }

    int label(long* n_components, long* n_bodies)
    {
        int rc = ensure(true);
        if (rc) return rc;
        if (n_components) *n_components = body_ncomp;
        if (n_bodies) *n_bodies = body_B;
        return FS_OK;
    }

    int counts(int* bodies, int* components)
    {
        int rc = ensure();
        if (rc) return rc;
        *bodies = body_B;
        *components = (int)std::min<long>(body_ncomp, 0x7fffffffL);
        return FS_OK;
    }

    int labels(int32_t* dst, size_t n)
    {
        int rc = ensure();
        if (rc) return rc;
        if ((long)n != eng.dense_cells()) return fail(FS_EINVAL, "fs_body_labels: expected %ld elements, got %zu", eng.dense_cells(), n);
        HIP_TRY(hipMemcpyAsync(dst, body_L.get(), n * sizeof(int32_t), hipMemcpyDeviceToHost, S->stream));
        HIP_TRY(hipStreamSynchronize(S->stream));
        return FS_OK;
    }

    int info(double* rows, long max_rows, long* n_rows)
    {
        int rc = ensure();
        if (rc) return rc;
        const long n = body_B + 1;
        if (n_rows) *n_rows = n;
        if (!rows) return FS_OK;
        if (max_rows < n) return fail(FS_EINVAL, "fs_body_info: %ld rows, room for %ld (pass rows = NULL to ask)", n, max_rows);
        memcpy(rows, body_info_host.data(), body_info_host.size() * sizeof(double));
        return FS_OK;
    }

    int query(double* out, long max_rows, long* n_rows, double* per_plane)
    {
        int rc = ensure();
        if (rc) return rc;
        const long n = body_B + 1;
        if (n_rows) *n_rows = n;
        if (!out) return FS_OK;
        if (max_rows < n) return fail(FS_EINVAL, "fs_body_force: %ld rows, room for %ld (pass out = NULL to ask)", n, max_rows);
        {
            ScopedSpan sp(S, FAM_BODYFORCES);
            fs::launch_body_forces<T>(S->stream, g, arr[slot[FS_PRESSURE]], flags, body_L.get(), body_bbox.get(), (int)n, S->moment_origin,
                                      body_planes.get(), body_total.get());
        }
        HIP_TRY(hipMemcpyAsync(out, body_total.get(), (size_t)n * fs::BODY_REC * sizeof(double), hipMemcpyDeviceToHost, S->stream));
        if (per_plane)
            HIP_TRY(hipMemcpyAsync(per_plane, body_planes.get(), (size_t)g.D * n * fs::BODY_REC * sizeof(double), hipMemcpyDeviceToHost, S->stream));
        HIP_TRY(hipStreamSynchronize(S->stream));
        return FS_OK;
    }

    int log_fetch(double* rows, long max_rows, long* n_rows, long* n_dropped)
    {
        if (S->comm.active()) return fail(FS_EINVAL, "bodies are labelled on a single-GPU handle");
        int rc = ensure_ring();
        if (rc) return rc;
        const long nrec = body_B + 1;                    // rows of one step
        const long steps = body_ring.at.retained(), n = steps * nrec;
        rc = body_ring.fetch_begin({"fs_body_force_log", "rows", "rows = NULL"}, n, max_rows, rows != nullptr, n_rows, n_dropped);
        if (rc != LogRing::GO_ON) return rc;
        const size_t per = 2 * body_slot_doubles();      // one step: both projections
        std::vector<double> mine((size_t)steps * per);
        HIP_TRY(body_ring.fetch_copy(S->stream, mine.data()));
        for (long i = 0; i < steps; ++i)
            for (long k = 0; k < nrec; ++k) {
                const double* a = &mine[(size_t)i * per + (size_t)k * fs::BODY_REC];
                const double* b = a + per / 2;
                double* o = rows + ((size_t)i * nrec + (size_t)k) * FS_BODY_LOG_COLS;
                o[0] = (double)body_ring.at.step_of(i);
                o[1] = (double)k;
                for (int c = 0; c < 6; ++c) {
                    o[2 + c] = a[c];
                    o[8 + c] = b[c];
                }
                o[14] = b[6];
                o[15] = b[7];
            }
        body_ring.fetch_end();
        return FS_OK;
    }

    void obs_changed() { bodies_dirty = true; }   // the flag bytes were rebuilt
    // "body_force_log": projection `proj` (0, 1) of the running step; the whole-grid records of every body go into the step's
    // ring slot (no host sync)
    void record(int proj)
    {
        if (!body_ring.on()) return;
        ScopedSpan sp(S, FAM_BODYFORCES);
        fs::launch_body_forces<T>(S->stream, g, arr[slot[FS_PRESSURE]], flags, body_L.get(), body_bbox.get(), body_B + 1, S->moment_origin,
                                  body_planes.get(), body_slot(body_ring.at.next(), proj));
    }
    void commit() { if (body_ring.on()) body_ring.at.commit(S->steps_total); }   // the step is complete

private:
    Engine<T>& eng;
    fs_sim* const S;
    const fs::GridDesc& g;
    T* (&arr)[NPOOL_MAX];
    int (&slot)[NSLOT];
    uint8_t*& flags;
    // the labels (dense padded int32), what the host keeps of the last labelling, and the per-step log, a device ring of
    // steps x 2 projections x (body_B + 1) whole-grid records
    DevBuf<int> body_L;
    bool bodies_dirty = true;           // obs changed since the last labelling
    int body_B = 0;                     // bodies 1 .. body_B; record 0 is the REST
    long body_ncomp = 0;                // components, the REST's included
    std::vector<double> body_info_host; // (body_B + 1) x BODY_INFO
    DevBuf<int> body_bbox;              // per record, the cells its workgroups scan
    DevBuf<double> body_planes;         // plane records of the last launch: g.D x (BODY_MAX + 1) x BODY_REC (stream-ordered reuse)
    DevBuf<double> body_total;          // fs_body_force: the whole-grid records
    LogRing body_ring;                  // for S->body_log_gen, -1 after a relabelling: the ring is set up anew, the log is cleared
};

}  // namespace
