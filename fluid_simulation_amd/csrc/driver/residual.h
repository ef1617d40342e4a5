// driver/residual.h -- residual of the linear solves (csrc/residual.h; beyond the reference)
#pragma once
#include "common.h"
#include "../residual.h"
#include "plane_records.h"

namespace {

template <class T>
struct Residual {
    explicit Residual(Engine<T>& e_) : eng(e_), S(e_.S), g(e_.g), arr(e_.arr), slot(e_.slot), flags(e_.flags) {}

    static constexpr int RES_SOLVES = FS_RESIDUAL_LOG_SOLVES;
    size_t plane_doubles() const { return (size_t)fs::RESIDUAL_REC * (size_t)g.D; }
    // ring slot k, solve j, when = 0 before the first sweep / 1 after the last: g.D plane records
    double* ring_slot(long k, int j, int when) const { return (double*)ring.slot(k) + ((size_t)j * 2 + (size_t)when) * plane_doubles(); }

    int ensure_partial()
    {
        HIP_TRY(partial.grow(fs::residual_partial_doubles(g)));
        return FS_OK;
    }

    // (re)allocate and clear the ring after fs_set_option("residual_log")
    int ensure_ring()
    {
        if (ring.gen == S->residual_log_gen) return FS_OK;
        HIP_TRY(ring.setup(S->stream, S->residual_log_gen));   // off, whatever fails below
        if (S->residual_log <= 0) return FS_OK;
        int rc = ensure_partial();
        if (rc) return rc;
        HIP_TRY(ring.setup(S->stream, S->residual_log_gen, S->residual_log, (size_t)RES_SOLVES * 2 * plane_doubles() * sizeof(double)));
        return FS_OK;
    }

    // "residual_log": solve k of the running step, before (when = 0) or after (1) its sweeps, straight into the step's ring
    // slot on the compute stream (no host sync).  On a z-slab the halo planes of `x` are current at both points: the
    // producer of x exchanged them (advection, inlet, the zeroed pressure), and so does the last pass of every solve.
    int log(int k, int when, int b, int x, int rhs, double a, double c)
    {
        if (k < 0 || !ring.on() || !eng.in_step) return FS_OK;
        ScopedSpan sp(S, FAM_RESIDUAL);
        fs::launch_residual<T>(S->stream, g, b, arr[x], arr[rhs], flags, a, c, partial.get(), ring_slot(ring.at.next(), k, when));
        if (when == 1) ran_now |= 1u << k;
        return FS_OK;
    }

    int query(int b, int field, int prev, double a, double c, double* out4, double* per_plane)
    {
        if (S->comm.active() && S->comm.null_transport) return fail(FS_EINVAL, "solve residuals need the other slabs' planes; the FSNULL transport carries none");
        int rc = eng.ensure_flags();
        if (rc) return rc;
        // a boundary plane's record reads the neighbour's plane of x: one exchange, on the query's account only
        if ((rc = eng.halo(arr[slot[field]]))) return rc;
        if ((rc = ensure_partial())) return rc;
        const size_t n = plane_doubles();
        HIP_TRY(scratch.grow(n));
        {
            ScopedSpan sp(S, FAM_RESIDUAL);
            fs::launch_residual<T>(S->stream, g, b, arr[slot[field]], arr[slot[prev]], flags, a, c, partial.get(), scratch.get());
        }
        std::vector<double> mine(n), all;
        HIP_TRY(hipMemcpyAsync(mine.data(), scratch.get(), n * sizeof(double), hipMemcpyDeviceToHost, S->stream));
        HIP_TRY(hipStreamSynchronize(S->stream));
        if ((rc = gather_plane_records(eng, mine, all, "solve residuals"))) return rc;
        combine_planes(S, g, [&](int r, int zl) { return &all[(size_t)r * n + (size_t)zl * fs::RESIDUAL_REC]; }, out4, fs::RESIDUAL_REC, 2);
        if (per_plane) memcpy(per_plane, all.data(), all.size() * sizeof(double));
        return FS_OK;
    }
    int solve_residual(int b, int field, int prev, double a, double c, double* out4, double* per_plane)
    {
        if (!std::is_same<T, double>::value) { a = (double)(float)a; c = (double)(float)c; }   // what an fp32 solve would use
        return query(b, field, prev, a, c, out4, per_plane);
    }
    int diffuse_residual(int b, int field, int prev, double* out4, double* per_plane)
    {
        const T a = eng.diffusion_a();
        return query(b, field, prev, (double)a, (double)((T)1 + (T)6 * a), out4, per_plane);
    }

    int log_fetch(double* rows, long max_rows, long* n_rows, long* n_dropped)
    {
        int rc = ensure_ring();
        if (rc) return rc;
        const long n = ring.at.retained();
        rc = ring.fetch_begin({"fs_residual_log", "rows", "rows = NULL"}, n, max_rows, rows != nullptr, n_rows, n_dropped);
        if (rc != LogRing::GO_ON) return rc;
        if (S->comm.active() && S->comm.null_transport) return fail(FS_EINVAL, "solve residuals need the other slabs' planes; the FSNULL transport carries none");
        const size_t rec = plane_doubles(), per = (size_t)RES_SOLVES * 2 * rec;   // one step: six solves, before and after
        std::vector<double> mine((size_t)n * per), all;
        HIP_TRY(ring.fetch_copy(S->stream, mine.data()));
        if ((rc = gather_plane_records(eng, mine, all, "solve residuals"))) return rc;
        const size_t blob = mine.size();
        const double nan = std::nan("");
        for (long i = 0; i < n; ++i) {
            double* o = rows + (size_t)i * FS_RESIDUAL_LOG_COLS;
            o[0] = (double)ring.at.step_of(i);
            for (int j = 0; j < RES_SOLVES; ++j) {
                double* q = o + 1 + 5 * j;               // r0_sq, r_sq, r_max, rhs_sq, cells
                if (!(ring.at.tag_of(i) >> j & 1u)) { q[0] = q[1] = q[2] = q[3] = nan; q[4] = 0.0; continue; }
                double s[2][fs::RESIDUAL_REC];
                for (int when = 0; when < 2; ++when)
                    combine_planes(S, g, [&](int r, int zl) {
                        return &all[(size_t)r * blob + (size_t)i * per + ((size_t)j * 2 + (size_t)when) * rec + (size_t)zl * fs::RESIDUAL_REC]; },
                        s[when], fs::RESIDUAL_REC, 2);
                q[0] = s[0][0];
                q[1] = s[1][0];
                q[2] = s[1][2];
                q[3] = s[1][1];
                q[4] = s[1][3];
            }
        }
        ring.fetch_end();
        return FS_OK;
    }

    bool on() const { return ring.on(); }
    void begin_step() { ran_now = 0; }
    void commit() { if (ring.on()) ring.at.commit(S->steps_total, ran_now); }   // the step is complete

private:
    Engine<T>& eng;
    fs_sim* const S;
    const fs::GridDesc& g;
    T* (&arr)[NPOOL_MAX];
    int (&slot)[NSLOT];
    uint8_t*& flags;
    // the per-step log is a device ring of steps x 6 solves x {before, after} x g.D plane records
    LogRing ring;                       // for S->residual_log_gen; a slot's tag, bit k: solve k of that step ran (an elided solve leaves no record)
    DevBuf<double> scratch;             // fs_solve_residual: one record per local plane
    DevBuf<double> partial;             // the row-chunk records between the two kernels of a launch (stream-ordered reuse)
    unsigned ran_now = 0;               // the tag of the step that is running
};

}  // namespace
