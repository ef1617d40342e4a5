// driver/flow_stats.h -- time-averaged flow statistics (csrc/flow_stats.h; beyond the reference)
#pragma once
#include "common.h"
#include "../flow_stats.h"

namespace {

template <class T>
struct FlowStats {
    explicit FlowStats(Engine<T>& e_) : eng(e_), S(e_.S), g(e_.g), sc(e_.sc), arr(e_.arr), slot(e_.slot) {}

    size_t bytes() const { return (size_t)fs::flow_stats_groups(g.sz, g.D) * 4 * sizeof(double); }

    // allocate, free and clear after fs_set_option("flow_stats"); a reset needs no pass over memory (the first sample overwrites)
    int config()
    {
        if (gen == S->flow_stats_gen) return FS_OK;
        gen = S->flow_stats_gen;
        S->flow_stats_n = 0;
        if (nacc == S->flow_stats) return FS_OK;
        HIP_TRY(hipStreamSynchronize(S->stream));        // a queued sample may still write what is freed here
        for (int k = 0; k < nacc; ++k) buf[k].release();
        acc = fs::FlowStatsAcc{};
        nacc = 0;
        for (int k = 0; k < S->flow_stats; ++k) {
            const hipError_t e = buf[k].alloc(bytes() / sizeof(double));
            acc.a[k] = buf[k].get();
            if (e != hipSuccess) {
                for (int j = 0; j < k; ++j) buf[j].release();
                acc = fs::FlowStatsAcc{};
                const int want = S->flow_stats;
                S->flow_stats = 0;
                return fail(FS_ENOMEM, "flow_stats: %d accumulator arrays of %zu bytes: %s (the feature is off now)", want, bytes(),
                            hipGetErrorString(e));
            }
        }
        nacc = S->flow_stats;
        return FS_OK;
    }

    int sample()
    {
        int rc = config();
        if (rc) return rc;
        if (nacc == 0) return fail(FS_EINVAL, "fs_flow_stats_sample: option \"flow_stats\" is off");
        ScopedSpan sp(S, FAM_FLOWSTATS);
        fs::launch_flow_stats<T>(S->stream, g, nacc, S->flow_stats_n == 0, arr[slot[FS_DENS]], arr[slot[FS_VX]], arr[slot[FS_VY]],
                                 arr[slot[FS_VZ]], arr[slot[FS_PRESSURE]], acc);
        S->flow_stats_n++;
        return FS_OK;
    }

    // which: selector without FS_STAT_RAW
    int check(const char* who, int sel)
    {
        const int which = sel & ~FS_STAT_RAW;
        const bool raw = (sel & FS_STAT_RAW) != 0;
        if (which < 0 || which > FS_STAT_TKE) return fail(FS_EINVAL, "%s: unknown selector %d", who, sel);
        if (nacc == 0) return fail(FS_EINVAL, "%s: option \"flow_stats\" is off", who);
        if (raw && which == FS_STAT_TKE) return fail(FS_EINVAL, "%s: FS_STAT_TKE has no raw sum", who);
        if (which >= fs::ST_NMEAN && nacc < fs::ST_NMOMENTS)
            return fail(FS_EINVAL, "%s: selector %d needs \"flow_stats\" = \"moments\" (the mode is \"mean\")", who, which);
        if (!raw && S->flow_stats_n == 0) return fail(FS_EINVAL, "%s: no samples taken yet (n = 0)", who);
        return FS_OK;
    }

    // The derived field goes into the staging buffer in the accumulators' layout, and from there through launch_pack into
    // the dense layout behind it.
    int field(int sel, void* dst, size_t n, int elem)
    {
        int rc = config();
        if (rc) return rc;
        if ((rc = check("fs_flow_stats_field", sel))) return rc;
        if ((long)n != eng.dense_cells()) return fail(FS_EINVAL, "fs_flow_stats_field: expected %ld elements, got %zu", eng.dense_cells(), n);
        if (elem != 4 && elem != 8) return fail(FS_EINVAL, "elem_size must be 4 or 8");
        if ((rc = eng.need_dense(bytes() + n * (size_t)elem))) return rc;
        double* pitched = (double*)eng.dense.get();
        void* packed = (char*)eng.dense.get() + bytes();
        if (S->flow_stats_n == 0) {                      // a raw sum before the first sample: +0.0 (the arrays hold nothing yet)
            HIP_TRY(hipMemsetAsync(packed, 0, n * (size_t)elem, S->stream));
        } else {
            fs::launch_flow_stats_finalize(S->stream, g, acc, sel & ~FS_STAT_RAW, (sel & FS_STAT_RAW) != 0, S->flow_stats_n,
                                           !sc.lo_wall, !sc.hi_wall, pitched);
            if (elem == 4) fs::launch_pack<double, float>(S->stream, g, pitched + fs::LEAD, (float*)packed, 0, g.D + 1);
            else fs::launch_pack<double, double>(S->stream, g, pitched + fs::LEAD, (double*)packed, 0, g.D + 1);
        }
        HIP_TRY(hipMemcpyAsync(dst, packed, n * elem, hipMemcpyDeviceToHost, S->stream));
        HIP_TRY(hipStreamSynchronize(S->stream));
        return FS_OK;
    }

    int dump(const char* dir)
    {
        int rc = config();
        if (rc) return rc;
        static const char* const names[7] = { "data.bin", "obs.bin", "v_x.bin", "v_y.bin", "v_z.bin", "p.bin", "tke.bin" };
        static const int sel[7] = { FS_STAT_MEAN_DENS, -1, FS_STAT_MEAN_VX, FS_STAT_MEAN_VY, FS_STAT_MEAN_VZ, FS_STAT_MEAN_P, FS_STAT_TKE };
        const int nfiles = nacc >= fs::ST_NMOMENTS ? 7 : 6;
        if ((rc = check("fs_flow_stats_dump", FS_STAT_MEAN_DENS))) return rc;
        // rank 0 truncates; the other slab ranks open the files for update once they exist (as dump_frame does)
        const bool lead = !S->comm.active() || S->comm.rank == 0;
        FILE* fp[7] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
        bool ok = true;
        for (int pass = 0; pass < 2; ++pass) {
            if ((pass == 0) == lead)
                for (int k = 0; k < nfiles; ++k) {
                    fp[k] = fopen((std::string(dir) + "/" + names[k]).c_str(), lead ? "wb" : "r+b");
                    if (!fp[k]) ok = false;
                }
            if (pass == 0 && S->comm.active()) {
                if (S->comm.shm && S->comm.shm_ready(g, S->D)) return fail(FS_ECOMM, "%s", S->comm.last_error());
                if ((rc = eng.slab_barrier())) return rc;
            }
        }
        // local planes written by this rank: its interior planes, plus the physical ghost planes
        const int zlo = sc.lo_wall ? 0 : 1, zhi = sc.hi_wall ? g.D + 1 : g.D;
        const size_t plane = (size_t)(g.W + 2) * (g.H + 2);
        std::vector<float> h((size_t)eng.dense_cells());
        for (int k = 0; k < nfiles && ok && !rc; ++k) {
            rc = sel[k] < 0 ? eng.get_field(FS_OBS, h.data(), h.size(), 4) : field(sel[k], h.data(), h.size(), 4);
            if (rc) break;
            if (fseek(fp[k], (long)(plane * (size_t)(sc.zoff + zlo) * sizeof(float)), SEEK_SET) != 0 ||
                fwrite(h.data() + plane * (size_t)zlo, sizeof(float), plane * (size_t)(zhi - zlo + 1), fp[k]) != plane * (size_t)(zhi - zlo + 1))
                ok = false;
        }
        for (int k = 0; k < nfiles; ++k)
            if (fp[k] && fclose(fp[k]) != 0) ok = false;
        if (S->comm.active() && !rc) rc = eng.slab_barrier();     // every rank's planes are in the files
        if (rc) return rc;
        if (!ok) return fail(FS_EIO, "fs_flow_stats_dump: cannot write the mean-flow frames under '%s'", dir);
        return FS_OK;
    }

    bool on() const { return nacc > 0; }
    // A source FS_SAMPLE_STAT | sel of the sampler (resolve_source): the derived field goes into the core's staging buffer in
    // the accumulators' layout, which is the fields' pitched one (-> stat, LEAD-shifted)
    int stage(const char* who, int sel, const double*& stat)
    {
        int rc;
        if ((rc = config())) return rc;
        if ((rc = check(who, sel))) return rc;
        if ((rc = eng.need_dense(bytes()))) return rc;
        if (S->flow_stats_n == 0)                    // a raw sum before the first sample: +0.0
            HIP_TRY(hipMemsetAsync(eng.dense.get(), 0, bytes(), S->stream));
        else
            fs::launch_flow_stats_finalize(S->stream, g, acc, sel & ~FS_STAT_RAW, (sel & FS_STAT_RAW) != 0, S->flow_stats_n,
                                           false, false, (double*)eng.dense.get());
        stat = (const double*)eng.dense.get() + fs::LEAD;
        return FS_OK;
    }

private:
    Engine<T>& eng;
    fs_sim* const S;
    const fs::GridDesc& g;
    const fs::SlabCtx& sc;
    T* (&arr)[NPOOL_MAX];
    int (&slot)[NSLOT];
    // private allocations, one per accumulator, never exported to slab neighbours
    DevBuf<double> buf[fs::ST_NMOMENTS];
    fs::FlowStatsAcc acc = {};          // their pointers, as the kernels take them
    int nacc = 0;                      // accumulators allocated: 0, 5 or 12
    long gen = -1;                      // S->flow_stats_gen they were set up for
};

}  // namespace
