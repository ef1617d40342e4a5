// driver/heat.h -- heat and buoyancy (csrc/heat.h; beyond the reference)
#pragma once
#include "common.h"
#include "../heat.h"

namespace {

template <class T>
struct Heat {
    explicit Heat(Engine<T>& e_) : eng(e_), S(e_.S), g(e_.g), arr(e_.arr), slot(e_.slot), flags(e_.flags) {}

    // The temperature and its pre-solve snapshot are slots F_THETA / F_THETA_PREV of the slot table, behind the public
    // fields, and two more arrays of the pool: allocated when heat is switched on, freed when it is switched off.
    // The pool itself is the core's: it takes the two arrays in (pool_extend) and gives them back (pool_shrink).
    bool on() const { return chunk.get() != nullptr; }
    int alloc_arrays()
    {
        if (on()) return FS_OK;
        DevBuf<T> fresh;
        hipError_t err = fresh.alloc((size_t)NHEAT * eng.pool_stride);
        if (err != hipSuccess) return fail(FS_ENOMEM, "fs_heat_params: the temperature arrays: %s", hipGetErrorString(err));
        if ((err = hipMemsetAsync(fresh.get(), 0, (size_t)NHEAT * eng.pool_stride * sizeof(T), S->stream)) != hipSuccess)
            return fail(FS_EHIP, "fs_heat_params: clearing the temperature arrays: %s", hipGetErrorString(err));
        chunk = std::move(fresh);
        eng.pool_extend(chunk.get());
        return FS_OK;
    }
    int free_arrays()
    {
        if (!on()) return FS_OK;
        const int rc = eng.pool_shrink();                  // synchronises: queued work may still use what is freed here
        if (rc) return rc;
        HIP_TRY(chunk.release());
        HIP_TRY(ws.release());
        return FS_OK;
    }
    // fs_heat_params with values the entry has checked: the arrays and the log first, then the values
    int config(const double* par)
    {
        const int mode = (int)par[fs::HP_MODE], log = mode ? (int)par[fs::HP_LOG] : 0;
        if (mode != 0 && S->comm.active()) return fail(FS_EINVAL, "fs_heat_params: heat needs a single GPU handle (it is not exchanged between slabs)");
        int rc = mode ? alloc_arrays() : free_arrays();
        if (rc) return rc;
        if (log != ring.at.cap) {
            if (log > 0) HIP_TRY(ws.grow(fs::heat_workspace_doubles(g)));
            HIP_TRY(ring.setup(S->stream, 0, log, (size_t)fs::HEAT_COLS * sizeof(double)));
        }
        for (int k = 0; k < fs::HEAT_PARAMS; ++k) S->heat[k] = par[k];
        return FS_OK;
    }
    fs::HeatPass pass_params() const
    {
        fs::HeatPass p;
        p.beta = S->heat[fs::HP_BETA];
        p.alpha = S->heat[fs::HP_ALPHA];
        p.dt = (double)S->dt;
        p.inlet = S->heat[fs::HP_INLET];
        p.wall_t = S->heat[fs::HP_WALL_T];
        p.up = (int)S->heat[fs::HP_UP];
        p.wall = (int)S->heat[fs::HP_WALL];
        for (int k = 0; k < 6; ++k) p.box[k] = (int)S->heat[fs::HP_X0 + k];
        return p;
    }
    int need(const char* who)
    {
        if (S->comm.active()) return fail(FS_EINVAL, "%s: heat needs a single GPU handle (it is not exchanged between slabs)", who);
        if (!on()) return fail(FS_EINVAL, "%s: heat is off (fs_heat_params, mode 1 or 2)", who);
        return FS_OK;
    }
    // Pass A: inlet and wall temperatures, buoyancy on the component along `up`, in place.  One launch.
    int apply_pass(const char* who)
    {
        int rc = need(who);
        if (rc) return rc;
        if ((rc = eng.ensure_flags())) return rc;
        const fs::HeatPass p = pass_params();
        const bool force = p.beta != 0.0 || p.alpha != 0.0;
        const int up = FS_VX + (p.up >> 1);
        if ((rc = eng.unalias(F_THETA))) return rc;
        if (force && (rc = eng.unalias(up))) return rc;
        {
            ScopedSpan sp(S, FAM_HEAT);
            fs::launch_heat_apply<T>(S->stream, g, p, arr[slot[F_THETA]], force ? arr[slot[up]] : nullptr,
                                     force ? arr[slot[FS_DENS]] : nullptr, flags);
        }
        ++S->n_heat_apply;
        return FS_OK;
    }
    // Pass B: the reference's diffusion and advection of a scalar, on the temperature (no new kernel)
    int transport_pass(const char* who)
    {
        int rc = need(who);
        if (rc) return rc;
        if ((rc = eng.ensure_flags())) return rc;
        // dt * kappa * width * height * depth, left to right like eng.diffusion_a()
        const T a = (T)S->dt * (T)S->heat[fs::HP_KAPPA] * (T)S->W * (T)S->H * (T)S->D;
        const T c = (T)1 + (T)6 * a;
        if (S->solver == FS_SOLVER_GS_LEX || S->acc <= 0) {
            if ((rc = eng.unalias(F_THETA)) || (rc = eng.unalias(F_THETA_PREV))) return rc;
            ScopedSpan sp(S, FAM_MISC);
            fs::launch_copy<T>(S->stream, g, arr[slot[F_THETA]], arr[slot[F_THETA_PREV]]);
        } else {
            slot[F_THETA_PREV] = slot[F_THETA];          // Jacobi never writes its input: the snapshot is an alias
        }
        int res;
        if ((rc = eng.solve(0, slot[F_THETA], slot[F_THETA_PREV], a, c, S->acc, &res))) return rc;
        eng.adopt(F_THETA_PREV, res);                        // the solved array: what the advection carries
        if ((rc = eng.advect(0, F_THETA, F_THETA_PREV))) return rc;
        ++S->n_heat_transport;
        return FS_OK;
    }
    int apply()
    {
        if (!eng.in_step) eng.vzmax_prev = -1.0;
        return apply_pass("fs_heat_apply");
    }
    int transport() { return transport_pass("fs_heat_transport"); }

    // Pass C: the heat budget of the state as it is now into `result` (a ring slot or the workspace's result slot)
    void budget_launch(double* result)
    {
        ScopedSpan sp(S, FAM_HEAT, 3);
        fs::launch_heat_budget<T>(S->stream, g, pass_params(), arr[slot[F_THETA]], arr[slot[FS_VX]], flags, ws.get(), result);
    }
    // fs_step, the heat log: the budget of the state the transport left (three launches, no host synchronisation)
    void record()
    {
        if (!ring.on()) return;
        budget_launch((double*)ring.slot(ring.at.next()));
        ring.at.commit(S->steps_total);
    }
    int budget(double* out, double* per_plane)
    {
        int rc = need("fs_heat_budget");
        if (rc) return rc;
        if ((rc = eng.ensure_flags())) return rc;
        const size_t total = fs::heat_workspace_doubles(g), planes = fs::heat_planes_offset(g);
        HIP_TRY(ws.grow(total));
        budget_launch(ws.get() + (total - fs::HEAT_COLS));
        std::vector<double> host(total - planes);        // the plane records, then the result
        HIP_TRY(hipMemcpyAsync(host.data(), ws.get() + planes, host.size() * sizeof(double), hipMemcpyDeviceToHost, S->stream));
        HIP_TRY(hipStreamSynchronize(S->stream));
        memcpy(out, host.data() + (size_t)g.D * fs::HEAT_COLS, fs::HEAT_COLS * sizeof(double));
        if (per_plane) memcpy(per_plane, host.data(), (size_t)g.D * fs::HEAT_COLS * sizeof(double));
        return FS_OK;
    }
    int log_fetch(double* rows, long max_rows, long* n_rows, long* n_dropped)
    {
        if (S->comm.active()) return fail(FS_EINVAL, "fs_heat_log: heat needs a single GPU handle");
        const long n = ring.at.retained();
        int rc = ring.fetch_begin({"fs_heat_log", "rows", "rows = NULL"}, n, max_rows, rows != nullptr, n_rows, n_dropped);
        if (rc != LogRing::GO_ON) return rc;
        std::vector<double> mine((size_t)n * fs::HEAT_COLS);
        HIP_TRY(ring.fetch_copy(S->stream, mine.data()));
        for (long i = 0; i < n; ++i) {
            double* o = rows + (size_t)i * FS_HEAT_LOG_COLS;
            o[0] = (double)ring.at.step_of(i);
            memcpy(o + 1, &mine[(size_t)i * fs::HEAT_COLS], fs::HEAT_COLS * sizeof(double));
        }
        ring.fetch_end();
        return FS_OK;
    }
    int get(void* dst, size_t n, int elem)
    {
        int rc = need("fs_heat_get");
        if (rc) return rc;
        return eng.get_field(F_THETA, dst, n, elem);
    }
    int set(const void* src, size_t n, int elem)
    {
        int rc = need("fs_heat_set");
        if (rc) return rc;
        return eng.set_field(F_THETA, src, n, elem);
    }

private:
    Engine<T>& eng;
    fs_sim* const S;
    const fs::GridDesc& g;
    T* (&arr)[NPOOL_MAX];
    int (&slot)[NSLOT];
    uint8_t*& flags;
    DevBuf<T> chunk;                    // the allocation behind the pool's two extra arrays
    DevBuf<double> ws;                  // workspace of the heat budget's three launches (stream-ordered reuse)
    LogRing ring;                       // the per-step heat log: records of HEAT_COLS doubles
};

}  // namespace
