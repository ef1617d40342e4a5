// fluidsim.cpp -- C-ABI host driver of libfluidsim.so (include/fluidsim.h).
//
// Owns device storage, orders the kernels of one time step on a HIP stream, converts
// between the device layout and the reference's dump layout, and (multi-GPU) exchanges
// z-slab halo planes over RCCL.  No arithmetic on field data happens on the host and
// there is no CPU fallback: without a usable HIP device fs_create fails.
//
// Orchestration follows Simulation::step()/run() of the reference (simulation.cpp:49-150);
// every numeric expression lives in the kernel files (kernels_dev.h lists them).
//
// One translation unit: this file holds the core of Engine<T> (the reference's step) and the C entries; each feature
// beyond the reference is a part of the engine in driver/<feature>.h, over driver/common.h.
#include "../../include/fluidsim.h"
#include "kernels.h"
#include "voxelize.h"
#include "comm.h"
#include "dump.h"
#include "streamlines.h"
#include "surface.h"
#include "multigrid.h"
#include "forces.h"
#include "bodies.h"
#include "image.h"
#include "volume.h"
#include "tracers.h"
#include "monitor.h"
#include "residual.h"
#include "flow_stats.h"
#include "vortex.h"
#include "confine.h"
#include "inflow.h"
#include "heat.h"
#include "zones.h"
#include "sample.h"
#include "step_ring.h"
#include "options.h"

#include "driver/common.h"
#include "driver/forces.h"
#include "driver/bodies.h"
#include "driver/residual.h"
#include "driver/flow_stats.h"
#include "driver/vortex.h"
#include "driver/sampling.h"
#include "driver/images.h"
#include "driver/volume.h"
#include "driver/tracers.h"
#include "driver/monitor.h"
#include "driver/inflow.h"
#include "driver/heat.h"
#include "driver/zones.h"
#include "driver/confine.h"
#include "driver/viewer.h"

namespace {

// what "auto" means for the options "zero_start" and "fuse_project_advect": decided by measurement.
// (-DFS_ZERO_START_AUTO=0|1, -DFS_PROJECT_ADVECT_AUTO=0|1: development builds for same-box A/B runs of an unchanged bench.py)
#ifndef FS_ZERO_START_AUTO
#define FS_ZERO_START_AUTO 1
#endif
#ifndef FS_PROJECT_ADVECT_AUTO
#define FS_PROJECT_ADVECT_AUTO 1
#endif
constexpr bool ZERO_START_AUTO = FS_ZERO_START_AUTO != 0, PROJECT_ADVECT_AUTO = FS_PROJECT_ADVECT_AUTO != 0;
// ... and for fs_set_int "z_alternate" (-DFS_Z_ALTERNATE_AUTO=0|1), on grids whose iterate, target and right-hand side together outgrow the
// Infinity Cache; smaller grids stay in it whichever way a pass runs, and auto leaves them alone.
#ifndef FS_Z_ALTERNATE_AUTO
#define FS_Z_ALTERNATE_AUTO 1
#endif
constexpr bool Z_ALTERNATE_AUTO = FS_Z_ALTERNATE_AUTO != 0;
constexpr size_t INFINITY_CACHE_BYTES = (size_t)256 << 20;
const char* const kFamilyNames[FAM_HEAT] = { "sweep", "sweep_pair", "sweep_triple", "divergence", "gradient", "advect", "bounds", "misc", "comm", "multigrid", "forces", "residual", "flow_stats", "vortex", "probes", "body_forces", "images", "tracers", "volume", "confinement", "monitor", "inflow" };
// the families added since (tests/test_inflow_cpu.py pins the text of the table above): FAM_HEAT onwards
const char* const kLaterFamilyNames[FAM_COUNT - FAM_HEAT] = { "heat", "zones" };

// ---------------------------------------------------------------------------------------
template <class T>
struct Engine : EngineBase {
    fs_sim* S;
    fs::GridDesc g;       // local slab
    fs::SlabCtx sc;
    static constexpr size_t ARENA_CHUNK_BYTES = (size_t)1 << 30;
    std::vector<T*> pool_chunks;        // the allocations behind arr[]: pool_per arrays each, pool_stride elements apart
    std::vector<size_t> pool_chunk_bytes;
    size_t pool_stride = 0;
    int pool_per = 1;
    std::vector<T*> gather_chunks;      // the same behind gathered / gathered3 (z-slabs, allocated at the first gather)
    T* arr[NPOOL_MAX] = {nullptr};      // LEAD-shifted pointers; the last NHEAT exist while heat is on
    int slot[NSLOT];                    // field -> array id (aliases allowed inside a step); F_THETA / F_THETA_PREV: -1 while heat is off
    bool held[NPOOL_MAX] = {false};     // temporaries owned by a running solve
    int npool = NPOOL;                  // arrays of the pool: NPOOL_MAX while heat is on
    DevBuf<uint8_t> flags_buf, kill_buf;   // what the two views below look into
    uint8_t* flags = nullptr;           // shifted like the fields
    uint8_t* kill = nullptr;            // one byte per four cells for the sweeps; byte (cell+3)/4
    fs::MaskPlan maskplan;              // single GPU, fp32: which rows are free of kill bytes (the three-sweep kernel's mask-free body)
    bool flags_dirty = true;
    bool halos_dirty = false;           // a host-side mutation may have changed a slab boundary plane
    DevBuf<char> dense;                 // device staging of fs_get_field / fs_set_field (dense local slab), grown on demand
    T* gathered = nullptr;              // gathered advection source (z-slabs only), LEAD-shifted global array
    T* gathered3[3] = {nullptr, nullptr, nullptr};   // the same for the three sources of the fused velocity advection
    DevBuf<double> red;                 // stats scratch
    T rb_omega = (T)1;                  // relaxation factor of the red-black / damped passes of the running solve
    bool rb_damped = false;             // those passes are two damped Jacobi sweeps (solver=mg level 0) instead of one red-black iteration
    fs::Multigrid<T> mg;                // coarse levels of solver=mg; rebuilt when the flag bytes change
    bool mg_current = false;
    DevBuf<T> coltab;                   // clamp tables of the advection row kernels: 6 x (H+2)(D+2) (single GPU only)
    // launch plan ids (launch_plan.h), chosen once per grid by choose_launch_plans
    int plan_two = -1;                  // fastest two-sweep plan, of the pair or the fused kernel (-1: not chosen yet)
    int plan_two_pair = 0;              // fastest plan of jacobi_pair_kernel itself: its red-black / damped passes (rbsor, mg level 0)
                                        // always run that kernel, also where the plain two-sweep passes went to the fused one
    int plan_three = -1;                // >= 0: three sweeps per pass beat two on this grid
    struct TunedFor {                   // what those choices were made under: options, and the "launch_plans" values
        int fuse = -1, pair_shape = -1, two_kind = -1, replay_two = -3, replay_three = -3;
        bool operator==(const TunedFor& o) const { return !memcmp(this, &o, sizeof o); }
    } tuned_for;
    hipStream_t comm_stream = nullptr;  // z-slabs: EVERY transport call runs on this one stream (a communicator is never driven from
                                        // two streams); events order it against the compute stream
    hipEvent_t ev_edges = nullptr, ev_halo = nullptr, ev_int = nullptr, ev_c2x = nullptr;
    // z-slabs: the reach of the advection back-trace without a host synchronisation.  max |v_z| after each of the step's two
    // projections is reduced over the ranks and copied to pinned memory asynchronously; the host waits for the EVENT behind the copy
    // when it sizes the gather, by which time the device has long passed it (see step()).
    double* reach_pinned = nullptr;     // 3 x {sum, min, max}: after the first / second projection, at the start of the step
    hipEvent_t ev_reach[3] = {nullptr, nullptr, nullptr};
    hipEvent_t ev_slack = nullptr;      // behind the independent work queued between a projection and the advection that needs its reach
    bool reach_posted[3] = {false, false, false};
    double vzmax_prev = -1.0;           // max |v_z| at the end of the previous step (= v_z_prev of this one), -1 = unknown
    double vzmax_end = -1.0;            // the same for the step that is running
    bool in_step = false;               // inside step(): the data flow between the solver's calls is known
    // the features beyond the reference's step, one part each (driver/*.h): a part's state is private to it, and it reaches the
    // core through its reference to the engine
    Forces<T> forces{*this};
    Bodies<T> bodies{*this};
    Residual<T> residual{*this};
    FlowStats<T> flow_stats{*this};
    Vortex<T> vortex{*this};
    Sampling<T> sampling{*this};
    Images<T> images{*this};
    Volume<T> volume{*this};
    Tracers<T> tracers{*this};
    Monitor<T> monitor{*this};
    Inflow<T> inflow{*this};
    Heat<T> heat{*this};
    Zones<T> zones{*this};
    Confine<T> confine{*this};
    Viewer<T> viewer{*this};
    static constexpr int SLOT_POOL = 0, SLOT_GATHER = NPOOL, SLOT_MG = NPOOL + 4;   // FSIPC export slots: one per arena chunk
    static constexpr int NRED = 3 * 1024 + 18;   // reduction scratch + up to six {sum, min, max} results (0, 1: stats / trace_reach; 2..4: post_vzmax)

    explicit Engine(fs_sim* s) : S(s) {}

    long dense_cells() const { return (long)(g.W + 2) * (g.H + 2) * (g.D + 2); }

    int need_dense(size_t bytes)
    {
        HIP_TRY(dense.grow(bytes));
        return FS_OK;
    }

    int init()
    {
        const fs::Comm& cm = S->comm;
        g.W = S->W; g.H = S->H;
        g.D = cm.active() ? cm.local_depth(S->D) : S->D;
        g.sy = ((long)(g.W + 5) + 3) / 4 * 4;
        g.sz = g.sy * (g.H + 2);
        // z-slabs keep as many halo planes per side as the deepest fused pass has levels (it recomputes the lower
        // levels of the neighbours' boundary planes): three where the three-sweep kernel exists, else two
        g.zh = !cm.active() ? 1 : (std::is_same<T, float>::value && g.W <= 512 && g.D >= 3) ? 3 : 2;
        g.lead = fs::LEAD + (long)(g.zh - 1) * g.sz;
        g.n = g.sz * (g.D + 2 * g.zh) + 8;   // lead + tail so that a dwordx4 at the last ghost stays in bounds
        g.n = (g.n + 3) / 4 * 4;
        sc.zoff = cm.active() ? cm.z_offset(S->D) : 0;
        sc.Dglobal = S->D;
        sc.lo_wall = (!cm.active() || cm.rank == 0) ? 1 : 0;
        sc.hi_wall = (!cm.active() || cm.rank == cm.nranks - 1) ? 1 : 0;
        // The field arrays live in a few large allocations ("arena chunks"), not one hipMalloc each: a slab rank exports
        // every chunk to its neighbours as one hipIpc handle.  Many small exports alias after a few handles of one process,
        // and an export beyond 2 GiB never returns on the HIP runtime PyTorch bundles (both seen in round 3's bench
        // rehearsals), so a chunk holds as many arrays as fit 1 GiB.
        pool_stride = (g.n + 63) / 64 * 64;              // keeps every array's first interior cell 16-byte aligned
        pool_per = (int)std::max<size_t>(1, ARENA_CHUNK_BYTES / (pool_stride * sizeof(T)));
        if (pool_per > NPOOL) pool_per = NPOOL;
        for (int i = 0; i < NPOOL; i += pool_per) {
            const size_t cnt = (size_t)std::min(pool_per, NPOOL - i) * pool_stride;
            T* chunk = nullptr;
            HIP_TRY(hipMalloc((void**)&chunk, cnt * sizeof(T)));
            pool_chunks.push_back(chunk);
            pool_chunk_bytes.push_back(cnt * sizeof(T));
            HIP_TRY(hipMemsetAsync(chunk, 0, cnt * sizeof(T), S->stream));   // simulation.cpp:38-43
        }
        for (int i = 0; i < NPOOL; ++i) arr[i] = pool_chunks[(size_t)(i / pool_per)] + (size_t)(i % pool_per) * pool_stride + g.lead;
        for (int f = 0; f < FS_NFIELDS; ++f) slot[f] = f;
        slot[F_THETA] = slot[F_THETA_PREV] = -1;
        HIP_TRY(flags_buf.alloc((size_t)g.n));
        HIP_TRY(hipMemsetAsync(flags_buf.get(), 0, g.n, S->stream));
        flags = flags_buf.get() + g.lead;
        HIP_TRY(kill_buf.alloc((size_t)g.n / 4 + 16));
        HIP_TRY(hipMemsetAsync(kill_buf.get(), 0, g.n / 4 + 16, S->stream));
        kill = kill_buf.get() + (g.lead - fs::LEAD) / 4;
        HIP_TRY(red.alloc(NRED));
        if (!cm.active()) HIP_TRY(coltab.alloc((size_t)6 * (size_t)(g.H + 2) * (size_t)(g.D + 2)));
        if (cm.active()) {
            int lo_pri = 0, hi_pri = 0;
            HIP_TRY(hipDeviceGetStreamPriorityRange(&lo_pri, &hi_pri));
            HIP_TRY(hipStreamCreateWithPriority(&comm_stream, hipStreamNonBlocking, hi_pri));
            for (hipEvent_t* ev : { &ev_edges, &ev_halo, &ev_int, &ev_c2x, &ev_reach[0], &ev_reach[1], &ev_reach[2], &ev_slack })
                HIP_TRY(hipEventCreateWithFlags(ev, hipEventDisableTiming));
            HIP_TRY(hipHostMalloc((void**)&reach_pinned, 9 * sizeof(double), hipHostMallocDefault));
            // FSIPC: the neighbours write straight into these arrays
            HIP_TRY(hipStreamSynchronize(S->stream));
            for (size_t k = 0; k < pool_chunks.size(); ++k)
                if (S->comm.register_buffer(SLOT_POOL + (int)k, pool_chunks[k], pool_chunk_bytes[k], false))
                    return fail(FS_ECOMM, "exporting the field arrays: %s", S->comm.last_error());
            if (S->comm_cus != 0) {
                // a second compute stream whose CU mask leaves CUs to the transport; mask bit i is CU i / 8 of XCD i % 8 (the
                // driver deals the bits round-robin over the XCDs), so clearing the top bits takes the same number from every XCD
                hipDeviceProp_t prop;
                HIP_TRY(hipGetDeviceProperties(&prop, S->device));
                const int ncu = prop.multiProcessorCount;
                int keep_free = S->comm_cus > 0 ? S->comm_cus : 8;
                if (keep_free > ncu / 2) keep_free = ncu / 2;
                std::vector<uint32_t> mask((size_t)(ncu + 31) / 32, 0u);
                for (int i = 0; i < ncu - keep_free; ++i) mask[(size_t)i / 32] |= 1u << (i % 32);
                HIP_TRY(hipExtStreamCreateWithCUMask(&S->stream_masked, (uint32_t)mask.size(), mask.data()));
                S->stream_full = S->stream;
                masked_cus = ncu - keep_free;
                if (S->comm_cus > 0) use_masked_stream(true);      // forced; "auto" decides with the overlap plan
            }
        }
        return FS_OK;
    }

    int masked_cus = 0;
    // switch the compute stream (everything queued on the old one first completes)
    int use_masked_stream(bool on)
    {
        hipStream_t want = on ? S->stream_masked : S->stream_full;
        if (!want || want == S->stream) return FS_OK;
        HIP_TRY(hipStreamSynchronize(S->stream));
        S->resolve_spans();
        S->stream = want;
        S->tune.cu_slots = on ? masked_cus : 256;
        S->cus_plan = on ? (S->comm_cus > 0 ? S->comm_cus : 8) : 0;
        plan_two = -1;                                   // the launch plans depend on how many CUs a launch can fill
        return FS_OK;
    }

    // Device memory frees itself (DevBuf), here and in the parts; what is left is the exported arena chunks, whose peers
    // fs_destroy has unmapped by now (release_buffers), and what is not device memory.
    ~Engine()
    {
        for (T* c : pool_chunks) hipFree(c);
        for (T* c : gather_chunks) hipFree(c);        // the four gathered advection sources
        mg.release();
        for (hipEvent_t ev : { ev_edges, ev_halo, ev_int, ev_c2x, ev_reach[0], ev_reach[1], ev_reach[2], ev_slack })
            if (ev) hipEventDestroy(ev);
        if (reach_pinned) hipHostFree(reach_pinned);
        if (comm_stream) hipStreamDestroy(comm_stream);
    }

    // ---- array pool ------------------------------------------------------------------
    bool referenced(int id) const
    {
        for (int f = 0; f < NSLOT; ++f)
            if (slot[f] == id) return true;
        return held[id];
    }
    int acquire(int not_a = -1, int not_b = -1)
    {
        for (int i = 0; i < npool; ++i)
            if (i != not_a && i != not_b && !referenced(i)) { held[i] = true; return i; }
        return -1;   // cannot happen: NPOOL covers the worst case of a step
    }
    // Scratch of a timing run: up to two pool arrays and an event pair, given back on every path out (error paths too).
    struct Scratch {
        bool* held; int a = -1, b = -1; hipEvent_t e0 = nullptr, e1 = nullptr;
        hipError_t events() { hipError_t e = hipEventCreate(&e0); return e != hipSuccess ? e : hipEventCreate(&e1); }
        ~Scratch() { if (a >= 0) held[a] = false; if (b >= 0) held[b] = false; if (e0) hipEventDestroy(e0); if (e1) hipEventDestroy(e1); }
    };
    // Timed choices: a later candidate has to win by 1.5 %, so that candidates within the noise of each other do not flip from
    // run to run (the chosen launch plan is part of what profiles/sweep_traffic.json is stamped with)
    template <class M>
    static bool beats(M ms, M best) { return ms < best * (M)0.985; }
    bool shared_slot(int f) const
    {
        for (int k = 0; k < NSLOT; ++k)
            if (k != f && slot[k] == slot[f]) return true;
        return false;
    }
    // give field f an array of its own (same contents)
    int unalias(int f)
    {
        if (!shared_slot(f)) return FS_OK;
        int id = acquire();
        if (id < 0) return fail(FS_ENOMEM, "array pool exhausted");
        fs::launch_copy<T>(S->stream, g, arr[slot[f]], arr[id]);
        slot[f] = id;
        held[id] = false;
        return FS_OK;
    }

    // Host-side writes (fs_set_field, fs_add_density, ...) reach only this rank's planes; before
    // the next kernel every rank refreshes the halo copies of all fields (collective).
    int ensure_halos()
    {
        if (!halos_dirty || !S->comm.active()) { halos_dirty = false; return FS_OK; }
        halos_dirty = false;
        bool done[NPOOL_MAX] = {false};
        for (int f = 0; f < FS_NFIELDS; ++f) {
            if (f == FS_OBS || done[slot[f]]) continue;
            done[slot[f]] = true;
            int rc = halo(arr[slot[f]]);
            if (rc) return rc;
        }
        return FS_OK;
    }

    int ensure_flags()
    {
        {
            int rc = ensure_halos();
            if (rc) return rc;
        }
        if (!flags_dirty) return FS_OK;
        int rc = unalias(FS_OBS);
        if (rc) return rc;
        if (S->comm.active() && (rc = halo(arr[slot[FS_OBS]]))) return rc;
        ScopedSpan sp(S, FAM_MISC);
        fs::launch_build_flags<T>(S->stream, g, sc, arr[slot[FS_OBS]], flags);
        fs::launch_build_kill(S->stream, g, sc, flags, kill);
        if ((rc = build_clean())) return rc;
        flags_dirty = false;
        bodies.obs_changed();
        images.obs_changed();
        mg_current = false;
        return FS_OK;
    }

    // The clean table and its host copy (one small device-to-host copy per mask change); the balanced chunk tables made from the
    // old one are dropped
    int build_clean()
    {
        maskplan.clear_chunks();
        if (!std::is_same<T, float>::value || S->comm.active() || g.W > 512) return FS_OK;   // where the three-sweep kernel is fp32 x 3
        const int words = (g.H + 2 + 31) / 32 + 1;
        if (words > 64) return FS_OK;                    // (rows beyond what build_clean_kernel's LDS holds: no mask-free body)
        const size_t n = (size_t)(g.D + 2) * words;
        if (!maskplan.tab) HIP_TRY(hipMalloc((void**)&maskplan.tab, n * sizeof(uint32_t)));
        maskplan.words = words;
        maskplan.host.resize(n);
        fs::launch_build_clean(S->stream, g, kill, maskplan.tab, words);
        HIP_TRY(hipMemcpyAsync(maskplan.host.data(), maskplan.tab, n * sizeof(uint32_t), hipMemcpyDeviceToHost, S->stream));
        HIP_TRY(hipStreamSynchronize(S->stream));
        return FS_OK;
    }

    // Every transport call of a slab rank goes through here: queued on the communication stream behind everything the
    // compute stream holds so far, and the compute stream continues behind it.  One stream per communicator: RCCL orders a
    // communicator's operations by issue order, and two streams sharing one would be serialised in ways the schedule
    // does not show (round-2 verdict).
    // Schedule 0 (a pass, then its exchange) overlaps nothing, so there the one stream is the compute stream itself and no
    // event is needed: a cross-stream dependency costs about 14 us each way on this runtime (measured: 240 passes per step
    // with an event pair each = 6.7 ms of a 26 ms slab step, profiles/r3e_*).
    bool comm_on_compute_stream() const { return S->overlap_plan == 0 || S->overlap_plan == 3; }
    template <class F>
    int comm_op(F&& op, const char* what)
    {
        if (comm_on_compute_stream()) {
            if (op(S->stream)) return fail(FS_ECOMM, "%s failed: %s", what, S->comm.last_error());
            return FS_OK;
        }
        HIP_TRY(hipEventRecord(ev_c2x, S->stream));
        HIP_TRY(hipStreamWaitEvent(comm_stream, ev_c2x, 0));
        if (op(comm_stream)) return fail(FS_ECOMM, "%s failed: %s", what, S->comm.last_error());
        HIP_TRY(hipEventRecord(ev_halo, comm_stream));
        HIP_TRY(hipStreamWaitEvent(S->stream, ev_halo, 0));
        return FS_OK;
    }

    int halo(T* a)
    {
        if (!S->comm.active()) return FS_OK;
        ScopedSpan sp(S, FAM_COMM);
        return comm_op([&](hipStream_t st) { return S->comm.exchange_halo(st, a, g, sizeof(T), S->D, g.zh); }, "halo exchange");
    }

    // ---- linearSolver (simulation.cpp:251-273) -----------------------------------------
    // One pass over memory that applies `levels` (1, 2 or 3) Jacobi sweeps to planes zf..zl (and, with
    // second >= 0, to the equally long range starting there).
    // push: the pass also stores the planes its z neighbours need into their halo planes (plain Jacobi passes, FSIPC)
    void launch_pass(hipStream_t st, int levels, bool rb, const T* src_, const T* rhs_, T* dst_, int b, T a, T inv_c, int zf,
                     int zl, int second = -1, const fs::PeerPush* push = nullptr, bool zero_src = false, bool zrev = false)
    {
        const T omega = rb ? rb_omega : (T)0;
        const bool fused2 = fs::decode_plan(false, plan_two).kind == fs::SweepKernel::Fused2;
        if (levels == 3)
            fs::launch_jacobi_fused<T>(st, S->tune, g, sc, 3, src_, rhs_, dst_, kill, b, a, inv_c, zf, zl, plan_three, second, push,
                                       &maskplan, zero_src, zrev);
        else if (levels == 2 && !rb && fused2)
            fs::launch_jacobi_fused<T>(st, S->tune, g, sc, 2, src_, rhs_, dst_, kill, b, a, inv_c, zf, zl, plan_two, second, push);
        else if (levels == 2)
            fs::launch_jacobi_pair<T>(st, S->tune, g, sc, src_, rhs_, dst_, kill, b, a, inv_c, zf, zl,
                                      fused2 ? plan_two_pair : plan_two, second, omega, rb_damped, push);
        else
            fs::launch_jacobi<T>(st, S->tune, g, sc, src_, rhs_, dst_, kill, b, a, inv_c, zf, zl, second, push);
    }
    // what of this grid and the options the launch plans depend on (launch_plan.h)
    fs::PlanGrid plan_grid() const { return {(int)sizeof(T), g.W, sc.lo_wall && sc.hi_wall, g.zh, S->tune.fuse}; }
    bool has_kernel(fs::SweepKernel k) const { return fs::plan_supported(plan_grid(), k); }
    bool two_sweep_kernels() const { return has_kernel(fs::SweepKernel::Pair) || has_kernel(fs::SweepKernel::Fused2); }
    int ensure_tuned(int cur, int rhs, int b, T a, T inv_c)
    {
        if (two_sweep_kernels() || has_kernel(fs::SweepKernel::Three)) {
            const TunedFor now{S->tune.fuse, S->tune.pair_shape, S->tune.two_kind, S->replay_two, S->replay_three};
            if (!(plan_two >= 0 && tuned_for == now)) {
                tuned_for = now;
                int rc = choose_launch_plans(cur, rhs, b, a, inv_c);
                if (rc) return rc;
            }
        }
        if (S->comm.active() && S->overlap_plan < 0) return choose_overlap(cur, rhs, b, a, inv_c);
        return FS_OK;
    }

    // all ranks have finished everything queued so far (host-blocking; tuning and dumps only)
    int slab_barrier()
    {
        HIP_TRY(hipStreamSynchronize(S->stream));
        if (S->comm.barrier(comm_on_compute_stream() ? S->stream : comm_stream, red.get())) return fail(FS_ECOMM, "barrier: %s", S->comm.last_error());
        return FS_OK;
    }
    // the largest `v` of any rank, the same bits on every rank (host-blocking; tuning only)
    int rank_max(double v, double* out)
    {
        double h[3] = { v, v, v };
        double* d3 = red.get() + 3 * 1024;
        HIP_TRY(hipMemcpyAsync(d3, h, sizeof h, hipMemcpyHostToDevice, S->stream));
        int rc = comm_op([&](hipStream_t st) { return S->comm.reduce_stats(st, d3, g, S->D); }, "all-reduce");
        if (rc) return rc;
        HIP_TRY(hipMemcpyAsync(h, d3, sizeof h, hipMemcpyDeviceToHost, S->stream));
        HIP_TRY(hipStreamSynchronize(S->stream));
        *out = h[2];
        return FS_OK;
    }

    // "overlap" = "auto" (and "comm_cus" = "auto"): the communication schedules are chosen the way launch plans are -- by the
    // clock, once, on the transport the run really uses.  Every candidate runs a chain of the solver's deepest passes with
    // their exchanges between two barriers; what counts is the slowest rank's time (all-reduced, so that every rank takes
    // the same decision: the schedule must not diverge).  A later candidate has to win by a margin (beats).  The bits do not depend on
    // the choice (tests/test_gpu_slabs.py runs every candidate).
    int choose_overlap(int src, int rhs, int b, T a, T inv_c)
    {
        const bool auto_cus = S->comm_cus < 0 && S->stream_masked;
        const bool can2 = two_sweep_kernels(), can3 = plan_three >= 0;
        const int lv = can3 ? 3 : can2 ? 2 : 1;
        std::vector<int> modes;
        if (S->overlap >= 0) modes.push_back(S->overlap);
        else if (g.D < 2 * lv + 8) modes.push_back(0);                 // too thin for a boundary/interior split: one schedule
        else modes = { 1, 0, 2 };
        if (S->overlap < 0 && S->comm.can_push()) modes.push_back(3);   // FSIPC: passes that store into the neighbours' halos
        if (modes.size() == 1 && !auto_cus) {
            S->overlap_plan = modes[0];
            if (S->cus_plan < 0) S->cus_plan = 0;
            return FS_OK;
        }
        const int t0 = acquire(src, rhs), t1 = acquire(src, rhs);
        Scratch rel{held, t0, t1};
        if (t0 < 0 || t1 < 0) return fail(FS_ENOMEM, "array pool exhausted");
        HIP_TRY(rel.events());
        const bool tune_log = getenv("FS_TUNE_LOG") != nullptr;
        const int NP = 6;
        double best = 1e300;
        int best_mode = modes[0], best_mask = 0;
        int rc = FS_OK;
        for (int mask = 0; mask < (auto_cus ? 2 : 1); ++mask) {
            if (auto_cus) {
                if ((rc = use_masked_stream(mask == 1))) return rc;
                if ((rc = choose_launch_plans(src, rhs, b, a, inv_c))) return rc;   // launch plans for that many CUs
            }
            for (int mode : modes) {
                double ms = 0.0;
                HIP_TRY(hipDeviceSynchronize());         // the transport's stream changes with the schedule: nothing may be in flight
                S->overlap_plan = mode;
                for (int rep = 0; rep < 2; ++rep) {          // the second chain is the timed one
                    if ((rc = slab_barrier())) return rc;
                    HIP_TRY(hipEventRecord(rel.e0, S->stream));
                    int from = src;
                    for (int p = 0; p < NP; ++p) {
                        const int to = (p & 1) ? t1 : t0;
                        if ((rc = slab_pass(mode, lv, lv, p == 0, p + 1 == NP, false, arr[from], arr[rhs], arr[to], b, a, inv_c))) return rc;
                        from = to;
                    }
                    HIP_TRY(hipEventRecord(rel.e1, S->stream));
                    HIP_TRY(hipEventSynchronize(rel.e1));
                    float t = 0;
                    HIP_TRY(hipEventElapsedTime(&t, rel.e0, rel.e1));
                    ms = (double)t / NP;
                }
                double worst = ms;
                if ((rc = rank_max(ms, &worst))) return rc;
                S->overlap_ms[4 * mask + mode] = worst;
                if (tune_log)
                    fprintf(stderr, "fluidsim tune: rank %d overlap=%d cu mask %s: %.4f ms per pass here, %.4f on the slowest rank\n",
                            S->comm.rank, mode, mask ? "on" : "off", ms, worst);
                if (beats(worst, best)) { best = worst; best_mode = mode; best_mask = mask; }
            }
        }
        if (auto_cus) {
            if ((rc = use_masked_stream(best_mask == 1))) return rc;
            if ((rc = choose_launch_plans(src, rhs, b, a, inv_c))) return rc;
        }
        if (S->cus_plan < 0) S->cus_plan = 0;
        HIP_TRY(hipDeviceSynchronize());
        S->overlap_plan = best_mode;
        if (S->comm.rank == 0 && !S->quiet)
            fprintf(stderr, "fluidsim: communication schedule overlap=%d, %d CUs kept free (timed: slowest rank %.3f ms per %d-sweep pass)\n",
                    best_mode, S->cus_plan, best, lv);
        return FS_OK;
    }

    // A solve in progress: the list of its passes and where it stands.  step() interleaves the (dead) density solve of
    // a slab run with the velocity advection, so a solve can be paused between two passes.
    struct SolveRun {
        std::vector<int> plan;       // levels of each pass
        int next = 0;                // first pass not yet launched
        int b = 0, rhs = -1, src = -1;
        bool src_temp = false, rb = false, damped = false;
        bool zero_src = false;       // the initial iterate is all zeros and its array is not read (zero_start_ok)
        bool prev_up = false;        // the previous pass of this solve marched upward in z (none yet: false)
        T a = (T)0, inv_c = (T)1, omega = (T)1;
    };

    // One pass of a slab rank and the exchange of its boundary planes: `e` planes per side go to the neighbours (what their
    // next pass needs).  `first` / `last`: first / last pass of a run of passes queued back to back (the two-stream
    // schedule chains its events from pass to pass).
    int slab_pass(int mode, int lv, int e, bool first, bool last, bool rb, const T* src, const T* rhs, T* dst, int b, T a, T inv_c)
    {
        auto exchange = [&](hipStream_t st) { return S->comm.exchange_halo(st, dst, g, sizeof(T), S->D, e); };
        if (mode == 3 && !rb && S->comm.can_push()) {
            // Push (FSIPC): the pass stores the `e` outermost planes per side straight into the neighbours' halo planes; a
            // handshake on the same stream ("my pass is complete" both ways) is all that separates it from the next
            // pass -- no boundary launch, no copy, no second stream, no event.  The neighbour's halo of this array is
            // free: its last reader there was the neighbour's previous pass, which the previous handshake covered.
            fs::PeerPush pp;
            if (S->comm.peer_push(dst, g, sizeof(T), e, &pp)) return fail(FS_ECOMM, "push exchange: %s", S->comm.last_error());
            launch_pass(S->stream, lv, false, src, rhs, dst, b, a, inv_c, 1, g.D, -1, &pp);
            if (S->comm.handshake(S->stream)) return fail(FS_ECOMM, "handshake: %s", S->comm.last_error());
            return FS_OK;
        }
        if (mode == 3) mode = 0;                          // a pass the push kernels do not cover (red-black): pass, then copy exchange
        if (g.D < 2 * e + 8) mode = 0;                    // too thin to split into boundary and interior
        const int in_lo = sc.lo_wall ? 1 : e + 1, in_hi = sc.hi_wall ? g.D : g.D - e;
        auto boundary = [&](hipStream_t st) {
            if (!sc.lo_wall && !sc.hi_wall) launch_pass(st, lv, rb, src, rhs, dst, b, a, inv_c, 1, e, g.D - e + 1);
            else if (!sc.lo_wall) launch_pass(st, lv, rb, src, rhs, dst, b, a, inv_c, 1, e);
            else if (!sc.hi_wall) launch_pass(st, lv, rb, src, rhs, dst, b, a, inv_c, g.D - e + 1, g.D);
        };
        if (mode == 2) {
            // Two streams: the boundary regions of pass k and its interior only depend on pass k-1, not on each other, so
            // they are queued side by side -- boundary launch + exchange on the communication stream, interior on the
            // compute stream.  Interior k reads the halo planes that exchange k-1 fills (a pass of lv levels reads lv
            // planes beyond its range) and overwrites what boundary k-1 read: it waits for the event behind exchange k-1
            // (round-2 advice: waiting for boundary k-1 alone was a race whenever a pass had more levels than the next).
            if (first) HIP_TRY(hipEventRecord(ev_int, S->stream));                 // everything queued so far
            else HIP_TRY(hipStreamWaitEvent(S->stream, ev_halo, 0));               // boundary k-1 and exchange k-1
            HIP_TRY(hipStreamWaitEvent(comm_stream, ev_int, 0));                   // boundary k reads interior k-1
            boundary(comm_stream);
            launch_pass(S->stream, lv, rb, src, rhs, dst, b, a, inv_c, in_lo, in_hi);
            HIP_TRY(hipEventRecord(ev_int, S->stream));
            if (exchange(comm_stream)) return fail(FS_ECOMM, "halo exchange failed: %s", S->comm.last_error());
            HIP_TRY(hipEventRecord(ev_halo, comm_stream));
            if (last) HIP_TRY(hipStreamWaitEvent(S->stream, ev_halo, 0));          // whoever reads the result next runs on the compute stream
        } else if (mode == 1) {
            // Boundary planes first (both regions in one launch); their exchange travels on the communication stream
            // while the interior planes are computed; the next launch waits for it.
            boundary(S->stream);
            HIP_TRY(hipEventRecord(ev_edges, S->stream));
            launch_pass(S->stream, lv, rb, src, rhs, dst, b, a, inv_c, in_lo, in_hi);
            HIP_TRY(hipStreamWaitEvent(comm_stream, ev_edges, 0));
            if (exchange(comm_stream)) return fail(FS_ECOMM, "halo exchange failed: %s", S->comm.last_error());
            HIP_TRY(hipEventRecord(ev_halo, comm_stream));
            HIP_TRY(hipStreamWaitEvent(S->stream, ev_halo, 0));
        } else {
            launch_pass(S->stream, lv, rb, src, rhs, dst, b, a, inv_c, 1, g.D);
            return comm_op(exchange, "halo exchange");   // schedule 0: on the compute stream; a thin slab of schedule 1 / 2: through the events
        }
        return FS_OK;
    }

    // `cur` holds the initial iterate (may equal rhs when the caller aliased a snapshot).
    // smoother = true: `sweeps` passes of two 6/7-damped Jacobi sweeps each (the level-0 smoothing step of solver=mg)
    int solve_begin(SolveRun& r, int b, int cur, int rhs, T a, T c, int sweeps, bool smoother = false, bool zero_src = false)
    {
        r = SolveRun();
        r.zero_src = zero_src;
        r.b = b; r.rhs = rhs; r.src = cur; r.a = a;
        r.inv_c = (T)1 / c;                              // cRecip, :257
        // solver=rbsor: every iteration is one pass of the pair kernel (its two levels are the two colours)
        r.rb = smoother || (S->solver == FS_SOLVER_RBSOR);
        r.omega = smoother ? (T)6 / (T)7 : (T)S->omega;
        r.damped = smoother;
        if (r.rb && !has_kernel(fs::SweepKernel::Pair))
            return fail(FS_EINVAL, "solver=rbsor / mg needs rows of at most 1024 cells and sweep_fuse >= 2");
        int rc = ensure_tuned(cur, rhs, b, a, r.inv_c);
        if (rc) return rc;
        // The passes of this solve: three sweeps per pass while at least three remain (where that kernel
        // exists and was found faster), then two, then one.  Under z-slabs every rank derives the same list
        // (it fixes the depth of every halo exchange).
        const bool can2 = two_sweep_kernels(), can3 = plan_three >= 0;
        for (int left = sweeps; left > 0;) {
            if (r.rb) { r.plan.push_back(2); left -= 1; continue; }      // an rbsor iteration runs as a two-level pass
            const int lv = (can3 && left >= 3) ? 3 : (can2 && left >= 2) ? 2 : 1;
            r.plan.push_back(lv);
            left -= lv;
        }
        const int npass = (int)r.plan.size();
        if (r.zero_src && !(npass > 0 && r.plan[0] == 3 && !r.rb && !S->comm.active() &&
                            fs::jacobi_fused_zero_start(S->tune, g, sc, (int)sizeof(T), plan_three)))
            return fail(FS_EINVAL, "zero start: the first pass of this solve has no zero-start kernel");   // zero_start_ok promised it
        if (npass > 0 && S->comm.active() && (r.plan[0] > 1 || npass > 1)) {
            // a fused pass recomputes the lower levels of the neighbours' boundary planes: it reads the
            // right-hand side there, so its halo planes must be current
            if ((rc = halo(arr[rhs]))) return rc;
        } else if (npass > 0 && S->overlap_plan == 3 && S->comm.can_push()) {
            // push schedule: the first pass writes into the neighbours' arrays, so whatever they queued before this solve
            // has to be complete (the exchange above is such a handshake; without it, one is issued)
            if (S->comm.handshake(S->stream)) return fail(FS_ECOMM, "handshake: %s", S->comm.last_error());
        }
        return FS_OK;
    }

    // launch passes next .. upto-1
    int solve_passes(SolveRun& r, int upto)
    {
        const int npass = (int)r.plan.size();
        if (upto > npass) upto = npass;
        if (r.next >= upto) return FS_OK;
        rb_omega = r.omega;
        rb_damped = r.damped;
        int span = -1, span_fam = -1;
        long span_launches = 0;
        auto close_span = [&]() {
            if (span >= 0) S->span_end(span, span_launches);
            span = -1;
            span_launches = 0;
        };
        const int first = r.next;
        for (int i = first; i < upto; ++i) {
            const int lv = r.plan[i];
            int dst = acquire(r.src, r.rhs);
            if (dst < 0) return fail(FS_ENOMEM, "array pool exhausted");
            // one event pair around each run of equal passes (an event pair per launch costs 2 % at 512^3 and
            // 16 % at 256^3); launches are counted so that time / launches is the mean launch time.  On slabs
            // the exchanges fall inside the span.
            const int fam = lv == 3 ? FAM_TRIPLE : lv == 2 ? FAM_PAIR : FAM_SWEEP;
            if (span >= 0 && fam != span_fam) close_span();
            if (span < 0) { span = S->span_begin(fam); span_fam = fam; }
            ++span_launches;
            if (!S->comm.active()) {
                // a three-sweep pass behind an upward pass of the same solve marches downward where such a build exists: it
                // starts on the planes the pass before it read and wrote last
                const bool zero = r.zero_src && i == 0;
                const bool zrev = lv == 3 && r.prev_up && !zero && !r.rb && z_alternate_ok();
                launch_pass(S->stream, lv, r.rb, arr[r.src], arr[r.rhs], arr[dst], r.b, r.a, r.inv_c, 1, g.D, -1, nullptr, zero, zrev);
                r.prev_up = !zrev;
                if (zrev) ++S->n_reversed;
            } else {
                // planes a neighbour needs of this pass's result: as many as its next pass has levels; after
                // the last pass the halos are brought to their full depth (what every other kernel assumes)
                const int e = (i + 1 < npass) ? r.plan[i + 1] : g.zh;
                int rc = slab_pass(S->overlap_plan, lv, e, i == first, i + 1 == upto, r.rb, arr[r.src], arr[r.rhs], arr[dst], r.b, r.a,
                                   r.inv_c);
                if (rc) { held[dst] = false; return rc; }
            }
            if (r.src_temp) held[r.src] = false;
            r.src = dst;
            r.src_temp = true;
        }
        close_span();
        r.next = upto;
        return FS_OK;
    }

    // the id of the array holding the result (held)
    int solve_end(SolveRun& r, int* result)
    {
        int rc = solve_passes(r, (int)r.plan.size());
        if (rc) return rc;
        if (!r.src_temp) held[r.src] = true;
        *result = r.src;
        return FS_OK;
    }

    int solve(int b, int cur, int rhs, T a, T c, int sweeps, int* result, bool smoother = false, bool zero_src = false)
    {
        if (S->solver == FS_SOLVER_GS_LEX) {
            if (S->comm.active()) return fail(FS_EINVAL, "gs_lex is a single-GPU verification mode");
            if (cur == rhs) return fail(FS_EINVAL, "gs_lex needs distinct field and prev arrays");
            ScopedSpan sp(S, FAM_SWEEP, sweeps);
            if (sweeps > 0) fs::launch_gs_lex<T>(S->stream, g, arr[cur], arr[rhs], flags, b, a, (T)1 / c, sweeps);
            held[cur] = true;
            *result = cur;
            return FS_OK;
        }
        SolveRun r;
        int rc = solve_begin(r, b, cur, rhs, a, c, sweeps, smoother, zero_src);
        if (rc) return rc;
        return solve_end(r, result);
    }

    // Times the candidate launch plans of the two-sweep kernels on this grid (launch_plan.h: the pair kernel's workgroup
    // shapes and the fused kernel's, each x the three best z-chunk counts of the launcher's model) -- two launches each
    // into a scratch array, the second one timed -- and keeps the fastest; then the same for the three-sweep kernel,
    // which is used where a sweep costs less that way.  Every plan computes the same bits, so this only ever changes speed.
    int choose_launch_plans(int src, int rhs, int b, T a, T inv_c)
    {
        plan_two = 0;
        plan_two_pair = 0;
        plan_three = -1;
        const fs::PlanGrid G = plan_grid();
        // "launch_plans" = "<two-sweep id>,<three-sweep id>" (as fs_get_int "pair_shape" / "triple_plan" report them): replay
        // the plans of another run instead of timing (tools/make_profiles.sh: the counter passes must run the plans the
        // bench line ran, and the clock is different under counter collection); -1 = time as usual / no such kernel.
        if (S->replay_two >= -1 && S->replay_three >= -1 && (S->replay_two >= 0 || S->replay_three >= 0)) {
            const fs::Replay two = fs::check_replay(G, false, S->replay_two), three = fs::check_replay(G, true, S->replay_three);
            const bool fused2 = fs::decode_plan(false, S->replay_two).kind == fs::SweepKernel::Fused2;
            if (two == fs::Replay::Refuse)
                return fail(FS_EINVAL, "launch_plans: two-sweep plan %d names a %s-kernel shape this grid does not have", S->replay_two,
                            fused2 ? "fused" : "pair");
            if (three == fs::Replay::Refuse)
                return fail(FS_EINVAL, "launch_plans: three-sweep plan %d names a shape this grid does not have", S->replay_three);
            if (two == fs::Replay::Use) plan_two = S->replay_two;
            if (!fused2) plan_two_pair = plan_two;
            if (three == fs::Replay::Use) plan_three = S->replay_three;
            return FS_OK;
        }
        Scratch rel{held, acquire(src, rhs)};
        const int tmp = rel.a;
        if (tmp < 0) return fail(FS_ENOMEM, "array pool exhausted");
        if (src == rhs) {
            // the first solve of a step reads iterate and right-hand side from ONE array (the snapshot alias): a
            // third less HBM traffic than every later pass, which would rank the candidates for the wrong regime
            rel.b = acquire(src, tmp);
            if (rel.b < 0) return fail(FS_ENOMEM, "array pool exhausted");
            fs::launch_copy<T>(S->stream, g, arr[src], arr[rel.b]);
            rhs = rel.b;
        }
        HIP_TRY(rel.events());
        hipEvent_t e0 = rel.e0, e1 = rel.e1;
        const bool tune_log = getenv("FS_TUNE_LOG") != nullptr;   // development: print every candidate's time
        auto timed = [&](int levels, int cand, float* ms) -> int {
            int& plan = levels == 3 ? plan_three : plan_two;
            const int keep = plan;
            plan = cand;
            int rc = FS_OK;
            for (int rep = 0; rep < 2 && !rc; ++rep) {
                if (hipEventRecord(e0, S->stream) != hipSuccess) { rc = fail(FS_EHIP, "hipEventRecord"); break; }
                launch_pass(S->stream, levels, false, arr[src], arr[rhs], arr[tmp], b, a, inv_c, 1, g.D);
                if (hipEventRecord(e1, S->stream) != hipSuccess || hipEventSynchronize(e1) != hipSuccess ||
                    hipEventElapsedTime(ms, e0, e1) != hipSuccess)
                    rc = fail(FS_EHIP, "timing a sweep launch plan failed: %s", hipGetErrorString(hipGetLastError()));
            }
            plan = keep;
            if (tune_log && !rc)
                fprintf(stderr, "fluidsim tune: %dx%dx%d %s levels=%d plan=%d  %.4f ms per pass\n", g.W, g.H, g.D,
                        sizeof(T) == 8 ? "fp64" : "fp32", levels, cand, *ms);
            return rc;
        };
        // the fastest two-sweep plan overall, the fastest of the pair kernel alone, the fastest three-sweep plan
        float best2 = 1e30f, best2_pair = 1e30f, best3 = 1e30f;
        int cand2 = -1, cand3 = -1, rc = FS_OK;
        auto time_all = [&](int levels, const std::vector<int>& cands, float& best, int& pick) {
            for (size_t i = 0; i < cands.size() && !rc; ++i) {
                float ms = 1e30f;
                if ((rc = timed(levels, cands[i], &ms))) return;
                if (beats(ms, best)) { best = ms; pick = cands[i]; }
                if (levels == 2 && fs::decode_plan(false, cands[i]).kind == fs::SweepKernel::Pair && beats(ms, best2_pair)) {
                    best2_pair = ms;
                    plan_two_pair = cands[i];
                }
            }
        };
        time_all(2, fs::two_sweep_candidates(G, S->tune.pair_shape, S->tune.two_kind), best2, cand2);
        if (cand2 >= 0) plan_two = cand2;
        // three sweeps per pass, where the kernel exists for this grid: keep it if a sweep costs less
        if (!rc) time_all(3, fs::kernel_candidates(G, fs::SweepKernel::Three), best3, cand3);
        if (rc) return rc;
        // fuse 4 forces it (tests, tuning); z-slab ranks must all take the same decision (it fixes the
        // exchange schedule), so there it is not left to each rank's clock
        if (S->tune.fuse >= 4 || S->comm.active() || cand2 < 0 || best3 / 3.0f < best2 / 2.0f) plan_three = cand3;
        return FS_OK;
    }

    // assign the result of a solve to a field slot
    void adopt(int field, int id)
    {
        slot[field] = id;
        held[id] = false;
    }

    T diffusion_a() const
    {
        // simulation.cpp:282: dt * diff * width * height * depth, left to right
        return (T)S->dt * (T)S->diff * (T)S->W * (T)S->H * (T)S->D;
    }

    int linear_solver(int b, int field, int prev, float a, float c)
    {
        if (!in_step) vzmax_prev = -1.0;             // a call from outside step(): what is known about v_z is void
        int rc = ensure_flags();
        if (rc) return rc;
        if (S->solver == FS_SOLVER_GS_LEX && (rc = unalias(field))) return rc;
        int res;
        if (S->solver == FS_SOLVER_MG && b == 0 && a == 1.0f && c == 6.0f) {
            // the pressure equation's coefficients (:320): V-cycles; every other system (diffusion) is relaxed as under jacobi
            if ((rc = unalias(field)) || (rc = unalias(prev))) return rc;
            rc = multigrid_solve(field, prev, &res);
        } else {
            rc = solve(b, slot[field], slot[prev], (T)a, (T)c, S->acc, &res);
        }
        if (rc) return rc;
        adopt(field, res);
        return FS_OK;
    }

    // log_k >= 0 (inside step() with "residual_log" on): solve k of the step, recorded before and after
    int diffuse_T(int b, int field, int prev, int log_k = -1)
    {
        const T a = diffusion_a();
        int rc = ensure_flags();
        if (rc) return rc;
        if (S->solver == FS_SOLVER_GS_LEX && (rc = unalias(field))) return rc;
        const T c = (T)1 + (T)6 * a;
        if ((rc = residual.log(log_k, 0, b, slot[field], slot[prev], (double)a, (double)c))) return rc;
        int res;
        rc = solve(b, slot[field], slot[prev], a, c, S->acc, &res);   // :283
        if (rc) return rc;
        adopt(field, res);
        return residual.log(log_k, 1, b, slot[field], slot[prev], (double)a, (double)c);
    }
    int diffuse(int b, int field, int prev) { if (!in_step) vzmax_prev = -1.0; return diffuse_T(b, field, prev); }

    int set_bounds(int b, int field)
    {
        if (!in_step) vzmax_prev = -1.0;             // a call from outside step(): what is known about v_z is void
        int rc = ensure_flags();
        if (rc) return rc;
        if ((rc = unalias(field))) return rc;
        ScopedSpan sp(S, FAM_BOUNDS, 2);
        fs::launch_set_bounds<T>(S->stream, g, sc, arr[slot[field]], flags, b);
        return halo(arr[slot[field]]);
    }

    // solver=mg (NOT the reference's arithmetic; defined in oracle/cpu_ref_mg.h): mg_cycles V-cycles on the pressure
    // equation of :320.  Level 0 is smoothed by the reference's update as damped Jacobi sweeps, two per pass of the pair
    // kernel (its red-black instantiation is 1.6x slower and smooths no better here), the coarse levels live in
    // multigrid.hip.  Single GPU.
    int multigrid_levels() const { return mg.levels(); }
    int multigrid_first_replicated() const { return mg.first_repl; }
    // the transport's part in the coarse levels of a slab run (multigrid.h): one-plane halo refreshes of distributed levels,
    // all-gathers at the seam to the levels every rank holds whole
    fs::MgHooks<T> mg_hooks()
    {
        fs::MgHooks<T> h;
        h.halo = [this](const fs::MgLevel<T>& l, T* a) -> int {
            fs::GridDesc lg = g;
            lg.sz = l.sz; lg.sy = l.sy; lg.D = l.D; lg.W = l.W; lg.H = l.H;
            return comm_op([&](hipStream_t st) { return S->comm.exchange_halo(st, a, lg, sizeof(T), l.D * S->comm.nranks, 1); },
                           "halo exchange of a multigrid level");
        };
        h.gather = [this](const fs::MgLevel<T>& l, T* a, int dl, int zoff) -> int {
            fs::GridDesc lg = g;
            lg.sz = l.sz; lg.sy = l.sy; lg.D = dl; lg.W = l.W; lg.H = l.H;
            return comm_op([&](hipStream_t st) { return S->comm.all_gather_planes(st, a + (long)zoff * l.sz, a, lg, l.D, sizeof(T)); },
                           "all-gather of a multigrid level");
        };
        return h;
    }
    int multigrid_solve(int field, int prev, int* result)
    {
        if (S->mg_cycles > 0 && !has_kernel(fs::SweepKernel::Pair))
            return fail(FS_EINVAL, "solver=mg needs rows of at most 1024 cells and sweep_fuse >= 2");
        const bool slabs = S->comm.active();
        fs::MgHooks<T> hooks;
        if (slabs) hooks = mg_hooks();
        if (!mg_current) {
            ScopedSpan sp(S, FAM_MG);
            int brc = mg.build(S->stream, g, sc, flags, slabs ? S->comm.nranks : 1, slabs ? S->comm.rank : 0, S->mg_min_planes,
                               slabs ? &hooks : nullptr);
            if (brc == -1) {
                // a fresh allocation on a slab rank: the neighbours (halo planes) and, at the seam, all ranks write into it
                if (S->comm.register_buffer(SLOT_MG, mg.pool, mg.pool_elems * sizeof(T), true))
                    return fail(FS_ECOMM, "exporting the multigrid levels: %s", S->comm.last_error());
                brc = mg.build(S->stream, g, sc, flags, S->comm.nranks, S->comm.rank, S->mg_min_planes, &hooks);
            }
            if (brc == 2) return fail(FS_EINVAL, "solver=mg on z-slabs needs an even number of planes per rank (%d)", g.D);
            if (brc == 3) return FS_ECOMM;               // the hook has set the message
            if (brc) return fail(FS_EHIP, "multigrid levels: %s", hipGetErrorString(hipGetLastError()));
            mg_current = true;
        }
        const int own = slot[field], rhs = slot[prev];
        if (own == rhs) return fail(FS_EINVAL, "solver=mg needs distinct field and prev arrays");
        int cur = own;
        auto smooth = [&](int n) -> int {
            if (n <= 0) return FS_OK;
            int res;
            int rc = solve(0, cur, rhs, (T)1, (T)6, n, &res, true);
            if (rc) return rc;
            if (cur != own && cur != res) held[cur] = false;
            cur = res;
            return FS_OK;
        };
        for (int cyc = 0; cyc < S->mg_cycles; ++cyc) {
            int rc;
            if (mg.levels() < 2) {                           // a grid that cannot be halved: the "coarsest level" is level 0
                if ((rc = smooth(S->mg_coarse))) return rc;
                continue;
            }
            if ((rc = smooth(S->mg_pre))) return rc;
            {
                ScopedSpan sp(S, FAM_MG);
                const int crc = mg.coarse_correction(S->stream, g, sc, flags, arr[cur], arr[rhs], S->mg_pre, S->mg_post, S->mg_coarse,
                                                     slabs ? &hooks : nullptr);
                if (crc == 3) return FS_ECOMM;
                if (crc) return fail(FS_EHIP, "multigrid cycle: %s", hipGetErrorString(hipGetLastError()));
            }
            // the correction changed this rank's planes of p: the neighbours' copies of its boundary planes are stale
            if (slabs && (rc = halo(arr[cur]))) return rc;
            if ((rc = smooth(S->mg_post))) return rc;
        }
        if (cur == own) held[own] = true;                 // adopt() releases it again
        *result = cur;
        return FS_OK;
    }

    // ---- project (simulation.cpp:289-362) ----------------------------------------------
    // fs_set_int "z_alternate": may a three-sweep pass of a solve march downward?  Where the launch has the reversed build; "auto" asks
    // also that the three arrays of a pass outgrow the Infinity Cache.
    bool z_alternate_ok() const
    {
        if (S->z_alternate == 0 || S->comm.active() || plan_three < 0) return false;
        if (S->z_alternate < 0 && !(Z_ALTERNATE_AUTO && 3 * (size_t)g.n * sizeof(T) > INFINITY_CACHE_BYTES)) return false;
        return fs::jacobi_fused_reversed(S->tune, g, sc, (int)sizeof(T), plan_three);
    }

    // "zero_start": may this projection leave p unzeroed in memory and start its solve from zeros that are not read?  Only
    // where the solve is `acc` >= 3 Jacobi sweeps whose first pass is the three-sweep kernel in a build that has the zero-start
    // form, the launch plans are already chosen (timing them reads the iterate), there are no slabs (the halo exchange of p
    // carries the zeros) and nothing reads p before the solve (the residual log's "before" record).
    bool zero_start_ok(int log_k) const
    {
        if (!(S->zero_start < 0 ? ZERO_START_AUTO : S->zero_start != 0) || S->solver != FS_SOLVER_JACOBI || S->acc < 3 || S->comm.active()) return false;
        if (log_k >= 0 && residual.on()) return false;
        const TunedFor now{S->tune.fuse, S->tune.pair_shape, S->tune.two_kind, S->replay_two, S->replay_three};
        if (!(plan_two >= 0 && tuned_for == now) || plan_three < 0) return false;
        return fs::jacobi_fused_zero_start(S->tune, g, sc, (int)sizeof(T), plan_three);
    }

    int project() { return project_T(false); }
    // defer_gradient (step(), "fuse_project_advect"): everything but the gradient pass -- v stays as it was before the
    // projection and FS_PRESSURE holds the solved pressure; the caller's next launch applies the gradient itself
    int project_T(bool defer_gradient)
    {
        if (!in_step) vzmax_prev = -1.0;             // a call from outside step(): what is known about v_z is void
        int rc = ensure_flags();
        if (rc) return rc;
        for (int f : { FS_VX, FS_VY, FS_VZ, FS_PRESSURE, FS_DIVERGENCE })
            if ((rc = unalias(f))) return rc;
        const T h = (T)1 / host_cbrt<T>((T)(S->W * S->H * S->D));   // :295 (int product, like the reference)
        const int proj = in_step ? projections_this_step++ : -1;   // which of the step's two projections this is
        const int log_k = (proj >= 0 && proj < 2) ? 3 + proj : -1;
        const bool zero_start = zero_start_ok(log_k);
        if (zero_start) ++S->n_zero_start;
        {
            ScopedSpan sp(S, FAM_DIV);
            fs::launch_divergence<T>(S->stream, S->tune, g, sc, arr[slot[FS_VX]], arr[slot[FS_VY]], arr[slot[FS_VZ]],
                                     arr[slot[FS_DIVERGENCE]], arr[slot[FS_PRESSURE]], flags, (T)(-0.5) * h, !zero_start);
        }
        // divergence of the neighbouring slabs' boundary planes is never read (the solve only reads
        // rhs at the cell itself); the pressure halo planes still hold the previous projection and
        // must become the neighbours' freshly zeroed planes before the first sweep reads them.
        if ((rc = halo(arr[slot[FS_PRESSURE]]))) return rc;
        if ((rc = residual.log(log_k, 0, 0, slot[FS_PRESSURE], slot[FS_DIVERGENCE], 1.0, 6.0))) return rc;
        int res;
        if (S->solver == FS_SOLVER_MG) rc = multigrid_solve(FS_PRESSURE, FS_DIVERGENCE, &res);
        else rc = solve(0, slot[FS_PRESSURE], slot[FS_DIVERGENCE], (T)1, (T)6, S->acc, &res, false, zero_start);   // :320
        if (rc) return rc;
        adopt(FS_PRESSURE, res);
        if ((rc = residual.log(log_k, 1, 0, slot[FS_PRESSURE], slot[FS_DIVERGENCE], 1.0, 6.0))) return rc;
        if (!defer_gradient) {
            ScopedSpan sp(S, FAM_GRAD);
            fs::launch_gradient<T>(S->stream, S->tune, g, sc, arr[slot[FS_PRESSURE]], arr[slot[FS_VX]], arr[slot[FS_VY]],
                                   arr[slot[FS_VZ]], flags, h, (T)2 * h);
        }
        if (proj >= 0 && proj < 2) {                  // "force_log", "body_force_log": this projection's records
            forces.record(proj);
            bodies.record(proj);
        }
        // the next consumer of v's z-halo planes is the divergence of the second projection
        // (v_z[z+-1]) and the advection back-trace; refresh them now.
        for (int f : { FS_VX, FS_VY, FS_VZ })
            if ((rc = halo(arr[slot[f]]))) return rc;
        if (proj >= 0 && S->comm.active() && (rc = post_vzmax(proj))) return rc;
        return FS_OK;
    }

    // ---- reach of the back-trace on a slab, without stalling the device ----------------------------------------
    // Inside step() the z velocity that carries each advection is known: after the first projection for v_x / v_y,
    // v_z_prev (= the end of the previous step) for v_z, after the second projection for the density.  Its global
    // max |.| is queued right behind the projection -- device reduction, all-reduce, copy into pinned memory, an event
    // -- and step() puts half of the density solve (independent work) between that and the gather that needs it.
    int projections_this_step = 0;
    int post_vzmax(int which)
    {
        if (which < 0 || which > 2) return FS_OK;
        ScopedSpan sp(S, FAM_COMM);
        double* out3 = red.get() + 3 * 1024 + 3 * (2 + which);
        const int zlo = sc.lo_wall ? 0 : 1, zhi = sc.hi_wall ? g.D + 1 : g.D;
        fs::launch_stats<T>(S->stream, g, arr[slot[FS_VZ]], out3, red.get(), 3 * 1024, zlo, zhi);
        int rc = comm_op([&](hipStream_t st) { return S->comm.reduce_stats(st, out3, g, S->D); }, "all-reduce of max |v_z|");
        if (rc) return rc;
        HIP_TRY(hipMemcpyAsync(reach_pinned + 3 * which, out3, 3 * sizeof(double), hipMemcpyDeviceToHost, S->stream));
        HIP_TRY(hipEventRecord(ev_reach[which], S->stream));
        reach_posted[which] = true;
        return FS_OK;
    }
    // max |v_z| posted by post_vzmax(which); false if nothing was posted (caller falls back to trace_reach)
    bool take_vzmax(int which, double* umax)
    {
        if (!reach_posted[which]) return false;
        ++S->n_reach_waits;
        if (hipEventQuery(ev_reach[which]) != hipSuccess) {
            ++S->n_reach_blocked;
            const auto t0 = std::chrono::steady_clock::now();
            if (hipEventSynchronize(ev_reach[which]) != hipSuccess) return false;
            S->reach_wait_ms += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        }
        const double* st = reach_pinned + 3 * which;
        *umax = std::fmax(std::fabs(st[1]), std::fabs(st[2]));
        return true;
    }
    // max |v_z_prev| of the running step: carried over from the previous step, or posted at the start of this one
    bool prev_vzmax_known(double* umax)
    {
        if (vzmax_prev < 0.0 && !take_vzmax(2, &vzmax_prev)) return false;
        *umax = vzmax_prev;
        return true;
    }
    int reach_of(double umax) const
    {
        const double planes = std::ceil(std::fabs((double)S->dt * (double)S->D) * umax) + 2.0;
        return planes >= (double)S->D ? S->D : (int)planes;
    }

    // ---- advect (simulation.cpp:367-424) ------------------------------------------------
    int advect(int b, int field, int prev)
    {
        if (!in_step) vzmax_prev = -1.0;             // a call from outside step(): what is known about v_z is void
        int rc = ensure_flags();
        if (rc) return rc;
        if (slot[field] == slot[prev]) {
            // in-place transport would read its own output: give the field a fresh array
            int id = acquire();
            if (id < 0) return fail(FS_ENOMEM, "array pool exhausted");
            adopt(field, id);
        }
        for (int f : { FS_VX, FS_VY, FS_VZ })
            if (f != field && slot[f] == slot[field]) return fail(FS_EINVAL, "advect target aliases a velocity array");
        const T kx = (T)S->dt * (T)S->W, ky = (T)S->dt * (T)S->H, kz = (T)S->dt * (T)S->D;   // :384-386
        const T* src = arr[slot[prev]];
        long zshift = 0;
        if (S->comm.active()) {
            // The back-trace may leave the slab by dt*D*|u_z| planes.  Bound it: the
            // carrying z velocity is `prev` for b == 3 and the current v_z otherwise
            // (simulation.cpp:382); its global max |.| gives the reach in planes, and only planes
            // within that reach of the slab are fetched from their owners.
            ScopedSpan sp(S, FAM_COMM);
            int reach = 0;
            double umax = -1.0;
            // inside step(): v_x / v_y are carried by v_z after the first projection, the density by v_z after the second,
            // v_z by v_z_prev (the end of the previous step, where known)
            const bool known = in_step && (b == 3 ? prev_vzmax_known(&umax) : take_vzmax(b == 0 ? 1 : 0, &umax));
            if (known && b == 0) vzmax_end = umax;       // v_z does not change any more in this step: next step's v_z_prev
            if (known) S->last_reach = reach = reach_of(umax);
            else if ((rc = trace_reach({ b == 3 ? prev : FS_VZ }, &reach))) return rc;
            if ((rc = gather_source(src, &gathered, reach, 0))) return rc;
            src = gathered;
            zshift = (long)sc.zoff * g.sz;
        }
        {
            ScopedSpan sp(S, FAM_ADVECT);
            fs::launch_advect<T>(S->stream, S->tune, g, sc, b, arr[slot[field]], src, arr[slot[FS_VX]], arr[slot[FS_VY]],
                                 arr[slot[FS_VZ]], flags, kill, coltab.get(), kx, ky, kz, zshift);
        }
        return halo(arr[slot[field]]);
    }

    // Reach, in planes, of any back-trace whose carrying z velocity is one of `fields`: global
    // max |u_z| over them (device reduction + all-reduce), times dt*D, plus the floor()/corner margin.
    int trace_reach(std::initializer_list<int> fields, int* reach)
    {
        // every field's reduction and all-reduce is queued first; ONE copy and ONE host synchronisation fetch them all
        // (the window sizes are arguments of host-side send/recv calls, so the host has to know the reach)
        double st[4][3];
        int k = 0;
        for (int f : fields) {
            if (k >= 4) break;
            double* out3 = red.get() + 3 * 1024 + 3 * k;
            const int zlo = sc.lo_wall ? 0 : 1, zhi = sc.hi_wall ? g.D + 1 : g.D;
            fs::launch_stats<T>(S->stream, g, arr[slot[f]], out3, red.get(), 3 * 1024, zlo, zhi);
            if (S->comm.active()) {
                int rc = comm_op([&](hipStream_t cs) { return S->comm.reduce_stats(cs, out3, g, S->D); }, "stats all-reduce");
                if (rc) return rc;
            }
            ++k;
        }
        HIP_TRY(hipMemcpyAsync(&st[0][0], red.get() + 3 * 1024, 3 * k * sizeof(double), hipMemcpyDeviceToHost, S->stream));
        HIP_TRY(hipStreamSynchronize(S->stream));
        ++S->n_stream_syncs;
        double umax = 0.0;
        for (int i = 0; i < k; ++i) umax = std::fmax(umax, std::fmax(std::fabs(st[i][1]), std::fabs(st[i][2])));
        *reach = reach_of(umax);
        S->last_reach = *reach;
        return FS_OK;
    }

    // `which`: 0 = `gathered`, 1..3 = `gathered3` (the FSIPC export slot of the buffer)
    int gather_source(const T* src, T** buf, int reach, int which)
    {
        const long n = (g.sz * ((long)S->D + 2) + 8 + 63) / 64 * 64;
        if (gather_chunks.empty()) {
            // all four at the first gather, in arena chunks like the field arrays: every rank allocates them at the same
            // point of the step, so the export is collective (FSIPC: the owners of the planes write into them)
            const int per = (int)std::min<size_t>(4, std::max<size_t>(1, ARENA_CHUNK_BYTES / ((size_t)n * sizeof(T))));
            T* at[4];
            for (int i = 0; i < 4; i += per) {
                const size_t cnt = (size_t)std::min(per, 4 - i) * (size_t)n;
                T* chunk = nullptr;
                HIP_TRY(hipMalloc((void**)&chunk, cnt * sizeof(T)));
                gather_chunks.push_back(chunk);
                HIP_TRY(hipMemsetAsync(chunk, 0, cnt * sizeof(T), S->stream));
                for (int j = 0; j < per && i + j < 4; ++j) at[i + j] = chunk + (size_t)j * (size_t)n;
            }
            HIP_TRY(hipStreamSynchronize(S->stream));
            ++S->n_alloc_syncs;
            for (size_t k = 0; k < gather_chunks.size(); ++k)
                if (S->comm.register_buffer(SLOT_GATHER + (int)k, gather_chunks[k],
                                            (size_t)std::min(per, 4 - (int)k * per) * (size_t)n * sizeof(T), true))
                    return fail(FS_ECOMM, "exporting the gathered advection sources: %s", S->comm.last_error());
            gathered = at[0] + fs::LEAD;
            for (int k = 0; k < 3; ++k) gathered3[k] = at[1 + k] + fs::LEAD;
        }
        (void)which;
        if (S->debug_poison) HIP_TRY(hipMemsetAsync(*buf - fs::LEAD, 0xFF, (g.sz * ((long)S->D + 2) + 8) * sizeof(T), S->stream));
        T* dst = *buf;
        return comm_op([&](hipStream_t st) {
            return (reach >= S->D) ? S->comm.all_gather_planes(st, src, dst, g, S->D, sizeof(T))
                                   : S->comm.gather_window(st, src, dst, g, S->D, sizeof(T), reach); },
                       "gather of the advection source");
    }

    // advect(1,v_x,v_x_prev); advect(2,v_y,v_y_prev); advect(3,v_z,v_z_prev) in one kernel
    int advect_velocity_fused()
    {
        int rc = ensure_flags();
        if (rc) return rc;
        const T kx = (T)S->dt * (T)S->W, ky = (T)S->dt * (T)S->H, kz = (T)S->dt * (T)S->D;   // :384-386
        const T* p[3] = { arr[slot[FS_VX_PREV]], arr[slot[FS_VY_PREV]], arr[slot[FS_VZ_PREV]] };
        long zshift = 0;
        if (S->comm.active()) {
            // the z velocity carrying the three traces is the current v_z (x, y) or v_z_prev (z)
            ScopedSpan sp(S, FAM_COMM);
            int reach = 0;
            double umax = -1.0;
            double uprev = -1.0;
            if (in_step && prev_vzmax_known(&uprev) && take_vzmax(0, &umax)) S->last_reach = reach = reach_of(std::fmax(umax, uprev));
            else if ((rc = trace_reach({ FS_VZ, FS_VZ_PREV }, &reach))) return rc;
            for (int k = 0; k < 3; ++k) {
                if ((rc = gather_source(p[k], &gathered3[k], reach, 1 + k))) return rc;
                p[k] = gathered3[k];
            }
            zshift = (long)sc.zoff * g.sz;
        }
        {
            ScopedSpan sp(S, FAM_ADVECT);
            fs::launch_advect_velocity<T>(S->stream, S->tune, g, sc, arr[slot[FS_VX]], arr[slot[FS_VY]], arr[slot[FS_VZ]], p[0], p[1],
                                          p[2], flags, kill, coltab.get(), kx, ky, kz, zshift);
        }
        for (int f : { FS_VX, FS_VY, FS_VZ })
            if ((rc = halo(arr[slot[f]]))) return rc;
        return FS_OK;
    }

    // The gradient pass a project_T(true) left out and advect_velocity_fused() in one kernel (single GPU).
    int gradient_advect_velocity_fused()
    {
        const T h = (T)1 / host_cbrt<T>((T)(S->W * S->H * S->D));   // :295, as in project_T
        const T kx = (T)S->dt * (T)S->W, ky = (T)S->dt * (T)S->H, kz = (T)S->dt * (T)S->D;   // :384-386
        ScopedSpan sp(S, FAM_ADVECT);
        fs::launch_gradient_advect_velocity<T>(S->stream, g, sc, arr[slot[FS_PRESSURE]], arr[slot[FS_VX]], arr[slot[FS_VY]],
                                               arr[slot[FS_VZ]], arr[slot[FS_VX_PREV]], arr[slot[FS_VY_PREV]],
                                               arr[slot[FS_VZ_PREV]], flags, h, (T)2 * h, kx, ky, kz);
        ++S->n_project_advect;
        return FS_OK;
    }

    // heat (driver/heat.h) lends the pool NHEAT more arrays, pool_stride elements apart in `chunk`, which stays heat's: the
    // temperature and its pre-solve snapshot take them
    void pool_extend(T* chunk)
    {
        for (int k = 0; k < NHEAT; ++k) {
            arr[NPOOL + k] = chunk + (size_t)k * pool_stride + g.lead;
            held[NPOOL + k] = false;
        }
        npool = NPOOL_MAX;
        slot[F_THETA] = NPOOL;
        slot[F_THETA_PREV] = NPOOL + 1;
    }
    // ... and takes them back.  The pool's arrays are interchangeable, so a field may live in one of the two that go: it moves
    // to a free one that stays.  Synchronises: queued work may still use what the caller frees next.
    int pool_shrink()
    {
        slot[F_THETA] = slot[F_THETA_PREV] = -1;
        for (int id = NPOOL; id < NPOOL_MAX; ++id) {
            if (!referenced(id)) continue;
            int to = -1;
            for (int i = 0; i < NPOOL && to < 0; ++i)
                if (!referenced(i)) to = i;
            if (to < 0) return fail(FS_ENOMEM, "array pool exhausted");   // cannot happen: NPOOL covers the fields
            fs::launch_copy<T>(S->stream, g, arr[id], arr[to]);
            for (int f = 0; f < FS_NFIELDS; ++f)
                if (slot[f] == id) slot[f] = to;
        }
        HIP_TRY(hipStreamSynchronize(S->stream));
        for (int k = 0; k < NHEAT; ++k) arr[NPOOL + k] = nullptr;
        npool = NPOOL;
        return FS_OK;
    }

    // ---- step (simulation.cpp:96-150) ---------------------------------------------------
    int step()
    {
        struct InStep {                                  // the reach bookkeeping of this step; cleared on every exit
            Engine* e;
            explicit InStep(Engine* e_) : e(e_) { e->in_step = true; e->projections_this_step = 0; e->reach_posted[0] = e->reach_posted[1] = e->reach_posted[2] = false; e->vzmax_end = -1.0; }
            ~InStep() { e->in_step = false; e->vzmax_prev = e->vzmax_end; }
        } scope(this);
        int rc = ensure_flags();
        if (rc) return rc;
        if ((rc = forces.ensure_ring())) return rc;
        if ((rc = residual.ensure_ring())) return rc;
        if ((rc = flow_stats.config())) return rc;
        if ((rc = sampling.ensure_probe_ring())) return rc;
        if ((rc = bodies.ensure_ring())) return rc;
        if ((rc = images.ensure_ring())) return rc;
        if ((rc = volume.ensure_ring())) return rc;
        if ((rc = tracers.ensure())) return rc;
        if ((rc = monitor.ensure_ring())) return rc;
        fs::InflowParams inflow_p;
        if (S->inflow) {
            if (S->comm.active()) return fail(FS_EINVAL, "fs_step: the inflow generator (option \"inflow\") needs a single-GPU handle");
            if ((rc = inflow.params("fs_step", S->steps_total, &inflow_p))) return rc;
            if ((rc = inflow.ensure())) return rc;
        }
        residual.begin_step();
        // "vorticity_confinement": the pass comes before everything the reference's step does
        if (S->confinement > 0.0 && (rc = confine.pass("fs_step", S->confinement))) return rc;
        // heat, mode 2: inlet and wall temperatures and the buoyancy force come next, still before the reference's step
        const bool heat_step = S->heat_mode() == 2;
        if (heat_step && (rc = heat.apply_pass("fs_step"))) return rc;
        // zones, mode 2: the log record -- the budget of the state the pass is about to change -- then the pass, the last thing
        // before the reference's step
        if (S->zone_mode == 2) {
            if ((rc = zones.need("fs_step"))) return rc;
            zones.record();
            if ((rc = zones.apply_pass("fs_step"))) return rc;
        }
        const bool gs =(S->solver == FS_SOLVER_GS_LEX);
        for (int f : { FS_VX, FS_VY, FS_VZ })
            if ((rc = unalias(f))) return rc;
        if (S->inflow) {                                 // "inflow": the face from the inflow generator, at step number steps_total
            inflow.launch(inflow_p, S->steps_total, nullptr);
            ++S->n_inflow;
        } else {
            ScopedSpan sp(S, FAM_MISC);
            fs::launch_inlet_velocity<T>(S->stream, g, sc, arr[slot[FS_VX]], arr[slot[FS_VY]], arr[slot[FS_VZ]],
                                         (T)(float)S->speed);   // :103-105
        }
        // z-slabs: v_z as it is now becomes v_z_prev, which carries the advection of v_z; where its max |.| is not known from
        // the previous step (first step, host-side edits) it is queued here and has the whole diffusion to arrive
        if (S->comm.active() && vzmax_prev < 0.0 && (rc = post_vzmax(2))) return rc;
        // :108-110  v_*_prev = v_*  (pre-diffusion snapshot).  Jacobi never writes its input, so
        // the snapshot is an alias and the copy costs nothing; the in-place mode really copies.
        const int V[3] = { FS_VX, FS_VY, FS_VZ }, V0[3] = { FS_VX_PREV, FS_VY_PREV, FS_VZ_PREV };
        for (int k = 0; k < 3; ++k) {
            if (gs || S->acc <= 0) {
                if ((rc = unalias(V0[k]))) return rc;
                ScopedSpan sp(S, FAM_MISC);
                fs::launch_copy<T>(S->stream, g, arr[slot[V[k]]], arr[slot[V0[k]]]);
            } else {
                slot[V0[k]] = slot[V[k]];
            }
        }
        for (int k = 0; k < 3; ++k)                      // :115-117
            if ((rc = diffuse_T(k + 1, V[k], V0[k], k))) return rc;
        // "fuse_project_advect": where :125-127 run as one kernel of the per-cell form on one GPU, that kernel also applies the
        // gradient of :120 (nothing else reads the projected velocities: the force logs read p)
        const bool fuse_pa = (S->fuse_project_advect < 0 ? PROJECT_ADVECT_AUTO : S->fuse_project_advect != 0) && !S->comm.active() &&
                             !gs && S->acc > 0 && S->fuse_advect && S->tune.advect_cell == 1 && slot[FS_VX] != slot[FS_VX_PREV] &&
                             slot[FS_VY] != slot[FS_VY_PREV] && slot[FS_VZ] != slot[FS_VZ_PREV];
        if ((rc = project_T(fuse_pa))) return rc;        // :120
        // z-slabs: :135's density solve (independent of the velocities; its result is dead, :136 overwrites it) is the work
        // the device does while the reach of each advection travels to the host -- half of its passes here, between the
        // first projection and the velocity advection, the other half where the reference has it, between the second
        // projection and the density advection.  Same passes, same order, same bits.
        const bool split = S->comm.active() && S->split_dens && !S->elide_dead && !gs && S->acc > 0;
        SolveRun dens_run;
        if (split) {
            const T a = diffusion_a();
            if ((rc = residual.log(5, 0, 0, slot[FS_DENS], slot[FS_BUFFER], (double)a, (double)((T)1 + (T)6 * a)))) return rc;
            if ((rc = solve_begin(dens_run, 0, slot[FS_DENS], slot[FS_BUFFER], a, (T)1 + (T)6 * a, S->acc))) return rc;   // :283
            if ((rc = solve_passes(dens_run, (int)dens_run.plan.size() / 2))) return rc;
            HIP_TRY(hipEventRecord(ev_slack, S->stream));
        }
        // was the device still busy with that work when the advection that waited for its reach had been queued?
        auto slack_check = [&]() {
            if (!split) return;
            if (hipEventQuery(ev_slack) == hipErrorNotReady) ++S->n_reach_hidden; else ++S->n_reach_exposed;
        };
        if (fuse_pa) {
            if ((rc = gradient_advect_velocity_fused())) return rc;
        } else if (S->fuse_advect && slot[FS_VX] != slot[FS_VX_PREV] && slot[FS_VY] != slot[FS_VY_PREV] &&
                   slot[FS_VZ] != slot[FS_VZ_PREV]) {
            // :125-127 in one pass (the three traces only chain through the cell's own values)
            if ((rc = advect_velocity_fused())) return rc;
        } else {
            for (int k = 0; k < 3; ++k)                  // :125-127
                if ((rc = advect(k + 1, V[k], V0[k]))) return rc;
        }
        slack_check();
        if ((rc = project())) return rc;                 // :130
        if (split) {
            int res;
            if ((rc = solve_end(dens_run, &res))) return rc;
            adopt(FS_DENS, res);
            const T a = diffusion_a();
            if ((rc = residual.log(5, 1, 0, slot[FS_DENS], slot[FS_BUFFER], (double)a, (double)((T)1 + (T)6 * a)))) return rc;
            HIP_TRY(hipEventRecord(ev_slack, S->stream));
        } else if (!S->elide_dead) {                     // :135 (its result is overwritten by :136)
            if ((rc = diffuse_T(0, FS_DENS, FS_BUFFER, 5))) return rc;
        }
        if ((rc = advect(0, FS_DENS, FS_BUFFER))) return rc;   // :136
        slack_check();
        if (heat_step && (rc = heat.transport_pass("fs_step"))) return rc;   // the temperature is diffused and carried last
        S->step_no++;
        S->steps_total++;
        forces.commit();
        bodies.commit();
        residual.commit();
        // the heat log: the budget of the state the transport left (three launches, no host synchronisation, the step's own stream)
        if (heat_step) heat.record();
        // "flow_stats": the state as :136 left it is a sample (no host synchronisation, the step's own stream)
        if (flow_stats.on() && S->steps_total > S->flow_stats_start &&
            (S->steps_total - S->flow_stats_start - 1) % S->flow_stats_every == 0 && (rc = flow_stats.sample()))
            return rc;
        // "monitor_log": the same state is a record of the flow monitor (three launches, no host synchronisation, the step's own stream)
        if (monitor.on() && (S->steps_total - 1) % S->monitor_every == 0) monitor.record();
        // "probe_log": the same state is a record of the probes (one launch, no host synchronisation, the step's own stream)
        sampling.probe_step();
        // "image_log": and a frame of the image views (the kernels of each view, no host synchronisation, the step's own stream)
        if (images.on() && (S->steps_total - 1) % S->image_every == 0 && (rc = images.record())) return rc;
        // "volume_log": and a frame of the volume views (one launch per view, no host synchronisation, the step's own stream)
        if (volume.on() && (S->steps_total - 1) % S->volume_every == 0 && (rc = volume.record())) return rc;
        // "tracers": the particles move through the same state, the emitters release, a snapshot is taken (one launch, no host
        // synchronisation, the step's own stream)
        tracers.step();
        if (S->in_run && S->dump_every > 0 && (S->step_no % S->dump_every) == 0) return dump_frame();   // :140-148
        return FS_OK;
    }

    // one iteration of Simulation::run()'s loop (simulation.cpp:63-71)
    int run_one()
    {
        int rc = ensure_halos();
        if (rc) return rc;
        if ((rc = unalias(FS_DENS))) return rc;
        {
            ScopedSpan sp(S, FAM_MISC);
            fs::launch_inlet_density<T>(S->stream, g, sc, arr[slot[FS_DENS]], (T)0.001f);   // :65-67
        }
        if (S->solver == FS_SOLVER_GS_LEX || S->acc <= 0 || S->elide_dead) {
            if ((rc = unalias(FS_BUFFER))) return rc;
            ScopedSpan sp(S, FAM_MISC);
            fs::launch_copy<T>(S->stream, g, arr[slot[FS_DENS]], arr[slot[FS_BUFFER]]);    // :70
        } else {
            slot[FS_BUFFER] = slot[FS_DENS];             // :70 as an alias (see step())
        }
        return step();
    }

    // ---- data access ----------------------------------------------------------------
    int get_field(int which, void* dst, size_t n, int elem)
    {
        if ((long)n != dense_cells()) return fail(FS_EINVAL, "get_field: expected %ld elements, got %zu", dense_cells(), n);
        const T* f = arr[slot[which]];
        if (elem != 1 && elem != 4 && elem != 8) return fail(FS_EINVAL, "elem_size must be 1, 4 or 8");
        {
            int rc = need_dense(n * (size_t)elem);
            if (rc) return rc;
        }
        if (elem == 4) fs::launch_pack<T, float>(S->stream, g, f, (float*)dense.get(), 0, g.D + 1);
        else if (elem == 8) fs::launch_pack<T, double>(S->stream, g, f, (double*)dense.get(), 0, g.D + 1);
        else if (elem == 1) fs::launch_pack<T, uint8_t>(S->stream, g, f, (uint8_t*)dense.get(), 0, g.D + 1);
        else return fail(FS_EINVAL, "elem_size must be 1, 4 or 8");
        HIP_TRY(hipMemcpyAsync(dst, dense.get(), n * elem, hipMemcpyDeviceToHost, S->stream));
        HIP_TRY(hipStreamSynchronize(S->stream));
        return FS_OK;
    }

    int set_field(int which, const void* src, size_t n, int elem)
    {
        if (!in_step) vzmax_prev = -1.0;             // a call from outside step(): what is known about v_z is void
        if ((long)n != dense_cells()) return fail(FS_EINVAL, "set_field: expected %ld elements, got %zu", dense_cells(), n);
        if (elem != 4 && elem != 8 && elem != 1) return fail(FS_EINVAL, "elem_size must be 1, 4 or 8");
        // a slot that shares its array gets a fresh one; contents are fully overwritten below
        if (shared_slot(which)) {
            int id = acquire();
            if (id < 0) return fail(FS_ENOMEM, "array pool exhausted");
            adopt(which, id);
        }
        {
            int rc = need_dense(n * (size_t)elem);
            if (rc) return rc;
        }
        HIP_TRY(hipMemcpyAsync(dense.get(), src, n * elem, hipMemcpyHostToDevice, S->stream));
        T* f = arr[slot[which]];
        if (elem == 4) fs::launch_unpack<T, float>(S->stream, g, (const float*)dense.get(), f, 0, g.D + 1);
        else if (elem == 8) fs::launch_unpack<T, double>(S->stream, g, (const double*)dense.get(), f, 0, g.D + 1);
        else fs::launch_unpack<T, uint8_t>(S->stream, g, (const uint8_t*)dense.get(), f, 0, g.D + 1);
        HIP_TRY(hipStreamSynchronize(S->stream));       // `src` may be freed by the caller
        if (which == FS_OBS) flags_dirty = true;
        else halos_dirty = true;
        return FS_OK;
    }

    int set_mask(const uint8_t* mask, size_t n) { return set_field(FS_OBS, mask, n, 1); }

    int point(int which, int x, int y, int z, float v, int set_instead)
    {
        if (!in_step) vzmax_prev = -1.0;             // a call from outside step(): what is known about v_z is void
        // x,y are global = local; z is global and must fall into this slab to have an effect.
        // The bookkeeping is the same on EVERY rank (every rank issues the same call): the slot maps
        // must not diverge, and ensure_halos() / ensure_flags() are collectives gated on these bits --
        // only the one-cell kernel launch depends on who owns plane z.
        int rc = unalias(which);
        if (rc) return rc;
        if (which == FS_OBS) flags_dirty = true;
        else halos_dirty = true;
        int zl = z - sc.zoff;
        if (zl < 1 || zl > g.D) return FS_OK;
        long idx = (long)x + (long)y * g.sy + (long)zl * g.sz;
        fs::launch_point_add<T>(S->stream, arr[slot[which]], idx, (T)v, set_instead);
        return FS_OK;
    }

    int tuned_two() const { return plan_two; }
    int halo_depth() const { return g.zh; }
    int tuned_three() const { return plan_three; }

    int apply_solid_cells(const int* cells, long n)
    {
        // cells: device array of packed global cell ids x + y*(W+2) + z*(W+2)*(H+2)
        int rc = unalias(FS_OBS);
        if (rc) return rc;
        fs::launch_mark_cells<T>(S->stream, g, sc, arr[slot[FS_OBS]], cells, n);
        flags_dirty = true;
        return FS_OK;
    }

    int stats(int which, double* out3) { return stats_of(arr[slot[which]], out3); }

    // The number Simulation::run() prints every 100 steps: std::reduce(dens.begin(), dens.end()) (simulation.cpp:76),
    // i.e. a sum in the field's own precision in libstdc++'s order -- groups of four as (a0 + a1) + (a2 + a3), added to the
    // running sum one group at a time (<numeric>, random-access branch).  A rounding chain cannot be reordered, so the
    // dense array comes to the host for it (once per 100 steps, console output only).
    int reference_order_sum(int which, double* out)
    {
        const long n = dense_cells();
        std::vector<T> h((size_t)n);
        int rc = get_field(which, h.data(), (size_t)n, (int)sizeof(T));
        if (rc) return rc;
        T init = (T)0;
        long i = 0;
        for (; n - i >= 4; i += 4) {
            const T v1 = h[i] + h[i + 1], v2 = h[i + 2] + h[i + 3];
            const T v3 = v1 + v2;
            init = init + v3;
        }
        for (; i < n; ++i) init = init + h[i];
        *out = (double)init;
        return FS_OK;
    }

    int stats_of(const T* field, double* out3)
    {
        // whole padded array (simulation.cpp:76, :82-89); a slab counts its own planes plus
        // the physical ghost planes it holds, and the partial results are all-reduced
        const int zlo = sc.lo_wall ? 0 : 1, zhi = sc.hi_wall ? g.D + 1 : g.D;
        fs::launch_stats<T>(S->stream, g, field, red.get() + 3 * 1024, red.get(), 3 * 1024, zlo, zhi);
        if (S->comm.active()) {
            int rc = comm_op([&](hipStream_t cs) { return S->comm.reduce_stats(cs, red.get() + 3 * 1024, g, S->D); }, "stats all-reduce");
            if (rc) return rc;
        }
        HIP_TRY(hipMemcpyAsync(out3, red.get() + 3 * 1024, 3 * sizeof(double), hipMemcpyDeviceToHost, S->stream));
        HIP_TRY(hipStreamSynchronize(S->stream));
        return FS_OK;
    }

    // ---- frame dump (simulation.cpp:56-60, 140-148) ---------------------------------------
    int dump_frame()
    {
        static const char* const names[5] = { "data.bin", "obs.bin", "v_x.bin", "v_y.bin", "v_z.bin" };
        static const int which[5] = { FS_DENS, FS_OBS, FS_VX, FS_VY, FS_VZ };
        if (!S->dump_open) {
            // rank 0 truncates like the reference's ofstream::open (simulation.cpp:56-60); the other
            // slab ranks open the same files for update once they exist
            const bool lead = !S->comm.active() || S->comm.rank == 0;
            bool ok = true;
            for (int pass = 0; pass < 2; ++pass) {
                if ((pass == 0) == lead) {
                    for (int k = 0; k < 5; ++k) {
                        std::string path = S->dump_dir + "/" + names[k];
                        S->dump_fp[k] = fopen(path.c_str(), lead ? "wb" : "r+b");
                        if (!S->dump_fp[k]) ok = false;
                    }
                }
                if (pass == 0 && S->comm.active()) {
                    if (S->comm.shm && S->comm.shm_ready(g, S->D)) return fail(FS_ECOMM, "%s", S->comm.last_error());
                    { int brc = slab_barrier(); if (brc) return brc; }
                }
            }
            if (!ok) {
                for (int k = 0; k < 5; ++k)
                    if (S->dump_fp[k]) { fclose(S->dump_fp[k]); S->dump_fp[k] = nullptr; }
                if (!S->dump_warned) {
                    // the reference silently writes nothing when data/ is missing (simulation.cpp:56-60)
                    fprintf(stderr, "fluidsim: cannot open frame dumps under '%s' -- continuing without dumps\n",
                            S->dump_dir.c_str());
                    S->dump_warned = true;
                }
                return FS_OK;
            }
            S->dump_open = true;
            S->dump_frames = 0;
        }
        // local planes written by this rank: its interior planes, plus the physical ghost planes
        const int zlo = sc.lo_wall ? 0 : 1, zhi = sc.hi_wall ? g.D + 1 : g.D;
        const long plane = (long)(g.W + 2) * (g.H + 2);
        const long frame_cells = plane * ((long)S->D + 2);
        const long nloc = plane * (zhi - zlo + 1);
        std::string werr;
        if (S->writer.init(S->device, nloc * 5, S->dump_fp, &werr)) return fail(FS_EHIP, "frame writer: %s", werr.c_str());
        const int k = (int)(S->dump_frames % fs::FrameWriter::NSLOT);
        if (S->writer.acquire(k, &werr)) return fail(FS_EIO, "%s (%s)", werr.c_str(), S->dump_dir.c_str());
        for (int f = 0; f < 5; ++f)
            fs::launch_pack<T, float>(S->stream, g, arr[slot[which[f]]], S->writer.dev[k] + (size_t)f * nloc, zlo, zhi);
        const long off = S->comm.active()
                             ? (S->dump_frames * frame_cells + plane * (long)(sc.zoff + zlo)) * (long)sizeof(float)
                             : -1;
        if (S->writer.submit(k, S->stream, nloc, off, &werr)) return fail(FS_EHIP, "frame writer: %s", werr.c_str());
        S->dump_frames++;
        if (!S->dump_async && S->writer.flush(&werr)) return fail(FS_EIO, "%s (%s)", werr.c_str(), S->dump_dir.c_str());
        return FS_OK;
    }

    // ---- measurement ----------------------------------------------------------------
    int time_sweeps(int b, int field, int prev, float a, float c, int reps, double* ms)
    {
        int rc = ensure_flags();
        if (rc) return rc;
        if (reps < 1) return fail(FS_EINVAL, "reps must be >= 1");
        int s1 = acquire(slot[field], slot[prev]);
        int s2 = acquire(slot[field], slot[prev]);
        Scratch rel{held, s1, s2};
        if (s1 < 0 || s2 < 0) return fail(FS_ENOMEM, "array pool exhausted");
        const T inv_c = (T)1 / (T)c;
        {                                                  // same launch plans as solve(); tuned BEFORE the clock starts
            int rc2 = ensure_tuned(slot[field], slot[prev], b, (T)a, inv_c);
            if (rc2) return rc2;
        }
        const bool can2 = two_sweep_kernels(), can3 = plan_three >= 0;
        HIP_TRY(rel.events());
        hipEvent_t e0 = rel.e0, e1 = rel.e1;
        // one untimed sweep to fault in code and scratch
        launch_pass(S->stream, 1, false, arr[slot[field]], arr[slot[prev]], arr[s1], b, (T)a, inv_c, 1, g.D);
        HIP_TRY(hipEventRecord(e0, S->stream));
        int src = s1, dst = s2;
        for (int r = 0; r < reps; ++r) {
            const int lv = (can3 && r + 2 < reps) ? 3 : (can2 && r + 1 < reps) ? 2 : 1;
            launch_pass(S->stream, lv, false, arr[src], arr[slot[prev]], arr[dst], b, (T)a, inv_c, 1, g.D);
            r += lv - 1;
            int t = src; src = dst; dst = t;
        }
        HIP_TRY(hipEventRecord(e1, S->stream));
        HIP_TRY(hipEventSynchronize(e1));
        float t = 0;
        HIP_TRY(hipEventElapsedTime(&t, e0, e1));
        *ms = (double)t / reps;
        return FS_OK;
    }
};

int ensure_engine(fs_sim* s)
{
    if (s->eng) return FS_OK;
    HIP_TRY(hipSetDevice(s->device));
    int rc;
    if (s->fp64) {
        auto* e = new Engine<double>(s);
        rc = e->init();
        if (rc) { delete e; return rc; }
        s->eng = e;
    } else {
        auto* e = new Engine<float>(s);
        rc = e->init();
        if (rc) { delete e; return rc; }
        s->eng = e;
    }
    return FS_OK;
}

// The call `call` on the engine of the handle's precision: ENG(s, step()), ENG(s, monitor.sample()).  Its arguments are
// evaluated once, in the branch taken.
#define ENG(s, call) ((s)->fp64 ? static_cast<Engine<double>*>((s)->eng)->call : static_cast<Engine<float>*>((s)->eng)->call)

bool in_box(fs_sim* s, int x, int y, int z) { return x >= 1 && x <= s->W && y >= 1 && y <= s->H && z >= 1 && z <= s->D; }

}  // namespace

// =======================================================================================
extern "C" {

const char* fs_last_error(void) { return g_err.c_str(); }
const char* fs_version(void) { return "fluidsim-amd 0.1 (gfx950)"; }

fs_sim* fs_create(int w, int h, int d, int iter, int speed, float dt, float diff, float visc, int acc)
{
    if (w < 1 || h < 1 || d < 1 || acc < 0 || iter < 0) {
        fail(FS_EINVAL, "fs_create: bad extents %dx%dx%d / iter %d / acc %d", w, h, d, iter, acc);
        return nullptr;
    }
    if ((double)(w + 2) * (h + 2) * (d + 2) >= 2147483647.0) {
        // the reference indexes with int (simulation.h:9,13); keep its limit on the dense layout
        fail(FS_EINVAL, "fs_create: padded grid exceeds 2^31 cells");
        return nullptr;
    }
    int ndev = 0;
    hipError_t e = hipGetDeviceCount(&ndev);
    if (e != hipSuccess || ndev < 1) {
        fail(FS_EHIP, "fs_create: no HIP device available (%s); this library has no CPU path",
             e == hipSuccess ? "device count is 0" : hipGetErrorString(e));
        return nullptr;
    }
    fs_sim* s = new fs_sim;
    s->W = w; s->H = h; s->D = d; s->iter = iter; s->speed = speed; s->acc = acc;
    s->dt = dt; s->diff = diff; s->visc = visc;
    s->heat[fs::HP_X1] = w; s->heat[fs::HP_Y1] = h; s->heat[fs::HP_Z1] = d;   // the wall box: the whole domain
    if (hipGetDevice(&s->device) != hipSuccess) s->device = 0;
    e = hipStreamCreateWithFlags(&s->stream, hipStreamNonBlocking);
    if (e != hipSuccess) {
        fail(FS_EHIP, "fs_create: hipStreamCreate: %s", hipGetErrorString(e));
        delete s;
        return nullptr;
    }
    return s;
}

// Waits for the frame writer, flushes and closes the five dump files; the next dump opens them anew.  Returns 0, or -1 with
// the first thing that went wrong in *err (a frame that did not reach its file); the files are closed in either case.
static int close_dumps(fs_sim* s, std::string* err)
{
    int rc = s->writer.flush(err);
    std::string cerr;
    if (fs::close_files(s->dump_fp, &cerr) && !rc) { *err = cerr; rc = -1; }
    s->dump_open = false;
    return rc;
}

int fs_destroy(fs_sim* s)
{
    if (!s) return FS_OK;
    hipSetDevice(s->device);
    if (s->stream) hipStreamSynchronize(s->stream);
    s->resolve_spans();
    for (hipEvent_t ev : s->event_pool) hipEventDestroy(ev);
    {
        std::string werr;
        close_dumps(s, &werr);
        s->writer.shutdown();
    }
    if (s->comm.active()) hipDeviceSynchronize();   // the communication stream too
    s->comm.release_buffers();       // FSIPC: collective; no peer maps (or still writes) this rank's arrays once it returns
    delete s->eng;
    s->comm.destroy();
    if (s->stream_full || s->stream_masked) {
        if (s->stream_full) hipStreamDestroy(s->stream_full);
        if (s->stream_masked) hipStreamDestroy(s->stream_masked);
    } else if (s->stream) {
        hipStreamDestroy(s->stream);
    }
    delete s;
    return FS_OK;
}

// Values are read by the parsers of options.h: nothing may follow a number.  The tuning options that read theirs with a bare
// atoi keep doing so, trailing characters and all ("12abc" is 12), because scripts in the field may rely on it: dump_every,
// sweep_zc, sweep_abl, pair_zc, pair_shape, mg_cycles, mg_pre, mg_post, mg_coarse_iters, mg_min_planes, advect_window,
// sweep_ry, sweep_fuse, vortex_ry, sweep_blocks, overlap, comm_cus.
int fs_set_option(fs_sim* s, const char* key, const char* value)
{
    if (!s || !key || !value) return fail(FS_EINVAL, "fs_set_option: null argument");
    std::string k = key, v = value;
    long num = 0;   // the value of an option that is a number
    int word = -1;  // ... that is a keyword: its place in the list
    if (k == "precision") {
        if (s->eng) return fail(FS_EINVAL, "precision must be set before first use");
        if ((word = fs::keyword(value, {"fp32", "fp64"})) < 0) return fail(FS_EINVAL, "precision: fp32 | fp64");
        s->fp64 = (word == 1);
    } else if (k == "solver") {
        const int solvers[] = {FS_SOLVER_JACOBI, FS_SOLVER_GS_LEX, FS_SOLVER_RBSOR, FS_SOLVER_MG};
        if ((word = fs::keyword(value, {"jacobi", "gs_lex", "rbsor", "mg"})) < 0) return fail(FS_EINVAL, "solver: jacobi | gs_lex | rbsor | mg");
        s->solver = solvers[word];
    } else if (k == "mg_cycles" || k == "mg_pre" || k == "mg_post" || k == "mg_coarse_iters") {
        const int n = atoi(value);
        if (n < (k == "mg_cycles" ? 0 : 1) || n > 1000) return fail(FS_EINVAL, "%s out of range", key);
        (k == "mg_cycles" ? s->mg_cycles : k == "mg_pre" ? s->mg_pre : k == "mg_post" ? s->mg_post : s->mg_coarse) = n;
    } else if (k == "mg_min_planes") {
        const int n = atoi(value);
        if (n < 1 || n > 1024) return fail(FS_EINVAL, "mg_min_planes: 1 .. 1024");
        s->mg_min_planes = n;
    } else if (k == "launch_plans") {
        int two = -2, three = -2;
        if (sscanf(value, "%d,%d", &two, &three) != 2 || two < -1 || three < -1 || two > 127 || three > 31)
            return fail(FS_EINVAL, "launch_plans: \"<two-sweep plan id>,<three-sweep plan id>\" (-1 = none)");
        s->replay_two = two;
        s->replay_three = three;
    } else if (k == "sor_omega") {
        const float om = (float)atof(value);
        if (!(om > 0.0f && om < 2.0f)) return fail(FS_EINVAL, "sor_omega must lie in (0, 2)");
        s->omega = om;
    } else if (k == "dump_dir") {
        // another directory: the files of the old one are finished and closed, the next dump opens the new ones.  The
        // change is made even if that reports a frame that did not reach the old files (FS_EIO, once)
        const bool moved = s->dump_open && v != s->dump_dir;
        const std::string old = s->dump_dir;
        s->dump_dir = v;
        std::string werr;
        if (moved && close_dumps(s, &werr)) return fail(FS_EIO, "frame writer: %s (%s)", werr.c_str(), old.c_str());
    } else if (k == "dump_every") {
        s->dump_every = atoi(value);
    } else if (k == "voxel_seed") {
        s->voxel_seed = (unsigned)strtoul(value, nullptr, 10);
    } else if (k == "quiet") {
        s->quiet = (v != "0");
    } else if (k == "profile") {
        s->profile = (v != "0");
    } else if (k == "elide_dead_density_solve") {
        s->elide_dead = (v != "0");
    } else if (k == "force_log") {
        if (!fs::parse_int(value, 0, 1L << 20, &num)) return fail(FS_EINVAL, "force_log: steps kept, 0 (off) .. 1048576");
        s->force_log = (int)num;
        s->force_log_gen++;
    } else if (k == "body_force_log") {
        if (!fs::parse_int(value, 0, 1L << 20, &num)) return fail(FS_EINVAL, "body_force_log: steps kept, 0 (off) .. 1048576");
        if (num > 0 && s->comm.active()) return fail(FS_EINVAL, "body_force_log: bodies are labelled on a single-GPU handle");
        s->body_log = (int)num;
        s->body_log_gen++;
    } else if (k == "moment_origin") {
        double r[3];
        const char* q = value;
        for (int a = 0; a < 3; ++a) {
            char* end = nullptr;
            r[a] = strtod(q, &end);
            if (end == q || !std::isfinite(r[a]) || *end != (a < 2 ? ',' : '\0'))
                return fail(FS_EINVAL, "moment_origin: \"x,y,z\", three finite numbers (padded index coordinates)");
            q = end + 1;
        }
        for (int a = 0; a < 3; ++a) s->moment_origin[a] = r[a];
        s->body_log_gen++;
    } else if (k == "residual_log") {
        if (!fs::parse_int(value, 0, 1L << 20, &num)) return fail(FS_EINVAL, "residual_log: steps kept, 0 (off) .. 1048576");
        s->residual_log = (int)num;
        s->residual_log_gen++;
    } else if (k == "probe_log") {
        if (!fs::parse_int(value, 0, 1L << 20, &num)) return fail(FS_EINVAL, "probe_log: records kept, 0 (off) .. 1048576");
        if ((size_t)num * (s->probes.size() / 3) * FS_PROBE_VALUES * sizeof(double) > ((size_t)1 << 30))
            return fail(FS_EINVAL, "probe_log: %ld records of %zu probes exceed 1 GiB", num, s->probes.size() / 3);
        s->probe_log = (int)num;
        s->probe_gen++;
    } else if (k == "image_log") {
        if (!fs::parse_int(value, 0, 65536, &num)) return fail(FS_EINVAL, "image_log: frames kept, 0 (off) .. 65536");
        if ((size_t)num * image_frame_bytes(s, s->image_views) > ((size_t)1 << 30))
            return fail(FS_EINVAL, "image_log: %ld frames of %zu bytes exceed 1 GiB", num, image_frame_bytes(s, s->image_views));
        s->image_log = (int)num;
        s->image_gen++;
        if (s->eng) {                                    // allocate or free now; a handle not yet in use does so at its first use
            hipSetDevice(s->device);
            return ENG(s, images.config());
        }
    } else if (k == "tracers" || k == "tracer_log") {
        const bool pool = (k == "tracers");
        if (s->comm.active()) return fail(FS_EINVAL, "%s: tracers need a single-GPU handle", key);
        if (!fs::parse_int(value, 0, pool ? 4194304L : 65536L, &num))
            return fail(FS_EINVAL, pool ? "tracers: slots of the pool, 0 (off) .. 4194304" : "tracer_log: frames kept, 0 (off) .. 65536");
        const size_t C = (size_t)(pool ? num : s->tracers), N = (size_t)(pool ? s->tracer_log : num);
        if (N * C * FS_TRACER_FRAME_BYTES > ((size_t)1 << 30))
            return fail(FS_EINVAL, "%s: %zu frames of %zu slots exceed 1 GiB", key, N, C);
        if (pool) { s->tracers = (int)num; s->tracer_gen++; }
        else { s->tracer_log = (int)num; s->tracer_log_gen++; }
        if (s->eng) {                                    // allocate or free now; a handle not yet in use does so at its first use
            hipSetDevice(s->device);
            return ENG(s, tracers.config());
        }
        if (pool) s->tracer_seeded = 0;
    } else if (k == "tracer_every") {
        if (s->comm.active()) return fail(FS_EINVAL, "tracer_every: tracers need a single-GPU handle");
        if (!fs::parse_int(value, 1, 1L << 30, &num)) return fail(FS_EINVAL, "tracer_every: K >= 1");
        s->tracer_every = num;
    } else if (k == "volume_log") {
        if (!fs::parse_int(value, 0, 65536, &num)) return fail(FS_EINVAL, "volume_log: frames kept, 0 (off) .. 65536");
        if ((size_t)num * volume_frame_bytes(s, s->volume_views) > ((size_t)1 << 30))
            return fail(FS_EINVAL, "volume_log: %ld frames of %zu bytes exceed 1 GiB", num, volume_frame_bytes(s, s->volume_views));
        if (num > 0 && s->comm.active()) return fail(FS_EINVAL, "volume_log: volumes are rendered on a single-GPU handle");
        s->volume_log = (int)num;
        s->volume_gen++;
        if (s->eng) {                                    // allocate or free now; a handle not yet in use does so at its first use
            hipSetDevice(s->device);
            return ENG(s, volume.config());
        }
    } else if (k == "monitor_log") {
        if (s->comm.active()) return fail(FS_EINVAL, "monitor_log: the flow monitor needs a single-GPU handle");
        if (!fs::parse_int(value, 0, 1L << 20, &num)) return fail(FS_EINVAL, "monitor_log: records kept, 0 (off) .. 1048576");
        s->monitor_log = (int)num;
        s->monitor_gen++;
    } else if (k == "monitor_every") {
        if (s->comm.active()) return fail(FS_EINVAL, "monitor_every: the flow monitor needs a single-GPU handle");
        if (!fs::parse_int(value, 1, 1L << 30, &num)) return fail(FS_EINVAL, "monitor_every: K >= 1");
        s->monitor_every = num;
    } else if (k == "monitor_stations") {
        if (s->comm.active()) return fail(FS_EINVAL, "monitor_stations: the flow monitor needs a single-GPU handle");
        fs::MonitorStations st = {{0, 0, 0, 0, 0, 0, 0, 0}};
        if (!fs::parse_int_list(value, 1, s->W, fs::MON_STATIONS, st.x, &s->monitor_nstations))
            return fail(FS_EINVAL, "monitor_stations: \"x1,x2,...\", up to %d indices in 1 .. %d (\"\" = none)", fs::MON_STATIONS, s->W);
        s->monitor_stations = st;
        s->monitor_gen++;
    } else if (k == "vorticity_confinement") {
        if (!fs::parse_real(value, 0.0, &s->confinement)) return fail(FS_EINVAL, "vorticity_confinement: a finite strength >= 0 (0 = off)");
    } else if (k == "inflow") {
        if ((word = fs::keyword(value, {"off", "on"})) < 0) return fail(FS_EINVAL, "inflow: on | off");
        s->inflow = (word == 1);
    } else if (k == "inflow_eddies") {
        if (!fs::parse_int(value, 0, fs::INFLOW_EDDIES_MAX, &num)) return fail(FS_EINVAL, "inflow_eddies: 0 .. %d", fs::INFLOW_EDDIES_MAX);
        s->inflow_n = (int)num;
    } else if (k == "inflow_sigma" || k == "inflow_rms" || k == "inflow_convect") {
        if (k == "inflow_convect" && v == "auto") {
            s->inflow_convect = -1.0;
        } else {
            const double least = (k == "inflow_sigma") ? 1.0 : 0.0;
            if (!fs::parse_real(value, least, k == "inflow_sigma" ? &s->inflow_sigma : k == "inflow_rms" ? &s->inflow_rms : &s->inflow_convect))
                return fail(FS_EINVAL, "%s: a finite number >= %g%s", key, least, k == "inflow_convect" ? ", or auto" : "");
        }
    } else if (k == "inflow_seed") {
        if (!fs::parse_u64(value, &s->inflow_seed)) return fail(FS_EINVAL, "inflow_seed: an unsigned 64-bit number");
    } else if (k == "volume_every") {
        if (!fs::parse_int(value, 1, 1L << 30, &num)) return fail(FS_EINVAL, "volume_every: K >= 1");
        s->volume_every = num;
    } else if (k == "image_every") {
        if (!fs::parse_int(value, 1, 1L << 30, &num)) return fail(FS_EINVAL, "image_every: K >= 1");
        s->image_every = num;
    } else if (k == "flow_stats") {
        const int kinds[] = {0, fs::ST_NMEAN, fs::ST_NMOMENTS};
        if ((word = fs::keyword(value, {"off", "mean", "moments"})) < 0) return fail(FS_EINVAL, "flow_stats: off | mean | moments");
        s->flow_stats = kinds[word];
        s->flow_stats_gen++;
        s->flow_stats_n = 0;
        if (s->eng) {                                    // allocate or free now; a handle not yet in use does so at its first use
            hipSetDevice(s->device);
            return ENG(s, flow_stats.config());
        }
    } else if (k == "flow_stats_every" || k == "flow_stats_start") {
        const bool every = (k == "flow_stats_every");
        if (!fs::parse_int(value, every ? 1 : 0, 1L << 30, &num))
            return fail(FS_EINVAL, every ? "flow_stats_every: N >= 1" : "flow_stats_start: S >= 0");
        (every ? s->flow_stats_every : s->flow_stats_start) = num;
    } else if (k == "dump_async") {
        s->dump_async = (v != "0");
    } else if (k == "fuse_advect") {
        s->fuse_advect = (v != "0");
    } else if (k == "zero_start" || k == "fuse_project_advect") {
        if ((word = fs::keyword(value, {"auto", "0", "1"})) < 0) return fail(FS_EINVAL, "%s: auto | 0 | 1", key);
        (k == "zero_start" ? s->zero_start : s->fuse_project_advect) = word - 1;
    } else if (k == "overlap") {
        if (s->eng && s->overlap_plan >= 0) return fail(FS_EINVAL, "overlap must be set before the first solve");
        s->overlap = (v == "auto") ? -1 : atoi(value);   // a refused value stays behind, as it always did
        if (s->overlap < -1 || s->overlap > 3 || fs::keyword(value, {"auto", "0", "1", "2", "3"}) < 0)
            return fail(FS_EINVAL, "overlap: auto | 0 | 1 | 2 | 3");
    } else if (k == "comm_cus") {
        if (s->eng) return fail(FS_EINVAL, "comm_cus must be set before first use");
        s->comm_cus = (v == "auto") ? -1 : atoi(value);
        if (s->comm_cus < -1 || s->comm_cus > 128) return fail(FS_EINVAL, "comm_cus: auto | 0 .. 128");
    } else if (k == "split_density_solve") {
        s->split_dens = (v != "0");
    } else if (k == "debug_poison_gather") {
        s->debug_poison = (v != "0");
    } else if (k == "sweep_ry") {
        int r = atoi(value);
        if (r != 2 && r != 4) return fail(FS_EINVAL, "sweep_ry: 2 | 4");
        s->tune.ry = r;
    } else if (k == "sweep_zc") {
        s->tune.zc_len = atoi(value);
    } else if (k == "sweep_blocks") {
        s->tune.target_blocks = atoi(value) > 0 ? atoi(value) : 2048;
    } else if (k == "sweep_abl") {
        s->tune.abl = atoi(value);
    } else if (k == "sweep_fuse") {
        int f = atoi(value);
        if (f < 1 || f > 4) return fail(FS_EINVAL, "sweep_fuse: 1 | 2 | 3 | 4");
        s->tune.fuse = f;
    } else if (k == "vortex_ry") {
        int r = atoi(value);
        if (r != 1 && r != 2) return fail(FS_EINVAL, "vortex_ry: 1 | 2");
        s->tune.vortex_ry = r;
    } else if (k == "project_kernels") {
        if ((word = fs::keyword(value, {"march", "cell"})) < 0) return fail(FS_EINVAL, "project_kernels: march | cell");
        s->tune.project_cell = word;
    } else if (k == "advect_kernels") {
        if ((word = fs::keyword(value, {"row", "cell", "celltab", "tile"})) < 0) return fail(FS_EINVAL, "advect_kernels: cell | celltab | tile | row");
        s->tune.advect_cell = word;
    } else if (k == "advect_window") {
        const int n = atoi(value);
        if (n < 1 || n > 128) return fail(FS_EINVAL, "advect_window: 1 .. 128");
        s->tune.advect_window = n;
    } else if (k == "wall_free" || k == "mask_free") {
        if ((word = fs::keyword(value, {"0", "auto", "1"})) < 0) return fail(FS_EINVAL, "%s: 0 | auto | 1", key);
        (k == "wall_free" ? s->tune.wall_free : s->tune.mask_free) = word;
    } else if (k == "chunk_cost") {
        // per-iteration costs of the general, wall-free and mask-free bodies the z chunks are balanced by; "0" = equal chunks
        fs::ChunkCost c;
        if (v != "0" && (sscanf(value, "%d,%d,%d", &c.general, &c.wall_free, &c.mask_free) != 3 || c.general <= 0 ||
                         c.wall_free <= 0 || c.mask_free <= 0 || c.general > 1000000 || c.wall_free > 1000000 || c.mask_free > 1000000))
            return fail(FS_EINVAL, "chunk_cost: 0 | general,wall_free,mask_free (positive integers)");
        s->tune.chunk_cost = c;
    } else if (k == "pair_zc") {
        s->tune.pair_zc = atoi(value);
    } else if (k == "pair_shape") {
        s->tune.pair_shape = atoi(value);
    } else if (k == "two_sweep_kernel") {
        if ((word = fs::keyword(value, {"auto", "pair", "fused"})) < 0) return fail(FS_EINVAL, "two_sweep_kernel: auto | pair | fused");
        s->tune.two_kind = word;
    } else {
        return fail(FS_EINVAL, "unknown option '%s'", key);
    }
    return FS_OK;
}

int fs_get_int(fs_sim* s, const char* name, int* out)
{
    if (!s || !name || !out) return fail(FS_EINVAL, "null argument");
    std::string n = name;
    if (n == "width") *out = s->W; else if (n == "height") *out = s->H; else if (n == "depth") *out = s->D;
    else if (n == "speed") *out = s->speed; else if (n == "acc") *out = s->acc; else if (n == "iter") *out = s->iter;
    else if (n == "local_depth") *out = s->comm.active() ? s->comm.local_depth(s->D) : s->D;
    else if (n == "z_offset") *out = s->comm.active() ? s->comm.z_offset(s->D) : 0;
    else if (n == "last_advect_reach") *out = s->last_reach;
    else if (n == "pair_shape") *out = s->eng ? ENG(s, tuned_two()) : -1;
    else if (n == "triple_plan") *out = s->eng ? ENG(s, tuned_three()) : -1;
    else if (n == "zero_start_projections") *out = s->n_zero_start;        // projections whose solve started from unread zeros
    else if (n == "z_alternate") *out = s->z_alternate;
    else if (n == "reversed_passes") *out = (int)s->n_reversed;            // three-sweep passes that marched downward in z
    else if (n == "project_advect_steps") *out = s->n_project_advect;      // steps whose first gradient ran inside the advection
    else if (n == "two_sweep_fused")   // 1: jacobi_fused_kernel<NL=2>, 0: jacobi_pair_kernel
        *out = (s->eng && fs::decode_plan(false, ENG(s, tuned_two())).kind == fs::SweepKernel::Fused2) ? 1 : 0;
    else if (n == "halo_depth") *out = s->eng ? ENG(s, halo_depth()) : 0;
    else if (n == "mg_levels") *out = s->eng ? ENG(s, multigrid_levels()) : 0;          // levels of the last solver=mg solve, level 0 included
    else if (n == "mg_first_replicated") *out = s->eng ? ENG(s, multigrid_first_replicated()) : 0;   // ... the first held whole by every rank
    // z-slab runs: the communication schedule in force (what "auto" chose), and the slab step's host-side waits
    else if (n == "overlap_plan") *out = s->overlap_plan;
    else if (n == "comm_cus_plan") *out = s->cus_plan;
    else if (n == "stream_syncs") *out = (int)s->n_stream_syncs;          // hipStreamSynchronize calls issued by slab steps (reach fallback)
    else if (n == "reach_waits") *out = (int)s->n_reach_waits;            // waits for an asynchronously delivered reach ...
    else if (n == "reach_waits_blocked") *out = (int)s->n_reach_blocked;  // ... that found it not yet delivered
    else if (n == "reach_wait_us") *out = (int)(s->reach_wait_ms * 1e3);  // host time spent blocked in them
    else if (n == "reach_hidden") *out = (int)s->n_reach_hidden;          // advections queued while the device still had the work placed before them ...
    else if (n == "reach_exposed") *out = (int)s->n_reach_exposed;        // ... and after it had run dry (a bubble on the device)
    else if (n == "dump_slot_waits") *out = (int)std::min<long>(s->writer.slot_waits, 2147483647L);   // frame dumps that found their staging slot still being written
    else if (n == "probe_count") *out = (int)(s->probes.size() / 3);      // probes set by fs_set_probes
    else if (n == "body_count" || n == "body_components") {               // bodies / components of the labelling (made now if obs changed)
        int b = 0, c = 0;
        { int rc_ = ensure_engine(s); if (rc_) return rc_; }
        hipSetDevice(s->device);
        const int rc = ENG(s, bodies.counts(&b, &c));
        if (rc) return rc;
        *out = (n == "body_count") ? b : c;
    }
    else if (n == "image_views") *out = (int)s->image_views.size();       // views set by fs_image_views
    else if (n == "volume_views") *out = (int)s->volume_views.size();     // views set by fs_volume_views
    else if (n == "volume_frame_bytes") *out = (int)volume_frame_bytes(s, s->volume_views);   // one frame of the volume log
    else if (n == "image_frame_bytes") *out = (int)image_frame_bytes(s, s->image_views);   // one frame of the image log
    else if (n == "tracer_capacity") *out = s->tracers;                    // slots of the tracer pool
    else if (n == "tracer_count") *out = (int)std::min<long>(s->tracer_seeded, s->tracers);   // slots a fetch returns
    else if (n == "tracer_seeded") *out = (int)std::min<long>(s->tracer_seeded, 2147483647L);   // particles seeded or released since the pool was cleared, saturating
    else if (n == "tracer_emitters") *out = (int)(s->tracer_emit.size() / 3);
    else if (n == "inflow") *out = s->inflow ? 1 : 0;
    else if (n == "inflow_eddies") *out = s->inflow_n;
    else if (n == "inflow_passes") *out = (int)std::min<long>(s->n_inflow, 2147483647L);   // inlet planes the steps wrote through the inflow generator
    else if (n == "heat_mode") *out = s->heat_mode();                     // 0 off, 1 manual, 2 in fs_step (fs_heat_params)
    else if (n == "heat_applies") *out = (int)std::min<long>(s->n_heat_apply, 2147483647L);       // passes A done, in steps and by fs_heat_apply
    else if (n == "heat_transports") *out = (int)std::min<long>(s->n_heat_transport, 2147483647L);   // passes B done, in steps and by fs_heat_transport
    else if (n == "zone_mode") *out = s->zone_mode;                       // 0 off, 1 manual, 2 in fs_step (fs_zones)
    else if (n == "zone_applies") *out = (int)std::min<long>(s->n_zone_apply, 2147483647L);       // zone passes done, in steps and by fs_zone_apply
    else if (n == "confinement_passes") *out = (int)std::min<long>(s->n_confine, 2147483647L);   // confinement passes done, in steps and by fs_confine_vorticity
    else if (n == "monitor_log") *out = s->monitor_log;
    else if (n == "monitor_every") *out = (int)s->monitor_every;
    else if (n == "monitor_stations") *out = s->monitor_nstations;        // how many stations are set
    else if (n == "flow_stats_samples") *out = (int)s->flow_stats_n;      // samples in the flow statistics since the last reset
    else return fail(FS_EINVAL, "unknown int member '%s'", name);
    return FS_OK;
}
int fs_set_int(fs_sim* s, const char* name, int value)
{
    if (!s || !name) return fail(FS_EINVAL, "null argument");
    std::string n = name;
    if (n == "speed") s->speed = value;
    else if (n == "acc") { if (value < 0) return fail(FS_EINVAL, "acc < 0"); s->acc = value; }
    else if (n == "iter") { if (value < 0) return fail(FS_EINVAL, "iter < 0"); s->iter = value; }
    else if (n == "z_alternate") { if (value < -1 || value > 1) return fail(FS_EINVAL, "z_alternate: -1 (auto) | 0 | 1"); s->z_alternate = value; }
    else return fail(FS_EINVAL, "member '%s' is fixed after construction", name);
    return FS_OK;
}
int fs_get_float(fs_sim* s, const char* name, float* out)
{
    if (!s || !name || !out) return fail(FS_EINVAL, "null argument");
    std::string n = name;
    if (n == "dt") *out = s->dt; else if (n == "diff") *out = s->diff; else if (n == "visc") *out = s->visc;
    else if (n == "vorticity_confinement") *out = (float)s->confinement;
    else if (n == "inflow_sigma") *out = (float)s->inflow_sigma;
    else if (n == "inflow_rms") *out = (float)s->inflow_rms;
    else if (n == "inflow_convect") *out = (float)s->inflow_convect_now();   // what "auto" stands for now
    else if (n.size() == 11 && n.compare(0, 7, "overlap") == 0 && n.compare(8, 3, "_ms") == 0 && n[7] >= '0' && n[7] <= '7')
        *out = (float)s->overlap_ms[n[7] - '0'];   // "overlap<k>_ms": slowest rank's ms per pass of candidate k = overlap mode + 4 * (CU mask on), 0 = not timed
    else return fail(FS_EINVAL, "unknown float member '%s'", name);
    return FS_OK;
}
int fs_set_float(fs_sim* s, const char* name, float value)
{
    if (!s || !name) return fail(FS_EINVAL, "null argument");
    std::string n = name;
    if (n == "dt") s->dt = value; else if (n == "diff") s->diff = value; else if (n == "visc") s->visc = value;
    else return fail(FS_EINVAL, "unknown float member '%s'", name);
    return FS_OK;
}

#define ENGINE_OR_RETURN(s)                                  \
    if (!(s)) return fail(FS_EINVAL, "null handle");         \
    { int rc_ = ensure_engine(s); if (rc_) return rc_; }     \
    hipSetDevice((s)->device);

int fs_add_obstacle(fs_sim* s, int x, int y, int z)
{
    ENGINE_OR_RETURN(s);
    if (!in_box(s, x, y, z)) return fail(FS_EINVAL, "addObstacle(%d,%d,%d) outside 1..%dx1..%dx1..%d", x, y, z, s->W, s->H, s->D);
    return ENG(s, point(FS_OBS, x, y, z, 1.0f, 1));
}
int fs_add_density(fs_sim* s, int x, int y, int z, float amount)
{
    ENGINE_OR_RETURN(s);
    if (!in_box(s, x, y, z)) return fail(FS_EINVAL, "addDensity(%d,%d,%d) outside the grid", x, y, z);
    return ENG(s, point(FS_DENS, x, y, z, amount, 0));
}
int fs_set_velocity(fs_sim* s, int x, int y, int z, float ax, float ay, float az)
{
    ENGINE_OR_RETURN(s);
    if (!in_box(s, x, y, z)) return fail(FS_EINVAL, "setVelocity(%d,%d,%d) outside the grid", x, y, z);
    int rc = ENG(s, point(FS_VX, x, y, z, ax, 1));
    if (!rc) rc = ENG(s, point(FS_VY, x, y, z, ay, 1));
    if (!rc) rc = ENG(s, point(FS_VZ, x, y, z, az, 1));
    return rc;
}

int fs_set_obstacle_mask(fs_sim* s, const uint8_t* mask, size_t n)
{
    ENGINE_OR_RETURN(s);
    if (!mask) return fail(FS_EINVAL, "null mask");
    return ENG(s, set_mask(mask, n));
}

int fs_load_stl(fs_sim* s, const char* stl_file, float scale, float rot_x, float rot_y, float rot_z,
                float translate_x, float translate_y, float translate_z, long* added)
{
    ENGINE_OR_RETURN(s);
    if (!stl_file) return fail(FS_EINVAL, "null path");
    fs::VoxelResult vr;
    int rc;
    try {                                                  // the parser and the setup allocate: nothing may leave a C function
        rc = fs::voxelize_stl(s->stream, stl_file, s->W, s->H, s->D, scale, rot_x, rot_y, rot_z, translate_x,
                              translate_y, translate_z, s->voxel_seed, s->quiet, &vr);
    } catch (const std::exception& e) {                    // std::bad_alloc, std::length_error: host memory for the mesh
        fs::voxelize_free(&vr);
        return fail(FS_ENOMEM, "voxelizer: %s", e.what());
    } catch (...) {
        fs::voxelize_free(&vr);
        return fail(FS_ENOMEM, "voxelizer: unknown exception");
    }
    if (rc) {                                              // every exit releases the voxelizer's device buffers
        const std::string msg = vr.error;
        fs::voxelize_free(&vr);
        return rc == FS_EIO ? fail(FS_EIO, "%s", msg.c_str()) : fail(rc, "voxelizer: %s", msg.c_str());
    }
    if (added) *added = vr.added;
    rc = ENG(s, apply_solid_cells(vr.d_cells, vr.added));
    hipStreamSynchronize(s->stream);
    fs::voxelize_free(&vr);
    return rc;
}

int fs_step(fs_sim* s) { ENGINE_OR_RETURN(s); return ENG(s, step()); }
int fs_run_one(fs_sim* s) { ENGINE_OR_RETURN(s); return ENG(s, run_one()); }

int fs_sync(fs_sim* s)
{
    if (!s) return fail(FS_EINVAL, "null handle");
    hipSetDevice(s->device);
    HIP_TRY(hipStreamSynchronize(s->stream));
    std::string werr;
    if (s->writer.flush(&werr)) return fail(FS_EIO, "frame writer: %s", werr.c_str());
    if (s->comm.check()) return fail(FS_ECOMM, "%s", s->comm.last_error());
    return FS_OK;
}

int fs_run(fs_sim* s)
{
    ENGINE_OR_RETURN(s);
    const bool talk = !s->quiet && (!s->comm.active() || s->comm.rank == 0);
    if (talk) printf("starting 3-D simulation: %dx%dx%d  steps = %d\n", s->W, s->H, s->D, s->iter);   // simulation.cpp:51-53
    // run() re-opens (truncates) the five files (simulation.cpp:56-60).  Whatever the frames dumped since the last run
    // still owe -- a failed write, flush or close -- is reported here, once: the files are closed either way, so the call
    // that follows starts clean
    {
        std::string werr;
        if (close_dumps(s, &werr)) return fail(FS_EIO, "frame writer: %s", werr.c_str());
    }
    s->in_run = true;
    s->step_no = 0;
    int rc = FS_OK;
    for (int i = 0; i < s->iter && !rc; ++i) {
        rc = ENG(s, run_one());
        if (!rc && (i + 1) % 100 == 0 && i > 0) {         // :73-77
            // one GPU: the reference's own float sum, digit for digit; z-slabs: the all-reduced double sum (a rounding
            // chain over the whole array does not split over ranks)
            double st[3] = {0, 0, 0};
            if (s->comm.active()) rc = ENG(s, stats(FS_DENS, st));
            else if (talk) rc = ENG(s, reference_order_sum(FS_DENS, &st[0]));
            if (!rc && talk) printf("step %d\n  density sum = %g\n", i + 1, st[0]);
        }
    }
    if (!rc && s->dump_every == -1) rc = ENG(s, dump_frame());
    s->in_run = false;
    {
        std::string werr;
        if (s->writer.flush(&werr) && !rc) rc = fail(FS_EIO, "frame writer: %s (%s)", werr.c_str(), s->dump_dir.c_str());
    }
    if (rc) {
        // a failed run leaves no files open and no error behind (the writer is drained: the flush above waited for it)
        std::string werr;
        close_dumps(s, &werr);
        return rc;
    }
    static const int which[4] = { FS_DENS, FS_VX, FS_VY, FS_VZ };
    static const char* const label[4] = { "density ", "velocity x", "velocity y", "velocity z" };
    if (talk) printf("\n--- statistics -------------------------------------------------\n");   // :81
    for (int k = 0; k < 4; ++k) {
        double st[3];
        rc = ENG(s, stats(which[k], st));
        if (rc) return rc;
        if (talk) printf("%s min = %g\n%s max = %g\n", label[k], st[1], label[k], st[2]);          // :82-89
    }
    if (talk) { printf("simulation finished\n"); fflush(stdout); }
    return FS_OK;
}

#define CHECK_FIELD(f) if ((f) < 0 || (f) >= FS_NFIELDS) return fail(FS_EINVAL, "bad field selector %d", (f));
#define CHECK_B(b) if ((b) < 0 || (b) > 3) return fail(FS_EINVAL, "bad boundary code %d", (b));

int fs_set_bounds(fs_sim* s, int b, int field) { ENGINE_OR_RETURN(s); CHECK_B(b); CHECK_FIELD(field); return ENG(s, set_bounds(b, field)); }
int fs_linear_solver(fs_sim* s, int b, int field, int prev, float a, float c)
{
    ENGINE_OR_RETURN(s); CHECK_B(b); CHECK_FIELD(field); CHECK_FIELD(prev);
    if (field == prev) return fail(FS_EINVAL, "field and prev must differ");
    return ENG(s, linear_solver(b, field, prev, a, c));
}
int fs_diffuse(fs_sim* s, int b, int field, int prev)
{
    ENGINE_OR_RETURN(s); CHECK_B(b); CHECK_FIELD(field); CHECK_FIELD(prev);
    if (field == prev) return fail(FS_EINVAL, "field and prev must differ");
    return ENG(s, diffuse(b, field, prev));
}
int fs_project(fs_sim* s) { ENGINE_OR_RETURN(s); return ENG(s, project()); }
int fs_advect(fs_sim* s, int b, int field, int prev)
{
    ENGINE_OR_RETURN(s); CHECK_B(b); CHECK_FIELD(field); CHECK_FIELD(prev);
    if (field == prev) return fail(FS_EINVAL, "field and prev must differ");
    return ENG(s, advect(b, field, prev));
}

int fs_get_field(fs_sim* s, int which, void* dst, size_t n, int elem_size)
{
    ENGINE_OR_RETURN(s); CHECK_FIELD(which);
    if (!dst) return fail(FS_EINVAL, "null buffer");
    return ENG(s, get_field(which, dst, n, elem_size));
}
int fs_set_field(fs_sim* s, int which, const void* src, size_t n, int elem_size)
{
    ENGINE_OR_RETURN(s); CHECK_FIELD(which);
    if (!src) return fail(FS_EINVAL, "null buffer");
    return ENG(s, set_field(which, src, n, elem_size));
}
size_t fs_padded_size(fs_sim* s)
{
    if (!s) return 0;
    int d = s->comm.active() ? s->comm.local_depth(s->D) : s->D;
    return (size_t)(s->W + 2) * (s->H + 2) * (d + 2);
}

int fs_dump_frame(fs_sim* s) { ENGINE_OR_RETURN(s); return ENG(s, dump_frame()); }

int fs_field_stats(fs_sim* s, int which, double* sum, double* mn, double* mx)
{
    ENGINE_OR_RETURN(s); CHECK_FIELD(which);
    double st[3];
    int rc = ENG(s, stats(which, st));
    if (rc) return rc;
    if (sum) *sum = st[0];
    if (mn) *mn = st[1];
    if (mx) *mx = st[2];
    return FS_OK;
}

int fs_get_timing(fs_sim* s, const char* family, double* total_ms, long* launches)
{
    if (!s || !family) return fail(FS_EINVAL, "null argument");
    hipSetDevice(s->device);
    s->resolve_spans();
    for (int f = 0; f < FAM_COUNT; ++f)
        if (strcmp(family, family_name(f)) == 0) {
            if (total_ms) *total_ms = s->fam_ms[f];
            if (launches) *launches = s->fam_launches[f];
            return FS_OK;
        }
    return fail(FS_EINVAL, "unknown kernel family '%s'", family);
}
int fs_reset_timing(fs_sim* s)
{
    if (!s) return fail(FS_EINVAL, "null handle");
    hipSetDevice(s->device);
    s->resolve_spans();
    for (int f = 0; f < FAM_COUNT; ++f) { s->fam_ms[f] = 0; s->fam_launches[f] = 0; }
    return FS_OK;
}

int fs_time_sweeps(fs_sim* s, int b, int field, int prev, float a, float c, int reps, double* ms_per_sweep)
{
    ENGINE_OR_RETURN(s); CHECK_B(b); CHECK_FIELD(field); CHECK_FIELD(prev);
    if (!ms_per_sweep) return fail(FS_EINVAL, "null output");
    return ENG(s, time_sweeps(b, field, prev, a, c, reps, ms_per_sweep));
}

int fs_streamlines(fs_sim* s, int density, double proximity, int max_length, double step_size,
                   double vel_change_threshold, long* n_lines, long* n_points)
{
    ENGINE_OR_RETURN(s);
    int rc = ENG(s, viewer.streamlines(density, proximity, max_length, step_size, vel_change_threshold));
    if (rc) return rc;
    if (n_lines) *n_lines = (long)s->sl_norm.size();
    if (n_points) *n_points = (long)(s->sl_points.size() / 3);
    return FS_OK;
}

int fs_streamlines_fetch(fs_sim* s, long* offsets, double* points, double* norm_speed)
{
    ENGINE_OR_RETURN(s);
    if (s->sl_offsets.empty()) return fail(FS_EINVAL, "fs_streamlines has not been called");
    if (offsets) memcpy(offsets, s->sl_offsets.data(), s->sl_offsets.size() * sizeof(long));
    if (points && !s->sl_points.empty()) memcpy(points, s->sl_points.data(), s->sl_points.size() * sizeof(double));
    if (norm_speed && !s->sl_norm.empty()) memcpy(norm_speed, s->sl_norm.data(), s->sl_norm.size() * sizeof(double));
    return FS_OK;
}

int fs_obstacle_surface(fs_sim* s, long* n_vertices, long* n_triangles)
{
    ENGINE_OR_RETURN(s);
    int rc = ENG(s, viewer.obstacle_surface());
    if (rc) return rc;
    if (n_vertices) *n_vertices = (long)(s->surf_verts.size() / 3);
    if (n_triangles) *n_triangles = (long)(s->surf_tris.size() / 3);
    return FS_OK;
}

int fs_obstacle_surface_fetch(fs_sim* s, float* vertices, int* triangles)
{
    if (!s) return fail(FS_EINVAL, "null handle");
    if (!s->surf_valid) return fail(FS_EINVAL, "fs_obstacle_surface has not been called");
    if (vertices && !s->surf_verts.empty()) memcpy(vertices, s->surf_verts.data(), s->surf_verts.size() * sizeof(float));
    if (triangles && !s->surf_tris.empty()) memcpy(triangles, s->surf_tris.data(), s->surf_tris.size() * sizeof(int));
    return FS_OK;
}

int fs_isosurface(fs_sim* s, int source, double level, long* n_vertices, long* n_triangles)
{
    ENGINE_OR_RETURN(s);
    int rc = ENG(s, vortex.isosurface(source, level));
    if (rc) return rc;
    if (n_vertices) *n_vertices = (long)(s->iso_verts.size() / 3);
    if (n_triangles) *n_triangles = (long)(s->iso_tris.size() / 3);
    return FS_OK;
}

int fs_isosurface_fetch(fs_sim* s, float* vertices, int* triangles)
{
    if (!s) return fail(FS_EINVAL, "null handle");
    if (!s->iso_valid) return fail(FS_EINVAL, "fs_isosurface has not been called");
    if (vertices && !s->iso_verts.empty()) memcpy(vertices, s->iso_verts.data(), s->iso_verts.size() * sizeof(float));
    if (triangles && !s->iso_tris.empty()) memcpy(triangles, s->iso_tris.data(), s->iso_tris.size() * sizeof(int));
    return FS_OK;
}

int fs_surface_case_table(int config, int* edges)
{
    if (!edges) return fail(FS_EINVAL, "null buffer");
    int n = fs::surface_case(config, edges);
    if (n < 0) return fail(FS_EINVAL, "bad cube configuration %d (0..255)", config);
    return n;
}

int fs_obstacle_force(fs_sim* s, double out[5], double* per_plane)
{
    ENGINE_OR_RETURN(s);
    if (!out) return fail(FS_EINVAL, "null output");
    return ENG(s, forces.obstacle_force(out, per_plane));
}

int fs_force_log(fs_sim* s, double* rows, long max_rows, long* n_rows, long* n_dropped)
{
    ENGINE_OR_RETURN(s);
    return ENG(s, forces.log_fetch(rows, max_rows, n_rows, n_dropped));
}

int fs_label_bodies(fs_sim* s, long* n_components, long* n_bodies)
{
    ENGINE_OR_RETURN(s);
    return ENG(s, bodies.label(n_components, n_bodies));
}
int fs_body_labels(fs_sim* s, int32_t* dst, size_t n)
{
    ENGINE_OR_RETURN(s);
    if (!dst) return fail(FS_EINVAL, "null buffer");
    return ENG(s, bodies.labels(dst, n));
}
int fs_body_info(fs_sim* s, double* rows, long max_rows, long* n_rows)
{
    ENGINE_OR_RETURN(s);
    return ENG(s, bodies.info(rows, max_rows, n_rows));
}
int fs_body_force(fs_sim* s, double* out, long max_rows, long* n_rows, double* per_plane)
{
    ENGINE_OR_RETURN(s);
    return ENG(s, bodies.query(out, max_rows, n_rows, per_plane));
}
int fs_body_force_log(fs_sim* s, double* rows, long max_rows, long* n_rows, long* n_dropped)
{
    ENGINE_OR_RETURN(s);
    return ENG(s, bodies.log_fetch(rows, max_rows, n_rows, n_dropped));
}

int fs_solve_residual(fs_sim* s, int b, int field, int prev, double a, double c, double out[4], double* per_plane)
{
    ENGINE_OR_RETURN(s); CHECK_B(b); CHECK_FIELD(field); CHECK_FIELD(prev);
    if (!out) return fail(FS_EINVAL, "null output");
    return ENG(s, residual.solve_residual(b, field, prev, a, c, out, per_plane));
}

int fs_diffuse_residual(fs_sim* s, int b, int field, int prev, double out[4], double* per_plane)
{
    ENGINE_OR_RETURN(s); CHECK_B(b); CHECK_FIELD(field); CHECK_FIELD(prev);
    if (!out) return fail(FS_EINVAL, "null output");
    return ENG(s, residual.diffuse_residual(b, field, prev, out, per_plane));
}

int fs_residual_log(fs_sim* s, double* rows, long max_rows, long* n_rows, long* n_dropped)
{
    ENGINE_OR_RETURN(s);
    return ENG(s, residual.log_fetch(rows, max_rows, n_rows, n_dropped));
}

int fs_flow_stats_sample(fs_sim* s) { ENGINE_OR_RETURN(s); return ENG(s, flow_stats.sample()); }
int fs_flow_stats_reset(fs_sim* s)
{
    if (!s) return fail(FS_EINVAL, "null handle");
    s->flow_stats_n = 0;
    return FS_OK;
}
int fs_flow_stats_field(fs_sim* s, int which, void* dst, size_t n_elems, int elem_size)
{
    ENGINE_OR_RETURN(s);
    if (!dst) return fail(FS_EINVAL, "null buffer");
    return ENG(s, flow_stats.field(which, dst, n_elems, elem_size));
}
int fs_flow_stats_dump(fs_sim* s, const char* dir)
{
    ENGINE_OR_RETURN(s);
    if (!dir) return fail(FS_EINVAL, "null directory");
    return ENG(s, flow_stats.dump(dir));
}

int fs_vortex_field(fs_sim* s, int which, void* dst, size_t n_elems, int elem_size)
{
    ENGINE_OR_RETURN(s);
    if (!dst) return fail(FS_EINVAL, "null buffer");
    return ENG(s, vortex.fetch(which, dst, n_elems, elem_size));
}
int fs_flow_monitor(fs_sim* s, double out[16], double* per_plane, double* x_profile)
{
    ENGINE_OR_RETURN(s);
    if (!out) return fail(FS_EINVAL, "null argument");
    return ENG(s, monitor.query(out, per_plane, x_profile));
}
int fs_monitor_sample(fs_sim* s) { ENGINE_OR_RETURN(s); return ENG(s, monitor.sample()); }
int fs_monitor_log(fs_sim* s, double* rows, long max_rows, long* n_rows, long* n_dropped)
{
    ENGINE_OR_RETURN(s);
    return ENG(s, monitor.log_fetch(rows, max_rows, n_rows, n_dropped));
}
int fs_confine_vorticity(fs_sim* s, double epsilon)
{
    ENGINE_OR_RETURN(s);
    return ENG(s, confine.vorticity(epsilon));
}
int fs_heat_params(fs_sim* s, const double* par, int n)
{
    ENGINE_OR_RETURN(s);
    if (!par) return fail(FS_EINVAL, "fs_heat_params: null argument");
    if (n != FS_HEAT_PARAMS) return fail(FS_EINVAL, "fs_heat_params: n = %d, the call takes FS_HEAT_PARAMS = %d numbers", n, FS_HEAT_PARAMS);
    static const char* const name[FS_HEAT_PARAMS] = { "mode", "kappa", "beta", "alpha", "up", "inlet temperature", "wall mode",
                                                      "wall temperature", "box x0", "box x1", "box y0", "box y1", "box z0", "box z1", "log" };
    for (int k = 0; k < FS_HEAT_PARAMS; ++k)
        if (!std::isfinite(par[k])) return fail(FS_EINVAL, "fs_heat_params: par[%d] (%s) is not finite", k, name[k]);
    auto whole = [&](int k, double lo, double hi) { return par[k] >= lo && par[k] <= hi && par[k] == std::floor(par[k]); };
    if (!whole(fs::HP_MODE, 0, 2)) return fail(FS_EINVAL, "fs_heat_params: par[0] (mode) is 0 (off), 1 (manual) or 2 (in fs_step)");
    for (int k : { fs::HP_KAPPA, fs::HP_BETA, fs::HP_ALPHA })
        if (!(par[k] >= 0.0)) return fail(FS_EINVAL, "fs_heat_params: par[%d] (%s) must be >= 0", k, name[k]);
    if (!whole(fs::HP_UP, 0, 5)) return fail(FS_EINVAL, "fs_heat_params: par[4] (up) is 0..5 = +x, -x, +y, -y, +z, -z");
    if (!whole(fs::HP_WALL, 0, 1)) return fail(FS_EINVAL, "fs_heat_params: par[6] (wall mode) is 0 or 1");
    const int ext[3] = { s->W, s->H, s->D };
    for (int a = 0; a < 3; ++a) {
        const int lo = fs::HP_X0 + 2 * a, hi = lo + 1;
        if (!whole(lo, 1, ext[a]) || !whole(hi, 1, ext[a]) || par[lo] > par[hi])
            return fail(FS_EINVAL, "fs_heat_params: par[%d], par[%d] (%s, %s) must be whole cells with 1 <= lo <= hi <= %d", lo, hi,
                        name[lo], name[hi], ext[a]);
    }
    if (!whole(fs::HP_LOG, 0, 1048576)) return fail(FS_EINVAL, "fs_heat_params: par[14] (log) is a record count 0 .. 2^20");
    return ENG(s, heat.config(par));
}
int fs_heat_params_get(fs_sim* s, double* par, int n)
{
    if (!s || !par) return fail(FS_EINVAL, "fs_heat_params_get: null argument");
    if (n != FS_HEAT_PARAMS) return fail(FS_EINVAL, "fs_heat_params_get: n = %d, the call fills FS_HEAT_PARAMS = %d numbers", n, FS_HEAT_PARAMS);
    for (int k = 0; k < FS_HEAT_PARAMS; ++k) par[k] = s->heat[k];
    return FS_OK;
}
int fs_heat_apply(fs_sim* s) { ENGINE_OR_RETURN(s); return ENG(s, heat.apply()); }
int fs_heat_transport(fs_sim* s) { ENGINE_OR_RETURN(s); return ENG(s, heat.transport()); }
int fs_heat_budget(fs_sim* s, double out[FS_HEAT_COLS], double* per_plane)
{
    ENGINE_OR_RETURN(s);
    if (!out) return fail(FS_EINVAL, "fs_heat_budget: null argument");
    return ENG(s, heat.budget(out, per_plane));
}
int fs_heat_log(fs_sim* s, double* rows, long max_rows, long* n_rows, long* n_dropped)
{
    ENGINE_OR_RETURN(s);
    return ENG(s, heat.log_fetch(rows, max_rows, n_rows, n_dropped));
}
int fs_heat_get(fs_sim* s, void* dst, size_t n_elems, int elem_size)
{
    ENGINE_OR_RETURN(s);
    if (!dst) return fail(FS_EINVAL, "fs_heat_get: null buffer");
    return ENG(s, heat.get(dst, n_elems, elem_size));
}
int fs_heat_set(fs_sim* s, const void* src, size_t n_elems, int elem_size)
{
    ENGINE_OR_RETURN(s);
    if (!src) return fail(FS_EINVAL, "fs_heat_set: null buffer");
    return ENG(s, heat.set(src, n_elems, elem_size));
}
int fs_zones(fs_sim* s, const double* par, int n_zones, int mode, int log)
{
    ENGINE_OR_RETURN(s);
    if (mode < 0 || mode > 2) return fail(FS_EINVAL, "fs_zones: mode = %d, it is 0 (off), 1 (manual) or 2 (in fs_step)", mode);
    if (n_zones < 0 || n_zones > FS_ZONE_MAX) return fail(FS_EINVAL, "fs_zones: n_zones = %d, a handle takes 0 .. FS_ZONE_MAX = %d zones", n_zones, FS_ZONE_MAX);
    if (log < 0 || log > 1048576) return fail(FS_EINVAL, "fs_zones: log = %d, it is a record count 0 .. 2^20", log);
    if (n_zones == 0 || mode == 0) return ENG(s, zones.config(nullptr, 0, 0, 0));
    if (!par) return fail(FS_EINVAL, "fs_zones: null argument");
    static const char* const name[FS_ZONE_PARAMS] = { "shape", "axis", "box x0", "box x1", "box y0", "box y1", "box z0", "box z1",
                                                      "centre 1", "centre 2", "radius", "g x", "g y", "g z", "D x", "D y", "D z",
                                                      "F x", "F y", "F z" };
    const int ext[3] = { s->W, s->H, s->D };
    for (int z = 0; z < n_zones; ++z) {
        const double* p = par + (size_t)z * FS_ZONE_PARAMS;
        for (int k = 0; k < FS_ZONE_PARAMS; ++k)
            if (!std::isfinite(p[k])) return fail(FS_EINVAL, "fs_zones: zone %d, par[%d] (%s) is not finite", z, k, name[k]);
        auto whole = [&](int k, double lo, double hi) { return p[k] >= lo && p[k] <= hi && p[k] == std::floor(p[k]); };
        if (!whole(fs::ZP_SHAPE, 0, 1)) return fail(FS_EINVAL, "fs_zones: zone %d, par[0] (shape) is 0 (box) or 1 (cylinder)", z);
        if (!whole(fs::ZP_AXIS, 0, 2)) return fail(FS_EINVAL, "fs_zones: zone %d, par[1] (axis) is 0, 1 or 2 = x, y, z", z);
        for (int a = 0; a < 3; ++a) {
            const int lo = fs::ZP_X0 + 2 * a, hi = lo + 1;
            if (!whole(lo, 1, ext[a]) || !whole(hi, 1, ext[a]) || p[lo] > p[hi])
                return fail(FS_EINVAL, "fs_zones: zone %d, par[%d], par[%d] (%s, %s) must be whole cells with 1 <= lo <= hi <= %d", z, lo,
                            hi, name[lo], name[hi], ext[a]);
        }
        for (int k : { (int)fs::ZP_RADIUS, (int)fs::ZP_DX, (int)fs::ZP_DY, (int)fs::ZP_DZ, (int)fs::ZP_FX, (int)fs::ZP_FY, (int)fs::ZP_FZ })
            if (!(p[k] >= 0.0)) return fail(FS_EINVAL, "fs_zones: zone %d, par[%d] (%s) must be >= 0", z, k, name[k]);
    }
    return ENG(s, zones.config(par, n_zones, mode, log));
}
int fs_zones_get(fs_sim* s, double* par, int* n_zones, int* mode, int* log)
{
    if (!s) return fail(FS_EINVAL, "fs_zones_get: null handle");
    if (par) memcpy(par, s->zones, (size_t)s->zone_n * FS_ZONE_PARAMS * sizeof(double));
    if (n_zones) *n_zones = s->zone_n;
    if (mode) *mode = s->zone_mode;
    if (log) *log = s->zone_log;
    return FS_OK;
}
int fs_zone_apply(fs_sim* s) { ENGINE_OR_RETURN(s); return ENG(s, zones.apply()); }
int fs_zone_budget(fs_sim* s, double* out, double* per_plane)
{
    ENGINE_OR_RETURN(s);
    if (!out) return fail(FS_EINVAL, "fs_zone_budget: null argument");
    return ENG(s, zones.budget(out, per_plane));
}
int fs_zone_log(fs_sim* s, double* rows, long max_rows, long* n_rows, long* n_dropped)
{
    ENGINE_OR_RETURN(s);
    return ENG(s, zones.log_fetch(rows, max_rows, n_rows, n_dropped));
}
int fs_zone_mask(fs_sim* s, uint8_t* dst, size_t n)
{
    ENGINE_OR_RETURN(s);
    if (!dst) return fail(FS_EINVAL, "fs_zone_mask: null buffer");
    return ENG(s, zones.mask(dst, n));
}
int fs_inflow_profile(fs_sim* s, const double* u, const double* rms, size_t n)
{
    if (!s) return fail(FS_EINVAL, "null handle");
    if (s->comm.active()) return fail(FS_EINVAL, "fs_inflow_profile: the inflow generator needs a single-GPU handle");
    const size_t want = (size_t)s->H * (size_t)s->D;
    if (n != want) return fail(FS_EINVAL, "fs_inflow_profile: %zu values given, the inlet plane has height * depth = %zu", n, want);
    for (const double* q : { u, rms })
        for (size_t i = 0; q && i < n; ++i)
            if (!std::isfinite(q[i])) return fail(FS_EINVAL, "fs_inflow_profile: entry %zu of the %s map is not finite", i, q == u ? "mean" : "scale");
    if (u) s->inflow_mean.assign(u, u + n); else s->inflow_mean.clear();
    if (rms) s->inflow_scale.assign(rms, rms + n); else s->inflow_scale.clear();
    s->inflow_gen++;
    return FS_OK;
}
int fs_inflow_gust(fs_sim* s, const double* steps, const double* factor, int n)
{
    if (!s) return fail(FS_EINVAL, "null handle");
    if (n < 0 || n > fs::INFLOW_KNOTS_MAX) return fail(FS_EINVAL, "fs_inflow_gust: 0 .. %d knots", fs::INFLOW_KNOTS_MAX);
    if (n > 0 && (!steps || !factor)) return fail(FS_EINVAL, "null argument");
    for (int i = 0; i < n; ++i) {
        if (!std::isfinite(steps[i]) || !std::isfinite(factor[i])) return fail(FS_EINVAL, "fs_inflow_gust: knot %d is not finite", i);
        if (i > 0 && !(steps[i] > steps[i - 1])) return fail(FS_EINVAL, "fs_inflow_gust: the step numbers must be strictly increasing (knot %d)", i);
    }
    s->gust_t.assign(steps, steps + n);
    s->gust_f.assign(factor, factor + n);
    return FS_OK;
}
int fs_inflow_plane(fs_sim* s, long step, double* out, size_t n)
{
    ENGINE_OR_RETURN(s);
    if (!out) return fail(FS_EINVAL, "null buffer");
    if (n != (size_t)3 * s->H * s->D) return fail(FS_EINVAL, "fs_inflow_plane: room for %zu values, the plane has 3 * height * depth = %zu", n, (size_t)3 * s->H * s->D);
    return ENG(s, inflow.plane(step, out));
}
int fs_inflow_eddies(fs_sim* s, long step, double* out, size_t n)
{
    ENGINE_OR_RETURN(s);
    if (n != (size_t)6 * s->inflow_n) return fail(FS_EINVAL, "fs_inflow_eddies: room for %zu values, there are 6 * %d", n, s->inflow_n);
    if (n == 0) return FS_OK;
    if (!out) return fail(FS_EINVAL, "null buffer");
    return ENG(s, inflow.eddies(step, out));
}
int fs_vortex_dump(fs_sim* s, const char* dir)
{
    ENGINE_OR_RETURN(s);
    if (!dir) return fail(FS_EINVAL, "null directory");
    return ENG(s, vortex.dump(dir));
}

int fs_sample_points(fs_sim* s, const double* xyz, long n)
{
    ENGINE_OR_RETURN(s);
    if (n < 0 || n > (1L << 24)) return fail(FS_EINVAL, "fs_sample_points: 0 .. 16777216 points, got %ld", n);
    if (n > 0 && !xyz) return fail(FS_EINVAL, "fs_sample_points: null points");
    return ENG(s, sampling.points(xyz, n));
}
int fs_sample(fs_sim* s, int source, int mode, double* out, long n)
{
    ENGINE_OR_RETURN(s);
    return ENG(s, sampling.sample(source, mode, out, n));
}
int fs_set_probes(fs_sim* s, const int* cells_xyz, long n)
{
    if (!s) return fail(FS_EINVAL, "null handle");
    if (n < 0 || n > FS_PROBE_MAX) return fail(FS_EINVAL, "fs_set_probes: 0 .. %d probes, got %ld", FS_PROBE_MAX, n);
    if (n > 0 && !cells_xyz) return fail(FS_EINVAL, "fs_set_probes: null cells");
    for (long k = 0; k < n; ++k) {
        const int x = cells_xyz[3 * k], y = cells_xyz[3 * k + 1], z = cells_xyz[3 * k + 2];
        if (x < 0 || x > s->W + 1 || y < 0 || y > s->H + 1 || z < 0 || z > s->D + 1)
            return fail(FS_EINVAL, "fs_set_probes: cell %ld (%d,%d,%d) outside 0..%dx0..%dx0..%d", k, x, y, z, s->W + 1, s->H + 1, s->D + 1);
    }
    if ((size_t)s->probe_log * (size_t)n * FS_PROBE_VALUES * sizeof(double) > ((size_t)1 << 30))
        return fail(FS_EINVAL, "fs_set_probes: %d records (\"probe_log\") of %ld probes exceed 1 GiB", s->probe_log, n);
    s->probes.assign(cells_xyz, cells_xyz + 3 * n);
    s->probe_gen++;
    return FS_OK;
}
int fs_probe_sample(fs_sim* s) { ENGINE_OR_RETURN(s); return ENG(s, sampling.probe_sample()); }
int fs_probe_log(fs_sim* s, double* rows, long max_rows, long* n_rows, long* n_dropped)
{
    ENGINE_OR_RETURN(s);
    return ENG(s, sampling.probe_log_fetch(rows, max_rows, n_rows, n_dropped));
}

// ---- slice and projection images ------------------------------------------------------------------------------
int fs_image_values(fs_sim* s, int source, int kind, int axis, int index, double* out, size_t n, int* cols, int* rows)
{
    ENGINE_OR_RETURN(s);
    return ENG(s, images.values(source, kind, axis, index, out, n, cols, rows));
}
int fs_image_rgb(fs_sim* s, int source, int kind, int axis, int index, double vmin, double vmax, double obstacle_alpha,
                 uint8_t* out, size_t n_bytes, int* cols, int* rows)
{
    ENGINE_OR_RETURN(s);
    return ENG(s, images.rgb(source, kind, axis, index, vmin, vmax, obstacle_alpha, out, n_bytes, cols, rows));
}
int fs_image_colormap(fs_sim* s, const uint8_t* rgb, int n)
{
    if (!s) return fail(FS_EINVAL, "null handle");
    if (n != 0 && (n < 2 || n > fs::IMG_TABLE_MAX)) return fail(FS_EINVAL, "fs_image_colormap: 2 .. %d triples (0: the built-in table), got %d", fs::IMG_TABLE_MAX, n);
    if (n > 0 && !rgb) return fail(FS_EINVAL, "fs_image_colormap: null table");
    if (n == 0) s->image_table.clear();
    else s->image_table.assign(rgb, rgb + 3 * (size_t)n);
    s->image_table_gen++;
    return FS_OK;
}
int fs_image_views(fs_sim* s, const int* spec, const double* range, int n)
{
    if (!s) return fail(FS_EINVAL, "null handle");
    if (n < 0 || n > FS_IMAGE_VIEWS_MAX) return fail(FS_EINVAL, "fs_image_views: 0 .. %d views, got %d", FS_IMAGE_VIEWS_MAX, n);
    if (n > 0 && (!spec || !range)) return fail(FS_EINVAL, "fs_image_views: null views");
    if (n > 0 && s->comm.active()) return fail(FS_EINVAL, "fs_image_views: images are taken on a single-GPU handle");
    std::vector<ImageView> views((size_t)n);
    for (int k = 0; k < n; ++k) {
        ImageView& v = views[(size_t)k];
        v.source = spec[4 * k]; v.kind = spec[4 * k + 1]; v.axis = spec[4 * k + 2]; v.index = spec[4 * k + 3];
        v.vmin = range[3 * k]; v.vmax = range[3 * k + 1]; v.alpha = range[3 * k + 2];
        if (!image_source_ok(v.source)) return fail(FS_EINVAL, "fs_image_views: view %d: unknown source %d", k, v.source);
        if (v.kind < 0 || v.kind >= fs::IMG_NKINDS) return fail(FS_EINVAL, "fs_image_views: view %d: unknown kind %d", k, v.kind);
        if (v.axis < 0 || v.axis > 2) return fail(FS_EINVAL, "fs_image_views: view %d: axis %d (0 = x, 1 = y, 2 = z)", k, v.axis);
        const int N = v.axis == 0 ? s->W : v.axis == 1 ? s->H : s->D;
        if (v.index < 0 || v.index > (v.kind == fs::IMG_SLICE ? N + 1 : 0))
            return fail(FS_EINVAL, "fs_image_views: view %d: index %d (a slice: 0 .. %d; a projection: 0)", k, v.index, N + 1);
        if (!image_range_ok(v.vmin, v.vmax, v.alpha))
            return fail(FS_EINVAL, "fs_image_views: view %d: vmin < vmax, both finite, and obstacle_alpha in [0, 1]", k);
    }
    if ((size_t)s->image_log * image_frame_bytes(s, views) > ((size_t)1 << 30))
        return fail(FS_EINVAL, "fs_image_views: %d frames (\"image_log\") of %zu bytes exceed 1 GiB", s->image_log, image_frame_bytes(s, views));
    s->image_views.swap(views);
    s->image_gen++;
    if (s->eng) {
        hipSetDevice(s->device);
        return ENG(s, images.config());
    }
    return FS_OK;
}
int fs_image_sample(fs_sim* s) { ENGINE_OR_RETURN(s); return ENG(s, images.sample()); }
int fs_image_log(fs_sim* s, uint8_t* frames, long* steps, long max_frames, long* n_frames, long* n_dropped)
{
    ENGINE_OR_RETURN(s);
    return ENG(s, images.log_fetch(frames, steps, max_frames, n_frames, n_dropped));
}

// ---- volume rendering -------------------------------------------------------------------------------------------------------
namespace {
bool volume_slot_used(const fs_sim* s, int slot)
{
    for (const VolumeLogView& v : s->volume_views)
        if (v.slot == slot) return true;
    return false;
}
// the checks and the bookkeeping around a slot's new ray set; `who`: the entry
int volume_set_rays(fs_sim* s, const char* who, int slot, const double* rays, int cols, int rows)
{
    const bool used = volume_slot_used(s, slot);
    if (cols == 0 && used) return fail(FS_EINVAL, "%s: slot %d is used by a view of the volume log (fs_volume_views)", who, slot);
    if (used && (size_t)s->volume_log * volume_frame_bytes(s, s->volume_views, slot, cols, rows) > ((size_t)1 << 30))
        return fail(FS_EINVAL, "%s: %d frames (\"volume_log\") of %zu bytes exceed 1 GiB", who, s->volume_log,
                    volume_frame_bytes(s, s->volume_views, slot, cols, rows));
    const int rc = ENG(s, volume.set_rays(slot, rays, cols, rows));
    if (rc) return rc;
    s->vol_cols[slot] = cols;
    s->vol_rows[slot] = rows;
    if (!used) return FS_OK;
    s->volume_gen++;                                     // a view uses the slot: the log is cleared
    return ENG(s, volume.config());
}
int volume_rays_args(fs_sim* s, const char* who, int slot, int cols, int rows, bool may_free)
{
    if (s->comm.active()) return fail(FS_EINVAL, "%s: volumes are rendered on a single-GPU handle", who);
    if (slot < 0 || slot >= FS_VOLUME_CAMERAS_MAX) return fail(FS_EINVAL, "%s: slot %d (0 .. %d)", who, slot, FS_VOLUME_CAMERAS_MAX - 1);
    if (may_free && cols == 0 && rows == 0) return FS_OK;
    if (cols < 1 || cols > fs::VOLUME_SIZE_MAX || rows < 1 || rows > fs::VOLUME_SIZE_MAX)
        return fail(FS_EINVAL, "%s: %d x %d rays (1 .. %d each%s)", who, cols, rows, fs::VOLUME_SIZE_MAX, may_free ? "; 0 x 0 frees the slot" : "");
    return FS_OK;
}
}  // namespace

int fs_volume_rays(fs_sim* s, int slot, const double* rays, int cols, int rows)
{
    ENGINE_OR_RETURN(s);
    const int rc = volume_rays_args(s, "fs_volume_rays", slot, cols, rows, true);
    if (rc) return rc;
    if (cols > 0 && !rays) return fail(FS_EINVAL, "fs_volume_rays: null rays");
    return volume_set_rays(s, "fs_volume_rays", slot, rays, cols, rows);
}
int fs_volume_camera(fs_sim* s, int slot, const double* cam, int cols, int rows)
{
    ENGINE_OR_RETURN(s);
    const int rc = volume_rays_args(s, "fs_volume_camera", slot, cols, rows, false);
    if (rc) return rc;
    if (!cam) return fail(FS_EINVAL, "fs_volume_camera: null camera");
    fs::VolumeCamera c;
    if (!fs::volume_camera_basis(cam, c))
        return fail(FS_EINVAL, "fs_volume_camera: every entry finite, half_height > 0, target != eye, and up not along the view direction");
    std::vector<double> rays((size_t)cols * (size_t)rows * 6);
    for (int i = 0; i < rows; ++i)
        for (int j = 0; j < cols; ++j) fs::volume_camera_ray(c, cols, rows, i, j, &rays[6 * ((size_t)i * (size_t)cols + (size_t)j)]);
    return volume_set_rays(s, "fs_volume_camera", slot, rays.data(), cols, rows);
}
int fs_volume_render(fs_sim* s, int source, int slot, const double* par, uint8_t* rgb, size_t n_bytes, double* acc, size_t n_acc)
{
    ENGINE_OR_RETURN(s);
    if (s->comm.active()) return fail(FS_EINVAL, "fs_volume_render: volumes are rendered on a single-GPU handle");
    if (slot < 0 || slot >= FS_VOLUME_CAMERAS_MAX) return fail(FS_EINVAL, "fs_volume_render: slot %d (0 .. %d)", slot, FS_VOLUME_CAMERAS_MAX - 1);
    if (s->vol_cols[slot] == 0) return fail(FS_EINVAL, "fs_volume_render: slot %d holds no rays (fs_volume_rays, fs_volume_camera)", slot);
    if (!par) return fail(FS_EINVAL, "fs_volume_render: null parameters");
    if (!fs::volume_params_ok(par, s->W, s->H, s->D, nullptr))
        return fail(FS_EINVAL, "fs_volume_render: vmin < vmax, opacity >= 0, step > 0 with (box diagonal) / step <= %d, 0 <= t_min < 1, colours in [0, 255], all finite", FS_VOLUME_SAMPLES_MAX);
    if (!image_source_ok(source)) return fail(FS_EINVAL, "fs_volume_render: unknown source %d", source);
    const size_t npix = (size_t)s->vol_cols[slot] * (size_t)s->vol_rows[slot];
    if (rgb && n_bytes != 3 * npix)
        return fail(FS_EINVAL, "fs_volume_render: the image has %d x %d x 3 bytes, the call has room for %zu", s->vol_cols[slot], s->vol_rows[slot], n_bytes);
    if (acc && n_acc != 4 * npix)
        return fail(FS_EINVAL, "fs_volume_render: the image has %d x %d x 4 values, the call has room for %zu", s->vol_cols[slot], s->vol_rows[slot], n_acc);
    return ENG(s, volume.render(source, slot, par, rgb, n_bytes, acc, n_acc));
}
int fs_volume_views(fs_sim* s, const int* spec, const double* par, int n)
{
    if (!s) return fail(FS_EINVAL, "null handle");
    if (n < 0 || n > FS_VOLUME_VIEWS_MAX) return fail(FS_EINVAL, "fs_volume_views: 0 .. %d views, got %d", FS_VOLUME_VIEWS_MAX, n);
    if (n > 0 && (!spec || !par)) return fail(FS_EINVAL, "fs_volume_views: null views");
    if (n > 0 && s->comm.active()) return fail(FS_EINVAL, "fs_volume_views: volumes are rendered on a single-GPU handle");
    std::vector<VolumeLogView> views((size_t)n);
    for (int k = 0; k < n; ++k) {
        VolumeLogView& v = views[(size_t)k];
        v.source = spec[2 * k];
        v.slot = spec[2 * k + 1];
        for (int j = 0; j < FS_VOLUME_PARAMS; ++j) v.par[j] = par[FS_VOLUME_PARAMS * k + j];
        if (!image_source_ok(v.source)) return fail(FS_EINVAL, "fs_volume_views: view %d: unknown source %d", k, v.source);
        if (v.slot < 0 || v.slot >= FS_VOLUME_CAMERAS_MAX) return fail(FS_EINVAL, "fs_volume_views: view %d: slot %d (0 .. %d)", k, v.slot, FS_VOLUME_CAMERAS_MAX - 1);
        if (s->vol_cols[v.slot] == 0) return fail(FS_EINVAL, "fs_volume_views: view %d: slot %d holds no rays (fs_volume_rays, fs_volume_camera)", k, v.slot);
        if (!fs::volume_params_ok(v.par, s->W, s->H, s->D, nullptr)) return fail(FS_EINVAL, "fs_volume_views: view %d: bad parameters (see fs_volume_render)", k);
    }
    if ((size_t)s->volume_log * volume_frame_bytes(s, views) > ((size_t)1 << 30))
        return fail(FS_EINVAL, "fs_volume_views: %d frames (\"volume_log\") of %zu bytes exceed 1 GiB", s->volume_log, volume_frame_bytes(s, views));
    s->volume_views.swap(views);
    s->volume_gen++;
    if (s->eng) {
        hipSetDevice(s->device);
        return ENG(s, volume.config());
    }
    return FS_OK;
}
int fs_volume_sample(fs_sim* s) { ENGINE_OR_RETURN(s); return ENG(s, volume.sample()); }
int fs_volume_log(fs_sim* s, uint8_t* frames, long* steps, long max_frames, long* n_frames, long* n_dropped)
{
    ENGINE_OR_RETURN(s);
    return ENG(s, volume.log_fetch(frames, steps, max_frames, n_frames, n_dropped));
}

// ---- tracer particles -----------------------------------------------------------------------------------------------------
namespace {
bool tracer_points_ok(const fs_sim* s, const double* xyz, long n, long* bad)
{
    for (long k = 0; k < n; ++k)
        if (!fs::tracer_in_box(xyz + 3 * k, s->W, s->H, s->D)) { *bad = k; return false; }
    return true;
}
}  // namespace
int fs_tracer_seed(fs_sim* s, const double* xyz, long n)
{
    ENGINE_OR_RETURN(s);
    if (s->comm.active()) return fail(FS_EINVAL, "fs_tracer_seed: tracers need a single-GPU handle");
    if (n < 0 || n > (1L << 24)) return fail(FS_EINVAL, "fs_tracer_seed: 0 .. 16777216 points, got %ld", n);
    if (n > 0 && !xyz) return fail(FS_EINVAL, "fs_tracer_seed: null points");
    long bad = 0;
    if (!tracer_points_ok(s, xyz, n, &bad))
        return fail(FS_EINVAL, "fs_tracer_seed: point %ld (%g,%g,%g) outside 0.5..%d.5 x 0.5..%d.5 x 0.5..%d.5", bad, xyz[3 * bad],
                    xyz[3 * bad + 1], xyz[3 * bad + 2], s->W, s->H, s->D);
    return ENG(s, tracers.seed(xyz, n));
}
int fs_tracer_emitters(fs_sim* s, const double* xyz, long n, long every)
{
    if (!s) return fail(FS_EINVAL, "null handle");
    if (s->comm.active()) return fail(FS_EINVAL, "fs_tracer_emitters: tracers need a single-GPU handle");
    if (n < 0 || n > FS_TRACER_EMITTERS_MAX) return fail(FS_EINVAL, "fs_tracer_emitters: 0 .. %d emitters, got %ld", FS_TRACER_EMITTERS_MAX, n);
    if (n > 0 && !xyz) return fail(FS_EINVAL, "fs_tracer_emitters: null points");
    if (every < 1 || every > (1L << 30)) return fail(FS_EINVAL, "fs_tracer_emitters: every >= 1, got %ld", every);
    long bad = 0;
    if (!tracer_points_ok(s, xyz, n, &bad))
        return fail(FS_EINVAL, "fs_tracer_emitters: point %ld (%g,%g,%g) outside 0.5..%d.5 x 0.5..%d.5 x 0.5..%d.5", bad, xyz[3 * bad],
                    xyz[3 * bad + 1], xyz[3 * bad + 2], s->W, s->H, s->D);
    s->tracer_emit.assign(xyz, xyz + 3 * n);
    s->tracer_emit_every = every;
    s->tracer_emit_gen++;
    return FS_OK;
}
int fs_tracer_clear(fs_sim* s) { ENGINE_OR_RETURN(s); return ENG(s, tracers.clear()); }
int fs_tracer_advance(fs_sim* s) { ENGINE_OR_RETURN(s); return ENG(s, tracers.advance()); }
int fs_tracer_fetch(fs_sim* s, double* xyz, int32_t* meta, long max, long* n)
{
    ENGINE_OR_RETURN(s);
    return ENG(s, tracers.fetch(xyz, meta, max, n));
}
int fs_tracer_sample(fs_sim* s, int source, int mode, double* out, long n)
{
    ENGINE_OR_RETURN(s);
    return ENG(s, tracers.sample(source, mode, out, n));
}
int fs_tracer_log(fs_sim* s, double* xyz, int32_t* status, long* steps, long max_frames, long* n_frames, long* n_dropped)
{
    ENGINE_OR_RETURN(s);
    return ENG(s, tracers.log_fetch(xyz, status, steps, max_frames, n_frames, n_dropped));
}

// An 8-bit RGB, non-interlaced PNG whose one IDAT chunk is a zlib stream of stored deflate blocks: filter type 0 on every
// scanline, no compression, no zlib dependency; the bytes are a pure function of the pixels.
int fs_image_png(const uint8_t* rgb, int cols, int rows, const char* path)
{
    if (!rgb || !path) return fail(FS_EINVAL, "fs_image_png: null argument");
    if (cols < 1 || rows < 1 || (double)cols * rows * 3 + rows > 1.0e9) return fail(FS_EINVAL, "fs_image_png: bad size %d x %d", cols, rows);
    uint32_t crc_table[256];
    for (uint32_t n = 0; n < 256; ++n) {
        uint32_t c = n;
        for (int k = 0; k < 8; ++k) c = (c & 1) ? 0xEDB88320u ^ (c >> 1) : c >> 1;
        crc_table[n] = c;
    }
    std::vector<uint8_t> file;
    auto be32 = [&](uint32_t v) { for (int k = 3; k >= 0; --k) file.push_back((uint8_t)(v >> (8 * k))); };
    auto chunk = [&](const char* type, const std::vector<uint8_t>& data) {
        be32((uint32_t)data.size());
        const size_t from = file.size();
        file.insert(file.end(), type, type + 4);
        file.insert(file.end(), data.begin(), data.end());
        uint32_t c = 0xFFFFFFFFu;
        for (size_t k = from; k < file.size(); ++k) c = crc_table[(c ^ file[k]) & 0xFF] ^ (c >> 8);
        be32(c ^ 0xFFFFFFFFu);
    };
    static const uint8_t magic[8] = {0x89, 'P', 'N', 'G', '\r', '\n', 0x1A, '\n'};
    file.assign(magic, magic + 8);
    std::vector<uint8_t> ihdr;
    for (uint32_t v : { (uint32_t)cols, (uint32_t)rows })
        for (int k = 3; k >= 0; --k) ihdr.push_back((uint8_t)(v >> (8 * k)));
    for (uint8_t b : { 8, 2, 0, 0, 0 }) ihdr.push_back(b);      // bit depth 8, colour type 2 (RGB), deflate, filter method 0, no interlace
    chunk("IHDR", ihdr);
    // the scanlines, each behind its filter byte 0
    const size_t line = 3 * (size_t)cols;
    std::vector<uint8_t> raw((line + 1) * (size_t)rows);
    for (int r = 0; r < rows; ++r) {
        raw[(line + 1) * (size_t)r] = 0;
        memcpy(&raw[(line + 1) * (size_t)r + 1], rgb + line * (size_t)r, line);
    }
    uint32_t a = 1, b = 0;                               // Adler-32 of the uncompressed data
    for (size_t k = 0; k < raw.size();) {
        const size_t run = std::min<size_t>(raw.size() - k, 5552);
        for (size_t j = 0; j < run; ++j) { a += raw[k + j]; b += a; }
        a %= 65521u;
        b %= 65521u;
        k += run;
    }
    std::vector<uint8_t> idat;
    idat.push_back(0x78);                                // deflate, 32 KiB window
    idat.push_back(0x01);                                // no dictionary, fastest; 0x7801 is a multiple of 31
    for (size_t k = 0; k < raw.size();) {
        const size_t run = std::min<size_t>(raw.size() - k, 65535);
        idat.push_back(k + run == raw.size() ? 1 : 0);   // BFINAL, BTYPE = 00 (stored)
        idat.push_back((uint8_t)(run & 0xFF));
        idat.push_back((uint8_t)(run >> 8));
        idat.push_back((uint8_t)(~run & 0xFF));
        idat.push_back((uint8_t)((~run >> 8) & 0xFF));
        idat.insert(idat.end(), raw.begin() + (long)k, raw.begin() + (long)(k + run));
        k += run;
    }
    const uint32_t adler = (b << 16) | a;
    for (int k = 3; k >= 0; --k) idat.push_back((uint8_t)(adler >> (8 * k)));
    chunk("IDAT", idat);
    chunk("IEND", std::vector<uint8_t>());
    FILE* fp = fopen(path, "wb");
    if (!fp) return fail(FS_EIO, "fs_image_png: cannot open '%s'", path);
    const bool ok = fwrite(file.data(), 1, file.size(), fp) == file.size();
    if (fclose(fp) != 0 || !ok) return fail(FS_EIO, "fs_image_png: cannot write '%s'", path);
    return FS_OK;
}

int fs_comm_unique_id(void* id_out)
{
    if (!id_out) return fail(FS_EINVAL, "null id buffer");
    std::string err;
    if (fs::Comm::unique_id(id_out, &err)) return fail(FS_ECOMM, "%s", err.c_str());
    return FS_OK;
}

int fs_comm_selftest(void)
{
    std::string err;
    hipStream_t st = nullptr;
    HIP_TRY(hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
    int rc = fs::Comm::selftest(st, &err);
    hipStreamDestroy(st);
    if (rc) return fail(FS_ECOMM, "RCCL self-test: %s", err.c_str());
    return FS_OK;
}

int fs_comm_init(fs_sim* s, int rank, int nranks, const void* id)
{
    if (!s || !id) return fail(FS_EINVAL, "null argument");
    if (s->eng) return fail(FS_EINVAL, "fs_comm_init must precede first use of the handle");
    if (nranks < 1 || rank < 0 || rank >= nranks) return fail(FS_EINVAL, "bad rank %d of %d", rank, nranks);
    if (s->D % nranks) return fail(FS_EINVAL, "depth %d does not divide over %d slabs", s->D, nranks);
    if (nranks > 1 && s->D / nranks < 2) return fail(FS_EINVAL, "a slab needs at least 2 planes (two-deep halos), got %d", s->D / nranks);
    if (nranks == 1) return FS_OK;
    if (s->body_log > 0) return fail(FS_EINVAL, "fs_comm_init: option \"body_force_log\" is on, and bodies are labelled on a single-GPU handle");
    if (s->image_log > 0 && !s->image_views.empty()) return fail(FS_EINVAL, "fs_comm_init: the image log is on, and images are taken on a single-GPU handle");
    if (s->volume_log > 0) return fail(FS_EINVAL, "fs_comm_init: option \"volume_log\" is on, and volumes are rendered on a single-GPU handle");
    if (s->monitor_log > 0) return fail(FS_EINVAL, "fs_comm_init: option \"monitor_log\" is on, and the flow monitor needs a single-GPU handle");
    if (s->tracers > 0) return fail(FS_EINVAL, "fs_comm_init: option \"tracers\" is on, and tracers move on a single-GPU handle");
    hipSetDevice(s->device);
    if (s->comm.init(rank, nranks, id)) return fail(FS_ECOMM, "%s", s->comm.last_error());
    if (rank == 0 && !s->quiet)          // one line of provenance for multi-GPU logs
        fprintf(stderr, "fluidsim: %d z-slabs of %d planes, halo transport: %s\n", nranks, s->D / nranks, s->comm.transport_name());
    return FS_OK;
}

const char* fs_comm_transport(fs_sim* s)
{
    if (!s) return "";
    return s->comm.active() ? s->comm.transport_name() : "single GPU";
}

}  // extern "C"
