// driver/common.h -- what the core of the host driver (fluidsim.cpp) and every part of it (driver/*.h) need: the error
// text, the timing families and spans, the handle, the device buffer and the ring of a per-step log.
#pragma once
#include "../../../include/fluidsim.h"
#include "../kernels.h"
#include "../comm.h"
#include "../dump.h"
#include "../image.h"
#include "../volume.h"
#include "../monitor.h"
#include "../heat.h"
#include "../zones.h"
#include "../step_ring.h"

#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <chrono>
#include <cerrno>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <exception>
#include <limits>
#include <string>
#include <type_traits>
#include <vector>

namespace {

thread_local std::string g_err;

int fail(int code, const char* fmt, ...)
{
    char buf[1024];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_err = buf;
    return code;
}

#define HIP_TRY(expr)                                                                             \
    do {                                                                                          \
        hipError_t e_ = (expr);                                                                   \
        if (e_ != hipSuccess) return fail(FS_EHIP, "%s: %s (%s:%d)", #expr, hipGetErrorString(e_), __FILE__, __LINE__); \
    } while (0)

enum Family { FAM_SWEEP = 0, FAM_PAIR, FAM_TRIPLE, FAM_DIV, FAM_GRAD, FAM_ADVECT, FAM_BOUNDS, FAM_MISC, FAM_COMM, FAM_MG, FAM_FORCES, FAM_RESIDUAL, FAM_FLOWSTATS, FAM_VORTEX, FAM_PROBES, FAM_BODYFORCES, FAM_IMAGES, FAM_TRACERS, FAM_VOLUME, FAM_CONFINE, FAM_MONITOR, FAM_INFLOW, FAM_HEAT, FAM_ZONES, FAM_COUNT };
// the names: two tables that stay in fluidsim.cpp (tests/test_inflow_cpu.py reads the first one's text there)
extern const char* const kFamilyNames[FAM_HEAT];
extern const char* const kLaterFamilyNames[FAM_COUNT - FAM_HEAT];
inline const char* family_name(int f) { return f < FAM_HEAT ? kFamilyNames[f] : kLaterFamilyNames[f - FAM_HEAT]; }

constexpr int NPOOL = FS_NFIELDS + 3;   // named fields + ping-pong scratch
// heat (heat.h): two more slots of the engine's slot table behind the public fields -- the temperature and its pre-solve
// snapshot -- and two more arrays in the pool while heat is on
constexpr int NHEAT = 2, NSLOT = FS_NFIELDS + NHEAT, NPOOL_MAX = NPOOL + NHEAT;
constexpr int F_THETA = FS_NFIELDS, F_THETA_PREV = FS_NFIELDS + 1;
static_assert(fs::HEAT_PARAMS == FS_HEAT_PARAMS && fs::HEAT_COLS == FS_HEAT_COLS && FS_HEAT_LOG_COLS == 1 + FS_HEAT_COLS, "heat.h restates the header");
static_assert(fs::ZONE_PARAMS == FS_ZONE_PARAMS && fs::ZONE_COLS == FS_ZONE_COLS && fs::ZONE_MAX == FS_ZONE_MAX, "zones.h restates the header");

struct Span {
    hipEvent_t a, b;
    int fam;
    long launches;
};

}  // namespace

// what fs_sim holds of its engine; the C entries reach Engine<float> or Engine<double> through ENG (fluidsim.cpp)
struct EngineBase {
    virtual ~EngineBase() {}
};

// one view of the image log (fs_image_views)
struct ImageView {
    int source, kind, axis, index;
    double vmin, vmax, alpha;
};

// one view of the volume log (fs_volume_views)
struct VolumeLogView {
    int source, slot;
    double par[fs::VOLUME_PARAMS];
};

struct fs_sim {
    // Simulation's public members (simulation.h:44-54); W/H/D are the GLOBAL extents
    int W = 0, H = 0, D = 0, iter = 0, speed = 0, acc = 0;
    float dt = 0, diff = 0, visc = 0;
    // options
    bool fp64 = false;
    int solver = FS_SOLVER_JACOBI;
    float omega = 1.0f;          // relaxation factor of solver=rbsor
    int replay_two = -2, replay_three = -2;   // "launch_plans": replay these plan ids instead of timing (-2: not set)
    int mg_cycles = 4, mg_pre = 1, mg_post = 1, mg_coarse = 30;   // solver=mg: V-cycles per pressure solve, smoothing steps, coarsest-level iterations
    int mg_min_planes = 32;      // z-slabs: a coarse level stays distributed while every rank keeps at least this many of its planes
                                 // (measured, 512^3 as four slabs: 4 -> 203, 16 -> 186, 32 -> 175, 64 -> 152 ms per step; below 32 the
                                 // exchanges of a level cost more than computing it whole on every rank, above it the whole-held level
                                 // of an 8-way split is as large as a rank's own slab)
    std::string dump_dir = "data";
    int dump_every = 1;
    unsigned voxel_seed = 1;
    bool quiet = false, profile = false, elide_dead = false;
    bool fuse_advect = true;     // one kernel for the three velocity advections of a step (single GPU)
    // "zero_start" / "fuse_project_advect": -1 = auto, 0, 1.  What auto means is decided by measurement.
    int zero_start = -1;         // project(): the divergence pass does not zero p in memory, the first pass of the solve takes zeros
    int z_alternate = -1;        // fs_set_int, -1 = auto, 0, 1.  Solves: a three-sweep pass behind an upward one marches downward in z (sweep_fused.hip, ZREV)
    int fuse_project_advect = -1;   // step(): the first projection's gradient pass runs inside the velocity advection's kernel
    double confinement = 0.0;    // "vorticity_confinement": strength of the confinement pass at the start of a step, 0 = off
    long n_confine = 0;          // confinement passes done, inside steps and by fs_confine_vorticity (fs_get_int)
    // heat and buoyancy (heat.h): the parameters as fs_heat_params last set them; mode 0 = off, 1 = manual, 2 = in fs_step
    double heat[fs::HEAT_PARAMS] = {0, 0, 0, 0, 2, 0, 0, 0, 1, 1, 1, 1, 1, 1, 0};
    int heat_mode() const { return (int)heat[fs::HP_MODE]; }
    long n_heat_apply = 0, n_heat_transport = 0;   // passes done, inside steps and by fs_heat_apply / fs_heat_transport (fs_get_int)
    // momentum zones (zones.h): the rows as fs_zones last set them; mode 0 = off, 1 = manual, 2 = in fs_step
    double zones[fs::ZONE_MAX * fs::ZONE_PARAMS] = {0};
    int zone_n = 0, zone_mode = 0, zone_log = 0;
    long n_zone_apply = 0;       // passes done, inside steps and by fs_zone_apply (fs_get_int)
    // turbulent inflow (inflow.h): with "inflow" on, fs_step writes the x = 1 face from these instead of (speed, 0, 0)
    bool inflow = false;
    int inflow_n = 0;            // "inflow_eddies"
    double inflow_sigma = 4.0, inflow_rms = 0.0;   // "inflow_sigma", "inflow_rms"
    double inflow_convect = -1.0;   // "inflow_convect": cells per step, < 0 = "auto" (dt * width * speed)
    uint64_t inflow_seed = 1;
    std::vector<double> inflow_mean, inflow_scale;   // fs_inflow_profile: h x d each, empty = speed everywhere / 1 everywhere
    std::vector<double> gust_t, gust_f;              // fs_inflow_gust: the knots
    long inflow_gen = 0;         // bumped by fs_inflow_profile: the maps are uploaded anew
    long n_inflow = 0;           // planes written by steps ("inflow_passes")
    double inflow_convect_now() const { return inflow_convect < 0.0 ? ((double)dt * (double)W) * (double)speed : inflow_convect; }
    long n_zero_start = 0, n_project_advect = 0;   // projections / steps that took those paths (fs_get_int)
    long n_reversed = 0;         // three-sweep passes that marched downward ("reversed_passes")
    int overlap = -1;            // z-slabs, how a pass and its halo exchange are scheduled: 0 the pass, then the exchange; 1 boundary
                                 // planes first, their exchange on the communication stream while the interior is computed; 2 boundary
                                 // launch + exchange on the communication stream beside the interior launch; -1 (default) = "auto":
                                 // the three are timed once over the real transport, the slowest rank's time decides (all ranks agree)
    int comm_cus = 0;            // z-slabs: CUs kept free of solver workgroups (the compute stream gets a CU mask) so that the
                                 // transport's kernels find room beside a launch that fills the chip; -1 = "auto": 0 and 8 are timed
    bool split_dens = true;      // z-slabs: run half of the (dead) density solve between the first projection and the velocity
                                 // advection, so that the reach of the back-trace arrives on the host without stalling the device
    // slab-step bookkeeping readable through fs_get_int
    long n_stream_syncs = 0;     // host synchronisations of the compute stream issued by the slab step (reach fallback path)
    long n_alloc_syncs = 0;      // ... by one-off allocations inside a step (the gathered sources at the first gather)
    long n_reach_waits = 0, n_reach_blocked = 0;   // waits for an asynchronously delivered reach; those that found it not yet there
    long n_reach_hidden = 0, n_reach_exposed = 0;  // gathers + advections queued while the device was still busy with the half density
                                                   // solve placed before them (hidden) / after it had run dry (exposed: a bubble)
    double reach_wait_ms = 0.0;  // host time spent in them
    int overlap_plan = -1, cus_plan = -1;          // what "auto" chose (or the forced values), -1 before the first slab solve
    double overlap_ms[8] = {0, 0, 0, 0, 0, 0, 0, 0};   // slowest rank's ms per pass of each timed candidate (overlap 0..3 x cu mask off/on)
    bool debug_poison = false;   // fill the gathered advection source with NaN bit patterns before each gather
    int last_reach = 0;          // planes of reach used by the most recent slab advection
    // device
    int device = 0;
    hipStream_t stream = nullptr;
    hipStream_t stream_full = nullptr, stream_masked = nullptr;   // z-slabs with comm_cus: `stream` is one of these two
    EngineBase* eng = nullptr;
    // z-slab partition (comm.h)
    fs::Comm comm;
    // timing
    std::vector<Span> spans;
    std::vector<hipEvent_t> event_pool;
    double fam_ms[FAM_COUNT] = {0};
    long fam_launches[FAM_COUNT] = {0};
    // dumps
    FILE* dump_fp[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
    bool dump_open = false, dump_warned = false, in_run = false;
    long step_no = 0;
    long steps_total = 0;        // steps this handle has completed (the "step" column of fs_force_log)
    int force_log = 0;           // "force_log": steps the per-step force log keeps, 0 = off
    long force_log_gen = 0;      // bumped by every fs_set_option("force_log"): the ring is reallocated and cleared
    int residual_log = 0;        // "residual_log": steps the per-step residual log keeps, 0 = off
    long residual_log_gen = 0;   // bumped by every fs_set_option("residual_log")
    int flow_stats = 0;          // "flow_stats": accumulators per cell, 0 = off, 5 = "mean", 12 = "moments" (flow_stats.h)
    long flow_stats_gen = 0;     // bumped by every fs_set_option("flow_stats"): the accumulators are (re)allocated and cleared
    long flow_stats_every = 1, flow_stats_start = 0;   // fs_step samples when steps_total > start and (steps_total - start - 1) % every == 0
    long flow_stats_n = 0;       // samples taken since the last reset
    std::vector<int> probes;     // fs_set_probes: x, y, z per probe, padded global coordinates
    int probe_log = 0;           // "probe_log": records the probe log keeps, 0 = off
    long probe_gen = 0;          // bumped by fs_set_probes and fs_set_option("probe_log"): list and ring are set up anew, the log is cleared
    int body_log = 0;            // "body_force_log": steps the per-body force log keeps, 0 = off
    long body_log_gen = 0;       // bumped by fs_set_option("body_force_log") and ("moment_origin"): the ring is reallocated and cleared
    double moment_origin[3] = {0.0, 0.0, 0.0};   // "moment_origin": r0 of the per-body moments, padded index coordinates
    std::vector<ImageView> image_views;   // fs_image_views
    int image_log = 0;           // "image_log": frames the image log keeps, 0 = off
    long image_every = 1;        // "image_every": fs_step takes a frame when (steps_total - 1) % image_every == 0
    long image_gen = 0;          // bumped by fs_image_views and fs_set_option("image_log"): the ring is set up anew, the log is cleared
    std::vector<uint8_t> image_table;   // fs_image_colormap: n RGB triples; empty = the built-in table
    long image_table_gen = 0;    // bumped by fs_image_colormap
    int vol_cols[fs::VOLUME_CAMERAS_MAX] = {0, 0, 0, 0}, vol_rows[fs::VOLUME_CAMERAS_MAX] = {0, 0, 0, 0};   // the ray set of each camera slot, 0 = free
    std::vector<VolumeLogView> volume_views;   // fs_volume_views
    int volume_log = 0;          // "volume_log": frames the volume log keeps, 0 = off
    long volume_every = 1;       // "volume_every": fs_step takes a frame when (steps_total - 1) % volume_every == 0
    long volume_gen = 0;         // bumped by fs_volume_views, fs_set_option("volume_log") and a new ray set of a slot a view uses
    int monitor_log = 0;         // "monitor_log": records the flow-monitor log keeps, 0 = off
    long monitor_every = 1;      // "monitor_every": fs_step takes a record when (steps_total - 1) % monitor_every == 0
    long monitor_gen = 0;        // bumped by fs_set_option("monitor_log") and ("monitor_stations"): the ring is reallocated and cleared
    int monitor_nstations = 0;   // "monitor_stations": how many are set
    fs::MonitorStations monitor_stations = {{0, 0, 0, 0, 0, 0, 0, 0}};   // their x indices, 0 = unused
    int tracers = 0;             // "tracers": slots of the tracer pool, 0 = off
    long tracer_gen = 0;         // bumped by fs_set_option("tracers"): pool and log are set up anew and cleared
    int tracer_log = 0;          // "tracer_log": snapshot frames the tracer log keeps, 0 = off
    long tracer_log_gen = 0;     // bumped by fs_set_option("tracer_log"): the ring is set up anew, the log is cleared
    long tracer_every = 1;       // "tracer_every": fs_step takes a snapshot when (steps_total - 1) % tracer_every == 0
    long tracer_seeded = 0;      // particles ever seeded or released since the pool was cleared: the next goes into slot seeded % C
    std::vector<double> tracer_emit;   // fs_tracer_emitters: x, y, z per emitter
    long tracer_emit_every = 1;  // fs_step releases one particle per emitter when (steps_total - 1) % tracer_emit_every == 0
    long tracer_emit_gen = 0;    // bumped by fs_tracer_emitters
    long dump_frames = 0;
    fs::FrameWriter writer;      // pinned double-buffered D2H + writer thread
    // result of the last fs_streamlines call
    std::vector<long> sl_offsets;
    std::vector<double> sl_points, sl_norm;
    // result of the last fs_obstacle_surface call
    std::vector<float> surf_verts;
    std::vector<int> surf_tris;
    bool surf_valid = false;
    // result of the last fs_isosurface call (a slot of its own)
    std::vector<float> iso_verts;
    std::vector<int> iso_tris;
    bool iso_valid = false;
    bool dump_async = true;
    fs::SweepTune tune;          // launch tunables of this handle (fs_set_option sweep_* / pair_* / project_kernels)

    int span_begin(int fam)
    {
        if (!profile) return -1;
        Span sp;
        sp.fam = fam;
        sp.launches = 0;
        for (hipEvent_t* ev : { &sp.a, &sp.b }) {
            if (!event_pool.empty()) { *ev = event_pool.back(); event_pool.pop_back(); }
            else if (hipEventCreate(ev) != hipSuccess) return -1;
        }
        hipEventRecord(sp.a, stream);
        spans.push_back(sp);
        return (int)spans.size() - 1;
    }
    void span_end(int id, long launches)
    {
        if (id < 0) return;
        spans[id].launches = launches;
        hipEventRecord(spans[id].b, stream);
    }
    void resolve_spans()
    {
        if (spans.empty()) return;
        hipStreamSynchronize(stream);
        for (Span& sp : spans) {
            float ms = 0;
            if (hipEventElapsedTime(&ms, sp.a, sp.b) == hipSuccess) {
                fam_ms[sp.fam] += ms;
                fam_launches[sp.fam] += sp.launches;
            }
            event_pool.push_back(sp.a);
            event_pool.push_back(sp.b);
        }
        spans.clear();
    }
};

namespace {

struct ScopedSpan {
    fs_sim* s; int id; long n;
    ScopedSpan(fs_sim* s_, int fam, long launches = 1) : s(s_), id(s_->span_begin(fam)), n(launches) {}
    ~ScopedSpan() { s->span_end(id, n); }
};

// Device memory with an owner: `n` elements of U behind `get()`, freed when the owner goes.  Every allocation of the engine
// and of its parts is one of these, so neither has a list of frees to keep.  Move-only.
template <class U>
struct DevBuf {
    DevBuf() = default;
    DevBuf(DevBuf&& o) noexcept : p(o.p), n(o.n) { o.p = nullptr; o.n = 0; }
    DevBuf& operator=(DevBuf&& o) noexcept
    {
        if (this != &o) { release(); p = o.p; n = o.n; o.p = nullptr; o.n = 0; }
        return *this;
    }
    DevBuf(const DevBuf&) = delete;
    DevBuf& operator=(const DevBuf&) = delete;
    ~DevBuf() { release(); }

    U* get() const { return p; }
    // `count` new elements in place of whatever was held; nothing is held where the allocation fails
    hipError_t alloc(size_t count)
    {
        hipError_t e = release();
        if (e == hipSuccess && (e = hipMalloc((void**)&p, count * sizeof(U))) == hipSuccess) n = count;
        else p = nullptr;
        return e;
    }
    // Room for at least `count` elements.  Old contents are not kept; with a stream, work queued there may still use the
    // old buffer and is waited for before it goes.
    hipError_t grow(size_t count, hipStream_t stream = nullptr)
    {
        if (count <= n) return hipSuccess;
        if (p && stream) {
            const hipError_t e = hipStreamSynchronize(stream);
            if (e != hipSuccess) return e;
        }
        return alloc(count);
    }
    hipError_t release()
    {
        const hipError_t e = p ? hipFree(p) : hipSuccess;
        p = nullptr;
        n = 0;
        return e;
    }

private:
    U* p = nullptr;
    size_t n = 0;
};

// The device ring of a per-step log: `at` keeps the books (step_ring.h), `base` holds at.cap slots of slot_bytes, set up for
// generation `gen` of the options that size it.  What a slot holds, when a record is committed and how the fetched slots
// become rows is the log's own business.
struct LogRing {
    fs::StepRing at;
    DevBuf<char> base;
    size_t slot_bytes = 0;
    long gen = -1;

    bool on() const { return at.cap > 0; }
    char* slot(long k) const { return base.get() + (size_t)k * slot_bytes; }
    // For generation `gen_`: the old ring goes (a queued record may still write to it: the stream is synchronised first) and
    // `cap` zero-filled slots of `bytes` come; cap <= 0 = the log is off.  Where the allocation fails, `base` holds nothing.
    hipError_t setup(hipStream_t stream, long gen_, int cap = 0, size_t bytes = 0)
    {
        hipError_t e = base.get() ? hipStreamSynchronize(stream) : hipSuccess;
        if (e == hipSuccess) e = base.release();
        if (e != hipSuccess) return e;
        slot_bytes = bytes;
        at.reset(0);
        gen = gen_;
        if (cap <= 0) return hipSuccess;
        if ((e = base.alloc((size_t)cap * bytes)) != hipSuccess) return e;
        if ((e = hipMemsetAsync(base.get(), 0, (size_t)cap * bytes, stream)) == hipSuccess) at.reset(cap);
        return e;
    }
    // The retained slots, oldest first, to the host buffer `dst`, in at most two copies on `stream`.  A ring laid out in
    // sections (the tracer log) names the section's first slot and its bytes per slot.
    hipError_t copy_out(hipStream_t stream, void* dst, const void* section = nullptr, size_t bytes = 0) const
    {
        const char* from = section ? (const char*)section : base.get();
        if (!section) bytes = slot_bytes;
        fs::StepRing::Run run[2];
        hipError_t e = hipSuccess;
        for (int r = 0, n = at.runs(run); r < n && e == hipSuccess; ++r) {
            e = hipMemcpyAsync(dst, from + (size_t)run[r].first_slot * bytes, (size_t)run[r].count * bytes, hipMemcpyDeviceToHost, stream);
            dst = (char*)dst + (size_t)run[r].count * bytes;
        }
        return e;
    }

    // The three steps every log's fetch shares; what lies between them (how slots become rows) is the log's own.
    // 1. The sizes go out: `rows` (what the retained records amount to, in the entry's unit) into *n_out, the overwritten
    //    records into *n_dropped.  Returns GO_ON, or the entry's answer: FS_OK for a caller that asked for the sizes alone
    //    (`wants_data` false: nothing is drained), FS_EINVAL for one without the room.
    struct FetchWords { const char *entry, *unit, *hint; };   // of the refusal: "fs_force_log", "rows", "rows = NULL"
    enum { GO_ON = 1 };                                        // neither FS_OK nor an error code
    int fetch_begin(const FetchWords& w, long rows, long room, bool wants_data, long* n_out, long* n_dropped) const
    {
        if (n_out) *n_out = rows;
        if (n_dropped) *n_dropped = at.dropped();
        if (!wants_data) return FS_OK;
        if (room < rows) return fail(FS_EINVAL, "%s: %ld %s retained, room for %ld (pass %s to ask)", w.entry, rows, w.unit, room, w.hint);
        return GO_ON;
    }
    // 2. The retained slots to the host, oldest first, and one synchronisation of `stream`: the whole slots into `dst`, or one
    //    or two sections of the ring into `dst` and `dst2` (a null one is left out).  An empty log costs nothing: its fetch
    //    is no synchronisation point.
    hipError_t fetch_copy(hipStream_t stream, void* dst, const void* section = nullptr, size_t bytes = 0, void* dst2 = nullptr,
                          const void* section2 = nullptr, size_t bytes2 = 0) const
    {
        if (at.retained() == 0) return hipSuccess;
        hipError_t e = dst ? copy_out(stream, dst, section, bytes) : hipSuccess;
        if (e == hipSuccess && dst2) e = copy_out(stream, dst2, section2, bytes2);
        return e == hipSuccess ? hipStreamSynchronize(stream) : e;
    }
    // 3. The records have been handed out: their step numbers into `steps` (if any), and the ring is empty again.
    void fetch_end(long* steps = nullptr)
    {
        if (steps)
            for (long i = 0, n = at.retained(); i < n; ++i) steps[i] = at.step_of(i);
        at.drain();
    }
};

// what the image entries accept without looking at the state: a source of fs_sample by its bits, and a colour range
bool image_source_ok(int source)
{
    if ((source >= 0 && source < FS_NFIELDS) || source == FS_SOURCE_HEAT) return true;
    if ((source & ~(FS_ISO_VORTEX - 1)) == FS_ISO_VORTEX) return (source & (FS_ISO_VORTEX - 1)) < FS_VORTEX_NFIELDS;
    if (source >= 0 && (source & ~(FS_SAMPLE_STAT - 1)) == FS_SAMPLE_STAT) {
        const int sel = source & (FS_SAMPLE_STAT - 1), which = sel & ~FS_STAT_RAW;
        return which >= 0 && which <= FS_STAT_TKE && !((sel & FS_STAT_RAW) && which == FS_STAT_TKE);
    }
    return false;
}
bool image_range_ok(double vmin, double vmax, double alpha)
{
    return std::isfinite(vmin) && std::isfinite(vmax) && vmin < vmax && alpha >= 0.0 && alpha <= 1.0;
}
// bytes of one frame of the image log: the views' RGB images one after the other
size_t image_frame_bytes(const fs_sim* s, const std::vector<ImageView>& views)
{
    size_t bytes = 0;
    for (const ImageView& v : views) {
        int c, r;
        fs::image_dims(v.axis, s->W, s->H, s->D, &c, &r);
        bytes += 3 * (size_t)c * (size_t)r;
    }
    return bytes;
}

// bytes of one frame of the volume log: the views' RGB images one after the other; `slot`, cols, rows: a slot about to change
size_t volume_frame_bytes(const fs_sim* s, const std::vector<VolumeLogView>& views, int slot = -1, int cols = 0, int rows = 0)
{
    size_t bytes = 0;
    for (const VolumeLogView& v : views)
        bytes += v.slot == slot ? 3 * (size_t)cols * (size_t)rows : 3 * (size_t)s->vol_cols[v.slot] * (size_t)s->vol_rows[v.slot];
    return bytes;
}

template <class T> T host_cbrt(T v);
template <> float host_cbrt<float>(float v) { return std::cbrt(v); }     // std::cbrt(float), simulation.cpp:295
template <> double host_cbrt<double>(double v) { return std::cbrt(v); }

template <class T> struct Engine;   // fluidsim.cpp; a part holds a reference to its engine

}  // namespace
