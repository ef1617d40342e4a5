// tools/abi_exercise.cpp -- drives most of the C ABI from plain C++ (no Python), meant to be built
// with a host sanitizer:  see the recipe in DESIGN.md ("host sanitizers").  Exit code 0 = ran clean.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include <sys/wait.h>
#include <unistd.h>

#include "../include/fluidsim.h"

#define CHECK(x) do { int rc_ = (x); if (rc_) { fprintf(stderr, "%s -> %d: %s\n", #x, rc_, fs_last_error()); return 1; } } while (0)

// One rank of a two-rank z-slab run over the FSIPC transport (both ranks share the GPU): the host side of the slab path --
// export / mapping of the arrays, the timed choice of the communication schedule (all four incl. the push schedule), the
// asynchronous reach, the split density solve, windowed gathers, per-rank dumps, reduced statistics, solver=mg on slabs.
static int slab_rank(int rank, const char* id, const char* ascii, const char* dumpdir)
{
    fs_sim* s = fs_create(32, 16, 32, 2, 30, 0.05f, 2.0e-5f, 1.5e-5f, 7);
    if (!s) { fprintf(stderr, "fs_create: %s\n", fs_last_error()); return 1; }
    CHECK(fs_set_option(s, "quiet", "1"));
    CHECK(fs_set_option(s, "dump_dir", dumpdir));
    CHECK(fs_set_option(s, "overlap", "auto"));
    CHECK(fs_set_option(s, "comm_cus", "auto"));
    char idbuf[FS_COMM_ID_BYTES] = {0};
    snprintf(idbuf, sizeof idbuf, "%s", id);
    CHECK(fs_comm_init(s, rank, 2, idbuf));
    CHECK(fs_set_option(s, "residual_log", "2"));
    {   // point probes on both sides of the slab boundary and in both z ghost planes; the sampler is single-GPU only
        const int cells[] = { 5, 5, 16, 5, 5, 17, 0, 0, 0, 33, 17, 33, 9, 7, 1 };
        CHECK(fs_set_probes(s, cells, 5));
        CHECK(fs_set_option(s, "probe_log", "3"));
        const double pt[3] = { 1.0, 1.0, 1.0 };
        if (fs_sample_points(s, pt, 1) != FS_EINVAL || fs_sample(s, FS_DENS, FS_SAMPLE_LINEAR, nullptr, 0) != FS_EINVAL) return 13;
    }
    long added = 0;
    CHECK(fs_load_stl(s, ascii, 0.6f, 0.f, 0.f, 0.f, 5.f, 0.f, 0.f, &added));
    CHECK(fs_add_obstacle(s, 9, 7, 16));
    CHECK(fs_add_obstacle(s, 9, 7, 17));
    CHECK(fs_run(s));                                            // two steps with dumps
    CHECK(fs_set_velocity(s, 6, 5, 16, 1.5f, -0.5f, 2.0f));      // v_z jumps between steps
    CHECK(fs_run_one(s));
    int plan = -1, syncs = -1;
    CHECK(fs_get_int(s, "overlap_plan", &plan));
    CHECK(fs_get_int(s, "stream_syncs", &syncs));
    if (plan < 0 || plan > 3 || syncs != 0) { fprintf(stderr, "rank %d: plan %d, %d stream syncs\n", rank, plan, syncs); return 11; }
    CHECK(fs_advect(s, 0, FS_DENS, FS_BUFFER));                  // from outside step(): the synchronous reach
    double sum, mn, mx;
    CHECK(fs_field_stats(s, FS_VX, &sum, &mn, &mx));
    CHECK(fs_set_option(s, "solver", "mg"));
    CHECK(fs_set_option(s, "mg_min_planes", "8"));              // level 1 distributed, level 2 held whole
    CHECK(fs_run_one(s));
    CHECK(fs_add_obstacle(s, 11, 5, 15));
    CHECK(fs_run_one(s));
    const size_t n = fs_padded_size(s);
    std::vector<float> f(n);
    CHECK(fs_get_field(s, FS_PRESSURE, f.data(), n, 4));
    {   // the residual log of the slab steps (collective drain) and the collective query with its per-plane records
        long nr = 0, nd = 0;
        CHECK(fs_residual_log(s, nullptr, 0, &nr, &nd));
        std::vector<double> rows((size_t)nr * FS_RESIDUAL_LOG_COLS + 1), planes((size_t)FS_RESIDUAL_COLS * 32);
        CHECK(fs_residual_log(s, rows.data(), nr, &nr, &nd));
        double out[FS_RESIDUAL_COLS];
        CHECK(fs_solve_residual(s, 0, FS_PRESSURE, FS_DIVERGENCE, 1.0, 6.0, out, planes.data()));
        if (nr != 2 || !(out[3] > 0.0)) { fprintf(stderr, "rank %d: %ld residual rows, %g cells\n", rank, nr, out[3]); return 12; }
    }
    {   // the probe log of the slab steps: a record on demand, then the collective drain (the ring of 3 wrapped)
        CHECK(fs_probe_sample(s));
        long nr = 0, nd = 0;
        CHECK(fs_probe_log(s, nullptr, 0, &nr, &nd));
        const size_t cols = 1 + 5 * (size_t)FS_PROBE_VALUES;
        std::vector<double> rows((size_t)nr * cols + 1);
        if (nr != 3 || nd != 3 || fs_probe_log(s, rows.data(), 2, &nr, &nd) != FS_EINVAL) { fprintf(stderr, "rank %d: %ld probe rows, %ld dropped\n", rank, nr, nd); return 14; }
        CHECK(fs_probe_log(s, rows.data(), nr, &nr, &nd));
        if (rows[2 * cols] != 5.0 || !(rows[2 * cols + 2] == rows[2 * cols + 2])) return 15;   // five steps completed; a number
    }
    CHECK(fs_sync(s));
    CHECK(fs_destroy(s));
    printf("slab rank %d ok: schedule %d, velocity x in [%g, %g]\n", rank, plan, mn, mx);
    fflush(stdout);
    return 0;
}

int main(int argc, char** argv)
{
    if (argc > 1 && strcmp(argv[1], "--slabs") == 0) {
        // before any HIP call: two rank processes
        const char* ascii = argc > 2 ? argv[2] : "tests/golden/plate_ascii.stl";
        const char* dumpdir = argc > 3 ? argv[3] : "/tmp";
        char id[64];
        snprintf(id, sizeof id, "FSIPC:/fs_abi_exercise_%d", (int)getpid());
        pid_t kids[2];
        for (int r = 0; r < 2; ++r) {
            kids[r] = fork();
            if (kids[r] == 0) {
                // _exit, not return: in a forked child the HIP runtime's own exit handler trips a CHECK inside the ASan runtime
                // (sanitizer_allocator_device.h, "dev_runtime_unloaded_") after everything of ours has run clean; address
                // and UB findings are reported where they happen, not at exit (leak checking is off under HIP anyway)
                const int rc = slab_rank(r, id, ascii, dumpdir);
                fflush(stdout);
                fflush(stderr);
                _exit(rc);
            }
        }
        int bad = 0;
        for (int r = 0; r < 2; ++r) {
            int st = 0;
            waitpid(kids[r], &st, 0);
            if (!WIFEXITED(st) || WEXITSTATUS(st)) bad = 1;
        }
        printf(bad ? "slab leg FAILED\n" : "slab leg ok\n");
        return bad;
    }
    const char* stl = argc > 1 ? argv[1] : "tests/golden/sphere_24x12.stl";
    const char* ascii = argc > 2 ? argv[2] : "tests/golden/plate_ascii.stl";
    const char* dumpdir = argc > 3 ? argv[3] : "/tmp";
    for (int fp64 = 0; fp64 < 2; ++fp64) {
        fs_sim* s = fs_create(40, 24, 20, 3, 30, 0.05f, 2.0e-5f, 1.5e-5f, 5);
        if (!s) { fprintf(stderr, "fs_create: %s\n", fs_last_error()); return 1; }
        CHECK(fs_set_option(s, "precision", fp64 ? "fp64" : "fp32"));
        CHECK(fs_set_option(s, "quiet", "1"));
        CHECK(fs_set_option(s, "dump_dir", dumpdir));
        CHECK(fs_set_option(s, "profile", "1"));
        if (fs_set_option(s, "nonsense", "1") != FS_EINVAL) return 2;
        long added = 0;
        CHECK(fs_load_stl(s, stl, 0.5f, 10.f, 20.f, 30.f, -4.f, 0.f, 0.f, &added));
        CHECK(fs_load_stl(s, ascii, 0.6f, 0.f, 0.f, 0.f, 5.f, 0.f, 0.f, &added));
        if (fs_load_stl(s, "/nonexistent.stl", 1.f, 0, 0, 0, 0, 0, 0, nullptr) != FS_EIO) return 3;
        CHECK(fs_add_obstacle(s, 3, 3, 3));
        CHECK(fs_add_density(s, 4, 4, 4, 0.5f));
        CHECK(fs_set_velocity(s, 5, 5, 5, 1.f, 2.f, 3.f));
        if (fs_add_obstacle(s, 0, 1, 1) != FS_EINVAL) return 4;
        const size_t n = fs_padded_size(s);
        std::vector<float> f32(n);
        std::vector<double> f64(n);
        std::vector<uint8_t> mask(n, 0);
        CHECK(fs_get_field(s, FS_OBS, f32.data(), n, 4));
        for (size_t i = 0; i < n; ++i) mask[i] = f32[i] > 0.5f;
        CHECK(fs_set_obstacle_mask(s, mask.data(), n));
        CHECK(fs_run(s));
        CHECK(fs_step(s));
        CHECK(fs_run_one(s));
        CHECK(fs_diffuse(s, 1, FS_VX, FS_VX_PREV));
        CHECK(fs_project(s));
        CHECK(fs_advect(s, 2, FS_VY, FS_VY_PREV));
        CHECK(fs_set_bounds(s, 3, FS_VZ));
        CHECK(fs_linear_solver(s, 0, FS_PRESSURE, FS_DIVERGENCE, 1.0f, 6.0f));
        CHECK(fs_get_field(s, FS_VX, f64.data(), n, 8));
        CHECK(fs_set_field(s, FS_VX, f64.data(), n, 8));
        if (fs_get_field(s, FS_VX, f32.data(), n - 1, 4) != FS_EINVAL) return 5;
        double sum, mn, mx, ms;
        long launches;
        CHECK(fs_field_stats(s, FS_DENS, &sum, &mn, &mx));
        CHECK(fs_get_timing(s, "sweep_pair", &ms, &launches));
        CHECK(fs_time_sweeps(s, 2, FS_VY, FS_VY_PREV, 0.3f, 2.8f, 4, &ms));
        CHECK(fs_dump_frame(s));
        CHECK(fs_sync(s));
        int w;
        CHECK(fs_get_int(s, "width", &w));
        {   // the viewer's streamlines: compute, then fetch into caller memory
            long nl = 0, np = 0;
            CHECK(fs_streamlines(s, 30, 2.0, 100, 0.2, 0.0, &nl, &np));
            std::vector<long> off((size_t)nl + 1);
            std::vector<double> pts((size_t)np * 3 + 1), norm((size_t)nl + 1);
            CHECK(fs_streamlines_fetch(s, off.data(), pts.data(), norm.data()));
            if (off[(size_t)nl] != np) return 6;
        }
        {   // the viewer's obstacle mesh: extract, then fetch into caller memory
            long nv = 0, nt = 0;
            CHECK(fs_obstacle_surface(s, &nv, &nt));
            std::vector<float> verts((size_t)nv * 3 + 1);
            std::vector<int> tris((size_t)nt * 3 + 1);
            CHECK(fs_obstacle_surface_fetch(s, verts.data(), tris.data()));
            for (long i = 0; i < 3 * nt; ++i)
                if (tris[(size_t)i] < 0 || tris[(size_t)i] >= nv) return 7;
            int edges[24];
            if (fs_surface_case_table(1, edges) != 1 || fs_surface_case_table(256, edges) != FS_EINVAL) return 8;
        }
        CHECK(fs_set_option(s, "sweep_fuse", "4"));     // force the three-sweep kernel (fp32 only; fp64 keeps pairs)
        CHECK(fs_run_one(s));
        CHECK(fs_set_option(s, "sweep_fuse", "3"));
        CHECK(fs_set_option(s, "two_sweep_kernel", "fused"));   // jacobi_fused_kernel<NL=2> (fp64 here; fp32 needs rows > 512 cells)
        CHECK(fs_run_one(s));
        CHECK(fs_set_option(s, "two_sweep_kernel", "pair"));
        CHECK(fs_run_one(s));
        CHECK(fs_set_option(s, "two_sweep_kernel", "auto"));
        CHECK(fs_set_option(s, "advect_kernels", "row"));
        CHECK(fs_run_one(s));
        CHECK(fs_set_option(s, "advect_kernels", "cell"));
        CHECK(fs_set_option(s, "solver", "mg"));                // multigrid pressure solve: 40x24x20 halves twice
        CHECK(fs_set_option(s, "mg_cycles", "2"));
        CHECK(fs_run_one(s));
        CHECK(fs_add_obstacle(s, 7, 7, 7));                      // rebuilds the coarse operators
        CHECK(fs_run_one(s));
        CHECK(fs_linear_solver(s, 0, FS_PRESSURE, FS_DIVERGENCE, 1.0f, 6.0f));
        int mgl = 0;
        CHECK(fs_get_int(s, "mg_levels", &mgl));
        if (mgl != 3) return 9;
        if (fs_set_option(s, "mg_pre", "0") != FS_EINVAL) return 10;
        {   // residual of the linear solves: the on-demand queries, then the per-step log through a wrap and a drain
            double out[FS_RESIDUAL_COLS];
            std::vector<double> planes((size_t)FS_RESIDUAL_COLS * 20);
            CHECK(fs_solve_residual(s, 0, FS_PRESSURE, FS_DIVERGENCE, 1.0, 6.0, out, planes.data()));
            if (!(out[0] >= 0.0) || !(out[3] > 0.0)) return 12;
            CHECK(fs_diffuse_residual(s, 1, FS_VX, FS_VX, out, nullptr));
            if (fs_solve_residual(s, 4, FS_DENS, FS_BUFFER, 1.0, 6.0, out, nullptr) != FS_EINVAL) return 13;
            CHECK(fs_set_option(s, "residual_log", "2"));
            for (int k = 0; k < 3; ++k) CHECK(fs_run_one(s));
            long nr = 0, nd = 0;
            CHECK(fs_residual_log(s, nullptr, 0, &nr, &nd));
            if (nr != 2 || nd != 1) return 14;
            std::vector<double> rows((size_t)nr * FS_RESIDUAL_LOG_COLS);
            if (fs_residual_log(s, rows.data(), 1, &nr, &nd) != FS_EINVAL) return 15;
            CHECK(fs_residual_log(s, rows.data(), nr, &nr, &nd));
            if (!(rows[5] > 0.0)) return 16;
            CHECK(fs_set_option(s, "residual_log", "0"));
        }
        {   // time-averaged flow statistics: samples inside steps and on demand, every selector, the error cases, off again
            const size_t np = fs_padded_size(s);
            std::vector<double> d(np);
            std::vector<float> f4(np);
            if (fs_flow_stats_field(s, FS_STAT_MEAN_VX, d.data(), np, 8) != FS_EINVAL) return 17;
            CHECK(fs_set_option(s, "flow_stats", "mean"));
            if (fs_flow_stats_field(s, FS_STAT_MEAN_VX, d.data(), np, 8) != FS_EINVAL) return 18;
            CHECK(fs_flow_stats_field(s, FS_STAT_MEAN_VX | FS_STAT_RAW, d.data(), np, 8));
            CHECK(fs_run_one(s));
            if (fs_flow_stats_field(s, FS_STAT_UU, d.data(), np, 8) != FS_EINVAL) return 19;
            CHECK(fs_set_option(s, "flow_stats", "moments"));
            CHECK(fs_set_option(s, "flow_stats_every", "2"));
            for (int k = 0; k < 3; ++k) CHECK(fs_run_one(s));
            CHECK(fs_flow_stats_sample(s));
            int ns = 0;
            CHECK(fs_get_int(s, "flow_stats_samples", &ns));
            if (ns < 2 || ns > 3) return 20;      // one or two of the three steps (every second one), and the one on demand
            for (int which = 0; which <= FS_STAT_TKE; ++which) {
                CHECK(fs_flow_stats_field(s, which, d.data(), np, 8));
                CHECK(fs_flow_stats_field(s, which, f4.data(), np, 4));
                if (which != FS_STAT_TKE) CHECK(fs_flow_stats_field(s, which | FS_STAT_RAW, d.data(), np, 8));
            }
            if (fs_flow_stats_field(s, FS_STAT_TKE | FS_STAT_RAW, d.data(), np, 8) != FS_EINVAL) return 21;
            if (fs_flow_stats_field(s, FS_STAT_TKE, d.data(), np - 1, 8) != FS_EINVAL) return 22;
            CHECK(fs_flow_stats_reset(s));
            CHECK(fs_set_option(s, "flow_stats", "off"));
            if (fs_flow_stats_sample(s) != FS_EINVAL) return 23;
        }
        {   // vortex identification and iso-surfaces: every selector in both element sizes, the dump, the two result slots, the error cases
            const size_t np = fs_padded_size(s);
            std::vector<double> d(np);
            std::vector<float> f4(np);
            for (int which = 0; which < FS_VORTEX_NFIELDS; ++which) {
                CHECK(fs_vortex_field(s, which, d.data(), np, 8));
                CHECK(fs_vortex_field(s, which, f4.data(), np, 4));
            }
            if (fs_vortex_field(s, FS_VORTEX_NFIELDS, d.data(), np, 8) != FS_EINVAL) return 24;
            if (fs_vortex_field(s, FS_VORTEX_Q, d.data(), np - 1, 8) != FS_EINVAL) return 25;
            if (fs_vortex_field(s, FS_VORTEX_Q, d.data(), np, 2) != FS_EINVAL) return 26;
            CHECK(fs_vortex_dump(s, dumpdir));
            long nv = 0, nt = 0, ov = 0, ot = 0;
            if (fs_isosurface_fetch(s, nullptr, nullptr) != FS_EINVAL) return 27;
            CHECK(fs_isosurface(s, FS_ISO_VORTEX | FS_VORTEX_W2, 0.0, &nv, &nt));
            CHECK(fs_obstacle_surface(s, &ov, &ot));
            std::vector<float> verts(3 * (size_t)nv + 1);
            std::vector<int> tris(3 * (size_t)nt + 1);
            CHECK(fs_isosurface_fetch(s, verts.data(), tris.data()));
            for (long i = 0; i < 3 * nt; ++i)
                if (tris[(size_t)i] < 0 || tris[(size_t)i] >= nv) return 28;
            CHECK(fs_isosurface(s, FS_OBS, 0.5, &nv, &nt));
            if (nv != ov || nt != ot) return 29;
            if (fs_isosurface(s, FS_ISO_VORTEX | 7, 0.0, &nv, &nt) != FS_EINVAL) return 30;
            if (fs_isosurface(s, FS_NFIELDS, 0.0, &nv, &nt) != FS_EINVAL) return 31;
        }
        {   // field sampling: every kind of source in every mode at the mesh's vertices and a few odd points, the error cases
            long nv = 0, nt = 0;
            CHECK(fs_obstacle_surface(s, &nv, &nt));
            std::vector<float> verts(3 * (size_t)nv + 1);
            CHECK(fs_obstacle_surface_fetch(s, verts.data(), nullptr));
            std::vector<double> pts(verts.begin(), verts.begin() + 3 * nv);
            const double odd[] = { 0.0, 0.0, 0.0, 41.0, 25.0, 21.0, 41.5, 1.0, 1.0, -0.5, 1.0, 1.0, 1.0, 0.0 / 0.0, 1.0, 7.25, 3.5, 20.75 };
            pts.insert(pts.end(), odd, odd + 18);
            const long np = (long)(pts.size() / 3);
            std::vector<double> out((size_t)np);
            if (fs_sample(s, FS_PRESSURE, FS_SAMPLE_LINEAR, out.data(), np) != FS_EINVAL) return 32;     // no points kept yet
            CHECK(fs_sample_points(s, pts.data(), np));
            CHECK(fs_set_option(s, "flow_stats", "moments"));
            CHECK(fs_run_one(s));
            const int sources[] = { FS_PRESSURE, FS_OBS, FS_VX_PREV, FS_ISO_VORTEX | FS_VORTEX_Q, FS_SAMPLE_STAT | FS_STAT_MEAN_P,
                                    FS_SAMPLE_STAT | FS_STAT_RAW | FS_STAT_UV, FS_SAMPLE_STAT | FS_STAT_TKE };
            for (int src : sources)
                for (int mode = FS_SAMPLE_NEAREST; mode <= FS_SAMPLE_FLUID; ++mode) {
                    CHECK(fs_sample(s, src, mode, out.data(), np));
                    if (out[(size_t)np - 3] == out[(size_t)np - 3] || out[(size_t)np - 2] == out[(size_t)np - 2]) return 33;   // outside the box: NaN
                }
            if (fs_sample(s, FS_NFIELDS, FS_SAMPLE_LINEAR, out.data(), np) != FS_EINVAL) return 34;
            if (fs_sample(s, FS_PRESSURE, 3, out.data(), np) != FS_EINVAL) return 35;
            if (fs_sample(s, FS_PRESSURE, FS_SAMPLE_FLUID, out.data(), np - 1) != FS_EINVAL) return 36;
            if (fs_sample_points(s, pts.data(), (1L << 24) + 1) != FS_EINVAL) return 37;
            CHECK(fs_set_option(s, "flow_stats", "off"));
            if (fs_sample(s, FS_SAMPLE_STAT | FS_STAT_MEAN_P, FS_SAMPLE_LINEAR, out.data(), np) != FS_EINVAL) return 38;
            CHECK(fs_sample_points(s, pts.data(), 2));          // a smaller set replaces it
            CHECK(fs_sample(s, FS_DENS, FS_SAMPLE_NEAREST, out.data(), 2));
            CHECK(fs_sample_points(s, nullptr, 0));
        }
        {   // point probes: the list, the ring through a wrap, a record on demand, the drain, the limits, off again
            const int cells[] = { 0, 0, 0, 41, 25, 21, 3, 3, 3, 20, 12, 10 };
            const int bad[] = { 42, 1, 1 };
            if (fs_probe_sample(s) != FS_EINVAL) return 39;
            if (fs_set_probes(s, bad, 1) != FS_EINVAL || fs_set_probes(s, cells, FS_PROBE_MAX + 1) != FS_EINVAL) return 40;
            CHECK(fs_set_probes(s, cells, 4));
            CHECK(fs_set_option(s, "probe_log", "2"));
            for (int k = 0; k < 3; ++k) CHECK(fs_run_one(s));
            CHECK(fs_probe_sample(s));
            long nr = 0, nd = 0;
            int count = 0;
            CHECK(fs_get_int(s, "probe_count", &count));
            CHECK(fs_probe_log(s, nullptr, 0, &nr, &nd));
            if (count != 4 || nr != 2 || nd != 2) return 41;
            const size_t cols = 1 + 4 * (size_t)FS_PROBE_VALUES;
            std::vector<double> rows((size_t)nr * cols);
            if (fs_probe_log(s, rows.data(), 1, &nr, &nd) != FS_EINVAL) return 42;
            CHECK(fs_probe_log(s, rows.data(), nr, &nr, &nd));
            if (rows[0] != rows[cols] || rows[1] != rows[cols + 1]) return 43;     // the last step's record and the one on demand
            if (fs_set_option(s, "probe_log", "1048577") != FS_EINVAL) return 44;
            CHECK(fs_get_timing(s, "probes", &ms, &launches));
            if (launches != 4) return 45;
            CHECK(fs_set_probes(s, nullptr, 0));
            CHECK(fs_run_one(s));
            CHECK(fs_set_option(s, "probe_log", "0"));
        }
        {   // tracer particles: seeds past the pool's end, emitters, steps and an advance on demand, the ring through a wrap, off again
            const double seeds[] = { 2.0, 12.0, 10.0, 0.5, 0.5, 0.5, 40.5, 24.5, 20.5, 3.0, 3.0, 3.0, 5.5, 6.25, 7.75 };
            const double bad[] = { 0.25, 1.0, 1.0 };
            if (fs_tracer_advance(s) != FS_EINVAL || fs_tracer_seed(s, seeds, 1) != FS_EINVAL) return 46;   // the option is off
            CHECK(fs_set_option(s, "tracers", "6"));
            CHECK(fs_set_option(s, "tracer_log", "2"));
            if (fs_tracer_seed(s, bad, 1) != FS_EINVAL || fs_tracer_emitters(s, seeds, 2, 0) != FS_EINVAL) return 47;
            CHECK(fs_tracer_seed(s, seeds, 5));
            CHECK(fs_tracer_emitters(s, seeds, 2, 2));
            for (int k = 0; k < 3; ++k) CHECK(fs_run_one(s));
            CHECK(fs_tracer_advance(s));
            long np = 0, nf = 0, nd = 0;
            CHECK(fs_tracer_fetch(s, nullptr, nullptr, 0, &np));
            if (np != 6) return 48;
            std::vector<double> xyz(3 * 6 * 2), val(6);
            std::vector<int32_t> meta(4 * 6), status(6 * 2);
            std::vector<long> steps(2);
            if (fs_tracer_fetch(s, xyz.data(), meta.data(), 5, &np) != FS_EINVAL) return 49;
            CHECK(fs_tracer_fetch(s, xyz.data(), meta.data(), 6, &np));
            CHECK(fs_tracer_sample(s, FS_PRESSURE, FS_SAMPLE_LINEAR, val.data(), 6));
            CHECK(fs_tracer_log(s, nullptr, nullptr, nullptr, 0, &nf, &nd));
            if (nf != 2 || nd != 2) return 50;
            CHECK(fs_tracer_log(s, xyz.data(), status.data(), steps.data(), 2, &nf, &nd));
            CHECK(fs_get_timing(s, "tracers", &ms, &launches));
            if (launches != 4) return 51;
            CHECK(fs_tracer_clear(s));
            CHECK(fs_set_option(s, "tracers", "0"));
        }
        CHECK(fs_set_option(s, "solver", "gs_lex"));
        CHECK(fs_run_one(s));
        CHECK(fs_destroy(s));
        printf("%s ok: %zu cells, density sum %.6g, %ld sample points\n", fp64 ? "fp64" : "fp32", n, sum, added);
    }
    return 0;
}
