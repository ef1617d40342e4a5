/* include/fluidsim.h -- C ABI of libfluidsim.so, the MI355X-native wind-tunnel solver.
 *
 * The reference (Ghundi/fluid_simulation) has no FFI or plugin interface; its seams are a
 * C++ class, one free function, a no-argument executable and a file layout (SURVEY.md
 * section 8b).  This header is the drop-in boundary for the first two: one handle type
 * and one function per public member of `class Simulation` (simulation.h:42-91) and for
 * loadSTLIntoObstacles (object_loader.h:7-17), with the same argument order, the same
 * 1-based interior coordinates and the same defaults.  Every entry point cites the
 * reference declaration it replaces.  Plain C types only; no device pointers cross.
 *
 * All compute happens in hand-written HIP kernels for gfx950; there is no CPU fallback.
 * fs_create fails (NULL + fs_last_error) when no HIP device is usable.
 *
 * Return convention: 0 on success, a negative FS_E* code on failure; fs_last_error()
 * describes the most recent failure on the calling thread.  The reference itself has no
 * error reporting (out-of-range mutators are UB there, simulation.cpp:157-177); here
 * they are FS_EINVAL.  A handle is driven by one host thread at a time.
 */
#ifndef FLUIDSIM_H
#define FLUIDSIM_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct fs_sim fs_sim;

enum {
    FS_OK = 0,
    FS_EINVAL = -1,   /* bad argument / out-of-range cell / call not legal in this state */
    FS_EIO = -2,      /* STL or dump-file I/O */
    FS_EHIP = -3,     /* HIP runtime error (no device, allocation, launch) */
    FS_ECOMM = -4,    /* RCCL error (multi-GPU slabs) */
    FS_ENOMEM = -5
};

/* Field selectors for fs_get_field / fs_set_field and the per-pass entry points.  The
 * order of 0..4 is the frame-dump order of simulation.cpp:143-147 with obs at 4; 5..10
 * are the reference's private scratch arrays (simulation.h:16-27). */
enum {
    FS_DENS = 0, FS_VX = 1, FS_VY = 2, FS_VZ = 3, FS_OBS = 4,
    FS_PRESSURE = 5, FS_DIVERGENCE = 6,
    FS_VX_PREV = 7, FS_VY_PREV = 8, FS_VZ_PREV = 9, FS_BUFFER = 10,
    FS_NFIELDS = 11
};

/* Solver used by linearSolver (simulation.cpp:251-273). */
enum {
    FS_SOLVER_JACOBI = 0,  /* ping-pong Jacobi, any grid, multi-GPU capable (default) */
    FS_SOLVER_GS_LEX = 1,  /* the reference's in-place sweep in its one-thread order; verification mode */
    FS_SOLVER_RBSOR = 2,   /* NOT the reference's arithmetic: red-black successive over-relaxation, `acc`
                            * iterations (even x+y+z cells, then odd, setBounds after each half), relaxation
                            * factor "sor_omega"; converges far faster per iteration; SURVEY.md 8f rank 4 */
    FS_SOLVER_MG = 3       /* NOT the reference's arithmetic: the projection's pressure equation (simulation.cpp:320) is
                            * solved by "mg_cycles" multigrid V-cycles instead of `acc` relaxation sweeps (2x2x2
                            * cell-centred coarsening, red-black smoothing, obstacle-aware coarse operators; defined in
                            * oracle/cpu_ref_mg.h); so does fs_linear_solver when called with that equation's coefficients
                            * (b = 0, a = 1, c = 6); every other solve (diffusion) runs Jacobi.  One GPU or z-slabs
                            * (a rank must then hold an even number of planes; option "mg_min_planes": coarse levels stay
                            * distributed while every rank keeps that many planes, default 32, and an even number of them
                            * unless the level is the coarsest, and are held whole by every rank below); grids whose extents
                            * cannot be halved get no coarse levels.  SURVEY.md 8f rank 4 */
};

/* ---- construction -------------------------------------------------------------- */

/* Simulation::Simulation(w,h,d,iter,speed=30,dt=0.05f,diff=2.0e-5f,visc=1.5e-5f,acc=15)
 * -- simulation.h:59-64, simulation.cpp:17-44.  Uses the calling thread's current HIP
 * device.  Fields are zero-initialised; storage is allocated on first use so that
 * fs_set_option("precision", ...) can still be applied. */
fs_sim* fs_create(int w, int h, int d, int iter, int speed, float dt, float diff, float visc, int acc);

/* Reference defaults for the trailing constructor arguments (simulation.h:60-64). */
#define FS_DEFAULT_SPEED 30
#define FS_DEFAULT_DT 0.05f
#define FS_DEFAULT_DIFF 2.0e-5f
#define FS_DEFAULT_VISC 1.5e-5f
#define FS_DEFAULT_ACC 15

int fs_destroy(fs_sim* s);

/* Options (string key/value), legal before the first step unless noted:
 *   "precision"   "fp32" (default) | "fp64"       field storage + arithmetic; before first use only
 *   "solver"      "jacobi" (default; out-of-place sweeps, deterministic, multi-GPU) | "gs_lex" (the
 *                 reference's in-place lexicographic sweep, simulation.cpp:259-271, bit-identical with
 *                 the reference at one OpenMP thread; single GPU) | "rbsor" (optional red-black SOR,
 *                 different arithmetic from the reference by design; defined by oracle/cpu_ref.c CR_RBSOR)
 *                 | "mg" (optional: the projection's pressure equation solved by multigrid V-cycles, every
 *                 other system relaxed as under "jacobi"; different arithmetic from the reference by design,
 *                 defined by oracle/cpu_ref_mg.h CR_MG; see FS_SOLVER_MG above)
 *   "sor_omega"   relaxation factor of "rbsor", in (0, 2), default 1 (= red-black Gauss-Seidel)
 *   "dump_dir"    directory for frame dumps, default "data" (simulation.cpp:56-60)
 *   "dump_every"  N>=1 dump every Nth step (default 1 = reference behaviour), 0 = never,
 *                 -1 = last step of fs_run only.  May be changed at any time.
 *   "dump_async"  "1" (default): frames go through a pinned double buffer and a writer thread while
 *                 the next step computes; "0": every dump completes before fs_step returns
 *   "voxel_seed"  seed of the voxelizer's minstd_rand stream (object_loader.cpp:399 uses a
 *                 thread-id hash; default here is 1)
 *   "quiet"       "1" suppresses the reference's console lines
 *   "profile"     "1" brackets each kernel family with HIP events (see fs_get_timing)
 *   "elide_dead_density_solve" "1" skips diffuse(0,dens,buffer) whose result the next
 *                 advect overwrites (simulation.cpp:135-136); default "0" = do it
 *   "force_log"   N >= 0: keep the obstacle pressure forces of the last N steps (fs_force_log); 0 (default) =
 *                 off, and the step launches nothing for it.  Setting it (re)allocates and clears the log.
 *                 May be changed at any time.
 *   "residual_log" N >= 0 (at most 1048576): keep the residuals of the six linear solves of the last N steps, before and
 *                 after each solve (fs_residual_log); 0 (default) = off, and the step launches and allocates nothing for
 *                 it.  Setting it (re)allocates and clears the log.  May be changed at any time.
 *   "flow_stats"  "off" (default) | "mean" | "moments", "flow_stats_every" N >= 1, "flow_stats_start" S >= 0: time-averaged
 *                 flow statistics on the device, see fs_flow_stats_field below.  May be changed at any time.
 *   "body_force_log" N >= 0 (at most 1048576): keep the per-body forces and moments of the last N steps (fs_body_force_log); 0
 *                 (default) = off, and the step launches and allocates nothing for it.  "moment_origin" "x,y,z": the origin of
 *                 the moments (default "0,0,0").  Setting either clears the log.  May be changed at any time.  Single GPU only.
 *   "probe_log"   N >= 0 (at most 1048576): keep the last N records of the point probes (fs_set_probes, fs_probe_log); 0 (default) =
 *                 off, and the step launches and allocates nothing for it.  Setting it (re)allocates and clears the log.  May be
 *                 changed at any time.
 *   "image_log"   N >= 0 (at most 65536): keep the last N frames of the image views (fs_image_views, fs_image_log); 0 (default) =
 *                 off, and the step launches and allocates nothing for it.  "image_every" K >= 1 (default 1): a frame every
 *                 Kth step.  Setting "image_log" (re)allocates and clears the log.  May be changed at any time.  Single GPU only.
 *   "tracers"     C >= 0 (at most 4194304): slots of the tracer-particle pool (fs_tracer_seed and the entries beside it); 0
 *                 (default) = off, and the step launches and allocates nothing for it.  "tracer_log" N >= 0 (at most 65536):
 *                 keep the last N snapshots of the pool (fs_tracer_log); "tracer_every" K >= 1 (default 1): a snapshot every
 *                 Kth step.  Setting "tracers" (re)allocates and clears the pool and the log, setting "tracer_log" the log.
 *                 May be changed at any time.  Single GPU only.
 *   "volume_log"  N >= 0 (at most 65536): keep the last N frames of the volume views (fs_volume_views, fs_volume_log); 0 (default)
 *                 = off, and the step launches and allocates nothing for it.  "volume_every" K >= 1 (default 1): a frame every
 *                 Kth step.  Setting "volume_log" (re)allocates and clears the log.  May be changed at any time.  Single GPU only.
 *   "monitor_log" N >= 0 (at most 1048576): keep the last N records of the flow monitor (fs_flow_monitor, fs_monitor_log); 0
 *                 (default) = off, and the step launches and allocates nothing for it.  "monitor_every" K >= 1 (default 1): a
 *                 record every Kth step.  "monitor_stations" "x1,x2,..." (up to 8 indices in 1..w, "" = none): the x whose
 *                 profile rows a record carries.  Setting "monitor_log" or "monitor_stations" (re)allocates and clears the log.
 *                 May be changed at any time.  Single GPU only.
 * Per-handle tuning keys that never change results (kernel selection and launch shapes):
 *   "sweep_fuse"  "1" one solver sweep per pass over memory, "2" two, "3" (default) two or three: the
 *                 three-sweep kernel (fp32, rows up to 512 cells) is timed against the two-sweep one
 *                 once per grid and used where a sweep costs less (z-slab ranks: always, so that all
 *                 ranks keep one exchange schedule), "4" three wherever that kernel exists;
 *   "two_sweep_kernel" "auto" (default: timed once per grid) | "pair" | "fused" -- which of the two
 *                 two-sweep kernels (jacobi_pair_kernel / jacobi_fused_kernel<NL=2>) runs those passes;
 *   "advect_kernels" "cell" (default: one thread per cell) | "celltab" (the same reading clamped traces from the
 *                 column tables) | "tile" (the tables' window around an 8 x 8 tile of rows staged in LDS, "advect_window"
 *                 rows / planes wide) | "row" (four cells per lane, clamp tables); all bit-identical, none faster on the
 *                 benchmark flow;
 *   "mg_cycles" (default 4: 75 % of the time of the 80 sweeps of config 3, residual 34x smaller), "mg_pre", "mg_post" (smoothing steps before / after the coarse correction, default 1),
 *                 "mg_coarse_iters" (iterations on the coarsest level, default 30): solver "mg" only;
 *   "launch_plans" "<two-sweep plan id>,<three-sweep plan id>" (what fs_get_int "pair_shape" / "triple_plan" reported
 *                 in another run; -1 = none): replay those launch plans instead of timing candidates (profiling);
 *   "wall_free"   "auto" (default) | "0" | "1": whether workgroups of the three-sweep kernel that touch no wall run its
 *                 wall-free second body (auto: when a launch has more than 256 workgroups);
 *   "zero_start"  "auto" (default: on) | "0" | "1": a projection whose pressure solve starts with the three-sweep kernel on
 *                 lane-aligned fp32 rows (256 or 512 cells, one GPU, acc >= 3, Jacobi, residual log off) does not zero p in
 *                 memory; the first pass takes the zeros as constants.  "0" = the launches without it;
 *   "fuse_project_advect" "auto" (default: on) | "0" | "1": on one GPU the gradient pass of a step's first projection runs
 *                 inside the kernel of the three velocity advections ("advect_kernels" = "cell", Jacobi, acc > 0; fs_project
 *                 and fs_advect are not affected).  fs_get_int "zero_start_projections" / "project_advect_steps" count
 *                 the projections / steps that took these paths;
 *   "sweep_ry" "sweep_zc" "sweep_blocks" "pair_zc" "pair_shape" "project_kernels" "fuse_advect"
 *                 -- see csrc/kernels.h (SweepTune), csrc/fluidsim.cpp and tools/tune_*.py.
 * z-slab handles only (never change results either):
 *   "overlap"     how a solver pass and the exchange of its boundary planes are scheduled: "0" the pass, then the exchange;
 *                 "1" boundary planes first, their exchange beside the interior launch; "2" boundary launch + exchange on
 *                 the communication stream beside the interior launch; "3" (FSIPC transport only, elsewhere = "0") the
 *                 kernels store the boundary planes straight into the neighbours' halo planes; "auto" (default) times
 *                 them once over the real transport, the slowest rank's time decides, every rank agrees.  Before the
 *                 first solve.  fs_get_int "overlap_plan" / fs_get_float "overlap<k>_ms" report the choice and the times;
 *   "comm_cus"    "0" (default) | N | "auto": CUs kept free of solver workgroups (CU-masked compute stream) for the
 *                 transport's kernels; "auto" adds "8 free" to the timed candidates.  Before first use;
 *   "split_density_solve" "1" (default) | "0": run half of the density solve (simulation.cpp:135) between the first
 *                 projection and the velocity advection, so that the reach of each advection gather reaches the host
 *                 without stalling the device (same passes, same order, same bits);
 *   "debug_poison_gather" "1": fill the gathered advection source with NaN patterns before each gather (tests);
 *   "vorticity_confinement" "<eps>": a decimal number, finite and >= 0; "0" (default) = off.  With eps > 0 every fs_step
 *                 begins with one confinement pass of that strength (see "vorticity confinement" below), before the inlet
 *                 forcing of simulation.cpp:103-105; the step then proceeds exactly as without it.  NOT the reference's
 *                 arithmetic.  May be changed at any time; single-GPU handles only (fs_step on a handle with a
 *                 communicator is FS_EINVAL while eps > 0).  fs_get_float "vorticity_confinement" answers it.
 *   "inflow"      "off" (default) | "on": fs_step writes the x = 1 face from the inflow generator (see "turbulent inflow" below)
 *                 instead of (speed, 0, 0); "on" with nothing else set writes the same numbers through the new path.  NOT the
 *                 reference's arithmetic once a map, a gust or eddies are set.  Single-GPU handles only (fs_step on a handle
 *                 with a communicator is FS_EINVAL while it is on);
 *   "inflow_eddies" N, 0 (default: no fluctuations) .. 65536;  "inflow_sigma" the eddy radius in cells, >= 1 (default 4);
 *   "inflow_rms"  the strength u_rms >= 0 (default 0);  "inflow_convect" cells an eddy moves per step, >= 0, or "auto" (default):
 *                 ((double)dt * (double)width) * (double)speed as they are when a plane is made;  "inflow_seed" an unsigned
 *                 64-bit number (default 1).  All may be changed at any time; a value that is not finite, negative, a sigma
 *                 below 1 or more than 65536 eddies is FS_EINVAL and changes nothing.  fs_get_int answers "inflow" (0 / 1),
 *                 "inflow_eddies" and "inflow_passes" (planes the steps wrote); fs_get_float "inflow_sigma" "inflow_rms"
 *                 "inflow_convect" (what "auto" stands for now).
 * fs_get_int also answers "local_depth" "z_offset" "halo_depth" "last_advect_reach" "pair_shape" "triple_plan"
 * "two_sweep_fused" "mg_levels" "mg_first_replicated" (the first coarse level every slab rank holds whole) and, for
 * slab handles, "stream_syncs" (compute-stream synchronisations issued by slab steps; 0 on the step path) "reach_waits"
 * "reach_waits_blocked" "reach_wait_us" "reach_hidden" "reach_exposed", and "flow_stats_samples" and "probe_count", and
 * "tracer_capacity" "tracer_count" "tracer_seeded" "tracer_emitters" (see the tracer particles below), and
 * "confinement_passes" (confinement passes done so far, inside steps and by fs_confine_vorticity), and "monitor_log"
 * "monitor_every" "monitor_stations" (the number of stations set), and "dump_slot_waits" (see fs_dump_frame).
 */
int fs_set_option(fs_sim* s, const char* key, const char* value);

/* Public data members of class Simulation (simulation.h:44-54), by name:
 * "width" "height" "depth" "speed" "acc" "iter" (int) and "dt" "diff" "visc" (float). */
int fs_get_int(fs_sim* s, const char* name, int* out);
int fs_set_int(fs_sim* s, const char* name, int value);      /* speed, acc, iter, z_alternate only */
/* "z_alternate" = -1 (auto, the default) | 0 | 1, never changes results: within a solve, a three-sweep pass that follows an upward
 * pass marches from plane D down to plane 1, so that it starts on the planes the pass before it touched last (what the 256 MiB
 * Infinity Cache still holds); fp32 rows of 512 cells on one GPU, elsewhere every pass runs upward.  Auto: only where iterate,
 * target and right-hand side together are larger than that cache; 0 = the launches without it.  fs_get_int "reversed_passes"
 * counts the passes that ran downward. */
int fs_get_float(fs_sim* s, const char* name, float* out);
int fs_set_float(fs_sim* s, const char* name, float value);

/* ---- mutators (1-based interior coordinates, like the reference) ---------------- */

int fs_add_obstacle(fs_sim* s, int x, int y, int z);                          /* Simulation::addObstacle  simulation.h:79, .cpp:155-158 */
int fs_add_density(fs_sim* s, int x, int y, int z, float amount);             /* Simulation::addDensity   simulation.h:84, .cpp:163-166 */
int fs_set_velocity(fs_sim* s, int x, int y, int z, float ax, float ay, float az); /* Simulation::setVelocity simulation.h:89, .cpp:171-178 */

/* loadSTLIntoObstacles(stlFile, sim, scale=0.8f, rot_x, rot_y, rot_z, translate_x/y/z)
 * -- object_loader.h:7-17, object_loader.cpp:270-452.  Ray-parity voxelisation runs on
 * the GPU.  A missing or empty STL prints the reference's message, leaves the tunnel
 * unchanged and returns FS_EIO (the reference returns void and carries on,
 * object_loader.cpp:282-285; callers that want that behaviour ignore the code).
 * On success *added (may be NULL) receives the "Added N obstacle points" count.
 * A truncated binary file keeps its complete records and nothing is sized by its count
 * field; host memory that runs out while the mesh is read is FS_ENOMEM, never an exception. */
int fs_load_stl(fs_sim* s, const char* stl_file, float scale, float rot_x, float rot_y, float rot_z,
                float translate_x, float translate_y, float translate_z, long* added);

/* Whole-mask injection (golden masks, analytic shapes): `mask` is a padded x-fastest
 * array of (w+2)(h+2)(d+2) bytes, non-zero = solid; ghost cells must be zero. */
int fs_set_obstacle_mask(fs_sim* s, const uint8_t* mask, size_t n);

/* ---- time stepping -------------------------------------------------------------- */

int fs_step(fs_sim* s);     /* Simulation::step()  simulation.h:74, .cpp:96-150 (incl. the frame dump, subject to dump_every) */
int fs_run_one(fs_sim* s);  /* one iteration of the loop in Simulation::run(): inlet density, buffer=dens, step()  .cpp:63-78 */
int fs_run(fs_sim* s);      /* Simulation::run()   simulation.h:69, .cpp:49-91: `iter` iterations + the console statistics */
int fs_sync(fs_sim* s);     /* wait for all queued GPU work of this handle */

/* The private passes of the reference, exposed for per-kernel parity tests.  `field` and
 * `prev` are FS_* selectors; b is the boundary code (0 scalar, 1/2/3 velocity component). */
int fs_set_bounds(fs_sim* s, int b, int field);                                  /* setBounds     simulation.cpp:183-246 */
int fs_linear_solver(fs_sim* s, int b, int field, int prev, float a, float c);   /* linearSolver  simulation.cpp:251-273 */
int fs_diffuse(fs_sim* s, int b, int field, int prev);                           /* diffuse       simulation.cpp:278-284 */
int fs_project(fs_sim* s);                                                       /* project       simulation.cpp:289-362 */
int fs_advect(fs_sim* s, int b, int field, int prev);                            /* advect        simulation.cpp:367-424 */

/* ---- data access ---------------------------------------------------------------- */

/* Copies one field in the reference's own layout: padded (w+2)(h+2)(d+2), x fastest
 * (simulation.h:9).  elem_size selects the host element type (4 = float, 8 = double,
 * 1 = uint8_t); conversion happens on the device.  n is the element count of the host buffer.
 * A transfer that keeps the format keeps every bit, NaN payloads included.  double -> float is IEEE round-to-nearest-even
 * (float subnormals kept, overflow to infinity), float -> double is exact; a NaN that is converted stays a NaN, its sign and
 * payload are not defined.  elem_size 1 is defined only for values v with 0 <= v < 256 (fs_get_field truncates toward zero,
 * fs_set_field stores the byte's value); what another value, an infinity or a NaN becomes is not defined.
 * A wrong n, another elem_size or a null buffer is FS_EINVAL and copies nothing.
 * The twelve edges of the padded box (cells that are ghosts in two or three directions) are written by no pass of the
 * reference, so they are 0 in every state a run reaches; a caller of fs_set_field keeps them 0.  Passes here do not
 * preserve other values there (a solve leaves its result in another array, row-wise kernels store whole 16-byte groups
 * across the row end), while the reference would carry them along and corner back-traces would read them. */
int fs_get_field(fs_sim* s, int which, void* dst, size_t n, int elem_size);
int fs_set_field(fs_sim* s, int which, const void* src, size_t n, int elem_size);
size_t fs_padded_size(fs_sim* s);   /* Simulation::size  simulation.cpp:35 */

/* Append one frame to <dump_dir>/{data,obs,v_x,v_y,v_z}.bin exactly as simulation.cpp:140-148.
 * Write errors: a frame that did not reach its file -- a short write, a failed flush or close, a failed copy -- is FS_EIO
 * from the first call that meets it: this one, a later fs_step / fs_dump_frame that needs the staging slot, fs_sync, fs_run
 * (which ends with every frame flushed, so a run that returns FS_OK has written its frames), or fs_set_option "dump_dir".
 * It is reported once.  A failed fs_run closes its files; fs_run reopens them, and a change of "dump_dir" closes the old
 * directory's files (the next dump opens the new ones), so the handle is usable again after a full disk.
 * fs_get_int "dump_slot_waits" counts the dumps that had to wait because their staging slot was still being written. */
int fs_dump_frame(fs_sim* s);

/* Diagnostics of run(): sum/min/max over the whole padded array (simulation.cpp:73-90).  The sum is taken in double (its
 * order is not defined), min and max ignore NaN (a field without any other value reports +infinity and -infinity). */
int fs_field_stats(fs_sim* s, int which, double* sum, double* min, double* max);

/* ---- measurement ---------------------------------------------------------------- */

/* With option "profile"="1": accumulated HIP-event time and launch count of one kernel
 * family since the last fs_reset_timing: "sweep" (one solver iteration per launch)
 * "sweep_pair" (two iterations per launch) "sweep_triple" (three iterations per launch)
 * "divergence" "gradient" "advect" "bounds" "misc" "comm" (z-slab exchanges and gathers)
 * "multigrid" (the coarse-level work of solver "mg"; its level-0 smoothing passes count as
 * "sweep_pair") "forces" (fs_obstacle_force and the "force_log" records) "residual" (fs_solve_residual / fs_diffuse_residual and the
 * "residual_log" records: one launch counted per record, i.e. per solve and point in time -- 12 per step with the log on,
 * 10 where the dead density solve is elided, 0 with it off) "flow_stats" (one launch per sample of the time-averaged flow
 * statistics, 0 with the feature off) "probes" (one launch per record of the point probes, 0 with the feature off) "body_forces"
 * (one launch counted per logged projection record of "body_force_log" and per fs_body_force call, 0 with the feature off) "images"
 * (one launch counted per rendered view of the image log, 0 with the feature off) "tracers" (one launch per advance of the tracer
 * particles, in fs_step or by fs_tracer_advance, 0 with the feature off) "volume" (one launch per rendered view of the volume log, 0
 * with the feature off) "confinement" (one launch per vorticity-confinement pass, in fs_step or by fs_confine_vorticity, 0
 * with the option off) "monitor" (one launch counted per record of the flow monitor, by the log or on demand, 0 with the
 * feature unused).  Events are recorded on the handle's own stream. */
int fs_get_timing(fs_sim* s, const char* family, double* total_ms, long* launches);
int fs_reset_timing(fs_sim* s);

/* Times `reps` back-to-back linearSolver sweeps (b, a, c as fs_linear_solver) on the
 * current state with HIP events on the handle's stream, without changing the state
 * (scratch output).  Writes the mean milliseconds per sweep. */
int fs_time_sweeps(fs_sim* s, int b, int field, int prev, float a, float c, int reps, double* ms_per_sweep);

/* ---- viewer post-processing on the device -------------------- */

/* The streamlines the reference's viewer computes on the CPU for the frame it shows --
 * generate_streamlines, GUI/utils.py:118-213, called from GUI/main_window.py:227-233 -- from the
 * fields as they are on the device now (a dumped frame holds the same values).  Parameters are
 * GUI/config.py:18-23: density = STREAMLINE_DENSITY (30), proximity = STREAMLINE_PROXIMITY (2),
 * max_length = INTEGRATION_STEPS (100), step_size = INTEGRATION_STEP_SIZE (0.2),
 * vel_change_threshold = VELOCITY_CHANGE_THRESHOLD (0.1).  Coordinates are the viewer's: indices
 * into the padded arrays, x first.  Lines come in the reference's seed order (z, y, x loops).
 * FS_OBS is read as the array it is, as the viewer reads its file: the box and the seed test take
 * cells > 0.5, a line stops where the trilinear interpolation of the array passes 0.5.
 * The result stays in the handle until the next call; *n_lines / *n_points (may be NULL) receive
 * its size.  Single-GPU handles only. */
int fs_streamlines(fs_sim* s, int density, double proximity, int max_length, double step_size,
                   double vel_change_threshold, long* n_lines, long* n_points);
/* Copies the last result: offsets[n_lines + 1] (index of each line's first point), points
 * [3 * n_points] (x, y, z per point), norm_speed[n_lines] -- the number the viewer hands to its
 * colour map, min(max speed along the line / (max(vx, vy, vz) + 1e-6), 1)  (utils.py:198-205), with numpy's max
 * over the three padded arrays, ghost layer included, and Python's min: NaN if any cell of them is NaN, 0 if
 * the largest is +Inf.  Any of the three may be NULL; after a call that was refused the result is empty
 * (n_lines = 0: the single offset 0). */
int fs_streamlines_fetch(fs_sim* s, long* offsets, double* points, double* norm_speed);

/* The obstacle mesh the reference's viewer builds on the CPU for the frame it shows --
 * generate_obstacle_mesh, GUI/utils.py:10-38 (scikit-image marching cubes of `obs` at level 0.5),
 * called from GUI/main_window.py:204-218 -- from `obs` as it is on the device: an indexed triangle mesh,
 * one vertex per grid edge on which obs crosses 0.5 (linear interpolation; for a 0/1 mask the edge
 * midpoint), in the viewer's coordinates (indices into the padded array, x first).  Closed, oriented
 * with normals from solid to fluid.  PARITY UNPINNED against scikit-image (vertex / triangle order and
 * the cut of ambiguous cubes may differ; see csrc/surface.h); the library's own vertex and triangle
 * order and its placement of vertices beside non-finite values are fixed: ORDER and DEGENERATE under
 * fs_isosurface below.  The result stays in the handle until the next call.  Single-GPU handles only. */
int fs_obstacle_surface(fs_sim* s, long* n_vertices, long* n_triangles);
/* Copies the last result: vertices[3 * n_vertices] (x, y, z), triangles[3 * n_triangles] (vertex
 * indices).  Either may be NULL. */
int fs_obstacle_surface_fetch(fs_sim* s, float* vertices, int* triangles);
/* The triangle table behind it, for one cube configuration (bit i set: corner
 * (i & 1, (i >> 1) & 1, (i >> 2) & 1) is solid): writes 3 cube-edge ids per triangle into
 * edges[24] and returns the triangle count (0..8); edge id = 4 * axis + 2 * (offset on the higher
 * other axis) + (offset on the lower other axis).  Needs neither a handle nor a GPU. */
int fs_surface_case_table(int config, int* edges);

/* ---- pressure force on the obstacles (beyond the reference: it has no force output, no file:line counterpart) ----
 *
 * A face is BLOCKED where the projection's gradient (simulation.cpp:328-356) takes its one-sided form across it: it
 * lies between a cell c with obs(c) != 1 (a cell the gradient updates) and a 6-neighbour n inside the interior range
 * (1..w, 1..h, 1..d) with obs(n) != 0.  Tunnel walls and ghost cells are never bodies.  For the pressure field p,
 *     S = sum over blocked faces of p(c) * e,   e = unit vector from c toward n
 * (pressure pushes into the body; the face pressure is the fluid cell's own p, the zero-gradient treatment the
 * one-sided stencil gives solids).  In the reference p solves lap(p) = div(v) and then v -= grad(p), so
 * p = dt * P / rho and, with h = 1 / cbrt(w * h * d) (simulation.cpp:295), the force per unit density is
 *     F = S * h^2 / dt
 * and the force coefficients are
 *     C = 2 * S / (dt * speed^2 * N_front)
 * (h^2 cancels), N_front = the number of (y, z) rows that hold at least one solid (obs == 1) cell, the frontal area
 * in cells.  This is the PRESSURE force only: the reference diffuses the velocities with `diff`
 * (simulation.cpp:282) and models no viscous stress.  Sums run in fp64 over the z-planes in increasing z; a z-slab
 * run gives the single-GPU bits.
 *
 * fs_obstacle_force: S of the pressure in FS_PRESSURE now.  out = {Sx, Sy, Sz, blocked faces, N_front}; per_plane
 * (may be NULL) receives the same five numbers for each global z-plane 1..d (5 * d doubles), the spanwise load
 * distribution.  On z-slab handles every rank calls it and every rank gets the global result.
 *
 * fs_force_log (option "force_log" = N): inside fs_step, S is taken right after EACH of the step's two projections
 * (simulation.cpp:120 and :130), S1 and S2, into a device ring without a host synchronisation; a step applies both
 * impulses, so its force is F = (S1 + S2) * h^2 / dt.  The call drains the log: rows[FS_FORCE_LOG_COLS * i + ...] =
 * {step, S1x, S1y, S1z, S2x, S2y, S2z, blocked faces, N_front}, oldest first, one per retained step (step = how many
 * steps the handle had completed with that one); *n_dropped = logged steps the ring overwrote since the last drain.
 * rows = NULL only reports *n_rows / *n_dropped and drains nothing; max_rows < *n_rows is FS_EINVAL.  Collective on
 * z-slab handles (every rank calls it with the same arguments).  Both need a transport that moves data (FSNULL: FS_EINVAL).
 */
#define FS_FORCE_LOG_COLS 9
int fs_obstacle_force(fs_sim* s, double out[5], double* per_plane);
int fs_force_log(fs_sim* s, double* rows, long max_rows, long* n_rows, long* n_dropped);

/* ---- per-body pressure forces and moments (beyond the reference: it has no force output, no file:line counterpart) ----
 *
 * The section above weighs everything in the tunnel at once.  Here the solid cells are labelled into bodies on the
 * device and force AND moment are reported per body.  Nothing above changes.  Single-GPU handles only: on a z-slab
 * handle all five entries and option "body_force_log" return FS_EINVAL, and so does fs_comm_init on a handle whose
 * "body_force_log" is on (connectivity across slabs is not built).
 *
 * BODY CELLS AND COMPONENTS.  A BODY CELL is an interior cell (1..w, 1..h, 1..d) with obs != 0 -- the condition under
 * which a neighbour blocks a face above.  A COMPONENT is a maximal set of body cells connected through faces
 * (6-connectivity); cells that touch only along an edge or at a corner are not connected.  A component's size is its
 * cell count, its anchor the smallest padded linear index x + (w + 2) * (y + (h + 2) * z) among its cells.
 *
 * BODIES.  Components are ordered by decreasing size, ties by increasing anchor.  The first B = min(components,
 * FS_BODY_MAX) are bodies 1..B; all remaining components together are record 0, the REST (with voxelised geometry: the
 * speckle).  The label array holds k on the cells of body k, -1 on REST cells and 0 on every other cell of the padded
 * array.  The labelling is a pure function of obs (integer work only: every number below that describes it is exact).
 *
 * BODY INFO, per record k = 0..B, exact integers carried in fp64 (FS_BODY_INFO_COLS = 12):
 *     {cells, anchor, xmin, xmax, ymin, ymax, zmin, zmax, sum x, sum y, sum z, frontal rows}
 * frontal rows = the number of (y, z) rows that hold a cell of record k with obs == 1.  For an empty REST anchor is -1
 * and the bounds are 0.  The centroid is sum / cells.
 *
 * FORCE AND MOMENT RECORD.  A BLOCKED face is exactly what the section above defines, between c with obs(c) != 1 and an
 * in-range neighbour n with obs(n) != 0; it belongs to the record of n's label.  With q = +p(c) for n on the positive
 * side of c along axis a and q = -p(c) on the negative side, the face adds q to S_a.  With r = (x, y, z) of cell c minus
 * the moment origin r0, in padded index coordinates, it adds r x (q e_a) to M:
 *     axis x: My += q * rz, Mz -= q * ry;   axis y: Mx -= q * rz, Mz += q * rx;   axis z: Mx += q * ry, My -= q * rx.
 * The face centre lies half a cell from c along e_a, and a cross product with e_a removes any offset along e_a: the half
 * cell never enters the moment, the arm of a face is its cell's.  All arithmetic is fp64 on the stored p widened; each
 * product and each add is rounded once, without contraction.  Per z-plane and record the result is (FS_BODY_COLS = 8)
 *     {Sx, Sy, Sz, Mx, My, Mz, faces, frontal rows of that plane}
 * and the whole-grid record adds the planes in increasing z in fp64, starting from +0.0.  Every blocked face is a term
 * of its own: a cell blocked on both sides of an axis by the same record adds +p and then -p.  fs_obstacle_force adds
 * its terms in another order, so the S of the records summed agrees with its S to rounding, not bit for bit.
 *
 * MOMENT ORIGIN.  r0 is option "moment_origin" = "x,y,z" (three doubles; default "0,0,0", the padded array's origin).
 * It may be set at any time; setting it clears the body-force log.  One origin serves all bodies; M about another point
 * is M - (r0' - r0) x S.
 *
 * UNITS.  F = S * h^2 / dt as above; torque per unit density T = M * h^3 / dt; C_M = 2 * M / (dt * speed^2 * N_front *
 * L_ref) with L_ref in cells supplied by the caller.  PRESSURE only, as above: there is no viscous stress.
 *
 * PURE FUNCTION.  A plane's record for a body is a pure function of that plane's p, the flag bytes, the labels, the
 * origin and (w, h): one workgroup of a fixed size per plane and record, a fixed assignment of cells to lanes, a fixed
 * shuffle / LDS tree, no floating-point atomics.  Launch shape and timing cannot change a bit of it.
 *
 * fs_label_bodies labels now, whatever changed; the other entries (and fs_get_int "body_count" = B, "body_components")
 * label lazily whenever obs has changed.  A labelling synchronises the stream: a mask change is a set-up event.
 * fs_body_labels writes the labels into a dense padded array of n = (w+2)(h+2)(d+2) entries.
 * fs_body_info writes rows[FS_BODY_INFO_COLS * k + ...] and *n_rows = B + 1.
 * fs_body_force writes out[FS_BODY_COLS * k + ...] for the pressure in FS_PRESSURE now; per_plane (may be NULL) receives
 * [((z - 1) * (B + 1) + k) * FS_BODY_COLS + col] for the planes z = 1..d.
 * In both, rows / out = NULL only reports *n_rows; max_rows < *n_rows is FS_EINVAL.
 *
 * fs_body_force_log (option "body_force_log" = N, 0 = off by default, at most 1048576): inside fs_step, right after EACH
 * of the step's two projections, the whole-grid records of all B + 1 records go into a device ring on the step's own
 * stream, without a host synchronisation; with the option off a step launches and allocates nothing for it.  If obs
 * changed, the labelling is made anew at the top of fs_step.  The call drains the log, B + 1 rows per retained step,
 * rows[FS_BODY_LOG_COLS * i + ...] = {step, body, S1x, S1y, S1z, M1x, M1y, M1z, S2x, S2y, S2z, M2x, M2y, M2z, faces,
 * frontal rows}; step, oldest-first order, rows = NULL, max_rows and *n_dropped (in steps) are as for fs_force_log.  A
 * relabelling, a change of "moment_origin" and setting the option each clear the log.
 */
#define FS_BODY_MAX 16
#define FS_BODY_COLS 8
#define FS_BODY_INFO_COLS 12
#define FS_BODY_LOG_COLS 16
int fs_label_bodies(fs_sim* s, long* n_components, long* n_bodies);
int fs_body_labels(fs_sim* s, int32_t* dst, size_t n);
int fs_body_info(fs_sim* s, double* rows, long max_rows, long* n_rows);
int fs_body_force(fs_sim* s, double* out, long max_rows, long* n_rows, double* per_plane);
int fs_body_force_log(fs_sim* s, double* rows, long max_rows, long* n_rows, long* n_dropped);

/* ---- residual of the linear solves (beyond the reference: it never evaluates one, no file:line counterpart) ----
 *
 * linearSolver(b, x, x0, a, c) (simulation.cpp:251-273) iterates on x = (x0 + a * (sum of the six neighbours)) / c and
 * applies setBounds(b, x) after each sweep.  A cell is FREE where setBounds leaves it to the sweep: an interior cell with
 * obs != 1 and, for b = 1, 2, 3, without an in-range solid 6-neighbour (those cells are zeroed, simulation.cpp:227-245).
 * The inlet column is not special.  For a free cell
 *     r = (x0 + a * (((((x[i+1] + x[i-1]) + x[j+1]) + x[j-1]) + x[l+1]) + x[l-1])) - c * x
 * evaluated in fp64 from the stored values (fp32 fields, and the a and c the solve uses, widen exactly), in exactly this
 * order, without contraction.  Neighbour values are whatever the arrays hold there: ghost cells as setBounds left them,
 * solid neighbours 0 after a sweep.  Per global z-plane the record is
 *     { sum r^2, sum x0^2, max |r|, free cells }        (fp64, FS_RESIDUAL_COLS numbers)
 * over the plane's free cells; the whole-grid record adds the planes' sums in increasing z in fp64 and takes the maximum
 * of their maxima.  A plane's record is a pure function of that plane, its two z neighbours and (width, height): launch
 * tuning, slab split and timing cannot change a bit of it, and a z-slab run gives the single-GPU bits.
 * sqrt(sum r^2 / sum x0^2) is the relative residual.
 *
 * fs_solve_residual: the record of the system (b, field, prev, a, c) -- arguments as fs_linear_solver, a and c as doubles
 * (fp32 handles round them to float first, as their solve would) -- for the state as it is now; it changes nothing.
 * out = {sum r^2, sum x0^2, max |r|, free cells}; per_plane (may be NULL) receives the record of each global z-plane
 * 1..d (4 * d doubles).  field == prev is legal (the state a diffusion solve of fs_step starts from).  On z-slab
 * handles every rank calls it and every rank gets the global result.
 * fs_diffuse_residual: the same with the handle's own diffusion coefficients, a = dt * diff * w * h * d and c = 1 + 6 a
 * in the handle's precision (simulation.cpp:282-283): to fs_solve_residual what fs_diffuse is to fs_linear_solver.
 *
 * fs_residual_log (option "residual_log" = N): inside fs_step the record of each of the step's six solves -- in step()'s
 * order diffuse v_x, v_y, v_z (simulation.cpp:115-117), the first projection (:120), the second (:130), diffuse density
 * (:135) -- is taken before its first sweep and after its last (for solver "mg": around the V-cycles), into a device
 * ring without a host synchronisation and on the step's own stream.  The call drains the log:
 * rows[FS_RESIDUAL_LOG_COLS * i + ...] = {step, then for each solve k = 0..5: r0_sq, r_sq, r_max, rhs_sq, cells},
 * r0_sq = sum r^2 before the solve, the others after it; sqrt(r_sq / r0_sq) is the reduction factor of the solve.  A
 * solve the step does not run ("elide_dead_density_solve") has NaN in its four real columns and 0 cells; a solve of zero
 * sweeps has r_sq == r0_sq.  On z-slab handles the density solve is recorded where it begins and where it ends
 * ("split_density_solve" runs other work in between).  step, oldest-first order, rows = NULL, max_rows and *n_dropped
 * are as for fs_force_log.  Collective on z-slab handles.  All three need a transport that moves data (FSNULL: FS_EINVAL).
 */
#define FS_RESIDUAL_COLS 4
int fs_solve_residual(fs_sim* s, int b, int field, int prev, double a, double c, double out[4], double* per_plane);
int fs_diffuse_residual(fs_sim* s, int b, int field, int prev, double out[4], double* per_plane);
#define FS_RESIDUAL_LOG_SOLVES 6
#define FS_RESIDUAL_LOG_COLS 31
int fs_residual_log(fs_sim* s, double* rows, long max_rows, long* n_rows, long* n_dropped);

/* ---- time-averaged flow statistics (beyond the reference: it has no averaging, no file:line counterpart) ----
 *
 * A SAMPLE is the state at the end of a step, after advect(0, dens, buffer) (simulation.cpp:136) and before the frame
 * dump: u = v_x, v = v_y, w = v_z, q = dens, and p = FS_PRESSURE as the step's second projection left it.  Every cell of
 * the padded array takes part, ghost faces included, with whatever value the array holds.
 * Each cell has fp64 accumulators that start at +0.0; each sample adds to them, in sample order, one rounding per addition:
 *     mode "mean":     S_q, S_u, S_v, S_w, S_p                                  (5 arrays)
 *     mode "moments":  those, and S_uu, S_vv, S_ww, S_uv, S_uw, S_vw, S_pp      (12 arrays)
 * A product is (double)a * (double)b, taken before the add: exact on fp32 handles (24 + 24 bits; contraction cannot change a
 * bit there), rounded once on fp64 handles with the add rounded separately (the library is built with -ffp-contract=off).
 * n is the number of samples taken since the last reset.  The derived fields, in fp64, every operation rounded, no contraction:
 *     mean_a = S_a / n        cov_ab = S_ab / n - mean_a * mean_b        tke = ((cov_uu + cov_vv) + cov_ww) * 0.5
 * LIMIT: these are raw power sums, not Welford updates, so that every bit is defined by the sampled values and their order;
 * the covariance is a difference of two large numbers.  In fp64 with fp32 inputs at speed 30 it resolves variances down to
 * roughly 1e-10 of the squared mean over 1e4 samples; smaller fluctuations drown in the rounding of the sums.
 * A cell's accumulators depend on that cell's sampled values and the order of the samples only: launch shape, tuning and slab
 * split cannot change a bit, and a z-slab run gives the single-GPU bits on the planes a rank owns.
 *
 * Options (fs_set_option, any time): "flow_stats" = "off" (default: the step launches and allocates nothing for it) | "mean"
 * | "moments" -- setting it allocates or frees the accumulators (fp64 arrays of the padded local slab: 1.10 GB each at 512^3,
 * 13.2 GB for "moments") and clears them; "flow_stats_every" = N >= 1 (default 1) and "flow_stats_start" = S >= 0 (default 0):
 * fs_step samples when the handle has completed steps_total steps with this one, steps_total > S and
 * (steps_total - S - 1) % N == 0, on the step's own stream, without a host synchronisation.
 * fs_flow_stats_sample takes one sample of the state as it is now (for callers that drive the passes themselves);
 * fs_flow_stats_reset sets n = 0 (no pass over memory: the next sample overwrites); fs_get_int "flow_stats_samples" reports n.
 *
 * fs_flow_stats_field: one derived field, with the semantics of fs_get_field (dense padded layout, the local slab on slab
 * handles, elem_size 4 or 8, converted on the device).  `which` | FS_STAT_RAW returns the sum S itself (exact values, and what
 * merges two averaging windows); not with FS_STAT_TKE.  FS_EINVAL when the feature is off, for a second-moment selector in
 * mode "mean", and for a derived field while n == 0.  On z-slab handles each rank accumulates its own slab and nothing is
 * exchanged: a rank's interior planes and its physical ghost planes are defined, an inter-slab halo plane (local plane 0 on
 * ranks > 0, local plane D + 1 on ranks < last) is written as 0.
 * fs_flow_stats_dump: writes ONE frame per file, truncating, to <dir>/{data,obs,v_x,v_y,v_z}.bin in the frame-dump layout
 * (simulation.cpp:140-148) with the means in place of the fields and obs as it is, and p.bin, and tke.bin in mode "moments";
 * float32 whatever the handle's precision, so the reference's viewers show the mean flow unchanged.  Synchronous.  On slab
 * handles collective: every rank writes its planes at its offset, as fs_dump_frame does.
 */
enum {
    FS_STAT_MEAN_DENS = 0, FS_STAT_MEAN_VX = 1, FS_STAT_MEAN_VY = 2, FS_STAT_MEAN_VZ = 3, FS_STAT_MEAN_P = 4,
    FS_STAT_UU = 5, FS_STAT_VV = 6, FS_STAT_WW = 7, FS_STAT_UV = 8, FS_STAT_UW = 9, FS_STAT_VW = 10, FS_STAT_PP = 11,
    FS_STAT_TKE = 12,
    FS_STAT_RAW = 256    /* or-ed into a selector: the raw sum */
};
int fs_flow_stats_sample(fs_sim* s);
int fs_flow_stats_reset(fs_sim* s);
int fs_flow_stats_field(fs_sim* s, int which, void* dst, size_t n_elems, int elem_size);
int fs_flow_stats_dump(fs_sim* s, const char* dir);

/* ---- vortex identification (beyond the reference: it has no vorticity, no Q-criterion, no file:line counterpart) ----
 *
 * Let u = v_x, v = v_y, w = v_z be the stored values as they are now.  A cell is a TARGET when it is an interior cell
 * (1..w, 1..h, 1..d; global z on slab handles) with obs != 1.  For a target cell and an axis b,
 *     D_b f = f[+1 along b] - f[-1 along b]
 * with neighbour values as the arrays hold them: ghost cells as setBounds left them, solid cells 0 after a step.  The
 * velocity gradient in index units is g_ab = 0.5 * D_b a (the factor is exact).  All arithmetic is fp64 on the stored values
 * widened, one rounding per written operation, in exactly this order, without contraction (the library is built with
 * -ffp-contract=off):
 *     WX = 0.5 * (D_y w - D_z v)      WY = 0.5 * (D_z u - D_x w)      WZ = 0.5 * (D_x v - D_y u)
 *     W2 = (WX*WX + WY*WY) + WZ*WZ                  (|omega|^2; no square root on purpose: callers take it)
 *     Q  = -0.5 * ((g_xx*g_xx + g_yy*g_yy) + g_zz*g_zz) - ((g_xy*g_yx + g_xz*g_zx) + g_yz*g_zy)
 * Q is -1/2 g_ij g_ji = (|Omega|^2 - |S|^2) / 2, valid without assuming a divergence-free field; Q > 0 marks a vortex.
 * Every other cell of the padded array -- solid cells, all ghost cells, and on slab handles the inter-slab halo planes -- is
 * +0.0.  The fp64 result is rounded once to the handle's precision; elem_size then converts exactly as fs_get_field does.
 * UNITS: the values are per cell.  With h = 1 / cbrt(w * h * d) (simulation.cpp:295) the physical vorticity is W* / h (W2 / h^2)
 * and the physical Q is Q / h^2.
 * A cell's value is a pure function of its 18 neighbour values and its obs: launch shape, tuning (option "vortex_ry" = 1 | 2,
 * the rows a wave of the kernel owns) and slab split cannot change a bit.
 *
 * fs_vortex_field: one field, with the semantics of fs_get_field (dense padded layout, the local slab on slab handles,
 * elem_size 4 or 8).  It changes no field.  One z-marching HIP kernel per call into a private array of the handle, allocated
 * at the first call; without a call a step launches and allocates nothing for it.  On z-slab handles it is collective: each
 * rank first exchanges one halo plane of v_x, v_y, v_z; a rank's owned planes and its physical ghost planes carry the
 * single-GPU bits, the inter-slab halo planes are 0.  It needs a transport that moves data (FSNULL: FS_EINVAL).  A bad
 * selector, size or elem_size is FS_EINVAL.
 * fs_vortex_dump: writes ONE frame per file, truncating, to <dir>/{vort_x,vort_y,vort_z,vort_sq,q}.bin in the frame-dump
 * layout (simulation.cpp:140-148), float32 whatever the handle's precision.  Synchronous; five passes.  On slab handles
 * collective: every rank writes its planes at its offset, as fs_flow_stats_dump does.
 *
 * fs_isosurface: the triangle mesh of {value > level} of a source over the padded box, by the marching-cubes extractor of
 * fs_obstacle_surface: the same cube cases, vertex ownership, orientation (normals point from inside to outside) and
 * int-range check.  `source` is a field selector 0 .. FS_NFIELDS - 1, or FS_ISO_VORTEX | FS_VORTEX_* (the field is computed
 * first).  The level is rounded to the handle's precision, L.  NaN counts as outside, and so does a value equal to L.  A vertex
 * on the grid edge from point c towards +axis lies at (float)coord + (float)t along that axis, t = (L - v0) / (v1 - v0) computed
 * in the handle's precision, v0 the value at c.
 * DEGENERATE: if v0 or v1 is not finite, or !(t >= 0 && t <= 1), then t = 0.5, the edge's midpoint -- what the obstacle mesh
 * has everywhere.  (A NaN cell is outside, so it has crossing edges; +-Inf end points give Inf / Inf; L - v0 and v1 - v0 can
 * both overflow in fp32.)  Every vertex of every mesh is therefore finite and on its edge.  Vertices may coincide: v0 == L is
 * outside and gives t = 0, the grid point itself, for each of its crossing edges; the triangles between them have no area.
 * ORDER, of fs_isosurface and fs_obstacle_surface alike: the vertices follow the grid points in memory order of the padded array
 * (z outer, y, x inner), at each point its owned crossing edges in axis order x, y, z -- the edge from point c towards +axis is
 * owned by c.  The triangles follow the cubes in the same memory order of their lowest corner (x <= W, y <= H, z <= D), within
 * a cube the triangles of fs_surface_case_table in table order, the three indices in table order.  (PARITY UNPINNED against
 * scikit-image stays true: this is the library's own order, restated in tests/surface_model.py.)
 * Without a crossing edge -- a level above or below every value, +-Inf or NaN on a finite field -- the mesh is empty: 0 vertices,
 * 0 triangles.  The mesh is closed when no cell on the padded boundary is inside (for vortex sources with level >= 0 that
 * always holds); otherwise it is open along the faces of the padded box and nowhere else.  The handle keeps the result in a slot of its own: a later
 * fs_obstacle_surface does not replace it, nor the reverse.  fs_isosurface(FS_OBS, 0.5) is fs_obstacle_surface's mesh, byte
 * for byte.  Single-GPU handles only (slab handles: FS_EINVAL).
 * fs_isosurface_fetch: copies the last result, as fs_obstacle_surface_fetch does.
 */
enum {
    FS_VORTEX_WX = 0, FS_VORTEX_WY = 1, FS_VORTEX_WZ = 2, FS_VORTEX_W2 = 3, FS_VORTEX_Q = 4,
    FS_VORTEX_NFIELDS = 5,
    FS_ISO_VORTEX = 512    /* or-ed with an FS_VORTEX_* selector: a source of fs_isosurface */
};
int fs_vortex_field(fs_sim* s, int which, void* dst, size_t n_elems, int elem_size);
int fs_vortex_dump(fs_sim* s, const char* dir);
int fs_isosurface(fs_sim* s, int source, double level, long* n_vertices, long* n_triangles);
int fs_isosurface_fetch(fs_sim* s, float* vertices, int* triangles);

/* ---- vorticity confinement (beyond the reference: it has no body force of this kind, no file:line counterpart) ----
 *
 * Fedkiw, Stam and Jensen's remedy (2001) for the vortices that semi-Lagrangian advection smears out: a body force
 * eps * h * (N x omega) that pushes velocity back into the vortex cores, N the unit vector up the gradient of |omega|.
 * INPUTS: v_x, v_y, v_z as stored -- padded, ghosts and solid cells as they are -- and obs; dt; a strength eps >= 0.
 * All arithmetic is fp64 on the stored values widened, for fp32 and fp64 handles alike, one rounding per written operation,
 * in exactly this order, without contraction.  A TARGET cell is an interior cell (1..w, 1..h, 1..d) with obs != 1.
 * CURL: omega = (WX, WY, WZ) of a target cell exactly as under "vortex identification" above (cell units).
 * MAGNITUDE: m = sqrt((WX*WX + WY*WY) + WZ*WZ), the correctly rounded square root.
 * NEIGHBOUR MAGNITUDES: for each of the six face neighbours n of a target cell c, m_n is the neighbour's m where the neighbour
 * is a target cell, else the cell's own m_c (a zero-gradient extension at walls and solids).  "Is a target cell" is read from
 * the cell's flag byte: the neighbour is interior and its obs == 0, which for a mask of 0 and 1 is the same thing.  No omega
 * is ever needed in a ghost or solid cell, so nothing outside the padded box is read.
 * GRADIENT: ex = 0.5 * (m_xp - m_xm), ey and ez likewise; e2 = (ex*ex + ey*ey) + ez*ez.
 * DEGENERATE CASE: if !(e2 > 0) -- zero, underflow, NaN -- the cell keeps its three stored values bit for bit (-0.0 too).
 * FORCE: otherwise len = sqrt(e2), N = (ex / len, ey / len, ez / len) with correctly rounded divisions, and
 *     f = N x omega = (Ny*WZ - Nz*WY, Nz*WX - Nx*WZ, Nx*WY - Ny*WX),   each component two rounded products and one subtraction.
 * UPDATE: k = (double)dt * eps, computed on the host and rounded once;  v_a' = (T)((double)v_a + k * f_a) for a = x, y, z, T the
 * handle's precision.  This is eps * h * (N x omega) * dt with omega in cell units: the cell size h cancels.
 * Every cell's update reads only the old fields (the pass is out of place).  Non-target cells keep their stored values.
 * BOUNDARIES: afterwards v_x, v_y, v_z are exactly as fs_set_bounds(1, FS_VX), (2, FS_VY), (3, FS_VZ) would leave them: ghost
 * faces recomputed from the new values, then solid cells and fluid cells beside a solid zeroed.
 * A uniform shear has constant m, so e2 == 0 and the pass leaves its interior alone; a zero field likewise.  The effect on a
 * flow is not monotone in eps: start near 0.25 and look at fs_vortex_field.
 *
 * fs_confine_vorticity: one such pass now, with the given strength, whatever the option "vorticity_confinement" says.  One
 * fused z-marching HIP kernel (timing family "confinement"), three result arrays from the handle's own array pool; nothing is
 * allocated.  epsilon == 0 is a no-op that launches nothing; a negative or non-finite epsilon is FS_EINVAL.  Works under
 * every solver mode and both precisions.  Single GPU only: on a handle with a communicator (the FSNULL one included) it is
 * FS_EINVAL -- the stencil needs two halo planes of three fields.  With the option off a step launches and allocates nothing
 * for it.  fs_get_int "confinement_passes" counts the passes done, those inside steps included.
 */
int fs_confine_vorticity(fs_sim* s, double epsilon);

/* ---- heat and buoyancy (beyond the reference: it transports one passive scalar and has no body force) ----
 *
 * A temperature theta, carried and diffused like the reference's density, heated at the inlet and at the walls of bodies, and
 * the second force of Fedkiw, Stam and Jensen (2001): f = (-alpha * q + beta * theta) * up, q the smoke density.  theta is
 * the EXCESS over ambient: 0 means ambient, so the boundary rule b = 0 (solid cells zero, ghost faces copied) reads "bodies at
 * ambient, adiabatic box walls".  Default off: a handle that never switches heat on allocates and launches nothing for it.
 * Single GPU only: with a communicator (the FSNULL one included) every entry below, and fs_step with heat on, is FS_EINVAL.
 * Both precisions, every solver mode (solver=mg relaxes the temperature system as it relaxes the other diffusion systems).
 *
 * fs_heat_params: all parameters in one atomic call, n == FS_HEAT_PARAMS; a bad n or entry is FS_EINVAL with a message naming
 * the first bad entry, and nothing changes.  Every entry must be finite.
 *    par[0]  mode: 0 = off (theta is freed), 1 = manual (theta exists, the passes run only when called), 2 = in fs_step.
 *            Switching between 1 and 2 keeps theta; switching on allocates theta = 0.
 *    par[1]  kappa >= 0, the thermal diffusivity;  par[2] beta >= 0, buoyancy per unit theta;  par[3] alpha >= 0, weight per
 *            unit smoke density;  par[4] up: 0..5 = +x, -x, +y, -y, +z, -z.
 *    par[5]  theta_in, forced on the inlet plane x = 1;  par[6] wall mode: 0 = bodies are not heated, 1 = HELD cells take
 *            par[7] theta_w;  par[8..13] a box x0, x1, y0, y1, z0, z1 in cells, 1 <= lo <= hi <= extent: only cells inside it
 *            are held (how one body of several is heated).
 *    par[14] records the per-step heat log keeps, 0 (off) .. 2^20.  A changed count clears the log.
 * fs_heat_params_get returns the values in force (before the first call: mode 0, up = +y, the box = the whole domain).
 *
 * A HELD cell: wall mode on, the cell is interior with obs != 1, has an interior 6-neighbour with obs == 1 (its flag byte
 * says so) and lies inside the box.
 *
 * PASS A, fs_heat_apply: one streaming HIP kernel, in place, per interior cell (x, y, z), solid or not; every intermediate is
 * fp64, every operation rounded once, in this order, without contraction; T is the handle's precision:
 *    1. t = theta;  if x == 1, t = (T)theta_in;  if the cell is HELD, t = (T)theta_w  (the wall wins over the inlet).
 *    2. only if beta != 0 or alpha != 0 (otherwise no velocity and no density is read or written, so -0.0 stays -0.0):
 *         b = beta * (double)t;  w = alpha * (double)q;  d = b - w;  f = (double)dt * d;
 *         v_up' = (T)((double)v_up + f) for up = +axis, (T)((double)v_up - f) for up = -axis;  the other two components stay.
 *    3. theta is left exactly as fs_set_bounds(0, .) would leave the array of t, v_up exactly as fs_set_bounds(1 + up / 2, .)
 *       would leave the array of v_up': ghost faces from the un-zeroed values, then cells with obs == 1 zeroed (for the
 *       velocity also their fluid neighbours).  The twelve box edges are not written or take +0.0.
 * PASS B, fs_heat_transport: no new arithmetic.  a = (T)dt * (T)kappa * (T)w * (T)h * (T)d left to right, c = 1 + 6a; the
 * reference's linear solver (0, theta, snapshot of theta, a, c) with the handle's acc and solver, then its advection (b = 0)
 * of the solved array by the velocities as they are.  The same bits as fs_linear_solver + fs_advect on a field.  It is not
 * one of the FS_RESIDUAL_LOG_SOLVES logged solves.
 * PASS C, fs_heat_budget: PLANE records of FS_HEAT_COLS = 9 doubles for z = 1..d into per_plane (may be NULL) and their
 * combination over increasing z into out.  Over the cells of plane z with obs != 1, theta widened to fp64:
 *    0 cells   1 sum theta   2 sum theta * theta   3 max theta (from -Inf, "if (a > m) m = a")   4 min theta (from +Inf)
 *    5 HELD cells   6 the conductive loss: over the HELD cells, s = 0, then s = s + (theta_c - theta_n) for each neighbour n in
 *    the order x-, x+, y-, y+, z-, z+ that is interior, has obs == 0 and is not HELD; the cell adds s
 *    7 outflow: sum of (double)v_x * theta over the column x = w   8 inflow: the same over x = 1.
 * ORDER: a COLUMN (z, x) adds its cells in increasing y from 0; a PLANE combines the columns' values in increasing x, the
 * WHOLE record the planes' in increasing z (the flow monitor's order).  Times kappa and the cell size, column 6 is the heat
 * flux off the heated walls: the numerator of a Nusselt number.
 * fs_heat_log: with par[14] > 0 every fs_step in mode 2 ends with a record { step, the 9 numbers of out } on a device ring,
 * written without a host synchronisation; the fetch has the shape of fs_monitor_log and drains the log.
 *
 * fs_step in mode 2: confinement (if on), pass A, the reference's step exactly as without heat, pass B, the log record, the
 * samplers.  It is bit-identical to fs_heat_apply, fs_step, fs_heat_transport on a mode-1 handle.
 * fs_heat_get / fs_heat_set: theta as a dense padded array under fs_get_field's rules for n_elems and elem_size; no bounds
 * are applied on set.  FS_SOURCE_HEAT is theta as a source of fs_sample, fs_tracer_sample, the image and volume entries and
 * fs_isosurface (FS_EINVAL while heat is off).  Timing family "heat"; fs_get_int "heat_mode", "heat_applies",
 * "heat_transports".
 */
#define FS_HEAT_PARAMS 15
#define FS_HEAT_COLS 9
#define FS_HEAT_LOG_COLS 10
#define FS_SOURCE_HEAT 8192   /* the temperature as a source of fs_sample, the image and volume entries and fs_isosurface */
int fs_heat_params(fs_sim* s, const double* par, int n);
int fs_heat_params_get(fs_sim* s, double* par, int n);
int fs_heat_apply(fs_sim* s);
int fs_heat_transport(fs_sim* s);
int fs_heat_budget(fs_sim* s, double out[FS_HEAT_COLS], double* per_plane);
int fs_heat_log(fs_sim* s, double* rows, long max_rows, long* n_rows, long* n_dropped);
int fs_heat_get(fs_sim* s, void* dst, size_t n_elems, int elem_size);
int fs_heat_set(fs_sim* s, const void* src, size_t n_elems, int elem_size);

/* ---- momentum zones (beyond the reference: it can put nothing into the flow that is not a solid voxel) ----
 *
 * A zone is a region of cells with a momentum source and a resistance: a screen, a honeycomb, a radiator as a porous block, a
 * fan, a rotor as an actuator disk, a sponge layer in front of the outlet.  Up to FS_ZONE_MAX = 8 zones, each a row of
 * FS_ZONE_PARAMS = 20 finite doubles.  Default off: a handle without zones allocates and launches nothing for them.  Single
 * GPU only: with a communicator (the FSNULL one included) every entry below but switching off, and fs_step with zones on, is
 * FS_EINVAL.  Both precisions, every solver mode.  Zones hold no state: a resumed run needs nothing of them.
 *
 * A ZONE'S ROW:
 *    par[0]      shape: 0 = box, 1 = cylinder;   par[1] axis: 0, 1, 2 = x, y, z -- the cylinder's axis and the direction of the
 *                flux column of the budget.
 *    par[2..7]   the box x0, x1, y0, y1, z0, z1 in whole cells, 1 <= lo <= hi <= extent.  A cylinder is clipped to it too: that
 *                is its length.
 *    par[8], [9] the cylinder's centre c1, c2 in cell coordinates (doubles) on the two axes other than `axis`, lower axis first;
 *    par[10]     its radius >= 0.
 *    par[11..13] the acceleration g (any finite value);   par[14..16] the linear resistance D_a >= 0 per axis;
 *    par[17..19] the quadratic resistance F_a >= 0 per axis.
 * IN: cell (x, y, z) is IN zone k if it is inside the box and, for a cylinder, p*p + q*q <= R2, all three values rounded
 * doubles: p = (double)i - c1 and q = (double)j - c2 with i, j the cell's indices on the two other axes (lower axis first),
 * R2 = radius * radius computed once on the host.
 * A TARGET cell is an interior cell whose flag byte has neither F_SOLID nor F_NEAR: obs != 1 and no interior 6-neighbour with
 * obs == 1.  The other interior cells end at 0 under setBounds(1..3) anyway.
 *
 * THE PASS, fs_zone_apply: one streaming HIP kernel over v_x, v_y, v_z, in place.  All arithmetic is fp64 on the stored values
 * widened, for fp32 and fp64 handles alike; every written operation is rounded once, in this order, without contraction.
 * DT = (double)dt; G_a = DT * g_a, computed per zone on the host.  A target cell that is in no zone keeps its three stored
 * values bit for bit (-0.0 too).  A target cell in at least one zone starts with u = (double)v and goes through its zones in
 * increasing index, each STAGE reading the previous stage's fp64 result:
 *     k0 = (ux*ux + uy*uy) + uz*uz;   m = sqrt(k0)   (correctly rounded)
 *     for a = x, y, z:   n = u_a + G_a;  r = F_a * m;  s = D_a + r;  t = DT * s;  d = 1.0 + t;  u_a' = n / d
 *     k1 = (ux'*ux' + uy'*uy') + uz'*uz'
 * and after the last stage v_a = (T)u_a, T the handle's precision.  The denominators are >= 1: the implicit form is stable for
 * any D, F and dt, so a sponge may be as stiff as one likes.  (x / 1.0 is x: an implementation may skip the divisions of a
 * zone with D = F = 0 where m is finite.)  Afterwards the three arrays are exactly as fs_set_bounds(1, FS_VX), (2, FS_VY),
 * (3, FS_VZ) would leave them: ghost faces from the un-zeroed values -- the stored ones where the cell is no target cell --
 * then solid cells and their fluid neighbours zeroed.  One formula covers every use: a fan is g; a porous block D and F; a
 * flow straightener a large D on the two transverse axes; a rotor disk F on its axis; a sponge D ramped over a few thin zones.
 *
 * THE BUDGET, fs_zone_budget: a pure function of the present state -- what a pass now would do; no field is written.  Per zone
 * FS_ZONE_COLS = 7 doubles over the target cells in the zone, from that zone's stage as defined above (the earlier zones'
 * stages are applied first):
 *    0 cells   1, 2, 3 sum of u_a' - u_a   4 sum of 0.5 * (k1 - k0)   5 sum of u_axis, the stage's input
 *    6 max of m, by "if (a > m) m = a" from -Inf.
 * ORDER: the flow monitor's.  A COLUMN (z, x) adds its cells in increasing y from +0.0; a PLANE combines its columns in
 * increasing x, the WHOLE the planes in increasing z.  Cells outside the zone are skipped, not added as zeros (a column without
 * cells is +0.0, or -Inf in column 6).  out takes n_zones * 7 doubles, [zone][column]; per_plane, which may be NULL, d * n_zones
 * * 7 doubles, [z - 1][zone][column].  INTEGRATION.md section 6m converts them to thrust, power and volume flux.
 *
 * fs_zones: the zones (n_zones rows of 20 at par), the mode -- 0 off, 1 manual (the pass runs only when called), 2 in fs_step --
 * and the records the per-step zone log keeps (0 = off .. 2^20), in one atomic call: a bad value is FS_EINVAL with a message
 * that names the zone and the entry, and nothing changes.  n_zones == 0 or mode 0 frees everything (par may be NULL).  A changed
 * record or zone count clears the log.  fs_zones_get returns the zones in force: the rows into par (room for FS_ZONE_MAX rows;
 * may be NULL), their count, the mode and the log's record count (each may be NULL).
 * fs_step in mode 2: confinement (if on), heat's pass A (if on), the zone log's record -- the budget of the state the pass is
 * about to change, { the running step's number, n_zones * 7 } -- the zone pass, then the reference's step exactly as without
 * zones.  It is bit-identical to fs_zone_apply, fs_step on a mode-1 handle.
 * fs_zone_log: the rows { step, n_zones * 7 } on a device ring written without a host synchronisation; the fetch has the shape
 * of fs_heat_log and drains the log.
 * fs_zone_mask: n = the padded size, one byte per cell as fs_get_field orders them; bit k is set where the cell is a target
 * cell in zone k; ghost cells take 0.
 * Timing family "zones"; fs_get_int "zone_mode", "zone_applies" (passes done, those inside steps included).
 */
#define FS_ZONE_MAX 8
#define FS_ZONE_PARAMS 20
#define FS_ZONE_COLS 7
int fs_zones(fs_sim* s, const double* par, int n_zones, int mode, int log);
int fs_zones_get(fs_sim* s, double* par, int* n_zones, int* mode, int* log);
int fs_zone_apply(fs_sim* s);
int fs_zone_budget(fs_sim* s, double* out, double* per_plane);
int fs_zone_log(fs_sim* s, double* rows, long max_rows, long* n_rows, long* n_dropped);
int fs_zone_mask(fs_sim* s, uint8_t* dst, size_t n);

/* ---- turbulent inflow (beyond the reference: its only inflow is (speed, 0, 0) on the x = 1 face, simulation.cpp:103-105) ----
 *
 * An inflow generator for boundary layers, gusts and free-stream turbulence.  With option "inflow" = "on" fs_step writes, where
 * the reference's step writes (speed, 0, 0) -- after the confinement pass, before the pre-diffusion snapshot -- to every cell
 * (1, y, z), y in 1..h, z in 1..d, solid or not (the step's own setBounds calls deal with solids afterwards), at step number t =
 * the steps this handle has completed:
 *     v_x = (T)( g(t) * U(y,z) + r(y,z) * u'_x(y,z,t) )     v_y = (T)( r(y,z) * u'_y(y,z,t) )     v_z = (T)( r(y,z) * u'_z(y,z,t) )
 * All arithmetic is fp64, one rounding per written operation, in exactly the order written here, without contraction; T, the
 * handle's precision, enters in the last rounding only.  The stream is STATELESS: the plane is a pure function of the
 * parameters and t, so a resumed run continues it and no launch shape can change a bit.
 * MAPS: U and r are h x d doubles, index (z-1)*h + (y-1); a missing U is (double)speed everywhere, a missing r is 1.
 * GUST: g(t) from up to FS_INFLOW_KNOTS_MAX knots (t_i, f_i), t_i strictly increasing; with x = (double)t: f_0 where x <= t_0,
 * f_last where x >= t_last, else for t_i <= x < t_(i+1):  f_i + (f_(i+1) - f_i) * ((x - t_i) / (t_(i+1) - t_i)).  No knots: 1.
 * Evaluated on the host.
 * FLUCTUATIONS: the synthetic-eddy method of Jarrin, Benhamadouche, Laurence and Prosser (2006) with isotropic eddies of one
 * radius.  Parameters: N eddies, radius sigma >= 1, strength u_rms >= 0, convection c >= 0 cells per step, a 64-bit seed.
 * The eddies live in the box x in [1-sigma, 1+sigma), y in [1-sigma, h+sigma), z in [1-sigma, d+sigma); with two = 2.0*sigma,
 * Ly = (double)(h-1) + two, Lz = (double)(d-1) + two its volume is V = (two * Ly) * Lz.
 * HASH: on 64-bit unsigned integers modulo 2^64, MIX(z): z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9; z = (z ^ (z >> 27)) *
 * 0x94D049BB133111EB; z ^ (z >> 31) (splitmix64's finaliser).  With G = 0x9E3779B97F4A7C15,
 *     HASH(k, gen, draw) = MIX( MIX( MIX(seed + G*(k+1)) + G*gen ) + G*(draw+1) ),     UNI(hash) = (double)(hash >> 11) * 2^-53.
 * EDDY k (0 <= k < N) AT STEP t:  u0 = UNI(HASH(k, 0, 0));  start = u0 * two;  moved = (double)t * c;  s = start + moved;
 * q = s / two;  gen = floor(q);  base = gen * two;  rem = s - base;  if rem < 0: rem = 0;  if not rem < two: rem = 0 and gen =
 * gen + 1 (either can happen only by the rounding of q or base).  Then
 *     ex = (1 - sigma) + rem,   ey = (1 - sigma) + UNI(HASH(k, gen, 1)) * Ly,   ez = (1 - sigma) + UNI(HASH(k, gen, 2)) * Lz,
 * and the sign eps_j of component j = 0, 1, 2 (x, y, z) is -1 where bit 63 of HASH(k, gen, 3 + j) is set, else +1.  An eddy
 * is so reborn at another (ey, ez) with other signs each time it leaves the box, however many times per step.  gen must stay
 * below 2^53: a step number with ((double)t * c) / two + 2 >= 2^53, or a negative one, is FS_EINVAL.
 * TENT: f(rho) = K * max(0, 1 - |rho|) with K = sqrt(3/2) correctly rounded (1.2247448713915890), so the integral of f^2 is 1.
 * AMPLITUDE: A = u_rms * sqrt(V / ((double)N * ((sigma*sigma)*sigma))), correctly rounded square root; it must be finite.
 * With inv = 1.0 / sigma:  ax_k = A * f((1 - ex_k) * inv),  and for the cell (y, z):
 *     w_k = (ax_k * f(((double)y - ey_k) * inv)) * f(((double)z - ez_k) * inv),        u'_j = sum over k of eps_j,k * w_k,
 * the sum in ascending k from +0.0, one addition per eddy (eps * w is exact).  An eddy with w_k == 0 adds +-0 and changes no bit,
 * which is what lets an implementation skip it.  E[u'_j^2] = u_rms^2 at every inlet cell, those at the plane's edges included
 * (the box is padded by sigma), and the three components are uncorrelated.
 *
 * fs_inflow_profile: sets both maps (n = h * d values each; a null pointer = that map is not given); a wrong n or an entry that
 * is not finite is FS_EINVAL and changes nothing.  fs_inflow_gust: sets the schedule (n = 0 clears it); knots out of order or
 * not finite, or more than FS_INFLOW_KNOTS_MAX, are FS_EINVAL and change nothing.  fs_inflow_plane: the three fp64 components
 * before the last rounding for any step number, n = 3 * h * d values, component j of cell (y, z) at j*h*d + (z-1)*h + (y-1);
 * works whether the option is on or off, changes no field and no counter but the timing family.  fs_inflow_eddies: n = 6 * N
 * values, per eddy ex, ey, ez and the three signs as -1.0 / +1.0 (tests, plotting).  Two HIP kernels per plane (the eddy
 * table, then the plane: a workgroup per 16 x 16 patch keeps the eddies that can reach it, in order; timing family "inflow",
 * one launch counted per plane).  The maps and the table are allocated at the first use; with the option off a step launches
 * and allocates nothing for it and is the step it was.  Every solver mode, both precisions.  Single GPU only: with a
 * communicator fs_step (option on), fs_inflow_profile, fs_inflow_plane and fs_inflow_eddies are FS_EINVAL.
 */
#define FS_INFLOW_EDDIES_MAX 65536
#define FS_INFLOW_KNOTS_MAX 4096
int fs_inflow_profile(fs_sim* s, const double* u, const double* rms, size_t n);
int fs_inflow_gust(fs_sim* s, const double* steps, const double* factor, int n);
int fs_inflow_plane(fs_sim* s, long step, double* out, size_t n);
int fs_inflow_eddies(fs_sim* s, long step, double* out, size_t n);

/* ---- point probes and field sampling (beyond the reference: it evaluates a field off the grid only inside advect) ----
 *
 * COORDINATES are the viewer's, as for fs_streamlines and fs_obstacle_surface: indices into the padded array, x first.  A cell's
 * value sits at its integer coordinates; the box is [0, w+1] x [0, h+1] x [0, d+1].
 * THE VALUE AT A POINT (x, y, z), in fp64; every written operation is rounded once, in exactly this order, without contraction
 * (the library is built with -ffp-contract=off):
 *     NaN (all modes) if a coordinate is NaN, below 0, or above w+1 / h+1 / d+1;
 *     i0 = min(floor(x), w), sx = x - i0 (exact), tx = 1.0 - sx; likewise j0, sy, ty with h and l0, sz, tz with d;
 *     v_abc = the stored value at (i0+a, j0+b, l0+c), widened to double.
 * FS_SAMPLE_NEAREST: v_abc with a = (sx >= 0.5), b = (sy >= 0.5), c = (sz >= 0.5): the exact stored value.
 * FS_SAMPLE_LINEAR: the reference's lerp form (simulation.cpp:412-420), x, then y, then z:
 *     c_bc = v_0bc*tx + v_1bc*sx        d_c = c_0c*ty + c_1c*sy        r = d_0*tz + d_1*sz
 * Every corner is multiplied: a NaN or infinite corner gives NaN even where its weight is 0.
 * FS_SAMPLE_FLUID: w_abc = ((a ? sx : tx) * (b ? sy : ty)) * (c ? sz : tz); a corner COUNTS when w_abc > 0 and obs(corner) != 1
 * (FS_OBS as it is now); num = sum of w*v and den = sum of w over the counting corners in memory order (c outer, b, a inner),
 * both starting from +0.0; r = num / den, or NaN if no corner counts.  The mode for points on an obstacle's surface, where solid
 * cells hold p = 0 and carry half of the trilinear weight: at the midpoint of an edge between a solid and a fluid cell it returns
 * exactly the fluid cell's value (0.5 v / 0.5).
 * SOURCES: a field selector 0 .. FS_NFIELDS - 1; FS_ISO_VORTEX | FS_VORTEX_* (the field is computed first, exactly as
 * fs_isosurface does); FS_SAMPLE_STAT | sel, sel with the selectors, FS_STAT_RAW and the errors of fs_flow_stats_field (the fp64
 * derived field is sampled as it is, not rounded to the handle's precision).  The output is always fp64.
 *
 * fs_sample_points: keeps n points (xyz[3 * k + ..] = x, y, z) on the device until they are replaced; n = 0 .. 2^24, else FS_EINVAL.
 * fs_sample: evaluates the source at the kept points into out[n]; n must equal the kept count.  One HIP kernel, one thread per
 * point; it changes no field.  Both are for single-GPU handles only (slab handles: FS_EINVAL).
 *
 * PROBES are cells, not points, so that ownership and bits are unambiguous.  fs_set_probes sets the probe list to n cells
 * (cells_xyz[3 * k + ..] = x, y, z), n = 0 (off) .. FS_PROBE_MAX, in integer padded global coordinates -- the numbers the
 * mutators use, ghost cells 0 and N+1 allowed, anything else FS_EINVAL; it replaces the list and clears the log.  Option
 * "probe_log" = N (0 .. 1048576) keeps the last N records; setting it (re)allocates and clears the ring.  Either is legal at any
 * time, and either is FS_EINVAL if N * n * 40 bytes would exceed 1 GiB.  With no probes or N = 0 a step launches and allocates
 * nothing for it.
 * A RECORD holds, per probe, {q, u, v, w, p} = dens, v_x, v_y, v_z, FS_PRESSURE: the stored values widened to fp64, exact.
 * fs_step takes one at the sample point of the flow statistics above -- after advect(0, dens, buffer) (simulation.cpp:136),
 * before the frame dump, p as the second projection left it -- by one launch on the step's own stream into a device ring,
 * without a host synchronisation.  fs_probe_sample takes one record of the state as it is now.
 * fs_probe_log drains the log: rows[(1 + FS_PROBE_VALUES * n) * i + ...] = {step, then q, u, v, w, p of each probe in list
 * order}.  step, oldest-first order, rows = NULL, max_rows and *n_dropped are as for fs_force_log.  fs_get_int "probe_count"
 * reports n; timing family "probes" counts one launch per record, 0 with the feature off.
 * On z-slab handles the owner of a probe is the rank that owns its global plane (z = 0: rank 0; z = d+1: the last rank) and
 * only the owner's value is used; every rank makes the same calls, the drain is collective and every rank receives the same
 * rows (FSNULL transport: FS_EINVAL).  A record is the stored value itself: a slab run gives the single-GPU bits, and launch
 * shape cannot matter.
 */
enum { FS_SAMPLE_NEAREST = 0, FS_SAMPLE_LINEAR = 1, FS_SAMPLE_FLUID = 2 };
#define FS_SAMPLE_STAT 1024   /* or-ed with an FS_STAT_* selector (and FS_STAT_RAW): a source of fs_sample */
#define FS_PROBE_MAX 4096
#define FS_PROBE_VALUES 5
int fs_sample_points(fs_sim* s, const double* xyz, long n);
int fs_sample(fs_sim* s, int source, int mode, double* out, long n);
int fs_set_probes(fs_sim* s, const int* cells_xyz, long n);
int fs_probe_sample(fs_sim* s);
int fs_probe_log(fs_sim* s, double* rows, long max_rows, long* n_rows, long* n_dropped);

/* ---- slice and projection images (the frames of the reference's 2-D viewer, gui.py:61-79 and 257-295, which it builds on
 *      the host from dumped volumes, one z-slice at a time; projections, the log and the PNG writer are beyond it) ----
 *
 * IMAGE GEOMETRY.  axis is 0 (x), 1 (y) or 2 (z).  The image spans the padded extents of the other two axes; columns run along
 * the lower remaining axis, rows along the higher one:
 *     axis z: cols = w+2, rows = h+2, pixel (r, c) is x = c, y = r
 *     axis y: cols = w+2, rows = d+2, pixel (r, c) is x = c, z = r
 *     axis x: cols = h+2, rows = d+2, pixel (r, c) is y = c, z = r
 * Row 0 comes first in memory, there is no flip: field[frame, slice] as gui.py:272 indexes it.
 *
 * THE VALUE IMAGE is fp64, rows * cols; the source's stored values are widened exactly.  With N the interior extent of the
 * axis and v_k the stored value of the pixel's column at padded index k along it:
 *     FS_IMG_SLICE   v_index, index = 0 .. N+1.
 *     FS_IMG_SUM     s = +0.0; for k = 1 .. N (increasing): s = s + v_k.  One rounding per add; interior cells of the axis
 *                    only, whatever they hold.
 *     FS_IMG_MAX     m = -inf; for k = 1 .. N: if (v_k > m) m = v_k.  NaN is never taken; of equal values the first stays.
 *     FS_IMG_MIN     m = +inf; for k = 1 .. N: if (v_k < m) m = v_k.
 * For SUM, MAX and MIN index must be 0.  The order along the axis is strictly sequential on all three axes: a pixel is a
 * pure function of its column of cells, and launch shape cannot change a bit.
 * THE OBSTACLE FLAG of a pixel: SLICE: obs > 0.5 at the slice cell; SUM, MAX, MIN: obs > 0.5 at any cell 1 .. N of the
 * column (the silhouette).
 * SOURCES are exactly those of fs_sample: a field selector 0 .. FS_NFIELDS - 1; FS_ISO_VORTEX | FS_VORTEX_* (the field is
 * computed first); FS_SAMPLE_STAT | sel, with the selectors, FS_STAT_RAW and the errors of fs_flow_stats_field.
 *
 * COLOURING.  The handle holds a colour table of n RGB triples, 2 <= n <= 4096 (fs_image_colormap; n = 0 restores the
 * default).  With vmin < vmax, both finite (else FS_EINVAL), in fp64, every operation rounded once, in this order:
 *     v NaN: (0, 0, 0);   otherwise   c = v < vmin ? vmin : (v > vmax ? vmax : v),   t = (c - vmin) / (vmax - vmin),
 *     k = min(n - 1, (int)(t * n)),   rgb = table[k].
 * If the pixel's obstacle flag is set and obstacle_alpha > 0 (obstacle_alpha in [0, 1], else FS_EINVAL): f = (float)(1.0 -
 * obstacle_alpha), and each byte b becomes (uint8)((float)b * f) (truncation).  These are the bytes of the 2-D viewer's
 * apply_cmap followed by overlay_obstacle (gui.py:61-79; checked against numpy 2.2 / matplotlib 3.10, whose Normalize works
 * in fp64 on float32 input; n = 256, obstacle_alpha = 0.2).
 * THE DEFAULT TABLE is the 256 triples matplotlib builds for the viewer's seven colour stops (gui.py:38-41): the first is
 * (255,255,255), entry 127 is (0,190,252), the last (255,0,0).  It is written out in csrc/image.h, not recomputed.
 *
 * fs_image_values / fs_image_rgb: one image of the state as it is now, out[rows * cols] doubles / out[rows * cols * 3]
 * bytes; *cols and *rows (may be NULL) receive the geometry, and out = NULL only reports them.  A wrong size, kind, axis,
 * index or source is FS_EINVAL.  Single-GPU handles only (slab handles: FS_EINVAL).  They change no field.
 * fs_image_png writes an 8-bit RGB, non-interlaced PNG: one IDAT chunk whose zlib stream consists of stored deflate blocks
 * only, filter type 0 on every scanline, correct Adler-32 and CRCs, no zlib dependency; the bytes are a pure function of the
 * pixels.  Needs neither a handle nor a GPU.
 *
 * THE IMAGE LOG.  fs_image_views sets n = 0 .. FS_IMAGE_VIEWS_MAX views: spec[4 k + ..] = {source, kind, axis, index},
 * range[3 k + ..] = {vmin, vmax, obstacle_alpha}, all validated at the call; it replaces the list and clears the log.  A
 * FRAME is the views' RGB images one after the other in list order.  Options (fs_set_option, any time): "image_log" = N, 0
 * (default: off, a step launches and allocates nothing for it) .. 65536 frames kept; "image_every" = K >= 1 (default 1).
 * Setting "image_log" or the views reallocates and clears the ring; either is FS_EINVAL if N * (bytes of one frame) would
 * exceed 1 GiB.  fs_step takes a frame at the sample point of the flow statistics and the probes -- after advect(0, dens,
 * buffer) (simulation.cpp:136), before the frame dump -- when (steps_total - 1) % K == 0, into a device ring on the step's
 * own stream, without a host synchronisation.  fs_image_sample takes one frame of the state as it is now.
 * fs_image_log drains the log: frames[i * frame bytes + ..], oldest first, with steps[i] (may be NULL) the steps the handle
 * had completed; frames = NULL, max_frames and *n_dropped (overwritten frames) are as for fs_force_log.  fs_get_int
 * "image_frame_bytes" and "image_views" report the frame size and the view count; timing family "images" counts one launch
 * per rendered view of the log, 0 with the feature off.
 */
enum { FS_IMG_SLICE = 0, FS_IMG_SUM = 1, FS_IMG_MAX = 2, FS_IMG_MIN = 3 };
#define FS_IMAGE_VIEWS_MAX 8
int fs_image_values(fs_sim* s, int source, int kind, int axis, int index, double* out, size_t n, int* cols, int* rows);
int fs_image_rgb(fs_sim* s, int source, int kind, int axis, int index, double vmin, double vmax, double obstacle_alpha,
                 uint8_t* out, size_t n_bytes, int* cols, int* rows);
int fs_image_colormap(fs_sim* s, const uint8_t* rgb, int n);      /* n = 0: back to the default table */
int fs_image_png(const uint8_t* rgb, int cols, int rows, const char* path);   /* needs neither a handle nor a GPU */
int fs_image_views(fs_sim* s, const int* spec, const double* range, int n);
int fs_image_sample(fs_sim* s);
int fs_image_log(fs_sim* s, uint8_t* frames, long* steps, long max_frames, long* n_frames, long* n_dropped);

/* ---- tracer particles (beyond the reference: it follows no fluid parcel through time, no file:line counterpart) ----
 *
 * Particles released into the flow and carried by it as it evolves: pathlines (one particle's positions over time) and
 * streaklines (the particles one emitter has released), where fs_streamlines integrates one frozen field.
 * COORDINATES are the viewer's, as for fs_sample: indices into the padded array, x first.
 * THE BOX B is 0.5 <= c <= N + 0.5 on each axis (N = w, h, d): the range advect clamps its back-traces to
 * (simulation.cpp:388-390).  A NaN coordinate is outside B.
 * THE DISPLACEMENT per step of a parcel with velocity (u, v, w) is what advect traces back (simulation.cpp:384-386):
 *     k = ((double)dt * w, (double)dt * h, (double)dt * d)      exact: a 24-bit dt times an extent below 2^11
 *     h = 0.5 * k                                               exact as well
 * A PARTICLE occupies one slot of a pool of C slots (option "tracers" = C).  Its state is the position xyz[3 * slot + ..] in
 * fp64, and four int32 {status, source, born, moves}, status one of FS_TRACER_FREE (0), FS_TRACER_ALIVE (1), FS_TRACER_OUT
 * (2), FS_TRACER_HIT (3).
 * THE MOVE of an ALIVE particle at P, in fp64; every written operation is rounded once, in exactly this order, without
 * contraction.  LIN(f, P) is exactly FS_SAMPLE_LINEAR of field f at P as fs_sample defines it above:
 *     u1 = (LIN(v_x, P), LIN(v_y, P), LIN(v_z, P))
 *     M_a = P_a + h_a * u1_a                                    a = x, y, z
 *     if M is in B:  u2 = (LIN(v_x, M), LIN(v_y, M), LIN(v_z, M)),   P'_a = P_a + k_a * u2_a
 *     else:          P' = M
 *     status' = P' not in B ? OUT : (obs at cell (floor(P'_x + 0.5), floor(P'_y + 0.5), floor(P'_z + 0.5)) == 1 ? HIT : ALIVE)
 *     moves' = moves + 1
 * the explicit midpoint rule on the velocity field frozen at the sample point.  P' is stored whatever the status, so an OUT
 * particle shows where it left.  A NaN velocity gives NaN and hence OUT.  Slots that are not ALIVE are never touched again
 * until they are overwritten.  A particle's move is a pure function of its position, the 48 corner values, one obs value, dt
 * and the extents: launch shape cannot change a bit.
 *
 * fs_tracer_seed appends n particles (xyz[3 * k + ..] = x, y, z; n = 0 .. 2^24): status ALIVE, source -1, born = the steps
 * the handle has completed, moves 0.  The j-th particle ever seeded or released (since the pool was last cleared) goes into
 * slot j % C, so a full pool overwrites its oldest particles.  Every point must lie in B, else FS_EINVAL and nothing is
 * seeded.  obs is not looked at: a particle seeded inside a solid sits on zero velocity and becomes HIT at its first move.
 * fs_tracer_emitters keeps n = 0 (off) .. FS_TRACER_EMITTERS_MAX points in B as the emitters, with every >= 1 (anything else
 * FS_EINVAL); it replaces the list.  fs_tracer_clear sets every slot FREE and the seed counter to 0, and clears the log.
 * INSIDE fs_step, at the sample point of the flow statistics, the probes and the images -- after advect(0, dens, buffer)
 * (simulation.cpp:136), before the frame dump -- on the step's own stream, by one launch, without a host synchronisation:
 *     1. every ALIVE particle moves;
 *     2. if emitters are set and (steps_total - 1) % every == 0, one particle per emitter is appended in list order, with
 *        source = the emitter's index and born = steps_total (the steps completed, this one included); it is not moved in
 *        this step;
 *     3. if "tracer_log" is on and (steps_total - 1) % "tracer_every" == 0, the pool's positions and status words go into
 *        the snapshot ring.
 * The slot cursor is the host's: how many particles an advance appends is known without asking the device.
 * fs_tracer_advance does 1 - 3 on the state as it is now, for callers who drive the passes themselves; it releases and
 * takes a snapshot whatever the two schedules say (as fs_image_sample takes a frame), born and the frame's step being the
 * steps completed so far.
 * Options (fs_set_option, any time): "tracers" = C, 0 (default: off, a step launches and allocates nothing for it) ..
 * 4194304; setting it (re)allocates and clears the pool and the log.  "tracer_log" = N frames kept, 0 .. 65536; setting it
 * (re)allocates and clears the log.  "tracer_every" = K >= 1.  Setting "tracers" or "tracer_log" is FS_EINVAL if N * C *
 * FS_TRACER_FRAME_BYTES would exceed 1 GiB; if the device cannot provide the memory the call (or the first use of the handle)
 * is FS_ENOMEM and the option is 0 again.  fs_get_int: "tracer_capacity" = C, "tracer_count" = min(seeded, C),
 * "tracer_seeded" (saturates at 2^31 - 1), "tracer_emitters".
 * fs_tracer_fetch copies slots 0 .. count-1: xyz[3 * count], meta[4 * count] = {status, source, born, moves} per slot;
 * either array may be NULL, with both NULL it only reports *n = count; max < count is FS_EINVAL.
 * fs_tracer_sample evaluates any source of fs_sample, in any of its modes, at the particles' current positions into out[n]:
 * the sampler's kernel on the pool's own position array, no host round trip; n must equal the count.  Dead particles are
 * evaluated where they stopped; the sampler's own rule gives NaN outside [0, N + 1].
 * fs_tracer_log drains the snapshot ring, oldest frame first: xyz[(i * C + slot) * 3 + ..], status[i * C + slot], steps[i]
 * (may be NULL) the steps the handle had completed.  Both arrays NULL only reports the counts; max_frames and *n_dropped
 * (overwritten frames) are as for fs_image_log.
 * Timing family "tracers" counts one launch per advance, 0 with the feature off.  Single-GPU handles only: every entry and
 * option here is FS_EINVAL on a z-slab handle, and so is fs_comm_init on a handle whose "tracers" is on.
 */
enum { FS_TRACER_FREE = 0, FS_TRACER_ALIVE = 1, FS_TRACER_OUT = 2, FS_TRACER_HIT = 3 };
#define FS_TRACER_EMITTERS_MAX 4096
#define FS_TRACER_FRAME_BYTES 28   /* one slot of one snapshot frame: three fp64 coordinates and the status word */
int fs_tracer_seed(fs_sim* s, const double* xyz, long n);
int fs_tracer_emitters(fs_sim* s, const double* xyz, long n, long every);
int fs_tracer_clear(fs_sim* s);
int fs_tracer_advance(fs_sim* s);
int fs_tracer_fetch(fs_sim* s, double* xyz, int32_t* meta, long max, long* n);
int fs_tracer_sample(fs_sim* s, int source, int mode, double* out, long n);
int fs_tracer_log(fs_sim* s, double* xyz, int32_t* status, long* steps, long max_frames, long* n_frames, long* n_dropped);

/* ---- volume rendering (the picture the reference's 3-D viewer, GUI/gl_widget.py, has no way to draw: it shows streamlines and
 *      the obstacle mesh from a camera orbiting the box, gl_widget.py:26-28 and 64-76; a ray-marched view of a field is beyond it) ----
 *
 * A direct volume rendering of any source of fs_sample through an arbitrary set of rays: one HIP kernel, one thread per ray,
 * trilinear samples composited front to back with early termination, obstacles as shaded opaque surfaces.  It hands over
 * cols * rows * 3 bytes instead of a volume.  Everything is fp64; every written operation is rounded once, in exactly this
 * order, without contraction; the march uses + - * / and comparisons only.  A pixel is a pure function of its ray, the
 * parameters, the colour table and the cells it touches: launch shape cannot change a bit.
 * COORDINATES are the viewer's, as for fs_sample: indices into the padded array, x first; the box is [0, w+1] x [0, h+1] x
 * [0, d+1].  N_a below is the interior extent of axis a (w, h, d).
 *
 * RAYS.  A camera slot (0 .. FS_VOLUME_CAMERAS_MAX - 1) holds a ray set of cols x rows rays, 1 <= cols, rows <= 2048, on the
 * device until it is replaced: rays[6 * (r * cols + c) + ..] = {ox, oy, oz, dx, dy, dz}, row 0 first (the top of the image).
 * Any ray set is legal; length along a ray is measured in units of |d|.
 * fs_volume_rays stores the given rays; cols = rows = 0 frees the slot (FS_EINVAL while a view of the log uses it).
 * fs_volume_camera builds them on the host, with + - * / and sqrt only (the library holds no trigonometry):
 * cam[FS_VOLUME_CAMERA] = {eye[3], target[3], up[3], half_height, ortho}.  half_height > 0 is the half height of the image
 * plane: at unit distance for a perspective camera (tan(fov / 2)), in cells for an orthographic one (ortho != 0).
 *     F = target - eye              f_a = F_a / sqrt((F_x F_x + F_y F_y) + F_z F_z)
 *     R = f x up = (f_y up_z - f_z up_y, f_z up_x - f_x up_z, f_x up_y - f_y up_x)        r_a = R_a / sqrt((R.R)), summed as above
 *     u = r x f, the same pattern
 *     pixel (i, j), row i, column j:   sx = (((2 (j + 0.5)) / cols - 1) * half_height) * (cols / rows)
 *                                      sy = (1 - (2 (i + 0.5)) / rows) * half_height
 *     perspective:   o = eye,   V_a = (f_a + sx r_a) + sy u_a,   d_a = V_a / sqrt((V.V))
 *     orthographic:  o_a = (eye_a + sx r_a) + sy u_a,   d = f
 * A non-finite entry, half_height <= 0, or F.F or R.R zero or not finite is FS_EINVAL.
 * Replacing the rays of a slot that a view of the log uses clears the log.
 *
 * PARAMETERS of a view: par[FS_VOLUME_PARAMS] = {vmin, vmax, opacity, step, t_min, obst_r, obst_g, obst_b, back_r, back_g,
 * back_b}, all finite: vmin < vmax; opacity >= 0; step > 0; 0 <= t_min < 1; the six colours in [0, 255]; and with diag =
 * sqrt((((w+1)^2 + (h+1)^2) + (d+1)^2)) and q = diag / step: q <= FS_VOLUME_SAMPLES_MAX.  Anything else is FS_EINVAL.
 * KMAX = (long)q + 2 is the march's loop limit: more samples than a ray with |d| >= 1 can take through the box (a ray with
 * |d| < 1 is cut off there), so no ray can spin.
 *
 * ONE RAY.  An INVALID ray -- a component of o or d not finite, or d = 0 -- and a ray that MISSES give acc = {0, 0, 0, 1}.
 * Box: t0 = 0, t1 = +inf; per axis a, in the order x, y, z:  d_a == 0: the ray misses unless 0 <= o_a <= N_a + 1;  otherwise
 *     ta = (0 - o_a) / d_a,  tb = ((N_a + 1) - o_a) / d_a,  t0 = max(t0, min(ta, tb)),  t1 = min(t1, max(ta, tb)).
 * The ray misses unless t0 < t1.
 * March: T = 1, C = (0, 0, 0); for k = 0, 1, .. KMAX - 1:
 *     tk = t0 + ((double)k + 0.5) * step; stop when !(tk < t1)                  (no running sum)
 *     p_a = o_a + tk * d_a, clamped to [0, N_a + 1]
 *     the nearest cell is i_a = (int)(p_a + 0.5); S(cell) = 1 where obs > 0.5 (image_solid), else 0.
 *     SOLID SAMPLE, if S(i) = 1:
 *         g_x = S(i_x + 1, i_y, i_z) - S(i_x - 1, i_y, i_z), likewise g_y, g_z; a neighbour outside the padded array counts 0
 *         n2 = g.g;  shade = 1 if n2 == 0, else s = 0.3 + 0.7 * (|(g_x d_x + g_y d_y) + g_z d_z| * RN[n2]), shade = s < 1 ? s : 1,
 *         RN[1 .. 3] = 1, 0.7071067811865476, 0.5773502691896257
 *         C_c = C_c + T * (obst_c * shade);  T = 0;  stop.
 *     FLUID SAMPLE otherwise: v = FS_SAMPLE_LINEAR of the source at p, exactly as fs_sample defines it (the clamped p is
 *     always inside).  If v is not NaN:
 *         cl = v < vmin ? vmin : (v > vmax ? vmax : v);  tn = (cl - vmin) / (vmax - vmin);  ao = (opacity * tn) * step;
 *         a = ao < 1 ? ao : 1;  if a > 0:  col = table[k], k the colour index of v under COLOURING above (the handle's table,
 *         fs_image_colormap);  w = T * a;  C_c = C_c + w * col_c;  T = T * (1 - a).
 *     Then stop if T < t_min.
 * Outputs: acc = {C_r, C_g, C_b, T}, before the background is added; byte_c = (uint8) min(255, (C_c + T * back_c) + 0.5).
 *
 * fs_volume_render: one image of the state as it is now through the rays of `slot`: rgb[rows * cols * 3] bytes and
 * acc[rows * cols * 4] doubles; either may be NULL; n_bytes / n_acc must be those counts (FS_EINVAL otherwise, and for an empty
 * slot).  SOURCES are exactly those of fs_sample, with its errors.  It changes no field.
 *
 * THE VOLUME LOG, shaped like the image log.  fs_volume_views sets n = 0 .. FS_VOLUME_VIEWS_MAX views: spec[2 k + ..] =
 * {source, slot}, par[FS_VOLUME_PARAMS * k + ..] the view's parameters, all validated at the call (the slot must hold rays); it
 * replaces the list and clears the log.  A FRAME is the views' RGB images one after the other in list order.  Options
 * (fs_set_option, any time): "volume_log" = N, 0 (default: off, a step launches and allocates nothing for it) .. 65536 frames
 * kept; "volume_every" = K >= 1 (default 1).  Setting "volume_log", the views or the rays of a slot in use reallocates and
 * clears the ring; each is FS_EINVAL if N * (bytes of one frame) would exceed 1 GiB.  fs_step takes a frame at the sample point
 * of the image log -- after advect(0, dens, buffer) (simulation.cpp:136), before the frame dump -- when (steps_total - 1) % K
 * == 0, into a device ring on the step's own stream, by one launch per view, without a host synchronisation.
 * fs_volume_sample takes one frame of the state as it is now.  fs_volume_log drains the log exactly as fs_image_log does.
 * fs_get_int "volume_frame_bytes" and "volume_views" report the frame size and the view count; timing family "volume" counts
 * one launch per rendered view of the log, 0 with the feature off.
 * Single-GPU handles only: every entry here and a "volume_log" above 0 are FS_EINVAL on a z-slab handle, and so is fs_comm_init
 * on a handle whose "volume_log" is on.
 */
#define FS_VOLUME_CAMERAS_MAX 4
#define FS_VOLUME_VIEWS_MAX 4
#define FS_VOLUME_PARAMS 11
#define FS_VOLUME_CAMERA 11        /* entries of fs_volume_camera's cam[] */
#define FS_VOLUME_SAMPLES_MAX 16384
int fs_volume_rays(fs_sim* s, int slot, const double* rays, int cols, int rows);
int fs_volume_camera(fs_sim* s, int slot, const double* cam, int cols, int rows);
int fs_volume_render(fs_sim* s, int source, int slot, const double* par, uint8_t* rgb, size_t n_bytes, double* acc, size_t n_acc);
int fs_volume_views(fs_sim* s, const int* spec, const double* par, int n);
int fs_volume_sample(fs_sim* s);
int fs_volume_log(fs_sim* s, uint8_t* frames, long* steps, long max_frames, long* n_frames, long* n_dropped);

/* ---- flow monitor (beyond the reference: its run() prints sum / min / max of whole padded arrays, simulation.cpp:73-93) ----
 *
 * Is the run still finite, what is the Courant number, is mass conserved between inlet and outlet, how much kinetic energy is
 * in the box, what is the momentum deficit in the wake: the integrals and extrema of the state, per plane, whole and per x,
 * each sum in one written order, so that a restatement in any language gives the same bits.
 * STATE: the values as stored, q = dens, u, v, w = v_x, v_y, v_z, p = FS_PRESSURE.  A TARGET cell is an interior cell (1..w,
 * 1..h, 1..d) with obs != 1 (read from the cell's flag byte).  Ghost cells and solid cells contribute no term, whatever they hold.
 * ARITHMETIC: fp64 on the stored values widened, for fp32 and fp64 handles alike; every written operation is rounded once,
 * without contraction (the library is built with -ffp-contract=off).  Products are (double)a * (double)b, which is exact on
 * fp32 handles.  e = (u*u + v*v) + w*w.
 * COLUMN record, one per (z, x), over the target cells of the rows y = 1..h in increasing y: the sums, each from +0.0,
 *     cells, nonfinite, sum q, sum u, sum v, sum w, sum e, sum p, sum (u*u), sum (q*u)
 * where a cell is nonfinite if any of its five values is NaN or +-Inf; the running maxima max |u|, max |v|, max |w|, max e, each
 * from 0 by "if (a > m) m = a", so that a NaN never replaces the running value; and min q, max q, min p, max p, from +Inf and
 * -Inf, by "if (a < m) m = a" and "if (a > m) m = a".
 * PLANE record (FS_MONITOR_COLS = 16 numbers) per global plane z:
 *     { cells, nonfinite, sum q, sum u, sum v, sum w, sum e, sum p, max |u|, max |v|, max |w|, max e, min q, max q, min p, max p }
 * the sums are the column sums added over x = 1..w in increasing x from +0.0, the extrema the extrema of the columns' extrema
 * by the same rules from the same starts.
 * WHOLE record: the plane sums added in increasing z from +0.0, the extrema of the planes' extrema.
 * X-PROFILE (FS_MONITOR_PROFILE_COLS = 5 numbers) per x = 1..w: { cells, sum u, sum (u*u), sum p, sum (q*u) }, the column sums
 * of that x added in increasing z from +0.0.  sum u is the volume flux through the plane x in cell units (times h^2
 * physically, h = 1 / cbrt(w*h*d)): with walls and solids at rest it is the same at every x of a divergence-free flow.
 * sum (u*u) + sum p is the momentum flux a wake survey needs, sum (q*u) the smoke flux.
 * EMPTY SET (no target cell): sums 0, the four maxima 0, each min +Inf, each max -Inf.
 * Every number is a pure function of the five arrays and the flags: launch shape, tuning and timing cannot change a bit (no
 * floating-point atomics; partial results are stored and added in the written order).
 * DERIVED by the caller, in fp64: cfl_x = ((double)dt * w) * max |u|, cfl_y = ((double)dt * h) * max |v|, cfl_z =
 * ((double)dt * d) * max |w| -- the length of the advection back-trace in cells (simulation.cpp:384-386); the kinetic energy
 * per unit density 0.5 * sum e * h^3.
 *
 * fs_flow_monitor: the records of the state as it is now; changes nothing.  out = the WHOLE record; per_plane (may be NULL)
 * receives 16 * d doubles, plane 1 first; x_profile (may be NULL) 5 * w doubles, x = 1 first.  Three launches: a streaming pass
 * (lanes along x, each walking its column in y: 21 bytes per cell on an fp32 handle) into a workspace of 18 * w * d doubles
 * that is allocated at the first use, never inside a later step; planes and profile; the whole record.
 * Option "monitor_log" = N: fs_step takes such a record when (steps so far - 1) % "monitor_every" == 0, after the density
 * advection of simulation.cpp:136 and before the frame dump, on the step's own stream without a host synchronisation.
 * "monitor_stations" = "x1,x2,...": up to FS_MONITOR_STATIONS_MAX indices in 1..w whose X-PROFILE rows a record carries.
 * fs_monitor_sample: appends a record of the state now (FS_EINVAL while the log is off), for callers who drive the passes
 * themselves; its step number is that of the last completed step.
 * fs_monitor_log: the retained records, oldest first, FS_MONITOR_LOG_COLS = 57 doubles each: { step, the 16 numbers of the
 * WHOLE record, then 5 numbers for each of 8 stations }, an unused station 5 x NaN.  Step numbering, rows = NULL, max_rows too
 * small and *n_dropped exactly as for fs_force_log; a fetch drains the log.
 * Timing family "monitor": one launch counted per record.  Single GPU only: on a handle with a communicator (the FSNULL one
 * included) the three entries and the three options are FS_EINVAL ("single-GPU"), and fs_comm_init on a handle whose
 * "monitor_log" is on is FS_EINVAL.  Plane records are per global z so that slabs can follow.
 */
#define FS_MONITOR_COLS 16
#define FS_MONITOR_PROFILE_COLS 5
#define FS_MONITOR_STATIONS_MAX 8
#define FS_MONITOR_LOG_COLS 57
int fs_flow_monitor(fs_sim* s, double out[16], double* per_plane, double* x_profile);
int fs_monitor_sample(fs_sim* s);
int fs_monitor_log(fs_sim* s, double* rows, long max_rows, long* n_rows, long* n_dropped);

/* ---- multi-GPU z-slabs (one process per GPU; RCCL halo exchange over xGMI) -------- */

/* Size of the opaque RCCL unique id; rank 0 fills it with fs_comm_unique_id and the
 * host layer broadcasts it to the other ranks (e.g. through torch.distributed).  An id that starts with
 * "FSIPC:" + a POSIX shared-memory name instead selects the stream-ordered device-to-device transport between rank
 * processes of one host (csrc/ipc.h: hipIpc-mapped arrays, copy engines, device-side handshakes; ranks may share a
 * GPU; at most 8 ranks); "FSSHM:" + name the host-staged synchronous development transport; "FSNULL:" none (timing). */
#define FS_COMM_ID_BYTES 128
int fs_comm_unique_id(void* id_out);
/* Turns the handle into the owner of z-slab `rank` of `nranks` of the global grid given
 * to fs_create (depth must divide evenly).  Must precede first use. */
int fs_comm_init(fs_sim* s, int rank, int nranks, const void* id);

/* Loads RCCL, builds a one-rank communicator on the current device and pushes data through
 * every collective the slab path uses (grouped send/recv, all-gather, broadcast, all-reduce).
 * A plumbing check for machines with a single GPU. */
int fs_comm_selftest(void);

/* What carries the halo planes of this handle: "single GPU", or the path of the RCCL library that was
 * loaded (it must be the one next to the HIP runtime the process runs on), or the name of a
 * development transport.  The string belongs to the handle. */
const char* fs_comm_transport(fs_sim* s);

const char* fs_last_error(void);
const char* fs_version(void);

#ifdef __cplusplus
}
#endif
#endif /* FLUIDSIM_H */
