// src/main.cpp -- `simulation.out`: the reference's process contract on top of libfluidsim.so.
//
// `make && ./simulation.out` with no arguments does what the reference's main() does
// (simulation.cpp:429-451): a 128x64x64 tunnel, 100 steps, inlet speed 30, the constructor
// defaults of simulation.h:60-64, one STL obstacle (scale 2, rot_x 90 deg, translate -16,0,0),
// then Simulation::run(), which appends every frame to ./data/{data,obs,v_x,v_y,v_z}.bin so
// that GUI/main.py, gui.py and make_pngs.py of the reference read the output unchanged.
//
// The reference hard-codes an absolute STL path from its author's machine; when that file
// does not exist the reference prints an error and simulates an empty tunnel
// (object_loader.cpp:282-285).  Same here; FS_STL or --stl names another mesh.
//
// The reference needs a recompile for every change of configuration.  Optional overrides
// (all default to the reference's values):
//   --grid WxHxD  --steps N  --acc N  --speed N  --dt F  --diff F
//   --stl PATH[,scale,rot_x,rot_y,rot_z,tx,ty,tz]   (repeatable; "none" = no obstacle)
//   --dump-every N (0 = never, -1 = last frame only)  --dump-dir DIR
//   --precision fp32|fp64   --solver jacobi|gs_lex|rbsor|mg   --omega W (rbsor)   --mg-cycles N (mg)   --seed N   --quiet
//   --resume DIR   start from the last frame of DIR/{data,obs,v_x,v_y,v_z}.bin (a dumped frame is
//                  a complete state: everything else is rebuilt every step)
//   --json         append one machine-readable timing line to stdout
//   --forces FILE  log the obstacle pressure force of every step (option "force_log") and write it to FILE as CSV:
//                  fs_force_log's columns, then F = (S1 + S2) h^2 / dt and C = 2 (S1 + S2) / (dt speed^2 N_front)
//                  (include/fluidsim.h)
//   --body-forces FILE  label the obstacles into bodies and log the pressure force and moment of every body and step
//                  (option "body_force_log") and write them to FILE as CSV: `#` lines with the body table (fs_body_info),
//                  then fs_body_force_log's columns and F, the torque T = (M1 + M2) h^3 / dt and the coefficients C and
//                  C_M (for L_ref = 1 cell); --moment-origin x,y,z sets the origin of the moments (option "moment_origin",
//                  padded index coordinates, default 0,0,0); single GPU, may be combined with --forces
//   --residuals FILE  log the residual of the step's six linear solves before and after each (option "residual_log") and
//                  write it to FILE as CSV: fs_residual_log's columns, then reduction_k = sqrt(r_sq_k / r0_sq_k);
//                  may be combined with --forces
//   --mean-flow DIR  time-average the flow on the device (option "flow_stats") and, at the end of the run, write the mean
//                  fields to DIR as one frame per file in the frame-dump layout (fs_flow_stats_dump: the viewers show it
//                  unchanged); --mean-from S skips the first S steps, --mean-every N samples every Nth step after them,
//                  --mean-moments (no value) also keeps the second moments and writes DIR/tke.bin
//   --vortex DIR   at the end of the run, write the vorticity components, |omega|^2 and the Q-criterion of the final
//                  velocities to DIR/{vort_x,vort_y,vort_z,vort_sq,q}.bin, one frame per file in the frame-dump layout
//                  (fs_vortex_dump); may be combined with the logs and --mean-flow
//   --probes FILE  point probes: a text file with one cell `x y z` per line in padded global coordinates (the numbers the
//                  mutators use; ghost cells 0 and N+1 allowed), `#` starts a comment; --probe-log FILE records dens, v_x,
//                  v_y, v_z and the pressure at every probe after every step (option "probe_log" = steps) and writes them
//                  to FILE as CSV: step,q_0,u_0,v_0,w_0,p_0,q_1,... with the values as %.17g (they read back exactly)
//   --images DIR   render image views on the device after every step (option "image_log", fs_image_views) and write them as
//                  uncompressed PNGs DIR/<view number>_<step>.png (fs_image_png); --image-every K takes every Kth step
//                  (steps 1, K+1, ...); --image-view SRC:KIND:AXIS:INDEX:VMIN:VMAX[:ALPHA] (repeatable, up to
//                  FS_IMAGE_VIEWS_MAX) replaces the default views -- SRC density|v_x|v_y|v_z|obs|pressure or a source
//                  selector as a number, KIND slice|sum|max|min, AXIS x|y|z, INDEX the padded slice index (0 for a
//                  projection), ALPHA the darkening of obstacle pixels (default 0.2).  Default views: density 0..0.01 and
//                  v_x -10..10 at the middle z-slice (D+2)/2, the 2-D viewer's frames (gui.py:271-279).  The ring holds the
//                  run's frames where they fit 256 MiB and is drained at the end; a longer run is driven step by step
//                  (fs_run_one, frame dumps through fs_dump_frame, without run()'s console lines) and the ring is drained
//                  whenever it is full.  Single GPU.
//   --volume DIR   render a ray-marched 3-D view of the density on the device after every step (option "volume_log",
//                  fs_volume_camera, fs_volume_views) and write it as uncompressed PNGs DIR/<step>.png (fs_image_png);
//                  --volume-view AZ,EL,DIST the 3-D viewer's orbit about the box centre in degrees and cells (default 45,30,200:
//                  GUI/gl_widget.py:26-28; 45 degree field of view, y up), --volume-size CxR the image (default 512x512),
//                  --volume-range LO,HI the colour range (default 0,0.01), --volume-opacity K the opacity per cell at HI
//                  (default 0.05), --volume-every K takes every Kth step (steps 1, K+1, ...).  The ring is sized and drained
//                  as for --images.  Single GPU.
//   --tracers C    tracer particles: a pool of C slots (option "tracers"); --tracer-emitters FILE sets the emitters, a text file
//                  with one point `x y z` per line in the viewer's padded index space (0.5 .. N + 0.5 on each axis), `#`
//                  starts a comment; --tracer-every K releases one particle per emitter every Kth step (steps 1, K+1, ...;
//                  default 1) -- the `every` of fs_tracer_emitters, NOT the library option "tracer_every", which is the
//                  cadence of the snapshot log and has no flag here; --tracer-out FILE writes the final pool after the run
//                  as CSV: slot,source,born,moves,status,x,y,z with the positions as %.17g (they read back exactly).
//                  --tracer-emitters and --tracer-out need --tracers, --tracer-every needs --tracer-emitters: anything
//                  else is refused.  Single GPU.
//   --confinement EPS  vorticity confinement: every step begins with one confinement pass of strength EPS (option
//                  "vorticity_confinement"; a decimal number >= 0, 0 = off; include/fluidsim.h has the definition).  Single GPU.
//   --monitor FILE log the flow monitor's record after every step (option "monitor_log": integrals and extrema of the state over
//                  the fluid cells, each sum in one written order; include/fluidsim.h has the definition) and write it to FILE
//                  as CSV: fs_monitor_log's columns, then cfl_x, cfl_y, cfl_z = ((double)dt * N) * max |.|, numbers as %.17g
//                  (they read back exactly).  --monitor-every K takes every Kth step (steps 1, K+1, ...), --monitor-stations
//                  LIST ("x1,x2,...", up to 8 indices in 1..w) adds the x-profile rows of those planes.  Single GPU.
//   --inflow-profile FILE  the inflow generator (option "inflow" = "on"; include/fluidsim.h, "turbulent inflow"): FILE is text,
//                  height * depth numbers of the mean map U (y fastest, then z), optionally followed by as many of the
//                  fluctuation scale r; `#` starts a comment.  --inflow-gust FILE: lines `step factor`, the knots of the gust
//                  schedule, steps strictly increasing.  --inflow-eddies N, --inflow-sigma S, --inflow-rms R, --inflow-convect C
//                  (cells per step, or auto), --inflow-seed K: the synthetic eddies (options "inflow_eddies", "inflow_sigma",
//                  "inflow_rms", "inflow_convect", "inflow_seed").  Any of these flags turns the generator on.  The step number
//                  the eddies are taken at counts this run's steps: --resume restores the fields, not the count.  Single GPU.
//   --heat KAPPA,BETA,ALPHA  heat and buoyancy (fs_heat_params, mode 2; include/fluidsim.h, "heat and buoyancy"): a temperature
//                  with thermal diffusivity KAPPA, buoyancy BETA per unit temperature and weight ALPHA per unit smoke density,
//                  applied and transported by every step.  --heat-up AXIS: +x, -x, +y (default), -y, +z or -z.  --heat-inlet T:
//                  the temperature forced on the inlet plane.  --heat-wall T[,x0,x1,y0,y1,z0,z1]: the fluid cells beside a body
//                  are held at T, with a box in cells only those inside it.  --heat-log FILE.csv: the heat budget after every
//                  step (fs_heat_log's columns, numbers as %.17g).  --heat-dump FILE: the temperature is appended to FILE as
//                  float32 in the frames' layout whenever a frame is dumped (the run then goes step by step, as for
//                  --images).  The other --heat-* flags need --heat.  A --resume run starts the temperature from zero: the
//                  dumped frames do not hold it.  Single GPU.
//   --zone SPEC    a momentum zone (fs_zones, mode 2; include/fluidsim.h, "momentum zones"): SPEC is the zone's 20 numbers,
//                  comma-separated -- shape, axis, x0, x1, y0, y1, z0, z1, c1, c2, radius, gx, gy, gz, Dx, Dy, Dz, Fx, Fy, Fz.
//                  Repeatable, up to 8 zones, applied in the order given.  --zone-log FILE.csv: every zone's budget before each
//                  step's pass (fs_zone_log's columns, numbers as %.17g); it needs --zone.  Zones hold no state: --resume
//                  needs nothing of them.  Single GPU.
// Each flag can also be given as an environment variable FS_GRID, FS_STEPS, ...
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include <sys/stat.h>

#include "../include/fluidsim.h"

namespace {

struct Stl {
    std::string path;
    float v[7] = { 2.0f, 90.0f, 0.0f, 0.0f, -16.0f, 0.0f, 0.0f };   // simulation.cpp:442-446
};

Stl parse_stl(const std::string& spec)
{
    Stl s;
    size_t pos = spec.find(',');
    s.path = spec.substr(0, pos);
    int k = 0;
    while (pos != std::string::npos && k < 7) {
        size_t next = spec.find(',', pos + 1);
        s.v[k++] = (float)atof(spec.substr(pos + 1, next == std::string::npos ? std::string::npos : next - pos - 1).c_str());
        pos = next;
    }
    return s;
}

const char* opt(int argc, char** argv, int& i, const char* flag, const char* env)
{
    (void)env;
    if (strcmp(argv[i], flag) == 0 && i + 1 < argc) return argv[++i];
    return nullptr;
}

// last frame of one dump file -> field `which` (simulation.cpp:143-147 layout)
int resume_field(fs_sim* sim, const std::string& dir, const char* name, int which)
{
    const size_t n = fs_padded_size(sim);
    std::string path = dir + "/" + name;
    FILE* fp = fopen(path.c_str(), "rb");
    if (!fp) { fprintf(stderr, "simulation.out: cannot open %s\n", path.c_str()); return 1; }
    fseek(fp, 0, SEEK_END);
    const long bytes = ftell(fp);
    if (bytes <= 0 || (size_t)bytes % (n * sizeof(float)) != 0) {
        fprintf(stderr, "simulation.out: %s is not a whole number of %zu-cell frames\n", path.c_str(), n);
        fclose(fp);
        return 1;
    }
    std::vector<float> frame(n);
    fseek(fp, bytes - (long)(n * sizeof(float)), SEEK_SET);
    const bool ok = fread(frame.data(), sizeof(float), n, fp) == n;
    fclose(fp);
    if (!ok) { fprintf(stderr, "simulation.out: short read from %s\n", path.c_str()); return 1; }
    if (fs_set_field(sim, which, frame.data(), n, 4)) { fprintf(stderr, "simulation.out: %s\n", fs_last_error()); return 1; }
    return 0;
}

// the per-step force log of the run -> CSV (the columns of Simulation.force_log() in the Python package)
int write_forces(fs_sim* sim, const char* path, int w, int h, int d, float dt, int speed)
{
    long n = 0, dropped = 0;
    if (fs_force_log(sim, nullptr, 0, &n, &dropped)) return 1;
    std::vector<double> rows((size_t)n * FS_FORCE_LOG_COLS);
    if (fs_force_log(sim, rows.data(), n, &n, &dropped)) return 1;
    FILE* fp = fopen(path, "w");
    if (!fp) { fprintf(stderr, "simulation.out: cannot write %s\n", path); return 1; }
    fprintf(fp, "step,s1x,s1y,s1z,s2x,s2y,s2z,faces,frontal,fx,fy,fz,cx,cy,cz\n");
    const double hh = 1.0 / std::cbrt((double)((long)w * h * d)), t = (double)dt, sp = (double)speed;
    for (long i = 0; i < n; ++i) {
        const double* r = &rows[(size_t)i * FS_FORCE_LOG_COLS];
        double f[3], c[3];
        const double denom = t * (sp * sp) * r[8];
        for (int k = 0; k < 3; ++k) {
            const double s = r[1 + k] + r[4 + k];
            f[k] = s * (hh * hh) / t;
            c[k] = denom != 0.0 ? 2.0 * s / denom : NAN;
        }
        fprintf(fp, "%ld,%.17g,%.17g,%.17g,%.17g,%.17g,%.17g,%ld,%ld,%.17g,%.17g,%.17g,%.17g,%.17g,%.17g\n", (long)r[0], r[1], r[2],
                r[3], r[4], r[5], r[6], (long)r[7], (long)r[8], f[0], f[1], f[2], c[0], c[1], c[2]);
    }
    const bool ok = fclose(fp) == 0;
    if (!ok) fprintf(stderr, "simulation.out: writing %s failed\n", path);
    return ok ? 0 : 1;
}

// the body table and the per-step body-force log of the run -> CSV (the columns of Simulation.body_force_log() in the
// Python package, for l_ref = 1)
int write_body_forces(fs_sim* sim, const char* path, int w, int h, int d, float dt, int speed)
{
    long nb = 0, n = 0, dropped = 0;
    if (fs_body_info(sim, nullptr, 0, &nb)) return 1;
    std::vector<double> info((size_t)nb * FS_BODY_INFO_COLS);
    if (fs_body_info(sim, info.data(), nb, &nb)) return 1;
    if (fs_body_force_log(sim, nullptr, 0, &n, &dropped)) return 1;
    std::vector<double> rows((size_t)n * FS_BODY_LOG_COLS);
    if (fs_body_force_log(sim, rows.data(), n, &n, &dropped)) return 1;
    FILE* fp = fopen(path, "w");
    if (!fp) { fprintf(stderr, "simulation.out: cannot write %s\n", path); return 1; }
    fprintf(fp, "# body,cells,anchor,xmin,xmax,ymin,ymax,zmin,zmax,sum_x,sum_y,sum_z,frontal (body 0 = the rest)\n");
    for (long k = 0; k < nb; ++k) {
        fprintf(fp, "# %ld", k);
        for (int c = 0; c < FS_BODY_INFO_COLS; ++c) fprintf(fp, ",%ld", (long)info[(size_t)k * FS_BODY_INFO_COLS + c]);
        fprintf(fp, "\n");
    }
    fprintf(fp, "step,body,s1x,s1y,s1z,m1x,m1y,m1z,s2x,s2y,s2z,m2x,m2y,m2z,faces,frontal,fx,fy,fz,tx,ty,tz,cx,cy,cz,cmx,cmy,cmz\n");
    const double hh = 1.0 / std::cbrt((double)((long)w * h * d)), t = (double)dt, sp = (double)speed;
    for (long i = 0; i < n; ++i) {
        const double* r = &rows[(size_t)i * FS_BODY_LOG_COLS];
        fprintf(fp, "%ld,%ld", (long)r[0], (long)r[1]);
        for (int k = 2; k < 14; ++k) fprintf(fp, ",%.17g", r[k]);
        fprintf(fp, ",%ld,%ld", (long)r[14], (long)r[15]);
        const double denom = t * (sp * sp) * r[15];
        double f[3], tq[3], c[3], cm[3];
        for (int k = 0; k < 3; ++k) {
            const double s = r[2 + k] + r[8 + k], m = r[5 + k] + r[11 + k];
            f[k] = s * (hh * hh) / t;
            tq[k] = m * (hh * hh * hh) / t;
            c[k] = denom != 0.0 ? 2.0 * s / denom : NAN;
            cm[k] = denom != 0.0 ? 2.0 * m / denom : NAN;
        }
        for (const double* v : { f, tq, c, cm }) fprintf(fp, ",%.17g,%.17g,%.17g", v[0], v[1], v[2]);
        fprintf(fp, "\n");
    }
    const bool ok = fclose(fp) == 0;
    if (!ok) fprintf(stderr, "simulation.out: writing %s failed\n", path);
    return ok ? 0 : 1;
}

// the per-step residual log of the run -> CSV (the columns of Simulation.residual_log() in the Python package)
int write_residuals(fs_sim* sim, const char* path)
{
    long n = 0, dropped = 0;
    if (fs_residual_log(sim, nullptr, 0, &n, &dropped)) return 1;
    std::vector<double> rows((size_t)n * FS_RESIDUAL_LOG_COLS);
    if (fs_residual_log(sim, rows.data(), n, &n, &dropped)) return 1;
    FILE* fp = fopen(path, "w");
    if (!fp) { fprintf(stderr, "simulation.out: cannot write %s\n", path); return 1; }
    fprintf(fp, "step");
    for (int k = 0; k < FS_RESIDUAL_LOG_SOLVES; ++k) fprintf(fp, ",r0_sq_%d,r_sq_%d,r_max_%d,rhs_sq_%d,cells_%d", k, k, k, k, k);
    for (int k = 0; k < FS_RESIDUAL_LOG_SOLVES; ++k) fprintf(fp, ",reduction_%d", k);
    fprintf(fp, "\n");
    for (long i = 0; i < n; ++i) {
        const double* r = &rows[(size_t)i * FS_RESIDUAL_LOG_COLS];
        fprintf(fp, "%ld", (long)r[0]);
        for (int k = 0; k < FS_RESIDUAL_LOG_SOLVES; ++k) {
            const double* q = r + 1 + 5 * k;
            fprintf(fp, ",%.17g,%.17g,%.17g,%.17g,%ld", q[0], q[1], q[2], q[3], (long)q[4]);
        }
        for (int k = 0; k < FS_RESIDUAL_LOG_SOLVES; ++k) {
            const double* q = r + 1 + 5 * k;
            fprintf(fp, ",%.17g", q[0] != 0.0 ? std::sqrt(q[1] / q[0]) : (double)NAN);
        }
        fprintf(fp, "\n");
    }
    const bool ok = fclose(fp) == 0;
    if (!ok) fprintf(stderr, "simulation.out: writing %s failed\n", path);
    return ok ? 0 : 1;
}

// the flow-monitor log of the run -> CSV (the columns of Simulation.monitor_log() in the Python package, then the Courant numbers)
int write_monitor(fs_sim* sim, const char* path, int width, int height, int depth, float dt)
{
    long n = 0, dropped = 0;
    if (fs_monitor_log(sim, nullptr, 0, &n, &dropped)) return 1;
    std::vector<double> rows((size_t)n * FS_MONITOR_LOG_COLS);
    if (fs_monitor_log(sim, rows.data(), n, &n, &dropped)) return 1;
    if (dropped) fprintf(stderr, "simulation.out: %ld monitor records were overwritten before they were written\n", dropped);
    FILE* fp = fopen(path, "w");
    if (!fp) { fprintf(stderr, "simulation.out: cannot write %s\n", path); return 1; }
    fprintf(fp, "step,cells,nonfinite,sum_q,sum_u,sum_v,sum_w,sum_e,sum_p,max_abs_u,max_abs_v,max_abs_w,max_e,min_q,max_q,min_p,max_p");
    for (int k = 0; k < FS_MONITOR_STATIONS_MAX; ++k) fprintf(fp, ",s%d_cells,s%d_sum_u,s%d_sum_uu,s%d_sum_p,s%d_sum_qu", k, k, k, k, k);
    fprintf(fp, ",cfl_x,cfl_y,cfl_z\n");
    for (long i = 0; i < n; ++i) {
        const double* r = &rows[(size_t)i * FS_MONITOR_LOG_COLS];
        fprintf(fp, "%ld", (long)r[0]);
        for (int k = 1; k < FS_MONITOR_LOG_COLS; ++k) fprintf(fp, ",%.17g", r[k]);
        fprintf(fp, ",%.17g,%.17g,%.17g\n", ((double)dt * width) * r[9], ((double)dt * height) * r[10], ((double)dt * depth) * r[11]);
    }
    const bool ok = fclose(fp) == 0;
    if (!ok) fprintf(stderr, "simulation.out: writing %s failed\n", path);
    return ok ? 0 : 1;
}

// the heat log of the run -> CSV (the columns of Simulation.heat_log() in the Python package)
int write_heat_log(fs_sim* sim, const char* path)
{
    long n = 0, dropped = 0;
    if (fs_heat_log(sim, nullptr, 0, &n, &dropped)) return 1;
    std::vector<double> rows((size_t)n * FS_HEAT_LOG_COLS);
    if (fs_heat_log(sim, rows.data(), n, &n, &dropped)) return 1;
    if (dropped) fprintf(stderr, "simulation.out: %ld heat records were overwritten before they were written\n", dropped);
    FILE* fp = fopen(path, "w");
    if (!fp) { fprintf(stderr, "simulation.out: cannot write %s\n", path); return 1; }
    fprintf(fp, "step,cells,sum,sum_sq,max,min,held,loss,outflow,inflow\n");
    for (long i = 0; i < n; ++i) {
        const double* r = &rows[(size_t)i * FS_HEAT_LOG_COLS];
        fprintf(fp, "%ld", (long)r[0]);
        for (int k = 1; k < FS_HEAT_LOG_COLS; ++k) fprintf(fp, ",%.17g", r[k]);
        fprintf(fp, "\n");
    }
    const bool ok = fclose(fp) == 0;
    if (!ok) fprintf(stderr, "simulation.out: writing %s failed\n", path);
    return ok ? 0 : 1;
}

// the zone log of the run -> CSV (the columns of Simulation.zone_log() in the Python package)
int write_zone_log(fs_sim* sim, int n_zones, const char* path)
{
    static const char* const name[FS_ZONE_COLS] = { "cells", "dvx", "dvy", "dvz", "dke", "flux", "max_speed" };
    const int cols = 1 + n_zones * FS_ZONE_COLS;
    long n = 0, dropped = 0;
    if (fs_zone_log(sim, nullptr, 0, &n, &dropped)) return 1;
    std::vector<double> rows((size_t)n * cols);
    if (fs_zone_log(sim, rows.data(), n, &n, &dropped)) return 1;
    if (dropped) fprintf(stderr, "simulation.out: %ld zone records were overwritten before they were written\n", dropped);
    FILE* fp = fopen(path, "w");
    if (!fp) { fprintf(stderr, "simulation.out: cannot write %s\n", path); return 1; }
    fprintf(fp, "step");
    for (int z = 0; z < n_zones; ++z)
        for (int k = 0; k < FS_ZONE_COLS; ++k) fprintf(fp, ",z%d_%s", z, name[k]);
    fprintf(fp, "\n");
    for (long i = 0; i < n; ++i) {
        const double* r = &rows[(size_t)i * cols];
        fprintf(fp, "%ld", (long)r[0]);
        for (int k = 1; k < cols; ++k) fprintf(fp, ",%.17g", r[k]);
        fprintf(fp, "\n");
    }
    const bool ok = fclose(fp) == 0;
    if (!ok) fprintf(stderr, "simulation.out: writing %s failed\n", path);
    return ok ? 0 : 1;
}

// the temperature as one more float32 frame at the end of `path`
int append_heat_frame(fs_sim* sim, const char* path)
{
    std::vector<float> frame(fs_padded_size(sim));
    if (fs_heat_get(sim, frame.data(), frame.size(), 4)) return 1;
    FILE* fp = fopen(path, "ab");
    if (!fp) { fprintf(stderr, "simulation.out: cannot write %s\n", path); return 1; }
    const bool ok = fwrite(frame.data(), sizeof(float), frame.size(), fp) == frame.size();
    return (fclose(fp) == 0 && ok) ? 0 : 1;
}

// the probe cells of --probes: `x y z` per line, `#` comments
int read_probes(const char* path, std::vector<int>& cells)
{
    FILE* fp = fopen(path, "r");
    if (!fp) { fprintf(stderr, "simulation.out: cannot open %s\n", path); return 1; }
    char line[512];
    int lineno = 0;
    bool ok = true;
    while (ok && fgets(line, sizeof line, fp)) {
        ++lineno;
        if (char* hash = strchr(line, '#')) *hash = 0;
        int x, y, z, used = 0;
        const int got = sscanf(line, "%d %d %d %n", &x, &y, &z, &used);
        if (got == EOF || (got <= 0 && strspn(line, " \t\r\n") == strlen(line))) continue;   // blank or comment
        if (got != 3 || line[used] != 0) {
            fprintf(stderr, "simulation.out: %s:%d: expected `x y z`\n", path, lineno);
            ok = false;
        } else {
            cells.push_back(x); cells.push_back(y); cells.push_back(z);
        }
    }
    fclose(fp);
    return ok ? 0 : 1;
}

// the per-step probe log of the run -> CSV (the rows of fs_probe_log)
int write_probes(fs_sim* sim, const char* path, long nprobes)
{
    long n = 0, dropped = 0;
    if (fs_probe_log(sim, nullptr, 0, &n, &dropped)) return 1;
    const size_t cols = 1 + (size_t)FS_PROBE_VALUES * (size_t)nprobes;
    std::vector<double> rows((size_t)n * cols + 1);
    if (fs_probe_log(sim, rows.data(), n, &n, &dropped)) return 1;
    FILE* fp = fopen(path, "w");
    if (!fp) { fprintf(stderr, "simulation.out: cannot write %s\n", path); return 1; }
    fprintf(fp, "step");
    for (long k = 0; k < nprobes; ++k) fprintf(fp, ",q_%ld,u_%ld,v_%ld,w_%ld,p_%ld", k, k, k, k, k);
    fprintf(fp, "\n");
    for (long i = 0; i < n; ++i) {
        const double* r = &rows[(size_t)i * cols];
        fprintf(fp, "%ld", (long)r[0]);
        for (size_t k = 1; k < cols; ++k) fprintf(fp, ",%.17g", r[k]);
        fprintf(fp, "\n");
    }
    const bool ok = fclose(fp) == 0;
    if (!ok) fprintf(stderr, "simulation.out: writing %s failed\n", path);
    return ok ? 0 : 1;
}

// the emitters of --tracer-emitters: `x y z` per line, `#` comments
int read_points(const char* path, std::vector<double>& pts)
{
    FILE* fp = fopen(path, "r");
    if (!fp) { fprintf(stderr, "simulation.out: cannot open %s\n", path); return 1; }
    char line[512];
    int lineno = 0;
    bool ok = true;
    while (ok && fgets(line, sizeof line, fp)) {
        ++lineno;
        if (char* hash = strchr(line, '#')) *hash = 0;
        double x, y, z;
        int used = 0;
        const int got = sscanf(line, "%lf %lf %lf %n", &x, &y, &z, &used);
        if (got == EOF || (got <= 0 && strspn(line, " \t\r\n") == strlen(line))) continue;   // blank or comment
        if (got != 3 || line[used] != 0) {
            fprintf(stderr, "simulation.out: %s:%d: expected `x y z`\n", path, lineno);
            ok = false;
        } else {
            pts.push_back(x); pts.push_back(y); pts.push_back(z);
        }
    }
    fclose(fp);
    return ok ? 0 : 1;
}

// the numbers of --inflow-profile and --inflow-gust: separated by white space, `#` comments
int read_numbers(const char* path, std::vector<double>& out)
{
    FILE* fp = fopen(path, "r");
    if (!fp) { fprintf(stderr, "simulation.out: cannot open %s\n", path); return 1; }
    static char line[1 << 16];
    int lineno = 0;
    bool ok = true, whole = true;                        // whole: the previous piece ended its line
    while (ok && fgets(line, sizeof line, fp)) {
        if (whole) ++lineno;
        const size_t len = strlen(line);
        whole = len > 0 && line[len - 1] == '\n';
        if (!whole && len + 1 == sizeof line) {
            fprintf(stderr, "simulation.out: %s:%d: a line is longer than %zu characters\n", path, lineno, sizeof line - 2);
            ok = false;
            break;
        }
        if (char* hash = strchr(line, '#')) *hash = 0;
        for (char* q = line; ok;) {
            q += strspn(q, " \t\r\n");
            if (!*q) break;
            char* end = nullptr;
            const double v = strtod(q, &end);
            if (end == q || !strchr(" \t\r\n", *end)) {
                fprintf(stderr, "simulation.out: %s:%d: not a number: %.20s\n", path, lineno, q);
                ok = false;
            } else {
                out.push_back(v);
                q = end;
            }
        }
    }
    fclose(fp);
    return ok ? 0 : 1;
}

// the final tracer pool -> CSV (the arrays of fs_tracer_fetch)
int write_tracers(fs_sim* sim, const char* path)
{
    long n = 0;
    if (fs_tracer_fetch(sim, nullptr, nullptr, 0, &n)) return 1;
    std::vector<double> xyz((size_t)n * 3 + 1);
    std::vector<int32_t> meta((size_t)n * 4 + 1);
    if (fs_tracer_fetch(sim, xyz.data(), meta.data(), n, &n)) return 1;
    FILE* fp = fopen(path, "w");
    if (!fp) { fprintf(stderr, "simulation.out: cannot write %s\n", path); return 1; }
    fprintf(fp, "slot,source,born,moves,status,x,y,z\n");
    for (long k = 0; k < n; ++k)
        fprintf(fp, "%ld,%d,%d,%d,%d,%.17g,%.17g,%.17g\n", k, (int)meta[4 * k + 1], (int)meta[4 * k + 2], (int)meta[4 * k + 3],
                (int)meta[4 * k], xyz[3 * k], xyz[3 * k + 1], xyz[3 * k + 2]);
    const bool ok = fclose(fp) == 0;
    if (!ok) fprintf(stderr, "simulation.out: writing %s failed\n", path);
    return ok ? 0 : 1;
}

// one view of --image-view: SRC:KIND:AXIS:INDEX:VMIN:VMAX[:ALPHA] -> spec[4], range[3]
bool parse_view(const char* text, int* spec, double* range)
{
    std::vector<std::string> part;
    std::string t = text;
    for (size_t at = 0;;) {
        const size_t next = t.find(':', at);
        part.push_back(t.substr(at, next == std::string::npos ? std::string::npos : next - at));
        if (next == std::string::npos) break;
        at = next + 1;
    }
    if (part.size() != 6 && part.size() != 7) return false;
    static const char* const src[] = { "density", "v_x", "v_y", "v_z", "obs", "pressure" };
    static const char* const kind[] = { "slice", "sum", "max", "min" };
    static const char* const axis[] = { "x", "y", "z" };
    auto pick = [](const std::string& p, const char* const* names, int n, int* out) {
        for (int k = 0; k < n; ++k)
            if (p == names[k]) { *out = k; return true; }
        char* end = nullptr;
        *out = (int)strtol(p.c_str(), &end, 10);
        return !p.empty() && *end == 0;
    };
    if (!pick(part[0], src, 6, &spec[0]) || !pick(part[1], kind, 4, &spec[1]) || !pick(part[2], axis, 3, &spec[2])) return false;
    char* end = nullptr;
    spec[3] = (int)strtol(part[3].c_str(), &end, 10);
    if (part[3].empty() || *end) return false;
    range[2] = 0.2;
    for (size_t k = 4; k < part.size(); ++k) {
        range[k - 4] = strtod(part[k].c_str(), &end);
        if (part[k].empty() || *end) return false;
    }
    return true;
}

// drains the image log into DIR/<view number>_<step>.png
int write_images(fs_sim* sim, const std::string& dir, const std::vector<int>& spec)
{
    long n = 0, dropped = 0;
    int frame_bytes = 0;
    if (fs_image_log(sim, nullptr, nullptr, 0, &n, &dropped) || fs_get_int(sim, "image_frame_bytes", &frame_bytes)) return 1;
    if (n == 0) return 0;
    std::vector<uint8_t> frames((size_t)n * (size_t)frame_bytes);
    std::vector<long> steps((size_t)n);
    if (fs_image_log(sim, frames.data(), steps.data(), n, &n, &dropped)) return 1;
    if (dropped) fprintf(stderr, "simulation.out: %ld image frames were overwritten before they were written\n", dropped);
    for (long i = 0; i < n; ++i) {
        size_t at = (size_t)i * (size_t)frame_bytes;
        for (size_t v = 0; v < spec.size() / 4; ++v) {
            int cols = 0, rows = 0;
            if (fs_image_values(sim, spec[4 * v], spec[4 * v + 1], spec[4 * v + 2], spec[4 * v + 3], nullptr, 0, &cols, &rows)) return 1;
            const std::string path = dir + "/" + std::to_string(v) + "_" + std::to_string(steps[(size_t)i]) + ".png";
            if (fs_image_png(&frames[at], cols, rows, path.c_str())) return 1;
            at += 3 * (size_t)cols * (size_t)rows;
        }
    }
    return 0;
}

// drains the volume log (one view of cols x rows) into DIR/<step>.png
int write_volumes(fs_sim* sim, const std::string& dir, int cols, int rows)
{
    long n = 0, dropped = 0;
    if (fs_volume_log(sim, nullptr, nullptr, 0, &n, &dropped)) return 1;
    if (n == 0) return 0;
    const size_t frame_bytes = 3 * (size_t)cols * (size_t)rows;
    std::vector<uint8_t> frames((size_t)n * frame_bytes);
    std::vector<long> steps((size_t)n);
    if (fs_volume_log(sim, frames.data(), steps.data(), n, &n, &dropped)) return 1;
    if (dropped) fprintf(stderr, "simulation.out: %ld volume frames were overwritten before they were written\n", dropped);
    for (long i = 0; i < n; ++i) {
        const std::string path = dir + "/" + std::to_string(steps[(size_t)i]) + ".png";
        if (fs_image_png(&frames[(size_t)i * frame_bytes], cols, rows, path.c_str())) return 1;
    }
    return 0;
}

int die(const char* what)
{
    fprintf(stderr, "simulation.out: %s: %s\n", what, fs_last_error());
    return 1;
}

}  // namespace

int main(int argc, char** argv)
{
    // simulation.cpp:431-436
    int scale = 1;
    int width = 128 * scale, height = 64 * scale, depth = 64 * scale;
    int iter = 100, speed = FS_DEFAULT_SPEED, acc = FS_DEFAULT_ACC;
    float dt = FS_DEFAULT_DT, diff = FS_DEFAULT_DIFF, visc = FS_DEFAULT_VISC;
    std::vector<Stl> stls;
    bool stl_given = false, json = false;
    std::string resume_dir, forces_path, residuals_path, mean_dir, vortex_dir, probes_path, probe_log_path, body_forces_path;
    bool mean_moments = false;
    std::string images_dir, tracer_emitters_path, tracer_out_path;
    long tracers = 0, tracer_every = 1;
    bool tracer_every_given = false;
    long image_every = 1;
    std::string volume_dir;
    double volume_view[3] = {45.0, 30.0, 200.0}, volume_range[2] = {0.0, 0.01}, volume_opacity = 0.05;
    int volume_cols = 512, volume_rows = 512;
    long volume_every = 1;
    std::string monitor_path, inflow_profile_path, inflow_gust_path;
    bool inflow = false;
    long monitor_every = 1;
    bool heat = false, heat_other = false;
    double heat_par[FS_HEAT_PARAMS] = { 2, 0, 0, 0, 2, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0 };   // mode 2, up = +y; a box of zeros = the whole domain
    std::string heat_log_path, heat_dump_path;
    std::vector<double> zone_rows;                       // --zone, FS_ZONE_PARAMS numbers each
    std::string zone_log_path;
    int dump_every = 1;
    std::vector<int> view_spec;
    std::vector<double> view_range;
    std::vector<std::pair<std::string, std::string>> options;

    auto apply = [&](const std::string& key, const char* val) -> bool {
        if (key == "grid") return sscanf(val, "%dx%dx%d", &width, &height, &depth) == 3;
        if (key == "steps") { iter = atoi(val); return true; }
        if (key == "acc") { acc = atoi(val); return true; }
        if (key == "speed") { speed = atoi(val); return true; }
        if (key == "dt") { dt = (float)atof(val); return true; }
        if (key == "diff") { diff = (float)atof(val); return true; }
        if (key == "stl") { stl_given = true; if (strcmp(val, "none") != 0) stls.push_back(parse_stl(val)); return true; }
        if (key == "dump-every") { dump_every = atoi(val); options.push_back({ "dump_every", val }); return true; }
        if (key == "images") { images_dir = val; return true; }
        if (key == "image-every") { image_every = atol(val); return image_every >= 1; }
        if (key == "image-view") {
            int sp[4];
            double rg[3];
            if (!parse_view(val, sp, rg)) return false;
            view_spec.insert(view_spec.end(), sp, sp + 4);
            view_range.insert(view_range.end(), rg, rg + 3);
            return true;
        }
        if (key == "volume") { volume_dir = val; return true; }
        if (key == "volume-view") return sscanf(val, "%lf,%lf,%lf", &volume_view[0], &volume_view[1], &volume_view[2]) == 3;
        if (key == "volume-size") return sscanf(val, "%dx%d", &volume_cols, &volume_rows) == 2;
        if (key == "volume-range") return sscanf(val, "%lf,%lf", &volume_range[0], &volume_range[1]) == 2;
        if (key == "volume-opacity") { volume_opacity = atof(val); return true; }
        if (key == "volume-every") { volume_every = atol(val); return volume_every >= 1; }
        if (key == "dump-dir") { options.push_back({ "dump_dir", val }); return true; }
        if (key == "precision") { options.push_back({ "precision", val }); return true; }
        if (key == "solver") { options.push_back({ "solver", val }); return true; }
        if (key == "omega") { options.push_back({ "sor_omega", val }); return true; }
        if (key == "mg-cycles") { options.push_back({ "mg_cycles", val }); return true; }
        if (key == "seed") { options.push_back({ "voxel_seed", val }); return true; }
        if (key == "resume") { resume_dir = val; return true; }
        if (key == "forces") { forces_path = val; return true; }
        if (key == "body-forces") { body_forces_path = val; return true; }
        if (key == "moment-origin") { options.push_back({ "moment_origin", val }); return true; }
        if (key == "residuals") { residuals_path = val; return true; }
        if (key == "mean-flow") { mean_dir = val; return true; }
        if (key == "vortex") { vortex_dir = val; return true; }
        if (key == "probes") { probes_path = val; return true; }
        if (key == "probe-log") { probe_log_path = val; return true; }
        if (key == "tracers") { tracers = atol(val); return tracers >= 0; }
        if (key == "tracer-emitters") { tracer_emitters_path = val; return true; }
        if (key == "tracer-every") { tracer_every = atol(val); tracer_every_given = true; return tracer_every >= 1; }
        if (key == "tracer-out") { tracer_out_path = val; return true; }
        if (key == "mean-from") { options.push_back({ "flow_stats_start", val }); return true; }
        if (key == "mean-every") { options.push_back({ "flow_stats_every", val }); return true; }
        if (key == "confinement") { options.push_back({ "vorticity_confinement", val }); return true; }
        if (key == "monitor") { monitor_path = val; return true; }
        if (key == "inflow-profile") { inflow_profile_path = val; inflow = true; return true; }
        if (key == "inflow-gust") { inflow_gust_path = val; inflow = true; return true; }
        if (key == "inflow-eddies") { options.push_back({ "inflow_eddies", val }); inflow = true; return true; }
        if (key == "inflow-sigma") { options.push_back({ "inflow_sigma", val }); inflow = true; return true; }
        if (key == "inflow-rms") { options.push_back({ "inflow_rms", val }); inflow = true; return true; }
        if (key == "inflow-convect") { options.push_back({ "inflow_convect", val }); inflow = true; return true; }
        if (key == "inflow-seed") { options.push_back({ "inflow_seed", val }); inflow = true; return true; }
        if (key == "heat") { heat = true; return sscanf(val, "%lf,%lf,%lf", &heat_par[1], &heat_par[2], &heat_par[3]) == 3; }
        if (key == "heat-up") {
            static const char* const axes[6] = { "+x", "-x", "+y", "-y", "+z", "-z" };
            heat_other = true;
            for (int k = 0; k < 6; ++k)
                if (strcmp(val, axes[k]) == 0) { heat_par[4] = k; return true; }
            return false;
        }
        if (key == "heat-inlet") { heat_other = true; return sscanf(val, "%lf", &heat_par[5]) == 1; }
        if (key == "heat-wall") {
            heat_other = true;
            heat_par[6] = 1;
            const int got = sscanf(val, "%lf,%lf,%lf,%lf,%lf,%lf,%lf", &heat_par[7], &heat_par[8], &heat_par[9], &heat_par[10],
                                   &heat_par[11], &heat_par[12], &heat_par[13]);
            if (got == 1) heat_par[8] = 0;
            return got == 1 || got == 7;
        }
        if (key == "heat-log") { heat_other = true; heat_log_path = val; return true; }
        if (key == "heat-dump") { heat_other = true; heat_dump_path = val; return true; }
        if (key == "zone") {
            const char* p = val;
            for (int k = 0; k < FS_ZONE_PARAMS; ++k) {
                char* end = nullptr;
                const double v = strtod(p, &end);
                if (end == p || *end != (k + 1 < FS_ZONE_PARAMS ? ',' : '\0')) return false;
                zone_rows.push_back(v);
                p = end + 1;
            }
            return true;
        }
        if (key == "zone-log") { zone_log_path = val; return true; }
        if (key == "monitor-every") { monitor_every = atol(val); return monitor_every >= 1; }
        if (key == "monitor-stations") { options.push_back({ "monitor_stations", val }); return true; }
        return false;
    };
    static const char* const keys[] = { "grid", "steps", "acc", "speed", "dt", "diff", "stl", "dump-every", "dump-dir",
                                        "precision", "solver", "omega", "mg-cycles", "seed", "resume", "forces", "residuals", "mean-flow", "mean-from",
                                        "mean-every", "vortex", "probes", "probe-log", "body-forces", "moment-origin", "images", "image-every",
                                        "image-view", "tracers", "tracer-emitters", "tracer-every", "tracer-out", "volume", "volume-view", "volume-size",
                                        "volume-range", "volume-opacity", "volume-every", "confinement", "monitor", "monitor-every", "monitor-stations",
                                        "inflow-profile", "inflow-gust", "inflow-eddies", "inflow-sigma", "inflow-rms", "inflow-convect", "inflow-seed",
                                        "heat", "heat-up", "heat-inlet", "heat-wall", "heat-log", "heat-dump", "zone", "zone-log" };
    for (const char* k : keys) {
        std::string env = "FS_";
        for (const char* p = k; *p; ++p) env += (*p == '-') ? '_' : (char)toupper(*p);
        if (const char* v = getenv(env.c_str()))
            if (!apply(k, v)) { fprintf(stderr, "simulation.out: bad value for %s\n", env.c_str()); return 2; }
    }
    if (getenv("FS_QUIET")) options.push_back({ "quiet", "1" });
    if (getenv("FS_MEAN_MOMENTS")) mean_moments = true;
    for (int i = 1; i < argc; ++i) {
        std::string a = argv[i];
        if (a == "--quiet") { options.push_back({ "quiet", "1" }); continue; }
        if (a == "--json") { json = true; continue; }
        if (a == "--mean-moments") { mean_moments = true; continue; }
        if (a.rfind("--", 0) != 0 || i + 1 >= argc || !apply(a.substr(2), argv[i + 1])) {
            fprintf(stderr, "simulation.out: unknown or malformed argument '%s' (see src/main.cpp)\n", argv[i]);
            return 2;
        }
        ++i;
    }
    if (tracers == 0 && (!tracer_emitters_path.empty() || !tracer_out_path.empty())) {
        fprintf(stderr, "simulation.out: --tracer-emitters and --tracer-out need --tracers C with C > 0\n");
        return 2;
    }
    if (tracer_every_given && tracer_emitters_path.empty()) {
        fprintf(stderr, "simulation.out: --tracer-every is the emitters' release period and needs --tracer-emitters\n");
        return 2;
    }
    if (heat_other && !heat) {
        fprintf(stderr, "simulation.out: --heat-up, --heat-inlet, --heat-wall, --heat-log and --heat-dump need --heat KAPPA,BETA,ALPHA\n");
        return 2;
    }
    if (!zone_log_path.empty() && zone_rows.empty()) {
        fprintf(stderr, "simulation.out: --zone-log needs --zone SPEC\n");
        return 2;
    }
    if (zone_rows.size() > (size_t)FS_ZONE_MAX * FS_ZONE_PARAMS) {
        fprintf(stderr, "simulation.out: --zone was given %zu times, a run takes %d zones\n", zone_rows.size() / FS_ZONE_PARAMS, FS_ZONE_MAX);
        return 2;
    }
    if (!stl_given) {
        Stl s;
        s.path = "/media/raoul/Speed/Data/3D-Printing/Models/Cars/F1Car-basic.stl";   // simulation.cpp:441
        stls.push_back(s);
    }

    fs_sim* sim = fs_create(width, height, depth, iter, speed, dt, diff, visc, acc);   // simulation.cpp:438
    if (!sim) return die("fs_create");
    if (!forces_path.empty()) options.push_back({ "force_log", std::to_string(iter) });
    if (!body_forces_path.empty()) options.push_back({ "body_force_log", std::to_string(iter) });
    if (!residuals_path.empty()) options.push_back({ "residual_log", std::to_string(iter) });
    if (!monitor_path.empty()) {
        options.push_back({ "monitor_every", std::to_string(monitor_every) });
        options.push_back({ "monitor_log", std::to_string(std::min(1048576L, iter > 0 ? (iter - 1) / monitor_every + 1 : 0L)) });
    }
    if (!mean_dir.empty()) options.push_back({ "flow_stats", mean_moments ? "moments" : "mean" });
    std::vector<int> probe_cells;
    if (!probes_path.empty()) {
        if (read_probes(probes_path.c_str(), probe_cells)) return 2;
        if (fs_set_probes(sim, probe_cells.data(), (long)(probe_cells.size() / 3))) return die("fs_set_probes");
    }
    if (!probe_log_path.empty()) options.push_back({ "probe_log", std::to_string(iter) });
    if (tracers > 0) options.push_back({ "tracers", std::to_string(tracers) });
    if (inflow) options.push_back({ "inflow", "on" });
    if (!inflow_profile_path.empty()) {
        std::vector<double> maps;
        const size_t cells = (size_t)height * (size_t)depth;
        if (read_numbers(inflow_profile_path.c_str(), maps)) return 2;
        if (maps.size() != cells && maps.size() != 2 * cells) {
            fprintf(stderr, "simulation.out: %s holds %zu numbers, not height * depth = %zu or twice as many\n", inflow_profile_path.c_str(),
                    maps.size(), cells);
            return 2;
        }
        if (fs_inflow_profile(sim, maps.data(), maps.size() == cells ? nullptr : maps.data() + cells, cells)) return die("fs_inflow_profile");
    }
    if (!inflow_gust_path.empty()) {
        std::vector<double> knots, steps, factors;
        if (read_numbers(inflow_gust_path.c_str(), knots)) return 2;
        if (knots.size() % 2) { fprintf(stderr, "simulation.out: %s: expected pairs `step factor`\n", inflow_gust_path.c_str()); return 2; }
        for (size_t i = 0; i < knots.size(); i += 2) { steps.push_back(knots[i]); factors.push_back(knots[i + 1]); }
        if (fs_inflow_gust(sim, steps.data(), factors.data(), (int)std::min<size_t>(steps.size(), 1u << 20))) return die("fs_inflow_gust");
    }
    for (auto& kv : options)
        if (fs_set_option(sim, kv.first.c_str(), kv.second.c_str())) return die(kv.first.c_str());
    if (!tracer_emitters_path.empty()) {
        std::vector<double> pts;
        if (read_points(tracer_emitters_path.c_str(), pts)) return 2;
        if (fs_tracer_emitters(sim, pts.data(), (long)(pts.size() / 3), tracer_every)) return die("fs_tracer_emitters");
    }
    if (heat) {
        if (heat_par[8] == 0) {                          // no box given: the whole domain
            const double whole[6] = { 1, (double)width, 1, (double)height, 1, (double)depth };
            for (int k = 0; k < 6; ++k) heat_par[8 + k] = whole[k];
        }
        if (!heat_log_path.empty()) heat_par[14] = (double)std::min(1048576L, (long)std::max(iter, 0));
        if (fs_heat_params(sim, heat_par, FS_HEAT_PARAMS)) return die("fs_heat_params");
        if (!heat_dump_path.empty()) remove(heat_dump_path.c_str());   // the run appends to it
    }
    const int n_zones = (int)(zone_rows.size() / FS_ZONE_PARAMS);
    if (n_zones > 0 &&
        fs_zones(sim, zone_rows.data(), n_zones, 2, zone_log_path.empty() ? 0 : (int)std::min(1048576L, (long)std::max(iter, 0))))
        return die("fs_zones");
    bool stepwise = !heat_dump_path.empty();            // --images, --volume: the run's frames do not fit the ring; --heat-dump
    long image_ring = 0;
    if (!images_dir.empty()) {
        if (view_spec.empty()) {                         // the 2-D viewer's density and v_x frames (gui.py:271-279)
            const int mid = (depth + 2) / 2;
            view_spec = { FS_DENS, FS_IMG_SLICE, 2, mid, FS_VX, FS_IMG_SLICE, 2, mid };
            view_range = { 0.0, 0.01, 0.2, -10.0, 10.0, 0.2 };
        }
        mkdir(images_dir.c_str(), 0777);
        if (fs_image_views(sim, view_spec.data(), view_range.data(), (int)(view_spec.size() / 4))) return die("fs_image_views");
        int frame_bytes = 0;
        if (fs_get_int(sim, "image_frame_bytes", &frame_bytes)) return die("image_frame_bytes");
        const long wanted = iter > 0 ? (iter - 1) / image_every + 1 : 0;
        const long room = std::max(1L, std::min(65536L, (256L << 20) / std::max(1, frame_bytes)));
        image_ring = std::max(1L, std::min(wanted, room));
        stepwise = wanted > room;
        if (fs_set_option(sim, "image_every", std::to_string(image_every).c_str())) return die("image_every");
        if (fs_set_option(sim, "image_log", std::to_string(image_ring).c_str())) return die("image_log");
    }
    long volume_ring = 0;
    if (!volume_dir.empty()) {
        // the 3-D viewer's orbit (GUI/gl_widget.py:71-74) about the box centre, y up; the library takes tan(fov / 2)
        const double rad = 3.14159265358979323846 / 180.0, az = volume_view[0] * rad, el = volume_view[1] * rad, dist = volume_view[2];
        const double centre[3] = { 0.5 * (width + 1), 0.5 * (height + 1), 0.5 * (depth + 1) };
        const double cam[FS_VOLUME_CAMERA] = { centre[0] - dist * std::cos(el) * std::sin(az), centre[1] + dist * std::sin(el),
                                               centre[2] + dist * std::cos(el) * std::cos(az), centre[0], centre[1], centre[2],
                                               0.0, 1.0, 0.0, std::tan(22.5 * rad), 0.0 };
        mkdir(volume_dir.c_str(), 0777);
        if (fs_volume_camera(sim, 0, cam, volume_cols, volume_rows)) return die("fs_volume_camera");
        const int vspec[2] = { FS_DENS, 0 };
        const double vpar[FS_VOLUME_PARAMS] = { volume_range[0], volume_range[1], volume_opacity, 0.5, 0.01, 128.0, 128.0, 128.0,
                                                26.0, 26.0, 26.0 };
        if (fs_volume_views(sim, vspec, vpar, 1)) return die("fs_volume_views");
        const long frame_bytes = 3L * volume_cols * volume_rows;
        const long wanted = iter > 0 ? (iter - 1) / volume_every + 1 : 0;
        const long room = std::max(1L, std::min(65536L, (256L << 20) / std::max(1L, frame_bytes)));
        volume_ring = std::max(1L, std::min(wanted, room));
        stepwise = stepwise || wanted > room;
        if (fs_set_option(sim, "volume_every", std::to_string(volume_every).c_str())) return die("volume_every");
        if (fs_set_option(sim, "volume_log", std::to_string(volume_ring).c_str())) return die("volume_log");
    }
    for (const Stl& s : stls) {
        int rc = fs_load_stl(sim, s.path.c_str(), s.v[0], s.v[1], s.v[2], s.v[3], s.v[4], s.v[5], s.v[6], nullptr);
        if (rc != FS_OK && rc != FS_EIO) return die("fs_load_stl");   // unreadable STL: carry on with an empty tunnel
    }
    if (!resume_dir.empty()) {
        static const char* const names[5] = { "data.bin", "obs.bin", "v_x.bin", "v_y.bin", "v_z.bin" };
        static const int which[5] = { FS_DENS, FS_OBS, FS_VX, FS_VY, FS_VZ };
        for (int k = 0; k < 5; ++k)
            if (resume_field(sim, resume_dir, names[k], which[k])) return 1;
    }
    const auto t0 = std::chrono::steady_clock::now();
    if (!stepwise) {
        if (fs_run(sim)) return die("fs_run");                          // simulation.cpp:448
    } else {
        for (int i = 0; i < iter; ++i) {
            if (fs_run_one(sim)) return die("fs_run_one");
            if (dump_every > 0 && (i + 1) % dump_every == 0) {
                if (fs_dump_frame(sim)) return die("fs_dump_frame");
                if (!heat_dump_path.empty() && append_heat_frame(sim, heat_dump_path.c_str())) return die("--heat-dump");
            }
            long kept = 0;
            if (!images_dir.empty()) {
                if (fs_image_log(sim, nullptr, nullptr, 0, &kept, nullptr)) return die("fs_image_log");
                if (kept == image_ring && write_images(sim, images_dir, view_spec)) return die("writing the images");
            }
            if (!volume_dir.empty()) {
                if (fs_volume_log(sim, nullptr, nullptr, 0, &kept, nullptr)) return die("fs_volume_log");
                if (kept == volume_ring && write_volumes(sim, volume_dir, volume_cols, volume_rows)) return die("writing the volume frames");
            }
        }
        if (dump_every == -1) {
            if (fs_dump_frame(sim)) return die("fs_dump_frame");
            if (!heat_dump_path.empty() && append_heat_frame(sim, heat_dump_path.c_str())) return die("--heat-dump");
        }
    }
    if (fs_sync(sim)) return die("fs_sync");
    const double secs = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    if (!forces_path.empty() && write_forces(sim, forces_path.c_str(), width, height, depth, dt, speed)) return die("fs_force_log");
    if (!body_forces_path.empty() && write_body_forces(sim, body_forces_path.c_str(), width, height, depth, dt, speed)) return die("fs_body_force_log");
    if (!residuals_path.empty() && write_residuals(sim, residuals_path.c_str())) return die("fs_residual_log");
    if (!monitor_path.empty() && write_monitor(sim, monitor_path.c_str(), width, height, depth, dt)) return die("fs_monitor_log");
    if (!heat_log_path.empty() && write_heat_log(sim, heat_log_path.c_str())) return die("fs_heat_log");
    if (!zone_log_path.empty() && write_zone_log(sim, n_zones, zone_log_path.c_str())) return die("fs_zone_log");
    if (!probe_log_path.empty() && write_probes(sim, probe_log_path.c_str(), (long)(probe_cells.size() / 3))) return die("fs_probe_log");
    if (!images_dir.empty() && write_images(sim, images_dir, view_spec)) return die("writing the images");
    if (!volume_dir.empty() && write_volumes(sim, volume_dir, volume_cols, volume_rows)) return die("writing the volume frames");
    if (!tracer_out_path.empty() && write_tracers(sim, tracer_out_path.c_str())) return die("fs_tracer_fetch");
    int mean_samples = 0;
    if (!mean_dir.empty()) {
        if (fs_get_int(sim, "flow_stats_samples", &mean_samples)) return die("flow_stats_samples");
        if (fs_flow_stats_dump(sim, mean_dir.c_str())) return die("fs_flow_stats_dump");
    }
    if (!vortex_dir.empty() && fs_vortex_dump(sim, vortex_dir.c_str())) return die("fs_vortex_dump");
    if (json)
        printf("{\"grid\": [%d, %d, %d], \"steps\": %d, \"acc\": %d, \"seconds\": %.6f, \"cells_steps_per_sec\": %.6g, "
               "\"mean_flow_samples\": %d}\n",
               width, height, depth, iter, acc, secs, (double)width * height * depth * iter / secs, mean_samples);
    fs_destroy(sim);
    return 0;
}
