"""ctypes binding of libfluidsim.so (C ABI: include/fluidsim.h).

The shared library is the product; this module only declares its signatures.  There is no
Python or CPU implementation behind it: if the library is missing or no MI355X is usable,
the error is raised to the caller.
"""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
# FLUIDSIM_LIB: development override (e.g. a host-sanitizer build of the same sources)
LIB_PATH = os.environ.get("FLUIDSIM_LIB") or os.path.join(_HERE, "libfluidsim.so")

OK, EINVAL, EIO, EHIP, ECOMM, ENOMEM = 0, -1, -2, -3, -4, -5
DENS, VX, VY, VZ, OBS, PRESSURE, DIVERGENCE, VX_PREV, VY_PREV, VZ_PREV, BUFFER = range(11)
FIELD_NAMES = ["dens", "v_x", "v_y", "v_z", "obs", "pressure", "divergence",
               "v_x_prev", "v_y_prev", "v_z_prev", "buffer"]
COMM_ID_BYTES = 128
FORCE_LOG_COLS = 9      # FS_FORCE_LOG_COLS: step, S1x, S1y, S1z, S2x, S2y, S2z, faces, frontal
BODY_MAX = 16           # FS_BODY_MAX: bodies with a record of their own; the other components share record 0, the REST
BODY_COLS = 8           # FS_BODY_COLS: Sx, Sy, Sz, Mx, My, Mz, faces, frontal rows
BODY_INFO_COLS = 12     # FS_BODY_INFO_COLS: cells, anchor, xmin, xmax, ymin, ymax, zmin, zmax, sum x, sum y, sum z, frontal rows
BODY_LOG_COLS = 16      # FS_BODY_LOG_COLS: step, body, S1xyz, M1xyz, S2xyz, M2xyz, faces, frontal rows
RESIDUAL_COLS = 4       # FS_RESIDUAL_COLS: sum r^2, sum x0^2, max |r|, free cells
RESIDUAL_LOG_SOLVES = 6     # FS_RESIDUAL_LOG_SOLVES: diffuse v_x, v_y, v_z, projection 1, projection 2, diffuse density
RESIDUAL_LOG_COLS = 31      # FS_RESIDUAL_LOG_COLS: step, then per solve r0_sq, r_sq, r_max, rhs_sq, cells
MONITOR_COLS = 16           # FS_MONITOR_COLS: the flow monitor's PLANE / WHOLE record
MONITOR_PROFILE_COLS = 5    # FS_MONITOR_PROFILE_COLS: cells, sum u, sum u*u, sum p, sum q*u of one x
MONITOR_STATIONS_MAX = 8    # FS_MONITOR_STATIONS_MAX
INFLOW_EDDIES_MAX = 65536   # FS_INFLOW_EDDIES_MAX: eddies of the inflow generator
INFLOW_KNOTS_MAX = 4096     # FS_INFLOW_KNOTS_MAX: knots of its gust schedule
MONITOR_LOG_COLS = 57       # FS_MONITOR_LOG_COLS: step, the whole record, then the profile row of each of 8 stations
# FS_STAT_*: selectors of fs_flow_stats_field -- the five means, the seven (co)variances, the turbulence kinetic energy;
# STAT_RAW or-ed in returns the raw sum instead
(STAT_MEAN_DENS, STAT_MEAN_VX, STAT_MEAN_VY, STAT_MEAN_VZ, STAT_MEAN_P,
 STAT_UU, STAT_VV, STAT_WW, STAT_UV, STAT_UW, STAT_VW, STAT_PP, STAT_TKE) = range(13)
STAT_RAW = 256
STAT_NAMES = ["mean_dens", "mean_vx", "mean_vy", "mean_vz", "mean_p", "uu", "vv", "ww", "uv", "uw", "vw", "pp", "tke"]
# FS_VORTEX_*: selectors of fs_vortex_field -- the three vorticity components, |omega|^2, Q; ISO_VORTEX or-ed in makes one
# of them a source of fs_isosurface.  VORTEX_NAMES: the file stems of fs_vortex_dump
VORTEX_WX, VORTEX_WY, VORTEX_WZ, VORTEX_W2, VORTEX_Q = range(5)
VORTEX_NFIELDS = 5
ISO_VORTEX = 512
VORTEX_NAMES = ["vort_x", "vort_y", "vort_z", "vort_sq", "q"]
# FS_SAMPLE_*: modes of fs_sample; SAMPLE_STAT or-ed with a STAT_* selector (and STAT_RAW) makes it a source of fs_sample
SAMPLE_NEAREST, SAMPLE_LINEAR, SAMPLE_FLUID = range(3)
SAMPLE_MODES = {"nearest": SAMPLE_NEAREST, "linear": SAMPLE_LINEAR, "fluid": SAMPLE_FLUID}
SAMPLE_STAT = 1024
PROBE_MAX = 4096        # FS_PROBE_MAX: probes fs_set_probes takes
PROBE_VALUES = 5        # FS_PROBE_VALUES: dens, v_x, v_y, v_z, pressure per probe and record
PROBE_NAMES = ["dens", "v_x", "v_y", "v_z", "pressure"]
# FS_IMG_*: kinds of fs_image_values / fs_image_rgb -- a slice, or the sum, maximum or minimum along the axis
IMG_SLICE, IMG_SUM, IMG_MAX, IMG_MIN = range(4)
IMG_KINDS = {"slice": IMG_SLICE, "sum": IMG_SUM, "max": IMG_MAX, "min": IMG_MIN}
IMAGE_VIEWS_MAX = 8     # FS_IMAGE_VIEWS_MAX: views fs_image_views takes
# FS_TRACER_*: the status word of a tracer slot; the emitters fs_tracer_emitters takes; bytes per slot of a snapshot frame
TRACER_FREE, TRACER_ALIVE, TRACER_OUT, TRACER_HIT = range(4)
TRACER_STATUS_NAMES = ["free", "alive", "out", "hit"]
TRACER_EMITTERS_MAX = 4096
TRACER_FRAME_BYTES = 28
# FS_VOLUME_*: camera slots and log views of the volume renderer, entries of a view's parameters and of a camera, and the
# most samples a ray may take through the box
VOLUME_CAMERAS_MAX = 4
VOLUME_VIEWS_MAX = 4
VOLUME_PARAMS = 11      # vmin, vmax, opacity, step, t_min, obstacle r g b, background r g b
VOLUME_CAMERA = 11      # eye[3], target[3], up[3], half_height, ortho
VOLUME_SAMPLES_MAX = 16384
# heat and buoyancy: entries of fs_heat_params, columns of the heat budget and of a row of fs_heat_log, the temperature as a
# source of fs_sample, the image and volume entries and fs_isosurface, the codes of `up`
HEAT_PARAMS = 15        # FS_HEAT_PARAMS
HEAT_COLS = 9           # FS_HEAT_COLS
HEAT_LOG_COLS = 10      # FS_HEAT_LOG_COLS: step, then the budget
SOURCE_HEAT = 8192      # FS_SOURCE_HEAT
HEAT_NAMES = ["cells", "sum", "sum_sq", "max", "min", "held", "loss", "outflow", "inflow"]
HEAT_UP = {"+x": 0, "-x": 1, "+y": 2, "-y": 3, "+z": 4, "-z": 5}
# momentum zones: zones of a handle, entries of a zone's row, columns of a zone's budget, modes of fs_zones
ZONE_MAX = 8            # FS_ZONE_MAX
ZONE_PARAMS = 20        # FS_ZONE_PARAMS
ZONE_COLS = 7           # FS_ZONE_COLS
ZONE_NAMES = ["cells", "dvx", "dvy", "dvz", "dke", "flux", "max_speed"]
ZONE_MODES = {"off": 0, "manual": 1, "step": 2}


class FluidsimError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__("fluidsim error %d: %s" % (code, msg))
        self.code = code


_lib = None

_SIGNATURES = {
    "fs_create": (C.c_void_p, [C.c_int] * 5 + [C.c_float] * 3 + [C.c_int]),
    "fs_destroy": (C.c_int, [C.c_void_p]),
    "fs_set_option": (C.c_int, [C.c_void_p, C.c_char_p, C.c_char_p]),
    "fs_get_int": (C.c_int, [C.c_void_p, C.c_char_p, C.POINTER(C.c_int)]),
    "fs_set_int": (C.c_int, [C.c_void_p, C.c_char_p, C.c_int]),
    "fs_get_float": (C.c_int, [C.c_void_p, C.c_char_p, C.POINTER(C.c_float)]),
    "fs_set_float": (C.c_int, [C.c_void_p, C.c_char_p, C.c_float]),
    "fs_add_obstacle": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int]),
    "fs_add_density": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_float]),
    "fs_set_velocity": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_float, C.c_float, C.c_float]),
    "fs_load_stl": (C.c_int, [C.c_void_p, C.c_char_p] + [C.c_float] * 7 + [C.POINTER(C.c_long)]),
    "fs_set_obstacle_mask": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t]),
    "fs_step": (C.c_int, [C.c_void_p]),
    "fs_run_one": (C.c_int, [C.c_void_p]),
    "fs_run": (C.c_int, [C.c_void_p]),
    "fs_sync": (C.c_int, [C.c_void_p]),
    "fs_set_bounds": (C.c_int, [C.c_void_p, C.c_int, C.c_int]),
    "fs_linear_solver": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_float, C.c_float]),
    "fs_diffuse": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int]),
    "fs_project": (C.c_int, [C.c_void_p]),
    "fs_advect": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int]),
    "fs_get_field": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_size_t, C.c_int]),
    "fs_set_field": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_size_t, C.c_int]),
    "fs_padded_size": (C.c_size_t, [C.c_void_p]),
    "fs_dump_frame": (C.c_int, [C.c_void_p]),
    "fs_field_stats": (C.c_int, [C.c_void_p, C.c_int] + [C.POINTER(C.c_double)] * 3),
    "fs_get_timing": (C.c_int, [C.c_void_p, C.c_char_p, C.POINTER(C.c_double), C.POINTER(C.c_long)]),
    "fs_reset_timing": (C.c_int, [C.c_void_p]),
    "fs_time_sweeps": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_float, C.c_float, C.c_int,
                                 C.POINTER(C.c_double)]),
    "fs_streamlines": (C.c_int, [C.c_void_p, C.c_int, C.c_double, C.c_int, C.c_double, C.c_double,
                                 C.POINTER(C.c_long), C.POINTER(C.c_long)]),
    "fs_streamlines_fetch": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "fs_obstacle_surface": (C.c_int, [C.c_void_p, C.POINTER(C.c_long), C.POINTER(C.c_long)]),
    "fs_obstacle_surface_fetch": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    "fs_surface_case_table": (C.c_int, [C.c_int, C.c_void_p]),
    "fs_obstacle_force": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    "fs_force_log": (C.c_int, [C.c_void_p, C.c_void_p, C.c_long, C.POINTER(C.c_long), C.POINTER(C.c_long)]),
    "fs_label_bodies": (C.c_int, [C.c_void_p, C.POINTER(C.c_long), C.POINTER(C.c_long)]),
    "fs_body_labels": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t]),
    "fs_body_info": (C.c_int, [C.c_void_p, C.c_void_p, C.c_long, C.POINTER(C.c_long)]),
    "fs_body_force": (C.c_int, [C.c_void_p, C.c_void_p, C.c_long, C.POINTER(C.c_long), C.c_void_p]),
    "fs_body_force_log": (C.c_int, [C.c_void_p, C.c_void_p, C.c_long, C.POINTER(C.c_long), C.POINTER(C.c_long)]),
    "fs_solve_residual": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_double, C.c_double, C.c_void_p, C.c_void_p]),
    "fs_diffuse_residual": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "fs_residual_log": (C.c_int, [C.c_void_p, C.c_void_p, C.c_long, C.POINTER(C.c_long), C.POINTER(C.c_long)]),
    "fs_flow_stats_sample": (C.c_int, [C.c_void_p]),
    "fs_flow_stats_reset": (C.c_int, [C.c_void_p]),
    "fs_flow_stats_field": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_size_t, C.c_int]),
    "fs_flow_stats_dump": (C.c_int, [C.c_void_p, C.c_char_p]),
    "fs_vortex_field": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_size_t, C.c_int]),
    "fs_vortex_dump": (C.c_int, [C.c_void_p, C.c_char_p]),
    "fs_confine_vorticity": (C.c_int, [C.c_void_p, C.c_double]),
    "fs_heat_params": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int]),
    "fs_heat_params_get": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int]),
    "fs_heat_apply": (C.c_int, [C.c_void_p]),
    "fs_heat_transport": (C.c_int, [C.c_void_p]),
    "fs_heat_budget": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    "fs_heat_log": (C.c_int, [C.c_void_p, C.c_void_p, C.c_long, C.POINTER(C.c_long), C.POINTER(C.c_long)]),
    "fs_heat_get": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]),
    "fs_heat_set": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]),
    "fs_zones": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int]),
    "fs_zones_get": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "fs_zone_apply": (C.c_int, [C.c_void_p]),
    "fs_zone_budget": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    "fs_zone_log": (C.c_int, [C.c_void_p, C.c_void_p, C.c_long, C.POINTER(C.c_long), C.POINTER(C.c_long)]),
    "fs_zone_mask": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t]),
    "fs_inflow_profile": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t]),
    "fs_inflow_gust": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]),
    "fs_inflow_plane": (C.c_int, [C.c_void_p, C.c_long, C.c_void_p, C.c_size_t]),
    "fs_inflow_eddies": (C.c_int, [C.c_void_p, C.c_long, C.c_void_p, C.c_size_t]),
    "fs_flow_monitor": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "fs_monitor_sample": (C.c_int, [C.c_void_p]),
    "fs_monitor_log": (C.c_int, [C.c_void_p, C.c_void_p, C.c_long, C.POINTER(C.c_long), C.POINTER(C.c_long)]),
    "fs_isosurface": (C.c_int, [C.c_void_p, C.c_int, C.c_double, C.POINTER(C.c_long), C.POINTER(C.c_long)]),
    "fs_isosurface_fetch": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    "fs_sample_points": (C.c_int, [C.c_void_p, C.c_void_p, C.c_long]),
    "fs_sample": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_long]),
    "fs_set_probes": (C.c_int, [C.c_void_p, C.c_void_p, C.c_long]),
    "fs_probe_sample": (C.c_int, [C.c_void_p]),
    "fs_probe_log": (C.c_int, [C.c_void_p, C.c_void_p, C.c_long, C.POINTER(C.c_long), C.POINTER(C.c_long)]),
    "fs_image_values": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_size_t,
                                  C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "fs_image_rgb": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_double, C.c_double, C.c_double, C.c_void_p,
                               C.c_size_t, C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "fs_image_colormap": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int]),
    "fs_image_png": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_char_p]),
    "fs_image_views": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]),
    "fs_image_sample": (C.c_int, [C.c_void_p]),
    "fs_image_log": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_long, C.POINTER(C.c_long), C.POINTER(C.c_long)]),
    "fs_tracer_seed": (C.c_int, [C.c_void_p, C.c_void_p, C.c_long]),
    "fs_tracer_emitters": (C.c_int, [C.c_void_p, C.c_void_p, C.c_long, C.c_long]),
    "fs_tracer_clear": (C.c_int, [C.c_void_p]),
    "fs_tracer_advance": (C.c_int, [C.c_void_p]),
    "fs_tracer_fetch": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_long, C.POINTER(C.c_long)]),
    "fs_tracer_sample": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_long]),
    "fs_tracer_log": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_long, C.POINTER(C.c_long),
                                C.POINTER(C.c_long)]),
    "fs_volume_rays": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int]),
    "fs_volume_camera": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int]),
    "fs_volume_render": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t]),
    "fs_volume_views": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]),
    "fs_volume_sample": (C.c_int, [C.c_void_p]),
    "fs_volume_log": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_long, C.POINTER(C.c_long), C.POINTER(C.c_long)]),
    "fs_comm_unique_id": (C.c_int, [C.c_void_p]),
    "fs_comm_init": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p]),
    "fs_comm_selftest": (C.c_int, []),
    "fs_comm_transport": (C.c_char_p, [C.c_void_p]),
    "fs_last_error": (C.c_char_p, []),
    "fs_version": (C.c_char_p, []),
}


def exported_symbols():
    """Every entry point include/fluidsim.h declares."""
    return sorted(_SIGNATURES)


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise FluidsimError(EHIP, "%s is missing: build it with `python -c 'import __graft_entry__ as g; "
                                "g.build()'` or `make -C fluid_simulation_amd/csrc` (no CPU fallback exists)" % LIB_PATH)
        L = C.CDLL(LIB_PATH)
        for name, (res, args) in _SIGNATURES.items():
            try:
                fn = getattr(L, name)
            except AttributeError:
                if os.environ.get("FLUIDSIM_LIB"):       # development: an older build named explicitly (tools/ab_lib.py)
                    continue
                raise
            fn.restype = res
            fn.argtypes = args
        _lib = L
    return _lib


def check(rc):
    if rc != 0:
        raise FluidsimError(rc, (lib().fs_last_error() or b"").decode(errors="replace"))
    return rc
