"""MI355X-native 3-D wind-tunnel solver: the per-step hot path of Ghundi/fluid_simulation
(`Simulation::step()`), rebuilt as hand-written HIP kernels behind a C ABI
(include/fluidsim.h).  Importing the package loads nothing; the shared library is bound
when the first `Simulation` is created and there is no CPU fallback.
"""
from ._lib import (BUFFER, DENS, DIVERGENCE, FIELD_NAMES, OBS, PRESSURE, VX, VX_PREV, VY, VY_PREV, VZ, VZ_PREV,
                   STAT_MEAN_DENS, STAT_MEAN_P, STAT_MEAN_VX, STAT_MEAN_VY, STAT_MEAN_VZ, STAT_NAMES, STAT_PP, STAT_RAW, STAT_TKE,
                   STAT_UU, STAT_UV, STAT_UW, STAT_VV, STAT_VW, STAT_WW, ISO_VORTEX, VORTEX_NAMES, VORTEX_Q, VORTEX_W2, VORTEX_WX,
                   VORTEX_WY, VORTEX_WZ, PROBE_MAX, PROBE_NAMES, PROBE_VALUES, SAMPLE_FLUID, SAMPLE_LINEAR, SAMPLE_NEAREST,
                   SAMPLE_STAT, IMG_SLICE, IMG_SUM, IMG_MAX, IMG_MIN, IMAGE_VIEWS_MAX, TRACER_ALIVE, TRACER_EMITTERS_MAX,
                   TRACER_FRAME_BYTES, TRACER_FREE, TRACER_HIT, TRACER_OUT, TRACER_STATUS_NAMES, BODY_COLS, BODY_INFO_COLS, BODY_LOG_COLS, BODY_MAX,
                   MONITOR_COLS, MONITOR_LOG_COLS, MONITOR_PROFILE_COLS, MONITOR_STATIONS_MAX, HEAT_COLS, HEAT_LOG_COLS, HEAT_NAMES, HEAT_PARAMS,
                   HEAT_UP, SOURCE_HEAT, ZONE_COLS, ZONE_MAX, ZONE_MODES, ZONE_NAMES, ZONE_PARAMS, FluidsimError)
from .simulation import (FORCE_LOG_DTYPE, RESIDUAL_LOG_DTYPE, Simulation, comm_unique_id, loadSTLIntoObstacles, pressure_force,
                         solve_reduction, BODY_INFO_DTYPE, BODY_LOG_DTYPE, pressure_moment, shift_moment,
                         MONITOR_LOG_NAMES, MONITOR_NAMES, MONITOR_PROFILE_NAMES, monitor_cfl)
from . import inflow  # noqa: F401  (host-side helpers of Simulation.set_inflow)
from . import zones  # noqa: F401  (rows for Simulation.set_zones)

__all__ = ["Simulation", "loadSTLIntoObstacles", "comm_unique_id", "pressure_force", "FORCE_LOG_DTYPE", "FluidsimError",
           "RESIDUAL_LOG_DTYPE", "solve_reduction",
           "BODY_INFO_DTYPE", "BODY_LOG_DTYPE", "pressure_moment", "shift_moment", "BODY_MAX", "BODY_COLS", "BODY_INFO_COLS",
           "BODY_LOG_COLS",
           "inflow", "MONITOR_COLS", "MONITOR_PROFILE_COLS", "MONITOR_STATIONS_MAX", "MONITOR_LOG_COLS", "MONITOR_NAMES",
           "MONITOR_PROFILE_NAMES", "MONITOR_LOG_NAMES", "monitor_cfl",
           "HEAT_PARAMS", "HEAT_COLS", "HEAT_LOG_COLS", "HEAT_NAMES", "HEAT_UP", "SOURCE_HEAT",
           "zones", "ZONE_MAX", "ZONE_PARAMS", "ZONE_COLS", "ZONE_NAMES", "ZONE_MODES",
           "FIELD_NAMES", "STAT_NAMES",
           "STAT_MEAN_DENS", "STAT_MEAN_VX", "STAT_MEAN_VY", "STAT_MEAN_VZ", "STAT_MEAN_P", "STAT_UU", "STAT_VV", "STAT_WW",
           "STAT_UV", "STAT_UW", "STAT_VW", "STAT_PP", "STAT_TKE", "STAT_RAW",
           "VORTEX_WX", "VORTEX_WY", "VORTEX_WZ", "VORTEX_W2", "VORTEX_Q", "VORTEX_NAMES", "ISO_VORTEX",
           "SAMPLE_NEAREST", "SAMPLE_LINEAR", "SAMPLE_FLUID", "SAMPLE_STAT", "PROBE_MAX", "PROBE_VALUES", "PROBE_NAMES",
           "IMG_SLICE", "IMG_SUM", "IMG_MAX", "IMG_MIN", "IMAGE_VIEWS_MAX",
           "TRACER_FREE", "TRACER_ALIVE", "TRACER_OUT", "TRACER_HIT", "TRACER_STATUS_NAMES", "TRACER_EMITTERS_MAX",
           "TRACER_FRAME_BYTES",
           "DENS", "VX", "VY", "VZ", "OBS", "PRESSURE", "DIVERGENCE", "VX_PREV", "VY_PREV", "VZ_PREV", "BUFFER"]
