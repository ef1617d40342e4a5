// monitor.h -- the flow monitor on the device (fs_flow_monitor, fs_monitor_sample, option "monitor_log"): order-defined
// integrals and extrema of the state over the TARGET cells, per plane, whole and per x.  include/fluidsim.h ("Flow monitor")
// defines every number; monitor_plan.h every index.  Internal to libfluidsim.so.  Beyond the reference, whose run() prints
// sum / min / max of whole padded arrays through the host (simulation.cpp:73-93).
#pragma once
#include "kernels.h"
#include "monitor_plan.h"

namespace fs {

// the x indices (1 .. W) whose X-PROFILE rows a record carries, 0 = unused
struct MonitorStations {
    int x[MON_STATIONS];
};

// doubles of the workspace for this grid (monitor_plan.h)
size_t monitor_workspace_doubles(const GridDesc& g);

// One record of the state q, u, v, w, p (LEAD-shifted field pointers) in three launches on `st`: the COLUMN records, then
// the PLANE records and the X-PROFILE, then the WHOLE record and the stations' profile rows into `result` (MON_RESULT doubles
// on the device: a ring slot, or the workspace's own result slot).  Reads rows 1..H of planes 1..D of the five fields and the
// flag bytes; writes `ws` and `result`, nothing else.  Single GPU (g.zh == 1); no atomics, every sum in its written order.
template <class T>
void launch_monitor(hipStream_t st, const GridDesc& g, const T* q, const T* u, const T* v, const T* w, const T* p,
                    const uint8_t* flags, const MonitorStations& stations, double* ws, double* result);

}  // namespace fs
