#!/usr/bin/env python3
"""Writes tests/golden/option_replies.json: what a libfluidsim.so answers to every option of fs_set_option -- accepted
extremes, the first refused value on either side, malformed values, every keyword -- and what the fetch entries of the
eight per-step logs answer at capacity 2.  tests/test_gpu_options.py holds the library under test to these replies, so
they are recorded from the library of the commit BEFORE a change to the option or fetch code, on a GPU:

    python tools/record_option_replies.py /path/to/the/parents/libfluidsim.so [out.json]
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

HUGE = "99999999999999999999"        # past a long: strtol saturates
MALFORMED = ["", " ", "x", "5x", "5 ", "1e3", "0x10", HUGE, "-" + HUGE]


def ints(lo, hi):
    """a decimal integer in lo .. hi"""
    return [str(lo), str(hi), str(lo - 1), str(hi + 1), " %d" % lo, "+%d" % hi, "-0", "-1", "007"] + MALFORMED


def reals(least):
    """a finite real >= least"""
    return [repr(float(least)), "%d" % least, "1e3", "1e300", "0x1p4", " 2.5", "+2.5", repr(least - 0.25), "-0.0", "-1",
            "nan", "-nan", "inf", "-inf", "1e400", "1e-400", "", " ", "x", "2.5x", "2.5 ", "2,5"]


def words(*w):
    """one of the keywords"""
    return list(w) + ["", " ", w[0] + " ", " " + w[0], w[0].upper(), w[0][:-1], w[0] + "x", "2", "-1", "on", "off", "auto", "0", "1"]


FLAG = ["0", "1", "", "00", "x", "off"]                      # everything but "0" is on
ATOI = ["0", "1", "-1", "7", "12abc", "abc", "", " 3", "2147483647", HUGE]   # a bare atoi: trailing characters pass


def each(key, values):
    return [[key, v] for v in values]


# option -> the calls put to one handle that is not yet in use
FRESH = {
    "precision": each("precision", words("fp32", "fp64")),
    "solver": each("solver", words("jacobi", "gs_lex", "rbsor", "mg")),
    "mg_cycles": each("mg_cycles", ["0", "1000", "-1", "1001"] + ATOI),
    "mg_pre": each("mg_pre", ["1", "1000", "0", "1001"] + ATOI),
    "mg_post": each("mg_post", ["1", "1000", "0", "1001"] + ATOI),
    "mg_coarse_iters": each("mg_coarse_iters", ["1", "1000", "0", "1001"] + ATOI),
    "mg_min_planes": each("mg_min_planes", ["1", "1024", "0", "1025"] + ATOI),
    "launch_plans": each("launch_plans", ["-1,-1", "127,31", "-2,0", "0,-2", "128,0", "0,32", "3", "3,", ",3", "a,b", "", "1,2,3", " 1, 2", "1;2"]),
    "sor_omega": each("sor_omega", ["1", "1.9999", "0.0001", "0", "2", "-1", "nan", "inf", "", "x", "1.5x", "1e-50"]),
    "dump_dir": each("dump_dir", ["data", "", "a/b c"]),
    "dump_every": each("dump_every", ATOI),
    "voxel_seed": each("voxel_seed", ["0", "1", "4294967295", "4294967296", "-1", "x", "", "5x"]),
    "quiet": each("quiet", FLAG),
    "profile": each("profile", FLAG),
    "elide_dead_density_solve": each("elide_dead_density_solve", FLAG),
    "force_log": each("force_log", ints(0, 1048576)),
    "body_force_log": each("body_force_log", ints(0, 1048576)),
    "moment_origin": each("moment_origin", ["0,0,0", "1.5,-2,3e2", " 1, 2, 3", "1,2", "1,2,3,4", "1,2,3 ", "1,,3", "nan,0,0", "0,inf,0",
                                            "0,0,1e400", "", "x", "1;2;3", "1,2,3x", "+1,-0.0,0x10"]),
    "residual_log": each("residual_log", ints(0, 1048576)),
    "probe_log": each("probe_log", ints(0, 1048576)) + [["@probes", "25"], ["probe_log", "1048576"], ["@probes", "26"], ["probe_log", "0"],
                                                        ["@probes", "26"], ["probe_log", "1048576"], ["probe_log", "1048575"], ["@probes", "0"]],
    "image_log": each("image_log", ints(0, 65536)),
    "tracers": each("tracers", ints(0, 4194304)) + [["tracers", "0"], ["tracer_log", "10"], ["tracers", "3834792"], ["tracers", "3834793"],
                                                    ["tracers", "4194304"]],
    "tracer_log": each("tracer_log", ints(0, 65536)) + [["tracer_log", "0"], ["tracers", "585"], ["tracer_log", "65536"], ["tracers", "586"],
                                                        ["tracer_log", "65536"], ["tracer_log", "65535"]],
    "tracer_every": each("tracer_every", ints(1, 1 << 30)),
    "volume_log": each("volume_log", ints(0, 65536)),
    "monitor_log": each("monitor_log", ints(0, 1048576)),
    "monitor_every": each("monitor_every", ints(1, 1 << 30)),
    "monitor_stations": each("monitor_stations", ["", "1", "8", "0", "9", "1,2,3,4,5,6,7,8", "1,2,3,4,5,6,7,8,1", "1,", ",1", "1,,2", "1 ,2",
                                                  "1, 2", "+3,-0", "3,x", "3x", " ", "8,8,8", HUGE, "2"]),
    "vorticity_confinement": each("vorticity_confinement", reals(0)),
    "inflow": each("inflow", words("on", "off")),
    "inflow_eddies": each("inflow_eddies", ints(0, 65536)),
    "inflow_sigma": each("inflow_sigma", reals(1)),
    "inflow_rms": each("inflow_rms", reals(0)),
    "inflow_convect": each("inflow_convect", reals(0) + ["auto", "auto ", "AUTO", "aut"]),
    "inflow_seed": each("inflow_seed", ["0", "1", "18446744073709551615", "18446744073709551616", "-1", "-0", " -1", "+5", " 5", "0x10", "0X1f",
                                        "010", "08", "0x", "5 ", "5x", "", " ", "x", "1e3", HUGE]),
    "volume_every": each("volume_every", ints(1, 1 << 30)),
    "image_every": each("image_every", ints(1, 1 << 30)),
    "flow_stats": each("flow_stats", words("off", "mean", "moments")),
    "flow_stats_every": each("flow_stats_every", ints(1, 1 << 30)),
    "flow_stats_start": each("flow_stats_start", ints(0, 1 << 30)),
    "dump_async": each("dump_async", FLAG),
    "fuse_advect": each("fuse_advect", FLAG),
    "zero_start": each("zero_start", words("auto", "0", "1")),
    "fuse_project_advect": each("fuse_project_advect", words("auto", "0", "1")),
    "overlap": each("overlap", words("auto", "0", "1", "2", "3") + ["4", "-1", "3x", "03", " 1"]),
    "comm_cus": each("comm_cus", ["auto", "0", "128", "-1", "129", "-2", "auto ", "AUTO"] + ATOI),
    "split_density_solve": each("split_density_solve", FLAG),
    "debug_poison_gather": each("debug_poison_gather", FLAG),
    "sweep_ry": each("sweep_ry", ["2", "4", "1", "3", "5"] + ATOI),
    "sweep_zc": each("sweep_zc", ATOI),
    "sweep_blocks": each("sweep_blocks", ATOI),
    "sweep_abl": each("sweep_abl", ATOI),
    "sweep_fuse": each("sweep_fuse", ["1", "4", "0", "5"] + ATOI),
    "vortex_ry": each("vortex_ry", ["1", "2", "0", "3"] + ATOI),
    "project_kernels": each("project_kernels", words("march", "cell")),
    "advect_kernels": each("advect_kernels", words("cell", "celltab", "tile", "row")),
    "advect_window": each("advect_window", ["1", "128", "0", "129"] + ATOI),
    "wall_free": each("wall_free", words("0", "auto", "1")),
    "mask_free": each("mask_free", words("0", "auto", "1")),
    "chunk_cost": each("chunk_cost", ["0", "1,1,1", "1000000,1000000,1000000", "0,1,1", "1,0,1", "1,1,0", "1000001,1,1", "1,1000001,1",
                                      "1,1,1000001", "1,1", "1,1,1,1", "", "x", " 3, 2, 1", "00"]),
    "pair_zc": each("pair_zc", ATOI),
    "pair_shape": each("pair_shape", ATOI),
    "two_sweep_kernel": each("two_sweep_kernel", words("auto", "pair", "fused")),
    "no_such_option": each("no_such_option", ["0", "", "auto"]) + [["", "0"], ["Precision", "fp32"], ["force_log ", "1"]],
}

# option -> the calls put to a handle in use: the branches that look at the engine, with sizes a test can afford
IN_USE = {
    "precision": each("precision", ["fp32", "fp64", "x"]),
    "comm_cus": each("comm_cus", ["0", "auto", "x"]),
    "overlap": each("overlap", ["auto", "0", "3", "4", "x"]),
    "image_log": each("image_log", ["2", "0", "65537", "x", "3"]),
    "tracers": each("tracers", ["4", "x", "0", "-1", "16"]),
    "tracer_log": [["tracers", "4"]] + each("tracer_log", ["2", "x", "0", "65537", "3"]),
    "volume_log": each("volume_log", ["2", "0", "65537", "x", "3"]),
    "flow_stats": each("flow_stats", ["mean", "moments", "x", "off", "Mean"]),
    "force_log": each("force_log", ["2", "x", "0"]),
    "probe_log": [["@probes", "3"]] + each("probe_log", ["2", "x", "0"]),
    "monitor_log": each("monitor_log", ["2", "x", "0"]),
}


def main():
    lib_path = os.path.abspath(sys.argv[1])
    out_path = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "tests", "golden", "option_replies.json")
    os.environ["FLUIDSIM_LIB"] = lib_path
    from fluid_simulation_amd import _lib
    import option_replies as R

    L = _lib.lib()
    assert os.path.samefile(_lib.LIB_PATH, lib_path)
    options, errors = [], [""]
    for table, engine in ((FRESH, False), (IN_USE, True)):
        for name, script in table.items():
            options.append(R.pack(name, engine, script, R.run_script(L, script, engine), errors))
    logs = {log: R.run_log(L, log) for log in R.LOGS}
    head = {"about": "recorded by tools/record_option_replies.py; the format: pack() of tests/option_replies.py",
            "version": L.fs_version().decode(), "readback": R.READBACK}
    dumps = lambda v: json.dumps(v, separators=(",", ":"), sort_keys=True)
    with open(out_path, "w") as f:                         # one line per option, per error text and per log
        f.write("{" + dumps(head)[1:-1] + ',\n"errors":[\n' + ",\n".join(dumps(e) for e in errors) + '],\n"options":[\n')
        f.write(",\n".join(dumps(o) for o in options) + '],\n"logs":{\n')
        f.write(",\n".join("%s:%s" % (dumps(k), dumps(v)) for k, v in sorted(logs.items())) + "}}\n")
    with open(out_path) as f:
        assert json.load(f)["options"] == options
    print("%s: %d options, %d calls, %d logs, %d refusals" % (out_path, len(options), sum(len(o["calls"]) for o in options), len(logs),
                                                              sum(r[0] != 0 for o in options for r in o["replies"])))


if __name__ == "__main__":
    main()
