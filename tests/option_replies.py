"""What tests/test_gpu_options.py and tools/record_option_replies.py share: how a script of fs_set_option calls and the
fetch calls of the eight per-step logs are put to a library (a ctypes handle with the signatures of
fluid_simulation_amd._lib) and what of each reply is kept.  The scripts themselves live in the fixture
(tests/golden/option_replies.json); the tool that writes it holds the table they come from."""
import ctypes as C

import numpy as np

W, H, D = 8, 6, 5
# members fs_get_int reads back after every fs_set_option call
READBACK = ["monitor_log", "monitor_every", "monitor_stations", "inflow", "inflow_eddies", "tracer_capacity",
            "image_frame_bytes", "volume_frame_bytes", "probe_count"]
LOGS = ["force", "body_force", "residual", "probe", "monitor", "image", "volume", "tracer"]
# doubles per row of the logs that come as rows; the step is column 0
ROW_COLS = {"force": 9, "body_force": 16, "residual": 31, "probe": 1 + 2 * 5, "monitor": 57}
TRACER_SLOTS = 4


def create(L):
    h = L.fs_create(W, H, D, 1, 1, 0.05, 2.0e-5, 1.5e-5, 1)
    assert h, L.fs_last_error()
    for key in (b"quiet", b"dump_every"):
        assert L.fs_set_option(h, key, b"1" if key == b"quiet" else b"0") == 0
    return h


def error_text(L, rc):
    return (L.fs_last_error() or b"").decode() if rc else ""


def set_probes(L, h, n):
    """n probes along x, inside the box"""
    cells = np.array([(1 + k % W, 1 + (k // W) % H, 1 + (k // (W * H)) % D) for k in range(n)], dtype=np.intc).reshape(-1, 3)
    return L.fs_set_probes(h, cells.ctypes.data_as(C.c_void_p), n)


def run_script(L, script, engine):
    """`script`: [key, value] pairs put to one new handle in turn; the key "@probes" sets that many probes instead.
    `engine`: the handle is in use (its engine exists) before the first call.  One reply per call: the return code, the
    error text of a refusal, and the READBACK members after it, in READBACK's order."""
    h = create(L)
    replies = []
    try:
        if engine:
            assert L.fs_field_stats(h, 0, None, None, None) == 0, L.fs_last_error()
        for key, value in script:
            if key == "@probes":
                rc = set_probes(L, h, int(value))
            else:
                rc = L.fs_set_option(h, key.encode(), value.encode())
            reply = {"rc": rc, "err": error_text(L, rc), "ints": []}
            for name in READBACK:
                out = C.c_int(-12345)
                assert L.fs_get_int(h, name.encode(), C.byref(out)) == 0, name
                reply["ints"].append(out.value)
            replies.append(reply)
    finally:
        L.fs_destroy(h)
    return replies


def pack(name, engine, script, replies, errors):
    """One option's script and replies as the fixture keeps them, short: a call is its value alone where its key is the
    option's name, else [key, value]; a reply is [return code, index of the error text in `errors` (-1: none)], with the
    READBACK members appended where they differ from the reply before (the first reply has them)."""
    calls, packed, last = [], [], None
    for (key, value), r in zip(script, replies):
        calls.append(value if key == name else [key, value])
        if r["err"] not in errors:
            errors.append(r["err"])
        packed.append([r["rc"], errors.index(r["err"]) if r["rc"] else -1] + ([r["ints"]] if r["ints"] != last else []))
        last = r["ints"]
    return {"name": name, "engine": engine, "calls": calls, "replies": packed}


def unpack(opt, errors):
    """-> (script, replies) as run_script takes and returns them"""
    script = [[opt["name"], c] if isinstance(c, str) else list(c) for c in opt["calls"]]
    replies, last = [], None
    for r in opt["replies"]:
        last = r[2] if len(r) > 2 else last
        replies.append({"rc": r[0], "err": errors[r[1]] if r[1] >= 0 else "", "ints": last})
    return script, replies


def _fill(L, h, log):
    """capacity 2 and two records of `log` on the new handle `h`; returns the bytes of one frame (image and volume logs)"""
    def opt(key, value):
        assert L.fs_set_option(h, key.encode(), str(value).encode()) == 0, L.fs_last_error()

    def twice(entry):
        for _ in range(2):
            assert getattr(L, entry)(h) == 0, L.fs_last_error()

    if log in ("force", "body_force", "residual"):
        opt(log + "_log", 2)
        assert L.fs_add_obstacle(h, 4, 3, 3) == 0, L.fs_last_error()
        twice("fs_step")
    elif log == "probe":
        assert set_probes(L, h, 2) == 0, L.fs_last_error()
        opt("probe_log", 2)
        twice("fs_probe_sample")
    elif log == "monitor":
        opt("monitor_log", 2)
        twice("fs_monitor_sample")
    elif log == "image":
        spec = np.array([0, 0, 2, 3], dtype=np.intc)                       # density, a slice, across z, at z = 3
        rng = np.array([0.0, 1.0, 0.5])
        assert L.fs_image_views(h, spec.ctypes.data_as(C.c_void_p), rng.ctypes.data_as(C.c_void_p), 1) == 0, L.fs_last_error()
        opt("image_log", 2)
        twice("fs_image_sample")
    elif log == "volume":
        cam = np.array([-10.0, 3.5, 3.0, 4.5, 3.5, 3.0, 0.0, 1.0, 0.0, 4.0, 1.0])   # looks along x, orthographic
        assert L.fs_volume_camera(h, 0, cam.ctypes.data_as(C.c_void_p), 3, 2) == 0, L.fs_last_error()
        spec = np.array([0, 0], dtype=np.intc)
        par = np.array([0.0, 1.0, 1.0, 0.5, 0.0, 128.0, 128.0, 128.0, 0.0, 0.0, 0.0])
        assert L.fs_volume_views(h, spec.ctypes.data_as(C.c_void_p), par.ctypes.data_as(C.c_void_p), 1) == 0, L.fs_last_error()
        opt("volume_log", 2)
        twice("fs_volume_sample")
    else:
        opt("tracers", TRACER_SLOTS)
        opt("tracer_log", 2)
        xyz = np.array([1.5, 1.5, 1.5, 2.0, 3.0, 2.5])
        assert L.fs_tracer_seed(h, xyz.ctypes.data_as(C.c_void_p), 2) == 0, L.fs_last_error()
        twice("fs_tracer_advance")
    if log in ("image", "volume"):
        out = C.c_int(0)
        assert L.fs_get_int(h, (log + "_frame_bytes").encode(), C.byref(out)) == 0 and out.value > 0
        return out.value
    return 0


def _fetch(L, h, log, room, data, frame_bytes):
    """one call of the log's fetch entry with room for `room` units (`data` false: the sizes-only form) -> a reply: return
    code, error text, both counts, and the steps of what came back"""
    n, dropped = C.c_long(-1), C.c_long(-1)
    units = max(room, 0) + 8                                               # the arrays hold more than the call is told
    steps = np.full(units, -1, dtype=np.int64)
    entry = getattr(L, "fs_%s_log" % log)
    if log in ROW_COLS:
        rows = np.full((units, ROW_COLS[log]), -1.0)
        rc = entry(h, rows.ctypes.data_as(C.c_void_p) if data else None, room, C.byref(n), C.byref(dropped))
        steps = rows[:, 0].astype(np.int64)
    elif log == "tracer":
        xyz, status = np.zeros((units, TRACER_SLOTS, 3)), np.zeros((units, TRACER_SLOTS), dtype=np.int32)
        rc = entry(h, xyz.ctypes.data_as(C.c_void_p) if data else None, status.ctypes.data_as(C.c_void_p) if data else None,
                   steps.ctypes.data_as(C.c_void_p), room, C.byref(n), C.byref(dropped))
    else:
        frames = np.zeros(units * frame_bytes, dtype=np.uint8)
        rc = entry(h, frames.ctypes.data_as(C.c_void_p) if data else None, steps.ctypes.data_as(C.c_void_p), room,
                   C.byref(n), C.byref(dropped))
    got = n.value if rc == 0 and data and n.value > 0 else 0
    return {"room": room, "data": bool(data), "rc": rc, "err": error_text(L, rc), "n": n.value, "dropped": dropped.value,
            "steps": [int(v) for v in steps[:got]]}


def run_log(L, log):
    """The replies of one log at capacity 2 holding two records: the sizes-only call, the fetch with room for 1, with room
    for 2, and with room for all (the body-force log returns a row per body and step), then, the log drained: the sizes,
    a fetch with room for 2 and one with room for -1."""
    h = create(L)
    try:
        frame_bytes = _fill(L, h, log)
        replies = [_fetch(L, h, log, 0, False, frame_bytes), _fetch(L, h, log, 1, True, frame_bytes),
                   _fetch(L, h, log, 2, True, frame_bytes)]
        if replies[-1]["rc"]:
            replies.append(_fetch(L, h, log, replies[0]["n"], True, frame_bytes))
        replies += [_fetch(L, h, log, 0, False, frame_bytes), _fetch(L, h, log, 2, True, frame_bytes),
                    _fetch(L, h, log, -1, True, frame_bytes)]
    finally:
        L.fs_destroy(h)
    return replies
