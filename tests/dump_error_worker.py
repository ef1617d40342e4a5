"""One run into dump files that cannot take the data, then one into a good directory on the same handle (spawned by
tests/test_gpu_boundary.py, which puts this process under a time limit: a failed write must not hang the step).
argv: W H D asynchronous full_dir good_dir result.json"""
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import boundary_model as M  # noqa: E402
import fluid_simulation_amd as F  # noqa: E402

STEPS = 3


def main():
    W, H, D, asynchronous = (int(v) for v in sys.argv[1:5])
    full, good, result = sys.argv[5:8]
    res = {}

    def build(**kw):
        sim = F.Simulation(W, H, D, STEPS, acc=2, quiet=1, **kw)
        sim.addObstacle(2, 2, 1)
        return sim

    sim = build(dump_every=1, dump_async=asynchronous, dump_dir=full)
    try:
        sim.run()
        res["first_run"] = "ok"
    except F.FluidsimError as e:
        res["first_run"], res["code"], res["message"] = "FluidsimError", e.code, str(e)
    # the twin starts from the state the failed run left, however many of its steps were made
    # (a step reads dens, obs and the velocities of the state before it and overwrites everything else)
    fields = (F.DENS, F.OBS, F.VX, F.VY, F.VZ)
    state = [sim.get(f) for f in fields]
    twin = build(dump_every=0)
    for f, a in zip(fields, state):
        twin.set(f, a)
    rec = []
    for _ in range(STEPS):
        twin.run_one()
        rec.append(M.frame_bytes([twin.get(f) for f in (F.DENS, F.OBS, F.VX, F.VY, F.VZ)]))
    twin.close()
    sim.set_option("dump_dir", good)
    try:
        sim.run()
        sim.sync()
        res["second_run"] = "ok"
    except F.FluidsimError as e:
        res["second_run"], res["second_message"] = "FluidsimError", str(e)
    sim.close()
    want = [b"".join(r[k] for r in rec) for k in range(5)]
    got = []
    for n in M.FILES:
        path = os.path.join(good, n + ".bin")
        got.append(open(path, "rb").read() if os.path.exists(path) else b"")
    res["frames_equal"] = bool(got == want)
    res["bytes"] = len(got[0])
    res["moved"] = bool(np.frombuffer(want[2], dtype=np.float32).any())
    with open(result, "w") as f:
        json.dump(res, f)


if __name__ == "__main__":
    main()
