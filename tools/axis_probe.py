"""C3's 288 problems (bench.c3_problems: 12 objects x 24 yaw starts) for 30 fixed iterations through
visma_icp_run_batch_multi (2 worker contexts on one GPU), unconstrained and with the rotation about +Y only
(visma_icp_set_rotation_axis): iterations per second, persistent sweep launches, the largest tilt of each result set.

    python tools/axis_probe.py [--reps 5] [--workers 2] [--out file.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402
from visma_amd import _lib  # noqa: E402

Y = np.array([0.0, 1.0, 0.0])


def tilt_deg(T):
    v = np.asarray(T)[:3, :3].T @ Y
    return float(np.degrees(np.arccos(np.clip(v @ Y, -1.0, 1.0))))


def measure(axis, batch, n, reps, workers):
    ctxs = [_lib.Context(0) for _ in range(workers)]
    for c in ctxs:
        c.set_rotation_axis(axis)
    # fixed work: 30 iterations of every problem (no stop test)
    _lib.run_batch_multi(ctxs, batch, 30, -1.0, -1.0)                          # warm-up
    times = []
    for _ in range(reps):
        t0 = time.perf_counter()
        res = _lib.run_batch_multi(ctxs, batch, 30, -1.0, -1.0)
        times.append(time.perf_counter() - t0)
    info = [c.sweep_info() for c in ctxs]
    for c in ctxs:
        c.close()
    iters = sum(r.iterations for r in res)
    med = float(np.median(times))
    return {"axis": None if axis is None else list(map(float, axis)), "seconds_median": med,
            "seconds_all": times, "iterations": iters, "iterations_per_s": iters / med,
            "sweep_launches": sum(i["launches"] for i in info), "sweep_aborts": sum(i["aborts"] for i in info),
            "max_tilt_deg": max(tilt_deg(r.transformation_) for r in res), "n": n}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--workers", type=int, default=2)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    _, probs = bench.c3_problems()
    plist = [p[:4] for p in probs]
    batch = _lib.Context.make_batch(plist)
    out = {"unconstrained": measure(None, batch, len(plist), a.reps, a.workers),
           "axis_y": measure(Y, batch, len(plist), a.reps, a.workers)}
    # (the two orders alternate once more: drift of the device's clocks shows as a difference between the repeats)
    out["unconstrained_again"] = measure(None, batch, len(plist), a.reps, a.workers)
    out["axis_y_again"] = measure(Y, batch, len(plist), a.reps, a.workers)
    u = 0.5 * (out["unconstrained"]["seconds_median"] + out["unconstrained_again"]["seconds_median"])
    c = 0.5 * (out["axis_y"]["seconds_median"] + out["axis_y_again"]["seconds_median"])
    out["constrained_over_unconstrained_time"] = c / u
    print(json.dumps(out, indent=1))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
