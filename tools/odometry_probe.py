#!/usr/bin/env python
"""Times of RGB-D odometry on one MI355X, for profiles/odometry_probe.txt: a 640 x 480 frame pair of tests/odometry_scene.py,
  * the whole visma_icp_rgbd_odometry with the default schedule {20, 10, 5} (upload, both pyramids, 35 iterations, the
    information matrix), hybrid and colour term;
  * per stage on the resident pyramids: the prepare, one step (correspondence kernel + reduction + the wait for its
    statistics) on every level, the correspondences of level 0 with their read-back, the information matrix.
A step is two launches and one host turn-around, so its time at the coarse levels is the launch and wait overhead: the
numbers say whether fusing the two kernels or solving on the device could pay.
tests/golden/gen_odometry.py --time times the compiled reference on the same frames.  The measurement runs in a child
process under its own time limit; one warm-up call, then the median and the spread of --reps calls."""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

W, H = 640, 480


def spread(t):
    t = np.array(t[1:]) * 1e3
    return dict(median_ms=float(np.median(t)), min_ms=float(t.min()), max_ms=float(t.max()))


def timed(fn, reps):
    t, out = [], None
    for _ in range(reps + 1):
        t0 = time.perf_counter()
        out = fn()
        t.append(time.perf_counter() - t0)
    return spread(t), out


def child(reps):
    import odometry_scene as scene
    from visma_amd import _lib
    fr = scene.frames(W, H)
    ctx = _lib.Context(0)
    out = {"case": "%d x %d, schedule [20, 10, 5]" % (W, H), "reps": reps}
    for name, method in (("hybrid", _lib.ODOMETRY_HYBRID), ("colour", _lib.ODOMETRY_COLOR)):
        t, r = timed(lambda: ctx.rgbd_odometry(*fr, None, method), reps)
        out["rgbd_odometry_" + name] = dict(t, success=bool(r.success), iterations=len(r.pairs), information_pairs=r.information_pairs,
                                            pose_error=float(np.linalg.norm(r.T - scene.truth())))
    out["prepare"], _ = timed(lambda: ctx.odometry_prepare(*fr), reps)
    T = scene.truth()
    for level in (2, 1, 0):
        out["step_level_%d" % level], s = timed(lambda: ctx.odometry_step(level, T, _lib.ODOMETRY_HYBRID), 4 * reps)
        out["step_level_%d" % level]["pairs"] = s[1]
    out["correspondences_level_0_with_readback"], _ = timed(lambda: ctx.odometry_correspondences(0, T), reps)
    out["information"], _ = timed(lambda: ctx.odometry_information(T), reps)
    ctx.close()
    print("RESULT " + json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "odometry_probe.txt"))
    a = ap.parse_args()
    if a.child:
        return child(a.reps)
    p = subprocess.run(["timeout", "-k", "10", "240", sys.executable, os.path.abspath(__file__), "--child", "--reps", str(a.reps)],
                       capture_output=True, text=True)
    if p.returncode != 0:
        print("exit %d\n%s" % (p.returncode, p.stderr[-2000:]))
        return 1
    lines = [ln[7:] for ln in p.stdout.splitlines() if ln.startswith("RESULT ")]
    res = json.loads(lines[-1])
    text = ["# tools/odometry_probe.py: %s, median of %d calls after one warm-up (min .. max), wall clock of the Python call" % (res["case"], res["reps"])]
    for k, v in res.items():
        if isinstance(v, dict):
            extra = ", ".join("%s %s" % (a, b) for a, b in v.items() if not a.endswith("_ms"))
            text.append("%-40s %9.3f ms (%.3f .. %.3f)%s" % (k, v["median_ms"], v["min_ms"], v["max_ms"], "  " + extra if extra else ""))
    text.append(lines[-1])
    print("\n".join(text))
    with open(a.out, "w") as f:
        f.write("\n".join(text) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
