#!/usr/bin/env python
"""Times of TSDF integration on one MI355X, for profiles/tsdf_probe.txt: a 640 x 480 RGB8 frame of tests/tsdf_scene.py into
a uniform 512^3 volume (length 4 m, sdf_trunc 0.04, origin (-2, -2, -2): Open3D's pipeline voxel of 4 / 512 m),
  * Integrate: the whole call (the frame's upload, the kernel, the wait for it);
  * ExtractPointCloud and ExtractVoxelPointCloud: count, scan and write passes and the read-back of the rows.
For the integrate it prints the bytes the voxels' updates must move -- every voxel's tsdf, weight and three colour floats
read once (20 B), those of the voxels the frame changes written once (20 B) -- over the call's time, as a share of the
8 TB/s peak of the HBM: an end-to-end rate of the call, not the kernel's own.
  * Integrate of the same frame into a scalable volume at Open3D's pipeline settings (voxel 4 / 512 m, sdf_trunc 0.04,
    units of 16, stride 4): the first frame, which opens every unit it touches, and a repeated frame, which opens none;
    and ExtractPointCloud of that volume.
The times are the wall clock of the Python call (each ends with the device idle) and include the host's allocation of the
result arrays; the spread (min .. max) is printed beside every median and belongs to it.
tests/golden/gen_tsdf.py --time times the compiled reference on the same input.  The measurement runs in a child process
under its own time limit; one warm-up call, then the median and the spread of --reps calls (default 20)."""
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
R, LENGTH, TRUNC, ORIGIN = 512, 4.0, 0.04, (-2.0, -2.0, -2.0)
PEAK_BYTES_PER_S = 8e12


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


def child(reps, resolution):
    import ctypes as C

    import tsdf_scene as scene
    from visma_amd import _lib
    frames, k = scene.frames(W, H, 1)
    depth, rgb, gray, E = frames[0]
    ctx = _lib.Context(0)
    vol = ctx.tsdf_uniform(LENGTH, resolution, TRUNC, _lib.TSDF_COLOR_RGB8, ORIGIN)
    out = {"case": "%d x %d RGB8 into a uniform %d^3 volume" % (W, H, resolution), "reps": reps}
    vol.integrate(depth, rgb, k, E)
    weight = np.empty(resolution ** 3, np.float32)
    ctx._chk(ctx.L.visma_icp_tsdf_get_volume(ctx._h, vol._v, None, None, weight.ctypes.data_as(C.POINTER(C.c_float)), None))
    changed = int(np.count_nonzero(weight))
    t, _ = timed(lambda: vol.integrate(depth, rgb, k, E), reps)
    moved = 20 * resolution ** 3 + 20 * changed
    out["integrate_uniform"] = dict(t, voxels=resolution ** 3, changed=changed, bytes=moved,
                                    share_of_8TBps=moved / (t["median_ms"] * 1e-3) / PEAK_BYTES_PER_S)
    t, pc = timed(vol.extract_point_cloud, reps)
    out["extract_point_cloud"] = dict(t, points=len(pc[0]))
    t, vx = timed(vol.extract_voxel_point_cloud, reps)
    out["extract_voxel_point_cloud"] = dict(t, points=len(vx[0]))
    vol.close()
    sv = ctx.tsdf_scalable(LENGTH / R, TRUNC, _lib.TSDF_COLOR_RGB8, 16, 4)
    first = []
    for _ in range(3):                                   # the first frame into an empty volume: every touched unit is opened
        sv.reset()
        t0 = time.perf_counter()
        sv.integrate(depth, rgb, k, E)
        first.append(time.perf_counter() - t0)
    first = np.array(first) * 1e3
    out["integrate_scalable_first_frame"] = dict(median_ms=float(np.median(first)), min_ms=float(first.min()), max_ms=float(first.max()),
                                                 units=len(sv.units()))
    t, _ = timed(lambda: sv.integrate(depth, rgb, k, E), reps)
    out["integrate_scalable"] = dict(t, units=len(sv.units()), voxels=len(sv.units()) * 16 ** 3)
    t, pc = timed(sv.extract_point_cloud, reps)
    out["extract_point_cloud_scalable"] = dict(t, points=len(pc[0]))
    sv.close()
    ctx.close()
    print("RESULT " + json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--resolution", type=int, default=R)
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tsdf_probe.txt"))
    a = ap.parse_args()
    if a.child:
        return child(a.reps, a.resolution)
    p = subprocess.run(["timeout", "-k", "10", "300", sys.executable, os.path.abspath(__file__), "--child", "--reps", str(a.reps),
                        "--resolution", str(a.resolution)], capture_output=True, text=True)
    if p.returncode != 0:
        print("exit %d\n%s" % (p.returncode, p.stderr[-2000:]))
        return 1
    lines = [ln[7:] for ln in p.stdout.splitlines() if ln.startswith("RESULT ")]
    res = json.loads(lines[-1])
    text = ["# tools/tsdf_probe.py: %s, median of %d calls after one warm-up (min .. max), wall clock of the Python call" % (res["case"], res["reps"])]
    for k, v in res.items():
        if isinstance(v, dict):
            extra = ", ".join("%s %s" % (a, ("%.4f" % b) if isinstance(b, float) else b) for a, b in v.items() if not a.endswith("_ms"))
            text.append("%-32s %9.3f ms (%.3f .. %.3f)%s" % (k, v["median_ms"], v["min_ms"], v["max_ms"], "  " + extra if extra else ""))
    text.append(lines[-1])
    print("\n".join(text))
    with open(a.out, "w") as f:
        f.write("\n".join(text) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
