#!/usr/bin/env python
"""Times of ExtractTriangleMesh on one MI355X, for profiles/tsdf_mesh_probe.txt, on the two workloads of tools/tsdf_probe.py:
a 640 x 480 RGB8 frame of tests/tsdf_scene.py into
  * a uniform 512^3 volume (length 4 m, sdf_trunc 0.04, origin (-2, -2, -2): Open3D's pipeline voxel of 4 / 512 m);
  * a scalable volume at Open3D's pipeline settings (voxel 4 / 512 m, sdf_trunc 0.04, units of 16, stride 4).
Beside each it times ExtractPointCloud on the SAME volume: that extraction is the yardstick (one ordered compaction with
normals; the mesh is a cube pass and two ordered compactions).  The times are the wall clock of the Python call (each ends
with the device idle) and include the read-back of the rows and the host's allocation of the result arrays; the spread
(min .. max) is printed beside every median and belongs to it.  tests/golden/gen_tsdf_mesh.py --time times the compiled
reference (one CPU thread) on the same inputs; pass what it printed with --reference to have it recorded beside.
Each workload runs in a child process of its own under its own time limit; one warm-up call, then the median and the
spread of --reps calls (default 20)."""
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


def child(which, reps, resolution):
    import tsdf_scene as scene
    from visma_amd import _lib
    frames, k = scene.frames(W, H, 1)
    depth, rgb, gray, E = frames[0]
    ctx = _lib.Context(0)
    if which == "uniform":
        vol = ctx.tsdf_uniform(LENGTH, resolution, TRUNC, _lib.TSDF_COLOR_RGB8, ORIGIN)
        out = {"case": "%d x %d RGB8 into a uniform %d^3 volume" % (W, H, resolution)}
    else:
        vol = ctx.tsdf_scalable(LENGTH / R, TRUNC, _lib.TSDF_COLOR_RGB8, 16, 4)
        out = {"case": "%d x %d RGB8 into a scalable volume, voxel 4 / 512 m, units of 16, stride 4" % (W, H)}
    vol.integrate(depth, rgb, k, E)
    if which == "scalable":
        out["units"] = len(vol.units())
    t, pc = timed(vol.extract_point_cloud, reps)
    out["extract_point_cloud"] = dict(t, points=len(pc[0]))
    t, mesh = timed(vol.extract_triangle_mesh, reps)
    out["extract_triangle_mesh"] = dict(t, vertices=len(mesh[0]), triangles=len(mesh[2]))
    vol.close()
    ctx.close()
    print("RESULT " + json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--resolution", type=int, default=R)
    ap.add_argument("--child", default="")
    ap.add_argument("--reference", default="", help="what tests/golden/gen_tsdf_mesh.py --time printed, recorded as it is")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tsdf_mesh_probe.txt"))
    a = ap.parse_args()
    if a.child:
        return child(a.child, a.reps, a.resolution)
    text = ["# tools/tsdf_mesh_probe.py: median of %d calls after one warm-up (min .. max), wall clock of the Python call" % a.reps]
    for which in ("uniform", "scalable"):
        p = subprocess.run(["timeout", "-k", "10", "300", sys.executable, os.path.abspath(__file__), "--child", which, "--reps", str(a.reps),
                            "--resolution", str(a.resolution)], capture_output=True, text=True)
        if p.returncode != 0:                            # nothing more is started on the device after a step that failed
            print("%s: exit %d\n%s" % (which, p.returncode, p.stderr[-2000:]))
            return 1
        lines = [ln[7:] for ln in p.stdout.splitlines() if ln.startswith("RESULT ")]
        res = json.loads(lines[-1])
        text.append("## " + res["case"] + (" (%d units)" % res["units"] if "units" in res else ""))
        for k, v in res.items():
            if isinstance(v, dict):
                extra = ", ".join("%s %s" % (x, y) for x, y in v.items() if not x.endswith("_ms"))
                text.append("%-24s %9.3f ms (%.3f .. %.3f)  %s" % (k, v["median_ms"], v["min_ms"], v["max_ms"], extra))
        text.append(lines[-1])
    if a.reference:
        text.append("## the compiled reference (tests/golden/gen_tsdf_mesh.py --time)")
        text.append(a.reference)
    print("\n".join(text))
    with open(a.out, "w") as f:
        f.write("\n".join(text) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
