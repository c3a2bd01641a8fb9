#!/usr/bin/env python
"""Times of the resident PointCloud on one MI355X, for profiles/cloud_probe.txt, on the clouds of two workloads (a 640 x 480
RGB8 frame of tests/tsdf_scene.py into a uniform 512^3 volume, and into a scalable volume at Open3D's pipeline settings: voxel
4 / 512 m, sdf_trunc 0.04, units of 16, stride 4).

Two chains over the cloud the volume extracted, alternated in one process, step by step:
  device    point_cloud() (visma_icp_cloud_from_tsdf: device to device), crop, voxel_down_sample, estimate_normals(Hybrid), get
  download  the read-back (visma_icp_tsdf_get_point_cloud), then the host-array entry points: a numpy crop,
            Context.voxel_down_sample, Context.estimate_normals
Both end in the same bytes (asserted).  Then every new operation alone on the whole cloud.  Every timed call ends with the
device idle (each entry point synchronises its stream before it returns), so the host clock around it is the call's time,
read-backs and the host's allocations included.  For the streaming operations the bytes the kernels must move, over that
WHOLE-CALL time, are given as a share of the 8 TB/s peak: a lower bound of what the kernels reach, launch and wait included.
Each workload runs in a child process of its own under its own time limit; one warm-up round, then the median and the spread
(min .. max) of --reps rounds (default 20).  --save-cloud DIR keeps each cloud and the chain's arguments as
DIR/cloud_probe_<workload>.npz: tests/golden/gen_cloud.py --time <that file> times the compiled reference (one CPU thread) on
the same chain; pass what it printed with --reference to have it recorded beside."""
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
VOXEL, RADIUS, MAX_NN = 2.0 * LENGTH / R, 6.0 * LENGTH / R, 30
PEAK = 8.0e12


def spread(t):
    t = np.array(t[1:]) * 1e3
    return dict(median_ms=float(np.median(t)), min_ms=float(t.min()), max_ms=float(t.max()))


def child(which, reps, resolution, save):
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
    n = len(vol.extract_point_cloud()[0])
    L, h, v = ctx.L, ctx._h, vol._v
    times = {}

    def clock(name, fn):
        t0 = time.perf_counter()
        r = fn()
        times.setdefault(name, []).append(time.perf_counter() - t0)
        return r

    def read_back():
        pts, nrm, col = np.empty((n, 3)), np.empty((n, 3)), np.empty((n, 3))
        ctx._chk(L.visma_icp_tsdf_get_point_cloud(h, v, _lib._p(pts, _lib._dp), _lib._p(nrm, _lib._dp), _lib._p(col, _lib._dp), n))
        return pts, nrm, col

    with vol.point_cloud() as whole:
        lo, hi = whole.bounds()
    lo, hi = lo + 0.15 * (hi - lo), hi - 0.15 * (hi - lo)
    for _ in range(reps + 1):
        c = clock("device: from_tsdf", vol.point_cloud)
        cropped = clock("device: crop", lambda: c.crop(lo, hi))
        down = clock("device: voxel_down_sample", lambda: cropped.voxel_down_sample(VOXEL))
        clock("device: estimate_normals", lambda: down.estimate_normals(knn=MAX_NN, radius=RADIUS))
        a = clock("device: get", down.get)
        kept = len(cropped)
        for x in (c, cropped, down):
            x.close()
        pts, nrm, col = clock("download: read-back", read_back)

        def host_crop():
            m = ((pts >= lo) & (pts <= hi)).all(axis=1)
            return pts[m], nrm[m], col[m]
        cp, cn, cc = clock("download: crop on the host (numpy)", host_crop)
        dp, dn, dc = clock("download: voxel_down_sample", lambda: ctx.voxel_down_sample(cp, VOXEL, normals=cn, colors=cc))
        dn = clock("download: estimate_normals", lambda: ctx.estimate_normals(dp, knn=MAX_NN, radius=RADIUS, normals=dn))
        for got, want in ((a["points"], dp), (a["normals"], dn), (a["colors"], dc)):
            assert got.tobytes() == want.tobytes()
    out.update(points=n, cropped=kept, down_sampled=len(dp))

    # every new operation alone, on the whole cloud; bytes: what its kernels must read and write
    rows = 24 * n
    T = np.eye(4); T[:3, 3] = (0.1, -0.2, 0.3); T[0, 1], T[1, 0] = -0.01, 0.01
    reverse = np.arange(n, dtype=np.int64)[::-1].copy()
    moved = {"transform": 4 * rows, "normalize_normals": 2 * rows, "paint_uniform_color": rows, "bounds": rows, "crop": 3 * rows + 6 * rows * kept // n,
             "uniform_down_sample (k = 7)": 3 * rows // 7 * 2, "select (reversed)": 6 * rows + 8 * n, "append (a copy)": 12 * rows,
             "orient_normals_to_align_with_direction": 2 * rows, "orient_normals_towards_camera_location": 3 * rows,
             "mean_and_covariance": rows, "mahalanobis_distance": 2 * rows + 8 * n}
    c = vol.point_cloud()
    for _ in range(reps + 1):
        clock("transform", lambda: c.transform(T))
        clock("normalize_normals", c.normalize_normals)
        clock("bounds", c.bounds)
        clock("crop", lambda: c.crop(lo, hi)).close()
        clock("uniform_down_sample (k = 7)", lambda: c.uniform_down_sample(7)).close()
        clock("select (reversed)", lambda: c.select(reverse)).close()
        clock("voxel_down_sample", lambda: c.voxel_down_sample(VOXEL)).close()
        clock("orient_normals_to_align_with_direction", lambda: c.orient_normals_to_align_with_direction((0.0, 0.0, 1.0)))
        clock("orient_normals_towards_camera_location", lambda: c.orient_normals_towards_camera_location((0.0, 0.0, -2.0)))
        clock("mean_and_covariance", c.mean_and_covariance)
        clock("mahalanobis_distance", c.mahalanobis_distance)
        with c.uniform_down_sample(1) as copy:
            clock("append (a copy)", lambda: copy.append(c))
        with c.uniform_down_sample(1) as copy:
            clock("paint_uniform_color", lambda: copy.paint_uniform_color((0.5, 0.25, 0.125)))
        clock("get", c.get)
    c.close()
    if save:
        os.makedirs(save, exist_ok=True)
        np.savez_compressed(os.path.join(save, "cloud_probe_%s.npz" % which), points=pts, normals=nrm, colors=col, lo=lo, hi=hi, voxel=VOXEL,
                            radius=RADIUS, max_nn=MAX_NN)
    steps = {name: spread(t) for name, t in times.items()}
    for name, b in moved.items():
        steps[name]["share_of_peak_over_the_whole_call"] = b / (steps[name]["median_ms"] * 1e-3) / PEAK
    out["steps"] = steps
    vol.close()
    ctx.close()
    print("RESULT " + json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--resolution", type=int, default=R)
    ap.add_argument("--child", default="")
    ap.add_argument("--save-cloud", default="")
    ap.add_argument("--reference", default="", help="what tests/golden/gen_cloud.py --time printed, recorded as it is")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cloud_probe.txt"))
    a = ap.parse_args()
    if a.child:
        return child(a.child, a.reps, a.resolution, a.save_cloud)
    text = ["# tools/cloud_probe.py: median of %d rounds after one warm-up (min .. max), host clock around calls that end with the device idle" % a.reps,
            "# share: the bytes the operation's kernels must move over the WHOLE CALL's time, as a share of the 8 TB/s peak (a lower bound of the kernels')"]
    for which in ("uniform", "scalable"):
        p = subprocess.run(["timeout", "-k", "10", "300", sys.executable, os.path.abspath(__file__), "--child", which, "--reps", str(a.reps),
                            "--resolution", str(a.resolution), "--save-cloud", a.save_cloud], capture_output=True, text=True)
        if p.returncode != 0:                            # nothing more is started on the device after a step that failed
            print("%s: exit %d\n%s" % (which, p.returncode, p.stderr[-2000:]))
            return 1
        lines = [ln[7:] for ln in p.stdout.splitlines() if ln.startswith("RESULT ")]
        res = json.loads(lines[-1])
        text.append("## %s: %d points, cropped to %d, down-sampled to %d" % (res["case"], res["points"], res["cropped"], res["down_sampled"]))
        for name, s in res["steps"].items():
            share = "   %.2f %% of peak" % (100.0 * s["share_of_peak_over_the_whole_call"]) if "share_of_peak_over_the_whole_call" in s else ""
            text.append("%-46s %9.3f ms (%.3f .. %.3f)%s" % (name, s["median_ms"], s["min_ms"], s["max_ms"], share))
        for chain in ("device", "download"):
            text.append("%-46s %9.3f ms (sum of the medians)" % (chain + ": whole chain", sum(s["median_ms"] for n, s in res["steps"].items() if n.startswith(chain + ":"))))
        text.append(lines[-1])
    if a.reference:
        text.append("## the compiled reference (tests/golden/gen_cloud.py --time; one thread of a CPU that is not the MI355X's host)")
        text.append(a.reference)
    print("\n".join(text))
    with open(a.out, "w") as f:
        f.write("\n".join(text) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
