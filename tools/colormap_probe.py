#!/usr/bin/env python
"""Times of color map optimization on one MI355X, for profiles/colormap_probe.txt: 50 cameras of 640 x 480, ray-cast from the
scene of tests/colormap_scene.py with extrinsics about 0.3 degrees and 3 mm off, and 1,000,000 vertices on its surfaces;
Open3D's default option.
  * prepare: images, masks, visibility (one-time);
  * sums: the iteration kernel over every camera and the read-back of the 50 rows, the proxies being valid: the launch, the
    kernel and one wait.  Beside it the bytes the kernel must read -- per visible (camera, vertex) pair the vertex (24 B),
    four texels (64 B) and its list entry (4 B) -- over that call's time: an end-to-end rate of the call, which bounds the
    kernel's own from below;
  * proxy: the poses' upload and the proxy kernel;
  * proxy+sums: the device side of one iteration in one call (the poses' upload, both kernels, the read-back, one wait);
  * step: one whole iteration = that + the 50 solves and pose updates on the host; host_solve_ms_per_iteration is the
    step's median less the median of proxy+sums: what the host's arithmetic adds;
  * run300: a whole 300-iteration run from the perturbed poses (Open3D's maximum_iteration).
The times are the wall clock of the Python call (each ends with the device idle); the spread (min .. max) is printed
beside every median and belongs to it.  tests/golden/gen_colormap.py --time times the compiled reference on the same
input.  The measurement runs in a child process under its own time limit; one warm-up call, then the median and the spread
of --reps calls (default 20)."""
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

W, H, N_CAMERAS, N_VERTICES = 640, 480, 50, 1000000
PEAK_BYTES_PER_S = 8e12


def workload(n_cameras=N_CAMERAS, w=W, h=H, n_vertices=N_VERTICES):
    """-> depths, colors, the perturbed extrinsics, intrinsic, vertices"""
    import colormap_scene as scene
    poses = [scene.camera_to_world(i % 5) @ scene.rigid((0.0, 0.004 * (i // 5), 0.0), (0.01 * (i // 5), -0.005 * (i // 5), 0.0))
             for i in range(n_cameras)]
    frames = [scene.render_from(C, i % 6, w, h) for i, C in enumerate(poses)]
    E = np.stack([scene.rigid(*scene._ERRORS[i % 6]) @ scene.invert_rigid(C) for i, C in enumerate(poses)])
    V = scene.vertices(n_wall=int(0.6 * n_vertices), n_floor=int(0.2 * n_vertices), n_sphere=n_vertices - int(0.6 * n_vertices) - int(0.2 * n_vertices) - 1)
    return np.stack([f[0] for f in frames]), np.stack([f[1] for f in frames]), E, scene.intrinsic(w, h), V


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


def child(reps, n_cameras, n_vertices):
    from visma_amd import _lib
    depths, colors, E, K, V = workload(n_cameras, W, H, n_vertices)
    ctx = _lib.Context(0)
    m = ctx.color_map(W, H, n_cameras, K, _lib.color_map_option())
    for i in range(n_cameras):
        m.set_image(i, depths[i], colors[i], E[i])
    m.set_vertices(V)
    out = {"case": "%d cameras of %d x %d, %d vertices" % (n_cameras, W, H, len(V)), "reps": reps}
    t, counts = timed(m.prepare, 3)
    visits = int(counts.sum())
    out["prepare"] = dict(t, visible_pairs=visits, most_per_camera=int(counts.max()))
    m.sums()
    t, rows = timed(m.sums, reps)
    moved = visits * (24 + 64 + 4)
    out["sums"] = dict(t, accepted=int(rows[:, 28].sum()), bytes=moved, share_of_8TBps=moved / (t["median_ms"] * 1e-3) / PEAK_BYTES_PER_S)

    def proxy():
        m.set_extrinsics(E)
        return m.proxy()
    tp, _ = timed(proxy, reps)
    out["proxy"] = tp

    def proxy_and_sums():
        m.set_extrinsics(E)
        return m.sums()
    tps, _ = timed(proxy_and_sums, reps)
    out["proxy+sums"] = tps

    def step():
        m.set_extrinsics(E)
        return m.step()
    ts, _ = timed(step, reps)
    out["step"] = dict(ts, host_solve_ms_per_iteration=ts["median_ms"] - tps["median_ms"])

    def run300():
        m.set_extrinsics(E)
        return m.run(300)
    tr, res = timed(run300, reps)
    out["run300"] = dict(tr, residual_first=float(res[0]), residual_last=float(res[-1]))
    tc, _ = timed(m.colors, reps)
    out["colors"] = tc
    m.close()
    ctx.close()
    print("RESULT " + json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--cameras", type=int, default=N_CAMERAS)
    ap.add_argument("--vertices", type=int, default=N_VERTICES)
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "colormap_probe.txt"))
    a = ap.parse_args()
    if a.child:
        return child(a.reps, a.cameras, a.vertices)
    p = subprocess.run(["timeout", "-k", "10", "540", sys.executable, os.path.abspath(__file__), "--child", "--reps", str(a.reps),
                        "--cameras", str(a.cameras), "--vertices", str(a.vertices)], capture_output=True, text=True)
    if p.returncode != 0:
        print("exit %d\n%s" % (p.returncode, p.stderr[-2000:]))
        return 1
    lines = [ln[7:] for ln in p.stdout.splitlines() if ln.startswith("RESULT ")]
    res = json.loads(lines[-1])
    text = ["# tools/colormap_probe.py: %s, median of %d calls after one warm-up (min .. max), wall clock of the Python call" % (res["case"], res["reps"])]
    for k, v in res.items():
        if isinstance(v, dict):
            extra = ", ".join("%s %s" % (a_, ("%.4g" % b) if isinstance(b, float) else b) for a_, b in v.items() if a_ not in ("median_ms", "min_ms", "max_ms"))
            text.append("%-10s %10.3f ms (%.3f .. %.3f)%s" % (k, v["median_ms"], v["min_ms"], v["max_ms"], "  " + extra if extra else ""))
    text.append(lines[-1])
    print("\n".join(text))
    with open(a.out, "w") as f:
        f.write("\n".join(text) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
