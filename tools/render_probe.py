#!/usr/bin/env python
"""Times of the mesh renderer on one MI355X, for profiles/render_probe.txt: whole calls of TriMesh.render (depth, index and
mask) and Context.render_edges at 640 x 480 on two workloads,

  fused   the mesh of a 640 x 480 RGB8 frame of tests/tsdf_scene.py in a uniform 512^3 volume (the mesh of
          profiles/trimesh_probe.txt: hundreds of thousands of triangles of about a pixel), rendered at the frame's pose,
          beside ExtractTriangleMesh on the same volume
  cad     a chair of six boxes (72 triangles; a stand-in for a CAD model of the corpus, which is not part of this tree) that
          fills the frame: few triangles of tens of thousands of pixels each

each beside the bytes one pass over the data must move -- the mesh read once (24 bytes per vertex, 12 per triangle), the key
buffer written and read once (16 bytes per pixel), the three images written (9 bytes per pixel) -- over the WHOLE-CALL time
as a share of the 8 TB/s peak: launches, the compaction's read-back and the final wait included, so a lower bound of what the
kernels reach.  Every timed call ends with the device idle, so the host clock around it is the call's time.  Each workload
runs in a child process under its own time limit; one warm-up round, then the median and the spread (min .. max) of --reps
rounds.  The device's images are checked against render_host once per workload."""
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
PEAK = 8.0e12


def spread(t):
    t = np.array(t[1:]) * 1e3
    return dict(median_ms=float(np.median(t)), min_ms=float(t.min()), max_ms=float(t.max()))


def chair():
    import render_cases as cases
    V, F = [], []
    for centre, half in (((0, 0, 0), (0.25, 0.03, 0.25)), ((0, -0.3, 0.23), (0.25, 0.3, 0.02)), ((-0.21, 0.25, -0.21), (0.03, 0.22, 0.03)),
                         ((0.21, 0.25, -0.21), (0.03, 0.22, 0.03)), ((-0.21, 0.25, 0.21), (0.03, 0.22, 0.03)), ((0.21, 0.25, 0.21), (0.03, 0.22, 0.03))):
        v, f = cases.box(*half)
        F.append(f + sum(len(x) for x in V))
        V.append(v + np.asarray(centre, np.float64))
    return np.concatenate(V), np.concatenate(F).astype(np.int32)


def child(which, reps):
    import ctypes as C
    import render_cases as cases
    import tsdf_scene as scene
    from visma_amd import _lib
    frames, k = scene.frames(W, H, 1)
    depth, rgb, gray, E = frames[0]
    ctx = _lib.Context(0)
    times = {}

    def clock(name, fn):
        t0 = time.perf_counter()
        r = fn()
        times.setdefault(name, []).append(time.perf_counter() - t0)
        return r

    def drop(x):
        for i in (x if isinstance(x, (list, tuple)) else [x]):
            i.close()

    vol = None
    if which == "fused":
        vol = ctx.tsdf_uniform(4.0, 512, 0.04, _lib.TSDF_COLOR_RGB8, (-2.0, -2.0, -2.0))
        vol.integrate(depth, rgb, k, E)
        vtx, _, tri = vol.extract_triangle_mesh()
        mesh = vol.triangle_mesh()
        out = {"case": "fused: %d x %d RGB8 into a uniform 512^3 volume, rendered at the frame's pose" % (W, H)}
    else:
        vtx, tri = chair()
        E = cases.pose((0.0, 0.03, 0.62), (1.0, 0.3, 0.0), 0.45)
        k = np.array([0.9 * W, 0.9 * W, (W - 1) / 2.0, (H - 1) / 2.0])
        mesh = ctx.trimesh(vtx, tri)
        out = {"case": "cad: a chair of six boxes filling %d x %d" % (W, H)}
    out["vertices"], out["triangles"] = len(vtx), len(tri)
    d, i, m = mesh.render(W, H, k, E)
    e = ctx.render_edges(d)
    got = [x.get() for x in (d, i, m, e)]
    want = _lib.render_host(vtx, tri, W, H, k, E)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(got, want)), "the device's images differ from render_host's"
    out["covered_pixels"] = int((got[2] == 255).sum())
    out["visible_triangles"] = int(len(np.unique(got[1])) - 1)
    nv, nt = C.c_int64(0), C.c_int64(0)
    for r in range(reps + 1):
        drop(clock("render: depth, index, mask", lambda: mesh.render(W, H, k, E)))
        drop(clock("render: depth-buffer encoding", lambda: mesh.render(W, H, k, E, encoding="depth_buffer")))
        drop(clock("render_edges", lambda: ctx.render_edges(d)))
        if vol is not None:
            clock("ExtractTriangleMesh on the same volume (no read-back)",
                  lambda: ctx._chk(ctx.L.visma_icp_tsdf_extract_triangle_mesh(ctx._h, vol._v, C.byref(nv), C.byref(nt))))
    out["steps"] = {name: spread(t) for name, t in times.items()}
    px = W * H
    moved = 24 * len(vtx) + 12 * len(tri) + 16 * px + 9 * px
    out["bytes_one_pass"] = moved
    out["share_of_peak"] = moved / (out["steps"]["render: depth, index, mask"]["median_ms"] * 1e-3) / PEAK
    out["edges_share_of_peak"] = 5 * px / (out["steps"]["render_edges"]["median_ms"] * 1e-3) / PEAK
    ctx.close()
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--child", default=None)
    ap.add_argument("--timeout", type=int, default=240)
    args = ap.parse_args()
    if args.child:
        child(args.child, args.reps)
        return
    print("# tools/render_probe.py: median of %d rounds after one warm-up (min .. max), host clock around calls that end with the device idle"
          % args.reps)
    for which in ("fused", "cad"):
        p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", which, "--reps", str(args.reps)], capture_output=True,
                           text=True, timeout=args.timeout)
        if p.returncode != 0:
            sys.stderr.write(p.stderr)
            raise SystemExit("the probe's child (%s) ended with %d" % (which, p.returncode))
        out = json.loads(p.stdout.strip().splitlines()[-1])
        print("## %s: %d vertices, %d triangles, %d covered pixels, %d visible triangles; images equal render_host's"
              % (out["case"], out["vertices"], out["triangles"], out["covered_pixels"], out["visible_triangles"]))
        for name, s in out["steps"].items():
            print("%-56s %8.3f ms (%.3f .. %.3f)" % (name, s["median_ms"], s["min_ms"], s["max_ms"]))
        print("one pass moves %.2f MB (mesh, key buffer twice, three images): %.2f %% of the 8 TB/s peak over the whole call; render_edges %.2f %%"
              % (out["bytes_one_pass"] / 1e6, 100 * out["share_of_peak"], 100 * out["edges_share_of_peak"]))
        sys.stdout.flush()


if __name__ == "__main__":
    main()
