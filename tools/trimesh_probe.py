#!/usr/bin/env python
"""Times of the TriangleMesh steps on one MI355X, for profiles/trimesh_probe.txt, on the meshes of tools/tsdf_mesh_probe.py's
two workloads (a 640 x 480 RGB8 frame of tests/tsdf_scene.py into a uniform 512^3 volume, and into a scalable volume at
Open3D's pipeline settings: voxel 4 / 512 m, sdf_trunc 0.04, units of 16, stride 4).

Two chains over the mesh the volume extracted, step by step:
  device    triangle_mesh() (visma_icp_trimesh_from_tsdf: device to device), compute_vertex_normals, purge, get
  download  extract's read-back (visma_icp_tsdf_get_triangle_mesh), Context.trimesh (the upload), compute_vertex_normals, purge, get
Both end in the same rows (asserted).  Every timed call ends with the device idle (each entry point synchronises its stream
before it returns), so the host clock around it is the call's time, read-backs and the host's allocations included.  Each
workload runs in a child process of its own under its own time limit; one warm-up round, then the median and the spread
(min .. max) of --reps rounds (default 20).  --save-mesh DIR keeps each mesh as DIR/trimesh_probe_<workload>.npz:
tests/golden/gen_trimesh.py --time <that file> times the compiled reference (one CPU thread) on the same mesh; pass what it
printed with --reference to have it recorded beside."""
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
    nv, nt = (len(a) for a in vol.extract_triangle_mesh()[::2])
    L, h, v = ctx.L, ctx._h, vol._v
    times = {}

    def clock(name, fn):
        t0 = time.perf_counter()
        r = fn()
        times.setdefault(name, []).append(time.perf_counter() - t0)
        return r

    def read_back():
        vtx, col, tri = np.empty((nv, 3)), np.empty((nv, 3)), np.empty((nt, 3), np.int32)
        ctx._chk(L.visma_icp_tsdf_get_triangle_mesh(h, v, _lib._p(vtx, _lib._dp), _lib._p(col, _lib._dp), _lib._p(tri, _lib._ip), nv, nt))
        return vtx, col, tri

    removed = None
    for _ in range(reps + 1):
        m = clock("device: from_tsdf", vol.triangle_mesh)
        clock("device: compute_vertex_normals", m.compute_vertex_normals)
        removed = clock("device: purge", m.purge)
        a = clock("device: get", m.get)
        m.close()
        vtx, col, tri = clock("download: read-back", read_back)
        m = clock("download: upload", lambda: ctx.trimesh(vtx, tri, vertex_colors=col))
        clock("download: compute_vertex_normals", m.compute_vertex_normals)
        assert clock("download: purge", m.purge) == removed
        b = clock("download: get", m.get)
        m.close()
        for key in a:
            assert (a[key] is None) == (b[key] is None) and (a[key] is None or a[key].tobytes() == b[key].tobytes()), key
    if save:
        os.makedirs(save, exist_ok=True)
        np.savez_compressed(os.path.join(save, "trimesh_probe_%s.npz" % which), vertices=vtx, colors=col, triangles=tri)
    out.update(vertices=nv, triangles=nt, purge_removed=list(removed), steps={name: spread(t) for name, t in times.items()})
    vol.close()
    ctx.close()
    print("RESULT " + json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--resolution", type=int, default=R)
    ap.add_argument("--child", default="")
    ap.add_argument("--save-mesh", default="")
    ap.add_argument("--reference", default="", help="what tests/golden/gen_trimesh.py --time printed, recorded as it is")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "trimesh_probe.txt"))
    a = ap.parse_args()
    if a.child:
        return child(a.child, a.reps, a.resolution, a.save_mesh)
    text = ["# tools/trimesh_probe.py: median of %d rounds after one warm-up (min .. max), host clock around calls that end with the device idle" % a.reps]
    for which in ("uniform", "scalable"):
        p = subprocess.run(["timeout", "-k", "10", "300", sys.executable, os.path.abspath(__file__), "--child", which, "--reps", str(a.reps),
                            "--resolution", str(a.resolution), "--save-mesh", a.save_mesh], capture_output=True, text=True)
        if p.returncode != 0:                            # nothing more is started on the device after a step that failed
            print("%s: exit %d\n%s" % (which, p.returncode, p.stderr[-2000:]))
            return 1
        lines = [ln[7:] for ln in p.stdout.splitlines() if ln.startswith("RESULT ")]
        res = json.loads(lines[-1])
        text.append("## %s: %d vertices, %d triangles, Purge removes %s" % (res["case"], res["vertices"], res["triangles"], res["purge_removed"]))
        for name, s in res["steps"].items():
            text.append("%-36s %9.3f ms (%.3f .. %.3f)" % (name, s["median_ms"], s["min_ms"], s["max_ms"]))
        for chain in ("device", "download"):
            text.append("%-36s %9.3f ms (sum of the medians)" % (chain + ": whole chain", sum(s["median_ms"] for n, s in res["steps"].items() if n.startswith(chain))))
        text.append(lines[-1])
    if a.reference:
        text.append("## the compiled reference (tests/golden/gen_trimesh.py --time; one thread of a CPU that is not the MI355X's host)")
        text.append(a.reference)
    print("\n".join(text))
    with open(a.out, "w") as f:
        f.write("\n".join(text) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
