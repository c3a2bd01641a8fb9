#!/usr/bin/env python
"""Kernel times of FPFH and feature matching on one MI355X, for profiles/fpfh_fgr_probe.txt:
  * FPFH at n = 262,144, Hybrid(0.05, 100), with both designs of the second pass (the first pass's lists kept in global
    memory / rebuilt by the second pass): device time of the grid build, the SPFH pass and the FPFH pass;
  * matching at 65,536 x 65,536 x 33 (the FPFH rows of two 65,536-point clouds): device time of the kernel.
The inputs are probe_cloud()'s (a bumpy sphere from a Philox stream, perturbed radial normals) --
tests/golden/gen_fpfh_fgr.py times the compiled reference on the same arrays.  Every measurement runs in a child process
under its own time limit; median of --reps calls."""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FPFH_N, FPFH_RADIUS, FPFH_MAX_NN = 262144, 0.05, 100
MATCH_N, MATCH_RADIUS = 65536, 0.1


def probe_cloud(n, seed):
    """n points on a bumpy sphere (directions: normalised normal deviates of a Philox stream; radius 1 + two low-frequency
    waves) with perturbed radial normals: a surface whose descriptors differ from point to point (on a perfect sphere with
    exact normals every pair falls into the middle bins and every FPFH row is the same)"""
    rng = np.random.Generator(np.random.Philox(seed))
    d = rng.standard_normal((n, 3))
    d /= np.linalg.norm(d, axis=1)[:, None]
    r = 1.0 + 0.1 * np.sin(6.0 * d[:, 0]) * np.cos(5.0 * d[:, 1]) + 0.05 * np.sin(9.0 * d[:, 2])
    nrm = d + 0.25 * rng.standard_normal((n, 3))
    nrm /= np.linalg.norm(nrm, axis=1)[:, None]
    return d * r[:, None], nrm


def child(what, reps):
    from visma_amd import _lib
    ctx = _lib.Context(0)
    out = {"case": what, "reps": reps}
    if what.startswith("fpfh"):
        mode = {"fpfh_keep": 1, "fpfh_rebuild": 2}[what]
        p, n = probe_cloud(FPFH_N, 1)
        rows = []
        for _ in range(reps + 1):
            ms = [0.0] * 3
            f = ctx.compute_fpfh(p, n, knn=FPFH_MAX_NN, radius=FPFH_RADIUS, second_pass=mode, timing=ms)
            rows.append(ms)
        m = np.median(np.array(rows[1:]), axis=0)               # (the first call warms the allocator and the code objects)
        out.update(n=FPFH_N, radius=FPFH_RADIUS, max_nn=FPFH_MAX_NN, grid_ms=float(m[0]), spfh_ms=float(m[1]), fpfh_ms=float(m[2]),
                   both_passes_ms=float(m[1] + m[2]), checksum=float(f.sum()), list_bytes=FPFH_N * FPFH_MAX_NN * 12)
    else:
        fa = ctx.compute_fpfh(*probe_cloud(MATCH_N, 2), knn=FPFH_MAX_NN, radius=MATCH_RADIUS)
        fb = ctx.compute_fpfh(*probe_cloud(MATCH_N, 3), knn=FPFH_MAX_NN, radius=MATCH_RADIUS)
        t = []
        for _ in range(reps + 1):
            ms = [0.0]
            idx, d2 = ctx.match_features(fa, fb, timing=ms)
            t.append(ms[0])
        out.update(na=MATCH_N, nb=MATCH_N, dim=33, match_ms=float(np.median(t[1:])), index_sum=int(idx.astype(np.int64).sum()),
                   d2_sum=float(d2.sum()), distinct_rows=int(len(np.unique(fa, axis=0))))
    ctx.close()
    print("RESULT " + json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--child", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fpfh_fgr_probe.txt"))
    a = ap.parse_args()
    if a.child:
        return child(a.child, a.reps)
    lines = []
    for what in ("fpfh_keep", "fpfh_rebuild", "match"):
        p = subprocess.run(["timeout", "-k", "10", "240", sys.executable, os.path.abspath(__file__), "--child", what, "--reps",
                            str(a.reps)], capture_output=True, text=True)
        if p.returncode != 0:
            print("%s: exit %d\n%s" % (what, p.returncode, p.stderr[-2000:]))
            return 1                                            # nothing more is started on the GPU after a failure
        lines += [ln[7:] for ln in p.stdout.splitlines() if ln.startswith("RESULT ")]
        print(lines[-1])
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
