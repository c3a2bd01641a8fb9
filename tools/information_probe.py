#!/usr/bin/env python
"""Times of the information matrix on one MI355X, for profiles/information_probe.txt:
  * all 1,225 pairs of 50 clouds of about 4,000 points in one visma_icp_information_matrices call (49 edges per target);
  * one edge at 262,144 -> 4,194,304 points (upload, search and reduction, and the reduction alone on the pass it left).
tests/golden/gen_posegraph.py --time times the compiled reference on reference_inputs().  Every measurement runs in a child
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

N_CLOUDS, CLOUD_POINTS, RADIUS = 50, 4000, 0.05
BIG_NS, BIG_NT = 262144, 4194304


def fifty_clouds():
    """50 samplings of one surface, each with its own seed: every pair overlaps everywhere"""
    from visma_amd import synth
    return [synth.surface_points(CLOUD_POINTS, 1000 + i) for i in range(N_CLOUDS)]


def big_pair():
    from visma_amd import synth
    src, tgt, T, r = synth.make_pair(BIG_NS, BIG_NT, motion="radius")
    return src, tgt, T, r


def reference_inputs():
    """what gen_posegraph.py --time hands the reference: one of the 1,225 pairs, and the large edge"""
    c = fifty_clouds()
    return {"one pair of the 50 clouds": (c[0], c[1], np.eye(4), RADIUS), "the large edge": big_pair()}


def spread(t):
    t = np.array(t[1:]) * 1e3
    return dict(median_ms=float(np.median(t)), min_ms=float(t.min()), max_ms=float(t.max()))


def child(what, reps):
    from visma_amd import _lib
    ctx = _lib.Context(0)
    out = {"case": what, "reps": reps}
    if what == "all_pairs":
        c = fifty_clouds()
        problems = [(c[i], c[j], np.eye(4), RADIUS) for j in range(N_CLOUDS) for i in range(j)]     # grouped by target j
        t = []
        for _ in range(reps + 1):
            t0 = time.perf_counter()
            M, k = ctx.information_matrices(problems)
            t.append(time.perf_counter() - t0)
        out.update(edges=len(problems), points=CLOUD_POINTS, mean_K=float(k.mean()), **spread(t))
    else:
        src, tgt, T, r = big_pair()
        ctx.set_clouds_f64(src, tgt)
        t, tr = [], []
        for _ in range(reps + 1):
            t0 = time.perf_counter()
            M, k = ctx.information_matrix(T, r)
            t.append(time.perf_counter() - t0)
            t0 = time.perf_counter()
            ctx.reduce_information()
            tr.append(time.perf_counter() - t0)
        out.update(ns=len(src), nt=len(tgt), K=int(k), search_and_reduce=spread(t), reduce_again=spread(tr))
    ctx.close()
    print("RESULT " + json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--child", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "information_probe.txt"))
    a = ap.parse_args()
    if a.child:
        return child(a.child, a.reps)
    lines = []
    for what in ("all_pairs", "large_edge"):
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
