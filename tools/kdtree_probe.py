#!/usr/bin/env python
"""Times of the public neighbour search (Context.kdtree) on one MI355X, for profiles/kdtree_probe.txt: 262,144 points of a
wavy surface patch of 4 x 4 against 262,144 queries scattered 2 cm around it (a fifth of them up to a patch width outside it),
  * creating the tree (the upload of the cloud);
  * SearchKNN(30), SearchHybrid(0.05, 100) and SearchRadius(0.05) of all the queries: the first call, which builds the
    grid for its parameter, and repeated calls, which find it kept.
The times are the wall clock of the Python call (each ends with the device idle) and include the upload of the queries, the
read-back of the lists and the host's allocation of the result arrays; the spread (min .. max) is printed beside every median
and belongs to it.  tests/golden/gen_kdtree.py --time times the compiled reference on the same input.  The measurement runs
in a child process under its own time limit; --reps repeated calls (default 10)."""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

N, NQ = 262144, 262144
KNN, RADIUS, MAX_NN = 30, 0.05, 100


def inputs(n, nq, seed=41):
    """-> (tree n x 3, queries nq x 3)"""
    rng = np.random.default_rng(seed)

    def patch(m, lo, hi):
        xy = rng.uniform(lo, hi, (m, 2))
        z = 0.3 * np.sin(1.7 * xy[:, 0]) * np.cos(1.3 * xy[:, 1])
        return np.concatenate([xy, z[:, None]], 1)
    tree = patch(n, 0.0, 4.0)
    q = patch(nq, 0.0, 4.0) + rng.normal(0.0, 0.02, (nq, 3))
    far = np.arange(nq) % 5 == 0
    q[far] = patch(int(far.sum()), -4.0, 8.0)
    return tree, q


def spread(t):
    t = np.array(t) * 1e3
    return dict(median_ms=float(np.median(t)), min_ms=float(t.min()), max_ms=float(t.max()))


def timed(fn, reps):
    t, out = [], None
    for _ in range(reps):
        t0 = time.perf_counter()
        out = fn()
        t.append(time.perf_counter() - t0)
    return t, out


def child(reps, n, nq):
    from visma_amd import _lib
    tree, q = inputs(n, nq)
    ctx = _lib.Context(0)
    out = {"case": "%d points, %d queries" % (n, nq), "reps": reps}
    t, kd = timed(lambda: ctx.kdtree(tree), 1)
    out["create"] = dict(ms=t[0] * 1e3)
    for name, fn, entries in (("knn%d" % KNN, lambda: kd.search_knn(q, KNN), lambda r: int(r[2].sum())),
                              ("hybrid%g_%d" % (RADIUS, MAX_NN), lambda: kd.search_hybrid(q, RADIUS, MAX_NN), lambda r: int(r[2].sum())),
                              ("radius%g" % RADIUS, lambda: kd.search_radius(q, RADIUS), lambda r: int(r[0][-1]))):
        first, res = timed(fn, 1)
        t, _ = timed(fn, reps)
        out[name] = dict(spread(t), first_call_ms=first[0] * 1e3, entries=entries(res))
    kd.close()
    ctx.close()
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--points", type=int, default=N)
    ap.add_argument("--queries", type=int, default=NQ)
    ap.add_argument("--timeout", type=int, default=300)
    ap.add_argument("--child", action="store_true")
    args = ap.parse_args()
    if args.child:
        child(args.reps, args.points, args.queries)
        return
    p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--reps", str(args.reps), "--points", str(args.points),
                        "--queries", str(args.queries)], capture_output=True, text=True, timeout=args.timeout)
    if p.returncode != 0:
        sys.stderr.write(p.stdout + p.stderr)
        sys.exit(p.returncode)
    r = json.loads(p.stdout.strip().splitlines()[-1])
    print("%s, %d repeated calls each" % (r["case"], r["reps"]))
    print("  create                      %9.2f ms" % r["create"]["ms"])
    for k, v in r.items():
        if isinstance(v, dict) and "median_ms" in v:
            print("  %-26s  %9.2f ms  (%.2f .. %.2f), first call %.2f ms, %d entries"
                  % (k, v["median_ms"], v["min_ms"], v["max_ms"], v["first_call_ms"], v["entries"]))


if __name__ == "__main__":
    main()
