#!/usr/bin/env python3
"""Time the cloud-to-cloud and nearest-neighbour distances (visma_amd/csrc/cloud_distance.hip) end to end: host arrays
in, distances out, the median of `--reps` calls after one warm-up call.  Prints one JSON line.  `--cpu` also times
the compiled reference's open3d::ComputePointCloudToPointCloudDistance (oracle/_ref, OpenMP with the thread count
the machine sets) on the same inputs and checks the results are equal."""
import argparse, json, os, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from visma_amd import _lib, synth  # noqa: E402


def med_s(fn, reps):
    fn()                                                           # warm-up
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter(); out = fn(); ts.append(time.perf_counter() - t0)
    return float(np.median(ts)), out


def far(s, t, frac=0.01):
    """`frac` of the queries moved 100x the target's extent away, in random directions."""
    ext = float((t.max(0) - t.min(0)).max())
    s = s.copy()
    k = np.random.default_rng(3).choice(len(s), int(len(s) * frac), replace=False)
    dirs = np.random.default_rng(4).standard_normal((len(k), 3))
    s[k] += 100.0 * ext * dirs / np.linalg.norm(dirs, axis=1, keepdims=True)
    return s


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--cpu", action="store_true")
    ap.add_argument("--small", action="store_true", help="only the 5,000 -> 20,000 row (a quick check)")
    a = ap.parse_args()
    ctx = _lib.Context(0)
    ref = None
    if a.cpu:
        from oracle.oracle import Ref
        ref = Ref()
    rows = []
    s5, t20, _, _ = synth.make_pair(5000, 20000)
    cases = [("pc_5k_20k", s5, t20)]
    if not a.small:
        s, t, _, _ = synth.make_pair(262144, 4194304, motion="radius")
        cases += [("pc_256k_4m", s, t), ("pc_256k_4m_far1pct", far(s, t), t)]
    for name, s, t in cases:
        gpu_s, d = med_s(lambda: ctx.point_cloud_distance(s, t), a.reps)
        row = dict(case=name, ns=len(s), nt=len(t), gpu_s=gpu_s)
        if ref is not None:
            t0 = time.perf_counter(); rd = ref.nn_distance(s, t); row["ref_s"] = time.perf_counter() - t0
            row["speedup"] = row["ref_s"] / gpu_s
            row["equal_to_ref"] = bool(np.array_equal(d, rd))
        rows.append(row)
    if not a.small:
        for n in (1048576, 4194304):
            _, x, _, _ = synth.make_pair(10, n, motion="radius")
            gpu_s, _ = med_s(lambda: ctx.nearest_neighbor_distance(x), a.reps)
            rows.append(dict(case="nn_self_%dk" % (n // 1024), n=n, gpu_s=gpu_s))
    ctx.close()
    print(json.dumps(dict(reps=a.reps, omp_num_threads=os.environ.get("OMP_NUM_THREADS"), rows=rows)))


if __name__ == "__main__":
    main()
