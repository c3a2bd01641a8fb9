#!/usr/bin/env python3
"""Time a trimmed ICP pass (visma_amd/csrc/trim.hip: search, three select launches, masked reduction) against a plain
pass on the path it extends: one launch per pass, host loop, the persistent launch off.  Passes from T_gt (warm
passes, what a registration spends its time in), `--passes` of them per measurement, the median of `--reps`
measurements after one warm-up; us per pass = wall clock of the loop / passes, the host's solve included on both sides.

Cases: 5,000 -> 20,000; 65,536 -> 1,048,576; the partial pair at C4's sizes (262,144 -> 4,194,304).
Every case runs in a child process of its own under a time limit; nothing is started after a failure.
Prints one JSON line per case."""
import argparse, json, os, subprocess, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CASES = {
    "5k_20k": dict(kind="pair", ns=5000, nt=20000, keep=0.7, limit=120),
    "64k_1m": dict(kind="pair", ns=65536, nt=1048576, keep=0.7, limit=240),
    "c4_partial": dict(kind="partial", ns=262144, nt=4194304, keep=0.5, limit=420),
}


def child(name, passes, reps):
    from visma_amd import _lib, synth
    c = CASES[name]
    if c["kind"] == "pair":
        src, tgt, T_gt, r = synth.make_pair(c["ns"], c["nt"], motion="radius")
    else:
        src, tgt, T_gt, r = synth.make_partial_pair(c["ns"], c["nt"], overlap=0.5)
    ctx = _lib.Context(0)
    ctx.set_device_loop(False)
    ctx.set_persistent(False)
    ctx.set_clouds_f64(src, tgt)

    def med(fn):
        fn()
        ts = []
        for _ in range(reps):
            t0 = time.perf_counter(); out = fn(); ts.append(time.perf_counter() - t0)
        return float(np.median(ts)) / passes * 1e6, out

    plain_us, _ = med(lambda: ctx.iterate(T_gt, r, passes))
    trim_us, res = med(lambda: ctx.run_trimmed(T_gt, r, c["keep"], passes - 1, 0.0, 0.0))
    all_us, _ = med(lambda: ctx.run_trimmed(T_gt, r, 0.999999, passes - 1, 0.0, 0.0))
    ctx.close()
    print(json.dumps(dict(case=name, ns=c["ns"], nt=c["nt"], radius=r, keep=c["keep"], passes=passes, reps=reps,
                          plain_us_per_pass=plain_us, trimmed_us_per_pass=trim_us, added_us_per_pass=trim_us - plain_us,
                          trimmed_keep_nearly_1_us_per_pass=all_us, found=res.num_correspondences, kept=res.trim.kept,
                          err_vs_T_gt=synth.rel_frobenius(res.transformation_, T_gt))), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--passes", type=int, default=50)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--cases", default=",".join(CASES))
    ap.add_argument("--child", default=None)
    a = ap.parse_args()
    if a.child:
        child(a.child, a.passes, a.reps)
        return 0
    for name in a.cases.split(","):
        cmd = [sys.executable, os.path.abspath(__file__), "--child", name, "--passes", str(a.passes), "--reps", str(a.reps)]
        try:
            rc = subprocess.run(cmd, timeout=CASES[name]["limit"]).returncode
        except subprocess.TimeoutExpired:
            rc = 124
        if rc != 0:
            print(json.dumps(dict(case=name, failed=rc)), flush=True)
            return rc                                       # nothing is started after a failure
    return 0


if __name__ == "__main__":
    sys.exit(main())
