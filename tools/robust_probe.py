#!/usr/bin/env python3
"""Time a robust ICP pass (visma_amd/csrc/robust.hip: search, with the automatic scale three select launches, weighted
reduction) against a plain pass on the path it extends: one launch per pass, host loop, the persistent launch off.
Passes from T_gt (warm passes, what a registration spends its time in), `--passes` of them per measurement, the median
of `--reps` measurements after one warm-up; us per pass = wall clock of the loop / passes, the host's solve included on
both sides.  Per case: plain, robust with a fixed scale (the radius / 3), robust with the automatic scale (Tukey).
--plain-only with VISMA_ICP_LIB=<an older build>: the plain pass of that build on the same machine.

Cases: 5,000 -> 20,000; 65,536 -> 1,048,576; the partial pair at C4's sizes (262,144 -> 4,194,304).
Every case runs in a child process of its own under a time limit; nothing is started after a failure.
Prints one JSON line per case and writes them to --out (profiles/robust_probe.jsonl)."""
import argparse, json, os, subprocess, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CASES = {
    "5k_20k": dict(kind="pair", ns=5000, nt=20000, limit=120),
    "64k_1m": dict(kind="pair", ns=65536, nt=1048576, limit=240),
    "c4_partial": dict(kind="partial", ns=262144, nt=4194304, limit=420),
}


def child(name, passes, reps, plain_only=False):
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
    if plain_only:                                          # (an older build through VISMA_ICP_LIB: the plain pass alone)
        ctx.close()
        print(json.dumps(dict(case=name, ns=c["ns"], nt=c["nt"], radius=r, passes=passes, reps=reps,
                              lib=os.environ.get("VISMA_ICP_LIB", ""), plain_us_per_pass=plain_us)), flush=True)
        return
    fixed_us, _ = med(lambda: ctx.run_robust(T_gt, r, _lib.ROBUST_TUKEY, scale=r / 3.0, max_iter=passes - 1, rel_fitness=0.0, rel_rmse=0.0))
    auto_us, res = med(lambda: ctx.run_robust(T_gt, r, _lib.ROBUST_TUKEY, max_iter=passes - 1, rel_fitness=0.0, rel_rmse=0.0))
    ctx.close()
    print(json.dumps(dict(case=name, ns=c["ns"], nt=c["nt"], radius=r, kernel="tukey", passes=passes, reps=reps,
                          plain_us_per_pass=plain_us, robust_fixed_scale_us_per_pass=fixed_us,
                          robust_auto_scale_us_per_pass=auto_us, added_fixed_us_per_pass=fixed_us - plain_us,
                          added_auto_us_per_pass=auto_us - plain_us, found=res.num_correspondences,
                          scale=res.robust.scale, zero_weight=res.robust.zero_weight,
                          err_vs_T_gt=synth.rel_frobenius(res.transformation_, T_gt))), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--passes", type=int, default=50)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--cases", default=",".join(CASES))
    ap.add_argument("--child", default=None)
    ap.add_argument("--plain-only", action="store_true", help="time the plain pass alone (a build without robust ICP, VISMA_ICP_LIB)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "robust_probe.jsonl"))
    a = ap.parse_args()
    if a.child:
        child(a.child, a.passes, a.reps, a.plain_only)
        return 0
    lines = []
    rc = 0
    for name in a.cases.split(","):
        cmd = [sys.executable, os.path.abspath(__file__), "--child", name, "--passes", str(a.passes), "--reps", str(a.reps)] + (["--plain-only"] if a.plain_only else [])
        try:
            p = subprocess.run(cmd, timeout=CASES[name]["limit"], stdout=subprocess.PIPE, text=True)
            rc, line = p.returncode, p.stdout.strip()
        except subprocess.TimeoutExpired:
            rc, line = 124, ""
        if rc != 0:
            line = json.dumps(dict(case=name, failed=rc))
        print(line, flush=True)
        lines.append(line)
        if rc != 0:
            break                                           # nothing is started after a failure
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    return rc


if __name__ == "__main__":
    sys.exit(main())
