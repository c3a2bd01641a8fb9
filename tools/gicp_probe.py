#!/usr/bin/env python3
"""Time a generalized ICP pass (visma_amd/csrc/gicp.hip: search, one pair reduction, two host waits) against the pass of
the same structure the library already had: the robust point-to-plane pass with a fixed scale.  Taken the way
tools/robust_probe.py takes its times: passes from T_gt (warm passes), host loop, the persistent launch off, `--passes`
per measurement, the median of `--reps` measurements after one warm-up; us per pass = wall clock of the loop / passes,
the host's solve included on both sides.  Normals of both clouds come from the library's estimate_normals.

--baseline-lib <an older build>: every case runs `--rounds` times with this build and with that one in turn (who goes
first alternates from round to round); the older build times its robust pass only.
Cases: 5,000 -> 20,000; 65,536 -> 1,048,576; the partial pair at C4's sizes (262,144 -> 4,194,304).
Every measurement runs in a child process of its own under a time limit; nothing is started after a failure.
Prints one JSON line per measurement, then medians and spreads per case, and writes all of it to --out."""
import argparse, json, os, subprocess, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CASES = {
    "5k_20k": dict(kind="pair", ns=5000, nt=20000, limit=120),
    "64k_1m": dict(kind="pair", ns=65536, nt=1048576, limit=240),
    "c4_partial": dict(kind="partial", ns=262144, nt=4194304, limit=420),
}


def child(name, passes, reps, epsilon):
    from visma_amd import _lib, synth
    c = CASES[name]
    if c["kind"] == "pair":
        src, tgt, T_gt, r = synth.make_pair(c["ns"], c["nt"], motion="radius")
    else:
        src, tgt, T_gt, r = synth.make_partial_pair(c["ns"], c["nt"], overlap=0.5)
    ctx = _lib.Context(0)
    ctx.set_device_loop(False)
    ctx.set_persistent(False)
    tn = ctx.estimate_normals(tgt)
    sn = ctx.estimate_normals(src)
    ctx.set_clouds_f64(src, tgt)
    ctx.set_target_normals_f64(tn)
    has_gicp = hasattr(ctx.L, "visma_icp_run_gicp")
    if has_gicp:
        ctx.set_source_normals_f64(sn)

    def med(fn):
        fn()
        ts = []
        for _ in range(reps):
            t0 = time.perf_counter(); out = fn(); ts.append(time.perf_counter() - t0)
        return float(np.median(ts)) / passes * 1e6, out

    out = dict(case=name, ns=c["ns"], nt=c["nt"], radius=r, passes=passes, reps=reps, lib=os.environ.get("VISMA_ICP_LIB", ""))
    out["robust_plane_fixed_scale_us_per_pass"], res = med(lambda: ctx.run_robust(
        T_gt, r, _lib.ROBUST_TUKEY, scale=r / 3.0, plane=True, max_iter=passes - 1, rel_fitness=0.0, rel_rmse=0.0))
    out["robust_found"] = res.num_correspondences
    if has_gicp:
        out["gicp_us_per_pass"], res = med(lambda: ctx.run_gicp(T_gt, r, epsilon, max_iter=passes - 1, rel_fitness=0.0, rel_rmse=0.0))
        out.update(epsilon=epsilon, gicp_found=res.num_correspondences, gicp_mahalanobis_rmse=res.gicp.mahalanobis_rmse,
                   gicp_err_vs_T_gt=synth.rel_frobenius(res.transformation_, T_gt),
                   added_us_per_pass=out["gicp_us_per_pass"] - out["robust_plane_fixed_scale_us_per_pass"])
    ctx.close()
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--passes", type=int, default=50)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--rounds", type=int, default=1)
    ap.add_argument("--epsilon", type=float, default=1e-3)
    ap.add_argument("--cases", default=",".join(CASES))
    ap.add_argument("--baseline-lib", default=None, help="an older build: its robust pass alternates with this build's passes")
    ap.add_argument("--child", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gicp_probe.txt"))
    a = ap.parse_args()
    if a.child:
        child(a.child, a.passes, a.reps, a.epsilon)
        return 0
    lines, rows = [], []
    rc = 0
    for name in a.cases.split(","):
        for rnd in range(a.rounds):
            libs = [None] if not a.baseline_lib else ([None, a.baseline_lib] if rnd % 2 == 0 else [a.baseline_lib, None])
            for lib in libs:
                env = dict(os.environ)
                env.pop("VISMA_ICP_LIB", None)
                if lib:
                    env["VISMA_ICP_LIB"] = os.path.abspath(lib)
                cmd = [sys.executable, os.path.abspath(__file__), "--child", name, "--passes", str(a.passes), "--reps", str(a.reps),
                       "--epsilon", str(a.epsilon)]
                try:
                    p = subprocess.run(cmd, timeout=CASES[name]["limit"], stdout=subprocess.PIPE, text=True, env=env)
                    rc, line = p.returncode, p.stdout.strip()
                except subprocess.TimeoutExpired:
                    rc, line = 124, ""
                if rc != 0:
                    line = json.dumps(dict(case=name, failed=rc))
                else:
                    rows.append((name, "baseline" if lib else "this", json.loads(line)))
                print(line, flush=True)
                lines.append(line)
                if rc != 0:
                    break                                   # nothing is started after a failure
            if rc != 0:
                break
        if rc != 0:
            break
    for name in a.cases.split(","):
        for who, key in (("baseline", "robust_plane_fixed_scale_us_per_pass"), ("this", "robust_plane_fixed_scale_us_per_pass"),
                         ("this", "gicp_us_per_pass")):
            v = [r[key] for n, w, r in rows if n == name and w == who and key in r]
            if v:
                line = "%-11s %-8s %-38s runs %d  min / median / max  %.2f / %.2f / %.2f" % (name, who, key, len(v), min(v), float(np.median(v)), max(v))
                print(line, flush=True)
                lines.append(line)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    return rc


if __name__ == "__main__":
    sys.exit(main())
