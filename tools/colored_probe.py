#!/usr/bin/env python3
"""Time a colored ICP pass (visma_amd/csrc/colored.hip: search, one pair reduction, two host waits) against the pass of
the same structure the library already had, the generalized pass, on the same clouds in the same run; and the colour
gradient kernel (color_gradient.hip) against estimate_normals' Hybrid search with the same radius and max_nn on the same
cloud (the same search: any gap is the per-neighbour projection and the intensity gather).  Taken the way
tools/gicp_probe.py takes its times: passes from T_gt (warm passes), host loop, the persistent launch off, `--passes`
per measurement, the median of `--reps` measurements after one warm-up; us per pass = wall clock of the loop / passes,
the host's solve included on both sides.  The gradient and the normals are timed as whole calls (upload, grid build,
kernel, download), ms, median of `--reps`.  Normals of both clouds come from the library's estimate_normals; colours
are a smooth synthetic texture evaluated at the points.

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


def texture(p, w):
    v = 0.5 + 0.25 * np.sin(2 * np.pi * p[:, 0] / w) * np.cos(2 * np.pi * 0.7 * p[:, 1] / w) + 0.2 * np.sin(2 * np.pi * (0.6 * p[:, 0] + p[:, 2]) / (2.6 * w))
    return np.stack([0.9 * v, v, 1.1 * v], 1)


def child(name, passes, reps, lam, epsilon):
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
    tc = texture(tgt, 20.0 * r)
    sc = texture((src @ T_gt[:3, :3].T) + T_gt[:3, 3], 20.0 * r)
    ctx.set_clouds_f64(src, tgt)
    ctx.set_target_normals_f64(tn); ctx.set_source_normals_f64(sn)
    ctx.set_target_colors_f64(tc); ctx.set_source_colors_f64(sc)

    def med(fn, scale):
        fn()
        ts = []
        for _ in range(reps):
            t0 = time.perf_counter(); out = fn(); ts.append(time.perf_counter() - t0)
        return float(np.median(ts)) * scale, out

    out = dict(case=name, ns=c["ns"], nt=c["nt"], radius=r, passes=passes, reps=reps)
    out["gicp_us_per_pass"], res = med(lambda: ctx.run_gicp(T_gt, r, epsilon, max_iter=passes - 1, rel_fitness=0.0, rel_rmse=0.0), 1e6 / passes)
    out["gicp_found"] = res.num_correspondences
    out["colored_us_per_pass"], res = med(lambda: ctx.run_colored(T_gt, r, lam, max_iter=passes - 1, rel_fitness=0.0, rel_rmse=0.0), 1e6 / passes)
    out.update(lambda_geometric=lam, colored_found=res.num_correspondences, colored_cost=res.colored.cost,
               colored_photometric_cost=res.colored.photometric_cost, colored_err_vs_T_gt=synth.rel_frobenius(res.transformation_, T_gt),
               colored_over_gicp=out["colored_us_per_pass"] / out["gicp_us_per_pass"])
    out["normals_hybrid_ms"], _ = med(lambda: ctx.estimate_normals(tgt, knn=30, radius=2.0 * r), 1e3)
    out["gradient_ms"], g = med(lambda: ctx.color_gradient(tgt, tn, tc, 2.0 * r, 30), 1e3)
    out.update(gradient_over_normals=out["gradient_ms"] / out["normals_hybrid_ms"], gradient_nonzero=int(np.any(g != 0.0, axis=1).sum()))
    ctx.close()
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--passes", type=int, default=50)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--rounds", type=int, default=1)
    ap.add_argument("--lambda-geometric", type=float, default=0.968)
    ap.add_argument("--epsilon", type=float, default=1e-3)
    ap.add_argument("--cases", default=",".join(CASES))
    ap.add_argument("--child", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "colored_probe.txt"))
    a = ap.parse_args()
    if a.child:
        child(a.child, a.passes, a.reps, a.lambda_geometric, a.epsilon)
        return 0
    lines, rows = [], []
    rc = 0
    for name in a.cases.split(","):
        for rnd in range(a.rounds):
            cmd = [sys.executable, os.path.abspath(__file__), "--child", name, "--passes", str(a.passes), "--reps", str(a.reps),
                   "--lambda-geometric", str(a.lambda_geometric), "--epsilon", str(a.epsilon)]
            try:
                p = subprocess.run(cmd, timeout=CASES[name]["limit"], stdout=subprocess.PIPE, text=True)
                rc, line = p.returncode, p.stdout.strip()
            except subprocess.TimeoutExpired:
                rc, line = 124, ""
            if rc != 0:
                line = json.dumps(dict(case=name, failed=rc))
            else:
                rows.append((name, json.loads(line)))
            print(line, flush=True)
            lines.append(line)
            if rc != 0:
                break                                       # nothing is started after a failure
        if rc != 0:
            break
    for name in a.cases.split(","):
        for key in ("gicp_us_per_pass", "colored_us_per_pass", "colored_over_gicp", "normals_hybrid_ms", "gradient_ms", "gradient_over_normals"):
            v = [r[key] for n, r in rows if n == name and key in r]
            if v:
                line = "%-11s %-24s runs %d  min / median / max  %.2f / %.2f / %.2f" % (name, key, len(v), min(v), float(np.median(v)), max(v))
                print(line, flush=True)
                lines.append(line)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    return rc


if __name__ == "__main__":
    sys.exit(main())
