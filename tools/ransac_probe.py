#!/usr/bin/env python
"""Times of RANSAC global registration on one MI355X and the fragment-pair finding, for profiles/ransac_probe.txt.  On the
full fragment pair of tests/golden/fragments.npz (3,903 x 3,458 points with normals), FPFH Hybrid(0.25, 100), one exact match:
  * the hypothesis stage at 4,000,000 trials, ransac_n = 4, all three checkers on: device time;
  * the whole call at Open3D's pipeline settings (4,000,000 iterations, 500 validations), its validation and hypothesis parts;
  * fast global registration and RANSAC from no pose: each pose's error against fragments.npz: init, and whether visma_icp_run
    from it (radius 0.25, point to point) reaches the pose the fixture's trace reaches.
tests/golden/gen_ransac.py --time times the compiled reference on the same call.  Every measurement runs in a child process
under its own time limit; median of --reps calls."""
import argparse
import json
import math
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FPFH_RADIUS, FPFH_MAX_NN = 0.25, 100
EDGE, DIST, ANGLE_DEG, MAX_DIST = 0.9, 0.075, 30.0, 0.075
RANSAC_N, MAX_ITERATION, MAX_VALIDATION = 4, 4000000, 500
SEED = 1


def fragments():
    f = np.load(os.path.join(ROOT, "tests", "golden", "fragments.npz"))
    return [f[k].astype(np.float64) for k in ("src", "src_normals", "tgt", "tgt_normals")], f


def pose_error(T, truth):
    d = T @ np.linalg.inv(truth)
    ang = math.degrees(math.acos(max(-1.0, min(1.0, (np.trace(d[:3, :3]) - 1.0) / 2.0))))
    return ang, float(np.linalg.norm(T[:3, 3] - truth[:3, 3]))


def child(what, reps):
    from visma_amd import _lib
    ctx = _lib.Context(0)
    (src, sn, tgt, tn), frag = fragments()
    fs = ctx.compute_fpfh(src, sn, knn=FPFH_MAX_NN, radius=FPFH_RADIUS); ft = ctx.compute_fpfh(tgt, tn, knn=FPFH_MAX_NN, radius=FPFH_RADIUS)
    out = {"case": what, "reps": reps, "ns": len(src), "nt": len(tgt)}
    opt = dict(ransac_n=RANSAC_N, max_iteration=MAX_ITERATION, max_validation=MAX_VALIDATION, edge_length_similarity=EDGE,
               distance_threshold=DIST, normal_angle=math.radians(ANGLE_DEG))
    if what == "hypotheses":
        nn = ctx.match_features(ft, fs)[0]
        t = []
        for _ in range(reps + 1):
            counts, ms = ctx.ransac_hypotheses_probe(src, tgt, nn, _lib.ransac_option(**opt), seed=SEED,
                                                     n_trials=MAX_ITERATION, src_normals=sn, tgt_normals=tn)
            t.append(ms)
        out.update(trials=MAX_ITERATION, ransac_n=RANSAC_N, hypothesis_ms=float(np.median(t[1:])), passed=counts[0],
                   rejected_before=counts[1], rejected_after=counts[2])
    elif what == "whole_call":
        rows = []
        for _ in range(reps + 1):
            t0 = time.perf_counter()
            r = ctx.registration_ransac_feature_matching(src, fs, tgt, ft, MAX_DIST, _lib.ransac_option(**opt), seed=SEED,
                                                         src_normals=sn, tgt_normals=tn)
            rows.append([(time.perf_counter() - t0) * 1e3, r.ransac.hypothesis_ms, r.ransac.validation_ms])
        m = np.median(np.array(rows[1:]), axis=0)
        out.update(whole_call_ms=float(m[0]), hypothesis_ms=float(m[1]), validation_ms=float(m[2]), trials=r.ransac.n_trials,
                   validated=r.ransac.n_validated, best_trial=r.ransac.best_trial, fitness=r.fitness_, rmse=r.inlier_rmse_,
                   K=r.num_correspondences)
    else:                                                       # the finding: FGR and RANSAC on the real pair
        init, final = frag["init"], frag["trace_p2p"][-1][:16].reshape(4, 4)
        Tf, _ = ctx.fast_global_registration(src, fs, tgt, ft, seed=SEED)
        r = ctx.registration_ransac_feature_matching(src, fs, tgt, ft, MAX_DIST, _lib.ransac_option(**opt), seed=SEED, src_normals=sn,
                                                     tgt_normals=tn)
        ctx.set_clouds_f64(src, tgt)
        for name, T in (("fgr", Tf), ("ransac", r.transformation_), ("init", init)):
            ang, dt = pose_error(T, init)
            at = ctx.run(T, MAX_DIST, 0, 0.0, 0.0)
            icp = ctx.run(T, float(frag["radius"]), 60, 0.0, 0.0)
            fang, fdt = pose_error(icp.transformation_, final)
            out[name] = dict(degrees_off_init=ang, shift_off_init=dt, fitness_at_pose=at.fitness_, rmse_at_pose=at.inlier_rmse_,
                             icp_fitness=icp.fitness_, icp_rmse=icp.inlier_rmse_, icp_degrees_off_trace=fang, icp_shift_off_trace=fdt,
                             icp_rel_frobenius_to_trace=float(np.linalg.norm(icp.transformation_ - final) / np.linalg.norm(final)))
        out["ransac_info"] = dict(trials=r.ransac.n_trials, validated=r.ransac.n_validated, best_trial=r.ransac.best_trial)
    ctx.close()
    print("RESULT " + json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--child", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ransac_probe.txt"))
    a = ap.parse_args()
    if a.child:
        return child(a.child, a.reps)
    lines = []
    for what in ("hypotheses", "whole_call", "fragment_pair"):
        p = subprocess.run(["timeout", "-k", "10", "200", sys.executable, os.path.abspath(__file__), "--child", what, "--reps",
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
