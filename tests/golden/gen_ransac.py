"""Generate tests/golden/ransac.npz: what the compiled reference computes for the inputs tests/test_ransac.py pins its numpy
specification with.  Run once where the reference checkout exists; the fixture holds DATA only.

The generator writes a small harness of its own into a scratch directory, compiles it there together with the reference's
CorrespondenceChecker.cpp, TransformationEstimation.cpp, Feature.cpp, KDTreeFlann.cpp, PointCloud.cpp, Eigen.cpp, Console.cpp
and Helper.cpp (the harness includes Registration.cpp itself: EvaluateRANSACBasedOnCorrespondence lives in its unnamed
namespace), runs it and records, on every third point of fragments.npz (src, tgt, with normals):
  nn                 a pair table made here, not by the reference: for every source point the target point nearest to it under
                     fragments.npz: init (brute force, f64), replaced by a random target point for three points in ten -- so
                     that the draw sets below meet every verdict
  draws, draw_n      240 draw sets of source indices (56 each of ransac_n = 3, 4, 6, 8, then 16 of ransac_n = 4 with one index
                     repeated), padded to 8 with -1
  T                  TransformationEstimationPointToPoint(false).ComputeTransformation(source, target, corres) per draw set
  edge, dist, normal the verdict of CorrespondenceCheckerBasedOnEdgeLength(0.9), ...BasedOnDistance(radius) and
                     ...BasedOnNormal(30 degrees) on that set at that T (1 = passed)
  count, fitness, rmse   EvaluateRegistration(source, target, max_dist, T)
  pairs              600 pairs (2 k, nn[2 k])
  corres_sets, corres_fitness, corres_rmse   EvaluateRANSACBasedOnCorrespondence(source moved by T, target, pairs, max_dist, T)
                     at the T of every 12th draw set (20 of them); those sets draw among the source points of `pairs`
With --time it also times the reference's RegistrationRANSACBasedOnFeatureMatching on the inputs of tools/ransac_probe.py
(this machine's CPU; printed, not stored).  Nothing compiled and no reference text is kept."""
import argparse
import os
import struct
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = os.environ.get("VISMA_REF", "/root/reference")
O3D = os.path.join(REF, "thirdparty", "Open3D")
SCRATCH = os.environ.get("VISMA_SCRATCH") or tempfile.mkdtemp(prefix="ransac_")      # outside the repository

EDGE, ANGLE_DEG, MAX_DIST = 0.9, 30.0, 0.1

HARNESS = r'''
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "%(o3d)s/src/Core/Registration/Registration.cpp"
#include <Core/Registration/CorrespondenceChecker.h>
using namespace open3d;
static void rd(FILE *f, void *p, size_t n) { if (fread(p, 1, n, f) != n) std::exit(2); }
static void cloud(FILE *f, std::vector<Eigen::Vector3d> &v, long long n)
{
    v.resize((size_t)n);
    for (long long i = 0; i < n; i++) { double p[3]; rd(f, p, 24); v[(size_t)i] = Eigen::Vector3d(p[0], p[1], p[2]); }
}
static void wd(FILE *o, double v) { fwrite(&v, 8, 1, o); }
static double now() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }
int main(int argc, char **argv)
{
    FILE *f = std::fopen(argv[2], "rb"), *o = std::fopen(argv[3], "wb");
    if (!f || !o) return 2;
    long long ns, nt;
    rd(f, &ns, 8); rd(f, &nt, 8);
    PointCloud src, tgt;
    cloud(f, src.points_, ns); cloud(f, src.normals_, ns); cloud(f, tgt.points_, nt); cloud(f, tgt.normals_, nt);
    if (!std::strcmp(argv[1], "fixture")) {
        long long nsets, K, ncs; double edge, radius, angle, max_dist;
        rd(f, &nsets, 8); rd(f, &K, 8); rd(f, &ncs, 8); rd(f, &edge, 8); rd(f, &radius, 8); rd(f, &angle, 8); rd(f, &max_dist, 8);
        std::vector<int> nn((size_t)ns);
        rd(f, nn.data(), 4 * (size_t)ns);
        CorrespondenceSet pairs;
        for (long long c = 0; c < K; c++) { int p[2]; rd(f, p, 8); pairs.push_back(Eigen::Vector2i(p[0], p[1])); }
        std::vector<int> cs((size_t)ncs);
        rd(f, cs.data(), 4 * (size_t)ncs);
        TransformationEstimationPointToPoint est(false);
        CorrespondenceCheckerBasedOnEdgeLength ce(edge);
        CorrespondenceCheckerBasedOnDistance cd(radius);
        CorrespondenceCheckerBasedOnNormal cn(angle);
        std::vector<Eigen::Matrix4d> Ts;
        for (long long s = 0; s < nsets; s++) {
            int d[9];
            rd(f, d, 36);                                       // n, then 8 indices
            CorrespondenceSet corres;
            for (int j = 0; j < d[0]; j++) corres.push_back(Eigen::Vector2i(d[1 + j], nn[(size_t)d[1 + j]]));
            Eigen::Matrix4d T = est.ComputeTransformation(src, tgt, corres);
            Ts.push_back(T);
            for (int i = 0; i < 4; i++) for (int j = 0; j < 4; j++) wd(o, T(i, j));
            wd(o, ce.Check(src, tgt, corres, T) ? 1.0 : 0.0);
            wd(o, cd.Check(src, tgt, corres, T) ? 1.0 : 0.0);
            wd(o, cn.Check(src, tgt, corres, T) ? 1.0 : 0.0);
            RegistrationResult r = EvaluateRegistration(src, tgt, max_dist, T);
            wd(o, (double)r.correspondence_set_.size()); wd(o, r.fitness_); wd(o, r.inlier_rmse_);
        }
        for (long long c = 0; c < ncs; c++) {
            PointCloud pcd = src;
            pcd.Transform(Ts[(size_t)cs[(size_t)c]]);
            RegistrationResult r = EvaluateRANSACBasedOnCorrespondence(pcd, tgt, pairs, max_dist, Ts[(size_t)cs[(size_t)c]]);
            wd(o, r.fitness_); wd(o, r.inlier_rmse_);
        }
    } else {                                                    // the whole registration, timed: features, then RANSAC
        double radius, edge, dist, angle, max_dist; int max_nn, ransac_n, max_iteration, max_validation;
        rd(f, &radius, 8); rd(f, &edge, 8); rd(f, &dist, 8); rd(f, &angle, 8); rd(f, &max_dist, 8);
        rd(f, &max_nn, 4); rd(f, &ransac_n, 4); rd(f, &max_iteration, 4); rd(f, &max_validation, 4);
        auto fs = ComputeFPFHFeature(src, KDTreeSearchParamHybrid(radius, max_nn));
        auto ft = ComputeFPFHFeature(tgt, KDTreeSearchParamHybrid(radius, max_nn));
        CorrespondenceCheckerBasedOnEdgeLength ce(edge);
        CorrespondenceCheckerBasedOnDistance cd(dist);
        CorrespondenceCheckerBasedOnNormal cn(angle);
        std::vector<std::reference_wrapper<const CorrespondenceChecker>> checkers;
        checkers.push_back(ce); checkers.push_back(cd); checkers.push_back(cn);
        double t0 = now();
        RegistrationResult r = RegistrationRANSACBasedOnFeatureMatching(src, tgt, *fs, *ft, max_dist,
                TransformationEstimationPointToPoint(false), ransac_n, checkers, RANSACConvergenceCriteria(max_iteration, max_validation));
        wd(o, now() - t0); wd(o, r.fitness_); wd(o, r.inlier_rmse_);
        for (int i = 0; i < 4; i++) for (int j = 0; j < 4; j++) wd(o, r.transformation_(i, j));
    }
    std::fclose(o);
    return 0;
}
'''


def build():
    os.makedirs(SCRATCH, exist_ok=True)
    src = os.path.join(SCRATCH, "harness.cpp")
    with open(src, "w") as f:
        f.write(HARNESS % {"o3d": O3D})
    exe = os.path.join(SCRATCH, "harness")
    core = os.path.join(O3D, "src", "Core")
    cmd = ["g++", "-std=c++11", "-O2", "-fopenmp", "-w", "-I" + os.path.join(O3D, "src"), "-I" + os.path.join(O3D, "3rdparty", "Eigen"),
           "-I" + os.path.join(O3D, "3rdparty"), "-I" + O3D, src, os.path.join(core, "Registration", "CorrespondenceChecker.cpp"),
           os.path.join(core, "Registration", "TransformationEstimation.cpp"), os.path.join(core, "Registration", "Feature.cpp"),
           os.path.join(core, "Geometry", "KDTreeFlann.cpp"), os.path.join(core, "Geometry", "PointCloud.cpp"),
           os.path.join(core, "Utility", "Eigen.cpp"), os.path.join(core, "Utility", "Console.cpp"),
           os.path.join(core, "Utility", "Helper.cpp"), "-o", exe]
    subprocess.check_call(cmd)
    return exe


def clouds(step):
    frag = np.load(os.path.join(HERE, "fragments.npz"))
    return [np.ascontiguousarray(frag[k].astype(np.float64)[::step]) for k in ("src", "src_normals", "tgt", "tgt_normals")], frag


def pair_table(src, tgt, init, rng):
    moved = src @ init[:3, :3].T + init[:3, 3]
    d2 = ((moved[:, None, :] - tgt[None, :, :]) ** 2).sum(2)
    nn = np.argmin(d2, axis=1).astype(np.int32)
    wrong = rng.random(len(src)) < 0.3
    nn[wrong] = rng.integers(0, len(tgt), int(wrong.sum()))
    return nn


def draw_sets(ns, rng):
    """every 12th set draws among the source points of `pairs` (the even indices below 1,200): its pairs are entries of the list"""
    sets = []
    pool = lambda: np.arange(600) * 2 if len(sets) % 12 == 0 else ns
    for n in (3, 4, 6, 8):
        for _ in range(56):
            sets.append(list(rng.choice(pool(), n, replace=False)))
    for _ in range(16):
        d = list(rng.choice(pool(), 3, replace=False))
        d.insert(int(rng.integers(0, 4)), d[int(rng.integers(0, 3))])
        sets.append(d)
    n = np.array([len(d) for d in sets], np.int32)
    out = np.full((len(sets), 8), -1, np.int32)
    for k, d in enumerate(sets):
        out[k, :len(d)] = d
    return out, n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--time", action="store_true")
    a = ap.parse_args()
    exe = build()
    (src, sn, tgt, tn), frag = clouds(3)
    radius = float(frag["radius"])
    rng = np.random.default_rng(20261019)
    nn = pair_table(src, tgt, frag["init"], rng)
    draws, draw_n = draw_sets(len(src), rng)
    pairs = np.stack([np.arange(600) * 2, nn[np.arange(600) * 2]], 1).astype(np.int32)
    corres_sets = (np.arange(20) * 12).astype(np.int32)
    inp, outp = os.path.join(SCRATCH, "in.bin"), os.path.join(SCRATCH, "out.bin")

    def head(f, arrs):
        f.write(struct.pack("<qq", len(arrs[0]), len(arrs[2])))
        for arr in arrs:
            f.write(np.ascontiguousarray(arr, "<f8").tobytes())

    with open(inp, "wb") as f:
        head(f, (src, sn, tgt, tn))
        f.write(struct.pack("<qqqdddd", len(draws), len(pairs), len(corres_sets), EDGE, radius, np.radians(ANGLE_DEG), MAX_DIST))
        f.write(nn.astype("<i4").tobytes())
        f.write(pairs.astype("<i4").tobytes())
        f.write(corres_sets.astype("<i4").tobytes())
        for k in range(len(draws)):
            f.write(struct.pack("<i8i", int(draw_n[k]), *[int(x) for x in np.maximum(draws[k], 0)]))
    subprocess.check_call([exe, "fixture", inp, outp])
    v = np.frombuffer(open(outp, "rb").read(), "<f8")
    per = v[:22 * len(draws)].reshape(len(draws), 22)
    cor = v[22 * len(draws):].reshape(len(corres_sets), 2)
    out = os.path.join(HERE, "ransac.npz")
    np.savez_compressed(out, nn=nn, draws=draws, draw_n=draw_n, T=per[:, :16].reshape(-1, 4, 4).copy(),
                        edge=per[:, 16].astype(np.int8), dist=per[:, 17].astype(np.int8), normal=per[:, 18].astype(np.int8),
                        count=per[:, 19].astype(np.int64), fitness=per[:, 20].copy(), rmse=per[:, 21].copy(), pairs=pairs,
                        corres_sets=corres_sets, corres_fitness=cor[:, 0].copy(), corres_rmse=cor[:, 1].copy(),
                        edge_similarity=EDGE, distance_threshold=radius, normal_angle=np.radians(ANGLE_DEG), max_dist=MAX_DIST)
    print("ransac.npz: %d bytes; verdicts passed: edge %d, distance %d, normal %d of %d; sets with a correspondence: %d; "
          "list fitness %s" % (os.path.getsize(out), per[:, 16].sum(), per[:, 17].sum(), per[:, 18].sum(), len(draws),
                               int((per[:, 19] > 0).sum()), np.round(cor[:, 0], 3)))
    if a.time:
        sys.path.insert(0, os.path.join(ROOT, "tools"))
        import ransac_probe as P
        (fsrc, fsn, ftgt, ftn), _ = clouds(1)
        with open(inp, "wb") as f:
            head(f, (fsrc, fsn, ftgt, ftn))
            f.write(struct.pack("<dddddiiii", P.FPFH_RADIUS, P.EDGE, P.DIST, np.radians(P.ANGLE_DEG), P.MAX_DIST, P.FPFH_MAX_NN,
                                P.RANSAC_N, P.MAX_ITERATION, P.MAX_VALIDATION))
        subprocess.check_call([exe, "time", inp, outp])
        r = np.frombuffer(open(outp, "rb").read(), "<f8")
        print("reference on this CPU (%d hardware threads, OpenMP): RegistrationRANSACBasedOnFeatureMatching, %d x %d points, "
              "ransac_n %d, %d iterations, %d validations, three checkers: %.1f ms (fitness %.4f, rmse %.5f)"
              % (os.cpu_count(), len(fsrc), len(ftgt), P.RANSAC_N, P.MAX_ITERATION, P.MAX_VALIDATION, r[0] * 1e3, r[1], r[2]))


if __name__ == "__main__":
    main()
