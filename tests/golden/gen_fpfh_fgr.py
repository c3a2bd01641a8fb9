"""Generate tests/golden/fpfh_fgr.npz: what the compiled reference computes for the inputs tests/test_fpfh_fgr.py pins its
numpy specification with.  Run once where the reference checkout exists; the fixture holds DATA only.

The generator writes a small harness of its own into a scratch directory, compiles it there together with the reference's
Feature.cpp, KDTreeFlann.cpp, PointCloud.cpp, Eigen.cpp, Console.cpp and Helper.cpp (the harness includes
FastGlobalRegistration.cpp itself: NormalizePointCloud, OptimizePairwiseRegistration and GetTransformationOriginalScale
live in its unnamed namespace), runs it and records
  fpfh_1200          (a) ComputeFPFHFeature(cloud, KDTreeSearchParamHybrid(0.25, 100)) of the first 1,200 points of
                         fragments.npz: src (with their normals) as a cloud of their own, (1200, 33), row i = column i
  pairs              (b) 600 fixed pairs (source index, target index) on the fragment pair: source point 6 k and the target
                         point nearest to it under fragments.npz: init (brute force, f64)
  T_opt, T_final         OptimizePairwiseRegistration(normalized clouds, pairs, scale_global, default options) and
                         GetTransformationOriginalScale(...).inverse(), row-major.  The reference's option constructor
                         leaves decrease_mu_ and maximum_correspondence_distance_ unset: the harness sets them to the
                         defaults its header declares (true, 0.025).
With --time it also times the reference on the inputs of tools/fpfh_fgr_probe.py (this machine's CPU; printed, not stored).
Nothing compiled and no reference text is kept."""
import argparse
import os
import struct
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "tools"))
REF = os.environ.get("VISMA_REF", "/root/reference")
O3D = os.path.join(REF, "thirdparty", "Open3D")
SCRATCH = os.environ.get("VISMA_SCRATCH") or tempfile.mkdtemp(prefix="fpfh_fgr_")      # outside the repository

HARNESS = r'''
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "%(o3d)s/src/Core/Registration/FastGlobalRegistration.cpp"
using namespace open3d;
static void rd(FILE *f, void *p, size_t n) { if (fread(p, 1, n, f) != n) std::exit(2); }
static void cloud(FILE *f, std::vector<Eigen::Vector3d> &v, long long n)
{
    v.resize((size_t)n);
    for (long long i = 0; i < n; i++) { double p[3]; rd(f, p, 24); v[(size_t)i] = Eigen::Vector3d(p[0], p[1], p[2]); }
}
static void mat(FILE *o, const Eigen::Matrix4d &M)
{
    for (int i = 0; i < 4; i++) for (int j = 0; j < 4; j++) { double v = M(i, j); fwrite(&v, 8, 1, o); }
}
static double now() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }
int main(int argc, char **argv)
{
    FILE *f = std::fopen(argv[2], "rb"), *o = std::fopen(argv[3], "wb");
    if (!f || !o) return 2;
    if (!std::strcmp(argv[1], "fixture")) {
        long long ns, nt, nsub, K;
        rd(f, &ns, 8); rd(f, &nt, 8); rd(f, &nsub, 8); rd(f, &K, 8);
        PointCloud src, tgt, sub;
        cloud(f, src.points_, ns); cloud(f, src.normals_, ns); cloud(f, tgt.points_, nt);
        std::vector<std::pair<int, int>> corres;
        for (long long c = 0; c < K; c++) { int p[2]; rd(f, p, 8); corres.push_back(std::make_pair(p[0], p[1])); }
        sub.points_.assign(src.points_.begin(), src.points_.begin() + nsub);
        sub.normals_.assign(src.normals_.begin(), src.normals_.begin() + nsub);
        auto feat = ComputeFPFHFeature(sub, KDTreeSearchParamHybrid(0.25, 100));
        for (long long i = 0; i < nsub; i++) for (int j = 0; j < 33; j++) { double v = feat->data_(j, i); fwrite(&v, 8, 1, o); }
        FastGlobalRegistrationOption option;
        option.decrease_mu_ = true;
        option.maximum_correspondence_distance_ = 0.025;
        std::vector<PointCloud> vec; vec.push_back(src); vec.push_back(tgt);
        double scale_global, scale_start;
        std::vector<Eigen::Vector3d> means;
        std::tie(means, scale_global, scale_start) = NormalizePointCloud(vec, option);
        Eigen::Matrix4d t = OptimizePairwiseRegistration(vec, corres, scale_global, option);
        mat(o, t);
        mat(o, GetTransformationOriginalScale(t, means, scale_global).inverse());
    } else if (!std::strcmp(argv[1], "fpfh")) {                 // a cloud with normals -> its FPFH, point-major, then the seconds
        long long n; double radius; int max_nn;
        rd(f, &n, 8); rd(f, &radius, 8); rd(f, &max_nn, 4);
        PointCloud c;
        cloud(f, c.points_, n); cloud(f, c.normals_, n);
        double t0 = now();
        auto feat = ComputeFPFHFeature(c, KDTreeSearchParamHybrid(radius, max_nn));
        double t1 = now() - t0;
        for (long long i = 0; i < n; i++) for (int j = 0; j < 33; j++) { double v = feat->data_(j, i); fwrite(&v, 8, 1, o); }
        fwrite(&t1, 8, 1, o);
    } else {                                                    // two sets of m feature rows -> seconds of AdvancedMatching's
        long long m;                                            // search (tree over fa, SearchKNN(., 1) per row of fb), index sum
        rd(f, &m, 8);
        Feature fa, fb;
        fa.Resize(33, (int)m); fb.Resize(33, (int)m);
        for (long long i = 0; i < m; i++) for (int j = 0; j < 33; j++) { double v; rd(f, &v, 8); fa.data_(j, i) = v; }
        for (long long i = 0; i < m; i++) for (int j = 0; j < 33; j++) { double v; rd(f, &v, 8); fb.data_(j, i) = v; }
        double t0 = now();
        KDTreeFlann tree(fa);
        std::vector<int> k; std::vector<double> d;
        long long sum = 0;
        for (long long j = 0; j < m; j++) { tree.SearchKNN(Eigen::VectorXd(fb.data_.col(j)), 1, k, d); sum += k[0]; }
        double r[2] = {now() - t0, (double)sum};
        fwrite(r, 8, 2, o);
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
           "-I" + os.path.join(O3D, "3rdparty"), "-I" + O3D, src, os.path.join(core, "Registration", "Feature.cpp"),
           os.path.join(core, "Geometry", "KDTreeFlann.cpp"), os.path.join(core, "Geometry", "PointCloud.cpp"),
           os.path.join(core, "Utility", "Eigen.cpp"), os.path.join(core, "Utility", "Console.cpp"),
           os.path.join(core, "Utility", "Helper.cpp"), "-o", exe]
    subprocess.check_call(cmd)
    return exe


def fixed_pairs(frag):
    src, tgt, init = frag["src"].astype(np.float64), frag["tgt"].astype(np.float64), frag["init"]
    si = np.arange(600) * 6
    moved = src[si] @ init[:3, :3].T + init[:3, 3]
    d2 = ((moved[:, None, :] - tgt[None, :, :]) ** 2).sum(2)
    return np.stack([si, np.argmin(d2, axis=1)], 1).astype(np.int32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--time", action="store_true")
    a = ap.parse_args()
    exe = build()
    frag = np.load(os.path.join(HERE, "fragments.npz"))
    src, sn, tgt = (frag[k].astype(np.float64) for k in ("src", "src_normals", "tgt"))
    pairs = fixed_pairs(frag)
    inp, outp = os.path.join(SCRATCH, "in.bin"), os.path.join(SCRATCH, "out.bin")
    with open(inp, "wb") as f:
        f.write(struct.pack("<qqqq", len(src), len(tgt), 1200, len(pairs)))
        for arr in (src, sn, tgt):
            f.write(np.ascontiguousarray(arr, "<f8").tobytes())
        f.write(np.ascontiguousarray(pairs, "<i4").tobytes())
    subprocess.check_call([exe, "fixture", inp, outp])
    v = np.frombuffer(open(outp, "rb").read(), "<f8")
    fpfh = v[:1200 * 33].reshape(1200, 33).copy()
    T_opt, T_final = v[1200 * 33:1200 * 33 + 16].reshape(4, 4).copy(), v[1200 * 33 + 16:].reshape(4, 4).copy()
    np.savez_compressed(os.path.join(HERE, "fpfh_fgr.npz"), fpfh_1200=fpfh, pairs=pairs, T_opt=T_opt, T_final=T_final)
    print("fpfh_fgr.npz: %d bytes; T_final =\n%s" % (os.path.getsize(os.path.join(HERE, "fpfh_fgr.npz")), T_final))
    if a.time:
        import fpfh_fgr_probe as P

        def ref_fpfh(cloud, radius):
            with open(inp, "wb") as f:
                f.write(struct.pack("<qdi", len(cloud[0]), radius, P.FPFH_MAX_NN))
                f.write(cloud[0].tobytes()); f.write(cloud[1].tobytes())
            subprocess.check_call([exe, "fpfh", inp, outp])
            v = np.frombuffer(open(outp, "rb").read(), "<f8")
            return v[:-1].reshape(-1, 33), float(v[-1])

        feat, sec = ref_fpfh(P.probe_cloud(P.FPFH_N, 1), P.FPFH_RADIUS)
        print("reference on this CPU (%d hardware threads, OpenMP): FPFH n = %d Hybrid(%g, %d): %.1f ms (checksum %.6f)"
              % (os.cpu_count(), P.FPFH_N, P.FPFH_RADIUS, P.FPFH_MAX_NN, sec * 1e3, feat.sum()))
        fa = ref_fpfh(P.probe_cloud(P.MATCH_N, 2), P.MATCH_RADIUS)[0]
        fb = ref_fpfh(P.probe_cloud(P.MATCH_N, 3), P.MATCH_RADIUS)[0]
        with open(inp, "wb") as f:
            f.write(struct.pack("<q", P.MATCH_N))
            f.write(np.ascontiguousarray(fa).tobytes()); f.write(np.ascontiguousarray(fb).tobytes())
        subprocess.check_call([exe, "match", inp, outp])
        r = np.frombuffer(open(outp, "rb").read(), "<f8")
        print("reference on this CPU (one thread, as AdvancedMatching runs it): matching %d x %d x 33, KD-tree build + SearchKNN "
              "per row: %.1f ms (index sum %d)" % (P.MATCH_N, P.MATCH_N, r[0] * 1e3, int(r[1])))

if __name__ == "__main__":
    main()
