"""Generate tests/golden/cloud.npz: what the compiled reference's PointCloud (GetMinBound / GetMaxBound, Transform,
NormalizeNormals, PaintUniformColor, operator+=), DownSample.cpp (SelectDownSample, UniformDownSample, CropPointCloud),
EstimateNormals.cpp (the two OrientNormals*) and PointCloud.cpp's ComputePointCloudMeanAndCovariance and
ComputePointCloudMahalanobisDistance make of the programs of tests/cloud_cases.py.  tests/test_cloud_spec.py pins the numpy
specification (tests/cloud_spec.py) with it, and tests/test_cloud.py the library with the specification.  Run once where the
reference checkout exists; the fixture holds DATA only.

The generator writes a small harness of its own into a scratch directory outside the repository, compiles it there against
the reference's Core/Geometry (PointCloud.cpp, DownSample.cpp, EstimateNormals.cpp, KDTreeFlann.cpp, TriangleMesh.cpp) and
Core/Utility, runs it and records per case <c> and program <p>:

  <c>_<p>_counts           n, has normals, has colours (the reference's HasX()), the number of result doubles
  <c>_<p>_sha              SHA-256 of the raw rows and results (tests/cloud_cases.py: raw_rows)
  <c>_<p>_<attribute>      ... and the rows in full (as their uint64 bits), where n <= cloud_cases.FULL_ROWS
  <c>_<p>_results          the results of the bounds / meancov / mahal steps in full, where they are at most that many doubles
Bits are compared as cloud_cases.bits gives them: every NaN as one pattern.

It asserts the properties that make each case bite (a case cannot silently stop testing anything), and that the
specification equals the reference bit for bit (the tests repeat that from the fixture).

--time FILE.npz prints the reference's one-thread time of the chain crop, VoxelDownSample, EstimateNormals(Hybrid) on the
cloud saved there by tools/cloud_probe.py (points, normals, colors, lo, hi, voxel, radius, max_nn); printed, not stored.
Nothing compiled and no reference text is kept."""
import argparse
import hashlib
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = os.environ.get("VISMA_REF", "/root/reference")
O3D = os.path.join(REF, "thirdparty", "Open3D")
SCRATCH = os.environ.get("VISMA_SCRATCH") or tempfile.mkdtemp(prefix="cloud_")        # outside the repository
sys.path.insert(0, os.path.join(ROOT, "tests"))
import cloud_spec as S  # noqa: E402
import cloud_cases as cases  # noqa: E402

HARNESS = r'''
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <tuple>
#include <vector>
#include <Core/Geometry/PointCloud.h>
#include <Core/Geometry/KDTreeSearchParam.h>
using namespace open3d;
static double rd(FILE *f) { double v; if (fread(&v, 8, 1, f) != 1) std::exit(2); return v; }
static void wd(FILE *o, double v) { fwrite(&v, 8, 1, o); }
static double now() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }
static void rows(FILE *f, std::vector<Eigen::Vector3d> &a, size_t n) { a.resize(n); for (auto &p : a) { p(0) = rd(f); p(1) = rd(f); p(2) = rd(f); } }
static void wrows(FILE *o, const std::vector<Eigen::Vector3d> &a) { wd(o, (double)a.size()); for (auto &p : a) { wd(o, p(0)); wd(o, p(1)); wd(o, p(2)); } }
static Eigen::Vector3d vec(FILE *f) { Eigen::Vector3d v; v(0) = rd(f); v(1) = rd(f); v(2) = rd(f); return v; }
static void cloud(FILE *f, PointCloud &c)
{
    const size_t n = (size_t)rd(f);
    const bool hn = rd(f) != 0, hc = rd(f) != 0;
    rows(f, c.points_, n);
    if (hn) rows(f, c.normals_, n);
    if (hc) rows(f, c.colors_, n);
}
int main(int argc, char **argv)
{
    FILE *f = std::fopen(argv[1], "rb"), *o = std::fopen(argv[2], "wb");
    if (!f || !o) return 2;
    PointCloud m;
    cloud(f, m);
    const int nops = (int)rd(f);
    std::vector<double> results, times;
    for (int k = 0; k < nops; k++) {
        const int op = (int)rd(f);
        Eigen::Matrix4d M;
        Eigen::Vector3d a, b;
        PointCloud other;
        std::vector<size_t> idx;
        bool self = false;
        double x = 0.0, y = 0.0;
        switch (op) {                                        // the arguments first: only the call is timed
        case 0: for (int i = 0; i < 16; i++) M(i / 4, i % 4) = rd(f); break;
        case 2: case 8: case 9: a = vec(f); break;
        case 3: self = rd(f) != 0; if (!self) cloud(f, other); break;
        case 5: idx.resize((size_t)rd(f)); for (auto &i : idx) i = (size_t)rd(f); break;
        case 6: case 12: x = rd(f); break;
        case 7: a = vec(f); b = vec(f); break;
        case 13: x = rd(f); y = rd(f); break;
        default: break;
        }
        const double s = now();
        switch (op) {
        case 0: m.Transform(M); break;
        case 1: m.NormalizeNormals(); break;
        case 2: m.PaintUniformColor(a); break;
        case 3: if (self) m += m; else m += other; break;
        case 4: { const Eigen::Vector3d lo = m.GetMinBound(), hi = m.GetMaxBound();
                  for (int i = 0; i < 3; i++) results.push_back(lo(i));
                  for (int i = 0; i < 3; i++) results.push_back(hi(i));
                  break; }
        case 5: { auto out = SelectDownSample(m, idx); m = *out; break; }
        case 6: { auto out = UniformDownSample(m, (size_t)x); m = *out; break; }
        case 7: { auto out = CropPointCloud(m, a, b); m = *out; break; }
        case 8: OrientNormalsToAlignWithDirection(m, a); break;
        case 9: OrientNormalsTowardsCameraLocation(m, a); break;
        case 10: { Eigen::Vector3d mean; Eigen::Matrix3d cov;
                   std::tie(mean, cov) = ComputePointCloudMeanAndCovariance(m);
                   for (int i = 0; i < 3; i++) results.push_back(mean(i));
                   for (int i = 0; i < 9; i++) results.push_back(cov(i / 3, i % 3));
                   break; }
        case 11: { const std::vector<double> d = ComputePointCloudMahalanobisDistance(m); results.insert(results.end(), d.begin(), d.end()); break; }
        case 12: { auto out = VoxelDownSample(m, x); m = *out; break; }
        case 13: EstimateNormals(m, KDTreeSearchParamHybrid(x, (int)y)); break;
        default: return 3;
        }
        times.push_back(now() - s);
    }
    wrows(o, m.points_); wrows(o, m.normals_); wrows(o, m.colors_);
    wd(o, (double)m.HasNormals()); wd(o, (double)m.HasColors());
    wd(o, (double)results.size()); for (double r : results) wd(o, r);
    wd(o, (double)times.size()); for (double r : times) wd(o, r);
    std::fclose(o);
    return 0;
}
'''


def build():
    os.makedirs(SCRATCH, exist_ok=True)
    src = os.path.join(SCRATCH, "harness.cpp")
    with open(src, "w") as f:
        f.write(HARNESS)
    exe = os.path.join(SCRATCH, "harness")
    core = os.path.join(O3D, "src", "Core")
    cmd = ["g++", "-std=c++11", "-O2", "-fopenmp", "-w", "-ffunction-sections", "-fdata-sections", "-Wl,--gc-sections",
           "-I" + os.path.join(O3D, "src"), "-I" + os.path.join(O3D, "3rdparty", "Eigen"), "-I" + os.path.join(O3D, "3rdparty"), "-I" + O3D,
           "-I" + os.path.join(O3D, "3rdparty", "flann"), src]
    cmd += [os.path.join(core, "Geometry", n + ".cpp") for n in ("PointCloud", "DownSample", "EstimateNormals", "KDTreeFlann", "TriangleMesh")]
    cmd += [os.path.join(core, "Utility", n + ".cpp") for n in ("Eigen", "Console", "Helper")]
    subprocess.check_call(cmd + ["-o", exe])
    return exe


def reference(exe, c, program, threads=None):
    """-> the reference's cloud (a specification dict), the results of its steps as one f64 array, the seconds each step took"""
    inp, outp = os.path.join(SCRATCH, "in.bin"), os.path.join(SCRATCH, "out.bin")
    with open(inp, "wb") as f:
        f.write(cases.encode(c, program))
    env = dict(os.environ)
    if threads:
        env["OMP_NUM_THREADS"] = str(threads)
    subprocess.check_call([exe, inp, outp], stdout=subprocess.DEVNULL, env=env)
    v = np.frombuffer(open(outp, "rb").read(), "<f8")
    at = [0]

    def take(n):
        out = v[at[0]:at[0] + n]
        assert len(out) == n
        at[0] += n
        return out

    def rows():
        n = int(take(1)[0])
        return take(3 * n).reshape(n, 3).copy()

    pts, nrm, col = rows(), rows(), rows()
    has = [bool(x) for x in take(2)]
    out = dict(points=pts, normals=nrm if has[0] else None, colors=col if has[1] else None)
    results = take(int(take(1)[0])).copy()
    times = take(int(take(1)[0])).tolist()
    assert at[0] == len(v)
    return out, results, times


def same_bits(a, b):
    return a.shape == b.shape and cases.bits(a).tobytes() == cases.bits(b).tobytes()


def bite(name, results):
    """the properties that make a case test something, on the REFERENCE's results"""
    c, programs = cases.load()[name]
    ref = lambda p: results[p][0]
    res = lambda p: results[p][1]
    n = len(c["points"])
    if name.startswith("tile"):
        masks = []
        for p, program in enumerate(programs):
            lo, hi = np.asarray(program[0][1]), np.asarray(program[0][2])
            with np.errstate(invalid="ignore"):
                inside = ((c["points"] >= lo) & (c["points"] <= hi)).all(axis=1) & ~(lo > hi).any()
            assert len(ref(p)["points"]) == np.count_nonzero(inside), (name, p)
            assert ref(p)["normals"] is not None or len(ref(p)["points"]) == 0
            masks.append(inside)
        # programs 0 and 4 keep and drop a row within a wave of either side of every tile border, and in the last wave
        for border in list(range(256, n, 256)) + [n]:
            for lo_i, hi_i in ((max(border - 64, 0), border), (border, border + 64)):
                parts = [masks[p][lo_i:hi_i] for p in (0, 4)]
                assert len(parts[0]) == 0 or (any(m.any() for m in parts) and any(not m.all() for m in parts)), (name, border)
                assert len(parts[0]) < 2 or (parts[0].any() and not parts[0].all()), (name, border)
        assert len(ref(1)["points"]) == n - 1 and len(ref(2)["points"]) == n - 1      # the NaN point alone fails
        assert len(ref(3)["points"]) == 0 and len(ref(5)["points"]) == 0 and len(ref(6)["points"]) == 0
        on = ref(4)["points"]                                # rows ON each bound were kept
        assert 0 < len(on) < n // 2 and (on[:, 0] == 0.25).all()
        assert (on[:, 1] == 0.5).any() and (on[:, 1] == 1.25).any() and (on[:, 2] == 0.25).any() and (on[:, 2] == 1.75).any()
    if name == "big":
        assert n == 524288 + 257 and n // 2 < len(ref(0)["points"]) * 7 < n
        assert not np.array_equal(res(0)[:6], res(0)[6:])
    if name.startswith("sums"):
        serial, chunked = S.mean_and_covariance(c)[2], S.mean_and_covariance(c, cases.CHUNK)[2]
        if n <= cases.CHUNK + 1:                             # (a second chunk of one point is added as in the serial order)
            assert serial.tobytes() == chunked.tobytes(), name
        else:
            assert serial.tobytes() != chunked.tobytes(), name
        if n == 2 * cases.CHUNK + 1:                         # ... and the difference reaches the results
            assert S.run(c, programs[0], cases.CHUNK)[1][0].tobytes() != res(0).tobytes()
        mag = np.abs(c["points"]).max(axis=1)
        assert mag.max() / mag.min() > 2.0 ** 50
        assert np.isfinite(res(1)).all() and (res(1) > 0).all()
    if name == "planar":
        assert not np.isfinite(res(1)).all() and res(0)[3 + 8] == 0.0
    if name == "bounds_nan_first":
        assert np.isnan(res(0)[[0, 3]]).all() and not np.isnan(res(0)[[1, 2, 4, 5]]).any()      # x starts with the NaN; y and z do not
    if name == "bounds_nan_middle":
        assert not np.isnan(res(0)).any()
    if name == "bounds_all_nan":
        assert np.isnan(res(0)).all()
    if name == "bounds_zero_pos_first":
        assert (res(0)[[0, 3]] == 0.0).all() and not np.signbit(res(0)[[0, 3]]).any() and np.signbit(res(0)[[1, 4]]).all()
    if name == "bounds_zero_neg_first":
        assert np.signbit(res(0)[[0, 3]]).all() and not np.signbit(res(0)[[1, 4]]).any()
    if name == "bounds_inf":
        assert (res(0)[:3] == -np.inf).all() and (res(0)[3:] == np.inf).all()
    if name == "bounds_last_max":
        assert res(0)[3] == 77.0 and c["points"][-1, 0] == 77.0 and n % 64 != 0 and n > 256
    if name == "bounds_last_min":
        assert res(0)[0] == -77.0 and c["points"][-1, 0] == -77.0
    if name == "select":
        assert len(ref(0)["points"]) == 7 and same_bits(ref(0)["points"][0], ref(0)["points"][1])
        assert same_bits(ref(1)["colors"], c["colors"][::-1]) and len(ref(2)["points"]) == 0 and len(ref(3)["points"]) == 3 * n
    if name == "uniform":
        assert [len(ref(p)["points"]) for p in range(6)] == [0, n, 12, 2, 1, 1]
        assert same_bits(ref(3)["points"], c["points"][[0, n - 1]])
    if name.startswith("append_"):
        lhs = name[7:]
        for j, rhs in enumerate(cases.KINDS):
            want_n = rhs != "empty" and (lhs == "empty" or lhs in ("normals", "both")) and rhs in ("normals", "both")
            want_c = rhs != "empty" and (lhs == "empty" or lhs in ("colors", "both")) and rhs in ("colors", "both")
            if rhs == "empty":                               # nothing changes, not even the attributes
                want_n, want_c = lhs in ("normals", "both"), lhs in ("colors", "both")
            assert ((ref(j)["normals"] is not None), (ref(j)["colors"] is not None)) == (want_n, want_c), (name, rhs)
            assert len(ref(j)["points"]) == n + (0 if rhs == "empty" else 4)
        assert len(ref(5)["points"]) == 2 * n
    if name == "transform":
        assert np.isnan(ref(1)["normals"][:, 1]).all() and not np.isnan(ref(1)["normals"][:, 0]).any()   # T_13 * 0 reaches the normals
        assert np.isnan(ref(2)["normals"][:, 0]).all() and np.isinf(ref(2)["points"][:, 0]).all()
        assert same_bits(ref(0)["colors"], c["colors"])
    if name == "normals":
        nn = ref(0)["normals"]
        assert nn[0].tolist() == [0, 0, 0] and nn[1].tolist() == [1e-200, 1e-200, 0] and nn[2].tolist() == [0, 0, 0]
        assert np.isnan(nn[3, 0]) and nn[3, 1] == 1.0 and np.isnan(nn[7, 0]) and nn[7, 1] == 0.0      # no (0, 0, 1) rule here
        d = ref(1)["normals"]
        assert d[0].tolist() == [0, 0, 1] and d[1].tolist() == [0, 0, 1] and d[9].tolist() == [3, 4, 12] and d[10].tolist() == [0, 0, 1]    # (1e-170)^2 underflows: norm() == 0
        cam = ref(5)["normals"]
        assert cam[8].tolist() == [0, 0, 1] and abs(np.linalg.norm(cam[0]) - 1.0) < 1e-15
        tiny = ref(7)["normals"]
        assert tiny[14].tolist() == [0, 0, 1] and tiny[0].tolist() != [0, 0, 1]          # camera - point is not zero, its squared norm is


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--time", metavar="FILE.npz", help="points (normals, colors), lo, hi, voxel, radius, max_nn: the chain to time the reference on")
    args = ap.parse_args()
    exe = build()
    if args.time:
        z = np.load(args.time)
        c = S.cloud(z["points"], z["normals"] if "normals" in z.files else None, z["colors"] if "colors" in z.files else None)
        program = [("crop", z["lo"], z["hi"]), ("voxel", float(z["voxel"])), ("normals", float(z["radius"]), int(z["max_nn"]))]
        out, _, t = reference(exe, c, program, threads=1)
        print("reference on this CPU (one thread), %d points: crop %.1f ms, VoxelDownSample %.1f ms, EstimateNormals(Hybrid) %.1f ms, "
              "chain %.1f ms -> %d points" % (len(c["points"]), t[0] * 1e3, t[1] * 1e3, t[2] * 1e3, sum(t) * 1e3, len(out["points"])))
        return
    fix = {}
    for name in cases.NAMES:
        c, programs = cases.load()[name]
        results = []
        for p, program in enumerate(programs):
            ref, res, _ = reference(exe, c, program)
            results.append((ref, res))
            mine, mine_res = cases.spec(name, p)
            mine_res = cases.flat_results(mine_res)
            assert same_bits(mine_res, res), (name, p, mine_res[:12], res[:12], np.nonzero(cases.bits(mine_res) != cases.bits(res))[0][:5])
            for k in S.ATTRS:
                assert (mine[k] is None) == (ref[k] is None), (name, p, k)
                if ref[k] is not None:
                    assert mine[k].shape == ref[k].shape, (name, p, k)
                    bad = np.nonzero((cases.bits(mine[k]) != cases.bits(ref[k])).any(axis=1))[0]
                    assert len(bad) == 0, (name, p, k, bad[:5], mine[k][bad[:3]], ref[k][bad[:3]])
            key = "%s_%d_" % (name, p)
            fix[key + "counts"] = np.array([len(ref["points"]), ref["normals"] is not None, ref["colors"] is not None, len(res)], np.int64)
            fix[key + "sha"] = np.frombuffer(hashlib.sha256(cases.raw_rows(ref, [res])).digest(), np.uint8).copy()
            if len(ref["points"]) <= cases.FULL_ROWS:
                for k in S.ATTRS:
                    if ref[k] is not None:
                        fix[key + k] = cases.bits(ref[k])
            if 0 < len(res) <= cases.FULL_ROWS:
                fix[key + "results"] = cases.bits(res)
            print("%s program %d: %d points, %d result doubles" % (name, p, len(ref["points"]), len(res)))
        bite(name, results)
    out = os.path.join(HERE, "cloud.npz")
    np.savez_compressed(out, **fix)
    print("cloud.npz: %d bytes" % os.path.getsize(out))
    if os.path.getsize(out) > 512 * 1024:
        raise SystemExit("the fixture is larger than 512 KB")


if __name__ == "__main__":
    main()
