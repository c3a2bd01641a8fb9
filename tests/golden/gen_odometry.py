"""Generate tests/golden/odometry.npz: what the compiled reference computes for the inputs tests/test_odometry.py pins its
numpy specification (tests/odometry_spec.py) and the library with.  Run once where the reference checkout exists; the
fixture holds DATA only.

The generator writes a small harness of its own into a scratch directory outside the repository, compiles it there (the
harness includes the reference's Odometry.cpp itself: InitializeRGBDOdometry, ComputeCorrespondence, DoSingleIteration and
CreateInformationMatrix live in its unnamed namespace) together with RGBDOdometryJacobian.cpp, Image.cpp, ImageFactory.cpp,
RGBDImage.cpp, RGBDImageFactory.cpp, Camera/PinholeCameraIntrinsic.cpp, Utility/{Eigen,Console,Helper,IJsonConvertible}.cpp
and jsoncpp, runs it and records three cases:

  A  100 x 75 frames of tests/odometry_scene.py, 3 levels (50 x 37, 25 x 18):
       a_src_gray .. a_tgt_depth, a_intrinsic, a_init            the input
       a_l<l>_<which>                the processed pyramid images (level 0: the four gray / depth images in full, the
                                     gradients and the xyz image as SHA-256 digests a_l0_<which>_sha of the fp32 bytes with
                                     every NaN canonical -- the fixture's size; src_xyz holds x and y: z is the depth)
       a_l<l>_idx                    the correspondences at init
       a_l<l>_m<m>_<p>_{JTJ,JTr,r2,rows}   one step per level and method (0 colour, 1 hybrid) at p = init and final
       a_final                       the pose the steps "final" are taken at (the hybrid run's result)
       a_hybrid_{poses,counts,ok}    the hybrid run with the default schedule, per iteration
       a_hybrid_{T,info}_<1|3>, a_hybrid_ok_<1|3>     ComputeRGBDOdometry with 1 and with 3 OpenMP threads
       a_color_*                     the same for the colour term with the schedule {3} at one level
  B  7 x 5, 1 level, depths that become NaN and a pixel on every border: images and one step per method (b_*)
  C  A's frames with the source depth all 5.0 (beyond max_depth): c_ok_1 = 0

It refuses a fixture where the specification's trace has a correspondence decision (the truncation of u_t and v_t, the image
border, the depth-difference test) closer than 1e-9 relative to its boundary, or a solve whose determinant is within a
factor 10 of the 1e-6 guard: such a fixture pins rounding, not the algorithm.  The normalisation: a pixel's f64 product
0.5 / mean * p within 1e-10 relative of an fp32 rounding midpoint is refused UNLESS the mean has one value whatever the
order of its sum (sums_exactly: the grays are fp32 values of similar magnitude, so every partial sum in f64 is exact) --
with 15,000 pixels some product always lies that close to a midpoint (the expected count is about 50), and with an exact
mean the product and its cast are single correctly rounded operations on both sides.

With --time it also times the reference's ComputeRGBDOdometry on the 640 x 480 input of tools/odometry_probe.py (this
machine's CPU; printed, not stored).  Nothing compiled and no reference text is kept."""
import argparse
import os
import struct
import subprocess
import sys
import tempfile
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = os.environ.get("VISMA_REF", "/root/reference")
O3D = os.path.join(REF, "thirdparty", "Open3D")
SCRATCH = os.environ.get("VISMA_SCRATCH") or tempfile.mkdtemp(prefix="odometry_")      # outside the repository
sys.path.insert(0, os.path.join(ROOT, "tests"))
import odometry_scene as scene  # noqa: E402
import odometry_spec as S  # noqa: E402

HARNESS = r'''
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include <omp.h>
#include "%(o3d)s/src/Core/Odometry/Odometry.cpp"
using namespace open3d;
static void rd(FILE *f, void *p, size_t n) { if (fread(p, 1, n, f) != n) std::exit(2); }
static void wd(FILE *o, double v) { fwrite(&v, 8, 1, o); }
static void img(FILE *f, Image &im, int W, int H) { im.PrepareImage(W, H, 1, 4); rd(f, im.data_.data(), (size_t)W * H * 4); }
static void wimg(FILE *o, const Image &im)
{
    const float *p = (const float *)im.data_.data();
    for (size_t i = 0; i < (size_t)im.width_ * im.height_ * im.num_of_channels_; i++) wd(o, (double)p[i]);
}
static void w4(FILE *o, const Eigen::Matrix4d &T) { for (int i = 0; i < 16; i++) wd(o, T(i / 4, i %% 4)); }
static double now() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

struct Pyr {
    RGBDImagePyramid s, t, dx, dy;
    std::vector<std::shared_ptr<Image>> xyz;
    std::vector<Eigen::Matrix3d> K;
};
static Pyr pyramids(const RGBDImage &sp, const RGBDImage &tp, const PinholeCameraIntrinsic &cam, int n)
{
    Pyr p;
    p.s = CreateRGBDImagePyramid(sp, n); p.t = CreateRGBDImagePyramid(tp, n);
    p.dx = FilterRGBDImagePyramid(p.t, Image::FilterType::Sobel3Dx); p.dy = FilterRGBDImagePyramid(p.t, Image::FilterType::Sobel3Dy);
    p.K = CreateCameraMatrixPyramid(cam, n);
    for (int l = 0; l < n; l++) p.xyz.push_back(ConvertDepthImageToXYZImage(p.s[l]->depth_, p.K[l]));
    return p;
}
static void step(FILE *o, const Pyr &p, int l, const Eigen::Matrix4d &T, int method, const OdometryOption &opt)
{
    auto c = ComputeCorrespondence(p.K[l], T, p.s[l]->depth_, p.t[l]->depth_, opt);
    RGBDOdometryJacobianFromColorTerm jc; RGBDOdometryJacobianFromHybridTerm jh;
    const RGBDOdometryJacobian &j = method == 0 ? (const RGBDOdometryJacobian &)jc : (const RGBDOdometryJacobian &)jh;
    Eigen::Matrix6d JTJ = Eigen::Matrix6d::Zero(); Eigen::Vector6d JTr = Eigen::Vector6d::Zero();
    double r2 = 0.0; long long rows = 0;
    std::vector<Eigen::Vector6d> J; std::vector<double> r;
    for (int i = 0; i < (int)c->size(); i++) {
        j.ComputeJacobianAndResidual(i, J, r, *p.s[l], *p.t[l], *p.xyz[l], *p.dx[l], *p.dy[l], p.K[l], T, *c);
        for (size_t k = 0; k < r.size(); k++) { JTJ += J[k] * J[k].transpose(); JTr += J[k] * r[k]; r2 += r[k] * r[k]; rows++; }
    }
    for (int i = 0; i < 36; i++) wd(o, JTJ(i / 6, i %% 6));
    for (int i = 0; i < 6; i++) wd(o, JTr(i));
    wd(o, r2); wd(o, (double)rows);
}
// ComputeMultiscale with its trajectory: the pose and the pair count of every iteration
static bool run(FILE *o, const Pyr &p, const Eigen::Matrix4d &init, int method, const OdometryOption &opt, Eigen::Matrix4d &out)
{
    RGBDOdometryJacobianFromColorTerm jc; RGBDOdometryJacobianFromHybridTerm jh;
    const RGBDOdometryJacobian &j = method == 0 ? (const RGBDOdometryJacobian &)jc : (const RGBDOdometryJacobian &)jh;
    const std::vector<int> &its = opt.iteration_number_per_pyramid_level_;
    const int n = (int)its.size();
    Eigen::Matrix4d T = init.isZero() ? Eigen::Matrix4d::Identity() : init;
    std::vector<double> rec;
    bool ok = true;
    for (int l = n - 1; l >= 0 && ok; l--)
        for (int it = 0; it < its[n - l - 1] && ok; it++) {
            auto c = ComputeCorrespondence(p.K[l], T, p.s[l]->depth_, p.t[l]->depth_, opt);
            Eigen::Matrix4d cur;
            std::tie(ok, cur) = DoSingleIteration(it, l, *p.s[l], *p.t[l], *p.xyz[l], *p.dx[l], *p.dy[l], p.K[l], T, j, opt);
            T = cur * T;
            rec.push_back((double)c->size());
            for (int i = 0; i < 16; i++) rec.push_back(T(i / 4, i %% 4));
        }
    wd(o, ok ? 1.0 : 0.0); wd(o, (double)(rec.size() / 17));
    for (double v : rec) wd(o, v);
    out = ok ? T : init;
    return ok;
}
int main(int argc, char **argv)
{
    FILE *f = std::fopen(argv[2], "rb"), *o = std::fopen(argv[3], "wb");
    if (!f || !o) return 2;
    int W, H, n, nc; double k[4], init16[16], od[3];
    rd(f, &W, 4); rd(f, &H, 4); rd(f, k, 32); rd(f, init16, 128);
    rd(f, &n, 4); std::vector<int> its((size_t)n); rd(f, its.data(), 4 * (size_t)n);
    rd(f, &nc, 4); std::vector<int> itc((size_t)nc); rd(f, itc.data(), 4 * (size_t)nc);
    rd(f, od, 24);
    Eigen::Matrix4d init; for (int i = 0; i < 16; i++) init(i / 4, i %% 4) = init16[i];
    RGBDImage s, t; img(f, s.color_, W, H); img(f, s.depth_, W, H); img(f, t.color_, W, H); img(f, t.depth_, W, H);
    PinholeCameraIntrinsic cam(W, H, k[0], k[1], k[2], k[3]);
    OdometryOption opt(its, od[0], od[1], od[2]), optc(itc, od[0], od[1], od[2]);
    if (!std::strcmp(argv[1], "time")) {
        double t0 = now();
        bool ok; Eigen::Matrix4d T; Eigen::Matrix6d I;
        std::tie(ok, T, I) = ComputeRGBDOdometry(s, t, cam, init, RGBDOdometryJacobianFromHybridTerm(), opt);
        wd(o, now() - t0); wd(o, ok ? 1.0 : 0.0); wd(o, I(5, 5));
        std::fclose(o);
        return 0;
    }
    omp_set_num_threads(1);
    std::shared_ptr<RGBDImage> sp, tp;
    std::tie(sp, tp) = InitializeRGBDOdometry(s, t, cam, init, opt);
    Pyr p = pyramids(*sp, *tp, cam, n);
    for (int l = 0; l < n; l++) {
        wd(o, (double)p.s[l]->color_.width_); wd(o, (double)p.s[l]->color_.height_);
        wimg(o, p.s[l]->color_); wimg(o, p.s[l]->depth_); wimg(o, p.t[l]->color_); wimg(o, p.t[l]->depth_);
        wimg(o, p.dx[l]->color_); wimg(o, p.dy[l]->color_); wimg(o, p.dx[l]->depth_); wimg(o, p.dy[l]->depth_);
        wimg(o, *p.xyz[l]);
        auto c = ComputeCorrespondence(p.K[l], init, p.s[l]->depth_, p.t[l]->depth_, opt);
        const int w = p.s[l]->color_.width_, h = p.s[l]->color_.height_;
        std::vector<double> idx((size_t)w * h, -1.0);
        for (auto &e : *c) idx[(size_t)e(1) * w + e(0)] = (double)(e(3) * w + e(2));
        for (double v : idx) wd(o, v);
    }
    Eigen::Matrix4d fin;
    run(o, p, init, 1, opt, fin);
    w4(o, fin);
    for (int l = 0; l < n; l++)
        for (int m = 0; m < 2; m++) { step(o, p, l, init, m, opt); step(o, p, l, fin, m, opt); }
    const int threads[2] = {1, 3};
    for (int m = 1; m >= 0; m--) {
        if (m == 0) { Pyr pc = pyramids(*sp, *tp, cam, nc); Eigen::Matrix4d e; run(o, pc, init, 0, optc, e); }
        for (int q = 0; q < 2; q++) {
            omp_set_num_threads(threads[q]);
            bool ok; Eigen::Matrix4d T; Eigen::Matrix6d I;
            if (m == 1) std::tie(ok, T, I) = ComputeRGBDOdometry(s, t, cam, init, RGBDOdometryJacobianFromHybridTerm(), opt);
            else std::tie(ok, T, I) = ComputeRGBDOdometry(s, t, cam, init, RGBDOdometryJacobianFromColorTerm(), optc);
            wd(o, ok ? 1.0 : 0.0); w4(o, T);
            for (int i = 0; i < 36; i++) wd(o, I(i / 6, i %% 6));
        }
        omp_set_num_threads(1);
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
    json = os.path.join(O3D, "3rdparty", "jsoncpp")
    cmd = ["g++", "-std=c++11", "-O2", "-fopenmp", "-w", "-I" + os.path.join(O3D, "src"), "-I" + os.path.join(O3D, "3rdparty", "Eigen"),
           "-I" + os.path.join(O3D, "3rdparty"), "-I" + O3D, "-I" + os.path.join(json, "include"), src,
           os.path.join(core, "Odometry", "RGBDOdometryJacobian.cpp"), os.path.join(core, "Camera", "PinholeCameraIntrinsic.cpp")]
    cmd += [os.path.join(core, "Geometry", n + ".cpp") for n in ("Image", "ImageFactory", "RGBDImage", "RGBDImageFactory")]
    cmd += [os.path.join(core, "Utility", n + ".cpp") for n in ("Eigen", "Console", "Helper", "IJsonConvertible")]
    cmd += [os.path.join(json, "json_" + n + ".cpp") for n in ("value", "reader", "writer")]
    subprocess.check_call(cmd + ["-o", exe])
    return exe


def write_input(path, frames, init, its, its_color, option):
    sg, sd, tg, td, k = frames
    h, w = sg.shape
    with open(path, "wb") as f:
        f.write(struct.pack("<ii4d", w, h, *[float(v) for v in k]))
        f.write(np.ascontiguousarray(init, "<f8").tobytes())
        f.write(struct.pack("<i%di" % len(its), len(its), *its))
        f.write(struct.pack("<i%di" % len(its_color), len(its_color), *its_color))
        f.write(struct.pack("<3d", option["max_depth_diff"], option["min_depth"], option["max_depth"]))
        for a in (sg, sd, tg, td):
            f.write(np.ascontiguousarray(a, "<f4").tobytes())


class Cursor:
    def __init__(self, v):
        self.v, self.at = v, 0

    def take(self, n):
        out = self.v[self.at:self.at + n]
        assert len(out) == n
        self.at += n
        return out


def run_case(exe, frames, init, its, its_color, option):
    inp, outp = os.path.join(SCRATCH, "in.bin"), os.path.join(SCRATCH, "out.bin")
    write_input(inp, frames, init, its, its_color, option)
    subprocess.check_call([exe, "case", inp, outp], stdout=subprocess.DEVNULL)
    c = Cursor(np.frombuffer(open(outp, "rb").read(), "<f8"))
    r = {"levels": []}
    for l in range(len(its)):
        w, h = int(c.take(1)[0]), int(c.take(1)[0])
        L = {}
        for name in S.WHICH[:8]:
            L[name] = c.take(w * h).astype(np.float32).reshape(h, w)
        L["src_xyz"] = c.take(3 * w * h).astype(np.float32).reshape(h, w, 3)
        L["idx"] = c.take(w * h).astype(np.int32)
        r["levels"].append(L)

    def trajectory():
        ok, n = int(c.take(1)[0]), int(c.take(1)[0])
        rec = c.take(17 * n).reshape(n, 17)
        return dict(ok=ok, counts=rec[:, 0].astype(np.int64), poses=rec[:, 1:].reshape(n, 4, 4).copy())

    def step():
        v = c.take(44)
        return dict(JTJ=v[:36].reshape(6, 6).copy(), JTr=v[36:42].copy(), r2=float(v[42]), rows=int(v[43]))

    def results():
        out = {}
        for th in (1, 3):
            v = c.take(53)
            out[th] = dict(ok=int(v[0]), T=v[1:17].reshape(4, 4).copy(), info=v[17:].reshape(6, 6).copy())
        return out

    r["hybrid"] = trajectory()
    r["final"] = c.take(16).reshape(4, 4).copy()
    r["steps"] = {(l, m, p): None for l in range(len(its)) for m in (0, 1) for p in ("init", "final")}
    for l in range(len(its)):
        for m in (0, 1):
            for p in ("init", "final"):
                r["steps"][(l, m, p)] = step()
    r["hybrid_result"] = results()
    r["color"] = trajectory()
    r["color_result"] = results()
    assert c.at == len(c.v)
    return r


digest = S.image_digest


def sums_exactly(v):
    """the f64 sum of these fp32 values has one value in ANY order: every value is a multiple of 2^(e_min - 24), e_min the
    smallest binary exponent among them, and the magnitudes sum below 2^53 of that unit -- every partial sum is exact"""
    v = np.asarray(v, np.float64)
    v = v[v != 0.0]
    if not len(v) or not np.all(np.isfinite(v)):
        return bool(np.all(np.isfinite(v)))
    unit = 2.0 ** (int(np.frexp(np.abs(v))[1].min()) - 24)
    return bool(np.abs(v).sum() * 1.0001 < unit * 2.0 ** 53)


def check_margins(name, frames, init, option, its, method_runs):
    """the refusals of the module docstring, on the specification's own trace of every run the case records"""
    sg, sd, tg, td, k = frames
    tr = S.Trace()
    prep = S.prepare(sg, sd, tg, td, k, init, dict(option, iterations=its), trace=tr)
    # fp32 rounding midpoints of the normalised pixels
    g0s, g0t = S.gaussian3(sg), S.gaussian3(tg)
    idx = S.correspondences(S.camera_matrix(k), init, prep["levels"][0]["src_depth"], prep["levels"][0]["tgt_depth"], option["max_depth_diff"])
    s = np.flatnonzero(idx >= 0)
    worst_mid = np.inf
    exact_means = True
    if len(s):
        for g, at in ((g0s, s), (g0t, idx[s])):
            exact_means = exact_means and sums_exactly(g.ravel()[at])
            p = S.normalized_products(g, at, len(s)).ravel()
            lo = p.astype(np.float32).astype(np.float64)
            other = np.where(lo <= p, np.nextafter(lo.astype(np.float32), np.float32(np.inf)), np.nextafter(lo.astype(np.float32), np.float32(-np.inf))).astype(np.float64)
            mid = 0.5 * (lo + other)
            with np.errstate(invalid="ignore", divide="ignore"):
                worst_mid = min(worst_mid, float(np.nanmin(np.abs(p - mid) / np.abs(p))))
    worst_det = np.inf
    for method, schedule in method_runs:
        opt = dict(option, iterations=schedule)
        pr = prep if len(schedule) == len(its) else S.prepare(sg, sd, tg, td, k, init, opt, trace=tr)
        ok, T, poses, counts, dets = S.multiscale(pr, init, method, opt, tr)
        for d in dets:
            if np.isfinite(d) and d != 0.0:
                worst_det = min(worst_det, max(abs(d) / 1e-6, 1e-6 / abs(d)))
        if ok:
            S.information(pr, T, opt, tr)
    print("%s: correspondence decisions at least %.3g (rounding) and %.3g (depth difference) from their boundaries; "
          "normalised products at least %.3g from an fp32 midpoint, the means %s; determinants a factor %.3g from the guard"
          % (name, tr.rounding, tr.depth, worst_mid, "exact in any order" if exact_means else "order-dependent", worst_det))
    if tr.margin() < 1e-9:
        raise SystemExit("%s: a correspondence decision sits within 1e-9 of its boundary: choose another input" % name)
    if worst_mid < 1e-10 and not exact_means:
        raise SystemExit("%s: a normalised pixel sits within 1e-10 of an fp32 rounding midpoint and the mean depends on the order "
                         "of its sum: choose another input" % name)
    if worst_det < 10.0:
        raise SystemExit("%s: a determinant sits within a factor 10 of the 1e-6 guard: choose another input" % name)


def case_b():
    """7 x 5: depths that become NaN (zero, negative, beyond max_depth, below min_depth) and a pixel on every border"""
    rng = np.random.default_rng(20261019)
    w, h = 7, 5
    k = np.array([6.0, 6.0, 3.0, 2.0])
    sd = (1.0 + 0.05 * rng.random((h, w))).astype(np.float32)
    td = (1.0 + 0.05 * rng.random((h, w))).astype(np.float32)
    sd[1, 2] = 0.0; sd[3, 5] = -1.0; td[2, 4] = 9.0; td[0, 0] = 0.2
    sg = rng.random((h, w)).astype(np.float32); tg = rng.random((h, w)).astype(np.float32)
    return sg, sd, tg, td, k


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--time", action="store_true")
    a = ap.parse_args()
    exe = build()
    opt = S.default_option()
    its, its_color = opt["iterations"], [3]
    fix = {}

    A = scene.frames(100, 75)
    init = np.eye(4)
    check_margins("A", A, init, opt, its, [(S.HYBRID, its), (S.COLOR, its_color)])
    r = run_case(exe, A, init, its, its_color, opt)
    for name, arr in zip(("src_gray", "src_depth", "tgt_gray", "tgt_depth", "intrinsic"), A):
        fix["a_" + name] = arr
    fix["a_init"] = init
    fix["a_option"] = np.array([opt["max_depth_diff"], opt["min_depth"], opt["max_depth"]])
    fix["a_iterations"] = np.array(its, np.int32); fix["a_color_iterations"] = np.array(its_color, np.int32)
    for l, L in enumerate(r["levels"]):
        for name in S.WHICH:
            img = L[name] if name != "src_xyz" else L[name][..., :2]
            if name == "src_xyz":
                assert S.same_image(L[name][..., 2], L["src_depth"])
            if l == 0 and name not in S.WHICH[:4]:
                fix["a_l0_%s_sha" % name] = digest(L[name])
            else:
                fix["a_l%d_%s" % (l, name)] = img
        fix["a_l%d_idx" % l] = L["idx"]
    fix["a_final"] = r["final"]
    for (l, m, p), s in r["steps"].items():
        for key, val in s.items():
            fix["a_l%d_m%d_%s_%s" % (l, m, p, key)] = val
    for run in ("hybrid", "color"):
        fix["a_%s_poses" % run] = r[run]["poses"]; fix["a_%s_counts" % run] = r[run]["counts"]; fix["a_%s_ok" % run] = r[run]["ok"]
        for th in (1, 3):
            res = r[run + "_result"][th]
            fix["a_%s_T_%d" % (run, th)] = res["T"]; fix["a_%s_info_%d" % (run, th)] = res["info"]; fix["a_%s_ok_%d" % (run, th)] = res["ok"]
        d = np.linalg.norm(r[run + "_result"][1]["T"] - r[run + "_result"][3]["T"]) / np.linalg.norm(r[run + "_result"][1]["T"])
        print("A %s: ok %d, pairs per iteration %s, information (5,5) %.1f with 1 thread, %.1f with 3; 1 against 3 threads %.2e; against the truth %.2e"
              % (run, r[run]["ok"], r[run]["counts"].tolist(), r[run + "_result"][1]["info"][5, 5], r[run + "_result"][3]["info"][5, 5], d,
                 np.linalg.norm(r[run + "_result"][1]["T"] - scene.truth())))
    assert r["hybrid"]["ok"] == 1 and r["color"]["ok"] == 1

    B = case_b()
    optb = dict(opt, min_depth=0.5)
    check_margins("B", B, init, optb, [1], [])
    rb = run_case(exe, B, init, [1], [1], optb)
    for name, arr in zip(("src_gray", "src_depth", "tgt_gray", "tgt_depth", "intrinsic"), B):
        fix["b_" + name] = arr
    fix["b_option"] = np.array([optb["max_depth_diff"], optb["min_depth"], optb["max_depth"]])
    for name in S.WHICH:
        fix["b_l0_" + name] = rb["levels"][0][name]
    fix["b_l0_idx"] = rb["levels"][0]["idx"]
    for m in (0, 1):
        for key, val in rb["steps"][(0, m, "init")].items():
            fix["b_l0_m%d_init_%s" % (m, key)] = val
    print("B: %d pairs at the identity, %d NaN depths in the processed source" % (np.count_nonzero(rb["levels"][0]["idx"] >= 0),
                                                                                 np.count_nonzero(np.isnan(rb["levels"][0]["src_depth"]))))

    Cf = (A[0], np.full_like(A[1], 5.0), A[2], A[3], A[4])
    rc = run_case(exe, Cf, init, its, its_color, opt)
    for th in (1, 3):
        fix["c_ok_%d" % th] = rc["hybrid_result"][th]["ok"]
        fix["c_T_%d" % th] = rc["hybrid_result"][th]["T"]; fix["c_info_%d" % th] = rc["hybrid_result"][th]["info"]
    print("C: ok %d" % rc["hybrid_result"][1]["ok"])
    assert rc["hybrid_result"][1]["ok"] == 0

    out = os.path.join(HERE, "odometry.npz")
    np.savez_compressed(out, **fix)
    print("odometry.npz: %d bytes" % os.path.getsize(out))
    if os.path.getsize(out) > 400 * 1024:
        raise SystemExit("the fixture is larger than 400 KB")
    if a.time:
        big = scene.frames(640, 480)
        inp, outp = os.path.join(SCRATCH, "in.bin"), os.path.join(SCRATCH, "out.bin")
        write_input(inp, big, init, its, its_color, opt)
        t0 = time.perf_counter()
        subprocess.check_call([exe, "time", inp, outp], stdout=subprocess.DEVNULL)
        res = np.frombuffer(open(outp, "rb").read(), "<f8")
        print("reference on this CPU (%d hardware threads, OpenMP): ComputeRGBDOdometry, hybrid term, 640 x 480, schedule %s: %.1f ms "
              "(ok %d, (5,5) = %.0f; the process took %.1f ms)" % (os.cpu_count(), its, res[0] * 1e3, int(res[1]), res[2], (time.perf_counter() - t0) * 1e3))


if __name__ == "__main__":
    main()
