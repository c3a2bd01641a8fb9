"""Generate tests/golden/tsdf.npz: what the compiled reference computes for the inputs tests/test_tsdf.py pins its numpy
specification (tests/tsdf_spec.py) and the library with.  Run once where the reference checkout exists; the fixture holds
DATA only.

The generator writes a small harness of its own into a scratch directory outside the repository, compiles it there against
the reference's Core/Integration/UniformTSDFVolume.cpp, Core/Geometry (Image, ImageFactory, RGBDImage, RGBDImageFactory,
PointCloud, PointCloudFactory, TriangleMesh), Core/Camera/PinholeCameraIntrinsic.cpp, Core/Utility and jsoncpp, runs it and
records, from the frames of tests/tsdf_scene.py (40 x 30):

  U21, U32, U67   a uniform volume of that resolution (length 1.6, origin (-0.8, -0.75, -0.85), sdf_trunc 3 voxels), the four
                  frames integrated one after another, for each colour type t in (none, rgb8, gray32):
       u<R>_s<k>_{tsdf,weight}_sha, u<R>_s<k>_t<t>_color_sha    SHA-256 of the fp32 bytes after the first frame (k = 0) and
                                    after the last (k = 1); tsdf and weight are the same for every colour type (asserted)
       u<R>_s<k>_{tsdf,weight}_p<a>, u<R>_s<k>_t<t>_color_p<a>   every voxel of the three probe planes: a = 0: x = R // 2,
                                    1: y = R // 3, 2: z = (2 R) // 3; weight as uint8; gray32 colour: one channel (the three
                                    are equal, asserted); resolution 21: the final volume in full instead (u21_s1_*_full)
       u<R>_pc_n, u<R>_pc_points_sha, u<R>_t<t>_pc_colors_sha    ExtractPointCloud of the final volume: count and digests of the
                                    f64 bytes, in the reference's order
       u<R>_pc_at, u<R>_pc_{points,normals}, u<R>_t<t>_pc_colors  ... and the rows `at` (an even stride, at most 150) in full
       u<R>_vx_n, u<R>_vx_{points,colors}_sha                     ExtractVoxelPointCloud of the final volume
  E    an all-zero depth frame into a fresh volume and into the final U21 volume: e_fresh_pc_n = e_fresh_vx_n = 0, the
       volumes unchanged (asserted here; the tests assert it of the library)
  P    CreatePointCloudFromDepthImage of frame 0 with strides 1 and 4, with the identity and with frame 1's extrinsic, and
       CreatePointCloudFromRGBDImage with RGB8 and float gray colours (p_*)

It asserts that the integration meets every branch (a voxel behind the camera, a projection beyond each of the four
borders, a depth-0 pixel, sdf <= -sdf_trunc, sdf > sdf_trunc, weights from 0 up to the frame count) and refuses a fixture
with an extracted point whose unnormalised gradient has norm below 1e-3: that would pin the rounding of a near-zero
normal, not the algorithm.  The fp32 decisions need no margin: the specification reproduces them exactly.

  S    scalable volumes s0 (units of 8, stride 4, RGB8, four frames), s1 (units of 16, stride 1, Gray32, two frames) and s2
       (units of 8, stride 4, no colour, sdf_trunc above the unit length: a point's bounds span three units per axis):
       s<i>_units_f<k>   the unit indices after frame k, rows sorted (the reference's order is an unordered_map's)
       s<i>_unit_sha8    per final unit, in that order, the first 8 bytes of the SHA-256 of its tsdf | weight | colour fp32
                         bytes; s<i>_units_sha: the SHA-256 of all the units' full digests in that order
       s<i>_probe_*      a few units in full
       s<i>_pc_*, s<i>_vx_*   the two extractions with their rows sorted by point, as for U
       The scene straddles the origin (asserted: negative and non-negative indices on every axis) and a later frame opens
       units the first did not (asserted).  The generator refuses a fixture where a floor of point / volume_unit_length
       after +- sdf_trunc sits within 1e-9 relative of its boundary: that would pin the rounding of extrinsic.inverse().

With --time it also times the reference's Integrate and extractions on the inputs of tools/tsdf_probe.py, the uniform 512^3
volume and the scalable volume at Open3D's pipeline settings (this
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
SCRATCH = os.environ.get("VISMA_SCRATCH") or tempfile.mkdtemp(prefix="tsdf_")      # outside the repository
sys.path.insert(0, os.path.join(ROOT, "tests"))
import tsdf_scene as scene  # noqa: E402
import tsdf_spec as S  # noqa: E402

W, H = 40, 30
LENGTH, ORIGIN = 1.6, (-0.8, -0.75, -0.85)
RESOLUTIONS = (21, 32, 67)
# S: name -> (volume_unit_resolution, depth_sampling_stride, voxel_length, sdf_trunc, colour type, frames); s2 has sdf_trunc
# above the unit length (0.24), so a point's bounds span three units per axis
S_CASES = {"s0": (8, 4, 0.05, 0.15, 1, 4), "s1": (16, 1, 0.025, 0.1, 2, 2), "s2": (8, 4, 0.03, 0.3, 0, 2)}

HARNESS = r'''
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include <Core/Integration/UniformTSDFVolume.h>
#include <Core/Integration/ScalableTSDFVolume.h>
#include <Core/Geometry/PointCloud.h>
#include <Core/Geometry/RGBDImage.h>
#include <Core/Camera/PinholeCameraIntrinsic.h>
using namespace open3d;
static void rd(FILE *f, void *p, size_t n) { if (fread(p, 1, n, f) != n) std::exit(2); }
static void wd(FILE *o, double v) { fwrite(&v, 8, 1, o); }
static double now() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }
static void wvec(FILE *o, const std::vector<Eigen::Vector3d> &v) { for (auto &p : v) { wd(o, p(0)); wd(o, p(1)); wd(o, p(2)); } }
static void wvol(FILE *o, const UniformTSDFVolume &v)
{
    for (float f : v.tsdf_) wd(o, (double)f);
    for (float f : v.weight_) wd(o, (double)f);
    for (auto &c : v.color_) { wd(o, (double)c(0)); wd(o, (double)c(1)); wd(o, (double)c(2)); }
}
static void wcloud(FILE *o, const PointCloud &pc)
{
    wd(o, (double)pc.points_.size()); wd(o, (double)pc.normals_.size()); wd(o, (double)pc.colors_.size());
    wvec(o, pc.points_); wvec(o, pc.normals_); wvec(o, pc.colors_);
}
struct Frame { Eigen::Matrix4d E; RGBDImage rgb, gray; };
static void frame(FILE *f, Frame &fr, int W, int H)
{
    double e[16]; rd(f, e, 128);
    for (int i = 0; i < 16; i++) fr.E(i / 4, i %% 4) = e[i];
    fr.rgb.depth_.PrepareImage(W, H, 1, 4); rd(f, fr.rgb.depth_.data_.data(), (size_t)W * H * 4);
    fr.rgb.color_.PrepareImage(W, H, 3, 1); rd(f, fr.rgb.color_.data_.data(), (size_t)W * H * 3);
    fr.gray.depth_ = fr.rgb.depth_;
    fr.gray.color_.PrepareImage(W, H, 1, 4); rd(f, fr.gray.color_.data_.data(), (size_t)W * H * 4);
}
int main(int argc, char **argv)
{
    FILE *f = std::fopen(argv[2], "rb"), *o = std::fopen(argv[3], "wb");
    if (!f || !o) return 2;
    int W, H, n; double k[4];
    rd(f, &W, 4); rd(f, &H, 4); rd(f, k, 32); rd(f, &n, 4);
    PinholeCameraIntrinsic cam(W, H, k[0], k[1], k[2], k[3]);
    if (!std::strcmp(argv[1], "P")) {
        int stride, ctype; rd(f, &stride, 4); rd(f, &ctype, 4);
        Frame fr; frame(f, fr, W, H);
        std::shared_ptr<PointCloud> pc = ctype == 0 ? CreatePointCloudFromDepthImage(fr.rgb.depth_, cam, fr.E, 1000.0, 1000.0, stride)
                                                    : CreatePointCloudFromRGBDImage(ctype == 1 ? fr.rgb : fr.gray, cam, fr.E);
        wcloud(o, *pc);
        std::fclose(o);
        return 0;
    }
    if (!std::strcmp(argv[1], "S") || !std::strcmp(argv[1], "Stime")) {
        int R, ctype, stride; double vl, trunc;
        rd(f, &R, 4); rd(f, &ctype, 4); rd(f, &stride, 4); rd(f, &vl, 8); rd(f, &trunc, 8);
        std::vector<Frame> frames((size_t)n);
        for (auto &fr : frames) frame(f, fr, W, H);
        ScalableTSDFVolume vol(vl, trunc, (TSDFVolumeColorType)ctype, R, stride);
        if (!std::strcmp(argv[1], "Stime")) {
            double t0 = now(); vol.Integrate(frames[0].rgb, cam, frames[0].E); wd(o, now() - t0);
            t0 = now(); auto pc = vol.ExtractPointCloud(); wd(o, now() - t0);
            wd(o, (double)vol.volume_units_.size()); wd(o, (double)pc->points_.size());
            std::fclose(o);
            return 0;
        }
        for (int i = 0; i < n; i++) {
            vol.Integrate(ctype == 2 ? frames[i].gray : frames[i].rgb, cam, frames[i].E);
            wd(o, (double)vol.volume_units_.size());
            for (auto &u : vol.volume_units_) { wd(o, u.second.index_(0)); wd(o, u.second.index_(1)); wd(o, u.second.index_(2)); }
        }
        for (auto &u : vol.volume_units_) wvol(o, *u.second.volume_);      // (in the order of the last index list)
        wcloud(o, *vol.ExtractPointCloud());
        wcloud(o, *vol.ExtractVoxelPointCloud());
        std::fclose(o);
        return 0;
    }
    int R, ctype; double length, trunc, org[3];
    rd(f, &R, 4); rd(f, &ctype, 4); rd(f, &length, 8); rd(f, &trunc, 8); rd(f, org, 24);
    std::vector<Frame> frames((size_t)n);
    for (auto &fr : frames) frame(f, fr, W, H);
    UniformTSDFVolume vol(length, R, trunc, (TSDFVolumeColorType)ctype, Eigen::Vector3d(org[0], org[1], org[2]));
    if (!std::strcmp(argv[1], "time")) {
        double t0 = now(); vol.Integrate(frames[0].rgb, cam, frames[0].E); wd(o, now() - t0);
        t0 = now(); auto pc = vol.ExtractPointCloud(); wd(o, now() - t0);
        t0 = now(); auto vx = vol.ExtractVoxelPointCloud(); wd(o, now() - t0);
        wd(o, (double)pc->points_.size()); wd(o, (double)vx->points_.size());
        std::fclose(o);
        return 0;
    }
    for (int i = 0; i < n; i++) {
        vol.Integrate(ctype == 2 ? frames[i].gray : frames[i].rgb, cam, frames[i].E);
        if (i == 0 || i == n - 1) wvol(o, vol);
    }
    wcloud(o, *vol.ExtractPointCloud());
    wcloud(o, *vol.ExtractVoxelPointCloud());
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
    # (sections of functions nothing here calls -- the k-d tree users of PointCloud.cpp and TriangleMesh.cpp -- are dropped
    #  at the link, and with them their references to libraries this harness does not have)
    cmd = ["g++", "-std=c++11", "-O2", "-fopenmp", "-w", "-ffunction-sections", "-fdata-sections", "-Wl,--gc-sections",
           "-I" + os.path.join(O3D, "src"), "-I" + os.path.join(O3D, "3rdparty", "Eigen"),
           "-I" + os.path.join(O3D, "3rdparty"), "-I" + O3D, "-I" + os.path.join(json, "include"),
           "-I" + os.path.join(O3D, "3rdparty", "flann"), src,
           os.path.join(core, "Integration", "UniformTSDFVolume.cpp"), os.path.join(core, "Integration", "ScalableTSDFVolume.cpp"), os.path.join(core, "Camera", "PinholeCameraIntrinsic.cpp")]
    cmd += [os.path.join(core, "Geometry", n + ".cpp") for n in ("Image", "ImageFactory", "RGBDImage", "RGBDImageFactory", "PointCloud",
                                                                  "PointCloudFactory", "TriangleMesh")]
    cmd += [os.path.join(core, "Utility", n + ".cpp") for n in ("Eigen", "Console", "Helper", "IJsonConvertible")]
    cmd += [os.path.join(json, "json_" + n + ".cpp") for n in ("value", "reader", "writer")]
    subprocess.check_call(cmd + ["-o", exe])
    return exe


def write_frames(f, frames):
    for depth, rgb, gray, E in frames:
        f.write(np.ascontiguousarray(E, "<f8").tobytes())
        f.write(np.ascontiguousarray(depth, "<f4").tobytes())
        f.write(np.ascontiguousarray(rgb, np.uint8).tobytes())
        f.write(np.ascontiguousarray(gray, "<f4").tobytes())


class Cursor:
    def __init__(self, v):
        self.v, self.at = v, 0

    def take(self, n):
        out = self.v[self.at:self.at + n]
        assert len(out) == n
        self.at += n
        return out

    def cloud(self):
        n, nn, nc = [int(v) for v in self.take(3)]
        return dict(points=self.take(3 * n).reshape(n, 3).copy(), normals=self.take(3 * nn).reshape(nn, 3).copy(),
                    colors=self.take(3 * nc).reshape(nc, 3).copy())


def run(exe, mode, w, h, k, frames, head):
    inp, outp = os.path.join(SCRATCH, "in.bin"), os.path.join(SCRATCH, "out.bin")
    with open(inp, "wb") as f:
        f.write(struct.pack("<ii4di", w, h, *[float(v) for v in k], len(frames)))
        f.write(head)
        write_frames(f, frames)
    subprocess.check_call([exe, mode, inp, outp], stdout=subprocess.DEVNULL)
    return Cursor(np.frombuffer(open(outp, "rb").read(), "<f8"))


def run_uniform(exe, R, ctype, frames, k, length=LENGTH, trunc=None, origin=ORIGIN, w=W, h=H):
    trunc = 3.0 * length / R if trunc is None else trunc
    c = run(exe, "U", w, h, k, frames, struct.pack("<ii5d", R, ctype, length, trunc, *origin))
    n = R ** 3
    stages = []
    for _ in range(1 if len(frames) == 1 else 2):
        stages.append(dict(tsdf=c.take(n).astype(np.float32), weight=c.take(n).astype(np.float32),
                           color=c.take(3 * n).astype(np.float32).reshape(n, 3) if ctype else None))
    out = dict(stages=stages, pc=c.cloud(), vx=c.cloud(), trunc=trunc)
    assert c.at == len(c.v)
    return out


def planes(R):
    return (R // 2, R // 3, (2 * R) // 3)


def probe(a, R, axis):
    """the voxels of probe plane `axis` of a per-voxel array (R^3 or R^3 x c)"""
    a = a.reshape((R, R, R) + a.shape[1:])
    return np.take(a, planes(R)[axis], axis=axis)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--time", action="store_true")
    args = ap.parse_args()
    exe = build()
    frames, k = scene.frames(W, H)
    fix = {"intrinsic": k, "length": np.float64(LENGTH), "origin": np.array(ORIGIN)}
    for i, (depth, rgb, gray, E) in enumerate(frames):
        fix["f%d_depth" % i] = depth; fix["f%d_rgb" % i] = rgb; fix["f%d_gray" % i] = gray; fix["f%d_extrinsic" % i] = E

    for R in RESOLUTIONS:
        res = [run_uniform(exe, R, t, frames, k) for t in (0, 1, 2)]
        fix["u%d_sdf_trunc" % R] = np.float64(res[0]["trunc"])
        # every branch, on the specification's own trace
        tr = {}
        vol = S.new_volume(LENGTH, R, res[0]["trunc"], S.COLOR_RGB8, ORIGIN)
        for depth, rgb, gray, E in frames:
            S.integrate(vol, depth, rgb, k, E, trace=tr)
        print("U%d: %s" % (R, tr))
        for key in ("behind", "left", "right", "top", "bottom", "hole", "far_behind", "clamped", "integrated"):
            assert tr[key] > 0, (R, key)
        wts = np.unique(res[0]["stages"][1]["weight"])
        assert wts[0] == 0 and wts[-1] == len(frames), wts
        for s in (0, 1):
            for t in (1, 2):
                assert np.array_equal(res[t]["stages"][s]["tsdf"], res[0]["stages"][s]["tsdf"])
                assert np.array_equal(res[t]["stages"][s]["weight"], res[0]["stages"][s]["weight"])
            g = res[2]["stages"][s]["color"]
            assert np.array_equal(g[:, 0], g[:, 1]) and np.array_equal(g[:, 0], g[:, 2])
            st = res[0]["stages"][s]
            fix["u%d_s%d_tsdf_sha" % (R, s)] = S.digest(st["tsdf"], np.float32)
            fix["u%d_s%d_weight_sha" % (R, s)] = S.digest(st["weight"], np.float32)
            for t in (1, 2):
                fix["u%d_s%d_t%d_color_sha" % (R, s, t)] = S.digest(res[t]["stages"][s]["color"], np.float32)
            if R ** 3 <= 10000 and s == 0:
                continue                                                 # (the first stage of 21: digests only)
            if R ** 3 <= 10000:
                fix["u%d_s%d_tsdf_full" % (R, s)] = st["tsdf"]; fix["u%d_s%d_weight_full" % (R, s)] = st["weight"].astype(np.uint8)
                fix["u%d_s%d_t1_color_full" % (R, s)] = res[1]["stages"][s]["color"]
                fix["u%d_s%d_t2_color_full" % (R, s)] = res[2]["stages"][s]["color"][:, 0]
                continue
            for ax in range(3):
                fix["u%d_s%d_tsdf_p%d" % (R, s, ax)] = probe(st["tsdf"], R, ax)
                fix["u%d_s%d_weight_p%d" % (R, s, ax)] = probe(st["weight"], R, ax).astype(np.uint8)
                fix["u%d_s%d_t1_color_p%d" % (R, s, ax)] = probe(res[1]["stages"][s]["color"], R, ax)
                fix["u%d_s%d_t2_color_p%d" % (R, s, ax)] = probe(res[2]["stages"][s]["color"], R, ax)[..., 0]
        pc = res[0]["pc"]; n = len(pc["points"])
        for t in (1, 2):
            assert np.array_equal(res[t]["pc"]["points"], pc["points"]) and np.array_equal(res[t]["pc"]["normals"], pc["normals"])
            assert len(res[t]["pc"]["colors"]) == n
        assert len(pc["normals"]) == n and len(pc["colors"]) == 0 and n > 0
        # the gradient margin, on the specification's own extraction of the reference's final volume
        vol = S.new_volume(LENGTH, R, res[0]["trunc"], S.COLOR_NONE, ORIGIN)
        vol["tsdf"], vol["weight"] = res[0]["stages"][1]["tsdf"].copy(), res[0]["stages"][1]["weight"].copy()
        sp, sn, _, grad = S.extract_point_cloud(vol, with_gradient=True)
        gmin = float(np.linalg.norm(grad, axis=1).min())
        print("U%d: %d extracted points, %d voxel points, the smallest unnormalised gradient %.3g" % (R, n, len(res[0]["vx"]["points"]), gmin))
        if gmin < 1e-3:
            raise SystemExit("U%d: an extracted point's unnormalised gradient has norm below 1e-3: choose another input" % R)
        at = np.arange(0, n, max(1, -(-n // 150)))
        fix["u%d_pc_n" % R] = np.int64(n); fix["u%d_pc_at" % R] = at
        fix["u%d_pc_points_sha" % R] = S.digest(pc["points"], np.float64)
        fix["u%d_pc_points" % R] = pc["points"][at]; fix["u%d_pc_normals" % R] = pc["normals"][at]
        for t in (1, 2):
            fix["u%d_t%d_pc_colors_sha" % (R, t)] = S.digest(res[t]["pc"]["colors"], np.float64)
            fix["u%d_t%d_pc_colors" % (R, t)] = res[t]["pc"]["colors"][at]
        vx = res[0]["vx"]
        for t in (1, 2):
            assert np.array_equal(res[t]["vx"]["points"], vx["points"]) and np.array_equal(res[t]["vx"]["colors"], vx["colors"])
        fix["u%d_vx_n" % R] = np.int64(len(vx["points"]))
        fix["u%d_vx_points_sha" % R] = S.digest(vx["points"], np.float64); fix["u%d_vx_colors_sha" % R] = S.digest(vx["colors"], np.float64)
        if R == RESOLUTIONS[0]:
            final21 = res[1]

    # S: scalable volumes
    for name, (R, stride, vl, trunc, ctype, nf) in S_CASES.items():
        c = run(exe, "S", W, H, k, frames[:nf], struct.pack("<iii2d", R, ctype, stride, vl, trunc))
        sets = []
        for i in range(nf):
            m = int(c.take(1)[0])
            sets.append(c.take(3 * m).astype(np.int32).reshape(m, 3))
        n3 = R ** 3
        units = {}
        for key in map(tuple, sets[-1].tolist()):
            units[key] = dict(tsdf=c.take(n3).astype(np.float32), weight=c.take(n3).astype(np.float32),
                              color=c.take(3 * n3).astype(np.float32).reshape(n3, 3) if ctype else None)
        pc, vx = c.cloud(), c.cloud()
        assert c.at == len(c.v)
        sets = [a[np.lexsort((a[:, 2], a[:, 1], a[:, 0]))] for a in sets]
        assert len(sets[-1]) > len(sets[0]) and set(map(tuple, sets[0].tolist())) < set(map(tuple, sets[-1].tolist()))   # a later frame opens units
        assert (sets[-1].min(0) < 0).all() and (sets[-1].max(0) >= 0).all()                    # negative indices on every axis
        # the f64 decisions, on the specification's own trace, and its gradients
        tr = {}
        sv = S.new_scalable(vl, trunc, ctype, R, stride)
        for i, fr in enumerate(frames[:nf]):
            S.scalable_integrate(sv, fr[0], (None, fr[1], fr[2])[ctype], k, fr[3], trace=tr)
            assert sorted(sv["units"]) == list(map(tuple, sets[i].tolist())), (name, i)
        if tr["floor_margin"] < 1e-9:
            raise SystemExit("%s: a floor of point / volume_unit_length sits within 1e-9 of its boundary: choose another input" % name)
        grad = S.scalable_extract_point_cloud(sv, with_gradient=True)[3]
        gmin = float(np.linalg.norm(grad, axis=1).min())
        if gmin < 1e-3:
            raise SystemExit("%s: an extracted point's unnormalised gradient has norm below 1e-3: choose another input" % name)
        print("%s: units per frame %s, %d extracted points, %d voxel points, floor margin %.3g, units spanned per axis %d, smallest gradient %.3g"
              % (name, [len(a) for a in sets], len(pc["points"]), len(vx["points"]), tr["floor_margin"], tr["span"], gmin))
        if name == "s2":
            assert tr["span"] >= 3
        fix[name + "_config"] = np.array([R, stride, vl, trunc, ctype, nf])
        for i, a in enumerate(sets):
            fix["%s_units_f%d" % (name, i)] = a
        keys = list(map(tuple, sets[-1].tolist()))
        sha = np.stack([S.digest(np.concatenate([units[q]["tsdf"], units[q]["weight"]] + ([units[q]["color"].ravel()] if ctype else [])),
                                                     np.float32) for q in keys])
        fix[name + "_unit_sha8"] = sha[:, :8].copy()                    # the first 8 bytes per unit, and one digest of all 32
        fix[name + "_units_sha"] = S.digest(sha, np.uint8)
        probe_units = keys[::max(1, len(keys) // 3)][:3]                 # a few units in full
        fix[name + "_probe_units"] = np.array(probe_units, np.int32)
        fix[name + "_probe_tsdf"] = np.stack([units[q]["tsdf"] for q in probe_units])
        fix[name + "_probe_weight"] = np.stack([units[q]["weight"] for q in probe_units]).astype(np.uint8)
        if ctype:
            fix[name + "_probe_color"] = np.stack([units[q]["color"] for q in probe_units])
        pts, nrm, col = S.sort_rows(pc["points"], pc["normals"], pc["colors"] if ctype else None)
        n = len(pts); at = np.arange(0, n, max(1, -(-n // 100)))
        fix[name + "_pc_n"] = np.int64(n); fix[name + "_pc_at"] = at
        fix[name + "_pc_points_sha"] = S.digest(pts, np.float64)
        fix[name + "_pc_points"] = pts[at]; fix[name + "_pc_normals"] = nrm[at]
        if ctype:
            fix[name + "_pc_colors_sha"] = S.digest(col, np.float64); fix[name + "_pc_colors"] = col[at]
        vp, vc = S.sort_rows(vx["points"], vx["colors"])
        fix[name + "_vx_n"] = np.int64(len(vp))
        fix[name + "_vx_points_sha"] = S.digest(vp, np.float64); fix[name + "_vx_colors_sha"] = S.digest(vc, np.float64)

    # E: an all-zero depth frame
    zero = [(np.zeros_like(frames[0][0]),) + frames[0][1:]]
    e = run_uniform(exe, 21, 1, zero, k)
    assert not e["stages"][0]["tsdf"].any() and not e["stages"][0]["weight"].any() and not e["stages"][0]["color"].any()
    assert len(e["pc"]["points"]) == 0 and len(e["vx"]["points"]) == 0
    fix["e_fresh_pc_n"] = np.int64(0); fix["e_fresh_vx_n"] = np.int64(0)
    e = run_uniform(exe, 21, 1, list(frames) + zero, k)
    for key in ("tsdf", "weight", "color"):
        assert np.array_equal(e["stages"][1][key], final21["stages"][1][key])
    assert np.array_equal(e["pc"]["points"], final21["pc"]["points"])
    fix["e_filled_unchanged"] = np.int64(1)

    # P: point clouds from a depth frame and from an RGB-D frame
    depth, rgb, gray, _ = frames[0]
    E1 = frames[1][3]
    for name, stride, ctype, E in (("p_s1_id", 1, 0, np.eye(4)), ("p_s4_id", 4, 0, np.eye(4)), ("p_s1_e1", 1, 0, E1), ("p_s4_e1", 4, 0, E1),
                                   ("p_rgb_id", 1, 1, np.eye(4)), ("p_gray_id", 1, 2, np.eye(4))):
        c = run(exe, "P", W, H, k, [(depth, rgb, gray, E)], struct.pack("<ii", stride, ctype))
        pc = c.cloud()
        assert c.at == len(c.v) and len(pc["normals"]) == 0 and len(pc["colors"]) == (len(pc["points"]) if ctype else 0)
        if name == "p_s1_e1":                                          # (compared within a tolerance: every 8th row is kept)
            fix[name + "_n"] = np.int64(len(pc["points"])); fix[name + "_points"] = pc["points"][::8]
        elif not ctype:
            fix[name + "_points"] = pc["points"]
        else:
            assert np.array_equal(pc["points"], fix["p_s1_id_points"])   # (the same points: stored once)
            fix[name + "_colors"] = pc["colors"].astype(np.float32 if ctype == 2 else np.float64)   # (gray: fp32 values, exactly)
            assert np.array_equal(fix[name + "_colors"].astype(np.float64), pc["colors"])
        print("%s: %d points" % (name, len(pc["points"])))
    fix["p_extrinsic"] = E1

    out = os.path.join(HERE, "tsdf.npz")
    np.savez_compressed(out, **fix)
    print("tsdf.npz: %d bytes" % os.path.getsize(out))
    if os.path.getsize(out) > 400 * 1024:
        raise SystemExit("the fixture is larger than 400 KB")
    if args.time:
        big, kb = scene.frames(640, 480, 1)
        t0 = time.perf_counter()
        c = run(exe, "time", 640, 480, kb, big, struct.pack("<ii5d", 512, 1, 4.0, 0.04, -2.0, -2.0, -2.0))
        r = c.v
        c = run(exe, "Stime", 640, 480, kb, big, struct.pack("<iii2d", 16, 1, 4, 4.0 / 512.0, 0.04))
        print("reference on this CPU: scalable, voxel 4 / 512 m, sdf_trunc 0.04, units of 16, stride 4, RGB8, 640 x 480: Integrate %.1f ms "
              "(%d units), ExtractPointCloud %.1f ms (%d points)" % (c.v[0] * 1e3, int(c.v[2]), c.v[1] * 1e3, int(c.v[3])))
        print("reference on this CPU (%d hardware threads, OpenMP): uniform 512^3, RGB8, 640 x 480: Integrate %.1f ms, ExtractPointCloud "
              "%.1f ms (%d points), ExtractVoxelPointCloud %.1f ms (%d points); the process took %.1f s"
              % (os.cpu_count(), r[0] * 1e3, r[1] * 1e3, int(r[3]), r[2] * 1e3, int(r[4]), time.perf_counter() - t0))


if __name__ == "__main__":
    main()
