"""Generate tests/golden/tsdf_mesh.npz: what the compiled reference's ExtractTriangleMesh gives for the inputs
tests/test_tsdf_mesh_spec.py pins the numpy specification (tests/tsdf_mesh_spec.py) with, and tests/test_tsdf_mesh.py the
library.  Run once where the reference checkout exists; the fixture holds DATA only.

The generator writes a small harness of its own into a scratch directory outside the repository, compiles it there against
the reference's Core/Integration (UniformTSDFVolume.cpp, ScalableTSDFVolume.cpp), Core/Geometry, Core/Camera, Core/Utility
and jsoncpp, runs it and records per case:

  <c>_nv, <c>_nt          vertex and triangle counts of the reference's mesh
  <c>_rows_sha            SHA-256 of the reference's [vertex | colour] rows (f64), sorted lexicographically by their bits;
  <c>_rows                ... and the rows in full where there are at most 1500
  <c>_euler               V - E + F
  <c>_boundary_n, _sha    the undirected edges used by exactly one triangle, as sorted pairs of vertex positions (6 f64 per
  <c>_boundary            row, rows sorted by their bits); in full where at most 600
  <c>_ambiguous           valid cubes with a face whose signs alternate diagonally, counted on the reference's volume
  winding_sign            the sign of normal . (direction of increasing tsdf) over every triangle of non-zero area of every
                          case, the direction being the sum over the triangle's vertices of the unit step along the vertex's
                          voxel edge from its inside end to its outside end: asserted uniform

The cases (frames: those of tests/golden/tsdf.npz, the scene of tests/tsdf_scene.py at 40 x 30):
  u21 (RGB8), u32 (Gray32), u67 (no colour)   the uniform volumes of gen_tsdf.py, four frames
  s0, s1, s2                                   the scalable volumes of gen_tsdf.py; s5: units of 5 voxels (0.04, stride 4, RGB8)
  sp5, sp8   a smooth slanted surface (24 x 18) into scalable volumes with units of 5 and of 8
  plane    exactly representable numbers: 5^3 voxels of 0.25, identity pose, a 17 x 17 frame of depth 0.25 (left of the
           principal point) and 0.5: the voxel layers at those depths have tsdf == 0.0f exactly, so f0 == 0 or f1 == 0,
           vertices coincide and triangles have zero area (asserted)
  ambig    a 16 x 16 frame of per-pixel alternating depths 1.2 / 1.4 into R = 16 (voxels of 0.1, about a pixel wide): at
           least 8 valid cubes with a diagonally signed face (asserted)
The scene's depth discontinuities leave such cubes in u32, u67 and s0 .. s5 too (9 .. 114 of them): those cases are compared
as ambig is (tests/tsdf_mesh_cases.py: AMBIGUOUS).  For u21, sp5, sp8 and plane the generator asserts that there is NO such
cube: there the triangulation's boundary and count are unique, and the tests compare them.  It also asserts that tests/tsdf_spec.py integrates every case's volume bit for bit (the
tests re-integrate instead of storing volumes) and that the specification's vertex rows equal the reference's.

--time prints the reference's ExtractTriangleMesh time at the sizes of tools/tsdf_mesh_probe.py (printed, not stored).
Nothing compiled and no reference text is kept."""
import argparse
import hashlib
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
SCRATCH = os.environ.get("VISMA_SCRATCH") or tempfile.mkdtemp(prefix="tsdf_mesh_")      # outside the repository
sys.path.insert(0, os.path.join(ROOT, "tests"))
import tsdf_scene as scene  # noqa: E402
import tsdf_spec as S  # noqa: E402
import tsdf_mesh_spec as M  # noqa: E402
import tsdf_mesh_cases as cases  # noqa: E402

HARNESS = r'''
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include <Core/Integration/UniformTSDFVolume.h>
#include <Core/Integration/ScalableTSDFVolume.h>
#include <Core/Geometry/TriangleMesh.h>
#include <Core/Geometry/RGBDImage.h>
#include <Core/Camera/PinholeCameraIntrinsic.h>
using namespace open3d;
static void rd(FILE *f, void *p, size_t n) { if (fread(p, 1, n, f) != n) std::exit(2); }
static void wd(FILE *o, double v) { fwrite(&v, 8, 1, o); }
static double now() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }
static void wvol(FILE *o, const UniformTSDFVolume &v)
{
    for (float f : v.tsdf_) wd(o, (double)f);
    for (float f : v.weight_) wd(o, (double)f);
    for (auto &c : v.color_) { wd(o, (double)c(0)); wd(o, (double)c(1)); wd(o, (double)c(2)); }
}
static void wmesh(FILE *o, const TriangleMesh &m)
{
    wd(o, (double)m.vertices_.size()); wd(o, (double)m.vertex_colors_.size()); wd(o, (double)m.triangles_.size());
    for (auto &p : m.vertices_) { wd(o, p(0)); wd(o, p(1)); wd(o, p(2)); }
    for (auto &p : m.vertex_colors_) { wd(o, p(0)); wd(o, p(1)); wd(o, p(2)); }
    for (auto &t : m.triangles_) { wd(o, t(0)); wd(o, t(1)); wd(o, t(2)); }
}
struct Frame { Eigen::Matrix4d E; RGBDImage rgb, gray; };
static void frame(FILE *f, Frame &fr, int W, int H)
{
    double e[16]; rd(f, e, 128);
    for (int i = 0; i < 16; i++) fr.E(i / 4, i % 4) = e[i];
    fr.rgb.depth_.PrepareImage(W, H, 1, 4); rd(f, fr.rgb.depth_.data_.data(), (size_t)W * H * 4);
    fr.rgb.color_.PrepareImage(W, H, 3, 1); rd(f, fr.rgb.color_.data_.data(), (size_t)W * H * 3);
    fr.gray.depth_ = fr.rgb.depth_;
    fr.gray.color_.PrepareImage(W, H, 1, 4); rd(f, fr.gray.color_.data_.data(), (size_t)W * H * 4);
}
int main(int argc, char **argv)
{
    FILE *f = std::fopen(argv[2], "rb"), *o = std::fopen(argv[3], "wb");
    if (!f || !o) return 2;
    const bool timed = std::strstr(argv[1], "time") != nullptr;
    int W, H, n; double k[4];
    rd(f, &W, 4); rd(f, &H, 4); rd(f, k, 32); rd(f, &n, 4);
    PinholeCameraIntrinsic cam(W, H, k[0], k[1], k[2], k[3]);
    if (argv[1][0] == 'S') {
        int R, ctype, stride; double vl, trunc;
        rd(f, &R, 4); rd(f, &ctype, 4); rd(f, &stride, 4); rd(f, &vl, 8); rd(f, &trunc, 8);
        std::vector<Frame> frames((size_t)n);
        for (auto &fr : frames) frame(f, fr, W, H);
        ScalableTSDFVolume vol(vl, trunc, (TSDFVolumeColorType)ctype, R, stride);
        for (int i = 0; i < n; i++) vol.Integrate(ctype == 2 ? frames[i].gray : frames[i].rgb, cam, frames[i].E);
        if (timed) {
            double t0 = now(); auto m = vol.ExtractTriangleMesh(); wd(o, now() - t0);
            wd(o, (double)vol.volume_units_.size()); wd(o, (double)m->vertices_.size()); wd(o, (double)m->triangles_.size());
            std::fclose(o);
            return 0;
        }
        wd(o, (double)vol.volume_units_.size());
        for (auto &u : vol.volume_units_) { wd(o, u.second.index_(0)); wd(o, u.second.index_(1)); wd(o, u.second.index_(2)); }
        for (auto &u : vol.volume_units_) wvol(o, *u.second.volume_);
        wmesh(o, *vol.ExtractTriangleMesh());
        std::fclose(o);
        return 0;
    }
    int R, ctype; double length, trunc, org[3];
    rd(f, &R, 4); rd(f, &ctype, 4); rd(f, &length, 8); rd(f, &trunc, 8); rd(f, org, 24);
    std::vector<Frame> frames((size_t)n);
    for (auto &fr : frames) frame(f, fr, W, H);
    UniformTSDFVolume vol(length, R, trunc, (TSDFVolumeColorType)ctype, Eigen::Vector3d(org[0], org[1], org[2]));
    for (int i = 0; i < n; i++) vol.Integrate(ctype == 2 ? frames[i].gray : frames[i].rgb, cam, frames[i].E);
    if (timed) {
        double t0 = now(); auto m = vol.ExtractTriangleMesh(); wd(o, now() - t0);
        wd(o, (double)m->vertices_.size()); wd(o, (double)m->triangles_.size());
        std::fclose(o);
        return 0;
    }
    wvol(o, vol);
    wmesh(o, *vol.ExtractTriangleMesh());
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
    json = os.path.join(O3D, "3rdparty", "jsoncpp")
    cmd = ["g++", "-std=c++11", "-O2", "-fopenmp", "-w", "-ffunction-sections", "-fdata-sections", "-Wl,--gc-sections",
           "-I" + os.path.join(O3D, "src"), "-I" + os.path.join(O3D, "3rdparty", "Eigen"),
           "-I" + os.path.join(O3D, "3rdparty"), "-I" + O3D, "-I" + os.path.join(json, "include"),
           "-I" + os.path.join(O3D, "3rdparty", "flann"), src,
           os.path.join(core, "Integration", "UniformTSDFVolume.cpp"), os.path.join(core, "Integration", "ScalableTSDFVolume.cpp"),
           os.path.join(core, "Camera", "PinholeCameraIntrinsic.cpp")]
    cmd += [os.path.join(core, "Geometry", n + ".cpp") for n in ("Image", "ImageFactory", "RGBDImage", "RGBDImageFactory", "PointCloud",
                                                                  "PointCloudFactory", "TriangleMesh")]
    cmd += [os.path.join(core, "Utility", n + ".cpp") for n in ("Eigen", "Console", "Helper", "IJsonConvertible")]
    cmd += [os.path.join(json, "json_" + n + ".cpp") for n in ("value", "reader", "writer")]
    subprocess.check_call(cmd + ["-o", exe])
    return exe


class Cursor:
    def __init__(self, v):
        self.v, self.at = v, 0

    def take(self, n):
        out = self.v[self.at:self.at + n]
        assert len(out) == n
        self.at += n
        return out

    def volume(self, R, ctype):
        n = R ** 3
        return dict(tsdf=self.take(n).astype(np.float32), weight=self.take(n).astype(np.float32),
                    color=self.take(3 * n).astype(np.float32).reshape(n, 3) if ctype else None)

    def mesh(self):
        nv, nc, nt = [int(v) for v in self.take(3)]
        return (self.take(3 * nv).reshape(nv, 3).copy(), self.take(3 * nc).reshape(nc, 3).copy() if nc else None,
                self.take(3 * nt).astype(np.int64).reshape(nt, 3))


def run(exe, mode, case, head):
    inp, outp = os.path.join(SCRATCH, "in.bin"), os.path.join(SCRATCH, "out.bin")
    frames = case["frames"]
    h, w = frames[0][0].shape
    with open(inp, "wb") as f:
        f.write(struct.pack("<ii4di", w, h, *[float(v) for v in case["intrinsic"]], len(frames)))
        f.write(head)
        for depth, rgb, gray, E in frames:
            f.write(np.ascontiguousarray(E, "<f8").tobytes())
            f.write(np.ascontiguousarray(depth, "<f4").tobytes())
            f.write(np.ascontiguousarray(rgb, np.uint8).tobytes())
            f.write(np.ascontiguousarray(gray, "<f4").tobytes())
    subprocess.check_call([exe, mode, inp, outp], stdout=subprocess.DEVNULL)
    return Cursor(np.frombuffer(open(outp, "rb").read(), "<f8"))


def head_of(case):
    if case["scalable"]:
        return struct.pack("<iii2d", case["R"], case["color_type"], case["stride"], case["voxel_length"], case["sdf_trunc"])
    return struct.pack("<ii5d", case["R"], case["color_type"], case["length"], case["sdf_trunc"], *case["origin"])


def reference(exe, case):
    """-> the specification's volume dict holding the REFERENCE's voxels, and the reference's mesh"""
    c = run(exe, "S" if case["scalable"] else "U", case, head_of(case))
    R, t = case["R"], case["color_type"]
    if case["scalable"]:
        m = int(c.take(1)[0])
        keys = c.take(3 * m).astype(np.int64).reshape(m, 3)
        vol = S.new_scalable(case["voxel_length"], case["sdf_trunc"], t, R, case["stride"])
        for key in map(tuple, keys.tolist()):
            u = S.new_volume(vol["unit_length"], R, case["sdf_trunc"], t, np.array(key, np.float64) * vol["unit_length"])
            u.update(c.volume(R, t))
            vol["units"][key] = u
    else:
        vol = S.new_volume(case["length"], R, case["sdf_trunc"], t, case["origin"])
        vol.update(c.volume(R, t))
    mesh = c.mesh()
    assert c.at == len(c.v)
    return vol, mesh


def dense_of(case, vol):
    """-> tsdf, weight on one grid, the global index of its voxel (0, 0, 0), which voxels are cube bases, the origin"""
    R = case["R"]
    if case["scalable"]:
        f, w, _, present, lo = S._dense(vol)
        return f, w, lo * R, np.repeat(np.repeat(np.repeat(present, R, 0), R, 1), R, 2), np.zeros(3)
    f, w = vol["tsdf"].reshape(R, R, R), vol["weight"].reshape(R, R, R)
    return f, w, np.zeros(3, np.int64), np.ones((R, R, R), bool), np.asarray(case["origin"], np.float64)


def ambiguous_cubes(f, w, base_ok):
    """valid cubes with a face whose four signs alternate diagonally"""
    X, Y, Z = f.shape
    ins = f < np.float32(0.0)
    live = w != np.float32(0.0)
    corner = lambda a, d: a[d[0]:X - 1 + d[0], d[1]:Y - 1 + d[1], d[2]:Z - 1 + d[2]]
    valid = base_ok[:-1, :-1, :-1].copy()
    for i in range(8):
        valid &= corner(live, M.corner_offset(i))
    amb = np.zeros_like(valid)
    for axis in range(3):
        u, v = [a for a in range(3) if a != axis]
        for side in (0, 1):
            s = {}
            for a in (0, 1):
                for b in (0, 1):
                    d = [0, 0, 0]; d[axis], d[u], d[v] = side, a, b
                    s[(a, b)] = corner(ins, d)
            amb |= (s[(0, 0)] == s[(1, 1)]) & (s[(0, 1)] == s[(1, 0)]) & (s[(0, 0)] != s[(0, 1)])
    return int(np.count_nonzero(valid & amb))


def winding(vertices, tri, spec_vertices, spec_rising):
    """tsdf_mesh_spec.winding_dots of the REFERENCE's triangles: a reference vertex takes the edge of the specification's
    vertex at the same position (the rows are equal as multisets: asserted by the caller)"""
    at = {tuple(p.view(np.uint64)): i for i, p in enumerate(spec_vertices)}
    rising = np.array([spec_rising[at[tuple(p.view(np.uint64))]] for p in vertices])
    return M.winding_dots(vertices, tri, rising)


def sha(a):
    return np.frombuffer(hashlib.sha256(np.ascontiguousarray(a, np.float64).tobytes()).digest(), np.uint8).copy()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--time", action="store_true")
    args = ap.parse_args()
    exe = build()
    fix = {}
    signs = set()
    groups = {False: [], True: []}                                       # without / with ambiguous valid cubes
    for name in cases.NAMES:
        case = cases.load(name)
        vol, (vertices, colors, tri) = reference(exe, case)
        # the tests re-integrate with tsdf_spec: it must give the reference's voxels bit for bit
        mine = cases.spec_volume(case)
        pairs = [(mine["units"][k], vol["units"][k]) for k in sorted(vol["units"])] if case["scalable"] else [(mine, vol)]
        if case["scalable"]:
            assert sorted(mine["units"]) == sorted(vol["units"]), name
        for m, r in pairs:
            for key in ("tsdf", "weight") + (("color",) if case["color_type"] else ()):
                assert np.array_equal(m[key].view(np.uint32), r[key].view(np.uint32)), (name, key)
        f, w, _, base_ok, _ = dense_of(case, vol)
        amb = ambiguous_cubes(f, w, base_ok)
        if name == "ambig":
            assert amb >= 8, amb
        groups[amb > 0].append(name)
        assert (colors is None) == (case["color_type"] == 0) and len(tri) > 0
        rows = M.sort_rows_bits(vertices, colors) if colors is not None else M.sort_rows_bits(vertices)
        euler, boundary, repeated = M.mesh_stats(vertices, tri)
        assert repeated == 0, name
        if name == "plane":
            assert len(np.unique(vertices, axis=0)) < len(vertices)
            zero = sum(int(np.count_nonzero(v["tsdf"][v["weight"] != 0] == 0)) for v in ([vol] if not case["scalable"] else vol["units"].values()))
            assert zero > 0
        # the specification against the reference, here too (the tests repeat it from the fixture)
        sv, sc, st, rising = (M.extract_scalable if case["scalable"] else M.extract_uniform)(vol, with_edges=True)
        srows = M.sort_rows_bits(sv, sc) if sc is not None else M.sort_rows_bits(sv)
        assert np.array_equal(srows.view(np.uint64), rows.view(np.uint64)), name
        dots, flat = winding(vertices, tri, sv, rising)
        signs |= set(np.sign(dots).astype(int).tolist())
        if name == "plane":
            assert flat > 0
        print("%s: %d vertices, %d triangles (the specification: %d), V - E + F = %d, %d boundary edges, %d ambiguous cubes, "
              "%d triangles of zero area, min |normal . direction| / voxel^2 %.3g"
              % (name, len(vertices), len(tri), len(st), euler, len(boundary), amb, flat, float(np.abs(dots).min()) / case["voxel_length"] ** 2))
        fix[name + "_nv"] = np.int64(len(vertices)); fix[name + "_nt"] = np.int64(len(tri))
        fix[name + "_euler"] = np.int64(euler); fix[name + "_ambiguous"] = np.int64(amb)
        fix[name + "_rows_sha"] = sha(rows)
        if len(rows) <= 1500:
            fix[name + "_rows"] = rows
        fix[name + "_boundary_n"] = np.int64(len(boundary)); fix[name + "_boundary_sha"] = sha(boundary)
        if len(boundary) <= 600:
            fix[name + "_boundary"] = boundary
    assert len(signs) == 1 and 0 not in signs, signs
    print("compared in full (no ambiguous cube): %s; vertices and manifoldness only: %s" % (groups[False], groups[True]))
    assert sorted(groups[False]) == sorted(cases.UNAMBIGUOUS), groups
    fix["winding_sign"] = np.int64(signs.pop())
    print("winding_sign %d" % int(fix["winding_sign"]))
    out = os.path.join(HERE, "tsdf_mesh.npz")
    np.savez_compressed(out, **fix)
    print("tsdf_mesh.npz: %d bytes" % os.path.getsize(out))
    if os.path.getsize(out) > 512 * 1024:
        raise SystemExit("the fixture is larger than 512 KB")
    if args.time:
        big, kb = scene.frames(640, 480, 1)
        t0 = time.perf_counter()
        case = dict(frames=big, intrinsic=kb, scalable=False, R=512, color_type=1, length=4.0, sdf_trunc=0.04, origin=(-2.0, -2.0, -2.0))
        r = run(exe, "Utime", case, head_of(case)).v
        print("reference on this CPU (one thread): uniform 512^3, RGB8, 640 x 480: ExtractTriangleMesh %.1f ms (%d vertices, %d triangles)"
              % (r[0] * 1e3, int(r[1]), int(r[2])))
        case = dict(frames=big, intrinsic=kb, scalable=True, R=16, color_type=1, stride=4, voxel_length=4.0 / 512.0, sdf_trunc=0.04)
        r = run(exe, "Stime", case, head_of(case)).v
        print("reference on this CPU (one thread): scalable, voxel 4 / 512 m, sdf_trunc 0.04, units of 16, stride 4, RGB8, 640 x 480: "
              "ExtractTriangleMesh %.1f ms (%d units, %d vertices, %d triangles); both took %.1f s"
              % (r[0] * 1e3, int(r[1]), int(r[2]), int(r[3]), time.perf_counter() - t0))


if __name__ == "__main__":
    main()
