"""Generate tests/golden/colormap.npz: what the compiled reference computes for the scene of tests/colormap_scene.py, which
tests/test_colormap.py pins the numpy specification (tests/colormap_spec.py) and the library with.  Run once where the
reference checkout exists; the fixture holds DATA only.

The generator writes a small harness of its own into a scratch directory outside the repository, compiles it there
(the harness includes the reference's Core/ColorMap/ColorMapOptimization.cpp to reach the functions of its unnamed
namespace; with it Core/Geometry, Core/Camera, Core/Utility and jsoncpp), runs it with ONE OpenMP thread and records:

  intrinsic, extrinsics0, vertices_sha, option_*          the inputs (the frames and vertices are rebuilt from the scene module;
                                                          their digests are checked by the tests)
  img_sha (n x 3 x 32), img_rows (n x 3 x 3 x w)          SHA-256 of gray, dx, dy of every frame and their rows 0, h // 2, h - 1
  mask_k0, mask_k1, mask_k3 (n x h x w uint8)             the dilated masks for half-sizes 0, 1 and 3 (3: the tests' option)
  vis_n (n), vis_list (concatenated int32)                the cameras' visible vertices, sorted
  proxy0                                                  the proxies before iteration 1
  extr_1, extr_2, extr_8                                  the extrinsics after 1, 2 and 8 iterations (after 0: extrinsics0, asserted)
  colors_0, colors_8                                      the vertex colours after 0 and after 8 iterations
  spec_residual (8), pose_spread                          the specification's residual history; the largest entry-wise distance
                                                          among the reference, the specification with sequential sums and the
                                                          specification with pairwise sums after 8 iterations (at least 1e-15)

It asserts that every branch is met (vertices no camera sees, a depth-0 pixel, a depth above maximum_allowable_depth, a
masked pixel and a dilation that adds to the mask, a vertex behind a camera, a camera that sees under 5 % of the vertices
but at least 50, vertices rejected by the margin), that the specification equals the reference at the levels of the tests,
that the residual falls, and that the decisions are STABLE: the specification run again with every initial extrinsic entry
scaled by (1 + 1e-12) and by (1 - 1e-12) takes the same visibility bits, margin tests and rounded pixels at every iteration.
Otherwise the fixture would pin a rounding and not the algorithm.

With --time it also times the reference on the inputs of tools/colormap_probe.py with 0 and with 20 iterations (this machine's
CPU, up to 8 OpenMP threads; printed, not stored: the difference over 20 is its time per iteration).
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
SCRATCH = os.environ.get("VISMA_SCRATCH") or tempfile.mkdtemp(prefix="colormap_")      # outside the repository
sys.path.insert(0, os.path.join(ROOT, "tests"))
import colormap_scene as scene  # noqa: E402
import colormap_spec as S  # noqa: E402

HARNESS = r'''
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include <Core/ColorMap/ColorMapOptimization.cpp>
using namespace open3d;
static void rd(FILE *f, void *p, size_t n) { if (fread(p, 1, n, f) != n) std::exit(2); }
static void wd(FILE *o, double v) { fwrite(&v, 8, 1, o); }
static double now() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }
static void wimg(FILE *o, const Image &im)
{
    for (int i = 0; i < im.width_ * im.height_; i++)
        wd(o, im.bytes_per_channel_ == 4 ? (double)((const float *)im.data_.data())[i] : (double)im.data_[i]);
}
static void wposes(FILE *o, const PinholeCameraTrajectory &cam)
{
    for (auto &E : cam.extrinsic_) for (int i = 0; i < 16; i++) wd(o, E(i / 4, i %% 4));
}
int main(int argc, char **argv)
{
    FILE *f = std::fopen(argv[2], "rb"), *o = std::fopen(argv[3], "wb");
    if (!f || !o) return 2;
    int W, H, n, nv, dil; double k[4], opt[4];
    rd(f, &W, 4); rd(f, &H, 4); rd(f, k, 32); rd(f, &n, 4); rd(f, &nv, 4); rd(f, opt, 32); rd(f, &dil, 4);
    ColorMapOptmizationOption option(false, 16, 0.316, opt[0], opt[1], opt[2], opt[3], dil);
    PinholeCameraTrajectory cam;
    cam.intrinsic_ = PinholeCameraIntrinsic(W, H, k[0], k[1], k[2], k[3]);
    std::vector<RGBDImage> frames((size_t)n);
    for (auto &fr : frames) {
        double e[16]; rd(f, e, 128);
        Eigen::Matrix4d E;
        for (int i = 0; i < 16; i++) E(i / 4, i %% 4) = e[i];
        cam.extrinsic_.push_back(E);
        fr.depth_.PrepareImage(W, H, 1, 4); rd(f, fr.depth_.data_.data(), (size_t)W * H * 4);
        fr.color_.PrepareImage(W, H, 3, 1); rd(f, fr.color_.data_.data(), (size_t)W * H * 3);
    }
    TriangleMesh mesh;
    mesh.vertices_.resize((size_t)nv);
    for (auto &v : mesh.vertices_) { double p[3]; rd(f, p, 24); v = Eigen::Vector3d(p[0], p[1], p[2]); }
    if (!std::strcmp(argv[1], "stages")) {
        std::vector<std::shared_ptr<Image>> gray, dx, dy;
        std::tie(gray, dx, dy) = MakeGradientImages(frames);
        for (int i = 0; i < n; i++) { wimg(o, *gray[i]); wimg(o, *dx[i]); wimg(o, *dy[i]); }
        auto masks = MakeDepthMasks(frames, option);
        for (int i = 0; i < n; i++) wimg(o, masks[i]);
        std::vector<std::vector<int>> v2i, i2v;
        std::tie(v2i, i2v) = MakeVertexAndImageVisibility(mesh, frames, masks, cam, option);
        for (int i = 0; i < n; i++) { wd(o, (double)i2v[i].size()); for (int j : i2v[i]) wd(o, (double)j); }
        std::vector<double> proxy;
        SetProxyIntensityForVertex(mesh, gray, cam, v2i, proxy);
        for (double p : proxy) wd(o, p);
    } else {
        double t0 = now();
        ColorMapOptimization(mesh, frames, cam, option);
        double t = now() - t0;
        if (!std::strcmp(argv[1], "time")) { wd(o, t); }
        else { wposes(o, cam); for (auto &c : mesh.vertex_colors_) { wd(o, c(0)); wd(o, c(1)); wd(o, c(2)); } }
    }
    std::fclose(o);
    return 0;
}
'''


def build():
    os.makedirs(SCRATCH, exist_ok=True)
    src = os.path.join(SCRATCH, "harness.cpp")
    with open(src, "w") as f:
        f.write(HARNESS % {})
    exe = os.path.join(SCRATCH, "harness")
    core = os.path.join(O3D, "src", "Core")
    json = os.path.join(O3D, "3rdparty", "jsoncpp")
    # (sections of functions nothing here calls -- the k-d tree users of TriangleMesh.cpp, the mesh readers -- are dropped at
    #  the link, and with them their references to libraries this harness does not have)
    cmd = ["g++", "-std=c++11", "-O2", "-fopenmp", "-w", "-ffunction-sections", "-fdata-sections", "-Wl,--gc-sections",
           "-I" + os.path.join(O3D, "src"), "-I" + os.path.join(O3D, "3rdparty", "Eigen"),
           "-I" + os.path.join(O3D, "3rdparty"), "-I" + O3D, "-I" + os.path.join(json, "include"),
           "-I" + os.path.join(O3D, "3rdparty", "flann"), src,
           os.path.join(core, "Camera", "PinholeCameraIntrinsic.cpp"), os.path.join(core, "Camera", "PinholeCameraTrajectory.cpp")]
    cmd += [os.path.join(core, "Geometry", n + ".cpp") for n in ("Image", "ImageFactory", "RGBDImage", "RGBDImageFactory", "PointCloud",
                                                                  "TriangleMesh")]
    cmd += [os.path.join(core, "Utility", n + ".cpp") for n in ("Eigen", "Console", "Helper", "IJsonConvertible")]
    cmd += [os.path.join(json, "json_" + n + ".cpp") for n in ("value", "reader", "writer")]
    subprocess.check_call(cmd + ["-o", exe])
    return exe


def run(exe, mode, depths, colors, E, K, V, option, iterations, threads=1):
    inp, outp = os.path.join(SCRATCH, "in.bin"), os.path.join(SCRATCH, "out.bin")
    n, h, w = depths.shape
    with open(inp, "wb") as f:
        f.write(struct.pack("<ii4dii", w, h, *[float(k) for k in K], n, len(V)))
        f.write(struct.pack("<4di", float(iterations), option["maximum_allowable_depth"], option["depth_threshold_for_visiblity_check"],
                            option["depth_threshold_for_discontinuity_check"], option["half_dilation_kernel_size_for_discontinuity_map"]))
        for i in range(n):
            f.write(np.ascontiguousarray(E[i], "<f8").tobytes())
            f.write(np.ascontiguousarray(depths[i], "<f4").tobytes())
            f.write(np.ascontiguousarray(colors[i], np.uint8).tobytes())
        f.write(np.ascontiguousarray(V, "<f8").tobytes())
    subprocess.check_call([exe, mode, inp, outp], env=dict(os.environ, OMP_NUM_THREADS=str(threads)), stdout=subprocess.DEVNULL)
    return np.frombuffer(open(outp, "rb").read(), "<f8")


def sha(a):
    return np.frombuffer(hashlib.sha256(np.ascontiguousarray(a).tobytes()).digest(), np.uint8).copy()


def test_option():
    o = S.default_option()
    o["maximum_allowable_depth"] = scene.MAX_DEPTH
    return o


def decisions(V, depths, colors, E, K, option, k):
    trace = []
    st = S.State(V, depths, colors, E, K, option, trace)
    st.run(k)
    st.colours()
    return trace


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--time", action="store_true")
    args = ap.parse_args()
    exe = build()
    depths, colors, E0, K = scene.frames()
    V = scene.vertices()
    n, h, w = depths.shape
    nv = len(V)
    option = test_option()
    g = dict(intrinsic=K, extrinsics0=E0, vertices_sha=sha(V), depths_sha=sha(depths), colors_sha=sha(colors),
             option_maximum_allowable_depth=np.float64(option["maximum_allowable_depth"]))

    # ---- the stages ----
    masks = {}
    for k in (0, 1, 3):
        o = dict(option, half_dilation_kernel_size_for_discontinuity_map=k)
        out = run(exe, "stages", depths, colors, E0, K, V, o, 0)
        at = 3 * n * h * w
        masks[k] = out[at:at + n * h * w].reshape(n, h, w).astype(np.uint8)
        g["mask_k%d" % k] = masks[k]
        for c in range(n):
            assert np.array_equal(S.depth_mask(depths[c], o["depth_threshold_for_discontinuity_check"], k), masks[k][c]), ("mask", k, c)
    imgs = out[:3 * n * h * w].reshape(n, 3, h, w).astype(np.float32)
    g["img_sha"] = np.stack([np.stack([O_digest(imgs[c, t]) for t in range(3)]) for c in range(n)])
    g["img_rows"] = imgs[:, :, (0, h // 2, h - 1), :].copy()
    at = 4 * n * h * w
    lists = []
    for c in range(n):
        m = int(out[at]); lists.append(np.sort(out[at + 1:at + 1 + m].astype(np.int32))); at += 1 + m
    g["vis_n"] = np.array([len(x) for x in lists], np.int64)
    g["vis_list"] = np.concatenate(lists)
    g["proxy0"] = out[at:at + nv].copy()
    assert at + nv == len(out)

    st = S.State(V, depths, colors, E0, K, option)
    for c in range(n):
        for t, im in enumerate((st.gray[c], st.dx[c], st.dy[c])):
            assert np.array_equal(im.view(np.uint32), imgs[c, t].view(np.uint32)), ("image", c, t)
        assert np.array_equal(st.lists[c], lists[c]), ("visibility", c)
    assert np.array_equal(st.proxy(), g["proxy0"]), "proxy"

    # ---- every branch ----
    frac = g["vis_n"] / nv
    assert (~st.vis.any(axis=0)).sum() > 50, "vertices no camera sees"
    assert (depths == 0).any() and (depths > option["maximum_allowable_depth"]).any()
    assert all((masks[0][c] == 255).any() and (masks[3][c] != masks[1][c]).any() and (masks[1][c] != masks[0][c]).any() for c in range(n))
    assert any(S.transform(E0[c], V)[2].min() < 0 for c in range(n)), "a vertex behind a camera"
    assert ((frac < 0.05) & (g["vis_n"] >= 50)).any(), ("a sparse camera", g["vis_n"])
    hit_deep = hit_mask = False
    for c in range(n):
        u, v, z = S.project(E0[c], K, V)
        ok = (z >= 0) & (S.round_pixel(u) >= 0) & (S.round_pixel(u) < w) & (S.round_pixel(v) >= 0) & (S.round_pixel(v) < h)
        ud, vd = S.round_pixel(u)[ok], S.round_pixel(v)[ok]
        hit_deep |= bool((depths[c][vd, ud] > option["maximum_allowable_depth"]).any())
        hit_mask |= bool((masks[3][c][vd, ud] == 255).any())
    assert hit_deep and hit_mask, "a vertex on a pixel that is too deep, and one on a masked pixel"
    p0 = st.proxy()
    assert any(len(st.terms(c, p0)) < len(st.lists[c]) for c in range(n)), "the margin rejects a visible vertex"

    # ---- the runs ----
    ref = {}
    for k in (0, 1, 2, 8):
        out = run(exe, "run", depths, colors, E0, K, V, option, k)
        ref[k] = (out[:16 * n].reshape(n, 4, 4).copy(), out[16 * n:].reshape(nv, 3).copy())
    assert np.array_equal(ref[0][0], E0)
    for k in (1, 2, 8):
        g["extr_%d" % k] = ref[k][0]
    g["colors_0"], g["colors_8"] = ref[0][1], ref[8][1]
    spec = {}
    for how in ("sequential", "pairwise"):
        s = S.State(V, depths, colors, E0, K, option)
        if how == "pairwise":
            assert np.abs(s.colours() - ref[0][1]).max() <= 1e-15
        res = s.run(8, how)
        spec[how] = (s.E.copy(), s.colours(), res)
    spread = max(np.abs(spec["sequential"][0] - ref[8][0]).max(), np.abs(spec["pairwise"][0] - ref[8][0]).max(),
                 np.abs(spec["sequential"][0] - spec["pairwise"][0]).max())
    print("pose spread after 8 iterations: %.3g" % spread)
    g["pose_spread"] = np.float64(max(spread, 1e-15))
    res = spec["pairwise"][2]
    g["spec_residual"] = res
    print("residual:", res)
    assert res[7] < res[0], "the residual falls"
    moved = np.abs(ref[8][0] - E0).max()
    print("largest pose change over 8 iterations: %.3g" % moved)
    assert moved > 1e-4
    for how in spec:
        assert np.abs(spec[how][1] - ref[8][1]).max() <= 1e-15, ("colours", how, np.abs(spec[how][1] - ref[8][1]).max())

    # ---- stable decisions ----
    base = decisions(V, depths, colors, E0, K, option, 8)
    for f in (1 + 1e-12, 1 - 1e-12):
        other = decisions(V, depths, colors, E0 * f, K, option, 8)
        assert len(base) == len(other)
        for i, (a, b) in enumerate(zip(base, other)):
            assert np.array_equal(a, b), ("an unstable decision", f, i)

    path = os.path.join(HERE, "colormap.npz")
    np.savez_compressed(path, **g)
    print(path, os.path.getsize(path), "bytes; visible:", g["vis_n"], "of", nv)

    if args.time:
        sys.path.insert(0, os.path.join(ROOT, "tools"))
        import colormap_probe
        d, c, E, K2, V2 = colormap_probe.workload()
        threads = min(8, os.cpu_count() or 1)
        for k in (0, 20):                                # (0: images, masks, visibility and colours alone)
            t0 = time.time()
            out = run(exe, "time", d, c, E, K2, V2, S.default_option(), k, threads)
            print("reference, %d OpenMP threads, %d iterations: %.2f s in ColorMapOptimization (%.1f s with the harness's input)"
                  % (threads, k, out[0], time.time() - t0))


def O_digest(a):
    import odometry_spec
    return odometry_spec.image_digest(a)


if __name__ == "__main__":
    main()
