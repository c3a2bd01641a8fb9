"""Generate tests/golden/colormap_warp.npz: what the compiled reference computes with non_rigid_camera_coordinate set, for the
scene of tests/colormap_scene.py with number_of_vertical_anchors 5 (a 7 x 5 field, 76 unknowns per camera) and 16 (the
default), and for the distorted copy of tests/colormap_warp_scene.py.  tests/test_colormap_warp.py pins the numpy
specification (tests/colormap_warp_spec.py) with it, tests/test_colormap_warp_gpu.py the library.  Run once where the reference
checkout exists; the fixture holds DATA only.

It works the way gen_colormap.py works (whose build() it uses): a harness of its own, written to a scratch directory outside
the repository, includes the reference's Core/ColorMap/ColorMapOptimization.cpp to reach its unnamed namespace, and runs with
ONE OpenMP thread.  The harness calls OptimizeImageCoorNonrigid with maximum_iteration 1 over and over -- the state (poses,
fields) carries over and every call begins and ends with the proxies, so k calls are one call of k iterations -- and
writes the state after every one.  Per anchors A in (5, 16), keys a{A}_*:

  weight                                  non_rigid_anchor_point_weight of the run (WEIGHTS below)
  shape (aw, ah), step, flow0             the anchor shape and the initial flow
  proxy0                                  the proxies under the initial field
  extr_1, extr_2, extr_8, flow_1, flow_2, flow_8   extrinsics and flows after 1, 2 and 8 iterations
  colors_0, colors_8                      the vertex colours after 0 and 8 iterations
  rr, rr_reg (8 each)                     the specification's residual histories (sequential sums, dense solve); the
                                          reference prints its own with six decimals: asserted equal at that precision
  pose_spread, flow_spread                the largest entry-wise distance after 8 iterations among four runs: the compiled
                                          reference; the specification with sequential sums and a dense solve; with pairwise
                                          sums; with the library's banded solve (floored at 1e-15)
and dist_rigid_8, dist_non_rigid_8: the reference's data residual on the distorted scene after 8 rigid and after 8 non-rigid
iterations (default anchors).

It asserts that every branch is met (a visit rejected by the warped margin, a camera with count == 0, a cell with no visit,
a visit with p < 0 in cell 0 -- the last two on variants of the scene that it builds and checks against the reference but
does not store), that no visit of a pinned run falls under deviation 1, that the decisions are STABLE (every truncation,
rounding and margin decision of every pinned iteration unchanged with the initial extrinsics scaled by 1 +- 1e-12), and that
on the distorted scene the non-rigid residual after 8 iterations is below the rigid one.

With --time it also times the reference on the inputs of tools/colormap_warp_probe.py (printed, not stored).
Nothing compiled and no reference text is kept."""
import argparse
import os
import re
import struct
import subprocess
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)
import gen_colormap as G  # noqa: E402
import colormap_spec as S  # noqa: E402
import colormap_warp_scene as scene  # noqa: E402
import colormap_warp_spec as WS  # noqa: E402

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
int main(int argc, char **argv)
{
    FILE *f = std::fopen(argv[2], "rb"), *o = std::fopen(argv[3], "wb");
    if (!f || !o) return 2;
    int W, H, n, nv, dil, anchors, iters; double k[4], opt[4], weight;
    rd(f, &W, 4); rd(f, &H, 4); rd(f, k, 32); rd(f, &n, 4); rd(f, &nv, 4); rd(f, opt, 32); rd(f, &dil, 4);
    rd(f, &anchors, 4); rd(f, &weight, 8); rd(f, &iters, 4);
    ColorMapOptmizationOption option(true, anchors, weight, 1.0, opt[1], opt[2], opt[3], dil);
    PinholeCameraTrajectory cam;
    cam.intrinsic_ = PinholeCameraIntrinsic(W, H, k[0], k[1], k[2], k[3]);
    std::vector<RGBDImage> frames((size_t)n);
    for (auto &fr : frames) {
        double e[16]; rd(f, e, 128);
        Eigen::Matrix4d E;
        for (int i = 0; i < 16; i++) E(i / 4, i % 4) = e[i];
        cam.extrinsic_.push_back(E);
        fr.depth_.PrepareImage(W, H, 1, 4); rd(f, fr.depth_.data_.data(), (size_t)W * H * 4);
        fr.color_.PrepareImage(W, H, 3, 1); rd(f, fr.color_.data_.data(), (size_t)W * H * 3);
    }
    TriangleMesh mesh;
    mesh.vertices_.resize((size_t)nv);
    for (auto &v : mesh.vertices_) { double p[3]; rd(f, p, 24); v = Eigen::Vector3d(p[0], p[1], p[2]); }
    if (!std::strcmp(argv[1], "time")) {
        option.maximum_iteration_ = iters;
        double t0 = now();
        ColorMapOptimization(mesh, frames, cam, option);
        wd(o, now() - t0);
        std::fclose(o);
        return 0;
    }
    SetVerbosityLevel(VerbosityLevel::VerboseDebug);
    std::vector<std::shared_ptr<Image>> gray, dx, dy;
    std::tie(gray, dx, dy) = MakeGradientImages(frames);
    auto masks = MakeDepthMasks(frames, option);
    std::vector<std::vector<int>> v2i, i2v;
    std::tie(v2i, i2v) = MakeVertexAndImageVisibility(mesh, frames, masks, cam, option);
    auto fields = MakeWarpingFields(gray, option), fields0 = MakeWarpingFields(gray, option);
    wd(o, fields[0].anchor_w_); wd(o, fields[0].anchor_h_); wd(o, fields[0].anchor_step_);
    for (int j = 0; j < fields[0].flow_.size(); j++) wd(o, fields[0].flow_(j));
    std::vector<double> proxy;
    SetProxyIntensityForVertex(mesh, gray, fields, cam, v2i, proxy);
    for (double p : proxy) wd(o, p);
    auto state = [&]() {
        for (auto &E : cam.extrinsic_) for (int i = 0; i < 16; i++) wd(o, E(i / 4, i % 4));
        for (auto &fl : fields) for (int j = 0; j < fl.flow_.size(); j++) wd(o, fl.flow_(j));
        SetGeometryColorAverage(mesh, frames, fields, cam, v2i);
        for (auto &c : mesh.vertex_colors_) { wd(o, c(0)); wd(o, c(1)); wd(o, c(2)); }
    };
    state();
    for (int it = 0; it < iters; it++) {
        if (!std::strcmp(argv[1], "rigid")) OptimizeImageCoorRigid(mesh, gray, dx, dy, cam, v2i, i2v, proxy, option);
        else OptimizeImageCoorNonrigid(mesh, gray, dx, dy, fields, fields0, cam, v2i, i2v, proxy, option);
        state();
    }
    std::fclose(o);
    return 0;
}
'''


def build():
    G.HARNESS = HARNESS.replace("%", "%%")               # (gen_colormap.build() formats its text)
    return G.build()


def run(exe, mode, depths, colors, E, K, V, option, iterations, threads=1):
    """-> (the harness's doubles, the residual lines it printed: k x 2)"""
    inp, outp = os.path.join(G.SCRATCH, "in.bin"), os.path.join(G.SCRATCH, "out.bin")
    n, h, w = depths.shape
    with open(inp, "wb") as f:
        f.write(struct.pack("<ii4dii", w, h, *[float(k) for k in K], n, len(V)))
        f.write(struct.pack("<4di", 1.0, option["maximum_allowable_depth"], option["depth_threshold_for_visiblity_check"],
                            option["depth_threshold_for_discontinuity_check"], option["half_dilation_kernel_size_for_discontinuity_map"]))
        f.write(struct.pack("<idi", option["number_of_vertical_anchors"], option["non_rigid_anchor_point_weight"], int(iterations)))
        for i in range(n):
            f.write(np.ascontiguousarray(E[i], "<f8").tobytes())
            f.write(np.ascontiguousarray(depths[i], "<f4").tobytes())
            f.write(np.ascontiguousarray(colors[i], np.uint8).tobytes())
        f.write(np.ascontiguousarray(V, "<f8").tobytes())
    text = subprocess.run([exe, mode, inp, outp], env=dict(os.environ, OMP_NUM_THREADS=str(threads)), stdout=subprocess.PIPE,
                          check=True).stdout.decode()
    printed = np.array([[float(a), float(b or 0)] for a, b in re.findall(r"Residual error : ([-0-9.naife]+)(?:, reg : ([-0-9.naife]+))?", text)])
    return np.frombuffer(open(outp, "rb").read(), "<f8"), printed.reshape(-1, 2)


def parse(out, n, nv, iters):
    """-> aw, ah, step, flow0, proxy0, states [(E, flows, colours)] after 0 .. iters"""
    aw, ah, step = int(out[0]), int(out[1]), out[2]
    A2 = aw * ah * 2
    at = 3
    flow0 = out[at:at + A2].copy(); at += A2
    proxy0 = out[at:at + nv].copy(); at += nv
    states = []
    for _ in range(iters + 1):
        E = out[at:at + 16 * n].reshape(n, 4, 4).copy(); at += 16 * n
        fl = out[at:at + n * A2].reshape(n, A2).copy(); at += n * A2
        col = out[at:at + 3 * nv].reshape(nv, 3).copy(); at += 3 * nv
        states.append((E, fl, col))
    assert at == len(out)
    return aw, ah, step, flow0, proxy0, states


# The default weight, 0.316, with 5 anchors.  With 16 anchors of 4 pixels on 83 x 61 images a cell has a handful of visits, the
# regulariser (weight = 0.316 * count / n_vertex: about 0.02) holds nothing, single anchors jump by pixels and within five
# iterations visits fall under deviation 1 (the reference reads a wrapped anchor there): the pinned run takes weight 1.0.
WEIGHTS = {5: 0.316, 16: 1.0}


def test_option(anchors):
    o = S.default_option()
    o["maximum_allowable_depth"] = scene.scene.MAX_DEPTH
    o["number_of_vertical_anchors"] = anchors
    o["non_rigid_anchor_point_weight"] = WEIGHTS[anchors]
    return o


def library_solve(*args):
    from visma_amd import _lib
    return _lib.color_map_solve_non_rigid(*args)


def decisions(V, depths, colors, E, K, option, k):
    trace = []
    st = WS.State(V, depths, colors, E, K, option, trace)
    st.colours()
    st.run(k)
    st.colours()
    return trace, st


def against_reference(exe, V, depths, colors, E, K, option, k, what):
    """the specification follows the reference over k iterations -> the reference's states, the specification's State"""
    out, printed = run(exe, "warp", depths, colors, E, K, V, option, k)
    aw, ah, step, flow0, proxy0, states = parse(out, len(E), len(V), k)
    st = WS.State(V, depths, colors, E, K, option)
    assert (st.aw, st.ah, st.anchor_step) == (aw, ah, step) and np.array_equal(st.flow_init, flow0), what
    assert np.array_equal(st.proxy(), proxy0), (what, "proxy")
    hist = st.run(k, "sequential")
    print("%s: |pose - reference| %.3g, |flow - reference| %.3g after %d iterations" %
          (what, np.abs(st.E - states[k][0]).max(), np.abs(st.flows - states[k][1]).max(), k))
    assert np.abs(st.E - states[k][0]).max() < 1e-9 and np.abs(st.flows - states[k][1]).max() < 1e-7, what
    assert np.allclose(hist, printed, rtol=0, atol=1.01e-6), (what, hist, printed)
    return states, st, hist


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--time", action="store_true")
    args = ap.parse_args()
    exe = build()
    depths, colors, E0, K = scene.frames()
    V = scene.vertices()
    n, nv = len(E0), len(V)
    g = dict(intrinsic=K, extrinsics0=E0, vertices_sha=G.sha(V), depths_sha=G.sha(depths), colors_sha=G.sha(colors))
    for anchors in (5, 16):
        option = test_option(anchors)
        key = "a%d_" % anchors
        out, printed = run(exe, "warp", depths, colors, E0, K, V, option, 8)
        aw, ah, step, flow0, proxy0, ref = parse(out, n, nv, 8)
        assert np.array_equal(ref[0][0], E0) and np.array_equal(ref[0][1], np.tile(flow0, (n, 1)))
        g[key + "weight"] = np.float64(option["non_rigid_anchor_point_weight"])
        g[key + "shape"], g[key + "step"], g[key + "flow0"], g[key + "proxy0"] = np.array([aw, ah]), np.float64(step), flow0, proxy0
        for k in (1, 2, 8):
            g[key + "extr_%d" % k], g[key + "flow_%d" % k] = ref[k][0], ref[k][1]
        g[key + "colors_0"], g[key + "colors_8"] = ref[0][2], ref[8][2]
        runs = {}
        for name, how, solve in (("sequential", "sequential", "dense"), ("pairwise", "pairwise", "dense"), ("banded", "sequential", library_solve)):
            st = WS.State(V, depths, colors, E0, K, option)
            if name == "sequential":
                assert (st.aw, st.ah, st.anchor_step) == (aw, ah, step) and np.array_equal(st.flow_init, flow0)
                assert np.array_equal(st.proxy(), proxy0), "proxy0"
                assert np.abs(st.colours() - ref[0][2]).max() <= 1e-15
            hist = st.run(8, how, solve)
            runs[name] = (st.E.copy(), st.flows.copy(), hist, st)
            assert np.abs(st.colours() - ref[8][2]).max() <= 1e-15, ("colours", name, np.abs(st.colours() - ref[8][2]).max())
        hist = runs["sequential"][2]
        assert np.allclose(hist, printed, rtol=0, atol=1.01e-6), (hist, printed)
        g[key + "rr"], g[key + "rr_reg"] = hist[:, 0].copy(), hist[:, 1].copy()
        all_E = [ref[8][0]] + [r[0] for r in runs.values()]
        all_F = [ref[8][1]] + [r[1] for r in runs.values()]
        g[key + "pose_spread"] = np.float64(max(1e-15, max(np.abs(a - b).max() for a in all_E for b in all_E)))
        g[key + "flow_spread"] = np.float64(max(1e-15, max(np.abs(a - b).max() for a in all_F for b in all_F)))
        print("anchors %d: %d x %d, step %.6g; pose spread %.3g, flow spread %.3g; largest flow change %.3g px" %
              (anchors, aw, ah, step, g[key + "pose_spread"], g[key + "flow_spread"], np.abs(ref[8][1] - flow0).max()))
        print("  rr", hist[:, 0], "\n  rr_reg", hist[:, 1])
        # every branch of the pinned runs, and none under deviation 1
        info = runs["sequential"][3].info
        assert all(i["skipped"] == 0 for i in info), "a visit under deviation 1 in a pinned run"
        assert any(i["rejected"] > 0 for i in info), "the warped margin rejects a visit"
        rows, _ = runs["sequential"][3].cell_sums()
        assert (rows[:, :, 120] == 0).any() and (rows[:, :, 120] > 0).any(), "a cell with no visit"
        # stable decisions
        base, _ = decisions(V, depths, colors, E0, K, option, 8)
        for f in (1 + 1e-12, 1 - 1e-12):
            other, _ = decisions(V, depths, colors, E0 * f, K, option, 8)
            assert len(base) == len(other)
            for i, (a, b) in enumerate(zip(base, other)):
                assert np.array_equal(a, b), ("an unstable decision", anchors, f, i)

    # ---- branches the pinned scene does not meet: checked against the reference, not stored ----
    option = test_option(5)
    d1, c1, e1 = scene.scene.turned_away()                                    # a camera with count == 0
    dd, cc, EE = np.concatenate([depths, d1[None]]), np.concatenate([colors, c1[None]]), np.concatenate([E0, e1[None]])
    states, st, _ = against_reference(exe, V, dd, cc, EE, K, option, 2, "a camera without a visit")
    assert len(st.lists[-1]) == 0 and np.array_equal(states[2][0][-1], e1) and np.array_equal(states[2][1][-1], states[0][1][-1])
    assert np.array_equal(st.E[-1], e1) and np.array_equal(st.flows[-1], st.flow_init)
    # p < 0 in cell 0: the visibility is that of prepare; a camera moved afterwards (set_extrinsics) sees its
    # list further left, and a field pushed right by 25 pixels (set_flow) brings u in (-step, 0) back inside the margin.  The
    # reference has no such entry points: here the specification alone decides (tests/test_colormap_warp_gpu.py runs the same)
    st = WS.State(V, depths, colors, E0, K, option)
    st.E[0, 0, 3] -= 0.3
    st.flows[0, 0::2] += 25.0
    st.info = []
    st.cell_sums()
    print("moved camera:", st.info[0])
    assert st.info[0]["negative_p"] > 0, "p < 0 in cell 0 is met by the moved camera"

    # ---- the distorted scene ----
    depths2, colors2, E2, K2 = scene.distorted_frames()
    option = test_option(16)
    out, printed_n = run(exe, "warp", depths2, colors2, E2, K2, V, option, 9)
    out, printed_r = run(exe, "rigid", depths2, colors2, E2, K2, V, option, 9)
    print("distorted scene, data residual per iteration\n  rigid    ", printed_r[:, 0], "\n  non-rigid", printed_n[:, 0])
    # (iteration k + 1 prints the residual of the state after k iterations)
    g["dist_rigid_8"], g["dist_non_rigid_8"] = np.float64(printed_r[8, 0]), np.float64(printed_n[8, 0])
    assert printed_n[8, 0] < printed_r[8, 0], "the warping fields absorb what no pose explains"

    path = os.path.join(HERE, "colormap_warp.npz")
    np.savez_compressed(path, **g)
    print(path, os.path.getsize(path), "bytes")

    if args.time:
        sys.path.insert(0, os.path.join(ROOT, "tools"))
        import colormap_warp_probe
        d, c, E, K3, V3 = colormap_warp_probe.workload()
        threads = min(8, os.cpu_count() or 1)
        for k in (0, 1, 2):                              # (with 4 the reference aborts on this input: an anchor index out of range)
            t0 = time.time()
            inp_option = dict(S.default_option())
            out, _ = run(exe, "time", d, c, E, K3, V3, inp_option, k, threads)
            print("reference, %d OpenMP threads, %d non-rigid iterations: %.2f s in ColorMapOptimization (%.1f s with the harness's input)"
                  % (threads, k, out[0], time.time() - t0))


if __name__ == "__main__":
    main()
