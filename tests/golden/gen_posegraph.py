"""Generate tests/golden/posegraph.npz: what the compiled reference computes for the inputs tests/test_information.py and
tests/test_posegraph.py pin their numpy specification (tests/posegraph_spec.py) and the library with.  Run once where the
reference checkout exists; the fixture holds DATA only.

The generator writes a small harness of its own into a scratch directory, compiles it there together with the reference's
PoseGraph.cpp, TransformationEstimation.cpp, Feature.cpp, CorrespondenceChecker.cpp, KDTreeFlann.cpp, PointCloud.cpp,
Utility/{IJsonConvertible,Eigen,Console,Helper,Timer}.cpp and jsoncpp (the harness includes Registration.cpp and
GlobalOptimization.cpp themselves: GetRegistrationResultAndCorrespondences, ComputeZeta and ComputeLinearSystem live in
their unnamed namespaces), runs it and records:

  information matrices, on every third point of fragments.npz, at three poses (fragments.npz: init, the identity, init moved
  5 m away: no pair inside the radius):
    info_T, info_max_dist        the poses and the radius
    info_ref_1, info_ref_3       GetInformationMatrixFromPointClouds with 1 and with 3 OpenMP threads
                                 (= sum G^T G + 2 I and + 4 I: the identity quirk visma_icp.h describes)
    info_pairs_<p>               the reference's correspondence set at pose p (K x 2: source, target)
  pose graphs g0 .. g4 (a loop with exact relative poses and perturbed node poses each; numpy seed [20261019, graph, attempt],
  the first attempt that passes the margin test below):
    g0   6 nodes, a false UNCERTAIN loop closure (the reference prunes it), reference_node -1
    g1   8 nodes, a false loop closure marked CERTAIN (kept), reference_node 0
    g2   5 nodes, INVALID: the edge 2 -> 3 is missing (comes back untouched)
    g3   4 nodes, a clean loop, reference_node 0
    g4  12 nodes, two loop closures, one of them false and uncertain, reference_node -1
    per graph: <g>_poses, <g>_edge_nodes (E x 2), <g>_edge_T, <g>_edge_info, <g>_edge_uncertain, <g>_edge_confidence,
    <g>_option (max_correspondence_distance, edge_prune_threshold, preference_loop_closure, reference_node),
    <g>_zeta, <g>_H, <g>_b (ComputeZeta / ComputeLinearSystem at the input), and per method m in (gn, lm):
    <g>_<m>_poses, <g>_<m>_edge_nodes, <g>_<m>_edge_confidence (GlobalOptimization's output)
  The edges' information matrices are the recorded ones (minus their identity terms), i.e. of realistic shape.

Branch margins: for every graph and method the specification's run is traced; the generator prints the test that decided
the run and the smallest factor between the two sides of a deciding test (one that fired and ended an optimisation, or the
pruning of an uncertain edge), and refuses a graph where that factor is below 10 -- a fixture that sits on a branch pins
rounding, not the algorithm -- or where any other test evaluated comes within 1 % of firing.

With --time it also times the reference's GetInformationMatrixFromPointClouds on the inputs of tools/information_probe.py
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
SCRATCH = os.environ.get("VISMA_SCRATCH") or tempfile.mkdtemp(prefix="posegraph_")      # outside the repository
sys.path.insert(0, os.path.join(ROOT, "tests"))
import posegraph_spec as S  # noqa: E402

HARNESS = r'''
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include <omp.h>
#include "%(o3d)s/src/Core/Registration/Registration.cpp"
#include "%(o3d)s/src/Core/Registration/GlobalOptimization.cpp"
using namespace open3d;
static void rd(FILE *f, void *p, size_t n) { if (fread(p, 1, n, f) != n) std::exit(2); }
static void cloud(FILE *f, std::vector<Eigen::Vector3d> &v, long long n)
{
    v.resize((size_t)n);
    for (long long i = 0; i < n; i++) { double p[3]; rd(f, p, 24); v[(size_t)i] = Eigen::Vector3d(p[0], p[1], p[2]); }
}
static void wd(FILE *o, double v) { fwrite(&v, 8, 1, o); }
static Eigen::Matrix4d m4(FILE *f) { double p[16]; rd(f, p, 128); Eigen::Matrix4d T; for (int i = 0; i < 16; i++) T(i / 4, i %% 4) = p[i]; return T; }
static void w4(FILE *o, const Eigen::Matrix4d &T) { for (int i = 0; i < 16; i++) wd(o, T(i / 4, i %% 4)); }
static double now() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }
int main(int argc, char **argv)
{
    FILE *f = std::fopen(argv[2], "rb"), *o = std::fopen(argv[3], "wb");
    if (!f || !o) return 2;
    if (!std::strcmp(argv[1], "info") || !std::strcmp(argv[1], "time")) {
        long long ns, nt, nposes;
        rd(f, &ns, 8); rd(f, &nt, 8); rd(f, &nposes, 8);
        PointCloud src, tgt;
        cloud(f, src.points_, ns); cloud(f, tgt.points_, nt);
        for (long long p = 0; p < nposes; p++) {
            Eigen::Matrix4d T = m4(f);
            double max_dist; rd(f, &max_dist, 8);
            if (!std::strcmp(argv[1], "time")) {
                double t0 = now();
                Eigen::Matrix6d G = GetInformationMatrixFromPointClouds(src, tgt, max_dist, T);
                wd(o, now() - t0); wd(o, G(5, 5));
                continue;
            }
            const int threads[2] = {1, 3};
            for (int k = 0; k < 2; k++) {
                omp_set_num_threads(threads[k]);
                Eigen::Matrix6d G = GetInformationMatrixFromPointClouds(src, tgt, max_dist, T);
                for (int i = 0; i < 36; i++) wd(o, G(i / 6, i %% 6));
            }
            PointCloud pcd = src;
            if (!T.isIdentity()) pcd.Transform(T);
            KDTreeFlann tree(tgt);
            RegistrationResult r = GetRegistrationResultAndCorrespondences(pcd, tgt, tree, max_dist, T);
            wd(o, (double)r.correspondence_set_.size());
            for (auto &c : r.correspondence_set_) { wd(o, (double)c(0)); wd(o, (double)c(1)); }
        }
    } else {
        long long nn, ne;
        rd(f, &nn, 8); rd(f, &ne, 8);
        PoseGraph g;
        for (long long i = 0; i < nn; i++) g.nodes_.push_back(PoseGraphNode(m4(f)));
        for (long long e = 0; e < ne; e++) {
            int id[3]; rd(f, id, 12);
            Eigen::Matrix4d T = m4(f);
            double I[36], conf; rd(f, I, 288); rd(f, &conf, 8);
            Eigen::Matrix6d info; for (int i = 0; i < 36; i++) info(i / 6, i %% 6) = I[i];
            g.edges_.push_back(PoseGraphEdge(id[0], id[1], T, info, id[2] != 0, conf));
        }
        double op[3]; int ref; rd(f, op, 24); rd(f, &ref, 4);
        GlobalOptimizationOption option(op[0], op[1], op[2], ref);
        GlobalOptimizationConvergenceCriteria criteria;
        bool ids_ok = true;
        for (auto &e : g.edges_) ids_ok = ids_ok && e.source_node_id_ >= 0 && e.source_node_id_ < nn && e.target_node_id_ >= 0 && e.target_node_id_ < nn;
        if (!ids_ok) return 3;
        Eigen::VectorXd zeta = ComputeZeta(g);
        Eigen::MatrixXd H; Eigen::VectorXd b;
        std::tie(H, b) = ComputeLinearSystem(g, zeta);
        for (long long i = 0; i < 6 * ne; i++) wd(o, zeta(i));
        for (long long i = 0; i < 6 * nn; i++) for (long long j = 0; j < 6 * nn; j++) wd(o, H(i, j));
        for (long long i = 0; i < 6 * nn; i++) wd(o, b(i));
        for (int m = 0; m < 2; m++) {
            PoseGraph h = g;
            if (m == 0) GlobalOptimization(h, GlobalOptimizationGaussNewton(), criteria, option);
            else GlobalOptimization(h, GlobalOptimizationLevenbergMarquardt(), criteria, option);
            wd(o, (double)h.edges_.size());
            for (auto &n : h.nodes_) w4(o, n.pose_);
            for (auto &e : h.edges_) { wd(o, e.source_node_id_); wd(o, e.target_node_id_); wd(o, e.uncertain_ ? 1.0 : 0.0); wd(o, e.confidence_); }
        }
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
           os.path.join(core, "Registration", "PoseGraph.cpp"), os.path.join(core, "Registration", "TransformationEstimation.cpp"),
           os.path.join(core, "Registration", "Feature.cpp"), os.path.join(core, "Registration", "CorrespondenceChecker.cpp"),
           os.path.join(core, "Geometry", "KDTreeFlann.cpp"), os.path.join(core, "Geometry", "PointCloud.cpp")]
    cmd += [os.path.join(core, "Utility", n + ".cpp") for n in ("IJsonConvertible", "Eigen", "Console", "Helper", "Timer")]
    cmd += [os.path.join(json, "json_" + n + ".cpp") for n in ("value", "reader", "writer")]
    subprocess.check_call(cmd + ["-o", exe])
    return exe


def rigid(w, t):
    w = np.asarray(w, np.float64); th = np.linalg.norm(w)
    T = np.eye(4)
    if th > 0:
        k = w / th
        K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
        T[:3, :3] = np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * K @ K
    T[:3, 3] = t
    return T


def make_graph(rng, n, infos=None, false_edge=None, false_uncertain=True, closures=((0, -1),), drop=None, reference_node=-1,
               max_dist=0.075):
    """a loop: node i's true pose, odometry edges i -> i + 1 and loop closures with EXACT relative poses, node poses
    perturbed by up to 0.02 rad / 0.02; false_edge (i, j): a loop closure 0.4 rad / 0.5 off"""
    truth = [np.eye(4)] + [rigid(rng.normal(size=3) * 0.4, rng.normal(size=3) * 1.5) for _ in range(n - 1)]
    rel = lambda i, j: np.linalg.inv(truth[j]) @ truth[i]
    edges = []
    for i in range(n - 1):
        if drop != i:
            edges.append(S.Edge(i, i + 1, rel(i, i + 1), infos[len(edges) % len(infos)], False))
    for i, j in closures:
        edges.append(S.Edge(i, j % n, rel(i, j % n), infos[len(edges) % len(infos)], True))
    if false_edge:
        i, j = false_edge
        wrong = rigid(rng.normal(size=3) * 0.25, rng.normal(size=3) * 0.3) @ rel(i, j)
        edges.append(S.Edge(i, j, wrong, infos[len(edges) % len(infos)], false_uncertain))
    poses = [rigid(rng.normal(size=3) * 0.012, rng.normal(size=3) * 0.012) @ T for T in truth]
    option = dict(max_correspondence_distance=max_dist, edge_prune_threshold=0.25, preference_loop_closure=1.0,
                  reference_node=reference_node)
    return poses, edges, option, truth


def run_graph(exe, poses, edges, option):
    inp, outp = os.path.join(SCRATCH, "g_in.bin"), os.path.join(SCRATCH, "g_out.bin")
    with open(inp, "wb") as f:
        f.write(struct.pack("<qq", len(poses), len(edges)))
        for T in poses:
            f.write(np.ascontiguousarray(T, "<f8").tobytes())
        for e in edges:
            f.write(struct.pack("<iii", e.source, e.target, int(e.uncertain)))
            f.write(np.ascontiguousarray(e.transformation, "<f8").tobytes())
            f.write(np.ascontiguousarray(e.information, "<f8").tobytes())
            f.write(struct.pack("<d", e.confidence))
        f.write(struct.pack("<dddi", option["max_correspondence_distance"], option["edge_prune_threshold"],
                            option["preference_loop_closure"], option["reference_node"]))
    subprocess.check_call([exe, "graph", inp, outp], stdout=subprocess.DEVNULL)
    v = np.frombuffer(open(outp, "rb").read(), "<f8")
    n, E = 6 * len(poses), len(edges)
    out = {"zeta": v[:6 * E].reshape(E, 6).copy(), "H": v[6 * E:6 * E + n * n].reshape(n, n).copy(),
           "b": v[6 * E + n * n:6 * E + n * n + n].copy()}
    at = 6 * E + n * n + n
    for m in ("gn", "lm"):
        ne = int(v[at]); at += 1
        out[m + "_poses"] = v[at:at + 16 * len(poses)].reshape(-1, 4, 4).copy(); at += 16 * len(poses)
        ed = v[at:at + 4 * ne].reshape(ne, 4); at += 4 * ne
        out[m + "_edge_nodes"] = ed[:, :2].astype(np.int32)
        out[m + "_edge_confidence"] = ed[:, 3].copy()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--time", action="store_true")
    a = ap.parse_args()
    exe = build()
    frag = np.load(os.path.join(HERE, "fragments.npz"))
    src = np.ascontiguousarray(frag["src"].astype(np.float64)[::3]); tgt = np.ascontiguousarray(frag["tgt"].astype(np.float64)[::3])
    init = frag["init"].astype(np.float64).reshape(4, 4)
    max_dist = 0.1
    far = init.copy(); far[:3, 3] += 5.0
    info_T = np.stack([init, np.eye(4), far])
    inp, outp = os.path.join(SCRATCH, "in.bin"), os.path.join(SCRATCH, "out.bin")

    def write_info(s, t, Ts, r):
        with open(inp, "wb") as f:
            f.write(struct.pack("<qqq", len(s), len(t), len(Ts)))
            f.write(np.ascontiguousarray(s, "<f8").tobytes()); f.write(np.ascontiguousarray(t, "<f8").tobytes())
            for T in Ts:
                f.write(np.ascontiguousarray(T, "<f8").tobytes()); f.write(struct.pack("<d", r))

    write_info(src, tgt, info_T, max_dist)
    subprocess.check_call([exe, "info", inp, outp], stdout=subprocess.DEVNULL)
    v = np.frombuffer(open(outp, "rb").read(), "<f8")
    fix = {"info_T": info_T, "info_max_dist": max_dist}
    ref1, ref3, at = [], [], 0
    for p in range(len(info_T)):
        ref1.append(v[at:at + 36].reshape(6, 6)); ref3.append(v[at + 36:at + 72].reshape(6, 6)); at += 72
        K = int(v[at]); at += 1
        fix["info_pairs_%d" % p] = v[at:at + 2 * K].reshape(K, 2).astype(np.int32); at += 2 * K
        print("information matrix at pose %d: K = %d, (5,5) with 1 thread %.1f, with 3 threads %.1f" % (p, K, ref1[-1][5, 5], ref3[-1][5, 5]))
    fix["info_ref_1"], fix["info_ref_3"] = np.stack(ref1), np.stack(ref3)
    assert len(fix["info_pairs_2"]) == 0 and len(fix["info_pairs_0"]) > 100
    infos = [ref1[0] - 2 * np.eye(6), ref1[1] - 2 * np.eye(6)]

    recipes = [
        dict(n=6, false_edge=(1, 4), false_uncertain=True, reference_node=-1),
        dict(n=8, false_edge=(2, 6), false_uncertain=False, reference_node=0),
        dict(n=5, drop=2, reference_node=-1),
        dict(n=4, reference_node=0),
        dict(n=12, false_edge=(3, 9), false_uncertain=True, closures=((0, -1), (2, 7)), reference_node=-1),
    ]
    graphs = []
    for gi, recipe in enumerate(recipes):                 # the first attempt whose runs stay clear of every branch
        for attempt in range(1000):
            rng = np.random.default_rng([20261019, gi, attempt])
            cand = make_graph(rng, infos=infos, **recipe)
            traces = [S.global_optimization(cand[0], cand[1], m, None, cand[2])[2] for m in ("gn", "lm")]
            margin, clearance = min(t.margin() for t in traces), min(t.clearance() for t in traces)
            if margin >= 10.0 and clearance >= 1.01:
                break
            print("g%d attempt %d rejected: a deciding test within a factor %.3g of its threshold (any test: %.3g)"
                  % (gi, attempt, margin, clearance))
        else:
            raise SystemExit("g%d: no graph clear of every branch in 1000 attempts" % gi)
        graphs.append(cand)
    fix["n_graphs"] = len(graphs)
    for gi, (poses, edges, option, truth) in enumerate(graphs):
        g = "g%d" % gi
        r = run_graph(exe, poses, edges, option)
        fix[g + "_poses"] = np.stack(poses)
        fix[g + "_truth"] = np.stack(truth)
        fix[g + "_edge_nodes"] = np.array([[e.source, e.target] for e in edges], np.int32)
        fix[g + "_edge_T"] = np.stack([e.transformation for e in edges])
        fix[g + "_edge_info"] = np.stack([e.information for e in edges])
        fix[g + "_edge_uncertain"] = np.array([e.uncertain for e in edges], np.int8)
        fix[g + "_edge_confidence"] = np.array([e.confidence for e in edges])
        fix[g + "_option"] = np.array([option["max_correspondence_distance"], option["edge_prune_threshold"],
                                       option["preference_loop_closure"], option["reference_node"]])
        for k, val in r.items():
            fix[g + "_" + k] = val
        for m in ("gn", "lm"):
            P, E, tr = S.global_optimization(poses, edges, m, None, option)
            d = tr.deciding()
            dp = max(np.linalg.norm(P[i] - r[m + "_poses"][i]) / np.linalg.norm(r[m + "_poses"][i]) for i in range(len(P)))
            err = max(np.linalg.norm(np.linalg.inv(r[m + "_poses"][i]) @ r[m + "_poses"][0] - np.linalg.inv(truth[i]) @ truth[0])
                      for i in range(len(P)))
            print("%s %s: %d nodes, %d -> %d edges (spec %d); last test fired: %s; margin of the deciding tests %.3g (of any test %.3g); "
                  "spec against reference %.2e; reference against truth (relative to node 0) %.2e"
                  % (g, m, len(poses), len(edges), len(r[m + "_edge_nodes"]), len(E), d[0] if d else "none (invalid graph)",
                     tr.margin(), tr.clearance(), dp, err))
            if tr.margin() < 10.0:
                raise SystemExit("%s %s sits within a factor 10 of a branch: choose another graph" % (g, m))
            assert len(E) == len(r[m + "_edge_nodes"])
    out = os.path.join(HERE, "posegraph.npz")
    np.savez_compressed(out, **fix)
    print("posegraph.npz: %d bytes" % os.path.getsize(out))
    if a.time:
        sys.path.insert(0, os.path.join(ROOT, "tools"))
        import information_probe as P
        for name, (s, t, T, r) in P.reference_inputs().items():
            write_info(s, t, [T], r)
            subprocess.check_call([exe, "time", inp, outp], stdout=subprocess.DEVNULL)
            res = np.frombuffer(open(outp, "rb").read(), "<f8")
            print("reference on this CPU (%d hardware threads, OpenMP): GetInformationMatrixFromPointClouds, %s, %d x %d points: "
                  "%.1f ms ((5,5) = %.0f)" % (os.cpu_count(), name, len(s), len(t), res[0] * 1e3, res[1]))


if __name__ == "__main__":
    main()
