"""Pose-graph optimisation of multiway registration (visma_icp_pose_graph_zeta, visma_icp_pose_graph_linear_system,
visma_icp_global_optimization, visma_icp_pose_graph_optimize; host only, no GPU).

The yardstick is tests/golden/posegraph.npz (tests/golden/gen_posegraph.py): what the compiled reference computes for five
small graphs -- zeta, H and b at the input, and GlobalOptimization's output under both methods.  The generator rejected
every graph whose run comes within a factor 10 of a stopping or pruning threshold, so the fixture pins the algorithm, not
rounding.  tests/posegraph_spec.py (numpy) is pinned to the same fixture: the GPU end-to-end test compares with it.

Tolerances.  zeta, H, b: a fixed number of f64 operations per edge, so 1e-12 relative to the entry's sum of |term| (the
same expression over absolute values, computed here).  Poses and confidences after the optimisation: the project's gate
for a transform, relative Frobenius difference <= 1e-5.

One comparison is made modulo what the reference itself leaves undefined: Gauss-Newton on a graph WITHOUT a reference node
solves a singular system (H has the 6-dimensional null space of a common rigid motion; the reference's LDLT divides
rounding noise by rounding noise there), so the rigid motion common to all its output poses is noise -- the numpy
specification and the reference, which agree to 1e-13 under Levenberg-Marquardt, differ by 0.13 (g0) and 0.064 (g4) in the
raw poses under Gauss-Newton, while every pose relative to node 0 agrees.  For (Gauss-Newton, reference_node outside the
graph) the poses are therefore compared relative to node 0; everywhere else raw.

Reached (this library against the fixture, printed by the tests): see DESIGN.md 4.4c9."""
import ctypes as C
import os
import struct
import subprocess
import sys

import numpy as np
import pytest

import posegraph_spec as S

HERE = os.path.dirname(os.path.abspath(__file__))
G = os.path.join(HERE, "golden")
sys.path.insert(0, os.path.join(HERE, "cpp"))
import build_shim  # noqa: E402

TOL_T = 1e-5        # a transform within 1e-5 relative Frobenius
TOL_OPS = 1e-12     # zeta, H, b: relative to the entry's sum of |term|
INVALID = 1
GRAPHS = ["g0", "g1", "g2", "g3", "g4"]
METHODS = ["gn", "lm"]


@pytest.fixture(scope="module")
def golden():
    g = np.load(os.path.join(G, "posegraph.npz"))
    return {k: g[k] for k in g.files}


def graph_of(golden, g, cls):
    poses = golden[g + "_poses"]
    edges = [cls(int(s), int(t), golden[g + "_edge_T"][k], golden[g + "_edge_info"][k], bool(golden[g + "_edge_uncertain"][k]),
                 float(golden[g + "_edge_confidence"][k])) for k, (s, t) in enumerate(golden[g + "_edge_nodes"])]
    o = golden[g + "_option"]
    return poses, edges, dict(max_correspondence_distance=float(o[0]), edge_prune_threshold=float(o[1]),
                              preference_loop_closure=float(o[2]), reference_node=int(o[3]))


def rel_frobenius(A, B):
    return float(np.linalg.norm(np.asarray(A) - np.asarray(B)) / np.linalg.norm(B))


def gauge_free(golden, g, method):
    """Gauss-Newton without a reference node: the common rigid motion of the output is undefined (the module's docstring)"""
    ref = int(golden[g + "_option"][3])
    return method == "gn" and not 0 <= ref < len(golden[g + "_poses"])


def pose_difference(P, R, relative_to_node_0):
    if relative_to_node_0:
        P = [np.linalg.inv(P[0]) @ T for T in P]; R = [np.linalg.inv(R[0]) @ T for T in R]
    return max(rel_frobenius(a, b) for a, b in zip(P, R))


# ---------------------------------------------------------------------------
# CPU
# ---------------------------------------------------------------------------
NEW_SYMBOLS = ["visma_icp_pose_graph_zeta", "visma_icp_pose_graph_linear_system", "visma_icp_global_optimization",
               "visma_icp_pose_graph_optimize", "visma_icp_pose_graph_validate", "visma_icp_global_optimization_option_clamp",
               "visma_icp_global_optimization_criteria_clamp"]


def test_symbols_and_functions(lib):
    L = lib.load()
    for name in NEW_SYMBOLS:
        assert hasattr(L, name), name
    for name in ("global_optimization", "pose_graph_optimize", "pose_graph_zeta", "pose_graph_linear_system", "pose_graph_validate",
                 "global_optimization_option", "global_optimization_criteria"):
        assert callable(getattr(lib, name, None)), name
    assert [f[0] for f in lib.CPoseGraphEdge._fields_] == ["source", "target", "transformation", "information", "uncertain", "confidence"]
    assert C.sizeof(lib.CPoseGraphEdge) == 8 + 16 * 8 + 36 * 8 + 8 + 8
    assert len(lib.CGlobalOptimizationOption._fields_) == 4 and len(lib.CGlobalOptimizationCriteria._fields_) == 8


def test_options_are_clamped_as_the_reference_clamps(lib):
    o = lib.global_optimization_option()
    assert (o.max_correspondence_distance, o.edge_prune_threshold, o.preference_loop_closure, o.reference_node) == (0.075, 0.25, 1.0, -1)
    o = lib.global_optimization_option(-1.0, 1.5, -2.0, 7)
    assert (o.max_correspondence_distance, o.edge_prune_threshold, o.preference_loop_closure, o.reference_node) == (0.075, 0.25, 1.0, 7)
    o = lib.global_optimization_option(0.0, -0.1, 0.0, -5)
    assert (o.max_correspondence_distance, o.edge_prune_threshold, o.preference_loop_closure, o.reference_node) == (0.0, 0.25, 0.0, -5)
    o = lib.global_optimization_option(0.05, 1.0, 2.0, 0)
    assert (o.max_correspondence_distance, o.edge_prune_threshold, o.preference_loop_closure) == (0.05, 1.0, 2.0)
    c = lib.global_optimization_criteria()
    assert (c.max_iteration, c.min_relative_increment, c.min_relative_residual_increment, c.min_right_term, c.min_residual,
            c.max_iteration_lm, c.upper_scale_factor, c.lower_scale_factor) == (100, 1e-6, 1e-6, 1e-6, 1e-6, 20, 2. / 3., 1. / 3.)
    c = lib.global_optimization_criteria(upper_scale_factor=1.5, lower_scale_factor=-0.5)
    assert (c.upper_scale_factor, c.lower_scale_factor) == (2. / 3., 1. / 3.)
    c = lib.global_optimization_criteria(upper_scale_factor=1.0, lower_scale_factor=0.0, max_iteration=-3)
    assert (c.upper_scale_factor, c.lower_scale_factor, c.max_iteration) == (1.0, 0.0, -3)     # (only the two factors are clamped)
    assert S.clamp_option(dict(edge_prune_threshold=1.5))["edge_prune_threshold"] == 0.25
    assert S.clamp_criteria(dict(upper_scale_factor=-1))["upper_scale_factor"] == 2. / 3.


def test_argument_checks(lib, golden):
    L = lib.load()
    poses, edges, _ = graph_of(golden, "g3", lib.PoseGraphEdge)
    P, arr = lib._pose_graph_args(poses, edges)
    dp = C.POINTER(C.c_double)
    n, ne = len(P), len(edges)
    z = np.zeros(6 * ne); H = np.zeros((6 * n, 6 * n)); b = np.zeros(6 * n)
    pz, pH, pb, pP = (a.ctypes.data_as(dp) for a in (z, H, b, P))
    ok = L.visma_icp_pose_graph_zeta(pP, n, arr, ne, pz)
    assert ok == 0
    # null pointers
    assert L.visma_icp_pose_graph_zeta(None, n, arr, ne, pz) == INVALID
    assert L.visma_icp_pose_graph_zeta(pP, n, None, ne, pz) == INVALID
    assert L.visma_icp_pose_graph_zeta(pP, n, arr, ne, None) == INVALID
    assert L.visma_icp_pose_graph_linear_system(pP, n, arr, ne, None, pb) == INVALID
    assert L.visma_icp_pose_graph_linear_system(pP, n, arr, ne, pH, None) == INVALID
    assert L.visma_icp_pose_graph_linear_system(None, n, arr, ne, pH, pb) == INVALID
    cne = C.c_int(ne)
    assert L.visma_icp_global_optimization(None, n, arr, C.byref(cne), 1, None, None) == INVALID
    assert L.visma_icp_global_optimization(pP, n, None, C.byref(cne), 1, None, None) == INVALID
    assert L.visma_icp_global_optimization(pP, n, arr, None, 1, None, None) == INVALID
    assert L.visma_icp_global_optimization_option_clamp(None) == INVALID and L.visma_icp_global_optimization_criteria_clamp(None) == INVALID
    # negative counts, an unknown method
    assert L.visma_icp_pose_graph_zeta(pP, -1, arr, ne, pz) == INVALID
    assert L.visma_icp_pose_graph_zeta(pP, n, arr, -1, pz) == INVALID
    assert L.visma_icp_pose_graph_linear_system(pP, -1, arr, ne, pH, pb) == INVALID
    assert L.visma_icp_pose_graph_validate(-1, arr, ne) == -INVALID and L.visma_icp_pose_graph_validate(n, None, ne) == -INVALID
    cneg = C.c_int(-1)
    assert L.visma_icp_global_optimization(pP, n, arr, C.byref(cneg), 1, None, None) == INVALID
    assert L.visma_icp_global_optimization(pP, -1, arr, C.byref(cne), 1, None, None) == INVALID
    assert L.visma_icp_global_optimization(pP, n, arr, C.byref(cne), 2, None, None) == INVALID
    assert L.visma_icp_pose_graph_optimize(pP, n, arr, ne, -1, None, None) == INVALID
    with pytest.raises(ValueError):
        lib.global_optimization(poses, edges, "newton")
    # an edge naming a node out of range: refused where it would be read, an invalid graph (untouched) for the whole optimisation
    for bad in (-1, n):
        e2 = [lib.PoseGraphEdge(e.source, e.target, e.transformation, e.information, e.uncertain, e.confidence) for e in edges]
        e2[-1].target = bad
        with pytest.raises(lib.IcpError):
            lib.pose_graph_zeta(poses, e2)
        with pytest.raises(lib.IcpError):
            lib.pose_graph_linear_system(poses, e2)
        _, a2 = lib._pose_graph_args(poses, e2)
        assert L.visma_icp_pose_graph_optimize(pP, n, a2, ne, 1, None, None) == INVALID
        assert not lib.pose_graph_validate(n, e2)
        P2, out = lib.global_optimization(poses, e2, "lm")
        assert np.array_equal(P2, poses) and len(out) == len(e2) and out[-1].target == bad
    # empty graphs
    P0, e0 = lib.global_optimization(np.zeros((0, 4, 4)), [], "gn")
    assert len(P0) == 0 and e0 == []
    P1, e1 = lib.global_optimization(np.eye(4)[None], [], "lm")
    assert np.array_equal(P1[0], np.eye(4)) and e1 == []
    assert lib.pose_graph_validate(1, []) and not lib.pose_graph_validate(2, [])


@pytest.mark.parametrize("g", GRAPHS)
def test_zeta_and_linear_system_equal_the_reference(lib, golden, g):
    """the library AND the numpy specification against ComputeZeta / ComputeLinearSystem, per entry within 1e-12 of the sum
    of |term| of that entry"""
    worst = {}
    for name, mod, cls in (("library", lib, lib.PoseGraphEdge), ("specification", None, S.Edge)):
        poses, edges, _ = graph_of(golden, g, cls)
        sp, se, _ = graph_of(golden, g, S.Edge)
        if mod is not None:
            z = mod.pose_graph_zeta(poses, edges)
            H, b = mod.pose_graph_linear_system(poses, edges)
        else:
            z = S.zeta(list(poses), edges)
            H, b = S.linear_system(list(poses), edges)
        za = S.zeta(list(sp), se, absolute=True)
        Ha, ba = S.linear_system(list(sp), se, absolute=True)
        for what, got, want, scale in (("zeta", z, golden[g + "_zeta"], za), ("H", H, golden[g + "_H"], Ha), ("b", b, golden[g + "_b"], ba)):
            assert got.shape == want.shape
            ratio = np.abs(got - want) / np.where(scale > 0, scale, 1.0)
            assert np.all(np.abs(got - want)[scale == 0] == 0.0), (name, what)
            worst[name + " " + what] = float(ratio.max())
            assert ratio.max() <= TOL_OPS, (name, what, ratio.max())
    print(g, "largest |difference| / sum |term|:", {k: "%.2e" % v for k, v in worst.items()})


@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("g", GRAPHS)
def test_global_optimization_equals_the_reference(lib, golden, g, method):
    poses, edges, option = graph_of(golden, g, lib.PoseGraphEdge)
    P, out = lib.global_optimization(poses, edges, method, option=lib.global_optimization_option(**option))
    want_nodes = golden["%s_%s_edge_nodes" % (g, method)]
    assert [(e.source, e.target) for e in out] == [tuple(int(v) for v in r) for r in want_nodes]        # the same edges survive
    conf = np.array([e.confidence for e in out]); want_conf = golden["%s_%s_edge_confidence" % (g, method)]
    R = golden["%s_%s_poses" % (g, method)]
    dp = pose_difference(P, R, gauge_free(golden, g, method))
    dc = float(np.abs(conf - want_conf).max() / np.linalg.norm(want_conf)) if len(conf) else 0.0
    print("%s %s: poses %.3e%s, confidences %.3e, %d -> %d edges" % (g, method, dp, " (relative to node 0)" if gauge_free(golden, g, method) else "",
                                                                      dc, len(edges), len(out)))
    assert dp <= TOL_T
    assert rel_frobenius(conf, want_conf) <= TOL_T if len(conf) else True
    # the other members of a surviving edge are the input's
    for e in out:
        k = [i for i, q in enumerate(edges) if (q.source, q.target, q.uncertain) == (e.source, e.target, e.uncertain)][0]
        assert np.array_equal(e.transformation, edges[k].transformation) and np.array_equal(e.information, edges[k].information)


@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("g", GRAPHS)
def test_specification_equals_the_reference(golden, g, method):
    """the numpy specification the GPU end-to-end test compares with, pinned to the same fixture by the same gate"""
    poses, edges, option = graph_of(golden, g, S.Edge)
    P, out, _ = S.global_optimization(list(poses), edges, method, None, option)
    assert [(e.source, e.target) for e in out] == [tuple(int(v) for v in r) for r in golden["%s_%s_edge_nodes" % (g, method)]]
    assert pose_difference(P, golden["%s_%s_poses" % (g, method)], gauge_free(golden, g, method)) <= TOL_T
    want_conf = golden["%s_%s_edge_confidence" % (g, method)]
    assert rel_frobenius([e.confidence for e in out], want_conf) <= TOL_T


def test_what_the_fixture_covers(golden):
    """a false uncertain edge that is pruned, a false certain edge that is kept, an invalid graph, both kinds of
    reference_node, information matrices that are no multiples of I, 4 to 12 nodes"""
    sizes = [len(golden[g + "_poses"]) for g in GRAPHS]
    assert min(sizes) >= 4 and max(sizes) <= 12 and len(GRAPHS) >= 4
    for m in METHODS:
        assert len(golden["g0_%s_edge_nodes" % m]) == len(golden["g0_edge_nodes"]) - 1           # pruned ...
        assert [1, 4] not in golden["g0_%s_edge_nodes" % m].tolist() and golden["g0_edge_uncertain"][-1] == 1
        assert len(golden["g1_%s_edge_nodes" % m]) == len(golden["g1_edge_nodes"]) and golden["g1_edge_uncertain"][-1] == 0   # ... kept
        assert np.array_equal(golden["g2_%s_poses" % m], golden["g2_poses"])                    # invalid: untouched
        truth = golden["g0_truth"]; R = golden["g0_%s_poses" % m]
        err = max(np.linalg.norm(np.linalg.inv(R[i]) @ R[0] - np.linalg.inv(truth[i]) @ truth[0]) for i in range(len(R)))
        assert err < 1e-4, err                                                                    # and the truth is found
    assert not S.validate(len(golden["g2_poses"]), graph_of(golden, "g2", S.Edge)[1])
    assert {int(golden[g + "_option"][3]) for g in GRAPHS} >= {-1, 0}
    info = golden["g0_edge_info"][0]
    assert np.abs(info - np.diag(np.diag(info))).max() > 1.0 and info[5, 5] == round(info[5, 5])


def test_invalid_graph_comes_back_untouched(lib, golden):
    poses, edges, option = graph_of(golden, "g2", lib.PoseGraphEdge)
    assert not lib.pose_graph_validate(len(poses), edges)
    for m in METHODS:
        P, out = lib.global_optimization(poses, edges, m, option=lib.global_optimization_option(**option))
        assert np.array_equal(P, poses) and len(out) == len(edges)
        assert all(np.array_equal(a.transformation, b.transformation) and a.confidence == b.confidence for a, b in zip(out, edges))


def test_reference_node_is_unchanged_and_one_optimisation_updates_confidences(lib, golden):
    poses, edges, option = graph_of(golden, "g1", lib.PoseGraphEdge)
    P, _ = lib.global_optimization(poses, edges, "lm", option=lib.global_optimization_option(**option))
    assert rel_frobenius(P[0], poses[0]) < 1e-12
    # visma_icp_pose_graph_optimize on g0: no pruning, the false edge's confidence is what the whole optimisation prunes by
    poses, edges, option = graph_of(golden, "g0", lib.PoseGraphEdge)
    _, once = lib.pose_graph_optimize(poses, edges, "lm", option=lib.global_optimization_option(**option))
    assert len(once) == len(edges) and once[-1].confidence < 0.25 and all(e.confidence > 0.25 for e in once[:-1])


# ---------------------------------------------------------------------------
# the C++ shim
# ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def driver_bins(lib):
    import build_posegraph
    if build_shim.eigen_dir() is not None:
        build_posegraph.build()
    paths = [os.path.join(HERE, "cpp", "_build", b) for b in build_posegraph.BINS]
    if not all(os.path.exists(p) for p in paths):
        pytest.skip("posegraph driver not prebuilt and no Eigen headers here")
    return paths


EDGE_REC = 21       # the driver's record of an edge: source, target, uncertain, confidence, 16 of the transformation, information(0, 0)


def write_driver_graph(path, poses, edges, option, method):
    with open(path, "wb") as f:
        f.write(struct.pack("<qqidddi", len(poses), len(edges), METHODS.index(method), option["max_correspondence_distance"],
                            option["edge_prune_threshold"], option["preference_loop_closure"], option["reference_node"]))
        f.write(np.ascontiguousarray(poses, "<f8").tobytes())
        for e in edges:
            f.write(struct.pack("<iii", e.source, e.target, int(e.uncertain)))
            f.write(np.ascontiguousarray(e.transformation, "<f8").tobytes()); f.write(np.ascontiguousarray(e.information, "<f8").tobytes())
            f.write(struct.pack("<d", e.confidence))


@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("g", ["g0", "g1", "g2"])
def test_shim_driver_reproduces_the_fixture(lib, golden, driver_bins, tmp_path, g, method):
    """open3d::GlobalOptimization and GlobalOptimizationMethod::OptimizePoseGraph through the stand-alone headers, both Eigen
    storage orders: the fixture's output, and one optimisation equal to visma_icp_pose_graph_optimize"""
    poses, edges, option = graph_of(golden, g, lib.PoseGraphEdge)
    inp, outp = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    write_driver_graph(inp, poses, edges, option, method)
    want_P, want_E = lib.global_optimization(poses, edges, method, option=lib.global_optimization_option(**option))
    for b in driver_bins:
        p = subprocess.run([b, "graph", inp, outp], capture_output=True, text=True, timeout=120)
        assert p.returncode == 0, (b, p.returncode, p.stdout, p.stderr)
        v = np.frombuffer(open(outp, "rb").read(), "<f8")
        ne = int(v[0]); P = v[1:1 + 16 * len(poses)].reshape(-1, 4, 4); ed = v[1 + 16 * len(poses):1 + 16 * len(poses) + EDGE_REC * ne].reshape(ne, EDGE_REC)
        for row, e in zip(ed, want_E):                   # every member of a surviving edge is that edge's own
            assert np.array_equal(row[4:20].reshape(4, 4), e.transformation) and row[20] == e.information[0, 0]
        assert ed[:, :2].astype(int).tolist() == golden["%s_%s_edge_nodes" % (g, method)].tolist()
        assert np.array_equal(P, want_P) and np.array_equal(ed[:, 3], [e.confidence for e in want_E])     # the same library underneath
        assert pose_difference(P, golden["%s_%s_poses" % (g, method)], gauge_free(golden, g, method)) <= TOL_T
        rest = v[1 + 16 * len(poses) + EDGE_REC * ne:]
        assert int(rest[0]) == len(edges)                                                         # one optimisation prunes nothing
        if g == "g2":
            continue                                     # (an invalid graph: one optimisation is not defined by the fixture)
        Pc, _ = lib.pose_graph_optimize(poses, edges, method, option=lib.global_optimization_option(**option))
        assert np.array_equal(rest[1:1 + 16 * len(poses)].reshape(-1, 4, 4), Pc)


@pytest.mark.parametrize("method", METHODS)
def test_shim_keeps_the_members_of_the_edge_that_survives(lib, golden, driver_bins, tmp_path, method):
    """two uncertain edges between the same nodes, the false one first and pruned, the true one second and kept: the edge
    that comes back carries the TRUE edge's transformation and information, not the first match's"""
    poses, edges, option = graph_of(golden, "g0", lib.PoseGraphEdge)
    truth = golden["g0_truth"]
    false_edge = edges[-1]
    assert (false_edge.source, false_edge.target, false_edge.uncertain) == (1, 4, True)
    true_edge = lib.PoseGraphEdge(1, 4, np.linalg.inv(truth[4]) @ truth[1], 0.5 * false_edge.information, True)
    edges = edges + [true_edge]
    inp, outp = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    write_driver_graph(inp, poses, edges, option, method)
    want_P, want_E = lib.global_optimization(poses, edges, method, option=lib.global_optimization_option(**option))
    assert len(want_E) == len(edges) - 1 and np.array_equal(want_E[-1].transformation, true_edge.transformation)
    for b in driver_bins:
        p = subprocess.run([b, "graph", inp, outp], capture_output=True, text=True, timeout=120)
        assert p.returncode == 0, (b, p.returncode, p.stdout, p.stderr)
        v = np.frombuffer(open(outp, "rb").read(), "<f8")
        ne = int(v[0]); ed = v[1 + 16 * len(poses):1 + 16 * len(poses) + EDGE_REC * ne].reshape(ne, EDGE_REC)
        assert ne == len(edges) - 1 and ed[-1, :3].tolist() == [1.0, 4.0, 1.0]
        assert np.array_equal(ed[-1, 4:20].reshape(4, 4), true_edge.transformation)
        assert ed[-1, 20] == true_edge.information[0, 0] and ed[-1, 3] == want_E[-1].confidence
