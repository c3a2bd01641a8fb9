"""The information matrix of a pose-graph edge on the GPU (visma_icp_information_matrix, visma_icp_reduce_information,
visma_icp_information_matrices; information.hip) and multiway registration end to end.

The yardstick is the numpy specification posegraph_spec.information_terms: sum G^T G over the target points of a pair list,
G = [-hat(q) | I].  tests/golden/posegraph.npz (tests/golden/gen_posegraph.py) pins it to the compiled reference on every
third point of fragments.npz: the reference's matrix with 1 and with 3 OpenMP threads is the specification on the
reference's own correspondence set PLUS 2 I and PLUS 4 I (Open3D 0.3.0 starts the sum and every thread's private copy at
the identity; this library returns the pure sum, visma_icp.h).

The tolerance per entry is derived, not measured: both sides sum K terms in f64 in some order, so
|a - b| <= 2 (K + 4) 2^-53 S with S the sum of |term| of that entry (posegraph_spec.information_bound), computed here.

Non-finite points, as the search defines them (measured on the MI355X, stated in visma_icp.h): a non-finite source point
is left out of the pairs; a non-finite target coordinate makes the centroid both clouds are centred on non-finite, so
nothing has a pair (K = 0, the zero matrix); neither is an error.  test_non_finite_source_point_is_left_out and
test_non_finite_target_point_leaves_no_pair assert exactly that."""
import ctypes as C
import os
import struct
import subprocess
import sys

import numpy as np
import pytest

import posegraph_spec as S
from oracle_engine import OracleEngine
from visma_amd import synth

HERE = os.path.dirname(os.path.abspath(__file__))
G = os.path.join(HERE, "golden")
sys.path.insert(0, os.path.join(HERE, "cpp"))
import build_shim  # noqa: E402

INVALID, STATE = 1, 5
TOL_T = 1e-5        # a transform within 1e-5 relative Frobenius
GRID_CAP = 1024 * 256   # the reduction's grid: at most 1024 workgroups of 256 threads (trim_reduce_blocks)


@pytest.fixture(scope="module")
def golden():
    g = np.load(os.path.join(G, "posegraph.npz"))
    return {k: g[k] for k in g.files}


@pytest.fixture(scope="module")
def frag3():
    f = np.load(os.path.join(G, "fragments.npz"))
    return {k: np.ascontiguousarray(f[k].astype(np.float64)[::3]) for k in ("src", "tgt")}


def rigid(w, t):
    w = np.asarray(w, np.float64); th = np.linalg.norm(w)
    T = np.eye(4)
    if th > 0:
        k = w / th
        K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
        T[:3, :3] = np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * K @ K
    T[:3, 3] = t
    return T


# ---------------------------------------------------------------------------
# CPU
# ---------------------------------------------------------------------------
NEW_SYMBOLS = ["visma_icp_information_matrix", "visma_icp_reduce_information", "visma_icp_information_matrices",
               "visma_icp_get_cloud_sizes"]
NEW_METHODS = ["information_matrix", "reduce_information", "information_matrices"]


def test_symbols_and_methods(lib):
    L = lib.load()
    for name in NEW_SYMBOLS:
        assert hasattr(L, name), name
    for name in NEW_METHODS:
        assert callable(getattr(lib.Context, name, None)), name


@pytest.mark.parametrize("pose", [0, 1, 2])
def test_specification_equals_the_reference_minus_its_identity_terms(golden, frag3, pose):
    """on the reference's own correspondence set: reference(1 thread) - 2 I and reference(3 threads) - 4 I"""
    pairs = golden["info_pairs_%d" % pose]
    K = len(pairs)
    M, Sabs = S.information_terms(frag3["tgt"][pairs[:, 1]])
    bound = S.information_bound(K, Sabs)
    d1 = np.abs(M - (golden["info_ref_1"][pose] - 2.0 * np.eye(6)))
    d3 = np.abs(M - (golden["info_ref_3"][pose] - 4.0 * np.eye(6)))
    print("pose %d: K = %d, largest |difference| %.3e (1 thread) %.3e (3 threads), as a share of its bound %.3g"
          % (pose, K, d1.max(), d3.max(), max((d1 / np.where(bound > 0, bound, 1)).max(), (d3 / np.where(bound > 0, bound, 1)).max())))
    assert np.all(d1 <= bound) and np.all(d3 <= bound)
    assert golden["info_ref_1"][pose][5, 5] == K + 2 and golden["info_ref_3"][pose][5, 5] == K + 4       # the quirk, pinned
    assert M[5, 5] == K
    if pose == 2:
        assert K == 0 and np.all(M == 0.0)
    else:
        assert K > 1000


@pytest.fixture()
def hctx(lib, oracle):
    eng = OracleEngine(oracle)
    ctx = eng.context()
    ctx.engine = eng
    yield ctx
    ctx.close()


def test_argument_checks(lib, hctx):
    """every argument error comes before anything reaches a device (a context on the oracle engine has none)"""
    L, h = hctx.L, hctx._h
    dp = C.POINTER(C.c_double)
    T = np.eye(4).ravel().copy(); out = np.full(36, 7.0); k = C.c_int64(-1)
    pT, po = T.ctypes.data_as(dp), out.ctypes.data_as(dp)
    assert L.visma_icp_information_matrix(None, pT, 0.1, po, C.byref(k)) == INVALID
    assert L.visma_icp_reduce_information(None, po) == INVALID
    assert L.visma_icp_information_matrices(None, None, 0, None, None) == INVALID
    # clouds not set
    assert L.visma_icp_information_matrix(h, pT, 0.1, po, C.byref(k)) == STATE
    assert L.visma_icp_reduce_information(h, po) == STATE
    xyz = np.random.default_rng(1).random((40, 3))
    hctx.set_clouds_f64(xyz, xyz)
    assert L.visma_icp_information_matrix(h, None, 0.1, po, C.byref(k)) == INVALID
    assert L.visma_icp_information_matrix(h, pT, 0.1, None, C.byref(k)) == INVALID
    assert L.visma_icp_information_matrix(h, pT, 0.0, po, C.byref(k)) == INVALID
    assert L.visma_icp_information_matrix(h, pT, float("nan"), po, C.byref(k)) == INVALID
    assert L.visma_icp_reduce_information(h, None) == INVALID
    # a non-finite T: the zero matrix and k = 0, no search
    for bad in (float("nan"), float("inf")):
        Tb = T.copy(); Tb[7] = bad; out[:] = 7.0; k.value = -1
        assert L.visma_icp_information_matrix(h, Tb.ctypes.data_as(dp), 0.1, po, C.byref(k)) == 0
        assert np.all(out == 0.0) and k.value == 0
    # the batch: counts, pointers, a problem's own arguments
    arr, n, keep, _ = lib.Context.make_batch([(xyz, xyz, None, 0.1)])
    outs = np.zeros(36); ks = np.zeros(1, np.int64)
    pk = ks.ctypes.data_as(C.POINTER(C.c_int64))
    assert L.visma_icp_information_matrices(h, arr, -1, outs.ctypes.data_as(dp), pk) == INVALID
    assert L.visma_icp_information_matrices(h, None, 1, outs.ctypes.data_as(dp), pk) == INVALID
    assert L.visma_icp_information_matrices(h, arr, 1, None, pk) == INVALID
    assert L.visma_icp_information_matrices(h, arr, 0, None, None) == 0
    for field, value in (("max_dist", 0.0), ("ns", -1), ("nt", -1)):
        old = getattr(arr[0], field); setattr(arr[0], field, value)
        assert L.visma_icp_information_matrices(h, arr, 1, outs.ctypes.data_as(dp), pk) == INVALID
        setattr(arr[0], field, old)


# ---------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ctx(lib):
    c = lib.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def surface():
    """a target of 4,000 surface points, shared and left unchanged"""
    t = synth.surface_points(4000, 11).astype(np.float32).astype(np.float64)
    t.setflags(write=False)
    return t


def check_against_specification(ctx, tgt_as_held, T, radius, what=""):
    """information_matrix at T against the specification on the correspondences the SAME context returns, per entry within
    the derived bound; (5, 5) is K exactly"""
    M, k = ctx.information_matrix(T, radius)
    si, ti, _ = ctx.get_correspondences()
    assert k == len(si), (k, len(si))
    want, Sabs = S.information_terms(tgt_as_held[ti])
    bound = S.information_bound(k, Sabs)
    d = np.abs(M - want)
    print("%s K = %d, largest |difference| %.3e, as a share of its bound %.3g" % (what, k, d.max(), (d / np.where(bound > 0, bound, 1)).max()))
    assert np.all(d <= bound), (d.max(), bound[np.unravel_index(np.argmax(d - bound), d.shape)])
    assert M[5, 5] == k and M[3, 3] == k and M[4, 4] == k
    assert np.array_equal(M, M.T)
    return M, k, si, ti


@pytest.mark.gpu
@pytest.mark.parametrize("pose", [0, 1, 2])
def test_information_matrix_equals_the_reference_on_the_fragments(ctx, golden, frag3, pose):
    ctx.set_clouds_f64(frag3["src"], frag3["tgt"])
    T, r = golden["info_T"][pose], float(golden["info_max_dist"])
    M, k, si, ti = check_against_specification(ctx, frag3["tgt"], T, r, "fragments pose %d:" % pose)
    pairs = golden["info_pairs_%d" % pose]
    pairs = pairs[np.argsort(pairs[:, 0], kind="stable")]                                  # (the reference lists them per OpenMP thread)
    assert k == len(pairs) and np.array_equal(np.stack([si, ti], 1), pairs)                 # the reference's correspondence set
    _, Sabs = S.information_terms(frag3["tgt"][pairs[:, 1]])
    bound = S.information_bound(k, Sabs)
    assert np.all(np.abs(M - (golden["info_ref_1"][pose] - 2.0 * np.eye(6))) <= bound)
    assert np.all(np.abs(M - (golden["info_ref_3"][pose] - 4.0 * np.eye(6))) <= bound)
    if pose == 2:
        assert k == 0 and np.all(M == 0.0)


@pytest.mark.gpu
@pytest.mark.parametrize("ns", [1, 63, 64, 65, 255, 256, 257, GRID_CAP + 1])
def test_source_sizes(ctx, surface, ns):
    """one lane, a wave more or less one, a workgroup more or less one, one point past the grid's cap (a second trip of
    the grid-stride loop)"""
    rng = np.random.default_rng(ns)
    src = surface[rng.integers(0, len(surface), ns)] + rng.normal(size=(ns, 3)) * 2e-3
    ctx.set_clouds_f64(src, surface)
    M, k, _, _ = check_against_specification(ctx, surface, rigid([0, 0, 0.001], [1e-3, 0, -1e-3]), 0.05, "ns = %d:" % ns)
    assert k == ns


@pytest.mark.gpu
def test_no_pair_and_exactly_one_pair(ctx, surface):
    rng = np.random.default_rng(5)
    src = surface[rng.integers(0, len(surface), 300)].copy()
    ctx.set_clouds_f64(src, surface)
    M, k = ctx.information_matrix(rigid([0, 0, 0], [50.0, 0, 0]), 0.05)
    assert k == 0 and np.all(M == 0.0)
    src = np.stack([surface[7] + [1e-4, 0, 0], surface[7] + [9.0, 0, 0], surface[9] + [0, 11.0, 0]])
    ctx.set_clouds_f64(src, surface)
    M, k, si, ti = check_against_specification(ctx, surface, np.eye(4), 0.01, "one pair:")
    assert k == 1 and si.tolist() == [0] and ti.tolist() == [7]


@pytest.mark.gpu
def test_clouds_metres_from_the_origin(ctx):
    """chair_offset3m: the device holds the clouds centred, the sums are formed from q + centre -- the caller's frame"""
    g = np.load(os.path.join(G, "chair_offset3m.npz"))
    src, tgt = g["src"].astype(np.float64), g["tgt"].astype(np.float64)
    assert np.abs(tgt.mean(0)).max() > 1.0
    ctx.set_clouds_f64(src, tgt)
    M, k, _, _ = check_against_specification(ctx, tgt, g["init"], float(g["radius"]), "chair_offset3m:")
    assert k > 1000


@pytest.mark.gpu
def test_fp32_uploads(lib, surface):
    """set_target / set_source: no f64 copy on the device, the kernel's fp32 branch"""
    c = lib.Context(0)
    try:
        rng = np.random.default_rng(3)
        src = (surface[rng.integers(0, len(surface), 700)] + rng.normal(size=(700, 3)) * 2e-3).astype(np.float32)
        c.set_target(surface.astype(np.float32)); c.set_source(src)
        check_against_specification(c, surface.astype(np.float32).astype(np.float64), np.eye(4), 0.05, "fp32 uploads:")
    finally:
        c.close()


@pytest.mark.gpu
def test_reduce_after_nn_pass_and_bit_identical_repeats(ctx, frag3, golden):
    ctx.set_clouds_f64(frag3["src"], frag3["tgt"])
    T, r = golden["info_T"][0], float(golden["info_max_dist"])
    A, ka = ctx.information_matrix(T, r)
    B, kb = ctx.information_matrix(T, r)
    assert ka == kb and A.tobytes() == B.tobytes()
    ctx.nn_pass(T, r)
    Cm = ctx.reduce_information()
    assert Cm.tobytes() == A.tobytes()
    assert ctx.reduce_information().tobytes() == A.tobytes()


@pytest.mark.gpu
def test_batch_equals_the_single_calls_bit_for_bit(ctx, surface):
    """6 edges on 3 clouds: shared targets, one edge without a pair, one non-finite T; every matrix bit-equal to the single
    call, whatever the order of the batch"""
    rng = np.random.default_rng(8)
    A = surface
    B = (surface[rng.integers(0, len(surface), 2500)] + rng.normal(size=(2500, 3)) * 2e-3)
    Cc = (surface[rng.integers(0, len(surface), 1800)] + rng.normal(size=(1800, 3)) * 2e-3)
    bad = np.eye(4); bad[1, 3] = np.nan
    r = 0.05
    edges = [(A, B, rigid([0, 0, 0.002], [1e-3, 0, 0]), r), (Cc, B, np.eye(4), r), (A, Cc, rigid([0.001, 0, 0], [0, 1e-3, 0]), r),
             (B, Cc, rigid([0, 0, 0], [40.0, 0, 0]), r), (A, B, bad, r), (B, A, np.eye(4), 0.03)]
    Ms, ks = ctx.information_matrices(edges)
    assert ks[3] == 0 and np.all(Ms[3] == 0.0) and ks[4] == 0 and np.all(Ms[4] == 0.0)
    assert all(ks[i] > 500 for i in (0, 1, 2, 5))
    # afterwards the context holds the last edge handled (groups by target in the caller's order: B, Cc, A -> edge 5)
    assert (ctx.ns, ctx.nt) == (len(B), len(A))
    assert len(ctx.get_correspondences()[0]) == ks[5]
    perm = [5, 3, 1, 4, 0, 2]
    Mp, kp = ctx.information_matrices([edges[i] for i in perm])
    for j, i in enumerate(perm):
        assert Mp[j].tobytes() == Ms[i].tobytes() and kp[j] == ks[i], i
    for i, (s, t, T, rr) in enumerate(edges):
        if i == 4:
            continue
        ctx.set_clouds_f64(s, t)
        M1, k1 = ctx.information_matrix(T, rr)
        assert M1.tobytes() == Ms[i].tobytes() and k1 == ks[i], i
        want, Sabs = S.information_terms(np.asarray(t)[ctx.get_correspondences()[1]])
        assert np.all(np.abs(M1 - want) <= S.information_bound(k1, Sabs))


@pytest.mark.gpu
@pytest.mark.parametrize("value", [np.nan, np.inf])
def test_non_finite_source_point_is_left_out(lib, surface, value):
    """what visma_icp.h states: no error; the point is in no pair; the matrix is that of the other pairs"""
    rng = np.random.default_rng(4)
    s = surface[rng.integers(0, len(surface), 500)] + rng.normal(size=(500, 3)) * 2e-3
    s[17, 1] = value
    c = lib.Context(0)
    try:
        c.set_clouds_f64(s, surface)
        M, k = c.information_matrix(np.eye(4), 0.05)
        si, ti, _ = c.get_correspondences()
        assert k == len(si) == 499 and 17 not in si.tolist()
        want, Sabs = S.information_terms(surface[ti])
        assert np.all(np.isfinite(M)) and np.all(np.abs(M - want) <= S.information_bound(k, Sabs))
    finally:
        c.close()


@pytest.mark.gpu
@pytest.mark.parametrize("value", [np.nan, np.inf])
def test_non_finite_target_point_leaves_no_pair(lib, surface, value):
    """what visma_icp.h states: no error; the centroid both clouds are centred on is not finite, so nothing has a pair:
    K = 0 and the zero matrix"""
    rng = np.random.default_rng(4)
    s = surface[rng.integers(0, len(surface), 500)] + rng.normal(size=(500, 3)) * 2e-3
    t = np.array(surface)
    t[17, 1] = value
    c = lib.Context(0)
    try:
        c.set_clouds_f64(s, t)
        M, k = c.information_matrix(np.eye(4), 0.05)
        assert k == 0 and np.all(M == 0.0)
        assert len(c.get_correspondences()[0]) == 0
    finally:
        c.close()


def cut_into_pieces(n_pieces=4, n_points=3000, seed=21):
    """one synthetic cloud cut into overlapping slabs along x (each 70 % of the extent, starting 10 % after the one
    before: every two pieces share at least 40 % of the extent), each piece moved into a frame of its own: piece i holds
    (world points of slab i) moved by inverse(pose_i)"""
    world = synth.surface_points(n_points, seed)
    x = world[:, 0]
    lo, extent = x.min(), x.max() - x.min()
    rng = np.random.default_rng(seed)
    poses, pieces = [], []
    for i in range(n_pieces):
        a = lo + 0.1 * i * extent
        sel = world[(x >= a) & (x <= a + 0.7 * extent)]
        pose = np.eye(4) if i == 0 else rigid(rng.normal(size=3) * 0.15, rng.normal(size=3) * 0.3)
        inv = np.linalg.inv(pose)
        pieces.append(np.ascontiguousarray(sel @ inv[:3, :3].T + inv[:3, 3]))
        poses.append(pose)
    return pieces, poses


@pytest.mark.gpu
def test_multiway_registration_end_to_end(lib, ctx):
    """4 overlapping pieces of one cloud with known poses: pairwise ICP from perturbed starts, the information matrices in
    one batched call, one false uncertain loop closure, global optimisation -- the false edge is pruned, the true ones kept,
    the largest pose error shrinks, and the poses equal the numpy specification run on the same edges"""
    pieces, truth = cut_into_pieces()
    assert all(1200 < len(p) < 4000 for p in pieces), [len(p) for p in pieces]
    n = len(pieces)
    r = 0.06
    rng = np.random.default_rng(2)
    rel = lambda i, j: np.linalg.inv(truth[j]) @ truth[i]
    pairs = [(0, 1, False), (1, 2, False), (2, 3, False), (0, 2, True), (1, 3, True)]
    edges, problems = [], []
    for i, j, uncertain in pairs:
        start = rigid(rng.normal(size=3) * 0.01, rng.normal(size=3) * 0.01) @ rel(i, j)
        ctx.set_clouds_f64(pieces[i], pieces[j])
        res = ctx.run(start, r, 40, 1e-9, 1e-9)
        assert synth.rel_frobenius(np.asarray(res.transformation_).reshape(4, 4), rel(i, j)) < 2e-2
        edges.append([i, j, np.array(res.transformation_).reshape(4, 4), uncertain])
        problems.append((pieces[i], pieces[j], edges[-1][2], r))
    false_T = rigid([0.0, 0.3, 0.0], [0.25, -0.2, 0.1]) @ rel(0, 3)
    edges.append([0, 3, false_T, True])
    problems.append((pieces[0], pieces[3], false_T, r))
    Ms, ks = ctx.information_matrices(problems)
    assert all(k > 100 for k in ks[:5]), ks
    graph = [lib.PoseGraphEdge(i, j, T, Ms[e] if ks[e] > 0 else np.eye(6), u) for e, (i, j, T, u) in enumerate(edges)]
    start_poses = [np.eye(4)]
    for i in range(1, n):                                   # odometry: chain the pairwise results
        start_poses.append(start_poses[-1] @ np.linalg.inv(edges[i - 1][2]))
    start_poses = [rigid(rng.normal(size=3) * 0.01, rng.normal(size=3) * 0.01) @ T if i else T for i, T in enumerate(start_poses)]
    option = dict(max_correspondence_distance=r, edge_prune_threshold=0.25, preference_loop_closure=1.0, reference_node=0)
    P, out = lib.global_optimization(start_poses, graph, "lm", option=lib.global_optimization_option(**option))
    kept = [(e.source, e.target) for e in out]
    assert (0, 3) not in kept and kept == [(i, j) for i, j, _ in pairs], kept
    err = lambda poses: max(synth.rel_frobenius(np.linalg.inv(poses[0]) @ poses[i], np.linalg.inv(truth[0]) @ truth[i]) for i in range(1, n))
    before, after = err(start_poses), err(P)
    print("largest pose error before %.3e, after %.3e; K per edge %s" % (before, after, ks.tolist()))
    assert after < before
    Ps, outs, _ = S.global_optimization(start_poses, [S.Edge(e.source, e.target, e.transformation, e.information, e.uncertain) for e in graph],
                                        "lm", None, option)
    assert [(e.source, e.target) for e in outs] == kept
    d = max(synth.rel_frobenius(a, b) for a, b in zip(P, Ps))
    print("library against the specification on the same edges: %.3e" % d)
    assert d <= TOL_T


@pytest.fixture(scope="module")
def driver_bins(lib):
    import build_posegraph
    if build_shim.eigen_dir() is not None:
        build_posegraph.build()
    paths = [os.path.join(HERE, "cpp", "_build", b) for b in build_posegraph.BINS]
    if not all(os.path.exists(p) for p in paths):
        pytest.skip("posegraph driver not prebuilt and no Eigen headers here")
    return paths


@pytest.mark.gpu
def test_shim_driver_fills_every_edge(lib, ctx, surface, driver_bins, tmp_path):
    """cicp::GetInformationMatrixFromPointClouds, the single call and the PoseGraph overload, both Eigen storage orders:
    equal to each other bit for bit and to the Python call"""
    rng = np.random.default_rng(12)
    clouds = [np.array(surface), surface[rng.integers(0, len(surface), 1500)] + rng.normal(size=(1500, 3)) * 2e-3,
              surface[rng.integers(0, len(surface), 900)] + rng.normal(size=(900, 3)) * 2e-3]
    edges = [(1, 0, rigid([0, 0, 0.002], [1e-3, 0, 0])), (2, 0, np.eye(4)), (2, 1, rigid([0, 0.001, 0], [0, 0, 1e-3]))]
    r = 0.05
    inp, outp = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(inp, "wb") as f:
        f.write(struct.pack("<q", len(clouds)))
        for c in clouds:
            f.write(struct.pack("<q", len(c))); f.write(np.ascontiguousarray(c, "<f8").tobytes())
        f.write(struct.pack("<dq", r, len(edges)))
        for s, t, T in edges:
            f.write(struct.pack("<ii", s, t)); f.write(np.ascontiguousarray(T, "<f8").tobytes())
    cp = lib.Context(0)
    cp.set_search_precision("exact")                     # (the shim's thread context asks for the exact search)
    try:
        want = []
        for s, t, T in edges:
            cp.set_clouds_f64(clouds[s], clouds[t])
            want.append(cp.information_matrix(T, r)[0])
    finally:
        cp.close()
    for b in driver_bins:
        p = subprocess.run([b, "info", inp, outp], capture_output=True, text=True, timeout=120)
        assert p.returncode == 0, (b, p.returncode, p.stdout, p.stderr)
        v = np.frombuffer(open(outp, "rb").read(), "<f8").reshape(2, len(edges), 6, 6)
        assert v[0].tobytes() == v[1].tobytes()
        assert v[0].tobytes() == np.stack(want).tobytes()
