"""Generalized ICP (visma_amd/csrc/gicp.hip; Segal, Haehnel, Thrun, RSS 2009): every pair of a pass weighted by
M = (C_t + R C_s R^T)^-1 with C = I - (1 - epsilon) n n^T (visma_icp.h states the step).

CPU: the symbols and methods exist, the argument checks, the C++ driver against the stand-alone headers, and the numpy
specification (np.linalg.inv for M, einsum sums) with the two identities that tie it to point-to-point and
point-to-plane.  No compiled reference has this estimator: the specification below is the yardstick of every GPU check.
GPU: every oracle is assembled here from pieces that are not under test -- the committed kernel specification
(Oracle.k_nn_pass for the pairs), numpy for the sums, the oracle's Gauss-Newton solve from statistics (k_solve_gn) for
the loop.
"""
import math
import os
import struct
import subprocess
import sys

import numpy as np
import pytest

from oracle_engine import OracleEngine
from visma_amd import _lib, synth

HERE = os.path.dirname(os.path.abspath(__file__))
G = os.path.join(HERE, "golden")
sys.path.insert(0, os.path.join(HERE, "cpp"))
import build_shim  # noqa: E402
import build_gicp  # noqa: E402

TOL_T = 1e-5       # north_star: final SE(3) within 1e-5 relative Frobenius of the CPU reference (test_gpu_kernels.py)
TOL_STATS = 1e-9   # the project's bar for the trimmed and robust statistics, relative to max(|spec|, 1)
INVALID, STATE = 1, 5
EPSILONS = [1.0, 1e-3]


# ---------------------------------------------------------------------------
# the yardstick: the generalized step in numpy
# ---------------------------------------------------------------------------
def hat(p):
    """[p]x per row: (K, 3) -> (K, 3, 3)"""
    H = np.zeros((len(p), 3, 3))
    H[:, 0, 1] = -p[:, 2]; H[:, 0, 2] = p[:, 1]
    H[:, 1, 0] = p[:, 2]; H[:, 1, 2] = -p[:, 0]
    H[:, 2, 0] = -p[:, 1]; H[:, 2, 1] = p[:, 0]
    return H


def transform(src, T):
    """p = T s in f64, row by row in the kernel's order"""
    s = np.asarray(src, np.float64)[:, :3]
    p = np.empty_like(s)
    for k in range(3):
        p[:, k] = ((T[k, 0] * s[:, 0] + T[k, 1] * s[:, 1]) + T[k, 2] * s[:, 2]) + T[k, 3]
    return p


def gicp_terms(p, q, m, n, eps):
    """per pair: d, M = (2 I - (1 - eps)(n n^T + m m^T))^-1 by np.linalg.inv, J = [-[p]x | I]"""
    d = p - q
    Cm = 2.0 * np.eye(3)[None] - (1.0 - eps) * (n[:, :, None] * n[:, None, :] + m[:, :, None] * m[:, None, :])
    M = np.linalg.inv(Cm) if len(p) else np.zeros((0, 3, 3))
    J = np.concatenate([-hat(p), np.broadcast_to(np.eye(3), (len(p), 3, 3))], 2)
    return d, M, J


def gicp_stats(p, q, m, n, eps):
    """(the 38 statistics of visma_icp.h, cost) over the pairs given"""
    d, M, J = gicp_terms(p, q, m, n, eps)
    st = np.zeros(38)
    st[0] = len(p)
    st[1] = (d * d).sum()
    st[2:23] = np.einsum("kia,kij,kjb->ab", J, M, J)[np.triu_indices(6)]
    st[23:29] = np.einsum("kia,kij,kj->a", J, M, d)
    return st, float(np.einsum("ki,kij,kj->", d, M, d))


def spec_pass(src, tgt, T, idx, ns_nrm, nt_nrm, eps):
    """the specification over the pairs idx (< 0: none) of a pass at T"""
    v = idx >= 0
    p = transform(src, T)[v]
    q = np.asarray(tgt, np.float64)[idx[v], :3]
    m = np.asarray(ns_nrm, np.float64)[v] @ T[:3, :3].T
    n = np.asarray(nt_nrm, np.float64)[idx[v]]
    return gicp_stats(p, q, m, n, eps)


def _unit_normals(rng, n):
    """random unit normals that fp32 holds exactly (the fp32 passes read the fp32 copy)"""
    v = rng.standard_normal((n, 3))
    v /= np.linalg.norm(v, axis=1, keepdims=True)
    return v.astype(np.float32).astype(np.float64)


def _rand_T(rng, ang=0.2, tr=0.1):
    w = rng.standard_normal(3)
    w *= ang / np.linalg.norm(w)
    th = np.linalg.norm(w)
    K = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])
    R = np.eye(3) + np.sin(th) / th * K + (1 - np.cos(th)) / th ** 2 * K @ K
    return synth.make_T(R, rng.standard_normal(3) * tr)


def _identity_case(seed, k=4000):
    rng = np.random.default_rng(seed)
    p = rng.standard_normal((k, 3)) + np.array([0.3, -0.2, 1.0])
    q = p + rng.standard_normal((k, 3)) * 0.02
    n = rng.standard_normal((k, 3))
    n /= np.linalg.norm(n, axis=1, keepdims=True)
    m = rng.standard_normal((k, 3))
    m /= np.linalg.norm(m, axis=1, keepdims=True)
    return p, q, m, n


def test_epsilon_one_is_half_the_point_to_point_gauss_newton_step():
    """eps = 1: C = 2 I whatever the normals, so cost = sum |d|^2 / 2 and A, b are half the rows of J = [-[p]x | I]"""
    p, q, m, n = _identity_case(1)
    st, cost = gicp_stats(p, q, m, n, 1.0)
    d, _, J = gicp_terms(p, q, m, n, 1.0)
    A = np.einsum("kia,kib->ab", J, J)[np.triu_indices(6)]
    b = np.einsum("kia,ki->a", J, d)
    scale = np.abs(A).max()
    assert abs(cost - 0.5 * (d * d).sum()) <= 1e-14 * cost
    assert np.abs(st[2:23] - 0.5 * A).max() <= 1e-13 * scale and np.abs(st[23:29] - 0.5 * b).max() <= 1e-13 * np.abs(b).max()
    assert st[0] == len(p) and st[1] == (d * d).sum() and not st[29:].any()


@pytest.mark.parametrize("eps", [1e-3, 0.05, 0.5])
def test_equal_normals_add_the_point_to_plane_term(eps):
    """m = n (unit): M = (I + (1 / eps - 1) n n^T) / 2, so cost = sum |d|^2 / 2 + (1 / (2 eps) - 1 / 2) sum (d . n)^2"""
    p, q, _, n = _identity_case(2)
    _, cost = gicp_stats(p, q, n, n, eps)
    d = p - q
    want = 0.5 * (d * d).sum() + (0.5 / eps - 0.5) * ((d * n).sum(1) ** 2).sum()
    assert abs(cost - want) <= 1e-12 * want, (cost, want)


def test_zero_source_normals_leave_the_source_isotropic():
    """m = 0: C = I + (I - (1 - eps) n n^T); along n the weight is 1 / (1 + eps), across it 1 / 2"""
    p, q, _, n = _identity_case(3)
    eps = 1e-3
    _, cost = gicp_stats(p, q, np.zeros_like(n), n, eps)
    d = p - q
    dn = (d * n).sum(1)
    want = 0.5 * ((d * d).sum() - (dn ** 2).sum()) + (dn ** 2).sum() / (1.0 + eps)
    assert abs(cost - want) <= 1e-12 * want


# ---------------------------------------------------------------------------
# CPU: interface
# ---------------------------------------------------------------------------
NEW_SYMBOLS = ["visma_icp_set_source_normals_f64", "visma_icp_reduce_gicp", "visma_icp_run_gicp", "visma_icp_run_yaw_sweep_gicp"]


def test_symbols_and_methods(lib):
    L = lib.load()
    for name in NEW_SYMBOLS:
        assert hasattr(L, name), name
    for name in ["set_source_normals_f64", "reduce_gicp", "run_gicp", "run_yaw_sweep_gicp"]:
        assert callable(getattr(lib.Context, name, None)), name
    assert hasattr(lib, "GicpInfo")


@pytest.fixture()
def hctx(lib, oracle):
    """A context on the oracle engine: the argument checks run, no call reaches a device."""
    eng = OracleEngine(oracle)
    ctx = eng.context()
    ctx.engine = eng
    yield ctx
    ctx.close()


def _small_clouds():
    rng = np.random.default_rng(3)
    tgt = rng.random((300, 3)).astype(np.float32)
    src = (tgt[:200] + 0.01).astype(np.float32)
    return src, tgt, _unit_normals(rng, 200), _unit_normals(rng, 300)


BAD_EPSILONS = [0.0, -1.0, 1.5, float("nan"), float("inf"), float("-inf")]


@pytest.mark.parametrize("eps", BAD_EPSILONS, ids=lambda e: "eps=%s" % e)
def test_bad_epsilon_is_invalid_before_any_pass(lib, hctx, eps):
    src, tgt, sn, tn = _small_clouds()
    hctx.set_target(tgt); hctx.set_source(src)
    hctx.set_target_normals_f64(tn); hctx.set_source_normals_f64(sn)
    hctx.nn_pass(np.eye(4), 0.1)
    calls = dict(hctx.engine.calls)
    for call in (lambda: hctx.run_gicp(None, 0.1, eps, max_iter=5), lambda: hctx.reduce_gicp(eps),
                 lambda: hctx.run_yaw_sweep_gicp(4, 0.1, eps, max_iter=5)):
        with pytest.raises(lib.IcpError) as e:
            call()
        assert e.value.code == INVALID
    assert hctx.engine.calls == calls                    # nothing was launched


def test_null_outputs_missing_clouds_and_missing_normals(lib, hctx):
    import ctypes as C
    L, h = hctx.L, hctx._h
    init = np.eye(4).reshape(16).copy()
    init[3] = 0.25
    dp = C.POINTER(C.c_double)
    res, info, st = lib.CResult(), lib.CGicpInfo(), np.zeros(38)
    ip, sp = init.ctypes.data_as(dp), st.ctypes.data_as(dp)
    src, tgt, sn, tn = _small_clouds()
    # a context without clouds
    assert L.visma_icp_run_gicp(h, ip, 0.1, 1e-3, 5, 0.0, 0.0, C.byref(res), C.byref(info)) == STATE
    assert L.visma_icp_reduce_gicp(h, 1e-3, sp, C.byref(info)) == STATE
    assert L.visma_icp_set_source_normals_f64(h, sn.ctypes.data_as(dp), len(sn), 3) == STATE
    hctx.set_target(tgt); hctx.set_source(src)
    # NULL result / init / statistics / info / normals; a wrong count or stride
    assert L.visma_icp_run_gicp(h, ip, 0.1, 1e-3, 5, 0.0, 0.0, None, C.byref(info)) == INVALID
    assert L.visma_icp_run_gicp(h, None, 0.1, 1e-3, 5, 0.0, 0.0, C.byref(res), C.byref(info)) == INVALID
    assert L.visma_icp_run_gicp(h, ip, 0.1, 1e-3, -1, 0.0, 0.0, C.byref(res), C.byref(info)) == INVALID
    assert L.visma_icp_run_gicp(None, ip, 0.1, 1e-3, 5, 0.0, 0.0, C.byref(res), C.byref(info)) == INVALID
    assert L.visma_icp_reduce_gicp(h, 1e-3, None, C.byref(info)) == INVALID
    assert L.visma_icp_reduce_gicp(h, 1e-3, sp, None) == INVALID
    assert L.visma_icp_run_yaw_sweep_gicp(h, 4, 0.1, 1e-3, 5, 0.0, 0.0, None, None, None, None, None) == INVALID
    assert L.visma_icp_run_yaw_sweep_gicp(h, 0, 0.1, 1e-3, 5, 0.0, 0.0, C.byref(res), None, None, None, None) == INVALID
    assert L.visma_icp_set_source_normals_f64(h, None, len(sn), 3) == INVALID
    assert L.visma_icp_set_source_normals_f64(h, sn.ctypes.data_as(dp), len(sn) - 1, 3) == INVALID
    assert L.visma_icp_set_source_normals_f64(h, sn.ctypes.data_as(dp), len(sn), 2) == INVALID
    # no normals, target normals only, source normals only: the run returns init (Registration.cpp:152-157), the pass is refused
    hctx.nn_pass(np.eye(4), 0.1)
    for setup in (lambda: None, lambda: hctx.set_target_normals_f64(tn),
                  lambda: (hctx.set_target(tgt), hctx.set_source_normals_f64(sn), hctx.nn_pass(np.eye(4), 0.1))):
        setup()
        calls = dict(hctx.engine.calls)
        assert L.visma_icp_run_gicp(h, ip, 0.1, 1e-3, 5, 0.0, 0.0, C.byref(res), None) == 0
        assert list(res.transformation) == list(init) and res.num_correspondences == 0 and res.iterations == 0
        assert hctx.engine.calls == calls
        assert L.visma_icp_reduce_gicp(h, 1e-3, sp, C.byref(info)) == STATE
    # a new source drops its normals, as a new target drops the target's
    hctx.set_target_normals_f64(tn)
    hctx.set_source(src)
    assert L.visma_icp_run_gicp(h, ip, 0.1, 1e-3, 5, 0.0, 0.0, C.byref(res), None) == 0
    assert list(res.transformation) == list(init)
    # a radius that is not positive returns init as every run does
    hctx.set_source_normals_f64(sn)
    assert L.visma_icp_run_gicp(h, ip, 0.0, 1e-3, 5, 0.0, 0.0, C.byref(res), C.byref(info)) == 0
    assert list(res.transformation) == list(init) and info.cost == 0.0 and info.mahalanobis_rmse == 0.0


def test_reduce_before_a_pass_is_state(lib, hctx):
    src, tgt, sn, tn = _small_clouds()
    hctx.set_target(tgt); hctx.set_source(src)
    hctx.set_target_normals_f64(tn); hctx.set_source_normals_f64(sn)
    with pytest.raises(lib.IcpError) as e:
        hctx.reduce_gicp(1e-3)
    assert e.value.code == STATE


def test_oracle_engine_reports_not_supported(lib, hctx):
    src, tgt, sn, tn = _small_clouds()
    hctx.set_target(tgt); hctx.set_source(src)
    hctx.set_target_normals_f64(tn); hctx.set_source_normals_f64(sn)
    hctx.nn_pass(np.eye(4), 0.1)
    with pytest.raises(lib.IcpError) as e:
        hctx.reduce_gicp(1e-3)
    assert e.value.code == STATE and "not supported" in str(e.value)
    with pytest.raises(lib.IcpError) as e:
        hctx.run_gicp(None, 0.1, 1e-3, max_iter=5)
    assert e.value.code == STATE and "not supported" in str(e.value)
    # the context still runs everything else
    a = hctx.run(None, 0.1, 5, 0.0, 0.0)
    assert a.num_correspondences > 0


def test_sharded_context_is_invalid(lib, hctx):
    src, tgt, sn, tn = _small_clouds()
    hctx.set_target(tgt); hctx.set_source(src)
    hctx.set_target_normals_f64(tn); hctx.set_source_normals_f64(sn)
    fn = lib.ALLREDUCE_FN(lambda user, buf, n: 0)
    hctx._keep.append(fn)
    assert hctx.L.visma_icp_set_allreduce(hctx._h, fn, None, 0, 2) == 0
    for call in (lambda: hctx.run_gicp(None, 0.1, 1e-3, max_iter=5), lambda: hctx.reduce_gicp(1e-3),
                 lambda: hctx.run_yaw_sweep_gicp(4, 0.1, 1e-3, max_iter=5)):
        with pytest.raises(lib.IcpError) as e:
            call()
        assert e.value.code == INVALID


@pytest.fixture(scope="module")
def driver_bins(lib):
    if build_shim.eigen_dir() is not None:
        build_gicp.build()
    paths = [os.path.join(HERE, "cpp", "_build", b) for b in build_gicp.BINS]
    if not all(os.path.exists(p) for p in paths):
        pytest.skip("generalized driver not prebuilt and no Eigen headers here")
    return paths


def test_cpp_driver_compiles_against_standalone_headers(driver_bins):
    """Both Eigen storage orders: the estimator goes through the stock open3d::RegistrationICP without Open3D."""
    for b in driver_bins:
        assert os.path.getsize(b) > 0 and os.access(b, os.X_OK)
    src = open(os.path.join(HERE, "cpp", "gicp_driver.cpp")).read()
    assert "cicp::TransformationEstimationGeneralized" in src and "open3d::RegistrationICP" in src


# ---------------------------------------------------------------------------
# the loop's oracle: k_nn_pass + the specification + k_solve_gn (axis: the 6 x 6 restricted to the axis, in numpy)
# ---------------------------------------------------------------------------
def _rot(a, th):
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + math.sin(th) * K + (1.0 - math.cos(th)) * K @ K


def _full(st):
    A = np.zeros((6, 6))
    A[np.triu_indices(6)] = st[2:23]
    return A + np.triu(A, 1).T, st[23:29]


def axis_step(st, axis):
    """the generalized normal equations restricted to x = [theta a; t] (as test_axis_solve restates point-to-plane)"""
    A, b = _full(st)
    P = np.zeros((6, 4))
    P[:3, 0] = axis
    P[3:, 1:] = np.eye(3)
    y = np.linalg.solve(P.T @ A @ P, -(P.T @ b))
    T = np.eye(4)
    T[:3, :3] = _rot(axis, y[0])
    T[:3, 3] = y[1:]
    return T


def oracle_loop(oracle, src32, tgt32, sn, tn, r, eps, iters, init=None, axis=None, nudge=None):
    """RegistrationICP's loop (Registration.cpp:167-185, no stop test) over the kernel specification's pairs.
    nudge: a matrix added to T before every search (the K-stability check)."""
    T = np.eye(4) if init is None else np.array(init, np.float64)
    r2 = np.float32(r * r)
    ks = []
    for it in range(iters + 1):
        Ts = T if nudge is None else T + nudge
        k, idx, _ = oracle.k_nn_pass(src32, tgt32, Ts[:3, :].astype(np.float32), r2, grid=True)
        ks.append(k)
        if it == iters:
            break
        st, _ = spec_pass(src32, tgt32, T, idx, sn, tn, eps)
        upd = axis_step(st, axis) if axis is not None else oracle.k_solve_gn(st)[1]
        T = upd @ T
    return T, ks


LOOP_R, LOOP_EPS, LOOP_ITERS = 0.075, 1e-3, 10
Y = np.array([0.0, 1.0, 0.0])


_loop_cache = {}


def chair(oracle):
    if "chair" not in _loop_cache:
        g = np.load(os.path.join(G, "chair_5k_20k.npz"))
        src, tgt = g["src"].astype(np.float32), g["tgt"].astype(np.float32)
        sn = oracle.estimate_normals(src.astype(np.float64))
        tn = oracle.estimate_normals(tgt.astype(np.float64))
        _loop_cache["chair"] = (src, tgt, sn, tn)
    return _loop_cache["chair"]


def chair_loop(oracle, axis):
    key = None if axis is None else tuple(axis)
    if key not in _loop_cache:
        src, tgt, sn, tn = chair(oracle)
        _loop_cache[key] = (src, tgt, sn, tn) + oracle_loop(oracle, src, tgt, sn, tn, LOOP_R, LOOP_EPS, LOOP_ITERS, axis=axis)
    return _loop_cache[key]


@pytest.mark.parametrize("axis", [None, Y], ids=["free", "axis"])
def test_oracle_loop_pair_count_is_stable_under_a_small_perturbation(oracle, axis):
    """The GPU loop test asks for K EQUAL to this loop's.  That is a fair demand only where no pair of the loop's last
    passes sits within rounding of the radius: here every entry of T is moved by +-1e-9 before each search (1e4 times the
    difference the GPU test allows to build up) and the pair count of every pass must not move."""
    src, tgt, sn, tn, T, ks = chair_loop(oracle, axis)
    nudge = np.zeros((4, 4))
    nudge[:3, :] = np.random.default_rng(7).choice([-1e-9, 1e-9], size=(3, 4))
    _, ks2 = oracle_loop(oracle, src, tgt, sn, tn, LOOP_R, LOOP_EPS, LOOP_ITERS, axis=axis, nudge=nudge)
    assert ks2 == ks, (ks, ks2)
    assert ks[-1] > 1000


# ---------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------
def _clouds(rng, ns, nt, spread=1.0):
    tgt = (rng.random((nt, 3)) * 2 - 1) * spread
    src = (rng.random((ns, 3)) * 2 - 1) * spread
    return src.astype(np.float32), tgt.astype(np.float32)


def _same(a, b):
    return (np.array_equal(a.transformation_, b.transformation_) and a.num_correspondences == b.num_correspondences and
            a.fitness_ == b.fitness_ and a.inlier_rmse_ == b.inlier_rmse_ and a.iterations == b.iterations)


def _same_info(a, b):
    return a.cost == b.cost and a.mahalanobis_rmse == b.mahalanobis_rmse


# ---- 1. one pass against the specification ----
SHAPES = [
    (1, 1, 10.0),
    (257, 513, 0.5),        # just past tile / chunk boundaries
    (1000, 777, 0.3),       # ragged, single chunk tail
    (5000, 20000, 0.075),   # C1/C2 shape
    (3, 100000, 0.05),
    (300000, 3000, 0.1),    # more than 1,024 x 256 source positions: the grid-stride loop runs twice
]
_pass_cache = {}


def _pass_case(oracle, ns, nt, radius):
    key = (ns, nt)
    if key not in _pass_cache:
        rng = np.random.default_rng(ns * 31 + nt)
        src, tgt = _clouds(rng, ns, nt)
        T = _rand_T(rng, 0.1, 0.05)
        k, oidx, od2 = oracle.k_nn_pass(src, tgt, T[:3, :].astype(np.float32), np.float32(radius * radius), grid=(ns * nt > 5e7))
        _pass_cache[key] = dict(src=src, tgt=tgt, T=T, k=k, oidx=oidx, od2=od2, sn=_unit_normals(rng, ns), tn=_unit_normals(rng, nt),
                                spec={})
    return _pass_cache[key]


def _spec_of(case, idx, eps, tag):
    if (tag, eps) not in case["spec"]:
        case["spec"][(tag, eps)] = spec_pass(case["src"], case["tgt"], case["T"], idx, case["sn"], case["tn"], eps)
    return case["spec"][(tag, eps)]


def _errors(st, info, ost, ocost):
    serr = float(np.max(np.abs(st - ost) / np.maximum(np.abs(ost), 1.0)))
    cerr = abs(info.cost - ocost) / max(abs(ocost), 1.0)
    return serr, cerr


def _check_reduction(ctx, case, eps, idx, tag, what):
    st, info = ctx.reduce_gicp(eps)
    ost, ocost = _spec_of(case, idx, eps, tag)
    serr, cerr = _errors(st, info, ost, ocost)
    k = int((idx >= 0).sum())
    print("generalized pass %s eps %g: statistics vs specification %.3e, cost %.3e (K = %d, cost = %.6g)" % (what, eps, serr, cerr, k, info.cost))
    assert np.isfinite(st).all()
    assert serr < TOL_STATS and cerr < TOL_STATS
    assert st[0] == k and not st[29:].any()
    assert info.mahalanobis_rmse == (math.sqrt(info.cost / k) if k else 0.0)
    return st, info


@pytest.mark.gpu
@pytest.mark.parametrize("eps", EPSILONS, ids=lambda e: "eps=%g" % e)
@pytest.mark.parametrize("ns,nt,radius", SHAPES)
def test_one_pass_against_the_specification(gpu_ctx, oracle, ns, nt, radius, eps):
    """The fp32 search (brute force and grid): its pairs are the kernel specification's bit for bit, the reduction reads
    the fp32 copies of points and normals.
    Bound: statistics and cost within 1e-9 relative to max(|spec|, 1), the project's bar for the trimmed and robust
    statistics; M's condition number 1 / eps = 1e3 leaves about 1e-13.
    Measured on the MI355X over all shapes, both epsilons, the two fp32 searches and the f64 search: statistics within
    8.3e-13, the cost within 8.9e-15."""
    case = _pass_case(oracle, ns, nt, radius)
    gpu_ctx.set_target(case["tgt"]); gpu_ctx.set_source(case["src"])
    gpu_ctx.set_target_normals_f64(case["tn"]); gpu_ctx.set_source_normals_f64(case["sn"])
    gpu_ctx.nn_pass(case["T"], radius)
    _check_reduction(gpu_ctx, case, eps, case["oidx"], "oracle", "fp32 %s" % gpu_ctx.nn_mode_name)
    # K and all pairs are still what get_correspondences returns
    v = case["oidx"] >= 0
    si, ti, d2 = gpu_ctx.get_correspondences()
    assert len(si) == case["k"] and np.array_equal(ti, case["oidx"][v]) and np.array_equal(d2, case["od2"][v])


@pytest.mark.gpu
@pytest.mark.parametrize("eps", EPSILONS, ids=lambda e: "eps=%g" % e)
@pytest.mark.parametrize("ns,nt,radius", SHAPES)
def test_one_pass_f64_search_against_the_specification(lib, oracle, ns, nt, radius, eps):
    """The default (exact, f64) search: the reduction reads the f64 copies of points and normals, the source in the
    engine's own order.  The exact search decides near-ties and pairs at the radius in f64, the kernel specification in
    fp32, so a few pairs in 1e5 may differ: the specification runs over the pairs the pass reports, which must be the
    kernel specification's but for that share.  Same bound.
    Measured on the MI355X: no pair differs on any shape."""
    case = _pass_case(oracle, ns, nt, radius)
    c = lib.Context(0)
    c.set_clouds_f64(case["src"].astype(np.float64), case["tgt"].astype(np.float64))
    c.set_target_normals_f64(case["tn"]); c.set_source_normals_f64(case["sn"])
    c.nn_pass(case["T"], radius)
    idx = c.correspondence_index().copy()
    differ = int((idx != case["oidx"]).sum())
    print("f64 search: %d of %d source points paired otherwise than by the fp32 specification" % (differ, ns))
    assert differ <= max(3, ns // 10000)
    _check_reduction(c, case, eps, idx, "f64", "f64")
    c.close()


@pytest.mark.gpu
def test_one_pass_f64_search_reads_the_f64_normals(lib, oracle):
    """Normals that fp32 does NOT hold exactly, on the f64 search: the reduction must read the f64 copies of both
    clouds' normals.  The specification over the fp32-rounded normals differs from the one over the f64 normals by far
    more than the bound (asserted below), so a kernel that read the fp32 copy of either array would miss it."""
    case = dict(_pass_case(oracle, 5000, 20000, 0.075))
    rng = np.random.default_rng(11)
    for key, n in (("sn", 5000), ("tn", 20000)):
        v = rng.standard_normal((n, 3))
        case[key] = v / np.linalg.norm(v, axis=1, keepdims=True)
    case["spec"] = {}
    c = lib.Context(0)
    c.set_clouds_f64(case["src"].astype(np.float64), case["tgt"].astype(np.float64))
    c.set_target_normals_f64(case["tn"]); c.set_source_normals_f64(case["sn"])
    c.nn_pass(case["T"], 0.075)
    idx = c.correspondence_index().copy()
    assert int((idx != case["oidx"]).sum()) <= 3
    st, _ = _check_reduction(c, case, 1e-3, idx, "f64", "f64, normals beyond fp32")
    c.close()
    ost, _ = _spec_of(case, idx, 1e-3, "f64")
    for key in ("sn", "tn"):                             # either array read from its fp32 copy would show
        rounded = dict(case)
        rounded[key] = case[key].astype(np.float32).astype(np.float64)
        rst, _ = spec_pass(rounded["src"], rounded["tgt"], rounded["T"], idx, rounded["sn"], rounded["tn"], 1e-3)
        gap = float(np.max(np.abs(rst - ost) / np.maximum(np.abs(ost), 1.0)))
        print("specification with the fp32-rounded %s against the f64 one: %.3e" % (key, gap))
        assert gap > 10.0 * TOL_STATS


def _few(near, seed):
    rng = np.random.default_rng(seed)
    _, tgt = _clouds(rng, 1, 2000)
    src = (rng.random((300, 3)).astype(np.float32) + 50.0).astype(np.float32)
    src[:near] = tgt[:near] + np.float32(0.001)
    perm = rng.permutation(300)
    return src[perm], tgt, _unit_normals(rng, 300), _unit_normals(rng, 2000)


@pytest.mark.gpu
@pytest.mark.parametrize("near", [1, 2])
def test_one_pass_with_few_pairs(gpu_ctx, oracle, near):
    src, tgt, sn, tn = _few(near, 79 + near)
    T = np.eye(4)
    k, oidx, od2 = oracle.k_nn_pass(src, tgt, T[:3, :].astype(np.float32), np.float32(0.05 * 0.05))
    assert k == near
    case = dict(src=src, tgt=tgt, T=T, sn=sn, tn=tn, spec={})
    gpu_ctx.set_target(tgt); gpu_ctx.set_source(src)
    gpu_ctx.set_target_normals_f64(tn); gpu_ctx.set_source_normals_f64(sn)
    gpu_ctx.nn_pass(T, 0.05)
    for eps in EPSILONS:
        _check_reduction(gpu_ctx, case, eps, oidx, "oracle", "K = %d" % near)


@pytest.mark.gpu
def test_one_pass_without_pairs(gpu_ctx, oracle):
    """K = 0 (radius 1e-6): every statistic and the cost are 0, the update is the identity, nothing faults"""
    src, tgt, sn, tn = _few(0, 79)
    T = _rand_T(np.random.default_rng(4), 0.1, 0.0)
    T[:3, 3] = 0.0
    k, oidx, _ = oracle.k_nn_pass(src, tgt, T[:3, :].astype(np.float32), np.float32(1e-6 * 1e-6))
    assert k == 0
    gpu_ctx.set_target(tgt); gpu_ctx.set_source(src)
    gpu_ctx.set_target_normals_f64(tn); gpu_ctx.set_source_normals_f64(sn)
    gpu_ctx.nn_pass(T, 1e-6)
    st, info = gpu_ctx.reduce_gicp(1e-3)
    assert not st.any() and info.cost == 0.0 and info.mahalanobis_rmse == 0.0
    res = gpu_ctx.run_gicp(T, 1e-6, 1e-3, max_iter=3, rel_fitness=0.0, rel_rmse=0.0)
    assert res.iterations == 3 and res.num_correspondences == 0 and res.fitness_ == 0.0 and res.inlier_rmse_ == 0.0
    assert np.array_equal(res.transformation_, T)
    assert res.gicp.cost == 0.0 and res.gicp.mahalanobis_rmse == 0.0


@pytest.mark.gpu
def test_zero_source_normals_are_an_isotropic_source(gpu_ctx, oracle):
    """every source normal 0: C = 2 I - (1 - eps) n n^T, nothing divides by a norm"""
    case = dict(_pass_case(oracle, 1000, 777, 0.3))
    case["sn"] = np.zeros_like(case["sn"])
    case["spec"] = {}
    gpu_ctx.set_target(case["tgt"]); gpu_ctx.set_source(case["src"])
    gpu_ctx.set_target_normals_f64(case["tn"]); gpu_ctx.set_source_normals_f64(case["sn"])
    gpu_ctx.nn_pass(case["T"], 0.3)
    for eps in EPSILONS:
        _check_reduction(gpu_ctx, case, eps, case["oidx"], "oracle", "zero source normals")


@pytest.mark.gpu
def test_non_finite_normals_reach_the_sums_only(gpu_ctx, oracle):
    """a NaN and an infinite normal among the pairs: K, the pairs and sum |d|^2 are those of the clean pass, the run ends"""
    case = _pass_case(oracle, 1000, 777, 0.3)
    v = np.flatnonzero(case["oidx"] >= 0)
    sn, tn = case["sn"].copy(), case["tn"].copy()
    sn[v[0]] = np.nan
    tn[case["oidx"][v[1]]] = np.inf
    gpu_ctx.set_target(case["tgt"]); gpu_ctx.set_source(case["src"])
    gpu_ctx.set_target_normals_f64(tn); gpu_ctx.set_source_normals_f64(sn)
    gpu_ctx.nn_pass(case["T"], 0.3)
    st, info = gpu_ctx.reduce_gicp(1e-3)
    ost, _ = _spec_of(case, case["oidx"], 1e-3, "oracle")
    assert st[0] == case["k"] and abs(st[1] - ost[1]) <= 1e-12 * ost[1]
    assert not np.isfinite(st[2:29]).all()
    si, ti, _ = gpu_ctx.get_correspondences()
    assert len(si) == case["k"] and np.array_equal(ti, case["oidx"][case["oidx"] >= 0])


# ---- 2. the loop against the numpy-built loop ----
@pytest.mark.gpu
@pytest.mark.parametrize("axis", [None, Y], ids=["free", "axis"])
def test_loop_against_the_oracle_built_loop(lib, oracle, axis):
    """The chair 5,000 -> 20,000 fixture with normals from estimate_normals, 10 iterations from the identity at the
    fixture's radius, without and with a rotation axis.  Bound: the project's TOL_T = 1e-5 relative Frobenius, K equal
    (test_oracle_loop_pair_count_is_stable_under_a_small_perturbation shows that K may be asked for).
    Measured on the MI355X: K equal (2,352), T within 2.3e-8 without and 1.4e-8 with the axis -- the fp32 pass reads the
    fp32 copy of the estimated normals (which fp32 does not hold exactly), the oracle loop their f64 values."""
    src, tgt, sn, tn, T_ref, ks = chair_loop(oracle, axis)
    c = lib.Context(0)
    c.set_search_precision("f32")                        # the kernel specification's search
    c.set_target(tgt); c.set_source(src)
    c.set_target_normals_f64(tn); c.set_source_normals_f64(sn)
    if axis is not None:
        c.set_rotation_axis(axis)
    res = c.run_gicp(None, LOOP_R, LOOP_EPS, max_iter=LOOP_ITERS, rel_fitness=0.0, rel_rmse=0.0)
    c.close()
    err = synth.rel_frobenius(res.transformation_, T_ref)
    print("generalized loop (%s) vs oracle-built loop: rel. Frobenius %.3e (K %d / %d)" %
          ("axis" if axis is not None else "free", err, res.num_correspondences, ks[-1]))
    assert res.iterations == LOOP_ITERS
    assert res.num_correspondences == ks[-1]
    assert err < TOL_T
    if axis is not None:
        assert np.abs(res.transformation_[:3, :3] @ axis - axis).max() < 1e-12


# ---- 3. it does what it is for ----
def _ellipsoid(n, seed, axes=(0.5, 0.3, 0.2), centre=(0.3, -0.2, 1.0), noise=0.0):
    """points on an ellipsoid with three different axes and their exact unit normals (as tests/test_axis_icp.py)"""
    rng = np.random.default_rng(seed)
    u = rng.normal(size=(n, 3))
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    a = np.asarray(axes)
    p = u * a
    nrm = p / a ** 2
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    p = p + rng.normal(size=p.shape) * noise + np.asarray(centre)
    return p, nrm


def quality_case():
    """an exact model of 3,000 points against a scan of 20,000 with 3 mm noise, 5 degrees / 3 cm off"""
    tgt, tn = _ellipsoid(20000, 40, noise=3e-3)
    src, sn = _ellipsoid(3000, 50)
    c0 = np.array([0.3, -0.2, 1.0])
    a = np.array([0.3, 1.0, -0.2]) / np.linalg.norm([0.3, 1.0, -0.2])
    T_gt = np.eye(4)
    T_gt[:3, :3] = _rot(a, math.radians(5.0))
    T_gt[:3, 3] = c0 - T_gt[:3, :3] @ c0 + np.array([0.02, -0.015, 0.017])
    Ti = np.linalg.inv(T_gt)
    return src @ Ti[:3, :3].T + Ti[:3, 3], sn @ Ti[:3, :3].T, tgt, tn, T_gt


@pytest.mark.gpu
@pytest.mark.parametrize("passes", [3, 15])
def test_generalized_beats_point_to_point_on_a_noisy_surface_with_exact_normals(lib, passes):
    """Relative Frobenius error to the true transform after the same number of passes from the identity at r = 0.15:
    generalized (eps = 1e-3) below point-to-point, a comparison with no constant.  A numpy loop of the specification
    over the CPU oracle's nearest neighbours gave, on this case, 2.0e-3 against 3.8e-2 after 3 passes and 1.2e-3 against
    1.6e-2 after 15.
    Measured on the MI355X: 2.043e-3 against 3.840e-2 (closed-form point-to-point 3.837e-2) after 3 passes, 1.245e-3
    against 1.569e-2 (1.554e-2) after 15."""
    src, sn, tgt, tn, T_gt = quality_case()
    c = lib.Context(0)
    c.set_clouds_f64(src, tgt)
    c.set_target_normals_f64(tn); c.set_source_normals_f64(sn)
    g = c.run_gicp(None, 0.15, 1e-3, max_iter=passes, rel_fitness=0.0, rel_rmse=0.0)
    p = c.run_gicp(None, 0.15, 1.0, max_iter=passes, rel_fitness=0.0, rel_rmse=0.0)
    k = c.run(None, 0.15, passes, 0.0, 0.0)
    c.close()
    eg, ep, ek = (synth.rel_frobenius(x.transformation_, T_gt) for x in (g, p, k))
    print("noisy ellipsoid, %d passes: generalized %.3e, eps = 1 (point-to-point Gauss-Newton) %.3e, closed-form point-to-point %.3e" %
          (passes, eg, ep, ek))
    assert g.iterations == passes and p.iterations == passes
    assert eg < ep and eg < ek


# ---- 4. state, repeatability, equivalence ----
def _state_case():
    src, sn, tgt, tn, _ = quality_case()
    return src, sn, tgt, tn


def _gicp_ctx(lib, case):
    src, sn, tgt, tn = case
    c = lib.Context(0)
    c.set_clouds_f64(src, tgt)
    c.set_target_normals_f64(tn); c.set_source_normals_f64(sn)
    return c


@pytest.mark.gpu
def test_two_runs_are_bit_identical(lib):
    case = _state_case()
    out = []
    for _ in range(2):
        c = _gicp_ctx(lib, case)
        res = c.run_gicp(None, 0.15, 1e-3, max_iter=8, rel_fitness=0.0, rel_rmse=0.0)
        c.nn_pass(res.transformation_, 0.15)
        st, info = c.reduce_gicp(1e-3)
        out.append((res, st.view(np.uint64).copy(), info))
        c.close()
    (a, sa, ia), (b, sb, ib) = out
    assert _same(a, b) and _same_info(a.gicp, b.gicp) and np.array_equal(sa, sb) and _same_info(ia, ib)


@pytest.mark.gpu
def test_other_passes_after_a_generalized_run_equal_a_fresh_context(lib):
    """a plain run, a trimmed pass and a robust pass (they share the pair-pass scratch) after a generalized run: what a
    fresh context returns, bit for bit"""
    case = _state_case()
    out = []
    for with_gicp in (True, False):
        c = _gicp_ctx(lib, case)
        if with_gicp:
            c.run_gicp(None, 0.15, 1e-3, max_iter=5, rel_fitness=0.0, rel_rmse=0.0)
        plain = c.run(None, 0.15, 10, 0.0, 0.0)
        c.nn_pass(plain.transformation_, 0.15)
        st_t, it = c.reduce_trimmed(0.7)
        mask = c.kept_mask().copy()
        c.nn_pass(plain.transformation_, 0.15)
        st_r, ir = c.reduce_robust("tukey", plane=True)
        w = c.pair_weights().copy()
        out.append((plain, st_t.view(np.uint64).copy(), (it.kept, it.trimmed_rmse, it.d2_cut), mask,
                    st_r.view(np.uint64).copy(), (ir.scale, ir.median_residual, ir.weight_sum, ir.zero_weight, ir.robust_rmse),
                    w.view(np.uint64).copy()))
        c.close()
    a, b = out
    assert _same(a[0], b[0])
    for x, y in zip(a[1:], b[1:]):
        assert np.array_equal(x, y) if isinstance(x, np.ndarray) else x == y


@pytest.mark.gpu
def test_sweep_equals_single_runs(lib):
    case = _state_case()
    level, r = 4, 0.15
    c = _gicp_ctx(lib, case)
    best, bl, per = c.run_yaw_sweep_gicp(level, r, 1e-3, max_iter=6, rel_fitness=0.0, rel_rmse=0.0)
    c.close()
    c = _gicp_ctx(lib, case)
    singles = []
    for i in range(level):
        a = 2.0 * math.pi / level * i
        init = np.eye(4)
        init[0, 0] = math.cos(a); init[0, 2] = math.sin(a); init[2, 0] = -math.sin(a); init[2, 2] = math.cos(a)
        singles.append(c.run_gicp(init, r, 1e-3, max_iter=6, rel_fitness=0.0, rel_rmse=0.0))
    c.close()
    for x, y in zip(per, singles):
        assert _same(x, y) and _same_info(x.gicp, y.gicp)
    ks = [x.num_correspondences for x in singles]
    assert bl == int(np.argmax(ks))                     # the first with strictly the most
    assert _same(best, singles[bl]) and _same_info(best.gicp, singles[bl].gicp)


@pytest.mark.gpu
def test_run_without_normals_returns_init(lib):
    src, sn, tgt, tn = _state_case()
    init = _rand_T(np.random.default_rng(8), 0.05, 0.01)
    for which in ("none", "target", "source"):
        c = lib.Context(0)
        c.set_clouds_f64(src, tgt)
        if which == "target":
            c.set_target_normals_f64(tn)
        if which == "source":
            c.set_source_normals_f64(sn)
        res = c.run_gicp(init, 0.15, 1e-3, max_iter=5)
        assert np.array_equal(res.transformation_, init) and res.num_correspondences == 0 and res.iterations == 0, which
        c.nn_pass(init, 0.15)
        with pytest.raises(lib.IcpError) as e:
            c.reduce_gicp(1e-3)
        assert e.value.code == STATE, which
        c.close()
    # both sets of normals, but no pass yet
    c = _gicp_ctx(lib, (src, sn, tgt, tn))
    with pytest.raises(lib.IcpError) as e:
        c.reduce_gicp(1e-3)
    assert e.value.code == STATE
    c.close()


@pytest.mark.gpu
def test_sharded_gpu_context_is_invalid(lib):
    src, tgt, _, r = synth.make_pair(2000, 8000)
    c = lib.Context(0)
    c.set_target_shard(0, len(tgt), tgt.mean(0))
    c.set_clouds_f64(src, tgt)
    with pytest.raises(lib.IcpError) as e:
        c.run_gicp(None, r, 1e-3, max_iter=5)
    assert e.value.code == INVALID
    c.close()


# ---- 5. the C++ shim ----
def _run_driver(binary, tmp_path, s, t, sn, tn, r, eps, iters):
    inp, outp = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(inp, "wb") as f:
        f.write(struct.pack("<qqddii", len(s), len(t), r, eps, iters, 0))
        for a in (s, t, sn, tn):
            f.write(np.ascontiguousarray(a, "<f8").tobytes())
    p = subprocess.run([binary, inp, outp], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, (p.returncode, p.stderr)
    raw = open(outp, "rb").read()
    off = 0
    T = np.frombuffer(raw, "<f8", 16, off).reshape(4, 4); off += 128
    fit, rmse = struct.unpack_from("<dd", raw, off); off += 16
    (n,) = struct.unpack_from("<q", raw, off); off += 8
    corr = np.frombuffer(raw, "<i4", 2 * n, off).reshape(n, 2); off += 8 * n
    (host_rmse,) = struct.unpack_from("<d", raw, off); off += 8
    host_T = np.frombuffer(raw, "<f8", 16, off).reshape(4, 4); off += 128
    (init_returned,) = struct.unpack_from("<i", raw, off)
    return T, fit, rmse, corr, host_rmse, host_T, init_returned, p.stderr


@pytest.mark.gpu
def test_shim_driver_equals_the_c_abi(lib, oracle, driver_bins, tmp_path):
    src, sn, tgt, tn = _state_case()
    r, eps, iters = 0.15, 1e-3, 10
    c = _gicp_ctx(lib, (src, sn, tgt, tn))
    res = c.run_gicp(None, r, eps, max_iter=iters)      # the reference's default criteria, like the driver
    corr = np.stack(c.get_correspondences()[:2], 1)
    c.close()
    # the host restatements against the specification over the same pairs
    T = res.transformation_
    p = transform(src, T)[corr[:, 0]]
    ost, ocost = gicp_stats(p, tgt[corr[:, 1]], (sn @ T[:3, :3].T)[corr[:, 0]], tn[corr[:, 1]], eps)
    ok, upd = oracle.k_solve_gn(ost)
    assert ok
    for b in driver_bins:
        T1, fit1, rmse1, corr1, host_rmse, host_T, init_returned, err = _run_driver(b, tmp_path, src, tgt, sn, tn, r, eps, iters)
        assert np.array_equal(T1, res.transformation_) and fit1 == res.fitness_ and rmse1 == res.inlier_rmse_, b
        assert np.array_equal(corr1, corr), b
        assert abs(host_rmse - math.sqrt(ocost / len(corr))) <= 1e-12 * host_rmse, b
        assert synth.rel_frobenius(host_T, upd) < 1e-9, b
        assert init_returned == 1 and "normal" in err, b   # without source normals: message, init, no pairs
