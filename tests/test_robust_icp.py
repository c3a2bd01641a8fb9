"""Robust ICP (visma_amd/csrc/robust.hip): iteratively re-weighted least squares with Huber, Tukey or Cauchy weights, the
scale fixed by the caller or max(tune * 1.4826 * lower median of the residuals, min_scale) per pass (visma_icp.h).

CPU: the symbols and methods exist, the argument checks, the C++ driver against the stand-alone headers, and the numpy
specification (weights, scale, the 38 weighted sums) every GPU check below uses as its yardstick.
GPU: every oracle is assembled here from pieces that are not under test -- the committed kernel specification
(Oracle.k_nn_pass for the pairs), numpy for weights and sums, the compiled reference (Ref.evaluate_registration) and the
oracle's solves from statistics (k_solve_kabsch, k_solve_gn) for the loop.
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
sys.path.insert(0, os.path.join(HERE, "cpp"))
import build_shim  # noqa: E402
import build_robust  # noqa: E402

TOL_T = 1e-5       # north_star: final SE(3) within 1e-5 relative Frobenius of the CPU reference (test_gpu_kernels.py)
INVALID, STATE = 1, 5
L2, HUBER, TUKEY, CAUCHY = 0, 1, 2, 3
FAMILIES = [HUBER, TUKEY, CAUCHY]
NAMES = {HUBER: "huber", TUKEY: "tukey", CAUCHY: "cauchy"}
TUNE = {HUBER: 1.345, TUKEY: 4.685, CAUCHY: 2.385}   # 95 % efficiency (Holland & Welsch 1977)


# ---------------------------------------------------------------------------
# the yardstick: weights, scale and the weighted statistics in numpy
# ---------------------------------------------------------------------------
def weights(kernel, r, c):
    """w(r) at scale c; c == 0: 1 where r == 0, else 0"""
    r = np.asarray(r, np.float64)
    if not c > 0.0:
        return (r == 0.0).astype(np.float64)
    u = r / c
    if kernel == HUBER:
        return np.where(r <= c, 1.0, c / np.where(r > 0.0, r, 1.0))
    if kernel == TUKEY:
        t = 1.0 - u * u
        return np.where(r < c, t * t, 0.0)
    if kernel == CAUCHY:
        return 1.0 / (1.0 + u * u)
    raise ValueError(kernel)


def lower_median(values):
    """the m-th smallest, m = (K + 1) / 2"""
    m = (len(values) + 1) // 2
    return np.partition(values, m - 1)[m - 1]


def auto_scale(v32, kernel, tune=0.0, min_scale=0.0):
    """c = max(tune * 1.4826 * sqrt((double)v), min_scale), v the fp32 squared lower median"""
    t = tune if tune else TUNE[kernel]
    return max(t * 1.4826 * math.sqrt(float(np.float32(v32))), min_scale)


def pairs(src, tgt, T, idx, normals=None):
    """p = T64 * s per pair in f64 (row by row, in the kernel's order), q, n, the residual; zeros where idx < 0"""
    v = idx >= 0
    s = np.asarray(src, np.float64)[:, :3]
    p = np.empty_like(s)
    for k in range(3):
        p[:, k] = ((T[k, 0] * s[:, 0] + T[k, 1] * s[:, 1]) + T[k, 2] * s[:, 2]) + T[k, 3]
    q = np.zeros_like(p)
    q[v] = np.asarray(tgt, np.float64)[idx[v], :3]
    d = p - q
    n = None
    if normals is None:
        r = np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])
    else:
        n = np.zeros_like(p)
        n[v] = np.asarray(normals, np.float64)[idx[v]]
        r = np.abs((d[:, 0] * n[:, 0] + d[:, 1] * n[:, 1]) + d[:, 2] * n[:, 2])
    r[~v] = 0.0
    return p, q, n, r, v


def weighted_stats(p, q, n, w, v):
    """the 38 statistics of visma_icp.h with every pair's contribution times w (n given: the point-to-plane rows)"""
    w, p, q = w[v], p[v], q[v]
    st = np.zeros(38)
    d = p - q
    W = st[0] = w.sum()
    st[1] = (w * (d * d).sum(1)).sum()
    if n is None:
        P = (w[:, None] * p).sum(0)
        Q = (w[:, None] * q).sum(0)
        S = np.einsum("i,ia,ib->ab", w, p, p)
        M = np.einsum("i,ia,ib->ab", w, q, p).reshape(9)                 # M[a, b] = sum w q_a p_b
        st[2:23] = [S[1, 1] + S[2, 2], -S[0, 1], -S[0, 2], 0.0, -P[2], P[1],
                    S[0, 0] + S[2, 2], -S[1, 2], P[2], 0.0, -P[0],
                    S[0, 0] + S[1, 1], -P[1], P[0], 0.0,
                    W, 0.0, 0.0, W, 0.0, W]
        st[23:26] = [-(M[7] - M[5]), -(M[2] - M[6]), -(M[3] - M[1])]
        st[26:29] = P - Q
        st[29:38] = M
    else:
        n = n[v]
        rr = (d * n).sum(1)
        J = np.concatenate([np.cross(p, n), n], 1)
        st[2:23] = np.einsum("i,ia,ib->ab", w, J, J)[np.triu_indices(6)]
        st[23:29] = (w[:, None] * J * rr[:, None]).sum(0)
    return st


def test_weight_functions_are_continuous_at_the_scale():
    c = 0.37
    for k in FAMILIES:
        below, at, above = weights(k, [np.nextafter(c, 0.0), c, np.nextafter(c, 1.0)], c)
        assert abs(below - at) < 1e-14 and abs(above - at) < 1e-14, NAMES[k]
    assert weights(HUBER, [c], c)[0] == 1.0 and weights(TUKEY, [c], c)[0] == 0.0 and weights(CAUCHY, [c], c)[0] == 0.5
    assert weights(HUBER, [2 * c], c)[0] == 0.5
    assert weights(TUKEY, [c / 2], c)[0] == 0.5625
    for k in FAMILIES:                                   # monotone, in [0, 1], 1 at r = 0
        w = weights(k, np.linspace(0.0, 3.0 * c, 301), c)
        assert w[0] == 1.0 and (np.diff(w) <= 0.0).all() and (w >= 0.0).all() and (w <= 1.0).all()


def test_weight_functions_zero_scale_and_tukey_support():
    r = np.array([0.0, 1e-300, 1e-12, 1.0])
    for k in FAMILIES:
        w = weights(k, r, 0.0)
        assert list(w) == [1.0, 0.0, 0.0, 0.0] and np.isfinite(w).all()
    w = weights(TUKEY, [0.5, 1.0, np.nextafter(1.0, 2.0), 7.0], 1.0)
    assert w[0] > 0.0 and list(w[1:]) == [0.0, 0.0, 0.0]


def test_scale_rule():
    assert lower_median(np.array([5.0, 1.0, 3.0])) == 3.0               # K = 3: m = 2
    assert lower_median(np.array([4.0, 1.0, 3.0, 2.0])) == 2.0          # K = 4: m = 2, the LOWER median
    assert lower_median(np.array([7.0])) == 7.0
    v = np.float32(0.04)
    assert auto_scale(v, TUKEY) == 4.685 * 1.4826 * math.sqrt(float(v))
    assert auto_scale(v, HUBER, tune=2.0) == 2.0 * 1.4826 * math.sqrt(float(v))
    assert auto_scale(v, CAUCHY, min_scale=10.0) == 10.0
    assert auto_scale(np.float32(0.0), HUBER) == 0.0


# ---------------------------------------------------------------------------
# CPU: interface
# ---------------------------------------------------------------------------
NEW_SYMBOLS = ["visma_icp_reduce_robust", "visma_icp_run_robust", "visma_icp_run_yaw_sweep_robust", "visma_icp_get_pair_weights"]


def test_symbols_and_methods(lib):
    L = lib.load()
    for name in NEW_SYMBOLS:
        assert hasattr(L, name), name
    for name in ["reduce_robust", "run_robust", "run_yaw_sweep_robust", "pair_weights"]:
        assert callable(getattr(lib.Context, name, None)), name
    assert hasattr(lib, "RobustInfo")


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
    return src, tgt


BAD = [float("nan"), float("inf"), float("-inf"), -1.0]
BAD_CONFIGS = ([dict(kernel=TUKEY, scale=b) for b in BAD] + [dict(kernel=HUBER, tune=b) for b in BAD] +
               [dict(kernel=CAUCHY, min_scale=b) for b in BAD] + [dict(kernel=4), dict(kernel=-1)])


@pytest.mark.parametrize("cfg", BAD_CONFIGS, ids=lambda c: ",".join("%s=%s" % kv for kv in c.items()))
def test_bad_configuration_is_invalid_before_any_pass(lib, hctx, cfg):
    src, tgt = _small_clouds()
    hctx.set_target(tgt); hctx.set_source(src)
    hctx.nn_pass(np.eye(4), 0.1)
    calls = dict(hctx.engine.calls)
    for call in (lambda: hctx.run_robust(None, 0.1, max_iter=5, **cfg), lambda: hctx.reduce_robust(**cfg),
                 lambda: hctx.run_yaw_sweep_robust(4, 0.1, max_iter=5, **cfg)):
        with pytest.raises(lib.IcpError) as e:
            call()
        assert e.value.code == INVALID
    assert hctx.engine.calls == calls                    # nothing was launched


def test_null_outputs_and_missing_clouds(lib, hctx):
    import ctypes as C
    L, h = hctx.L, hctx._h
    init = np.eye(4).reshape(16)
    dp = C.POINTER(C.c_double)
    res, info, st = lib.CResult(), lib.CRobustInfo(), np.zeros(38)
    cfg = lib.CRobust(TUKEY, 0.0, 0.0, 0.0)
    ip = init.ctypes.data_as(dp)
    # a context without clouds
    assert L.visma_icp_run_robust(h, ip, 0.1, C.byref(cfg), 0, 5, 0.0, 0.0, 0, C.byref(res), C.byref(info)) == STATE
    assert L.visma_icp_reduce_robust(h, C.byref(cfg), 0, st.ctypes.data_as(dp), C.byref(info)) == STATE
    assert L.visma_icp_get_pair_weights(h, (C.c_double * 4)()) == STATE
    src, tgt = _small_clouds()
    hctx.set_target(tgt); hctx.set_source(src)
    # NULL result / init / configuration / statistics / info / weights
    assert L.visma_icp_run_robust(h, ip, 0.1, C.byref(cfg), 0, 5, 0.0, 0.0, 0, None, C.byref(info)) == INVALID
    assert L.visma_icp_run_robust(h, None, 0.1, C.byref(cfg), 0, 5, 0.0, 0.0, 0, C.byref(res), C.byref(info)) == INVALID
    assert L.visma_icp_run_robust(h, ip, 0.1, None, 0, 5, 0.0, 0.0, 0, C.byref(res), C.byref(info)) == INVALID
    assert L.visma_icp_reduce_robust(h, C.byref(cfg), 0, None, C.byref(info)) == INVALID
    assert L.visma_icp_reduce_robust(h, C.byref(cfg), 0, st.ctypes.data_as(dp), None) == INVALID
    assert L.visma_icp_reduce_robust(h, None, 0, st.ctypes.data_as(dp), C.byref(info)) == INVALID
    assert L.visma_icp_get_pair_weights(h, None) == INVALID
    assert L.visma_icp_run_yaw_sweep_robust(h, 4, 0.1, C.byref(cfg), 0, 5, 0.0, 0.0, None, None, None, None, None) == INVALID
    assert L.visma_icp_run_yaw_sweep_robust(h, 0, 0.1, C.byref(cfg), 0, 5, 0.0, 0.0, C.byref(res), None, None, None, None) == INVALID
    # negative iteration count; NULL context; a rotation axis does not go with scaling
    assert L.visma_icp_run_robust(h, ip, 0.1, C.byref(cfg), 0, -1, 0.0, 0.0, 0, C.byref(res), C.byref(info)) == INVALID
    assert L.visma_icp_run_robust(None, ip, 0.1, C.byref(cfg), 0, 5, 0.0, 0.0, 0, C.byref(res), C.byref(info)) == INVALID
    hctx.set_rotation_axis([0.0, 1.0, 0.0])
    assert L.visma_icp_run_robust(h, ip, 0.1, C.byref(cfg), 0, 5, 0.0, 0.0, 1, C.byref(res), C.byref(info)) == INVALID


def test_pair_weights_before_any_robust_pass_is_state(lib, hctx):
    src, tgt = _small_clouds()
    hctx.set_target(tgt); hctx.set_source(src)
    hctx.run(None, 0.1, 2, 0.0, 0.0)
    with pytest.raises(lib.IcpError) as e:
        hctx.pair_weights()
    assert e.value.code == STATE


def test_oracle_engine_reports_not_supported(lib, hctx):
    src, tgt = _small_clouds()
    hctx.set_target(tgt); hctx.set_source(src)
    hctx.nn_pass(np.eye(4), 0.1)
    with pytest.raises(lib.IcpError) as e:
        hctx.reduce_robust(TUKEY)
    assert e.value.code == STATE and "not supported" in str(e.value)
    with pytest.raises(lib.IcpError) as e:
        hctx.run_robust(None, 0.1, HUBER, max_iter=5)
    assert e.value.code == STATE and "not supported" in str(e.value)
    # L2 is the plain run on every engine
    a = hctx.run_robust(None, 0.1, L2, max_iter=5, rel_fitness=0.0, rel_rmse=0.0)
    b = hctx.run(None, 0.1, 5, 0.0, 0.0)
    assert np.array_equal(a.transformation_, b.transformation_) and a.num_correspondences == b.num_correspondences
    assert a.robust.weight_sum == a.num_correspondences and a.robust.robust_rmse == b.inlier_rmse_
    w = hctx.pair_weights()
    assert w.sum() == a.num_correspondences and set(np.unique(w)) <= {0.0, 1.0}


def test_sharded_context_is_invalid(lib, hctx):
    src, tgt = _small_clouds()
    hctx.set_target(tgt); hctx.set_source(src)
    fn = lib.ALLREDUCE_FN(lambda user, buf, n: 0)
    hctx._keep.append(fn)
    assert hctx.L.visma_icp_set_allreduce(hctx._h, fn, None, 0, 2) == 0
    for call in (lambda: hctx.run_robust(None, 0.1, TUKEY, max_iter=5), lambda: hctx.reduce_robust(TUKEY),
                 lambda: hctx.run_yaw_sweep_robust(4, 0.1, TUKEY, max_iter=5)):
        with pytest.raises(lib.IcpError) as e:
            call()
        assert e.value.code == INVALID


@pytest.fixture(scope="module")
def driver_bins(lib):
    if build_shim.eigen_dir() is not None:
        build_robust.build()
    paths = [os.path.join(HERE, "cpp", "_build", b) for b in build_robust.BINS]
    if not all(os.path.exists(p) for p in paths):
        pytest.skip("robust driver not prebuilt and no Eigen headers here")
    return paths


def test_cpp_driver_compiles_against_standalone_headers(driver_bins):
    """Both Eigen storage orders: the estimators go through the stock open3d::RegistrationICP without Open3D."""
    for b in driver_bins:
        assert os.path.getsize(b) > 0 and os.access(b, os.X_OK)
    src = open(os.path.join(HERE, "cpp", "robust_driver.cpp")).read()
    assert "cicp::TransformationEstimationPointToPointRobust" in src and "cicp::TransformationEstimationPointToPlaneRobust" in src
    assert "cicp::RegisterModelToScene" in src and "cicp::RobustKernel" in src


# ---------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------
def _rand_T(rng, ang=0.2, tr=0.1):
    w = rng.standard_normal(3)
    w *= ang / np.linalg.norm(w)
    th = np.linalg.norm(w)
    K = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])
    R = np.eye(3) + np.sin(th) / th * K + (1 - np.cos(th)) / th ** 2 * K @ K
    return synth.make_T(R, rng.standard_normal(3) * tr)


def _clouds(rng, ns, nt, spread=1.0):
    tgt = (rng.random((nt, 3)) * 2 - 1) * spread
    src = (rng.random((ns, 3)) * 2 - 1) * spread
    return src.astype(np.float32), tgt.astype(np.float32)


def _unit_normals(rng, n):
    """random unit normals that fp32 holds exactly (the fp32 passes read the fp32 copy)"""
    v = rng.standard_normal((n, 3))
    v /= np.linalg.norm(v, axis=1, keepdims=True)
    return v.astype(np.float32).astype(np.float64)


def _same(a, b):
    return (np.array_equal(a.transformation_, b.transformation_) and a.num_correspondences == b.num_correspondences and
            a.fitness_ == b.fitness_ and a.inlier_rmse_ == b.inlier_rmse_ and a.iterations == b.iterations)


def _same_info(a, b):
    return (a.scale == b.scale and a.median_residual == b.median_residual and a.weight_sum == b.weight_sum and
            a.zero_weight == b.zero_weight and a.robust_rmse == b.robust_rmse)


def _bits64(x):
    return np.float64(x).view(np.uint64)


# ---- 1. one pass, exact and independent (fp32 uploads, the kernel specification as the oracle for the pairs) ----
SHAPES = [
    (1000, 777, 0.3),       # ragged, single chunk tail
    (5000, 20000, 0.075),   # C1/C2 shape
    (257, 513, 0.5),        # just past tile / chunk boundaries
    (70000, 3000, 0.1),     # large-source path (8 points per thread)
    (1, 1, 10.0),
    (3, 100000, 0.05),
    (300000, 3000, 0.1),    # more than 1,024 x 256 source positions: the grid-stride loop runs twice
]
_spec_cache = {}


def _spec_pass(oracle, ns, nt, radius):
    key = (ns, nt)
    if key not in _spec_cache:
        rng = np.random.default_rng(ns * 31 + nt)
        src, tgt = _clouds(rng, ns, nt)
        T = _rand_T(rng, 0.1, 0.05)
        k, oidx, od2 = oracle.k_nn_pass(src, tgt, T[:3, :].astype(np.float32), np.float32(radius * radius), grid=(ns * nt > 5e7))
        nrm = _unit_normals(rng, nt)
        _spec_cache[key] = (src, tgt, T, k, oidx, od2, nrm)
    return _spec_cache[key]


def _check_pass(ctx, src, tgt, T, radius, kernel, scale, min_scale, k, oidx, od2, normals=None, tune=0.0, upload=True):
    """one nn_pass + reduce_robust against the specification; scale 0: the automatic scale.  -> (stats, info, errors)"""
    plane = normals is not None
    if upload:
        ctx.set_target(tgt)
        ctx.set_source(src)
        if plane:
            ctx.set_target_normals_f64(normals)
    ctx.nn_pass(T, radius)
    st, info = ctx.reduce_robust(kernel, scale, tune, min_scale, plane=plane)
    w = ctx.pair_weights()
    p, q, n, r, v = pairs(src, tgt, T, oidx, normals)
    assert int(v.sum()) == k
    if scale > 0.0:
        c = scale
        assert info.scale == scale and info.median_residual == 0.0
    elif k == 0:
        c = min_scale
        assert info.scale == min_scale and info.median_residual == 0.0
    elif not plane:
        v32 = lower_median(od2[v])                       # the fp32 d2 the pass reports
        c = auto_scale(v32, kernel, tune, min_scale)
        assert _bits64(info.scale) == _bits64(c), (info.scale, c)
        assert _bits64(info.median_residual) == _bits64(math.sqrt(float(v32)))
    else:
        v_np = np.float32(lower_median((r[v] * r[v]).astype(np.float32)))
        v_lib = np.float32(info.median_residual ** 2)    # (an fp32 value: sqrt and square in f64 give it back)
        ulps = abs(int(v_lib.view(np.uint32)) - int(v_np.view(np.uint32)))
        print("point-to-plane median^2: library %.9g, numpy %.9g (%d fp32 ulps apart)" % (v_lib, v_np, ulps))
        assert ulps <= 2
        assert _bits64(info.scale) == _bits64(auto_scale(v_lib, kernel, tune, min_scale))
        c = info.scale                                   # the library's own scale goes into the specification
    w_spec = np.where(v, weights(kernel, r, c), 0.0)
    werr = float(np.abs(w - w_spec).max())
    assert werr <= 1e-12, werr
    ost = weighted_stats(p, q, n, w_spec, v)
    serr = float(np.max(np.abs(st - ost) / np.maximum(np.abs(ost), 1.0)))
    print("%s %s scale %.6g: weights vs specification %.3e, statistics %.3e (K = %d, sum w = %.6g, %d with w = 0)" %
          (NAMES[kernel], "plane" if plane else "point", c, werr, serr, k, st[0], info.zero_weight))
    assert np.isfinite(st).all()
    assert serr < 1e-9
    assert info.weight_sum == st[0]
    assert info.zero_weight == int((w_spec[v] == 0.0).sum())
    assert info.robust_rmse == (math.sqrt(st[1] / st[0]) if st[0] > 0.0 else 0.0)
    # all K pairs are still what get_correspondences returns
    si, ti, d2 = ctx.get_correspondences()
    assert len(si) == k and np.array_equal(ti, oidx[v]) and np.array_equal(d2, od2[v])
    return st, info, (werr, serr)


@pytest.mark.gpu
@pytest.mark.parametrize("kernel", FAMILIES, ids=[NAMES[k] for k in FAMILIES])
@pytest.mark.parametrize("ns,nt,radius", SHAPES)
def test_one_pass_against_the_specification(gpu_ctx, oracle, ns, nt, radius, kernel):
    """Bounds: weights 1e-12 absolute (coordinates are O(1), the residual is a few dozen f64 operations: the error is a
    few 1e-14), statistics 1e-9 relative to max(|spec|, 1) (the project's bar for the trimmed statistics), the
    automatic scale equal in its bits.
    Measured on the MI355X over all shapes, families, both scales and both searches: every weight equal to the
    specification's (0 difference), statistics within 2.5e-12."""
    src, tgt, T, k, oidx, od2, _ = _spec_pass(oracle, ns, nt, radius)
    _check_pass(gpu_ctx, src, tgt, T, radius, kernel, radius / 3.0, 0.0, k, oidx, od2)
    _check_pass(gpu_ctx, src, tgt, T, radius, kernel, 0.0, 0.0, k, oidx, od2, upload=False)


@pytest.mark.gpu
@pytest.mark.parametrize("kernel", FAMILIES, ids=[NAMES[k] for k in FAMILIES])
@pytest.mark.parametrize("ns,nt,radius", SHAPES[:2])
def test_one_pass_point_to_plane_against_the_specification(gpu_ctx, oracle, ns, nt, radius, kernel):
    """The automatic scale may differ from numpy's by at most 2 fp32 ulps of v (a last-bit difference in an f64 residual
    can move its fp32 rounding); the library's own scale then goes into the specification.
    Measured on the MI355X: the squared median 0 fp32 ulps from numpy's in every case, every weight equal to the
    specification's, statistics within 1.2e-14."""
    src, tgt, T, k, oidx, od2, nrm = _spec_pass(oracle, ns, nt, radius)
    _check_pass(gpu_ctx, src, tgt, T, radius, kernel, radius / 3.0, 0.0, k, oidx, od2, normals=nrm)
    _check_pass(gpu_ctx, src, tgt, T, radius, kernel, 0.0, 0.0, k, oidx, od2, normals=nrm, upload=False)


@pytest.mark.gpu
def test_one_pass_tune_and_min_scale(gpu_ctx, oracle):
    """a tuning constant of the caller's, and a lower bound that binds"""
    src, tgt, T, k, oidx, od2, _ = _spec_pass(oracle, 1000, 777, 0.3)
    _check_pass(gpu_ctx, src, tgt, T, 0.3, HUBER, 0.0, 0.0, k, oidx, od2, tune=0.7)
    _, info, _ = _check_pass(gpu_ctx, src, tgt, T, 0.3, TUKEY, 0.0, 5.0, k, oidx, od2, upload=False)
    assert info.scale == 5.0 and info.median_residual > 0.0


def _few(near, seed):
    rng = np.random.default_rng(seed)
    _, tgt = _clouds(rng, 1, 2000)
    src = (rng.random((300, 3)).astype(np.float32) + 50.0).astype(np.float32)
    src[:near] = tgt[:near] + np.float32(0.001)
    return src[rng.permutation(300)], tgt


@pytest.mark.gpu
@pytest.mark.parametrize("kernel", FAMILIES, ids=[NAMES[k] for k in FAMILIES])
@pytest.mark.parametrize("near", [1, 2])
def test_one_pass_with_few_pairs(gpu_ctx, oracle, near, kernel):
    """K = 1, 2: the lower median is the smallest residual"""
    src, tgt = _few(near, 79 + near)
    T = np.eye(4)
    k, oidx, od2 = oracle.k_nn_pass(src, tgt, T[:3, :].astype(np.float32), np.float32(0.05 * 0.05))
    assert k == near
    _check_pass(gpu_ctx, src, tgt, T, 0.05, kernel, 0.0, 0.0, k, oidx, od2)
    _check_pass(gpu_ctx, src, tgt, T, 0.05, kernel, 0.001, 0.0, k, oidx, od2, upload=False)


@pytest.mark.gpu
@pytest.mark.parametrize("kernel", FAMILIES, ids=[NAMES[k] for k in FAMILIES])
def test_one_pass_without_pairs(gpu_ctx, oracle, kernel):
    """K = 0 (radius 1e-6): every statistic 0, the scale is min_scale"""
    src, tgt = _few(0, 79)
    T = np.eye(4)
    k, oidx, od2 = oracle.k_nn_pass(src, tgt, T[:3, :].astype(np.float32), np.float32(1e-6 * 1e-6))
    assert k == 0
    for min_scale in (0.0, 0.25):
        st, info, _ = _check_pass(gpu_ctx, src, tgt, T, 1e-6, kernel, 0.0, min_scale, k, oidx, od2)
        assert not st.any() and info.scale == min_scale and info.zero_weight == 0 and info.robust_rmse == 0.0
        assert not gpu_ctx.pair_weights().any()


@pytest.mark.gpu
@pytest.mark.parametrize("min_scale", [0.0, 1e-3])
@pytest.mark.parametrize("kernel", FAMILIES, ids=[NAMES[k] for k in FAMILIES])
def test_cloud_against_itself(gpu_ctx, oracle, kernel, min_scale):
    """the source IS (part of) the target at T = I: every residual is 0, the automatic scale is min_scale (0: the
    c == 0 rule); every weight is exactly 1, no NaN anywhere, and the update is the identity"""
    rng = np.random.default_rng(78)
    _, tgt = _clouds(rng, 1, 3000)
    src = tgt[rng.permutation(3000)[:1500]].copy()
    T = np.eye(4)
    k, oidx, od2 = oracle.k_nn_pass(src, tgt, T[:3, :].astype(np.float32), np.float32(0.01))
    assert k == 1500 and not od2[oidx >= 0].any()
    st, info, _ = _check_pass(gpu_ctx, src, tgt, T, 0.1, kernel, 0.0, min_scale, k, oidx, od2)
    assert info.scale == min_scale and info.median_residual == 0.0
    assert np.array_equal(gpu_ctx.pair_weights(), np.ones(1500))
    assert st[0] == 1500.0 and st[1] == 0.0 and info.zero_weight == 0
    res = gpu_ctx.run_robust(None, 0.1, kernel, min_scale=min_scale, max_iter=3, rel_fitness=0.0, rel_rmse=0.0)
    assert res.iterations == 3 and res.num_correspondences == 1500 and np.isfinite(res.transformation_).all()
    assert np.abs(res.transformation_ - np.eye(4)).max() < 1e-12


@pytest.mark.gpu
@pytest.mark.parametrize("kernel", FAMILIES, ids=[NAMES[k] for k in FAMILIES])
def test_one_pass_ties_at_the_median(gpu_ctx, oracle, kernel):
    """duplicated source points: exact ties in d2 on both sides of the median's rank"""
    rng = np.random.default_rng(77)
    base, tgt = _clouds(rng, 50, 4000)
    src = np.repeat(base, 8, axis=0)[:396][rng.permutation(396)]          # 49 groups of 8 and one of 4
    T = np.eye(4)
    k, oidx, od2 = oracle.k_nn_pass(src, tgt, T[:3, :].astype(np.float32), np.float32(0.25))
    srt = np.sort(od2[oidx >= 0])
    m = (k + 1) // 2
    # rank 198 = 24 * 8 + 6 (or, the group of 4 before it, 23 * 8 + 4 + 10): inside a group of 8 either way
    assert k == 396 and m == 198 and srt[m - 2] == srt[m - 1] == srt[m]
    _check_pass(gpu_ctx, src, tgt, T, 0.5, kernel, 0.0, 0.0, k, oidx, od2)


@pytest.mark.gpu
def test_every_weight_zero(gpu_ctx, oracle):
    """a Tukey scale below every residual: sum w = 0, every solve is the identity, the run returns init, no error"""
    src, tgt, T, k, oidx, od2, _ = _spec_pass(oracle, 1000, 777, 0.3)
    st, info, _ = _check_pass(gpu_ctx, src, tgt, T, 0.3, TUKEY, 1e-9, 0.0, k, oidx, od2)
    assert k > 0 and not st.any() and info.zero_weight == k and info.weight_sum == 0.0 and info.robust_rmse == 0.0
    res = gpu_ctx.run_robust(T, 0.3, TUKEY, scale=1e-9, max_iter=4, rel_fitness=0.0, rel_rmse=0.0)
    assert res.iterations == 4 and res.num_correspondences == k
    assert np.array_equal(res.transformation_, T)
    assert res.robust.weight_sum == 0.0 and res.robust.zero_weight == k


# ---- 2. the full loop against a loop built from the reference ----
def _restated_weighted(p, q, w, a):
    """test_axis_solve.restated with weights: weighted means, the weighted angle in the plane normal to a"""
    from test_axis_solve import basis, rot
    a = a / np.linalg.norm(a)
    W = w.sum()
    pm, qm = (w[:, None] * p).sum(0) / W, (w[:, None] * q).sum(0) / W
    pc, qc = p - pm, q - qm
    u, v = basis(a)
    pu, pv, qu, qv = pc @ u, pc @ v, qc @ u, qc @ v
    th = np.arctan2((w * (pu * qv - pv * qu)).sum(), (w * (pu * qu + pv * qv)).sum())
    R = rot(a, th)
    T = np.eye(4)
    T[:3, :3] = R
    T[:3, 3] = qm - R @ pm
    return T


def ref_robust_loop(ref, oracle, src, tgt, r, kernel, iters, axis=None, normals=None):
    """RegistrationICP's loop (Registration.cpp:167-185, no stop test): the reference's pairs, the numpy weights over
    their f64 residuals (scale from their lower median), the solve from the weighted statistics."""
    T = np.eye(4)
    for it in range(iters + 1):
        idx = ref.evaluate_registration(src, tgt, r, T).idx
        v = idx >= 0
        if it == iters:
            break
        p = src @ T[:3, :3].T + T[:3, 3]
        q = np.zeros_like(p); q[v] = tgt[idx[v]]
        d = p - q
        n = None
        if normals is None:
            res = np.sqrt((d * d).sum(1))
        else:
            n = np.zeros_like(p); n[v] = normals[idx[v]]
            res = np.abs((d * n).sum(1))
        c = TUNE[kernel] * 1.4826 * lower_median(res[v])
        w = np.where(v, weights(kernel, res, c), 0.0)
        if axis is not None and normals is None:
            upd = _restated_weighted(p[v], q[v], w[v], axis)
        else:
            st = weighted_stats(p, q, n, w, v)
            upd = oracle.k_solve_gn(st)[1] if normals is not None else oracle.k_solve_kabsch(st)
        T = upd @ T
    return T, int(v.sum())


def _loop_case(lib, ref, oracle, src, tgt, r, kernel, axis=None, normals=None):
    T_ref, k_ref = ref_robust_loop(ref, oracle, src, tgt, r, kernel, 20, axis, normals)
    c = lib.Context(0)
    c.set_clouds_f64(src, tgt)
    if normals is not None:
        c.set_target_normals_f64(normals)
    if axis is not None:
        c.set_rotation_axis(axis)
    res = c.run_robust(None, r, kernel, plane=normals is not None, max_iter=20, rel_fitness=0.0, rel_rmse=0.0)
    c.close()
    err = synth.rel_frobenius(res.transformation_, T_ref)
    print("robust loop (%s) vs reference-built loop: rel. Frobenius %.3e (K %d / %d, scale %.6g, %d with w = 0)" %
          (NAMES[kernel], err, res.num_correspondences, k_ref, res.robust.scale, res.robust.zero_weight))
    assert res.iterations == 20
    assert res.num_correspondences == k_ref
    assert err < TOL_T
    return err


LOOP_KERNELS = pytest.mark.parametrize("kernel", [TUKEY, HUBER], ids=["tukey", "huber"])


@pytest.mark.gpu
@LOOP_KERNELS
def test_loop_against_reference_built_loop_5k(lib, ref, oracle, kernel):
    """Bound: the project's TOL_T = 1e-5 relative Frobenius, K equal.  (The library ranks the fp32 d2 of the pass for its
    median, the reference-built loop the f64 distances: the scales differ by a few 1e-8 relative.)
    Measured on the MI355X (Tukey / Huber, K equal in every case): 5 k -> 20 k 1.8e-12 /
    2.7e-12, the partial pair at 8 x its radius 7.2e-12 / 1.9e-10, with a rotation axis 7.6e-13 / 1.7e-12,
    point-to-plane 8.6e-11 / 4.7e-13."""
    src, tgt, _, _ = synth.make_pair(5000, 20000)
    _loop_case(lib, ref, oracle, src, tgt, 0.075, kernel)


@pytest.mark.gpu
@LOOP_KERNELS
def test_loop_against_reference_built_loop_partial_wide_radius(lib, ref, oracle, kernel):
    src, tgt, _, r = synth.make_partial_pair(20000, 80000, overlap=0.5)
    _loop_case(lib, ref, oracle, src, tgt, 8.0 * r, kernel)


@pytest.mark.gpu
@LOOP_KERNELS
def test_loop_against_reference_built_loop_rotation_axis(lib, ref, oracle, kernel):
    from test_axis_icp import yaw_pair, Y
    src, tgt, _ = yaw_pair(Y)
    _loop_case(lib, ref, oracle, src, tgt, synth.default_radius(len(tgt)), kernel, axis=Y)


@pytest.mark.gpu
@LOOP_KERNELS
def test_loop_against_reference_built_loop_point_to_plane(lib, ref, oracle, kernel):
    src, tgt, _, _ = synth.make_pair(5000, 20000)
    nrm = ref.estimate_normals(tgt)
    _loop_case(lib, ref, oracle, src, tgt, 0.075, kernel, normals=nrm)


# ---- 3. it does what it is for ----
@pytest.mark.gpu
def test_robust_weights_help_on_a_partial_scan_with_a_wide_radius(lib):
    """Relative Frobenius error to the true motion after 20 iterations from T = I at 8 x the radius.  A CPU experiment
    (numpy, KD-tree) gave plain 1.46e-1, Tukey 2.99e-3, Cauchy 6.2e-2, Huber 8.5e-2 (trimmed ICP told the true overlap:
    7.45e-3).  Tukey must end below a tenth of the plain run's error, Huber and Cauchy below it.
    Measured on the MI355X: plain 1.463e-1,
    Tukey 2.987e-3, Cauchy 6.223e-2, Huber 8.459e-2."""
    src, tgt, T_gt, r = synth.make_partial_pair(20000, 80000, overlap=0.5)
    c = lib.Context(0)
    c.set_clouds_f64(src, tgt)
    plain = c.run(None, 8.0 * r, 20, 0.0, 0.0)
    e = {"plain": synth.rel_frobenius(plain.transformation_, T_gt)}
    for k in FAMILIES:
        res = c.run_robust(None, 8.0 * r, k, max_iter=20, rel_fitness=0.0, rel_rmse=0.0)
        e[NAMES[k]] = synth.rel_frobenius(res.transformation_, T_gt)
    c.close()
    print("partial scan, 8 x radius, 20 iterations: plain %.3e, tukey %.3e, cauchy %.3e, huber %.3e" %
          (e["plain"], e["tukey"], e["cauchy"], e["huber"]))
    assert e["tukey"] < 0.1 * e["plain"]
    assert e["huber"] < e["plain"] and e["cauchy"] < e["plain"]


# ---- 4. context state ----
@pytest.mark.gpu
@pytest.mark.parametrize("plane", [False, True], ids=["point", "plane"])
def test_l2_is_the_plain_run(lib, plane):
    src, tgt, _, _ = synth.make_pair(5000, 20000)
    nrm = _unit_normals(np.random.default_rng(5), len(tgt))
    out = []
    for robust in (False, True):
        c = lib.Context(0)
        c.set_clouds_f64(src, tgt)
        if plane:
            c.set_target_normals_f64(nrm)
        if robust:
            res = c.run_robust(None, 0.075, L2, plane=plane, max_iter=20, rel_fitness=0.0, rel_rmse=0.0)
        else:
            res = c.run_point_to_plane(None, 0.075, 20, 0.0, 0.0) if plane else c.run(None, 0.075, 20, 0.0, 0.0)
        out.append((res, c.get_correspondences(), c.pair_weights() if robust else None))
        c.close()
    (a, ca, _), (b, cb, w) = out
    assert _same(a, b)
    for x, y in zip(ca, cb):
        assert np.array_equal(x, y)
    assert b.robust.weight_sum == b.num_correspondences == int(w.sum()) and b.robust.robust_rmse == b.inlier_rmse_


@pytest.mark.gpu
def test_context_state_consistent_after_a_robust_run(lib):
    """run, run_robust, run == run, run on a fresh context, at a size that takes the persistent launch"""
    s, t, _, r = synth.make_pair(131072, 1048576, motion="radius")
    out = []
    for with_call in (True, False):
        c = lib.Context(0)
        c.set_clouds_f64(s, t)
        a = c.run(None, r, 20, 0.0, 0.0)
        if with_call:
            c.run_robust(None, r, TUKEY, max_iter=5, rel_fitness=0.0, rel_rmse=0.0)
        b = c.run(None, r, 20, 0.0, 0.0)
        out.append((a, b, c.correspondence_index().copy()))
        c.close()
    assert _same(out[0][0], out[1][0]) and _same(out[0][1], out[1][1])
    assert np.array_equal(out[0][2], out[1][2])


@pytest.mark.gpu
@pytest.mark.parametrize("plane", [False, True], ids=["point", "plane"])
def test_two_robust_runs_are_bit_identical(lib, plane):
    src, tgt, _, r = synth.make_partial_pair(65536, 262144, overlap=0.5)
    nrm = _unit_normals(np.random.default_rng(6), len(tgt))
    out = []
    for _ in range(2):
        c = lib.Context(0)
        c.set_clouds_f64(src, tgt)
        if plane:
            c.set_target_normals_f64(nrm)
        res = c.run_robust(None, 4.0 * r, TUKEY, plane=plane, max_iter=10, rel_fitness=0.0, rel_rmse=0.0)
        out.append((res, c.pair_weights().copy()))
        c.close()
    (a, wa), (b, wb) = out
    assert _same(a, b) and np.array_equal(wa, wb) and _same_info(a.robust, b.robust)


def _pair_pass_outputs(c, T, radius, step):
    """one nn_pass + one trimmed or robust reduction -> every value it returns, as bit patterns"""
    kind, kw = step
    c.nn_pass(T, radius)
    if kind == "trimmed":
        st, info = c.reduce_trimmed(kw["keep"])
        fields = [float(info.kept), info.trimmed_rmse, info.d2_cut]
        per_src = c.kept_mask().astype(np.uint8)
    else:
        st, info = c.reduce_robust(kw["kernel"], scale=kw.get("scale", 0.0), plane=kw.get("plane", False))
        fields = [info.scale, info.median_residual, info.weight_sum, float(info.zero_weight), info.robust_rmse]
        per_src = c.pair_weights().view(np.uint64)
    return st.view(np.uint64).copy(), np.array(fields, np.float64).view(np.uint64), per_src.copy(), info


@pytest.mark.gpu
def test_trimmed_and_robust_passes_share_one_context(lib):
    """The trimmed and the robust pass work in ONE set of work words, partial rows and host granules per context.
    Passes of both kinds in turn on one context -- the early return that launches nothing and the reduction without a
    select among them -- must each return what the same call returns on a fresh context, bit for bit: statistics,
    info, kept mask, weights.  16,500 sources give 65 partial rows, the smallest count at which a thread of the fold
    takes a second trip.  (No keep alone makes m = 0 -- below 3 pairs m is min(K, 3) --, so the early return is
    reached with a radius that finds no pair; the smallest keep at the working radius, m = 3, runs as well.)"""
    rng = np.random.default_rng(165)
    src, tgt = _clouds(rng, 16500, 4096)
    nrm = _unit_normals(rng, len(tgt))
    T = _rand_T(rng, 0.1, 0.05)
    r, r_none = 0.15, 1e-6
    steps = [
        (("trimmed", dict(keep=0.5)), r),
        (("robust", dict(kernel=TUKEY, plane=True)), r),                    # automatic scale, point-to-plane
        (("trimmed", dict(keep=1e-6)), r),                                  # floor(keep * ns) = 0: m = 3
        (("trimmed", dict(keep=1e-6)), r_none),                             # K = 0, m = 0: nothing is launched
        (("robust", dict(kernel=HUBER, scale=r / 3.0)), r),                 # fixed scale, point-to-point
        (("robust", dict(kernel=TUKEY)), r_none),                           # K = 0: the reduction without the select
        (("trimmed", dict(keep=0.9)), r),
    ]

    def context():
        c = lib.Context(0)
        c.set_target(tgt)
        c.set_source(src)
        c.set_target_normals_f64(nrm)
        return c

    shared = context()
    for step, radius in steps:
        got = _pair_pass_outputs(shared, T, radius, step)
        fresh = context()
        want = _pair_pass_outputs(fresh, T, radius, step)
        fresh.close()
        for g, w in zip(got[:3], want[:3]):
            assert np.array_equal(g, w), (step, radius)
        info = got[3]
        if step[0] == "trimmed":                       # (the cases are what they claim to be)
            if radius == r_none:
                assert info.kept == 0
            elif step[1]["keep"] == 1e-6:
                assert info.kept == 3
            else:
                assert info.kept > 3
        else:
            assert (info.weight_sum > 0.0) == (radius == r)
    shared.close()


@pytest.mark.gpu
def test_sweep_equals_single_runs(lib):
    src, tgt, _, _ = synth.make_pair(5000, 20000)
    level, r = 4, 0.075
    c = lib.Context(0)
    c.set_clouds_f64(src, tgt)
    best, bl, per = c.run_yaw_sweep_robust(level, r, TUKEY, max_iter=10, rel_fitness=0.0, rel_rmse=0.0)
    c.close()
    c = lib.Context(0)
    c.set_clouds_f64(src, tgt)
    singles = []
    for i in range(level):
        a = 2.0 * math.pi / level * i
        init = np.eye(4)
        init[0, 0] = math.cos(a); init[0, 2] = math.sin(a); init[2, 0] = -math.sin(a); init[2, 2] = math.cos(a)
        singles.append(c.run_robust(init, r, TUKEY, max_iter=10, rel_fitness=0.0, rel_rmse=0.0))
    c.close()
    for x, y in zip(per, singles):
        assert _same(x, y) and _same_info(x.robust, y.robust)
    ks = [x.num_correspondences for x in singles]
    assert bl == int(np.argmax(ks))                     # the first with strictly the most
    assert _same(best, singles[bl]) and _same_info(best.robust, singles[bl].robust)


# ---- 5. the C++ shim ----
def _run_driver(binary, tmp_path, s, t, nrm, r, kernel, iters, level):
    inp, outp = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(inp, "wb") as f:
        f.write(struct.pack("<qqdiiii", len(s), len(t), r, kernel, iters, level, 0))
        f.write(np.ascontiguousarray(s, "<f8").tobytes())
        f.write(np.ascontiguousarray(t, "<f8").tobytes())
        f.write(np.ascontiguousarray(nrm, "<f8").tobytes())
    p = subprocess.run([binary, inp, outp], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, (p.returncode, p.stderr)
    raw = open(outp, "rb").read()
    out, off = [], 0
    for _ in range(3):                                   # RegistrationICP point / plane, RegisterModelToScene
        T = np.frombuffer(raw, "<f8", 16, off).reshape(4, 4); off += 128
        fit, rmse = struct.unpack_from("<dd", raw, off); off += 16
        (n,) = struct.unpack_from("<q", raw, off); off += 8
        corr = np.frombuffer(raw, "<i4", 2 * n, off).reshape(n, 2); off += 8 * n
        out.append((T, fit, rmse, corr))
    (both_refused,) = struct.unpack_from("<i", raw, off)
    return out, both_refused, p.stderr


@pytest.mark.gpu
def test_shim_driver_equals_the_c_abi(lib, driver_bins, tmp_path):
    src, tgt, _, _ = synth.make_partial_pair(5000, 20000, overlap=0.5)
    nrm = _unit_normals(np.random.default_rng(9), len(tgt))
    r, iters, level = 0.075, 10, 6
    c = lib.Context(0)
    c.set_clouds_f64(src, tgt)
    c.set_target_normals_f64(nrm)
    point = c.run_robust(None, r, TUKEY, max_iter=iters)            # the reference's default criteria, like the driver
    corr_point = np.stack(c.get_correspondences()[:2], 1)
    plane = c.run_robust(None, r, TUKEY, plane=True, max_iter=iters)
    corr_plane = np.stack(c.get_correspondences()[:2], 1)
    best, bl, per = c.run_yaw_sweep_robust(level, r, TUKEY, max_iter=30)
    at_best = c.run_robust(best.transformation_, r, TUKEY, max_iter=0)   # one pass at the winner: its pairs
    corr_best = np.stack(c.get_correspondences()[:2], 1)
    c.close()
    for b in driver_bins:
        ((T1, fit1, rmse1, corr1), (T2, fit2, rmse2, corr2), (T3, fit3, rmse3, corr3)), refused, err = \
            _run_driver(b, tmp_path, src, tgt, nrm, r, TUKEY, iters, level)
        assert np.array_equal(T1, point.transformation_) and fit1 == point.fitness_ and rmse1 == point.robust.robust_rmse, b
        assert np.array_equal(corr1, corr_point), b
        assert np.array_equal(T2, plane.transformation_) and fit2 == plane.fitness_ and rmse2 == plane.robust.robust_rmse, b
        assert np.array_equal(corr2, corr_plane), b
        assert np.array_equal(T3, best.transformation_), b
        assert fit3 == at_best.fitness_ and rmse3 == at_best.robust.robust_rmse, b
        assert np.array_equal(corr3, corr_best), b
        assert refused == 1 and "not both" in err, b     # robust weights together with keep < 1: message, empty result


@pytest.mark.gpu
def test_sharded_gpu_context_is_invalid(lib):
    """target-sharded HIP context: the median across ranks does not exist"""
    src, tgt, _, r = synth.make_pair(2000, 8000)
    c = lib.Context(0)
    c.set_target_shard(0, len(tgt), tgt.mean(0))
    c.set_clouds_f64(src, tgt)
    with pytest.raises(lib.IcpError) as e:
        c.run_robust(None, r, TUKEY, max_iter=5)
    assert e.value.code == INVALID
    c.close()
