"""Trimmed ICP (visma_amd/csrc/trim.hip; Chetverikov et al., ICPR 2002): per pass only the m pairs with the smallest
key (fp32 d2, source index) enter the solve, m = min(K, floor(keep * NS)), at least min(K, 3).

CPU: the symbols and methods exist, the argument checks, the C++ driver against the stand-alone headers, and the numpy
selection rule every GPU check below uses as its yardstick.
GPU: every oracle is assembled here from pieces that are not under test -- the committed kernel specification
(Oracle.k_nn_pass, k_reduce_stats), the compiled reference (Ref.evaluate_registration, compute_transformation) and
numpy's lexsort for the selection.
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
import build_trimmed  # noqa: E402

TOL_T = 1e-5       # north_star: final SE(3) within 1e-5 relative Frobenius of the CPU reference (test_gpu_kernels.py)
INVALID, STATE = 1, 5
KEEPS = [0.05, 1.0 / 3.0, 0.5, 0.9]


# ---------------------------------------------------------------------------
# the yardstick: the selection rule in numpy
# ---------------------------------------------------------------------------
def trim_count(K, NS, keep):
    """m = min(K, floor(keep * NS)); below 3: min(K, 3)"""
    m = min(K, int(math.floor(keep * float(NS))))
    if m < 3:
        m = min(K, 3)
    return m


def select(idx, d2, keep):
    """idx (NS,) target index or -1, d2 (NS,) ranking value -> (bool mask of the kept sources, m).
    Kept: the m pairs with the smallest (d2, source index)."""
    idx = np.asarray(idx)
    i = np.flatnonzero(idx >= 0)
    m = trim_count(len(i), len(idx), keep)
    order = np.lexsort((i, np.asarray(d2)[i]))[:m]
    mask = np.zeros(len(idx), bool)
    mask[i[order]] = True
    return mask, m


def test_selection_rule_count():
    assert trim_count(1000, 2000, 0.5) == 1000           # min(K, .) binds exactly
    assert trim_count(900, 2000, 0.5) == 900             # K below the share: every pair
    assert trim_count(1500, 2000, 0.5) == 1000
    assert trim_count(1500, 2000, 1.0) == 1500           # keep = 1: m = K
    assert trim_count(1500, 2001, 1.0 / 3.0) == 667      # floor
    assert trim_count(100, 10, 0.05) == 3                # floor(keep * NS) = 0 -> 3
    assert trim_count(2, 10, 0.05) == 2 and trim_count(1, 10, 0.05) == 1 and trim_count(0, 10, 0.05) == 0
    assert trim_count(50, 40, 0.06) == 3                 # floor = 2 < 3 -> 3
    assert trim_count(0, 1000, 0.5) == 0


def test_selection_rule_ties_by_index():
    idx = np.array([5, -1, 7, 7, 2, 9, -1, 4], np.int32)
    d2 = np.array([0.5, 0.0, 0.25, 0.25, 0.25, 0.1, 0.0, 0.25], np.float32)
    # pairs by (d2, i): (0.1, 5) (0.25, 2) (0.25, 3) (0.25, 4) (0.25, 7) (0.5, 0); NS = 8
    mask, m = select(idx, d2, 0.5)                       # m = 4: the tie at 0.25 is cut after source 4
    assert m == 4 and list(np.flatnonzero(mask)) == [2, 3, 4, 5]
    mask, m = select(idx, d2, 0.4)                       # floor(3.2) = 3
    assert m == 3 and list(np.flatnonzero(mask)) == [2, 3, 5]
    mask, m = select(idx, d2, 1.0)
    assert m == 6 and list(np.flatnonzero(mask)) == [0, 2, 3, 4, 5, 7]
    mask, m = select(idx, d2, 0.01)                      # floor = 0 -> 3
    assert m == 3 and list(np.flatnonzero(mask)) == [2, 3, 5]
    assert not select(np.full(4, -1), np.zeros(4), 0.5)[0].any()


# ---------------------------------------------------------------------------
# CPU: interface
# ---------------------------------------------------------------------------
NEW_SYMBOLS = ["visma_icp_reduce_trimmed", "visma_icp_run_trimmed", "visma_icp_run_yaw_sweep_trimmed", "visma_icp_get_kept_mask"]


def test_symbols_and_methods(lib):
    L = lib.load()
    for name in NEW_SYMBOLS:
        assert hasattr(L, name), name
    for name in ["reduce_trimmed", "run_trimmed", "run_yaw_sweep_trimmed", "kept_mask"]:
        assert callable(getattr(lib.Context, name, None)), name


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


@pytest.mark.parametrize("keep", [0.0, -0.5, 1.5, float("nan"), float("inf"), float("-inf")])
def test_bad_keep_is_invalid_before_any_pass(lib, hctx, keep):
    src, tgt = _small_clouds()
    hctx.set_target(tgt); hctx.set_source(src)
    hctx.nn_pass(np.eye(4), 0.1)
    calls = dict(hctx.engine.calls)
    for call in (lambda: hctx.run_trimmed(None, 0.1, keep, 5), lambda: hctx.reduce_trimmed(keep),
                 lambda: hctx.run_yaw_sweep_trimmed(4, 0.1, keep, 5)):
        with pytest.raises(lib.IcpError) as e:
            call()
        assert e.value.code == INVALID
    assert hctx.engine.calls == calls                    # nothing was launched


def test_null_outputs_and_missing_clouds(lib, hctx):
    import ctypes as C
    L, h = hctx.L, hctx._h
    init = np.eye(4).reshape(16)
    dp = C.POINTER(C.c_double)
    res, info, st = lib.CResult(), lib.CTrimInfo(), np.zeros(38)
    # a context without clouds
    assert L.visma_icp_run_trimmed(h, init.ctypes.data_as(dp), 0.1, 0.5, 5, 0.0, 0.0, 0, 0, C.byref(res), C.byref(info)) == STATE
    assert L.visma_icp_reduce_trimmed(h, 0.5, st.ctypes.data_as(dp), C.byref(info)) == STATE
    assert L.visma_icp_get_kept_mask(h, (C.c_uint8 * 4)()) == STATE
    src, tgt = _small_clouds()
    hctx.set_target(tgt); hctx.set_source(src)
    # NULL result / init / statistics / info / mask
    assert L.visma_icp_run_trimmed(h, init.ctypes.data_as(dp), 0.1, 0.5, 5, 0.0, 0.0, 0, 0, None, C.byref(info)) == INVALID
    assert L.visma_icp_run_trimmed(h, None, 0.1, 0.5, 5, 0.0, 0.0, 0, 0, C.byref(res), C.byref(info)) == INVALID
    assert L.visma_icp_reduce_trimmed(h, 0.5, None, C.byref(info)) == INVALID
    assert L.visma_icp_reduce_trimmed(h, 0.5, st.ctypes.data_as(dp), None) == INVALID
    assert L.visma_icp_get_kept_mask(h, None) == INVALID
    assert L.visma_icp_run_yaw_sweep_trimmed(h, 4, 0.1, 0.5, 5, 0.0, 0.0, 0, None, None, None, None, None) == INVALID
    assert L.visma_icp_run_yaw_sweep_trimmed(h, 0, 0.1, 0.5, 5, 0.0, 0.0, 0, C.byref(res), None, None, None, None) == INVALID
    # Gauss-Newton point-to-point solvers are not offered trimmed; negative iteration count
    assert L.visma_icp_run_trimmed(h, init.ctypes.data_as(dp), 0.1, 0.5, 5, 0.0, 0.0, 1, 0, C.byref(res), C.byref(info)) == INVALID
    assert L.visma_icp_run_trimmed(h, init.ctypes.data_as(dp), 0.1, 0.5, -1, 0.0, 0.0, 0, 0, C.byref(res), C.byref(info)) == INVALID
    assert L.visma_icp_run_trimmed(None, init.ctypes.data_as(dp), 0.1, 0.5, 5, 0.0, 0.0, 0, 0, C.byref(res), C.byref(info)) == INVALID


def test_oracle_engine_reports_not_supported(lib, hctx):
    src, tgt = _small_clouds()
    hctx.set_target(tgt); hctx.set_source(src)
    hctx.nn_pass(np.eye(4), 0.1)
    with pytest.raises(lib.IcpError) as e:
        hctx.reduce_trimmed(0.5)
    assert e.value.code == STATE and "not supported" in str(e.value)
    with pytest.raises(lib.IcpError) as e:
        hctx.run_trimmed(None, 0.1, 0.5, 5)
    assert e.value.code == STATE and "not supported" in str(e.value)
    # keep = 1 is the plain run on every engine
    a = hctx.run_trimmed(None, 0.1, 1.0, 5, 0.0, 0.0)
    b = hctx.run(None, 0.1, 5, 0.0, 0.0)
    assert np.array_equal(a.transformation_, b.transformation_) and a.trim.kept == a.num_correspondences == b.num_correspondences
    assert hctx.kept_mask().sum() == a.num_correspondences


def test_sharded_context_is_invalid(lib, hctx):
    src, tgt = _small_clouds()
    hctx.set_target(tgt); hctx.set_source(src)
    fn = lib.ALLREDUCE_FN(lambda user, buf, n: 0)
    hctx._keep.append(fn)
    assert hctx.L.visma_icp_set_allreduce(hctx._h, fn, None, 0, 2) == 0
    with pytest.raises(lib.IcpError) as e:
        hctx.run_trimmed(None, 0.1, 0.5, 5)
    assert e.value.code == INVALID


@pytest.fixture(scope="module")
def driver_bins(lib):
    if build_shim.eigen_dir() is not None:
        build_trimmed.build()
    paths = [os.path.join(HERE, "cpp", "_build", b) for b in build_trimmed.BINS]
    if not all(os.path.exists(p) for p in paths):
        pytest.skip("trimmed driver not prebuilt and no Eigen headers here")
    return paths


def test_cpp_driver_compiles_against_standalone_headers(driver_bins):
    """Both Eigen storage orders: the estimator goes through the stock open3d::RegistrationICP without Open3D."""
    for b in driver_bins:
        assert os.path.getsize(b) > 0 and os.access(b, os.X_OK)
    src = open(os.path.join(HERE, "cpp", "trimmed_driver.cpp")).read()
    assert "cicp::TransformationEstimationPointToPointTrimmed" in src and "cicp::RegisterModelToScene" in src


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


def _same(a, b):
    return (np.array_equal(a.transformation_, b.transformation_) and a.num_correspondences == b.num_correspondences and
            a.fitness_ == b.fitness_ and a.inlier_rmse_ == b.inlier_rmse_ and a.iterations == b.iterations)


def _bits(x):
    return np.float32(x).view(np.uint32)


# ---- 1. keep = 1 is today's result ----
def _keep_one(lib, src, tgt, r):
    out = []
    for trimmed in (False, True):
        c = lib.Context(0)
        c.set_clouds_f64(src, tgt)
        res = c.run_trimmed(None, r, 1.0, 20, 0.0, 0.0) if trimmed else c.run(None, r, 20, 0.0, 0.0)
        out.append((res, c.get_correspondences(), c.kept_mask() if trimmed else None))
        c.close()
    (a, ca, _), (b, cb, mask) = out
    assert _same(a, b)
    for x, y in zip(ca, cb):
        assert np.array_equal(x, y)
    assert b.trim.kept == b.num_correspondences == int(mask.sum())
    assert b.trim.trimmed_rmse == b.inlier_rmse_
    assert _bits(b.trim.d2_cut) == _bits(cb[2].max())


@pytest.mark.gpu
def test_keep_one_is_the_plain_run_5k(lib):
    s, t, _, r = synth.make_pair(5000, 20000)
    _keep_one(lib, s, t, 0.075)


@pytest.mark.gpu
def test_keep_one_is_the_plain_run_partial_65k(lib):
    s, t, _, r = synth.make_partial_pair(65536, 262144)
    _keep_one(lib, s, t, r)


@pytest.mark.gpu
@pytest.mark.timeout(900)
def test_keep_one_is_the_plain_run_c4(lib):
    s, t, _, r = synth.make_pair(262144, 4194304, motion="radius")
    _keep_one(lib, s, t, r)


# ---- 2. one pass, exact and independent (fp32 uploads, the kernel specification as the oracle) ----
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
        _spec_cache[key] = (src, tgt, T, k, oidx, od2)
    return _spec_cache[key]


def _check_pass(ctx, oracle, src, tgt, T, radius, keep, k, oidx, od2):
    ctx.set_target(tgt)
    ctx.set_source(src)
    ctx.nn_pass(T, radius)
    st, info = ctx.reduce_trimmed(keep)
    mask = ctx.kept_mask()
    omask, m = select(oidx, od2, keep)
    assert info.kept == m == int(round(st[0]))
    assert np.array_equal(mask, omask)
    assert _bits(info.d2_cut) == _bits(od2[omask].max() if m else 0.0)
    ost = oracle.k_reduce_stats(src, tgt, np.where(omask, oidx, -1).astype(np.int32), T[:3, :])
    scale = np.maximum(np.abs(ost), 1.0)
    err = np.max(np.abs(st - ost) / scale)
    print("trimmed statistics vs specification: %.3e (m = %d of K = %d)" % (err, m, k))
    assert err < 1e-9
    # all K pairs are still what get_correspondences returns
    si, ti, d2 = ctx.get_correspondences()
    assert len(si) == k and np.array_equal(ti, oidx[oidx >= 0])
    if m:
        assert info.trimmed_rmse == math.sqrt(st[1] / st[0])
    return st, info


@pytest.mark.gpu
@pytest.mark.parametrize("keep", KEEPS, ids=["0.05", "third", "0.5", "0.9"])
@pytest.mark.parametrize("ns,nt,radius", SHAPES)
def test_one_pass_against_the_kernel_specification(gpu_ctx, oracle, ns, nt, radius, keep):
    src, tgt, T, k, oidx, od2 = _spec_pass(oracle, ns, nt, radius)
    _check_pass(gpu_ctx, oracle, src, tgt, T, radius, keep, k, oidx, od2)


@pytest.mark.gpu
def test_one_pass_distance_ties_straddle_the_cut(gpu_ctx, oracle):
    """duplicated source points: exact ties in d2; the lower SOURCE index is kept, wherever the engine stores the point"""
    rng = np.random.default_rng(77)
    base, tgt = _clouds(rng, 50, 4000)
    src = np.repeat(base, 8, axis=0)[rng.permutation(400)]
    radius = 0.5
    T = np.eye(4)
    k, oidx, od2 = oracle.k_nn_pass(src, tgt, T[:3, :].astype(np.float32), np.float32(radius * radius))
    keep = 0.51                                          # m = 204 = 25 groups of 8 + 4
    i = np.flatnonzero(oidx >= 0)
    m = trim_count(len(i), len(src), keep)
    srt = np.sort(od2[i])
    assert k == 400 and m == 204 and srt[m - 1] == srt[m]          # the tie does straddle the cut
    _check_pass(gpu_ctx, oracle, src, tgt, T, radius, keep, k, oidx, od2)


@pytest.mark.gpu
def test_one_pass_everything_tied(gpu_ctx, oracle):
    """the source IS (part of) the target: every d2 is 0, the cut is decided by the source index alone"""
    rng = np.random.default_rng(78)
    _, tgt = _clouds(rng, 1, 3000)
    src = tgt[rng.permutation(3000)[:1500]].copy()
    T = np.eye(4)
    k, oidx, od2 = oracle.k_nn_pass(src, tgt, T[:3, :].astype(np.float32), np.float32(0.01))
    assert k == 1500 and not od2[oidx >= 0].any()
    _check_pass(gpu_ctx, oracle, src, tgt, T, 0.1, 0.5, k, oidx, od2)


@pytest.mark.gpu
@pytest.mark.parametrize("near", [0, 1, 2])
def test_one_pass_with_few_pairs(gpu_ctx, oracle, near):
    """K = 0, 1, 2: m = K"""
    rng = np.random.default_rng(79 + near)
    _, tgt = _clouds(rng, 1, 2000)
    src = (rng.random((300, 3)).astype(np.float32) + 50.0).astype(np.float32)
    src[:near] = tgt[:near] + np.float32(0.001)
    src = src[rng.permutation(300)]
    T = np.eye(4)
    k, oidx, od2 = oracle.k_nn_pass(src, tgt, T[:3, :].astype(np.float32), np.float32(0.05 * 0.05))
    assert k == near
    st, info = _check_pass(gpu_ctx, oracle, src, tgt, T, 0.05, 0.5, k, oidx, od2)
    assert info.kept == near
    if near == 0:
        assert not st.any() and info.d2_cut == 0.0 and info.trimmed_rmse == 0.0


@pytest.mark.gpu
def test_one_pass_share_rounds_to_zero(gpu_ctx, oracle):
    """floor(keep * NS) = 0: three pairs are kept"""
    rng = np.random.default_rng(83)
    src, tgt = _clouds(rng, 10, 5000, spread=0.3)
    T = np.eye(4)
    k, oidx, od2 = oracle.k_nn_pass(src, tgt, T[:3, :].astype(np.float32), np.float32(0.25))
    assert k == 10
    _, info = _check_pass(gpu_ctx, oracle, src, tgt, T, 0.5, 0.05, k, oidx, od2)
    assert info.kept == 3


# ---- 3. one pass, f64 uploads ----
def _pairs_f64():
    return {
        "pair": lambda: synth.make_pair(5000, 20000),
        "partial": lambda: synth.make_partial_pair(20000, 80000, overlap=0.5),
        "offset_3m": lambda: synth.make_pair(5000, 20000, offset=[3.0, 0.0, 0.0]),
    }


@pytest.mark.gpu
@pytest.mark.parametrize("at", ["identity", "T_gt"])
@pytest.mark.parametrize("keep", [0.5, 0.9])
@pytest.mark.parametrize("name", ["pair", "partial", "offset_3m"])
def test_one_pass_f64_uploads(lib, ref, name, keep, at):
    src, tgt, T_gt, r = _pairs_f64()[name]()
    T = np.eye(4) if at == "identity" else T_gt
    c = lib.Context(0)
    c.set_clouds_f64(src, tgt)
    c.nn_pass(T, r)
    st, info = c.reduce_trimmed(keep)
    mask = c.kept_mask()
    si, ti, d2 = c.get_correspondences()
    c.close()
    # (a) against the (d2, i) the library itself reports
    idx = np.full(len(src), -1, np.int32); idx[si] = ti
    dd = np.zeros(len(src), np.float32); dd[si] = d2
    omask, m = select(idx, dd, keep)
    assert info.kept == m == int(round(st[0])) and np.array_equal(mask, omask)
    assert _bits(info.d2_cut) == _bits(dd[omask].max())
    # (b) against the reference's pairs and their f64 distances
    rr = ref.evaluate_registration(src, tgt, r, T)
    assert np.array_equal(rr.idx, idx)
    p = src @ T[:3, :3].T + T[:3, 3]
    d64 = np.zeros(len(src))
    v = rr.idx >= 0
    d64[v] = ((p[v] - tgt[rr.idx[v]]) ** 2).sum(1)
    rmask, rm = select(rr.idx, d64, keep)
    assert rm == m
    cut = np.sqrt(np.sort(d64[v])[m - 1])                 # the reference's cut, as a distance
    # the header of visma_icp_set_search_precision: a distance is off by at most 2.4e-7 (|p|_1 + r) + 4.8e-7 r
    # (p in the frame the library searches in: both clouds shifted by the target centroid on upload)
    pc = np.abs(p - tgt.mean(0)).sum(1)
    band = 2.4e-7 * (pc + r) + 4.8e-7 * r
    inside = v & (np.abs(np.sqrt(d64) - cut) <= band)
    differ = mask != rmask
    print("%s keep %.2f at %s: %d pairs differ from the f64 selection, %d reference pairs inside the band" %
          (name, keep, at, int(differ.sum()), int(inside.sum())))
    assert not (differ & ~inside).any()
    assert differ.sum() <= inside.sum()


# ---- 4. the full loop against a loop built from the reference ----
def ref_trimmed_loop(ref, src, tgt, r, keep, iters, solve):
    """RegistrationICP's loop (Registration.cpp:167-185, no stop test): the reference's pairs, numpy's selection over
    their f64 distances, solve(p, tgt, corr) -> update."""
    T = np.eye(4)
    for it in range(iters + 1):
        idx = ref.evaluate_registration(src, tgt, r, T).idx
        p = src @ T[:3, :3].T + T[:3, 3]
        v = idx >= 0
        d = np.zeros(len(src))
        d[v] = ((p[v] - tgt[idx[v]]) ** 2).sum(1)
        mask, m = select(idx, d, keep)
        if it == iters:
            break
        i = np.flatnonzero(mask)
        T = solve(p, tgt, np.stack([i, idx[i]], 1).astype(np.int32)) @ T
    return T, int(v.sum()), m


def _loop_case(lib, ref, src, tgt, r, keep, axis=None):
    if axis is None:
        def solve(p, t, corr):
            return ref.compute_transformation(p, t, corr)
    else:
        from test_axis_solve import restated

        def solve(p, t, corr):
            return restated(p[corr[:, 0]], t[corr[:, 1]], axis)[0]
    T_ref, k_ref, m_ref = ref_trimmed_loop(ref, src, tgt, r, keep, 20, solve)
    c = lib.Context(0)
    c.set_clouds_f64(src, tgt)
    if axis is not None:
        c.set_rotation_axis(axis)
    res = c.run_trimmed(None, r, keep, 20, 0.0, 0.0)
    c.close()
    err = synth.rel_frobenius(res.transformation_, T_ref)
    print("trimmed loop vs reference-built loop: rel. Frobenius %.3e (K %d / %d, m %d / %d)" %
          (err, res.num_correspondences, k_ref, res.trim.kept, m_ref))
    assert res.iterations == 20
    assert res.num_correspondences == k_ref and res.trim.kept == m_ref
    assert err < TOL_T
    return err


@pytest.mark.gpu
@pytest.mark.parametrize("keep", [0.5, 0.7])
def test_loop_against_reference_built_loop_5k(lib, ref, keep):
    """Measured on the MI355X (relative Frobenius to the reference-built loop, K and m equal in every case):
    5 k -> 20 k 2.2e-15 / 2.4e-15 (keep 0.5 / 0.7), the partial pair at 8 x its radius 1.4e-15 / 1.6e-15, with a
    rotation axis 4.4e-16 / 9.3e-16."""
    src, tgt, _, _ = synth.make_pair(5000, 20000)
    _loop_case(lib, ref, src, tgt, 0.075, keep)


@pytest.mark.gpu
@pytest.mark.parametrize("keep", [0.5, 0.7])
def test_loop_against_reference_built_loop_partial_wide_radius(lib, ref, keep):
    src, tgt, _, r = synth.make_partial_pair(20000, 80000, overlap=0.5)
    _loop_case(lib, ref, src, tgt, 8.0 * r, keep)


@pytest.mark.gpu
@pytest.mark.parametrize("keep", [0.5, 0.7])
def test_loop_against_reference_built_loop_rotation_axis(lib, ref, keep):
    from test_axis_icp import yaw_pair, Y, upright_err
    src, tgt, _ = yaw_pair(Y)
    _loop_case(lib, ref, src, tgt, synth.default_radius(len(tgt)), keep, axis=Y)


# ---- 5. it does what it is for ----
@pytest.mark.gpu
def test_trimming_helps_on_a_partial_scan_with_a_wide_radius(lib):
    src, tgt, T_gt, r = synth.make_partial_pair(20000, 80000, overlap=0.5)
    c = lib.Context(0)
    c.set_clouds_f64(src, tgt)
    plain = c.run(None, 8.0 * r, 20, 0.0, 0.0)
    trimmed = c.run_trimmed(None, 8.0 * r, 0.5, 20, 0.0, 0.0)
    c.close()
    e_plain = synth.rel_frobenius(plain.transformation_, T_gt)
    e_trim = synth.rel_frobenius(trimmed.transformation_, T_gt)
    print("partial scan, 8 x radius, 20 iterations: plain %.3e, trimmed (keep 0.5) %.3e" % (e_plain, e_trim))
    assert e_trim < e_plain


# ---- 6. context state ----
@pytest.mark.gpu
def test_context_state_consistent_after_a_trimmed_run(lib):
    """run, run_trimmed, run == run, run on a fresh context, at a size that takes the persistent launch"""
    s, t, _, r = synth.make_pair(131072, 1048576, motion="radius")
    out = []
    for with_call in (True, False):
        c = lib.Context(0)
        c.set_clouds_f64(s, t)
        a = c.run(None, r, 20, 0.0, 0.0)
        if with_call:
            c.run_trimmed(None, r, 0.7, 5, 0.0, 0.0)
        b = c.run(None, r, 20, 0.0, 0.0)
        out.append((a, b, c.correspondence_index().copy()))
        c.close()
    assert _same(out[0][0], out[1][0]) and _same(out[0][1], out[1][1])
    assert np.array_equal(out[0][2], out[1][2])


# ---- 7. sweep ----
@pytest.mark.gpu
def test_sweep_equals_single_runs(lib):
    src, tgt, _, _ = synth.make_pair(5000, 20000)
    level, r, keep = 24, 0.075, 0.6
    c = lib.Context(0)
    c.set_clouds_f64(src, tgt)
    best, bl, per = c.run_yaw_sweep_trimmed(level, r, keep, 10, 0.0, 0.0)
    c.close()
    c = lib.Context(0)
    c.set_clouds_f64(src, tgt)
    singles = []
    for i in range(level):
        a = 2.0 * math.pi / level * i
        init = np.eye(4)
        init[0, 0] = math.cos(a); init[0, 2] = math.sin(a); init[2, 0] = -math.sin(a); init[2, 2] = math.cos(a)
        singles.append(c.run_trimmed(init, r, keep, 10, 0.0, 0.0))
    c.close()
    for x, y in zip(per, singles):
        assert _same(x, y) and x.trim.kept == y.trim.kept and x.trim.trimmed_rmse == y.trim.trimmed_rmse and x.trim.d2_cut == y.trim.d2_cut
    ks = [x.num_correspondences for x in singles]
    assert bl == int(np.argmax(ks))                     # the first with strictly the most
    assert _same(best, singles[bl]) and best.trim.kept == singles[bl].trim.kept


# ---- 8. the C++ shim ----
def _run_driver(binary, tmp_path, s, t, r, keep, iters, level):
    inp, outp = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(inp, "wb") as f:
        f.write(struct.pack("<qqddii", len(s), len(t), r, keep, iters, level))
        f.write(np.ascontiguousarray(s, "<f8").tobytes())
        f.write(np.ascontiguousarray(t, "<f8").tobytes())
    p = subprocess.run([binary, inp, outp], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, (p.returncode, p.stderr)
    raw = open(outp, "rb").read()
    out, off = [], 0
    for _ in range(2):                                   # RegistrationICP, RegisterModelToScene
        T = np.frombuffer(raw, "<f8", 16, off).reshape(4, 4); off += 128
        fit, rmse = struct.unpack_from("<dd", raw, off); off += 16
        (n,) = struct.unpack_from("<q", raw, off); off += 8
        corr = np.frombuffer(raw, "<i4", 2 * n, off).reshape(n, 2); off += 8 * n
        out.append((T, fit, rmse, corr))
    (solve_diff,) = struct.unpack_from("<d", raw, off)
    return out, solve_diff


@pytest.mark.gpu
def test_shim_driver_equals_the_c_abi(lib, driver_bins, tmp_path):
    src, tgt, _, _ = synth.make_partial_pair(5000, 20000, overlap=0.5)
    r, keep, iters, level = 0.075, 0.5, 10, 6
    c = lib.Context(0)
    c.set_clouds_f64(src, tgt)
    res = c.run_trimmed(None, r, keep, iters)            # the reference's default criteria, like the driver
    mask = c.kept_mask()
    idx = c.correspondence_index()
    i = np.flatnonzero(mask)
    kept_pairs = np.stack([i, idx[i]], 1)
    best, bl, per = c.run_yaw_sweep_trimmed(level, r, keep, 30)
    init = best.transformation_
    at_best = c.run_trimmed(init, r, keep, 0)            # one pass at the winner: its kept pairs
    mask_b = c.kept_mask()
    idx_b = c.correspondence_index()
    c.close()
    ib = np.flatnonzero(mask_b)
    for b in driver_bins:
        ((T1, fit1, rmse1, corr1), (T2, fit2, rmse2, corr2)), solve_diff = _run_driver(b, tmp_path, src, tgt, r, keep, iters, level)
        assert np.array_equal(T1, res.transformation_) and fit1 == res.fitness_ and rmse1 == res.trim.trimmed_rmse, b
        assert np.array_equal(corr1, kept_pairs), b      # the KEPT set, sorted by source index
        assert len(corr1) == res.trim.kept
        assert np.array_equal(T2, best.transformation_), b
        assert fit2 == at_best.fitness_ and rmse2 == at_best.trim.trimmed_rmse, b
        assert np.array_equal(corr2, np.stack([ib, idx_b[ib]], 1)), b
        assert solve_diff == 0.0, b                      # its host ComputeTransformation solves over what it is given


# ---- 9. determinism ----
@pytest.mark.gpu
def test_two_trimmed_runs_are_bit_identical(lib):
    src, tgt, _, r = synth.make_partial_pair(65536, 262144, overlap=0.5)
    out = []
    for _ in range(2):
        c = lib.Context(0)
        c.set_clouds_f64(src, tgt)
        res = c.run_trimmed(None, 4.0 * r, 0.5, 20, 0.0, 0.0)
        out.append((res, c.kept_mask().copy()))
        c.close()
    (a, ma), (b, mb) = out
    assert _same(a, b) and np.array_equal(ma, mb)
    assert a.trim.kept == b.trim.kept and a.trim.trimmed_rmse == b.trim.trimmed_rmse and a.trim.d2_cut == b.trim.d2_cut


@pytest.mark.gpu
def test_sharded_gpu_context_is_invalid(lib):
    """target-sharded HIP context: the order statistic across ranks does not exist"""
    src, tgt, _, r = synth.make_pair(2000, 8000)
    c = lib.Context(0)
    c.set_target_shard(0, len(tgt), tgt.mean(0))
    c.set_clouds_f64(src, tgt)
    with pytest.raises(lib.IcpError) as e:
        c.run_trimmed(None, r, 0.5, 5)
    assert e.value.code == INVALID
    c.close()
