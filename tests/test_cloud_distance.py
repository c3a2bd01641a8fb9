"""Exact, unbounded cloud-to-cloud and nearest-neighbour distances (visma_amd/csrc/cloud_distance.hip):
open3d::ComputePointCloudToPointCloudDistance (O3D/Core/Geometry/PointCloud.cpp:122-142) and
ComputePointCloudNearestNeighborDistance (:200-219).

CPU: the C ABI's symbols and argument checks, and the C++ driver built against the stand-alone header set.
GPU: every result against the compiled reference (Ref.nn_distance) or an exhaustive restatement in flann's
arithmetic, bit for bit; the pruning's worst cases under a time limit; NaN rows; the context's ICP state untouched;
the shim's four entry points against the C ABI.
"""
import ctypes
import os
import struct
import subprocess
import sys
import time

import numpy as np
import pytest

from oracle_engine import OracleEngine
from visma_amd import synth

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "cpp"))
import build_cloud_distance  # noqa: E402
import build_shim  # noqa: E402

INVALID = 1
INT32_MAX = 2**31 - 1


def flann_nn(q, t, exclude_self=False, rows=None, chunk=8):
    """sqrt(min_j ((dx*dx + dy*dy) + dz*dz)) in f64 -- flann's L2<double> -- by exhaustive search.  `rows`: the
    query rows to answer (default all); exclude_self: q is t and row i skips column i."""
    q = np.asarray(q, np.float64); t = np.asarray(t, np.float64)
    rows = np.arange(len(q)) if rows is None else np.asarray(rows)
    out = np.empty(len(rows))
    for s in range(0, len(rows), chunk):
        r = rows[s:s + chunk]
        a = q[r]
        dx = a[:, None, 0] - t[None, :, 0]
        dy = a[:, None, 1] - t[None, :, 1]
        dz = a[:, None, 2] - t[None, :, 2]
        d2 = (dx * dx + dy * dy) + dz * dz
        if exclude_self:
            d2[np.arange(len(r)), r] = np.inf
        out[s:s + len(r)] = np.sqrt(d2.min(1))
    return out


# ---------------------------------------------------------------------------
# CPU
# ---------------------------------------------------------------------------
@pytest.fixture()
def hctx(lib, oracle):
    """A context on the oracle engine: the argument checks run, no call reaches a device."""
    ctx = OracleEngine(oracle).context()
    yield ctx
    ctx.close()


def test_abi_exports_both_distance_calls(lib):
    L = ctypes.CDLL(lib.LIB_PATH)
    assert hasattr(L, "visma_icp_point_cloud_distance")
    assert hasattr(L, "visma_icp_nearest_neighbor_distance")
    ctx = lib.Context
    assert hasattr(ctx, "point_cloud_distance") and hasattr(ctx, "nearest_neighbor_distance")


def test_argument_checks_without_a_device(lib, hctx):
    L, h = hctx.L, hctx._h
    dp = ctypes.POINTER(ctypes.c_double)
    p = np.zeros((4, 3)); d = np.zeros(4)
    P, D = p.ctypes.data_as(dp), d.ctypes.data_as(dp)
    pcd, nnd = L.visma_icp_point_cloud_distance, L.visma_icp_nearest_neighbor_distance
    # NULL context
    assert pcd(None, P, 4, P, 4, D) == INVALID
    assert nnd(None, P, 4, D) == INVALID
    # negative counts
    assert pcd(h, P, -1, P, 4, D) == INVALID
    assert pcd(h, P, 4, P, -1, D) == INVALID
    assert nnd(h, P, -1, D) == INVALID
    # a NULL array with a positive count
    assert pcd(h, None, 4, P, 4, D) == INVALID
    assert pcd(h, P, 4, None, 4, D) == INVALID
    assert pcd(h, P, 4, P, 4, None) == INVALID
    assert nnd(h, None, 4, D) == INVALID
    assert nnd(h, P, 4, None) == INVALID
    # more than 2^31 - 1 points per cloud (checked before anything is read)
    assert pcd(h, P, INT32_MAX + 1, P, 4, D) == INVALID
    assert pcd(h, P, 4, P, INT32_MAX + 1, D) == INVALID
    assert nnd(h, P, INT32_MAX + 1, D) == INVALID
    # an empty source (or cloud) is nothing to do, whatever the engine; NULL arrays allowed at count 0
    assert pcd(h, None, 0, None, 0, None) == 0
    assert pcd(h, None, 0, P, 4, None) == 0
    assert nnd(h, None, 0, None) == 0


@pytest.fixture(scope="module")
def driver_bins(lib):
    if build_shim.eigen_dir() is not None:
        build_cloud_distance.build()
    paths = [os.path.join(HERE, "cpp", "_build", b) for b in build_cloud_distance.BINS]
    if not all(os.path.exists(p) for p in paths):
        pytest.skip("cloud distance driver not prebuilt and no Eigen headers here")
    return paths


def test_driver_compiles_against_the_standalone_headers(driver_bins):
    """Both Eigen storage orders: a caller of the stock names and of open3d::cicp:: builds without Open3D."""
    for b in driver_bins:
        assert os.path.getsize(b) > 0 and os.access(b, os.X_OK)
    src = open(os.path.join(HERE, "cpp", "cloud_distance_driver.cpp")).read()
    for name in ("cicp::ComputePointCloudToPointCloudDistance", "cicp::ComputePointCloudNearestNeighborDistance"):
        assert name in src


# ---------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ctx(lib):
    c = lib.Context(0)
    c.point_cloud_distance(np.zeros((2, 3)), np.ones((3, 3)))      # first call: module load, allocator warm-up
    yield c
    c.close()


@pytest.mark.gpu
def test_known_answer_vector(ctx, oracle):
    """O3D/UnitTest/Core/Geometry/PointCloud.cpp:1074-1111."""
    g = np.load(os.path.join(HERE, "golden", "open3d_known_answers.npz"))
    p = g["rand_points"]
    d = ctx.point_cloud_distance(p[:50], p[50:100])
    assert np.abs(d - g["nn_distance_ref"]).max() < 1e-6
    assert np.array_equal(d, oracle.nn_distance(p[:50], p[50:100]))


def _moved(src, T):
    return src @ T[:3, :3].T + T[:3, 3]


def _cases():
    """name -> (source, target), built on demand."""
    rng = np.random.default_rng(7)

    def pair(ns, nt, moved):
        s, t, T, _ = synth.make_pair(ns, nt)
        return (_moved(s, T) if moved else s), t

    def far():
        s, t, _, _ = synth.make_pair(20000, 80000)
        ext = float((t.max(0) - t.min(0)).max())
        s = s.copy()
        k = np.random.default_rng(3).choice(len(s), len(s) // 100, replace=False)
        dirs = np.random.default_rng(4).standard_normal((len(k), 3))
        s[k] += 100.0 * ext * dirs / np.linalg.norm(dirs, axis=1, keepdims=True)
        return s, t

    def on_points():
        _, t, _, _ = synth.make_pair(10, 50000)
        return t[np.random.default_rng(5).choice(len(t), 10000, replace=False)], t

    def plane():
        t = rng.uniform(-1, 1, (40000, 3)); t[:, 2] = 0.0
        return rng.uniform(-1.2, 1.2, (8000, 3)), t

    def line():
        a = rng.uniform(-1, 1, 30000)
        t = np.c_[a, 0.5 * a + 0.25, -2.0 * a]
        return rng.uniform(-1.5, 1.5, (8000, 3)), t

    def repeated():
        s, t, _, _ = synth.make_pair(10000, 20000)
        return s, np.repeat(t, 3, axis=0)

    return {
        "pair_5k_20k": lambda: pair(5000, 20000, False),
        "pair_5k_20k_moved": lambda: pair(5000, 20000, True),
        "pair_64k_1m": lambda: pair(65536, 1048576, False),
        "pair_64k_1m_moved": lambda: pair(65536, 1048576, True),
        "partial_pair": lambda: synth.make_partial_pair(20000, 80000)[:2],
        "uniform_cube": lambda: (rng.uniform(-1, 1, (20000, 3)), rng.uniform(-1, 1, (100000, 3))),
        "offset_1e3": lambda: synth.make_pair(10000, 40000, offset=[1e3, -2e3, 1.5e3])[:2],
        "plane_z0": plane,
        "collinear": line,
        "far_queries": far,
        "queries_on_points": on_points,
        "target_repeated_3x": repeated,
        "one_point_target": lambda: (rng.uniform(-1, 1, (5000, 3)), np.array([[0.1, -0.2, 0.3]])),
        "empty_target": lambda: (rng.uniform(-1, 1, (1000, 3)), np.zeros((0, 3))),
        "empty_source": lambda: (np.zeros((0, 3)), rng.uniform(-1, 1, (1000, 3))),
    }


CASES = _cases()


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CASES))
def test_equals_the_reference(ctx, ref, name):
    s, t = CASES[name]()
    d = ctx.point_cloud_distance(s, t)
    assert d.shape == (len(s),)
    assert np.array_equal(d, ref.nn_distance(s, t)), name
    if name == "empty_target":
        assert np.array_equal(d, np.zeros(len(s)))
    if name == "queries_on_points":
        assert not d.any()


@pytest.mark.gpu
def test_full_size_c4_pair(ctx, ref):
    s, t, _, _ = synth.make_pair(262144, 4194304, motion="radius")
    assert np.array_equal(ctx.point_cloud_distance(s, t), ref.nn_distance(s, t))


@pytest.mark.gpu
@pytest.mark.parametrize("n", [2, 3, 9, 17, 1000, 20000])
def test_nearest_neighbor_distance_exhaustive(ctx, n):
    x = synth.surface_points(n, 11 + n)
    d = ctx.nearest_neighbor_distance(x)
    assert np.array_equal(d, flann_nn(x, x, exclude_self=True, chunk=256))


@pytest.mark.gpu
def test_nearest_neighbor_distance_1m_sampled(ctx):
    _, x, _, _ = synth.make_pair(10, 1048576)
    d = ctx.nearest_neighbor_distance(x)
    rows = np.random.default_rng(9).choice(len(x), 500, replace=False)
    assert np.array_equal(d[rows], flann_nn(x, x, exclude_self=True, rows=rows))


@pytest.mark.gpu
def test_nearest_neighbor_distance_edge_cases(ctx):
    x = synth.surface_points(5000, 3)
    assert not ctx.nearest_neighbor_distance(np.repeat(x, 2, axis=0)).any()          # every point duplicated
    y = np.r_[x, x[[17]]]                                                             # one duplicate
    d = ctx.nearest_neighbor_distance(y)
    assert d[17] == 0.0 and d[-1] == 0.0 and np.array_equal(d, flann_nn(y, y, exclude_self=True, chunk=256))
    assert np.array_equal(ctx.nearest_neighbor_distance(np.array([[1.0, 2.0, 3.0]])), [0.0])
    p = np.array([[0.1, 0.2, 0.3], [-0.4, 0.9, 2.5]])
    dd = np.sqrt(((p[0, 0] - p[1, 0]) ** 2 + (p[0, 1] - p[1, 1]) ** 2) + (p[0, 2] - p[1, 2]) ** 2)
    assert np.array_equal(ctx.nearest_neighbor_distance(p), [dd, dd])
    assert ctx.nearest_neighbor_distance(np.zeros((0, 3))).shape == (0,)


@pytest.mark.gpu
def test_worst_case_one_repeated_point(ctx):
    """1,048,576 copies of one point: every box bound equals the seed's d2, so the walk stops at the root."""
    c = np.array([0.3, -0.7, 1.1])
    t = np.repeat(c[None, :], 1048576, axis=0)
    s = c + np.random.default_rng(1).standard_normal((262144, 3)) * 1e-3
    t0 = time.perf_counter()
    d = ctx.point_cloud_distance(s, t)
    assert time.perf_counter() - t0 < 5.0
    assert np.array_equal(d, flann_nn(s, t[:1], chunk=262144))
    t0 = time.perf_counter()
    assert not ctx.nearest_neighbor_distance(t).any()
    assert time.perf_counter() - t0 < 5.0


@pytest.mark.gpu
def test_worst_case_centre_of_a_sphere(ctx, oracle):
    """64 queries at the centre of a sphere: (nearly) every leaf box is nearer than every point."""
    rng = np.random.default_rng(2)
    t = rng.standard_normal((1048576, 3))
    t /= np.linalg.norm(t, axis=1, keepdims=True)
    s = rng.standard_normal((64, 3)) * 1e-9
    t0 = time.perf_counter()
    d = ctx.point_cloud_distance(s, t)
    assert time.perf_counter() - t0 < 5.0
    assert np.array_equal(d, oracle.nn_distance(s, t))


@pytest.mark.gpu
def test_nan_rows(ctx):
    s, t, _, _ = synth.make_pair(5000, 20000)
    sn = s.copy(); sn[[0, 77, 4999], [0, 1, 2]] = np.nan
    ok = ~np.isnan(sn).any(1)
    d = ctx.point_cloud_distance(sn, t)
    assert np.array_equal(d[ok], ctx.point_cloud_distance(s[ok], t))
    tn = t.copy(); tn[[5, 600, 19999], [2, 0, 1]] = np.nan
    okt = ~np.isnan(tn).any(1)
    assert np.array_equal(ctx.point_cloud_distance(s, tn), ctx.point_cloud_distance(s, t[okt]))
    x = t.copy(); x[[3, 1000], [1, 1]] = np.nan
    okx = ~np.isnan(x).any(1)
    assert np.array_equal(ctx.nearest_neighbor_distance(x)[okx], ctx.nearest_neighbor_distance(x[okx]))


def _same(a, b):
    return (np.array_equal(a.transformation_, b.transformation_) and a.fitness_ == b.fitness_
            and a.inlier_rmse_ == b.inlier_rmse_ and a.num_correspondences == b.num_correspondences)


@pytest.mark.gpu
def test_context_state_untouched_single_registration(lib):
    """run, distance call, run == run, run, on a registration big enough for the persistent launch path."""
    s, t, _, r = synth.make_pair(131072, 1048576, motion="radius")
    other_s, other_t, _, _ = synth.make_pair(20000, 60000, seed_t=99, seed_s=98)
    out = []
    for with_call in (True, False):
        c = lib.Context(0)
        c.set_clouds_f64(s, t)
        a = c.run(None, r, 20, 0.0, 0.0)
        if with_call:
            c.point_cloud_distance(other_s, other_t)
            c.nearest_neighbor_distance(other_t)
        b = c.run(None, r, 20, 0.0, 0.0)
        out.append((a, b, c.correspondence_index().copy()))
        c.close()
    assert _same(out[0][0], out[1][0]) and _same(out[0][1], out[1][1])
    assert np.array_equal(out[0][2], out[1][2])


@pytest.mark.gpu
def test_context_state_untouched_yaw_sweep(lib):
    s, t, _, _ = synth.make_pair(5000, 20000)
    out = []
    for with_call in (True, False):
        c = lib.Context(0)
        c.set_clouds_f64(s, t)
        a = c.run_yaw_sweep(8, 0.05, 10, 0.0, 0.0)
        if with_call:
            c.point_cloud_distance(t[:3000], s)
            c.nearest_neighbor_distance(s)
        b = c.run_yaw_sweep(8, 0.05, 10, 0.0, 0.0)
        out.append((a, b))
        c.close()
    for (ra, la, pa), (rb, lb, pb) in zip(out[0], out[1]):
        assert la == lb and _same(ra, rb) and all(_same(x, y) for x, y in zip(pa, pb))


def _run_driver(binary, tmp_path, s, t):
    inp, outp = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(inp, "wb") as f:
        f.write(struct.pack("<qq", len(s), len(t)))
        f.write(np.ascontiguousarray(s, "<f8").tobytes())
        f.write(np.ascontiguousarray(t, "<f8").tobytes())
    p = subprocess.run([binary, inp, outp], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, (p.returncode, p.stderr)
    return np.fromfile(outp, "<f8").reshape(4, len(s))


@pytest.mark.gpu
def test_shim_entry_points_equal_the_c_abi(ctx, driver_bins, tmp_path):
    s, t, _, _ = synth.make_pair(5000, 20000)
    s = np.r_[s, t[:100]]                                  # some queries on target points, a duplicate or two
    s = np.r_[s, s[:3]]
    want_pc = ctx.point_cloud_distance(s, t)
    want_nn = ctx.nearest_neighbor_distance(s)
    for b in driver_bins:
        got = _run_driver(b, tmp_path, s, t)
        for k, want in enumerate((want_pc, want_pc, want_nn, want_nn)):
            assert np.array_equal(got[k], want), (b, k)
        empty = _run_driver(b, tmp_path, s[:10], np.zeros((0, 3)))
        assert not empty[:2].any()
