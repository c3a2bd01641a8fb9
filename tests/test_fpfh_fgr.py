"""FPFH features, exact feature matching and fast global registration (visma_icp_compute_fpfh, visma_icp_match_features,
visma_icp_fgr_correspondences / _fgr_optimize / visma_icp_fast_global_registration).

The yardstick is a numpy f64 specification written from the reference's lines (O3D/Core/Registration/Feature.cpp:38-157,
FastGlobalRegistration.cpp:42-375, flann/algorithms/dist.h:150-177): spec_fpfh (brute-force neighbour lists), spec_match,
spec_fgr_correspondences, spec_fgr_optimize.  tests/golden/fpfh_fgr.npz (tests/golden/gen_fpfh_fgr.py) pins it to the
compiled reference: (a) the reference's FPFH of the first 1,200 points of fragments.npz: src, (b) its
OptimizePairwiseRegistration and final transform for a fixed list of 600 pairs on the fragment pair.

Comparing FPFH values.  Another libm may move a pair across a bin edge or flip ComputePairFeatures' swap test.  A pair is
AMBIGUOUS when, in the specification, a bin argument lies within 1e-9 of an integer in 1..10, or |angle1| and |angle2|
differ by a non-zero amount below 1e-12.  A point is ambiguous if its own list, or the list of any point in its list,
holds such a pair.  Unambiguous points agree within 1e-9 absolute (values are at most 200); an ambiguous point within one
hist_incr per ambiguous pair: a pair of point k moves 100 / (len_k - 1) between two bins of SPFH_k, and the FPFH of a
point that lists k moves by that times (1 / d2_k) / sum(1 / d2) <= 1 -- the histogram's sum, by which the column is
rescaled, does not change.  At most 1 % of the points may be ambiguous, asserted on the specification alone."""
import math
import os
import struct
import subprocess
import sys

import numpy as np
import pytest

from nn_spec import cube_cloud, spec_lists  # noqa: F401  (the neighbour lists: shared with tests/test_nn_lists.py)
from oracle_engine import OracleEngine
from visma_amd import _lib, synth  # noqa: F401

HERE = os.path.dirname(os.path.abspath(__file__))
G = os.path.join(HERE, "golden")
sys.path.insert(0, os.path.join(HERE, "cpp"))
import build_shim  # noqa: E402
import build_fgr  # noqa: E402

TOL_T = 1e-5        # north_star: final SE(3) within 1e-5 relative Frobenius (test_gpu_kernels.py)
TOL_F = 1e-9        # FPFH values, absolute (they are at most 200); transforms, relative Frobenius
INVALID, STATE = 1, 5
DIM = 33


# ---------------------------------------------------------------------------
# the specification
# ---------------------------------------------------------------------------
def _bin(v):
    """(int)floor(v) clamped to [0, 10]; not finite -> 0 (Feature.cpp:92-94 on x86-64)"""
    with np.errstate(invalid="ignore"):
        f = np.floor(v)
        b = np.where(np.isfinite(f), np.clip(f, 0, 10), 0)
    return b.astype(np.int64)


def _near_edge(v):
    with np.errstate(invalid="ignore"):
        r = np.rint(v)
        return np.isfinite(v) & (r >= 1) & (r <= 10) & (np.abs(v - r) < 1e-9)


def spec_pair_features(p1, n1, p2, n2):
    """ComputePairFeatures (Feature.cpp:38-70), batched -> f (m, 3): result(0..2); amb (m,): the swap test is a near-tie."""
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        d = p2 - p1
        ln = np.sqrt(d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2])
        a1 = (n1[:, 0] * d[:, 0] + n1[:, 1] * d[:, 1] + n1[:, 2] * d[:, 2]) / ln
        a2 = (n2[:, 0] * d[:, 0] + n2[:, 1] * d[:, 1] + n2[:, 2] * d[:, 2]) / ln
        swap = np.arccos(np.abs(a1)) > np.arccos(np.abs(a2))
        gap = np.abs(np.abs(a1) - np.abs(a2))
        amb = (gap > 0) & (gap < 1e-12)
        a = np.where(swap[:, None], n2, n1)
        b = np.where(swap[:, None], n1, n2)
        d = np.where(swap[:, None], d * -1.0, d)
        f2 = np.where(swap, -a2, a1)
        v = np.stack([d[:, 1] * a[:, 2] - d[:, 2] * a[:, 1], d[:, 2] * a[:, 0] - d[:, 0] * a[:, 2],
                      d[:, 0] * a[:, 1] - d[:, 1] * a[:, 0]], 1)
        vn = np.sqrt(v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1] + v[:, 2] * v[:, 2])
        v = v / vn[:, None]
        w = np.stack([a[:, 1] * v[:, 2] - a[:, 2] * v[:, 1], a[:, 2] * v[:, 0] - a[:, 0] * v[:, 2],
                      a[:, 0] * v[:, 1] - a[:, 1] * v[:, 0]], 1)
        f1 = v[:, 0] * b[:, 0] + v[:, 1] * b[:, 1] + v[:, 2] * b[:, 2]
        f0 = np.arctan2(w[:, 0] * b[:, 0] + w[:, 1] * b[:, 1] + w[:, 2] * b[:, 2],
                        a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1] + a[:, 2] * b[:, 2])
        zero = (ln == 0.0) | (vn == 0.0)
    f = np.stack([f0, f1, f2], 1)
    f[zero] = 0.0
    return f, amb & ~zero


def spec_fpfh(xyz, nrm, search_type=0, knn=100, radius=0.0, details=False):
    """ComputeFPFHFeature (Feature.cpp:72-157) -> (n, 33), row i the reference's column i."""
    p = np.asarray(xyz, np.float64); nr = np.asarray(nrm, np.float64)
    n = len(p)
    idx, d2, cnt = spec_lists(p, search_type, knn, radius)
    cap = idx.shape[1]
    spfh = np.zeros((n, DIM))
    amb_pairs = np.zeros(n, np.int64)
    incr = np.where(cnt > 1, 100.0 / np.maximum(cnt - 1, 1), 0.0)
    npairs = 0
    for k in range(1, cap):
        rows = np.nonzero(cnt > k)[0]
        if not len(rows):
            break
        npairs += len(rows)
        j = idx[rows, k]
        f, amb = spec_pair_features(p[rows], nr[rows], p[j], nr[j])
        with np.errstate(invalid="ignore"):
            args = [11 * (f[:, 0] + math.pi) / (2.0 * math.pi), 11 * (f[:, 1] + 1.0) * 0.5, 11 * (f[:, 2] + 1.0) * 0.5]
        for h, v in enumerate(args):
            np.add.at(spfh, (rows, _bin(v) + 11 * h), incr[rows])
            amb = amb | _near_edge(v)
        amb_pairs[rows] += amb
    out = np.zeros((n, DIM))
    sums = np.zeros((n, 3))
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        for k in range(1, cap):
            live = (cnt > k) & (d2[:, k] != 0.0)
            val = np.where(live[:, None], spfh[idx[:, k]] / d2[:, k][:, None], 0.0)
            for j in range(DIM):
                sums[:, j // 11] += val[:, j]
            out += val
        scale = np.where(sums != 0.0, 100.0 / sums, sums)
        out = out * np.repeat(scale, 11, axis=1)
        out = out + spfh
    out[cnt <= 1] = 0.0
    if not details:
        return out
    # what a point's value may move by: its own ambiguous pairs and those of the points it lists, one hist_incr each
    slack = amb_pairs * incr
    listed = np.zeros(n)
    for k in range(1, cap):
        live = cnt > k
        listed += np.where(live, slack[idx[:, k]], 0.0)
    return out, dict(idx=idx, d2=d2, cnt=cnt, spfh=spfh, pairs=npairs, amb_pairs=amb_pairs, slack=slack + listed)


def spec_match(fa, fb, chunk=32):
    """For every row of fb the row of fa at the smallest flann L2 (dist.h:150-177: whole groups of four added as
    result += ((s0 + s1) + s2) + s3, the rest one by one), lowest index on ties; NaN / +inf never win -> (idx, d2)."""
    a = np.asarray(fa, np.float64); b = np.asarray(fb, np.float64)
    nb = len(b)
    idx = np.full(nb, -1, np.int32); dd = np.full(nb, np.inf)
    if len(a) == 0 or nb == 0:
        return idx, dd
    dim = a.shape[1]
    for s in range(0, nb, chunk):
        with np.errstate(invalid="ignore", over="ignore"):
            e = b[s:s + chunk, None, :] - a[None, :, :]
            e = e * e
            d = np.zeros(e.shape[:2])
            for g in range(dim // 4):
                d += ((e[..., 4 * g] + e[..., 4 * g + 1]) + e[..., 4 * g + 2]) + e[..., 4 * g + 3]
            for j in range(4 * (dim // 4), dim):
                d += e[..., j]
        d = np.where(np.isnan(d), np.inf, d)
        k = np.argmin(d, axis=1)                                   # the first minimum: the lowest index
        best = d[np.arange(len(k)), k]
        idx[s:s + chunk] = np.where(best < np.inf, k, -1)
        dd[s:s + chunk] = best
    return idx, dd


_MATCH_MEMO = {}


def spec_match_memo(fa, fb):
    """spec_match, computed once per pair of arrays (the fragment pair's two directions serve several tests unchanged)"""
    key = (id(fa), id(fb))
    if key not in _MATCH_MEMO:
        _MATCH_MEMO[key] = (fa, fb) + spec_match(fa, fb)          # (the arrays are kept alive: their ids stay theirs)
    return _MATCH_MEMO[key][2:]


OPT = dict(division_factor=1.4, max_corr_dist=0.025, tuple_scale=0.95, use_absolute_scale=False, decrease_mu=True,
           iteration_number=64, maximum_tuple_count=1000)       # FastGlobalRegistration.h:44-50


def _opt(**kw):
    o = dict(OPT); o.update(kw)
    return o


def spec_normalize(src, tgt, use_absolute_scale=False):
    """NormalizePointCloud (FastGlobalRegistration.cpp:189-240) -> ([src', tgt'], [mean_s, mean_t], scale_global, scale_start)"""
    out, means, scale = [], [], 0.0
    for c in (src, tgt):
        c = np.asarray(c, np.float64)
        m = np.zeros(3)
        for a in range(3):
            m[a] = np.cumsum(c[:, a])[-1]                        # the reference's running sum, in order
        m = m / len(c)
        c = c - m
        scale = max(scale, float(np.max(np.sqrt(c[:, 0] * c[:, 0] + c[:, 1] * c[:, 1] + c[:, 2] * c[:, 2]))))
        out.append(c); means.append(m)
    sg, ss = (1.0, scale) if use_absolute_scale else (scale, 1.0)
    return [c / sg for c in out], means, sg, ss


def philox4x32(c0, c1, k0, k1):
    """Philox4x32-10 at counter (c0, c1, 0, 0), key (k0, k1) -> 4 words (mesh.hip / host_math.hpp)"""
    M = 0xFFFFFFFF
    c = [c0 & M, c1 & M, 0, 0]
    for _ in range(10):
        p0, p1 = 0xD2511F53 * c[0], 0xCD9E8D57 * c[2]
        c = [(p1 >> 32) ^ c[1] ^ k0, p1 & M, (p0 >> 32) ^ c[3] ^ k1, p0 & M]
        k0 = (k0 + 0x9E3779B9) & M; k1 = (k1 + 0xBB67AE85) & M
    return c


def spec_fgr_correspondences(src, fs, tgt, ft, opt=OPT, seed=0, triples=None, match=spec_match_memo):
    """AdvancedMatching (FastGlobalRegistration.cpp:42-186) on the normalized clouds -> ((k, 2) pairs (source, target),
    dict(n_mutual, n_tuple_corres, n_trials))"""
    (ps, pt), _, _, _ = spec_normalize(src, tgt, opt["use_absolute_scale"])
    swapped = len(pt) > len(ps)
    (pi, fi), (pj, fj) = ((pt, ft), (ps, fs)) if swapped else ((ps, fs), (pt, ft))
    nn_i_of_j, _ = match(fi, fj)
    nn_j_of_i, _ = match(fj, fi)
    cross = [(i, int(nn_j_of_i[i])) for i in range(len(pi)) if nn_j_of_i[i] >= 0 and nn_i_of_j[nn_j_of_i[i]] == i]
    ncorr = len(cross)
    trials = 100 * ncorr
    if triples is not None:
        triples = np.asarray(triples, np.int64).reshape(-1, 3)
        trials = min(trials, len(triples))
    scale, out, cnt, t = opt["tuple_scale"], [], 0, 0
    while t < trials:
        if triples is not None:
            r = [int(x) % ncorr for x in triples[t]]
        else:
            r = [w % ncorr for w in philox4x32(t & 0xFFFFFFFF, t >> 32, seed & 0xFFFFFFFF, seed >> 32)[:3]]
        ii = [cross[x][0] for x in r]; jj = [cross[x][1] for x in r]

        def edge(P, u, v):
            e = P[u] - P[v]
            return math.sqrt(e[0] * e[0] + e[1] * e[1] + e[2] * e[2])
        li = [edge(pi, ii[0], ii[1]), edge(pi, ii[1], ii[2]), edge(pi, ii[2], ii[0])]
        lj = [edge(pj, jj[0], jj[1]), edge(pj, jj[1], jj[2]), edge(pj, jj[2], jj[0])]
        if all(li[k] * scale < lj[k] and lj[k] < li[k] / scale for k in range(3)):
            out += [(ii[k], jj[k]) for k in range(3)]
            cnt += 1
        t += 1
        if cnt >= opt["maximum_tuple_count"]:
            break
    pairs = np.array(out, np.int32).reshape(-1, 2)
    if swapped:
        pairs = pairs[:, ::-1].copy()
    return pairs, dict(n_mutual=ncorr, n_tuple_corres=len(pairs), n_trials=t)


def _euler(x):
    """TransformVector6dToMatrix4d (Eigen.cpp:58-68): Rz(x2) Ry(x1) Rx(x0), translation x[3:6]"""
    ca, sa, cb, sb, cg, sg = math.cos(x[0]), math.sin(x[0]), math.cos(x[1]), math.sin(x[1]), math.cos(x[2]), math.sin(x[2])
    Rx = np.array([[1, 0, 0], [0, ca, -sa], [0, sa, ca]]); Ry = np.array([[cb, 0, sb], [0, 1, 0], [-sb, 0, cb]])
    Rz = np.array([[cg, -sg, 0], [sg, cg, 0], [0, 0, 1]])
    T = np.eye(4); T[:3, :3] = Rz @ Ry @ Rx; T[:3, 3] = x[3:6]
    return T


def spec_optimize_pairs(p0, p1, pairs, opt, par):
    """OptimizePairwiseRegistration (FastGlobalRegistration.cpp:242-325) -> trans with trans * p1 ~ p0"""
    trans = np.eye(4)
    if len(pairs) < 10:
        return trans
    p = p0[pairs[:, 0]]; q = p1[pairs[:, 1]].copy()
    for itr in range(opt["iteration_number"]):
        rpq = p - q
        s = (par / ((rpq * rpq).sum(1) + par)) ** 2
        JTJ = np.zeros((6, 6)); JTr = np.zeros(6)
        z, o = np.zeros(len(q)), -np.ones(len(q))
        rows = [np.stack([z, -q[:, 2], q[:, 1], o, z, z], 1), np.stack([q[:, 2], z, -q[:, 0], z, o, z], 1),
                np.stack([-q[:, 1], q[:, 0], z, z, z, o], 1)]
        for k, J in enumerate(rows):
            JTJ += (J * s[:, None]).T @ J
            JTr += (J * (rpq[:, k] * s)[:, None]).sum(0)
        A = -JTJ
        det = np.linalg.det(A)
        x = np.zeros(6) if (abs(det) < 1e-6 or not np.isfinite(det)) else np.linalg.solve(A, JTr)
        delta = _euler(x)
        trans = delta @ trans
        q = q @ delta[:3, :3].T + delta[:3, 3]
        if opt["decrease_mu"] and itr % 4 == 0 and par > opt["max_corr_dist"]:
            par /= opt["division_factor"]
    return trans


def spec_fgr_optimize(src, tgt, pairs, opt=OPT):
    """Normalize, OptimizePairwiseRegistration from par = scale_global, GetTransformationOriginalScale, inverse
    (FastGlobalRegistration.cpp:347-375) -> (T source-to-target, the optimisation's own result)"""
    (ps, pt), means, sg, _ = spec_normalize(src, tgt, opt["use_absolute_scale"])
    t = spec_optimize_pairs(ps, pt, np.asarray(pairs).reshape(-1, 2), opt, sg)
    back = np.eye(4)
    back[:3, :3] = t[:3, :3]
    back[:3, 3] = -t[:3, :3] @ means[1] + t[:3, 3] * sg + means[0]
    return np.linalg.inv(back), t


def spec_fgr(src, fs, tgt, ft, opt=OPT, seed=0, triples=None, match=spec_match_memo):
    pairs, info = spec_fgr_correspondences(src, fs, tgt, ft, opt, seed, triples, match)
    return spec_fgr_optimize(src, tgt, pairs, opt)[0], pairs, info


# ---------------------------------------------------------------------------
# inputs
# ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(G, "fpfh_fgr.npz"))


@pytest.fixture(scope="module")
def frag():
    f = np.load(os.path.join(G, "fragments.npz"))
    return {k: f[k].astype(np.float64) for k in ("src", "src_normals", "tgt", "tgt_normals")}


_CACHE = {}


def frag1200(frag, kind):
    """the first 1,200 points of the fragment as a cloud of their own: (points, normals, spec value, details)"""
    if kind not in _CACHE:
        p, n = frag["src"][:1200], frag["src_normals"][:1200]
        args = dict(hybrid=(2, 100, 0.25), knn=(0, 30, 0.0))[kind]
        _CACHE[kind] = (p, n) + spec_fpfh(p, n, *args, details=True)
    return _CACHE[kind]


def corner_grid():
    """a 20 x 20 planar grid (z = 0, normal +z) joined to a perpendicular 20 x 19 grid (x = 0, normal +x), spacing 0.05:
    symmetric pairs sit mid-bin"""
    h = 0.05
    i, j = np.meshgrid(np.arange(20), np.arange(20), indexing="ij")
    floor = np.stack([i.ravel() * h, j.ravel() * h, np.zeros(400)], 1)
    i, j = np.meshgrid(np.arange(1, 20), np.arange(20), indexing="ij")
    wall = np.stack([np.zeros(380), j.ravel() * h, i.ravel() * h], 1)
    nrm = np.concatenate([np.tile([0.0, 0.0, 1.0], (400, 1)), np.tile([1.0, 0.0, 0.0], (380, 1))])
    return np.concatenate([floor, wall]), nrm


def check_fpfh(got, spec, det, what):
    """the comparison rule of the module's docstring"""
    amb = det["slack"] > 0
    assert amb.sum() <= 0.01 * len(spec), (what, int(amb.sum()))
    err = np.abs(got - spec).max(1) if len(spec) else np.zeros(0)
    print("FPFH %s: %d points, %d pairs, %d ambiguous pairs, %d ambiguous points; max |diff| %.3e (unambiguous), %.3e (ambiguous)"
          % (what, len(spec), det["pairs"], int(det["amb_pairs"].sum()), int(amb.sum()),
             float(err[~amb].max()) if (~amb).any() else 0.0, float(err[amb].max()) if amb.any() else 0.0))
    assert np.isfinite(got).all(), what
    assert (err[~amb] <= TOL_F).all(), (what, float(err[~amb].max()))
    assert (err[amb] <= det["slack"][amb] + TOL_F).all(), what


def rel_fro(A, B):
    return float(np.linalg.norm(A - B) / np.linalg.norm(B))


# ---------------------------------------------------------------------------
# CPU
# ---------------------------------------------------------------------------
NEW_SYMBOLS = ["visma_icp_compute_fpfh", "visma_icp_match_features", "visma_icp_fgr_correspondences", "visma_icp_fgr_optimize",
               "visma_icp_fast_global_registration"]
NEW_METHODS = ["compute_fpfh", "match_features", "fgr_correspondences", "fgr_optimize", "fast_global_registration"]


def test_symbols_and_methods(lib):
    L = lib.load()
    for name in NEW_SYMBOLS:
        assert hasattr(L, name), name
    for name in NEW_METHODS:
        assert callable(getattr(lib.Context, name, None)), name
    assert hasattr(lib, "CFgrOption") and hasattr(lib, "CFgrInfo") and lib.FPFH_DIM == 33
    o = lib.fgr_option()
    assert (o.division_factor, o.max_corr_dist, o.tuple_scale, o.use_absolute_scale, o.decrease_mu, o.iteration_number,
            o.maximum_tuple_count) == (1.4, 0.025, 0.95, 0, 1, 64, 1000)


@pytest.fixture()
def hctx(lib, oracle):
    eng = OracleEngine(oracle)
    ctx = eng.context()
    ctx.engine = eng
    yield ctx
    ctx.close()


def test_argument_checks(lib, hctx):
    """every argument error comes before anything reaches a device (a context on the oracle engine has none)"""
    import ctypes as C
    L, h = hctx.L, hctx._h
    dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int32)
    xyz = np.random.default_rng(1).random((50, 3)); out = np.zeros((50, 33)); nn = np.zeros(50, np.int32)
    x, o, f, n_ = xyz.ctypes.data_as(dp), out.ctypes.data_as(dp), out.ctypes.data_as(dp), nn.ctypes.data_as(ip)
    for knn in (1, 171, 0, -3):
        assert L.visma_icp_compute_fpfh(h, x, 50, x, 0, knn, 0.0, o) == INVALID
        assert L.visma_icp_compute_fpfh(h, x, 50, x, 2, knn, 0.1, o) == INVALID
    assert L.visma_icp_compute_fpfh(h, x, 50, x, 1, 30, 0.1, o) == INVALID          # Radius is not offered
    assert L.visma_icp_compute_fpfh(h, x, 50, x, 3, 30, 0.1, o) == INVALID
    assert L.visma_icp_compute_fpfh(h, None, 50, x, 0, 30, 0.0, o) == INVALID
    assert L.visma_icp_compute_fpfh(h, x, 50, None, 0, 30, 0.0, o) == INVALID
    assert L.visma_icp_compute_fpfh(h, x, 50, x, 0, 30, 0.0, None) == INVALID
    assert L.visma_icp_compute_fpfh(h, x, -1, x, 0, 30, 0.0, o) == INVALID
    assert L.visma_icp_compute_fpfh(None, x, 50, x, 0, 30, 0.0, o) == INVALID
    assert L.visma_icp_compute_fpfh(h, x, 50, x, 0, 30, 0.0, o) == STATE            # no HIP engine
    for dim in (0, 65, -1):
        assert L.visma_icp_match_features(h, f, 10, f, 10, dim, n_, None) == INVALID
    assert L.visma_icp_match_features(h, None, 10, f, 10, 33, n_, None) == INVALID
    assert L.visma_icp_match_features(h, f, 10, None, 10, 33, n_, None) == INVALID
    assert L.visma_icp_match_features(h, f, 10, f, 10, 33, None, None) == INVALID
    assert L.visma_icp_match_features(h, f, -1, f, 10, 33, n_, None) == INVALID
    assert L.visma_icp_match_features(h, f, 10, f, 0, 33, n_, None) == 0             # nothing to do
    assert L.visma_icp_match_features(h, f, 10, f, 10, 33, n_, None) == STATE
    T = np.zeros(16); k = C.c_int64(0)
    t_ = T.ctypes.data_as(dp)
    assert L.visma_icp_fast_global_registration(h, x, 0, f, x, 50, f, None, 0, None, 0, t_, None) == INVALID   # an empty cloud
    assert L.visma_icp_fast_global_registration(h, x, 50, f, x, 50, f, None, 0, None, 0, None, None) == INVALID
    assert L.visma_icp_fast_global_registration(h, x, 50, f, x, 50, f, None, 0, None, 5, t_, None) == INVALID  # triples missing
    assert L.visma_icp_fast_global_registration(h, x, 50, f, x, 50, f, None, 0, None, 0, t_, None) == STATE
    assert L.visma_icp_fgr_correspondences(h, x, 50, f, x, 50, f, None, 0, None, 0, n_, n_, 50, None, None) == INVALID
    assert L.visma_icp_fgr_correspondences(h, x, 50, f, x, 50, f, None, 0, None, 0, None, n_, 50, C.byref(k), None) == INVALID
    assert L.visma_icp_fgr_correspondences(h, x, 50, f, x, 50, f, None, 0, None, 0, n_, n_, 50, C.byref(k), None) == STATE
    # the optimisation is host arithmetic: index errors, and fewer than 10 pairs give the identity
    idx = np.arange(12, dtype=np.int32)
    i_ = idx.ctypes.data_as(ip)
    bad = idx.copy(); bad[3] = 50
    assert L.visma_icp_fgr_optimize(x, 50, x, 50, bad.ctypes.data_as(ip), i_, 12, None, t_, None) == INVALID
    assert L.visma_icp_fgr_optimize(x, 50, x, 50, i_, bad.ctypes.data_as(ip), 12, None, t_, None) == INVALID
    assert L.visma_icp_fgr_optimize(x, 50, x, 50, i_, i_, 12, None, None, None) == INVALID
    assert L.visma_icp_fgr_optimize(x, 0, x, 50, i_, i_, 12, None, t_, None) == INVALID
    Tm, Topt = lib.fgr_optimize(xyz, xyz + [0.5, 0.0, 0.0], idx[:9], idx[:9])
    assert np.array_equal(Topt, np.eye(4))
    assert np.allclose(Tm, np.array([[1, 0, 0, 0.5], [0, 1, 0, 0], [0, 0, 1, 0], [0, 0, 0, 1.0]]), atol=1e-15)   # the means only
    with pytest.raises(lib.IcpError):
        lib.fgr_optimize(xyz, xyz, bad, idx)
    # the context still runs everything else
    hctx.set_target(xyz.astype(np.float32)); hctx.set_source(xyz.astype(np.float32))
    assert hctx.run(None, 0.1, 3, 0.0, 0.0).num_correspondences > 0


def test_specification_fpfh_equals_the_reference(golden, frag):
    """fixture (a): the compiled reference's FPFH, Hybrid(0.25, 100), of the first 1,200 fragment points"""
    p, n, spec, det = frag1200(frag, "hybrid")
    assert not det["slack"].any(), "no pair of this input is ambiguous"
    ref = golden["fpfh_1200"]
    assert ref.shape == (1200, 33)
    err = float(np.abs(spec - ref).max())
    print("spec_fpfh vs the reference: max |diff| %.3e over %d points, %d pairs" % (err, len(p), det["pairs"]))
    assert err <= TOL_F
    assert 99.0 < ref[:, :11].sum(1).min() and ref.max() <= 200.0 + 1e-9


def test_ambiguous_pairs_are_rare_in_the_inputs(frag):
    """the 1 % cap is never the reason a test passes: count on the specification alone"""
    _, det = spec_fpfh(frag["src"], frag["src_normals"], 2, 100, 0.25, details=True)
    g, gn = corner_grid()
    _, gdet = spec_fpfh(g, gn, 2, 30, 0.12, details=True)
    print("ambiguous pairs: fragment src %d of %d, corner grid %d of %d"
          % (int(det["amb_pairs"].sum()), det["pairs"], int(gdet["amb_pairs"].sum()), gdet["pairs"]))
    assert (det["slack"] > 0).sum() <= 0.01 * len(frag["src"])
    assert (gdet["slack"] > 0).sum() <= 0.01 * len(g)


def test_specification_optimize_equals_the_reference(golden, frag):
    """fixture (b): the reference's OptimizePairwiseRegistration and final transform for 600 fixed pairs"""
    T, t = spec_fgr_optimize(frag["src"], frag["tgt"], golden["pairs"])
    print("spec_fgr_optimize vs the reference: %.3e (optimisation), %.3e (final)"
          % (rel_fro(t, golden["T_opt"]), rel_fro(T, golden["T_final"])))
    assert rel_fro(t, golden["T_opt"]) <= TOL_F
    assert rel_fro(T, golden["T_final"]) <= TOL_F


def test_host_optimize_equals_the_reference_and_the_specification(lib, golden, frag):
    """visma_icp_fgr_optimize is host arithmetic: pinned here without a GPU"""
    for opt in (OPT, _opt(use_absolute_scale=True, max_corr_dist=0.05), _opt(decrease_mu=False, iteration_number=7)):
        T, t = lib.fgr_optimize(frag["src"], frag["tgt"], golden["pairs"][:, 0], golden["pairs"][:, 1], lib.fgr_option(**opt))
        sT, st = spec_fgr_optimize(frag["src"], frag["tgt"], golden["pairs"], opt)
        assert rel_fro(t, st) <= TOL_F and rel_fro(T, sT) <= TOL_F, opt
    T, t = lib.fgr_optimize(frag["src"], frag["tgt"], golden["pairs"][:, 0], golden["pairs"][:, 1])
    assert rel_fro(t, golden["T_opt"]) <= TOL_F and rel_fro(T, golden["T_final"]) <= TOL_F


@pytest.fixture(scope="module")
def driver_bins(lib):
    if build_shim.eigen_dir() is not None:
        build_fgr.build()
    paths = [os.path.join(HERE, "cpp", "_build", b) for b in build_fgr.BINS]
    if not all(os.path.exists(p) for p in paths):
        pytest.skip("fgr driver not prebuilt and no Eigen headers here")
    return paths


def _write_driver_input(path, s, sn, t, tn, pairs, opt, radius, max_nn, seed):
    with open(path, "wb") as f:
        f.write(struct.pack("<qqqddddiiiiiiq", len(s), len(t), len(pairs), opt["division_factor"], opt["max_corr_dist"],
                            opt["tuple_scale"], radius, int(opt["use_absolute_scale"]), int(opt["decrease_mu"]),
                            opt["iteration_number"], opt["maximum_tuple_count"], max_nn, 0, seed))
        for a in (s, sn, t, tn):
            f.write(np.ascontiguousarray(a, "<f8").tobytes())
        f.write(np.ascontiguousarray(pairs, "<i4").tobytes())


def test_driver_host_path_equals_the_specification(golden, frag, driver_bins, tmp_path):
    """the shim's host optimisation (cicp::detail::fgr_optimize), both Eigen storage orders"""
    inp, outp = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    for opt in (OPT, _opt(use_absolute_scale=True)):
        _write_driver_input(inp, frag["src"], frag["src_normals"], frag["tgt"], frag["tgt_normals"], golden["pairs"], opt, 0.25, 100, 0)
        sT, st = spec_fgr_optimize(frag["src"], frag["tgt"], golden["pairs"], opt)
        for b in driver_bins:
            p = subprocess.run([b, "host", inp, outp], capture_output=True, text=True, timeout=120)
            assert p.returncode == 0, (b, p.returncode, p.stderr)
            v = np.frombuffer(open(outp, "rb").read(), "<f8")
            assert rel_fro(v[:16].reshape(4, 4), sT) <= TOL_F and rel_fro(v[16:32].reshape(4, 4), st) <= TOL_F, b


# ---------------------------------------------------------------------------
# GPU: FPFH
# ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ctx(lib):
    c = lib.Context(0)
    yield c
    c.close()


@pytest.mark.gpu
def test_fpfh_fragment_hybrid_against_the_specification_and_the_reference(ctx, golden, frag):
    p, n, spec, det = frag1200(frag, "hybrid")
    got = ctx.compute_fpfh(p, n, knn=100, radius=0.25)
    check_fpfh(got, spec, det, "fragment[:1200] Hybrid(0.25, 100)")
    assert float(np.abs(got - golden["fpfh_1200"]).max()) <= TOL_F
    for mode in (1, 2):                                           # both designs of the second pass: the same bits
        assert np.array_equal(ctx.compute_fpfh(p, n, knn=100, radius=0.25, second_pass=mode), got), mode


@pytest.mark.gpu
def test_fpfh_fragment_knn_against_the_specification(ctx, frag):
    p, n, spec, det = frag1200(frag, "knn")
    check_fpfh(ctx.compute_fpfh(p, n, knn=30), spec, det, "fragment[:1200] KNN(30)")
    assert np.array_equal(ctx.compute_fpfh(p, n, knn=30, second_pass=2), ctx.compute_fpfh(p, n, knn=30, second_pass=1))


@pytest.mark.gpu
def test_fpfh_corner_grid(ctx):
    g, gn = corner_grid()
    spec, det = spec_fpfh(g, gn, 2, 30, 0.12, details=True)
    check_fpfh(ctx.compute_fpfh(g, gn, knn=30, radius=0.12), spec, det, "corner grid Hybrid(0.12, 30)")


def cube_case(kind):
    """nn_spec.cube_cloud(shuffled): a 9 x 9 x 9 lattice in a seeded order, normals from a seed.  Nearly every list is cut
    inside an exact tie, so the columns say which of the tied points the (d2, index) order lets in."""
    key = ("cube",) + kind
    if key not in _CACHE:
        p = cube_cloud(shuffled=True)
        nr = np.random.default_rng(19).standard_normal(p.shape)
        nr /= np.linalg.norm(nr, axis=1)[:, None]
        _CACHE[key] = (p, nr) + spec_fpfh(p, nr, *kind, details=True)
    return _CACHE[key]


CUBE_KINDS = [(0, 30, 0.0), (2, 30, 0.3)]


@pytest.mark.parametrize("kind", CUBE_KINDS)
def test_specification_fpfh_of_the_lattice_depends_on_the_tie_break(kind):
    """with the ties broken by DESCENDING index instead (the same cloud, its order reversed) the columns differ: the case
    sees the rule"""
    p, nr, spec, det = cube_case(kind)
    assert (det["slack"] > 0).sum() <= 0.01 * len(p)
    other = spec_fpfh(p[::-1], nr[::-1], *kind)[::-1]
    assert (np.abs(other - spec).max(1) > 1e-3).sum() > 0.5 * len(p)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", CUBE_KINDS)
def test_fpfh_lattice_with_the_cut_inside_ties(ctx, kind):
    p, nr, spec, det = cube_case(kind)
    for mode in (1, 2):                                           # both designs of the second pass
        got = ctx.compute_fpfh(p, nr, knn=kind[1], radius=kind[2] if kind[0] == 2 else None, second_pass=mode)
        check_fpfh(got, spec, det, "shuffled 9 x 9 x 9 lattice %s, second pass %d" % (kind, mode))


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 2])
def test_fpfh_one_and_two_points(ctx, n):
    p = np.array([[0.1, 0.2, 0.3], [0.15, 0.2, 0.35]])[:n]; nr = np.array([[0.0, 0.0, 1.0], [0.0, 0.6, 0.8]])[:n]
    for kind in (dict(knn=30), dict(knn=30, radius=0.5), dict(knn=2)):
        spec, det = spec_fpfh(p, nr, 2 if "radius" in kind else 0, kind["knn"], kind.get("radius", 0.0), details=True)
        got = ctx.compute_fpfh(p, nr, **kind)
        check_fpfh(got, spec, det, "n = %d %s" % (n, kind))
        assert (n == 1) == (not got.any())


@pytest.mark.gpu
def test_fpfh_duplicates_skip_zero_distance_and_bin_the_zero_pair(ctx):
    p = np.array([[0, 0, 0], [0.1, 0, 0], [0, 0, 0], [0, 0.1, 0.02], [0.05, 0.05, 0.1]], np.float64)
    nr = np.array([[0, 0, 1], [0, 0.6, 0.8], [0, 0, 1], [0.6, 0, 0.8], [1, 0, 0]], np.float64)
    spec, det = spec_fpfh(p, nr, 0, 5, details=True)
    assert (det["d2"][[0, 2], 1] == 0.0).all()
    assert det["spfh"][0, 5] >= 25.0 and det["spfh"][0, 16] >= 25.0 and det["spfh"][0, 27] >= 25.0      # the zero 4-vector: 5 / 16 / 27
    got = ctx.compute_fpfh(p, nr, knn=5)
    check_fpfh(got, spec, det, "5 points, 2 duplicates")
    check_fpfh(ctx.compute_fpfh(p, nr, knn=5, radius=1.0), spec_fpfh(p, nr, 2, 5, 1.0), det, "5 points, 2 duplicates, Hybrid")


@pytest.mark.gpu
def test_fpfh_lds_maximum_and_list_length_limits(ctx, lib):
    rng = np.random.default_rng(7)
    p = rng.random((300, 3)); nr = rng.standard_normal((300, 3)); nr /= np.linalg.norm(nr, axis=1)[:, None]
    spec, det = spec_fpfh(p, nr, 0, 170, details=True)
    check_fpfh(ctx.compute_fpfh(p, nr, knn=170), spec, det, "300 points KNN(170)")
    spec, det = spec_fpfh(p, nr, 2, 170, 0.6, details=True)
    check_fpfh(ctx.compute_fpfh(p, nr, knn=170, radius=0.6), spec, det, "300 points Hybrid(0.6, 170)")
    for bad in (171, 1):
        with pytest.raises(lib.IcpError) as e:
            ctx.compute_fpfh(p, nr, knn=bad)
        assert e.value.code == INVALID
    # knn > n: the list is the whole cloud
    spec, det = spec_fpfh(p[:40], nr[:40], 0, 100, details=True)
    assert (det["cnt"] == 40).all()
    check_fpfh(ctx.compute_fpfh(p[:40], nr[:40], knn=100), spec, det, "40 points KNN(100)")


@pytest.mark.gpu
def test_fpfh_ragged_tail_isolated_point_and_determinism(ctx):
    rng = np.random.default_rng(11)
    p = rng.random((257, 3)) * [1.0, 1.0, 0.1]; nr = np.tile([0.0, 0.0, 1.0], (257, 1)) + rng.standard_normal((257, 3)) * 0.2
    nr /= np.linalg.norm(nr, axis=1)[:, None]
    p[256] = [5.0, 5.0, 5.0]                                      # nobody within the radius
    for kind in ((2, 30, 0.2), (0, 30, 0.0), (2, 100, 0.2)):
        spec, det = spec_fpfh(p, nr, *kind, details=True)
        got = ctx.compute_fpfh(p, nr, knn=kind[1], radius=kind[2] if kind[0] == 2 else None)
        check_fpfh(got, spec, det, "257 points %s" % (kind,))
        if kind[0] == 2:
            assert det["cnt"][256] == 1 and not got[256].any()
        assert np.array_equal(ctx.compute_fpfh(p, nr, knn=kind[1], radius=kind[2] if kind[0] == 2 else None), got)
    assert not ctx.compute_fpfh(p, nr, knn=30, radius=0.0).any()                       # no radius, no neighbours
    assert not ctx.compute_fpfh(p, nr, knn=30, radius=float("inf")).any()
    assert not ctx.compute_fpfh(p, nr, knn=30, radius=-1.0).any()
    assert not ctx.compute_fpfh(p, nr, knn=30, radius=float("nan")).any()


@pytest.mark.gpu
@pytest.mark.parametrize("kind", [(2, 30, 0.2), (0, 30, 0.0)])
def test_fpfh_nan_normal_and_nan_coordinate_stay_local(ctx, kind):
    """a non-finite value reaches sums only: a point whose list holds neither poisoned point, nor a point whose list does,
    keeps its column bit for bit, and the run ends clean"""
    rng = np.random.default_rng(13)
    p = rng.random((600, 3)) * [1.0, 1.0, 0.1]; nr = np.tile([0.0, 0.0, 1.0], (600, 1)) + rng.standard_normal((600, 3)) * 0.2
    nr /= np.linalg.norm(nr, axis=1)[:, None]
    a, b = 100, 400
    _, det = spec_fpfh(p, nr, *kind, details=True)
    call = lambda P, N: ctx.compute_fpfh(P, N, knn=kind[1], radius=kind[2] if kind[0] == 2 else None)     # noqa: E731
    clean = call(p, nr)
    pp, nn = p.copy(), nr.copy()
    nn[a, 1] = np.nan; pp[b, 0] = np.nan
    got = call(pp, nn)
    live = np.arange(det["idx"].shape[1])[None, :] < det["cnt"][:, None]
    touched = ((np.isin(det["idx"], [a, b]) & live).any(1))
    touched[[a, b]] = True
    dirty = touched | (touched[det["idx"]] & live).any(1)
    assert 0 < dirty.sum() < 0.5 * len(p)
    assert np.array_equal(got[~dirty], clean[~dirty])
    assert not got[b].any()                                       # the point without coordinates has no neighbours
    assert np.array_equal(call(pp, nn), got, equal_nan=True)


# ---------------------------------------------------------------------------
# GPU: matching -- indices identical to spec_match, d2 bit-identical
# ---------------------------------------------------------------------------
def check_match(ctx, fa, fb, what):
    idx, d2 = ctx.match_features(fa, fb)
    sidx, sd2 = spec_match(fa, fb)
    assert np.array_equal(idx, sidx), what
    assert np.array_equal(d2, sd2), what
    return idx, d2


@pytest.mark.gpu
@pytest.mark.parametrize("dim", [1, 33, 64])
@pytest.mark.parametrize("na,nb", [(1, 1), (1, 300), (300, 1), (257, 513)])
def test_match_sizes_and_dimensions(ctx, na, nb, dim):
    rng = np.random.default_rng(na * 1000 + nb + dim)
    check_match(ctx, rng.random((na, dim)) * 100.0, rng.random((nb, dim)) * 100.0, (na, nb, dim))


@pytest.mark.gpu
@pytest.mark.parametrize("dim", [2, 3, 4, 5, 16, 17, 34, 35, 36, 37, 63])
def test_match_every_group_and_tail_length(ctx, dim):
    """flann adds whole groups of four, then the rest one by one: every dim % 4, either side of each kernel width"""
    rng = np.random.default_rng(dim)
    check_match(ctx, rng.random((130, dim)) * 100.0, rng.random((70, dim)) * 100.0, dim)


@pytest.mark.gpu
def test_match_real_features_against_themselves(ctx, frag):
    p, n, spec, det = frag1200(frag, "hybrid")
    f = ctx.compute_fpfh(p, n, knn=100, radius=0.25)
    idx, d2 = check_match(ctx, f, f, "1,200 FPFH rows against themselves")
    first = np.array([np.nonzero((f == f[i]).all(1))[0][0] for i in range(len(f))])
    assert np.array_equal(idx, first) and not d2.any()           # the identity (a duplicate row: its first copy)


@pytest.mark.gpu
def test_match_ties_empty_set_nan_rows_and_invalid_dims(ctx, lib):
    rng = np.random.default_rng(5)
    fa = rng.integers(0, 3, (200, 33)).astype(np.float64)
    fa[50] = fa[7]; fa[120] = fa[7]; fa[10] = 0.0; fa[3] = 0.0     # duplicate rows, all-zero rows
    fb = np.concatenate([fa[[7, 120, 10]], np.zeros((2, 33)), rng.integers(0, 3, (60, 33)).astype(np.float64)])
    idx, d2 = check_match(ctx, fa, fb, "ties")
    assert list(idx[:5]) == [7, 7, 3, 3, 3] and not d2[:5].any()
    idx, d2 = ctx.match_features(np.zeros((0, 33)), fb)            # na = 0
    assert (idx == -1).all() and np.isposinf(d2).all()
    fan, fbn = fa.copy(), fb.copy()
    fan[7, 4] = np.nan; fbn[1, 32] = np.nan
    idx, d2 = check_match(ctx, fan, fbn, "a NaN row on each side")
    assert idx[1] == -1 and np.isposinf(d2[1]) and idx[0] == 50 and (idx != 7).all()
    idx, d2 = check_match(ctx, np.full((3, 5), np.nan), fb[:4, :5], "nothing finite")
    assert (idx == -1).all()
    for dim in (65, 0):
        with pytest.raises(lib.IcpError) as e:
            ctx.match_features(np.zeros((4, dim)), np.zeros((4, dim)))
        assert e.value.code == INVALID


# ---------------------------------------------------------------------------
# GPU: fast global registration, triples given explicitly
# ---------------------------------------------------------------------------
def triples_for(n, seed=3):
    return np.random.default_rng(seed).integers(0, 2 ** 31 - 1, (n, 3)).astype(np.int32)


@pytest.fixture(scope="module")
def frag_features(ctx, frag):
    return (ctx.compute_fpfh(frag["src"], frag["src_normals"], knn=100, radius=0.25),
            ctx.compute_fpfh(frag["tgt"], frag["tgt_normals"], knn=100, radius=0.25))


@pytest.mark.gpu
def test_fgr_fragment_pair_correspondences_transform_and_counts(ctx, frag, frag_features):
    fs, ft = frag_features
    tr = triples_for(200000)
    sT, spairs, sinfo = spec_fgr(frag["src"], fs, frag["tgt"], ft, triples=tr)
    pairs, info = ctx.fgr_correspondences(frag["src"], fs, frag["tgt"], ft, triples=tr)
    assert np.array_equal(pairs, spairs)
    assert (info.n_mutual, info.n_tuple_corres, info.n_trials) == (sinfo["n_mutual"], sinfo["n_tuple_corres"], sinfo["n_trials"])
    T, info2 = ctx.fast_global_registration(frag["src"], fs, frag["tgt"], ft, triples=tr)
    print("FGR fragment pair: %s, vs the specification %.3e" % (info2, rel_fro(T, sT)))
    assert rel_fro(T, sT) <= TOL_F
    assert (info2.n_mutual, info2.n_tuple_corres, info2.n_trials) == (info.n_mutual, info.n_tuple_corres, info.n_trials)
    # a swapped order (the smaller cloud first) gives the inverse pairing
    rp, rinfo = ctx.fgr_correspondences(frag["tgt"], ft, frag["src"], fs, triples=tr)
    assert np.array_equal(rp, pairs[:, ::-1]) and rinfo.n_mutual == info.n_mutual
    assert np.array_equal(rp, spec_fgr_correspondences(frag["tgt"], ft, frag["src"], fs, triples=tr)[0])


@pytest.mark.gpu
def test_fgr_optimize_on_the_fixture_list(ctx, golden, frag):
    T, t = ctx.fgr_optimize(frag["src"], frag["tgt"], golden["pairs"][:, 0], golden["pairs"][:, 1])
    assert rel_fro(t, golden["T_opt"]) <= TOL_F and rel_fro(T, golden["T_final"]) <= TOL_F


def _pose_error(T, truth):
    d = T @ np.linalg.inv(truth)
    ang = math.degrees(math.acos(max(-1.0, min(1.0, (np.trace(d[:3, :3]) - 1.0) / 2.0))))
    return ang, float(np.linalg.norm(T[:3, 3] - truth[:3, 3]))


@pytest.mark.gpu
def test_fgr_finds_a_pose_icp_cannot_reach_from_the_identity(ctx, lib, frag):
    """the case the feature exists for: tgt = src moved by 150 degrees about a tilted axis plus (0.7, -0.4, 0.3), every
    second point kept"""
    ax = np.array([0.3, 0.2, 0.9]); ax /= np.linalg.norm(ax)
    th = math.radians(150.0)
    K = np.array([[0, -ax[2], ax[1]], [ax[2], 0, -ax[0]], [-ax[1], ax[0], 0]])
    truth = np.eye(4)
    truth[:3, :3] = np.eye(3) + math.sin(th) * K + (1 - math.cos(th)) * K @ K
    truth[:3, 3] = [0.7, -0.4, 0.3]
    src, sn = frag["src"], frag["src_normals"]
    tgt = (src @ truth[:3, :3].T + truth[:3, 3])[::2].copy(); tn = (sn @ truth[:3, :3].T)[::2].copy()
    fs = ctx.compute_fpfh(src, sn, knn=100, radius=0.25); ft = ctx.compute_fpfh(tgt, tn, knn=100, radius=0.25)
    tr = triples_for(200000, 9)
    sT, _, sinfo = spec_fgr(src, fs, tgt, ft, triples=tr)
    ang, dt = _pose_error(sT, truth)
    print("FGR by the specification: %.3f degrees, %.4f off the truth (%s)" % (ang, dt, sinfo))
    assert ang < 5.0 and dt < 0.05
    T, info = ctx.fast_global_registration(src, fs, tgt, ft, triples=tr)
    ang, dt = _pose_error(T, truth)
    print("FGR on the GPU path: %.3f degrees, %.4f off the truth (%s)" % (ang, dt, info))
    assert ang < 5.0 and dt < 0.05
    # visma_icp_run from the FGR pose, coarse to fine: the target keeps every second point, so half of the source has no
    # exact partner, and at a radius of 0.1 (FGR's error bound and more) those points pair with a neighbour of their partner and
    # hold the pose 1.2e-3 off.  11 of the 1,951 dropped points lie within 0.01 of a kept one, 2 within 0.002: the schedule
    # ends with (almost) only exact pairs.  The same schedule from the identity finds no pair at all.
    ctx.set_clouds_f64(src, tgt)

    def schedule(start):
        pose, trace = start, []
        for r in (0.1, 0.01, 0.002):
            pose = ctx.run(pose, r, 60, 0.0, 0.0).transformation_
            trace.append(rel_fro(pose, truth))
        return pose, trace
    warm, wtrace = schedule(T)
    cold, ctrace = schedule(None)
    print("ICP at radii 0.1, 0.01, 0.002 from the FGR pose: %s, from the identity: %s (relative Frobenius to the truth)"
          % (wtrace, ctrace))
    assert rel_fro(warm, truth) < TOL_T
    assert not rel_fro(cold, truth) < TOL_T


@pytest.mark.gpu
def test_fgr_options_and_seeds(ctx, lib, frag, frag_features):
    fs, ft = frag_features
    src, tgt = frag["src"], frag["tgt"]
    tr = triples_for(200000)
    # fewer than 10 correspondences: the optimisation returns the identity, and mapping back leaves the means' difference
    T, info = ctx.fast_global_registration(src, fs, tgt, ft, lib.fgr_option(maximum_tuple_count=3), triples=tr)
    assert info.n_tuple_corres == 9 and np.array_equal(T[:3, :3], np.eye(3)) and np.array_equal(T[3], [0, 0, 0, 1])
    assert np.allclose(T[:3, 3], tgt.mean(0) - src.mean(0), rtol=0, atol=1e-12)
    p9, _ = ctx.fgr_correspondences(src, fs, tgt, ft, lib.fgr_option(maximum_tuple_count=3), triples=tr)
    assert np.array_equal(ctx.fgr_optimize(src, tgt, p9[:, 0], p9[:, 1])[1], np.eye(4))
    # maximum_tuple_count is honoured, and the pairs are a prefix of the longer run's
    p50, i50 = ctx.fgr_correspondences(src, fs, tgt, ft, lib.fgr_option(maximum_tuple_count=50), triples=tr)
    p1000, i1000 = ctx.fgr_correspondences(src, fs, tgt, ft, triples=tr)
    assert len(p50) == 150 == i50.n_tuple_corres and i50.n_trials <= i1000.n_trials and np.array_equal(p50, p1000[:150])
    assert np.array_equal(p50, spec_fgr_correspondences(src, fs, tgt, ft, _opt(maximum_tuple_count=50), triples=tr)[0])
    # few triples given: no more trials than triples
    _, ifew = ctx.fgr_correspondences(src, fs, tgt, ft, triples=tr[:40])
    assert ifew.n_trials == 40
    # the seed path: deterministic for one seed, different for two, the specification's draws, every tuple inside the ratios
    a, ia = ctx.fgr_correspondences(src, fs, tgt, ft, seed=5)
    b, _ = ctx.fgr_correspondences(src, fs, tgt, ft, seed=5)
    c, _ = ctx.fgr_correspondences(src, fs, tgt, ft, seed=6)
    assert np.array_equal(a, b) and not np.array_equal(a, c) and len(a) and len(a) % 3 == 0
    sa, sia = spec_fgr_correspondences(src, fs, tgt, ft, seed=5, match=lambda x, y: ctx.match_features(x, y))
    assert np.array_equal(a, sa) and ia.n_trials == sia["n_trials"]
    (ps, pt), _, _, _ = spec_normalize(src, tgt)
    for k in range(0, len(a), 3):
        for u, v in ((0, 1), (1, 2), (2, 0)):
            ls = np.linalg.norm(ps[a[k + u, 0]] - ps[a[k + v, 0]]); lt = np.linalg.norm(pt[a[k + u, 1]] - pt[a[k + v, 1]])
            assert ls * 0.95 < lt < ls / 0.95


@pytest.mark.gpu
def test_shim_driver_runs_the_registration(ctx, frag, driver_bins, tmp_path):
    """open3d::ComputeFPFHFeature + open3d::FastGlobalRegistration(seed) through the shim equal the C ABI"""
    inp, outp = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    _write_driver_input(inp, frag["src"], frag["src_normals"], frag["tgt"], frag["tgt_normals"], np.zeros((0, 2), np.int32), OPT,
                        0.25, 100, 17)
    fs = ctx.compute_fpfh(frag["src"], frag["src_normals"], knn=100, radius=0.25)
    ft = ctx.compute_fpfh(frag["tgt"], frag["tgt_normals"], knn=100, radius=0.25)
    T, _ = ctx.fast_global_registration(frag["src"], fs, frag["tgt"], ft, seed=17)
    for b in driver_bins:
        p = subprocess.run([b, "run", inp, outp], capture_output=True, text=True, timeout=120)
        assert p.returncode == 0, (b, p.returncode, p.stderr)
        v = np.frombuffer(open(outp, "rb").read(), "<f8")
        assert np.array_equal(v[:16].reshape(4, 4), T), b
        assert np.array_equal(v[16:].reshape(-1, 33), fs), b
