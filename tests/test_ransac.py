"""RANSAC global registration (visma_icp_ransac_hypotheses / _host, visma_icp_registration_ransac_feature_matching,
visma_icp_registration_ransac_correspondence).

The yardstick is a numpy f64 specification written from the reference's lines (O3D/Core/Registration/Registration.cpp:98-123,
188-353, CorrespondenceChecker.cpp:35-89, Eigen/src/Geometry/Umeyama.h:118-159): spec_hypothesis (draw, gather, checkers,
umeyama), spec_evaluate (brute force), spec_ransac_feature, spec_ransac_corres.  tests/golden/ransac.npz
(tests/golden/gen_ransac.py) pins it to the compiled reference on every third point of fragments.npz: ComputeTransformation,
the verdict of each checker and EvaluateRegistration for 240 fixed draw sets, EvaluateRANSACBasedOnCorrespondence for a list
of 600 pairs at 20 of those transforms.

Ambiguity is a condition, not a tolerance.  The specification marks a trial AMBIGUOUS when a comparison lies within 1e-9
relative of its threshold or sigma's second singular value is below 1e-6 of its first (the rotation is not defined), and an
evaluation when a nearest distance lies within 1e-9 relative of the radius.  Every comparison below is made on trials that
are not: test_no_trial_is_ambiguous asserts it for the fixture and for every seeded run whose pair table is known without a
GPU (the seeds are written here); the runs on FPFH features assert it where they compute their specification.

Pair tables without a GPU: features of dimension 3, source feature i = target point nn[i], target feature j = target point
j.  The exact match of source feature i is then nn[i] (distance 0; the target has no duplicate point), so the registration
runs on the fixture's pair table."""
import math
import os
import struct
import subprocess
import sys

import numpy as np
import pytest

from oracle_engine import OracleEngine
from visma_amd import _lib  # noqa: F401

HERE = os.path.dirname(os.path.abspath(__file__))
G = os.path.join(HERE, "golden")
sys.path.insert(0, os.path.join(HERE, "cpp"))
import build_shim  # noqa: E402
import build_ransac  # noqa: E402

TOL_T = 1e-5        # north_star: final SE(3) within 1e-5 relative Frobenius (test_fpfh_fgr.py, test_gpu_kernels.py)
TOL_F = 1e-9        # transforms against the reference and the specification, relative Frobenius
TOL_HD = 1e-12      # GPU against the host entry (same functions, another compiler back end), relative Frobenius; rmse
INVALID, STATE = 1, 5
PASS, BEFORE, AFTER = 0, 1, 2
AMB = 1e-9


# ---------------------------------------------------------------------------
# the specification
# ---------------------------------------------------------------------------
def philox4x32(c0, c1, c2, k0, k1):
    """Philox4x32-10 at counters (c0, c1, c2, 0) (arrays), key (k0, k1) -> 4 arrays of words (mesh.hip / host_math.hpp)"""
    M = np.uint64(0xFFFFFFFF)
    c = [np.asarray(c0, np.uint64) & M, np.asarray(c1, np.uint64) & M, np.asarray(c2, np.uint64) & M, np.zeros_like(np.asarray(c0, np.uint64))]
    k0, k1 = np.uint64(k0 & 0xFFFFFFFF), np.uint64(k1 & 0xFFFFFFFF)
    for _ in range(10):
        p0, p1 = np.uint64(0xD2511F53) * c[0], np.uint64(0xCD9E8D57) * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ k0, p1 & M, (p0 >> np.uint64(32)) ^ c[3] ^ k1, p0 & M]
        k0 = (k0 + np.uint64(0x9E3779B9)) & M; k1 = (k1 + np.uint64(0xBB67AE85)) & M
    return c


def spec_draws(n_pairs, ransac_n, t0, n_trials, seed=0, draws=None):
    """indices into the pair table, (n_trials, ransac_n): draws[t] mod n_pairs, or word j mod 4 at counter (t, j / 4)"""
    t = np.arange(t0, t0 + n_trials, dtype=np.uint64)
    if draws is not None:
        return np.mod(np.asarray(draws, np.int64).reshape(-1, ransac_n)[t0:t0 + n_trials], n_pairs)
    out = np.empty((n_trials, ransac_n), np.int64)
    for g in range((ransac_n + 3) // 4):
        w = philox4x32(t & np.uint64(0xFFFFFFFF), t >> np.uint64(32), np.full(n_trials, g, np.uint64), seed & 0xFFFFFFFF, seed >> 32)
        for j in range(4 * g, min(ransac_n, 4 * g + 4)):
            out[:, j] = (w[j - 4 * g] % np.uint64(n_pairs)).astype(np.int64)
    return out


def _near(a, b):
    """a within 1e-9 relative of the threshold b (two exact zeros -- a repeated pair's edge -- compare exactly)"""
    with np.errstate(invalid="ignore"):
        return (np.abs(a - b) <= AMB * np.abs(b)) & ~((a == 0) & (b == 0))


def spec_umeyama(p, q):
    """Eigen::umeyama(p, q, false) for stacks (T, n, 3) -> R (T, 3, 3), t (T, 3), singular values (T, 3).  A sigma that is not
    finite: R = I and t = NaN, what the reference's Eigen returns (every comparison of its JacobiSVD is false, so no rotation
    is applied to U = V = I; checked with Eigen::umeyama on a set holding a NaN point)"""
    n = p.shape[1]
    pm, qm = p.sum(1) / n, q.sum(1) / n
    sigma = np.einsum("tna,tnb->tab", q - qm[:, None], p - pm[:, None]) / n
    ok = np.isfinite(sigma).all((1, 2))
    R = np.tile(np.eye(3), (len(p), 1, 1)); S = np.full((len(p), 3), np.nan)
    if ok.any():
        U, s, Vt = np.linalg.svd(sigma[ok])
        D = np.ones((len(U), 3))
        D[:, 2] = np.where(np.linalg.det(U) * np.linalg.det(Vt) < 0, -1.0, 1.0)
        R[ok] = (U * D[:, None, :]) @ Vt
        S[ok] = s
    t = qm - np.einsum("tab,tb->ta", R, pm)
    return R, t, S


def spec_checkers(P, si, ti, R, t, edge=None, dist=None, angle=None):
    """the three CorrespondenceCheckers on stacks of pairs -> (edge_ok, dist_ok, normal_ok, ambiguous_before, ambiguous_after);
    a threshold None: that checker passes everything"""
    n = si.shape[1]
    p, q = P["src"][si], P["tgt"][ti]
    T_ = len(si)
    e_ok = np.ones(T_, bool); d_ok = np.ones(T_, bool); n_ok = np.ones(T_, bool)
    amb_b = np.zeros(T_, bool); amb_a = np.zeros(T_, bool)
    with np.errstate(invalid="ignore"):
        if edge is not None:
            for i in range(n):
                for j in range(i + 1, n):
                    ds = np.sqrt(((p[:, i] - p[:, j]) ** 2).sum(1)); dt = np.sqrt(((q[:, i] - q[:, j]) ** 2).sum(1))
                    e_ok &= ~((ds < dt * edge) | (dt < ds * edge))
                    amb_b |= _near(ds, dt * edge) | _near(dt, ds * edge)
        if dist is not None:
            moved = np.einsum("tab,tnb->tna", R, p) + t[:, None]
            r = np.sqrt(((q - moved) ** 2).sum(2))
            d_ok &= ~(r > dist).any(1)
            amb_a |= _near(r, dist).any(1)
        if angle is not None and P.get("sn") is not None and P.get("tn") is not None:
            c = math.cos(angle)
            dot = (P["tn"][ti] * np.einsum("tab,tnb->tna", R, P["sn"][si])).sum(2)
            n_ok &= ~(dot < c).any(1)
            amb_a |= _near(dot, c).any(1)
    return e_ok, d_ok, n_ok, amb_b, amb_a


def spec_hypothesis(P, idx, edge=None, dist=None, angle=None):
    """one trial per row of idx (indices into the pair table) -> verdict (T,), T (T, 4, 4), ambiguous (T,)"""
    si = P["pair_src"][idx] if P.get("pair_src") is not None else idx
    ti = P["pair_tgt"][idx]
    lone = (ti < 0).any(1)
    ti = np.maximum(ti, 0)
    R, t, S = spec_umeyama(P["src"][si], P["tgt"][ti])
    e_ok, d_ok, n_ok, amb_b, amb_a = spec_checkers(P, si, ti, R, t, edge, dist, angle)
    before = lone | ~e_ok
    with np.errstate(invalid="ignore"):
        amb_a = amb_a | (S[:, 1] < 1e-6 * S[:, 0])
    verdict = np.where(before, BEFORE, np.where(d_ok & n_ok, PASS, AFTER)).astype(np.int8)
    T = np.zeros((len(idx), 4, 4))
    T[:, :3, :3] = R; T[:, :3, 3] = t; T[:, 3, 3] = 1.0
    T[before] = 0.0
    return verdict, T, (~lone & amb_b) | (~before & amb_a)


def spec_evaluate(src, tgt, T, max_dist):
    """EvaluateRegistration by brute force: the nearest target point of every moved source point, kept where its squared
    distance is < (double)(float)(max_dist^2) (KDTreeFlann::SearchHybrid hands flann a float radius)
    -> (count, fitness, rmse, smallest relative margin of a nearest distance to the radius)"""
    thr = float(np.float32(max_dist * max_dist))
    with np.errstate(invalid="ignore"):
        moved = src @ T[:3, :3].T + T[:3, 3]
        d2 = np.empty(len(src))
        for a in range(0, len(src), 512):
            d2[a:a + 512] = ((moved[a:a + 512, None, :] - tgt[None, :, :]) ** 2).sum(2).min(1)
        ok = d2 < thr
        fin = np.isfinite(d2)
    k = int(ok.sum())
    margin = float((np.abs(d2[fin] - thr) / thr).min()) if fin.any() else math.inf
    if k == 0:
        return 0, 0.0, 0.0, margin
    return k, k / len(src), math.sqrt(d2[ok].sum() / k), margin


def spec_best(fitness, rmse):
    best, bf, br = -1, 0.0, 0.0
    for i in range(len(fitness)):
        if fitness[i] > bf or (fitness[i] == bf and rmse[i] < br):
            best, bf, br = i, fitness[i], rmse[i]
    return best


def spec_ransac_feature(P, max_dist, ransac_n=4, max_iteration=1000, max_validation=1000, edge=None, dist=None, angle=None,
                        seed=0, draws=None):
    """the serial loop of RegistrationRANSACBasedOnFeatureMatching on the pair table P["pair_tgt"]"""
    trials = max_iteration if draws is None else min(max_iteration, len(np.asarray(draws).reshape(-1, ransac_n)))
    if max_validation <= 0:
        trials = 0
    verdicts, passed, Ts, amb = [], [], [], False
    t = 0
    while t < trials and len(passed) < max_validation:
        m = min(4096, trials - t)
        v, T, a = spec_hypothesis(P, spec_draws(len(P["pair_tgt"]), ransac_n, t, m, seed, draws), edge, dist, angle)
        for i in np.flatnonzero(v == PASS):
            if len(passed) < max_validation:
                passed.append(t + int(i)); Ts.append(T[i])
        stop = passed[-1] + 1 - t if len(passed) >= max_validation else m
        verdicts.append(v[:stop]); amb = amb or bool(a[:stop].any())
        t += stop
    v = np.concatenate(verdicts) if verdicts else np.zeros(0, np.int8)
    ev = [spec_evaluate(P["src"], P["tgt"], T, max_dist) if np.isfinite(T).all() else (0, 0.0, 0.0, math.inf) for T in Ts]
    b = spec_best([e[1] for e in ev], [e[2] for e in ev])
    out = dict(n_trials=len(v), n_rejected_before=int((v == BEFORE).sum()), n_rejected_after=int((v == AFTER).sum()),
               n_validated=len(passed), validated=passed, evals=ev, ambiguous=amb,
               margin=min([e[3] for e in ev], default=math.inf), best_trial=-1, T=np.eye(4), count=0, fitness=0.0, rmse=0.0)
    if b >= 0:
        out.update(best_trial=passed[b], T=Ts[b], count=ev[b][0], fitness=ev[b][1], rmse=ev[b][2])
        # the runner-up: the best of the others must not tie with the winner
        rest = [(e[1], -e[2]) for i, e in enumerate(ev) if i != b]
        out["lead"] = (ev[b][1], -ev[b][2]) > max(rest) if rest else True
    return out


def spec_score(src, tgt, pairs, T, max_dist):
    """EvaluateRANSACBasedOnCorrespondence -> (good, fitness, rmse)"""
    with np.errstate(invalid="ignore"):
        d2 = ((src[pairs[:, 0]] @ T[:3, :3].T + T[:3, 3] - tgt[pairs[:, 1]]) ** 2).sum(1)
        ok = d2 < max_dist * max_dist
    g = int(ok.sum())
    return (g, g / len(pairs), math.sqrt(d2[ok].sum() / g)) if g else (0, 0.0, 0.0)


def spec_ransac_corres(src, tgt, pairs, max_dist, ransac_n=6, max_iteration=1000, max_validation=1000, seed=0, draws=None):
    trials = max(min(max_iteration, max_validation), 0)
    if draws is not None:
        trials = min(trials, len(np.asarray(draws).reshape(-1, ransac_n)))
    P = dict(src=src, tgt=tgt, pair_src=pairs[:, 0], pair_tgt=pairs[:, 1])
    out = dict(n_trials=trials, best_trial=-1, T=np.eye(4), count=0, fitness=0.0, rmse=0.0, ambiguous=False, lead=True)
    if trials == 0:
        return out
    v, T, amb = spec_hypothesis(P, spec_draws(len(pairs), ransac_n, 0, trials, seed, draws))
    sc = [spec_score(src, tgt, pairs, T[i], max_dist) for i in range(trials)]
    b = spec_best([s[1] for s in sc], [s[2] for s in sc])
    out["ambiguous"] = bool(amb.any())
    if b >= 0:
        rest = [(s[1], -s[2]) for i, s in enumerate(sc) if i != b]
        out.update(best_trial=b, T=T[b], count=sc[b][0], fitness=sc[b][1], rmse=sc[b][2],
                   lead=(sc[b][1], -sc[b][2]) > max(rest) if rest else True)
    return out


# ---------------------------------------------------------------------------
# inputs
# ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def golden():
    g = np.load(os.path.join(G, "ransac.npz"))
    return {k: g[k] for k in g.files}


@pytest.fixture(scope="module")
def frag3(golden):
    """every third point of the fragment pair with the fixture's pair table"""
    f = np.load(os.path.join(G, "fragments.npz"))
    P = {k: np.ascontiguousarray(f[v].astype(np.float64)[::3]) for k, v in
         (("src", "src"), ("sn", "src_normals"), ("tgt", "tgt"), ("tn", "tgt_normals"))}
    P["pair_tgt"] = golden["nn"].astype(np.int32)
    return P


def coordinate_features(P):
    """features whose exact match is the pair table (the module's docstring)"""
    assert len(np.unique(P["tgt"], axis=0)) == len(P["tgt"])
    return P["tgt"][P["pair_tgt"]].copy(), P["tgt"].copy()


def thresholds(golden):
    return dict(edge=float(golden["edge_similarity"]), dist=float(golden["distance_threshold"]), angle=float(golden["normal_angle"]))


def option(lib, ransac_n=4, max_iteration=1000, max_validation=1000, edge=None, dist=None, angle=None, **kw):
    return lib.ransac_option(ransac_n, max_iteration, max_validation, edge or 0.0, dist or 0.0, angle or 0.0, **kw)


def rel_fro(A, B):
    return float(np.linalg.norm(A - B) / np.linalg.norm(B))


def assert_rows(verdict, T, sv, sT, tol, what):
    assert np.array_equal(verdict, sv), (what, np.flatnonzero(verdict != sv)[:10])
    solved = sv != BEFORE
    assert not T[~solved].any(), what
    err = [rel_fro(T[i], sT[i]) for i in np.flatnonzero(solved) if np.isfinite(sT[i]).all()]
    print("%s: %d trials, %d solved, %d passed; max relative Frobenius %.3e" % (what, len(sv), int(solved.sum()),
                                                                             int((sv == PASS).sum()), max(err, default=0.0)))
    assert max(err, default=0.0) <= tol, what


# the seeded runs on the fixture's pair table: name -> (keywords of spec_ransac_feature); the seeds were chosen so that
# no consumed trial is ambiguous and the best validated trial leads (test_no_trial_is_ambiguous)
SEEDED = {
    "early_stop": dict(ransac_n=4, max_iteration=20000, max_validation=5, seed=11, checkers=True),
    "end_to_end": dict(ransac_n=4, max_iteration=20000, max_validation=100, seed=11, checkers=True),
    "three": dict(ransac_n=3, max_iteration=3000, max_validation=40, seed=13, checkers=True),
}
HOST_SEED, HOST_TRIALS = {3: 32, 4: 21, 5: 21, 6: 21, 7: 21, 8: 21}, 2000      # (ransac_n = 3: a repeated draw leaves two points)
COUNT_SEED, CHECKER_SEED, WINDOW_SEED, NAN_SEED, BIG = 21, 40, 7, 9, 2 ** 32 + 5
CORRES_SEED, SIX_SEED = {3: 50, 6: 31}, 2
SIX = [0, 100, 200, 300, 400, 500]


def explicit_draws(n_pairs, ransac_n, n_trials, seed):
    """the seeded draws of `seed`, each moved by a multiple of n_pairs (negative ones too): the same pairs through the
    modulo of the explicit path"""
    idx = spec_draws(n_pairs, ransac_n, 0, n_trials, seed)
    k = np.random.default_rng(seed).integers(-1000, 1000, idx.shape)
    return (idx + k * n_pairs).astype(np.int32)
_MEMO = {}


def seeded_spec(name, P, golden):
    if name not in _MEMO:
        kw = dict(SEEDED[name])
        th = thresholds(golden) if kw.pop("checkers") else {}
        _MEMO[name] = (spec_ransac_feature(P, float(golden["max_dist"]), **kw, **th), kw, th)
    return _MEMO[name]


# ---------------------------------------------------------------------------
# CPU
# ---------------------------------------------------------------------------
NEW_SYMBOLS = ["visma_icp_ransac_hypotheses", "visma_icp_ransac_hypotheses_host", "visma_icp_registration_ransac_feature_matching",
               "visma_icp_registration_ransac_correspondence"]
NEW_METHODS = ["ransac_hypotheses", "registration_ransac_feature_matching", "registration_ransac_correspondence"]


def test_symbols_and_methods(lib):
    L = lib.load()
    for name in NEW_SYMBOLS:
        assert hasattr(L, name), name
    for name in NEW_METHODS:
        assert callable(getattr(lib.Context, name, None)), name
    assert hasattr(lib, "CRansacOption") and hasattr(lib, "CRansacInfo") and callable(lib.ransac_hypotheses_host)
    o = lib.ransac_option()
    assert (o.ransac_n, o.max_iteration, o.max_validation, o.edge_length_similarity, o.distance_threshold, o.normal_angle,
            o.chunk_trials) == (4, 1000, 1000, 0.0, 0.0, 0.0, 0)
    assert [f[0] for f in lib.CRansacInfo._fields_][:5] == ["n_trials", "n_rejected_before", "n_rejected_after", "n_validated",
                                                            "best_trial"]
    assert (lib.RANSAC_PASS, lib.RANSAC_REJECTED_BEFORE, lib.RANSAC_REJECTED_AFTER) == (PASS, BEFORE, AFTER)


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
    dp, ip, bp = C.POINTER(C.c_double), C.POINTER(C.c_int32), C.POINTER(C.c_int8)
    xyz = np.random.default_rng(1).random((50, 3)); feat = np.random.default_rng(2).random((50, 33))
    idx = np.arange(50, dtype=np.int32); bad = idx.copy(); bad[7] = 50; neg = idx.copy(); neg[7] = -1; low = idx.copy(); low[7] = -2
    x, f, i_ = xyz.ctypes.data_as(dp), feat.ctypes.data_as(dp), idx.ctypes.data_as(ip)
    res = lib.CResult(); r_ = C.byref(res)
    fm = L.visma_icp_registration_ransac_feature_matching
    assert fm(None, x, 50, f, x, 50, f, 33, None, None, 0.1, None, 0, None, 0, r_, None) == INVALID
    assert fm(h, x, 0, f, x, 50, f, 33, None, None, 0.1, None, 0, None, 0, r_, None) == INVALID          # an empty cloud
    assert fm(h, x, 50, f, x, 0, f, 33, None, None, 0.1, None, 0, None, 0, r_, None) == INVALID
    assert fm(h, None, 50, f, x, 50, f, 33, None, None, 0.1, None, 0, None, 0, r_, None) == INVALID
    assert fm(h, x, 50, None, x, 50, f, 33, None, None, 0.1, None, 0, None, 0, r_, None) == INVALID
    assert fm(h, x, 50, f, x, 50, None, 33, None, None, 0.1, None, 0, None, 0, r_, None) == INVALID
    assert fm(h, x, 50, f, x, 50, f, 33, None, None, 0.1, None, 0, None, 0, None, None) == INVALID
    for dim in (0, 65, -1):
        assert fm(h, x, 50, f, x, 50, f, dim, None, None, 0.1, None, 0, None, 0, r_, None) == INVALID
    for md in (0.0, -1.0, float("nan")):
        assert fm(h, x, 50, f, x, 50, f, 33, None, None, md, None, 0, None, 0, r_, None) == INVALID      # the reference's early return
    for n in (2, 9, 0, -1):
        assert fm(h, x, 50, f, x, 50, f, 33, None, None, 0.1, C.byref(lib.ransac_option(n)), 0, None, 0, r_, None) == INVALID
    assert fm(h, x, 50, f, x, 50, f, 33, x, None, 0.1, None, 0, None, 0, r_, None) == INVALID            # normals for one cloud only
    assert fm(h, x, 50, f, x, 50, f, 33, None, None, 0.1, None, 0, None, 5, r_, None) == INVALID         # draws missing
    assert fm(h, x, 50, f, x, 50, f, 33, None, None, 0.1, C.byref(lib.ransac_option(chunk_trials=-1)), 0, None, 0, r_, None) == INVALID
    assert fm(h, x, 50, f, x, 50, f, 33, None, None, 0.1, None, 0, None, 0, r_, None) == STATE           # no HIP engine
    co = L.visma_icp_registration_ransac_correspondence
    assert co(h, x, 50, x, 50, i_, i_, 50, 0.1, 2, 10, 10, 0, None, 0, r_, None) == INVALID
    assert co(h, x, 50, x, 50, i_, i_, 50, 0.1, 9, 10, 10, 0, None, 0, r_, None) == INVALID
    assert co(h, x, 50, x, 50, i_, i_, 5, 0.1, 6, 10, 10, 0, None, 0, r_, None) == INVALID               # K < ransac_n
    assert co(h, x, 50, x, 50, i_, i_, 50, 0.0, 6, 10, 10, 0, None, 0, r_, None) == INVALID
    assert co(h, x, 50, x, 50, bad.ctypes.data_as(ip), i_, 50, 0.1, 6, 10, 10, 0, None, 0, r_, None) == INVALID
    assert co(h, x, 50, x, 50, i_, bad.ctypes.data_as(ip), 50, 0.1, 6, 10, 10, 0, None, 0, r_, None) == INVALID
    assert co(h, x, 50, x, 50, i_, neg.ctypes.data_as(ip), 50, 0.1, 6, 10, 10, 0, None, 0, r_, None) == INVALID
    assert co(h, x, 50, x, 50, None, i_, 50, 0.1, 6, 10, 10, 0, None, 0, r_, None) == INVALID
    assert co(h, x, 0, x, 50, i_, i_, 50, 0.1, 6, 10, 10, 0, None, 0, r_, None) == INVALID
    assert co(h, x, 50, x, 50, i_, i_, 50, 0.1, 6, 10, 10, 0, None, 0, None, None) == INVALID
    assert co(h, x, 50, x, 50, i_, i_, 50, 0.1, 6, 10, 10, 0, None, 0, r_, None) == STATE
    v = np.zeros(8, np.int8); T = np.zeros((8, 16))
    v_, t_ = v.ctypes.data_as(bp), T.ctypes.data_as(dp)
    hy = L.visma_icp_ransac_hypotheses
    assert hy(h, x, 50, x, 50, None, None, None, bad.ctypes.data_as(ip), 50, None, 0, None, 0, 8, v_, t_) == INVALID
    assert hy(h, x, 50, x, 50, None, None, None, low.ctypes.data_as(ip), 50, None, 0, None, 0, 8, v_, t_) == INVALID
    assert hy(h, x, 50, x, 50, None, None, bad.ctypes.data_as(ip), i_, 50, None, 0, None, 0, 8, v_, t_) == INVALID
    assert hy(h, x, 50, x, 50, None, None, None, i_, 40, None, 0, None, 0, 8, v_, t_) == INVALID        # a table needs ns entries
    assert hy(h, x, 50, x, 50, None, None, None, i_, 50, None, 0, None, -1, 8, v_, t_) == INVALID
    assert hy(h, x, 50, x, 50, None, None, None, i_, 50, None, 0, None, 0, 8, None, t_) == INVALID
    assert hy(h, x, 50, x, 50, None, None, None, i_, 50, None, 0, None, 0, 0, v_, t_) == 0              # nothing to do
    assert hy(h, x, 50, x, 50, None, None, None, neg.ctypes.data_as(ip), 50, None, 0, None, 0, 8, v_, t_) == STATE   # (-1 is legal)
    hh = L.visma_icp_ransac_hypotheses_host
    assert hh(x, 50, x, 50, None, None, None, bad.ctypes.data_as(ip), 50, None, 0, None, 0, 8, v_, t_) == INVALID
    assert hh(x, 50, x, 50, None, None, None, i_, 50, C.byref(lib.ransac_option(9)), 0, None, 0, 8, v_, t_) == INVALID
    assert hh(x, 50, x, 50, None, None, None, i_, 50, None, 0, None, 0, 8, v_, t_) == 0
    assert (v == PASS).all() and np.allclose(T.reshape(-1, 4, 4), np.eye(4), atol=1e-12)                # a cloud onto itself
    # the context still runs everything else
    hctx.set_target(xyz.astype(np.float32)); hctx.set_source(xyz.astype(np.float32))
    assert hctx.run(None, 0.1, 3, 0.0, 0.0).num_correspondences > 0


def fixture_rows(P, golden):
    """the specification on the fixture's 240 draw sets, per ransac_n: (rows, verdict parts, T, ambiguous)"""
    th = thresholds(golden)
    out = []
    for n in (3, 4, 6, 8):
        rows = np.flatnonzero(golden["draw_n"] == n)
        idx = golden["draws"][rows, :n].astype(np.int64)
        ti = P["pair_tgt"][idx]
        R, t, S = spec_umeyama(P["src"][idx], P["tgt"][ti])
        e_ok, d_ok, n_ok, amb_b, amb_a = spec_checkers(P, idx, ti, R, t, **th)
        T = np.zeros((len(rows), 4, 4)); T[:, :3, :3] = R; T[:, :3, 3] = t; T[:, 3, 3] = 1.0
        out.append((n, rows, idx, e_ok, d_ok, n_ok, T, amb_b | amb_a | (S[:, 1] < 1e-6 * S[:, 0])))
    return out


def test_specification_equals_the_reference(golden, frag3):
    """the fixture: ComputeTransformation, each checker's verdict, EvaluateRegistration, the list's score"""
    P, md = frag3, float(golden["max_dist"])
    worst_T = worst_r = 0.0
    for n, rows, idx, e_ok, d_ok, n_ok, T, amb in fixture_rows(P, golden):
        assert not amb.any(), n
        assert np.array_equal(e_ok, golden["edge"][rows] == 1), n
        assert np.array_equal(d_ok, golden["dist"][rows] == 1), n
        assert np.array_equal(n_ok, golden["normal"][rows] == 1), n
        for k, row in enumerate(rows):
            worst_T = max(worst_T, rel_fro(T[k], golden["T"][row]))
        for k, row in enumerate(rows):
            cnt, fit, rmse, margin = spec_evaluate(P["src"], P["tgt"], golden["T"][row], md)
            assert margin > AMB
            assert cnt == golden["count"][row] and fit == golden["fitness"][row], (n, row)
            worst_r = max(worst_r, abs(rmse - golden["rmse"][row]) / golden["rmse"][row])
    print("specification against the reference: T %.3e relative Frobenius, rmse %.3e relative" % (worst_T, worst_r))
    assert worst_T <= TOL_F and worst_r <= TOL_HD
    for k, s in enumerate(golden["corres_sets"]):
        g, fit, rmse = spec_score(P["src"], P["tgt"], golden["pairs"], golden["T"][s], md)
        assert fit == golden["corres_fitness"][k], k
        assert abs(rmse - golden["corres_rmse"][k]) <= TOL_HD * max(golden["corres_rmse"][k], 1e-300), k
    assert (golden["corres_fitness"] > 0).sum() >= 10


def test_no_trial_is_ambiguous(golden, frag3):
    """the fixture's draw sets (asserted above too) and every trial the seeded tests of this file consume: none within 1e-9 of
    a threshold, none with an undefined rotation; the best validated trial leads"""
    P = frag3
    th = thresholds(golden)
    bare = {k: v for k, v in P.items() if k not in ("sn", "tn")}
    K = len(P["pair_tgt"])

    def clean(Q, idx, **c):
        return not spec_hypothesis(Q, idx, **c)[2].any()
    for n in (3, 4, 5, 6, 7, 8):
        assert clean(P, spec_draws(K, n, 0, HOST_TRIALS, HOST_SEED[n]), **th), n
    assert clean(P, spec_draws(K, 4, 0, 5000, COUNT_SEED), **th)
    for c in CHECKERS:
        assert clean(P, spec_draws(K, 4, 0, 257, CHECKER_SEED), **c) and clean(bare, spec_draws(K, 4, 0, 257, CHECKER_SEED), **c), c
    assert np.array_equal(spec_draws(K, 4, 0, 257, draws=explicit_draws(K, 4, 257, CHECKER_SEED)), spec_draws(K, 4, 0, 257, CHECKER_SEED))
    assert clean(P, spec_draws(K, 4, 0, 700, WINDOW_SEED), **th) and clean(P, spec_draws(K, 4, BIG, 64, WINDOW_SEED), **th)
    assert clean(P, spec_draws(K, 4, 0, 5000, NAN_SEED), **th)
    for name in SEEDED:
        s, kw, _ = seeded_spec(name, P, golden)
        print(name, {k: s[k] for k in ("n_trials", "n_rejected_before", "n_rejected_after", "n_validated", "best_trial", "count")},
              "margin %.3e" % s["margin"])
        assert not s["ambiguous"] and s["margin"] > AMB and s["best_trial"] >= 0 and s["lead"], name
        assert s["n_validated"] == kw["max_validation"] and s["n_trials"] < kw["max_iteration"], name     # the early stop is met
    for n in (3, 6):
        s = spec_ransac_corres(P["src"], P["tgt"], golden["pairs"], float(golden["max_dist"]), n, 300, 300, seed=CORRES_SEED[n])
        assert not s["ambiguous"] and s["lead"] and s["best_trial"] >= 0, n
    s = spec_ransac_corres(P["src"], P["tgt"], golden["pairs"][SIX], float(golden["max_dist"]), 6, 50, 50, seed=SIX_SEED)
    assert not s["ambiguous"] and s["lead"] and s["best_trial"] >= 0


def test_host_entry_equals_the_specification(lib, golden, frag3):
    """visma_icp_ransac_hypotheses_host on the fixture's draw sets and on 2,000 seeded trials per ransac_n: pins the Philox
    mapping and the arithmetic the kernels share"""
    P = frag3
    th = thresholds(golden)
    for n, rows, idx, e_ok, d_ok, n_ok, T, amb in fixture_rows(P, golden):
        o = option(lib, n, **th)
        v, Tm = lib.ransac_hypotheses_host(P["src"], P["tgt"], P["pair_tgt"], o, draws=idx, n_trials=len(idx), src_normals=P["sn"],
                                           tgt_normals=P["tn"])
        sv = np.where(~e_ok, BEFORE, np.where(d_ok & n_ok, PASS, AFTER))
        sT = T.copy(); sT[~e_ok] = 0.0
        assert_rows(v, Tm, sv, sT, TOL_F, "host entry, fixture sets, ransac_n %d" % n)
        for k, row in enumerate(rows):
            if e_ok[k]:
                assert rel_fro(Tm[k], golden["T"][row]) <= TOL_F
        sv, sT, _ = spec_hypothesis(P, spec_draws(len(P["pair_tgt"]), n, 0, HOST_TRIALS, HOST_SEED[n]), **th)
        v, Tm = lib.ransac_hypotheses_host(P["src"], P["tgt"], P["pair_tgt"], o, seed=HOST_SEED[n], n_trials=HOST_TRIALS,
                                           src_normals=P["sn"], tgt_normals=P["tn"])
        assert_rows(v, Tm, sv, sT, TOL_F, "host entry, seeded, ransac_n %d" % n)
    # every checker off, no normals, a pair list with a source column, a partner missing, a window of trials
    pairs = golden["pairs"]
    o = option(lib, 6)
    Pc = dict(src=P["src"], tgt=P["tgt"], pair_src=pairs[:, 0], pair_tgt=pairs[:, 1])
    sv, sT, _ = spec_hypothesis(Pc, spec_draws(600, 6, 100, 300, 5))
    v, Tm = lib.ransac_hypotheses_host(P["src"], P["tgt"], pairs[:, 1], o, seed=5, first_trial=100, n_trials=300, pair_src=pairs[:, 0])
    assert_rows(v, Tm, sv, sT, TOL_F, "host entry, pair list")
    lone = dict(P); lone["pair_tgt"] = P["pair_tgt"].copy(); lone["pair_tgt"][::7] = -1
    sv, sT, _ = spec_hypothesis(lone, spec_draws(len(P["src"]), 4, 0, 500, 6))
    v, Tm = lib.ransac_hypotheses_host(P["src"], P["tgt"], lone["pair_tgt"], option(lib, 4), seed=6, n_trials=500)
    assert (sv == BEFORE).sum() > 100
    assert_rows(v, Tm, sv, sT, TOL_F, "host entry, rows without a partner")


    # a source point that is not finite: R = I and t = NaN, as the reference's Eigen::umeyama returns
    bad = dict(P); bad["src"] = P["src"].copy(); bad["src"][23] = np.nan
    idx = spec_draws(len(P["src"]), 4, 0, 5000, NAN_SEED)
    forced = idx[spec_hypothesis(P, idx, **th)[0] == PASS][:10].copy(); forced[:, 0] = 23
    sv, sT, amb = spec_hypothesis(bad, forced, **th)
    v, Tm = lib.ransac_hypotheses_host(bad["src"], P["tgt"], P["pair_tgt"], option(lib, 4, **th), draws=forced.astype(np.int32),
                                       n_trials=10, src_normals=P["sn"], tgt_normals=P["tn"])
    assert not amb.any() and np.array_equal(v, sv) and (sv != BEFORE).all()
    assert all(np.array_equal(T[:3, :3], np.eye(3)) and np.isnan(T[:3, 3]).all() for T in Tm)


@pytest.fixture(scope="module")
def driver_bins(lib):
    if build_shim.eigen_dir() is not None:
        build_ransac.build()
    paths = [os.path.join(HERE, "cpp", "_build", b) for b in build_ransac.BINS]
    if not all(os.path.exists(p) for p in paths):
        pytest.skip("ransac driver not prebuilt and no Eigen headers here")
    return paths


def _write_driver_input(path, P, pairs, max_dist, ransac_n, max_iteration, max_validation, th, seed):
    fs, ft = coordinate_features(P)
    with open(path, "wb") as f:
        f.write(struct.pack("<qqqqddddiiiq", len(P["src"]), len(P["tgt"]), len(pairs), fs.shape[1], max_dist, th.get("edge") or 0.0,
                            th.get("dist") or 0.0, th.get("angle") or 0.0, ransac_n, max_iteration, max_validation, seed))
        for a in (P["src"], P["sn"], P["tgt"], P["tn"], fs, ft):
            f.write(np.ascontiguousarray(a, "<f8").tobytes())
        f.write(np.ascontiguousarray(pairs, "<i4").tobytes())


def test_driver_argument_and_error_paths(golden, frag3, driver_bins, tmp_path):
    """the shim's early returns (RegistrationResult() for ransac_n < 3 or > 8, too few pairs, max_dist <= 0) and its report of
    an estimator or a checker it cannot run: before any context exists, both Eigen storage orders"""
    inp, outp = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    _write_driver_input(inp, frag3, golden["pairs"], float(golden["max_dist"]), 4, 100, 10, thresholds(golden), 3)
    for b in driver_bins:
        p = subprocess.run([b, "errors", inp, outp], capture_output=True, text=True, timeout=120)
        assert p.returncode == 0, (b, p.returncode, p.stdout, p.stderr)
        assert "unsupported" in p.stderr


# ---------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ctx(lib):
    c = lib.Context(0)
    yield c
    c.close()


def both_hypotheses(lib, ctx, P, o, normals=True, **kw):
    nk = dict(src_normals=P["sn"], tgt_normals=P["tn"]) if normals else {}
    hv, hT = lib.ransac_hypotheses_host(P["src"], P["tgt"], P["pair_tgt"], o, pair_src=P.get("pair_src"), **nk, **kw)
    gv, gT = ctx.ransac_hypotheses(P["src"], P["tgt"], P["pair_tgt"], o, pair_src=P.get("pair_src"), **nk, **kw)
    return hv, hT, gv, gT


@pytest.mark.gpu
@pytest.mark.parametrize("n_trials", [1, 63, 64, 65, 257, 5000])
def test_hypotheses_equal_the_host_entry_trial_counts(lib, ctx, golden, frag3, n_trials):
    o = option(lib, 4, **thresholds(golden))
    hv, hT, gv, gT = both_hypotheses(lib, ctx, frag3, o, seed=COUNT_SEED, n_trials=n_trials)
    assert_rows(gv, gT, hv, hT, TOL_HD, "GPU against the host entry, %d trials" % n_trials)


@pytest.mark.gpu
@pytest.mark.parametrize("ransac_n", [3, 4, 5, 6, 7, 8])
def test_hypotheses_equal_the_host_entry_every_ransac_n(lib, ctx, golden, frag3, ransac_n):
    o = option(lib, ransac_n, chunk_trials=100, **thresholds(golden))
    hv, hT, gv, gT = both_hypotheses(lib, ctx, frag3, o, seed=HOST_SEED[ransac_n], n_trials=HOST_TRIALS)
    assert_rows(gv, gT, hv, hT, TOL_HD, "ransac_n %d, chunks of 100" % ransac_n)
    if ransac_n in (3, 4, 6, 8):
        sv, sT, _ = spec_hypothesis(frag3, spec_draws(len(frag3["src"]), ransac_n, 0, HOST_TRIALS, HOST_SEED[ransac_n]), **thresholds(golden))
        assert_rows(gv, gT, sv, sT, TOL_F, "... against the specification")


CHECKERS = [dict(), dict(edge=0.9), dict(dist=0.25), dict(angle=math.radians(30.0)), dict(edge=0.9, dist=0.25, angle=math.radians(30.0))]


@pytest.mark.gpu
@pytest.mark.parametrize("explicit", [False, True])
@pytest.mark.parametrize("normals", [True, False])
@pytest.mark.parametrize("which", range(len(CHECKERS)))
def test_hypotheses_equal_the_host_entry_checkers_and_draws(lib, ctx, golden, frag3, which, normals, explicit):
    o = option(lib, 4, **CHECKERS[which])
    kw = dict(n_trials=257)
    if explicit:
        kw["draws"] = explicit_draws(len(frag3["src"]), 4, 257, CHECKER_SEED)
    else:
        kw["seed"] = CHECKER_SEED
    hv, hT, gv, gT = both_hypotheses(lib, ctx, frag3, o, normals, **kw)
    assert_rows(gv, gT, hv, hT, TOL_HD, "checkers %s, normals %s, explicit %s" % (CHECKERS[which], normals, explicit))
    if not CHECKERS[which]:
        assert (gv == PASS).all()


@pytest.mark.gpu
def test_hypotheses_first_trial_is_the_tail_of_a_longer_call(lib, ctx, golden, frag3):
    P = frag3
    o = option(lib, 4, **thresholds(golden))
    nk = dict(src_normals=P["sn"], tgt_normals=P["tn"])
    v, T = ctx.ransac_hypotheses(P["src"], P["tgt"], P["pair_tgt"], o, seed=WINDOW_SEED, n_trials=700, **nk)
    v2, T2 = ctx.ransac_hypotheses(P["src"], P["tgt"], P["pair_tgt"], o, seed=WINDOW_SEED, first_trial=443, n_trials=257, **nk)
    assert np.array_equal(v[443:], v2) and np.array_equal(T[443:], T2)
    d = explicit_draws(len(P["src"]), 4, 700, WINDOW_SEED)
    v, T = ctx.ransac_hypotheses(P["src"], P["tgt"], P["pair_tgt"], o, draws=d, n_trials=700, **nk)
    v2, T2 = ctx.ransac_hypotheses(P["src"], P["tgt"], P["pair_tgt"], o, draws=d, first_trial=443, n_trials=257, **nk)
    assert np.array_equal(v[443:], v2) and np.array_equal(T[443:], T2)
    # a trial index past 2^32 reaches the second counter word
    sv, sT, _ = spec_hypothesis(P, spec_draws(len(P["src"]), 4, BIG, 64, WINDOW_SEED), **thresholds(golden))
    v3, T3 = ctx.ransac_hypotheses(P["src"], P["tgt"], P["pair_tgt"], o, seed=WINDOW_SEED, first_trial=BIG, n_trials=64, **nk)
    assert_rows(v3, T3, sv, sT, TOL_F, "trials from 2^32 + 5")


def run_feature(lib, ctx, P, golden, kw, th, **extra):
    fs, ft = coordinate_features(P)
    kw = dict(kw)
    seed = kw.pop("seed", 0)
    o = option(lib, **kw, **th, **extra)
    return ctx.registration_ransac_feature_matching(P["src"], fs, P["tgt"], ft, float(golden["max_dist"]), o, seed=seed,
                                                    src_normals=P["sn"], tgt_normals=P["tn"])


def assert_info(info, s, what):
    assert (info.n_trials, info.n_rejected_before, info.n_rejected_after, info.n_validated, info.best_trial) == (
        s["n_trials"], s["n_rejected_before"], s["n_rejected_after"], s["n_validated"], s["best_trial"]), (what, info, s)


@pytest.mark.gpu
def test_order_and_early_stop(lib, ctx, golden, frag3):
    """all checkers on, max_validation = 5: the validated trials are the specification's first five passers whatever the
    chunking, and two runs give the same bits"""
    s, kw, th = seeded_spec("early_stop", frag3, golden)
    assert s["n_validated"] == 5 and s["n_trials"] == s["validated"][-1] + 1
    runs = []
    for extra in (dict(), dict(chunk_trials=64), dict(chunk_trials=1000), dict(chunk_trials=7),
                  dict()):
        r = run_feature(lib, ctx, frag3, golden, kw, th, **extra)
        assert_info(r.ransac, s, extra)
        runs.append(r)
    for r in runs[1:]:
        assert np.array_equal(r.transformation_, runs[0].transformation_) and r.fitness_ == runs[0].fitness_
        assert r.inlier_rmse_ == runs[0].inlier_rmse_ and r.num_correspondences == runs[0].num_correspondences
    assert rel_fro(runs[0].transformation_, s["T"]) <= TOL_F and runs[0].num_correspondences == s["count"]


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["end_to_end", "three"])
def test_feature_matching_on_the_fixture_pair_table(lib, ctx, golden, frag3, name):
    s, kw, th = seeded_spec(name, frag3, golden)
    r = run_feature(lib, ctx, frag3, golden, kw, th)
    print(name, r, r.ransac, "T vs the specification %.3e" % rel_fro(r.transformation_, s["T"]))
    assert_info(r.ransac, s, name)
    assert r.num_correspondences == s["count"] and r.fitness_ == s["fitness"]
    # (rmse: the specification sums f64 squared distances; a search that keeps them in fp32 carries 2^-24 each)
    assert rel_fro(r.transformation_, s["T"]) <= TOL_F and abs(r.inlier_rmse_ - s["rmse"]) <= 2.0 ** -23 * s["rmse"]
    # the context holds the pair and the pass at the returned pose
    si, ti, _ = ctx.get_correspondences()
    assert len(si) == r.num_correspondences
    again = ctx.run(r.transformation_, float(golden["max_dist"]), 0, 0.0, 0.0)
    assert (again.num_correspondences, again.fitness_, again.inlier_rmse_) == (r.num_correspondences, r.fitness_, r.inlier_rmse_)
    assert np.array_equal(again.transformation_, r.transformation_)


@pytest.mark.gpu
def test_feature_matching_end_to_end_on_fpfh(lib, ctx, golden, frag3):
    """FPFH from compute_fpfh, one exact match, 20,000 trials at most, 100 validations: the specification runs on the pair table
    match_features returns (the matching itself is test_fpfh_fgr.py's subject)"""
    P, md, th = dict(frag3), float(golden["max_dist"]), thresholds(golden)
    fs = ctx.compute_fpfh(P["src"], P["sn"], knn=100, radius=0.25); ft = ctx.compute_fpfh(P["tgt"], P["tn"], knn=100, radius=0.25)
    P["pair_tgt"] = ctx.match_features(ft, fs)[0]
    for seed in (51, 52, 53, 54, 55, 56):                              # the first seed whose run is free of ambiguity
        s = spec_ransac_feature(P, md, 4, 20000, 100, seed=seed, edge=th["edge"], dist=th["dist"])
        if not s["ambiguous"] and s["margin"] > AMB and s["best_trial"] >= 0 and s["lead"]:
            break
    else:
        pytest.fail("every seed met an ambiguous trial")
    print("seed %d: %s" % (seed, {k: s[k] for k in ("n_trials", "n_rejected_before", "n_rejected_after", "n_validated", "best_trial", "count")}))
    assert s["n_validated"] * len(P["src"]) * len(P["tgt"]) < 3e8
    r = ctx.registration_ransac_feature_matching(P["src"], fs, P["tgt"], ft, md, option(lib, 4, 20000, 100, th["edge"], th["dist"]),
                                                 seed=seed, src_normals=P["sn"], tgt_normals=P["tn"])
    assert_info(r.ransac, s, "FPFH")
    assert r.num_correspondences == s["count"] and r.fitness_ == s["fitness"] and rel_fro(r.transformation_, s["T"]) <= TOL_F
    again = ctx.run(r.transformation_, md, 0, 0.0, 0.0)
    assert (again.num_correspondences, again.fitness_, again.inlier_rmse_) == (r.num_correspondences, r.fitness_, r.inlier_rmse_)


@pytest.mark.gpu
def test_correspondence_variant(lib, ctx, golden, frag3):
    P, md = frag3, float(golden["max_dist"])
    pairs = golden["pairs"]
    for n in (3, 6):
        s = spec_ransac_corres(P["src"], P["tgt"], pairs, md, n, 300, 300, seed=CORRES_SEED[n])
        r = ctx.registration_ransac_correspondence(P["src"], P["tgt"], pairs, md, n, 300, 1000, seed=CORRES_SEED[n])
        print("correspondences, ransac_n %d: %s %s" % (n, r, r.ransac))
        assert (r.ransac.n_trials, r.ransac.n_validated, r.ransac.best_trial) == (300, 300, s["best_trial"])
        assert r.fitness_ == s["fitness"] and r.num_correspondences == s["count"]
        assert abs(r.inlier_rmse_ - s["rmse"]) <= TOL_HD * s["rmse"] and rel_fro(r.transformation_, s["T"]) <= TOL_F
        r2 = ctx.registration_ransac_correspondence(P["src"], P["tgt"], pairs, md, n, 300, 1000, seed=CORRES_SEED[n])
        assert np.array_equal(r.transformation_, r2.transformation_) and r.inlier_rmse_ == r2.inlier_rmse_
    # K == ransac_n: every trial draws from the same six pairs
    six = pairs[SIX]
    s = spec_ransac_corres(P["src"], P["tgt"], six, md, 6, 50, 50, seed=SIX_SEED)
    r = ctx.registration_ransac_correspondence(P["src"], P["tgt"], six, md, 6, 50, 50, seed=SIX_SEED)
    assert r.ransac.best_trial == s["best_trial"] and r.fitness_ == s["fitness"] and abs(r.inlier_rmse_ - s["rmse"]) <= TOL_HD * s["rmse"]


def cross_checked(ctx, fs, ft):
    """step 2 of fast global registration's matching: (i, j) with nn(i) == j and nn(j) == i, ascending i"""
    t_of_s = ctx.match_features(ft, fs)[0]; s_of_t = ctx.match_features(fs, ft)[0]
    i = np.arange(len(fs))
    keep = (t_of_s >= 0) & (s_of_t[np.maximum(t_of_s, 0)] == i)
    return np.stack([i[keep], t_of_s[keep]], 1).astype(np.int32)


@pytest.mark.gpu
def test_correspondence_variant_on_the_cross_checked_list(lib, ctx, golden, frag3):
    """FGR's cross-checked list of the FPFH matches as the pair list"""
    P, md = frag3, float(golden["max_dist"])
    fs = ctx.compute_fpfh(P["src"], P["sn"], knn=100, radius=0.25); ft = ctx.compute_fpfh(P["tgt"], P["tn"], knn=100, radius=0.25)
    cc = cross_checked(ctx, fs, ft)
    assert len(cc) >= 50, len(cc)
    # (three draws among K pairs repeat one with probability 3 / K, and two points define no rotation: few trials for
    #  ransac_n = 3, so that a seed without such a trial exists among the sixteen)
    for n, trials in ((3, 40), (6, 200)):
        why = []
        for seed in range(71, 87):                                    # the first seed whose run is free of ambiguity
            s = spec_ransac_corres(P["src"], P["tgt"], cc, md, n, trials, trials, seed=seed)
            if not s["ambiguous"] and s["best_trial"] >= 0 and s["lead"]:
                break
            why.append((seed, s["ambiguous"], s["best_trial"], s["lead"]))
        else:
            pytest.fail("every seed met an ambiguous trial: %d pairs, %s" % (len(cc), why))
        r = ctx.registration_ransac_correspondence(P["src"], P["tgt"], cc, md, n, trials, trials, seed=seed)
        print("cross-checked list, %d pairs, ransac_n %d, seed %d: %s %s" % (len(cc), n, seed, r, r.ransac))
        assert (r.ransac.n_trials, r.ransac.n_validated, r.ransac.best_trial) == (trials, trials, s["best_trial"])
        assert r.fitness_ == s["fitness"] and r.num_correspondences == s["count"]
        assert abs(r.inlier_rmse_ - s["rmse"]) <= TOL_HD * s["rmse"] and rel_fro(r.transformation_, s["T"]) <= TOL_F


@pytest.mark.gpu
def test_correspondence_scores_equal_the_reference(lib, ctx, golden, frag3):
    """the 20 stored transforms: one trial whose draws are the stored set (its pairs are entries of the list) solves that T
    and scores the 600 pairs as EvaluateRANSACBasedOnCorrespondence did in the compiled reference"""
    P, md = frag3, float(golden["max_dist"])
    pairs = golden["pairs"]
    seen = 0
    for k, sset in enumerate(golden["corres_sets"]):
        n = int(golden["draw_n"][sset])
        rows = golden["draws"][sset, :n]
        assert (rows % 2 == 0).all() and (rows < 1200).all()
        r = ctx.registration_ransac_correspondence(P["src"], P["tgt"], pairs, md, n, 1, 1, draws=(rows // 2).astype(np.int32)[None])
        assert (r.ransac.n_trials, r.ransac.n_validated) == (1, 1)
        assert r.fitness_ == golden["corres_fitness"][k], k
        if r.fitness_ > 0:
            seen += 1
            assert r.ransac.best_trial == 0 and rel_fro(r.transformation_, golden["T"][sset]) <= TOL_F
            assert abs(r.inlier_rmse_ - golden["corres_rmse"][k]) <= TOL_HD * golden["corres_rmse"][k], k
        else:
            assert r.ransac.best_trial == -1 and np.array_equal(r.transformation_, np.eye(4))
    assert seen >= 10


@pytest.mark.gpu
def test_edges(lib, ctx, golden):
    rng = np.random.default_rng(5)
    # ns = nt = 3: one triangle onto its moved copy
    tri = rng.random((3, 3)); moved = tri + [0.5, 0.0, -0.25]
    d = np.array([[2, 0, 1]], np.int32)                              # (one trial: three equal fitnesses would tie on rounding)
    r = ctx.registration_ransac_feature_matching(tri, tri, moved, tri, 0.1, option(lib, 3, 50, 50, edge=0.9), draws=d)
    s = spec_ransac_feature(dict(src=tri, tgt=moved, pair_tgt=np.arange(3, dtype=np.int32)), 0.1, 3, 50, 50, edge=0.9, draws=d)
    assert_info(r.ransac, s, "3 x 3")
    assert s["best_trial"] == 0 and r.num_correspondences == s["count"] == 3 and rel_fro(r.transformation_, s["T"]) <= TOL_F
    # nt = 1: every target edge has length 0 -- the edge checker rejects every trial with two different source points
    one = moved[:1]
    src = rng.random((40, 3))
    P1 = dict(src=src, tgt=one, pair_tgt=np.zeros(40, np.int32))
    r = ctx.registration_ransac_feature_matching(src, src, one, one, 0.1, option(lib, 3, 200, 50, edge=0.9), seed=2)
    s = spec_ransac_feature(P1, 0.1, 3, 200, 50, edge=0.9, seed=2)
    assert_info(r.ransac, s, "nt = 1, edge on")
    assert r.ransac.n_validated == 0 and r.ransac.best_trial == -1 and r.fitness_ == 0 and r.inlier_rmse_ == 0
    assert np.array_equal(r.transformation_, np.eye(4))
    r = ctx.registration_ransac_feature_matching(src, src, one, one, 0.1, option(lib, 3, 200, 50), seed=2)
    assert r.ransac.n_validated == 50 and r.ransac.n_trials == 50
    # max_validation = 0, max_iteration = 0
    for o in (option(lib, 3, 200, 0), option(lib, 3, 0, 50)):
        r = ctx.registration_ransac_feature_matching(src, src, one, one, 0.1, o, seed=2)
        assert (r.ransac.n_trials, r.ransac.n_validated, r.ransac.best_trial) == (0, 0, -1) and np.array_equal(r.transformation_, np.eye(4))
    r = ctx.registration_ransac_correspondence(src, src, np.stack([np.arange(40)] * 2, 1), 0.1, 3, 0, 10)
    assert r.ransac.n_trials == 0 and r.ransac.best_trial == -1 and np.array_equal(r.transformation_, np.eye(4))
    # all trials rejected: a distance threshold nothing meets
    tgt = rng.random((40, 3))
    r = ctx.registration_ransac_feature_matching(src, src, tgt, rng.random((40, 3)), 0.1, option(lib, 4, 300, 50, dist=1e-9), seed=3)
    assert (r.ransac.n_trials, r.ransac.n_rejected_after, r.ransac.n_validated, r.ransac.best_trial) == (300, 300, 0, -1)
    assert r.fitness_ == 0 and np.array_equal(r.transformation_, np.eye(4))


@pytest.mark.gpu
def test_nan_feature_row_and_nan_source_point(lib, ctx, golden, frag3):
    P, md, th = frag3, float(golden["max_dist"]), thresholds(golden)
    fs, ft = coordinate_features(P)
    kw = dict(SEEDED["early_stop"]); kw.pop("checkers"); seed = kw.pop("seed")
    # a source feature row of NaN: no partner, every trial that draws it is rejected before alignment
    fn = fs.copy(); fn[17] = np.nan
    Pn = dict(P); Pn["pair_tgt"] = P["pair_tgt"].copy(); Pn["pair_tgt"][17] = -1
    s = spec_ransac_feature(Pn, md, seed=seed, **kw, **th)
    assert not s["ambiguous"] and s["margin"] > AMB and s["best_trial"] >= 0 and s["lead"]
    r = ctx.registration_ransac_feature_matching(P["src"], fn, P["tgt"], ft, md, option(lib, **kw, **th), seed=seed,
                                                 src_normals=P["sn"], tgt_normals=P["tn"])
    assert_info(r.ransac, s, "a NaN feature row")
    assert r.num_correspondences == s["count"]
    # one NaN source point: a comparison with a NaN is false, so the point passes every check it takes part in (as in the
    # reference); every trial that does not draw it keeps its row
    bad = P["src"].copy(); bad[23] = np.nan
    Pb = dict(P); Pb["src"] = bad
    o = option(lib, 4, **th)
    nk = dict(src_normals=P["sn"], tgt_normals=P["tn"])
    idx = spec_draws(len(bad), 4, 0, 5000, NAN_SEED)
    v0, T0 = ctx.ransac_hypotheses(P["src"], P["tgt"], P["pair_tgt"], o, seed=NAN_SEED, n_trials=5000, **nk)
    v1, T1 = ctx.ransac_hypotheses(bad, P["tgt"], P["pair_tgt"], o, seed=NAN_SEED, n_trials=5000, **nk)
    hit = (idx == 23).any(1)
    assert hit.sum() > 5 and np.array_equal(v0[~hit], v1[~hit]) and np.array_equal(T0[~hit], T1[~hit])
    assert np.array_equal(v1, spec_hypothesis(Pb, idx, **th)[0])
    # ten trials that passed, their first draw replaced by the NaN point.  The reference's umeyama returns R = I and t = NaN
    # for them: the edge and distance checkers pass (a NaN fails no comparison), the normal checker sees unrotated normals
    good = idx[v0 == PASS][:10]
    forced = good.copy(); forced[:, 0] = 23
    d = np.concatenate([forced, good]).astype(np.int32)
    v2, T2 = ctx.ransac_hypotheses(bad, P["tgt"], P["pair_tgt"], o, draws=d, n_trials=20, **nk)
    sv, sT, amb = spec_hypothesis(Pb, d.astype(np.int64), **th)
    assert len(good) == 10 and not amb.any() and np.array_equal(v2, sv) and (v2[10:] == PASS).all()
    assert np.array_equal(T2[10:], T0[v0 == PASS][:10])
    assert all(np.array_equal(T[:3, :3], np.eye(3)) and np.isnan(T[:3, 3]).all() for T in T2[:10])
    # without the normal checker they pass, validate to zero correspondences and never win; nothing faults, and the NaN
    # point is nobody's correspondence
    th2 = dict(edge=th["edge"], dist=th["dist"])
    v3, T3 = ctx.ransac_hypotheses(bad, P["tgt"], P["pair_tgt"], option(lib, 4, **th2), draws=d, n_trials=20, **nk)
    assert (v3 == PASS).all() and not np.isfinite(T3[:10]).all((1, 2)).any()
    s = spec_ransac_feature(Pb, md, 4, 20, 20, draws=d, **th2)
    assert not s["ambiguous"] and s["margin"] > AMB and s["best_trial"] >= 10 and s["lead"] and all(e[0] == 0 for e in s["evals"][:10])
    r = ctx.registration_ransac_feature_matching(bad, fs, P["tgt"], ft, md, option(lib, 4, 20, 20, **th2), draws=d, **nk)
    assert_info(r.ransac, s, "a NaN source point")
    assert r.ransac.n_validated == 20
    assert r.num_correspondences == s["count"] and r.fitness_ == s["fitness"] and rel_fro(r.transformation_, s["T"]) <= TOL_F
    si, ti, _ = ctx.get_correspondences()
    assert len(si) == s["count"] and 23 not in si


def _pose_error(T, truth):
    d = T @ np.linalg.inv(truth)
    ang = math.degrees(math.acos(max(-1.0, min(1.0, (np.trace(d[:3, :3]) - 1.0) / 2.0))))
    return ang, float(np.linalg.norm(T[:3, 3] - truth[:3, 3]))


@pytest.mark.gpu
def test_ransac_finds_a_pose_icp_cannot_reach_from_the_identity(lib, ctx):
    """test_fpfh_fgr.py's case: tgt = src moved by 150 degrees about a tilted axis plus (0.7, -0.4, 0.3), every second point
    kept.  RANSAC with the edge checker at 0.9 and a distance checker lands where the specification does, and visma_icp_run
    from there on FGR's radius schedule reaches the truth within the bound the FGR test asserts."""
    f = np.load(os.path.join(G, "fragments.npz"))
    src, sn = f["src"].astype(np.float64), f["src_normals"].astype(np.float64)
    ax = np.array([0.3, 0.2, 0.9]); ax /= np.linalg.norm(ax)
    th = math.radians(150.0)
    K = np.array([[0, -ax[2], ax[1]], [ax[2], 0, -ax[0]], [-ax[1], ax[0], 0]])
    truth = np.eye(4)
    truth[:3, :3] = np.eye(3) + math.sin(th) * K + (1 - math.cos(th)) * K @ K
    truth[:3, 3] = [0.7, -0.4, 0.3]
    tgt = (src @ truth[:3, :3].T + truth[:3, 3])[::2].copy(); tn = (sn @ truth[:3, :3].T)[::2].copy()
    fs = ctx.compute_fpfh(src, sn, knn=100, radius=0.25); ft = ctx.compute_fpfh(tgt, tn, knn=100, radius=0.25)
    P = dict(src=src, tgt=tgt, sn=sn, tn=tn, pair_tgt=ctx.match_features(ft, fs)[0])
    for seed in (61, 62, 63, 64, 65, 66):
        s = spec_ransac_feature(P, 0.1, 4, 20000, 20, edge=0.9, dist=0.1, seed=seed)
        if not s["ambiguous"] and s["margin"] > AMB and s["best_trial"] >= 0 and s["lead"]:
            break
    else:
        pytest.fail("every seed met an ambiguous trial")
    ang, dt = _pose_error(s["T"], truth)
    print("RANSAC by the specification (seed %d): %.3f degrees, %.4f off the truth, %d trials, %d validated"
          % (seed, ang, dt, s["n_trials"], s["n_validated"]))
    assert ang < 5.0 and dt < 0.05
    r = ctx.registration_ransac_feature_matching(src, fs, tgt, ft, 0.1, option(lib, 4, 20000, 20, edge=0.9, dist=0.1), seed=seed)
    assert_info(r.ransac, s, "150 degrees")
    assert rel_fro(r.transformation_, s["T"]) <= TOL_F and r.num_correspondences == s["count"]
    ang, dt = _pose_error(r.transformation_, truth)
    assert ang < 5.0 and dt < 0.05
    pose = r.transformation_
    trace = []
    for radius in (0.1, 0.01, 0.002):
        pose = ctx.run(pose, radius, 60, 0.0, 0.0).transformation_
        trace.append(rel_fro(pose, truth))
    print("ICP at radii 0.1, 0.01, 0.002 from the RANSAC pose: %s (relative Frobenius to the truth)" % trace)
    assert rel_fro(pose, truth) < TOL_T


@pytest.mark.gpu
def test_shim_driver_runs_both_registrations(lib, ctx, golden, frag3, driver_bins, tmp_path):
    """cicp::RegistrationRANSACBasedOnFeatureMatching / ...BasedOnCorrespondence(seed) through the shim equal the C ABI"""
    P, md, th = frag3, float(golden["max_dist"]), thresholds(golden)
    s, kw, _ = seeded_spec("early_stop", P, golden)
    inp, outp = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    _write_driver_input(inp, P, golden["pairs"], md, kw["ransac_n"], kw["max_iteration"], kw["max_validation"], th, kw["seed"])
    rf = run_feature(lib, ctx, P, golden, kw, th)
    rc = ctx.registration_ransac_correspondence(P["src"], P["tgt"], golden["pairs"], md, kw["ransac_n"], kw["max_iteration"],
                                                kw["max_validation"], seed=kw["seed"])
    for b in driver_bins:
        p = subprocess.run([b, "run", inp, outp], capture_output=True, text=True, timeout=120)
        assert p.returncode == 0, (b, p.returncode, p.stderr)
        v = np.frombuffer(open(outp, "rb").read(), "<f8")
        assert np.array_equal(v[:16].reshape(4, 4), rf.transformation_) and (v[16], v[17], v[18]) == (
            rf.fitness_, rf.inlier_rmse_, rf.num_correspondences), b
        assert rel_fro(v[:16].reshape(4, 4), s["T"]) <= TOL_F
        assert np.array_equal(v[19:35].reshape(4, 4), rc.transformation_) and (v[35], v[36]) == (rc.fitness_, rc.inlier_rmse_), b
