"""Colored ICP (visma_amd/csrc/color_gradient.hip, colored.hip; Park, Zhou, Koltun, ICCV 2017): a colour gradient per
target point, then two rows per pair -- the point-to-plane row and a photometric row (visma_icp.h states the step).

No compiled reference has this estimator: the numpy f64 specification below, written from the cited lines of the
reference's ColoredICP.cpp, is the yardstick of every check here -- spec_gradient (brute-force neighbours sorted by
(d2, index), np.linalg.det for the guard, np.linalg.solve) and spec_pass (einsum over explicit per-pair J rows).  Pairs
come from the committed kernel specification (Oracle.k_nn_pass), the loop's solve is the oracle's k_solve_gn.
CPU: symbols, methods and argument checks, the C++ driver's host restatement against the specification, and two
identities that tie the specification to tested code.  GPU: the gradient through both callers, the statistics, the
loop, the planar case the feature exists for, the error paths.
"""
import math
import os
import struct
import subprocess
import sys

import numpy as np
import pytest

from nn_spec import spec_lists
from oracle_engine import OracleEngine
from visma_amd import _lib, synth  # noqa: F401

HERE = os.path.dirname(os.path.abspath(__file__))
G = os.path.join(HERE, "golden")
sys.path.insert(0, os.path.join(HERE, "cpp"))
import build_shim  # noqa: E402
import build_colored  # noqa: E402

TOL_T = 1e-5       # north_star: final SE(3) within 1e-5 relative Frobenius of the CPU reference (test_gpu_kernels.py)
TOL_STATS = 1e-9   # the project's bar for the trimmed, robust and generalized statistics, relative to max(|spec|, 1)
INVALID, STATE = 1, 5
LAMBDAS = [0.968, 0.0, 1.0, 0.5]
DET_GUARD = 1e-6   # Eigen.cpp:41-43


# ---------------------------------------------------------------------------
# the yardstick: the colored step in numpy
# ---------------------------------------------------------------------------
def intensity(rgb):
    """ColoredICP.cpp:94-95: (r + g + b) / 3.0 in that order"""
    c = np.asarray(rgb, np.float64)
    return ((c[:, 0] + c[:, 1]) + c[:, 2]) / 3.0


def transform(src, T):
    """p = T s in f64, row by row in the kernel's order"""
    s = np.asarray(src, np.float64)[:, :3]
    p = np.empty_like(s)
    for k in range(3):
        p[:, k] = ((T[k, 0] * s[:, 0] + T[k, 1] * s[:, 1]) + T[k, 2] * s[:, 2]) + T[k, 3]
    return p


def _have_scipy():
    try:
        import scipy.spatial  # noqa: F401
        return True
    except ImportError:
        return False


def _spec_gradient_batched(xyz, nrm, I, r, max_nn):
    """spec_gradient for all points at once (20,000 points in about a second instead of half a minute): a k-d tree
    proposes the max_nn + 8 nearest candidates per point (8 more than needed, so that rounding in ITS distances cannot
    lose a member of the list); flann's d2, the strict radius test, the (d2, index) order, the rows, np.linalg.det and
    np.linalg.solve are those of the loop below, batched.  test_batched_specification_gradient_is_the_loop ties the two."""
    from scipy.spatial import cKDTree
    n = len(xyz)
    r2 = float(np.float32(r * r))
    K = min(n, max_nn + 8)
    _, nb = cKDTree(xyz).query(xyz, k=K, distance_upper_bound=1.001 * r)
    nb = np.asarray(nb).reshape(n, K)
    valid = nb < n
    d = xyz[:, None, :] - xyz[np.where(valid, nb, 0)]
    d2 = d[..., 0] * d[..., 0]
    d2 = d2 + d[..., 1] * d[..., 1]
    d2 = d2 + d[..., 2] * d[..., 2]
    ok = valid & (d2 < r2)
    d2 = np.where(ok, d2, np.inf)
    idk = np.where(ok, nb, n)
    o = np.lexsort((idk, d2), axis=1)[:, :max_nn]
    lst = np.take_along_axis(idk, o, 1)
    okl = np.take_along_axis(ok, o, 1)
    nn = okl.sum(1)
    w = okl.copy()
    w[:, 0] = False                                        # entry 0 is skipped whatever it holds (:108)
    safe = np.where(okl, lst, 0)
    a, p, nt = xyz[safe], xyz[:, None, :], nrm[:, None, :]
    proj = a - ((a - p) * nt).sum(2)[..., None] * nt
    A = np.where(w[..., None], proj - p, 0.0)
    b = np.where(w, I[safe] - I[:, None], 0.0)
    last = (nn - 1)[:, None] * nrm
    AtA = np.einsum("kji,kjl->kil", A, A) + last[:, :, None] * last[:, None, :]
    Atb = np.einsum("kji,kj->ki", A, b)
    det = np.linalg.det(AtA)
    good = (nn >= 3) & ~(np.abs(det) < DET_GUARD) & np.isfinite(det)
    g = np.zeros((n, 3))
    if good.any():
        g[good] = np.linalg.solve(AtA[good], Atb[good][..., None])[..., 0]
    return g, np.where(nn >= 3, det, np.nan), nn.astype(np.int64)


def spec_gradient(xyz, nrm, I, r, max_nn, details=False, batched=None):
    """ColoredICP.cpp:74-137.  Neighbours by brute force: every point with flann's d2 < (double)(float)(r * r)
    (candidates pre-cut to the slab |dx| <= 1.001 r, which holds them all), sorted by (d2, index), the first max_nn kept.
    batched (None: from 4,000 finite points on, where scipy is there): the same for all points at once.
    details: also the determinant per point (NaN where the list has fewer than 3 entries) and the list lengths."""
    xyz = np.asarray(xyz, np.float64); nrm = np.asarray(nrm, np.float64); I = np.asarray(I, np.float64)
    n = len(xyz)
    r2 = float(np.float32(r * r))
    g = np.zeros((n, 3)); dets = np.full(n, np.nan); cnts = np.zeros(n, np.int64)
    if batched is None:
        batched = n >= 4000 and np.isfinite(xyz).all() and _have_scipy()
    if batched:
        g, dets, cnts = _spec_gradient_batched(xyz, nrm, I, r, max_nn)
        return (g, dets, cnts) if details else g
    ox = np.argsort(xyz[:, 0], kind="stable")
    xs = xyz[ox, 0]
    for k in range(n):
        p = xyz[k]
        lo, hi = np.searchsorted(xs, [p[0] - 1.001 * r, p[0] + 1.001 * r])
        cand = ox[lo:hi]
        d = p - xyz[cand]
        d2 = d[:, 0] * d[:, 0]
        d2 = d2 + d[:, 1] * d[:, 1]
        d2 = d2 + d[:, 2] * d[:, 2]
        m = d2 < r2
        cand, d2 = cand[m], d2[m]
        lst = cand[np.lexsort((cand, d2))[:max_nn]]
        nn = len(lst); cnts[k] = nn
        if nn < 3:
            continue
        nt = nrm[k]
        a = xyz[lst[1:]]                                   # entry 0 is skipped whatever it holds (:108)
        proj = a - ((a - p) @ nt)[:, None] * nt
        A = np.vstack([proj - p, (nn - 1) * nt])
        b = np.concatenate([I[lst[1:]] - I[k], [0.0]])
        AtA, Atb = A.T @ A, A.T @ b
        det = np.linalg.det(AtA); dets[k] = det
        if abs(det) < DET_GUARD or not np.isfinite(det):
            continue
        g[k] = np.linalg.solve(AtA, Atb)
    return (g, dets, cnts) if details else g


def colored_rows(p, q, n, g, Is, It, lam):
    """per pair: J (K, 2, 6) and r (K, 2): the geometric row, then the photometric one (ColoredICP.cpp:154-188)"""
    d = p - q
    dn = (d * n).sum(1)
    sg, sc = math.sqrt(lam), math.sqrt(1.0 - lam)
    rg = sg * dn
    pp = p - dn[:, None] * n
    rc = sc * (Is - ((g * (pp - q)).sum(1) + It))
    M = np.eye(3)[None] - n[:, :, None] * n[:, None, :]
    h = -np.einsum("ki,kij->kj", g, M)
    J = np.stack([sg * np.concatenate([np.cross(p, n), n], 1), sc * np.concatenate([np.cross(p, h), h], 1)], 1)
    return J, np.stack([rg, rc], 1), d


def colored_stats(p, q, n, g, Is, It, lam):
    """(the 38 statistics of visma_icp.h, sum r_g^2, sum r_c^2) over the pairs given"""
    J, r, d = colored_rows(p, q, n, g, Is, It, lam)
    st = np.zeros(38)
    st[0] = len(p)
    st[1] = (d * d).sum()
    st[2:23] = np.einsum("kra,krb->ab", J, J)[np.triu_indices(6)]
    st[23:29] = np.einsum("kra,kr->a", J, r)
    return st, float((r[:, 0] ** 2).sum()), float((r[:, 1] ** 2).sum())


def spec_pass(src, tgt, T, idx, tn, Is, It, grad, lam):
    """the specification over the pairs idx (< 0: none) of a pass at T"""
    v = idx >= 0
    j = idx[v]
    return colored_stats(transform(src, T)[v], np.asarray(tgt, np.float64)[j, :3], np.asarray(tn, np.float64)[j],
                         np.asarray(grad, np.float64)[j], np.asarray(Is, np.float64)[v], np.asarray(It, np.float64)[j], lam)


def spec_loop(oracle, src32, tgt32, tn, Is, It, grad, r, lam, iters, init=None):
    """RegistrationICP's loop (Registration.cpp:159-185, no stop test) over the kernel specification's pairs"""
    T = np.eye(4) if init is None else np.array(init, np.float64)
    ks = []
    for it in range(iters + 1):
        k, idx, _ = oracle.k_nn_pass(src32, tgt32, T[:3, :].astype(np.float32), np.float32(r * r), grid=True)
        ks.append(k)
        if it == iters:
            break
        st, _, _ = spec_pass(src32, tgt32, T, idx, tn, Is, It, grad, lam)
        T = oracle.k_solve_gn(st)[1] @ T
    return T, ks


def texture(x, y, w1, w2):
    """a smooth two-frequency texture in [0.05, 0.95]"""
    return (0.5 + 0.25 * np.sin(2 * np.pi * x / w1) * np.cos(2 * np.pi * 0.7 * y / w1)
            + 0.2 * np.sin(2 * np.pi * (0.6 * x + y) / w2))


def rgb_of(I):
    """colours whose intensity is I up to rounding: the three channels differ"""
    I = np.asarray(I, np.float64)
    return np.stack([0.9 * I, I, 1.1 * I], 1)


def _f32(a):
    return np.asarray(a, np.float64).astype(np.float32).astype(np.float64)


def _unit(v):
    return v / np.linalg.norm(v, axis=1, keepdims=True)


def _rand_T(rng, ang=0.2, tr=0.1):
    w = rng.standard_normal(3)
    w *= ang / np.linalg.norm(w)
    th = np.linalg.norm(w)
    K = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])
    R = np.eye(3) + np.sin(th) / th * K + (1 - np.cos(th)) / th ** 2 * K @ K
    return synth.make_T(R, rng.standard_normal(3) * tr)


# ---------------------------------------------------------------------------
# the gradient's clouds (jittered: no two distances tie -- but for `lattice`, `lattice04` and `dups`, which are there for
# the ties) and their specification, computed once
# ---------------------------------------------------------------------------
def plane_cloud(n=48, h=0.05, seed=1, lo=0.0):
    rng = np.random.default_rng(seed)
    i, j = np.meshgrid(np.arange(n), np.arange(n), indexing="ij")
    xy = (np.stack([i.ravel(), j.ravel()], 1) + rng.uniform(-0.3, 0.3, (n * n, 2))) * h + lo
    return np.concatenate([xy, np.zeros((n * n, 1))], 1)


def _grad_cloud(name):
    """-> (xyz, normals, colours, radius)"""
    if name == "plane":                                    # 48 x 48 jittered planar grid, spacing 0.05, smooth texture
        p = plane_cloud()
        return p, np.tile([0.0, 0.0, 1.0], (len(p), 1)), rgb_of(texture(p[:, 0], p[:, 1], 0.9, 2.3)), 0.4
    if name == "plane_tiny":                               # ... scaled until every determinant is below the guard
        p = plane_cloud() * 1e-4
        return p, np.tile([0.0, 0.0, 1.0], (len(p), 1)), rgb_of(texture(p[:, 0], p[:, 1], 0.9e-4, 2.3e-4)), 0.4e-4
    if name.startswith("sphere"):                          # a patch of the unit sphere, 3,000 points; sphere<n>: its first n
        rng = np.random.default_rng(7)
        th = 0.5 * np.sqrt(rng.random(3000)); ph = 2 * np.pi * rng.random(3000)
        p = np.stack([np.sin(th) * np.cos(ph), np.sin(th) * np.sin(ph), np.cos(th)], 1)
        c = rgb_of(texture(p[:, 0], p[:, 1], 0.35, 0.9))
        n = int(name[6:] or 3000)
        return p[:n], p[:n].copy(), c[:n], (0.15 if n == 3000 else 2.0)
    if name == "sparse":                                   # 200 points, many with fewer than 3 neighbours
        rng = np.random.default_rng(9)
        p = rng.random((200, 3))
        return p, _unit(rng.standard_normal((200, 3))), rng.random((200, 3)), 0.12
    if name in ("lattice", "lattice04"):                   # NOT jittered: a 32 x 32 lattice, spacing 0.0625 (every d2 exact, so
        i, j = np.meshgrid(np.arange(32), np.arange(32), indexing="ij")     # ties are exact ties); radius 0.25 / 0.4
        p = np.stack([i.ravel() * 0.0625, j.ravel() * 0.0625, np.zeros(1024)], 1)
        return p, np.tile([0.0, 0.0, 1.0], (1024, 1)), rgb_of(texture(p[:, 0], p[:, 1], 0.9, 2.3)), (0.25 if name == "lattice" else 0.4)
    if name == "dups":                                     # the plane with every 7th point once more at a lower and at a higher index
        q = plane_cloud()
        p = np.concatenate([q[::7], q, q[::7]])
        return p, np.tile([0.0, 0.0, 1.0], (len(p), 1)), rgb_of(texture(p[:, 0], p[:, 1], 0.9, 2.3)), 0.4
    raise KeyError(name)


GRAD_CLOUDS = ["plane", "sphere", "sparse", "sphere1", "sphere2", "sphere3", "sphere65", "plane_tiny", "lattice", "lattice04", "dups"]
MAX_NNS = [3, 30, 170]
_grad_cache = {}


def grad_case(name, max_nn):
    key = (name, max_nn)
    if key not in _grad_cache:
        p, n, c, r = _grad_cloud(name)
        g, dets, cnts = spec_gradient(p, n, intensity(c), r, max_nn, details=True)
        near = np.isfinite(dets) & (np.abs(np.abs(dets) / DET_GUARD - 1.0) <= 1e-6)
        _grad_cache[key] = dict(p=p, n=n, c=c, r=r, g=g, dets=dets, cnts=cnts, near=near)
    return _grad_cache[key]


@pytest.mark.parametrize("max_nn", MAX_NNS)
@pytest.mark.parametrize("name", GRAD_CLOUDS)
def test_specification_gradient_excludes_no_point_and_covers_the_zero_cases(name, max_nn):
    """The clouds are chosen so that no specification determinant lies within 1 +- 1e-6 of the guard; the cases the GPU
    test speaks of exist: lists shorter than 3, determinants below the guard, lists cut at max_nn, and solved points."""
    c = grad_case(name, max_nn)
    assert not c["near"].any()
    short = c["cnts"] < 3
    below = np.isfinite(c["dets"]) & (np.abs(c["dets"]) < DET_GUARD)
    assert not c["g"][short | below].any()
    if name == "sparse":
        assert short.sum() > 20 and (~short).sum() > 20
    if name in ("sphere1", "sphere2"):
        assert short.all()
    if name == "sphere3":
        assert (c["cnts"] == 3).all()
    if name == "plane_tiny":
        assert below.all() and not short.any()
    if name in ("plane", "sphere"):
        assert (c["cnts"] == max_nn).sum() > 0.5 * len(c["p"])          # most lists are cut at max_nn (not at the rim)
        if max_nn >= 30:
            assert (~below).all() and np.abs(c["g"]).max() > 0.1
    if name == "plane" and max_nn == 3:
        assert below.sum() > 10 and (~below).sum() > 10                  # both sides of the guard
    if name == "lattice":
        # the cut at max_nn falls inside a tie (the max_nn-th and the next distance are equal): which of the tied points
        # enters is the (d2, index) order's to say, and the gradient is of order 1, so it shows
        _, d2, cnt = spec_lists(c["p"], 2, max_nn + 1, c["r"])
        tied = (cnt == max_nn + 1) & (d2[:, max_nn - 1] == d2[:, max_nn])
        assert int(tied.sum()) == {3: 1020, 30: 888, 170: 0}[max_nn]
        assert np.abs(c["g"]).max() > 1.0
    if name == "dups":
        idx, d2, cnt = spec_lists(c["p"], 2, 3, c["r"])
        twice = idx[:, 0] != np.arange(len(idx))                         # entry 0, the one that is skipped, is a duplicate ...
        assert twice.sum() == 2 * 330 and (d2[twice, :3] == 0.0).all()   # ... and the point itself is listed: a zero row
        assert (c["cnts"] == max_nn).sum() > 0.5 * len(c["p"])


@pytest.mark.parametrize("max_nn", [3, 30])
def test_batched_specification_gradient_is_the_loop(max_nn):
    """the batched form used for the 20,000-point fixture against the per-point loop: the same lists (lengths equal,
    determinants to rounding), gradients within 1e-12 relative to max(|g|, 1) (the sums run in another order)"""
    if not _have_scipy():
        pytest.skip("no scipy here: the loop is used throughout")
    for name in ("sphere", "sparse", "plane"):
        p, n, c, r = _grad_cloud(name)
        loop = grad_case(name, max_nn)
        g, dets, cnts = spec_gradient(p, n, intensity(c), r, max_nn, details=True, batched=True)
        assert np.array_equal(cnts, loop["cnts"])
        both = np.isfinite(dets)
        assert np.array_equal(both, np.isfinite(loop["dets"]))
        assert np.allclose(dets[both], loop["dets"][both], rtol=1e-9, atol=1e-9 * DET_GUARD)     # (tiny ones cancel)
        assert np.array_equal(np.abs(dets[both]) < DET_GUARD, np.abs(loop["dets"][both]) < DET_GUARD)
        assert np.max(np.abs(g - loop["g"]) / np.maximum(np.abs(loop["g"]), 1.0)) < 1e-10


# ---------------------------------------------------------------------------
# CPU: the two identities that tie the specification to tested code
# ---------------------------------------------------------------------------
def _pairs_case(seed=5, k=3000):
    rng = np.random.default_rng(seed)
    q = rng.standard_normal((k, 3)) + np.array([0.3, -0.2, 1.0])
    p = q + rng.standard_normal((k, 3)) * 0.02
    n = _unit(rng.standard_normal((k, 3)))
    g = rng.standard_normal((k, 3)) * 3.0
    return p, q, n, g, rng.random(k), rng.random(k)


def test_lambda_one_is_the_point_to_plane_step(oracle):
    """lambda = 1: sqrt(1) times the point-to-plane rows, the photometric rows times 0 -- [2:29] are the reference's own
    JTJ / JTr of TransformationEstimationPointToPlane (the compiled oracle).  Bound 1e-12 relative to max(|.|, 1): two
    f64 sums of 3,000 terms in different orders."""
    p, q, n, g, Is, It = _pairs_case()
    st, cg, cc = colored_stats(p, q, n, g, Is, It, 1.0)
    corr = np.stack([np.arange(len(p)), np.arange(len(p))], 1)
    JTJ, JTr, r2 = oracle.jtj_jtr(p, q, corr, n)
    ref = np.concatenate([JTJ[np.triu_indices(6)], JTr])
    err = np.max(np.abs(st[2:29] - ref) / np.maximum(np.abs(ref), 1.0))
    assert err < 1e-12, err
    assert cc == 0.0 and abs(cg - r2) <= 1e-12 * r2 and st[0] == len(p)


@pytest.mark.parametrize("lam", LAMBDAS)
def test_constant_colour_gives_zero_gradient_and_zero_photometric_part(lam):
    p, n, _, r = _grad_cloud("sphere")
    p, n = p[:400], n[:400]
    I = np.full(len(p), 0.625)
    g = spec_gradient(p, n, I, 2.0, 30)
    assert not g.any()
    rng = np.random.default_rng(2)
    src = p + rng.standard_normal(p.shape) * 0.01
    idx = np.arange(len(p), dtype=np.int32)
    st, cg, cc = spec_pass(src, p, np.eye(4), idx, n, I, I, g, lam)
    geo, _, _ = spec_pass(src, p, np.eye(4), idx, n, I, I + 1.0, g, 1.0)           # the point-to-plane rows alone
    assert cc == 0.0
    assert np.allclose(st[2:29], lam * geo[2:29], rtol=1e-13, atol=1e-15)


# ---------------------------------------------------------------------------
# CPU: symbols, methods, argument checks (a context on the oracle engine: no call reaches a device)
# ---------------------------------------------------------------------------
NEW_SYMBOLS = ["visma_icp_set_source_colors_f64", "visma_icp_set_target_colors_f64", "visma_icp_prepare_colored",
               "visma_icp_get_color_gradient", "visma_icp_reduce_colored", "visma_icp_run_colored", "visma_icp_color_gradient"]
NEW_METHODS = ["set_source_colors_f64", "set_target_colors_f64", "prepare_colored", "color_gradient_of_target", "reduce_colored",
               "run_colored", "color_gradient"]


def test_symbols_and_methods(lib):
    L = lib.load()
    for name in NEW_SYMBOLS:
        assert hasattr(L, name), name
    for name in NEW_METHODS:
        assert callable(getattr(lib.Context, name, None)), name
    assert hasattr(lib, "ColoredInfo") and hasattr(lib, "CColoredInfo")


@pytest.fixture()
def hctx(lib, oracle):
    eng = OracleEngine(oracle)
    ctx = eng.context()
    ctx.engine = eng
    yield ctx
    ctx.close()


def _small_clouds():
    rng = np.random.default_rng(3)
    tgt = rng.random((300, 3)).astype(np.float32)
    src = (tgt[:200] + 0.01).astype(np.float32)
    return src, tgt, _f32(_unit(rng.standard_normal((300, 3)))), rng.random((200, 3)), rng.random((300, 3))


def test_argument_checks(lib, hctx):
    import ctypes as C
    L, h = hctx.L, hctx._h
    dp = C.POINTER(C.c_double)
    init = np.eye(4).reshape(16).copy()
    init[3] = 0.25
    res, info, st = lib.CResult(), lib.CColoredInfo(), np.zeros(38)
    ip, sp = init.ctypes.data_as(dp), st.ctypes.data_as(dp)
    src, tgt, tn, sc, tc = _small_clouds()
    scp, tcp = sc.ctypes.data_as(dp), tc.ctypes.data_as(dp)
    out = np.zeros((300, 3))
    # a context without clouds
    assert L.visma_icp_set_source_colors_f64(h, scp, 200, 3) == STATE
    assert L.visma_icp_set_target_colors_f64(h, tcp, 300, 3) == STATE
    assert L.visma_icp_run_colored(h, ip, 0.1, 0.968, 5, 0.0, 0.0, C.byref(res), C.byref(info)) == STATE
    assert L.visma_icp_reduce_colored(h, 0.968, sp, C.byref(info)) == STATE
    assert L.visma_icp_prepare_colored(h, 0.2, 30) == STATE
    hctx.set_target(tgt); hctx.set_source(src)
    # NULL arguments, a wrong count or stride
    assert L.visma_icp_set_source_colors_f64(h, None, 200, 3) == INVALID
    assert L.visma_icp_set_source_colors_f64(h, scp, 199, 3) == INVALID
    assert L.visma_icp_set_source_colors_f64(h, scp, 200, 2) == INVALID
    assert L.visma_icp_set_target_colors_f64(h, None, 300, 3) == INVALID
    assert L.visma_icp_set_target_colors_f64(h, tcp, 301, 3) == INVALID
    assert L.visma_icp_set_target_colors_f64(h, tcp, 300, 2) == INVALID
    assert L.visma_icp_set_source_colors_f64(None, scp, 200, 3) == INVALID
    assert L.visma_icp_run_colored(h, ip, 0.1, 0.968, 5, 0.0, 0.0, None, C.byref(info)) == INVALID
    assert L.visma_icp_run_colored(h, None, 0.1, 0.968, 5, 0.0, 0.0, C.byref(res), C.byref(info)) == INVALID
    assert L.visma_icp_run_colored(h, ip, 0.1, 0.968, -1, 0.0, 0.0, C.byref(res), C.byref(info)) == INVALID
    assert L.visma_icp_reduce_colored(h, 0.968, None, C.byref(info)) == INVALID
    assert L.visma_icp_reduce_colored(h, 0.968, sp, None) == INVALID
    assert L.visma_icp_get_color_gradient(h, out.ctypes.data_as(dp), 299) == INVALID
    assert L.visma_icp_get_color_gradient(h, None, 300) == INVALID
    assert L.visma_icp_get_color_gradient(h, out.ctypes.data_as(dp), 300) == STATE          # no gradient yet
    # max_nn outside [3, 170], whatever else is missing
    for bad in (2, 171, 0, -1):
        assert L.visma_icp_prepare_colored(h, 0.2, bad) == INVALID
        assert L.visma_icp_color_gradient(h, out.ctypes.data_as(dp), 300, out.ctypes.data_as(dp), tcp, 0.2, bad, out.ctypes.data_as(dp)) == INVALID
    assert L.visma_icp_color_gradient(h, None, 300, out.ctypes.data_as(dp), tcp, 0.2, 30, out.ctypes.data_as(dp)) == INVALID
    assert L.visma_icp_color_gradient(h, out.ctypes.data_as(dp), 300, out.ctypes.data_as(dp), tcp, 0.2, 30, out.ctypes.data_as(dp)) == STATE   # no HIP engine
    # every missing ingredient: the run returns init (as run_gicp without normals), the pass and prepare_colored are refused
    hctx.nn_pass(np.eye(4), 0.1)
    steps = [lambda: None, lambda: hctx.set_target_normals_f64(tn), lambda: hctx.set_target_colors_f64(tc)]
    for k, setup in enumerate(steps):
        setup()
        calls = dict(hctx.engine.calls)
        assert L.visma_icp_run_colored(h, ip, 0.1, 0.968, 5, 0.0, 0.0, C.byref(res), None) == 0
        assert list(res.transformation) == list(init) and res.num_correspondences == 0 and res.iterations == 0
        assert hctx.engine.calls == calls
        assert L.visma_icp_reduce_colored(h, 0.968, sp, C.byref(info)) == STATE
        if k < 2:
            assert L.visma_icp_prepare_colored(h, 0.2, 30) == STATE
    # everything given: this engine has no colored pass, and says so
    hctx.set_source_colors_f64(sc)
    for call in (lambda: hctx.prepare_colored(0.2, 30), lambda: hctx.run_colored(None, 0.1, 0.968, max_iter=5)):
        with pytest.raises(lib.IcpError) as e:
            call()
        assert e.value.code == STATE and "not supported" in str(e.value)
    with pytest.raises(lib.IcpError) as e:
        hctx.reduce_colored(0.968)                           # (no gradient)
    assert e.value.code == STATE
    # a radius that is not positive returns init as every run does
    assert L.visma_icp_run_colored(h, ip, 0.0, 0.968, 5, 0.0, 0.0, C.byref(res), C.byref(info)) == 0
    assert list(res.transformation) == list(init) and info.cost == 0.0
    # a new source drops its colours, a new target its own: the run returns init again
    hctx.set_source(src)
    assert L.visma_icp_run_colored(h, ip, 0.1, 0.968, 5, 0.0, 0.0, C.byref(res), None) == 0
    assert list(res.transformation) == list(init)
    hctx.set_source_colors_f64(sc)
    hctx.set_target(tgt); hctx.set_target_normals_f64(tn)
    assert L.visma_icp_run_colored(h, ip, 0.1, 0.968, 5, 0.0, 0.0, C.byref(res), None) == 0
    assert list(res.transformation) == list(init)
    # the context still runs everything else
    assert hctx.run(None, 0.1, 5, 0.0, 0.0).num_correspondences > 0


def test_sharded_context_is_invalid(lib, hctx):
    src, tgt, tn, sc, tc = _small_clouds()
    hctx.set_target(tgt); hctx.set_source(src)
    hctx.set_target_normals_f64(tn); hctx.set_target_colors_f64(tc); hctx.set_source_colors_f64(sc)
    fn = lib.ALLREDUCE_FN(lambda user, buf, n: 0)
    hctx._keep.append(fn)
    assert hctx.L.visma_icp_set_allreduce(hctx._h, fn, None, 0, 2) == 0
    for call in (lambda: hctx.run_colored(None, 0.1, 0.968, max_iter=5), lambda: hctx.reduce_colored(0.968),
                 lambda: hctx.prepare_colored(0.2, 30)):
        with pytest.raises(lib.IcpError) as e:
            call()
        assert e.value.code == INVALID


# ---------------------------------------------------------------------------
# CPU: the C++ driver's host restatement against the specification
# ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def driver_bins(lib):
    if build_shim.eigen_dir() is not None:
        build_colored.build()
    paths = [os.path.join(HERE, "cpp", "_build", b) for b in build_colored.BINS]
    if not all(os.path.exists(p) for p in paths):
        pytest.skip("colored driver not prebuilt and no Eigen headers here")
    return paths


def _write_driver_input(path, s, t, tn, sc, tc, grad, corr, lam, r, iters):
    with open(path, "wb") as f:
        f.write(struct.pack("<qqqddii", len(s), len(t), len(corr), lam, r, iters, 0))
        for a in (s, t, tn, sc, tc, grad):
            f.write(np.ascontiguousarray(a, "<f8").tobytes())
        f.write(np.ascontiguousarray(corr, "<i4").tobytes())


def _driver_case():
    rng = np.random.default_rng(21)
    p, n, c, r = _grad_cloud("sphere")
    t, tn, tc = p[:600], n[:600], c[:600]
    g = spec_gradient(t, tn, intensity(tc), 0.3, 30)
    ti = rng.permutation(600)[:400].astype(np.int32)
    s = t[ti] + rng.standard_normal((400, 3)) * 0.004
    sc = rgb_of(np.clip(intensity(tc)[ti] + rng.standard_normal(400) * 0.02, 0, 1))
    corr = np.stack([np.arange(400, dtype=np.int32), ti], 1)
    return s, t, tn, sc, tc, g, corr


@pytest.mark.parametrize("lam,used", [(0.968, 0.968), (0.0, 0.0), (1.0, 1.0), (0.5, 0.5), (1.5, 0.968), (-0.1, 0.968),
                                      (float("nan"), 0.968), (float("inf"), 0.968)])
def test_host_restatement_equals_the_specification(oracle, driver_bins, tmp_path, lam, used):
    """cicp::TransformationEstimationForColoredICP on the host, both Eigen storage orders, against the numpy
    specification over the same pairs: the statistics and the cost (ComputeRMSE: the reference returns the SUM) within
    1e-12 relative to max(|spec|, 1) -- two f64 sums of 400 pairs in different orders --, the update against the oracle's
    solve of the specification's statistics within 1e-9 (the bound test_gicp.py gives its driver: the 6 x 6 solve
    amplifies the 1e-12).  A lambda_geometric outside [0, 1] or not finite is 0.968 (ColoredICP.cpp:54-55)."""
    s, t, tn, sc, tc, g, corr = _driver_case()
    idx = np.full(len(s), -1, np.int32); idx[corr[:, 0]] = corr[:, 1]
    ost, ocg, occ = spec_pass(s, t, np.eye(4), idx, tn, intensity(sc), intensity(tc), g, used)
    assert occ > 0.0 or used == 1.0
    ok, upd = oracle.k_solve_gn(ost)
    assert ok
    inp, outp = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    _write_driver_input(inp, s, t, tn, sc, tc, g, corr, lam, 0.0, 0)
    for b in driver_bins:
        p = subprocess.run([b, "host", inp, outp], capture_output=True, text=True, timeout=120)
        assert p.returncode == 0, (b, p.returncode, p.stderr)
        v = np.frombuffer(open(outp, "rb").read(), "<f8")
        lam_used, rmse, T, st, cost, bare_rmse, bare_T = v[0], v[1], v[2:18].reshape(4, 4), v[18:56], v[56], v[57], v[58:74].reshape(4, 4)
        assert lam_used == used, b
        serr = float(np.max(np.abs(st - ost) / np.maximum(np.abs(ost), 1.0)))
        assert serr < 1e-12, (b, serr)
        assert rmse == cost and abs(cost - (ocg + occ)) <= 1e-12 * max(ocg + occ, 1.0), b
        assert synth.rel_frobenius(T, upd) < 1e-9, b
        assert bare_rmse == 0.0 and np.array_equal(bare_T, np.eye(4)), b      # without a gradient of the target's size


# ---------------------------------------------------------------------------
# GPU 1: the gradient against spec_gradient, through both callers
# ---------------------------------------------------------------------------
def _check_gradient(got, c, what):
    ok = ~c["near"]
    assert c["near"].sum() <= 0.01 * len(c["p"])
    err = float(np.max(np.abs(got - c["g"])[ok] / np.maximum(np.abs(c["g"][ok]), 1.0))) if ok.any() else 0.0
    zero = (c["cnts"] < 3) | (np.isfinite(c["dets"]) & (np.abs(c["dets"]) < DET_GUARD))
    print("colour gradient %s: max error vs specification %.3e relative to max(|spec|, 1) (%d points, %d zero by rule, %d excluded)"
          % (what, err, len(got), int(zero.sum()), int(c["near"].sum())))
    assert np.isfinite(got).all()
    assert err < TOL_STATS
    assert not got[zero & ok].any()                          # the zero cases are exactly zero


@pytest.mark.gpu
@pytest.mark.parametrize("max_nn", MAX_NNS)
@pytest.mark.parametrize("name", GRAD_CLOUDS)
def test_gradient_standalone_against_the_specification(lib, name, max_nn):
    """visma_icp_color_gradient (host arrays in and out).  Bound: 1e-9 relative to max(|spec|, 1), the project's
    TOL_STATS; only points whose specification determinant lies within 1 +- 1e-6 of the guard are excluded (none:
    test_specification_gradient_excludes_no_point_and_covers_the_zero_cases)."""
    c = grad_case(name, max_nn)
    ctx = lib.Context(0)
    got = ctx.color_gradient(c["p"], c["n"], c["c"], c["r"], max_nn)
    ctx.close()
    _check_gradient(got, c, "%s max_nn %d, stand-alone" % (name, max_nn))


@pytest.mark.gpu
@pytest.mark.parametrize("max_nn", MAX_NNS)
@pytest.mark.parametrize("name", GRAD_CLOUDS)
def test_gradient_of_the_context_target_against_the_specification(lib, name, max_nn):
    """visma_icp_prepare_colored + visma_icp_get_color_gradient on the f64 clouds of set_clouds_f64 (the context holds
    them centred on their centroid: the gradient does not depend on the frame).  Same bound.  estimate_normals on the
    same context returns what it returned before."""
    c = grad_case(name, max_nn)
    ctx = lib.Context(0)
    before = ctx.estimate_normals(c["p"], knn=30, radius=c["r"])
    ctx.set_clouds_f64(c["p"][:1], c["p"])
    ctx.set_target_normals_f64(c["n"]); ctx.set_target_colors_f64(c["c"])
    ctx.prepare_colored(c["r"], max_nn)
    got = ctx.color_gradient_of_target()
    after = ctx.estimate_normals(c["p"], knn=30, radius=c["r"])
    ctx.close()
    _check_gradient(got, c, "%s max_nn %d, context" % (name, max_nn))
    assert np.array_equal(before, after)


@pytest.mark.gpu
def test_gradient_non_finite_colour_and_normal_reach_the_sums_only(lib):
    c = grad_case("sphere", 30)
    col, nrm = c["c"].copy(), c["n"].copy()
    col[5] = np.nan; nrm[11] = np.inf
    ctx = lib.Context(0)
    got = ctx.color_gradient(c["p"], nrm, col, c["r"], 30)
    ctx.close()
    ref = spec_gradient(c["p"], c["n"], intensity(c["c"]), c["r"], 30)
    clean = np.isfinite(got).all(1)
    assert 2500 < clean.sum() < 3000                         # the neighbourhoods of the two points are spoilt, nothing else
    touched = np.abs(got - ref).max(1) > TOL_STATS * np.maximum(np.abs(ref).max(1), 1.0)
    assert not (touched & clean).sum() > 400                 # (a NaN intensity spoils its neighbours' sums only)


# ---------------------------------------------------------------------------
# GPU 2: statistics and info against spec_pass
# ---------------------------------------------------------------------------
def _surface(rng, n, spread=1.0):
    xy = (rng.random((n, 2)) * 2 - 1) * spread
    z = 0.1 * np.sin(3.0 * xy[:, 0]) * np.cos(2.0 * xy[:, 1])
    nx = -0.3 * np.cos(3.0 * xy[:, 0]) * np.cos(2.0 * xy[:, 1]); ny = 0.2 * np.sin(3.0 * xy[:, 0]) * np.sin(2.0 * xy[:, 1])
    nrm = _unit(np.stack([nx, ny, np.ones(n)], 1))
    return np.concatenate([xy, z[:, None]], 1), nrm


_stat_cache = {}
STAT_SIZES = [(300, 2000, 1e-6), (1, 500, 0.05), (255, 2000, 0.05), (256, 2000, 0.05), (257, 2000, 0.05), (3000, 6000, 0.05),
              (20000, 20000, 0.03),
              (262145, 2000, 0.05)]   # one source position past 1,024 x 256: the grid-stride loop runs twice


def stat_case(ns, nt, radius):
    """fp32-exact clouds and normals (the fp32 passes read the fp32 copies), a source near the target, and the same
    source moved by T^-1 for the pass at a rotated T"""
    key = (ns, nt)
    if key not in _stat_cache:
        rng = np.random.default_rng(ns * 31 + nt)
        tgt, tn = _surface(rng, nt)
        tgt, tn = _f32(tgt), _f32(tn)
        ti = rng.integers(0, nt, ns)
        near = tgt[ti] + rng.standard_normal((ns, 3)) * 0.004
        if radius < 1e-3:
            near = near + 5.0                                # no pairs at all
        T = _rand_T(rng, 0.1, 0.05)
        Ti = np.linalg.inv(T)
        moved = near @ Ti[:3, :3].T + Ti[:3, 3]
        It = texture(tgt[:, 0], tgt[:, 1], 0.35, 0.9)
        Is = np.clip(texture(near[:, 0], near[:, 1], 0.35, 0.9) + rng.standard_normal(ns) * 0.01, 0, 1)
        _stat_cache[key] = dict(tgt=tgt, tn=tn, T=T, srcs={"identity": (_f32(near), np.eye(4)), "rotated": (_f32(moved), T)},
                                tc=rgb_of(It), sc=rgb_of(Is), radius=radius)
    return _stat_cache[key]


def _errors(st, info, ost, ocg, occ):
    serr = float(np.max(np.abs(st - ost) / np.maximum(np.abs(ost), 1.0)))
    cerr = max(abs(info.geometric_cost - ocg) / max(abs(ocg), 1.0), abs(info.photometric_cost - occ) / max(abs(occ), 1.0),
               abs(info.cost - (ocg + occ)) / max(abs(ocg + occ), 1.0))
    return serr, cerr


def _check_pass(ctx, src, tgt, T, idx, tn, Is, It, grad, what):
    """every lambda on the pending pass; two calls give bit-identical output; a lambda outside [0, 1] is 0.968"""
    worst = 0.0
    for lam in LAMBDAS:
        st, info = ctx.reduce_colored(lam)
        st2, info2 = ctx.reduce_colored(lam)
        ost, ocg, occ = spec_pass(src, tgt, T, idx, tn, Is, It, grad, lam)
        serr, cerr = _errors(st, info, ost, ocg, occ)
        worst = max(worst, serr, cerr)
        k = int((idx >= 0).sum())
        print("colored pass %s lambda %g: statistics vs specification %.3e, costs %.3e (K = %d, cost = %.6g + %.6g)"
              % (what, lam, serr, cerr, k, info.geometric_cost, info.photometric_cost))
        assert np.isfinite(st).all()
        assert serr < TOL_STATS and cerr < TOL_STATS
        assert st[0] == k and not st[29:].any()
        assert np.array_equal(st, st2) and (info.cost, info.geometric_cost, info.photometric_cost) == (info2.cost, info2.geometric_cost, info2.photometric_cost)
        if k == 0:
            assert not st.any() and info.cost == 0.0
    ref, iref = ctx.reduce_colored(0.968)
    for bad in (1.5, -0.25, float("nan"), float("inf")):
        st, info = ctx.reduce_colored(bad)
        assert np.array_equal(st, ref) and info.cost == iref.cost
    return worst


@pytest.mark.gpu
@pytest.mark.parametrize("ns,nt,radius", STAT_SIZES)
def test_one_pass_fp32_search_against_the_specification(lib, oracle, ns, nt, radius):
    """The fp32 search: its pairs are the kernel specification's bit for bit; the reduction reads the fp32 copies of
    points and normals, the f64 intensities and the f64 gradient the context holds (an input of the reduction like the
    normals; the gradient kernel has its own tests).  An identity T and a rotated T; every lambda.
    Bound: statistics and the three costs within 1e-9 relative to max(|spec|, 1), the project's TOL_STATS."""
    case = stat_case(ns, nt, radius)
    c = lib.Context(0)
    c.set_search_precision("f32")
    c.set_target(case["tgt"].astype(np.float32))
    c.set_target_normals_f64(case["tn"]); c.set_target_colors_f64(case["tc"])
    c.prepare_colored(2.0 * max(radius, 0.03), 30)
    grad = c.color_gradient_of_target()
    assert np.abs(grad).max() > 0.1
    for name, (src, T) in case["srcs"].items():
        src32 = src.astype(np.float32)
        c.set_source(src32); c.set_source_colors_f64(case["sc"])
        k, oidx, _ = oracle.k_nn_pass(src32, case["tgt"].astype(np.float32), T[:3, :].astype(np.float32), np.float32(radius * radius), grid=True)
        c.nn_pass(T, radius)
        assert np.array_equal(c.correspondence_index(), oidx)
        if radius < 1e-3:
            assert k == 0
        elif ns > 1:
            assert k > 0.5 * ns
        _check_pass(c, src, case["tgt"], T, oidx, case["tn"], intensity(case["sc"]), intensity(case["tc"]), grad, "fp32 %d -> %d %s" % (ns, nt, name))
    c.close()


@pytest.mark.gpu
@pytest.mark.parametrize("ns,nt,radius", STAT_SIZES)
def test_one_pass_f64_search_against_the_specification(lib, oracle, ns, nt, radius):
    """The default (exact, f64) search: the reduction reads the f64 copies, the source in the engine's own order.  The
    specification runs over the pairs the pass reports, which must be the kernel specification's but for a few in 1e4
    (near-ties and pairs at the radius are decided in f64 here, in fp32 there).  Normals that fp32 does not hold
    exactly: a reduction that read their fp32 copy would miss the bound.  Same bound."""
    case = stat_case(ns, nt, radius)
    rng = np.random.default_rng(17)
    tn = _unit(case["tn"] + rng.standard_normal(case["tn"].shape) * 1e-3)
    c = lib.Context(0)
    for name, (src, T) in case["srcs"].items():
        c.set_clouds_f64(src, case["tgt"])
        c.set_target_normals_f64(tn); c.set_target_colors_f64(case["tc"]); c.set_source_colors_f64(case["sc"])
        c.prepare_colored(2.0 * max(radius, 0.03), 30)
        grad = c.color_gradient_of_target()
        k, oidx, _ = oracle.k_nn_pass(src.astype(np.float32), case["tgt"].astype(np.float32), T[:3, :].astype(np.float32), np.float32(radius * radius), grid=True)
        c.nn_pass(T, radius)
        idx = c.correspondence_index().copy()
        assert int((idx != oidx).sum()) <= max(3, ns // 10000)
        _check_pass(c, src, case["tgt"], T, idx, tn, intensity(case["sc"]), intensity(case["tc"]), grad, "f64 %d -> %d %s" % (ns, nt, name))
    c.close()


_chair = {}


def chair(lib, name):
    """a chair fixture with fp32-exact normals from the library's estimate_normals (tests/test_normals.py pins it to the
    compiled reference; the CPU oracle takes ten times as long) and a smooth synthetic texture evaluated at the points"""
    if name not in _chair:
        g = np.load(os.path.join(G, name))
        src, tgt = g["src"].astype(np.float32), g["tgt"].astype(np.float32)
        with lib.Context(0) as nc:
            tn = _f32(nc.estimate_normals(tgt.astype(np.float64)))
        c0 = tgt.astype(np.float64).mean(0)

        def tex(p):
            q = p.astype(np.float64) - c0
            return np.clip(texture(q[:, 0] + 0.5 * q[:, 1], q[:, 2] - 0.3 * q[:, 1], 0.45, 1.1), 0, 1)
        _chair[name] = dict(src=src, tgt=tgt, tn=tn, Is=tex(src), It=tex(tgt), r=float(g["radius"]), init=np.array(g["init"], np.float64))
    return _chair[name]


@pytest.mark.gpu
def test_one_pass_in_an_offset_frame(lib, oracle):
    """The 3 m fixture: set_clouds_f64 centres both clouds, the statistics come back in the caller's frame (offset = the
    centre).  Same bound against the specification in the caller's coordinates."""
    ch = chair(lib, "chair_offset3m.npz")
    c = lib.Context(0)
    c.set_clouds_f64(ch["src"].astype(np.float64), ch["tgt"].astype(np.float64))
    c.set_target_normals_f64(ch["tn"]); c.set_target_colors_f64(rgb_of(ch["It"])); c.set_source_colors_f64(rgb_of(ch["Is"]))
    c.prepare_colored(2.0 * ch["r"], 30)
    grad = c.color_gradient_of_target()
    c.nn_pass(ch["init"], ch["r"])
    idx = c.correspondence_index().copy()
    assert (idx >= 0).sum() > 1000 and np.abs(ch["tgt"].mean(0)).max() > 1.0
    _check_pass(c, ch["src"], ch["tgt"], ch["init"], idx, ch["tn"], intensity(rgb_of(ch["Is"])), intensity(rgb_of(ch["It"])), grad, "offset frame")
    c.close()


# ---------------------------------------------------------------------------
# GPU 3: the loop against the numpy-built loop
# ---------------------------------------------------------------------------
LOOP_ITERS = 10
_loop = {}


def chair_loop(lib, oracle):
    if "chair" not in _loop:
        ch = chair(lib, "chair_5k_20k.npz")
        grad = spec_gradient(ch["tgt"].astype(np.float64), ch["tn"], ch["It"], 2.0 * ch["r"], 30)
        _loop["chair"] = (ch, grad) + spec_loop(oracle, ch["src"], ch["tgt"], ch["tn"], ch["Is"], ch["It"], grad, ch["r"], 0.968, LOOP_ITERS)
    return _loop["chair"]


@pytest.mark.gpu
def test_loop_against_the_numpy_built_loop(lib, oracle):
    """chair_5k_20k.npz with a synthetic smooth texture, 10 iterations from the identity at the fixture's radius: the
    numpy loop is spec_gradient + k_nn_pass + spec_pass + k_solve_gn.  K equal, T within TOL_T = 1e-5."""
    ch, grad, T_ref, ks = chair_loop(lib, oracle)
    c = lib.Context(0)
    c.set_search_precision("f32")                        # the kernel specification's search
    c.set_target(ch["tgt"]); c.set_source(ch["src"])
    c.set_target_normals_f64(ch["tn"]); c.set_target_colors_f64(rgb_of(ch["It"])); c.set_source_colors_f64(rgb_of(ch["Is"]))
    res = c.run_colored(None, ch["r"], 0.968, max_iter=LOOP_ITERS, rel_fitness=0.0, rel_rmse=0.0)
    gerr = float(np.max(np.abs(c.color_gradient_of_target() - grad) / np.maximum(np.abs(grad), 1.0)))
    st, info = c.reduce_colored(0.968)
    again = c.run_colored(None, ch["r"], 0.968, max_iter=LOOP_ITERS, rel_fitness=0.0, rel_rmse=0.0)
    c.close()
    err = synth.rel_frobenius(res.transformation_, T_ref)
    print("colored loop vs numpy-built loop: rel. Frobenius %.3e (K %d / %d), gradient %.3e" % (err, res.num_correspondences, ks[-1], gerr))
    assert res.iterations == LOOP_ITERS and res.nn_passes == LOOP_ITERS + 1
    assert res.num_correspondences == ks[-1]
    assert err < TOL_T
    assert gerr < TOL_STATS                               # run_colored prepared (2 r, 30) itself
    assert res.colored.cost == info.cost and res.colored.cost == res.colored.geometric_cost + res.colored.photometric_cost
    assert res.inlier_rmse_ == math.sqrt(st[1] / st[0])   # the plain rmse of the last pass
    assert np.array_equal(res.transformation_, again.transformation_) and res.colored.cost == again.colored.cost


# ---------------------------------------------------------------------------
# GPU 4: the case the feature exists for
# ---------------------------------------------------------------------------
PLANE_H, PLANE_R, PLANE_W = 0.01, 0.03, (0.12, 0.31)
PLANE_SHIFT = np.array([1.5 * PLANE_H * 0.8, 1.5 * PLANE_H * 0.6, 0.0])     # 1.5 point spacings, inside the plane
PLANE_ITERS = 30
_plane = {}


def plane_case(oracle):
    """Target: a jittered planar patch (48 x 48, spacing 0.01) with a two-frequency texture.  Source: the same plane
    sampled at other points (40 x 40), moved inside the plane by 1.5 point spacings."""
    if "case" not in _plane:
        tgt = plane_cloud(48, PLANE_H, 1).astype(np.float32)
        s0 = plane_cloud(40, PLANE_H, 2, lo=0.04)
        Is = texture(s0[:, 0], s0[:, 1], *PLANE_W)
        It = texture(tgt[:, 0].astype(np.float64), tgt[:, 1].astype(np.float64), *PLANE_W)
        src = (s0 + PLANE_SHIFT).astype(np.float32)
        tn = np.tile([0.0, 0.0, 1.0], (len(tgt), 1))
        grad = spec_gradient(tgt.astype(np.float64), tn, It, 2.0 * PLANE_R, 30)
        T_ref, ks = spec_loop(oracle, src, tgt, tn, Is, It, grad, PLANE_R, 0.968, PLANE_ITERS)
        _plane["case"] = dict(src=src, tgt=tgt, tn=tn, Is=Is, It=It, T_ref=T_ref, ks=ks)
    return _plane["case"]


def in_plane_offset(T):
    """how far the patch's middle is from where the true motion (-PLANE_SHIFT) puts it"""
    m = np.array([0.24, 0.24, 0.0])
    return float(np.linalg.norm((T[:3, :3] @ m + T[:3, 3]) - (m - PLANE_SHIFT)))


def test_the_specification_loop_removes_the_in_plane_offset(oracle):
    """CPU: the numpy loop on the planar case ends with less than a tenth of the initial in-plane offset (measured:
    4.3e-5 of 1.5e-2 after 30 iterations)."""
    pc = plane_case(oracle)
    rem, first = in_plane_offset(pc["T_ref"]), in_plane_offset(np.eye(4))
    print("planar case, specification loop: in-plane offset %.3e -> %.3e" % (first, rem))
    assert abs(first - 0.015) < 1e-12
    assert rem < 0.1 * first


@pytest.mark.gpu
def test_colored_icp_moves_along_a_textured_plane_where_point_to_plane_cannot(lib, oracle):
    pc = plane_case(oracle)
    c = lib.Context(0)
    c.set_search_precision("f32")
    c.set_target(pc["tgt"]); c.set_source(pc["src"])
    c.set_target_normals_f64(pc["tn"])
    flat = c.run_point_to_plane(None, PLANE_R, PLANE_ITERS, 0.0, 0.0)
    c.set_target_colors_f64(rgb_of(pc["It"])); c.set_source_colors_f64(rgb_of(pc["Is"]))
    res = c.run_colored(None, PLANE_R, 0.968, max_iter=PLANE_ITERS, rel_fitness=0.0, rel_rmse=0.0)
    c.close()
    err = synth.rel_frobenius(res.transformation_, pc["T_ref"])
    print("planar case: point-to-plane leaves %.3e, colored ICP %.3e (specification loop %.3e); T vs specification loop %.3e, K %d / %d"
          % (in_plane_offset(flat.transformation_), in_plane_offset(res.transformation_), in_plane_offset(pc["T_ref"]), err,
             res.num_correspondences, pc["ks"][-1]))
    # the plane leaves the 6 x 6 singular: the guard returns the identity, the offset stays where it was
    assert abs(in_plane_offset(flat.transformation_) - in_plane_offset(np.eye(4))) < 1e-9
    assert err < TOL_T and res.num_correspondences == pc["ks"][-1]
    assert in_plane_offset(res.transformation_) < 0.1 * in_plane_offset(np.eye(4))


# ---------------------------------------------------------------------------
# GPU 5: error paths and state
# ---------------------------------------------------------------------------
@pytest.mark.gpu
def test_missing_ingredients_and_dropped_gradient(lib, oracle):
    case = stat_case(255, 2000, 0.05)
    src, T = case["srcs"]["identity"]
    c = lib.Context(0)
    c.set_clouds_f64(src, case["tgt"])

    def state(call):
        with pytest.raises(lib.IcpError) as e:
            call()
        assert e.value.code == STATE

    state(lambda: c.prepare_colored(0.1, 30))                # no normals, no colours
    c.set_target_normals_f64(case["tn"])
    state(lambda: c.prepare_colored(0.1, 30))                # no colours
    c.set_target_colors_f64(case["tc"])
    state(lambda: c.color_gradient_of_target())              # no gradient yet
    c.prepare_colored(0.1, 30)
    g1 = c.color_gradient_of_target()
    c.set_source_colors_f64(case["sc"])
    state(lambda: c.reduce_colored(0.968))                   # before a pass
    c.nn_pass(T, 0.05)
    st, _ = c.reduce_colored(0.968)
    assert st[0] > 100
    for bad in (2, 171):
        with pytest.raises(lib.IcpError) as e:
            c.prepare_colored(0.1, bad)
        assert e.value.code == INVALID
    assert np.array_equal(c.color_gradient_of_target(), g1)  # a refused call leaves the gradient
    # new target colours, new target normals, a new target: each drops the gradient
    c.set_target_colors_f64(case["tc"])
    state(lambda: c.color_gradient_of_target()); state(lambda: c.reduce_colored(0.968))
    c.prepare_colored(0.1, 30)
    c.set_target_normals_f64(case["tn"])
    state(lambda: c.color_gradient_of_target())
    c.prepare_colored(0.1, 30)
    assert np.array_equal(c.color_gradient_of_target(), g1)
    c.set_clouds_f64(src, case["tgt"])
    state(lambda: c.color_gradient_of_target())
    init = np.eye(4); init[0, 3] = 0.25
    res = c.run_colored(init, 0.05, 0.968, max_iter=3)       # normals and colours went with the clouds: init comes back
    assert np.array_equal(res.transformation_, init) and res.num_correspondences == 0
    # run_colored keeps a gradient made for exactly (2 * max_dist, 30) and replaces any other
    c.set_target_normals_f64(case["tn"]); c.set_target_colors_f64(case["tc"]); c.set_source_colors_f64(case["sc"])
    c.prepare_colored(0.1, 12)
    g12 = c.color_gradient_of_target()
    c.run_colored(None, 0.05, 0.968, max_iter=1)
    assert np.array_equal(c.color_gradient_of_target(), g1) and not np.array_equal(g12, g1)
    c.close()


@pytest.mark.gpu
def test_sharded_gpu_context_is_invalid(lib):
    src, tgt, _, r = synth.make_pair(2000, 8000)
    c = lib.Context(0)
    c.set_target_shard(0, len(tgt), tgt.mean(0))
    c.set_clouds_f64(src, tgt)
    for call in (lambda: c.run_colored(None, r, 0.968, max_iter=5), lambda: c.prepare_colored(2 * r, 30)):
        with pytest.raises(lib.IcpError) as e:
            call()
        assert e.value.code == INVALID
    c.close()


@pytest.mark.gpu
def test_shim_driver_equals_the_c_abi(lib, oracle, driver_bins, tmp_path):
    """open3d::RegistrationColoredICP of the stand-alone header set against Context.run_colored on the same clouds"""
    pc = plane_case(oracle)
    s, t = pc["src"].astype(np.float64), pc["tgt"].astype(np.float64)
    c = lib.Context(0)
    c.set_clouds_f64(s, t)
    c.set_target_normals_f64(pc["tn"]); c.set_target_colors_f64(rgb_of(pc["It"])); c.set_source_colors_f64(rgb_of(pc["Is"]))
    res = c.run_colored(None, PLANE_R, 0.968, max_iter=10)
    corr = np.stack(c.get_correspondences()[:2], 1)
    c.close()
    inp, outp = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    _write_driver_input(inp, s, t, pc["tn"], rgb_of(pc["Is"]), rgb_of(pc["It"]), np.zeros_like(t), np.zeros((0, 2), np.int32), 0.968, PLANE_R, 10)
    for b in driver_bins:
        p = subprocess.run([b, "run", inp, outp], capture_output=True, text=True, timeout=300)
        assert p.returncode == 0, (b, p.returncode, p.stderr)
        raw = open(outp, "rb").read()
        T1 = np.frombuffer(raw, "<f8", 16, 0).reshape(4, 4)
        fit1, rmse1 = struct.unpack_from("<dd", raw, 128)
        (n,) = struct.unpack_from("<q", raw, 144)
        corr1 = np.frombuffer(raw, "<i4", 2 * n, 152).reshape(n, 2)
        assert np.array_equal(T1, res.transformation_) and fit1 == res.fitness_ and rmse1 == res.inlier_rmse_, b
        assert np.array_equal(corr1, corr), b
