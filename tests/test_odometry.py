"""RGB-D odometry on the GPU (visma_icp_rgbd_odometry and the calls of its stages; odometry_image.hip, odometry.hip).

The yardstick is the numpy specification tests/odometry_spec.py; tests/golden/odometry.npz (tests/golden/gen_odometry.py)
pins it to the compiled reference: every processed image bit for bit, every correspondence map equal, every J^T J, J^T r
and sum r^2 within the bound DERIVED in odometry_spec (2 (rows + 32) 2^-53 S, S the sum of the absolute forms), the pair
counts of every iteration equal, the final poses within TOL_T, the information matrix the reference's minus its
(1 + threads) I within posegraph's information_bound.  Every test prints the measured share of its bound.

Case A is 100 x 75 with 3 levels (50 x 37, 25 x 18: the floors), B is 7 x 5 with NaN-producing depths and a pixel on every
border, C has no pair at all.  Frames of other sizes come from tests/odometry_scene.py."""
import ctypes as C
import os

import numpy as np
import pytest

import odometry_scene as scene
import odometry_spec as S
from oracle_engine import OracleEngine

HERE = os.path.dirname(os.path.abspath(__file__))
INVALID, STATE = 1, 5
TOL_T = 1e-5        # a transform within 1e-5 relative Frobenius
FRAME_KEYS = ("src_gray", "src_depth", "tgt_gray", "tgt_depth", "intrinsic")


@pytest.fixture(scope="module")
def golden():
    g = np.load(os.path.join(HERE, "golden", "odometry.npz"))
    return {k: g[k] for k in g.files}


def frames_of(golden, case):
    return [golden["%s_%s" % (case, k)] for k in FRAME_KEYS]


def option_of(golden, case, iterations):
    o = golden[case + "_option"]
    return dict(iterations=list(iterations), max_depth_diff=float(o[0]), min_depth=float(o[1]), max_depth=float(o[2]))


@pytest.fixture(scope="module")
def spec_a(golden):
    """the specification's pyramids of case A, computed once, shared and left unchanged"""
    return S.prepare(*frames_of(golden, "a"), golden["a_init"], option_of(golden, "a", golden["a_iterations"]))


@pytest.fixture(scope="module")
def spec_b(golden):
    return S.prepare(*frames_of(golden, "b"), np.eye(4), option_of(golden, "b", [1]))


def rel(a, b):
    return np.linalg.norm(a - b) / np.linalg.norm(b)


def golden_image_matches(golden, case, level, name, img):
    """a level's image against the fixture: in full, or through its digest (level 0 of A: gradients and xyz)"""
    key = "%s_l%d_%s" % (case, level, name)
    if key + "_sha" in golden:
        return np.array_equal(S.image_digest(img), golden[key + "_sha"])
    want = golden[key]
    if name == "src_xyz" and want.shape[-1] == 2:                     # (the fixture holds x and y: z is the depth)
        return S.same_image(img[..., :2], want)
    return S.same_image(img, want)


def check_step(name, got, spec, want=None):
    """J^T J, J^T r and sum r^2 of `got` against the specification's (and the reference's `want`) within the derived bound;
    -> the largest share of the bound"""
    worst = 0.0
    for other in [spec] + ([want] if want is not None else []):
        for key, skey in (("JTJ", "S_JTJ"), ("JTr", "S_JTr"), ("r2", "S_r2")):
            bound = S.step_bound(spec["rows"], spec[skey])
            d = np.abs(np.asarray(got[key]) - np.asarray(other[key]))
            assert np.all(d <= bound), (name, key, float(np.max(d)), float(np.max(bound)))
            worst = max(worst, float(np.max(d / np.where(bound > 0, bound, 1.0))))
    print("%s: %d rows, largest share of the derived bound %.3g" % (name, spec["rows"], worst))
    return worst


def unpack(stats):
    JTJ = np.zeros((6, 6)); o = 2
    for a in range(6):
        for b in range(a, 6):
            JTJ[a, b] = JTJ[b, a] = stats[o]; o += 1
    return dict(K=int(round(stats[0])), r2=stats[1], JTJ=JTJ, JTr=np.array(stats[23:29]))


# ---------------------------------------------------------------------------
# CPU
# ---------------------------------------------------------------------------
NEW_SYMBOLS = ["visma_icp_rgbd_odometry", "visma_icp_odometry_prepare", "visma_icp_odometry_get_image",
               "visma_icp_odometry_correspondences", "visma_icp_odometry_step", "visma_icp_odometry_information",
               "visma_icp_odometry_option_default"]
NEW_METHODS = ["rgbd_odometry", "odometry_prepare", "odometry_image", "odometry_correspondences", "odometry_step", "odometry_information"]


def test_symbols_and_methods(lib):
    L = lib.load()
    for name in NEW_SYMBOLS:
        assert hasattr(L, name), name
    for name in NEW_METHODS:
        assert callable(getattr(lib.Context, name, None)), name
    o = lib.odometry_option()
    d = lib.COdometryOption()
    assert L.visma_icp_odometry_option_default(C.byref(d)) == 0
    assert (o.n_levels, list(o.iterations)[:3], o.max_depth_diff, o.min_depth, o.max_depth) == (3, [20, 10, 5], 0.03, 0.0, 4.0)
    assert (d.n_levels, list(d.iterations), d.max_depth_diff, d.min_depth, d.max_depth) == (3, [20, 10, 5, 0, 0, 0, 0, 0], 0.03, 0.0, 4.0)


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
    dp, fp = C.POINTER(C.c_double), C.POINTER(C.c_float)
    w, hh = 8, 6
    img = np.ones((hh, w), np.float32); pi = img.ctypes.data_as(fp)
    k = np.array([7.0, 7.0, 3.5, 2.5]); pk = k.ctypes.data_as(dp)
    T = np.eye(4).ravel().copy(); pT = T.ctypes.data_as(dp)
    oT = np.zeros(16); info = np.zeros(36); poT, pinfo = oT.ctypes.data_as(dp), info.ctypes.data_as(dp)
    opt = lib.odometry_option()
    res = lib.COdometryResult()

    def run(w=w, h_=hh, sg=pi, sd=pi, tg=pi, td=pi, k=pk, init=pT, method=1, option=opt, out=poT, ctx=h):
        return L.visma_icp_rgbd_odometry(ctx, w, h_, sg, sd, tg, td, k, init, method, C.byref(option) if option is not None else None,
                                         out, pinfo, C.byref(res))

    def prepare(w=w, h_=hh, sg=pi, k=pk, init=pT, option=opt, ctx=h):
        return L.visma_icp_odometry_prepare(ctx, w, h_, sg, pi, pi, pi, k, init, C.byref(option))

    assert run(ctx=None) == INVALID and prepare(ctx=None) == INVALID
    for name in ("sg", "sd", "tg", "td", "k", "init", "out"):
        assert run(**{name: None}) == INVALID, name
    assert prepare(sg=None) == INVALID and prepare(k=None) == INVALID and prepare(init=None) == INVALID
    for bad in (dict(w=0), dict(h_=0), dict(w=-3)):
        assert run(**bad) == INVALID and prepare(**bad) == INVALID
    for n in (0, 9, -1):
        o = lib.odometry_option(); o.n_levels = n
        assert run(option=o) == INVALID and prepare(option=o) == INVALID
    o = lib.odometry_option([1, 1, 1, 1])                            # min(8, 6) >> 3 == 0: a level without pixels
    assert run(option=o) == INVALID and prepare(option=o) == INVALID
    o = lib.odometry_option([5, -1, 5])
    assert run(option=o) == INVALID and prepare(option=o) == INVALID
    for i, bad in ((0, 0.0), (1, 0.0), (0, float("nan")), (1, float("inf"))):
        kb = k.copy(); kb[i] = bad
        assert run(k=kb.ctypes.data_as(dp)) == INVALID and prepare(k=kb.ctypes.data_as(dp)) == INVALID
    assert run(method=2) == INVALID and run(method=-1) == INVALID
    res.pairs_capacity = 4                                            # ... without room
    assert run() == INVALID
    room = np.zeros(35, np.int64); res.pairs = room.ctypes.data_as(C.POINTER(C.c_int64))
    res.pairs_capacity = 34                                           # ... with room below the schedule's 20 + 10 + 5 steps
    assert run() == INVALID
    res.pairs_capacity = 35                                           # (enough: the call gets as far as the engine)
    assert run() == STATE
    res.pairs_capacity = -1
    assert run() == INVALID
    res.pairs = None; res.pairs_capacity = 0
    # before a prepare: the call order
    stats = np.zeros(38); kk = C.c_int64(0); r2 = C.c_double(0)
    idx = np.zeros(w * hh, np.int32); out = np.zeros(3 * w * hh, np.float32)
    pidx, pout = idx.ctypes.data_as(C.POINTER(C.c_int32)), out.ctypes.data_as(fp)
    assert L.visma_icp_odometry_step(h, 0, pT, 1, stats.ctypes.data_as(dp), C.byref(kk), C.byref(r2)) == STATE
    assert L.visma_icp_odometry_correspondences(h, 0, pT, pidx, C.byref(kk)) == STATE
    assert L.visma_icp_odometry_get_image(h, 0, 0, pout) == STATE
    assert L.visma_icp_odometry_information(h, pT, pinfo, C.byref(kk)) == STATE
    # ... and what is checked before the order
    assert L.visma_icp_odometry_step(None, 0, pT, 1, stats.ctypes.data_as(dp), None, None) == INVALID
    assert L.visma_icp_odometry_step(h, 0, None, 1, stats.ctypes.data_as(dp), None, None) == INVALID
    assert L.visma_icp_odometry_step(h, 0, pT, 1, None, None, None) == INVALID
    assert L.visma_icp_odometry_step(h, 0, pT, 7, stats.ctypes.data_as(dp), None, None) == INVALID
    assert L.visma_icp_odometry_correspondences(h, 0, None, pidx, C.byref(kk)) == INVALID
    assert L.visma_icp_odometry_correspondences(h, 0, pT, pidx, None) == INVALID
    assert L.visma_icp_odometry_get_image(h, 0, 0, None) == INVALID
    assert L.visma_icp_odometry_get_image(h, 9, 0, pout) == INVALID and L.visma_icp_odometry_get_image(h, -1, 0, pout) == INVALID
    assert L.visma_icp_odometry_information(h, None, pinfo, None) == INVALID
    for level in (-1, 8, -2**31, 2**31 - 1):                          # a level no pyramid has: INVALID, resident frames or not
        assert L.visma_icp_odometry_step(h, level, pT, 1, stats.ctypes.data_as(dp), None, None) == INVALID, level
        assert L.visma_icp_odometry_correspondences(h, level, pT, pidx, C.byref(kk)) == INVALID, level
        assert L.visma_icp_odometry_get_image(h, 0, level, pout) == INVALID, level
    for level in (1, 7):                                              # one that a pyramid can have: the call order
        assert L.visma_icp_odometry_step(h, level, pT, 1, stats.ctypes.data_as(dp), None, None) == STATE, level
        assert L.visma_icp_odometry_correspondences(h, level, pT, pidx, C.byref(kk)) == STATE, level
        assert L.visma_icp_odometry_get_image(h, 0, level, pout) == STATE, level
    assert L.visma_icp_odometry_option_default(None) == INVALID
    # valid arguments reach the engine, and this one has no odometry: the call order code, nothing prepared
    assert prepare() == STATE
    assert L.visma_icp_odometry_step(h, 0, pT, 1, stats.ctypes.data_as(dp), None, None) == STATE


def test_specification_images_equal_the_reference_bit_for_bit(golden, spec_a, spec_b):
    n = 0
    for case, prep in (("a", spec_a), ("b", spec_b)):
        for l, L in enumerate(prep["levels"]):
            for name in S.WHICH:
                assert golden_image_matches(golden, case, l, name, L[name]), (case, l, name)
                n += 1
    assert [L["src_gray"].shape for L in spec_a["levels"]] == [(75, 100), (37, 50), (18, 25)]       # the floors
    assert np.isnan(spec_b["levels"][0]["src_depth"]).sum() == np.isnan(golden["b_l0_src_depth"]).sum() > 0
    print("%d images bit for bit" % n)


def test_specification_correspondences_equal_the_reference(golden, spec_a, spec_b):
    opt = spec_a["option"]
    for l, L in enumerate(spec_a["levels"]):
        idx = S.correspondences(spec_a["K"][l], golden["a_init"], L["src_depth"], L["tgt_depth"], opt["max_depth_diff"])
        assert np.array_equal(idx, golden["a_l%d_idx" % l]), l
        assert np.count_nonzero(idx >= 0) > 300
    L = spec_b["levels"][0]
    idx = S.correspondences(spec_b["K"][0], np.eye(4), L["src_depth"], L["tgt_depth"], spec_b["option"]["max_depth_diff"])
    assert np.array_equal(idx, golden["b_l0_idx"])
    on_border = [i for i in np.flatnonzero(idx >= 0) if i % 7 in (0, 6) or i // 7 in (0, 4)]
    assert 0 < np.count_nonzero(idx >= 0) < 35 and len({i % 7 for i in on_border} & {0, 6}) == 2 and len({i // 7 for i in on_border} & {0, 4}) == 2


def golden_step(golden, case, l, m, p):
    pre = "%s_l%d_m%d_%s_" % (case, l, m, p)
    return dict(JTJ=golden[pre + "JTJ"], JTr=golden[pre + "JTr"], r2=float(golden[pre + "r2"]), rows=int(golden[pre + "rows"]))


@pytest.mark.parametrize("method", [S.COLOR, S.HYBRID])
def test_specification_steps_equal_the_reference_within_the_derived_bound(golden, spec_a, spec_b, method):
    opt = spec_a["option"]
    for l, L in enumerate(spec_a["levels"]):
        for p, T in (("init", golden["a_init"]), ("final", golden["a_final"])):
            idx = S.correspondences(spec_a["K"][l], T, L["src_depth"], L["tgt_depth"], opt["max_depth_diff"])
            s = S.step_sums(L, spec_a["K"][l], T, idx, method)
            want = golden_step(golden, "a", l, method, p)
            assert s["rows"] == want["rows"] == (2 if method == S.HYBRID else 1) * s["K"]
            check_step("A level %d method %d at %s" % (l, method, p), want, s)
    L = spec_b["levels"][0]
    idx = S.correspondences(spec_b["K"][0], np.eye(4), L["src_depth"], L["tgt_depth"], spec_b["option"]["max_depth_diff"])
    s = S.step_sums(L, spec_b["K"][0], np.eye(4), idx, method)
    assert s["rows"] == int(golden["b_l0_m%d_init_rows" % method])
    check_step("B method %d" % method, golden_step(golden, "b", 0, method, "init"), s)


@pytest.fixture(scope="module")
def spec_runs(golden, spec_a):
    """the specification's two full runs of case A, once"""
    fr = frames_of(golden, "a")
    opt = spec_a["option"]
    hy = S.multiscale(spec_a, golden["a_init"], S.HYBRID, opt)
    hy_info = S.information(spec_a, hy[1], opt)
    optc = dict(opt, iterations=[int(i) for i in golden["a_color_iterations"]])
    co = S.rgbd_odometry(*fr, golden["a_init"], S.COLOR, optc)
    return dict(hybrid=hy, hybrid_info=hy_info, color=co)


def test_specification_runs_equal_the_reference(golden, spec_runs):
    ok, T, poses, counts, dets = spec_runs["hybrid"]
    assert ok and golden["a_hybrid_ok_1"] == 1 and golden["a_hybrid_ok_3"] == 1
    assert counts == golden["a_hybrid_counts"].tolist() and len(counts) == 35
    d1, d3 = rel(T, golden["a_hybrid_T_1"]), rel(T, golden["a_hybrid_T_3"])
    per_iteration = max(rel(p, q) for p, q in zip(poses, golden["a_hybrid_poses"]))
    print("hybrid: final pose %.2e from the reference (1 thread), %.2e (3 threads); the reference's own spread %.2e; per iteration at most %.2e"
          % (d1, d3, rel(golden["a_hybrid_T_1"], golden["a_hybrid_T_3"]), per_iteration))
    assert d1 <= TOL_T and d3 <= TOL_T and per_iteration <= TOL_T
    assert rel(T, scene.truth()) < 0.01                                # (it IS the motion between the frames)
    ok, T, M, ex = spec_runs["color"]
    assert ok and ex["counts"] == golden["a_color_counts"].tolist() == [5889, 6541, 6349]
    print("colour, one level, 3 iterations: final pose %.2e from the reference" % rel(T, golden["a_color_T_1"]))
    assert rel(T, golden["a_color_T_1"]) <= TOL_T and rel(T, golden["a_color_T_3"]) <= TOL_T


def test_specification_information_equals_the_reference_minus_its_identity_terms(golden, spec_runs):
    M, K, Sabs = spec_runs["hybrid_info"]
    bound = S.information_bound(K, Sabs)
    d1 = np.abs(M - (golden["a_hybrid_info_1"] - 2.0 * np.eye(6)))
    d3 = np.abs(M - (golden["a_hybrid_info_3"] - 4.0 * np.eye(6)))
    print("K = %d, largest |difference| %.3e (1 thread) %.3e (3 threads), as a share of its bound %.3g"
          % (K, d1.max(), d3.max(), max((d1 / np.where(bound > 0, bound, 1)).max(), (d3 / np.where(bound > 0, bound, 1)).max())))
    assert np.all(d1 <= bound) and np.all(d3 <= bound)
    assert golden["a_hybrid_info_1"][5, 5] == K + 2 and golden["a_hybrid_info_3"][5, 5] == K + 4         # the quirk, pinned
    assert M[5, 5] == K == 5687


def frames_c(golden):
    fr = frames_of(golden, "a")
    fr[1] = np.full_like(fr[1], 5.0)                                  # beyond max_depth: no pair
    return fr


def test_specification_reports_failure_without_pairs(golden):
    assert golden["c_ok_1"] == 0 and golden["c_ok_3"] == 0
    assert np.array_equal(golden["c_T_1"], np.eye(4)) and np.array_equal(golden["c_info_1"], np.eye(6))   # the reference: I and I
    ok, T, M, ex = S.rgbd_odometry(*frames_c(golden), np.eye(4), S.HYBRID, S.default_option())
    assert not ok and ex["counts"] == [0] and np.array_equal(T, np.eye(4)) and np.all(M == 0.0)


# ---------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ctx(lib):
    c = lib.Context(0)
    yield c
    c.close()


def lib_option(lib, opt):
    return lib.odometry_option(opt["iterations"], opt["max_depth_diff"], opt["min_depth"], opt["max_depth"])


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["a", "b"])
def test_images_correspondences_and_steps_equal_the_reference(lib, ctx, golden, spec_a, spec_b, case):
    prep = spec_a if case == "a" else spec_b
    opt = prep["option"]
    init = golden["a_init"] if case == "a" else np.eye(4)
    ctx.odometry_prepare(*frames_of(golden, case), init, lib_option(lib, opt))
    poses = [("init", init)] + ([("final", golden["a_final"])] if case == "a" else [])
    for l, L in enumerate(prep["levels"]):
        for name in S.WHICH:
            img = ctx.odometry_image(name, l)
            assert S.same_image(img, L[name]), (case, l, name, "specification")
            assert golden_image_matches(golden, case, l, name, img), (case, l, name, "reference")
        idx, K = ctx.odometry_correspondences(l, init)
        assert np.array_equal(idx, golden["%s_l%d_idx" % (case, l)]) and K == np.count_nonzero(idx >= 0)
        for method in (S.COLOR, S.HYBRID):
            for p, T in poses:
                stats, K, r2 = ctx.odometry_step(l, T, method)
                sidx = S.correspondences(prep["K"][l], T, L["src_depth"], L["tgt_depth"], opt["max_depth_diff"])
                s = S.step_sums(L, prep["K"][l], T, sidx, method)
                got = unpack(stats)
                assert K == got["K"] == s["K"] and r2 == got["r2"] and np.all(stats[29:] == 0.0)
                check_step("%s level %d method %d at %s" % (case.upper(), l, method, p), got, s, golden_step(golden, case, l, method, p))


@pytest.mark.gpu
def test_hybrid_run_information_and_repeats(lib, ctx, golden, spec_a, spec_runs):
    fr = frames_of(golden, "a")
    opt = lib_option(lib, spec_a["option"])
    r = ctx.rgbd_odometry(*fr, golden["a_init"], lib.ODOMETRY_HYBRID, opt)
    ok, T, info = r
    assert ok and r.pairs.tolist() == golden["a_hybrid_counts"].tolist()
    d1, d3 = rel(T, golden["a_hybrid_T_1"]), rel(T, golden["a_hybrid_T_3"])
    print("hybrid: final pose %.2e from the reference (1 thread), %.2e (3 threads), %.2e from the specification; the reference's own "
          "1-thread against 3-thread spread %.2e" % (d1, d3, rel(T, spec_runs["hybrid"][1]), rel(golden["a_hybrid_T_1"], golden["a_hybrid_T_3"])))
    assert d1 <= TOL_T and d3 <= TOL_T
    # the information matrix and K
    M, K, Sabs = spec_runs["hybrid_info"]
    bound = S.information_bound(K, Sabs)
    assert r.information_pairs == K == info[5, 5] == info[4, 4] == info[3, 3] and np.array_equal(info, info.T)
    for want in (M, golden["a_hybrid_info_1"] - 2.0 * np.eye(6), golden["a_hybrid_info_3"] - 4.0 * np.eye(6)):
        d = np.abs(info - want)
        print("information: largest |difference| %.3e, as a share of its bound %.3g" % (d.max(), (d / np.where(bound > 0, bound, 1)).max()))
        assert np.all(d <= bound)
    M2, K2 = ctx.odometry_information(T)
    assert K2 == K and np.array_equal(M2, info)
    # two identical calls are bit-identical; an all-zero init is the identity init
    again = ctx.rgbd_odometry(*fr, golden["a_init"], lib.ODOMETRY_HYBRID, opt)
    zero = ctx.rgbd_odometry(*fr, np.zeros((4, 4)), lib.ODOMETRY_HYBRID, opt)
    for other in (again, zero):
        assert other.success and np.array_equal(other.T, T) and np.array_equal(other.information, info)
        assert np.array_equal(other.pairs, r.pairs) and other.information_pairs == K


@pytest.mark.gpu
def test_colour_run(lib, ctx, golden, spec_a, spec_runs):
    opt = lib_option(lib, dict(spec_a["option"], iterations=[int(i) for i in golden["a_color_iterations"]]))
    r = ctx.rgbd_odometry(*frames_of(golden, "a"), golden["a_init"], lib.ODOMETRY_COLOR, opt)
    assert r.success and r.pairs.tolist() == golden["a_color_counts"].tolist()
    d1, d3 = rel(r.T, golden["a_color_T_1"]), rel(r.T, golden["a_color_T_3"])
    print("colour: final pose %.2e from the reference (1 thread), %.2e (3 threads), %.2e from the specification; the reference's own "
          "spread %.2e" % (d1, d3, rel(r.T, spec_runs["color"][1]), rel(golden["a_color_T_1"], golden["a_color_T_3"])))
    assert d1 <= TOL_T and d3 <= TOL_T
    assert r.information_pairs == golden["a_color_info_1"][5, 5] - 2


@pytest.mark.gpu
def test_no_pairs_is_no_success_and_no_error(lib, ctx, golden):
    r = ctx.rgbd_odometry(*frames_c(golden), np.eye(4), lib.ODOMETRY_HYBRID)
    assert not r.success and np.array_equal(r.T, np.eye(4)) and np.all(r.information == 0.0)
    assert r.information_pairs == 0 and r.pairs.tolist() == [0]


@pytest.mark.gpu
def test_a_level_outside_the_resident_pyramid_is_invalid(lib, ctx, golden, spec_a, spec_b):
    """after a prepare the bound is the resident pyramid's n_levels (3 for A, 1 for B), not the most a pyramid can have"""
    L, h = ctx.L, ctx._h
    dp = C.POINTER(C.c_double)
    T = np.eye(4).ravel().copy(); pT = T.ctypes.data_as(dp)
    stats = np.zeros(38); kk = C.c_int64(0)
    idx = np.zeros(100 * 75, np.int32); out = np.zeros(3 * 100 * 75, np.float32)
    pidx, pout = idx.ctypes.data_as(C.POINTER(C.c_int32)), out.ctypes.data_as(C.POINTER(C.c_float))
    for case, prep, init in (("a", spec_a, golden["a_init"]), ("b", spec_b, np.eye(4))):
        n = len(prep["levels"])
        ctx.odometry_prepare(*frames_of(golden, case), init, lib_option(lib, prep["option"]))
        for level in (-1, n, n + 1, 8):
            assert L.visma_icp_odometry_get_image(h, 0, level, pout) == INVALID, (case, level)
            assert L.visma_icp_odometry_correspondences(h, level, pT, pidx, C.byref(kk)) == INVALID, (case, level)
            for method in (0, 1):
                assert L.visma_icp_odometry_step(h, level, pT, method, stats.ctypes.data_as(dp), None, None) == INVALID, (case, level)
        for which in (-1, 9):
            assert L.visma_icp_odometry_get_image(h, which, 0, pout) == INVALID, (case, which)
        assert L.visma_icp_odometry_get_image(h, 8, n - 1, pout) == 0      # (the last level and the last image are there)
        assert L.visma_icp_odometry_correspondences(h, n - 1, pT, pidx, C.byref(kk)) == 0
    assert (len(spec_a["levels"]), len(spec_b["levels"])) == (3, 1)


@pytest.fixture(scope="module")
def big():
    """640 x 480 frames and the specification's single level of them, once"""
    fr = scene.frames(640, 480)
    opt = dict(S.default_option(), iterations=[1])
    return fr, opt, S.prepare(*fr, np.eye(4), opt)


@pytest.mark.gpu
def test_640_by_480_runs_the_grid_stride_loop_twice(lib, ctx, big):
    """307,200 pixels: above the reduction's cap of 1,024 workgroups x 256 threads, the only shape at which a thread visits
    a second pixel"""
    fr, opt, prep = big
    assert 640 * 480 > 1024 * 256
    ctx.odometry_prepare(*fr, np.eye(4), lib_option(lib, opt))
    L = prep["levels"][0]
    for name in S.WHICH:
        assert S.same_image(ctx.odometry_image(name, 0), L[name]), name
    T = scene.rigid([0.002, -0.006, 0.003], [0.007, -0.002, 0.005])
    idx, K = ctx.odometry_correspondences(0, T)
    sidx = S.correspondences(prep["K"][0], T, L["src_depth"], L["tgt_depth"], opt["max_depth_diff"])
    assert np.array_equal(idx, sidx) and K == np.count_nonzero(sidx >= 0)
    assert np.count_nonzero(sidx[1024 * 256:] >= 0) > 1000            # pairs that only a thread's second trip visits
    stats, K2, r2 = ctx.odometry_step(0, T, lib.ODOMETRY_HYBRID)
    assert K2 == K
    check_step("640 x 480 hybrid", unpack(stats), S.step_sums(L, prep["K"][0], T, sidx, S.HYBRID))


@pytest.mark.gpu
def test_a_pose_that_throws_most_projections_out(lib, ctx, golden, spec_a):
    """30 degrees about y and 2.4 m toward the scene: most projections leave the image, the sphere's pixels end up behind
    the camera (transformed depth <= 0: no pair, where the reference's cast is undefined)"""
    T = scene.rigid([0.0, np.pi / 6, 0.0], [0.0, 0.0, -2.4])
    ctx.odometry_prepare(*frames_of(golden, "a"), golden["a_init"], lib_option(lib, spec_a["option"]))
    seen_behind = seen_outside = 0
    for l, L in enumerate(spec_a["levels"]):
        idx, K = ctx.odometry_correspondences(l, T)
        assert K == np.count_nonzero(idx >= 0)
        xyz = L["src_xyz"].reshape(-1, 3).astype(np.float64)
        z = xyz @ T[2, :3] + T[2, 3]
        seen_behind += int(np.count_nonzero(z <= 0))
        sidx = S.correspondences(spec_a["K"][l], T, L["src_depth"], L["tgt_depth"], spec_a["option"]["max_depth_diff"])
        assert np.array_equal(idx, sidx), l
        h, w = L["src_depth"].shape
        Kl = spec_a["K"][l]
        with np.errstate(invalid="ignore", divide="ignore"):
            u = Kl[0, 0] * (xyz @ T[0, :3] + T[0, 3]) / z + Kl[0, 2]
        seen_outside += int(np.count_nonzero((z > 0) & ((u < -1) | (u > w))))
    assert seen_behind > 100 and seen_outside > 100
    # a wide depth tolerance at the same pose: pairs exist, and they are the specification's
    o = dict(spec_a["option"], max_depth_diff=10.0)
    ctx.odometry_prepare(*frames_of(golden, "a"), golden["a_init"], lib_option(lib, o))
    L = spec_a["levels"][0]
    idx, K = ctx.odometry_correspondences(0, T)
    sidx = S.correspondences(spec_a["K"][0], T, L["src_depth"], L["tgt_depth"], 10.0)
    assert np.array_equal(idx, sidx) and 0 < K < 7500
