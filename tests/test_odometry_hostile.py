"""RGB-D odometry on frames chosen to break it (odometry_image.hip, odometry.hip), where tests/test_odometry.py has one
well-behaved pair.  The yardsticks are those of test_odometry.py: the numpy specification tests/odometry_spec.py, pinned
to the compiled reference by tests/golden/rgbd_hostile.npz (tests/golden/gen_rgbd_hostile.py): every processed image bit
for bit, every correspondence map equal, the sums of a step within odometry_spec.step_bound, the pair counts of every
iteration equal, a pose within TOL_T, the information matrix the reference's minus its (1 + threads) I within
information_bound.  No bound is new.  The cases (tests/odometry_scene.py hostile_cases; the fixture holds results only):

  o_const          constant gray over a fronto-parallel plane, 9 x 7: every gradient is zero, both systems are singular
  o_n1 .. o_n6     exactly 1 .. 6 pairs (a block of depths in an image without): none can be solved
  o_v, o_v2        NaN, +inf, -inf, negative, 0, below min_depth = 0.3, 1e30 and 1e-40 in BOTH 16 x 12 frames, fx != fy, a
                   principal point off the centre; o_v runs both methods in full at one level, o_v2 has two levels (NaN
                   through the down-sampling; six pairs at level 1, and no solution).  Paired target pixels have NaN depth
                   gradients: the hybrid term's isnan -> 0 is met (the generator asserts it).
  o_1x1, o_1x5, o_5x1, o_9x7 (two levels: 4 x 3), o_deep (256 x 128, eight levels down to 2 x 1, pinned by digests)"""
import os

import numpy as np
import pytest

import odometry_scene as scene
import odometry_spec as S
import packed_npz
from test_odometry import TOL_T, check_step, golden_image_matches, golden_step, lib_option, rel, unpack
from tsdf_spec import digest

HERE = os.path.dirname(os.path.abspath(__file__))
CASES = list(scene.hostile_cases())


@pytest.fixture(scope="module")
def golden():
    return packed_npz.load(os.path.join(HERE, "golden", "rgbd_hostile.npz"))


class Memo:
    """the inputs and the specification's results of a case, computed once, shared by the CPU and GPU tests, unchanged"""

    def __init__(self):
        self.cases, self.have = scene.hostile_cases(), {}

    def case(self, name):
        """-> frames, option (the hybrid schedule), the colour schedule"""
        fr, its, itc, min_depth = self.cases[name]
        return fr, dict(S.default_option(), iterations=list(its), min_depth=min_depth), list(itc)

    def prepare(self, name):
        if name not in self.have:
            fr, opt, _ = self.case(name)
            self.have[name] = S.prepare(*fr, np.eye(4), opt)
        return self.have[name]

    def step(self, name, level, method):
        key = (name, level, method)
        if key not in self.have:
            prep = self.prepare(name)
            L = prep["levels"][level]
            idx = S.correspondences(prep["K"][level], np.eye(4), L["src_depth"], L["tgt_depth"], prep["option"]["max_depth_diff"])
            self.have[key] = (idx, S.step_sums(L, prep["K"][level], np.eye(4), idx, method))
        return self.have[key]

    def run(self, name, method):
        """-> ok, T, info, extras of the specification's full run"""
        key = (name, "run", method)
        if key not in self.have:
            fr, opt, itc = self.case(name)
            self.have[key] = S.rgbd_odometry(*fr, np.eye(4), method, opt if method == S.HYBRID else dict(opt, iterations=itc))
        return self.have[key]


@pytest.fixture(scope="module")
def spec():
    return Memo()


def idx_matches(golden, case, level, idx):
    if "%s_l%d_idx_sha" % (case, level) in golden:
        return np.array_equal(digest(idx, np.int32), golden["%s_l%d_idx_sha" % (case, level)])
    return np.array_equal(idx, golden["%s_l%d_idx" % (case, level)])


def check_run(golden, case, run, ok, T, info, counts, info_K, info_S, who):
    """a full run against the reference's: the success flag and the pairs of every iteration equal; with success the pose
    within TOL_T of the reference's with 1 and with 3 threads and the information matrix its minus (1 + threads) I within
    information_bound; without, T = I and information = 0 where the reference returns I and I"""
    assert bool(ok) == bool(golden["%s_%s_ok" % (case, run)]), (case, run)
    assert list(counts) == golden["%s_%s_counts" % (case, run)].tolist(), (case, run)
    if not ok:
        assert np.array_equal(T, np.eye(4)) and np.all(info == 0.0)
        assert np.array_equal(golden["%s_%s_T_1" % (case, run)], np.eye(4)) and np.array_equal(golden["%s_%s_info_1" % (case, run)], np.eye(6))
        print("%s %s (%s): no solution after %s pairs, as in the reference" % (case, run, who, list(counts)))
        return
    bound = S.information_bound(info_K, info_S)
    share = 0.0
    for th in (1, 3):
        d = rel(T, golden["%s_%s_T_%d" % (case, run, th)])
        assert d <= TOL_T, (case, run, th, d)
        di = np.abs(info - (golden["%s_%s_info_%d" % (case, run, th)] - (1.0 + th) * np.eye(6)))
        assert np.all(di <= bound), (case, run, th, float(di.max()))
        share = max(share, float((di / np.where(bound > 0, bound, 1.0)).max()))
    print("%s %s (%s): pairs %s, pose %.2e from the reference (bound %.0e), information at %.3g of its bound"
          % (case, run, who, list(counts), rel(T, golden["%s_%s_T_1" % (case, run)]), TOL_T, share))


# ---------------------------------------------------------------------------
# CPU
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES)
def test_specification_images_and_correspondences_equal_the_reference(golden, spec, case):
    prep = spec.prepare(case)
    assert len(prep["levels"]) == len(golden[case + "_iterations"])
    for l, L in enumerate(prep["levels"]):
        for name in S.WHICH:
            assert golden_image_matches(golden, case, l, name, L[name]), (case, l, name)
        idx, _ = spec.step(case, l, S.COLOR)
        assert idx_matches(golden, case, l, idx) and np.count_nonzero(idx >= 0) == int(golden["%s_l%d_pairs" % (case, l)]), (case, l)
    if case.startswith("o_n"):
        assert int(golden[case + "_l0_pairs"]) == int(case[3:])
    if case in ("o_v", "o_v2"):
        assert 0 < np.isnan(prep["levels"][0]["src_depth"]).sum() < 16 * 12 and np.isnan(prep["levels"][0]["tgt_depth"]).any()
    if case == "o_deep":
        assert [L["src_gray"].shape for L in prep["levels"]][-2:] == [(2, 4), (1, 2)]


@pytest.mark.parametrize("method", [S.COLOR, S.HYBRID])
@pytest.mark.parametrize("case", CASES)
def test_specification_steps_equal_the_reference_within_the_derived_bound(golden, spec, case, method):
    for l in range(len(spec.prepare(case)["levels"])):
        idx, s = spec.step(case, l, method)
        want = golden_step(golden, case, l, method, "init")
        assert s["rows"] == want["rows"] == (2 if method == S.HYBRID else 1) * s["K"]
        check_step("%s level %d method %d" % (case, l, method), want, s)
    if case == "o_const" and method == S.COLOR:
        assert not golden_step(golden, case, 0, method, "init")["JTJ"].any() and not spec.step(case, 0, method)[1]["JTJ"].any()


@pytest.mark.parametrize("method", [S.COLOR, S.HYBRID])
@pytest.mark.parametrize("case", CASES)
def test_specification_runs_equal_the_reference(golden, spec, case, method):
    ok, T, info, ex = spec.run(case, method)
    check_run(golden, case, "hybrid" if method == S.HYBRID else "color", ok, T, info, ex["counts"], ex["info_K"], ex.get("info_S"), "specification")


# ---------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ctx(lib):
    c = lib.Context(0)
    yield c
    c.close()


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES)
def test_images_correspondences_and_steps_equal_the_reference(lib, ctx, golden, spec, case):
    fr, opt, _ = spec.case(case)
    prep = spec.prepare(case)
    ctx.odometry_prepare(*fr, np.eye(4), lib_option(lib, opt))
    for l, L in enumerate(prep["levels"]):
        for name in S.WHICH:
            img = ctx.odometry_image(name, l)
            assert S.same_image(img, L[name]), (case, l, name, "specification")
            assert golden_image_matches(golden, case, l, name, img), (case, l, name, "reference")
        idx, K = ctx.odometry_correspondences(l, np.eye(4))
        assert idx_matches(golden, case, l, idx) and K == np.count_nonzero(idx >= 0) == int(golden["%s_l%d_pairs" % (case, l)])
        assert np.array_equal(idx, spec.step(case, l, S.COLOR)[0])
        for method in (S.COLOR, S.HYBRID):
            stats, K2, r2 = ctx.odometry_step(l, np.eye(4), method)
            s = spec.step(case, l, method)[1]
            got = unpack(stats)
            assert K2 == got["K"] == s["K"] == K and r2 == got["r2"] and np.all(stats[29:] == 0.0)
            check_step("%s level %d method %d" % (case, l, method), got, s, golden_step(golden, case, l, method, "init"))


@pytest.mark.gpu
@pytest.mark.parametrize("method", [S.COLOR, S.HYBRID])
@pytest.mark.parametrize("case", CASES)
def test_runs_equal_the_reference(lib, ctx, golden, spec, case, method):
    fr, opt, itc = spec.case(case)
    o = lib_option(lib, opt if method == S.HYBRID else dict(opt, iterations=itc))
    r = ctx.rgbd_odometry(*fr, np.eye(4), lib.ODOMETRY_HYBRID if method == S.HYBRID else lib.ODOMETRY_COLOR, o)
    sok, sT, sinfo, ex = spec.run(case, method)
    assert bool(r.success) == bool(sok) and r.pairs.tolist() == list(ex["counts"]) and r.information_pairs == ex["info_K"]
    check_run(golden, case, "hybrid" if method == S.HYBRID else "color", r.success, r.T, r.information, r.pairs.tolist(),
              ex["info_K"], ex.get("info_S"), "library")
    if sok:
        assert rel(r.T, sT) <= TOL_T
