"""Color map optimization on inputs chosen to break it (colormap.hip, compact.h), where tests/test_colormap.py has one
well-behaved scene.  The yardsticks are those of test_colormap.py: the numpy specification tests/colormap_spec.py, pinned to
the compiled reference by tests/golden/rgbd_hostile.npz (tests/golden/gen_rgbd_hostile.py): masks and visibility lists
equal, proxies bit for bit, a camera's sums within colormap_spec.sum_bound, colours within 1e-15, poses within 100 x the
spread the generator measured for the case among the reference and the specification's two summation orders.  No bound
is new.  The cases (tests/colormap_scene.py; exact numbers: 32 x 24, fx = fy = 16, no rotation, vertices on z = 1):

  m_b     vertices projecting exactly to u == 10, u == w - 10, v == 10, v == h - 10 and one fp32 ulp either side; two that
          fp32 (the proxy) and f64 (the iteration) decide differently; a NaN and an inf coordinate, the camera centre, behind
          the camera; vertices on pixels whose depth is NaN, +inf, -1
  m_k     cameras with 1 .. 5 accepted vertices, with exactly 6, and with constant images: the first and the last keep their
          pose bit for bit (the reference does not: DESIGN.md lists both outcomes), and the ordinary cameras compute what
          they compute without them (m_k2)
  m_d*    dilation half-sizes 10, 11 and 64 on 21 x 21 images
  m_v*    1, 255, 256, 257, 512 vertices (at 256 and 512 the padded count equals the count: a camera's list starts at a tile
          edge); m_c*: 1, 32, 33, 64, 65 cameras; all on 21 x 21 images, whose inside region is one pixel
  poses moved after prepare: a listed vertex outside every margin has proxy 0; vertices behind a camera (G2 < 0)"""
import os

import numpy as np
import pytest

import colormap_scene as scene
import colormap_spec as S
import packed_npz
from test_colormap import bits, check_sums

HERE = os.path.dirname(os.path.abspath(__file__))
SEAM_VERTICES, SEAM_CAMERAS, DILATIONS = (1, 255, 256, 257, 512), (1, 32, 33, 64, 65), (10, 11, 64)
SEAMS = [("m_v%d" % n, n, 2) for n in SEAM_VERTICES] + [("m_c%d" % n, 40, n) for n in SEAM_CAMERAS]
KEPT = [2, 3, 4, 5, 6, scene.KEEP_CONSTANT]                            # 1 .. 5 accepted vertices; constant images


@pytest.fixture(scope="module")
def golden():
    return packed_npz.load(os.path.join(HERE, "golden", "rgbd_hostile.npz"))


def lists_of(golden, name):
    at = np.concatenate([[0], np.cumsum(golden[name + "_vis_n"])])
    return [golden[name + "_vis_list"][at[c]:at[c + 1]] for c in range(len(golden[name + "_vis_n"]))]


def option_of(case):
    return dict(S.default_option(), **case[5])


class Memo:
    """a case's inputs and the specification's prepared state, once; states that a test steps are made by fresh()"""

    def __init__(self):
        self.have = {}

    def get(self, name, make):
        if name not in self.have:
            case = make()
            st = S.State(case[4], case[0], case[1], case[2], case[3], option_of(case))
            self.have[name] = (case, st, st.proxy())
        return self.have[name]

    @staticmethod
    def fresh(case):
        return S.State(case[4], case[0], case[1], case[2], case[3], option_of(case))


@pytest.fixture(scope="module")
def spec():
    return Memo()


def check_stages(golden, name, st, proxy):
    assert np.array_equal([len(x) for x in st.lists], golden[name + "_vis_n"])
    for c, want in enumerate(lists_of(golden, name)):
        assert np.array_equal(st.lists[c], want), (name, c)
    assert np.array_equal(bits(proxy), bits(golden[name + "_proxy0"])), name


# ---------------------------------------------------------------------------
# CPU
# ---------------------------------------------------------------------------
def test_specification_vertices_on_the_decisions(golden, spec):
    case, st, proxy = spec.get("m_b", scene.boundary_case)
    depths, colors, E, K, V, _ = case
    check_stages(golden, "m_b", st, proxy)
    assert not st.vis[:, 62:66].any()                                  # NaN, inf, a camera centre, behind the cameras
    u, v, _ = S.project(E[0], K, V)
    in32 = S.inside(u, v, scene.HW, scene.HH)
    assert in32[48:60].tolist() == [True, False, True, False, True, False] * 2      # at, one ulp below, one ulp above: 10 | w - 10 | 10 | h - 10
    tr = []
    S.terms(V, np.arange(62), E[0], K, st.gray[0], st.dx[0], st.dy[0], proxy, tr)
    assert tr[0][48:60].tolist() == in32[48:60].tolist()
    assert in32[60] and not tr[0][60] and not in32[61] and tr[0][61]    # fp32 and f64 disagree, both ways
    assert np.abs(st.colours() - golden["m_b_colors_0"]).max() <= 1e-15
    run = spec.fresh(case)
    run.run(2)
    d, tol = np.abs(run.E - golden["m_b_extr_2"]).max(), 100.0 * float(golden["m_b_pose_spread"])
    print("m_b: poses after 2 iterations %.3g from the reference (tolerance %.3g)" % (d, tol))
    assert d <= tol


def test_specification_cameras_that_keep_their_pose(golden, spec):
    case, st, proxy = spec.get("m_k", scene.keep_pose_case)
    case2, st2, proxy2 = spec.get("m_k2", lambda: scene.keep_pose_case(False))
    check_stages(golden, "m_k", st, proxy)
    check_stages(golden, "m_k2", st2, proxy2)
    assert [len(st.terms(c, proxy)) for c in range(9)] == [72, 72, 1, 2, 3, 4, 5, 6, 10]
    run, run2 = spec.fresh(case), spec.fresh(case2)
    rows, rows2 = run.step(), run2.step()
    for c in KEPT:
        assert np.array_equal(bits(run.E[c]), bits(case[2][c])), c      # kept, bit for bit
    assert np.array_equal(bits(rows[:2]), bits(rows2)) and np.array_equal(bits(run.E[:2]), bits(run2.E))
    assert np.abs(run.E[:2] - golden["m_k_ref_extr_1"][:2]).max() <= 100.0 * float(golden["m_k_pose_spread"])
    assert np.isfinite(run.E[7]).all() and not np.array_equal(run.E[7], case[2][7])               # exactly 6: solved
    assert np.abs(run.E[7] - golden["m_k_ref_extr_1"][7]).max() <= 100.0 * float(golden["m_k_pose_spread_7"])
    # what the reference does with the cameras the library keeps: it moves every one of them, to NaN
    # where its LDLT meets a zero pivot (one vertex; constant images), to a finite pose without meaning otherwise
    assert not golden["m_k_ref_kept"].any()
    assert golden["m_k_ref_finite"].tolist() == [True, True, False, True, True, True, True, True, False]


@pytest.mark.parametrize("k", DILATIONS)
def test_specification_dilation_equals_the_reference(golden, k):
    depths = scene.seam_case(40, 2, k)[0]
    for c in range(2):
        assert np.array_equal(S.depth_mask(depths[c], 0.1, k), golden["m_d%d_mask" % k][c])
    assert (golden["m_d%d_mask" % k] != 255).any() == (k < 64)


@pytest.mark.parametrize("name,nv,nc", SEAMS)
def test_specification_counts_at_the_seams(golden, spec, name, nv, nc):
    case, st, proxy = spec.get(name, lambda: scene.seam_case(nv, nc))
    check_stages(golden, name, st, proxy)


# ---------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ctx(lib):
    c = lib.Context(0)
    yield c
    c.close()


def new_map(lib, ctx, case):
    depths, colors, E, K, V, over = case
    n, h, w = depths.shape
    m = ctx.color_map(w, h, n, K, lib.color_map_option(**over))
    for i in range(n):
        m.set_image(i, depths[i], colors[i], E[i])
    m.set_vertices(V)
    return m


def check_prepared(golden, name, m, st, proxy):
    counts = m.prepare()
    assert np.array_equal(counts, golden[name + "_vis_n"])
    for c, want in enumerate(lists_of(golden, name)):
        assert np.array_equal(m.visible(c), want) and np.array_equal(m.visible(c), st.lists[c]), (name, c)
        assert np.array_equal(m.image(c, "mask"), st.mask[c]), (name, c)
    p = m.proxy()
    assert np.array_equal(bits(p), bits(golden[name + "_proxy0"])) and np.array_equal(bits(p), bits(proxy)), name


@pytest.mark.gpu
def test_vertices_on_the_decisions(lib, ctx, golden, spec):
    case, st, proxy = spec.get("m_b", scene.boundary_case)
    m = new_map(lib, ctx, case)
    check_prepared(golden, "m_b", m, st, proxy)
    check_sums(m.sums(), st, proxy)
    assert np.abs(m.colors() - golden["m_b_colors_0"]).max() <= 1e-15
    m.run(2)
    d, tol = np.abs(m.extrinsics() - golden["m_b_extr_2"]).max(), 100.0 * float(golden["m_b_pose_spread"])
    print("m_b: poses after 2 iterations %.3g from the reference (pose_spread %.3g, tolerance %.3g)" % (d, float(golden["m_b_pose_spread"]), tol))
    assert d <= tol
    m.close()


@pytest.mark.gpu
def test_cameras_that_keep_their_pose(lib, ctx, golden, spec):
    case, st, proxy = spec.get("m_k", scene.keep_pose_case)
    case2, st2, proxy2 = spec.get("m_k2", lambda: scene.keep_pose_case(False))
    m, m2 = new_map(lib, ctx, case), new_map(lib, ctx, case2)
    check_prepared(golden, "m_k", m, st, proxy)
    check_prepared(golden, "m_k2", m2, st2, proxy2)
    rows, rows2 = m.sums(), m2.sums()
    check_sums(rows, st, proxy)
    assert np.array_equal(bits(rows[:2]), bits(rows2))                  # the ordinary cameras' sums, with and without the others
    rr, count = m.step()
    m2.step()
    assert count.tolist() == [72, 72, 1, 2, 3, 4, 5, 6, 10]
    E1, E1b = m.extrinsics(), m2.extrinsics()
    for c in KEPT:
        assert np.array_equal(bits(E1[c]), bits(case[2][c])), c         # kept, bit for bit
    assert np.array_equal(bits(E1[:2]), bits(E1b))
    d, tol = np.abs(E1[:2] - golden["m_k_ref_extr_1"][:2]).max(), 100.0 * float(golden["m_k_pose_spread"])
    d7, tol7 = np.abs(E1[7] - golden["m_k_ref_extr_1"][7]).max(), 100.0 * float(golden["m_k_pose_spread_7"])
    print("m_k: cameras 0, 1 %.3g from the reference (tolerance %.3g); camera 7, exactly 6 vertices, %.3g (tolerance %.3g)" % (d, tol, d7, tol7))
    assert d <= tol and np.isfinite(E1[7]).all() and not np.array_equal(E1[7], case[2][7]) and d7 <= tol7
    m.close(); m2.close()


@pytest.mark.gpu
@pytest.mark.parametrize("k", DILATIONS)
def test_dilation_beyond_half_the_image(lib, ctx, golden, k):
    case = scene.seam_case(40, 2, k)
    m = new_map(lib, ctx, case)
    m.prepare()
    for c in range(2):
        got = m.image(c, "mask")
        assert np.array_equal(got, S.depth_mask(case[0][c], 0.1, k)) and np.array_equal(got, golden["m_d%d_mask" % k][c])
    m.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name,nv,nc", SEAMS)
def test_counts_at_the_seams(lib, ctx, golden, spec, name, nv, nc):
    case, st, proxy = spec.get(name, lambda: scene.seam_case(nv, nc))
    m = new_map(lib, ctx, case)
    check_prepared(golden, name, m, st, proxy)
    check_sums(m.sums(), st, proxy)
    assert np.abs(m.colors() - st.colours()).max() <= 1e-15
    m.close()


@pytest.mark.gpu
def test_poses_moved_after_prepare(lib, ctx, spec):
    """visibility stays that of the prepare; the margin tests follow the poses.  Six pixels further in u the listed vertices
    right of u = 16 are outside every camera's margin: proxy 0, no term.  With camera 0 turned half a turn about y, its
    listed vertices are BEHIND it (G2 < 0) and still project into its margin: neither the proxy nor the iteration tests z
    (nor does the reference), and both sides agree on the terms that gives."""
    case, st, proxy = spec.get("m_b", scene.boundary_case)
    m = new_map(lib, ctx, case)
    m.prepare()
    moved = spec.fresh(case)
    for name, E in (("six pixels further", np.stack([scene.shifted(6.0), scene.shifted(7.0)])),
                    ("turned", np.stack([scene.rigid((0.0, np.pi, 0.0), (0.0, 0.0, 0.0)) @ case[2][0], case[2][1]]))):
        m.set_extrinsics(E)
        moved.E = E.copy()
        p = moved.proxy()
        got = m.proxy()
        assert np.array_equal(bits(got), bits(p)), name
        listed = st.vis.any(0)
        if name == "six pixels further":
            gone = listed & (case[4][:, 0] * 16.0 + 16.0 >= 16.0)
            assert gone.sum() > 20 and not got[gone].any() and got[listed & ~gone].all()
        else:
            assert (S.transform(E[0], case[4][st.lists[0]])[2] < 0).all() and (S.transform(E[1], case[4][st.lists[1]])[2] > 0).all()
        check_sums(m.sums(), moved, p)
        rr, count = m.step()
        rows = moved.step()
        assert count.tolist() == rows[:, 28].astype(int).tolist() and count.min() > 10
        print("%s: counts %s" % (name, count.tolist()))
    m.close()
