"""The renderer's rule in f64 (tests/render_spec.py) against the same rule in exact rational arithmetic over the same f64
inputs (fractions.Fraction; exact z compared as rationals): coverage and the visible triangle equal at EVERY pixel of the
general scenes, depth within a measured tolerance; the tie scenes, whose f64 arithmetic is exact, equal with no tolerance and
as the inclusive rule says; the screen box of the rule by hand, conservative against exact arithmetic (every pixel a triangle
draws there lies inside its box), changing no byte of the scenes that were here before it, and deciding the cull scenes (slivers
through the eye, triangles a few ulps under z_near), where the rule without the box draws noise; the edge rule on a hand-made image; the depth-buffer encoding against LinearizeDepth; the
watertight property.  No GPU."""
from fractions import Fraction

import numpy as np
import pytest

import render_cases as cases
import render_spec as S

# The largest relative depth error of the f64 rule against exact arithmetic over SPEC_SCENES is 1.17e-14 (sphere_anchor
# 1.38e-15, sphere_tilted 2.78e-15, torus_rotated 1.17e-14, box_rotated 3.65e-16: measured, printed by the test below); 16 x
# that is allowed.  There is no general bound: det and s both cancel.
DEPTH_RTOL = 16 * 1.17e-14


def exact_render(c, cover=None):
    """-> index (int, -1 where nothing is drawn) and the exact depth (Fraction or None) per pixel.  Every triangle is tested at
    every pixel.  cover (a list): gets the set of pixels (y, x) each triangle draws, hidden or not"""
    Fr = Fraction
    E = [[Fr(float(x)) for x in row] for row in np.asarray(c["E"]).reshape(4, 4)]
    P = [[E[r][0] * Fr(float(v[0])) + E[r][1] * Fr(float(v[1])) + E[r][2] * Fr(float(v[2])) + E[r][3] for r in range(3)] for v in c["V"]]
    fx, fy, cx, cy = (Fr(float(x)) for x in c["K"])
    zn, zf = Fr(float(c["z_near"])), Fr(float(c["z_far"]))
    w, h = c["w"], c["h"]
    dx = [(Fr(x) - cx) / fx for x in range(w)]
    dy = [(Fr(y) - cy) / fy for y in range(h)]
    cross = lambda u, v: (u[1] * v[2] - u[2] * v[1], u[2] * v[0] - u[0] * v[2], u[0] * v[1] - u[1] * v[0])
    index = np.full((h, w), -1, np.int64)
    depth = [[None] * w for _ in range(h)]
    for t, (a, b, d) in enumerate(c["F"]):
        A, B, C = P[a], P[b], P[d]
        n = (cross(B, C), cross(C, A), cross(A, B))
        det = A[0] * n[0][0] + A[1] * n[0][1] + A[2] * n[0][2]
        drawn = set()
        if cover is not None:
            cover.append(drawn)
        for y in range(h):
            row = [(m[1] * dy[y] + m[2], m[0]) for m in n]
            for x in range(w):
                e = [r + k * dx[x] for r, k in row]
                s = e[0] + e[1] + e[2]
                if s == 0 or not (all(v >= 0 for v in e) or all(v <= 0 for v in e)):
                    continue
                z = det / s
                if z < zn or z > zf:
                    continue
                drawn.add((y, x))
                if depth[y][x] is None or z < depth[y][x]:         # (an equal depth: the lower index stays)
                    depth[y][x], index[y, x] = z, t
    return index, depth


_EXACT = {}


def exact_of(name):
    """-> index, depth, cover of exact_render over a scene of render_cases.CASES: computed once and shared (read-only)"""
    if name not in _EXACT:
        cover = []
        index, depth = exact_render(cases.CASES[name], cover)
        index.setflags(write=False)
        _EXACT[name] = index, depth, cover
    return _EXACT[name]


@pytest.mark.parametrize("name", list(cases.SPEC_SCENES))
def test_the_rule_in_f64_equals_the_rule_in_exact_arithmetic(name):
    c = cases.SPEC_SCENES[name]
    depth, index, mask, z64 = S.render(c["V"], c["F"], c["w"], c["h"], c["K"], c["E"], c["z_near"], c["z_far"])
    want_index, want_depth, _ = exact_of(name)
    covered = want_index >= 0
    assert int(np.sum((mask == 255) != covered)) == 0
    assert int(np.sum(index != want_index)) == 0
    assert covered.sum() > 20
    worst = max(abs(Fraction(float(z64[y, x])) - want_depth[y][x]) / want_depth[y][x] for y, x in zip(*np.nonzero(covered)))
    print("%s: %d covered pixels, largest relative depth error %.3g" % (name, covered.sum(), float(worst)))
    assert float(worst) <= DEPTH_RTOL
    assert np.array_equal(depth, np.where(covered, z64, 0.0).astype(np.float32))


def test_the_anchor_scene_is_the_one_of_the_record():
    c = cases.SPEC_SCENES["sphere_anchor"]
    assert c["V"].shape == (42, 3) and c["F"].shape == (80, 3)
    assert int((cases.spec_of("sphere_anchor")[2] == 255).sum()) == 144


def test_the_box_of_the_rule_by_hand():
    K, zn = (10.0, 10.0, 5.0, 5.0), 0.05
    A, B, C = (0.0, 0.0, 1.0), (1.0, 0.0, 1.0), (0.0, 2.0, 2.0)          # projects onto (5, 5), (15, 5), (5, 15)
    assert S.setup_box(A, B, C, 32, 32, K, zn) == (4, 4, 16, 16)          # floor - 1 .. ceil + 1
    assert S.setup_box(A, B, C, 12, 10, K, zn) == (4, 4, 11, 9)           # clamped to the image
    assert S.setup_box(A, B, C, 32, 32, (10.0, 10.0, 5.25, 5.5), zn) == (4, 4, 17, 17)    # 5.25 .. 15.25, 5.5 .. 15.5
    shift = lambda p, dx: (p[0] + dx, p[1], p[2])
    assert S.setup_box(shift(A, -1.625), shift(B, -1.625), shift(C, -3.25), 32, 32, K, zn) == (0, 4, 0, 16)   # u <= -1.25: ceil + 1 is 0
    assert S.setup_box(shift(A, -1.75), shift(B, -1.75), shift(C, -3.5), 32, 32, K, zn) is None              # u <= -2.5: ceil + 1 is -1
    assert S.setup_box(shift(A, 2.75), shift(B, 2.75), shift(C, 5.5), 32, 32, K, zn) == (31, 4, 31, 16)      # u >= 32.5: floor - 1 is 31
    assert S.setup_box(shift(A, 3.0), shift(B, 3.0), shift(C, 6.0), 32, 32, K, zn) is None                   # u >= 35: floor - 1 is 34
    # one or two vertices at z >= z_near: the whole image; none: nothing; z_near itself counts as in front
    assert S.setup_box(A, B, (0.0, 2.0, 0.04), 32, 24, K, zn) == (0, 0, 31, 23)
    assert S.setup_box(A, (1.0, 0.0, -1.0), (0.0, 2.0, 0.04), 32, 24, K, zn) == (0, 0, 31, 23)
    assert S.setup_box((0.0, 0.0, 0.04), (1.0, 0.0, -1.0), (0.0, 2.0, 0.0), 32, 24, K, zn) is None
    under = float(np.nextafter(np.float64(zn), 0.0))
    assert S.setup_box((0.0, 0.0, under), (1.0, 0.0, under), (0.0, 2.0, under), 32, 24, K, zn) is None
    assert S.setup_box((0.0, 0.0, zn), (1.0, 0.0, under), (0.0, 2.0, under), 32, 24, K, zn) == (0, 0, 31, 23)
    assert S.setup_box((0.0, 0.0, zn), (0.05, 0.0, zn), (0.0, 0.1, zn), 32, 32, K, zn) == (4, 4, 16, 26)
    # a non-finite camera coordinate: nothing; a projection that overflows: that whole span
    assert S.setup_box(A, B, (np.nan, 2.0, 2.0), 32, 32, K, zn) is None
    assert S.setup_box(A, B, (0.0, np.inf, 2.0), 32, 32, K, zn) is None
    assert S.setup_box(A, B, (1e308, 2.0, 0.06), 32, 24, K, zn)[::2] == (0, 31)
    assert S.setup_box(A, B, (0.0, -1e308, 0.06), 32, 24, K, zn) == (4, 0, 16, 23)


@pytest.mark.parametrize("name", cases.OLD_NAMES)
def test_the_box_moves_no_scene_that_was_here_before_it(name):
    """The rule once tested every triangle at every pixel.  On every scene of that time the box changes no byte."""
    boxed, unboxed = cases.spec_of(name), cases.spec(cases.CASES[name], unboxed=True)
    for g, w, what in zip(boxed[:3], unboxed[:3], ("depth", "index", "mask")):
        assert g.dtype == w.dtype and cases.bits(g).tobytes() == cases.bits(w).tobytes(), what


def inside_box(b, y, x):
    return b is not None and b[0] <= x <= b[2] and b[1] <= y <= b[3]


@pytest.mark.parametrize("name", list(cases.CULL_SCENES) + list(cases.SPEC_SCENES))
def test_the_box_holds_what_exact_arithmetic_draws_and_what_f64_adds(name):
    """The box is conservative: every pixel a triangle draws in exact arithmetic, visible or hidden, lies inside that
    triangle's box.  And where the boxed f64 rule shows a triangle that exact arithmetic does not show there, the pixel lies
    inside that triangle's box: what rounding adds stays where the triangle is."""
    c = cases.CASES[name]
    box = cases.boxes(c)
    want_index, _, cover = exact_of(name)
    assert len(cover) == len(box) == len(c["F"])
    for t, drawn in enumerate(cover):
        assert all(inside_box(box[t], y, x) for y, x in drawn), t
    index = cases.spec_of(name)[1]
    extra = (index >= 0) & (index != want_index)
    assert all(inside_box(box[index[y, x]], y, x) for y, x in zip(*np.nonzero(extra)))
    print("%s: exact arithmetic shows %d pixels, f64 in the box %d, %d of them another triangle's or nobody's in exact arithmetic"
          % (name, (want_index >= 0).sum(), (index >= 0).sum(), extra.sum()))
    if name in cases.SPEC_SCENES:
        assert not extra.any() and sum(len(d) for d in cover) > (want_index >= 0).sum()     # (hidden pixels were checked too)


def outside_their_box(c, index):
    box = cases.boxes(c)
    return sum(not inside_box(box[index[y, x]], y, x) for y, x in zip(*np.nonzero(index >= 0)))


def test_the_cull_scenes_are_not_vacuous():
    """Without the box the f64 rule draws what exact arithmetic does not; with it, it does not; the ordinary triangle beside
    the degenerate ones (index 32) is drawn all the same."""
    ordinary = 32
    # the triangle of the record, alone: 114 pixels without the box, none in exact arithmetic, a box of 4 x 2 pixels
    c = cases.CULL_SCENES["sliver_through_eye"]
    alone = cases.with_(c, F=c["F"][:1])
    assert int((cases.spec(alone, unboxed=True)[2] == 255).sum()) == 114
    assert cases.boxes(alone) == [(1, 22, 4, 23)] and (exact_render(alone)[0] == -1).all()
    assert int((cases.spec(alone)[2] == 255).sum()) <= 8
    assert outside_their_box(c, cases.spec(c, unboxed=True)[1]) >= 1
    assert set(np.unique(exact_of("sliver_through_eye")[0]).tolist()) == {-1, ordinary}
    c = cases.CULL_SCENES["under_near"]
    assert all(b is None for b in cases.boxes(c)[:ordinary])
    unboxed = cases.spec(c, unboxed=True)[1]
    assert ((unboxed >= 0) & (unboxed < ordinary)).sum() >= 1
    assert set(np.unique(cases.spec_of("under_near")[1]).tolist()) == {-1, ordinary}
    assert np.array_equal(cases.spec_of("under_near")[1], exact_of("under_near")[0])
    for name in ("sliver_through_eye", "under_near", "sliver_collinear", "sliver_tiny"):
        index = cases.spec_of(name)[1]
        assert (index == ordinary).sum() > 20, name
        assert len(cases.CULL_SCENES[name]["F"]) == 33
        if name != "sliver_through_eye":                     # (there the noise inside the small boxes is drawn)
            assert np.array_equal(index, exact_of(name)[0]), name
    # astride: the whole image is the box, and both triangles are seen
    c = cases.CULL_SCENES["astride_near_by_an_ulp"]
    assert cases.boxes(c)[:2] == [(0, 0, 31, 23)] * 2
    assert [int(np.sum(c["V"][f][:, 2] == cases.Z_NEAR)) for f in c["F"][:2]] == [1, 2]
    assert all((c["V"][f][:, 2] >= np.nextafter(cases.Z_NEAR, 0.0)).all() for f in c["F"][:2])
    assert {0, 1} <= set(np.unique(cases.spec_of("astride_near_by_an_ulp")[1]).tolist())


@pytest.mark.parametrize("name", list(cases.TIE_SCENES))
def test_tie_scenes_follow_the_inclusive_rule_exactly(name):
    c = cases.TIE_SCENES[name]
    depth, index, mask, z64 = S.render(c["V"], c["F"], c["w"], c["h"], c["K"], c["E"], c["z_near"], c["z_far"])
    want_index, want_depth = exact_render(c)
    assert np.array_equal(index, want_index)
    # the square's projection is the pixels 4 .. 12 x 2 .. 10, its border included: every edge and vertex pixel is drawn
    inside = np.zeros((c["h"], c["w"]), bool)
    inside[2:11, 4:13] = True
    assert np.array_equal(mask == 255, inside)
    assert all(Fraction(float(z64[y, x])) == want_depth[y][x] == 1 for y, x in zip(*np.nonzero(inside)))
    assert np.array_equal(depth, inside.astype(np.float32))
    # the diagonal (4, 2) .. (12, 10) runs through pixel centres and lies in both triangles: the lower index has it, and
    # each side belongs to the triangle that lies there
    ys, xs = np.nonzero(inside)
    above = (xs - 4) > (ys - 2)                               # towards the corner (12, 2): triangle (0, 1, 2)
    on = (xs - 4) == (ys - 2)
    first_has_upper = tuple(c["F"][0]) == (0, 1, 2)
    upper, lower = (0, 1) if first_has_upper else (1, 0)
    assert np.all(index[ys[above], xs[above]] == upper)
    assert np.all(index[ys[~above & ~on], xs[~above & ~on]] == lower)
    assert np.all(index[ys[on], xs[on]] == 0)
    assert index.max() <= 1                                   # (two copies: the first copy wins everywhere)


def around(terms):
    """a 16 x 12 image of ones whose pixel (5, 5) sees |W - E|, |S - N|, |NW - SE| = terms (fp32 each, as 2 t - t) and SW = NE"""
    d = np.full((12, 16), 1.0, np.float32)
    for t, (a, b) in zip(terms, (((5, 4), (5, 6)), ((6, 5), (4, 5)), ((4, 4), (6, 6)))):
        assert np.float32(t) == t and np.float32(2 * t) == 2 * t
        d[a], d[b] = 2 * t, t
    return d


def split(target):
    """target (f64 > 0) as a sum of three fp32 numbers whose partial sums are exact in f64"""
    terms, rest = [], np.float64(target)
    for _ in range(3):
        t = np.float32(rest)
        if np.float64(t) > rest:
            t = np.nextafter(t, np.float32(0.0))
        terms.append(np.float64(t))
        rest = rest - np.float64(t)
    assert rest == 0.0 and (terms[0] + terms[1]) + terms[2] == target
    return terms


def test_the_edge_rule_on_a_hand_made_image():
    d = np.full((12, 16), 2.0, np.float32)
    d[:, 8:] = 2.5                                           # a step of 0.5 between columns 7 and 8
    d[6, 6] = 0.0                                            # a background centre
    d[:, 0] = 9.0                                            # (the border is 0 whatever lies there)
    e = S.edges(d)
    assert e.shape == d.shape and e.dtype == np.uint8
    border = np.ones_like(d, bool)
    border[5:7, 5:11] = False
    assert not e[border].any()
    assert e[6, 6] == 0
    # columns 7 and 8 see the step through three of the four pairs: 0.25 * 3 * 0.5 = 0.375 >= 0.10
    assert e[5, 7] == 255 and e[5, 8] == 255 and e[5, 9] == 0 and e[5, 10] == 0
    # next to the hole the neighbour is -1: |2 - (-1)| = 3 through one pair
    assert e[6, 5] == 255 and e[5, 5] == 255
    # the ramp: delta = 0.25 |W - E| with the other pairs level; c = (delta - 0.05) / 0.05, the pixel floor(255 c + 0.5)
    for step, want in ((0.1875, 0), (0.25, 64), (0.3125, 143), (0.375, 223), (0.4375, 255)):
        assert S.edges(around([step, 0.0, 0.0]))[5, 5] == want, step
    # both thresholds hit exactly: 4 x 0.05 and 4 x 0.10 as exact sums of three fp32 differences
    for target, want, below in ((np.float64(0.05) * 4.0, 0, 0), (np.float64(0.10) * 4.0, 255, 255)):
        assert 0.25 * target in (np.float64(0.05), np.float64(0.10))
        assert S.edges(around(split(target)))[5, 5] == want
        assert S.edges(around(split(np.nextafter(target, 0.0))))[5, 5] == below
    just_above = S.edges(around(split(np.nextafter(np.float64(0.2), 1.0))))[5, 5]
    assert just_above == 0                                   # (255 x one ulp of the ramp)


def test_the_depth_buffer_encoding_inverts_linearize_depth():
    zn, zf = 0.05, 10.0
    for z in (0.05, 0.0500001, 0.3, 1.0, 2.71828, 9.999, 10.0):
        zb = S.depth_buffer(np.float64(z), zn, zf)
        assert 0.0 <= zb <= 1.0
        assert abs(S.linearize_depth(zb, zn, zf) - z) <= 1e-9 * z
    assert S.depth_buffer(np.float64(zn), zn, zf) == 0.0 and S.depth_buffer(np.float64(zf), zn, zf) == 1.0
    c = cases.CASES["sphere_anchor_depth_buffer"]
    depth, index, mask, z64 = S.render(c["V"], c["F"], c["w"], c["h"], c["K"], c["E"], c["z_near"], c["z_far"], S.DEPTH_BUFFER)
    assert np.all(depth[mask == 0] == 1.0) and np.all(depth[mask == 255] < 1.0)
    back = S.linearize_depth(depth[mask == 255].astype(np.float64), zn, zf)
    # an fp32 depth-buffer value near 1 resolves (z_far - z_near) 2^-24 / (dzb/dz) in depth: z^2 / (2 zn zf) * 2^-24 * (zf - zn)
    z = z64[mask == 255]
    assert np.all(np.abs(back - z) <= 2.0 ** -23 * z * z * (zf - zn) / (2 * zn * zf) + 1e-12)


def test_the_sphere_is_watertight():
    """Every ray through the unit sphere's inscribed polyhedron meets a triangle: the coverage has no hole and equals the
    silhouette of the polyhedron, which lies between the discs of the inscribed sphere of the facets and the unit sphere."""
    for name in ("sphere_anchor", "sphere_tilted", "sphere_64x48", "sphere_close_64x48"):
        c = cases.CASES[name]
        mask = cases.spec_of(name)[2] == 255
        DX, DY = S.rays(c["w"], c["h"], c["K"])
        centre = np.asarray(c["E"])[:3, 3]
        d = np.stack([DX, DY, np.ones_like(DX)], -1)
        d /= np.linalg.norm(d, axis=-1, keepdims=True)
        dist = np.linalg.norm(np.cross(d, centre), axis=-1)   # of the sphere's centre from each pixel's ray
        V, F = c["V"], c["F"]
        r_in = min(abs(np.dot(np.cross(V[b] - V[a], V[k] - V[a]) / np.linalg.norm(np.cross(V[b] - V[a], V[k] - V[a])), V[a])) for a, b, k in F)
        assert np.all(mask[dist <= r_in - 1e-9]), name
        assert not np.any(mask[dist >= 1.0 + 1e-9]), name
        # no hole: every row's and every column's covered pixels are one run (the silhouette is convex)
        for line in list(mask) + list(mask.T):
            on = np.nonzero(line)[0]
            assert len(on) == 0 or np.all(line[on[0]:on[-1] + 1]), name
        assert mask.sum() > 0
