"""The neighbour search under normal estimation, the colour gradient and FPFH (visma_amd/csrc/nn_list.h, nn_grid.hip), list by
list: visma_icp_selftest_neighbor_lists hands out the lists the GPU builds, nn_spec.spec_lists is the exhaustive f64 scan.

What is asserted, for BOTH kinds of list (the sorted list in LDS, the max-heap in global memory) wherever cap <= 170: idx
equal, d2 BIT-equal, cnt equal, -1 / +inf behind every list, and a second call identical.  Bit equality is derived, not
measured: the kernel's d2 and the specification's are the same three f64 products and two f64 sums in the same order, and
the build keeps -ffp-contract=off; the order is ascending (d2, index), which leaves nothing open where distances tie.

The CPU tests assert that every cloud has the property it is there for: exact ties at the cut, pairs on the radius bound,
grids of one cell along an axis, cells far larger than the radius, non-finite points."""
import ctypes as C

import numpy as np
import pytest

from nn_spec import cube_cloud, nonfinite_cloud, spec_lists, spec_pairs, spec_radius_count

INVALID = 1
KNN, RADIUS, HYBRID = 0, 1, 2
LDS_MAX = 170           # kNormalsMaxList: the longest list the LDS holds


# ---------------------------------------------------------------------------
# the clouds, each from a seed or a formula
# ---------------------------------------------------------------------------
def _bound_points(q, direction, r2, x_share=0.999):
    """three points p with the specification's d2(q, p) one ulp below r2, equal to r2 and one ulp above it: the first
    offset coordinate fixed at sqrt(r2) * x_share, the second found by bisection over the f64 values (d2 is monotone in it)"""
    ax, ay = direction
    out = []
    for target in (np.nextafter(r2, -np.inf), r2, np.nextafter(r2, np.inf)):
        p = q.copy()
        p[ax] = q[ax] + np.sqrt(r2) * x_share

        def d2_of(bits):                                            # (the offset by its bits: positive, so ordered like them)
            p[ay] = q[ay] + np.array(bits, np.int64).view(np.float64)
            d = q - p
            return (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]
        lo = int(np.float64(1e-6).view(np.int64))
        hi = int(np.float64(np.sqrt(r2)).view(np.int64))
        assert d2_of(lo) < target < d2_of(hi)
        while hi - lo > 1:                                          # the smallest value at which d2 >= target
            mid = (lo + hi) // 2
            if d2_of(mid) >= target:
                hi = mid
            else:
                lo = mid
        assert d2_of(hi) == target, (q, direction, target)          # (no value may be skipped: the caller's assert says so)
        out.append(p.copy())
    return out


BOUND_RADII = (0.3, 0.2)          # (float)(r * r) rounds up / down


def bound_cloud():
    """six queries near the origin; for either radius and every query three points at d2 = bound - 1 ulp, bound, bound +
    1 ulp in the plane of two axes; 150 random points around them"""
    rng = np.random.default_rng(17)
    queries = np.array([[0, 0, 0], [1, 2, 3], [-3, 1, 2], [2, -1, -2], [5, 5, 0], [0, -4, 4]], np.float64) / 1024.0
    dirs = [(0, 1), (1, 2), (2, 0), (1, 0), (2, 1), (0, 2)]
    pts = [q for q in queries]
    for r in BOUND_RADII:
        r2 = float(np.float32(r * r))
        for q, d in zip(queries, dirs):
            pts += _bound_points(q, d, r2)
    pts += list(rng.uniform(-0.5, 0.5, (150, 3)))
    return np.array(pts)


def dups_cloud():
    """300 copies of one point among 200 random ones, in a seeded order -> (xyz, the indices of the copies)"""
    rng = np.random.default_rng(23)
    p = rng.random((500, 3))
    copies = np.sort(rng.permutation(500)[:300])
    p[copies] = [0.4, 0.55, 0.35]
    return p, copies


def line_cloud(axis):
    """500 points on a line along `axis`, geometric spacing (1 mm growing by 2 % a step): the grid is one cell wide in the
    other two dimensions and a KNN search needs several rings on the sparse side"""
    p = np.tile([0.3, -0.2, 0.7], (500, 1))
    p[:, axis] = 1e-3 * (1.02 ** np.arange(500) - 1.0) / 0.02
    return p


def plane_cloud():
    """25 x 20 points in the plane z = 0.25, geometric spacing along both axes"""
    x = 1e-2 * (1.2 ** np.arange(25) - 1.0) / 0.2
    y = 1e-2 * (1.25 ** np.arange(20) - 1.0) / 0.25
    i, j = np.meshgrid(x, y, indexing="ij")
    return np.stack([i.ravel(), j.ravel(), np.full(500, 0.25)], 1)


def outlier_cloud(first):
    """2,000 points in the unit cube and one at (1e4, 0, 0), first (it is then the binning origin) or last"""
    p = np.random.default_rng(29).random((2000, 3))
    far = np.array([[1e4, 0.0, 0.0]])
    return np.concatenate([far, p] if first else [p, far])


FAR_OFFSET = np.array([1.2e5, -8e4, 4e4])


def far_cloud():
    """a 2,000-point surface patch of 0.5 x 0.5 at FAR_OFFSET: about ten points within 0.02 of a point"""
    rng = np.random.default_rng(31)
    xy = rng.random((2000, 2)) * 0.5
    z = 0.05 * np.sin(7.0 * xy[:, 0]) * np.cos(5.0 * xy[:, 1])
    return np.concatenate([xy, z[:, None]], 1) + FAR_OFFSET


def small_cloud(n):
    return np.random.default_rng(100 + n).random((n, 3))


def no_finite_cloud():
    """50 rows, each with at least one NaN: no distance is a number"""
    p = np.random.default_rng(37).random((50, 3))
    p[np.arange(50), np.arange(50) % 3] = np.nan
    p[::7] = np.nan
    p[3, 0] = np.inf                                               # (3 % 3 == 0: the NaN went there; put it elsewhere)
    p[3, 1] = np.nan
    return p


# the searches of every cloud: (search_type, cap, radius)
CUBE_SEARCHES = ([(KNN, c, 0.0) for c in (1, 2, 5, 10, 30, 170, 171, 400, 729, 1000)] +
                 [(HYBRID, c, r) for r in (0.25, 0.3) for c in (5, 30)] + [(RADIUS, 1, 0.25)])
CASES = {}
for _name, _shuf in (("cube", False), ("cube_shuffled", True)):
    for _s in CUBE_SEARCHES:
        CASES["%s-%s" % (_name, "-".join(map(str, _s)))] = (lambda shuf=_shuf: cube_cloud(shuf), _s)
for _r in BOUND_RADII:
    CASES["bound-hybrid-%g" % _r] = (bound_cloud, (HYBRID, 30, _r))
    CASES["bound-radius-%g" % _r] = (bound_cloud, (RADIUS, 1, _r))
CASES["dups-knn"] = (lambda: dups_cloud()[0], (KNN, 30, 0.0))
CASES["dups-hybrid"] = (lambda: dups_cloud()[0], (HYBRID, 30, 0.1))
for _s in ((KNN, 30, 0.0), (HYBRID, 30, 0.1), (RADIUS, 1, 0.1), (KNN, 100, 0.0)):
    CASES["one_point_64_times-%s" % "-".join(map(str, _s))] = (lambda: np.tile([0.4, 0.55, 0.35], (64, 1)), _s)
for _name, _make in (("line_x", lambda: line_cloud(0)), ("line_y", lambda: line_cloud(1)), ("line_z", lambda: line_cloud(2)),
                     ("plane_xy", plane_cloud)):
    for _s in ((KNN, 30, 0.0), (HYBRID, 30, 0.5), (RADIUS, 1, 0.5), (KNN, 200, 0.0)):
        CASES["%s-%s" % (_name, "-".join(map(str, _s)))] = (_make, _s)
for _first in (True, False):
    for _s in ((HYBRID, 30, 0.02), (KNN, 30, 0.0), (RADIUS, 1, 0.02)):
        CASES["outlier_%s-%s" % ("first" if _first else "last", "-".join(map(str, _s)))] = \
            (lambda first=_first: outlier_cloud(first), _s)
for _s in ((HYBRID, 30, 0.02), (RADIUS, 1, 0.02), (KNN, 12, 0.0)):
    CASES["far-%s" % "-".join(map(str, _s))] = (far_cloud, _s)
for _n in (1, 2, 3, 63, 64, 65, 257):
    for _c in (1, 3, 20, 30, 60, 170):                             # (256 / 128 / 64 threads a workgroup: cap 20 / 30 / 60 and up)
        CASES["small%d-knn%d" % (_n, _c)] = (lambda n=_n: small_cloud(n), (KNN, _c, 0.0))
        CASES["small%d-hybrid%d" % (_n, _c)] = (lambda n=_n: small_cloud(n), (HYBRID, _c, 0.4))
for _s in ((KNN, 12, 0.0), (KNN, 170, 0.0), (KNN, 171, 0.0), (KNN, 600, 0.0), (HYBRID, 30, 0.3), (RADIUS, 1, 0.2)):
    CASES["nonfinite-%s" % "-".join(map(str, _s))] = (lambda: nonfinite_cloud()[0], _s)
for _s in ((KNN, 5, 0.0), (KNN, 171, 0.0), (HYBRID, 5, 0.3), (RADIUS, 1, 0.3)):
    CASES["no_finite_point-%s" % "-".join(map(str, _s))] = (no_finite_cloud, _s)

_SPEC = {}


def expected(name):
    """(xyz, search, what the self-test must return): idx int32 padded with -1, d2 padded with +inf, cnt; computed once"""
    if name not in _SPEC:
        make, (st, cap, radius) = CASES[name]
        xyz = make()
        assert len(xyz) <= 4096
        if st == RADIUS:
            want = (None, None, spec_radius_count(xyz, radius).astype(np.int32))
        else:
            idx, d2, cnt = spec_lists(xyz, st, cap, radius)
            live = np.arange(cap)[None, :] < cnt[:, None]
            pad = cap - idx.shape[1]                                # cap > n: the row is padded to the caller's cap
            idx = np.pad(idx, ((0, 0), (0, pad))); d2 = np.pad(d2, ((0, 0), (0, pad)))
            want = (np.where(live, idx, -1).astype(np.int32), np.where(live, d2, np.inf), cnt.astype(np.int32))
        _SPEC[name] = (xyz, (st, cap, radius), want)
    return _SPEC[name]


def _same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.int64), np.ascontiguousarray(b).view(np.int64))


# ---------------------------------------------------------------------------
# CPU: every cloud has the property it is there for
# ---------------------------------------------------------------------------
def _cut_in_a_tie(xyz, cap):
    """rows whose cap-th and (cap + 1)-th distance are equal: the cut falls inside a tie"""
    _, d2, cnt = spec_lists(xyz, KNN, cap + 1, 0.0)
    return int(((cnt == cap + 1) & (d2[:, cap - 1] == d2[:, cap])).sum())


@pytest.mark.parametrize("shuffled", [False, True])
def test_cube_cuts_fall_inside_ties_and_pairs_sit_on_the_bound(shuffled):
    p = cube_cloud(shuffled)
    assert p.shape == (729, 3)
    assert [_cut_in_a_tie(p, c) for c in (2, 5, 10, 30, 171)] == [729, 645, 645, 721, 654]
    # r = 0.25: (double)(float)(r * r) = 0.0625 is a distance of the lattice (two steps along an axis): strictly outside
    assert float(np.float32(0.25 * 0.25)) == 0.0625
    d2, ok = spec_pairs(p, HYBRID, 0.25)
    on = d2 == 0.0625
    assert on.sum() == 2 * 3 * 7 * 81 and not (on & ok).any()
    assert (ok.sum(1) == spec_radius_count(p, 0.25)).all() and ok.sum(1).max() == 27       # 1 + 6 + 12 + 8
    if shuffled:
        assert not np.array_equal(p, cube_cloud(False)) and np.array_equal(np.unique(p, axis=0), np.unique(cube_cloud(), axis=0))


def test_bound_cloud_has_pairs_one_ulp_either_side_of_the_bound_and_on_it():
    p = bound_cloud()
    ups = []
    for r in BOUND_RADII:
        r2 = float(np.float32(r * r))
        ups.append(r2 > r * r)
        d2, ok = spec_pairs(p, HYBRID, r)
        below, on, above = (d2 == np.nextafter(r2, -np.inf)), (d2 == r2), (d2 == np.nextafter(r2, np.inf))
        assert below.sum() >= 12 and on.sum() >= 12 and above.sum() >= 12              # (either direction of a pair)
        assert ok[below].all() and not ok[on].any() and not ok[above].any()
    assert ups == [True, False]                                     # one bound rounds up, one down


def test_duplicate_clouds():
    p, copies = dups_cloud()
    assert len(copies) == 300 and len(np.unique(p, axis=0)) == 201
    for st, r in ((KNN, 0.0), (HYBRID, 0.1)):
        idx, d2, cnt = spec_lists(p, st, 30, r)
        assert (cnt[copies] == 30).all() and not d2[copies].any()
        assert (idx[copies] == copies[:30]).all()                   # the 30 lowest indices among the copies
    one = np.tile([0.4, 0.55, 0.35], (64, 1))
    idx, d2, cnt = spec_lists(one, KNN, 30, 0.0)
    assert (idx == np.arange(30)).all() and not d2.any() and (cnt == 30).all() and not np.ptp(one, axis=0).any()


def test_lines_and_plane_are_one_cell_wide():
    for axis in range(3):
        p = line_cloud(axis)
        assert (np.ptp(p, axis=0) > 0).tolist() == [k == axis for k in range(3)]
        step = np.diff(p[:, axis])
        assert step.min() > 0 and step.max() / step.min() > 1e4      # the 30 nearest of a dense point lie many sparse steps apart
    p = plane_cloud()
    assert p.shape == (500, 3) and (np.ptp(p, axis=0) > 0).tolist() == [True, True, False]
    assert len(np.unique(p, axis=0)) == 500


def test_outlier_and_far_clouds():
    for first in (True, False):
        p = outlier_cloud(first)
        assert len(p) == 2001 and p[0 if first else -1].tolist() == [1e4, 0.0, 0.0]
        # 2,048 cells an axis at the most: a cell of 1e4 / 2048 = 4.9 holds the unit cube whole, 244 radii wide
        assert np.ptp(p[:, 0]) / 2048 > 100 * 0.02
        cnt = spec_radius_count(p, 0.02)
        assert cnt[0 if first else -1] == 1 and 1 < cnt.max() < 30
    p = far_cloud()
    assert np.abs(p).min(0).tolist() > [1e5, 7e4, 3e4]
    cnt = spec_radius_count(p, 0.02)
    assert 5 < np.median(cnt) < 30 and cnt.min() >= 1


def test_nonfinite_clouds():
    p, a, b, nan_row = nonfinite_cloud()
    finite = np.isfinite(p).all(1)
    assert finite.sum() == 597 and not finite[[a, b, nan_row]].any()
    assert np.isnan(p[a]).sum() == 1 and np.isinf(p[b]).sum() == 1 and np.isnan(p[nan_row]).all()
    for st, cap, r in ((KNN, 12, 0.0), (KNN, 170, 0.0), (KNN, 171, 0.0), (KNN, 600, 0.0), (HYBRID, 30, 0.3)):
        idx, d2, cnt = spec_lists(p, st, cap, r)
        live = np.arange(idx.shape[1])[None, :] < cnt[:, None]
        assert not (np.isin(idx, [a, nan_row]) & live).any()        # a and the NaN row appear in no list
        assert cnt[a] == 0 and cnt[nan_row] == 0
        assert not np.isnan(d2).any()
        has_b = (live & (idx == b)).any(1)
        if cap < 597:
            assert not has_b.any()                                  # cap finite points exist: b is nobody's neighbour
            assert cnt[b] == (cap if st == KNN else 0) and (st != KNN or np.isinf(d2[b]).all())
        else:
            assert has_b[finite].all() and (cnt[finite] == 598).all()
            assert (idx[finite, 597] == b).all() and np.isinf(d2[finite, 597]).all() and np.isfinite(d2[finite, :597]).all()
            assert cnt[b] == 597 and not has_b[b]                   # inf - inf: b is not its own neighbour
    assert spec_radius_count(p, 0.2)[[a, b, nan_row]].tolist() == [0, 0, 0]
    q = no_finite_cloud()
    assert not np.isfinite(q).all(1).any() and np.isnan(q).any(1).all()
    assert not spec_lists(q, KNN, 5, 0.0)[2].any() and not spec_radius_count(q, 0.3).any()


def test_small_clouds_cover_every_workgroup_size_and_cap_above_n():
    caps = sorted({c[1][1] for k, c in CASES.items() if k.startswith("small")})
    # threads per workgroup by the LDS 12-byte entries take: within 60 KiB down to 64 (nn_list_threads)
    threads = lambda cap: next(t for t in (256, 128, 64) if cap * 12 * t <= 60 * 1024 or t == 64)     # noqa: E731
    assert {threads(c) for c in caps} == {256, 128, 64} and threads(LDS_MAX) == 64
    ns = sorted({len(c[0]()) for k, c in CASES.items() if k.startswith("small")})
    assert ns == [1, 2, 3, 63, 64, 65, 257] and min(caps) == 1 and max(caps) > 65


def test_argument_errors_are_refused_before_any_launch(lib):
    L = lib.load()
    p = np.ascontiguousarray(small_cloud(10))
    idx = np.zeros((10, 200), np.int32); d2 = np.zeros((10, 200)); cnt = np.zeros(10, np.int32)
    dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int32)
    P, I, D, N = p.ctypes.data_as(dp), idx.ctypes.data_as(ip), d2.ctypes.data_as(dp), cnt.ctypes.data_as(ip)
    call = L.visma_icp_selftest_neighbor_lists
    for cap in (0, -1):
        for kind in (0, 1):
            assert call(P, 10, KNN, cap, 0.0, kind, I, D, N) == INVALID
    assert call(P, 10, KNN, LDS_MAX + 1, 0.0, 0, I, D, N) == INVALID          # the LDS holds 170 entries
    assert call(P, 10, HYBRID, LDS_MAX + 1, 0.5, 0, I, D, N) == INVALID
    assert call(P, 10, 3, 5, 0.5, 0, I, D, N) == INVALID and call(P, 10, -1, 5, 0.5, 0, I, D, N) == INVALID
    assert call(P, 10, KNN, 5, 0.0, 2, I, D, N) == INVALID and call(P, 10, KNN, 5, 0.0, -1, I, D, N) == INVALID
    assert call(None, 10, KNN, 5, 0.0, 0, I, D, N) == INVALID
    assert call(P, 10, KNN, 5, 0.0, 0, None, D, N) == INVALID
    assert call(P, 10, KNN, 5, 0.0, 1, I, None, N) == INVALID
    assert call(P, 10, HYBRID, 5, 0.5, 0, I, D, None) == INVALID
    assert call(P, 10, RADIUS, 1, 0.5, 0, None, None, None) == INVALID        # (Radius: idx / d2 may be NULL, cnt not)
    assert call(P, 0, KNN, 5, 0.0, 0, I, D, N) == INVALID
    for r in (0.0, -1.0, float("nan"), float("inf")):
        assert call(P, 10, HYBRID, 5, r, 0, I, D, N) == INVALID and call(P, 10, RADIUS, 1, r, 0, None, None, N) == INVALID
    assert not idx.any() and not d2.any() and not cnt.any()


# ---------------------------------------------------------------------------
# GPU: every list against the specification
# ---------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(CASES))
def test_lists_equal_the_specification_bit_for_bit(lib, name):
    xyz, (st, cap, radius), (idx, d2, cnt) = expected(name)
    if st == RADIUS:
        got = lib.selftest_neighbor_lists(xyz, RADIUS, 1, radius)
        assert np.array_equal(got, cnt), (name, int((got != cnt).sum()))
        assert np.array_equal(lib.selftest_neighbor_lists(xyz, RADIUS, 1, radius), got)
        return
    for kind in ((0, 1) if cap <= LDS_MAX else (1,)):
        gi, gd, gc = lib.selftest_neighbor_lists(xyz, st, cap, radius, kind)
        what = (name, "heap" if kind else "lds")
        assert gi.shape == (len(xyz), cap) and gd.shape == (len(xyz), cap)
        assert np.array_equal(gc, cnt), (what, int((gc != cnt).sum()), int(np.argmax(gc != cnt)))
        rows = np.nonzero((gi != idx).any(1))[0]
        assert not len(rows), (what, len(rows), int(rows[0]), gi[rows[0]].tolist(), idx[rows[0]].tolist())
        assert _same_bits(gd, d2), (what, int((gd.view(np.int64) != d2.view(np.int64)).any(1).sum()))
        live = np.arange(cap)[None, :] < gc[:, None]
        assert (gi[~live] == -1).all() and np.isposinf(gd[~live]).all()                 # the padding
        ai, ad, ac = lib.selftest_neighbor_lists(xyz, st, cap, radius, kind)            # a second call: identical
        assert np.array_equal(ai, gi) and _same_bits(ad, gd) and np.array_equal(ac, gc), what
