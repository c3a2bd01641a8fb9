"""The public neighbour search (visma_icp_kdtree_*, Context.kdtree; visma_amd/csrc/kdtree.hip): KNN, Radius and Hybrid for
ANY query points against a cloud resident on the device.

CPU: the numpy specification (tests/kdtree_spec.py) gives what the compiled reference's KDTreeFlann returned
(tests/golden/kdtree.npz, tests/golden/gen_kdtree.py) -- counts, the digests of all lists, sampled lists in full, d2 to the
bit --, and every cloud has the property it is there for.

GPU: the library against the specification: idx equal, d2 BIT-equal, cnt and offsets equal, -1 / +inf behind every list, a
second call identical; on the fixture's cases also against the fixture directly.  Bit equality is derived, not measured: the
kernel's d2 and the specification's are the same three f64 products and two f64 sums in the same order, the build keeps
-ffp-contract=off, and the order is ascending (d2, index), which leaves nothing open where distances tie."""
import ctypes as C
import hashlib
import os

import numpy as np
import pytest

import kdtree_spec as S
from kdtree_spec import HYBRID, KNN, LDS_MAX, RADIUS

HERE = os.path.dirname(os.path.abspath(__file__))
INVALID, STATE = 1, 5
CLOUD_CELL = 0.1


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, np.float64), np.ascontiguousarray(b, np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.int64), b.view(np.int64))


def sha(a):
    return np.frombuffer(hashlib.sha256(np.ascontiguousarray(a).tobytes()).digest(), np.uint8)


# ---------------------------------------------------------------------------
# the fixture
# ---------------------------------------------------------------------------
FIXTURE_SEARCHES = {
    "cloud": [(KNN, 1, 0.0), (KNN, 30, 0.0), (KNN, 171, 0.0), (KNN, 2000, 0.0), (KNN, 2005, 0.0), (HYBRID, 10, 0.1),
              (HYBRID, 100, 0.1), (HYBRID, 171, 0.25), (RADIUS, 0, 0.1), (RADIUS, 0, 0.04)],
    "line": [(KNN, 30, 0.0), (KNN, 200, 0.0), (HYBRID, 30, 0.5), (RADIUS, 0, 0.5)],
    "bound": [(HYBRID, 30, 0.3), (RADIUS, 0, 0.3), (HYBRID, 30, 0.2), (RADIUS, 0, 0.2)],
}
FIXTURE_CASES = [(c, s) for c, ss in FIXTURE_SEARCHES.items() for s in ss]


def search_name(s):
    t, cap, r = s
    return "knn%d" % cap if t == KNN else "hybrid%g_%d" % (r, cap) if t == HYBRID else "radius%g" % r


@pytest.fixture(scope="module")
def golden():
    g = np.load(os.path.join(HERE, "golden", "kdtree.npz"))
    return {k: g[k] for k in g.files}


def flat_lists(result, s):
    """(cnt, idx, d2) of a search with all lists end to end, from what spec_search / spec_radius or the library return"""
    if s[0] == RADIUS:
        off, idx, d2 = result
        return np.diff(off).astype(np.int32), idx, d2
    idx, d2, cnt = result
    live = np.arange(idx.shape[1])[None, :] < cnt[:, None]
    return cnt, idx[live], d2[live]


def check_against_fixture(g, case, s, result):
    cnt, idx, d2 = flat_lists(result, s)
    name = "%s_%s" % (case, search_name(s))
    assert np.array_equal(cnt, g[name + "_cnt"]), name
    assert np.array_equal(sha(idx.astype(np.int32)), g[name + "_idx_sha"]), name
    assert np.array_equal(sha(d2), g[name + "_d2_sha"]), name
    off = np.concatenate([[0], np.cumsum(cnt)])
    rows = g[name + "_rows"]
    assert np.array_equal(np.concatenate([idx[off[i]:off[i + 1]] for i in rows]), g[name + "_idx"]), name
    assert same_bits(np.concatenate([d2[off[i]:off[i + 1]] for i in rows]), g[name + "_d2"]), name


def spec_of(tree, queries, s):
    t, cap, r = s
    return S.spec_radius(tree, queries, r) if t == RADIUS else S.spec_search(tree, queries, t, cap, r)


# ---------------------------------------------------------------------------
# CPU: the specification against the reference, and the clouds
# ---------------------------------------------------------------------------
def test_fixture_inputs_are_the_spec_modules(golden):
    tree = S.cloud(2000)
    q = np.concatenate([S.queries_around(tree, 257, 7), S.outside_queries(tree, CLOUD_CELL), S.far_queries(tree)])
    assert same_bits(golden["cloud_tree"], tree) and same_bits(golden["cloud_queries"], q)
    assert same_bits(golden["line_tree"], S.line_cloud(0)) and same_bits(golden["line_queries"], S.line_queries(0))
    bt, bq = S.bound_case()
    assert same_bits(golden["bound_tree"], bt) and same_bits(golden["bound_queries"], bq)
    assert os.path.getsize(os.path.join(HERE, "golden", "kdtree.npz")) < 400 * 1024


@pytest.mark.parametrize("case,s", FIXTURE_CASES, ids=["%s-%s" % (c, search_name(s)) for c, s in FIXTURE_CASES])
def test_specification_gives_the_reference(golden, case, s):
    tree, queries = golden[case + "_tree"], golden[case + "_queries"]
    check_against_fixture(golden, case, s, spec_of(tree, queries, s))


def test_fixture_lists_have_no_ties_so_the_comparison_is_total(golden):
    for case, s in FIXTURE_CASES:
        d2, ok = S.spec_pairs(golden[case + "_tree"], golden[case + "_queries"], s[0], s[2])
        for row, keep in zip(d2, ok):
            assert (np.diff(np.sort(row[keep])) > 0).all(), (case, s)
        name = "%s_%s" % (case, search_name(s))
        cnt = golden[name + "_cnt"][golden[name + "_rows"]]
        at = np.concatenate([[0], np.cumsum(cnt)])
        for a, b in zip(at[:-1], at[1:]):                            # the stored lists come back ascending
            assert (np.diff(golden[name + "_d2"][a:b]) > 0).all(), name


def test_degenerate_arguments_of_the_reference(golden):
    g = golden
    tree, q = g["deg_tree"], g["deg_queries"]
    assert len(tree) == 5 and (g["deg_knn8_cnt"] == 5).all()        # knn > n: the list holds n
    idx, d2, cnt = S.spec_search(tree, q, KNN, 8)
    assert np.array_equal(idx[:, :5].ravel(), g["deg_knn8_idx"]) and same_bits(d2[:, :5].ravel(), g["deg_knn8_d2"])
    assert (g["deg_knn_negative"] == -1).all() and (g["deg_max_nn_negative"] == -1).all() and (g["deg_empty_tree"] == -1).all()
    # a negative radius is squared: the answer of its absolute value
    off, idx, d2 = S.spec_radius(tree, q, 0.5)
    assert np.array_equal(np.diff(off), g["deg_radius_negative_cnt"]) and np.array_equal(idx, g["deg_radius_negative_idx"])
    assert same_bits(d2, g["deg_radius_negative_d2"])
    cnt, idx, d2 = flat_lists(S.spec_search(tree, q, HYBRID, 3, 0.5), (HYBRID, 3, 0.5))
    assert np.array_equal(cnt, g["deg_hybrid_negative_cnt"]) and np.array_equal(idx, g["deg_hybrid_negative_idx"])
    assert same_bits(d2, g["deg_hybrid_negative_d2"])


def knn_cell(tree, knn):
    """the first cell edge NnGrid::build plans for a KNN grid: 0.6 diagonal sqrt(knn / n)"""
    return 0.6 * S.diagonal(tree) * np.sqrt(min(knn, len(tree)) / len(tree))


def test_queries_lie_where_they_should():
    tree = S.cloud(2000)
    lo, hi = tree.min(0), tree.max(0)
    q = S.queries_around(tree, 257, 7)
    hit = (S.spec_pairs(tree, q, KNN, 0.0)[0] == 0.0).any(1)
    inside = ((q >= lo) & (q <= hi)).all(1)
    assert 80 <= hit.sum() <= 90 and inside.sum() >= 170 and (~inside).sum() >= 60
    out = S.outside_queries(tree, CLOUD_CELL)
    assert out.shape == (12, 3)
    beyond = np.maximum(lo - out, out - hi).max(1) / CLOUD_CELL       # how far outside, in cells
    assert np.allclose(beyond, [0.4, 3.7] * 6) and (np.sum((out < lo) | (out > hi), 1) == 1).all()
    faces = {(int(np.argmax((o < lo) | (o > hi))), bool((o > hi).any())) for o in out}
    assert len(faces) == 6
    # hybrid with the cell as radius: the near ones find partners, the far ones cannot
    cnt = S.spec_search(tree, out, HYBRID, 30, CLOUD_CELL)[2]
    assert cnt[0::2].sum() > 0 and not cnt[1::2].any()


def test_far_queries_the_old_rule_scans_the_whole_grid_the_new_one_does_not():
    tree = S.cloud(2000)
    far = S.far_queries(tree)
    d = S.diagonal(tree)
    dist = np.sqrt(S.spec_pairs(tree, far, KNN, 0.0)[0].min(1))
    assert (dist > 999 * d).all() and (dist < 1001 * d).all()
    for knn in (1, 30):
        cell = knn_cell(tree, knn)
        for k, q in enumerate(far):
            old, whole = S.rings_scanned(tree, q, knn, cell, "old")
            new, _ = S.rings_scanned(tree, q, knn, cell, "new")
            assert old == whole and whole >= 4, (knn, old, whole)  # the covered radius never reaches the query's distance
            # along the box's longest axis and along its diagonal the new bound stops early.  Along its SHORTEST axis (-z) it
            # cannot: rings are cubes of cells, and the ring that closes the faces across x is the last ring of the grid
            assert new < whole if k != 1 else new <= whole, (knn, k, new, whole)
        # a query of the cloud: neither rule scans the whole grid
        old, whole = S.rings_scanned(tree, tree[0], knn, cell, "old")
        new, _ = S.rings_scanned(tree, tree[0], knn, cell, "new")
        assert old < whole and new <= old


def test_line_bound_tie_and_nonfinite_cases():
    for axis in range(3):
        p, q = S.line_cloud(axis), S.line_queries(axis)
        assert (np.ptp(p, axis=0) > 0).tolist() == [k == axis for k in range(3)]
        off_line = (np.abs(q - p[0])[:, [k for k in range(3) if k != axis]] > 0).any(1)
        assert off_line.tolist() == [True, True, False, True, False, True]
    tree, queries = S.bound_case()
    ups = []
    for r in S.BOUND_RADII:
        r2 = float(np.float32(r * r))
        ups.append(r2 > r * r)
        d2, ok = S.spec_pairs(tree, queries, HYBRID, r)
        below, on, above = (d2 == np.nextafter(r2, -np.inf)), (d2 == r2), (d2 == np.nextafter(r2, np.inf))
        assert (below.sum(1) == 1).all() and (on.sum(1) == 1).all() and (above.sum(1) == 1).all()
        assert ok[below].all() and not ok[on].any() and not ok[above].any()
    assert ups == [True, False]                                     # one bound rounds up, one down
    assert not (S.spec_pairs(tree, queries, KNN, 0.0)[0] == 0.0).any()          # the queries are no points of the tree
    tree, copies, queries = S.tie_case()
    assert len(copies) == 300 and len(np.unique(tree, axis=0)) == 201
    d2 = S.spec_pairs(tree, queries, KNN, 0.0)[0]
    assert all(len(np.unique(row[copies])) == 1 for row in d2) and d2[0, copies[0]] == 0.0
    for cap in (30, 171, 300):
        idx, _, cnt = S.spec_search(tree, queries[:2], KNN, cap)
        assert (idx == copies[:cap]).all() and (cnt == cap).all()  # the lowest indices among the copies: the index decides
    tree, a, b, nan_row = S.nonfinite_cloud()
    q = S.nonfinite_queries()
    idx, d2, cnt = S.spec_search(tree, q, KNN, 12)
    assert cnt.tolist() == [0, 12, 12, 0, 0, 12, 12]
    assert np.isposinf(d2[[1, 2, 5]]).all() and np.isfinite(d2[6]).all()
    finite = np.nonzero(np.isfinite(tree).all(1))[0]
    assert (idx[[1, 2, 5]] == finite[:12]).all()                    # an infinite query: the lowest indices, at +inf
    assert S.spec_search(tree, q, HYBRID, 12, 0.3)[2].tolist() == [0, 0, 0, 0, 0, 0, 12]
    assert np.diff(S.spec_radius(tree, q, 0.3)[0]).tolist()[:6] == [0] * 6
    live = np.arange(12)[None, :] < cnt[:, None]
    assert not (np.isin(idx, [a, nan_row]) & live).any()


def test_argument_errors_are_refused_before_any_launch(lib):
    """without a device no tree can be made: a NULL tree and a bad create are refused with INVALID all the same"""
    L = lib.load()
    dp, ip, lp = C.POINTER(C.c_double), C.POINTER(C.c_int32), C.POINTER(C.c_int64)
    q = np.zeros((2, 3)); idx = np.zeros((2, 4), np.int32); d2 = np.zeros((2, 4)); cnt = np.zeros(2, np.int32)
    off = np.zeros(3, np.int64); total = C.c_int64(0)
    Q, I, D, N = q.ctypes.data_as(dp), idx.ctypes.data_as(ip), d2.ctypes.data_as(dp), cnt.ctypes.data_as(ip)
    assert L.visma_icp_kdtree_search_knn(None, Q, 2, 4, I, D, N) == INVALID
    assert L.visma_icp_kdtree_search_hybrid(None, Q, 2, 0.5, 4, I, D, N) == INVALID
    assert L.visma_icp_kdtree_search_radius(None, Q, 2, 0.5, off.ctypes.data_as(lp), C.byref(total)) == INVALID
    assert L.visma_icp_kdtree_get_radius_result(None, I, D) == INVALID
    assert L.visma_icp_kdtree_destroy(None) == INVALID and L.visma_icp_kdtree_size(None) == 0
    t = C.c_void_p()
    assert L.visma_icp_kdtree_create(None, Q, 2, C.byref(t)) == INVALID and not t.value


# ---------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ctx(lib):
    c = lib.Context(0)
    yield c
    c.close()


def run(kd, queries, s):
    t, cap, r = s
    return kd.search_radius(queries, r) if t == RADIUS else kd.search_knn(queries, cap) if t == KNN else kd.search_hybrid(queries, r, cap)


def check(kd, tree, queries, s, want=None):
    """one search against the specification, and a second call against the first -> what the library returned"""
    want = spec_of(tree, queries, s) if want is None else want
    got = run(kd, queries, s)
    what = (len(tree), len(queries), s)
    if s[0] == RADIUS:
        (off, idx, d2), (woff, widx, wd2) = got, want
        assert off.dtype == np.int64 and idx.dtype == np.int32
        assert np.array_equal(off, woff), (what, "offsets")
        assert np.array_equal(idx, widx), (what, "idx", int((idx != widx).sum()))
        assert same_bits(d2, wd2), (what, "d2")
    else:
        (idx, d2, cnt), (widx, wd2, wcnt) = got, want
        assert idx.shape == (len(queries), s[1]) and d2.shape == idx.shape and cnt.shape == (len(queries),)
        assert np.array_equal(cnt, wcnt), (what, "cnt", int((cnt != wcnt).sum()))
        rows = np.nonzero((idx != widx).any(1))[0]
        assert not len(rows), (what, len(rows), int(rows[0]), idx[rows[0]].tolist()[:12], widx[rows[0]].tolist()[:12])
        assert same_bits(d2, wd2), (what, "d2")
        live = np.arange(s[1])[None, :] < cnt[:, None]
        assert (idx[~live] == -1).all() and np.isposinf(d2[~live]).all()                # the padding
    again = run(kd, queries, s)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(got, again)), (what, "a second call differs")
    return got


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 2000])
def test_tree_sizes_query_counts_and_caps(ctx, n):
    tree = S.cloud(n)
    with ctx.kdtree(tree) as kd:
        assert len(kd) == n and ctx.L.visma_icp_kdtree_size(kd._t) == n
        for nq in (0, 1, 64, 65, 257):
            q = S.queries_around(tree, nq, 50 + nq)
            for s in ((KNN, 1, 0.0), (KNN, n, 0.0), (KNN, n + 5, 0.0), (HYBRID, 10, 0.3), (HYBRID, n + 5, 0.3), (RADIUS, 0, 0.3)):
                if s[1] > 200 and nq not in (1, 257):
                    continue                                         # (the long lists of the 2,000-point tree: two query counts)
                got = check(kd, tree, q, s)
                if s[0] == KNN and nq:
                    assert (got[1][0::3, 0] == 0.0).all()           # every third query is a point of the tree: d2 = 0 first


@pytest.mark.gpu
def test_lds_list_and_global_heap_agree_at_170(ctx):
    tree = S.cloud(400)
    q = S.queries_around(tree, 65, 3)
    with ctx.kdtree(tree) as kd:
        for t, r in ((KNN, 0.0), (HYBRID, 0.6)):
            lds = check(kd, tree, q, (t, LDS_MAX, r))
            heap = check(kd, tree, q, (t, LDS_MAX + 1, r))          # the first cap that takes the global heap
            assert (lds[2] == LDS_MAX).all() if t == KNN else (lds[2] == LDS_MAX).any()
            assert np.array_equal(heap[0][:, :LDS_MAX], lds[0]) and same_bits(heap[1][:, :LDS_MAX], lds[1])


@pytest.mark.gpu
def test_queries_of_more_than_one_slab(ctx):
    """2,100 queries x knn 2,000 = 4.2e6 entries: more than the 2^22 of one launch (heap lists); and 36,000 x 117 (LDS lists)"""
    tree = S.cloud(2000)
    with ctx.kdtree(tree) as kd:
        q = S.queries_around(tree, 2100, 11)
        assert len(q) * 2000 > S.SLAB_ENTRIES > 2000 * 2000
        check(kd, tree, q, (KNN, 2000, 0.0))
    tree = S.cloud(150)
    with ctx.kdtree(tree) as kd:
        q = S.queries_around(tree, 36000, 12)
        assert len(q) * 117 > S.SLAB_ENTRIES
        check(kd, tree, q, (HYBRID, 117, 0.4))


@pytest.mark.gpu
def test_queries_outside_the_box_and_far_away(ctx):
    tree = S.cloud(2000)
    far = S.far_queries(tree)
    with ctx.kdtree(tree) as kd:
        for cell in (CLOUD_CELL, 0.02):
            out = S.outside_queries(tree, cell)
            for s in ((HYBRID, 30, cell / 1.001), (RADIUS, 0, cell / 1.001), (RADIUS, 0, 5 * cell), (KNN, 30, 0.0), (KNN, 1, 0.0)):
                check(kd, tree, np.concatenate([out, far]), s)
        for s in ((KNN, 1, 0.0), (KNN, 30, 0.0), (KNN, 171, 0.0), (KNN, 2000, 0.0)):
            idx, d2, cnt = check(kd, tree, far, s)
            assert (cnt == s[1]).all() and (d2[:, 0] > (999 * S.diagonal(tree)) ** 2).all()
        assert not check(kd, tree, far, (HYBRID, 5, 0.5))[2].any()
        assert not check(kd, tree, far, (RADIUS, 0, 0.5))[0].any()


@pytest.mark.gpu
@pytest.mark.parametrize("axis", [0, 1, 2])
def test_a_cloud_one_cell_wide_in_two_axes(ctx, axis):
    tree, q = S.line_cloud(axis), S.line_queries(axis)
    with ctx.kdtree(tree) as kd:
        for s in ((KNN, 30, 0.0), (KNN, 200, 0.0), (KNN, 500, 0.0), (HYBRID, 30, 0.5), (RADIUS, 0, 0.5), (RADIUS, 0, 45.0)):
            check(kd, tree, q, s)


@pytest.mark.gpu
def test_radius_extremes(ctx):
    tree = S.cloud(300)
    q = S.queries_around(tree, 300, 5)
    with ctx.kdtree(tree) as kd:
        off, idx, d2 = check(kd, tree, q[1::3], (RADIUS, 0, 1e-7))  # (no points of the tree among them) matches nothing
        assert not off.any() and len(idx) == 0 and len(d2) == 0
        assert not check(kd, tree, q[1::3], (HYBRID, 5, 1e-7))[2].any()
        off, idx, d2 = check(kd, tree, q, (RADIUS, 0, 10.0))        # every point for every query
        assert off[-1] == 90000 and (np.diff(off) == 300).all()
        assert (np.sort(idx.reshape(300, 300), 1) == np.arange(300)).all()


@pytest.mark.gpu
def test_the_radius_boundary(ctx):
    tree, q = S.bound_case()
    with ctx.kdtree(tree) as kd:
        for r in S.BOUND_RADII:
            r2 = float(np.float32(r * r))
            idx, d2, cnt = check(kd, tree, q, (HYBRID, 30, r))
            assert (cnt < 30).all() and (d2[np.arange(6), cnt - 1] == np.nextafter(r2, -np.inf)).all()
            off, idx, d2 = check(kd, tree, q, (RADIUS, 0, r))
            assert (d2[off[1:] - 1] == np.nextafter(r2, -np.inf)).all()                 # one ulp below: the last of each list


@pytest.mark.gpu
def test_ties_the_index_decides(ctx):
    tree, copies, q = S.tie_case()
    with ctx.kdtree(tree) as kd:
        for s in ((KNN, 30, 0.0), (KNN, LDS_MAX, 0.0), (KNN, LDS_MAX + 1, 0.0), (KNN, 300, 0.0), (KNN, 350, 0.0), (HYBRID, 30, 0.1),
                  (HYBRID, 200, 0.1), (RADIUS, 0, 0.1), (RADIUS, 0, 1.2)):
            got = check(kd, tree, q, s)
            if s[0] == KNN and s[1] <= 300:
                assert (got[0][:2] == copies[:s[1]]).all()          # at the cut too: the lowest indices among the copies


@pytest.mark.gpu
def test_non_finite_queries_and_points(ctx):
    tree = S.nonfinite_cloud()[0]
    q = np.concatenate([S.nonfinite_queries(), S.queries_around(tree[np.isfinite(tree).all(1)], 60, 8)])
    with ctx.kdtree(tree) as kd:
        for s in ((KNN, 12, 0.0), (KNN, LDS_MAX + 1, 0.0), (KNN, 600, 0.0), (KNN, 605, 0.0), (HYBRID, 30, 0.3), (HYBRID, 200, 0.6),
                  (RADIUS, 0, 0.3)):
            check(kd, tree, q, s)
    tree = np.full((40, 3), np.nan)                                 # no distance is a number
    tree[::2, 0] = np.inf
    with ctx.kdtree(tree) as kd:
        for s in ((KNN, 5, 0.0), (HYBRID, 5, 0.3), (RADIUS, 0, 0.3)):
            got = check(kd, tree, q[:10], s)
            assert not (got[0] if s[0] == RADIUS else got[2]).any()


@pytest.mark.gpu
def test_the_grid_is_kept_and_rebuilt(ctx):
    tree = S.cloud(2000)
    q = S.queries_around(tree, 257, 13)
    order = [(RADIUS, 0, 0.07), (HYBRID, 20, 0.07), (RADIUS, 0, 0.2), (KNN, 12, 0.0), (HYBRID, 20, 0.2), (KNN, 40, 0.0), (RADIUS, 0, 0.07),
             (KNN, 12, 0.0)]
    with ctx.kdtree(tree) as kd:
        got = [check(kd, tree, q, s) for s in order]
    for s, g in zip(order, got):                                    # ... and the same as on a fresh tree
        with ctx.kdtree(tree) as fresh:
            f = run(fresh, q, s)
        assert all(x.tobytes() == y.tobytes() for x, y in zip(g, f)), s


@pytest.mark.gpu
def test_argument_errors_leave_the_tree_usable(ctx, lib):
    L = ctx.L
    dp, ip, lp = C.POINTER(C.c_double), C.POINTER(C.c_int32), C.POINTER(C.c_int64)
    tree = S.cloud(64)
    q = np.ascontiguousarray(S.queries_around(tree, 5, 2))
    idx = np.zeros((5, 4), np.int32); d2 = np.zeros((5, 4)); cnt = np.zeros(5, np.int32); off = np.zeros(6, np.int64); total = C.c_int64(7)
    Q, I, D, N, O = q.ctypes.data_as(dp), idx.ctypes.data_as(ip), d2.ctypes.data_as(dp), cnt.ctypes.data_as(ip), off.ctypes.data_as(lp)
    t = C.c_void_p()
    assert L.visma_icp_kdtree_create(ctx._h, Q, 0, C.byref(t)) == INVALID and not t.value
    assert L.visma_icp_kdtree_create(ctx._h, None, 5, C.byref(t)) == INVALID and not t.value
    assert L.visma_icp_kdtree_create(ctx._h, Q, 5, None) == INVALID
    with ctx.kdtree(tree) as kd:
        T = kd._t
        assert L.visma_icp_kdtree_get_radius_result(T, I, D) == STATE                  # no radius search yet
        assert L.visma_icp_kdtree_search_knn(T, Q, -1, 4, I, D, N) == INVALID
        assert L.visma_icp_kdtree_search_hybrid(T, Q, -1, 0.5, 4, I, D, N) == INVALID
        assert L.visma_icp_kdtree_search_radius(T, Q, -1, 0.5, O, C.byref(total)) == INVALID
        for cap in (0, -1):
            assert L.visma_icp_kdtree_search_knn(T, Q, 5, cap, I, D, N) == INVALID
            assert L.visma_icp_kdtree_search_hybrid(T, Q, 5, 0.5, cap, I, D, N) == INVALID
        for r in (0.0, -1.0, float("nan"), float("inf"), float("-inf")):
            assert L.visma_icp_kdtree_search_hybrid(T, Q, 5, r, 4, I, D, N) == INVALID
            assert L.visma_icp_kdtree_search_radius(T, Q, 5, r, O, C.byref(total)) == INVALID
        assert L.visma_icp_kdtree_search_knn(T, None, 5, 4, I, D, N) == INVALID
        assert L.visma_icp_kdtree_search_knn(T, Q, 5, 4, None, D, N) == INVALID
        assert L.visma_icp_kdtree_search_radius(T, Q, 5, 0.5, None, C.byref(total)) == INVALID
        assert not idx.any() and not d2.any() and not cnt.any() and not off.any() and total.value == 7
        with pytest.raises(lib.IcpError) as e:
            kd.search_knn(q, 0)
        assert e.value.code == INVALID
        assert L.visma_icp_kdtree_search_knn(T, Q, 0, 4, I, D, N) == 0                  # nq == 0 is not an error
        assert L.visma_icp_kdtree_search_radius(T, Q, 0, 0.5, O, C.byref(total)) == 0 and total.value == 0
        assert L.visma_icp_kdtree_get_radius_result(T, None, None) == 0                 # ... and its result is empty
        for s in ((KNN, 4, 0.0), (HYBRID, 4, 0.5), (RADIUS, 0, 0.5)):                   # the tree is as usable as before
            check(kd, tree, q, s)


@pytest.mark.gpu
@pytest.mark.parametrize("case", sorted(FIXTURE_SEARCHES))
def test_library_gives_the_reference(ctx, golden, case):
    tree, queries = golden[case + "_tree"], golden[case + "_queries"]
    with ctx.kdtree(tree) as kd:
        for s in FIXTURE_SEARCHES[case]:
            check_against_fixture(golden, case, s, check(kd, tree, queries, s))
    if case == "cloud":                                             # knn > n on the 5-point tree: the list holds n
        with ctx.kdtree(golden["deg_tree"]) as kd:
            idx, d2, cnt = kd.search_knn(golden["deg_queries"], 8)
            assert (cnt == 5).all() and np.array_equal(idx[:, :5].ravel(), golden["deg_knn8_idx"])
            assert same_bits(d2[:, :5].ravel(), golden["deg_knn8_d2"]) and (idx[:, 5:] == -1).all()
