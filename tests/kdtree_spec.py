"""The specification of the public neighbour search (visma_icp_kdtree_*, visma_amd/csrc/kdtree.hip), shared by
tests/test_kdtree.py, tests/test_kdtree_shim.py and tests/golden/gen_kdtree.py: an exhaustive f64 scan per query.

The rules are nn_spec's, for queries that need not be points of the cloud: d2 = ((dx*dx) + dy*dy) + dz*dz in f64 with
d = query - point (flann/algorithms/dist.h:159-176), a list ascending in (d2, index), Radius / Hybrid: d2 <
(double)(float)(r*r), strictly (KDTreeFlann.cpp:157-158, 184-185).  A neighbour at a NaN distance is never listed; one at an
infinite distance is a legitimate KNN entry, behind every finite one.

Also here: the clouds and queries of the tests, each from a seed or a formula, and the model of the KNN stopping rules
(nn_list.h) that says how many rings of cells a query scans."""
import numpy as np

from nn_spec import nonfinite_cloud  # noqa: F401  (re-exported: the tests take every cloud from here)

KNN, RADIUS, HYBRID = 0, 1, 2
LDS_MAX = 170           # kNormalsMaxList: the longest list the LDS holds
SLAB_ENTRIES = 1 << 22  # kKdTreeSlabEntries: the list entries of one KNN / Hybrid launch


def spec_pairs(tree, queries, search_type, radius):
    """-> d2 (nq, n) and ok (nq, n): which points a list of the search type may hold"""
    p = np.asarray(tree, np.float64).reshape(-1, 3)
    q = np.asarray(queries, np.float64).reshape(-1, 3)
    with np.errstate(invalid="ignore", over="ignore"):
        d = q[:, None, :] - p[None, :, :]
        d2 = d[..., 0] * d[..., 0]
        d2 = d2 + d[..., 1] * d[..., 1]
        d2 = d2 + d[..., 2] * d[..., 2]
    ok = ~np.isnan(d2)
    if search_type != KNN:
        with np.errstate(invalid="ignore"):
            ok &= d2 < float(np.float32(radius * radius))
    return d2, ok


def _ordered(tree, queries, search_type, radius):
    d2, ok = spec_pairs(tree, queries, search_type, radius)
    key = np.where(ok, d2, np.inf)
    order = np.argsort(key, axis=1, kind="stable")                  # stable: ties in ascending index
    out = ~np.take_along_axis(ok, order, 1)                         # a listed neighbour at +inf comes before what is not listed
    order = np.take_along_axis(order, np.argsort(out, axis=1, kind="stable"), 1)
    return order, np.take_along_axis(key, order, 1), ok.sum(1)


def spec_search(tree, queries, search_type, cap, radius=0.0):
    """KNN / Hybrid as the C ABI returns them -> idx (nq, cap) int32 padded with -1, d2 (nq, cap) padded with +inf, cnt (nq,)
    int32: the min(cap, n) first of every query's ordered neighbours"""
    order, d2, found = _ordered(tree, queries, search_type, radius)
    n = order.shape[1]
    cnt = np.minimum(found, min(cap, n))
    idx = np.full((len(order), cap), -1, np.int32)
    out = np.full((len(order), cap), np.inf)
    m = min(cap, n)
    live = np.arange(m)[None, :] < cnt[:, None]
    idx[:, :m] = np.where(live, order[:, :m], -1)
    out[:, :m] = np.where(live, d2[:, :m], np.inf)
    return idx, out, cnt.astype(np.int32)


def spec_radius(tree, queries, radius):
    """Radius as the C ABI returns it -> offsets (nq + 1) int64, idx (total) int32, d2 (total)"""
    order, d2, found = _ordered(tree, queries, RADIUS, radius)
    offsets = np.concatenate([[0], np.cumsum(found)]).astype(np.int64)
    live = np.arange(order.shape[1])[None, :] < found[:, None]
    return offsets, order[live].astype(np.int32), d2[live]


# ---------------------------------------------------------------------------
# clouds and queries
# ---------------------------------------------------------------------------
def cloud(n, seed=None):
    """n random points of the box [0, 1] x [0, 0.8] x [0, 0.5]"""
    return np.random.default_rng(1000 + n if seed is None else seed).random((n, 3)) * [1.0, 0.8, 0.5]


def queries_around(tree, nq, seed):
    """nq queries: a third points of the tree (d2 = 0 first), a third inside its box, a third up to half a box outside"""
    rng = np.random.default_rng(seed)
    lo, hi = tree.min(0), tree.max(0)
    q = lo + (hi - lo) * rng.uniform(-0.5, 1.5, (nq, 3))
    inside = np.arange(nq) % 3 == 1
    q[inside] = lo + (hi - lo) * rng.random((int(inside.sum()), 3))
    hits = np.arange(nq) % 3 == 0
    q[hits] = tree[rng.integers(0, len(tree), int(hits.sum()))]
    return q


def outside_queries(tree, cell, steps=(0.4, 3.7)):
    """for each of the six faces of the tree's bounding box and each step (in cells of edge `cell`): a query that far
    beyond the face, over a seeded place of the face -> (12, 3)"""
    rng = np.random.default_rng(3)
    lo, hi = tree.min(0), tree.max(0)
    out = []
    for axis in range(3):
        for side in (0, 1):
            for s in steps:
                q = lo + (hi - lo) * rng.random(3)
                q[axis] = hi[axis] + s * cell if side else lo[axis] - s * cell
                out.append(q)
    return np.array(out)


def diagonal(tree):
    return float(np.linalg.norm(tree.max(0) - tree.min(0)))


def far_queries(tree):
    """1,000 cloud diagonals away: along +x, along -z, and along the diagonal of the box -> (3, 3)"""
    c, d = tree.mean(0), diagonal(tree)
    return np.array([c + [1000 * d, 0, 0], c - [0, 0, 1000 * d], c + 1000 * d * np.ones(3) / np.sqrt(3.0)])


def line_cloud(axis):
    """500 points on a line along `axis`, geometric spacing (1 mm growing by 2 % a step): the grid is one cell wide in the
    other two dimensions (tests/test_nn_lists.py, line_cloud)"""
    p = np.tile([0.3, -0.2, 0.7], (500, 1))
    p[:, axis] = 1e-3 * (1.02 ** np.arange(500) - 1.0) / 0.02
    return p


def line_queries(axis):
    """off the line: beside its dense end, beside its sparse end, beyond either end, and one on it -> (6, 3)"""
    p = line_cloud(axis)
    a, b = (axis + 1) % 3, (axis + 2) % 3
    q = np.tile(p[0], (6, 1))
    q[0, axis] = p[40, axis]; q[0, a] += 0.05
    q[1, axis] = p[480, axis]; q[1, b] -= 0.3
    q[2, axis] = p[0, axis] - 0.5
    q[3, axis] = p[-1, axis] + 2.0; q[3, a] += 1.0
    q[4] = p[250]
    q[5, axis] = p[300, axis]; q[5, a] -= 40.0; q[5, b] += 30.0
    return q


def _bound_points(q, direction, r2, x_share=0.999):
    """three points p with the specification's d2(q, p) one ulp below r2, equal to r2 and one ulp above it: the first offset
    coordinate fixed at sqrt(r2) * x_share, the second found by bisection over the f64 values (d2 is monotone in it).  The
    construction of tests/test_nn_lists.py, restated."""
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
        assert d2_of(hi) == target, (q, direction, target)
        out.append(p.copy())
    return out


BOUND_RADII = (0.3, 0.2)          # (float)(r * r) rounds up / down


def bound_case():
    """-> (tree, queries): six queries, NOT points of the tree, each a unit from the origin along the axis its three points
    do not use (their offsets stay as exact as near the origin); for either radius and every query three points of the tree at
    d2 = bound - 1 ulp, bound, bound + 1 ulp; 1,000 random points around them.  (Apart: the three points of one query, one ulp
    apart in a coordinate, are out of every other query's reach -- from there they would tie.)"""
    rng = np.random.default_rng(17)
    queries = np.array([[0, 0, 0], [1, 2, 3], [-3, 1, 2], [2, -1, -2], [5, 5, 0], [0, -4, 4]], np.float64) / 1024.0
    dirs = [(0, 1), (1, 2), (2, 0), (1, 0), (2, 1), (0, 2)]
    for k, (q, d) in enumerate(zip(queries, dirs)):
        q[3 - d[0] - d[1]] += 1.0 if k < 3 else -1.0
    pts = []
    for r in BOUND_RADII:
        r2 = float(np.float32(r * r))
        for q, d in zip(queries, dirs):
            pts += _bound_points(q, d, r2)
    pts += list(rng.uniform(-1.5, 1.5, (1000, 3)))
    return np.array(pts), queries


def tie_case():
    """-> (tree, copies, queries): 300 copies of one point among 200 random ones in a seeded order; queries: the point
    itself, a point nearby, and one outside the box -- every copy is at the same distance from each"""
    rng = np.random.default_rng(23)
    p = rng.random((500, 3))
    copies = np.sort(rng.permutation(500)[:300])
    p[copies] = [0.4, 0.55, 0.35]
    return p, copies, np.array([[0.4, 0.55, 0.35], [0.41, 0.54, 0.36], [1.5, 0.55, 0.35]])


def nonfinite_queries():
    """queries with a NaN, a +inf and a -inf coordinate, a row entirely NaN, one with both inf and NaN, and a finite one"""
    return np.array([[0.5, np.nan, 0.05], [np.inf, 0.5, 0.05], [0.5, 0.5, -np.inf], [np.nan] * 3, [np.inf, np.nan, 0.0],
                     [-np.inf, np.inf, 0.05], [0.5, 0.5, 0.05]])


# ---------------------------------------------------------------------------
# the KNN stopping rules of nn_list.h, modelled: how many rings of cells a query scans
# ---------------------------------------------------------------------------
def rings_scanned(tree, query, knn, cell, rule):
    """The rings R = 0, 1, ... of cells of edge `cell` (a grid over the tree's bounding box, dim = floor(extent / cell) + 1
    an axis, the query clamped into it) that a KNN search scans before it stops -> (rings scanned, rings of the whole grid).
    rule "old": list full and farthest <= (R * cell * 0.999)^2.  rule "new": list full and farthest < the squared distance
    from the query to the nearest slab of the grid's box beyond a face of the scanned block that still has cells beyond it,
    every length 0.1 % of R + 1 cells short."""
    tree = np.asarray(tree, np.float64)
    lo = tree.min(0)
    dim = np.floor((tree.max(0) - lo) / cell).astype(int) + 1
    cells = np.clip(np.floor((tree - lo) / cell).astype(int), 0, dim - 1)
    c = np.clip(np.floor((query - lo) / cell), 0, dim - 1).astype(int)
    d2 = ((query - tree) ** 2).sum(1)
    ring = np.abs(cells - c).max(1)
    whole = int(max(c.max(), (dim - 1 - c).max()))
    u = query - lo
    for R in range(whole + 1):
        if R == whole:
            return R + 1, whole + 1
        seen = np.sort(d2[ring <= R])
        if len(seen) < knn:
            continue
        far = seen[knn - 1]
        if rule == "old":
            if R >= 1 and far <= (R * cell * 0.999) ** 2:
                return R + 1, whole + 1
            continue
        slack = 1e-3 * (R + 1) * cell
        out = np.maximum(np.maximum(-u, u - dim * cell) - slack, 0.0)
        best = np.inf
        for a in range(3):
            rest = out[(a + 1) % 3] ** 2 + out[(a + 2) % 3] ** 2
            if c[a] - R > 0:
                best = min(best, max(u[a] - (c[a] - R) * cell - slack, 0.0) ** 2 + rest)
            if c[a] + R < dim[a] - 1:
                best = min(best, max((c[a] + R + 1) * cell - u[a] - slack, 0.0) ** 2 + rest)
        if far < best:
            return R + 1, whole + 1
    raise AssertionError("unreachable")
