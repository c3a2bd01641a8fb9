"""The specification of the neighbour lists under normal estimation, the colour gradient and FPFH (visma_amd/csrc/nn_list.h),
shared by tests/test_fpfh_fgr.py, tests/test_nn_lists.py and tests/test_normals.py: an exhaustive f64 scan in flann's order.

d2 = ((dx*dx) + dy*dy) + dz*dz in f64 (flann/algorithms/dist.h:159-176), the list ascending in (d2, index), Radius / Hybrid:
d2 < (double)(float)(r*r), strictly (KDTreeFlann.cpp:157-158, 184-185).  A neighbour at a NaN distance is never listed, in any
search type; one at an infinite distance is a legitimate KNN entry, behind every finite one."""
import numpy as np


def spec_pairs(xyz, search_type, radius):
    """-> d2 (n, n) and ok (n, n): which pairs a list of the search type may hold (0 KNN, 1 Radius, 2 Hybrid)"""
    p = np.asarray(xyz, np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        d = p[:, None, :] - p[None, :, :]
        d2 = d[..., 0] * d[..., 0]
        d2 = d2 + d[..., 1] * d[..., 1]
        d2 = d2 + d[..., 2] * d[..., 2]
    ok = ~np.isnan(d2)
    if search_type != 0:
        if not (np.isfinite(radius) and radius > 0):
            ok[:] = False
        else:
            with np.errstate(invalid="ignore"):
                ok &= d2 < float(np.float32(radius * radius))
    return d2, ok


def spec_lists(xyz, search_type, knn, radius):
    """Brute-force neighbour lists in flann's order: ascending (d2, index), d2 = ((dx*dx) + dy*dy) + dz*dz in f64;
    Hybrid: d2 < (double)(float)(r*r), strictly.  A NaN distance is never listed.  -> idx (n, cap), d2 (n, cap), cnt (n,);
    cap = min(knn, n); behind its cnt entries a row holds +inf and indices that mean nothing."""
    d2, ok = spec_pairs(xyz, search_type, radius)
    cap = min(knn, len(d2))
    key = np.where(ok, d2, np.inf)
    order = np.argsort(key, axis=1, kind="stable")                  # stable: ties in ascending index
    # a listed neighbour at +inf comes before every pair that is not listed
    out = ~np.take_along_axis(ok, order, 1)
    order = np.take_along_axis(order, np.argsort(out, axis=1, kind="stable"), 1)[:, :cap]
    cnt = np.minimum(ok.sum(1), cap)
    return order.astype(np.int64), np.take_along_axis(key, order, 1), cnt


def spec_radius_count(xyz, radius):
    """the Radius search: how many points lie within the bound of every point (itself included) -> cnt (n,)"""
    return spec_pairs(xyz, 1, radius)[1].sum(1)


def nonfinite_cloud(n=600, seed=21, a=100, b=400, nan_row=250):
    """`n` random points of [0, 1]^2 x [0, 0.1] with one NaN coordinate (point a), one +inf coordinate (point b) and one
    row entirely NaN -> (xyz, a, b, nan_row)"""
    rng = np.random.default_rng(seed)
    p = rng.random((n, 3)) * [1.0, 1.0, 0.1]
    p[a, 1] = np.nan
    p[b, 0] = np.inf
    p[nan_row] = np.nan
    return p, a, b, nan_row


def cube_cloud(shuffled=False, seed=5):
    """the 9 x 9 x 9 lattice of spacing 0.125 (every coordinate and every d2 exact in f64: ties are exact ties); shuffled:
    the same points in a seeded random order, so that the index tie-break does not follow the lattice"""
    i, j, k = np.meshgrid(np.arange(9), np.arange(9), np.arange(9), indexing="ij")
    p = np.stack([i.ravel(), j.ravel(), k.ravel()], 1) * 0.125
    return p[np.random.default_rng(seed).permutation(len(p))] if shuffled else p
