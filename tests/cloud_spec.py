"""The specification of the PointCloud operations on the device (visma_icp_cloud_*; include/visma_icp.h): a plain numpy
restatement of the reference's Core/Geometry/PointCloud.h, PointCloud.cpp :47-198, DownSample.cpp :90-105 and :222-254 and
EstimateNormals.cpp :158-204, with Eigen's normalize() (Dot.h) and its 3 x 3 inverse (LU/InverseImpl.h).
tests/test_cloud_spec.py pins it to the compiled reference bit for bit (tests/golden/cloud.npz); tests/test_cloud.py pins the
library to it.

A cloud is a dict: points (n x 3 f64), normals, colors (n x 3 f64 or None).  An attribute of no rows is None: the
reference's HasX() is false for it.  The in-place functions change the cloud they are given; select, uniform_down_sample and
crop return a new one.  numpy evaluates one operation per rounding, and np.cumsum adds serially in index order."""
import numpy as np

ATTRS = ("points", "normals", "colors")


def cloud(points, normals=None, colors=None):
    f = lambda a: None if a is None else np.array(a, np.float64).reshape(-1, 3)
    return _settle(dict(points=f(points), normals=f(normals), colors=f(colors)))


def copy(c):
    return {k: None if v is None else v.copy() for k, v in c.items()}


def _settle(c):
    """HasNormals(), HasColors(): nothing is had on no rows"""
    if len(c["points"]) == 0:
        c["normals"] = c["colors"] = None
    return c


def _sum3(a, b, c):
    """a three-term sum as the compiled reference associates it (Eigen's redux over a Vector3d)"""
    return (a + b) + c


# ---- bounds ----
def _extreme(v, largest):
    """std::min_element / max_element with a < b over one coordinate"""
    if len(v) == 0:
        return 0.0
    if np.isnan(v[0]):
        return v[0]                                          # nothing compares less than (or to) a NaN: the first stays
    ok = v[~np.isnan(v)]
    m = ok.max() if largest else ok.min()
    return v[np.nonzero(v == m)[0][0]]                       # among equal values (-0.0 == 0.0) the lowest index


def bounds(c):
    """GetMinBound(), GetMaxBound() -> 6 doubles"""
    p = c["points"]
    return np.array([_extreme(p[:, a], False) for a in range(3)] + [_extreme(p[:, a], True) for a in range(3)], np.float64)


# ---- in place ----
def transform(c, T):
    """a row: ((T_i0 x + T_i1 y) + T_i2 z) + T_i3 w; w = 1 for points, 0 for normals; the fourth row is not read"""
    T = np.asarray(T, np.float64).reshape(4, 4)
    for k, w in (("points", 1.0), ("normals", 0.0)):
        a = c[k]
        if a is None or not len(a):
            continue
        with np.errstate(all="ignore"):
            c[k] = np.stack([((T[r, 0] * a[:, 0] + T[r, 1] * a[:, 1]) + T[r, 2] * a[:, 2]) + T[r, 3] * w for r in range(3)], axis=1)


def _normalized(a):
    """Eigen's normalize() row by row: z = squaredNorm(); if (z > 0) v /= sqrt(z).  (PointCloud.h has no NaN rule.)"""
    with np.errstate(all="ignore"):
        x, y, z = a[:, 0], a[:, 1], a[:, 2]
        n2 = _sum3(x * x, y * y, z * z)
        pos = n2 > 0
        length = np.sqrt(np.where(pos, n2, 1.0))
        return np.where(pos[:, None], a / length[:, None], a)


def normalize_normals(c):
    if c["normals"] is not None:
        c["normals"] = _normalized(c["normals"])


def paint_uniform_color(c, rgb):
    n = len(c["points"])
    if n:
        c["colors"] = np.tile(np.asarray(rgb, np.float64).reshape(1, 3), (n, 1))


def append(c, other):
    """operator+= (PointCloud.cpp:89-115); other may be c"""
    if len(other["points"]) == 0:
        return
    empty = len(c["points"]) == 0
    for k in ("normals", "colors"):
        if (empty or c[k] is not None) and other[k] is not None:
            c[k] = other[k].copy() if empty else np.concatenate([c[k], other[k]])
        else:
            c[k] = None
    c["points"] = np.concatenate([c["points"], other["points"]])


def _norm(a):
    with np.errstate(all="ignore"):
        return np.sqrt(_sum3(a[:, 0] * a[:, 0], a[:, 1] * a[:, 1], a[:, 2] * a[:, 2]))


def _flip_against(nrm, ref):
    with np.errstate(all="ignore"):
        dot = _sum3(nrm[:, 0] * ref[:, 0], nrm[:, 1] * ref[:, 1], nrm[:, 2] * ref[:, 2])
        return np.where((dot < 0.0)[:, None], nrm * -1.0, nrm)


def orient_normals_to_align_with_direction(c, ref):
    """EstimateNormals.cpp:168-175; the cloud has normals"""
    nrm = c["normals"]
    ref = np.tile(np.asarray(ref, np.float64).reshape(1, 3), (len(nrm), 1))
    c["normals"] = np.where((_norm(nrm) == 0.0)[:, None], ref, _flip_against(nrm, ref))


def orient_normals_towards_camera_location(c, camera):
    """EstimateNormals.cpp:188-202; the cloud has normals"""
    nrm = c["normals"]
    with np.errstate(all="ignore"):
        ref = np.asarray(camera, np.float64).reshape(1, 3) - c["points"]
    fresh = np.where((_norm(ref) == 0.0)[:, None], np.array([[0.0, 0.0, 1.0]]), _normalized(ref))
    c["normals"] = np.where((_norm(nrm) == 0.0)[:, None], fresh, _flip_against(nrm, ref))


# ---- a new cloud ----
def select(c, indices):
    idx = np.asarray(indices, np.int64).reshape(-1)
    return _settle({k: None if c[k] is None else c[k][idx] for k in ATTRS})


def uniform_down_sample(c, every_k):
    if every_k == 0:
        return cloud(np.zeros((0, 3)))
    return select(c, np.arange(0, len(c["points"]), every_k))


def crop(c, min_bound, max_bound):
    lo, hi = np.asarray(min_bound, np.float64), np.asarray(max_bound, np.float64)
    if (lo > hi).any():
        return cloud(np.zeros((0, 3)))
    p = c["points"]
    with np.errstate(invalid="ignore"):
        inside = ((p >= lo) & (p <= hi)).all(axis=1)         # a NaN fails every comparison
    return select(c, np.nonzero(inside)[0])


# ---- statistics ----
def _serial_sum(t):
    """0.0 + t[0] + t[1] + ... left to right, per column"""
    return np.cumsum(np.concatenate([np.zeros((1, t.shape[1])), t]), axis=0)[-1]


def cumulant_terms(p):
    """n x 9: x, y, z, xx, xy, xz, yy, yz, zz, each product rounded"""
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    with np.errstate(all="ignore"):
        return np.stack([x, y, z, x * x, x * y, x * z, y * y, y * z, z * z], axis=1)


def mean_and_covariance(c, chunk=None):
    """ComputePointCloudMeanAndCovariance -> mean (3), covariance (3 x 3), the nine cumulant SUMS (before the division).
    chunk None: the reference's serial order.  Else the library's: serial sums over chunks of `chunk` consecutive points, the
    chunk sums added in chunk order."""
    p = c["points"]
    n = len(p)
    if n == 0:
        return np.zeros(3), np.eye(3), np.zeros(9)
    t = cumulant_terms(p)
    with np.errstate(all="ignore"):
        if chunk is None:
            sums = _serial_sum(t)
        else:
            sums = _serial_sum(np.stack([_serial_sum(t[a:a + chunk]) for a in range(0, n, chunk)]))
        q = sums / float(n)
        cov = np.empty((3, 3))
        cov[0, 0] = q[3] - q[0] * q[0]
        cov[1, 1] = q[6] - q[1] * q[1]
        cov[2, 2] = q[8] - q[2] * q[2]
        cov[0, 1] = cov[1, 0] = q[4] - q[0] * q[1]
        cov[0, 2] = cov[2, 0] = q[5] - q[0] * q[2]
        cov[1, 2] = cov[2, 1] = q[7] - q[1] * q[2]
    return q[:3].copy(), cov, sums


def inverse3(m):
    """Eigen 3.3.2's 3 x 3 inverse (InverseImpl.h:126-169): cofactors, det from the first cofactor column, no test"""
    m = np.asarray(m, np.float64)
    with np.errstate(all="ignore"):
        cof = lambda i, j: (m[(i + 1) % 3, (j + 1) % 3] * m[(i + 2) % 3, (j + 2) % 3]
                            - m[(i + 1) % 3, (j + 2) % 3] * m[(i + 2) % 3, (j + 1) % 3])
        c0 = [cof(0, 0), cof(1, 0), cof(2, 0)]
        det = _sum3(c0[0] * m[0, 0], c0[1] * m[1, 0], c0[2] * m[2, 0])
        invdet = np.float64(1.0) / det
        r = np.empty((3, 3))
        for j in range(3):
            r[0, j] = c0[j] * invdet
        for i in (1, 2):
            for j in range(3):
                r[i, j] = cof(j, i) * invdet
    return r


def mahalanobis_distance(c, chunk=None):
    """ComputePointCloudMahalanobisDistance: sqrt((p^T C^-1) p) per point"""
    mean, cov, _ = mean_and_covariance(c, chunk)
    inv = inverse3(cov)
    with np.errstate(all="ignore"):
        d = c["points"] - mean
        row = [_sum3(d[:, 0] * inv[0, j], d[:, 1] * inv[1, j], d[:, 2] * inv[2, j]) for j in range(3)]
        return np.sqrt(_sum3(row[0] * d[:, 0], row[1] * d[:, 1], row[2] * d[:, 2]))


# ---- programs: what a case's fixture records and the tests replay (tests/cloud_cases.py) ----
# "voxel" and "normals" are known to the reference harness alone (its --time chain); the library's are pinned to the
# host-array entry points instead (tests/test_cloud.py)
OPS = ("transform", "norm", "paint", "append", "bounds", "select", "uniform", "crop", "orient_dir", "orient_cam", "meancov",
       "mahal", "voxel", "normals")


def run(c, program, chunk=None):
    """program: a list of (op, argument ...) applied in order to a copy of c -> the final cloud and the f64 results of its
    bounds (6), meancov (3 + 9) and mahal (n) steps in order.  append's argument is a cloud, or None for the cloud itself."""
    c, results = copy(c), []
    for op, *arg in program:
        if op == "transform":
            transform(c, arg[0])
        elif op == "norm":
            normalize_normals(c)
        elif op == "paint":
            paint_uniform_color(c, arg[0])
        elif op == "append":
            append(c, copy(c) if arg[0] is None else arg[0])
        elif op == "bounds":
            results.append(bounds(c))
        elif op == "select":
            c = select(c, arg[0])
        elif op == "uniform":
            c = uniform_down_sample(c, arg[0])
        elif op == "crop":
            c = crop(c, arg[0], arg[1])
        elif op == "orient_dir":
            orient_normals_to_align_with_direction(c, arg[0])
        elif op == "orient_cam":
            orient_normals_towards_camera_location(c, arg[0])
        elif op == "meancov":
            mean, cov, _ = mean_and_covariance(c, chunk)
            results.append(np.concatenate([mean, cov.reshape(-1)]))
        elif op == "mahal":
            results.append(mahalanobis_distance(c, chunk))
        else:
            raise ValueError(op)
    return c, results
