"""The specification of the TriangleMesh operations on the device (visma_icp_trimesh_*; include/visma_icp.h): a plain, serial
numpy / Python restatement of the reference's Core/Geometry/TriangleMesh.cpp, TriangleMesh.h and DownSample.cpp
(SelectDownSample, CropTriangleMesh).  tests/test_trimesh_spec.py pins it to the compiled reference bit for bit
(tests/golden/trimesh.npz); tests/test_trimesh.py pins the library to it.

A mesh is a dict: vertices (nv x 3 f64), triangles (nt x 3 int32), vertex_normals, vertex_colors (nv x 3 f64 or None),
triangle_normals (nt x 3 f64 or None).  An attribute of no rows is None: the reference's HasX() is false for it.  Every
function changes the mesh it is given; select and crop return a new one.  numpy evaluates one operation per rounding."""
import numpy as np

ATTRS = ("vertices", "vertex_normals", "vertex_colors", "triangles", "triangle_normals")


def mesh(vertices, triangles, vertex_normals=None, vertex_colors=None, triangle_normals=None):
    f = lambda a: None if a is None else np.array(a, np.float64).reshape(-1, 3)
    m = dict(vertices=f(vertices), triangles=np.array(triangles, np.int32).reshape(-1, 3), vertex_normals=f(vertex_normals),
             vertex_colors=f(vertex_colors), triangle_normals=f(triangle_normals))
    return _settle(m)


def copy(m):
    return {k: None if v is None else v.copy() for k, v in m.items()}


def _settle(m):
    """HasX(): nothing is had on no rows; triangle normals need vertices too"""
    nv, nt = len(m["vertices"]), len(m["triangles"])
    if nv == 0:
        m["vertex_normals"] = m["vertex_colors"] = None
    if nv == 0 or nt == 0:
        m["triangle_normals"] = None
    return m


def _normalized(a):
    """Eigen's normalize() row by row (z = squaredNorm(); if (z > 0) v /= sqrt(z)), then TriangleMesh.h:96: x NaN -> (0, 0, 1)"""
    with np.errstate(all="ignore"):
        x, y, z = a[:, 0], a[:, 1], a[:, 2]
        n2 = (x * x + y * y) + z * z
        pos = n2 > 0
        length = np.sqrt(np.where(pos, n2, 1.0))
        out = np.where(pos[:, None], a / length[:, None], a)
    out[np.isnan(out[:, 0])] = (0.0, 0.0, 1.0)
    return out


def normalize_normals(m):
    for k in ("vertex_normals", "triangle_normals"):
        if m[k] is not None:
            m[k] = _normalized(m[k])


def compute_triangle_normals(m, normalized=True):
    v, t = m["vertices"], m["triangles"]
    if len(t):
        with np.errstate(all="ignore"):
            a = v[t[:, 1]] - v[t[:, 0]]
            b = v[t[:, 2]] - v[t[:, 0]]
            m["triangle_normals"] = np.stack([a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1], a[:, 2] * b[:, 0] - a[:, 0] * b[:, 2],
                                              a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]], axis=1)
    if normalized:
        normalize_normals(m)


def compute_vertex_normals(m, normalized=True, reverse=False):
    """reverse: the triangles walked backwards -- NOT the reference; what the fixture generator shows the order with"""
    if m["triangle_normals"] is None:
        compute_triangle_normals(m, False)
    nv = len(m["vertices"])
    if nv and m["vertex_normals"] is None:
        m["vertex_normals"] = np.zeros((nv, 3))
    if len(m["triangles"]):
        acc = m["vertex_normals"].tolist()                   # Python floats: IEEE doubles, one addition per rounding
        tn = m["triangle_normals"].tolist()
        order = range(len(tn) - 1, -1, -1) if reverse else range(len(tn))
        tri = m["triangles"].tolist()
        for i in order:
            n = tn[i]
            for c in tri[i]:
                a = acc[c]
                a[0] += n[0]; a[1] += n[1]; a[2] += n[2]
        m["vertex_normals"] = np.array(acc, np.float64).reshape(-1, 3)
    if normalized:
        normalize_normals(m)


def _keep_vertices(m, keep):
    for k in ("vertices", "vertex_normals", "vertex_colors"):
        if m[k] is not None:
            m[k] = m[k][keep]


def _keep_triangles(m, keep):
    for k in ("triangles", "triangle_normals"):
        if m[k] is not None:
            m[k] = m[k][keep]


def remove_duplicated_vertices(m):
    v = m["vertices"]
    first, old_to_new, keep = {}, np.zeros(len(v), np.int64), []
    for i, p in enumerate(v.tolist()):
        key = tuple(p)                                       # (-0.0 == 0.0 and they hash alike)
        nan = p[0] != p[0] or p[1] != p[1] or p[2] != p[2]   # a NaN equals nothing, itself included
        if nan or key not in first:
            if not nan:
                first[key] = i
            old_to_new[i] = len(keep)
            keep.append(i)
        else:
            old_to_new[i] = old_to_new[first[key]]
    _keep_vertices(m, np.array(keep, np.int64))
    m["triangles"] = old_to_new[m["triangles"]].astype(np.int32).reshape(-1, 3)
    _settle(m)
    return len(v) - len(keep)


def triangle_key(t):
    """TriangleMesh.cpp:235-251, the <= as written"""
    if t[0] <= t[1]:
        return (t[0], t[1], t[2]) if t[0] <= t[2] else (t[2], t[0], t[1])
    return (t[1], t[2], t[0]) if t[1] <= t[2] else (t[2], t[0], t[1])


def remove_duplicated_triangles(m):
    seen, keep = set(), []
    tri = m["triangles"].tolist()
    for i, t in enumerate(tri):
        key = triangle_key(t)
        if key not in seen:
            seen.add(key)
            keep.append(i)
    _keep_triangles(m, np.array(keep, np.int64))
    _settle(m)
    return len(tri) - len(keep)


def remove_non_manifold_triangles(m):
    t = m["triangles"]
    keep = (t[:, 0] != t[:, 1]) & (t[:, 1] != t[:, 2]) & (t[:, 2] != t[:, 0])
    _keep_triangles(m, keep)
    _settle(m)
    return int(len(t) - np.count_nonzero(keep))


def remove_non_manifold_vertices(m):
    nv = len(m["vertices"])
    used = np.zeros(nv, bool)
    used[m["triangles"].reshape(-1)] = True
    old_to_new = np.cumsum(used) - 1
    _keep_vertices(m, used)
    m["triangles"] = old_to_new[m["triangles"]].astype(np.int32).reshape(-1, 3)
    _settle(m)
    return int(nv - np.count_nonzero(used))


def purge(m):
    return (remove_duplicated_vertices(m), remove_duplicated_triangles(m), remove_non_manifold_triangles(m),
            remove_non_manifold_vertices(m))


def select(m, indices):
    nv = len(m["vertices"])
    chosen = np.zeros(nv, bool)
    chosen[np.asarray(indices, np.int64).reshape(-1)] = True
    t = m["triangles"]
    keep_t = chosen[t[:, 0]] & chosen[t[:, 1]] & chosen[t[:, 2]]
    used = np.zeros(nv, bool)
    used[t[keep_t].reshape(-1)] = True
    out = copy(m)
    old_to_new = np.cumsum(used) - 1
    _keep_triangles(out, keep_t)
    _keep_vertices(out, used)
    out["triangles"] = old_to_new[out["triangles"]].astype(np.int32).reshape(-1, 3)
    _settle(out)
    purge(out)
    return out


def crop(m, min_bound, max_bound):
    lo, hi = np.asarray(min_bound, np.float64), np.asarray(max_bound, np.float64)
    if (lo > hi).any():
        return mesh(np.zeros((0, 3)), np.zeros((0, 3), np.int32))
    v = m["vertices"]
    with np.errstate(invalid="ignore"):
        inside = ((v >= lo) & (v <= hi)).all(axis=1)         # a NaN fails every comparison
    return select(m, np.nonzero(inside)[0])


def transform(m, T):
    """a row: ((T_i0 x + T_i1 y) + T_i2 z) + T_i3 w; w = 1 for vertices, 0 for normals"""
    T = np.asarray(T, np.float64).reshape(4, 4)
    for k, w in (("vertices", 1.0), ("vertex_normals", 0.0), ("triangle_normals", 0.0)):
        a = m[k]
        if a is None or not len(a):
            continue
        with np.errstate(all="ignore"):
            m[k] = np.stack([((T[r, 0] * a[:, 0] + T[r, 1] * a[:, 1]) + T[r, 2] * a[:, 2]) + T[r, 3] * w for r in range(3)], axis=1)


# ---- programs: what a case's fixture records and the tests replay (tests/trimesh_cases.py) ----
OPS = ("ctn", "cvn", "norm", "rdv", "rdt", "rnmt", "rnmv", "purge", "select", "crop", "transform")


def run(m, program):
    """program: a list of (op, argument ...) applied in order to a copy of m -> the final mesh and the removed counts of the
    remove_* and purge steps in order"""
    m, removed = copy(m), []
    for op, *arg in program:
        if op == "ctn":
            compute_triangle_normals(m, bool(arg[0]))
        elif op == "cvn":
            compute_vertex_normals(m, bool(arg[0]))
        elif op == "norm":
            normalize_normals(m)
        elif op == "rdv":
            removed.append(remove_duplicated_vertices(m))
        elif op == "rdt":
            removed.append(remove_duplicated_triangles(m))
        elif op == "rnmt":
            removed.append(remove_non_manifold_triangles(m))
        elif op == "rnmv":
            removed.append(remove_non_manifold_vertices(m))
        elif op == "purge":
            removed.extend(purge(m))
        elif op == "select":
            m = select(m, arg[0])
        elif op == "crop":
            m = crop(m, arg[0], arg[1])
        elif op == "transform":
            transform(m, arg[0])
        else:
            raise ValueError(op)
    return m, removed
